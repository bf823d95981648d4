"""Independent references for the shared arithmetic headers (bio_ik_amd/csrc/bioik_sincos.h, bioik_fused.h, bioik_acos.h): NumPy long double (x87 80-bit: 64-bit
mantissa) for bulk comparisons and mpmath (50 digits) to validate the long double values themselves.  Used by tests/test_arith_headers.py at test time
(no reference value is stored); `python tools/arith_reference.py` prints the agreement of the two references, and with `--sincos-domain LIBRARY` the table behind
BIOIK_SINCOS_DOMAIN.  Written from the mathematical definitions (frame.h:108-172 of the reference for the quaternion algebra), not from the headers under test.
The one stored file, tests/golden/sincos_bits.npz, holds no reference but the header's OWN bits at 4096 arguments (write_sincos_golden), to pin that they do not move."""
import numpy as np

LD = np.longdouble
PIO2_LD = (LD(np.pi) + LD(1.2246467991473532e-16)) / 2  # pi / 2 to long double precision: fl(pi) and the double behind it


def sincos_special_arguments():
    k = np.arange(-64, 65, dtype=np.float64)
    base = np.concatenate([k * (np.pi / 4), k * (np.pi / 2)])
    near = np.concatenate([base, np.nextafter(base, np.inf), np.nextafter(base, -np.inf), base + 1e-9, base - 1e-9])
    return np.concatenate([near, [0.0, -0.0, 1e-300, -1e-300, 1e-8, 0.5, 1.0, 2.0, 3.0, 1e4 + 0.1]])


GOLDEN_SINCOS = "sincos_bits.npz"  # under tests/golden


def sincos_golden_arguments():
    """the 4096 fixed arguments of tests/golden/sincos_bits.npz: random over +-4, +-100, +-1e5 and +-3.3e9 (below 2^31 pi / 2, where the quadrant of the header as
    first written was right on every target), and the special arguments"""
    rng = np.random.default_rng(20261018)
    special = sincos_special_arguments()
    n = (4096 - len(special)) // 4
    xs = [rng.uniform(-a, a, n) for a in (4.0, 100.0, 1e5)] + [rng.uniform(-3.3e9, 3.3e9, 4096 - len(special) - 3 * n), special]
    return np.concatenate(xs)


def write_sincos_golden(path, ev):
    """record the bits ev(0, x) gives on the golden arguments (run ONCE, on the commit before bioik_sincos.h took its quadrant from an addition: the file pins
    that the header's bits did not move where they were right)"""
    x = sincos_golden_arguments()
    out = np.ascontiguousarray(ev(0, x))
    np.savez(path, x=x.view(np.uint64), sin=np.ascontiguousarray(out[:, 0]).view(np.uint64), cos=np.ascontiguousarray(out[:, 1]).view(np.uint64))


def sincos_quadrant_arguments(domain):
    """arguments whose multiple of pi / 2 does not fit an int32: 3.4e9, +-1e10, 1e12, 1e15 (clipped to the domain) and fl(k pi / 2) for k around 2^31 and 2^40, both signs"""
    k = np.array([2.0 ** 31 + d for d in (-2, -1, 0, 1, 2)] + [2.0 ** 40 - 1, 2.0 ** 40 + 1])
    a = np.concatenate([[3.4e9, 1e10, 1e12, 1e15], (k.astype(LD) * PIO2_LD).astype(np.float64)])
    a = np.minimum(a, np.nextafter(domain, 0.0))
    return np.concatenate([a, -a])


def sincos_domain_arguments(domain, n, seed, lo=2.0 ** 17, n_multiples=64):
    """per binade from lo to the domain end: n random arguments of both signs and the neighbours (nextafter both ways, and itself) of fl(k pi / 2) for n_multiples
    random k of that binade; returns [(binade exponent, arguments)]"""
    rng = np.random.default_rng(seed)
    out = []
    e = int(np.log2(lo))
    while 2.0 ** e < domain:
        a, b = 2.0 ** e, min(2.0 ** (e + 1), domain)
        x = rng.uniform(a, b, n) * rng.choice([-1.0, 1.0], n)
        k = np.floor(rng.uniform(a, b, n_multiples) / (np.pi / 2))
        m = (k.astype(LD) * PIO2_LD).astype(np.float64) * rng.choice([-1.0, 1.0], n_multiples)
        m = np.concatenate([m, np.nextafter(m, np.inf), np.nextafter(m, -np.inf)])
        out.append((e, np.concatenate([x, m[np.abs(m) < domain]])))
        e += 1
    return out


def sincos_every_double_arguments(n=200000, seed=5):
    """for host == device: log-uniform over 1e-308 ... DBL_MAX in both signs, the neighbourhoods of +-2^31 pi / 2 and +-2^32 pi / 2 on both sides, subnormals, +-0,
    +-DBL_MAX (no infinity, no NaN)"""
    rng = np.random.default_rng(seed)
    big = np.finfo(np.float64).max
    x = 10.0 ** rng.uniform(-308, np.log10(big), n) * rng.choice([-1.0, 1.0], n)
    near = []
    for k in (2.0 ** 31, 2.0 ** 32):
        c = k * (np.pi / 2)
        near += [c + rng.uniform(-64.0, 64.0, 4096), c + np.arange(-32, 33) * (np.pi / 2), c + np.arange(-32, 33) * (np.pi / 4)]
        near.append(c + np.arange(-64, 65) * np.spacing(c))
    near = np.concatenate(near)
    tiny = np.finfo(np.float64).tiny
    sub = np.concatenate([5e-324 * np.array([1.0, 2.0, 3.0, 1e3, 1e10]), [np.nextafter(tiny, 0.0), tiny], rng.uniform(0.0, tiny, 256)])
    edge = np.array([0.0, big, np.nextafter(big, 0.0), 2.0 ** 52, 2.0 ** 53, 2.0 ** 63, 2.0 ** 64, 2.0 ** 1023])
    pos = np.concatenate([near, sub, edge])
    return np.concatenate([x, pos, -pos])


def sincos_longdouble(x):
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    return np.sin(xl), np.cos(xl)


def sincos_mpmath(x):
    import mpmath
    mpmath.mp.dps = 50
    s = np.array([LD(mpmath.nstr(mpmath.sin(mpmath.mpf(float(v))), 30)) for v in x], dtype=LD)
    c = np.array([LD(mpmath.nstr(mpmath.cos(mpmath.mpf(float(v))), 30)) for v in x], dtype=LD)
    return s, c


def acos_special_arguments():
    """the branch points of the fdlibm algorithm (0.5, 1, tiny arguments), both signs, and their neighbours"""
    base = np.array([0.0, 2.0 ** -58, 2.0 ** -57, 2.0 ** -56, 1e-300, 1e-10, 0.25, 0.4999999, 0.5, 0.5000001, 0.75, 0.9, 0.99, 0.999999, 1.0 - 2.0 ** -52, 1.0 - 2.0 ** -53, 1.0])
    near = np.concatenate([base, np.nextafter(base, 2.0), np.nextafter(base, -2.0)])
    near = near[np.abs(near) <= 1.0]
    return np.concatenate([near, -near])


def acos_longdouble(x):
    return np.arccos(np.asarray(x, dtype=np.float64).astype(LD))


def acos_mpmath(x):
    import mpmath
    mpmath.mp.dps = 50
    return np.array([LD(mpmath.nstr(mpmath.acos(mpmath.mpf(float(v))), 30)) for v in x], dtype=LD)


def atan2_special_arguments():
    """the reduction thresholds of atan (0.4375, 0.6875, 1.1875, 2.4375) as ratios, the axes, both signs of everything"""
    r = np.array([0.0, 1e-300, 2.0 ** -30, 2.0 ** -29, 0.4374999, 0.4375, 0.6875, 1.0, 1.1875, 2.4375, 1e10, 2.0 ** 61, 1e300])
    r = np.concatenate([r, np.nextafter(r, np.inf), np.nextafter(r, -np.inf)])
    r = r[r >= 0.0]
    ys, xs = [], []
    for sy in (1.0, -1.0):
        for sx in (1.0, -1.0):
            ys.append(sy * r), xs.append(np.full(r.shape, sx))          # y / x = the ratio
            ys.append(np.full(r.shape, sy)), xs.append(sx * np.maximum(r, 1e-300))  # x / y = the ratio
    return np.stack([np.concatenate(ys), np.concatenate(xs)], axis=1)


def atan2_longdouble(yx):
    yx = np.asarray(yx, dtype=np.float64).astype(LD)
    return np.arctan2(yx[:, 0], yx[:, 1])


def atan2_mpmath(yx):
    import mpmath
    mpmath.mp.dps = 50
    return np.array([LD(mpmath.nstr(mpmath.atan2(mpmath.mpf(float(y)), mpmath.mpf(float(x))), 30)) for y, x in yx], dtype=LD)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def qrot_longdouble(x):
    """v rotated by q (not necessarily of unit length, as frame.h:108-149 computes it): v + 2 (w t + u x t), t = u x v, q = (u, w); and the magnitude of its terms"""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    u, w, v = x[:, 0:3], x[:, 3:4], x[:, 4:7]
    t = _cross(u, v)
    r = v + 2 * (w * t + _cross(u, t))
    au, av = np.abs(u), np.abs(v)
    at = _cross(au, av) + 2 * np.stack([au[:, 2] * av[:, 1], au[:, 0] * av[:, 2], au[:, 1] * av[:, 0]], axis=1)  # |u| x |v| with every term positive
    mag = av + 2 * (np.abs(w) * at + _cross(au, at) + 2 * np.stack([au[:, 2] * at[:, 1], au[:, 0] * at[:, 2], au[:, 1] * at[:, 0]], axis=1))
    return r, mag


def qmul_longdouble(x):
    """Hamilton product p (x) q (frame.h:151-172), components x y z w"""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    px, py, pz, pw, qx, qy, qz, qw = [x[:, i] for i in range(8)]
    terms = [[pw * qx, px * qw, py * qz, -pz * qy], [pw * qy, py * qw, pz * qx, -px * qz], [pw * qz, pz * qw, px * qy, -py * qx], [pw * qw, -px * qx, -py * qy, -pz * qz]]
    r = np.stack([sum(t) for t in terms], axis=1)
    mag = np.stack([sum(np.abs(v) for v in t) for t in terms], axis=1)
    return r, mag


def dot3_longdouble(x):
    x = np.asarray(x, dtype=np.float64).astype(LD)
    p = x[:, 0:3] * x[:, 3:6]
    return p.sum(axis=1, keepdims=True), np.abs(p).sum(axis=1, keepdims=True)


def dot4_longdouble(x):
    x = np.asarray(x, dtype=np.float64).astype(LD)
    p = x[:, 0:4] * x[:, 4:8]
    return p.sum(axis=1, keepdims=True), np.abs(p).sum(axis=1, keepdims=True)


def revolute_longdouble(x):
    """frame (p, q) o (cpos, cos(h) ca + sin(h) cb): p' = p + q cpos q^-1, q' = q (x) (cos(h) ca + sin(h) cb)   (forward_kinematics.h:89-112, :331-354)"""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    p, q, h, cpos, ca, cb = x[:, 0:3], x[:, 3:7], x[:, 7:8], x[:, 8:11], x[:, 11:15], x[:, 15:19]
    lq = np.cos(h) * ca + np.sin(h) * cb
    rp, mp = qrot_longdouble(np.concatenate([q, cpos], axis=1).astype(np.float64))
    rq, mq = qmul_longdouble(np.concatenate([q, lq.astype(np.float64)], axis=1).astype(np.float64))
    return np.concatenate([p + rp, rq], axis=1), np.concatenate([np.abs(p) + mp, mq + 1e-300], axis=1)


def sincos_abs_error(ev, x):
    """the worst absolute error of either component of ev(0, x) against long double"""
    out = ev(0, x)
    rs, rc = sincos_longdouble(x)
    return float(max(np.max(np.abs(out[:, 0].astype(LD) - rs)), np.max(np.abs(out[:, 1].astype(LD) - rc))))


def sincos_domain_table(ev, per_binade=400000, seed=1, n_mp=200):
    """the measurement behind BIOIK_SINCOS_DOMAIN (bioik_sincos.h): the worst absolute error on |x| <= 1e5, then per binade [2^e, 2^(e+1)) from e = 17 to 52, long double
    as the reference, itself held against mpmath (50 digits) on n_mp arguments of every binade.  Returns (base, [(e, worst, long double's own error)])."""
    rng = np.random.default_rng(seed)
    base = max(sincos_abs_error(ev, rng.uniform(-a, a, per_binade)) for a in (4.0, 100.0, 1e5, 1e5, 1e5))
    rows = []
    for e in range(17, 53):
        x = rng.uniform(2.0 ** e, 2.0 ** (e + 1), per_binade) * rng.choice([-1.0, 1.0], per_binade)
        ls, lc = sincos_longdouble(x[:n_mp])
        ms, mc = sincos_mpmath(x[:n_mp])
        rows.append((e, sincos_abs_error(ev, x), float(max(np.max(np.abs(ls - ms)), np.max(np.abs(lc - mc))))))
    return base, rows


if __name__ == "__main__":
    import sys
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.uniform(-1e5, 1e5, 2000), sincos_special_arguments()])
    a, b = sincos_longdouble(xs), sincos_mpmath(xs)
    print("long double vs mpmath (50 digits), %d arguments: max |sin| diff %.3g, max |cos| diff %.3g" % (len(xs), float(np.max(np.abs(a[0] - b[0]))), float(np.max(np.abs(a[1] - b[1])))))
    if len(sys.argv) > 2 and sys.argv[1] == "--sincos-domain":  # python tools/arith_reference.py --sincos-domain tests/hostsim/libbioik_hostsim.so
        import os
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
        from bio_ik_amd import solver
        lib = solver.load_library(sys.argv[2])
        base, rows = sincos_domain_table(lambda op, x: solver.eval_arith(op, x, lib=lib))
        print("worst absolute error of either component, |x| <= 1e5: %.3g" % base)
        for e, worst, ld in rows:
            print("2^%d .. 2^%d: %.3g (%.2f x)   long double vs mpmath %.1g" % (e, e + 1, worst, worst / base, ld))
