"""The small-half-angle path of the chain walks (bioik_sincos.h: bioik_sincos_small; bioik_platform.h: p_sincos_n and its wavefront vote), shared by the
host-simulator suite (tests/test_hostsim_sincos_small.py) and the GPU suite (tests/test_gpu_sincos_small.py).  The tolerance is zero bits everywhere.

  function level   bioik_sincos_small against bioik_sincos on |x| <= BIOIK_SINCOS_SMALL (bioik_eval_arith ops 9 and 0), and the bound itself
  the vote         bioik_eval_arith op 8 runs p_sincos_n with lane = item (blocks of 256 lanes, so items 64 b ... 64 b + 63 are one wavefront): blocks of 64
                   that are all small, all large, small with ONE large value at lane 0, 31, 32 or 63, at the bound and one ulp either side, small with one
                   NaN, and a last block of 37 items.  Expected: bioik_sincos (op 0) item by item.
  walk level       function-level FK and fitness (fk_walk, one individual per lane: a wavefront is 64 consecutive individuals) of the serial chains of
                   tests/walk_length_cases.py with 2, 3 and 4 joints and of the right arm (seven joints behind a prefix of one op), 128 individuals, with every
                   joint within +-1.5 rad (every half angle small), every joint beyond +-1.6 rad (every half angle large) and one individual beyond in one
                   joint (one lane of one wavefront turns that joint's vote; the other wavefront stays on the small path) -- against the oracle in the
                   arithmetic it shares with the device, bit for bit.  (The walks of SEVERAL children per lane, serial_joint_n and the general loop of fk_walk_n,
                   are inside the solve kernels: whole solves of these chains, tests/walk_length_cases.py, the snakes on the small path at every joint.)
"""
import numpy as np

import walk_length_cases as wl
from bio_ik_amd import abi, solver
from oracle import orc

INVPIO2 = 6.36619772367581382433e-01  # bioik_sincos.h
OP_SINCOS, OP_VOTED, OP_SMALL = 0, 8, 9


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, want, x, what):
    differ = np.nonzero(np.any(bits(got) != bits(want), axis=1))[0]
    assert differ.size == 0, "%s: %d of %d differ, first at item %d, x = %r: %s, expected %s" % (what, differ.size, len(x), differ[0], float(x[differ[0]]),
                                                                                                  got[differ[0]], want[differ[0]])


# ---- function level ---------------------------------------------------------------------------------------------------------------------------------

def small_arguments(bound):
    """+-0, the smallest subnormal, +-BIOIK_SINCOS_SMALL and its neighbours below, 10^5 random arguments inside the range: half of them uniform, half log-uniform
    in magnitude down to the subnormals"""
    rng = np.random.default_rng(20)
    tiny = np.nextafter(0.0, 1.0)
    special = np.array([0.0, -0.0, tiny, -tiny, bound, -bound, np.nextafter(bound, 0.0), -np.nextafter(bound, 0.0), 2.2250738585072014e-308, -2.2250738585072014e-308])
    uniform = rng.uniform(-bound, bound, 50000)
    logarithmic = np.minimum(bound, 10.0 ** rng.uniform(-320, np.log10(bound), 50000)) * rng.choice([-1.0, 1.0], 50000)
    x = np.concatenate([special, uniform, logarithmic])
    assert np.all(np.abs(x) <= bound) and x.size >= 100000
    return x


def check_bound(lib):
    """BIOIK_SINCOS_SMALL: below pi / 4, and the multiple of pi / 2 nearest to it is zero -- rint is monotonic, so it is zero for every smaller magnitude"""
    bound = solver.sincos_small_bound(lib)
    assert 0.5 < bound < np.pi / 4
    assert np.rint(bound * INVPIO2) == 0.0 and np.rint(-bound * INVPIO2) == 0.0
    return bound


def check_small_is_sincos(ev, bound):
    """bioik_sincos_small == bioik_sincos on |x| <= BIOIK_SINCOS_SMALL, bit for bit"""
    x = small_arguments(bound)
    want, got = ev(OP_SINCOS, x), ev(OP_SMALL, x)
    assert_same_bits(got, want, x, "bioik_sincos_small")
    assert np.all(bits(got[:2, 0]) == 0) and np.all(got[:2, 1] == 1.0)  # sin(+-0) = +0 in both forms (their last step is +0 + -0), cos = 1
    # (the comparison can fail: just beyond the first quadrant the kernels alone are NOT the function)
    y = np.array([1.0, -2.0, 3.0])
    assert np.all(np.any(bits(ev(OP_SMALL, y)) != bits(ev(OP_SINCOS, y)), axis=1))


# ---- the vote ----------------------------------------------------------------------------------------------------------------------------------------

def vote_arguments(bound, last_block_large):
    """blocks of 64 consecutive items (name, values); the last one has 37 items"""
    rng = np.random.default_rng(21)
    small = lambda n: rng.uniform(-bound, bound, n)  # noqa: E731
    large = lambda n: rng.uniform(0.8, 40.0, n) * rng.choice([-1.0, 1.0], n)  # noqa: E731
    up, down = np.nextafter(bound, 1.0), np.nextafter(bound, 0.0)
    blocks = [("all small", small(64)), ("all large", large(64))]
    for lane in (0, 31, 32, 63):
        b = small(64)
        b[lane] = large(1)[0]
        blocks.append(("one large at lane %d" % lane, b))
    # at the bound: a wavefront whose largest magnitude IS the bound (both signs) stays on the small path, one ulp beyond turns it
    b = small(64)
    b[[3, 40]] = bound, -bound
    b[[4, 41]] = down, -down
    blocks.append(("at the bound and one ulp below", b))
    for lane, v in ((17, up), (50, -up)):
        b = small(64)
        b[[3, 40]] = bound, -bound
        b[lane] = v
        blocks.append(("one ulp beyond the bound at lane %d" % lane, b))
    blocks.append(("every lane at the bound", np.where(np.arange(64) % 2 == 0, bound, -bound)))
    blocks.append(("every lane one ulp beyond", np.where(np.arange(64) % 2 == 0, up, -up)))
    b = small(64)
    b[29] = np.nan
    blocks.append(("one NaN among small values", b))
    blocks.append(("all small again", small(64)))  # (a wavefront behind one that took the general path)
    b = small(37)
    if last_block_large:
        b[36] = large(1)[0]
    blocks.append(("a partial wavefront of 37" + (", its last lane large" if last_block_large else ""), b))
    assert all(len(v) == 64 for _, v in blocks[:-1])
    return blocks


def check_vote(ev, bound):
    """p_sincos_n with lane = item == bioik_sincos item by item, whatever the wavefront voted; returns the outputs (for device against simulator)"""
    out = []
    for last_block_large in (False, True):
        blocks = vote_arguments(bound, last_block_large)
        x = np.concatenate([v for _, v in blocks])
        assert x.size % 64 == 37
        want, got = ev(OP_SINCOS, x), ev(OP_VOTED, x)
        at = 0
        for name, v in blocks:
            w, g = want[at:at + len(v)], got[at:at + len(v)]
            nan = np.isnan(v)
            assert np.all(np.isnan(g[nan])) and np.all(np.isnan(w[nan]))
            assert_same_bits(g[~nan], w[~nan], v[~nan], name)
            at += len(v)
        out.append((x, got))
    return out


# ---- walk level --------------------------------------------------------------------------------------------------------------------------------------

ROBOTS = ("snake2", "snake3", "snake4", "right_arm")  # serial arms of walk_length_cases: 2, 3, 4 joints; seven joints behind a prefix of one op
INDIVIDUALS = 128
GENE_SETS = ("within", "beyond", "one_beyond")

_walk_reference = {}


def gene_set(kind, D):
    """128 individuals: every joint within +-1.5 rad / every joint beyond +-1.6 rad / within, but individual 70 (lane 6 of the second wavefront) beyond in joint
    D // 2 only"""
    rng = np.random.default_rng(22)
    within = rng.uniform(-1.5, 1.5, (INDIVIDUALS, D))
    beyond = rng.uniform(1.6, 6.0, (INDIVIDUALS, D)) * rng.choice([-1.0, 1.0], (INDIVIDUALS, D))
    if kind == "within":
        g = within
    elif kind == "beyond":
        g = beyond
    else:
        g = within.copy()
        g[70, D // 2] = beyond[70, D // 2]
    bound = 0.78
    half = np.abs(g) * 0.5
    assert {"within": np.all(half <= bound), "beyond": np.all(half > bound), "one_beyond": np.sum(half > bound) == 1}[kind]
    return g


def walk_reference(name):
    """(template, oracle, seed, goal parameters, {gene set: (genes, the oracle's frames, primary, secondary)}): computed once in the oracle's device arithmetic
    (trig mode 1, the caller's fixture), shared, never written to"""
    if name not in _walk_reference:
        t = wl.CASES[name][0]()
        o = orc.Oracle(t)
        rng = np.random.default_rng(23)
        seed = np.asarray(t.model.default_positions(), dtype=np.float64).copy()
        par = rng.normal(size=o.P)
        sets = {}
        for kind in GENE_SETS:
            genes = gene_set(kind, o.D)
            frames = o.fk_genes(seed, genes)
            prim, sec = o.fitness(abi.FK_EXACT, seed, par, genes)
            assert np.isfinite(frames).all() and np.isfinite(prim).all() and np.ptp(prim) > 0
            for a in (genes, frames, prim, sec):
                a.setflags(write=False)
            sets[kind] = (genes, frames, prim, sec)
        seed.setflags(write=False), par.setflags(write=False)
        _walk_reference[name] = (t, o, seed, par, sets)
    return _walk_reference[name]


def check_walk(name, kind, make_solver):
    """function-level FK and fitness of the robot at the gene set: the oracle's bits; returns them"""
    t, o, seed, par, sets = walk_reference(name)
    genes, frames, prim, sec = sets[kind]
    h = make_solver(t)
    assert (h.D, h.T) == (o.D, o.T)
    got = h.fk_genes(seed, genes)
    assert np.array_equal(bits(got), bits(frames)), "%s, %s: frames differ at individuals %s" % (name, kind, np.unique(np.nonzero(got != frames)[0])[:8])
    p, s = h.fitness(abi.FK_EXACT, seed, par, genes)
    assert np.array_equal(bits(p), bits(prim)) and np.array_equal(bits(s), bits(sec)), "%s, %s: fitness differs" % (name, kind)
    return got, p, s
