// bioik_sincos.h — one sincos for every side of the boundary.
//
// The joint frames of revolute joints need sin/cos of the half angle (reference src/forward_kinematics.h:89-112
// calls libm).  libm on the host and the device math library disagree in the last ulp, and bio2_memetic amplifies
// last-ulp differences into different search trajectories (its line search divides by a second difference of
// fitness values taken 1e-7 apart, src/ik_evolution_2.cpp:498-506).  To make "same inputs -> same results" hold
// bit for bit between the gfx950 kernels and the CPU oracle, both evaluate THIS function: a two-term reduction by pi/2
// (pi/2 = P1 + P2, each step ONE fused multiply-add, exact under cancellation) followed by the fdlibm minimax kernels as plain
// Horner chains, written with *, rint and EXPLICIT fused multiply-adds (compiler contraction is off everywhere), so any IEEE-754
// double implementation produces identical bits.  Error <= 1.56 ulp for |x| <= 1e5 (joint half angles are a few radians):
// tests/test_oracle_frame.py.  32 instructions on gfx950 against 45 for the three-term reduction with a tail carried through the
// kernels (1.02 ulp) that it replaces: +3 % chip-wide step rate (profiles/r02_ab_sincos.log).
// Polynomial coefficients: fdlibm k_sin.c, k_cos.c (Sun Microsystems, 1993).
//
// Domain.  Every double gives the same bits on x86-64 and gfx950 (IEEE operations only, the quadrant included); the values are RIGHT for |x| < BIOIK_SINCOS_DOMAIN,
// the largest power of two up to which the worst absolute error of either component stays within 1.1 x its worst on |x| <= 1e5.  Measured in the host simulator
// (the device's bits) against long double, itself within 6e-20 of mpmath at 50 digits, 400 000 arguments per binade (python tools/arith_reference.py --sincos-domain):
//     |x| <= 1e5        1.72e-16   (1.56 ulp of a value in [0.5, 1))
//     2^17 ... 2^47     1.67e-16 ... 1.76e-16 in every binade (0.97 x ... 1.02 x)
//     2^47 ... 2^48     2.00e-16   (1.16 x)          2^48 ... 2^49   8.7e-16
//     2^49 ... 2^50     1.2e-14                      2^50 ... 2^51   4.9e-13
//     2^51 and beyond   no digit is right (x * 2 / pi no longer rounds to the right integer; from 2^53 on the values leave [-1, 1], at 1e300 they are infinite)
// Beyond the domain the solver evaluates nothing: BIOIK_CANDIDATE_BOUND (bioik_kernels.h), and the same bound in the test-suite's CPU checker.
#pragma once

#define BIOIK_SINCOS_DOMAIN 140737488355328.0  // 2^47

#ifndef BIOIK_SINCOS_FN
#define BIOIK_SINCOS_FN inline
#endif

// The three pieces of bioik_sincos, each inline in this header: the reduction (fn, r), the two fdlibm kernels on r, the quadrant step.  bioik_sincos composes
// them; bioik_sincos_small is the kernels alone.
BIOIK_SINCOS_FN void bioik_sincos_reduce(double x, double* fn_out, double* r_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double invpio2 = 6.36619772367581382433e-01;
    const double P1 = 1.57079632679489655800e+00, P2 = 6.12323399573676603587e-17;
    const double fn = __builtin_rint(x * invpio2);
    double r = __builtin_fma(-fn, P1, x);
    r = __builtin_fma(-fn, P2, r);
    *fn_out = fn;
    *r_out = r;
}
BIOIK_SINCOS_FN void bioik_sincos_kernels(double r, double* s_out, double* c_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = r * r;
    const double ps = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, S6, S5), S4), S3), S2), S1);
    *s_out = __builtin_fma(z * r, ps, r);
    const double pc = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, C6, C5), C4), C3), C2), C1);
    *c_out = __builtin_fma(z * z, pc, __builtin_fma(-0.5, z, 1.0));
}
BIOIK_SINCOS_FN void bioik_sincos_quadrant(double fn, double s, double c, double* sn, double* cs) {
    // The quadrant, fn mod 4: the low word of fn + 1.5 * 2^52 holds fn's low 32 bits in two's complement (|fn| < 2^51) -- ONE IEEE addition, the same
    // bits on every target for every double.  (A conversion to int is out of range from |fn| = 2^31 on, a half angle of 3.37e9: undefined in C++, INT_MIN
    // on x86-64 and a saturated value on gfx950, so the two sides parted and both were wrong.)
    unsigned w[2];
    const double shifted = fn + 6755399441055744.0;
    __builtin_memcpy(w, &shifted, 8);
#if defined(BIOIK_SINCOS_SIGN_BRANCHES)
    const unsigned q = w[0] & 3u;
    const double so = (q & 1) ? c : s;
    const double co = (q & 1) ? s : c;
    *sn = q >= 2 ? -so : so;
    *cs = (q == 1 || q == 2) ? -co : co;
#else
    // quadrants 2, 3 negate both kernels' values (bit 1 of fn moved onto the sign bit: a shift and one bit operation on each high word; negation IS the
    // sign flip, for every double); the odd quadrants then take (c, -s) for (s, c): a select per word, the negation in the select
    const unsigned m1 = (w[0] << 30) & 0x80000000u;
    const bool odd = (w[0] << 31) != 0u;
    unsigned sw[2], cw[2];
    __builtin_memcpy(sw, &s, 8);
    __builtin_memcpy(cw, &c, 8);
    sw[1] ^= m1;
    cw[1] ^= m1;
    const unsigned so[2] = {odd ? cw[0] : sw[0], odd ? cw[1] : sw[1]};
    const unsigned co[2] = {odd ? sw[0] : cw[0], odd ? sw[1] ^ 0x80000000u : cw[1]};
    __builtin_memcpy(sn, so, 8);
    __builtin_memcpy(cs, co, 8);
#endif
}

BIOIK_SINCOS_FN void bioik_sincos(double x, double* sn, double* cs) {
    double fn, r, s, c;
    bioik_sincos_reduce(x, &fn, &r);
    bioik_sincos_kernels(r, &s, &c);
    bioik_sincos_quadrant(fn, s, c, sn, cs);
}

// Half angles of at most BIOIK_SINCOS_SMALL in magnitude need neither the reduction nor the quadrant.  rint is monotonic and odd, and
// rint(BIOIK_SINCOS_SMALL * invpio2) = rint(0.4965...) == 0, so fn is (a signed) zero for every |x| <= BIOIK_SINCOS_SMALL: both reduction steps then return x itself
// (fma(-+0, P, x) == x for every x but -0, which becomes +0: the sine kernel returns +0 for either zero, its last step being +0 + -0), the shifted sum's low
// word is 0, and the quadrant step hands s and c through.  bioik_sincos_small is bioik_sincos without those pieces: the same bits on |x| <= BIOIK_SINCOS_SMALL
// (tests/sincos_small_cases.py); beyond, and for NaN, it is NOT bioik_sincos.
#define BIOIK_SINCOS_SMALL 0.78  // < pi / 4 = 0.78539...
BIOIK_SINCOS_FN void bioik_sincos_small(double x, double* sn, double* cs) { bioik_sincos_kernels(x, sn, cs); }
