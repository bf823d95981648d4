// bioik_bounded_rows.h — the rows of the solve-kernel table (bioik_hip.hip: BIOIK_SOLVE_KERNELS) for calls with per-query variable bounds, in a header of their own
// because two translation units read them: bioik_hip.hip (the SolveKernel enum, the report names, launch_kernel, the allowance of more than 64 KiB of LDS) and
// bioik_bounded.hip (their __global__ definitions).  ROW(X, name, __launch_bounds__, body...), as in bioik_hip.hip.
#pragma once
#ifndef BIOIK_SOLVE_WAVES_PER_SIMD
#define BIOIK_SOLVE_WAVES_PER_SIMD 3  // register budget of k_solve: wavefronts per SIMD (its __launch_bounds__)
#endif
// k_solve_bounded: solve_body of the general flavour with the bounded pointer type, under k_solve's launch bounds; k_solve_point_bounded: point_body, likewise
#define BIOIK_BOUNDED_BODY_KERNELS(ROW, X) ROW(X, k_solve_bounded, (256, BIOIK_SOLVE_WAVES_PER_SIMD), solve_body<false, false, false, false, 0, true>)
#define BIOIK_BOUNDED_KERNELS(ROW) BIOIK_BOUNDED_BODY_KERNELS(ROW, ) ROW(, k_solve_point_bounded, (64), point_body<true>)
