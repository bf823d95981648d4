// bioik_bounded.hip — the __global__ definitions of the solve kernels for calls with per-query variable bounds (bioik_bounded_rows.h), in a device module of
// their own: compiled next to k_solve and k_solve_lean they change those kernels' register allocation (8 spilled scalar registers and 160 bytes of code in
// k_solve_lean, profiles/per_query_bounds_metadata.log), and a feature no existing call uses is not to move the kernels every existing call runs.  bioik_hip.hip
// declares them and launches them by its table like every other row.  The product build only: the host simulator of the test-suite calls the kernel bodies
// directly and compiles bioik_hip.hip alone.
#include <cfloat>
#include <cmath>

#include "bioik_bounded_rows.h"
#include "bioik_gradient.h"
#include "bioik_kernels.h"

#define BIOIK_GLOBAL_(X, name, bounds, ...)                      \
    __global__ void __launch_bounds__ bounds name(SolveArgs a) { \
        extern __shared__ double lds[];                          \
        __VA_ARGS__(a, blockIdx.x, lds);                         \
    }
BIOIK_BOUNDED_KERNELS(BIOIK_GLOBAL_)
#undef BIOIK_GLOBAL_
