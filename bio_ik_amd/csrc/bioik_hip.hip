// bioik_hip.hip — the C-ABI of include/bioik_hip.h: __global__ entry points for gfx950 and the thin host shim
// that owns device memory and launches them.  No torch, no C++ types across the boundary.
//
// The library is built by hipcc for gfx950 and refuses to do anything without a HIP device; there is no CPU execution path in it.
// (The test-suite compiles this file a second time with a substitute back end that lives under tests/hostsim and arrives through
// BIOIK_BACKEND_HEADER / BIOIK_PLATFORM_HEADER; the product build defines neither.)
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "bioik_compile.h"
#include "bioik_gradient.h"
#include "bioik_kernels.h"
#include "bioik_layouts.h"

static_assert((int)G_POSITION == (int)BIOIK_GOAL_POSITION && (int)G_POSE == (int)BIOIK_GOAL_POSE && (int)G_CONE == (int)BIOIK_GOAL_CONE &&
                  (int)G_JOINT_VARIABLE == (int)BIOIK_GOAL_JOINT_VARIABLE && (int)G_MINIMAL_DISPLACEMENT == (int)BIOIK_GOAL_MINIMAL_DISPLACEMENT &&
                  (int)G_AVOID_JOINT_LIMITS == (int)BIOIK_GOAL_AVOID_JOINT_LIMITS && (int)G_TOUCH == (int)BIOIK_GOAL_TOUCH && (int)G_CLEARANCE == (int)BIOIK_GOAL_CLEARANCE &&
                  (int)G_SELF_CLEARANCE == (int)BIOIK_GOAL_SELF_CLEARANCE && BIOIK_DEV_MAX_OBSTACLES == BIOIK_MAX_OBSTACLES && BIOIK_DEV_MAX_TOUCH_POINTS == BIOIK_MAX_TOUCH_POINTS &&
                  BIOIK_DEV_MAX_LINK_CAPSULES == BIOIK_MAX_LINK_CAPSULES,
              "goal opcodes out of sync with include/bioik_hip.h");
static_assert((int)FK_LINEAR == (int)BIOIK_FK_LINEAR && (int)FK_EXACT == (int)BIOIK_FK_EXACT, "fk modes out of sync");

using bioik::Error;

static thread_local std::string g_err;

// The solve kernels, each described ONCE: name, __launch_bounds__, the kernel body it is a build of -- solve_body<LEAN, CL, JOINT, SLIM, FIXED> (bioik_kernels.h) or
// point_body (bioik_gradient.h).  The __global__ definitions of the HIP back end, the SolveKernel enum, the names of the BIOIK_SOLVE_REPORT lines, launch_kernel (both
// back ends) and the solve kernels' part of BIOIK_WIDE_LDS_KERNELS all come from these rows; SolveLauncher::choose_kernel says which row a launch takes.
//
// k_solve, k_solve_lean: two flavours of the solver (bioik_platform.h, pb_flavour): k_solve_lean for problems without floating / planar joints whose ops
// meet the genes in gene order (every BASELINE.json configuration), k_solve for everything
// k_solve_lean_cl: the lean flavour with the children computed where they are read (no genotype columns in LDS: the LDS-bound problems, C3 / C4)
// k_solve_lean_cl4: the same body under the register budget of FOUR wavefronts per SIMD (128 VGPRs instead of 168).  The hot loops of the computed-children
// flavour fit it; its once-per-step code then keeps some values in scratch memory, so a lone step is slower (110 against 102 us) and it
// only pays where the LDS footprint lets the fourth wavefront be resident AND the generation loops dominate a step: the launcher
// picks it when a CU holds at least 16 wavefronts of the problem and a lane walks eight or more children per generation (the
// 31-joint, 512-children configuration: +12 %; the first launch of a 7-joint, 128-children solve: -2 %; profiles/r03_ab_four_waves.log).
// (solve_body<.., SLIM>: the species record is read from LDS per generation instead of living in scratch memory across the chain walks: 67 -> 31 spilled values)
// k_solve_lean_cl4h: k_solve_lean_cl4 with two HELPER wavefronts (solve_body<.., FIXED = 5>), for launches that leave most of the chip idle -- a single pose of the plugin, a few
// hundred queries, the stragglers a chip-filling call hands over when the chip runs empty: wavefronts 0 and 1 are k_solve_lean_cl4's (a species each), wavefronts
// 2 and 3 walk half of every generation's children for them, so that a generation's walks take a wavefront half the instructions.  A lone wavefront issues one
// instruction per ~4.3 cycles whatever it does and k_solve_lean_cl4 keeps two of a CU's four SIMDs busy: this keeps four.  Hand-overs between the wavefronts
// are words in LDS, the helpers reach no barrier (profiles/r05_helped_kernel.log)
// k_solve_lean_cl64w4: the computed-children kernel for BIOIK_SCHEDULE_THROUGHPUT: ONE wavefront per query (both species on its halves; the compiler knows it and drops the
// barriers) under the register budget of four wavefronts per SIMD
// (solve_body<.., DENSE>: what the launcher guarantees for this kernel -- 64 lanes, the species on the halves of the wavefront, exact FK, children in
// pairs, no secondary goal -- is known at compile time, and the fitness values of a generation cross its walks in LDS instead of in registers).
// The whole solve of a stream of batches under the dense mapping: sixteen queries per CU instead of twelve (+11 % with six solves in flight;
// 30 values -- the lane's best two across the chain walk, a few kernel-lifetime ones -- then live in scratch memory; profiles/r03_ab_dense_four_waves.log)
// k_solve_lean_lin: populations of up to 32 children per species with LINEARISED phenotypes (the reference's own parameters: 16 children, RobotFK_Mutator): both species on
// the halves of one wavefront, children computed where they are read, under the register budget of four wavefronts per SIMD (solve_body<.., FIXED = 3>).
// Such solves are bound by the latency of their single-individual phases (linearisation, line search, ranking), not by arithmetic: sixteen queries
// per CU instead of twelve (profiles/r04_ab_small_population_kernel.log)
// k_solve_lean_clj4: computed children with both species of a query on the halves of one wavefront AND secondary goals: the children of the two species are walked as one list over
// the 64 lanes (solve_body<.., JOINT>), so that the wavefront does not wait for the longer of two random prefixes (C3: +7 %, profiles/r03_ab_joint_walk.log) -- under
// the register budget of four wavefronts per SIMD (FIXED = 4: fitness values parked in LDS, accessors rebuilt behind the walks).  (Its 168-register sibling
// k_solve_lean_clj of rounds 3 - 5 served the one LDS band in which a CU holds exactly twelve queries; retired in round 6: this build runs there too.)
// k_solve_point: the point solvers gd_c / jac (bioik_gradient.h): one wavefront per query, at most 64 KiB of LDS (SolveLauncher::solve_point)
// k_solve_bounded, k_solve_point_bounded: k_solve's and k_solve_point's bodies with the third pointer flavour (BoundedProbPtr, bioik_platform.h): a call with per-query variable
//                   bounds (bioik_solve_batch_bounded) reads every bound from its query's table in LDS instead of from the problem block.  Only such calls reach them,
//                   and they reach no other row -- the gating by which a TouchGoal only ever reaches k_solve.  Their rows are written in bioik_bounded_rows.h and their
//                   __global__ definitions are compiled in a translation unit of their own (bioik_bounded.hip): in one device module with them, the register allocation
//                   of k_solve and k_solve_lean comes out differently (profiles/per_query_bounds_metadata.log), and the existing kernels are to stay as they are
#include "bioik_bounded_rows.h"  // (BIOIK_SOLVE_WAVES_PER_SIMD: the register budget of k_solve)
#ifndef BIOIK_DENSE_WAVES
#define BIOIK_DENSE_WAVES 4
#endif
// (ROW(X, name, bounds, body...): X is handed through to the row macro, for lists whose entries are X(name))
#define BIOIK_SOLVE_BODY_KERNELS_HERE(ROW, X)                                                              \
    ROW(X, k_solve, (256, BIOIK_SOLVE_WAVES_PER_SIMD), solve_body<false>)                                  \
    ROW(X, k_solve_lean, (256, BIOIK_SOLVE_WAVES_PER_SIMD), solve_body<true>)                              \
    ROW(X, k_solve_lean_cl, (256, BIOIK_SOLVE_WAVES_PER_SIMD), solve_body<true, true>)                     \
    ROW(X, k_solve_lean_cl4, (128, 4), solve_body<true, true, false, true, 2>)                             \
    ROW(X, k_solve_lean_cl4h, (256, 4), solve_body<true, true, false, true, 5>)                            \
    ROW(X, k_solve_lean_cl64w4, (64, BIOIK_DENSE_WAVES), solve_body<true, true, false, true, 1>)           \
    ROW(X, k_solve_lean_lin, (64, 4), solve_body<true, true, false, true, 3>)                              \
    ROW(X, k_solve_lean_clj4, (64, 4), solve_body<true, true, true, true, 4>)
#define BIOIK_SOLVE_KERNELS_HERE(ROW) BIOIK_SOLVE_BODY_KERNELS_HERE(ROW, ) ROW(, k_solve_point, (64), point_body)  // (defined in this translation unit)
#define BIOIK_SOLVE_BODY_KERNELS(ROW, X) BIOIK_SOLVE_BODY_KERNELS_HERE(ROW, X) BIOIK_BOUNDED_BODY_KERNELS(ROW, X)
#define BIOIK_SOLVE_KERNELS(ROW) BIOIK_SOLVE_KERNELS_HERE(ROW) BIOIK_BOUNDED_KERNELS(ROW)
#define BIOIK_ENUM_(X, name, ...) name,
enum class SolveKernel { BIOIK_SOLVE_KERNELS(BIOIK_ENUM_) };
#undef BIOIK_ENUM_
#define BIOIK_NAME_(X, name, ...) #name,
static const char* const kSolveKernelNames[] = {BIOIK_SOLVE_KERNELS(BIOIK_NAME_)};
#undef BIOIK_NAME_

// The kernels that may be launched with more than 64 KiB of dynamic LDS: above 64 KiB a launch needs an explicit allowance, which be_allow_lds(bytes)
// gives every kernel of this list.  Both back ends take the list from here.
#define BIOIK_WIDE_ROW_(X, name, ...) X(name)
#define BIOIK_WIDE_LDS_KERNELS(X) \
    BIOIK_SOLVE_BODY_KERNELS(BIOIK_WIDE_ROW_, X) X(k_eval_fk) X(k_eval_fitness) X(k_eval_approximator) X(k_eval_reproduce) X(k_eval_check) X(k_stream_fitness)

// ------------------------------------------------------------------------------------------------------------
// back end: memory + launch
// ------------------------------------------------------------------------------------------------------------
#if defined(BIOIK_BACKEND_HEADER)
#include BIOIK_BACKEND_HEADER  // test builds only (tests/hostsim): a substitute back end; the product never defines it
#else
typedef hipStream_t stream_t;
#define HIP_CHECK(expr)                                                                                       \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) throw Error(BIOIK_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
static int be_device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
static void be_set_device(int d) { HIP_CHECK(hipSetDevice(d)); }
// what the launcher sizes its mappings to (MI355X: 256 CUs in 8 XCDs, 160 KiB of LDS per CU)
struct DeviceInfo {
    size_t lds_cu = 160 * 1024;
    int cus = 256, xcds = 8;
};
static DeviceInfo be_device_info(int d) {
    DeviceInfo di;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d) == hipSuccess) {
        if (prop.maxSharedMemoryPerMultiProcessor >= 64 * 1024) di.lds_cu = prop.maxSharedMemoryPerMultiProcessor;
        if (prop.multiProcessorCount > 0) di.cus = prop.multiProcessorCount;
    }
    int x = 0;
    if (hipDeviceGetAttribute(&x, hipDeviceAttributeNumberOfXccs, d) == hipSuccess && x > 0 && x <= 16) di.xcds = x;
    return di;
}
static int be_get_device() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d;
}
static void* be_alloc(size_t bytes) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, bytes ? bytes : 8));
    return p;
}
static void be_free(void* p) {
    if (p) (void)hipFree(p);
}
static void* be_alloc_pinned(size_t bytes) {  // page-locked host memory: hipMemcpyAsync from / to it is one DMA, no staging copy
    void* p = nullptr;
    HIP_CHECK(hipHostMalloc(&p, bytes ? bytes : 8, hipHostMallocDefault));
    return p;
}
static void be_free_pinned(void* p) {
    if (p) (void)hipHostFree(p);
}
// stream-ordered scratch: launches of one problem handle on different streams never share it
static void* be_alloc_async(size_t bytes, stream_t s) {
    void* p = nullptr;
    HIP_CHECK(hipMallocAsync(&p, bytes ? bytes : 8, s));
    return p;
}
static void be_free_async(void* p, stream_t s) {
    if (p) (void)hipFreeAsync(p, s);
}
static bool be_stream_capturing(stream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) return false;
    return st != hipStreamCaptureStatusNone;
}
static void be_h2d(void* d, const void* h, size_t bytes, stream_t s) {
    if (bytes) HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
}
static void be_d2h(void* h, const void* d, size_t bytes, stream_t s) {
    if (bytes) HIP_CHECK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s));
}
static void be_sync(stream_t s) { HIP_CHECK(hipStreamSynchronize(s)); }
// The words a solve needs (re)set in stream order -- the hand-over's counters, the launch clock, the islands' first-success words -- are written by a KERNEL
// of this library, not by hipMemsetAsync: a hipGraph that holds a memset node in front of these kernels replays correctly once and writes to a wild address
// from its second replay on under this runtime's AQL packet capture (ROCm 7.2; DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 cures it, so does having no memset node:
// profiles/r05_graph_replay_root_cause.log, tools/graph_replay_raw_probe.py).  g_memset_nodes (BIOIK_SOLVE_MEMSET_NODES=1) brings the memsets back for that probe.
__global__ void __launch_bounds__(256) k_fill_words(unsigned int* p, size_t n, unsigned int value) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = value;
}
static bool g_memset_nodes = false;
static void be_fill_async(void* p, size_t bytes, int byte_value, stream_t s) {  // bytes: a multiple of four
    if (bytes == 0) return;
    if (g_memset_nodes) {
        HIP_CHECK(hipMemsetAsync(p, byte_value, bytes, s));
        return;
    }
    const size_t n = bytes / 4;
    hipLaunchKernelGGL(k_fill_words, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (unsigned int*)p, n, (unsigned int)(byte_value & 0xff) * 0x01010101u);
    HIP_CHECK(hipGetLastError());
}
__global__ void k_read_clock(unsigned long long* out) { *out = wall_clock64(); }
// the device's constant 100 MHz clock as of "now" (a one-lane kernel on a stream of its own and a wait for it: ~30 us; launch_solve calls it rarely).
// The stream and the word the kernel writes exist once per DEVICE for the life of the process (a map under a mutex) -- whatever thread asks, and however often the
// caller's threads come and go: per-thread copies keyed on the last device leaked a stream and a pinned block whenever a thread alternated between two devices
// (the plugin's shards) or was created per call (bioik_solve_batch_multi's workers).
struct ClockReader {
    hipStream_t stream = nullptr;
    unsigned long long* word = nullptr;  // (page-locked and mapped: the kernel writes it, the host reads it after the wait)
};
static std::mutex g_clock_mtx;
static std::map<int, ClockReader> g_clock_readers;
static unsigned long long be_device_clock_now() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(g_clock_mtx);
    ClockReader& r = g_clock_readers[dev];
    if (!r.stream) {
        HIP_CHECK(hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking));
        HIP_CHECK(hipHostMalloc((void**)&r.word, 64, hipHostMallocDefault));
    }
    hipLaunchKernelGGL(k_read_clock, dim3(1), dim3(1), 0, r.stream, r.word);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(r.stream));
    return *(volatile unsigned long long*)r.word;
}
// wall time of what `enqueue` puts on stream s, in ms (two events and a wait for the second): the launcher's measured mapping choice (solve_dispatch)
static bool be_can_time() { return true; }
template <class F>
static double be_time_ms(stream_t s, F&& enqueue) {
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    float ms = 0.0f;
    try {
        HIP_CHECK(hipEventRecord(e0, s));
        enqueue();
        HIP_CHECK(hipEventRecord(e1, s));
        HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    } catch (...) {
        (void)hipEventDestroy(e0), (void)hipEventDestroy(e1);
        throw;
    }
    (void)hipEventDestroy(e0), (void)hipEventDestroy(e1);
    return (double)ms;
}
static void be_zero_async(void* p, size_t bytes, stream_t s) { be_fill_async(p, bytes, 0, s); }
static void be_fill_ff_async(void* p, size_t bytes, stream_t s) { be_fill_async(p, bytes, 0xff, s); }
static stream_t be_stream_create() {
    hipStream_t s = nullptr;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
}
static void be_stream_destroy(stream_t s) {
    if (s) (void)hipStreamDestroy(s);
}

#define BIOIK_GLOBAL_(X, name, bounds, ...)                      \
    __global__ void __launch_bounds__ bounds name(SolveArgs a) { \
        extern __shared__ double lds[];                          \
        __VA_ARGS__(a, blockIdx.x, lds);                         \
    }
BIOIK_SOLVE_KERNELS_HERE(BIOIK_GLOBAL_)
#undef BIOIK_GLOBAL_
#define BIOIK_GLOBAL_DECL_(X, name, bounds, ...) __global__ void name(SolveArgs a);  // (bioik_bounded.hip)
BIOIK_BOUNDED_KERNELS(BIOIK_GLOBAL_DECL_)
#undef BIOIK_GLOBAL_DECL_
__global__ void k_select(SelectArgs a) { select_body(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x); }
__global__ void __launch_bounds__(64) k_select_wave(SelectArgs a) { select_coop(a, (uint64_t)blockIdx.x, (int)threadIdx.x); }  // a wavefront per query: calls of few queries with many islands
// island migration between two launches of a solve (migrate_mark, migrate_coop): a lane per entry of the hand-over list, then a wavefront per query
__global__ void __launch_bounds__(256) k_migrate_mark(MigrateArgs a) { migrate_mark(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x); }
__global__ void __launch_bounds__(64) k_migrate(MigrateArgs a) { migrate_coop(a, (uint64_t)blockIdx.x, (int)threadIdx.x); }
// the k best distinct islands of every query, ranked (bioik_solve_batch_ranked): a wavefront per query, lane = island
__global__ void __launch_bounds__(64) k_select_ranked(RankedArgs a) {
    extern __shared__ double lds[];
    select_ranked(a, (uint64_t)blockIdx.x, (int)threadIdx.x, lds);
}
__global__ void __launch_bounds__(256) k_eval_fk(EvalArgs a) {
    extern __shared__ double lds[];
    eval_fk_body(a, blockIdx.x, lds);
}
__global__ void __launch_bounds__(256) k_eval_fitness(EvalArgs a) {
    extern __shared__ double lds[];
    eval_fitness_body(a, blockIdx.x, lds);
}
__global__ void __launch_bounds__(256) k_eval_approximator(EvalArgs a) {
    extern __shared__ double lds[];
    eval_approximator_body(a, lds);
}
__global__ void __launch_bounds__(256) k_eval_reproduce(EvalArgs a) {
    extern __shared__ double lds[];
    eval_reproduce_body(a, blockIdx.x, lds);
}
__global__ void __launch_bounds__(256) k_eval_check(EvalArgs a) {
    extern __shared__ double lds[];
    eval_check_body(a, blockIdx.x, lds);
}
__global__ void __launch_bounds__(64) k_eval_bounds(BoundsArgs a) { eval_bounds_body(a, (uint64_t)blockIdx.x, (int)threadIdx.x); }
__global__ void __launch_bounds__(256) k_eval_arith(ArithArgs a) { arith_body(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x); }
__global__ void __launch_bounds__(256) k_stream_fitness(StreamArgs a) {
    extern __shared__ double lds[];
    stream_fitness_body(a, blockIdx.x, lds);
}
// a launch: KERNEL with `args`; BODYCALL names the same kernel body as a function of (b_, l_) = (block index, LDS base) for back ends
// that call it directly
#define LAUNCH(KERNEL, BODYCALL, grid, block, lds, stream, args)                                      \
    do {                                                                                              \
        hipLaunchKernelGGL(KERNEL, dim3((unsigned)(grid)), dim3(block), lds, stream, args);           \
        HIP_CHECK(hipGetLastError());                                                                 \
    } while (0)
// more than 64 KiB of dynamic LDS per workgroup must be allowed explicitly (every kernel of BIOIK_WIDE_LDS_KERNELS)
static void be_allow_lds(size_t bytes) {
#define BIOIK_ALLOW_(k) HIP_CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    BIOIK_WIDE_LDS_KERNELS(BIOIK_ALLOW_)
#undef BIOIK_ALLOW_
}
#endif
// a launch of the solve kernel `kind` (its row of BIOIK_SOLVE_KERNELS: the kernel, and its body for back ends that call it directly)
static void launch_kernel(SolveKernel kind, const SolveArgs& args, uint64_t grid, int lanes, size_t lds, stream_t stream) {
    switch (kind) {
#define BIOIK_LAUNCH_(X, name, bounds, ...)                                        \
    case SolveKernel::name:                                                        \
        LAUNCH(name, (__VA_ARGS__(args, b_, l_)), grid, lanes, lds, stream, args); \
        break;
        BIOIK_SOLVE_KERNELS(BIOIK_LAUNCH_)
#undef BIOIK_LAUNCH_
    }
}

// The arrays of one solve call as an entry point was given them, host or device pointers alike: a parameter bundle and nothing more
struct SolveArrays {
    size_t n;  // queries
    const double *seeds, *goal_params;
    double *solutions, *fitness;
    int32_t *success, *steps;
    int32_t* count;  // ranked calls (bioik_solve_batch_ranked): the distinct solutions returned per query; null otherwise
    // per-query variable bounds (bioik_solve_batch_bounded), [n][V] each: both set (a bounded call: k_solve_bounded / k_solve_point_bounded) or both null
    const double* var_lo = nullptr;
    const double* var_hi = nullptr;
    bool bounded() const { return var_lo != nullptr; }
};

// ------------------------------------------------------------------------------------------------------------
// handles
// ------------------------------------------------------------------------------------------------------------
struct bioik_model {
    bioik::HostModel host;
    int device;
    DeviceInfo dev;  // of `device`: LDS per CU, CUs, XCDs (hipDeviceProp_t)
    bioik_model(const bioik_model_desc& d, int dv) : host(d), device(dv), dev(be_device_info(dv)) {}
};
struct bioik_problem {
    bioik_model* model;
    bioik::HostProblem host;
    DevProblem* d_pb = nullptr;
    double* d_touch = nullptr;  // DevProblem::touch_points: the collision points the problem's TouchGoals read, the points and obstacle blocks of its ClearanceGoals, the rows of both links of its SelfClearanceGoals (null without any)
    // Host-pointer solves (bioik_solve_batch, bioik_solve_batch_submit / _wait) go through one of kIoSlots slots, each with a grow-only
    // device arena, its page-locked host mirror (one DMA in, one DMA out per solve) and its own stream: up to kIoSlots batches of one
    // handle are in flight together, the tail of one solve behind the bulk of the next.  Streams are created at a
    // slot's first use, not with the handle: HIP multiplexes streams onto four hardware queues per device, and a stream that a
    // device-pointer caller never uses would push one of the caller's own streams onto a shared queue.
    static constexpr int kIoSlots = 6;  // (three solves in flight fill the chip under BIOIK_SCHEDULE_LATENCY, six under BIOIK_SCHEDULE_THROUGHPUT)
    struct IoSlot {
        void* dev = nullptr;
        void* host = nullptr;
        size_t bytes = 0;
        stream_t stream = nullptr;
        bool stream_made = false;
        // the solve in flight on this slot, if any: where its results go when it completes
        bool pending = false;
        uint64_t ticket = 0;
        bioik::IoArenaLayout arena;  // of `host`: its result blocks
        SolveArrays caller{};  // (its inputs were copied at the submission: only n and the result arrays are used)
        // a solve of this slot that ended in a device error: remembered for ITS ticket's wait (the slot itself is free again)
        uint64_t failed_ticket = 0;
        int failed_code = 0;
        std::string failed_message;
    } io[kIoSlots];
    uint64_t next_ticket = 1;  // ticket t runs on slot t % kIoSlots
    uint64_t first_query = 0;
    // The caller's timeout counts from the call's SUBMISSION (ik_parallel.h:160, 200): the host reads the device's 100 MHz clock next to its own steady
    // clock (when the handle first needs it, and again when the pair is older than a few seconds: the two clocks drift by parts per million) and hands every
    // eager solve its deadline in device ticks (SolveArgs::deadline).  A solve captured into a hipGraph cannot know when it will be replayed: it counts from
    // its first workgroup's start, on a word of its own that a kernel in the graph zeroes -- one of kCaptureClocks per handle, never reused.
    bool clock_valid = false;
    std::chrono::steady_clock::time_point clock_host0;
    unsigned long long clock_dev0 = 0;
    unsigned long long* d_clocks = nullptr;
    unsigned clock_next = 0;
    static constexpr unsigned kCaptureClocks = 64;
    // SolveArgs::error: one word per host-pointer slot and one for the device-pointer entry, in page-locked host memory the kernels can write: a rendezvous between
    // wavefronts that gave up (k_solve_lean_cl4h) sets the word of its call; the call's wait (or, for the device-pointer entry, the handle's next call) reports it
    unsigned int* h_error = nullptr;
    unsigned int* d_resident = nullptr;  // workgroups of the throughput schedule's launches that are running now (SolveArgs::resident), all streams of this handle
    // Scratch of a solve that needs some (per-island results, the state of handed-over units): one persistent buffer per (stream, purpose), grown when a
    // solve asks for more.  Solves on one stream follow each other, so they may share it; solves on other streams have their own.  (Stream-ordered
    // allocations did this until round 4 -- but a captured graph that contains an allocation and its release aborts on its second replay on this ROCm.)
    // Lifetime under hipGraph capture: a captured solve bakes the buffer's address into its graph, so a buffer a capture has used is PINNED -- it is never
    // released or handed to an eager solve again before the handle goes; the next eager solve on that stream retires it (the graphs keep it) and allocates its own.
    struct Scratch {
        void* base = nullptr;
        size_t capacity = 0;
        bool pinned = false;
        // purpose 0 (the islands' results): the control words of SolveArgs::island_done -- per query a count of the islands that have filed and the first_success word --
        // lie at the buffer's start, `ctl_n` of each, and are back in their resting state (0 / 0xffffffff) whenever no solve is running on them: the kernel that uses
        // them puts them back.  ctl_base != base (or a call of more than ctl_n queries): they have to be set up (a new buffer, a call of the other kind in between).
        // Eager calls only: a captured call sets its words up inside its graph, on every replay (graphs on one pinned buffer lay it out each their own way)
        void* ctl_base = nullptr;
        size_t ctl_n = 0;
        // how many words of each kind rest at this buffer's start for an EAGER call on it (a pinned buffer is never an eager call's)
        size_t words_at_rest() const { return !pinned && ctl_base == base ? ctl_n : 0; }
        void words_set_up(void* at, size_t n) { ctl_base = at, ctl_n = n; }
        void forget_words() { ctl_base = nullptr, ctl_n = 0; }  // (a call that lays the buffer out its own way, a solve that broke off)
    };
    std::map<std::pair<stream_t, int>, Scratch> scratch;
    // The launcher's MEASURED mapping choice (solve_dispatch): per kind of call -- (children per species, FK mode, islands or not) under the latency schedule --
    // the preset that ran a chip-filling call fastest, and what each eligible preset took (ms; < 0: not eligible)
    struct Tuned {
        int preset = -1;
        double ms[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    };
    std::map<std::tuple<int, int, int, int>, Tuned> tuned;  // (..., floor(log2(units)): a choice holds for calls of about the size it was measured on)
    // pinned buffers that eager solves have moved away from: captured graphs may still replay into them -- and LATER captures on the same stream take them again
    // (graphs captured from one stream share that stream's pinned buffer anyway), so that a caller who alternates eager calls and captures holds two buffers
    // per stream, not one more per alternation
    struct Retired {
        void* base;
        size_t capacity;
        stream_t stream;
        int purpose;
    };
    std::vector<Retired> retired_scratch;
    std::mutex mtx;
    bioik_problem(bioik_model* m, const bioik_problem_desc& d) : model(m), host(&m->host, d) {}
    ProbPtr pb() const { return (ProbPtr)d_pb; }
};

static int fail(const Error& e) {
    g_err = e.what();
    return e.code;
}
static int fail(const std::exception& e) {
    g_err = e.what();
    return BIOIK_ERR_INVALID_ARGUMENT;
}
#define API_BEGIN try {
#define API_END                      \
    return BIOIK_OK;                 \
    }                                \
    catch (const Error& e) {         \
        return fail(e);              \
    }                                \
    catch (const std::exception& e) { \
        return fail(e);              \
    }

// ------------------------------------------------------------------------------------------------------------
// Diagnostic switches (tools/README.md).  The environment is read ONCE, when the library is loaded, into this struct -- and again only when
// a test or a probe asks for it (bioik_debug_reload_switches): nothing on the launch path touches the environment.
// ------------------------------------------------------------------------------------------------------------
struct SolveSwitches {
    int threads = 0;            // BIOIK_SOLVE_THREADS: lanes per (query, island), 0 = the launcher's choice
    int store_children = -1;    // BIOIK_SOLVE_STORE_CHILDREN (-1: not set)
    int child_pairs = -1;       // BIOIK_SOLVE_CHILD_PAIRS
    int species_parallel = -1;  // BIOIK_SOLVE_SPECIES_PARALLEL
    int columnless = -1;        // BIOIK_SOLVE_COLUMNLESS (1: children computed where they are read, 2: ... and scored in pairs)
    bool general = false, general_set = false;  // BIOIK_SOLVE_GENERAL
    bool report = false;        // BIOIK_SOLVE_REPORT
    bool three_waves = false, four_waves = false, no_joint = false;
    int dense_handover = 0;     // BIOIK_SOLVE_DENSE_HANDOVER=K: a throughput solve hands the queries that pass K steps over to the latency mapping (0: never)
    int drain_below = 1024;     // BIOIK_SOLVE_DRAIN_BELOW=N: the dense kernel's stragglers leave for the latency mapping when fewer than N wavefronts of the handle's launches
                                // are left on the chip (0: never): isolated chip-filling calls of the latency schedule (launch_solve: latency_drain)
    bool drain_throughput = true;   // BIOIK_SOLVE_DRAIN_THROUGHPUT=0: the throughput schedule's solves do NOT hand their stragglers over (round 5: they do -- with k_solve_lean_cl4h as the
                                    // stragglers' kernel a stream's tail gains more than the bookkeeping costs: 20 timed steps +3.5 %, 60 steps +-0, profiles/r05_drain_throughput.log)
    int drain_min_units = 1025;  // BIOIK_SOLVE_DRAIN_MIN_UNITS=N: the latency schedule starts a call of N units and more (on 256 CUs; scaled to the chip) under the dense kernel and hands the
                                 // stragglers over; smaller calls run k_solve_lean_cl4 (or its helped build) from the start.  (With four and more islands per query, which stop
                                 // each other after a few steps, the dense kernel's long steps cost more than they bring below 3072 units: profiles/r05_drain_min_units.log)
    int drain_below_throughput = 512;  // BIOIK_SOLVE_DRAIN_BELOW_THROUGHPUT=N: ... when fewer than N wavefronts are left (a stream keeps the chip fuller than an isolated call: later)
    int drain_min_steps = 4;    // BIOIK_SOLVE_DRAIN_MIN_STEPS: ... and have run this many steps
    int drain_test = 0;         // BIOIK_SOLVE_DRAIN_TEST=n (parity suites): any solve, unit u leaves its first launch after 1 + hash(u) % n steps
    int helped = 1024;  // BIOIK_SOLVE_HELPED=N: launches of up to N (query, island) units of a problem k_solve_lean_cl4 covers without a secondary goal run its helped
                        // build (k_solve_lean_cl4h: four wavefronts per unit), as do the stragglers a chip-filling call hands over; 0: never
    int debug_flags = 0;  // BIOIK_SOLVE_DEBUG_FLAGS (tests): SolveArgs::debug_flags
    int fused_select = 1;  // BIOIK_SOLVE_FUSED_SELECT=0: the islands of a one-launch solve are reduced by a kernel of their own (and the first_success words set up by a fill kernel), as until round 5; -1: ... by k_select's lane per query whatever the island count (tests)
    int autotune = 1;  // BIOIK_SOLVE_AUTOTUNE: 1 (default) = the host-pointer entries time the eligible lane mappings on a handle's first chip-filling call of a kind and keep
                       // the fastest (solve_dispatch); 2 = the device-pointer entry does so too (it then waits for its stream once); 0 = the rules alone
    bool memset_nodes = false;  // BIOIK_SOLVE_MEMSET_NODES=1 (probe of the runtime's graph-replay defect): hipMemsetAsync instead of the library's own fill kernel
    bool capture_one_launch = false;  // BIOIK_SOLVE_CAPTURE_ONE_LAUNCH=1: a call on a stream that is being captured gets a one-launch mapping (round 4's rule)
    int sort_key_drop = 10;     // BIOIK_SOLVE_SORT_KEY_DROP=b (parity suites, 10 ... 52): the pre-selection's sort keys give up b low bits of a fitness, so that the exact path runs often
    int preselect = 1;          // BIOIK_SOLVE_PRESELECT: 1 (default) = the pre-selection's survivors by selection of the k-th key (select_threshold), 0 = by the sort of all children
    int tie_test_bits = 0;      // BIOIK_SOLVE_TIE_TEST_BITS=b (parity suites, 0 ... 52): the children's fitness loses b low bits before the selection, so that children tie
    bool two_phase_set = false, two_phase_init = false;
    std::vector<long> two_phase;  // BIOIK_SOLVE_TWO_PHASE: K or K1,K2,... (hand-overs after those steps), "init", 0 = never
    std::string phase_dump;       // BIOIK_PHASE_DUMP (profiling builds)
    std::string handover_dump;    // BIOIK_SOLVE_HANDOVER_DUMP=path (probes): every solve in several launches appends "scratch list_off count_off units" to this file
    bool manual() const { return threads > 0 || store_children >= 0 || child_pairs >= 0 || species_parallel >= 0 || columnless >= 0; }
};
static SolveSwitches parse_switches() {
    SolveSwitches w;  // (every default is written once, above: a switch that is not set keeps its field)
    auto geti = [](const char* name, int unset) {
        const char* e = std::getenv(name);
        return e ? std::atoi(e) : unset;
    };
    w.threads = geti("BIOIK_SOLVE_THREADS", w.threads);
    if (std::getenv("BIOIK_SOLVE_THREADS") && w.threads <= 0) w.threads = 64;
    w.store_children = geti("BIOIK_SOLVE_STORE_CHILDREN", w.store_children);
    w.child_pairs = geti("BIOIK_SOLVE_CHILD_PAIRS", w.child_pairs);
    w.species_parallel = geti("BIOIK_SOLVE_SPECIES_PARALLEL", w.species_parallel);
    w.columnless = geti("BIOIK_SOLVE_COLUMNLESS", w.columnless);
    if (const char* e = std::getenv("BIOIK_SOLVE_GENERAL")) w.general_set = true, w.general = std::atoi(e) != 0;
    w.report = std::getenv("BIOIK_SOLVE_REPORT") != nullptr;
    w.three_waves = std::getenv("BIOIK_SOLVE_THREE_WAVES") != nullptr;
    w.four_waves = std::getenv("BIOIK_SOLVE_FOUR_WAVES") != nullptr;
    w.no_joint = std::getenv("BIOIK_SOLVE_NO_JOINT") != nullptr;
    w.dense_handover = geti("BIOIK_SOLVE_DENSE_HANDOVER", w.dense_handover);
    w.drain_below = geti("BIOIK_SOLVE_DRAIN_BELOW", w.drain_below);
    w.drain_throughput = geti("BIOIK_SOLVE_DRAIN_THROUGHPUT", w.drain_throughput) != 0;
    w.drain_below_throughput = geti("BIOIK_SOLVE_DRAIN_BELOW_THROUGHPUT", w.drain_below_throughput);
    w.drain_min_units = geti("BIOIK_SOLVE_DRAIN_MIN_UNITS", w.drain_min_units);
    w.drain_min_steps = geti("BIOIK_SOLVE_DRAIN_MIN_STEPS", w.drain_min_steps);
    w.drain_test = geti("BIOIK_SOLVE_DRAIN_TEST", w.drain_test);
    w.sort_key_drop = geti("BIOIK_SOLVE_SORT_KEY_DROP", w.sort_key_drop);
    w.preselect = geti("BIOIK_SOLVE_PRESELECT", w.preselect) != 0 ? 1 : 0;
    w.tie_test_bits = geti("BIOIK_SOLVE_TIE_TEST_BITS", w.tie_test_bits);
    if (w.tie_test_bits < 0 || w.tie_test_bits > 52) w.tie_test_bits = 0;
    w.capture_one_launch = geti("BIOIK_SOLVE_CAPTURE_ONE_LAUNCH", w.capture_one_launch) != 0;
    w.memset_nodes = geti("BIOIK_SOLVE_MEMSET_NODES", w.memset_nodes) != 0;
    w.autotune = geti("BIOIK_SOLVE_AUTOTUNE", w.autotune);
    w.helped = geti("BIOIK_SOLVE_HELPED", w.helped);
    w.debug_flags = geti("BIOIK_SOLVE_DEBUG_FLAGS", w.debug_flags);
    w.fused_select = geti("BIOIK_SOLVE_FUSED_SELECT", w.fused_select);
    if (w.sort_key_drop < 10 || w.sort_key_drop > 52) w.sort_key_drop = SolveSwitches().sort_key_drop;
    if (const char* e = std::getenv("BIOIK_SOLVE_TWO_PHASE")) {
        w.two_phase_set = true;
        w.two_phase_init = std::strcmp(e, "init") == 0;
        for (const char* c = e; *c && !w.two_phase_init;) {
            char* end = nullptr;
            const long k = std::strtol(c, &end, 10);
            if (end == c) break;
            w.two_phase.push_back(k);
            c = *end == ',' ? end + 1 : end;
        }
    }
    if (const char* e = std::getenv("BIOIK_PHASE_DUMP")) w.phase_dump = e;
    if (const char* e = std::getenv("BIOIK_SOLVE_HANDOVER_DUMP")) w.handover_dump = e;
    return w;
}
static std::mutex g_switch_mtx;
static SolveSwitches apply_switches(SolveSwitches w) {  // (what the back end itself reads of them)
#if !defined(BIOIK_BACKEND_HEADER)
    g_memset_nodes = w.memset_nodes;
#endif
    return w;
}
static SolveSwitches g_switches = apply_switches(parse_switches());
static SolveSwitches switches() {
    std::lock_guard<std::mutex> lock(g_switch_mtx);
    return g_switches;
}

// lanes per (query, island).  The two species run concurrently on two lane groups when the workgroup has >= 2 wavefronts;
// each group gets one lane per child up to 128 lanes (pop=128 -> 256 lanes: 4 wavefronts on the 4 SIMDs of a CU).
static int solve_threads(const DevSolveParams& sp, uint64_t units, const SolveSwitches& sw, uint64_t cus) {
    int t;
    if (sw.threads > 0) {
        t = sw.threads;
    } else {
        // one wavefront per species, two children per lane and trip at pop=128: every wavefront is busy in every phase; with
        // children evaluated in pairs this is also as fast per query as one lane per child (measured: 165 vs 161 us per
        // step for a lone query, 95 k vs 84 k solves/s at batch 1024)
        int per_species = sp.lambda > 32 ? 64 : 32;
        t = 2 * per_species;
        // a launch that cannot fill the chip anyway (a single query of the plugin, a few hundred queries): one lane per child,
        // two wavefronts per species — a lone step takes 131 instead of 141 us, 1024 queries run 6 % faster; beyond ~768
        // queries the 128-lane mapping wins (profiles/r01_batch_sweep.log, r01_lone_workgroup_phases.log)
        if (sp.lambda >= 128 && units <= 3 * cus) t = 256;  // (768 on MI355X)
    }
    if (t < 64) t = 64;
    t = (t + 63) / 64 * 64;
    if (t > 256) t = 256;
    return t;
}

// every entry point runs on its handle's device and leaves the caller's current device as it found it
struct DeviceGuard {
    int prev;
    explicit DeviceGuard(int device) : prev(be_get_device()) {
        if (prev != device) be_set_device(device);
    }
    ~DeviceGuard() {
        if (be_get_device() != prev) {
            try {
                be_set_device(prev);
            } catch (...) {
            }
        }
    }
    DeviceGuard(const DeviceGuard&) = delete;
};

struct DevBuf {
    void* p = nullptr;
    const size_t bytes;
    explicit DevBuf(size_t bytes_) : p(be_alloc(bytes_)), bytes(bytes_) {}
    // ... filled from `src` on the default stream (null: left as allocated)
    DevBuf(const void* src, size_t bytes_) : DevBuf(bytes_) {
        if (src) be_h2d(p, src, bytes, 0);
    }
    void download(void* dst) const { be_d2h(dst, p, bytes, 0); }  // (enqueued: the caller waits for the default stream)
    ~DevBuf() { be_free(p); }
    DevBuf(const DevBuf&) = delete;
    template <class T>
    T* as() const { return (T*)p; }
};

// The two lane mappings with a kernel compiled for exactly them, both with the children computed where they are read and walked in pairs:
static constexpr LaneMapping kWavePerSpecies{128, 1, 1, 1, 1};  // 128 lanes, a wavefront per species (k_solve_lean_cl4 and its helped build)
static constexpr LaneMapping kHalves{64, 1, 1, 1, 1};           // 64 lanes, the species on the halves of one wavefront (k_solve_lean_cl64w4, k_solve_lean_clj4)
static LaneMapping mapping_of(const DevSolveParams& sp, int lanes) { return LaneMapping{lanes, sp.species_parallel, sp.child_cols, sp.child_pairs, sp.columnless}; }
static void set_mapping(DevSolveParams& sp, int& lanes, const LaneMapping& m) {
    lanes = m.lanes, sp.species_parallel = m.species_parallel, sp.child_cols = m.child_cols, sp.child_pairs = m.child_pairs, sp.columnless = m.columnless;
}
// the LDS layout of a solve's workgroup under a lane mapping: solve_layout (bioik_kernels.h), the function solve_setup takes its own layout from
static LdsLayout solve_layout(const DevProblem& d, int lambda, bool exact, const LaneMapping& m, bool helped = false, bool bounded = false) {
    return solve_layout(d.n_ops, d.V, d.P, d.T, d.n_slots, d.n_secondary > 0, lambda, exact, m, helped, bounded);
}
// the dynamic LDS of a function-level kernel of `nth` lanes, in bytes: the layout the eval_*_body / stream_fitness_body functions index (bioik_kernels.h)
static size_t eval_lds_bytes(const bioik_problem* p, int nth) {
    const DevProblem& d = p->host.dev;
    return (size_t)make_layout(d.n_ops, d.V, d.P, d.T, d.n_slots, nth, 0, 0).total * 8;
}
// The dynamic LDS of a function-level launch (a kernel of BIOIK_WIDE_LDS_KERNELS): a problem whose need is beyond a CU's LDS is refused before anything is
// allocated or launched, a need above 64 KiB is allowed for the kernel.  (Every problem bioik_problem_create accepts runs or is refused here: 64 tips x 64 ops
// need about 290 KiB, tables of 7 T m doubles.)
static size_t eval_lds(const bioik_problem* p, size_t bytes) {
    if (bytes > p->model->dev.lds_cu)
        throw Error(BIOIK_ERR_UNSUPPORTED, "problem needs " + std::to_string(bytes) + " B of LDS per workgroup for this entry point, more than a CU has");
    if (bytes > 64 * 1024) be_allow_lds(bytes);
    return bytes;
}

// a problem a lean kernel can run (bioik_platform.h, pb_flavour): no floating / planar joints, ops that meet the genes in gene order, no BalanceGoal, no TouchGoal, no
// ClearanceGoal (either one puts its tables into touch_points: the buffer is there exactly for a problem with one of the two), no based goal
// a problem with a based goal (BASE LINKS, include/bioik_hip.h): some tip holds its frame for a later one
static bool has_based_goal(const DevProblem& d) {
    for (int t = 0; t < d.T; t++)
        if (d.tips[t].pad0 != 0) return true;
    return false;
}
static bool lean_capable(const DevProblem& d) {
    return d.multi_op < 0 && d.n_quat == 0 && d.genes_follow_ops != 0 && d.n_balance == 0 && d.touch_points == nullptr && !has_based_goal(d);
}

// the timeout of a solve on the device clock (bioik_problem: clock_*)
static void set_deadline(bioik_problem* p, const DevSolveParams& sp, stream_t stream, bool captured, SolveArgs& a) {
    a.launch_clock = nullptr, a.deadline = 0ull;
    if (sp.timeout_ticks == 0) return;
    if (captured) {
        if (p->clock_next >= bioik_problem::kCaptureClocks) throw Error(BIOIK_ERR_UNSUPPORTED, "more than 64 solves with a timeout captured into hipGraphs on one problem handle");
        a.launch_clock = p->d_clocks + p->clock_next++;
        be_zero_async(a.launch_clock, sizeof(unsigned long long), stream);
        return;
    }
    const auto now = std::chrono::steady_clock::now();
    if (!p->clock_valid || now - p->clock_host0 > std::chrono::seconds(4)) {
        try {
            // (the first reading of a process pays for the reader's stream, its page-locked word and the kernel's first launch -- milliseconds, with the kernel at their
            // END: paired with the middle of that interval the deadline of every call of the next four seconds came ~3 ms late, tools/timeout_probe.py.  So: one
            // reading to set things up, then the pairing from the tighter of two)
            if (!p->clock_valid) (void)be_device_clock_now();
            std::chrono::steady_clock::duration best = std::chrono::steady_clock::duration::max();
            for (int attempt = 0; attempt < 2; attempt++) {
                const auto t0 = std::chrono::steady_clock::now();
                const unsigned long long dev = be_device_clock_now();
                const auto t1 = std::chrono::steady_clock::now();
                if (t1 - t0 < best) best = t1 - t0, p->clock_dev0 = dev, p->clock_host0 = t0 + (t1 - t0) / 2;  // (the kernel ran somewhere between the two readings: +- half the ~30 us between them)
            }
            p->clock_valid = true;
        } catch (const Error&) {
            if (!p->clock_valid) throw;  // (a reading that is a few seconds old still serves: the clocks drift by parts per million)
        }
    }
    const double since = std::chrono::duration<double>(std::chrono::steady_clock::now() - p->clock_host0).count();
    a.deadline = p->clock_dev0 + (unsigned long long)(since * 1e8) + sp.timeout_ticks;
}

// ------------------------------------------------------------------------------------------------------------
// One solve = SolveLauncher: what the call was given, where its results go (scratch, result_arrays, select_islands), the lane mapping the rules below pick
// for it (choose_mapping), the kernel that mapping is compiled as (choose_kernel: a row of BIOIK_SOLVE_KERNELS, which launch reports by the row's name and hands to
// launch_kernel), and the launches it is cut into (plan_handovers, run).  launch_solve at the end puts them in order.
// ------------------------------------------------------------------------------------------------------------
struct SolveLauncher {
    bioik_problem* p;
    DevSolveParams sp;
    const SolveArrays call;  // (device pointers, or the page-locked arena of a host-pointer call)
    const size_t n;
    stream_t stream;
    const bool captured;  // the stream is being captured into a hipGraph (asked once per solve, by launch_solve's caller)
    const SolveSwitches& sw;
    unsigned int* error_word;
    const DevProblem& dp;
    const size_t kLds;    // LDS of a CU (160 KiB on MI355X)
    const uint64_t kCus;
    uint64_t units = 0;
    void* island_ws = nullptr;  // (a stream-ordered fallback allocation of the per-island results, if any)
    bool fused_select = false;
    const bool bounded;  // per-query variable bounds (SolveArrays::var_lo / var_hi): the bounded rows of the kernel table, and their LDS layout
    const RankedArgs* ranked = nullptr;  // bioik_solve_batch_ranked: the per-island arrays are ranked by k_select_ranked (k, min_distance and the outputs: here), never reduced to one
    // the mapping (choose_mapping)
    int nth = 0, groups = 1;
    size_t lds = 0;
    bool exact = false, quat = false, manual = false, can_columnless = false, prefer_cl4 = false, small_sec_cl4 = false, small_linear = false, throughput = false, dense_ok = false,
         one_launch_capture = false, latency_drain = false, dense = false, lean = false, halves_ok = false, halves_shape = false, dense_shape = false;
    // the launches (plan_handovers)
    std::vector<int> handovers;  // the steps after which the unsolved units pass to the next launch (ascending)
    bool when_draining = false;  // ... or: whenever the chip runs empty (SolveArgs::resident), every unit from the step it is at
    bool migrating = false;      // ... or: the boundaries of bioik_solve_params::island_migration, with k_migrate_mark and k_migrate between two launches

    SolveLauncher(bioik_problem* p_, const DevSolveParams& sp_in, const SolveArrays& arrays, stream_t s, bool captured_, const SolveSwitches& w, unsigned int* err)
        : p(p_), sp(sp_in), call(arrays), n(arrays.n), stream(s), captured(captured_), sw(w), error_word(err), dp(p_->host.dev), kLds(p_->model->dev.lds_cu), kCus((uint64_t)p_->model->dev.cus), bounded(arrays.bounded()) {
        if (dp.n_secondary > 0 && sp.lambda < 2) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "population must be >= 2 when secondary goals are present");
        units = (uint64_t)n * sp.islands;
        if (units > 0x7fffffffull) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "too many (query, island) units for one launch: split the batch");
    }
    ~SolveLauncher() { be_free_async(island_ws, stream); }
    SolveLauncher(const SolveLauncher&) = delete;
    struct AsyncFree {
        void*& p;
        stream_t s;
        ~AsyncFree() { be_free_async(p, s); }
    };

    // scratch of this solve: the handle's persistent buffer for (stream, purpose), or -- while the stream is being captured and the buffer would have to
    // grow, or for the sixty-fifth stream of a handle -- a stream-ordered allocation released on every path out (null: nothing to release)
    // (*entry: the handle's record of (stream, purpose), if it holds one -- whether or not the pointer returned is that record's buffer)
    void* scratch(int purpose, size_t bytes, void*& async_owned, bioik_problem::Scratch** entry = nullptr) {
        const auto key = std::make_pair(stream, purpose);
        auto it = p->scratch.find(key);
        if (it == p->scratch.end() && p->scratch.size() < 128) it = p->scratch.emplace(key, bioik_problem::Scratch{}).first;
        if (it != p->scratch.end()) {
            bioik_problem::Scratch& sc = it->second;
            if (entry) *entry = &sc;
            if (captured) {
                for (const auto& r : p->retired_scratch)
                    if (r.stream == stream && r.purpose == purpose && r.capacity >= bytes) return r.base;  // (pinned by an earlier capture on this stream)
                if (sc.capacity >= bytes) {
                    sc.pinned = true;  // (the graph being captured keeps this address: see bioik_problem::Scratch)
                    return sc.base;
                }
                // (a stream-ordered allocation inside the capture would replay once and abort at the second replay on this ROCm: refuse, and say what to do)
                throw Error(BIOIK_ERR_UNSUPPORTED, "a solve captured into a hipGraph needs scratch memory this handle does not hold yet for the stream: run ONE eager call of the same size "
                                                   "(queries, islands) on the stream before capturing");
            } else {
                if (sc.pinned) p->retired_scratch.push_back(bioik_problem::Retired{sc.base, sc.capacity, stream, purpose}), sc = bioik_problem::Scratch{};
                if (sc.capacity >= bytes) return sc.base;
                // (stream-ordered on THIS stream, kept until it has to grow or the handle goes: no call here waits for the device -- hipMalloc / hipFree do, which
                // cost the first solves of a pipeline over the handle's six streams a factor of three)
                be_free_async(sc.base, stream);
                sc = bioik_problem::Scratch{};  // (the control words too: a new buffer holds none, even where the allocator hands the old address out again)
                sc.base = be_alloc_async(bytes + bytes / 2, stream), sc.capacity = bytes + bytes / 2;
                return sc.base;
            }
        }
        async_owned = be_alloc_async(bytes, stream);
        return async_owned;
    }
    // where the launch writes its results: the caller's arrays, or (islands > 1) per-island arrays that are then reduced to them -- by the query's last island
    // itself (`fused`: SolveArgs::island_done; one launch in all) or by k_select behind the solve's launches (select_islands)
    void result_arrays(SolveArgs& args, bool fused) {
        if (sp.islands == 1) {
            args.solutions = call.solutions, args.fitness = call.fitness, args.success = call.success, args.steps = call.steps;
            return;
        }
        const size_t ctl_n = fused ? std::max<size_t>(n, 256) : 0;  // (the control words of the fused form: room for calls of up to this many queries)
        const auto layout = [&](size_t ctl_words) { return bioik::island_scratch_layout(n, (size_t)sp.islands, (size_t)dp.V, ctl_words, sp.island_sync != 0); };
        // Eager: control words at rest from an earlier fused call with a larger ctl_n stay where they are, and this call's arrays go behind THEM -- the layout the
        // buffer is requested with counts them.  Captured: the graph sets up its own words on every replay (other graphs on the same pinned buffer lay it out their own way).
        size_t prior = 0;
        if (fused && !captured) {
            auto it = p->scratch.find(std::make_pair(stream, 0));
            if (it != p->scratch.end()) prior = it->second.words_at_rest();
        }
        bioik::IslandScratchLayout L = layout(std::max(prior, ctl_n));
        bioik_problem::Scratch* sc = nullptr;
        void* const w = scratch(0, L.bytes, island_ws, &sc);
        if (sc && sc->base != w) sc = nullptr;  // (a retired buffer: pinned, no eager call's)
        if (fused) {
            size_t have = !captured && sc ? sc->words_at_rest() : 0;
            const bool set_up = have < n;  // a new buffer, a larger call, a call of the other kind in between, or a capture: set the words up (the kernels keep them from then on)
            if (set_up) have = ctl_n;
            if (have > L.ctl_words) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "internal: the islands' scratch was requested for fewer control words than it is laid out with");
            if (have < L.ctl_words) L = layout(have);  // (a buffer that had to grow holds no earlier call's words: this call's own, in fewer bytes than were asked for)
            if (set_up) {
                be_fill_ff_async(L.first_success.at(w), L.first_success.bytes(), stream);
                be_zero_async(L.island_done.at(w), L.island_done.bytes(), stream);
                if (sc && captured) sc->forget_words();  // (a pinned buffer is never an eager call's again)
                else if (sc) sc->words_set_up(w, ctl_n);
            }
            if (sw.report) std::fprintf(stderr, "[bioik] islands: reduced by the last island in the launch (control words of %zu queries)\n", have);
            if (L.sync) args.first_success = L.first_success.at(w);
            args.island_done = L.island_done.at(w);
            args.final_solutions = call.solutions, args.final_fitness = call.fitness, args.final_success = call.success, args.final_steps = call.steps;
            fused_select = true;
        } else {
            if (sc) sc->forget_words();  // (this call lays the buffer out its own way)
            if (L.sync) {  // "any island succeeds => all stop": the least step count of a passing island, per query (0xffffffff: none yet)
                args.first_success = L.first_success.at(w);
                be_fill_ff_async(args.first_success, L.first_success.bytes(), stream);
            }
        }
        args.solutions = L.solutions.at(w), args.fitness = L.fitness.at(w), args.success = L.success.at(w), args.steps = L.steps.at(w);
    }
    void select_islands(const SolveArgs& args) {  // ik_parallel.h:220-269: the best island of every query
        if (ranked) {  // ... or its k best distinct ones, in that order (islands = 1: the solve wrote the row itself, the kernel adds the count)
            RankedArgs r = *ranked;
            r.pb = p->pb(), r.islands = sp.islands, r.V = dp.V, r.D = dp.D, r.n = n, r.seeds = call.seeds;
            r.isl_solutions = args.solutions, r.isl_fitness = args.fitness, r.isl_success = args.success, r.isl_steps = args.steps;
            const size_t lds_r = r.min_distance >= 0.0 && sp.islands > 1 ? (size_t)dp.D * 64 * 8 : 0;  // (at most 63 x 64 doubles: 31.5 KiB)
            if (sw.report) std::fprintf(stderr, "[bioik] launch: k_select_ranked, islands %d, k %d, %zu B of LDS\n", (int)sp.islands, (int)r.k, lds_r);
            LAUNCH(k_select_ranked, select_ranked(r, b_, p_tid(), l_), n, 64, lds_r, stream, r);
            return;
        }
        if (sp.islands == 1 || fused_select) return;
        SelectArgs s;
        s.islands = sp.islands, s.V = dp.V, s.n = n;
        s.sync = sp.island_sync, s.pad = 0;
        s.isl_solutions = args.solutions, s.isl_fitness = args.fitness, s.isl_success = args.success, s.isl_steps = args.steps;
        s.solutions = call.solutions, s.fitness = call.fitness, s.success = call.success, s.steps = call.steps;
        const bool wave = sp.islands >= 8 && n <= 4096 && sw.fused_select >= 0;
        if (sw.report) std::fprintf(stderr, "[bioik] launch: %s, islands %d\n", wave ? "k_select_wave" : "k_select", (int)sp.islands);
        if (wave) LAUNCH(k_select_wave, select_coop(s, b_, p_tid()), n, 64, 0, stream, s);
        else LAUNCH(k_select, select_body(s, b_ * 256 + (uint64_t)p_tid()), (n + 255) / 256, 256, 0, stream, s);
    }
    // gd / gd_r / gd_c / jac: one wavefront per (query, island), its own (small) LDS layout
    void solve_point() {
        const size_t lds_point = (size_t)make_point_layout(dp.n_ops, dp.V, dp.P, dp.T, dp.n_slots, dp.D, 64, bounded ? 1 : 0).total * 8;
        if (lds_point > 64 * 1024) throw Error(BIOIK_ERR_UNSUPPORTED, "problem too large for the gd / jac kernels (more than 64 KiB of LDS per query)");
        SolveArgs pa;
        pa.pb = p->pb(), pa.sp = sp, pa.seeds = call.seeds, pa.params = call.goal_params;
        pa.var_lo = call.var_lo, pa.var_hi = call.var_hi;
        result_arrays(pa, false);
        pa.phase_cycles = nullptr;
        set_deadline(p, sp, stream, captured, pa);
        const SolveKernel kind = bounded ? SolveKernel::k_solve_point_bounded : SolveKernel::k_solve_point;
        if (sw.report) std::fprintf(stderr, "[bioik] launch: %s, 64 lanes, %zu B of LDS\n", kSolveKernelNames[(int)kind], lds_point);
        launch_kernel(kind, pa, units, 64, lds_point, stream);
        select_islands(pa);
    }
    size_t lds_need(const LaneMapping& m, bool helped = false) const { return (size_t)solve_layout(dp, sp.lambda, exact, m, helped, bounded).total * 8; }  // bytes of LDS per workgroup
    void choose_mapping() {
        // Mapping of a (query, island) onto lanes.  Candidates: 128 lanes (one wavefront per species) with every child kept in LDS
        // and evaluated in pairs / kept / re-derived from the RNG, or 64 lanes (one wavefront, the species one after the other).  A CU
        // holds 160 KiB of LDS and, at this kernel's register budget, 12 wavefronts: the candidate that puts most wavefronts on a CU
        // wins; among equals the richer mapping wins when the CU is full (C2: 20 KiB per workgroup) and the leaner one when LDS is
        // what limits residency (C3, C4: measured +7 % and +26 % for 64 lanes, tools/mapping_sweep.py).
        nth = solve_threads(sp, units, sw, kCus);
        exact = sp.fk_mode == BIOIK_FK_EXACT;  // (the LDS layout of exact-FK solves is smaller, make_layout)
        if (sw.threads <= 0 && nth == 256 && lds_need(LaneMapping{256, 1, 1, 0, 0}) > 48 * 1024) nth = 128;  // LDS-heavy problem
        quat = dp.n_quat > 0;  // winners re-derived: their momentum is taken before the quaternion genes are renormalised
        manual = sw.manual();
        // children computed where they are read (no genotype columns in LDS): the lean flavour can, whenever it is chosen below
        can_columnless = lean_capable(dp) && !sw.general_set && !bounded;  // (a bounded call: the general flavour's kernel with the query's table, k_solve_bounded, and no other)
        sp.columnless = 0;
        // the problems the mapping with both species on the halves of one wavefront exists for (kHalves: the first launch of a solve in two, plan_handovers), and those
        // among them the dense kernel is compiled for (the throughput schedule's whole solve, the latency schedule's chip-filling start: `throughput`, `dense_ok` below)
        halves_shape = can_columnless && exact && sp.lambda >= 128 && dp.D < 32;
        dense_shape = halves_shape && sp.lambda <= 256 && dp.n_secondary == 0;
        // k_solve_lean_cl4's mapping first -- 128 lanes, a wavefront per species, children computed where they are read and walked in pairs, the kernel compiled
        // for exactly that under the budget of four wavefronts per SIMD (no register spills since round 4): for problems without a secondary goal whose
        // lanes get at least one pair of children per generation and whose LDS footprint lets sixteen wavefronts share a CU it beats the kernel with the
        // children kept in columns on every count (C2: lone step 94 -> 91 us, fixed work at 4096 queries +30 %, three solves in flight +26 %, an isolated
        // call +16 %: profiles/r04_ab_latency_schedule_kernel.log)
        const bool cl4_shape = !manual && !sw.three_waves && can_columnless && exact && dp.serial_chain != 0 && !(dp.n_quat > 0) && sp.lambda >= 128 &&
                               lds_need(kWavePerSpecies) * 8 <= kLds;  // (what the rule above and the one below ask of a problem alike)
        const bool cl4_eligible = cl4_shape && dp.n_secondary == 0;
        // (... also for the launches that cannot fill the chip, where solve_threads asks for a lane per child: one query 0.928 against 0.942 ms, 256 queries 5.49 against
        // 5.74 ms, profiles/r04_small_batches.log)
        if (cl4_eligible && nth == 256) nth = 128;
        prefer_cl4 = cl4_eligible && nth == 128;
        // ... and, for launches small enough for its helped build (k_solve_lean_cl4h), the same mapping for serial chains WITH secondary goals (a 7-joint arm with a
        // MinimalDisplacementGoal, the 31-joint chain with AvoidJointLimitsGoal: the usual MoveIt configurations of bio_ik): the kernel pre-selects, the helper takes
        // half of the survivors' walks.  Chip-filling batches of such problems keep the mappings chosen below (the joint walk, the 128-register build by residency).
        small_sec_cl4 = cl4_shape && dp.n_secondary > 0 && sw.helped > 0 && units <= (uint64_t)sw.helped;
        if (prefer_cl4 || small_sec_cl4) {
            set_mapping(sp, nth, kWavePerSpecies);
        } else if (!manual && nth == 128) {
            // richest first: children kept in LDS and scored in pairs / kept / computed where they are read / one reusable column per lane.  (128 lanes: a wavefront
            // per species; 64: the species one after the other.  Either way a species has 64 lanes: `all` columns keep every child of a generation)
            const int all = (sp.lambda + 63) / 64;
            const LaneMapping cands[] = {{128, 1, all, 1, 0}, {128, 1, all, 0, 0}, {128, 1, 1, 1, 1}, {128, 1, 1, 0, 1}, {128, 1, 1, 0, 0}, {64, 0, 1, 1, 1}, {64, 0, 1, 0, 1}, {64, 0, 1, 0, 0}};
            const int kCuWaves = 4 * BIOIK_SOLVE_WAVES_PER_SIMD;  // wavefronts a CU holds at this kernel's register budget
            int best = -1, best_waves = -1;
            for (int i = 0; i < 8; i++) {
                const LaneMapping& c = cands[i];
                if ((c.child_cols > 1 || c.child_pairs) && quat) continue;  // (child_cols > 1: the children kept)
                if (c.columnless && !can_columnless) continue;
                if (c.child_pairs && !exact) continue;
                if (c.child_pairs && !c.columnless && c.child_cols < 2) continue;
                // (computed children in pairs: measured +1.5 % with eight children per lane and generation (C4), -4 % with two (C3))
                if (c.child_pairs && c.columnless && sp.lambda < 4 * 64) continue;
                const size_t bytes = lds_need(c);
                if (bytes > kLds) continue;
                int waves = (int)(kLds / bytes) * (c.lanes / 64);
                if (waves > kCuWaves) waves = kCuWaves;
                // full CU: first (richest) candidate wins; LDS-limited: a later (leaner) candidate wins ties
                if (waves > best_waves || (waves == best_waves && waves < kCuWaves)) best = i, best_waves = waves;
            }
            if (best < 0) throw Error(BIOIK_ERR_UNSUPPORTED, "problem needs more LDS per workgroup than a CU has");
            set_mapping(sp, nth, cands[best]);
            // Problems with secondary goals score only a random prefix of the pre-selected children, so the phases besides the chain walk (the
            // pre-selection itself, selection, the memetic phase) weigh more; with both species of a query on the halves of ONE wavefront those
            // run once for the two.  Measured: C3 (128 children per species) +14 %, C4 (512: sixteen children per lane) -22 % (tools/c34_mapping_probe.sh).
            if (sp.columnless && dp.n_secondary > 0 && exact && sp.lambda >= 128 && sp.lambda <= 256 && dp.D < 32 && lds_need(kHalves) * kCuWaves <= kLds)
                set_mapping(sp, nth, kHalves);
        } else {
            while (nth > 64 && lds_need(LaneMapping{nth, 1, 1, 0, 0}) > 64 * 1024) nth -= 64;  // genotype columns scale with the lane count
            // two lane groups, one species each: whole wavefronts (128 / 256 lanes), or the two halves of one wavefront (64 lanes)
            // (small populations, <= 32 children per species: +65..80 % measured, tools/halfwave_sweep.sh; at 64 and more children
            // per species the sequential single wavefront or the two-wavefront mapping is as good or better)
            sp.species_parallel = (nth % 128 == 0 || (nth == 64 && sp.lambda <= 32 && dp.D < 32)) ? 1 : 0;  // (the memetic phase wants lane D of a group)
            if (sw.species_parallel >= 0) sp.species_parallel = (sw.species_parallel != 0 && (nth % 128 == 0 || (nth == 64 && dp.D < 32))) ? 1 : 0;
            const int groups_m = sp.species_parallel ? 2 : 1, G_m = nth / groups_m;
            sp.child_cols = (sp.lambda + G_m - 1) / G_m;
            if (quat) {
                sp.child_cols = 1;
            } else if (sw.store_children >= 0) {
                if (sw.store_children == 0) sp.child_cols = 1;
            } else if (lds_need(LaneMapping{nth, sp.species_parallel, sp.child_cols, 0, 0}) > 48 * 1024) {
                sp.child_cols = 1;
            }
            // children two at a time per lane (two independent dependency chains): needs both columns of the pair and, for branching
            // trees, a second set of parked frames
            sp.child_pairs = (sp.child_cols >= 2 && exact && lds_need(LaneMapping{nth, sp.species_parallel, sp.child_cols, 1, 0}) <= 64 * 1024) ? 1 : 0;
            if (sw.child_pairs == 0) sp.child_pairs = 0;
        }
        // small populations, linearised phenotypes (the reference's own parameters), both species on the halves of one wavefront: children computed where
        // they are read, and the kernel compiled for exactly that (k_solve_lean_lin: sixteen queries per CU)
        small_linear = !manual && !sw.three_waves && can_columnless && !exact && nth == 64 && sp.species_parallel && sp.lambda <= 32 && sp.solver == 0;
        if (small_linear) sp.columnless = 1, sp.child_cols = 1, sp.child_pairs = 0;
        // BIOIK_SCHEDULE_THROUGHPUT: the whole solve under the mapping that retires most steps per ms on a full chip -- both species of a query on the
        // halves of one wavefront, children computed where they are read and scored in pairs (the first launch's mapping of the two-launch solve
        // below) -- for callers that keep six or more batches in flight (include/bioik_hip.h; profiles/r03_inflight_and_schedule.log)
        throughput = sp.schedule == BIOIK_SCHEDULE_THROUGHPUT && !manual && dense_shape;
        // (nth / sp keep the LATENCY mapping: a throughput solve may hand its stragglers over to it, sw.dense_handover; its own launch takes the
        // dense mapping where it is made, `halves` below)
        // k_solve_lean_cl64w4 (solve_body<.., DENSE>): the 128-register build of that mapping, four wavefronts per SIMD
        // BIOIK_SCHEDULE_LATENCY, a batch beyond what the chip holds of k_solve_lean_cl4's workgroups (2048; 2048 queries: 7.27 ms alone, 7.51 ms this way) under its mapping: the dense kernel first -- every query of up to 4096
        // resident from the start, most steps retired per ms while the chip is full -- and, when the chip runs empty, the stragglers on to k_solve_lean_cl4 whose lone
        // step is a third shorter (SolveArgs::resident).  An isolated 4096-query call: 9.2 -> 8.5 ms (profiles/r04_drain_handover.log).  Streams of solves keep the
        // chip full, never see the hand-over and pay for its bookkeeping: the throughput schedule does without (BIOIK_SOLVE_DRAIN_THROUGHPUT=1: with).
        dense_ok = !manual && dense_shape && !sw.three_waves && dp.serial_chain != 0;  // (can_columnless: a lean-capable problem)
        // (BIOIK_SOLVE_CAPTURE_ONE_LAUNCH=1: round 4's rule -- a call on a stream that is being captured gets a one-launch mapping.  The replay defect it worked around
        // was the runtime's memset NODE in front of the kernels, not the hand-over; the library fills its words with a kernel of its own now
        // and captured calls take the same mapping as eager ones)
        one_launch_capture = sw.capture_one_launch && captured;
        latency_drain = sp.schedule != BIOIK_SCHEDULE_THROUGHPUT && prefer_cl4 && dense_ok && units >= (uint64_t)(sp.islands <= 2 ? sw.drain_min_units : 3072) * kCus / 256 && sw.drain_below > 0 && sp.max_steps > sw.drain_min_steps + 1 &&
                                   !sw.two_phase_set && !one_launch_capture;
        dense = (throughput || latency_drain) && dense_ok;
        if (sw.columnless > 0 && can_columnless) {
            sp.columnless = 1, sp.child_cols = 1;
            sp.child_pairs = (sw.columnless == 2 && sp.fk_mode == BIOIK_FK_EXACT) ? 1 : 0;  // 2: children scored two at a time
        }
        groups = sp.species_parallel ? 2 : 1;
        lds = lds_need(mapping_of(sp, nth));
        if (lds > kLds) throw Error(BIOIK_ERR_UNSUPPORTED, "problem needs more LDS per workgroup than a CU has");
        lean = lean_capable(dp) && !(sw.general_set && sw.general) && !bounded;
        halves_ok = lean && halves_shape;  // the first launch's mapping exists for this problem
    }
    void report_mapping() const {  // diagnostics: the lane mapping and the residency it gives
        const LdsLayout L = solve_layout(dp, sp.lambda, exact, mapping_of(sp, nth), false, bounded);
        int n_rev = 0, n_pos = 0, n_rot = 0;  // revolute ops and how many of them the walk takes through a sparse form
        for (int k = 0; k < dp.n_chain_ops; k++)
            if (dp.ops[k].type == BIOIK_OP_REVOLUTE) n_rev++, n_pos += dp.ops[k].pos_kind != BIOIK_POS_GENERAL, n_rot += dp.ops[k].rot_kind != BIOIK_ROT_GENERAL;
        std::fprintf(stderr, "[bioik] joint program: %d revolute ops, sparse position %d, sparse rotation %d\n", n_rev, n_pos, n_rot);
        std::string prog;  // op (source, gene): the shape of the tree the walk takes
        for (int k = 0; k < dp.n_chain_ops; k++) {
            char buf[48];
            std::snprintf(buf, sizeof buf, " %d(%d,%d%s%s)", k, (int)dp.ops[k].src, (int)dp.ops[k].gene, dp.ops[k].load_slot >= 0 ? ",load" : "", dp.ops[k].save_slot >= 0 ? ",save" : "");
            prog += buf;
        }
        std::fprintf(stderr, "[bioik] joint program: prefix %d, serial %d, op(source,gene):%s\n", (int)dp.n_prefix, (int)dp.serial_chain, prog.c_str());
        std::fprintf(stderr, "[bioik] solve: ops %d genes %d tips %d slots %d | lanes %d species_parallel %d child_cols %d pairs %d columnless %d | LDS %zu B "
                     "(genotype columns %d, parked frames %d, per-group %d x %d) -> %d workgroups = %d wavefronts per CU\n",
                     dp.n_ops, dp.D, dp.T, dp.n_slots, nth, sp.species_parallel, sp.child_cols, sp.child_pairs, sp.columnless, lds, (L.slots - L.xcol) * 8,
                     (L.g_first - L.slots) * 8, L.g_stride * 8, groups, (int)(kLds / lds), (int)(kLds / lds) * (nth / 64));
    }
    // the kernel a launch of `lanes` lanes and `lds_b` bytes of LDS under the mapping of args.sp is compiled as
    SolveKernel choose_kernel(const SolveArgs& args, int lanes, size_t lds_b) const {
        // computed children: the 128-register build when a CU's LDS holds at least the 16 wavefronts it makes room for and a lane walks
        // at least eight children per generation (the generation loops, which fit the smaller budget, are then most of a step)
        const int group_lanes = lanes / (args.sp.species_parallel ? 2 : 1);
        // (k_solve_lean_cl4 is compiled for exactly this mapping -- solve_body<.., FIXED = 2> --: 128 lanes, a wavefront per species, exact FK, children in pairs)
        const bool cl4_mapping = lanes == 128 && args.sp.species_parallel && args.sp.child_pairs && args.sp.fk_mode == BIOIK_FK_EXACT && dp.serial_chain != 0;
        const bool four_waves = cl4_mapping && (((kLds / lds_b) * (size_t)(lanes / 64) >= 16 && (args.sp.lambda >= 8 * group_lanes || prefer_cl4 || small_sec_cl4) && !sw.three_waves) ||
                                                sw.four_waves);  // (diagnostic: the 128-register build wherever its mapping is the one in use)
        // both species on one wavefront, secondary goals, exact FK, children in pairs: the joint walk of the two species' children
        // (with a wavefront per species -- 128 lanes, C4 -- the same walk gains nothing: a wavefront that waits at a barrier costs no issue slots,
        // profiles/r03_ab_joint_walk.log)
        const bool joint = lanes == 64 && args.sp.species_parallel && args.sp.child_pairs && dp.n_secondary > 0 && args.sp.fk_mode == BIOIK_FK_EXACT &&
                           !sw.no_joint;
        const bool dense_launch = lanes == 64 && dense && args.sp.species_parallel && args.sp.child_pairs && args.sp.columnless;  // (what solve_body<.., FIXED = 1> is compiled for)
        const bool lin_launch = small_linear && lanes == 64 && args.sp.species_parallel && args.sp.columnless && !args.sp.child_pairs && args.sp.fk_mode == BIOIK_FK_LINEAR;
        // k_solve_lean_cl4's helped build: launches that leave most of the chip idle (every unit gets four wavefronts instead of two), and the stragglers of a
        // chip-filling call (the list is a fraction of the grid)
        // (since its second version also for problems with secondary goals -- the 31-joint chain with AvoidJointLimitsGoal --: the helper takes the upper half of the
        // pre-selected children's walks)
        const bool helped_launch = lean && four_waves && !manual && !sw.four_waves && args.sp.columnless && sw.helped > 0 &&
                                   (units <= (uint64_t)sw.helped || (args.unit_list != nullptr && args.resident != nullptr));
        if (helped_launch) return SolveKernel::k_solve_lean_cl4h;
        if (bounded) return SolveKernel::k_solve_bounded;
        if (!lean) return SolveKernel::k_solve;
        if (lin_launch) return SolveKernel::k_solve_lean_lin;
        if (!args.sp.columnless) return SolveKernel::k_solve_lean;
        if (joint) return SolveKernel::k_solve_lean_clj4;
        if (dense_launch) return SolveKernel::k_solve_lean_cl64w4;
        return four_waves ? SolveKernel::k_solve_lean_cl4 : SolveKernel::k_solve_lean_cl;
    }
    void launch(const SolveArgs& args, int lanes, size_t lds_b) {
        const SolveKernel kind = choose_kernel(args, lanes, lds_b);
        const bool helped = kind == SolveKernel::k_solve_lean_cl4h;
        if (helped) {
            lds_b = lds_need(mapping_of(args.sp, lanes), true), lanes = 256;  // (the layout with the sixteen words of the hand-overs; two helper wavefronts beside the mapping's two)
            if (lds_b > 64 * 1024) be_allow_lds(lds_b);
        }
        if (sw.report)
            std::fprintf(stderr, "[bioik] launch: %s, %d lanes%s, %zu B of LDS, steps [%d, %d)\n", kSolveKernelNames[(int)kind], lanes,
                         helped ? " (two of the four wavefronts are helpers)" : "", lds_b, (int)args.step_begin, (int)(args.step_end < args.sp.max_steps ? args.step_end : args.sp.max_steps));
        launch_kernel(kind, args, units, lanes, lds_b, stream);
    }
    // One launch, or two (SolveArgs::step_begin ...).  Measured on streams of distinct 4096-query PoseGoal batches (profiles/r02_two_launch_sweep.log):
    // split after the first step(), the state of the unsolved queries handed over through HBM, the first launch with both species of a query on
    // the halves of ONE wavefront and the children computed where they are read, a stream of batches runs 2.6 % faster and an isolated call 3.5 %
    // (later hand-overs give the same on uniformly seeded queries and cost up to 11 % on tracking seeds, most of which are solved within six steps).
    // The second launch takes the queries in the order the first finished them: solves in flight whose long-running queries would otherwise
    // coincide (the same batch solved again on another stream) do not lose the 8 % such a coincidence costs.
    // BIOIK_SOLVE_TWO_PHASE=K (or K1,K2,... / init) forces hand-overs after those steps for any problem (0: never) -- the parity suites run every
    // mapping through it.
    void plan_handovers() {
        // island migration: the boundaries E, 2E, ... < max_steps, BIOIK_MAX_MIGRATIONS at most, instead of every other plan (one island, or no boundary below max_steps: the
        // call's plan is the one E = 0 takes)
        if (sp.island_migration > 0 && sp.islands > 1 && sp.solver == 0 && sp.island_migration < sp.max_steps) {
            if (captured) throw Error(BIOIK_ERR_UNSUPPORTED, "island_migration > 0 on a stream that is being captured into a hipGraph is not supported");
            migrating = true;
            for (long long k = sp.island_migration; k < (long long)sp.max_steps && handovers.size() < (size_t)BIOIK_MAX_MIGRATIONS; k += sp.island_migration) handovers.push_back((int)k);
            return;
        }
        if (sw.drain_test > 0 && sp.max_steps > 1 && sp.solver == 0) {
            when_draining = true;
            handovers.push_back(sp.max_steps);
        } else if (sw.two_phase_set) {  // "K" or "K1,K2,..." (experiments: more than one hand-over)
            if (sw.two_phase_init) handovers.push_back(0);  // (experiment: the first launch only initialises)
            for (const long k : sw.two_phase)
                if (k > (handovers.empty() ? 0 : handovers.back()) && k < sp.max_steps) handovers.push_back((int)k);
        } else if (throughput) {
            // the dense mapping retires most steps per ms but its steps are 2.5 x as long: the stragglers of a batch may pass to the latency mapping
            if (sw.dense_handover > 0 && sw.dense_handover < sp.max_steps) handovers.push_back(sw.dense_handover);
            else if (dense && prefer_cl4 && units >= 8 * kCus && sw.drain_throughput && sw.drain_below > 0 && sw.drain_below_throughput > 0 && sp.max_steps > sw.drain_min_steps + 1 && !one_launch_capture)
                when_draining = true, handovers.push_back(sp.max_steps);
        } else if (latency_drain) {
            when_draining = true, handovers.push_back(sp.max_steps);
        } else if (lean && dense_shape && !manual && !prefer_cl4 && units >= 8 * kCus && sp.max_steps >= 24 && !one_launch_capture) {
            // (not under k_solve_lean_cl4's mapping: there one launch is faster -- three in flight 9.9e5 against 9.3e5, an isolated call 8.9 against 9.3 ms,
            // profiles/r04_ab_latency_schedule_kernel.log)
            handovers.push_back(1);
        }
    }
    // the mapping with both species of a query on the halves of ONE wavefront, children computed where they are read and walked in pairs: the
    // first launch of a solve in several launches, and the whole of a throughput solve
    void halves(SolveArgs& aj, int& lanes, size_t& lds_j) {
        set_mapping(aj.sp, lanes, kHalves);
        lds_j = lds_need(kHalves);
        if (lds_j > 64 * 1024) be_allow_lds(lds_j);
    }
    // the launch(es) of a solve whose arguments `a` are complete
    void run(const SolveArgs& a) {
        if (handovers.empty() && throughput) {
            SolveArgs a0 = a;
            int lanes = nth;
            size_t lds_0 = lds;
            halves(a0, lanes, lds_0);
            launch(a0, lanes, lds_0);
        } else if (handovers.empty()) {
            launch(a, nth, lds);
        } else {
            const size_t nh = handovers.size();
            // (migration: one word per unit behind the counters, the number of the last boundary it was live at)
            const bioik::HandoverLayout H = bioik::handover_layout((size_t)units, (size_t)carry_doubles(dp.n_ops), nh, migrating);
            void* ws_async = nullptr;
            AsyncFree ws_guard{ws_async, stream};
            void* ws = scratch(1, H.bytes, ws_async);
            be_zero_async(H.cleared.at(ws), H.cleared.bytes(), stream);
            if (!sw.handover_dump.empty())
                if (FILE* f = std::fopen(sw.handover_dump.c_str(), "a")) {
                    std::fprintf(f, "%llu %zu %zu %llu %zu\n", (unsigned long long)(size_t)ws, H.lists_off, H.counters_off, (unsigned long long)units, H.carry_doubles);
                    std::fclose(f);
                }
            for (size_t j = 0; j <= nh; j++) {  // launch j runs the steps [handovers[j-1], handovers[j])
                SolveArgs aj = a;
                int lanes = nth;
                size_t lds_j = lds;
                if (j == 0 && halves_ok && !manual) halves(aj, lanes, lds_j);
                aj.carry = H.rows.at(ws);
                if (when_draining) {  // (the last launch counts its wavefronts too; it has no list to leave for)
                    aj.resident = p->d_resident;
                    {  // (per XCD -- eight on MI355X --, the threshold itself scaled to the chip's CUs: BIOIK_SOLVE_DRAIN_BELOW names it for 256 of them)
                        const int xcds = p->model->dev.xcds > 0 ? p->model->dev.xcds : 1;
                        const long long below = (long long)(throughput ? sw.drain_below_throughput : sw.drain_below) * (long long)kCus / 256;
                        aj.drain_below = sw.drain_test > 0 ? -sw.drain_test : (int32_t)((below + xcds - 1) / xcds);
                    }
                    aj.drain_min_steps = sw.drain_min_steps;
                }
                if (j > 0) {
                    aj.step_begin = when_draining ? -1 : handovers[j - 1];
                    aj.unit_list = H.list(j - 1).at(ws);
                    aj.unit_count = H.counter(j - 1).at(ws);
                }
                if (j < nh) {
                    aj.step_end = handovers[j];
                    aj.carry_list = H.list(j).at(ws);
                    aj.carry_count = H.counter(j).at(ws);
                }
                launch(aj, lanes, lds_j);  // (always a grid of `units` workgroups: those beyond the list's length leave at once)
                if (migrating && j < nh) {     // boundary j + 1: mark the units this launch handed over, then a wavefront per query rewrites its recipients' rows
                    MigrateArgs m;
                    m.islands = sp.islands, m.n_ops = dp.n_ops, m.exact = exact ? 1 : 0, m.mark = (int)j + 1, m.n = n;
                    m.list = aj.carry_list, m.count = aj.carry_count, m.live = H.marks.at(ws), m.rows = H.rows.at(ws);
                    if (sw.report) std::fprintf(stderr, "[bioik] launch: k_migrate_mark + k_migrate, boundary %d after step %d, islands %d\n", (int)j + 1, handovers[j], (int)sp.islands);
                    LAUNCH(k_migrate_mark, migrate_mark(m, b_ * 256 + (uint64_t)p_tid()), (units + 255) / 256, 256, 0, stream, m);
                    LAUNCH(k_migrate, migrate_coop(m, b_, p_tid()), n, 64, 0, stream, m);
                }
            }
        }
    }
};

// (captured: be_stream_capturing(stream), which the caller has asked -- once per solve)
static void launch_solve(bioik_problem* p, const DevSolveParams& sp_in, const SolveArrays& arrays, stream_t stream, bool captured, const SolveSwitches& sw, unsigned int* error_word,
                         const RankedArgs* ranked = nullptr) {
    if (sp_in.solver == 2 && has_based_goal(p->host.dev))
        throw Error(BIOIK_ERR_UNSUPPORTED, "BIOIK_MODE_JAC on a problem with a based goal (bioik_problem_desc::goal_base_link): its tip objectives are world poses; gd, gd_r and gd_c work");
    if (arrays.n == 0) return;
    SolveLauncher s(p, sp_in, arrays, stream, captured, sw, error_word);
    s.ranked = ranked;
    if (s.sp.solver != 0) return s.solve_point();
    s.choose_mapping();
    if (sw.report) s.report_mapping();
    if (s.lds > 64 * 1024) be_allow_lds(s.lds);
    SolveArgs a;
    a.pb = p->pb();
    a.sp = s.sp;
    a.seeds = arrays.seeds;
    a.params = arrays.goal_params;
    a.var_lo = arrays.var_lo, a.var_hi = arrays.var_hi;
    a.phase_cycles = nullptr;
    a.sort_key_drop = sw.sort_key_drop;
    a.preselect = sw.preselect | (sw.tie_test_bits << 8);
    a.error = error_word;
    a.debug_flags = sw.debug_flags;
    set_deadline(p, s.sp, stream, captured, a);
#if defined(BIOIK_PHASE_TIMING)
    DevBuf phase_buf(s.units * PHASE_SLOTS * sizeof(unsigned long long));
    const char* phase_path = sw.phase_dump.empty() ? nullptr : sw.phase_dump.c_str();
    if (phase_path) a.phase_cycles = phase_buf.as<unsigned long long>();
#endif
    s.plan_handovers();
#if defined(BIOIK_PHASE_TIMING)
    if (phase_path) s.handovers.clear();
#endif
    // (a solve in ONE launch reduces its islands itself, SolveArgs::island_done; BIOIK_SOLVE_FUSED_SELECT=0: by k_select as before)
    s.result_arrays(a, s.handovers.empty() && sw.fused_select > 0 && !ranked);  // (a ranked call keeps every island's result: never fused)
    s.run(a);
#if defined(BIOIK_PHASE_TIMING)
    if (phase_path) {  // profiling build only: synchronous dump of the per-phase cycle counters
        std::vector<unsigned long long> h(s.units * PHASE_SLOTS);
        be_d2h(h.data(), phase_buf.p, h.size() * sizeof(unsigned long long), stream);
        be_sync(stream);
        if (FILE* f = std::fopen(phase_path, "wb")) {
            std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
            std::fclose(f);
        }
    }
#endif
    s.select_islands(a);
}

// ------------------------------------------------------------------------------------------------------------
// The launcher's rules (launch_solve) were fitted to the three robots of BASELINE.json.  For a handle's FIRST chip-filling call of a kind under the latency
// schedule the entry points that may wait for their stream (the host-pointer ones; the device-pointer one under BIOIK_SOLVE_AUTOTUNE=2) run the call once
// per ELIGIBLE lane mapping -- every mapping returns the same bits, so each run is the caller's solve -- time it with events, keep the fastest in the handle
// and use it from then on (BIOIK_SOLVE_REPORT prints the table).  The presets are what the BIOIK_SOLVE_* switches can force; a preset the problem has no
// room or no kernel for is skipped.  Not for captured streams, solves with a timeout (their time is the caller's), the gradient family, or the throughput
// schedule (a lone call says nothing about a stream of ten: its dense mapping is the measured choice of profiles/r03_inflight_and_schedule.log).
// ------------------------------------------------------------------------------------------------------------
static const int kPresets = 5;
static const char* preset_name(int i) {
    static const char* names[kPresets] = {"the rules", "128 lanes, computed children in pairs (128-register build where it exists)", "64 lanes, species on the halves, computed children in pairs",
                                          "128 lanes, children kept in columns", "128 lanes, computed children one at a time"};
    return names[i];
}
static SolveSwitches preset_switches(const SolveSwitches& base, int i) {
    SolveSwitches w = base;
    if (i == 1) w.threads = 128, w.columnless = 2, w.four_waves = true;
    if (i == 2) w.threads = 64, w.species_parallel = 1, w.columnless = 2;
    if (i == 3) w.threads = 128;
    if (i == 4) w.threads = 128, w.columnless = 1;
    return w;
}
static void solve_dispatch(bioik_problem* p, const DevSolveParams& sp, const SolveArrays& arrays, stream_t stream, bool may_wait, unsigned int* error_word) {
    const SolveSwitches sw = switches();  // (the diagnostic switches as last parsed: no environment access on the launch path)
    const bool captured = be_stream_capturing(stream);
    auto run = [&](const SolveSwitches& w) { launch_solve(p, sp, arrays, stream, captured, w, error_word); };
    const uint64_t units = (uint64_t)arrays.n * (uint64_t)sp.islands;
    const bool kind_ok = !arrays.bounded() /* (a bounded call neither takes nor changes the measured choice, as the ranked entries) */ && sw.autotune > 0 && !sw.manual() && !sw.general_set && !sw.two_phase_set && sw.drain_test == 0 && sw.dense_handover == 0 && sp.solver == 0 &&
                         sp.schedule != BIOIK_SCHEDULE_THROUGHPUT && sp.timeout_ticks == 0 && units >= 8 * (uint64_t)p->model->dev.cus && sp.max_steps >= 8;
    if (!kind_ok || captured) {
        run(sw);
        return;
    }
    int bucket = 0;  // floor(log2(units)): a mapping measured on 2048 units says little about 65536 (whether the hand-over to the helped kernel pays, ...)
    for (uint64_t u = units; u > 1; u >>= 1) bucket++;
    const auto key = std::make_tuple((int)sp.lambda, (int)sp.fk_mode, sp.islands > 1 ? 1 : 0, bucket);
    auto it = p->tuned.find(key);
    if (it != p->tuned.end() && it->second.preset >= 0) {
        run(preset_switches(sw, it->second.preset));
        return;
    }
    // (not while other solves of the handle are in flight on its other slots: their work would be in the timings, and a submit would block for five solves)
    bool others_pending = false;
    for (const auto& sl : p->io) others_pending = others_pending || sl.pending;
    if (!(may_wait || sw.autotune >= 2) || !be_can_time() || others_pending) {
        run(sw);
        return;
    }
    bioik_problem::Tuned t;
    int best = 0;
    for (int i = 0; i < kPresets; i++) {
        const SolveSwitches w = preset_switches(sw, i);
        try {
            t.ms[i] = be_time_ms(stream, [&]() { run(w); });
        } catch (const Error& e) {
            if (i == 0 || (e.code != BIOIK_ERR_UNSUPPORTED && e.code != BIOIK_ERR_INVALID_ARGUMENT)) throw;  // (a preset this problem has no room for: skipped)
            t.ms[i] = -1.0;
        }
        if (t.ms[i] >= 0.0 && t.ms[i] < t.ms[best]) best = i;
    }
    if (best != 0 && t.ms[best] > 0.97 * t.ms[0]) best = 0;  // (the rules stand unless something beats them by more than the run-to-run spread)
    t.preset = best;
    p->tuned[key] = t;
    if (sw.report) {
        std::fprintf(stderr, "[bioik] measured mapping choice (population %d, fk %d, islands %s; %llu units):\n", (int)sp.lambda, (int)sp.fk_mode, sp.islands > 1 ? "yes" : "no", (unsigned long long)units);
        for (int i = 0; i < kPresets; i++)
            if (t.ms[i] >= 0.0) std::fprintf(stderr, "[bioik]   %c %-90s %9.3f ms\n", i == best ? '*' : ' ', preset_name(i), t.ms[i]);
            else std::fprintf(stderr, "[bioik]     %-90s   not eligible\n", preset_name(i));
    }
    // (the caller's arrays hold the last eligible run's results: every mapping's are the same bits, nothing to redo)
}

// what every solve entry point asks of its arrays (goal parameters only where the problem has some)
static void check_arrays(const bioik_problem* p, const SolveArrays& a) {
    if ((a.var_lo == nullptr) != (a.var_hi == nullptr)) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "var_lo and var_hi: both or neither (exactly one of them is null)");
    if (a.n && (!a.seeds || !a.solutions || !a.fitness || !a.success || !a.steps || (p->host.dev.P > 0 && !a.goal_params))) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null array");
}
// The device-pointer entries do not wait for their solves: a rendezvous time-out of an EARLIER solve through one of them is reported by the handle's next call
static void report_stale_error(bioik_problem* p) {
    unsigned int& err = p->h_error[bioik_problem::kIoSlots];
    if (err == 0u) return;
    err = 0u;
    throw Error(BIOIK_ERR_HIP, "an earlier solve of this handle through a device-pointer entry timed out at a rendezvous between its wavefronts (k_solve_lean_cl4h): its results are not valid");
}
// a solve that broke off may have left the control words of the handle's scratch buffers anywhere: every buffer sets them up again (bioik_problem::Scratch)
static void reset_control_words(bioik_problem* p) {
    for (auto& kv : p->scratch) kv.second.forget_words();
}

// ------------------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------------------
extern "C" {

const char* bioik_last_error(void) { return g_err.c_str(); }
int bioik_abi_version(void) { return BIOIK_ABI_VERSION; }
int bioik_device_count(void) { return be_device_count(); }
int bioik_goal_param_count(int goal_type) { return bioik::goal_param_count(goal_type); }
int bioik_debug_reload_switches(void) {  // diagnostics only: the BIOIK_SOLVE_* switches are otherwise read once, when the library is loaded
    SolveSwitches w = parse_switches();
    std::lock_guard<std::mutex> lock(g_switch_mtx);
    g_switches = apply_switches(std::move(w));
    return BIOIK_OK;
}

void bioik_default_solve_params(bioik_solve_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(*p);
    p->mode = BIOIK_MODE_BIO2_MEMETIC;
    p->fk_mode = BIOIK_FK_EXACT;
    p->population = 128;
    p->islands = 1;
    p->max_steps = 64;
    p->random_seed = 0;
    p->dpos = -1.0;
    p->drot = -1.0;
    p->dtwist = 1e-5;
    p->no_wipeout = 0;
    p->timeout = 0.0;
    p->island_sync = 0;
}

int bioik_model_create(const bioik_model_desc* desc, int device, bioik_model** out) {
    API_BEGIN
    if (!desc || !out) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    int n = be_device_count();
    if (n <= 0) throw Error(BIOIK_ERR_NO_DEVICE, "no HIP device available: this solver has no CPU path");
    if (device < 0 || device >= n) throw Error(BIOIK_ERR_NO_DEVICE, "HIP device index out of range");
    *out = new bioik_model(*desc, device);
    API_END
}
void bioik_model_destroy(bioik_model* m) { delete m; }

int bioik_problem_create(bioik_model* model, const bioik_problem_desc* desc, bioik_problem** out) {
    API_BEGIN
    if (!model || !desc || !out) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    bioik::problem_desc_has_base_links(*desc);  // (throws on a struct_size that is none of the descriptor's: before any field beyond it is read)
    if ((desc->n_goals && !desc->goals) || (desc->n_group_joints && !desc->group_joints) || (desc->n_fixed_joints && !desc->fixed_joints))
        throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_problem_desc: a count is non-zero but its array is null");
    std::unique_ptr<bioik_problem> p(new bioik_problem(model, *desc));
    DeviceGuard on_device(model->device);
    p->d_pb = (DevProblem*)be_alloc(sizeof(DevProblem));
    p->d_clocks = (unsigned long long*)be_alloc(bioik_problem::kCaptureClocks * sizeof(unsigned long long));
    p->d_resident = (unsigned int*)be_alloc(16 * 128);
    be_zero_async(p->d_resident, 16 * 128, 0);
    p->h_error = (unsigned int*)be_alloc_pinned(64);
    std::memset(p->h_error, 0, 64);
    if (!p->host.touch_points.empty()) {
        p->d_touch = (double*)be_alloc(p->host.touch_points.size() * sizeof(double));
        be_h2d(p->d_touch, p->host.touch_points.data(), p->host.touch_points.size() * sizeof(double), 0);
        p->host.dev.touch_points = p->d_touch;
    }
    be_h2d(p->d_pb, &p->host.dev, sizeof(DevProblem), 0);
    be_sync(0);
    *out = p.release();
    API_END
}
static void io_finish(bioik_problem* p, bioik_problem::IoSlot& sl);
void bioik_problem_destroy(bioik_problem* p) {
    if (!p) return;
    {  // submitted solves nobody waited for are completed here, as include/bioik_hip.h promises: waited for and their results copied into their callers' arrays,
       // before anything they use goes
        std::lock_guard<std::mutex> lock(p->mtx);
        for (auto& sl : p->io) {
            try {
                io_finish(p, sl);
            } catch (...) {
            }
        }
    }
    be_free(p->d_pb);
    if (p->d_touch) be_free(p->d_touch);
    be_free(p->d_clocks);
    be_free(p->d_resident);
    be_free_pinned(p->h_error);
    for (auto& kv : p->scratch) be_free(kv.second.base);
    for (const auto& r : p->retired_scratch) be_free(r.base);
    for (auto& sl : p->io) {
        be_stream_destroy(sl.stream);
        be_free(sl.dev);
        be_free_pinned(sl.host);
    }
    delete p;
}

int bioik_problem_active_variable_count(const bioik_problem* p) { return p ? p->host.dev.D : BIOIK_ERR_INVALID_ARGUMENT; }
int bioik_problem_active_variables(const bioik_problem* p, int32_t* out) {
    if (!p || !out) return BIOIK_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < p->host.active_variables.size(); i++) out[i] = p->host.active_variables[i];
    return BIOIK_OK;
}
int bioik_problem_tip_count(const bioik_problem* p) { return p ? p->host.dev.T : BIOIK_ERR_INVALID_ARGUMENT; }
int bioik_problem_tip_links(const bioik_problem* p, int32_t* out) {
    if (!p || !out) return BIOIK_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < p->host.tip_links.size(); i++) out[i] = p->host.tip_links[i];
    return BIOIK_OK;
}
int bioik_problem_param_count(const bioik_problem* p) { return p ? p->host.dev.P : BIOIK_ERR_INVALID_ARGUMENT; }
int bioik_problem_variable_count(const bioik_problem* p) { return p ? p->host.dev.V : BIOIK_ERR_INVALID_ARGUMENT; }
int bioik_problem_set_first_query(bioik_problem* p, uint64_t first_query) {
    if (!p) return BIOIK_ERR_INVALID_ARGUMENT;
    p->first_query = first_query;
    return BIOIK_OK;
}

// ---- obstacle tables of the ClearanceGoals (include/bioik_hip.h; the block's layout: bioik_types.h) ----
// the first row of goal `goal_index`'s obstacle block in touch_points; throws for anything that is no ClearanceGoal of the problem
static size_t obstacle_block(const bioik_problem* p, int goal_index, const char* who) {
    if (!p) throw Error(BIOIK_ERR_INVALID_ARGUMENT, std::string(who) + ": null handle");
    if (goal_index < 0 || (size_t)goal_index >= p->host.clearance_block.size())
        throw Error(BIOIK_ERR_INVALID_ARGUMENT, std::string(who) + ": goal index " + std::to_string(goal_index) + " out of range (the problem has " + std::to_string(p->host.clearance_block.size()) + " goals)");
    if (p->host.clearance_block[goal_index] < 0) throw Error(BIOIK_ERR_INVALID_ARGUMENT, std::string(who) + ": goal " + std::to_string(goal_index) + " is not a CLEARANCE goal");
    return (size_t)p->host.clearance_block[goal_index];
}
static void upload_obstacles(bioik_problem* p, size_t row, size_t n, const double* spheres);
int bioik_problem_set_obstacles(bioik_problem* p, int goal_index, size_t n, const double* spheres) {
    API_BEGIN
    const size_t row = obstacle_block(p, goal_index, "bioik_problem_set_obstacles");
    if (n > (size_t)BIOIK_MAX_OBSTACLES)
        throw Error(BIOIK_ERR_UNSUPPORTED, "bioik_problem_set_obstacles: " + std::to_string(n) + " obstacles, more than BIOIK_MAX_OBSTACLES (" + std::to_string(BIOIK_MAX_OBSTACLES) + ")");
    if (n > 0 && !spheres) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_problem_set_obstacles: spheres is null");
    for (size_t i = 0; i < n; i++) {
        for (int c = 0; c < 4; c++)
            if (!std::isfinite(spheres[4 * i + c])) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_problem_set_obstacles: row " + std::to_string(i) + " holds a number that is not finite");
        if (spheres[4 * i + 3] < 0.0) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_problem_set_obstacles: row " + std::to_string(i) + " has a radius < 0");
    }
    upload_obstacles(p, row, n, spheres);
    API_END
}
static void upload_obstacles(bioik_problem* p, size_t row, size_t n, const double* spheres) {  // (checked rows)
    std::lock_guard<std::mutex> lock(p->mtx);
    DeviceGuard on_device(p->model->device);
    // nothing of this handle reads the table while it changes: the submitted tickets are completed, the handle's own streams drained (the slots' and the default
    // stream of the function-level entries); device-pointer solves on the caller's streams are the caller's to wait for
    for (auto& sl : p->io) io_finish(p, sl);
    for (auto& sl : p->io)
        if (sl.stream_made) be_sync(sl.stream);
    be_sync(0);
    // count row and rows in ONE copy, to an address that never changes (the host's copy of the buffer is kept current: obstacle_count reads it)
    double* block = p->host.touch_points.data() + 4 * row;
    const int32_t count = (int32_t)n;
    std::memset(block, 0, 4 * sizeof(double));
    std::memcpy(block, &count, sizeof(count));
    if (n) std::memcpy(block + 4, spheres, n * 4 * sizeof(double));
    be_h2d(p->d_touch + 4 * row, block, (1 + n) * 4 * sizeof(double), 0);
    be_sync(0);
}
// bioik_solve_batch_multi: the shards are parts of ONE solve, so every handle gets the obstacle tables of problems[0] (a handle that holds them already is left alone)
static void share_obstacles(bioik_problem* const* problems, int n_problems) {
    bioik_problem* p0 = problems[0];
    for (size_t g = 0; g < p0->host.clearance_block.size(); g++) {
        if (p0->host.clearance_block[g] < 0) continue;
        std::vector<double> block((size_t)(1 + BIOIK_MAX_OBSTACLES) * 4);
        {
            std::lock_guard<std::mutex> lock(p0->mtx);
            std::memcpy(block.data(), p0->host.touch_points.data() + 4 * (size_t)p0->host.clearance_block[g], block.size() * sizeof(double));
        }
        int32_t count = 0;
        std::memcpy(&count, block.data(), sizeof(count));
        for (int r = 1; r < n_problems; r++) {
            bioik_problem* q = problems[r];
            if (q->host.clearance_block.size() != p0->host.clearance_block.size() || q->host.clearance_block[g] < 0)
                throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_solve_batch_multi: the handles were compiled from different problem templates");
            bool same;
            {
                std::lock_guard<std::mutex> lock(q->mtx);
                same = std::memcmp(q->host.touch_points.data() + 4 * (size_t)q->host.clearance_block[g], block.data(), (size_t)(1 + count) * 4 * sizeof(double)) == 0;
            }
            if (!same) upload_obstacles(q, (size_t)q->host.clearance_block[g], (size_t)count, block.data() + 4);
        }
    }
}
int bioik_problem_obstacle_count(const bioik_problem* p, int goal_index) {
    API_BEGIN
    const size_t row = obstacle_block(p, goal_index, "bioik_problem_obstacle_count");
    std::lock_guard<std::mutex> lock(const_cast<bioik_problem*>(p)->mtx);
    int32_t count = 0;
    std::memcpy(&count, p->host.touch_points.data() + 4 * row, sizeof(count));
    return count;
    API_END
}

int bioik_resolve_islands(const bioik_problem* p,const bioik_solve_params* params, size_t n, int32_t* islands, int32_t* island_sync) {
    API_BEGIN
    if (!p || !params || !islands || !island_sync) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    const DevSolveParams r = bioik::normalize_params(*params, 0, n, 8 * (size_t)p->model->dev.cus);
    *islands = r.islands, *island_sync = r.island_sync;
    API_END
}
// (the plain entries are the bounded ones with both arrays of bounds null: one path, the same launches, kernels and bits)
int bioik_solve_batch_device(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* d_seeds, const double* d_goal_params,
                             double* d_solutions, double* d_fitness, int32_t* d_success, int32_t* d_steps, void* hip_stream) {
    return bioik_solve_batch_bounded_device(p, params, n, d_seeds, d_goal_params, nullptr, nullptr, d_solutions, d_fitness, d_success, d_steps, hip_stream);
}
int bioik_solve_batch_bounded_device(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* d_seeds, const double* d_goal_params,
                                     const double* d_var_lo, const double* d_var_hi, double* d_solutions, double* d_fitness, int32_t* d_success, int32_t* d_steps,
                                     void* hip_stream) {
    API_BEGIN
    if (!p || !params) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    const SolveArrays arrays{n, d_seeds, d_goal_params, d_solutions, d_fitness, d_success, d_steps, nullptr, d_var_lo, d_var_hi};
    check_arrays(p, arrays);
    std::lock_guard<std::mutex> lock(p->mtx);
    DeviceGuard on_device(p->model->device);
    DevSolveParams sp = bioik::normalize_params(*params, p->first_query, n, 8 * (size_t)p->model->dev.cus);
    report_stale_error(p);
    solve_dispatch(p, sp, arrays, (stream_t)hip_stream, false, p->h_error + bioik_problem::kIoSlots);
    API_END
}

// ---- ranked solves: the k best distinct islands of every query (include/bioik_hip.h; select_ranked) ----
// The solve parameters of a ranked call and its argument checks, all before anything is allocated or launched: an explicit island_sync = 1 is refused (islands that
// stop each other leave at timing-dependent steps: their individual results are not defined), BIOIK_ISLANDS_AUTO gives max(k, what bioik_resolve_islands gives)
// with island_sync off, and 1 <= k <= islands <= 64.
static DevSolveParams ranked_params(bioik_problem* p, const bioik_solve_params& params, uint64_t first_query, size_t n, int32_t k, const int32_t* count) {
    if (!count) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_solve_batch_ranked: count is null");
    if (k < 1) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_solve_batch_ranked: k must be at least 1");
    if (params.island_sync == 1) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_solve_batch_ranked: island_sync = 1 is refused (the results of islands that stop each other are not defined one by one)");
    DevSolveParams sp = bioik::normalize_params(params, first_query, n, 8 * (size_t)p->model->dev.cus);
    if (params.islands <= 0 && sp.islands < k) sp.islands = k;  // BIOIK_ISLANDS_AUTO
    sp.island_sync = 0;
    if (sp.islands > 64) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_solve_batch_ranked: at most 64 islands (a lane of one wavefront each)");
    if (k > sp.islands) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_solve_batch_ranked: k = " + std::to_string(k) + " is more than the call's " + std::to_string(sp.islands) + " islands");
    return sp;
}
static RankedArgs ranked_args(int32_t k, double min_distance, const SolveArrays& out) {
    RankedArgs r;
    std::memset(&r, 0, sizeof(r));
    r.k = k, r.min_distance = min_distance;
    r.solutions = out.solutions, r.fitness = out.fitness, r.success = out.success, r.steps = out.steps, r.count = out.count;
    return r;
}
struct RankedCall {  // a ranked solve through the host-pointer path (io_begin): its checked parameters, k, the distance
    DevSolveParams sp;
    int32_t k;
    double min_distance;
};

// host arrays in, host arrays out: staged through a slot's page-locked arena, one DMA each way, on the slot's own stream.
// io_finish: the slot's solve is complete and its results are in the caller's arrays (no-op for an idle slot).  Called with p->mtx held.
static void io_finish(bioik_problem* p, bioik_problem::IoSlot& sl) {
    if (!sl.pending) return;
    DeviceGuard on_device(p->model->device);
    try {
        be_sync(sl.stream);
    } catch (const Error& e) {
        // the device failed under THIS slot's solve: its ticket's wait reports it (not whichever call came by to reuse the slot), its result arrays
        // stay untouched, and the slot is free again
        sl.failed_ticket = sl.ticket, sl.failed_code = e.code, sl.failed_message = e.what();
        sl.pending = false;
        reset_control_words(p);
        return;
    }
    sl.pending = false;
    unsigned int& err = p->h_error[&sl - p->io];
    if (err != 0u) {  // (SolveArgs::error: a wavefront of this solve gave up waiting for its partner and went on unsynchronised)
        err = 0u;
        reset_control_words(p);
        sl.failed_ticket = sl.ticket, sl.failed_code = BIOIK_ERR_HIP;
        sl.failed_message = "a rendezvous between the wavefronts of a workgroup timed out (k_solve_lean_cl4h): the results of this solve are not valid";
        return;
    }
    const bioik::IoArenaLayout& A = sl.arena;
    const SolveArrays& to = sl.caller;
    std::memcpy(to.solutions, A.solutions.at(sl.host), A.solutions.bytes());
    std::memcpy(to.fitness, A.fitness.at(sl.host), A.fitness.bytes());
    std::memcpy(to.success, A.success.at(sl.host), A.success.bytes());
    std::memcpy(to.steps, A.steps.at(sl.host), A.steps.bytes());
    if (to.count) std::memcpy(to.count, A.count.at(sl.host), A.count.bytes());
}
// io_begin: copy in, enqueue the transfer in, the solve and the transfer out on the slot's stream; returns without waiting.
// A solve still pending on the slot is completed first (its results reach its caller's arrays).  Called with p->mtx held.
static void io_begin(bioik_problem* p, bioik_problem::IoSlot& sl, uint64_t ticket, const bioik_solve_params& params, uint64_t first_query, const SolveArrays& caller,
                     const RankedCall* ranked = nullptr) {
    io_finish(p, sl);
    DeviceGuard on_device(p->model->device);
    const size_t n = caller.n;
    // (a bounded call: its two arrays of bounds behind the goal parameters, where they stay as long as the call's launches; a ranked call: k result rows per query, and count [n])
    const bioik::IoArenaLayout A = bioik::io_arena_layout(n, (size_t)p->host.dev.V, (size_t)p->host.dev.P, ranked ? (size_t)ranked->k : 1, caller.bounded(), ranked != nullptr);
    if (sl.bytes < A.bytes) {
        be_free(sl.dev);
        be_free_pinned(sl.host);
        sl.dev = sl.host = nullptr, sl.bytes = 0;
        const size_t cap = A.bytes + A.bytes / 4;
        sl.dev = be_alloc(cap);
        sl.host = be_alloc_pinned(cap);
        sl.bytes = cap;
    }
    void* const hd = sl.host;
    if (!sl.stream_made) sl.stream = be_stream_create(), sl.stream_made = true;
    const stream_t st = sl.stream;
    std::memcpy(A.seeds.at(hd), caller.seeds, A.seeds.bytes());
    if (A.goal_params.count) std::memcpy(A.goal_params.at(hd), caller.goal_params, A.goal_params.bytes());
    if (A.var_lo.count) std::memcpy(A.var_lo.at(hd), caller.var_lo, A.var_lo.bytes()), std::memcpy(A.var_hi.at(hd), caller.var_hi, A.var_hi.bytes());
    // (a call of a few queries -- MoveIt's one pose per call -- reads its inputs where they lie: the page-locked arena is mapped into the device's address space, and a
    // few hundred bytes per workgroup over the bus cost less than a DMA transfer in front of the launch)
    const bool direct_inputs = n <= 16;
    if (!direct_inputs) be_h2d(sl.dev, hd, A.in_bytes, st);
    const void* in_base = direct_inputs ? hd : sl.dev;
    DevSolveParams sp = ranked ? ranked->sp : bioik::normalize_params(params, first_query, n, 8 * (size_t)p->model->dev.cus);
    // The results go from the kernels straight into the page-locked arena (it is mapped into the device's address space; 1.5 MB per 4096 queries,
    // written once per query).  A transfer out enqueued behind the solve would sit at the head of a DMA queue until the solve is over -- 12 ms
    // for a one-launch solve -- with the transfers in of the handle's next solves behind it: nothing would overlap
    // (profiles/r03_inflight_and_schedule.log, host pipeline).
    const SolveArrays arena{n, A.seeds.at(in_base), A.goal_params.at(in_base), A.solutions.at(hd), A.fitness.at(hd), A.success.at(hd), A.steps.at(hd),
                            ranked ? A.count.at(hd) : nullptr, A.var_lo.count ? A.var_lo.at(in_base) : nullptr, A.var_hi.count ? A.var_hi.at(in_base) : nullptr};
    if (ranked) {  // (the rules alone: the measured mapping choice is neither taken nor made by a ranked call)
        const RankedArgs r = ranked_args(ranked->k, ranked->min_distance, arena);
        launch_solve(p, sp, arena, st, be_stream_capturing(st), switches(), p->h_error + (&sl - p->io), &r);
    } else {
        solve_dispatch(p, sp, arena, st, true, p->h_error + (&sl - p->io));
    }
    sl.pending = true, sl.ticket = ticket, sl.arena = A, sl.caller = caller;
}
static void solve_host(bioik_problem* p, const bioik_solve_params& params, uint64_t first_query, const SolveArrays& caller, const RankedCall* ranked = nullptr) {
    if (caller.n == 0) return;
    std::lock_guard<std::mutex> lock(p->mtx);
    const uint64_t ticket = p->next_ticket++;
    // (a synchronous call needs no slot of its own: an idle one whose stream and arenas exist already, so that a loop of searchPositionIK calls does not pay for
    // six streams and six pairs of arenas -- 10 ms each -- during its first six calls)
    size_t pick = ticket % bioik_problem::kIoSlots;
    for (size_t i = 0; i < (size_t)bioik_problem::kIoSlots; i++)
        if (!p->io[i].pending && p->io[i].stream_made) {
            pick = i;
            break;
        }
    bioik_problem::IoSlot& sl = p->io[pick];
    io_begin(p, sl, ticket, params, first_query, caller, ranked);
    io_finish(p, sl);
    if (sl.failed_ticket == ticket) throw Error(sl.failed_code, "the solve failed on the device: " + sl.failed_message);  // (the synchronous call is its own ticket's wait)
}

int bioik_solve_batch(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* seeds, const double* goal_params, double* solutions,
                      double* fitness, int32_t* success, int32_t* steps) {
    return bioik_solve_batch_bounded(p, params, n, seeds, goal_params, nullptr, nullptr, solutions, fitness, success, steps);
}
int bioik_solve_batch_bounded(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* seeds, const double* goal_params, const double* var_lo,
                              const double* var_hi, double* solutions, double* fitness, int32_t* success, int32_t* steps) {
    API_BEGIN
    if (!p || !params) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    const SolveArrays arrays{n, seeds, goal_params, solutions, fitness, success, steps, nullptr, var_lo, var_hi};
    check_arrays(p, arrays);
    solve_host(p, *params, p->first_query, arrays);
    API_END
}

int bioik_solve_batch_ranked_device(bioik_problem* p, const bioik_solve_params* params, size_t n, int32_t k, double min_distance, const double* d_seeds,
                                    const double* d_goal_params, double* d_solutions, double* d_fitness, int32_t* d_success, int32_t* d_steps, int32_t* d_count,
                                    void* hip_stream) {
    API_BEGIN
    if (!p || !params) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    const SolveArrays arrays{n, d_seeds, d_goal_params, d_solutions, d_fitness, d_success, d_steps, d_count};
    check_arrays(p, arrays);
    std::lock_guard<std::mutex> lock(p->mtx);
    DeviceGuard on_device(p->model->device);
    const DevSolveParams sp = ranked_params(p, *params, p->first_query, n, k, d_count);
    report_stale_error(p);
    const RankedArgs r = ranked_args(k, min_distance, arrays);
    // (the rules alone: the measured mapping choice is neither taken nor made by a ranked call)
    launch_solve(p, sp, arrays, (stream_t)hip_stream, be_stream_capturing((stream_t)hip_stream), switches(), p->h_error + bioik_problem::kIoSlots, &r);
    API_END
}
int bioik_solve_batch_ranked(bioik_problem* p, const bioik_solve_params* params, size_t n, int32_t k, double min_distance, const double* seeds,
                             const double* goal_params, double* solutions, double* fitness, int32_t* success, int32_t* steps, int32_t* count) {
    API_BEGIN
    if (!p || !params) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    const SolveArrays arrays{n, seeds, goal_params, solutions, fitness, success, steps, count};
    check_arrays(p, arrays);
    const uint64_t first_query = p->first_query;
    const RankedCall call{ranked_params(p, *params, first_query, n, k, count), k, min_distance};
    solve_host(p, *params, first_query, arrays, &call);  // (the handle's arena, lock and slots, as bioik_solve_batch)
    API_END
}

// Asynchronous host-pointer solve: a caller with a stream of batches keeps up to kIoSlots (six) of them in flight on ONE handle.
int bioik_solve_batch_submit(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* seeds, const double* goal_params, double* solutions,
                             double* fitness, int32_t* success, int32_t* steps, uint64_t* ticket) {
    return bioik_solve_batch_bounded_submit(p, params, n, seeds, goal_params, nullptr, nullptr, solutions, fitness, success, steps, ticket);
}
int bioik_solve_batch_bounded_submit(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* seeds, const double* goal_params, const double* var_lo,
                                     const double* var_hi, double* solutions, double* fitness, int32_t* success, int32_t* steps, uint64_t* ticket) {
    API_BEGIN
    if (!p || !params || !ticket) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    const SolveArrays arrays{n, seeds, goal_params, solutions, fitness, success, steps, nullptr, var_lo, var_hi};
    check_arrays(p, arrays);
    std::lock_guard<std::mutex> lock(p->mtx);
    const uint64_t t = p->next_ticket++;
    *ticket = t;
    if (n == 0) return BIOIK_OK;  // (nothing to do: waiting for this ticket returns at once)
    bioik_solve_params sp = *params;
    if (sp.schedule == BIOIK_SCHEDULE_AUTO) {  // a pipeline three or more solves deep (this one and two before it) pays for the dense mapping (include/bioik_hip.h)
        int in_flight = 0;
        for (auto& sl : p->io) in_flight += (sl.pending && &sl != &p->io[t % bioik_problem::kIoSlots]) ? 1 : 0;
        sp.schedule = in_flight >= 2 ? BIOIK_SCHEDULE_THROUGHPUT : BIOIK_SCHEDULE_LATENCY;
    }
    io_begin(p, p->io[t % bioik_problem::kIoSlots], t, sp, p->first_query, arrays);
    API_END
}
int bioik_solve_batch_wait(bioik_problem* p, uint64_t ticket) {
    API_BEGIN
    if (!p) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    bioik_problem::IoSlot& sl = p->io[ticket % bioik_problem::kIoSlots];
    stream_t st = nullptr;
    {
        std::lock_guard<std::mutex> lock(p->mtx);
        if (ticket == 0 || ticket >= p->next_ticket) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_solve_batch_wait: unknown ticket");
        if (sl.failed_ticket == ticket) throw Error(sl.failed_code, "the solve of this ticket failed on the device: " + sl.failed_message);
        if (!sl.pending || sl.ticket != ticket) return BIOIK_OK;  // completed when its slot was taken again, or an empty batch
        st = sl.stream;
    }
    {  // the wait itself happens outside the handle's lock: another thread may submit the next batch meanwhile
        DeviceGuard on_device(p->model->device);
        try {
            be_sync(st);
        } catch (const Error&) {  // (io_finish below meets the same error under the lock and files it with the ticket)
        }
    }
    std::lock_guard<std::mutex> lock(p->mtx);
    if (sl.pending && sl.ticket == ticket) io_finish(p, sl);
    if (sl.failed_ticket == ticket) throw Error(sl.failed_code, "the solve of this ticket failed on the device: " + sl.failed_message);
    API_END
}

// One batch over several problem handles of the SAME template -- one per device of the node, or several on one device: shard r =
// queries [r n / W, (r + 1) n / W), one host thread per handle, each on its handle's stream; no exchange between the shards (the
// queries are independent), and the query-indexed random streams make the result identical to the unsharded solve.
int bioik_solve_batch_multi(bioik_problem* const* problems, int n_problems, const bioik_solve_params* params, size_t n, const double* seeds,
                            const double* goal_params, double* solutions, double* fitness, int32_t* success, int32_t* steps) {
    API_BEGIN
    if (!problems || n_problems <= 0 || !params) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    for (int r = 0; r < n_problems; r++) {
        if (!problems[r]) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null problem handle");
        const DevProblem &a = problems[0]->host.dev, &b = problems[r]->host.dev;
        if (a.V != b.V || a.P != b.P || a.D != b.D || a.T != b.T || a.n_ops != b.n_ops)
            throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_solve_batch_multi: the handles were compiled from different problem templates");
        for (int q = 0; q < r; q++)
            if (problems[q] == problems[r]) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_solve_batch_multi: the same handle twice");
    }
    const size_t V = problems[0]->host.dev.V, P = problems[0]->host.dev.P;
    check_arrays(problems[0], SolveArrays{n, seeds, goal_params, solutions, fitness, success, steps, nullptr});
    share_obstacles(problems, n_problems);
    const uint64_t first = problems[0]->first_query;
    const size_t W = (size_t)n_problems;
    // BIOIK_ISLANDS_AUTO: one island count for the whole batch, sized to the largest shard (what one device gets), so that every shard runs the same solve
    bioik_solve_params shard_params = *params;
    if (params->islands <= 0 && n > 0) {
        const DevSolveParams r = bioik::normalize_params(*params, 0, (n + W - 1) / W, 8 * (size_t)problems[0]->model->dev.cus);
        shard_params.islands = r.islands, shard_params.island_sync = r.island_sync;
    }
    std::vector<int> status(W, BIOIK_OK);
    std::vector<std::string> message(W);
    std::vector<std::thread> workers;
    for (size_t r = 0; r < W; r++) {
        const size_t a = r * n / W, b = (r + 1) * n / W;
        if (a == b) continue;
        workers.emplace_back([&, r, a, b]() {
            try {
                solve_host(problems[r], shard_params, first + a, SolveArrays{b - a, seeds + a * V, P ? goal_params + a * P : nullptr, solutions + a * V, fitness + a, success + a, steps + a, nullptr});
            } catch (const Error& e) {
                status[r] = e.code, message[r] = e.what();
            } catch (const std::exception& e) {
                status[r] = BIOIK_ERR_INVALID_ARGUMENT, message[r] = e.what();
            }
        });
    }
    for (auto& w : workers) w.join();
    for (size_t r = 0; r < W; r++)
        if (status[r] != BIOIK_OK) throw Error(status[r], "shard " + std::to_string(r) + ": " + message[r]);
    API_END
}

// ---- function-level entry points -------------------------------------------------------------------------
static EvalArgs eval_args(bioik_problem* p) {
    EvalArgs a;
    std::memset(&a, 0, sizeof(a));
    a.pb = p->pb();
    a.dpos = a.drot = a.dtwist = DBL_MAX;
    return a;
}

int bioik_eval_fk(bioik_problem* p, size_t n, const double* seed, const double* genes, double* tip_frames) {
    API_BEGIN
    if (!p || !seed || (n && (!genes || !tip_frames))) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return BIOIK_OK;
    std::lock_guard<std::mutex> lock(p->mtx);
    DeviceGuard on_device(p->model->device);
    const int nth = 64;
    const size_t lds = eval_lds(p, eval_lds_bytes(p, nth));
    const size_t V = p->host.dev.V, D = p->host.dev.D, T = p->host.dev.T;
    DevBuf dseed(seed, V * 8), dgenes(genes, n * D * 8), dout(n * T * 7 * 8);
    EvalArgs a = eval_args(p);
    a.n = n, a.seed = dseed.as<double>(), a.genes = dgenes.as<double>(), a.out0 = dout.as<double>();
    LAUNCH(k_eval_fk, eval_fk_body(a, b_, l_), (n + nth - 1) / nth, nth, lds, 0, a);
    dout.download(tip_frames);
    be_sync(0);
    API_END
}

int bioik_eval_fitness(bioik_problem* p, int fk_mode, size_t n, const double* seed, const double* goal_params, const double* base_genes, const double* genes,
                       double* primary, double* secondary) {
    API_BEGIN
    if (!p || !seed || (n && (!genes || !primary || !secondary))) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    if (fk_mode != BIOIK_FK_LINEAR && fk_mode != BIOIK_FK_EXACT) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "unknown fk_mode");
    if (fk_mode == BIOIK_FK_LINEAR && !base_genes) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "base_genes required for the linear model");
    if (p->host.dev.P > 0 && !goal_params) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "goal_params required");
    if (n == 0) return BIOIK_OK;
    std::lock_guard<std::mutex> lock(p->mtx);
    DeviceGuard on_device(p->model->device);
    const int nth = 64;
    const size_t lds = eval_lds(p, eval_lds_bytes(p, nth));
    const size_t V = p->host.dev.V, D = p->host.dev.D, P = p->host.dev.P;
    DevBuf dseed(seed, V * 8), dpar(goal_params, P * 8), dbase(base_genes, D * 8), dgenes(genes, n * D * 8), d0(n * 8), d1(n * 8);
    EvalArgs a = eval_args(p);
    a.n = n, a.seed = dseed.as<double>(), a.params = dpar.as<double>(), a.genes = dgenes.as<double>(), a.base = dbase.as<double>();
    a.out0 = d0.as<double>(), a.out1 = d1.as<double>(), a.fk_mode = fk_mode;
    LAUNCH(k_eval_fitness, eval_fitness_body(a, b_, l_), (n + nth - 1) / nth, nth, lds, 0, a);
    d0.download(primary);
    d1.download(secondary);
    be_sync(0);
    API_END
}

int bioik_eval_approximator(bioik_problem* p, const double* seed, const double* base_genes, double* tip_frames, double* deltas) {
    API_BEGIN
    if (!p || !seed || !base_genes || !tip_frames || !deltas) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lock(p->mtx);
    DeviceGuard on_device(p->model->device);
    const int nth = 64;
    const size_t lds = eval_lds(p, eval_lds_bytes(p, nth));
    const size_t V = p->host.dev.V, D = p->host.dev.D, T = p->host.dev.T;
    DevBuf dseed(seed, V * 8), dbase(base_genes, D * 8), d0(T * 7 * 8), d1(T * D * 7 * 8);
    EvalArgs a = eval_args(p);
    a.n = 1, a.seed = dseed.as<double>(), a.base = dbase.as<double>(), a.out0 = d0.as<double>(), a.out1 = d1.as<double>();
    LAUNCH(k_eval_approximator, eval_approximator_body(a, l_), 1, nth, lds, 0, a);
    d0.download(tip_frames);
    d1.download(deltas);
    be_sync(0);
    API_END
}

int bioik_eval_reproduce(bioik_problem* p, int population, uint32_t rng_key, int species, uint32_t generation, const double* parents, double* children_genes,
                         double* children_gradients) {
    API_BEGIN
    if (!p || !parents || !children_genes || !children_gradients || population <= 0) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bad argument");
    std::lock_guard<std::mutex> lock(p->mtx);
    DeviceGuard on_device(p->model->device);
    const int nth = 64;
    const size_t M = p->host.dev.n_ops > 0 ? p->host.dev.n_ops : 1;
    const size_t lds = eval_lds(p, (4 * M + 2 * M * nth) * 8);  // (eval_reproduce_body: the parents, then a genotype and a gradient column per lane)
    const size_t D = p->host.dev.D, n = (size_t)population;
    DevBuf dpar(parents, 4 * D * 8), d0(n * D * 8), d1(n * D * 8);
    EvalArgs a = eval_args(p);
    a.n = n, a.genes = dpar.as<double>(), a.out0 = d0.as<double>(), a.out1 = d1.as<double>();
    a.rng_key = rng_key;
    a.rng_ctr1 = (generation << 4) | ((uint32_t)species << 3) | 0u;
    LAUNCH(k_eval_reproduce, eval_reproduce_body(a, b_, l_), (n + nth - 1) / nth, nth, lds, 0, a);
    d0.download(children_genes);
    d1.download(children_gradients);
    be_sync(0);
    API_END
}

int bioik_eval_check(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* seed, const double* goal_params, const double* genes,
                     int32_t* ok) {
    API_BEGIN
    if (!p || !params || !seed || (n && (!genes || !ok))) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    if (p->host.dev.P > 0 && !goal_params) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "goal_params required");
    if (n == 0) return BIOIK_OK;
    std::lock_guard<std::mutex> lock(p->mtx);
    DeviceGuard on_device(p->model->device);
    DevSolveParams sp = bioik::normalize_params(*params, 0);
    const int nth = 64;
    const size_t lds = eval_lds(p, eval_lds_bytes(p, nth));
    const size_t V = p->host.dev.V, D = p->host.dev.D, P = p->host.dev.P;
    DevBuf dseed(seed, V * 8), dpar(goal_params, P * 8), dgenes(genes, n * D * 8), dok(n * 4);
    EvalArgs a = eval_args(p);
    a.n = n, a.seed = dseed.as<double>(), a.params = dpar.as<double>(), a.genes = dgenes.as<double>(), a.outi = dok.as<int32_t>();
    a.dpos = sp.dpos, a.drot = sp.drot, a.dtwist = sp.dtwist;
    LAUNCH(k_eval_check, eval_check_body(a, b_, l_), (n + nth - 1) / nth, nth, lds, 0, a);
    dok.download(ok);
    be_sync(0);
    API_END
}

int bioik_eval_bounds(bioik_problem* p, size_t n, const double* var_lo, const double* var_hi, double* out) {
    API_BEGIN
    if (!p || (n && (!var_lo || !var_hi || !out))) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return BIOIK_OK;
    if (n > 0x7fffffffull) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "too many queries for one launch");
    std::lock_guard<std::mutex> lock(p->mtx);
    DeviceGuard on_device(p->model->device);
    const size_t V = p->host.dev.V, M = p->host.dev.n_ops > 0 ? p->host.dev.n_ops : 1;
    DevBuf dlo(var_lo, n * V * 8), dhi(var_hi, n * V * 8), dout(n * M * 6 * 8);
    BoundsArgs a;
    a.pb = p->pb(), a.n = n, a.var_lo = dlo.as<double>(), a.var_hi = dhi.as<double>(), a.out = dout.as<double>();
    LAUNCH(k_eval_bounds, eval_bounds_body(a, b_, p_tid()), n, 64, 0, 0, a);
    dout.download(out);
    be_sync(0);
    API_END
}

int bioik_eval_arith(int device, int op, size_t n, const double* in, double* out) {
    API_BEGIN
    const int ni = arith_in(op), no = arith_out(op);
    if (ni == 0) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bioik_eval_arith: unknown op");
    if (n && (!in || !out)) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null array");
    if (n == 0) return BIOIK_OK;
    const int nd = be_device_count();
    if (nd <= 0) throw Error(BIOIK_ERR_NO_DEVICE, "no HIP device available: this library has no CPU path");
    if (device < 0 || device >= nd) throw Error(BIOIK_ERR_NO_DEVICE, "HIP device index out of range");
    DeviceGuard on_device(device);
    DevBuf din(in, n * ni * 8), dout(n * no * 8);
    ArithArgs a;
    a.op = op, a.pad = 0, a.n = n, a.in = din.as<double>(), a.out = dout.as<double>();
    const uint64_t grid = (n + 255) / 256;
    if (grid > 0x7fffffffull) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "too many elements for one launch");
    LAUNCH(k_eval_arith, arith_body(a, b_ * 256 + (uint64_t)p_tid()), grid, 256, 0, 0, a);
    dout.download(out);
    be_sync(0);
    API_END
}

int bioik_problem_op_count(const bioik_problem* p) { return p ? p->host.dev.n_ops : BIOIK_ERR_INVALID_ARGUMENT; }
int bioik_problem_op_variables(const bioik_problem* p, int32_t* variable, int32_t* gene) {
    if (!p || !variable || !gene) return BIOIK_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < p->host.dev.n_ops; k++) variable[k] = p->host.dev.ops[k].var, gene[k] = p->host.dev.ops[k].gene;
    return BIOIK_OK;
}
int bioik_problem_carry_doubles(const bioik_problem* p) { return p ? carry_doubles(p->host.dev.n_ops) : BIOIK_ERR_INVALID_ARGUMENT; }
int bioik_eval_migrate(bioik_problem* p, int32_t islands, size_t n_queries, const int32_t* live, double* rows) {
    API_BEGIN
    if (!p || islands < 1 || (n_queries && (!live || !rows))) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bad argument");
    if (n_queries == 0) return BIOIK_OK;
    const uint64_t units = (uint64_t)n_queries * (uint64_t)islands;
    if (units > 0x7fffffffull) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "too many (query, island) rows for one launch");
    std::lock_guard<std::mutex> lock(p->mtx);
    DeviceGuard on_device(p->model->device);
    const size_t R = (size_t)bioik_problem_carry_doubles(p);
    std::vector<int32_t> marks(units);  // (the solve's marks hold the boundary's number: here 1 for a live island)
    for (uint64_t u = 0; u < units; u++) marks[u] = live[u] != 0 ? 1 : 0;
    DevBuf dlive(marks.data(), units * 4), drows(rows, units * R * 8);
    MigrateArgs m;
    std::memset(&m, 0, sizeof(m));
    m.islands = islands, m.n_ops = p->host.dev.n_ops, m.exact = 1, m.mark = 1, m.n = n_queries;
    m.live = dlive.as<int32_t>(), m.rows = drows.as<double>();
    LAUNCH(k_migrate, migrate_coop(m, b_, p_tid()), n_queries, 64, 0, 0, m);
    drows.download(rows);
    be_sync(0);
    API_END
}

double bioik_sincos_domain(void) { return BIOIK_SINCOS_DOMAIN; }
double bioik_sincos_small_bound(void) { return BIOIK_SINCOS_SMALL; }

int bioik_stream_fitness_device(bioik_problem* p, size_t n_units, int population, const double* d_seeds, const double* d_goal_params, const double* d_genes,
                                double* d_fitness, void* hip_stream) {
    API_BEGIN
    if (!p || population <= 0) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "bad argument");
    if (n_units && (!d_seeds || !d_genes || !d_fitness || (p->host.dev.P > 0 && !d_goal_params))) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "null array");
    if (n_units == 0) return BIOIK_OK;
    std::lock_guard<std::mutex> lock(p->mtx);
    DeviceGuard on_device(p->model->device);
    int nth = population >= 256 ? 256 : (population + 63) / 64 * 64;
    // (a lane per individual: the genotype columns and parked frames grow with the lanes -- fewer lanes per workgroup where a CU would not hold them; the
    // lanes score their individuals independently, so the result does not change)
    while (nth > 64 && eval_lds_bytes(p, nth) > p->model->dev.lds_cu) nth -= 64;
    const size_t lds = eval_lds(p, eval_lds_bytes(p, nth));
    StreamArgs a;
    a.pb = p->pb();
    a.n_units = n_units;
    a.population = population;
    a.blocks_per_unit = (population + nth - 1) / nth;
    a.seeds = d_seeds, a.params = d_goal_params, a.genes = d_genes, a.fitness = d_fitness;
    uint64_t grid = (uint64_t)n_units * a.blocks_per_unit;
    if (grid > 0x7fffffffull) throw Error(BIOIK_ERR_INVALID_ARGUMENT, "too many units for one launch");
    LAUNCH(k_stream_fitness, stream_fitness_body(a, b_, l_), grid, nth, lds, (stream_t)hip_stream, a);
    API_END
}

}  // extern "C"
