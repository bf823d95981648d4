// hostsim_backend.h — TEST INFRASTRUCTURE (tests/hostsim): substitute for the HIP back end of bio_ik_amd/csrc/bioik_hip.hip.
// "Device memory" is host memory and a launch runs every workgroup as a gang of fibres (one per lane) of the calling thread that call the kernel body
// directly.  Injected with -DBIOIK_BACKEND_HEADER; never part of the product library.
#include <atomic>
#include <chrono>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <ucontext.h>
namespace sim {
thread_local Block* blk = nullptr;
thread_local int tid = 0;
}  // namespace sim
#include <chrono>
unsigned long long sim_wall_clock() {
    return (unsigned long long)(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() / 10);
}
static unsigned long long be_device_clock_now() { return sim_wall_clock(); }
static bool be_can_time() { return false; }  // (the simulator's times say nothing about the device: the launcher's measured mapping choice stays off)
template <class F>
static double be_time_ms(void*, F&& enqueue) {
    enqueue();
    return 0.0;
}
typedef void* stream_t;
// ---- guarded "device" allocations: every block of be_alloc / be_alloc_async lies between two redzones of a fixed pattern (64 B before it, 16 KiB behind
// it); be_free / be_free_async and hostsim_guard_violations() check them.  A damaged redzone is a write out of bounds on the device -- counted once per block,
// the first few reported on stderr with the block's size and the offset of the first damaged byte; nothing aborts.
namespace sim {
constexpr size_t kRedBefore = 64, kRedAfter = 16 * 1024;
constexpr unsigned char kRedByte = 0xa5;
struct Guarded {
    size_t bytes;
    bool reported;
};
static std::mutex guard_mtx;
static std::map<char*, Guarded> guarded;  // user pointer -> block
static unsigned long long n_guard_violations = 0;
static void check_block(char* p, Guarded& g, const char* when) {  // (guard_mtx held)
    if (g.reported) return;
    long first = 0;
    bool bad = false;
    for (size_t i = 0; i < kRedBefore && !bad; i++)
        if ((unsigned char)p[-(long)kRedBefore + (long)i] != kRedByte) bad = true, first = -(long)kRedBefore + (long)i;
    for (size_t i = 0; i < kRedAfter && !bad; i++)
        if ((unsigned char)p[g.bytes + i] != kRedByte) bad = true, first = (long)(g.bytes + i);
    if (!bad) return;
    g.reported = true;
    if (n_guard_violations++ < 8)
        std::fprintf(stderr, "[hostsim] write out of bounds (%s): block of %zu B, first damaged byte at offset %ld\n", when, g.bytes, first);
}
static void* guarded_alloc(size_t bytes) {
    const size_t total = (kRedBefore + bytes + kRedAfter + 63) / 64 * 64;
    char* raw = (char*)std::aligned_alloc(64, total);
    if (!raw) throw Error(BIOIK_ERR_HIP, "hipMalloc: out of host memory (hostsim)");
    std::memset(raw, kRedByte, kRedBefore);
    std::memset(raw + kRedBefore + bytes, kRedByte, kRedAfter);
    char* p = raw + kRedBefore;
    std::lock_guard<std::mutex> lock(guard_mtx);
    guarded[p] = Guarded{bytes, false};
    return p;
}
static void guarded_free(void* vp) {
    if (!vp) return;
    char* p = (char*)vp;
    std::lock_guard<std::mutex> lock(guard_mtx);
    auto it = guarded.find(p);
    if (it == guarded.end()) {
        n_guard_violations++;
        std::fprintf(stderr, "[hostsim] free of a pointer that is no live device block\n");
        return;
    }
    check_block(p, it->second, "at its release");
    guarded.erase(it);
    std::free(p - kRedBefore);
}
}  // namespace sim
extern "C" unsigned long long hostsim_guard_violations() {
    std::lock_guard<std::mutex> lock(sim::guard_mtx);
    for (auto& kv : sim::guarded) sim::check_block(kv.first, kv.second, "live block");
    return sim::n_guard_violations;
}
// ---- stream capture: tests pass small integers as streams (solve_batch_device); between hostsim_capture_begin(s) and hostsim_capture_end(s) the fills, the
// copies to the device and the launches enqueued on `s` are recorded in order -- closures that hold their arguments by value -- instead of run, and
// hostsim_graph_replay runs them again.  What HIP would refuse inside a capture (a stream-ordered allocation or release, a synchronisation, a copy to the
// host) is counted (hostsim_capture_violations) and done at once.
namespace sim {
static std::mutex capture_mtx;
static std::map<stream_t, std::vector<std::function<void()>>> capturing;
static std::map<long long, std::vector<std::function<void()>>> graphs;
static long long next_graph = 1;
static unsigned long long n_capture_violations = 0;
static bool is_capturing(stream_t s) {
    std::lock_guard<std::mutex> lock(capture_mtx);
    return capturing.count(s) != 0;
}
// `op` recorded when `s` is being captured (true), or not (false: the caller runs it)
static bool record(stream_t s, std::function<void()> op) {
    std::lock_guard<std::mutex> lock(capture_mtx);
    auto it = capturing.find(s);
    if (it == capturing.end()) return false;
    it->second.push_back(std::move(op));
    return true;
}
static void capture_violation(stream_t s, const char* what) {
    if (!is_capturing(s)) return;
    std::lock_guard<std::mutex> lock(capture_mtx);
    if (n_capture_violations++ < 8) std::fprintf(stderr, "[hostsim] %s on a stream that is being captured (HIP invalidates the capture)\n", what);
}
}  // namespace sim
static bool hostsim_overlapping();
extern "C" int hostsim_capture_begin(void* stream) {
    if (hostsim_overlapping()) return -1;  // (no capture in overlap mode)
    std::lock_guard<std::mutex> lock(sim::capture_mtx);
    return sim::capturing.emplace(stream, std::vector<std::function<void()>>{}).second ? 0 : -1;
}
extern "C" long long hostsim_capture_end(void* stream) {
    std::lock_guard<std::mutex> lock(sim::capture_mtx);
    auto it = sim::capturing.find(stream);
    if (it == sim::capturing.end()) return -1;
    const long long id = sim::next_graph++;
    sim::graphs[id] = std::move(it->second);
    sim::capturing.erase(it);
    return id;
}
extern "C" int hostsim_graph_replay(long long graph) {
    if (hostsim_overlapping()) return -1;
    std::vector<std::function<void()>> ops;
    {
        std::lock_guard<std::mutex> lock(sim::capture_mtx);
        auto it = sim::graphs.find(graph);
        if (it == sim::graphs.end()) return -1;
        ops = it->second;
    }
    for (auto& op : ops) op();
    return 0;
}
extern "C" int hostsim_graph_destroy(long long graph) {
    std::lock_guard<std::mutex> lock(sim::capture_mtx);
    return sim::graphs.erase(graph) ? 0 : -1;
}
extern "C" unsigned long long hostsim_capture_violations() {
    std::lock_guard<std::mutex> lock(sim::capture_mtx);
    return sim::n_capture_violations;
}
// ---- overlap mode: between hostsim_overlap_begin(seed) and hostsim_overlap_end() the fills, the copies to the device, the stream-ordered releases and the launches
// enqueued on ANY stream are queued per stream (held by value, as the capture recorder holds them) instead of run.  be_sync(s) and be_d2h(.., s) run the scheduler
// until stream s is empty, be_free (hipFree waits for the device) and hostsim_overlap_end() until every stream is: it picks a non-empty stream with a counter
// generator seeded by `seed` and runs the next WORKGROUP of that stream's head launch, or its head fill / copy / release.  Order within a stream is kept and a launch
// is complete before its stream's next operation starts; workgroups of launches on different streams interleave.  Capturing and replaying are refused meanwhile.
namespace sim {
struct Op {
    uint64_t grid = 0, next = 0;        // grid 0: a fill, a copy or a release (one step)
    std::function<void(uint64_t)> run;  // workgroup b of a launch (its LDS buffer lives in the closure)
};
static std::mutex overlap_mtx;  // held while an operation is enqueued and for the whole of a scheduler run (kernel bodies never come back to the back end)
static bool overlap_on = false;
static uint64_t overlap_seed = 0, overlap_ctr = 0;
static std::map<stream_t, std::deque<Op>> overlap_q;
static unsigned long long n_interleaved = 0;  // workgroups run while a launch of ANOTHER stream was part-way through its grid
static bool defer(stream_t s, Op op) {  // queued (true), or overlap mode is off (false: the caller runs it)
    std::lock_guard<std::mutex> lock(overlap_mtx);
    if (!overlap_on) return false;
    overlap_q[s].push_back(std::move(op));
    return true;
}
static uint64_t overlap_draw() {  // splitmix64 of seed + counter
    uint64_t z = overlap_seed + 0x9e3779b97f4a7c15ull * ++overlap_ctr;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static void drain_locked(const stream_t* only) {  // (overlap_mtx held) until stream *only is empty, or every stream
    std::vector<std::deque<Op>*> ready;
    for (;;) {
        ready.clear();
        int part_way = 0;
        for (auto& kv : overlap_q)
            if (!kv.second.empty()) ready.push_back(&kv.second), part_way += kv.second.front().next > 0 ? 1 : 0;
        if (ready.empty()) return;
        if (only) {
            auto it = overlap_q.find(*only);
            if (it == overlap_q.end() || it->second.empty()) return;
        }
        std::deque<Op>& q = *ready[overlap_draw() % ready.size()];
        Op& op = q.front();
        if (op.grid > 0 && part_way - (op.next > 0 ? 1 : 0) > 0) n_interleaved++;
        op.run(op.next);
        if (++op.next >= op.grid) q.pop_front();
    }
}
static void drain(const stream_t* only) {
    std::lock_guard<std::mutex> lock(overlap_mtx);
    if (overlap_on) drain_locked(only);
}
}  // namespace sim
extern "C" int hostsim_overlap_begin(unsigned long long seed) {
    std::lock_guard<std::mutex> lock(sim::overlap_mtx);
    {
        std::lock_guard<std::mutex> cap(sim::capture_mtx);
        if (!sim::capturing.empty()) return -1;
    }
    if (sim::overlap_on) return -1;
    sim::overlap_on = true, sim::overlap_seed = seed, sim::overlap_ctr = 0;
    return 0;
}
extern "C" int hostsim_overlap_end() {
    std::lock_guard<std::mutex> lock(sim::overlap_mtx);
    if (!sim::overlap_on) return -1;
    sim::drain_locked(nullptr);
    sim::overlap_on = false;
    sim::overlap_q.clear();
    return 0;
}
extern "C" unsigned long long hostsim_overlap_interleaved() {
    std::lock_guard<std::mutex> lock(sim::overlap_mtx);
    return sim::n_interleaved;
}
static bool hostsim_overlapping() {
    std::lock_guard<std::mutex> lock(sim::overlap_mtx);
    return sim::overlap_on;
}
// a fill, a copy or a release on stream s: recorded (capture), queued (overlap mode) or done at once
template <class F>
static void be_stream_op(stream_t s, F f) {
    if (sim::record(s, f)) return;
    if (sim::defer(s, sim::Op{0, 0, [f](uint64_t) { f(); }})) return;
    f();
}
static void be_zero_async(void* p, size_t bytes, stream_t s) {
    be_stream_op(s, [p, bytes]() { std::memset(p, 0, bytes); });
}
static void be_fill_ff_async(void* p, size_t bytes, stream_t s) {
    be_stream_op(s, [p, bytes]() { std::memset(p, 0xff, bytes); });
}
static void* be_alloc(size_t bytes) { return sim::guarded_alloc(bytes); }
static void be_free(void* p) {
    if (p) sim::drain(nullptr);  // (hipFree waits for the device)
    sim::guarded_free(p);
}
static void* be_alloc_pinned(size_t bytes) { return std::malloc(bytes ? bytes : 1); }
static void be_free_pinned(void* p) { std::free(p); }
static void* be_alloc_async(size_t bytes, stream_t s) {
    sim::capture_violation(s, "a stream-ordered allocation");
    return sim::guarded_alloc(bytes);
}
static bool be_stream_capturing(stream_t s) { return sim::is_capturing(s); }
static void be_free_async(void* p, stream_t s) {
    if (!p) return;
    sim::capture_violation(s, "a stream-ordered release");
    if (!sim::defer(s, sim::Op{0, 0, [p](uint64_t) { sim::guarded_free(p); }})) sim::guarded_free(p);  // (behind what the stream still holds)
}
static void be_h2d(void* d, const void* h, size_t bytes, stream_t s) {
    be_stream_op(s, [d, h, bytes]() { std::memcpy(d, h, bytes); });
}
static void be_d2h(void* h, const void* d, size_t bytes, stream_t s) {
    sim::capture_violation(s, "a copy to the host");
    sim::drain(&s);
    std::memcpy(h, d, bytes);
}
static void be_sync(stream_t s) {
    sim::capture_violation(s, "a synchronisation");
    sim::drain(&s);
}
static int be_device_count() { return 1; }
struct DeviceInfo {  // (the simulator stands for an MI355X)
    size_t lds_cu = 160 * 1024;
    int cus = 256, xcds = 8;
};
static DeviceInfo be_device_info(int) { return DeviceInfo{}; }
static void be_set_device(int) {}
static int be_get_device() { return 0; }
// (distinct tokens, far from the small integers the tests pass as streams: the scratch of the host-pointer slots is keyed per slot, as on the device)
static stream_t be_stream_create() {
    static std::atomic<uintptr_t> next{0};
    return (stream_t)(uintptr_t)(0x10000u + 16u * ++next);
}
static void be_stream_destroy(stream_t) {}
// One workgroup at a time; its lanes are fibres of the calling thread, scheduled round-robin: a lane runs until it waits at a rendezvous
// (or ends), then the next unfinished lane continues.  sim::tid is the running lane.
namespace sim {
struct Fibres {
    static constexpr size_t kStack = 2u << 20;  // per lane (the kernel bodies are one large inlined frame)
    ucontext_t main;
    std::vector<ucontext_t> ctx;
    std::vector<char> done;
    std::vector<std::unique_ptr<char[]>> stacks;  // kept across workgroups and launches
    int n = 0, alive = 0;
    std::function<void()> run;  // the kernel body of the running lane
};
static thread_local Fibres fib;
static int next_unfinished(int me) {
    int nx = me;
    do nx = nx + 1 == fib.n ? 0 : nx + 1;
    while (fib.done[nx] && nx != me);
    return nx;
}
static unsigned long long n_site_mismatches = 0;  // (relaxed: a diagnostic counter read by the tests between launches)
void site_mismatch(int first, int now) {
    // (the second rendezvous of a two-phase collective carries the negated line)
    if (__atomic_fetch_add(&n_site_mismatches, 1ull, __ATOMIC_RELAXED) < 8)
        std::fprintf(stderr, "[hostsim] divergent collective: lane %d of workgroup %d arrived from line %d at a rendezvous opened from line %d\n", tid, blk->block_id, now, first);
    if (std::getenv("BIOIK_HOSTSIM_SITES_FATAL")) std::abort();
}
void yield() {
    const int me = tid, nx = next_unfinished(me);
    if (nx == me) return;
    tid = nx;
    swapcontext(&fib.ctx[me], &fib.ctx[nx]);  // (whoever resumes this lane has set tid back to it)
}
static void lane_main() {
    fib.run();
    const int me = tid;
    fib.done[me] = 1;
    if (--fib.alive == 0) setcontext(&fib.main);
    tid = next_unfinished(me);
    setcontext(&fib.ctx[tid]);
}
}  // namespace sim
// "run block b" of a launch that has been set up (its lanes, its LDS buffer, its body): the whole workgroup, on the calling thread
template <class Body>
static void be_run_block(uint64_t b, int block, double* lds, const Body& body) {
    sim::Fibres& f = sim::fib;
    while ((int)f.stacks.size() < block) f.stacks.emplace_back(new char[sim::Fibres::kStack]);
    sim::Block blk;
    blk.nthreads = block;
    blk.block_id = (int)b;
    blk.bar.n = block;
    blk.bar.rounds.assign((size_t)block, 0ull);
    {
        sim::Rendezvous of_a_wave;
        of_a_wave.n = 64;
        of_a_wave.rounds.assign((size_t)block, 0ull);
        blk.wave_bar.assign((size_t)(block / 64), of_a_wave);
    }
    blk.xchg.assign((size_t)block, 0);
    f.n = f.alive = block;
    f.ctx.assign((size_t)block, ucontext_t());
    f.done.assign((size_t)block, 0);
    f.run = [&]() { body(b, lds); };
    for (int t = 0; t < block; t++) {
        getcontext(&f.ctx[t]);
        f.ctx[t].uc_stack.ss_sp = f.stacks[t].get();
        f.ctx[t].uc_stack.ss_size = sim::Fibres::kStack;
        f.ctx[t].uc_link = nullptr;
        makecontext(&f.ctx[t], sim::lane_main, 0);
    }
    sim::blk = &blk;
    sim::tid = 0;
    swapcontext(&f.main, &f.ctx[0]);  // returns when the last lane has ended
    sim::blk = nullptr;
}
// every workgroup of a launch now, one after the other, sharing one LDS buffer
template <class Body>
static void be_launch_now(uint64_t grid, int block, size_t lds_bytes, const Body& body) {
    std::vector<double> lds(lds_bytes / 8 + 2);
    for (uint64_t b = 0; b < grid; b++) be_run_block(b, block, lds.data(), body);
}
// ... or, in overlap mode, queued on its stream with an LDS buffer of its own (`body` holds its arguments by value)
template <class Body>
static void be_launch(uint64_t grid, int block, size_t lds_bytes, stream_t s, Body body) {
    if (grid == 0) return;
    if (hostsim_overlapping()) {
        auto lds = std::make_shared<std::vector<double>>(lds_bytes / 8 + 2);
        if (sim::defer(s, sim::Op{grid, 0, [block, lds, body](uint64_t b) { be_run_block(b, block, lds->data(), body); }})) return;
    }
    be_launch_now(grid, block, lds_bytes, body);
}
// The device's rules for dynamic LDS, enforced where the device enforces them: a launch that asks for more than 64 KiB fails unless its kernel is one of
// BIOIK_WIDE_LDS_KERNELS and was allowed at least that much (be_allow_lds), an allowance or a launch beyond a CU's LDS fails.  Both fail as a failed
// hipFuncSetAttribute / hipGetLastError() does on the device (BIOIK_ERR_HIP), so that the CPU suite sees what the device would.
static std::atomic<size_t> g_allowed_lds{64 * 1024};
static bool wide_lds_kernel(const char* name) {
#define HOSTSIM_NAME_(k) #k,
    static const char* const names[] = {BIOIK_WIDE_LDS_KERNELS(HOSTSIM_NAME_)};
#undef HOSTSIM_NAME_
    for (const char* n : names)
        if (std::strcmp(n, name) == 0) return true;
    return false;
}
static void be_check_lds(const char* kernel, size_t bytes) {
    if (bytes > DeviceInfo{}.lds_cu) throw Error(BIOIK_ERR_HIP, std::string("hipGetLastError(): ") + kernel + " launched with " + std::to_string(bytes) + " B of LDS (more than a CU has)");
    if (bytes <= 64 * 1024) return;
    if (!wide_lds_kernel(kernel) || g_allowed_lds.load() < bytes)
        throw Error(BIOIK_ERR_HIP, std::string("hipGetLastError(): ") + kernel + " launched with " + std::to_string(bytes) + " B of LDS, more than 64 KiB and more than it was allowed");
}
static void be_allow_lds(size_t bytes) {
    if (bytes > DeviceInfo{}.lds_cu) throw Error(BIOIK_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize): " + std::to_string(bytes) + " B is more than a CU has");
    g_allowed_lds.store(bytes);
}
#define LAUNCH(KERNEL, BODYCALL, grid, block, lds, stream, args)                                        \
    do {                                                                                                \
        be_check_lds(#KERNEL, lds);                                                                     \
        auto body_ = [args](uint64_t b_, double* l_) { BODYCALL; }; /* (by value: nothing else may be named) */ \
        const uint64_t grid_ = (grid);                                                                  \
        const int block_ = (block);                                                                     \
        const size_t lds_ = (lds);                                                                      \
        if (!sim::record((stream_t)(stream), [=]() { be_launch_now(grid_, block_, lds_, body_); })) \
            be_launch(grid_, block_, lds_, (stream_t)(stream), body_);                                   \
    } while (0)
// What the tests read of the simulator itself (tests/test_hostsim_parity.py): how often lanes met at DIFFERENT collectives so far -- on the device that
// is a silent exchange of garbage --, and a launch that does it on purpose (odd lanes synchronise from another line than even ones)
extern "C" unsigned long long hostsim_divergent_collectives() { return __atomic_load_n(&sim::n_site_mismatches, __ATOMIC_RELAXED); }
extern "C" void hostsim_selftest_divergence(int diverge) {
    be_launch_now(1, 64, 64, [&](uint64_t, double* l) {
        const int lane = p_tid();
        l[0] = 0.0;
        p_wave_sync();
        if (diverge && (lane & 1)) {
            p_wave_sync();
        } else {
            p_wave_sync();
        }
        const int sum = p_read_lane(lane, 63) + p_shfl_xor(lane, 1);  // (collectives from one line each: no report)
        if (lane == 0) l[0] = (double)sum;
    });
}
// ... and the two other detectors, on purpose (tests/test_hostsim_sequences.py): one byte written at offset `at` of a fresh block of `bytes` (at >= bytes: past
// its end), and a 0xff fill of words[0] followed by a launch of two workgroups whose first lanes add one to words[1] each, enqueued on `stream`
extern "C" void hostsim_selftest_write(unsigned long long bytes, unsigned long long at) {
    char* p = (char*)be_alloc((size_t)bytes);
    p[at] = 0x11;
    be_free(p);
}
extern "C" void hostsim_selftest_enqueue(void* stream, unsigned int* words) {
    struct {
        unsigned int* w;
    } a{words};
    be_fill_ff_async(words, 4, (stream_t)stream);
    LAUNCH(k_selftest, (void)(p_tid() == 0 && ++a.w[1]), 2, 64, 0, (stream_t)stream, a);
}
// ... and the scheduler of overlap mode: a launch of `blocks` workgroups on `stream` whose first lanes append (id, block) to log[1..] (log[0]: entries so far)
extern "C" void hostsim_selftest_log(void* stream, int id, int blocks, int* log) {
    struct {
        int* log;
        int id;
    } a{log, id};
    LAUNCH(k_selftest_log, (void)(p_tid() == 0 && (a.log[1 + 2 * a.log[0]] = a.id, a.log[2 + 2 * a.log[0]] = (int)b_, ++a.log[0])), (uint64_t)blocks, 64, 0, (stream_t)stream, a);
}
