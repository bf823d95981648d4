// bioik_layouts.h — the three device buffers the solve launcher cuts into blocks itself, each described ONCE: the function that takes a call's dimensions returns
// the blocks' offsets AND the buffer's size, so that the bytes asked of an allocator and the pointers handed to a kernel cannot disagree (finding 1).
// Host-only, plain arithmetic: no HIP, nothing of the device headers (tests/cpp/test_launcher_layouts.cpp compiles it alone).
#pragma once
#include <cstddef>
#include <cstdint>

namespace bioik {

// `count` elements of T at byte `off` of a buffer.  Offsets, not pointers: a layout exists before its buffer does.
template <class T>
struct Block {
    size_t off = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
    size_t end() const { return off + bytes(); }
    T* at(void* base) const { return (T*)((char*)base + off); }
    const T* at(const void* base) const { return (const T*)((const char*)base + off); }
};
inline size_t round_up(size_t bytes, size_t to) { return (bytes + to - 1) / to * to; }
// blocks one behind the other, each rounded up to `align` bytes
struct BlockCursor {
    size_t at = 0;
    template <class T>
    Block<T> take(size_t count, size_t align = 1) {
        const Block<T> b{at, count};
        at += round_up(b.bytes(), align);
        return b;
    }
};

// The arena of a host-pointer call (io_begin / io_finish): [seeds | goal_params | var_lo | var_hi] in, [solutions | fitness | success | steps | count] out, every
// block rounded up to 64 B; the bounds of a call that is not bounded and the count of one that is not ranked are empty blocks.  One layout serves the device arena
// and its page-locked host mirror.
struct IoArenaLayout {
    Block<double> seeds, goal_params, var_lo, var_hi;
    size_t in_bytes = 0;  // the inputs: what one transfer brings to the device
    Block<double> solutions, fitness;
    Block<int32_t> success, steps, count;
    size_t bytes = 0;
    bool bounded = false, ranked = false;
};
// n queries of V variables and P goal parameters, K result rows per query
inline IoArenaLayout io_arena_layout(size_t n, size_t V, size_t P, size_t K, bool bounded, bool ranked) {
    IoArenaLayout L;
    BlockCursor c;
    L.bounded = bounded, L.ranked = ranked;
    L.seeds = c.take<double>(n * V, 64);
    L.goal_params = c.take<double>(n * P, 64);
    L.var_lo = c.take<double>(bounded ? n * V : 0, 64);
    L.var_hi = c.take<double>(bounded ? n * V : 0, 64);
    L.in_bytes = c.at;
    L.solutions = c.take<double>(n * K * V, 64);
    L.fitness = c.take<double>(n * K, 64);
    L.success = c.take<int32_t>(n * K, 64);
    L.steps = c.take<int32_t>(n * K, 64);
    L.count = c.take<int32_t>(ranked ? n : 0, 64);
    L.bytes = c.at;
    return L;
}

// The scratch of a call with islands > 1 (SolveLauncher::result_arrays): the per-island result arrays, packed without padding, behind the control words of the fused
// island reduction -- `ctl_words` first_success words, then as many island_done words, the pair rounded up to 64 B; ctl_words = 0: not fused.  A call that is not
// fused keeps its first_success words (island_sync only) behind the arrays.  Both forms ask for 64 B + a word per query behind the arrays.
struct IslandScratchLayout {
    size_t ctl_words = 0;
    bool sync = false;
    Block<unsigned int> first_success, island_done;
    Block<double> solutions, fitness;
    Block<int32_t> success, steps;
    size_t bytes = 0;
};
inline IslandScratchLayout island_scratch_layout(size_t n, size_t islands, size_t V, size_t ctl_words, bool island_sync) {
    IslandScratchLayout L;
    BlockCursor c;
    const size_t units = n * islands;
    L.ctl_words = ctl_words, L.sync = island_sync;
    if (ctl_words) {
        L.first_success = c.take<unsigned int>(ctl_words);
        L.island_done = c.take<unsigned int>(ctl_words);
        c.at = round_up(c.at, 64);
    }
    L.solutions = c.take<double>(units * V);
    L.fitness = c.take<double>(units);
    L.success = c.take<int32_t>(units);
    L.steps = c.take<int32_t>(units);
    if (!ctl_words) L.first_success = Block<unsigned int>{c.at, island_sync ? n : 0};
    L.bytes = c.at + 64 + n * 4;
    return L;
}

// The workspace of a solve in several launches (SolveLauncher::run): the carried rows of every unit, then per hand-over a list of units (a word per unit, rounded up
// to 64 B) and, behind all lists, a counter in 64 B of its own; a migrating solve keeps a mark per unit behind the counters.  Launch j leaves through list(j) /
// counter(j) and launch j + 1 enters through them.
struct HandoverLayout {
    size_t units = 0, carry_doubles = 0, nh = 0;
    size_t list_stride = 0;
    Block<double> rows;
    size_t lists_off = 0, counters_off = 0;
    Block<int32_t> marks;
    Block<unsigned int> cleared;  // what every solve zeroes first: the counters and, behind them, the marks
    size_t bytes = 0;
    Block<int32_t> list(size_t j) const { return Block<int32_t>{lists_off + j * list_stride, units}; }
    Block<unsigned int> counter(size_t j) const { return Block<unsigned int>{counters_off + j * 64, 1}; }
};
inline HandoverLayout handover_layout(size_t units, size_t carry_doubles, size_t nh, bool migrating) {
    HandoverLayout L;
    BlockCursor c;
    L.units = units, L.carry_doubles = carry_doubles, L.nh = nh;
    L.list_stride = round_up(units * 4, 64);
    L.rows = c.take<double>(units * carry_doubles, 64);
    L.lists_off = c.at;
    c.at += nh * L.list_stride;
    L.counters_off = c.at;
    c.at += nh * 64;
    L.marks = c.take<int32_t>(migrating ? units : 0, 64);
    L.bytes = c.at;
    L.cleared = Block<unsigned int>{L.counters_off, (L.bytes - L.counters_off) / 4};
    return L;
}

}  // namespace bioik
