// The launcher's three buffer layouts (bio_ik_amd/csrc/bioik_layouts.h) over a grid of call dimensions: the blocks lie in the documented order without overlap, each is
// aligned for its element type (64 B where the launcher rounds), the last one ends inside `bytes`, and `bytes` is the closed form the launcher has always asked its
// allocators for -- restated here, not taken from the header.  Stand-alone: the header and the C-ABI's constants, no library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bioik_hip.h"
#include "bioik_layouts.h"

using namespace bioik;

static long n_checks = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        n_checks++;                                        \
        if (!(cond)) {                                     \
            std::printf("FAILED %s: ", #cond);             \
            std::printf(__VA_ARGS__);                      \
            std::printf(" (line %d)\n", __LINE__);         \
            std::exit(1);                                  \
        }                                                  \
    } while (0)

static size_t up64(size_t b) { return (b + 63) / 64 * 64; }

struct Span {
    const char* name;
    size_t off, bytes, align;
};
template <class T>
static Span span(const char* name, const Block<T>& b, size_t align = alignof(T)) {
    return Span{name, b.off, b.bytes(), align};
}
// the spans in the order given: ascending, disjoint, aligned, inside the buffer
static void check_spans(const char* layout, const std::vector<Span>& spans, size_t bytes) {
    size_t end = 0;
    for (const Span& s : spans) {
        CHECK(s.off >= end, "%s: %s at %zu begins inside the block before it (ends at %zu)", layout, s.name, s.off, end);
        CHECK(s.off % s.align == 0, "%s: %s at %zu is not aligned to %zu", layout, s.name, s.off, s.align);
        end = s.off + s.bytes;
    }
    CHECK(end <= bytes, "%s: the last block ends at %zu, beyond the %zu B of the buffer", layout, end, bytes);
}

static void check_arena(size_t n, size_t V, size_t P, size_t K, bool bounded, bool ranked) {
    const IoArenaLayout L = io_arena_layout(n, V, P, K, bounded, ranked);
    const size_t nb = bounded ? n * V * 8 : 0;
    const size_t in = up64(n * V * 8) + up64(n * P * 8) + 2 * up64(nb);
    const size_t want = in + up64(n * K * V * 8) + up64(n * K * 8) + 2 * up64(n * K * 4) + (ranked ? up64(n * 4) : 0);
    CHECK(L.bytes == want, "arena n %zu V %zu P %zu K %zu: %zu B, the closed form gives %zu", n, V, P, K, L.bytes, want);
    CHECK(L.in_bytes == in && L.solutions.off == in, "arena: the inputs end at %zu, the results begin at %zu, closed form %zu", L.in_bytes, L.solutions.off, in);
    CHECK(L.seeds.count == n * V && L.goal_params.count == n * P && L.solutions.count == n * K * V && L.fitness.count == n * K && L.success.count == n * K && L.steps.count == n * K,
          "arena n %zu: a block's element count", n);
    CHECK(L.var_lo.count == (bounded ? n * V : 0) && L.var_hi.count == L.var_lo.count && L.count.count == (ranked ? n : 0), "arena n %zu: the optional blocks", n);
    check_spans("arena", {span("seeds", L.seeds, 64), span("goal_params", L.goal_params, 64), span("var_lo", L.var_lo, 64), span("var_hi", L.var_hi, 64), span("solutions", L.solutions, 64),
                          span("fitness", L.fitness, 64), span("success", L.success, 64), span("steps", L.steps, 64), span("count", L.count, 64)},
                L.bytes);
}

static size_t island_request(size_t n, size_t islands, size_t V, size_t words) { return (2 * words * 4 + 63) / 64 * 64 + n * islands * (V * 8 + 8 + 4 + 4) + 64 + n * 4; }
static void check_islands(size_t n, size_t islands, size_t V, size_t words, bool sync) {
    const IslandScratchLayout L = island_scratch_layout(n, islands, V, words, sync);
    const size_t units = n * islands;
    CHECK(L.bytes == island_request(n, islands, V, words), "islands n %zu x %zu V %zu words %zu: %zu B, the closed form gives %zu", n, islands, V, words, L.bytes, island_request(n, islands, V, words));
    CHECK(L.solutions.count == units * V && L.fitness.count == units && L.success.count == units && L.steps.count == units, "islands: a block's element count");
    CHECK(L.ctl_words == words && L.sync == sync, "islands: the dimensions kept");
    // the four arrays are packed: no padding between them
    CHECK(L.fitness.off == L.solutions.end() && L.success.off == L.fitness.end() && L.steps.off == L.success.end(), "islands: the arrays are not packed");
    if (words) {  // fused: [first_success | island_done] rounded up to 64 B, then the arrays
        CHECK(L.first_success.off == 0 && L.first_success.count == words && L.island_done.off == words * 4 && L.island_done.count == words, "islands: the control words");
        CHECK(L.solutions.off == up64(8 * words), "islands: the arrays begin at %zu behind %zu control words", L.solutions.off, words);
        check_spans("islands (fused)", {span("first_success", L.first_success), span("island_done", L.island_done), span("solutions", L.solutions, 64), span("fitness", L.fitness),
                                        span("success", L.success), span("steps", L.steps)},
                    L.bytes);
    } else {  // the arrays, then first_success (island_sync only)
        CHECK(L.solutions.off == 0 && L.island_done.count == 0, "islands: the unfused form begins with the arrays");
        CHECK(L.first_success.off == L.steps.end() && L.first_success.count == (sync ? n : 0), "islands: the unfused form's first_success words");
        check_spans("islands", {span("solutions", L.solutions, 64), span("fitness", L.fitness), span("success", L.success), span("steps", L.steps), span("first_success", L.first_success)}, L.bytes);
    }
}

static void check_handover(size_t units, size_t carry, size_t nh, bool migrating) {
    const HandoverLayout L = handover_layout(units, carry, nh, migrating);
    const size_t list_bytes = up64(units * 4), list_off = up64(units * carry * 8), count_off = list_off + nh * list_bytes, mark_off = count_off + nh * 64;
    const size_t want = mark_off + (migrating ? list_bytes : 0);
    CHECK(L.bytes == want, "hand-over units %zu carry %zu nh %zu: %zu B, the closed form gives %zu", units, carry, nh, L.bytes, want);
    CHECK(L.lists_off == list_off && L.counters_off == count_off && L.marks.off == mark_off, "hand-over: the offsets of the lists, the counters, the marks");
    CHECK(L.rows.off == 0 && L.rows.count == units * carry && L.marks.count == (migrating ? units : 0), "hand-over: a block's element count");
    CHECK(L.cleared.off == count_off && L.cleared.bytes() == nh * 64 + (migrating ? list_bytes : 0), "hand-over: what a solve zeroes");
    std::vector<Span> spans{span("rows", L.rows, 64)};
    for (size_t j = 0; j < nh; j++) {
        CHECK(L.list(j).off == list_off + j * list_bytes && L.list(j).count == units, "hand-over: list %zu", j);
        spans.push_back(span("list", L.list(j), 64));
    }
    for (size_t j = 0; j < nh; j++) {
        CHECK(L.counter(j).off == count_off + j * 64 && L.counter(j).count == 1, "hand-over: counter %zu", j);
        spans.push_back(span("counter", L.counter(j), 64));
    }
    spans.push_back(span("marks", L.marks, 64));
    check_spans("hand-over", spans, L.bytes);
}

int main() {
    const size_t Vs[] = {1, 7, 63}, ns[] = {1, 16, 17, 255, 256, 257, 1000}, islands_of[] = {1, 2, 64}, Ks[] = {1, 3}, Ps[] = {0, 7, 10};
    const size_t nhs[] = {1, 2, (size_t)BIOIK_MAX_MIGRATIONS}, carries[] = {1, 9, 130};
    for (size_t V : Vs)
        for (size_t n : ns) {
            for (size_t P : Ps)
                for (size_t K : Ks)
                    for (int bounded = 0; bounded < 2; bounded++)
                        for (int ranked = 0; ranked < 2; ranked++) check_arena(n, V, P, K, bounded != 0, ranked != 0);
            for (size_t islands : islands_of) {
                const size_t words_of[] = {0, 256, n, 1000};
                for (size_t words : words_of)
                    for (int sync = 0; sync < 2; sync++) check_islands(n, islands, V, words, sync != 0);
                for (size_t nh : nhs)
                    for (size_t carry : carries)
                        for (int migrating = 0; migrating < 2; migrating++) check_handover(n * islands, carry, nh, migrating != 0);
            }
        }
    {  // finding 1 by its numbers, V = 7: call A, 1000 queries x 2 islands, then call B, 50 queries x 64 islands, on A's buffer
        const IslandScratchLayout A = island_scratch_layout(1000, 2, 7, 1000, false);
        CHECK(A.bytes == 156064, "finding 1: A asks for %zu B", A.bytes);
        const size_t capacity = A.bytes + A.bytes / 2;
        CHECK(capacity == 234096, "finding 1: A's buffer holds %zu B", capacity);
        const IslandScratchLayout B = island_scratch_layout(50, 64, 7, 1000, false);  // behind A's 1000 words at rest
        CHECK(B.bytes == 238664 && B.bytes > capacity, "finding 1: B behind A's words asks for %zu B (the buffer has to grow)", B.bytes);
        CHECK(B.steps.end() <= B.bytes && B.steps.end() > capacity, "finding 1: B's last array ends at %zu", B.steps.end());
        const IslandScratchLayout B_own = island_scratch_layout(50, 64, 7, 256, false);  // with 256 words of its own
        CHECK(B_own.bytes == 232712 && B_own.bytes <= capacity && B_own.steps.end() <= B_own.bytes, "finding 1: B with its own words asks for %zu B", B_own.bytes);
    }
    std::printf("%ld checks\nok\n", n_checks);
    return 0;
}
