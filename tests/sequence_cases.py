"""Call sequences on ONE problem handle, shared by the host-simulator suite (tests/test_hostsim_sequences.py) and the GPU suite
(tests/test_gpu_sequences.py).  A handle keeps state from one call to the next -- the persistent scratch buffer per (stream, purpose), the fused island
reduction's control words that rest in it between calls, buffers pinned by captures and taken again by later ones, the hand-over workspace -- and every
case here makes a call whose answer could depend on what an earlier, DIFFERENT call left behind.  For every call of a sequence:

  (a) solutions, fitness, success and steps equal, bit for bit, the same call on a fresh handle of the same template;
  (b) small calls equal the oracle (trig mode 1, set by the calling suite) bit for bit, islands included;
  (c) the launcher took the path the case is about (BIOIK_SOLVE_REPORT): "single" (islands = 1), "fused" (the islands reduced by the solve's last island,
      SolveArgs::island_done), "k_select" / "k_select_wave" (a launch of their own), "handover" (more than one solve launch), "point" (k_solve_point).

`dev` is the suite's device: buffers (`buf(array)` -> .ptr, .get(), .zero()), streams (`stream(i)`, `handle(s)`, `on(s)`), `sync()` and captured graphs
(`capture(s, enqueue)`, `replay(g)`, `destroy(g)`).  The caller asserts what its device can see besides (the host simulator: no write out of bounds, nothing
inside a capture that HIP would refuse)."""
import contextlib
import re

import numpy as np

from bio_ik_amd import abi
from bio_ik_amd.workload import make_queries
from oracle import orc

ORACLE_UNITS = 48  # (b) for calls of at most this many (query, island) units


# ---- the scratch layout of a call with islands (bioik_hip.hip: SolveLauncher::result_arrays, scratch) --------------------------------------------------
def per_unit(V):
    """bytes per (query, island) of the per-island result arrays: solution, fitness, success, steps"""
    return 8 * V + 16


def ctl_bytes(words):
    """the fused form's control words (first_success, island_done) of `words` queries, rounded up to 64 B"""
    return (8 * words + 63) // 64 * 64


def request(V, n, islands, ctl_n):
    """bytes a call asks of the scratch buffer when its control words are laid out for `ctl_n` queries (0: not fused)"""
    return ctl_bytes(ctl_n) + n * islands * per_unit(V) + 64 + 4 * n


def grown(bytes_):
    """capacity of a buffer allocated for a request (1.5 x)"""
    return bytes_ + bytes_ // 2


def finding1_sizes(V, islands_a=2):
    """The smallest pair of fused calls A, B (fewest units in all) where B reuses A's buffer but, placing its arrays behind A's control words, would write past
    its end: A has n_a > 256 queries; B has n_b <= 256 (its own words are laid out for 256), asks for request(.., 256) <= capacity and would write up to
    ctl_bytes(n_a) + units_b * per > capacity.  Returns (n_a, n_b, islands_b, capacity, bytes past the end)."""
    per = per_unit(V)
    for n_a in range(257, 4096):
        cap = grown(request(V, n_a, islands_a, n_a))
        best = None
        for n_b in range(1, 257):
            i_b = max(2, (cap - ctl_bytes(n_a)) // (per * n_b) + 1)  # the fewest islands whose arrays behind A's words cross the end
            if request(V, n_b, i_b, 256) <= cap and (best is None or n_b * i_b < best[0] * best[1]):
                best = (n_b, i_b)
        if best:
            n_b, i_b = best
            return n_a, n_b, i_b, cap, ctl_bytes(n_a) + n_b * i_b * per - cap
    raise AssertionError("no such pair")


# ---- calls ---------------------------------------------------------------------------------------------------------------------------------------------
class Call:
    """One call: n queries (make_queries with `seed`), solve parameters, BIOIK_SOLVE_* switches in force during it, the path it must take"""

    def __init__(self, n, expect, islands=1, pop=16, steps=1, seed=1, env=None, **kw):
        self.n, self.expect, self.islands, self.env = n, expect, islands, dict(env or {})
        self.kw = dict(population=pop, max_steps=steps, islands=islands, random_seed=11, **kw)
        self.seed = seed

    def params(self):
        return abi.default_solve_params(**self.kw)

    def key(self):
        return (self.n, self.seed, tuple(sorted(self.kw.items())), tuple(sorted(self.env.items())))

    def __repr__(self):
        return "Call(n=%d, %s, env=%s)" % (self.n, ", ".join("%s=%s" % kv for kv in sorted(self.kw.items()) if kv[0] != "random_seed"), self.env)


def path_of(text):
    """the set of path tags of the launcher's report of one call"""
    kernels = re.findall(r"\[bioik\] launch: (k_\w+)", text)
    solves = [k for k in kernels if k not in ("k_select", "k_select_wave")]
    tags = set(k for k in kernels if k in ("k_select", "k_select_wave"))
    if "[bioik] islands: reduced by the last island in the launch" in text:
        tags.add("fused")
    if "k_solve_point" in solves:
        tags.add("point")
    if len(solves) > 1:
        tags.add("handover")
    if not tags & {"fused", "k_select", "k_select_wave"}:
        tags.add("single")
    assert solves, text[-1500:]
    return tags


_fresh_cache = {}


class Sequences:
    """Runs calls on handles of the library under test and checks (a), (b), (c) for each"""

    def __init__(self, make_solver, dev, report, monkeypatch, templates, oracles):
        self.make_solver, self.dev, self.report, self.mp = make_solver, dev, report, monkeypatch
        self.templates, self.oracles = templates, oracles

    @contextlib.contextmanager
    def switches(self, call):
        for k, v in call.env.items():
            self.mp.setenv(k, v)
        try:
            yield
        finally:
            for k in call.env:
                self.mp.delenv(k, raising=False)

    def queries(self, cfg, h, call):
        return make_queries(self.templates[cfg], h.active_variables, h.fk_genes, call.n, seed=call.seed)[:2]

    def fresh(self, cfg, call):
        """(a): the call on a fresh handle of the template (cached per device, template and call)"""
        key = (type(self.dev).__name__, cfg, call.key())
        if key not in _fresh_cache:
            h = self.make_solver(self.templates[cfg])
            seeds, params = self.queries(cfg, h, call)
            with self.switches(call):
                _fresh_cache[key] = h.solve_batch(call.params(), seeds, params)
            h.close()
            if call.n * call.islands <= ORACLE_UNITS and "timeout" not in call.kw:  # (b)
                want = self.oracles[cfg].solve_batch(call.params(), orc.RNG_COUNTER, seeds, params, n_threads=4)
                assert all(np.array_equal(x, y) for x, y in zip(want, _fresh_cache[key])), ("oracle", cfg, call)
            self.report.read()
        return _fresh_cache[key]

    def prepare(self, cfg, h, call):
        """device buffers of one call: inputs and outputs"""
        seeds, params = self.queries(cfg, h, call)
        ins = (self.dev.buf(np.ascontiguousarray(seeds)), self.dev.buf(np.ascontiguousarray(params)))
        outs = (self.dev.buf(np.zeros((call.n, h.V))), self.dev.buf(np.zeros(call.n)), self.dev.buf(np.zeros(call.n, dtype=np.int32)),
                self.dev.buf(np.zeros(call.n, dtype=np.int32)))
        return ins, outs

    def enqueue(self, h, call, io, s):
        (ds, dp), o = io
        with self.switches(call), self.dev.on(s):
            h.solve_batch_device(call.params(), call.n, ds.ptr, dp.ptr, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, self.dev.handle(s))

    def took(self, case, call):
        """(c): the path of the call(s) reported since the last read"""
        tags = path_of(self.report.read())
        assert call.expect in tags, (case, call, tags)

    def check(self, case, cfg, call, io, what=""):
        """(a) and (b): the outputs of `io` against the fresh handle's answer"""
        got = tuple(b.get() for b in io[1])
        want = self.fresh(cfg, call)
        for name, x, y in zip(("solutions", "fitness", "success", "steps"), got, want):
            assert np.array_equal(x, y), "%s %s: %s differ from a fresh handle's %s%s" % (case, cfg, name, call, what)

    def eager(self, case, cfg, h, call, s, io=None):
        """one call through bioik_solve_batch_device on stream s, waited for and checked"""
        io = io or self.prepare(cfg, h, call)
        self.fresh(cfg, call)
        for b in io[1]:
            b.zero()
        self.dev.sync()
        self.report.read()
        self.enqueue(h, call, io, s)
        self.dev.sync()
        self.took(case, call)
        self.check(case, cfg, call, io)
        return io

    def run(self, case, cfg, calls, h=None, s=None):
        """the calls one after the other on one handle and stream"""
        h = h or self.make_solver(self.templates[cfg])
        s = s if s is not None else self.dev.stream(1)
        for c in calls:
            self.eager(case, cfg, h, c, s)
        return h


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------
def s1_finding1(seq, cfg="c2"):
    """Finding 1, an eager write past the scratch buffer: a fused call A with many queries leaves its control words (laid out for n_a) at rest; a fused call B
    with few queries and many islands fits the buffer by its own request but placed its arrays behind A's words -- past the end of the allocation.  The sizes
    are the fewest units that cross the end for the template's V (finding1_sizes)."""
    h = seq.make_solver(seq.templates[cfg])
    n_a, n_b, i_b, cap, past = finding1_sizes(h.V)
    assert past > 0 and request(h.V, n_b, i_b, 256) <= cap
    seq.run("S1", cfg, [Call(n_a, "fused", islands=2, seed=2), Call(n_b, "fused", islands=i_b, seed=3)], h=h)
    return n_a, n_b, i_b, past


def s2_reverse_and_kinds(seq, cfg="c2"):
    """S1's calls in the reverse order; fused, then the same call reduced by k_select_wave (BIOIK_SOLVE_FUSED_SELECT=0), then fused again; island_sync on,
    off, on -- one handle, one stream"""
    h = seq.make_solver(seq.templates[cfg])
    n_a, n_b, i_b, _, _ = finding1_sizes(h.V)
    seq.run("S2", cfg, [Call(n_b, "fused", islands=i_b, seed=3), Call(n_a, "fused", islands=2, seed=2)], h=h)
    off = {"BIOIK_SOLVE_FUSED_SELECT": "0"}
    seq.run("S2", cfg, [Call(3, "fused", islands=8, seed=4), Call(3, "k_select_wave", islands=8, seed=4, env=off), Call(5, "k_select", islands=3, seed=5, env=off),
                        Call(3, "fused", islands=8, seed=4), Call(2, "fused", islands=3, seed=6, steps=3)], h=h)
    seq.run("S2", cfg, [Call(2, "fused", islands=4, seed=7, steps=3, island_sync=1), Call(2, "fused", islands=4, seed=7, steps=3, island_sync=0),
                        Call(2, "fused", islands=4, seed=8, steps=3, island_sync=1), Call(3, "k_select", islands=4, seed=8, steps=3, island_sync=1, env=off),
                        Call(2, "fused", islands=4, seed=7, steps=3, island_sync=1)], h=h)


def s3_interleaved(seq, cfg):
    """islands = 1, islands > 1, the point solvers gd_r / jac (their islands reduced by k_select) and a hand-over call (BIOIK_SOLVE_TWO_PHASE) between fused
    calls, on one handle and stream"""
    two = {"BIOIK_SOLVE_TWO_PHASE": "1"}
    seq.run("S3", cfg, [
        Call(3, "fused", islands=4, seed=9, steps=2),
        Call(4, "single", seed=10, steps=2),
        Call(2, "point", islands=3, seed=11, steps=4, mode="gd_r"),
        Call(3, "fused", islands=4, seed=9, steps=2),
        Call(2, "handover", islands=3, seed=12, steps=3, env=two),
        Call(5, "fused", islands=2, seed=13, steps=2, island_sync=1),
        Call(2, "point", islands=2, seed=14, steps=3, mode="jac"),
        Call(1, "single", seed=15, steps=2, env=two),
        Call(3, "fused", islands=4, seed=9, steps=2),
    ])


def s4_captures(seq, cfg="c2"):
    """Finding 2, graphs that corrupt each other: three graphs captured from ONE stream of one handle share its pinned scratch buffer -- G1 fused with
    n <= 256 (island_sync, a timeout), G2 fused with n > 256, G3 a hand-over solve with islands (its per-island arrays laid over the buffer's start, where the
    fused graphs keep their control words).  Each has had one eager call of the same plan on the stream (G2's last: the words at rest for its n); captured G2,
    G1, G3 (G1 finds G2's words at rest), they are replayed G1, G2, G1, G3, G2, G1 with eager calls of other sizes on the same stream between some replays,
    the outputs zeroed before every replay (an unwritten array fails), every replay equal to the answer of a fresh handle.  (G2 is S1's first call.)"""
    h = seq.make_solver(seq.templates[cfg])
    s = seq.dev.stream(2)
    two = {"BIOIK_SOLVE_TWO_PHASE": "1"}
    g1c = Call(3, "fused", islands=4, seed=21, steps=3, island_sync=1, timeout=3600.0)
    g2c = Call(finding1_sizes(h.V)[0], "fused", islands=2, seed=2)
    g3c = Call(20, "handover", islands=2, seed=23, steps=2, env=two)
    between = [Call(5, "fused", islands=3, seed=24), Call(2, "k_select", islands=2, seed=25, steps=2, env=two)]
    graphs = []
    try:
        ios = {}
        for name, c in (("G3", g3c), ("G1", g1c), ("G2", g2c)):
            ios[name] = seq.eager("S4 warm " + name, cfg, h, c, s)
        for name, c in (("G2", g2c), ("G1", g1c), ("G3", g3c)):  # (the largest first: the later captures fit its buffer)
            seq.report.read()
            g = seq.dev.capture(s, lambda: seq.enqueue(h, c, ios[name], s))
            seq.took("S4 capture " + name, c)
            graphs.append((name, c, g))
        by = {name: (c, g) for name, c, g in graphs}
        for i, name in enumerate(("G1", "G2", "G1", "G3", "G2", "G1")):
            c, g = by[name]
            for b in ios[name][1]:
                b.zero()
            seq.dev.sync()
            seq.dev.replay(g)
            seq.dev.sync()
            seq.check("S4", cfg, c, ios[name], " (replay %d of %s)" % (i, name))
            if i in (1, 3):
                seq.eager("S4 eager", cfg, h, between[i // 2], s)
    finally:
        for _, _, g in graphs:
            seq.dev.destroy(g)
    h.close()


def s5_two_streams(seq, cfg="c2"):
    """two streams of one handle, each with its own sequence, interleaved call by call: the scratch is keyed per stream"""
    h = seq.make_solver(seq.templates[cfg])
    s1, s2 = seq.dev.stream(3), seq.dev.stream(4)
    a = [Call(3, "fused", islands=4, seed=31, steps=2), Call(2, "k_select", islands=3, seed=32, steps=3, env={"BIOIK_SOLVE_TWO_PHASE": "1"}),
         Call(4, "fused", islands=2, seed=33, steps=2, island_sync=1)]
    b = [Call(2, "fused", islands=8, seed=34, steps=2), Call(3, "single", seed=35, steps=2), Call(1, "fused", islands=6, seed=36, steps=3)]
    for x, y in zip(a, b):
        seq.eager("S5 stream A", cfg, h, x, s1)
        seq.eager("S5 stream B", cfg, h, y, s2)
