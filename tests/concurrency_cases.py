"""Solves that are in flight TOGETHER, shared by the host-simulator suite (tests/test_hostsim_concurrency.py) and the GPU suite (tests/test_gpu_concurrency.py):
the concurrent counterpart of tests/sequence_cases.py.  Overlapping solves of one handle share the counter of resident workgroups, the scratch map and the
control words resting in it, the retired and pinned buffers, the error words and the slot / ticket bookkeeping; host threads share the per-device clock reader,
the switches and -- each its own -- the last error.  Every answer is deterministic (no wall-clock limit here can expire), so every check is bit for bit:

  (a) every call equals the same call on a fresh handle, run alone (Sequences.fresh / check);
  (b) calls of at most sequence_cases.ORACLE_UNITS units also equal the oracle in trig mode 1 (inside Sequences.fresh);
  (c) the launcher's report of a window of overlapping calls cannot be attributed per call: the COUNT of every path in the window ("fused", "k_select",
      "k_select_wave", "handover", "point", "single") equals what the calls of the window must take -- no call loses its path silently.

On the host simulator "overlap" is its overlap mode (hostsim_overlap_begin: launches queued per stream, workgroups of different streams interleaved by a seeded
scheduler), run for every seed of `dev.overlap_seeds`; on the GPU it is real: nothing synchronises between the enqueues.  BIOIK_SOLVE_* switches are process-wide: a
window sets them once, before its first concurrent call, and nothing changes them while calls are in flight."""
import contextlib
import ctypes as C
import queue
import re
import threading

import numpy as np

import sequence_cases as sq
from bio_ik_amd import PoseGoal, ProblemTemplate, abi, snake
from bio_ik_amd import solver as solver_mod
from bio_ik_amd.solver import BioIKError
from bio_ik_amd.workload import make_queries
from conftest import random_configuration
from sequence_cases import Call

PATHS = ("fused", "k_select", "k_select_wave", "handover", "point", "single")
JOIN_SECONDS = 600.0  # (a thread still alive after this fails its test: nothing here waits for anything that long)


# ---- (c): the paths of a window ------------------------------------------------------------------------------------------------------------------------
def is_point(call):
    return str(call.kw.get("mode", "")).startswith(("gd", "jac"))


def tags_of(call, env):
    """the paths one call takes under the switches `env` (bioik_hip.hip: plan_handovers, result_arrays, select_islands)"""
    reduced = "k_select_wave" if call.islands >= 8 else "k_select"
    if is_point(call):
        return {"point", reduced if call.islands > 1 else "single"}
    handover = call.kw["max_steps"] > 1 and ("BIOIK_SOLVE_TWO_PHASE" in env or "BIOIK_SOLVE_DRAIN_TEST" in env)
    if call.islands == 1:
        tags = {"single"}
    elif handover or env.get("BIOIK_SOLVE_FUSED_SELECT") == "0":
        tags = {reduced}
    else:
        tags = {"fused"}
    return tags | ({"handover"} if handover else set())


def paths_expected(calls, env):
    want = dict.fromkeys(PATHS, 0)
    for c in calls:
        for t in tags_of(c, env):
            want[t] += 1
    return want


def paths_seen(text):
    """how often each path appears in the launcher's report of a window (one hand-over per call that has any: BIOIK_SOLVE_TWO_PHASE=1, BIOIK_SOLVE_DRAIN_TEST)"""
    first = len(re.findall(r"\[bioik\] launch: k_solve\w*, [^\n]*steps \[0, ", text))
    later = len(re.findall(r"\[bioik\] launch: k_solve\w*, [^\n]*steps \[-?[1-9]\d*, ", text))
    got = {"fused": text.count("[bioik] islands: reduced by the last island in the launch"), "k_select": text.count("[bioik] launch: k_select,"),
           "k_select_wave": text.count("[bioik] launch: k_select_wave,"), "point": text.count("[bioik] launch: k_solve_point,"), "handover": later}
    got["single"] = first + got["point"] - got["fused"] - got["k_select"] - got["k_select_wave"]
    return got


def mk(env, n, seed, **kw):
    """a Call under the window's switches, its `expect` the path that tells its kind"""
    c = Call(n, "?", seed=seed, env=env, **kw)
    tags = tags_of(c, env)
    c.expect = next(t for t in ("point", "handover", "fused", "k_select_wave", "k_select", "single") if t in tags)
    return c


class Concurrency(sq.Sequences):
    @contextlib.contextmanager
    def window(self, h, env):
        """the switches of a window of concurrent calls: set and read by the library once, before the first call; put back when nothing is in flight any more"""
        for k, v in env.items():
            self.mp.setenv(k, v)
        solver_mod.sync_debug_switches(h.L)
        try:
            yield
        finally:
            self.dev.sync()
            for k in env:
                self.mp.delenv(k, raising=False)
            solver_mod.sync_debug_switches(h.L)

    def enqueue_raw(self, h, call, io, s):
        """bioik_solve_batch_device on stream s under the window's switches; no wait"""
        (ds, dp), o = io
        with self.dev.on(s):
            h.solve_batch_device(call.params(), call.n, ds.ptr, dp.ptr, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, self.dev.handle(s))

    def reference(self, call):
        return getattr(call, "reference", call)

    def rounds(self, case, cfg, h, lanes, env, n_rounds=None, heavy=True):
        """`lanes` = [(stream, [calls])] of one handle: all calls enqueued round-robin over the streams with no synchronisation, then ONE sync; every output
        checked; repeated on the same handle with the outputs zeroed (the words at rest must be back in place), each round under the next overlap seed -- one round
        per seed, three at least, in EVERY window.  Calls marked `heavy` (S1's pair: 800 units and more, minutes in the simulator) are part of the rounds `dev.heavy_rounds(cfg)` names."""
        dev = self.dev
        heavy_in = dev.heavy_rounds(cfg) if heavy else ()  # (None: every round)

        def takes_part(c, r=None):
            """call c is part of round r (r = None: of any round)"""
            if not getattr(c, "heavy", False) or heavy_in is None:
                return True
            return bool(heavy_in) if r is None else r in heavy_in
        lanes = [(s, [c for c in cs if takes_part(c)]) for s, cs in lanes]
        calls = [c for _, cs in lanes for c in cs]
        for c in calls:
            self.fresh(cfg, self.reference(c))
        ios = {id(c): self.prepare(cfg, h, c) for c in calls}
        n_rounds = n_rounds or max(3, len(dev.overlap_seeds))
        with self.window(h, env):
            for r in range(n_rounds):
                lanes_r = [(s, [c for c in cs if takes_part(c, r)]) for s, cs in lanes]
                calls = [c for _, cs in lanes_r for c in cs]
                want = paths_expected(calls, env)
                for c in calls:
                    for b in ios[id(c)][1]:
                        b.zero()
                dev.sync()
                self.report.read()
                before = dev.interleaved()
                with dev.overlap(dev.overlap_seeds[r % len(dev.overlap_seeds)]):
                    for k in range(max(len(cs) for _, cs in lanes_r)):
                        for s, cs in lanes_r:
                            if k < len(cs):
                                self.enqueue_raw(h, cs[k], ios[id(cs[k])], s)
                dev.sync()
                got = paths_seen(self.report.read())
                assert got == want, (case, cfg, env, r, got, want)
                if before is not None:
                    assert dev.interleaved() > before, "%s: no workgroups of different streams interleaved" % case
                for c in calls:
                    self.check(case, cfg, self.reference(c), ios[id(c)], " (round %d, %s)" % (r, env))


def streams(seq, base, n=4):
    return [seq.dev.stream(base + i) for i in range(n)]


# ---- K1: streams of one handle, device-pointer entry ---------------------------------------------------------------------------------------------------
def k1_lists(env, V):
    """four lists of mixed kinds; S1's pair (finding1_sizes: a fused call of many queries, then one of few queries and many islands) split over two streams"""
    n_a, n_b, i_b, _, _ = sq.finding1_sizes(V)
    pair = [mk(env, n_a, 2, islands=2), mk(env, n_b, 3, islands=i_b)]
    for c in pair:
        c.heavy = True
    return [
        [mk(env, 3, 41, islands=4, steps=2), pair[0], mk(env, 2, 42, islands=3, steps=4, mode="gd_r"), mk(env, 4, 43, steps=2)],
        [mk(env, 2, 44, islands=8, steps=2, island_sync=1), pair[1], mk(env, 3, 45, steps=2)],
        [mk(env, 5, 46, islands=2, steps=2, island_sync=1), mk(env, 2, 47, islands=2, steps=3, mode="jac"), mk(env, 3, 41, islands=4, steps=2)],
        [mk(env, 1, 48, islands=6, steps=3), mk(env, 4, 49, steps=2), mk(env, 2, 50, islands=9, steps=2)],
    ]


def k1_streams(seq, cfg):
    """fused islands with and without island_sync, islands = 1, gd_r / jac with islands and S1's pair on four streams of one handle; then the same lists with the
    islands reduced by k_select / k_select_wave (BIOIK_SOLVE_FUSED_SELECT=0), then fused once more (the control words have to be set up again)"""
    h = seq.make_solver(seq.templates[cfg])
    ss = streams(seq, 10)
    for i, env in enumerate(({}, {"BIOIK_SOLVE_FUSED_SELECT": "0"}, {})):
        seq.rounds("K1", cfg, h, list(zip(ss, k1_lists(env, h.V))), env, heavy=i == 0)  # (S1's pair is about the fused form: the first window)
    h.close()


# ---- K2: hand-overs in flight together -----------------------------------------------------------------------------------------------------------------
def k2_lists(env):
    return [
        [mk(env, 3, 51, islands=3, steps=3), mk(env, 7, 23, islands=2, steps=2), mk(env, 2, 52, steps=4)],
        [mk(env, 2, 53, islands=8, steps=3), mk(env, 4, 54, steps=3), mk(env, 2, 55, islands=2, steps=3, mode="jac")],
        [mk(env, 5, 56, steps=4), mk(env, 3, 57, islands=4, steps=3, island_sync=1), mk(env, 1, 58, steps=1)],
        [mk(env, 2, 59, islands=2, steps=4), mk(env, 6, 60, steps=2), mk(env, 3, 61, islands=3, steps=2)],
    ]


def k2_handovers(seq, cfg):
    """K1's shape with every evolutionary call cut into two launches -- after its first step (BIOIK_SOLVE_TWO_PHASE=1), then unit by unit
    (BIOIK_SOLVE_DRAIN_TEST=3): several streams are each in the middle of a solve of several launches, their hand-over lists and counters in their own scratch"""
    h = seq.make_solver(seq.templates[cfg])
    ss = streams(seq, 20)
    for env in ({"BIOIK_SOLVE_TWO_PHASE": "1"}, {"BIOIK_SOLVE_DRAIN_TEST": "3"}):
        seq.rounds("K2", cfg, h, list(zip(ss, k2_lists(env))), env)
    h.close()


# ---- K7: a far wall-clock limit among overlapping calls ------------------------------------------------------------------------------------------------
def k7_far_timeout(seq, cfg="c2"):
    """timeout = 3600 s on some calls of a K1-like round: the deadline arithmetic must not cut a call short -- their results are the UNTIMED calls' results"""
    h = seq.make_solver(seq.templates[cfg])

    def timed(n, seed, **kw):
        c = mk({}, n, seed, timeout=3600.0, **kw)
        c.reference = mk({}, n, seed, **kw)
        return c
    lanes = [
        [timed(3, 62, islands=4, steps=3, island_sync=1), mk({}, 2, 63, islands=3, steps=2), timed(4, 64, steps=3)],
        [mk({}, 4, 65, steps=2), timed(2, 66, islands=2, steps=4, mode="gd_r"), mk({}, 3, 67, islands=4, steps=2)],
        [timed(2, 68, islands=8, steps=2), timed(5, 69, steps=2), mk({}, 2, 70, islands=2, steps=3, island_sync=1)],
        [timed(1, 71, islands=6, steps=3), mk({}, 3, 72, steps=3), timed(3, 73, islands=2, steps=2)],
    ]
    seq.rounds("K7", cfg, h, list(zip(streams(seq, 30), lanes)), {})
    h.close()


# ---- K3: submit / wait from one thread, mixed sizes and kinds ------------------------------------------------------------------------------------------
def k3_calls(h):
    """ten submits on six slots: 1, 3, 16 | 17 (either side of io_begin's direct_inputs), 64 and 300 queries; islands explicit and BIOIK_ISLANDS_AUTO; every schedule"""
    specs = [(1, dict(islands=abi.ISLANDS_AUTO, schedule="auto")), (3, dict(islands=abi.ISLANDS_AUTO, schedule="latency")), (16, dict(islands=2, schedule="throughput")),
             (17, dict(islands=1, schedule="auto")), (64, dict(islands=2, schedule="latency", island_sync=1)), (300, dict(islands=1, schedule="throughput")),
             (17, dict(islands=3, schedule="auto")), (16, dict(islands=1, schedule="latency")), (3, dict(islands=4, schedule="throughput", pop=128)),
             (1, dict(islands=1, schedule="auto", steps=3))]
    calls = []
    for k, (n, kw) in enumerate(specs):
        c = mk({}, n, 80 + k, **dict(dict(steps=2), **kw))
        c.islands = h.resolve_islands(c.params(), n)[0]  # (BIOIK_ISLANDS_AUTO: what the library makes of it -- the units of rule (b), the path of rule (c))
        c.expect = "single" if c.islands == 1 else "fused"
        calls.append(c)
    return calls


def same(got, want):
    return all(np.array_equal(x, y) for x, y in zip(got, want))


def k3_submit_wait(seq, cfg="c2"):
    """Ten submits per pass on the six slots of one handle, one pass per overlap seed (two on the device): tickets 0 - 3 are completed by the submits that take their
    slots again, five are waited for in a scrambled order (one of them complete already), 5 and 7 are never waited for -- the next pass's submits complete them, the
    last pass's are completed by close().  Every result equals the synchronous call's on a fresh handle."""
    h = seq.make_solver(seq.templates[cfg])
    calls = k3_calls(h)
    want = [seq.fresh(cfg, c) for c in calls]
    ins = [seq.queries(cfg, h, c) for c in calls]
    expected = paths_expected(calls, {})
    passes = list(seq.dev.overlap_seeds) * (2 if len(seq.dev.overlap_seeds) == 1 else 1)
    left = []
    with seq.window(h, {}):
        sizer = mk({}, max(c.n for c in calls), 5, steps=1)  # (every slot's arena sized for the largest batch first: a slot that grows waits for the whole device, hipFree)
        sq_ = seq.queries(cfg, h, sizer)
        for _ in range(6):
            h.wait_batch(h.submit_batch(sizer.params(), *sq_))
        for i, seed in enumerate(passes):
            seq.report.read()
            before = seq.dev.interleaved()
            with seq.dev.overlap(seed):
                tickets = [h.submit_batch(c.params(), *q) for c, q in zip(calls, ins)]
                for k, old in left:  # (never waited for: their slots have been taken again)
                    assert same(old[1], want[k]), ("K3 completed by the next pass", i, calls[k])
                for k in range(4):
                    assert same(tickets[k][1], want[k]), ("K3 completed by a later submit", i, calls[k])
                for k in (8, 4, 9, 0, 6):
                    assert same(h.wait_batch(tickets[k]), want[k]), ("K3 waited", i, calls[k])
                left = [(k, tickets[k]) for k in (5, 7)]
            got = paths_seen(seq.report.read())
            assert got == expected, ("K3", i, got, expected)
            if before is not None:  # (the simulator: at least as many workgroups ran beside another slot's launch as the pass has submits)
                assert seq.dev.interleaved() - before >= len(calls), ("K3: the submits of a pass did not overlap", i, seq.dev.interleaved() - before)
    h.close()
    for k, old in left:
        assert same(old[1], want[k]), ("K3 completed by close()", calls[k])


def finding3_destroy_completes_tickets(seq, cfg="c2"):
    """Finding 3: "a ticket that is never waited for is completed by a later submit or by bioik_problem_destroy" (include/bioik_hip.h) -- destroy waited for the
    slot's stream but never copied the results out of the slot's arena: the caller's arrays stayed as they were.  Three submits (direct inputs and staged ones),
    no wait, close(): the arrays hold the synchronous call's results."""
    h = seq.make_solver(seq.templates[cfg])
    calls = [mk({}, 2, 85, islands=2, steps=2), mk({}, 17, 86, steps=2), mk({}, 1, 87, steps=3)]
    want = [seq.fresh(cfg, c) for c in calls]
    tickets = [h.submit_batch(c.params(), *seq.queries(cfg, h, c)) for c in calls]
    h.close()
    for c, tk, w in zip(calls, tickets, want):
        assert same(tk[1], w), ("a ticket nobody waited for, after bioik_problem_destroy", c)


# ---- threads -------------------------------------------------------------------------------------------------------------------------------------------
def run_threads(jobs, case):
    """`jobs` (at most 8 callables) each on a thread of its own, started behind one barrier; exceptions are collected and the first re-raised here; a thread that is
    still alive after JOIN_SECONDS fails the test"""
    assert len(jobs) <= 8
    barrier = threading.Barrier(len(jobs))
    errors = []

    def body(job):
        try:
            barrier.wait(timeout=JOIN_SECONDS)
            job()
        except BaseException as e:  # noqa: B902 (whatever it is, the main thread raises it)
            errors.append((job.__name__, e))
            barrier.abort()
    threads = [threading.Thread(target=body, args=(j,), name="%s-%s" % (case, j.__name__), daemon=True) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    alive = [t.name for t in threads if t.is_alive()]
    assert not alive, "%s: threads still running: %s" % (case, alive)
    if errors:
        raise AssertionError("%s: %s failed: %r" % (case, errors[0][0], errors[0][1])) from errors[0][1]


def function_level_values(h, t, rng):
    """one set of function-level calls on handle h and their results"""
    full = random_configuration(t.model, rng, 9)
    seed, genes, par = full[0], full[1:, h.active_variables], t.pack_params()
    p = abi.default_solve_params()
    calls = [lambda: h.fk_genes(seed, genes), lambda: h.fitness(abi.FK_EXACT, seed, par, genes), lambda: h.fitness(abi.FK_LINEAR, seed, par, genes, genes[0]),
             lambda: h.check(p, seed, par, genes), lambda: h.approximator(seed, genes[0])]
    return calls, [c() for c in calls]


def as_tuple(x):
    return x if isinstance(x, tuple) else (x,)


def k4_threads_one_handle(seq, cfg="c2", rounds=12):
    """Six host threads on ONE handle for `rounds` rounds each: synchronous solves; submits whose tickets another thread waits for (handed over through a queue, waited
    for in pairs, the later first); device-pointer solves on a stream of their own; the function-level entries; bioik_resolve_islands.  Every thread checks its own
    results against what the same call gives single-threaded (solves: on a fresh handle)."""
    t = seq.templates[cfg]
    h = seq.make_solver(t)
    sync_calls = [mk({}, 3, 90, islands=4, steps=2), mk({}, 2, 91, steps=3), mk({}, 17, 92, islands=2, steps=2)]
    sub_calls = [mk({}, 2, 93, islands=3, steps=2), mk({}, 20, 94, steps=2), mk({}, 1, 95, islands=8, steps=2, island_sync=1), mk({}, 4, 96, steps=3)]
    dev_calls = [mk({}, 3, 97, islands=2, steps=3), mk({}, 5, 98, steps=2), mk({}, 2, 99, islands=8, steps=2)]
    for c in sync_calls + sub_calls + dev_calls:
        seq.fresh(cfg, c)
    q_of = {id(c): seq.queries(cfg, h, c) for c in sync_calls + sub_calls}
    ios = {id(c): seq.prepare(cfg, h, c) for c in dev_calls}
    s = seq.dev.stream(40)
    fl_calls, fl_want = function_level_values(h, t, np.random.default_rng(44))
    isl_cases = [(abi.default_solve_params(islands=abi.ISLANDS_AUTO), n) for n in (1, 16, 200, 1025)] + [(abi.default_solve_params(islands=3), 5)]
    isl_want = [h.resolve_islands(p, n) for p, n in isl_cases]
    tickets = queue.Queue()

    def synchronous():
        for r in range(rounds):
            c = sync_calls[r % len(sync_calls)]
            assert same(h.solve_batch(c.params(), *q_of[id(c)]), seq.fresh(cfg, c)), ("K4 solve_batch", r, c)

    def submitter():
        try:
            for r in range(rounds):
                c = sub_calls[r % len(sub_calls)]
                tickets.put((c, h.submit_batch(c.params(), *q_of[id(c)])))
        finally:
            tickets.put(None)

    def waiter():
        held, done = [], False
        while not done or held:
            if not done:
                item = tickets.get(timeout=JOIN_SECONDS)
                done = item is None
                if not done:
                    held.append(item)
            if len(held) == 2 or done:
                for c, tk in reversed(held):
                    assert same(h.wait_batch(tk), seq.fresh(cfg, c)), ("K4 submit / wait", c)
                held = []

    def device_pointer():
        for r in range(rounds):
            c = dev_calls[r % len(dev_calls)]
            with seq.dev.on(s):
                for b in ios[id(c)][1]:
                    b.zero()
            seq.enqueue_raw(h, c, ios[id(c)], s)
            seq.dev.sync_stream(s)
            seq.check("K4 solve_batch_device", cfg, c, ios[id(c)], " (round %d)" % r)

    def function_level():
        for r in range(rounds):
            for k, (call, want) in enumerate(zip(fl_calls, fl_want)):
                assert same(as_tuple(call()), as_tuple(want)), ("K4 function level", r, k)

    def resolve_islands():
        for r in range(rounds * 20):
            for (p, n), want in zip(isl_cases, isl_want):
                assert h.resolve_islands(p, n) == want, ("K4 resolve_islands", r, n)

    n_calls = {"sync": [sync_calls[r % len(sync_calls)] for r in range(rounds)], "sub": [sub_calls[r % len(sub_calls)] for r in range(rounds)],
               "dev": [dev_calls[r % len(dev_calls)] for r in range(rounds)]}
    with seq.window(h, {}):
        seq.report.read()
        run_threads([synchronous, submitter, waiter, device_pointer, function_level, resolve_islands], "K4")
        seq.dev.sync()
        got = paths_seen(seq.report.read())
    want = paths_expected(n_calls["sync"] + n_calls["sub"] + n_calls["dev"], {})
    assert got == want, ("K4", got, want)
    h.close()


# ---- K5: host threads, several handles -----------------------------------------------------------------------------------------------------------------
def k5_jobs(seq, gnarly_template):
    """(template, parameters, seeds, goal parameters, the answer of a fresh handle run alone) for c2, c3, c4 and the gnarly robot"""
    out = {}
    for name, t in list(seq.templates.items()) + [("gnarly", gnarly_template)]:
        h = seq.make_solver(t)
        if name == "gnarly":
            seeds = random_configuration(t.model, np.random.default_rng(5), 3)
            params = np.tile(t.pack_params(), (3, 1))
        else:
            seeds, params = make_queries(t, h.active_variables, h.fk_genes, 3, seed=77)[:2]
        p = abi.default_solve_params(population=16, max_steps=2, islands=2, random_seed=11)
        out[name] = (t, p, seeds, params, h.solve_batch(p, seeds, params))
        h.close()
    return out


def k5_threads_many_handles(seq, gnarly_template, rounds=6):
    """Two threads create a handle (c2, c3, c4, the gnarly robot in turn), solve on it and destroy it, `rounds` times each, while two others keep solving on long-lived
    handles; a fifth runs bioik_solve_batch_multi over three handles while a sixth solves on one of those three -- its result is the unsharded one."""
    jobs = k5_jobs(seq, gnarly_template)
    names = sorted(jobs)
    lived = {n: seq.make_solver(jobs[n][0]) for n in ("c2", "c4")}
    tri = [seq.make_solver(seq.templates["c2"]) for _ in range(3)]
    mc = mk({}, 7, 78, islands=2, steps=2)
    mq = seq.queries("c2", tri[0], mc)
    multi_want = seq.fresh("c2", mc)
    oc = mk({}, 3, 79, steps=3)
    oq = seq.queries("c2", tri[1], oc)
    seq.fresh("c2", oc)

    def churn(first):
        def job():
            for r in range(rounds):
                t, p, seeds, params, want = jobs[names[(first + r) % len(names)]]
                h = seq.make_solver(t)
                try:
                    assert same(h.solve_batch(p, seeds, params), want), ("K5 short-lived handle", names[(first + r) % len(names)], r)
                finally:
                    h.close()
        job.__name__ = "churn%d" % first
        return job

    def keep(name):
        def job():
            t, p, seeds, params, want = jobs[name]
            for r in range(rounds * 2):
                assert same(lived[name].solve_batch(p, seeds, params), want), ("K5 long-lived handle", name, r)
        job.__name__ = "keep_" + name
        return job

    def multi():
        for r in range(rounds):
            assert same(tri[0].solve_batch_multi(tri[1:], mc.params(), *mq), multi_want), ("K5 solve_batch_multi", r)

    def on_a_shard_handle():
        for r in range(rounds * 2):
            assert same(tri[1].solve_batch(oc.params(), *oq), seq.fresh("c2", oc)), ("K5 a solve on a handle bioik_solve_batch_multi is using", r)

    with seq.window(tri[0], {}):
        seq.report.read()
        run_threads([churn(0), churn(2), keep("c2"), keep("c4"), multi, on_a_shard_handle], "K5")
        got = paths_seen(seq.report.read())
    # (c): two-island solves of the short- and long-lived handles and of the three shards; one-island solves on the shard handle
    want = dict(dict.fromkeys(PATHS, 0), fused=2 * rounds + 2 * 2 * rounds + 3 * rounds, single=2 * rounds)
    assert got == want, ("K5", got, want)
    for h in list(lived.values()) + tri:
        h.close()


# ---- K6: errors stay with their thread -----------------------------------------------------------------------------------------------------------------
def k6_errors_stay_with_their_thread(seq, cfg="c2", rounds=10):
    """One thread makes failing calls in a loop -- a null array, an unknown ticket, a problem of 65 ops refused with BIOIK_ERR_UNSUPPORTED (limit_cases) -- and always
    reads its own code and message from bioik_last_error; another solves on the same handle, never sees an error, and its results are right."""
    t = seq.templates[cfg]
    h = seq.make_solver(t)
    too_large = ProblemTemplate(snake(65), "snake", [PoseGoal("tip")])
    c = mk({}, 3, 74, islands=2, steps=2)
    q = seq.queries(cfg, h, c)
    want = seq.fresh(cfg, c)
    p = c.params()

    def null_array():
        rc = h.L.bioik_solve_batch(h.problem, C.byref(p), 1, None, None, None, None, None, None)
        return rc, h.L.bioik_last_error().decode()

    def unknown_ticket():
        rc = h.L.bioik_solve_batch_wait(h.problem, C.c_uint64(10 ** 9))
        return rc, h.L.bioik_last_error().decode()

    def refused():
        try:
            seq.make_solver(too_large).close()
        except BioIKError as e:
            return e.code, str(e)
        return abi.OK, ""
    failing = (null_array, unknown_ticket, refused)
    alone = [f() for f in failing]  # single-threaded: the codes and messages
    assert [a[0] for a in alone] == [abi.ERR_INVALID_ARGUMENT, abi.ERR_INVALID_ARGUMENT, abi.ERR_UNSUPPORTED], alone
    assert "null array" in alone[0][1] and "unknown ticket" in alone[1][1] and all(a[1] for a in alone) and len({a[1] for a in alone}) == 3

    def fails():
        for r in range(rounds * 10):
            for f, a in zip(failing, alone):
                assert f() == a, ("K6 another call's error", r, f.__name__)

    def solves():
        assert h.L.bioik_last_error() == b"", "K6: a new thread starts with another thread's error"
        for r in range(rounds):
            assert same(h.solve_batch(p, *q), want), ("K6 results", r)
            tk = h.submit_batch(p, *q)
            assert same(h.wait_batch(tk), want), ("K6 results of a ticket", r)
            assert h.L.bioik_last_error() == b"", ("K6: the solving thread sees an error", r, h.L.bioik_last_error())

    with seq.window(h, {}):
        seq.report.read()
        run_threads([fails, solves], "K6")
        got = paths_seen(seq.report.read())
    want = paths_expected([c] * (2 * rounds), {})  # (the failing calls launch nothing)
    assert got == want, ("K6", got, want)
    h.close()


# ---- K8, K9: the device only ---------------------------------------------------------------------------------------------------------------------------
def k8_graphs_of_two_streams(seq, cfg="c2"):
    """One linear graph per stream of one handle, each captured after its eager warm-up call on that stream (include/bioik_hip.h), both launched with no sync between
    them, three rounds with the outputs zeroed, every replay checked; the graphs are destroyed before the handle"""
    h = seq.make_solver(seq.templates[cfg])
    ss = streams(seq, 50, 2)
    cs = [mk({}, 3, 21, islands=4, steps=3, island_sync=1), mk({}, sq.finding1_sizes(h.V)[0], 2, islands=2)]
    graphs = []
    try:
        ios = [seq.eager("K8 warm-up", cfg, h, c, s) for c, s in zip(cs, ss)]
        for c, s, io in zip(cs, ss, ios):
            graphs.append(seq.dev.capture(s, lambda: seq.enqueue(h, c, io, s)))
        for r in range(3):
            for io in ios:
                for b in io[1]:
                    b.zero()
            seq.dev.sync()
            for g, s in zip(graphs, ss):
                seq.dev.replay_on(g, s)
            seq.dev.sync()
            for c, io in zip(cs, ios):
                seq.check("K8", cfg, c, io, " (round %d)" % r)
    finally:
        for g in graphs:
            seq.dev.destroy(g)
    h.close()


def k9_chip_filling_calls_together(seq, cfg="c2", n=4096):
    """Two threads make a handle's FIRST chip-filling host-pointer calls (4096 queries, latency schedule) at the same moment.  Both go through bioik_solve_batch, which
    holds the handle's lock for the whole call: the "contention" is strict serialisation in either order, and what is checked is that the measured mapping choice is
    taken ONCE -- whichever call comes second finds the first one's entry -- and that both results are right.  Then six 4096-query submits under BIOIK_SCHEDULE_AUTO are
    waited for from two threads.  Results: a fresh handle's synchronous ones.  (Rule (c) is not asserted here: the measurement runs the first call once per eligible
    lane mapping, and which mappings are eligible is the launcher's business.)"""
    first = [mk({}, n, 100 + k, pop=128, steps=8) for k in range(2)]
    auto = [mk({}, n, 102 + k, pop=128, steps=8, schedule="auto") for k in range(2)]
    for c in first + auto:
        seq.fresh(cfg, c)
    h = seq.make_solver(seq.templates[cfg])
    qs = {id(c): seq.queries(cfg, h, c) for c in first + auto}

    def first_call(c):
        def job():
            assert same(h.solve_batch(c.params(), *qs[id(c)]), seq.fresh(cfg, c)), ("K9 first chip-filling call", c)
        job.__name__ = "first_call_%d" % c.seed
        return job
    with seq.window(h, {}):
        seq.report.read()
        run_threads([first_call(c) for c in first], "K9")
        text = seq.report.read()
        assert text.count("[bioik] measured mapping choice") == 1, text[-3000:]
        tickets = [(auto[k % 2], h.submit_batch(auto[k % 2].params(), *qs[id(auto[k % 2])])) for k in range(6)]

        def waits(mine):
            def job():
                for c, tk in mine:
                    assert same(h.wait_batch(tk), seq.fresh(cfg, c)), ("K9 submit / wait", c)
            job.__name__ = "waits_%d" % mine[0][1][0]
            return job
        run_threads([waits(tickets[0::2][::-1]), waits(tickets[1::2])], "K9")
    h.close()
