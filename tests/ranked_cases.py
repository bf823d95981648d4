"""Ranked solves (bioik_solve_batch_ranked: the k best distinct islands of every query), shared by the host-simulator suite (tests/test_hostsim_ranked.py)
and the GPU suite (tests/test_gpu_ranked.py).

The expectation is built without the code under test: the oracle's stateful single-island solver is stepped like run_island (step, check, stop at success or
max_steps) on the random stream of (random_seed, first_query + q, island); Oracle.fitness supplies the secondary sum a success adds; the order -- passed
first, ascending fitness, ties to the lower island -- and the greedy distance rule -- kept iff max over the active variables |a - b| > min_distance against
every row kept before -- are applied in numpy.

`ctx` is the suite's context: make_solver(template), dev (buffers, streams, captures: as sequence_cases), templates, oracles, mp (monkeypatch)."""
import contextlib

import numpy as np

from bio_ik_amd import abi
from bio_ik_amd.solver import BioIKError
from bio_ik_amd.workload import make_queries
from oracle import orc

NAMES = ("solutions", "fitness", "success", "steps", "count")


class Ctx:
    def __init__(self, make_solver, dev, templates, oracles, mp):
        self.make_solver, self.dev, self.templates, self.oracles, self.mp = make_solver, dev, templates, oracles, mp

    @contextlib.contextmanager
    def env(self, **kw):
        for k, v in kw.items():
            self.mp.setenv(k, v)
        try:
            yield
        finally:
            for k in kw:
                self.mp.delenv(k, raising=False)


# ---- the expectation -----------------------------------------------------------------------------------------------------------------------------------
_island_cache = {}


def island_results(oracle, kw, seeds, gparams, first_query=0):
    """every island of every query by the oracle: (solutions [n][I][V], fitness [n][I], success [n][I], steps [n][I]); fitness holds the secondary term of a success"""
    key = (id(oracle), tuple(sorted(kw.items())), seeds.tobytes(), gparams.tobytes(), first_query)
    if key in _island_cache:
        return _island_cache[key]
    p = abi.default_solve_params(**kw)
    n, islands = seeds.shape[0], kw["islands"]
    active = np.asarray(oracle.active_variables)
    sol = np.zeros((n, islands, oracle.V))
    fit = np.zeros((n, islands))
    suc = np.zeros((n, islands), dtype=np.int32)
    steps = np.zeros((n, islands), dtype=np.int32)
    for q in range(n):
        for i in range(islands):
            s = oracle.solver(p, orc.RNG_COUNTER, orc.query_key(p.random_seed, first_query + q, i), seeds[q], gparams[q])
            x, ok, f, st = seeds[q].copy(), False, 0.0, 0
            while st < p.max_steps:
                s.step()
                st += 1
                ok, f = s.check()
                x = s.state()[2]
                if ok:
                    break
            if ok:
                f = f + oracle.fitness(p.fk_mode, seeds[q], gparams[q], x[active])[1][0]
            sol[q, i], fit[q, i], suc[q, i], steps[q, i] = x, f, int(ok), st
    _island_cache[key] = (sol, fit, suc, steps)
    return _island_cache[key]


def distance(a, b, active):
    return np.abs(a[active] - b[active]).max()


def ranked(isl, seeds, active, k, min_distance):
    """the order and the greedy distance rule on the per-island results -> (solutions [n][k][V], fitness, success, steps, count)"""
    sol, fit, suc, steps = isl
    n, islands, V = sol.shape
    o_sol = np.repeat(seeds[:, None, :], k, axis=1).copy()
    o_fit = np.full((n, k), np.inf)
    o_suc = np.zeros((n, k), dtype=np.int32)
    o_steps = np.zeros((n, k), dtype=np.int32)
    count = np.zeros(n, dtype=np.int32)
    for q in range(n):
        order = sorted(range(islands), key=lambda i: (0 if suc[q, i] else 1, fit[q, i], i))
        kept = []
        for i in order:
            if min_distance < 0 or all(distance(sol[q, i], sol[q, j], active) > min_distance for j in kept):
                kept.append(i)
        kept = kept[:k]
        count[q] = len(kept)
        for r, i in enumerate(kept):
            o_sol[q, r], o_fit[q, r], o_suc[q, r], o_steps[q, r] = sol[q, i], fit[q, i], suc[q, i], steps[q, i]
    return o_sol, o_fit, o_suc, o_steps, count


def same(got, want, what):
    for name, x, y in zip(NAMES, got, want):
        assert x.shape == y.shape and np.array_equal(x, y), "%s: %s differ" % (what, name)


def queries(ctx, cfg, h, n, seed):
    return make_queries(ctx.templates[cfg], h.active_variables, h.fk_genes, n, seed=seed)[:2]


def met_at_seed(ctx, cfg, h, n, seed):
    """queries whose goal is already met at the seed (the goal pose IS the seed's pose): with max_steps = 1 every island ends where it began -- equal
    solutions, equal fitness bits"""
    seeds, gparams = queries(ctx, cfg, h, n, seed)
    gparams = gparams.copy()
    gparams[:, :7] = ctx.oracles[cfg].fk(seeds)[:, 0, :]
    return seeds, gparams


C2 = dict(population=128, islands=8, max_steps=3, random_seed=7)


# ---- 1: rank 0 is the existing answer --------------------------------------------------------------------------------------------------------------------
RANK0 = {
    "c2": ("c2", 24, dict(population=128, islands=8, max_steps=2, random_seed=7)),
    "c3": ("c3", 6, dict(population=128, islands=4, max_steps=2, random_seed=8)),
    "c4": ("c4", 6, dict(population=128, islands=4, max_steps=2, random_seed=9)),
    "c2_linear": ("c2", 24, dict(population=16, islands=8, max_steps=3, random_seed=10, fk_mode=abi.FK_LINEAR)),
    "c2_gd_c": ("c2", 24, dict(population=16, islands=8, max_steps=6, random_seed=11, mode="gd_c")),
}


def r1_rank0(ctx, name):
    cfg, n, kw = RANK0[name]
    h = ctx.make_solver(ctx.templates[cfg])
    seeds, gparams = queries(ctx, cfg, h, n, 41)
    want = h.solve_batch(abi.default_solve_params(island_sync=0, **kw), seeds, gparams)
    for k in (1, kw["islands"]):
        got = h.solve_batch_ranked(abi.default_solve_params(**kw), seeds, gparams, k, -1.0)
        assert np.array_equal(got[4], np.full(n, k))
        for nm, x, y in zip(NAMES, got[:4], want):
            assert np.array_equal(x[:, 0], y), "%s k=%d: row 0 of %s is not bioik_solve_batch's" % (name, k, nm)
    h.close()


# ---- 2: every island, in order -----------------------------------------------------------------------------------------------------------------------------
def r2_every_island(ctx, cfg="c2", n=6, kw=C2):
    h = ctx.make_solver(ctx.templates[cfg])
    o = ctx.oracles[cfg]
    seeds, gparams = queries(ctx, cfg, h, n, 42)
    isl = island_results(o, kw, seeds, gparams)
    # (the expectation itself: its best island is the oracle's own best-of over the islands)
    best = o.solve_batch(abi.default_solve_params(**kw), orc.RNG_COUNTER, seeds, gparams, n_threads=4)
    want = ranked(isl, seeds, h.active_variables, kw["islands"], -1.0)
    for x, y in zip(want[:4], best):
        assert np.array_equal(x[:, 0], y)
    got = h.solve_batch_ranked(abi.default_solve_params(**kw), seeds, gparams, kw["islands"], -1.0)
    assert np.array_equal(got[4], np.full(n, kw["islands"]))
    same(got, want, "every island of " + cfg)
    h.close()


def r2_ties(ctx, cfg="c2"):
    """equal fitness bits (max_steps = 1 on a goal already met) go to the lower island"""
    kw = dict(population=16, islands=4, max_steps=1, random_seed=12)
    h = ctx.make_solver(ctx.templates[cfg])
    seeds, gparams = met_at_seed(ctx, cfg, h, 3, 43)
    isl = island_results(ctx.oracles[cfg], kw, seeds, gparams)
    assert all(len(set(isl[1][q].tolist())) < 4 for q in range(3)), "precondition: islands with equal fitness"
    got = h.solve_batch_ranked(abi.default_solve_params(**kw), seeds, gparams, 4, -1.0)
    same(got, ranked(isl, seeds, h.active_variables, 4, -1.0), "ties")
    h.close()
    return isl, seeds, gparams, kw


# ---- 3: distinctness ---------------------------------------------------------------------------------------------------------------------------------------
def r3_distinct(ctx, cfg="c2", n=6, kw=C2):
    h = ctx.make_solver(ctx.templates[cfg])
    seeds, gparams = queries(ctx, cfg, h, n, 42)
    isl = island_results(ctx.oracles[cfg], kw, seeds, gparams)
    act, islands = h.active_variables, kw["islands"]
    md = float(np.median([distance(isl[0][q, i], isl[0][q, j], act) for q in range(n) for i in range(islands) for j in range(i)]))
    full = ranked(isl, seeds, act, islands, md)
    assert (full[4] < islands).any() and (full[4] >= 2).any(), "precondition: rows both kept and dropped"
    for k in (islands, 3, 1):
        got = h.solve_batch_ranked(abi.default_solve_params(**kw), seeds, gparams, k, md)
        same(got, ranked(isl, seeds, act, k, md), "min_distance %r, k %d" % (md, k))
    h.close()


def r3_equal_rows(ctx, cfg="c2"):
    """min_distance = 0 drops rows equal in every active variable: islands forced equal keep one"""
    kw = dict(population=16, islands=2, max_steps=1, random_seed=12)
    h = ctx.make_solver(ctx.templates[cfg])
    seeds, gparams = met_at_seed(ctx, cfg, h, 3, 43)
    isl = island_results(ctx.oracles[cfg], kw, seeds, gparams)
    act = np.asarray(h.active_variables)
    assert all(np.array_equal(isl[0][q, 0][act], isl[0][q, 1][act]) for q in range(3)), "precondition: two equal islands"
    got = h.solve_batch_ranked(abi.default_solve_params(**kw), seeds, gparams, 2, 0.0)
    assert np.array_equal(got[4], np.ones(3))
    same(got, ranked(isl, seeds, act, 2, 0.0), "min_distance 0")
    h.close()


# ---- 4: paths ----------------------------------------------------------------------------------------------------------------------------------------------
def r4_paths(ctx, cfg="c2"):
    kw = dict(population=16, islands=4, max_steps=3, random_seed=13)
    n, k, md = 20, 3, 0.3
    h = ctx.make_solver(ctx.templates[cfg])
    seeds, gparams = queries(ctx, cfg, h, n, 44)
    plain = h.solve_batch_ranked(abi.default_solve_params(**kw), seeds, gparams, k, md)
    want = ranked(island_results(ctx.oracles[cfg], kw, seeds[:4], gparams[:4]), seeds[:4], h.active_variables, k, md)
    same([x[:4] for x in plain], want, "paths: the plain call against the oracle")
    for steps in ("1", "1,2"):  # hand-overs
        with ctx.env(BIOIK_SOLVE_TWO_PHASE=steps):
            same(h.solve_batch_ranked(abi.default_solve_params(**kw), seeds, gparams, k, md), plain, "hand-overs after " + steps)
    with ctx.env(BIOIK_SOLVE_DRAIN_TEST="3"):  # the latency drain's hand-overs
        same(h.solve_batch_ranked(abi.default_solve_params(**kw), seeds, gparams, k, md), plain, "drain")
    same(h.solve_batch_ranked(abi.default_solve_params(timeout=3600.0, **kw), seeds, gparams, k, md), plain, "a far timeout")
    # shards against the whole batch
    parts = []
    for a, b in ((0, 7), (7, 20)):
        h.set_first_query(a)
        parts.append(h.solve_batch_ranked(abi.default_solve_params(**kw), seeds[a:b], gparams[a:b], k, md))
    h.set_first_query(0)
    same([np.concatenate(x) for x in zip(*parts)], plain, "set_first_query shards")
    # plain solves in flight on other streams of the handle
    p1 = abi.default_solve_params(**kw)
    alone = h.solve_batch(p1, seeds, gparams)
    with ctx.dev.overlap(ctx.dev.overlap_seeds[0]):
        t1 = h.submit_batch(p1, seeds, gparams)
        t2 = h.submit_batch(p1, seeds, gparams)
        got = h.solve_batch_ranked(abi.default_solve_params(**kw), seeds, gparams, k, md)
        o1, o2 = h.wait_batch(t1), h.wait_batch(t2)
    same(got, plain, "with plain solves in flight")
    for o in (o1, o2):
        assert all(np.array_equal(x, y) for x, y in zip(o, alone))
    # BIOIK_ISLANDS_AUTO = max(k, resolved), island_sync off
    auto = dict(kw, islands=0)
    for kk, nn in ((2, 20), (6, 1200)):
        resolved = h.resolve_islands(abi.default_solve_params(**auto), nn)[0]
        s2, g2 = (seeds, gparams) if nn == n else queries(ctx, cfg, h, nn, 45)
        a1 = dict(kw, max_steps=1) if nn != n else kw
        got = h.solve_batch_ranked(abi.default_solve_params(**dict(a1, islands=0)), s2, g2, kk, md)
        same(got, h.solve_batch_ranked(abi.default_solve_params(**dict(a1, islands=max(kk, resolved))), s2, g2, kk, md), "BIOIK_ISLANDS_AUTO")
        assert nn == n or resolved < kk
    h.close()


# ---- 5: one handle, one stream, mixed ----------------------------------------------------------------------------------------------------------------------
class DeviceIO:
    """device buffers of one call (plain: k = 0)"""

    def __init__(self, ctx, h, seeds, gparams, k):
        n, b = seeds.shape[0], ctx.dev.buf
        self.n, self.k = n, k
        self.ins = (b(np.ascontiguousarray(seeds)), b(np.ascontiguousarray(gparams)))
        shape = (n, k) if k else (n,)
        self.outs = [b(np.zeros(shape + (h.V,))), b(np.zeros(shape)), b(np.zeros(shape, dtype=np.int32)), b(np.zeros(shape, dtype=np.int32))]
        if k:
            self.outs.append(b(np.zeros(n, dtype=np.int32)))

    def zero(self):
        for o in self.outs:
            o.zero()

    def get(self):
        return tuple(o.get() for o in self.outs)


def enqueue(ctx, h, io, kw, s, md=-1.0):
    p = abi.default_solve_params(**kw)
    ptrs = [x.ptr for x in io.ins + tuple(io.outs)]
    with ctx.dev.on(s):
        if io.k:
            h.solve_batch_ranked_device(p, io.n, io.k, md, *ptrs, ctx.dev.handle(s))
        else:
            h.solve_batch_device(p, io.n, *ptrs, ctx.dev.handle(s))


def r5_mixed(ctx, cfg="c2"):
    """a fused-islands plain call, a ranked call of another size and island count, the plain call again: the control words' resting state and the scratch sizing"""
    plain_kw = dict(population=16, islands=2, max_steps=2, random_seed=14)
    ranked_kw = dict(population=16, islands=12, max_steps=2, random_seed=15)
    n_a, n_b, k, md = 300, 9, 5, 0.2
    f = ctx.make_solver(ctx.templates[cfg])
    sa, ga = queries(ctx, cfg, f, n_a, 46)
    sb, gb = queries(ctx, cfg, f, n_b, 47)
    want_a = f.solve_batch(abi.default_solve_params(**plain_kw), sa, ga)
    f.close()
    f = ctx.make_solver(ctx.templates[cfg])
    want_b = f.solve_batch_ranked(abi.default_solve_params(**ranked_kw), sb, gb, k, md)
    f.close()
    same([x[:2] for x in want_b], ranked(island_results(ctx.oracles[cfg], ranked_kw, sb[:2], gb[:2]), sb[:2], f.active_variables, k, md), "mixed: the oracle")
    h = ctx.make_solver(ctx.templates[cfg])
    s = ctx.dev.stream(1)
    io_a, io_b = DeviceIO(ctx, h, sa, ga, 0), DeviceIO(ctx, h, sb, gb, k)
    for io, kw, want in ((io_a, plain_kw, want_a), (io_b, ranked_kw, want_b), (io_a, plain_kw, want_a), (io_b, ranked_kw, want_b)):
        io.zero()
        ctx.dev.sync()
        enqueue(ctx, h, io, kw, s, md)
        ctx.dev.sync()
        for nm, x, y in zip(NAMES, io.get(), want):
            assert np.array_equal(x, y), "mixed calls on one handle and stream: %s differ from a fresh handle's" % nm
    h.close()


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------------------------
def r6_refusals(ctx, cfg="c2"):
    import ctypes as C
    h = ctx.make_solver(ctx.templates[cfg])
    seeds, gparams = queries(ctx, cfg, h, 2, 48)
    base = dict(population=16, max_steps=1, random_seed=1)
    for k, kw in ((0, dict(islands=4)), (5, dict(islands=4)), (2, dict(islands=65)), (2, dict(islands=4, island_sync=1)), (65, dict(islands=0)), (-1, dict(islands=4))):
        kk = max(k, 1)
        outs = [np.full((2, kk, h.V), 7.0), np.full((2, kk), 7.0), np.full((2, kk), 7, dtype=np.int32), np.full((2, kk), 7, dtype=np.int32), np.full(2, 7, dtype=np.int32)]
        p = abi.default_solve_params(**dict(base, **kw))
        d, i = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
        rc = h.L.bioik_solve_batch_ranked(h.problem, C.byref(p), 2, k, -1.0, d(seeds), d(gparams), d(outs[0]), d(outs[1]), i(outs[2]), i(outs[3]), i(outs[4]))
        assert rc == abi.ERR_INVALID_ARGUMENT, (k, kw, rc)
        assert h.L.bioik_last_error()
        assert all((o == 7).all() for o in outs), (k, kw)
    p = abi.default_solve_params(islands=4, **base)
    outs = [np.full((2, 2, h.V), 7.0), np.full((2, 2), 7.0), np.full((2, 2), 7, dtype=np.int32), np.full((2, 2), 7, dtype=np.int32)]
    rc = h.L.bioik_solve_batch_ranked(h.problem, C.byref(p), 2, 2, -1.0, d(seeds), d(gparams), d(outs[0]), d(outs[1]), i(outs[2]), i(outs[3]), None)
    assert rc == abi.ERR_INVALID_ARGUMENT and all((o == 7).all() for o in outs)
    rc = h.L.bioik_solve_batch_ranked_device(h.problem, C.byref(p), 2, 2, -1.0, seeds.ctypes.data, gparams.ctypes.data, outs[0].ctypes.data, outs[1].ctypes.data,
                                             outs[2].ctypes.data, outs[3].ctypes.data, None, None)
    assert rc == abi.ERR_INVALID_ARGUMENT
    h.close()


def r6_unsupported(ctx, make_template):
    """a problem whose solve is BIOIK_ERR_UNSUPPORTED stays so through the ranked entry"""
    t = make_template()
    h = ctx.make_solver(t)
    seeds = np.tile(t.model.default_positions(), (1, 1))
    gp = np.tile(t.pack_params(), (1, 1))
    p = abi.default_solve_params(population=16, max_steps=1, islands=2)
    codes = []
    for call in (lambda: h.solve_batch(p, seeds, gp), lambda: h.solve_batch_ranked(p, seeds, gp, 2)):
        try:
            call()
            codes.append(abi.OK)
        except BioIKError as e:
            codes.append(e.code)
    assert codes == [abi.ERR_UNSUPPORTED, abi.ERR_UNSUPPORTED], codes
    h.close()


# ---- 7 (GPU): the device-pointer entry, captured ------------------------------------------------------------------------------------------------------------
def r7_device_and_graph(ctx, cfg="c2"):
    kw = dict(population=128, islands=8, max_steps=3, random_seed=16)
    plain_kw = dict(population=128, islands=4, max_steps=2, random_seed=17)
    n, k, md = 12, 4, 0.2
    h = ctx.make_solver(ctx.templates[cfg])
    seeds, gparams = queries(ctx, cfg, h, n, 49)
    want = h.solve_batch_ranked(abi.default_solve_params(**kw), seeds, gparams, k, md)
    want_plain = h.solve_batch(abi.default_solve_params(**plain_kw), seeds, gparams)
    s = ctx.dev.stream(2)
    io, io_p = DeviceIO(ctx, h, seeds, gparams, k), DeviceIO(ctx, h, seeds, gparams, 0)
    enqueue(ctx, h, io, kw, s, md)  # (the eager call of the same plan)
    ctx.dev.sync()
    same(io.get(), want, "the device-pointer entry")
    g = ctx.dev.capture(s, lambda: enqueue(ctx, h, io, kw, s, md))
    try:
        for r in range(4):
            io.zero()
            ctx.dev.sync()
            ctx.dev.replay(g)
            ctx.dev.sync()
            same(io.get(), want, "replay %d" % r)
            io_p.zero()
            enqueue(ctx, h, io_p, plain_kw, s)
            ctx.dev.sync()
            assert all(np.array_equal(x, y) for x, y in zip(io_p.get(), want_plain))
    finally:
        ctx.dev.destroy(g)
    h.close()


# ---- 8: result level ---------------------------------------------------------------------------------------------------------------------------------------
def r8_results(ctx, n, cfg="c2", seed=50):
    kw = dict(population=128, islands=16, max_steps=64, random_seed=18)
    k, md = 8, 0.1
    h = ctx.make_solver(ctx.templates[cfg])
    o = ctx.oracles[cfg]
    seeds, gparams = queries(ctx, cfg, h, n, seed)
    sol, fit, suc, steps, count = h.solve_batch_ranked(abi.default_solve_params(**kw), seeds, gparams, k, md)
    act = np.asarray(h.active_variables)
    model = ctx.templates[cfg].model
    act_b = act[np.asarray(model.var_bounded)[act] != 0]  # (continuous joints have no limits: var_min / var_max only say where to draw them from)
    lo, hi = np.asarray(model.var_min)[act_b], np.asarray(model.var_max)[act_b]
    several = 0
    for q in range(n):
        assert (suc[q, count[q]:] == 0).all() and np.isinf(fit[q, count[q]:]).all()
        ok = np.nonzero(suc[q])[0]
        several += len(ok) >= 2
        if len(ok):
            tips = o.fk(sol[q, ok])
            for r, t in zip(ok, tips):
                assert np.linalg.norm(t[0, :3] - gparams[q, :3]) < 1e-4
                assert 2 * np.arccos(min(1.0, abs(float(t[0, 3:] @ gparams[q, 3:7])))) < 1e-3
                assert (sol[q, r][act_b] >= lo).all() and (sol[q, r][act_b] <= hi).all()
                for j in range(count[q]):
                    assert j == r or distance(sol[q, r], sol[q, j], act) > md
    assert several >= 1, "no query returned two or more successes"
    h.close()
    return several
