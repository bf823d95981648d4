"""ctypes binding of the HIP solver library (include/bioik_hip.h) — the product compute path.

`HipSolver` owns one (model, problem template) pair on one MI355X and exposes the batched solve plus the
function-level entry points.  There is no CPU path: if `libbioik_hip.so` is missing, or no HIP device is visible,
construction raises (`bioik_model_create` -> BIOIK_ERR_NO_DEVICE).  Host arrays are NumPy; the `*_device` methods take
raw device pointers (e.g. `torch.Tensor.data_ptr()` of CUDA tensors) and a HIP stream handle.
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbioik_hip.so")
_lib = None

_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int32)

EXPORTS = [
    "bioik_goal_param_count", "bioik_default_solve_params", "bioik_last_error", "bioik_abi_version", "bioik_device_count",
    "bioik_model_create", "bioik_model_destroy", "bioik_problem_create", "bioik_problem_destroy",
    "bioik_problem_active_variable_count", "bioik_problem_active_variables", "bioik_problem_tip_count", "bioik_problem_tip_links",
    "bioik_problem_param_count", "bioik_problem_variable_count", "bioik_problem_set_first_query", "bioik_solve_batch", "bioik_solve_batch_multi",
    "bioik_solve_batch_device", "bioik_eval_fk", "bioik_eval_fitness", "bioik_eval_approximator", "bioik_eval_reproduce",
    "bioik_eval_check", "bioik_stream_fitness_device", "bioik_solve_batch_submit", "bioik_solve_batch_wait", "bioik_debug_reload_switches", "bioik_eval_arith",
    "bioik_resolve_islands", "bioik_solve_batch_ranked", "bioik_solve_batch_ranked_device", "bioik_sincos_domain", "bioik_sincos_small_bound",
    "bioik_problem_carry_doubles", "bioik_eval_migrate",
    "bioik_solve_batch_bounded", "bioik_solve_batch_bounded_submit", "bioik_solve_batch_bounded_device", "bioik_eval_bounds",
    "bioik_problem_op_count", "bioik_problem_op_variables",
    "bioik_problem_set_obstacles", "bioik_problem_obstacle_count",
]


class BioIKError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bioik status %d: %s" % (code, msg))
        self.code = code


def _declare(L):
    L.bioik_last_error.restype = C.c_char_p
    L.bioik_model_create.argtypes = [C.POINTER(abi.ModelDesc), C.c_int, C.POINTER(C.c_void_p)]
    L.bioik_model_destroy.argtypes = [C.c_void_p]
    L.bioik_model_destroy.restype = None
    L.bioik_problem_create.argtypes = [C.c_void_p, C.POINTER(abi.ProblemDesc), C.POINTER(C.c_void_p)]
    L.bioik_problem_destroy.argtypes = [C.c_void_p]
    L.bioik_problem_destroy.restype = None
    for f in ("bioik_problem_active_variable_count", "bioik_problem_tip_count", "bioik_problem_param_count", "bioik_problem_variable_count"):
        getattr(L, f).argtypes = [C.c_void_p]
    L.bioik_problem_active_variables.argtypes = [C.c_void_p, _pi]
    L.bioik_problem_tip_links.argtypes = [C.c_void_p, _pi]
    L.bioik_problem_set_first_query.argtypes = [C.c_void_p, C.c_uint64]
    L.bioik_default_solve_params.argtypes = [C.POINTER(abi.SolveParams)]
    L.bioik_default_solve_params.restype = None
    L.bioik_solve_batch.argtypes = [C.c_void_p, C.POINTER(abi.SolveParams), C.c_size_t, _pd, _pd, _pd, _pd, _pi, _pi]
    L.bioik_solve_batch_submit.argtypes = [C.c_void_p, C.POINTER(abi.SolveParams), C.c_size_t, _pd, _pd, _pd, _pd, _pi, _pi, C.POINTER(C.c_uint64)]
    L.bioik_solve_batch_wait.argtypes = [C.c_void_p, C.c_uint64]
    L.bioik_solve_batch_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(abi.SolveParams), C.c_size_t, _pd, _pd, _pd, _pd, _pi, _pi]
    L.bioik_solve_batch_device.argtypes = [C.c_void_p, C.POINTER(abi.SolveParams), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    L.bioik_eval_fk.argtypes = [C.c_void_p, C.c_size_t, _pd, _pd, _pd]
    L.bioik_eval_fitness.argtypes = [C.c_void_p, C.c_int, C.c_size_t, _pd, _pd, _pd, _pd, _pd, _pd]
    L.bioik_eval_approximator.argtypes = [C.c_void_p, _pd, _pd, _pd, _pd]
    L.bioik_eval_reproduce.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_uint32, _pd, _pd, _pd]
    L.bioik_eval_check.argtypes = [C.c_void_p, C.POINTER(abi.SolveParams), C.c_size_t, _pd, _pd, _pd, _pi]
    if hasattr(L, "bioik_eval_arith"):
        L.bioik_eval_arith.argtypes = [C.c_int, C.c_int, C.c_size_t, _pd, _pd]
    L.bioik_stream_fitness_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bioik_problem_carry_doubles.argtypes = [C.c_void_p]
    L.bioik_eval_migrate.argtypes = [C.c_void_p, C.c_int32, C.c_size_t, _pi, _pd]
    L.bioik_resolve_islands.argtypes = [C.c_void_p, C.POINTER(abi.SolveParams), C.c_size_t, _pi, _pi]
    L.bioik_solve_batch_ranked.argtypes = [C.c_void_p, C.POINTER(abi.SolveParams), C.c_size_t, C.c_int32, C.c_double, _pd, _pd, _pd, _pd, _pi, _pi, _pi]
    L.bioik_solve_batch_ranked_device.argtypes = [C.c_void_p, C.POINTER(abi.SolveParams), C.c_size_t, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bioik_solve_batch_bounded.argtypes = [C.c_void_p, C.POINTER(abi.SolveParams), C.c_size_t, _pd, _pd, _pd, _pd, _pd, _pd, _pi, _pi]
    L.bioik_solve_batch_bounded_submit.argtypes = [C.c_void_p, C.POINTER(abi.SolveParams), C.c_size_t, _pd, _pd, _pd, _pd, _pd, _pd, _pi, _pi, C.POINTER(C.c_uint64)]
    L.bioik_solve_batch_bounded_device.argtypes = [C.c_void_p, C.POINTER(abi.SolveParams), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bioik_eval_bounds.argtypes = [C.c_void_p, C.c_size_t, _pd, _pd, _pd]
    L.bioik_problem_op_count.argtypes = [C.c_void_p]
    L.bioik_problem_op_variables.argtypes = [C.c_void_p, _pi, _pi]
    if hasattr(L, "bioik_problem_set_obstacles"):  # (BIOIK_HIP_LIBRARY may name an earlier build of ABI 6 for an A/B run: it has no ClearanceGoal)
        L.bioik_problem_set_obstacles.argtypes = [C.c_void_p, C.c_int, C.c_size_t, _pd]
        L.bioik_problem_obstacle_count.argtypes = [C.c_void_p, C.c_int]
    return L


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  Two HIP runtimes in one process cannot both
    open the GPU, so when torch is installed but not imported yet, its bundled runtime is loaded first and
    libbioik_hip.so binds to it by SONAME — whichever of the two libraries is used first, they share one runtime.
    (torch itself is not imported: it only supplies device memory and streams to callers that want it.)"""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def load_library(path=None):
    """Load (once) the HIP solver library.  Raises if it has not been built: there is no fallback."""
    global _lib
    if path is not None:
        return _declare(C.CDLL(path))
    if _lib is None:
        path = os.environ.get("BIOIK_HIP_LIBRARY", LIB_PATH)  # deployment override: another build of the same library
        if path != LIB_PATH:
            _share_hip_runtime_with_torch()
            L = C.CDLL(path)
            # (the override is for other BUILDS of the product library -- A/B variants, a profiling build; the test-suite's host simulator of the kernels is
            # handed to HipSolver explicitly, `lib=`, and must never stand behind the product classes through the environment)
            if hasattr(L, "hostsim_divergent_collectives"):
                raise ImportError("BIOIK_HIP_LIBRARY names the test-suite's host simulator (%s): bio_ik_amd has no CPU compute path" % path)
            _lib = _declare(L)
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); bio_ik_amd has no CPU compute path" % LIB_PATH)
        _share_hip_runtime_with_torch()
        _lib = _declare(C.CDLL(LIB_PATH))
    return _lib


_switch_snapshot = {}


def sync_debug_switches(L):
    """The library parses its BIOIK_SOLVE_* diagnostic switches once, when it is loaded.  Tests and probes that change them inside a
    process (monkeypatch.setenv) get them re-read here, before a solve, when the environment differs from what library `L` last saw."""
    snap = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("BIOIK_SOLVE_") or k == "BIOIK_PHASE_DUMP"))
    key = id(L)
    if _switch_snapshot.get(key, ()) != snap:
        if hasattr(L, "bioik_debug_reload_switches"):
            L.bioik_debug_reload_switches()
        _switch_snapshot[key] = snap


ARITH_IN = {0: 1, 1: 7, 2: 8, 3: 6, 4: 8, 5: 22, 6: 1, 7: 2, 8: 1, 9: 1}
ARITH_OUT = {0: 2, 1: 3, 2: 4, 3: 1, 4: 1, 5: 14, 6: 1, 7: 1, 8: 2, 9: 2}


def eval_arith(op, x, device=0, lib=None):
    """bioik_eval_arith: the shared arithmetic headers on the device, one function at a time (include/bioik_hip.h)"""
    L = lib if lib is not None else load_library()
    a = _f64(x).reshape(-1, ARITH_IN[op])
    out = np.zeros((a.shape[0], ARITH_OUT[op]))
    rc = L.bioik_eval_arith(int(device), int(op), a.shape[0], _d(a), _d(out))
    if rc != abi.OK:
        raise BioIKError(rc, L.bioik_last_error().decode())
    return out


def sincos_domain(lib=None):
    """bioik_sincos_domain: BIOIK_SINCOS_DOMAIN as library `lib` was compiled with it -- where the shared sincos stops being accurate and the line search stops taking candidates"""
    L = lib if lib is not None else load_library()
    L.bioik_sincos_domain.restype = C.c_double
    return float(L.bioik_sincos_domain())


def sincos_small_bound(lib=None):
    """bioik_sincos_small_bound: BIOIK_SINCOS_SMALL as library `lib` was compiled with it -- the half angle up to which the chain walks skip the reduction and the quadrant"""
    L = lib if lib is not None else load_library()
    L.bioik_sincos_small_bound.restype = C.c_double
    return float(L.bioik_sincos_small_bound())


def device_count():
    return int(load_library().bioik_device_count())


def _d(a):
    return a.ctypes.data_as(_pd)


def _i(a):
    return a.ctypes.data_as(_pi)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class HipSolver:
    """One problem template on one GPU.  `lib` is for the test suite only (it injects the host simulator)."""

    def __init__(self, template, device=0, lib=None):
        self.L = lib if lib is not None else load_library()
        self.template = template
        self.model = C.c_void_p()
        self.problem = C.c_void_p()
        md = template.model.desc()
        self._chk(self.L.bioik_model_create(C.byref(md), int(device), C.byref(self.model)))
        pd = template.desc()
        rc = self.L.bioik_problem_create(self.model, C.byref(pd), C.byref(self.problem))
        if rc != abi.OK:
            msg = self.L.bioik_last_error().decode()
            self.L.bioik_model_destroy(self.model)
            self.model = C.c_void_p()
            raise BioIKError(rc, msg)
        self.D = self.L.bioik_problem_active_variable_count(self.problem)
        self.T = self.L.bioik_problem_tip_count(self.problem)
        self.P = self.L.bioik_problem_param_count(self.problem)
        self.V = self.L.bioik_problem_variable_count(self.problem)
        self.active_variables = np.zeros(self.D, dtype=np.int32)
        self.L.bioik_problem_active_variables(self.problem, _i(self.active_variables))
        self.tip_links = np.zeros(self.T, dtype=np.int32)
        self.L.bioik_problem_tip_links(self.problem, _i(self.tip_links))
        self.obstacles = {}
        # the obstacle tables of the template's ClearanceGoals (data of the goals, not of the descriptor): a new handle's are empty
        try:
            tables = template.obstacle_tables() if hasattr(template, "obstacle_tables") else {}
            for k, rows in tables.items():
                if len(rows):
                    self.set_obstacles(k, rows)
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "problem", None):
            self.L.bioik_problem_destroy(self.problem)
            self.problem = C.c_void_p()
        if getattr(self, "model", None):
            self.L.bioik_model_destroy(self.model)
            self.model = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != abi.OK:
            raise BioIKError(rc, self.L.bioik_last_error().decode())

    def _gp(self, goal_params, n=None):
        if n is None:
            g = _f64(goal_params).ravel() if self.P else np.zeros(1)
            if self.P and g.size != self.P:
                raise ValueError("goal_params must have %d entries" % self.P)
            return g
        return _f64(goal_params).reshape(n, self.P) if self.P else np.zeros((n, 1))

    def resolve_islands(self, params, n):
        """bioik_resolve_islands: (islands, island_sync) a solve of `n` queries with `params` runs with (BIOIK_ISLANDS_AUTO resolved for this device)"""
        isl, sync = C.c_int32(0), C.c_int32(0)
        self._chk(self.L.bioik_resolve_islands(self.problem, C.byref(params), int(n), C.byref(isl), C.byref(sync)))
        return isl.value, sync.value

    def _bounds(self, bounds, n):
        """bounds=(lo, hi), [n][V] each (or one row [V] for every query), as contiguous float64 arrays; an entry None stays None (a null pointer: the library refuses
        exactly one null)"""
        lo, hi = bounds
        out = []
        for b in (lo, hi):
            if b is None:
                out.append(None)
                continue
            b = _f64(b)
            if b.size == self.V and n != 1:
                b = np.tile(b.reshape(1, self.V), (n, 1))
            out.append(np.ascontiguousarray(b.reshape(n, self.V)))
        return out

    def eval_bounds(self, lo, hi):
        """bioik_eval_bounds: the rule of the per-query variable bounds in isolation: rows lo, hi [n][V] -> [n][max(ops, 1)][6], the columns of abi.BOUNDS_COLUMNS"""
        lo = _f64(lo).reshape(-1, self.V)
        hi = _f64(hi).reshape(-1, self.V)
        n = lo.shape[0]
        out = np.zeros((n, max(self.n_ops(), 1), 6))
        self._chk(self.L.bioik_eval_bounds(self.problem, n, _d(lo), _d(hi), _d(out)))
        return out

    def n_ops(self):
        """bioik_problem_op_count: ops of the problem's joint program"""
        return int(self.L.bioik_problem_op_count(self.problem))

    def op_variables(self):
        """bioik_problem_op_variables: per op its robot variable and its index among the active variables (-1: no gene)"""
        n = self.n_ops()
        var, gene = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self.L.bioik_problem_op_variables(self.problem, _i(var), _i(gene)))
        return var[:n], gene[:n]

    def set_obstacles(self, goal_index, spheres):
        """bioik_problem_set_obstacles: replace the obstacle table of ClearanceGoal `goal_index` (an index into the template's goals) by rows cx cy cz R.  The
        library completes this handle's submitted tickets and waits for its own streams first; device-pointer solves on the caller's streams are the caller's to
        wait for."""
        a = np.ascontiguousarray(np.array(spheres, dtype=np.float64).reshape(-1, 4))
        self._chk(self.L.bioik_problem_set_obstacles(self.problem, int(goal_index), a.shape[0], _d(a) if a.shape[0] else None))
        self.obstacles[int(goal_index)] = a  # (what the handle holds now: bio_ik_amd.batch hands it to the other ranks' handles)

    def obstacle_count(self, goal_index):
        """bioik_problem_obstacle_count: rows of the goal's obstacle table on this handle"""
        rc = self.L.bioik_problem_obstacle_count(self.problem, int(goal_index))
        if rc < 0:
            self._chk(rc)
        return int(rc)

    def set_first_query(self, first_query):
        self._chk(self.L.bioik_problem_set_first_query(self.problem, int(first_query)))

    # ---- the hot path -------------------------------------------------------------------------------------
    def solve_batch(self, params, seeds, goal_params, bounds=None):
        """n independent queries: seeds [n][V], goal_params [n][P] -> (solutions [n][V], fitness, success, steps).
        bounds=(lo, hi): per-query variable bounds, [n][V] each (bioik_solve_batch_bounded; include/bioik_hip.h: the rule)."""
        sync_debug_switches(self.L)
        s = _f64(seeds).reshape(-1, self.V)
        n = s.shape[0]
        gp = self._gp(goal_params, n)
        sol = np.zeros((n, self.V))
        fit = np.zeros(n)
        suc = np.zeros(n, dtype=np.int32)
        steps = np.zeros(n, dtype=np.int32)
        if bounds is not None:
            lo, hi = self._bounds(bounds, n)
            self._chk(self.L.bioik_solve_batch_bounded(self.problem, C.byref(params), n, _d(s), _d(gp), _d(lo) if lo is not None else None, _d(hi) if hi is not None else None,
                                                       _d(sol), _d(fit), _i(suc), _i(steps)))
            return sol, fit, suc, steps
        self._chk(self.L.bioik_solve_batch(self.problem, C.byref(params), n, _d(s), _d(gp), _d(sol), _d(fit), _i(suc), _i(steps)))
        return sol, fit, suc, steps

    def solve_batch_ranked(self, params, seeds, goal_params, k, min_distance=-1.0):
        """bioik_solve_batch_ranked: the k best distinct islands of every query, ranked (include/bioik_hip.h: order, distance, fill) ->
        (solutions [n][k][V], fitness [n][k], success [n][k], steps [n][k], count [n])."""
        sync_debug_switches(self.L)
        s = _f64(seeds).reshape(-1, self.V)
        n, k = s.shape[0], int(k)
        gp = self._gp(goal_params, n)
        kk = max(k, 0)
        sol = np.zeros((n, kk, self.V))
        fit = np.zeros((n, kk))
        suc = np.zeros((n, kk), dtype=np.int32)
        steps = np.zeros((n, kk), dtype=np.int32)
        count = np.zeros(n, dtype=np.int32)
        self._chk(self.L.bioik_solve_batch_ranked(self.problem, C.byref(params), n, k, float(min_distance), _d(s), _d(gp), _d(sol), _d(fit), _i(suc), _i(steps),
                                                  _i(count)))
        return sol, fit, suc, steps, count

    def solve_batch_ranked_device(self, params, n, k, min_distance, d_seeds, d_goal_params, d_solutions, d_fitness, d_success, d_steps, d_count, stream=0):
        """The ranked solve on device pointers (ints): enqueues on `stream`, does not synchronise."""
        sync_debug_switches(self.L)
        self._chk(self.L.bioik_solve_batch_ranked_device(self.problem, C.byref(params), int(n), int(k), float(min_distance), d_seeds, d_goal_params, d_solutions,
                                                         d_fitness, d_success, d_steps, d_count, stream))

    def submit_batch(self, params, seeds, goal_params, bounds=None):
        """bioik_solve_batch_submit: the same solve without waiting.  Returns a ticket object; `wait_batch(ticket)` returns what solve_batch
        returns.  Up to six batches of this handle are in flight together (the library rotates over six internal streams)."""
        sync_debug_switches(self.L)
        s = _f64(seeds).reshape(-1, self.V)
        n = s.shape[0]
        gp = self._gp(goal_params, n)
        out = (np.zeros((n, self.V)), np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
        t = C.c_uint64(0)
        if bounds is not None:
            lo, hi = self._bounds(bounds, n)
            self._chk(self.L.bioik_solve_batch_bounded_submit(self.problem, C.byref(params), n, _d(s), _d(gp), _d(lo) if lo is not None else None,
                                                              _d(hi) if hi is not None else None, _d(out[0]), _d(out[1]), _i(out[2]), _i(out[3]), C.byref(t)))
            return (t.value, out, (s, gp, lo, hi))
        self._chk(self.L.bioik_solve_batch_submit(self.problem, C.byref(params), n, _d(s), _d(gp), _d(out[0]), _d(out[1]), _i(out[2]), _i(out[3]), C.byref(t)))
        return (t.value, out, (s, gp))  # (the arrays stay alive with the ticket)

    def wait_batch(self, ticket):
        self._chk(self.L.bioik_solve_batch_wait(self.problem, C.c_uint64(ticket[0])))
        return ticket[1]

    def solve_batch_multi(self, others, params, seeds, goal_params):
        """One batch over this handle and `others` (HipSolver objects of the same template, e.g. one per GPU): contiguous shards, one host
        thread and stream per handle inside the library (bioik_solve_batch_multi); equals solve_batch on one handle bit for bit."""
        sync_debug_switches(self.L)
        s = _f64(seeds).reshape(-1, self.V)
        n = s.shape[0]
        gp = self._gp(goal_params, n)
        sol = np.zeros((n, self.V))
        fit = np.zeros(n)
        suc = np.zeros(n, dtype=np.int32)
        steps = np.zeros(n, dtype=np.int32)
        handles = (C.c_void_p * (1 + len(others)))(self.problem, *[o.problem for o in others])
        self._chk(self.L.bioik_solve_batch_multi(handles, 1 + len(others), C.byref(params), n, _d(s), _d(gp), _d(sol), _d(fit), _i(suc), _i(steps)))
        return sol, fit, suc, steps

    def solve_batch_device(self, params, n, d_seeds, d_goal_params, d_solutions, d_fitness, d_success, d_steps, stream=0, bounds=None):
        """All arguments are device pointers (ints) of arrays resident in HBM; enqueues on `stream`, does not synchronise.
        bounds=(d_lo, d_hi): device pointers of the per-query variable bounds, [n][V] each; they must stay valid and unchanged until the call's kernels have run."""
        sync_debug_switches(self.L)
        if bounds is not None:
            self._chk(self.L.bioik_solve_batch_bounded_device(self.problem, C.byref(params), int(n), d_seeds, d_goal_params, bounds[0], bounds[1], d_solutions, d_fitness,
                                                              d_success, d_steps, stream))
            return
        self._chk(self.L.bioik_solve_batch_device(self.problem, C.byref(params), int(n), d_seeds, d_goal_params, d_solutions, d_fitness,
                                                  d_success, d_steps, stream))

    def stream_fitness_device(self, n_units, population, d_seeds, d_goal_params, d_genes, d_fitness, stream=0):
        self._chk(self.L.bioik_stream_fitness_device(self.problem, int(n_units), int(population), d_seeds, d_goal_params, d_genes, d_fitness, stream))

    # ---- function-level entry points -----------------------------------------------------------------------
    def fk_genes(self, seed, genes):
        g = _f64(genes).reshape(-1, self.D)
        tips = np.zeros((g.shape[0], self.T, 7))
        self._chk(self.L.bioik_eval_fk(self.problem, g.shape[0], _d(_f64(seed)), _d(g), _d(tips)))
        return tips

    def fk(self, vars_):
        """exact FK of full variable vectors (every row is its own seed)"""
        v = _f64(vars_).reshape(-1, self.V)
        return np.concatenate([self.fk_genes(row, row[self.active_variables][None, :]) for row in v], axis=0)

    def fitness(self, fk_mode, seed, goal_params, genes, base_genes=None):
        g = _f64(genes).reshape(-1, self.D)
        n = g.shape[0]
        prim, sec = np.zeros(n), np.zeros(n)
        b = _f64(base_genes) if base_genes is not None else None
        self._chk(self.L.bioik_eval_fitness(self.problem, int(fk_mode), n, _d(_f64(seed)), _d(self._gp(goal_params)), _d(b) if b is not None else None,
                                            _d(g), _d(prim), _d(sec)))
        return prim, sec

    def approximator(self, seed, base_genes):
        tips = np.zeros((self.T, 7))
        deltas = np.zeros((self.T, self.D, 7))
        self._chk(self.L.bioik_eval_approximator(self.problem, _d(_f64(seed)), _d(_f64(base_genes)), _d(tips), _d(deltas)))
        return tips, deltas

    def reproduce(self, population, rng_key, species, generation, parents):
        par = _f64(parents).reshape(2, 2, self.D)
        genes = np.zeros((population, self.D))
        grads = np.zeros((population, self.D))
        self._chk(self.L.bioik_eval_reproduce(self.problem, int(population), int(rng_key), int(species), int(generation), _d(par), _d(genes), _d(grads)))
        return genes, grads

    def carry_doubles(self):
        """bioik_problem_carry_doubles: doubles of an island's row between two launches (include/bioik_hip.h, bioik_eval_migrate: the layout)"""
        return int(self.L.bioik_problem_carry_doubles(self.problem))

    def migrate(self, live, rows):
        """bioik_eval_migrate: the island-migration rule of a boundary on rows [n][islands][carry_doubles] with live [n][islands] -> the rows after it"""
        lv = np.ascontiguousarray(live, dtype=np.int32)
        n, islands = lv.shape
        out = np.array(_f64(rows).reshape(n, islands, self.carry_doubles()), copy=True, order="C")
        self._chk(self.L.bioik_eval_migrate(self.problem, islands, n, _i(lv), _d(out)))
        return out

    def check(self, params, seed, goal_params, genes):
        g = _f64(genes).reshape(-1, self.D)
        ok = np.zeros(g.shape[0], dtype=np.int32)
        self._chk(self.L.bioik_eval_check(self.problem, C.byref(params), g.shape[0], _d(_f64(seed)), _d(self._gp(goal_params)), _d(g), _i(ok)))
        return ok
