"""round 6: the latency of ONE pose per plugin call (bioik_plugin_search_each), call by call: mean, percentiles, and where the slow calls are -- their indices and times.
usage: python tools/one_pose_probe.py [timeout_ms] [calls] [arm|arm_md|all|snake] [gpu_islands] [gpu_population] [gpu_max_steps] [exact|linear] [gpu_island_migration]
timeout_ms and gpu_island_migration may be comma-separated lists (island migration: every E under every timeout, one pass each, and -- through the C-ABI, one pose
per call with the plugin's parameters and the longest timeout -- the mean number of steps of the poses that succeed)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bio_ik_amd import abi  # noqa: E402
from bio_ik_amd import AvoidJointLimitsGoal, MinimalDisplacementGoal, PoseGoal, ProblemTemplate, pr2_like, snake  # noqa: E402
from bio_ik_amd.goals import BioIKKinematicsQueryOptions  # noqa: E402
from bio_ik_amd.plugin import BioIKKinematicsPlugin  # noqa: E402
from bio_ik_amd.solver import HipSolver  # noqa: E402
from bio_ik_amd.workload import make_queries  # noqa: E402


def main():
    timeouts = [float(x) * 1e-3 for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [0.005]
    migrations = [int(x) for x in sys.argv[8].split(",")] if len(sys.argv) > 8 else None
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    which = sys.argv[3] if len(sys.argv) > 3 else "arm"
    islands = int(sys.argv[4]) if len(sys.argv) > 4 else 0
    pop = int(sys.argv[5]) if len(sys.argv) > 5 else 128
    max_steps = int(sys.argv[6]) if len(sys.argv) > 6 else 4096
    fk = sys.argv[7] if len(sys.argv) > 7 else "exact"
    model, group, tips, extra = {"arm": (pr2_like(), "right_arm", ["r_wrist_roll_link"], []),
                                 "arm_md": (pr2_like(), "right_arm", ["r_wrist_roll_link"], [MinimalDisplacementGoal()]),
                                 "all": (pr2_like(), "all", ["r_wrist_roll_link", "l_wrist_roll_link"], [MinimalDisplacementGoal()]),
                                 "snake": (snake(31), "snake", ["tip"], [AvoidJointLimitsGoal()])}[which]
    template = ProblemTemplate(model, group, [PoseGoal(t) for t in tips] + extra)
    h = HipSolver(template, device=0)
    seeds, params, _ = make_queries(template, h.active_variables, h.fk_genes, n, seed=0x0E905E)
    plug = BioIKKinematicsPlugin()
    plug.initialize(model, group, model.link_names[0], tips, params={"random_seed": 1, "gpu_max_steps": max_steps, "gpu_islands": islands, "gpu_population": pop, "gpu_fk": fk})
    gv = plug._group_vars
    poses = np.stack([params[:, 8 * t:8 * t + 7] for t in range(len(tips))], axis=1)
    opts = BioIKKinematicsQueryOptions()
    opts.goals = list(extra)
    plug.searchPositionIKEach(poses[:8], seeds[:8, gv], opts, timeout=0.02)
    print("%s, gpu_islands %d, gpu_population %d, gpu_max_steps %d, gpu_fk %s" % (which, islands, pop, max_steps, fk))
    for e in migrations or [None]:
        if e is not None:
            plug.params["gpu_island_migration"] = e
            plug.searchPositionIKEach(poses[:8], seeds[:8, gv], opts, timeout=0.02)
        for timeout in timeouts:
            for rep in range(2 if e is None else 1):
                _, ok, _, sec = plug.searchPositionIKEach(poses, seeds[:, gv], opts, timeout=timeout)
                order = np.argsort(sec)[::-1][:8]
                print("%stimeout %.1f ms: success %.4f mean %.3f ms median %.3f p90 %.3f p99 %.3f max %.3f | slowest calls (index: ms): %s" % (
                    "" if e is None else "gpu_island_migration %d, " % e, 1e3 * timeout, ok.mean(), 1e3 * sec.mean(), 1e3 * np.median(sec), 1e3 * np.quantile(sec, 0.9),
                    1e3 * np.quantile(sec, 0.99), 1e3 * sec.max(), ", ".join("%d: %.2f" % (i, 1e3 * sec[i]) for i in order)), flush=True)
        if e is not None:  # the plugin does not hand out step counts: the same poses through the C-ABI, one per call
            sp = abi.default_solve_params(population=pop, islands=islands, island_sync=1 if islands != 1 else 0, max_steps=max_steps, random_seed=1,
                                          fk_mode=abi.FK_LINEAR if fk == "linear" else abi.FK_EXACT, timeout=max(timeouts), island_migration=e)
            steps = []
            for i in range(n):
                h.set_first_query(i)
                _, _, suc, st = h.solve_batch(sp, seeds[i:i + 1], params[i:i + 1])
                if suc[0]:
                    steps.append(int(st[0]))
            print("gpu_island_migration %d, C-ABI, one pose per call, timeout %.1f ms: %d of %d succeed, mean steps to success %.2f, median %.1f" % (
                e, 1e3 * max(timeouts), len(steps), n, np.mean(steps) if steps else float("nan"), np.median(steps) if steps else float("nan")), flush=True)


if __name__ == "__main__":
    main()
