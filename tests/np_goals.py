"""Goal costs, approximator tables, linearised frames and the success test of the reference, restated in NumPy long double from their definitions
(include/bio_ik/goal_types.h, src/problem.cpp:244-341, src/forward_kinematics.h:600-730, 1172-1233), with rotation matrices from tests/np_fk.py.  Nothing here
calls the oracle, the device's headers or the stand-in headers of the reference: it is the independent arbiter of both.

Structure that is not arithmetic -- the active variables, the tip links -- comes from the caller (`Problem`), checked elsewhere against the oracle."""
import numpy as np

from bio_ik_amd import abi
from np_fk import LD, fk_batch, quat_from_rot_batch, rot_from_quat, rot_from_quat_batch

DBL_MAX = np.finfo(np.float64).max
JOINT_SET = (abi.GOAL_AVOID_JOINT_LIMITS, abi.GOAL_CENTER_JOINTS, abi.GOAL_REGULARIZATION, abi.GOAL_MINIMAL_DISPLACEMENT, abi.GOAL_JOINT_VARIABLE)


def qrot(q, v):
    """tf2 quatRotate in its polynomial form v + 2 w (u x v) + 2 u x (u x v), u = (x, y, z): the rotation by q for a unit q, and what the reference
    computes for the unnormalised quaternions of a linearised frame.  q (n, 4), v (3,) or (n, 3)"""
    u, w = q[:, :3], q[:, 3:4]
    v = np.broadcast_to(np.asarray(v, dtype=LD), u.shape)
    t = np.cross(u, v)
    return v + 2 * (w * t + np.cross(u, t))


def _n(v):
    return v / np.sqrt(np.sum(v * v, axis=1, keepdims=True))


def link_cost(op, P, p, q):
    """the unweighted cost of one link goal (opcode op, parameters P) for frames (p (n, 3), q (n, 4)): goal_types.h, one expression per goal"""
    P = np.asarray(P, dtype=LD)
    sq = lambda a: np.sum(a * a, axis=1)  # noqa: E731
    if op == abi.GOAL_POSITION:
        return sq(p - P[:3])
    if op == abi.GOAL_ORIENTATION:
        return np.minimum(sq(P[:4] - q), sq(P[:4] + q))
    if op == abi.GOAL_POSE:
        return sq(p - P[:3]) + P[7] ** 2 * np.minimum(sq(P[3:7] - q), sq(P[3:7] + q))
    if op == abi.GOAL_LOOK_AT:
        return sq(_n(P[3:6] - p) - _n(qrot(q, P[:3])))
    if op in (abi.GOAL_MAX_DISTANCE, abi.GOAL_MIN_DISTANCE):
        d = np.sqrt(sq(p - P[:3]))
        return np.maximum(LD(0), d - P[3] if op == abi.GOAL_MAX_DISTANCE else P[3] - d) ** 2
    if op == abi.GOAL_LINE:
        d = P[3:6]
        return sq(P[:3] - (p - d[None] * ((p - P[:3]) @ d)[:, None]))
    if op == abi.GOAL_PLANE:
        return ((p - P[:3]) @ P[3:6]) ** 2
    if op == abi.GOAL_SIDE:
        return np.maximum(LD(0), qrot(q, P[:3]) @ P[3:6]) ** 2
    if op == abi.GOAL_DIRECTION:
        return sq(qrot(q, P[:3]) - P[3:6])
    if op == abi.GOAL_CONE:
        v = qrot(q, P[4:7])
        x = (v @ P[7:10]) / np.sqrt(sq(v) * (P[7:10] @ P[7:10]))
        return np.maximum(LD(0), np.arccos(np.clip(x, -1, 1)) - P[10]) ** 2 + P[3] ** 2 * sq(P[:3] - p)
    raise AssertionError(op)


class Problem:
    """what the costs need of a problem template: active variables (from the caller), the minimal-displacement factors (problem.cpp:206-225), the variables'
    bounds (a variable without limits counts in no joint-limit goal, goal_types.h:387-425, and keeps no limits in a solve)"""

    def __init__(self, template, active_variables, tip_links):
        m = self.model = template.model
        self.template = template
        self.active = np.asarray(active_variables)
        self.tips = [int(t) for t in tip_links]
        rcp = np.array([1 / LD(m.var_max_velocity[v]) if m.var_max_velocity[v] > 0 else LD(0) for v in self.active], dtype=LD)
        self.w = rcp / rcp.sum() if rcp.sum() > 0 else np.full(len(self.active), LD(1) / len(self.active), dtype=LD)
        lo, hi = np.asarray(m.var_min, dtype=LD)[self.active], np.asarray(m.var_max, dtype=LD)[self.active]
        self.mid = (lo + hi) * LD(0.5)
        span = hi - lo
        self.span = np.where((span >= 0) & (span < LD(np.finfo(np.float32).max)), span, LD(1))
        # (robot_info.h:82-84: a revolute joint whose limits span a full turn counts as one without limits)
        revolute = np.array([m.joint_type[self._joint_of(v)] == abi.JOINT_REVOLUTE for v in self.active], dtype=bool)
        self.bounded = np.asarray(m.var_bounded, dtype=bool)[self.active] & ~(revolute & (np.asarray(span, dtype=np.float64) >= 2 * np.pi * 0.9999))

    def _joint_of(self, v):
        m = self.model
        for l in range(m.n_links):
            f = m.joint_first_variable[l]
            if f >= 0 and f <= v < f + abi.JOINT_VAR_COUNT[m.joint_type[l]]:
                return l
        raise KeyError(v)

    def joint_cost(self, op, P, genes, seed, goal):
        """the goals over the joint values, for genes (n, D) and the full seed vector (goal_types.h:387-498)"""
        g = np.asarray(genes, dtype=LD)
        s = np.asarray(seed, dtype=LD)
        if op == abi.GOAL_AVOID_JOINT_LIMITS:
            d = np.maximum(LD(0), np.abs(g - self.mid) * 2 - self.span * LD(0.5)) * self.w
            return np.sum((d * self.bounded) ** 2, axis=1)
        if op == abi.GOAL_CENTER_JOINTS:
            return np.sum(((g - self.mid) * self.w * self.bounded) ** 2, axis=1)
        if op == abi.GOAL_REGULARIZATION:
            return np.sum((g - s[self.active]) ** 2, axis=1)
        if op == abi.GOAL_MINIMAL_DISPLACEMENT:
            return np.sum(((g - s[self.active]) * self.w) ** 2, axis=1)
        if op == abi.GOAL_JOINT_VARIABLE:
            v = self.model.variable_index(goal.variable_name())
            where = np.nonzero(self.active == v)[0]
            x = g[:, where[0]] if len(where) else np.full(g.shape[0], s[v], dtype=LD)
            return (LD(P[0]) - x) ** 2
        raise AssertionError(op)

    def full(self, seed, genes):
        x = np.tile(np.asarray(seed, dtype=LD), (genes.shape[0], 1))
        x[:, self.active] = genes
        return x

    def frames(self, seed, genes):
        """the global frames of all links: R (L, n, 3, 3), p (L, n, 3), and q (L, n, 4) for the tips' links"""
        R, p = fk_batch(self.model, self.full(seed, genes))
        return R, p

    def costs(self, seed, params, genes, frames=None, tip_frames=None):
        """the weighted cost of every goal: (n, n_goals) long double.  tip_frames: {link: (p (n, 3), q (n, 4))} in place of exact FK (linearised frames);
        BalanceGoal reads them too."""
        g = np.atleast_2d(np.asarray(genes, dtype=LD))
        n = g.shape[0]
        if tip_frames is None:
            R, p = frames if frames is not None else self.frames(seed, g)
            tip_frames = {l: (p[l], quat_from_rot_batch(R[l])) for l in set(self.tips)}
        out = np.zeros((n, len(self.template.goals)), dtype=LD)
        for k, (goal, off) in enumerate(zip(self.template.goals, self.template.param_offsets)):
            op = goal.opcode
            P = np.asarray(params[off:off + abi.GOAL_PARAM_COUNT[op]], dtype=LD)
            if op in JOINT_SET:
                c = self.joint_cost(op, P, g, seed, goal)
            elif op == abi.GOAL_BALANCE:
                c = self.balance_cost(P, tip_frames)
            else:
                pl, ql = tip_frames[self.model.link_index(goal.link_name())]
                c = link_cost(op, P, pl, ql)
            out[:, k] = c * LD(goal.getWeight()) ** 2
        return out

    def balance_cost(self, P, tip_frames):
        """goal_types.cpp:257-272: the centre of mass (every link with mass, its share of the total) off the target, perpendicular to the axis"""
        m = self.model
        mass = np.asarray(m.link_mass, dtype=LD)
        com = 0
        for l in np.nonzero(mass > 0)[0]:
            pl, ql = tip_frames[int(l)]
            com = com + (pl + qrot(ql, np.asarray(m.link_center[l], dtype=LD))) * (mass[l] / mass.sum())
        c = com - P[:3]
        c = c - P[None, 3:6] * (c @ P[3:6])[:, None]
        return np.sum(c * c, axis=1)

    def fitness(self, seed, params, genes, **kw):
        """(primary, secondary) sums (problem.cpp:244-257; ik_base.h:163-185)"""
        c = self.costs(seed, params, genes, **kw)
        sec = np.array([g.isSecondary() for g in self.template.goals], dtype=bool)
        return c[:, ~sec].sum(axis=1), c[:, sec].sum(axis=1)

    # -- approximator tables and linearised frames --------------------------------------------------------------------------------------------------------

    def approximator(self, seed, base, step=1e-5):
        """tips (T, 7) and deltas (T, D, 7) at the base genes, in the world-frame form of bioik_eval_approximator: position change and quaternion change per
        unit of the gene.  Revolute / prismatic genes: the analytic derivative, mimic joints that follow the gene on the tip's chain added with their factor
        (forward_kinematics.h:600-730).  Floating / planar variables: the reference's own forward difference -- bump by `step`, the tip's twist in its own
        frame over `step` (jacobian_numeric) -- in long double.  Returns also the quaternions' sign reference: the tips' q have w >= 0 where possible."""
        m = self.model
        x = self.full(seed, np.atleast_2d(np.asarray(base, dtype=LD)))
        R, p = fk_batch(m, x)
        T, D = len(self.tips), len(self.active)
        tips = np.zeros((T, 7), dtype=LD)
        deltas = np.zeros((T, D, 7), dtype=LD)
        var_link = {}
        for l in range(m.n_links):
            for k in range(abi.JOINT_VAR_COUNT[m.joint_type[l]]):
                var_link[m.joint_first_variable[l] + k] = l
        for ti, t in enumerate(self.tips):
            q = quat_from_rot_batch(R[t])[0]
            tips[ti, :3], tips[ti, 3:] = p[t, 0], q
            chain = set()
            l = t
            while l >= 0:
                chain.add(l)
                l = m.link_parent[l]
            for gi, v in enumerate(self.active):
                l = var_link[int(v)]
                jt = m.joint_type[l]
                if jt in (abi.JOINT_FLOATING, abi.JOINT_PLANAR):
                    if l not in chain:
                        continue
                    x2 = x.copy()
                    x2[0, v] += LD(step)
                    R2, p2 = fk_batch(m, x2)
                    lin = R[t, 0].T @ (p2[t, 0] - p[t, 0]) / LD(step)
                    ang = quat_twist(R[t, 0].T @ R2[t, 0]) / LD(step)
                    dp = R[t, 0] @ lin
                else:
                    dp, ang_w = np.zeros(3, dtype=LD), np.zeros(3, dtype=LD)
                    for j in [j for j in chain if m.joint_type[j] in (abi.JOINT_REVOLUTE, abi.JOINT_PRISMATIC)]:
                        f = self.follow_factor(j, l)
                        if f == 0:
                            continue
                        axis = R[j, 0] @ np.asarray(m.joint_axis[j], dtype=LD)
                        axis = axis / np.sqrt(axis @ axis)
                        if m.joint_type[j] == abi.JOINT_REVOLUTE:
                            dp = dp + f * np.cross(axis, p[t, 0] - p[j, 0])
                            ang_w = ang_w + f * axis
                        else:
                            dp = dp + f * axis
                    ang = R[t, 0].T @ ang_w
                dq = qmul(q, np.array([ang[0] * LD(0.5), ang[1] * LD(0.5), ang[2] * LD(0.5), LD(0)], dtype=LD))
                deltas[ti, gi, :3], deltas[ti, gi, 3:] = dp, dq
        return tips, deltas

    def follow_factor(self, j, l):
        """d(variable of joint j) / d(variable of joint l): 1 for j == l, the composed mimic factor if j follows l, 0 otherwise"""
        m = self.model
        if j == l:
            return LD(1)
        f = LD(1)
        k = j
        while m.joint_mimic[k] >= 0:
            f, k = f * LD(m.joint_mimic_factor[k]), m.joint_mimic[k]
            if k == l:
                return f
        return LD(0)

    def linear_frames(self, tips, deltas, base, genes):
        """forward_kinematics.h:1186-1231: tip + sum over the genes of delta * (gene - base), the quaternion not renormalised"""
        dv = np.asarray(genes, dtype=LD) - np.asarray(base, dtype=LD)[None]
        out = {}
        for ti, t in enumerate(self.tips):
            f = tips[ti][None] + dv @ deltas[ti]
            out[t] = (f[:, :3], f[:, 3:])
        return out

    # -- the success test ---------------------------------------------------------------------------------------------------------------------------------

    def check(self, seed, params, genes, dpos, drot, dtwist, frames=None):
        """Problem::checkSolutionActiveVariables (problem.cpp:259-341) for every row of genes: (ok (n,), values) where values lists, per check, the
        (n,) quantity, its threshold, its kind ('pos', 'rot', 'tw_lin', 'tw_ang', 'cost') and the goal's link -- so that a caller can tell the rows whose
        decision lies within an error bound of the threshold"""
        g = np.atleast_2d(np.asarray(genes, dtype=LD))
        n = g.shape[0]
        R, p = frames if frames is not None else self.frames(seed, g)
        ok = np.ones(n, dtype=bool)
        vals = []
        costs = None
        for k, (goal, off) in enumerate(zip(self.template.goals, self.template.param_offsets)):
            if goal.isSecondary():
                continue
            op = goal.opcode
            P = np.asarray(params[off:off + abi.GOAL_PARAM_COUNT[op]], dtype=LD)
            link = None if goal.link_name() is None else self.model.link_index(goal.link_name())
            if op in (abi.GOAL_POSITION, abi.GOAL_ORIENTATION, abi.GOAL_POSE):
                pa = P[:3] if op != abi.GOAL_ORIENTATION else np.zeros(3, dtype=LD)
                qa = P[3:7] if op == abi.GOAL_POSE else (P[:4] if op == abi.GOAL_ORIENTATION else np.array([0, 0, 0, 1], dtype=LD))
                pb, Rb = p[link], R[link]
                A = rot_from_quat(qa)
                checks = []
                if op == abi.GOAL_POSITION:
                    if dpos != DBL_MAX:
                        checks.append((np.sqrt(np.sum((pb - pa) ** 2, axis=1)), dpos, "pos", True))
                elif op == abi.GOAL_ORIENTATION:
                    if drot != DBL_MAX:
                        checks.append((angle_shortest_path(quat_from_rot_batch(Rb), qa) * 180 / np.pi, drot, "rot", True))
                elif dpos != DBL_MAX or drot != DBL_MAX:
                    checks.append((np.sqrt(np.sum((pb - pa) ** 2, axis=1)), dpos, "pos", True))
                    checks.append((angle_shortest_path(quat_from_rot_batch(Rb), qa) * 180 / np.pi, drot, "rot", True))
                if dtwist != DBL_MAX:
                    lin = (pb - pa) @ A  # A^T (pb - pa)
                    ang = np.stack([kdl_get_rot(A.T @ Rb[i]) for i in range(n)])
                    comps = ([lin[:, c] for c in range(3)] if op != abi.GOAL_ORIENTATION else []) + ([ang[:, c] for c in range(3)] if op != abi.GOAL_POSITION else [])
                    kinds = (["tw_lin"] * 3 if op != abi.GOAL_ORIENTATION else []) + (["tw_ang"] * 3 if op != abi.GOAL_POSITION else [])
                    for c, kd in zip(comps, kinds):
                        checks.append((np.abs(c), dtwist, kd, False))
                for v, th, kd, le in checks:
                    ok &= (v <= th) if le else (v < th)
                    vals.append((v, th, kd, link))
            else:
                if costs is None:
                    costs = self.costs(seed, params, g, frames=(R, p))
                dmax = min(DBL_MAX, min(dpos, dtwist))
                ok &= costs[:, k] < LD(dmax) * LD(dmax)
                vals.append((costs[:, k], LD(dmax) * LD(dmax), "cost", k))
        return ok, vals


def qmul(a, b):
    """Hamilton product of two quaternions (x, y, z, w)"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], dtype=LD)


def quat_twist(Rrel):
    """the rotation vector of a relative rotation as tf2 takes it apart (frame.h:240-259): angle 2 acos(w) folded into (-pi, pi], times the unit axis"""
    q = quat_from_rot_batch(Rrel[None])[0]
    w = np.clip(q[3], -1, 1)
    a = 2 * np.arccos(w)
    if a > np.pi:
        a -= 2 * np.pi
    s = np.sqrt(np.maximum(LD(0), 1 - w * w))
    if s < LD(10 * 2.220446049250313e-16):
        return np.array([a, 0, 0], dtype=LD)
    return q[:3] / s * a


def angle_shortest_path(q, qa):
    """tf2 Quaternion::angleShortestPath: 2 acos(|q . qa| / (|q| |qa|)), q (n, 4)"""
    qa = np.asarray(qa, dtype=LD)
    s = np.sqrt(np.sum(q * q, axis=1) * (qa @ qa))
    return 2 * np.arccos(np.clip(np.abs(q @ qa) / s, -1, 1))


def kdl_get_rot(d):
    """KDL::Rotation::GetRot of a 3x3 long-double matrix, with its branches: (almost) symmetric -- identity within 1e-5 gives 0, else an angle of pi --
    and otherwise atan2(|v| / 2, (trace - 1) / 2) about v = the skew part"""
    d = d.reshape(9)
    eps, eps2 = 1e-6, 1e-5
    if abs(d[1] - d[3]) < eps and abs(d[2] - d[6]) < eps and abs(d[5] - d[7]) < eps:
        if abs(d[1] + d[3]) < eps2 and abs(d[2] + d[6]) < eps2 and abs(d[5] + d[7]) < eps2 and abs(d[0] + d[4] + d[8] - 3) < eps2:
            return np.zeros(3, dtype=LD)
        xx, yy, zz = (d[0] + 1) / 2, (d[4] + 1) / 2, (d[8] + 1) / 2
        xy, xz, yz = (d[1] + d[3]) / 4, (d[2] + d[6]) / 4, (d[5] + d[7]) / 4
        if xx > yy and xx > zz:
            x = np.sqrt(xx)
            v = (x, xy / x, xz / x)
        elif yy > zz:
            y = np.sqrt(yy)
            v = (xy / y, y, yz / y)
        else:
            z = np.sqrt(zz)
            v = (xz / z, yz / z, z)
        return np.array(v, dtype=LD) * LD(np.pi)
    f = (d[0] + d[4] + d[8] - 1) / 2
    v = np.array([d[7] - d[5], d[2] - d[6], d[3] - d[1]], dtype=LD)
    nrm = np.sqrt(v @ v)
    return v / nrm * np.arctan2(nrm / 2, f)


def np_goal_cost(goal, frame, genes, seed, o, model):
    """one goal's unweighted cost for one frame (7,) and gene vector: the checks of tests/test_oracle_goals.py (o: the oracle under test, for its active
    variables only)"""
    op = goal.opcode
    P = np.asarray(goal.params(), dtype=LD)
    p = np.asarray(frame[:3], dtype=LD)[None]
    q = np.asarray(frame[3:], dtype=LD)[None]
    if op in JOINT_SET:
        t = type("T", (), {"model": model, "goals": [goal], "param_offsets": [0]})
        pr = Problem(t, o.active_variables, [])
        return pr.joint_cost(op, P, np.asarray(genes, dtype=LD)[None], seed, goal)[0]
    if op in (abi.GOAL_LOOK_AT, abi.GOAL_SIDE, abi.GOAL_DIRECTION, abi.GOAL_CONE):
        q = q / np.sqrt(np.sum(q * q))  # (the frame of exact FK: a unit quaternion; rotate with its matrix)
        R = rot_from_quat_batch(q)[0]
        if op == abi.GOAL_LOOK_AT:
            a, d = R @ P[:3], P[3:6] - p[0]
            return np.sum((d / np.sqrt(d @ d) - a / np.sqrt(a @ a)) ** 2)
        if op == abi.GOAL_SIDE:
            return max(LD(0), (R @ P[:3]) @ P[3:6]) ** 2
        if op == abi.GOAL_DIRECTION:
            return np.sum((R @ P[:3] - P[3:6]) ** 2)
        v = R @ P[4:7]
        ang = np.arccos(np.clip((v @ P[7:10]) / np.sqrt((v @ v) * (P[7:10] @ P[7:10])), -1, 1))
        return max(LD(0), ang - P[10]) ** 2 + P[3] ** 2 * np.sum((P[:3] - p[0]) ** 2)
    return link_cost(op, P, p, q)[0]
