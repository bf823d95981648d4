"""Random kinematic trees and goal lists, shared by the robot and goal soaks (tools/robot_fuzz_hostsim.py, tools/goal_fuzz_hostsim.py) and by the random-robot
cases (tests/random_robot_cases.py).  It lives beside the soaks, not under tests/, so that the soaks run with any test tree.  The two tools draw through `random_robot`, `fuzz_case` and `link_goal` exactly as they did when these lived in them:
their case lines for a given [cases] [seed] do not depend on this module's extensions, which draw only when asked for (`multi`, `random_case`)."""
import numpy as np

from bio_ik_amd import (AvoidJointLimitsGoal, BalanceGoal, CenterJointsGoal, ConeGoal, DirectionGoal, JointVariableGoal, LineGoal, LookAtGoal, MaxDistanceGoal,
                        MinDistanceGoal, MinimalDisplacementGoal, OrientationGoal, PlaneGoal, PoseGoal, PositionGoal, RegularizationGoal, RobotModel, SideGoal, abi)

# the device's limit on floating joints whose orientation variables are genes (bioik_compile.cpp)
MAX_ACTIVE_QUATERNIONS = 4


def unit(rng, n):
    v = rng.normal(size=n)
    return tuple(v / np.linalg.norm(v))


def random_robot(rng, case, big=False, plain=False, balance=False, multi=0.0, mimic=True):
    """A random tree of 4 - 14 links (big: 12 - 30): revolute, continuous, prismatic and fixed joints anywhere, rotated origins, oblique axes, mimic joints
    (also of a joint that mimics another), branches at any depth.  plain: trees whose DEFAULT joint program folds exactly (no rotated origin, no prismatic
    joint, fixed links without offset).  balance: links with mass.  multi > 0: each moving joint becomes a floating or planar joint with that probability
    (never a mimic, never mimicked); the translation variables of a floating joint and x, y of a planar one are bounded to +-1 m.  mimic=False: no mimic joint.
    Returns (model, the group's joints, number of links)."""
    m = RobotModel("r%d" % case)
    m.add_link("l0")
    n = int(rng.integers(4, 15)) if not big else int(rng.integers(12, 31))
    joints, moving, mimicable = [], [], []
    for i in range(1, n):
        parent = "l%d" % (i - 1 if rng.random() < 0.7 else int(rng.integers(0, i)))
        kind = str(rng.choice(["revolute", "revolute", "revolute", "continuous", "prismatic", "fixed"]))
        xyz = tuple(rng.normal(size=3) * 0.15) if rng.random() < 0.8 else (0.0, 0.0, 0.0)
        rpy = tuple(rng.normal(size=3) * 0.6) if rng.random() < 0.5 else (0.0, 0.0, 0.0)
        if plain:
            rpy = (0.0, 0.0, 0.0)
            if kind == "prismatic":
                kind = "revolute"
            if kind == "fixed":
                xyz = (0.0, 0.0, 0.0)
        axis = unit(rng, 3) if rng.random() < 0.5 else tuple(np.eye(3)[int(rng.integers(3))])
        if multi > 0.0 and kind != "fixed" and rng.random() < multi:
            kind = str(rng.choice(["floating", "planar"]))
        kw = {}
        if kind in ("revolute", "prismatic"):
            lo, hi = sorted(rng.normal(size=2) * (1.5 if kind == "revolute" else 0.2))
            kw = {"lower": float(lo - 0.1), "upper": float(hi + 0.1)}
        if kind != "fixed":
            kw["velocity"] = float(rng.uniform(0.3, 3.0))
            if moving and kind in ("revolute", "prismatic") and rng.random() < 0.12 and mimic:
                kw["mimic"] = (str(rng.choice(mimicable)), float(rng.choice([1.0, -0.5, 2.0])), float(rng.choice([0.0, 0.1])))
        if balance and rng.random() < 0.6:
            kw["mass"], kw["com"] = float(rng.uniform(0.2, 3.0)), tuple(rng.normal(size=3) * 0.05)
        m.add_link("l%d" % i, parent, "j%d" % i, kind, xyz=xyz, rpy=rpy, axis=axis, **kw)
        if kind != "fixed":
            joints.append("j%d" % i)
            if kind in ("revolute", "prismatic"):
                mimicable.append("j%d" % i)
                if "mimic" not in kw:
                    moving.append("j%d" % i)
    for v, name in enumerate(m.variable_names):
        if name.split("/")[-1] in ("trans_x", "trans_y", "trans_z", "x", "y"):
            m.var_min[v], m.var_max[v], m.var_bounded[v] = -1.0, 1.0, 1
    m._keep = None
    return m, joints, n


def walk_order(model, tips):
    """the tips in the order the chain walk completes them (bioik_compile.cpp: the links are scheduled chain by chain in the order of the tips, a tip is complete with
    the op of its nearest moving ancestor -- a tip behind fixed links only hangs off the root and is complete before the walk starts)"""
    tips = list(tips)
    for _ in range(len(tips) + 1):
        schedule = []
        for t in tips:
            chain, l = [], t
            while l >= 0:
                chain.append(l)
                l = model.link_parent[l]
            for l in reversed(chain):
                if l not in schedule:
                    schedule.append(l)
        ops = [l for l in schedule if model.joint_type[l] != 0]

        def src(t):
            l = t
            while l >= 0 and model.joint_type[l] == 0:
                l = model.link_parent[l]
            return ops.index(l) if l >= 0 else -1
        again = sorted(tips, key=lambda t: (src(t), tips.index(t)))
        if again == tips:
            break
        tips = again
    return tips


def link_goal(rng, link):
    """one link goal of any of the eleven link types (the goal soak's draw)"""
    w = float(rng.choice([0.2, 0.5, 1.0, 1.7]))
    p = tuple(rng.normal(size=3) * 0.4)
    k = int(rng.integers(11))
    if k == 0:
        return PositionGoal(link, p, weight=w)
    if k == 1:
        return OrientationGoal(link, unit(rng, 4), weight=w)
    if k == 2:
        return PoseGoal(link, p, unit(rng, 4), weight=w)
    if k == 3:
        return LookAtGoal(link, unit(rng, 3), p, weight=w)
    if k == 4:
        return MaxDistanceGoal(link, p, float(rng.uniform(0.1, 0.6)), weight=w)
    if k == 5:
        return MinDistanceGoal(link, p, float(rng.uniform(0.1, 0.6)), weight=w)
    if k == 6:
        return LineGoal(link, p, unit(rng, 3), weight=w)
    if k == 7:
        return PlaneGoal(link, p, unit(rng, 3), weight=w)
    if k == 8:
        return SideGoal(link, unit(rng, 3), unit(rng, 3), weight=w)
    if k == 9:
        return DirectionGoal(link, unit(rng, 3), unit(rng, 3), weight=w)
    return ConeGoal(link, unit(rng, 3), unit(rng, 3), float(rng.uniform(0.1, 0.8)), weight=w, position=p if rng.random() < 0.5 else None, position_weight=0.5)


def gene_goals(rng, joints, n, weights=(0.1, 0.5)):
    """up to n - 1 goals over the joint values, each primary or secondary"""
    goals = []
    for _ in range(int(rng.integers(0, n))):
        k, w, sec = int(rng.integers(5)), float(rng.choice(list(weights))), bool(rng.random() < 0.5)
        if k == 0:
            goals.append(JointVariableGoal(str(rng.choice(joints)), float(rng.normal() * 0.3), weight=w, secondary=sec))
        elif k == 1:
            g = RegularizationGoal(weight=w)
            g.secondary_ = sec
            goals.append(g)
        else:
            goals.append((MinimalDisplacementGoal, AvoidJointLimitsGoal, CenterJointsGoal)[k - 2](weight=w, secondary=sec))
    return goals


def robot_goals(rng, model, tips, joints, balance=False):
    """the robot soak's goal list: one or two link goals per tip in the order given, a BalanceGoal (balance and a link with mass), gene-only goals behind"""
    goals = []
    for t in tips:
        for _ in range(int(rng.choice([1, 1, 2]))):
            link, w, p = "l%d" % t, float(rng.choice([0.3, 1.0, 1.6])), tuple(rng.normal(size=3) * 0.3)
            k = int(rng.integers(11))
            goals.append([PositionGoal(link, p, weight=w), OrientationGoal(link, unit(rng, 4), weight=w), PoseGoal(link, p, unit(rng, 4), weight=w),
                          MaxDistanceGoal(link, p, 0.3, weight=w), MinDistanceGoal(link, p, 0.3, weight=w), LineGoal(link, p, unit(rng, 3), weight=w),
                          PlaneGoal(link, p, unit(rng, 3), weight=w), LookAtGoal(link, unit(rng, 3), p, weight=w), SideGoal(link, unit(rng, 3), unit(rng, 3), weight=w),
                          DirectionGoal(link, unit(rng, 3), unit(rng, 3), weight=w), ConeGoal(link, unit(rng, 3), unit(rng, 3), 0.4, weight=w)][k])
    if balance and sum(model.link_mass) > 0:
        goals.append(BalanceGoal(tuple(rng.normal(size=3) * 0.1), weight=float(rng.choice([0.4, 1.0]))))
    return goals + gene_goals(rng, joints, 3)


def describe(n, tips, fixed, goals):
    return "%d links, tips %s, fixed %s | %s" % (n, list(tips), fixed, " ".join("%s%s" % (type(g).__name__.replace("Goal", ""), "*" if g.secondary_ else "") for g in goals))


def fuzz_case(rng, case, big=False, plain=False, balance=False, gradient=False):
    """One case of the robot soak: (model, joints, tips, goals, fixed, desc, mode, fk, pop, steps); None where the tree has no moving joint"""
    model, joints, n = random_robot(rng, case, big=big, plain=plain, balance=balance)
    if not joints:
        return None
    tips = walk_order(model, sorted(int(t) for t in rng.choice(np.arange(1, n), size=min(int(rng.integers(1, 7 if big else 4)), n - 1), replace=False)))
    model.add_group("g", joints=joints, tips=["l%d" % t for t in tips])
    goals = robot_goals(rng, model, tips, joints, balance)
    fixed = [str(rng.choice(joints))] if rng.random() < 0.2 else []
    desc = describe(n, tips, fixed, goals)
    mode = str(rng.choice(["bio2", "bio2_memetic", "bio2_memetic_l"]))
    fk = int(rng.choice([abi.FK_EXACT, abi.FK_LINEAR]))
    pop, steps = int(rng.choice([8, 16, 33])), int(rng.choice([1, 2, 3]))
    if gradient and case % 3 == 0:  # (the gradient family's point solvers on the same trees)
        mode, fk, steps = str(("gd", "gd_r", "gd_c")[(case // 3) % 3]), abi.FK_EXACT, int(rng.choice([1, 5, 20]))
    return model, joints, tips, goals, fixed, desc, mode, fk, pop, steps


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# the random-robot cases: floating / planar joints, masses, goal lists in walk order or not, and what the device must refuse

def chain_of(model, l):
    out = []
    while l >= 0:
        out.append(l)
        l = model.link_parent[l]
    return out


def mimic_depth(model, l):
    """how many mimic links lead from joint l to the joint that moves it (0: not a mimic joint)"""
    d = 0
    while model.joint_mimic[l] >= 0:
        l, d = model.joint_mimic[l], d + 1
    return d


def descendants(model, l):
    out, frontier = [], [l]
    while frontier:
        c = frontier.pop()
        out.append(c)
        frontier += [k for k in range(model.n_links) if model.link_parent[k] == c]
    return out


class Case:
    """One generated problem: model, group "g", goals, fixed joints; `refusal`: why the device must refuse it (None: it must take it)"""

    def __init__(self, seed, model, joints, tips, goals, fixed, walk, refusal):
        self.seed, self.model, self.joints, self.tips, self.goals, self.fixed = seed, model, joints, tips, goals, fixed
        self.walk, self.refusal = walk, refusal
        self.may_refuse = None  # (a shape the device refuses in some trees: the message it then gives)

    def template(self):
        from bio_ik_amd import ProblemTemplate
        return ProblemTemplate(self.model, "g", self.goals, fixed_joints=self.fixed)

    def multi(self):
        return [l for l in range(self.model.n_links) if self.model.joint_type[l] in (abi.JOINT_FLOATING, abi.JOINT_PLANAR)]

    def __repr__(self):
        types = "".join("-RPFQ"[self.model.joint_type[l]] for l in range(1, self.model.n_links))
        return "seed %d [%s] tips %s fixed %s %s| %s%s" % (self.seed, types, self.tips, self.fixed, "walk " if self.walk else "", " ".join(
            "%s%s" % (type(g).__name__.replace("Goal", ""), "*" if g.secondary_ else "") for g in self.goals), "  (refused: %s)" % self.refusal if self.refusal else "")


def random_case(seed, multi=0.15, balance=True, plain=False, walk=None, big=False, n_tips=None, secondary=True, serial=False, gene_goals_secondary=False):
    """A random-robot case: a tree with floating / planar joints on the goal chains (multi), links with mass and a BalanceGoal (balance), two to three tips
    (one of them often on a fixed link), every link goal type with several goals per link, gene-only goals primary and secondary, a fixed joint now and then,
    the goals in walk order (walk=True), in a random order (walk=False) or either (None); n_tips: that many tips instead; secondary=False: every goal primary; serial: trees
    whose joint program is one serial chain (the kernels compiled for one lane mapping take only those); gene_goals_secondary: every goal over the joint
    values secondary.  A few cases are shapes the device refuses: a goal on a variable
    of a floating / planar joint that moves no tip, five floating joints with active orientation."""
    rng = np.random.default_rng(seed)
    crowd = multi > 0.0 and rng.random() < 0.1  # (a robot with many floating joints: beyond the device's four active orientations)
    if serial:  # (one tip, no mimic joint, every goal primary, no goal that names a variable: the joint program is one serial chain)
        n_tips, secondary, multi, balance, crowd = 1, False, 0.0, False, False
    model, joints, n = random_robot(rng, seed, big=big or crowd, plain=plain, balance=balance, multi=0.9 if crowd else multi, mimic=not serial)
    model.drawn_mimic_depth = max([mimic_depth(model, l) for l in range(model.n_links)] + [0])
    tips = sorted(int(t) for t in rng.choice(np.arange(1, n), size=min(int(rng.integers(1, 4)) if n_tips is None else n_tips, n - 1), replace=False))
    for l in range(1, n):  # floating / planar joints on a goal chain: a tip behind them (now and then none: the device refuses such a joint)
        if model.joint_type[l] in (abi.JOINT_FLOATING, abi.JOINT_PLANAR) and not any(l in chain_of(model, t) for t in tips) and rng.random() < 0.85:
            tips.append(int(rng.choice(descendants(model, l))))
    tips = walk_order(model, sorted(set(tips)))
    if not joints:
        return None
    model.add_group("g", joints=joints, tips=["l%d" % t for t in tips])
    single = [j for j in joints if model.joint_type[model.joint_names.index(j)] in (abi.JOINT_REVOLUTE, abi.JOINT_PRISMATIC)]
    goals = []
    for t in tips:
        for _ in range(int(rng.choice([1, 1, 2, 3]))):
            goals.append(link_goal(rng, "l%d" % t))
    if balance and sum(model.link_mass) > 0 and rng.random() < 0.6:
        b = BalanceGoal(tuple(rng.normal(size=3) * 0.1), weight=float(rng.choice([0.4, 1.0])))
        if rng.random() < 0.3:
            b.setAxis(unit(rng, 3))
        goals.append(b)
    goals += gene_goals(rng, single or ["j0"], 4, weights=(0.1, 0.5, 1.2)) if single else []
    on_chain = set(l for t in tips for l in chain_of(model, t))
    for l in range(1, n):  # (a goal on a variable of a floating / planar joint off the chains)
        if model.joint_type[l] in (abi.JOINT_FLOATING, abi.JOINT_PLANAR) and l not in on_chain and rng.random() < 0.7:
            v = model.joint_first_variable[l] + int(rng.integers(abi.JOINT_VAR_COUNT[model.joint_type[l]]))
            goals.append(JointVariableGoal(model.variable_names[v], float(rng.normal() * 0.3), weight=0.5))
    if not secondary:
        for g in goals:
            g.secondary_ = False
    if serial:
        goals = [g for g in goals if g.opcode != abi.GOAL_JOINT_VARIABLE]
    if gene_goals_secondary:  # (no primary goal over the joint values: a solve that meets the link goals succeeds)
        for g in goals:
            if g.link_name() is None and g.opcode != abi.GOAL_BALANCE:
                g.secondary_ = True
    in_walk = bool(rng.random() < 0.6) if walk is None else walk
    if not in_walk:
        goals = [goals[k] for k in rng.permutation(len(goals))]
    fixed = [str(rng.choice(single))] if single and rng.random() < 0.2 else []
    c = Case(seed, model, joints, tips, goals, fixed, in_walk, expected_refusal(model, tips, fixed, goals))
    named = set(model.variable_index(g.variable_name()) for g in goals if g.opcode == abi.GOAL_JOINT_VARIABLE)
    if any(var_joint(model, v) not in on_chain and model.joint_type[var_joint(model, v)] in (abi.JOINT_FLOATING, abi.JOINT_PLANAR) for v in named):
        c.may_refuse = "variables of floating / planar joints outside the goal chains"  # (refused where the joint program has no op for the variable)
    return c


def var_joint(model, v):
    """the link whose joint owns variable v"""
    for l in range(model.n_links):
        f = model.joint_first_variable[l]
        if f >= 0 and f <= v < f + abi.JOINT_VAR_COUNT[model.joint_type[l]]:
            return l
    raise KeyError(v)


def expected_refusal(model, tips, fixed, goals):
    """what the device refuses of the shapes random_case draws (bioik_compile.cpp): None if nothing"""
    on_chain = set(l for t in tips for l in chain_of(model, t))
    named = set(model.variable_index(g.variable_name()) for g in goals if g.opcode == abi.GOAL_JOINT_VARIABLE)
    quats = 0
    for l in range(model.n_links):
        jt = model.joint_type[l]
        if jt in (abi.JOINT_FLOATING, abi.JOINT_PLANAR) and model.joint_names[l] not in fixed:
            f = model.joint_first_variable[l]
            quats += jt == abi.JOINT_FLOATING and (l in on_chain or bool(named & set(range(f + 3, f + 7))))
    if quats > MAX_ACTIVE_QUATERNIONS:
        return "more than 4 floating joints with active orientation"
    return None


def sample_configurations(model, rng, n, odd_norms=True):
    """n full variable vectors: uniform in [min, max] (continuous joints and planar theta: [-pi, pi], translations of floating / planar joints: +-1 m), the
    quaternion of a floating joint a random unit quaternion -- or, one time in four, one of norm 0.5 ... 2 (the reference normalises it,
    forward_kinematics.h:120-126; odd_norms=False: unit quaternions only)"""
    lo, hi = np.asarray(model.var_min), np.asarray(model.var_max)
    x = lo + (hi - lo) * rng.random((n, model.n_variables))
    for l in range(model.n_links):
        if model.joint_type[l] == abi.JOINT_FLOATING:
            f = model.joint_first_variable[l]
            q = rng.normal(size=(n, 4))
            q /= np.linalg.norm(q, axis=1, keepdims=True)
            if odd_norms:
                q *= np.where(rng.random((n, 1)) < 0.25, rng.uniform(0.5, 2.0, size=(n, 1)), 1.0)
            x[:, f + 3:f + 7] = q
    return x


def coverage(cases, templates=None):
    """what a set of cases covers: joint types (0 fixed ... 4 planar, 'continuous' apart), goal opcodes, the deepest mimic chain (as drawn, before the model
    resolves it), tips on fixed links, fixed joints, secondary goals, goal lists out of walk order, refusals"""
    out = {"joint_types": set(), "continuous": 0, "opcodes": set(), "mimic_depth": 0, "tips_on_fixed_links": 0, "fixed_joints": 0, "secondary_goals": 0,
           "not_walk_order": 0, "refused": 0}
    for c in cases:
        m = c.model
        for l in range(1, m.n_links):
            out["joint_types"].add(int(m.joint_type[l]))
            out["continuous"] += int(m.joint_type[l] == abi.JOINT_REVOLUTE and m.joint_first_variable[l] >= 0 and not m.var_bounded[m.joint_first_variable[l]])
        out["mimic_depth"] = max(out["mimic_depth"], getattr(m, "drawn_mimic_depth", 0))
        out["opcodes"] |= set(int(g.opcode) for g in c.goals)
        out["tips_on_fixed_links"] += sum(1 for t in c.tips if m.joint_type[t] == abi.JOINT_FIXED)
        out["fixed_joints"] += len(c.fixed)
        out["secondary_goals"] += sum(1 for g in c.goals if g.secondary_)
        out["not_walk_order"] += int(not c.walk)
        out["refused"] += int(c.refusal is not None)
    return out


def normalise_quaternions(model, X):
    """X with the quaternion of every floating joint scaled to unit norm"""
    X = np.array(X, dtype=np.float64, copy=True)
    for l in range(model.n_links):
        if model.joint_type[l] == abi.JOINT_FLOATING:
            f = model.joint_first_variable[l]
            X[:, f + 3:f + 7] /= np.linalg.norm(X[:, f + 3:f + 7], axis=1, keepdims=True)
    return X
