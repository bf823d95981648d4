/*
 * bioik_hip.h — C-ABI boundary of the MI355X-native bio2_memetic IK solver.
 *
 * This header is the drop-in boundary described in DESIGN.md §1.  It replaces, for the hot path
 * only, the pair of calls
 *
 *     ik->initialize(problem);   ik->solve();           (reference src/kinematics_plugin.cpp:566-578)
 *
 * i.e. `bio_ik::IKParallel::initialize/solve/getSolution/getSuccess/getSolutionFitness`
 * (reference src/ik_parallel.h:141-145, 193-276), and everything those calls execute:
 * `IKEvolution2<'q'>::initialize/step` (src/ik_evolution_2.cpp:111-230, 328-646), `RobotFK`
 * (src/forward_kinematics.h:65-1234), `Problem::computeGoalFitness/checkSolutionActiveVariables`
 * (src/problem.cpp:244-341) and the built-in `Goal::evaluate`s (include/bio_ik/goal_types.h).
 *
 * Only plain C types cross this boundary: no C++ classes, no torch types, no HIP types (streams and
 * device pointers travel as `void*`).  The reference-side adapter that marshals
 * `moveit::core::RobotModel` / `bio_ik::Goal` objects into these PODs is shown in INTEGRATION.md and
 * implemented (against stand-in MoveIt headers) in bio_ik_amd/cpp/.
 *
 * Conventions
 *   - a frame is 7 doubles: px py pz qx qy qz qw  (Hamilton quaternion, reference
 *     include/bio_ik/frame.h:51-56 stores the same 7 numbers + 1 pad)
 *   - every function returns BIOIK_OK (0) or a negative status; it never aborts or throws.
 *     `bioik_last_error()` returns a thread-local human-readable message for the last failure.
 *   - handles are opaque and must be destroyed by the matching *_destroy.
 */
#ifndef BIOIK_HIP_H
#define BIOIK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BIOIK_ABI_VERSION 6 /* 6, additions that break no caller of 6: bioik_model_desc::link_capsule_first / link_capsules behind the fields every caller of 6 fills (a shorter struct_size
                               gets none), BIOIK_MAX_LINK_CAPSULES (CAPSULES: a segment with a radius as a link's collision shape; opcodes 17, 19 and 20 read it, no new opcode).
                               6, additions that break no caller of 6: BIOIK_GOAL_SELF_CLEARANCE (opcode 20: the spheres of two links of the robot keep apart; the second link in goal_base_link).
                               6, additions that break no caller of 6: BIOIK_GOAL_CLEARANCE (opcode 19; 18 stays unknown), BIOIK_MAX_OBSTACLES, bioik_problem_set_obstacles,
                               bioik_problem_obstacle_count (a link's spheres keep clear of a table of obstacle spheres).
                               6, additions that break no caller of 6: bioik_problem_desc::goal_base_link behind the fields every caller of 6 fills (a shorter struct_size gets none),
                               BIOIK_MAX_HELD_FRAMES (BASE LINKS: a link goal evaluated in another link's frame).
                               6, additions that break no caller of 6: bioik_solve_batch_bounded, bioik_solve_batch_bounded_submit, bioik_solve_batch_bounded_device, bioik_eval_bounds,
                               bioik_problem_op_count, bioik_problem_op_variables
                               (per-query variable bounds).
                               6, additions that break no caller of 6: bioik_solve_params::island_migration in the slot of `reserved0` (0, what every caller of 6 wrote there, is off),
                               BIOIK_MAX_MIGRATIONS, bioik_eval_migrate, bioik_problem_carry_doubles (the islands of a query share their best every E steps).
                               6, additions that break no caller of 6: bioik_solve_batch_ranked, bioik_solve_batch_ranked_device (the k best distinct islands of every query).
                               6 (round 6): bioik_resolve_islands (the island count BIOIK_ISLANDS_AUTO gives a call of n queries, for callers that shard a request themselves);
                               a rendezvous time-out inside a workgroup is BIOIK_ERR_HIP for its call; a line-search candidate with a joint value of magnitude >= bioik_sincos_domain()
                               (2^47; 1e300 until the shared sincos had a stated domain) is no candidate: no solve returns such a value for a variable without bounds.  A joint's half angle
                               is factor x value / 2, so every angle a solve evaluates lies inside the domain for mimic factors of magnitude up to 2.
                               5 (round 5): bioik_solve_params::islands = 0 means BIOIK_ISLANDS_AUTO (versions up to 4 took 0 as 1); `timeout` counts from the call */

/* ---- status codes ------------------------------------------------------------------------- */
enum {
    BIOIK_OK = 0,
    BIOIK_ERR_INVALID_ARGUMENT = -1, /* malformed descriptor (reference: ERROR(...) -> std::runtime_error, src/utils.h:122-129) */
    BIOIK_ERR_UNSUPPORTED = -2,      /* joint/goal type that has no device implementation */
    BIOIK_ERR_NO_DEVICE = -3,        /* no HIP device / extension not usable: the product path never falls back to CPU */
    BIOIK_ERR_HIP = -4,              /* a HIP runtime call failed; message in bioik_last_error() */
    BIOIK_ERR_NOT_FOUND = -5         /* link/variable not part of the group (reference src/problem.cpp:125,141) */
};

/* ---- joint types: moveit::core::JointModel::JointType as used by
 *      RobotJointEvaluator::getJointFrame (reference src/forward_kinematics.h:78-139) ---------- */
enum {
    BIOIK_JOINT_FIXED = 0,
    BIOIK_JOINT_REVOLUTE = 1,  /* also URDF "continuous" (unbounded revolute) */
    BIOIK_JOINT_PRISMATIC = 2,
    BIOIK_JOINT_FLOATING = 3,  /* 7 variables x y z qx qy qz qw; device: anywhere on the goal chains (general flavour of the solver kernel); refused: such
                                  a joint as a mimic of another, its variables off the goal chains, more than four with an active orientation              */
    BIOIK_JOINT_PLANAR = 4     /* 3 variables x y theta;          device: as FLOATING                                                     */
};

/* ---- goal opcodes: one per closed-form class of reference include/bio_ik/goal_types.h.
 *      `n_params` doubles per query, laid out as listed.  Vectors that the reference normalises
 *      in its setters/constructors (quaternions, directions) must arrive normalised. ------------ */
enum {
    BIOIK_GOAL_POSITION = 0,             /* goal_types.h:80-97    params: pos[3]                                  */
    BIOIK_GOAL_ORIENTATION = 1,          /* goal_types.h:99-124   params: quat[4]                                 */
    BIOIK_GOAL_POSE = 2,                 /* goal_types.h:126-181  params: pos[3] quat[4] rotation_scale           */
    BIOIK_GOAL_LOOK_AT = 3,              /* goal_types.h:183-212  params: axis[3] target[3]                       */
    BIOIK_GOAL_MAX_DISTANCE = 4,         /* goal_types.h:214-241  params: target[3] distance                      */
    BIOIK_GOAL_MIN_DISTANCE = 5,         /* goal_types.h:243-270  params: target[3] distance                      */
    BIOIK_GOAL_LINE = 6,                 /* goal_types.h:272-298  params: position[3] direction[3]                */
    BIOIK_GOAL_PLANE = 7,                /* goal_types.h:300-328  params: position[3] normal[3]                   */
    BIOIK_GOAL_AVOID_JOINT_LIMITS = 8,   /* goal_types.h:379-402  params: -                                       */
    BIOIK_GOAL_CENTER_JOINTS = 9,        /* goal_types.h:404-426  params: -                                       */
    BIOIK_GOAL_REGULARIZATION = 10,      /* goal_types.h:428-445  params: -                                       */
    BIOIK_GOAL_MINIMAL_DISPLACEMENT = 11,/* goal_types.h:447-466  params: -                                       */
    BIOIK_GOAL_JOINT_VARIABLE = 12,      /* goal_types.h:468-499  params: position                                */
    BIOIK_GOAL_SIDE = 13,                /* goal_types.h:585-614  params: axis[3] direction[3]                    */
    BIOIK_GOAL_DIRECTION = 14,           /* goal_types.h:616-644  params: axis[3] direction[3]                    */
    BIOIK_GOAL_CONE = 15,                /* goal_types.h:646-712  params: position[3] position_weight axis[3] direction[3] angle */
    BIOIK_GOAL_BALANCE = 16,             /* goal_types.h:540-566, goal_types.cpp:231-272  params: target[3] axis[3].  Reads the frames of
                                            EVERY link of the model with a positive mass (bioik_model_desc::link_mass), each of which
                                            becomes a tip of the problem, as BalanceGoal::describe does                              */
    BIOIK_GOAL_TOUCH = 17,               /* goal_types.h:330-377, goal_types.cpp:152-228  params: position[3] normal[3].  The collision shapes of the
                                            link touch the plane through `position` with unit `normal`: with the link's frame (p, q), its
                                            points (v_i, r_i) of bioik_model_desc::link_points and its disks (c_j, a_j, r_j) of link_disks,
                                                n_l = rotate(conjugate(q), normal)
                                                d = min( min_i (n_l . v_i - r_i),  min_j (n_l . c_j - r_j |n_l x a_j|) ) - normal . (position - p)
                                            and the cost is d * d.  No FCL: a box is its 8 corners, a sphere one point with a radius, a mesh its
                                            vertices, a cylinder its two end disks, a cone its base disk and its apex (the support function along
                                            the normal, what the reference's hill climb returns; a disk's is exact in closed form, and n_l is not
                                            assumed to be of unit length).  A CAPSULE of the link (link_capsules: ends A, B, radius r) joins the points as
                                            its two end spheres (A, r) and (B, r): along any normal the support of a capsule is the smaller of theirs, so
                                            this is exact; bioik_problem_create appends the two rows per capsule behind the link's points.  A link with
                                            neither points nor disks nor capsules: BIOIK_ERR_INVALID_ARGUMENT; more than BIOIK_MAX_TOUCH_POINTS points and
                                            disks together, a capsule counting as two points: BIOIK_ERR_UNSUPPORTED                                */
    BIOIK_GOAL_TYPE_COUNT = 18,          /* the opcodes 0 ... 17 are the reference's closed-form classes.  OPCODE 18 IS NO GOAL AND STAYS UNKNOWN: bioik_goal_param_count(18) is -1
                                            and bioik_problem_create refuses it (callers and tests of ABI 6 rely on that) */
    BIOIK_GOAL_CLEARANCE = 19            /* no reference counterpart (there: a solution_callback behind the search).  params: margin.  The spheres of the link keep at least
                                            `margin` away from the goal's table of OBSTACLE SPHERES in the world frame (bioik_problem_set_obstacles below).  With the
                                            link's frame (p, q), its rows (v_i, r_i), i < n, of bioik_model_desc::link_points and the obstacle rows (c_j, R_j), j < m:
                                                w_i  = p + rotate(q, v_i)            q as it is, not normalised (the phenotypes of BIOIK_FK_LINEAR included)
                                                s_ij = (margin + r_i) + R_j
                                                pen  = s_ij > 0 ? max(0, s_ij - |w_i - c_j|) : 0
                                                cost = sum_i sum_j pen^2             i outer, j inner, both ascending, one running sum from 0
                                            The operations, each rounded once, in this order (fma(a, b, c) = a b + c with one rounding; bio_ik_amd/csrc/bioik_fused.h):
                                                t = q.xyz x v:      t.x = fma(q.y, v.z, -(q.z v.y)),  t.y = fma(q.z, v.x, -(q.x v.z)),  t.z = fma(q.x, v.y, -(q.y v.x))
                                                u = q.w t + q.xyz x t: u.x = fma(q.w, t.x, fma(q.y, t.z, -(q.z t.y))),  u.y = fma(q.w, t.y, fma(q.z, t.x, -(q.x t.z))),  u.z = fma(q.w, t.z, fma(q.x, t.y, -(q.y t.x)))
                                                rotate(q, v) = fma(2, u, v) per component (bk_qrot of bioik_fused.h), then w = p + that: three additions
                                                sm = margin + r_i;   s = sm + R_j;   e = c_j - w_i (three subtractions);   d2 = fma(e.x, e.x, fma(e.y, e.y, e.z e.z))
                                                if (s > 0 && d2 < s s) { pen = max(0, s - sqrt(d2));  sum = fma(pen, pen, sum); }          sqrt correctly rounded
                                            The test in front of the root skips nothing that would count: sqrt(fl(s s)) == s for a correctly rounded root, rounding is
                                            monotone, so d2 >= fl(s s) implies fl(sqrt(d2)) >= s and pen = 0.  A NaN in d2 or s fails the test: the pair adds nothing.
                                            m = 0 (a new problem; an empty table): the cost is exactly 0.  Success test: the default branch of every non-pose link goal,
                                            weighted cost < min(dpos, dtwist)^2 -- "clear of every obstacle by the margin, up to the threshold".  A secondary
                                            ClearanceGoal reads the null frame, like every secondary link goal of this library.  jac, gd*, ranked, bounded, migration,
                                            timeout and island_sync behave as for a problem with a TouchGoal; such a problem runs in the general kernel flavour.
                                            CAPSULES of the link (below the opcodes): its k capsules follow its n points -- each against every obstacle j, ascending, into
                                            the same running sum.  Refused by bioik_problem_create: a link with neither points nor capsules
                                            BIOIK_ERR_INVALID_ARGUMENT; a link that carries disks or a marker row (r == -1: never approximated silently), more than
                                            BIOIK_MAX_LINK_CAPSULES capsules, more than BIOIK_MAX_TOUCH_POINTS points and capsules together, a base link on the goal
                                            (self-collision): BIOIK_ERR_UNSUPPORTED.  About nine FP64 issue slots per pair that does not penetrate and eighteen per point (counted in the
                                            code, not timed): 8 points against 16 obstacles cost about as much as the chain walk of a 7-joint arm
                                            (measured rates: profiles/clearance_goal_metadata_and_bench.log) */
    ,
    BIOIK_GOAL_SELF_CLEARANCE = 20       /* no reference counterpart (there: a solution_callback behind the search).  params: margin.  SELF-COLLISION BETWEEN TWO LINKS: the
                                            spheres of the goal's link L keep at least `margin` away from the spheres of a second link O of the same robot (the "other"
                                            link), which bioik_problem_desc::goal_base_link[g] names -- for this opcode the field is REQUIRED.  L's rows (v_i, r_i), i < n, and
                                            O's rows (c_j, R_j), j < m, both of bioik_model_desc::link_points, each in its own link's frame; both tables are known when the
                                            problem is created (no bioik_problem_set_obstacles table, no count word in device memory).  With A = O's frame and B = L's
                                            frame of the same individual:
                                                R    = concat(invert(A), B)          exactly the R of BASE LINKS below, in its order of operations: nothing normalised, the
                                                                                     phenotypes of BIOIK_FK_LINEAR included
                                                w_i  = R.p + rotate(R.q, v_i)        L's sphere centres in O's frame
                                                s_ij = (margin + r_i) + R_j
                                                pen  = s_ij > 0 ? max(0, s_ij - |w_i - c_j|) : 0
                                                cost = sum_i sum_j pen^2             i outer, j inner, both ascending, one running sum from 0
                                            From w_i on the operations, their order, the fused ones and the exact test in front of the root (s > 0 && d2 < s s) are those of
                                            BIOIK_GOAL_CLEARANCE above, word for word, with (R.p, R.q) in place of (p, q).  Success test: the default branch of every non-pose
                                            link goal, weighted cost < min(dpos, dtwist)^2, on R.  jac, gd*, ranked, bounded, migration, timeout and island_sync behave as
                                            for any problem with a based goal: BIOIK_MODE_JAC is refused at the solve call.  The goal (L, O) and the goal (O, L) state the
                                            same distances and differ in the order of summation: equal up to rounding, not bit for bit.
                                            Refused by bioik_problem_create, the message naming the goal's index: no other link (-1, a NULL goal_base_link, a struct_size
                                            that ends in front of the field), a goal that names no link, the other link the goal's own, either link with neither points
                                            nor capsules: BIOIK_ERR_INVALID_ARGUMENT; either link with disks or a marker row (r == -1: never approximated), either link
                                            with more than BIOIK_MAX_LINK_CAPSULES capsules, L with more than BIOIK_MAX_TOUCH_POINTS points and capsules together, O with
                                            more than BIOIK_MAX_OBSTACLES, a secondary goal, more than BIOIK_MAX_HELD_FRAMES held links: BIOIK_ERR_UNSUPPORTED; an unknown
                                            other link: BIOIK_ERR_NOT_FOUND.  bioik_problem_set_obstacles and bioik_problem_obstacle_count say "not a CLEARANCE goal" of
                                            it.  Such a problem runs in the general kernel flavour.
                                            CAPSULES of either link (below): L's primitives are outermost, its points, then its capsules; for each of them O's points come
                                            first, then O's capsules; everything in O's frame through the same R; one running sum.  A capsule of O needs no transform
                                            (its u, u.u and ru are formed once, when the problem is created, by the operations below: the same bits); a capsule of L has
                                            its two ends carried over once, in front of the inner loops.  Not built: a broad phase, pairs taken automatically from an
                                            SRDF's collision matrix, capsules or boxes in the obstacle table of opcode 19
                                            (measured: profiles/self_clearance_metadata_and_bench.log, profiles/capsules_metadata_and_bench.log) */
    /* CAPSULES (bioik_model_desc::link_capsules; no opcode of their own: opcodes 19 and 20 measure against them, opcode 17 reads each as two spheres).  A capsule is
       a segment with a radius r >= 0: every point within r of the segment.  Write A, B for its two ends CARRIED INTO THE FRAME THE GOAL WORKS IN -- the world
       through the link's frame (p, q) for opcode 19, O's frame through R for a capsule of L under opcode 20 -- by the same p + rotate(q, v) as a point's, with q as
       it is, not normalised (the phenotypes of BIOIK_FK_LINEAR included); a capsule of O under opcode 20 is taken as it stands.  Every operation below is rounded
       once; fma(a, b, c) = a b + c with one rounding; x.y of two vectors is fma(x.x, y.x, fma(x.y, y.y, x.z y.z)); clamp(x) = min(max(x, 0), 1).
       Per segment (A, B), formed once per segment and not per pair:
           u = B - A (three subtractions)      uu = u.u      ru = uu > DBL_MIN ? 1 / uu : 0          (one division, correctly rounded)
       ru = 0 makes the segment count as its FIRST END: the zero quaternion of a linearised phenotype collapses every segment of a link to a point (A == B == p), and
       0 / 0 is never formed.
       SPHERE (c, R) AGAINST CAPSULE (A, B, r):
           e = c - A (three subtractions)      t = clamp((e.u) ru)
           X = A + t u:  fma(t, u.x, A.x) ... per component          x = c - X (three subtractions)          d2 = x.x
       CAPSULE (A, B, r1) AGAINST CAPSULE (C, D, r2), (A, B) the capsule of the goal's link, with u, uu, ru of (A, B) and v, vv, rv of (C, D):
           w = A - C (three subtractions)      uv = u.v      uw = u.w      vw = v.w
           den = fma(uu, vv, -(uv uv))                                                                 (= uu vv sin^2 of the angle between the axes)
           s = den > 0 ? clamp(fma(uv, vw, -(vv uw)) / den) : 0                                        the two-line solution; 0 for parallel axes
           t = fma(uv, s, vw) rv               tc = clamp(t)
           if (tc != t || rv == 0)  s = clamp(fma(uv, tc, -uw) ru)                                     t left [0, 1] (or (C, D) counts as a point): s solved again
           X = A + s u,  Y = C + tc v  (fma per component, as above)          x = X - Y (three subtractions)          d2 = x.x
       Then for both, with the radius of the GOAL'S LINK's primitive first (for opcode 20: L's, whether it is the sphere or the capsule):
           s_pair = (margin + r_link) + r_other
           if (s_pair > 0 && d2 < s_pair s_pair) { pen = max(0, s_pair - sqrt(d2));  sum = fma(pen, pen, sum); }     opcode 19's tail, word for word
       d2 is the squared distance of two points that lie ON the two primitives, so it is never below the true squared distance; it exceeds it only through the
       error of s, which is large relative to 1 only where den cancels (axes within about 1e-7 rad of parallel: up to a few 1e-8 m on segments of 0.3 m; exactly
       parallel axes are exact, any s gives the same distance).  No finite input whose squares stay finite yields a NaN or an infinity: every quotient has a
       denominator > 0 or is replaced by 0, and clamp() returns 0 or 1 for an infinite argument.
       One routine per formula serves every site (bio_ik_amd/csrc/bioik_device.h: seg_make, seg_point_d2, seg_seg_d2, clearance_tail).  A model WITHOUT capsules
       gives, for both opcodes, exactly the bits it gave before capsules existed (tests/golden/clearance_parent_bits.npz). */
    /* JointFunctionGoal / LinkFunctionGoal (std::function) have no device opcode: DESIGN.md §7. */
};
/* Obstacle spheres one BIOIK_GOAL_CLEARANCE may hold (every evaluation of every individual reads all of them against every point of the link). */
#define BIOIK_MAX_OBSTACLES 256
/* Points one BIOIK_GOAL_TOUCH may read (the table of its link).  The minimum is a loop every evaluation of every individual runs in full: about five
 * FP64 issue slots per point (three fused multiply-adds, a minimum and its canonicalisation; counted in the compiled loop, not timed), so by that count a few
 * hundred points cost as much as the whole chain walk of a 7-joint arm (profiles/touch_goal_metadata_and_bench.log has measured solves per second at 8, 64 and 1024 points).
 * Hand meshes over as their convex hull or decimated: only hull vertices can be the minimum.
 * A disk counts as one point towards this limit and costs about 29 FP64 issue slots, as much as six points: six for the cross product, three for its
 * squared norm, fourteen for the square root (a reciprocal square root estimate, its refinement to the correctly rounded root and the scaling around it), three
 * for n . c, and the closing fused multiply-add, minimum and canonicalisation (again counted in the compiled loop, not timed). */
#define BIOIK_MAX_TOUCH_POINTS 1024
/* Capsules one goal may read from one link (CAPSULES at the goal opcodes).  Points and capsules of a goal's link together stay within BIOIK_MAX_TOUCH_POINTS, those of
 * BIOIK_GOAL_SELF_CLEARANCE's other link within BIOIK_MAX_OBSTACLES; for BIOIK_GOAL_TOUCH a capsule counts as two points. */
#define BIOIK_MAX_LINK_CAPSULES 64

/* number of per-query parameter doubles of a goal opcode, or -1 for an unknown opcode */
int bioik_goal_param_count(int goal_type);

/* ---- solver modes: IKFactory names of reference src/ik_evolution_2.cpp:652-654 -------------- */
enum {
    BIOIK_MODE_BIO2 = 0,            /* "bio2":           16 generations per step, no memetic phase      */
    BIOIK_MODE_BIO2_MEMETIC = 1,    /* "bio2_memetic":   8 generations + quadratic ('q') line search    */
    BIOIK_MODE_BIO2_MEMETIC_L = 2,  /* "bio2_memetic_l": 8 generations + linear ('l') line search       */
    /* IKFactory names of reference src/ik_gradient.cpp:254-292 (population / fk_mode are not used).  Island 0 of a query starts at the seed;
       with islands = N > 1 the islands 1 ... N - 1 start at random configurations, as the solver threads 1 ... N - 1 of the reference's
       "gd_2" ... "gd_8", "gd_r_2" ..., "gd_c_2" ..., "jac_2" ... "jac_8" do (:157-159, :283-285), and the best island is returned        */
    BIOIK_MODE_GD_C = 3,            /* "gd_c": gradient descent by central differences of the exact fitness, linear step estimate,
                                       always continue (ik_gradient.cpp:136-251, if_stuck = 'c')                                   */
    BIOIK_MODE_GD = 5,              /* "gd":   as gd_c, but a step is kept only if it lowers the fitness (src/ik_gradient.cpp:225-232) */
    BIOIK_MODE_JAC = 4,             /* "jac":  pseudo-inverse-Jacobian steps on the twists between the tips and their pose goals
                                       (ik_gradient.cpp:42-133, 269-292)                                                          */
    BIOIK_MODE_GD_R = 6             /* "gd_r": as gd, but a configuration that a step failed to improve is replaced by a random one
                                       before the next step (:165-170, :233-237); the best configuration seen is returned          */
};

/* What the launcher optimises a solve for (the measured figures of the current round: DESIGN.md section 6).
 * LATENCY (default): the time of THIS call.  A query gets the lanes that make its steps short (128 and two helper wavefronts: ~90 us per step of the 7-joint
 *   arm), and a batch beyond what the chip holds of such workgroups (3072 queries and more) starts under the denser mapping below -- every query resident from
 *   the first moment -- and hands its stragglers to the short-step mapping when the chip runs empty.  Three such solves in flight keep an MI355X busy.
 * THROUGHPUT: solves per second of a STREAM of batches.  Both species of a query share one wavefront and the children are computed where they
 *   are read, sixteen queries per CU: a third more steps per ms on a full chip, but a step takes 2.5 x as long, so the stragglers of a batch run for
 *   up to 12 ms.  It pays with six to ten batches in flight on as many streams -- and hardware queues: the HIP runtime maps streams onto four unless
 *   GPU_MAX_HW_QUEUES says otherwise -- and costs an isolated call about a fifth more time.  Problems the denser mapping does not exist for (secondary
 *   goals with more than 256 children, 32 or more genes, floating joints) run as under LATENCY.  So does a call with per-query variable bounds
 *   (bioik_solve_batch_bounded): the dense mapping's kernel has no build that reads them.
 * AUTO: LATENCY, except in bioik_solve_batch_submit when two or more solves of the handle are already in flight: THROUGHPUT then (a caller
 *   that streams batches through the asynchronous entry gets the dense mapping once its pipeline is three deep; an isolated call stays as fast as it
 *   can be). */
enum { BIOIK_SCHEDULE_LATENCY = 0, BIOIK_SCHEDULE_THROUGHPUT = 1, BIOIK_SCHEDULE_AUTO = 2 };
/* bioik_solve_params::islands = BIOIK_ISLANDS_AUTO (0): as many islands per query as the part of the chip the call leaves idle can carry --
 * for a call of n queries (per device) max(min(16, 2048 / n), min(64, 512 / n)), at least four up to n = 1024, one beyond that: 64 for up to eight queries
 * (MoveIt's one pose per call), 32 for sixteen, 16 up to 128 ... -- stopping each other (island_sync is then taken as 1): the reference's four island
 * threads with "any thread succeeds => all stop" (ik_parallel.h:102, 141-178), sized to the hardware.  A call that cannot fill the chip is bound by its
 * slowest query's number of steps, and islands cut exactly that (MI355X, PoseGoal on a 7-joint arm, pop 128: 16 queries 3.5 -> 1.25 ms per call, 256 queries
 * 6.2 -> 2.8 ms, one query 1.2 -> 0.71 ms: bench.py's small_batches).  bioik_resolve_islands() returns the count a call of n queries would get.
 * THE ANSWER OF A QUERY THEN DEPENDS ON THE SIZE OF THE CALL IT CAME IN (the island count is a function of n, and the islands' streams of random numbers are
 * part of the answer): give an explicit count where answers must not depend on batching.  The bio2 family only: for gd / jac an island count names another
 * solver ("gd_8"). */
enum { BIOIK_ISLANDS_AUTO = 0 };

/* how a child's phenotype (tip frames) is obtained inside the evolution loop */
enum {
    BIOIK_FK_LINEAR = 0, /* the reference's first-order extrapolation RobotFK_Mutator::computeApproximateMutations
                            (src/forward_kinematics.h:1172-1233) around the species' elite                       */
    BIOIK_FK_EXACT = 1   /* exact chain walk per individual, RobotFK_Fast_Base::applyConfiguration semantics
                            (src/forward_kinematics.h:331-354) — the north-star GPU path                         */
};

/* ---- flattened robot model = what RobotJointEvaluator/RobotFK_Fast_Base/RobotInfo read from
 *      moveit::core::RobotModel (reference src/forward_kinematics.h:192-213, 230-246, 268-329;
 *      include/bio_ik/robot_info.h:70-106).  One entry per link; entry i also describes the link's
 *      parent joint (MoveIt: every link has exactly one parent joint). --------------------------- */
typedef struct bioik_model_desc {
    uint32_t struct_size;               /* sizeof(bioik_model_desc), for ABI evolution */
    uint32_t n_links;
    uint32_t n_variables;
    uint32_t reserved;
    const int32_t* link_parent;          /* [n_links] parent link index, -1 for the root link; parent < child */
    const double* link_origin;           /* [n_links*7] LinkModel::getJointOriginTransform()            */
    const int32_t* joint_type;           /* [n_links] BIOIK_JOINT_*                                      */
    const double* joint_axis;            /* [n_links*3] Revolute/PrismaticJointModel::getAxis()          */
    const int32_t* joint_first_variable; /* [n_links] JointModel::getFirstVariableIndex(), -1 if none   */
    const int32_t* joint_mimic;          /* [n_links] link index whose joint this joint mimics, -1 (a mimic of a mimic is resolved to the joint at the end of the chain with the composed factor and offset, as MoveIt's RobotModel::buildMimic does) */
    const double* joint_mimic_factor;    /* [n_links] getMimicFactor()                                   */
    const double* joint_mimic_offset;    /* [n_links] getMimicOffset()                                   */
    const double* var_min;               /* [n_variables] VariableBounds::min_position_                  */
    const double* var_max;               /* [n_variables] VariableBounds::max_position_                  */
    const uint8_t* var_bounded;          /* [n_variables] VariableBounds::position_bounded_              */
    const double* var_max_velocity;      /* [n_variables] VariableBounds::max_velocity_                  */
    const double* link_mass;             /* [n_links] urdf::Link::inertial->mass, 0 where the link has no <inertial>; NULL: no link
                                            has one (only BIOIK_GOAL_BALANCE reads it, goal_types.cpp:236-247)                  */
    const double* link_center;           /* [n_links*3] urdf::Link::inertial->origin.position (link frame); NULL with link_mass   */
    /* Collision points of the links (BIOIK_GOAL_TOUCH reads them, BIOIK_GOAL_CLEARANCE and BIOIK_GOAL_SELF_CLEARANCE as spheres), in compressed rows: link l owns the points link_point_first[l] ... link_point_first[l + 1]
       - 1.  A point is x y z r IN THE LINK FRAME (the shape's collision origin already applied by the caller), r >= 0 the radius of a sphere around it.  A row with
       r == -1 exactly is no point but a MARKER (any other negative radius is BIOIK_ERR_INVALID_ARGUMENT): the link carries a mesh whose vertices are not there, or a shape the caller did not convert into points or disks (a cylinder or a cone it left as it was) -- the model is accepted, a BIOIK_GOAL_TOUCH that names
       the link is refused with BIOIK_ERR_UNSUPPORTED (such a shape is never approximated silently).  Both NULL: no link has shapes.  A caller whose struct_size ends in front of these two fields (a build against the header without them) gets none.                    */
    const int32_t* link_point_first;     /* [n_links + 1] ascending, [0] = 0                                                       */
    const double* link_points;           /* [link_point_first[n_links] * 4]                                                        */
    /* Collision disks of the links (only BIOIK_GOAL_TOUCH reads them), rows like the points': link l owns the disks link_disk_first[l] ... link_disk_first[l + 1] - 1.
       A disk is cx cy cz r ax ay az 0 IN THE LINK FRAME: centre, radius r >= 0, axis of unit length (|a| within 1e-9 of 1), and a zero that fills the row;
       everything finite, else BIOIK_ERR_INVALID_ARGUMENT.  A cylinder is the hull of its two end disks, a cone that of its base disk and its apex (a point with
       r = 0 in link_points): both exact.  Both NULL: no link has disks.  A caller whose struct_size ends in front of these two fields, or in front of
       link_point_first (builds against the two earlier headers), gets none; a size between two of the three is BIOIK_ERR_INVALID_ARGUMENT.                  */
    const int32_t* link_disk_first;      /* [n_links + 1] ascending, [0] = 0                                                       */
    const double* link_disks;            /* [link_disk_first[n_links] * 8]                                                         */
    /* Collision capsules of the links (CAPSULES at the goal opcodes: BIOIK_GOAL_CLEARANCE and BIOIK_GOAL_SELF_CLEARANCE measure against them, BIOIK_GOAL_TOUCH reads each as its two
       end spheres), rows like the disks': link l owns the capsules link_capsule_first[l] ... link_capsule_first[l + 1] - 1.  A capsule is ax ay az r bx by bz 0 IN THE
       LINK FRAME: the two ends A and B of a segment, a radius r >= 0, and a zero that fills the row -- every point within r of the segment.  BIOIK_ERR_INVALID_ARGUMENT:
       a number that is not finite, r < 0, an eighth number that is not 0, A == B (a sphere is a point row of link_points).  Both NULL: no link has capsules.  A caller
       whose struct_size ends in front of these two fields (or in front of one of the two earlier pairs: builds against the three earlier headers) gets none; a size
       between two of the four, or beyond the struct, is BIOIK_ERR_INVALID_ARGUMENT. */
    const int32_t* link_capsule_first;   /* [n_links + 1] ascending, [0] = 0                                                       */
    const double* link_capsules;         /* [link_capsule_first[n_links] * 8]                                                      */
} bioik_model_desc;

/* ---- one goal of the problem template (structure shared by every query of a batch; the numeric
 *      parameters are per query).  Mirrors what Goal::describe() puts into GoalContext
 *      (reference include/bio_ik/goal.h:87-90, 113-117) plus the goal's class. ------------------ */
typedef struct bioik_goal_desc {
    int32_t type;      /* BIOIK_GOAL_*                                                     */
    int32_t link;      /* link index for LinkGoalBase-derived goals, -1 otherwise          */
    int32_t variable;  /* variable index for BIOIK_GOAL_JOINT_VARIABLE, -1 otherwise       */
    int32_t secondary; /* Goal::isSecondary()                                              */
    double weight;     /* Goal::getWeight()                                                */
} bioik_goal_desc;

/* BASE LINKS (no reference counterpart: there such a goal is a LinkFunctionGoal or a Goal subclass with two addLink calls).  A link goal -- POSITION, ORIENTATION,
 * POSE, LOOK_AT, MAX_DISTANCE, MIN_DISTANCE, LINE, PLANE, SIDE, DIRECTION, CONE -- may name a BASE LINK in bioik_problem_desc::goal_base_link.  With A the base
 * link's frame and B the goal link's frame of the same individual, the goal is evaluated on
 *     R = concat(invert(A), B):   R.q = conj(A.q) (x) B.q,   R.p = rotate(conj(A.q), -A.p) + rotate(conj(A.q), B.p)        (reference frame.h:189-209)
 * in place of the link's world frame -- the formula as it stands, nothing normalised, also for the unnormalised quaternions of BIOIK_FK_LINEAR phenotypes -- in
 * both places a link goal reads a frame: its cost (the parameters keep their meaning, read in the base link's frame) and the success test (Position / Orientation /
 * Pose: the dpos / drot / dtwist test on R; the others: weighted cost < min(dpos, dtwist)^2, problem.cpp:327-334).  Base -1 is the world: everything as without the field.
 * The base link becomes a tip link of the problem and the joints of its chain active variables, as any link a goal names (problem.cpp:125, 191-204).
 * A walk keeps no table of tip frames: a based goal is attached to whichever of its two links the walk completes LATER, the earlier one's frame is held until then;
 * at most BIOIK_MAX_HELD_FRAMES DISTINCT links of a problem can be held (the number of based goals is limited only by the goal tables).  Such a problem runs in the
 * general kernel flavour (k_solve / k_solve_bounded / k_solve_point*), 56 bytes of LDS per lane more for every held link and for every link a based goal sits at.
 * Refused by bioik_problem_create: base >= n_links BIOIK_ERR_NOT_FOUND; a base on a goal without a link, or equal to the goal's own link: BIOIK_ERR_INVALID_ARGUMENT;
 * a base on a secondary goal (secondary link goals read the null frame, ik_base.h:163: it would be a constant), on BIOIK_GOAL_TOUCH or BIOIK_GOAL_BALANCE, or more
 * than BIOIK_MAX_HELD_FRAMES distinct held links: BIOIK_ERR_UNSUPPORTED.  Refused by every solve entry: BIOIK_MODE_JAC on a problem with a based goal,
 * BIOIK_ERR_UNSUPPORTED (its tip objectives are world poses, ik_gradient.cpp:64-66; gd, gd_r, gd_c minimise the fitness and work).
 * BIOIK_GOAL_SELF_CLEARANCE reads the same R with its base link as the OTHER link, and for it the field is required (a base on BIOIK_GOAL_CLEARANCE stays refused). */
#define BIOIK_MAX_HELD_FRAMES 4

/* ---- problem template = the arguments of Problem::initialize (reference src/problem.cpp:72-228)
 *      that do not change from query to query. -------------------------------------------------- */
typedef struct bioik_problem_desc {
    uint32_t struct_size;
    uint32_t n_group_joints;
    const int32_t* group_joints; /* link indices of JointModelGroup::getActiveJointModels(), in that order */
    uint32_t n_goals;
    uint32_t n_fixed_joints;
    const bioik_goal_desc* goals;
    const int32_t* fixed_joints; /* link indices of BioIKKinematicsQueryOptions::fixed_joints (goal.h:124) */
    /* BASE LINKS (above).  A caller whose struct_size ends in front of this field (a build against the header without it) gets none; a size that ends inside it
       is BIOIK_ERR_INVALID_ARGUMENT. */
    const int32_t* goal_base_link; /* [n_goals] link index, -1 = world; NULL: no goal has one */
} bioik_problem_desc;

/* ---- solver parameters = IKParams (reference src/utils.h:64-85) restricted to bio2*, plus the
 *      additive GPU keys of DESIGN.md §5. -------------------------------------------------------- */
typedef struct bioik_solve_params {
    uint32_t struct_size;
    int32_t mode;            /* BIOIK_MODE_*; yaml "mode" (kinematics_plugin.cpp:252)                    */
    int32_t fk_mode;         /* BIOIK_FK_*;  new key "gpu_fk"                                            */
    int32_t population;      /* children per species per generation (reference hard-codes 16,
                                ik_evolution_2.cpp:138); new key "gpu_population"                        */
    int32_t islands;         /* independent islands per query (reference concurrency()==4 identical
                                clones, ik_evolution_2.cpp:649 + utils.h:423); new key "gpu_islands".  Applies to
                                every mode: for gd / gd_r / gd_c / jac, islands = N > 1 is the reference's "gd_N" ...
                                (islands 1 ... N - 1 start at random configurations).  0 = BIOIK_ISLANDS_AUTO (above);
                                bioik_default_solve_params sets 1                                            */
    int32_t max_steps;       /* budget in IKEvolution2::step() calls per island (deterministic; checked after
                                every step like the success test of ik_parallel.h:173-181)               */
    uint64_t random_seed;    /* yaml "random_seed" (kinematics_plugin.cpp:256)                           */
    double dpos, drot, dtwist; /* yaml keys (kinematics_plugin.cpp:259-261); <0 or >=FLT_MAX disables   */
    int32_t no_wipeout;      /* debugging aid: disable species wipe-outs                                 */
    int32_t schedule;        /* BIOIK_SCHEDULE_*: what the launcher optimises for; new key "gpu_schedule".  The results do not
                                depend on it (the lane mapping never changes a trajectory).                              */
    double timeout;          /* the caller's `timeout` of searchPositionIK [s] (kinematics_plugin.cpp:504, 574;
                                ik_parallel.h:160, 200 `ros::WallTime::now() < timeout`): wall-clock budget of ONE
                                bioik_solve_batch* call, counted FROM THE CALL (round 5): the library keeps the device's
                                100 MHz clock paired with the host's steady clock and hands the kernels the call's deadline in
                                device ticks, so a solve that waits behind other solves of the caller's pipeline (several
                                submits in flight, several device-pointer solves on busy streams) is not granted its wait on
                                top.  Every query runs at least one step (ik_parallel.h:160 `iteration != 0`), then stops at
                                the first of: success, max_steps, timeout.  A call CAPTURED into a hipGraph cannot know when it
                                will be replayed: its budget counts from the moment the replay's first workgroup starts (at most
                                64 captured calls with a timeout per handle).  <= 0: no wall-clock limit (results are then
                                independent of timing).                                                                    */
    int32_t island_sync;     /* islands > 1: 0 = every island runs to its own success or budget and the best one is returned (ik_parallel.h:220-269
                                over independent islands); 1 = "any island succeeds => all stop" (the reference's `finished` flag, ik_parallel.h:102,
                                160-178) in its deterministic form: the islands of a query advance step by step together and all stop at the end of the
                                FIRST step in which any of them passes the success test; the result is the best of the islands that passed in that
                                step, `steps` is that step's number.  (On the device an island leaves as soon as it sees that another one has passed at
                                an earlier or the same step -- its own result can no longer be chosen -- so WHEN it leaves depends on timing, WHAT is
                                returned does not.)  New key "gpu_island_sync". */
    int32_t island_migration; /* E (the slot of `reserved0`; 0 = off, the default; < 0: BIOIK_ERR_INVALID_ARGUMENT): the islands of a query share their best solution
                                every E steps -- ISLAND MIGRATION below.  New key "gpu_island_migration". */
} bioik_solve_params;

/* ISLAND MIGRATION (bioik_solve_params::island_migration = E > 0, more than one island once BIOIK_ISLANDS_AUTO is resolved, a mode of the bio2 family).  Without
 * it the islands of a query are independent restarts; with it the solve is cut at the steps E, 2E, 3E, ... < max_steps -- at most BIOIK_MAX_MIGRATIONS of them,
 * behind the last one the islands run independently to the end -- and at every such BOUNDARY, per query:
 *   live       the islands handed over at the boundary: neither solved, nor out of time, nor overtaken (island_sync) after the boundary's step.
 *   donor      the live island with the least solution fitness, equal values: the lower island index.  A query with fewer than two live islands is left alone.
 *   recipient  every other live island whose own solution fitness is STRICTLY greater than the donor's.  Its species of rank 1 (the worse of the two after the step's
 *              ranking) is re-founded exactly as a wipe-out re-founds it (ik_evolution_2.cpp:617-645), with the donor's solution in place of the uniform draws: both
 *              elites take the donor's solution for every op, both gradients are zeroed, and under BIOIK_FK_EXACT the two elites' fitness words take the donor's
 *              solution fitness (under BIOIK_FK_LINEAR every generation re-evaluates them, as after a wipe-out).  Every other word of the recipient -- its rank-0
 *              species, its own solution, the rest of its bookkeeping -- stays; the donor is only read.
 * The result is a function of (seed, query, islands, parameters): a boundary is a kernel boundary, the order in which islands reach it takes no part.  The cap is part of
 * that contract (the host queues every launch of a call up front; once every island has finished the remaining launches are empty grids, each a launch latency on the
 * one-pose calls this is for).  The migration plan replaces the launcher's other plans (its hand-overs, BIOIK_SOLVE_TWO_PHASE); the mapping switches keep working; the
 * islands are reduced by k_select / k_select_ranked behind the last launch.  island_sync, timeout, ranked calls (row 0 stays the plain call's answer for the same
 * parameters) work unchanged.  E > 0 with one island or E >= max_steps is the call E = 0 is: the same launches.  Refused with BIOIK_ERR_UNSUPPORTED: E > 0 with a mode
 * of the gradient family (gd, gd_r, gd_c, jac), and E > 0 on a stream that is being captured into a hipGraph. */
#define BIOIK_MAX_MIGRATIONS 8

/* defaults: bio2_memetic, exact FK, population 128, 1 island, 64 steps, no timeout, seed 0, dpos=drot=off, dtwist=1e-5 */
void bioik_default_solve_params(bioik_solve_params* p);

typedef struct bioik_model bioik_model;
typedef struct bioik_problem bioik_problem;

const char* bioik_last_error(void);
int bioik_abi_version(void);
/* number of usable HIP devices (0 when none); never fails */
int bioik_device_count(void);
/* Diagnostics (no reference counterpart): the library reads its BIOIK_SOLVE_* / BIOIK_PHASE_DUMP switches (tools/README.md: forced lane mappings,
 * hand-overs, the mapping report) from the environment ONCE, when it is loaded; this call reads them again.  The test-suite uses it to run every
 * lane mapping in one process; nothing on the solve path touches the environment. */
int bioik_debug_reload_switches(void);
/* The launcher's lane mappings are chosen by rules fitted to the robots of BASELINE.json -- and, since round 5, checked by measurement: the FIRST
 * chip-filling call (2048 (query, island) units and more) of a kind -- (population, fk_mode, islands or not) under the latency schedule, no timeout -- that a
 * handle sees through a host-pointer entry (bioik_solve_batch, bioik_solve_batch_submit, bioik_solve_batch_multi) is run once per eligible mapping (each
 * run IS the caller's solve: every mapping returns the same bits), timed with events, and the fastest is kept for the handle; bioik_solve_batch_device uses
 * a handle's choice but never waits for its stream to make one (BIOIK_SOLVE_AUTOTUNE=2: it does; =0: the rules alone).  That first call takes about five
 * times as long as the ones after it.  BIOIK_SOLVE_REPORT=1 prints the table (profiles/r05_measured_mapping_choice.log). */

/* replaces RobotFK/RobotInfo construction from a RobotModel (ik_base.h:144-151) */
int bioik_model_create(const bioik_model_desc* desc, int device, bioik_model** out);
void bioik_model_destroy(bioik_model* m);

/* replaces Problem::initialize + IKBase::initialize(problem) -> RobotFK::initialize(tips)
 * (problem.cpp:72-228, ik_base.h:154-161, forward_kinematics.h:253-330, 566-599).
 * Size limits of one problem (BIOIK_ERR_UNSUPPORTED beyond them): 64 moving joints on the union of the goal chains (a short
 * chain in front of a branch counts once per branch), 63 active variables, 64 tip links, 24 primary + 24 secondary goals, 4 BalanceGoals,
 * BIOIK_MAX_TOUCH_POINTS collision points and disks together per TouchGoal (gathered once into a device buffer the handle owns: global memory, no LDS),
 * BIOIK_MAX_TOUCH_POINTS points per ClearanceGoal and BIOIK_MAX_OBSTACLES obstacles in its table (the same buffer; the table's storage is there at full capacity from the start).
 * Capsules: BIOIK_MAX_LINK_CAPSULES per link a ClearanceGoal or SelfClearanceGoal reads, counted with that link's points towards the limits above.
 * Tips and joints are further bounded TOGETHER by the 160 KiB of LDS of a CU: the function-level entry points hold 7 x tips x joints doubles
 * of tables plus a genotype column per lane (64 tips on 12 joints: 71 KiB; 24 tips on 63 joints: about 137 KiB; 64 tips on 63 joints: about
 * 290 KiB), the solvers hold more.  A problem beyond that is accepted here and refused with BIOIK_ERR_UNSUPPORTED by every entry point that
 * cannot hold it, before any launch; gd / gd_r / gd_c / jac stop at 64 KiB. */
int bioik_problem_create(bioik_model* model, const bioik_problem_desc* desc, bioik_problem** out);
void bioik_problem_destroy(bioik_problem* p);

/* introspection of what Problem::initialize derived */
int bioik_problem_active_variable_count(const bioik_problem* p);          /* Problem::active_variables.size()  */
int bioik_problem_active_variables(const bioik_problem* p, int32_t* out); /* robot variable index per gene      */
int bioik_problem_tip_count(const bioik_problem* p);                      /* Problem::tip_link_indices.size()   */
int bioik_problem_tip_links(const bioik_problem* p, int32_t* out);
int bioik_problem_param_count(const bioik_problem* p);                    /* doubles per query in goal_params   */
int bioik_problem_variable_count(const bioik_problem* p);                 /* robot variables V                  */
/* Global index of query 0 of the following bioik_solve_batch* calls (default 0).  The random stream of a query is
 * keyed by (random_seed, global query index, island), so a batch sharded over several GPUs / calls reproduces the
 * unsharded run when every shard announces its offset.  (New: the reference has one query per call.) */
int bioik_problem_set_first_query(bioik_problem* p, uint64_t first_query);
/* OBSTACLE TABLES of the problem's BIOIK_GOAL_CLEARANCE goals: one table per goal, at most BIOIK_MAX_OBSTACLES rows cx cy cz R (centre in the world frame, radius
 * R >= 0), shared by every query.  `goal_index` counts bioik_problem_desc::goals.  A new problem has empty tables (such a goal then costs exactly 0).
 * set_obstacles replaces the goal's whole table by the n rows of `spheres` (host pointer; n = 0: `spheres` may be NULL).  Refused, and the table then is what it was:
 * a null handle, an index out of range or a goal that is no CLEARANCE goal, n > 0 with spheres NULL, a number that is not finite or R < 0:
 * BIOIK_ERR_INVALID_ARGUMENT; n > BIOIK_MAX_OBSTACLES: BIOIK_ERR_UNSUPPORTED.
 * The call takes the handle's lock, completes the handle's submitted tickets (their results are delivered), waits for the handle's own streams and copies before it
 * returns: every solve or evaluation called after it reads the new table, every one completed before it read the old one.  Device-pointer solves on the CALLER's
 * streams are the caller's to wait for (CONCURRENCY below).  The storage is allocated once, at full capacity, by bioik_problem_create and its address never
 * changes; the row count lives in device memory beside the rows, not in anything a launch is given: a solve captured into a hipGraph REPLAYS WITH WHATEVER TABLE
 * IS CURRENT at the replay.  obstacle_count: the rows of the goal's table, or BIOIK_ERR_INVALID_ARGUMENT as above. */
int bioik_problem_set_obstacles(bioik_problem* p, int goal_index, size_t n, const double* spheres /* [n][4] cx cy cz R, world frame */);
int bioik_problem_obstacle_count(const bioik_problem* p, int goal_index);
/* What bioik_solve_params::islands = BIOIK_ISLANDS_AUTO means for a call of n queries on this handle's device: the island count and island_sync the call would
 * run with (an explicit count comes back as it is).  For callers that cut ONE request into several calls -- the MoveIt plugin's shards over `gpu_devices` --
 * and want every part to run the same solve whatever its size: resolve once for the largest part (ceil(rows / W), as bioik_solve_batch_multi does) and pass the
 * explicit figures to every call.  (The reference has no counterpart: its island count is the host's thread count, src/ik_parallel.h:84, utils.h:423.) */
int bioik_resolve_islands(const bioik_problem* p, const bioik_solve_params* params, size_t n, int32_t* islands, int32_t* island_sync);

/*
 * The batched solve: replaces IKParallel::solve() for n independent queries
 * (reference src/ik_parallel.h:193-270, per query).
 *   seeds        [n][V]  Problem::initial_guess (kinematics_plugin.cpp:466-485, 507): full variable vectors
 *   goal_params  [n][P]  per-query goal parameters, goals in template order (P = bioik_problem_param_count)
 *   solutions    [n][V]  IKParallel::getSolution(): full variable vector (inactive variables = seed)
 *   fitness      [n]     IKParallel::getSolutionFitness(): primary fitness of the exact-FK pose, plus its secondary fitness where the query succeeded and the
 *                        problem has secondary goals (ik_parallel.h:222-246)
 *   success      [n]     IKParallel::getSuccess(): Problem::checkSolutionActiveVariables on the exact-FK pose
 *   steps        [n]     number of step() calls executed by the winning island (new: device counter)
 * Host-pointer variant: copies in, solves, copies out, synchronises.
 */
int bioik_solve_batch(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* seeds,
                      const double* goal_params, double* solutions, double* fitness, int32_t* success,
                      int32_t* steps);

/* CONCURRENCY.  Safe from any thread, at the same time, on ONE handle: bioik_solve_batch, bioik_solve_batch_submit / _wait, bioik_solve_batch_device (on different
 * streams the solves then overlap on the device), bioik_solve_batch_multi, the function-level entries (bioik_eval_*, bioik_stream_fitness_device) -- each works on
 * the handle's mutable state under the handle's lock, for the length of the CALL, not of the device work it enqueues (the wait of bioik_solve_batch_wait itself
 * happens outside the lock: another thread may submit meanwhile) -- and bioik_resolve_islands and the bioik_problem_*_count / _variables / _links getters, which
 * read what never changes after bioik_problem_create and take no lock.  A synchronous call holds the lock until its results are there: the synchronous calls of
 * several threads on ONE handle run one after the other (use bioik_solve_batch_submit, or a handle per thread -- handles are independent of each other, also on one
 * device, and may be created and destroyed while other handles are solving).  bioik_last_error() is per thread.
 * NOT allowed while any call of that handle is running or any solve of it is in flight (no lock covers them): bioik_problem_set_first_query (bioik_solve_batch and
 * bioik_solve_batch_multi read the offset before they take the lock), bioik_problem_destroy (wait for device-pointer solves on your own streams first; submitted
 * tickets are completed by it) and, process-wide, bioik_debug_reload_switches (diagnostics).  (tests/concurrency_cases.py)
 * bioik_problem_set_obstacles stands between the two groups: it takes the handle's lock, completes the handle's submitted tickets and waits for the handle's own streams
 * before it copies, so it is safe beside every call of the first group -- but a device-pointer solve that is still RUNNING on one of the caller's own streams is the
 * caller's to wait for first (the library does not know those streams): such a solve may read rows of either table.  bioik_problem_obstacle_count takes the lock too. */

/* The same solve without waiting for it — for a caller with a STREAM of batches, the batched counterpart of calling
 * IKParallel::solve() from several threads (reference src/ik_parallel.h:193-218 keeps its own worker threads busy the same way).
 * `submit` copies the inputs into a page-locked arena of the handle, enqueues transfer in / solve / transfer out on one of the
 * handle's SIX internal streams (tickets rotate over them) and returns a ticket; `wait` blocks until that solve is complete and
 * its results are in the arrays given to `submit`, which must stay valid until then.  Up to six solves of a handle are in flight
 * together (three fill the chip under BIOIK_SCHEDULE_LATENCY, six under BIOIK_SCHEDULE_THROUGHPUT): the slow tail of one (a few queries that use the whole step budget) runs behind the bulk of the next, which is worth
 * about a factor of two in solves per second on 4096-query batches.  Submitting a seventh solve first
 * completes the oldest one (its results are delivered; its `wait` then returns at once).  Tickets may be waited for in any
 * order, from any thread; a ticket that is never waited for is completed by a later submit or by bioik_problem_destroy. */
int bioik_solve_batch_submit(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* seeds,
                             const double* goal_params, double* solutions, double* fitness, int32_t* success,
                             int32_t* steps, uint64_t* ticket);
int bioik_solve_batch_wait(bioik_problem* p, uint64_t ticket);

/* The same batch over several problem handles of ONE template — one handle per GPU of the node (the "device list" of the batched
 * searchPositionIK()), or several handles on one device.  Shard r = queries [r n / W, (r + 1) n / W) goes
 * to problems[r] on its own host thread and stream; there is no exchange between shards, and because the random stream of a query is
 * keyed by its global index (the offset set on problems[0] + its position in this batch) the result equals the unsharded solve bit
 * for bit.  Host pointers; returns when every shard is complete; the first failing shard's status is returned. */
int bioik_solve_batch_multi(bioik_problem* const* problems, int n_problems, const bioik_solve_params* params, size_t n,
                            const double* seeds, const double* goal_params, double* solutions, double* fitness,
                            int32_t* success, int32_t* steps);

/* Device-pointer variant: all arrays already resident in HBM on the problem's device; enqueues on
 * `hip_stream` (a hipStream_t passed as void*, NULL = default stream) and returns without synchronising.
 * Solves of ONE problem handle on different streams may be in flight together (their result arrays must differ; the scratch
 * of a solve is one persistent buffer per (handle, stream), taken from the stream-ordered pool by the first call on that stream and
 * released with the handle): keeping two or three batches in flight hides the slow tail of each
 * solve behind the bulk of the next.  A call enqueues one kernel or a short chain of kernels (large
 * batches pass their stragglers from a first launch to a second through device memory; islands > 1 add a selection
 * kernel); nothing in it waits for the host, so it may be captured into a hipGraph and replayed any number of times, on new contents of the
 * captured arrays too: make one eager call of the same size on the stream first (it sizes the scratch).  The words a solve resets per
 * call (hand-over counters, the timeout's clock, the islands' first-success words) are written by a kernel of this library, NOT by
 * hipMemsetAsync: on ROCm 7.2 a graph with a memset node in front of these kernels faults on its second replay (HISTORY.md).
 * Lifetime of the scratch under capture: a buffer a captured call has used is PINNED -- the graph holds its address -- and stays alive until
 * bioik_problem_destroy; the next eager call on that stream moves on to a buffer of its own, whatever its size.  Graphs captured from ONE
 * stream of one handle may share that stream's pinned buffer, whatever their kinds (one launch or several, islands reduced in the launch or by
 * k_select, a hand-over, a timeout, any number of queries and islands): every captured call sets up the words it relies on itself on each replay
 * (the islands' control words laid out for ITS query count), so one graph's replay leaves nothing another's depends on.  Replays of graphs that
 * share a buffer must not overlap: launch them on one stream, or wait for one before launching the next (or capture from different streams).
 * The one eager call before a capture must take the same plan as the captured call -- the same queries, islands, mode, population and steps,
 * under the same BIOIK_SOLVE_* switches: a call in one launch sizes other scratch than one with hand-overs.  Destroy the graphs before the
 * handle.  A problem with a BIOIK_GOAL_CLEARANCE: the captured kernels read the goal's obstacle table and its row count from the handle's device memory at every replay, so a
 * replay runs with WHATEVER TABLE IS CURRENT (bioik_problem_set_obstacles between two replays takes effect; wait for a replay before changing the table).
 * A call with island_migration > 0 that would migrate (more than one island, E < max_steps) is NOT capturable: BIOIK_ERR_UNSUPPORTED on a capturing stream. */
int bioik_solve_batch_device(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* d_seeds,
                             const double* d_goal_params, double* d_solutions, double* d_fitness,
                             int32_t* d_success, int32_t* d_steps, void* hip_stream);

/* PER-QUERY VARIABLE BOUNDS: the solves above with two more arrays, var_lo and var_hi, [n][V] doubles each, indexed by robot variable (MoveIt: the
 * consistency_limits of KinematicsBase::searchPositionIK, trajectory continuity, sampling inside joint-space boxes, pinning a joint for some queries only).
 * THE RULE.  For query q and robot variable v that is an ACTIVE variable of the problem (bioik_problem_active_variables):
 *   - lo = var_lo[q][v] and hi = var_hi[q][v] both finite and lo <= hi: the query is solved AS IF THE MODEL HAD BEEN CREATED WITH var_min[v] = lo, var_max[v] = hi,
 *     var_bounded[v] = 1 -- with everything the library derives from those three: a revolute variable with hi - lo >= 2 pi 0.9999 loses its clip (and counts as
 *     unbounded for AvoidJointLimitsGoal / CenterJointsGoal); clip_min / clip_max; span = hi - lo, 1 where that is not in [0, FLT_MAX); the limits the limit goals
 *     and the random re-founding of a species (and the random configurations of gd_r / the gradient family's islands) read.
 *   - otherwise (a NaN, an infinity, lo > hi): the variable keeps the model's own bounds for that query.  This is how a caller bounds only some variables.
 * Entries of variables that are no active variables of the problem are not read.  All islands of a query share its row.  Nothing else about the solve changes:
 * the same random streams, bioik_problem_set_first_query keying, timeout, island_sync, island_migration; every mode and both fk_modes.
 * THE SOLVER DOES NOT CLIP THE SEED: a query whose seed lies outside its bounds may return that seed (the reference's solvers on a model narrowed that way do);
 * a query whose seed lies inside its bounds returns a solution inside them, success or not.
 * Both arrays NULL: the call IS the plain call (bioik_solve_batch / _submit / _device: the same launches, kernels and bits).  Exactly one NULL:
 * BIOIK_ERR_INVALID_ARGUMENT, nothing launched, outputs untouched.  A bounded call runs the general kernel's build that reads a query's bounds from a table in
 * LDS (k_solve_bounded; k_solve_point_bounded for gd / jac): 32 m bytes of LDS per workgroup more (m ops); a problem that no longer fits a CU's LDS with it is
 * refused with BIOIK_ERR_UNSUPPORTED before any launch.  Under BIOIK_SCHEDULE_THROUGHPUT it runs as under LATENCY.  It neither takes nor changes the handle's
 * measured mapping choice.  bioik_solve_batch_bounded_submit is completed by bioik_solve_batch_wait.  The device form is capturable under the contract of
 * bioik_solve_batch_device (a linear chain, no memset node, one eager call of the same plan first); its two arrays are read by every launch of the call and must
 * stay valid and unchanged until the call's last kernel has run.  Not provided: bounds for the ranked entries and for bioik_solve_batch_multi. */
int bioik_solve_batch_bounded(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* seeds, const double* goal_params,
                              const double* var_lo /*[n][V]*/, const double* var_hi /*[n][V]*/, double* solutions, double* fitness, int32_t* success, int32_t* steps);
int bioik_solve_batch_bounded_submit(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* seeds, const double* goal_params,
                                     const double* var_lo, const double* var_hi, double* solutions, double* fitness, int32_t* success, int32_t* steps,
                                     uint64_t* ticket);
int bioik_solve_batch_bounded_device(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* d_seeds, const double* d_goal_params,
                                     const double* d_var_lo, const double* d_var_hi, double* d_solutions, double* d_fitness, int32_t* d_success,
                                     int32_t* d_steps, void* hip_stream);
/* The rule above in isolation (the device function the bounded kernels stage a query's table with, and nothing else): for n rows of bounds the six numbers of
 * every op of the problem's joint program, out [n][max(ops, 1)][6] = vmin, vmax, span, clip_min, clip_max, unbounded (0 / 1).  Host pointers. */
int bioik_eval_bounds(bioik_problem* p, size_t n, const double* var_lo, const double* var_hi, double* out);
/* the ops of the problem's joint program (the rows of bioik_eval_bounds): their number, and per op its robot variable and its index among the active variables
 * (-1: the op is no gene -- a mimic joint, a joint outside the group: its bounds are never changed) */
int bioik_problem_op_count(const bioik_problem* p);
int bioik_problem_op_variables(const bioik_problem* p, int32_t* variable /*[ops]*/, int32_t* gene /*[ops]*/);

/* RANKED SOLVES: the k best DISTINCT solutions of every query instead of the best one (MoveIt: the KinematicsBase::getPositionIK overload that fills a
 * std::vector<std::vector<double>>).  A query's islands are independent searches; each ends with a complete result, and where bioik_solve_batch keeps the
 * best island (reference src/ik_parallel.h:220-269) these entries rank all of them on the device and return the first k that differ:
 *   order     ik_parallel.h:220-269 read as a total order: the islands that passed come first, by ascending fitness (for a success that figure holds the
 *             secondary goals' term, exactly what the reference compares); then the islands that did not pass, by ascending fitness; ties go to the lower
 *             island index.  Row 0 is therefore the island bioik_solve_batch returns with the same parameters and island_sync = 0, bit for bit.
 *   distance  rows are taken greedily in that order: a row is kept iff, against EVERY row kept before it, the maximum over the problem's active variables of
 *             |a - b| is greater than min_distance (a plain IEEE difference, fabs and max: no wrapping modulo 2 pi).  min_distance < 0 keeps every row,
 *             min_distance = 0 drops only rows equal in every active variable.  Inactive variables are the seed's in every island and take no part.
 *   fill      per query the first min(k, kept) kept rows go to solutions [n][k][V], fitness [n][k], success [n][k], steps [n][k], and count [n] is their
 *             number; the rows from count to k - 1 hold the query's seed row, fitness +inf, success 0 and steps 0.  Every byte of the outputs is defined.
 * `params` as for bioik_solve_batch, with 1 <= k <= islands <= 64 and count != NULL (else BIOIK_ERR_INVALID_ARGUMENT, nothing launched, outputs untouched);
 * island_sync = 1 is refused the same way (islands that stop each other leave at timing-dependent steps: their individual results are not defined);
 * BIOIK_ISLANDS_AUTO resolves to max(k, what bioik_resolve_islands gives) with island_sync off.  Every solver mode, a timeout, bioik_problem_set_first_query.
 * The host form goes through the handle's page-locked arena under the handle's lock, as bioik_solve_batch.  The device form enqueues on `hip_stream` and
 * returns; it may be captured into a hipGraph under the contract of bioik_solve_batch_device (one eager call of the same plan first; a linear chain of
 * kernels, no memset node).  Neither takes nor changes the handle's measured mapping choice. */
int bioik_solve_batch_ranked(bioik_problem* p, const bioik_solve_params* params, size_t n, int32_t k, double min_distance, const double* seeds,
                             const double* goal_params, double* solutions /*[n][k][V]*/, double* fitness /*[n][k]*/, int32_t* success /*[n][k]*/,
                             int32_t* steps /*[n][k]*/, int32_t* count /*[n]*/);
int bioik_solve_batch_ranked_device(bioik_problem* p, const bioik_solve_params* params, size_t n, int32_t k, double min_distance, const double* d_seeds,
                                    const double* d_goal_params, double* d_solutions, double* d_fitness, int32_t* d_success, int32_t* d_steps,
                                    int32_t* d_count, void* hip_stream);

/* ---- function-level entry points (device-resident math exposed one function at a time so that
 *      each kernel can be parity-checked against the matching reference function) -------------- */

/* RobotFK_Fast_Base::applyConfiguration + getTipFrames (forward_kinematics.h:331-356) for n genotypes.
 *   seed [V] supplies the inactive variables; genes [n][D]; tip_frames [n][T][7].  Host pointers. */
int bioik_eval_fk(bioik_problem* p, size_t n, const double* seed, const double* genes, double* tip_frames);

/* Problem::computeGoalFitness over goals / secondary_goals (problem.cpp:244-257) with the phenotype from
 * exact FK (fk_mode = BIOIK_FK_EXACT) or from the linear extrapolation around `base_genes`
 * (fk_mode = BIOIK_FK_LINEAR; base_genes [D]).  One query's seed [V] and goal_params [P]; genes [n][D];
 * primary [n], secondary [n].  Host pointers. */
int bioik_eval_fitness(bioik_problem* p, int fk_mode, size_t n, const double* seed, const double* goal_params,
                       const double* base_genes, const double* genes, double* primary, double* secondary);

/* RobotFK_Mutator::initializeMutationApproximator (forward_kinematics.h:802-930): the per-(tip,gene) delta
 * frames around base_genes.  deltas [T][D][7] (dpx dpy dpz dqx dqy dqz dqw), tip_frames [T][7]. Host pointers. */
int bioik_eval_approximator(bioik_problem* p, const double* seed, const double* base_genes, double* tip_frames,
                            double* deltas);

/* IKEvolution2::reproduce (ik_evolution_2.cpp:242-326) with the counter-based RNG of DESIGN.md §4:
 * parents [2][2][D] (parent, {genes,gradients}, gene); out children_genes / children_gradients [population][D].
 * rng_key/species/generation select the random stream. Host pointers. */
int bioik_eval_reproduce(bioik_problem* p, int population, uint32_t rng_key, int species, uint32_t generation,
                         const double* parents, double* children_genes, double* children_gradients);

/* Problem::checkSolutionActiveVariables (problem.cpp:259-341) on the exact-FK pose of n genotypes. */
int bioik_eval_check(bioik_problem* p, const bioik_solve_params* params, size_t n, const double* seed,
                     const double* goal_params, const double* genes, int32_t* ok);

/* The migration rule of bioik_solve_params::island_migration on rows the caller supplies: exactly the kernel a solve runs at a boundary (k_migrate), under
 * BIOIK_FK_EXACT.  rows [n_queries][islands][bioik_problem_carry_doubles(p)], rewritten in place; live [n_queries][islands], non-zero = the island is live.
 * A ROW is what an unsolved island is between two steps, R = 9 M + 24 doubles with M = max(ops of the problem, 1):
 *   [0, 4M)       the species of rank 0: elite 0's genes [M], its gradient [M], elite 1's genes [M], its gradient [M]  (one value per op; untouched)
 *   [4M, 8M)      the species of rank 1, the same four blocks                                                        (WRITTEN in a recipient)
 *   [8M, 9M)      the island's solution, one value per op                                                            (READ in the donor)
 *   [9M, 9M + 24) bookkeeping: words 0-7 the species of rank 0 and 8-15 the species of rank 1 as (fitness, fitness of elite 0, of elite 1, id, slot, buffer,
 *                 improved, ok) -- words 9 and 10 are WRITTEN in a recipient --, 16 the step count, 17-19 scratch, 20 the solution's fitness (READ in every live
 *                 island: what donor and recipients are chosen by), 21 its success flag, 22-23 the deadline.
 * Every word not marked WRITTEN comes back unchanged, and so does every row of an island that is no recipient.  Host pointers. */
int bioik_problem_carry_doubles(const bioik_problem* p);
int bioik_eval_migrate(bioik_problem* p, int32_t islands, size_t n_queries, const int32_t* live /*[n_queries][islands]*/,
                       double* rows /*[n_queries][islands][carry_doubles], in place*/);

/* The shared arithmetic of both sides of the boundary, one function at a time on the device (bio_ik_amd/csrc/bioik_sincos.h, bioik_fused.h, bioik_acos.h -- the
 * headers the kernels and the test-suite's CPU checker both include): so that a test can hold them against an INDEPENDENT high-precision
 * reference (tests/test_arith_headers.py).  op / doubles in / doubles out per element:
 *   0 sincos        x                                      -> sin x, cos x           (reference: libm, src/forward_kinematics.h:89-112)
 *   1 qrot          q[4] v[3]                              -> q v q^-1                (frame.h:108-149)
 *   2 qmul          p[4] q[4]                              -> p (x) q                 (frame.h:151-172)
 *   3 dot3          a[3] b[3]   4 dot4  a[4] b[4]          -> a . b
 *   5 revolute      frame[7] half_angle cpos[3] ca[4] cb[4] pos_kind rot_kind pad  -> frame'[7] by the general form, frame'[7] by the sparse form
 *   6 acos          x                                      -> acos x                  (reference: tf2Acos -> libm, include/bio_ik/goal_types.h:183-212, 646-712)
 *   7 atan2         y x                                    -> atan2(y, x)             (reference: KDL::Rotation::GetRot -> libm, src/problem.cpp:281-321)
 *   8 sincos, voted x                                      -> sin x, cos x           (the chain walks' form: element i is lane i mod 64 of a wavefront that votes once on
 *                                                                                       "every |x| <= BIOIK_SINCOS_SMALL"; the same bits as 0 for every x)
 *   9 sincos, small x                                      -> sin x, cos x           (bioik_sincos_small: the same bits as 0 on |x| <= BIOIK_SINCOS_SMALL only)
 * Host pointers. */
int bioik_eval_arith(int device, int op, size_t n, const double* in, double* out);

/* BIOIK_SINCOS_DOMAIN (bio_ik_amd/csrc/bioik_sincos.h), a power of two: the shared sincos gives the same bits on the host and on the device for every double and is
 * accurate for |x| below this value; a line-search candidate with a joint value of this magnitude or more is no candidate (BIOIK_CANDIDATE_BOUND). */
double bioik_sincos_domain(void);

/* BIOIK_SINCOS_SMALL (bio_ik_amd/csrc/bioik_sincos.h), below pi / 4: where no lane of a wavefront holds a half angle beyond it, the chain walks evaluate the shared
 * sincos without its reduction and its quadrant step (the same bits). */
double bioik_sincos_small_bound(void);

/* streamed (unfused) generation: n_units (query,species) populations resident in HBM, layout
 * genes [n_units][D][population] (individual index fastest — coalesced), fitness [n_units][population].
 * One launch evaluates exact-FK fitness of every individual.  Used for the HBM-streamed measurement of
 * DESIGN.md §6; device pointers, enqueued on hip_stream. */
int bioik_stream_fitness_device(bioik_problem* p, size_t n_units, int population, const double* d_seeds,
                                const double* d_goal_params, const double* d_genes, double* d_fitness,
                                void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* BIOIK_HIP_H */
