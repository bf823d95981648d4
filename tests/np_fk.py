"""Independent forward kinematics in NumPy long double with ROTATION MATRICES (not quaternions), used to pin the
oracle's quaternion FK (SURVEY.md §4 "golden FK ... cross-checked against an independent restatement").
Follows the URDF/MoveIt definition directly: T_link = T_parent * T_origin * T_joint(q)."""
import numpy as np

LD = np.longdouble


def rot_from_quat(q):
    x, y, z, w = [LD(v) for v in q]
    n = np.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=LD)


def rot_axis_angle(axis, angle):
    a = np.asarray(axis, dtype=LD)
    a = a / np.sqrt(np.dot(a, a))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=LD)
    s, c = np.sin(LD(angle)), np.cos(LD(angle))
    return np.eye(3, dtype=LD) + s * K + (1 - c) * (K @ K)


def fk_all(model, variables):
    """global (R, p) of every link for one full variable vector."""
    v = np.asarray(variables, dtype=LD).copy()
    for j in range(model.n_links):  # mimic
        if model.joint_mimic[j] >= 0 and model.joint_first_variable[j] >= 0:
            src = model.joint_first_variable[model.joint_mimic[j]]
            v[model.joint_first_variable[j]] = v[src] * LD(model.joint_mimic_factor[j]) + LD(model.joint_mimic_offset[j])
    R = [None] * model.n_links
    p = [None] * model.n_links
    for l in range(model.n_links):
        o = model.link_origin[l]
        Ro, po = rot_from_quat(o[3:7]), np.asarray(o[0:3], dtype=LD)
        jt = model.joint_type[l]
        fv = model.joint_first_variable[l]
        Rj, pj = np.eye(3, dtype=LD), np.zeros(3, dtype=LD)
        if jt == 1:
            Rj = rot_axis_angle(model.joint_axis[l], v[fv])
        elif jt == 2:
            pj = np.asarray(model.joint_axis[l], dtype=LD) * v[fv]
        elif jt == 3:
            pj = v[fv:fv + 3]
            Rj = rot_from_quat(v[fv + 3:fv + 7])
        elif jt == 4:
            pj = np.array([v[fv], v[fv + 1], 0], dtype=LD)
            Rj = rot_axis_angle((0, 0, 1), v[fv + 2])
        Rl, pl = Ro @ Rj, po + Ro @ pj
        par = model.link_parent[l]
        if par >= 0:
            R[l] = R[par] @ Rl
            p[l] = p[par] + R[par] @ pl
        else:
            R[l], p[l] = Rl, pl
    return R, p


def quat_to_rot64(q):
    return np.asarray(rot_from_quat(q), dtype=np.float64)


def rot_from_quat_batch(q):
    """(n, 4) quaternions (x, y, z, w), any norm -> (n, 3, 3) rotation matrices of the normalised quaternions"""
    q = np.asarray(q, dtype=LD)
    q = q / np.sqrt(np.sum(q * q, axis=1, keepdims=True))
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def rot_axis_angle_batch(axis, angle):
    """unit axis (3,), angles (n,) -> (n, 3, 3): Rodrigues' formula"""
    a = np.asarray(axis, dtype=LD)
    a = a / np.sqrt(np.dot(a, a))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=LD)
    th = np.asarray(angle, dtype=LD)
    return np.eye(3, dtype=LD)[None] + np.sin(th)[:, None, None] * K[None] + (1 - np.cos(th))[:, None, None] * (K @ K)[None]


def mimic_resolved(model, variables):
    """the variable vectors with every mimic joint's variable set from the joint it follows (after MoveIt's resolution of chains of mimics)"""
    v = np.array(variables, dtype=LD, copy=True)
    for j in range(model.n_links):
        if model.joint_mimic[j] >= 0 and model.joint_first_variable[j] >= 0:
            m, f, o = model.joint_mimic[j], LD(model.joint_mimic_factor[j]), LD(model.joint_mimic_offset[j])
            while model.joint_mimic[m] >= 0:  # (a model whose chains are not resolved yet: x = f1 (f2 y + o2) + o1)
                f, o = f * LD(model.joint_mimic_factor[m]), o + f * LD(model.joint_mimic_offset[m])
                m = model.joint_mimic[m]
            v[..., model.joint_first_variable[j]] = v[..., model.joint_first_variable[m]] * f + o
    return v


def fk_batch(model, variables):
    """fk_all over a batch: variables (n, V) -> R (n_links, n, 3, 3), p (n_links, n, 3), the global frame of every link in long double"""
    v = mimic_resolved(model, np.atleast_2d(variables))
    n = v.shape[0]
    R = np.zeros((model.n_links, n, 3, 3), dtype=LD)
    p = np.zeros((model.n_links, n, 3), dtype=LD)
    for l in range(model.n_links):
        o = model.link_origin[l]
        Ro, po = rot_from_quat(o[3:7]), np.asarray(o[0:3], dtype=LD)
        jt = model.joint_type[l]
        fv = model.joint_first_variable[l]
        Rj, pj = np.broadcast_to(np.eye(3, dtype=LD), (n, 3, 3)), np.zeros((n, 3), dtype=LD)
        if jt == 1:
            Rj = rot_axis_angle_batch(model.joint_axis[l], v[:, fv])
        elif jt == 2:
            pj = np.asarray(model.joint_axis[l], dtype=LD)[None, :] * v[:, fv:fv + 1]
        elif jt == 3:
            pj = v[:, fv:fv + 3]
            Rj = rot_from_quat_batch(v[:, fv + 3:fv + 7])
        elif jt == 4:
            pj = np.stack([v[:, fv], v[:, fv + 1], np.zeros(n, dtype=LD)], axis=1)
            Rj = rot_axis_angle_batch((0, 0, 1), v[:, fv + 2])
        Rl = Ro[None] @ Rj
        pl = po[None] + pj @ Ro.T
        par = model.link_parent[l]
        if par >= 0:
            R[l] = R[par] @ Rl
            p[l] = p[par] + np.einsum("nij,nj->ni", R[par], pl)
        else:
            R[l], p[l] = Rl, pl
    return R, p


def quat_from_rot_batch(R):
    """(n, 3, 3) rotation matrices -> (n, 4) unit quaternions (x, y, z, w), w >= 0 where it can be (Shepperd's choice of the largest component)"""
    R = np.asarray(R, dtype=LD)
    n = R.shape[0]
    t = np.stack([R[:, 0, 0] - R[:, 1, 1] - R[:, 2, 2], -R[:, 0, 0] + R[:, 1, 1] - R[:, 2, 2], -R[:, 0, 0] - R[:, 1, 1] + R[:, 2, 2],
                  R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]], axis=1)
    k = np.argmax(t, axis=1)
    s = np.sqrt(1 + t[np.arange(n), k]) * 2
    d = lambda i, j: R[:, i, j]  # noqa: E731
    cand = np.stack([np.stack([s / 4, (d(0, 1) + d(1, 0)) / s, (d(0, 2) + d(2, 0)) / s, (d(2, 1) - d(1, 2)) / s], axis=1),
                     np.stack([(d(0, 1) + d(1, 0)) / s, s / 4, (d(1, 2) + d(2, 1)) / s, (d(0, 2) - d(2, 0)) / s], axis=1),
                     np.stack([(d(0, 2) + d(2, 0)) / s, (d(1, 2) + d(2, 1)) / s, s / 4, (d(1, 0) - d(0, 1)) / s], axis=1),
                     np.stack([(d(2, 1) - d(1, 2)) / s, (d(0, 2) - d(2, 0)) / s, (d(1, 0) - d(0, 1)) / s, s / 4], axis=1)], axis=0)
    return cand[k, np.arange(n)]
