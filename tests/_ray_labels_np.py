"""Numpy restatement of the pre-train ray supervision (csrc/pw_ray_labels.hip): stage A, lidar sweep -> per-camera point lists
(tools/gen_data/gen_depth_gt.py / gen_seg_gt_from_lidarseg.py, map_pointcloud_to_image), and stage B, lists + frames -> the
(R, 16) ray table and its sampling weights (nuscenes_dataset_occ.py load_depth / load_seg_label / get_rays, ray.py).  No torch,
no reference code.  Every cast is spelled out, so NumPy 1.x and 2.x give the same bits (a float32 array plus a float64 scalar
stays float32 under 1.x and is promoted under 2.x: nothing here relies on either).

THE ROUNDING RULE OF STAGE A is defined here and nowhere else.  The devkit keeps the cloud as a float32 array, so each of the
eight rigid sub-steps ends in a rounding to float32: a rotation is the float64 product (r0 x + r1 y) + r2 z, rounded; a
translation is a float32 add of the translation rounded to float32.  Pixel and mask are float64.  This is a reading of the
devkit (nuscenes / pyquaternion are not installable here), not a recording of it.

`project_ideal` is the same projection as ONE float64 4x4 chain with no intermediate rounding."""
import numpy as np

F32, F64 = np.float32, np.float64
MEAN = np.array([0.485, 0.456, 0.406], F32)
STD = np.array([0.229, 0.224, 0.225], F32)
POSE_DOUBLES = 57


def quat_matrix(q):
    """pyquaternion's Quaternion(q).rotation_matrix (w, x, y, z), float64"""
    w, x, y, z = [float(v) for v in q]
    n = np.sqrt(np.dot([w, x, y, z], [w, x, y, z]))
    if abs(1.0 - n) > 1e-14 and n > 0:
        w, x, y, z = w / n, x / n, y / n, z / n
    Q = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])
    Qb = np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])
    return np.dot(Q, Qb.conj().transpose())[1:][:, 1:]


def yaw_quat(yaw, tilt=0.0):
    """a rotation about z by yaw after a small rotation about x by tilt, as (w, x, y, z)"""
    a = np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
    b = np.array([np.cos(tilt / 2), np.sin(tilt / 2), 0, 0])
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return [w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
            w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2]


def rot_to_quat(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    x, y, z = np.copysign(x, R[2, 1] - R[1, 2]), np.copysign(y, R[0, 2] - R[2, 0]), np.copysign(z, R[1, 0] - R[0, 1])
    return [float(w), float(x), float(y), float(z)]


# ------------------------------------------------------------------------------------------------------------ stage A
def view_pose(info, cam):
    """the 57 doubles of one view: R1 t1 (lidar->ego) R2 t2 (ego->global) | -t3 R3^T (global->camera ego) -t4 R4^T (camera
    ego->camera) | K.  info: the sweep's sample (lidar2ego_*, ego2global_*), cam: one of its cams entries."""
    parts = [quat_matrix(info['lidar2ego_rotation']).ravel(), np.array(info['lidar2ego_translation'], F64),
             quat_matrix(info['ego2global_rotation']).ravel(), np.array(info['ego2global_translation'], F64),
             -np.array(cam['ego2global_translation'], F64), quat_matrix(cam['ego2global_rotation']).T.ravel(),
             -np.array(cam['sensor2ego_translation'], F64), quat_matrix(cam['sensor2ego_rotation']).T.ravel(),
             np.array(cam['cam_intrinsic'], F64).ravel()]
    out = np.concatenate(parts)
    assert out.shape == (POSE_DOUBLES,)
    return out


def view_poses(infos, cam_names):
    return np.stack([view_pose(info, info['cams'][name]) for info in infos for name in cam_names])


def _rot(R, p):
    x, y, z = [p[:, k].astype(F64) for k in range(3)]
    R = np.asarray(R, F64).reshape(3, 3)
    return np.stack([((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z).astype(F32) for r in range(3)], 1)


def _tran(t, p):
    t32 = np.asarray(t, F64).astype(F32)
    return np.stack([p[:, k] + t32[k] for k in range(3)], 1).astype(F32)       # float32 + float32 scalar: float32 in 1.x and 2.x


def project(points, pose, H, W):
    """-> keep (P,) bool, uvd (P,3) float32 = (u, v, depth) as the gen tools write them"""
    p = np.ascontiguousarray(points[:, :3], F32)
    assert p.dtype == F32
    P = np.asarray(pose, F64)
    p = _rot(P[0:9], p)
    p = _tran(P[9:12], p)
    p = _rot(P[12:21], p)
    p = _tran(P[21:24], p)
    p = _tran(P[24:27], p)
    p = _rot(P[27:36], p)
    p = _tran(P[36:39], p)
    p = _rot(P[39:48], p)
    assert p.dtype == F32
    K = P[48:57].reshape(3, 3)
    X, Y, Z = [p[:, k].astype(F64) for k in range(3)]
    with np.errstate(all='ignore'):
        pw = (K[2, 0] * X + K[2, 1] * Y) + K[2, 2] * Z
        u = ((K[0, 0] * X + K[0, 1] * Y) + K[0, 2] * Z) / pw
        v = ((K[1, 0] * X + K[1, 1] * Y) + K[1, 2] * Z) / pw
        keep = (p[:, 2] > F32(0)) & (u > 1.0) & (u < float(W - 1)) & (v > 1.0) & (v < float(H - 1))
        uvd = np.stack([u.astype(F32), v.astype(F32), p[:, 2]], 1)
    return keep, uvd


def chain_ideal(pose):
    """lidar -> camera as one float64 4x4 from the UNROUNDED poses"""
    P = np.asarray(pose, F64)

    def m(R, t_after=None, t_before=None):
        M = np.eye(4)
        M[:3, :3] = R.reshape(3, 3)
        if t_after is not None:
            M[:3, 3] = t_after
        if t_before is not None:
            M[:3, 3] = M[:3, :3] @ t_before
        return M
    return m(P[39:48], t_before=P[36:39]) @ m(P[27:36], t_before=P[24:27]) @ m(P[12:21], t_after=P[21:24]) @ m(P[0:9], t_after=P[9:12])


def project_ideal(points, pose):
    """-> u, v, depth float64, no intermediate rounding"""
    P = np.asarray(pose, F64)
    M = chain_ideal(P)
    p = np.asarray(points[:, :3], F64) @ M[:3, :3].T + M[:3, 3]
    K = P[48:57].reshape(3, 3)
    with np.errstate(all='ignore'):
        q = p @ K.T
        return q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], p[:, 2]


def stage_a(points, labels, lut, poses, N, H, W):
    """points: list of T (P_t, >= 3) float32 sweeps, labels: list of T uint8 arrays, lut uint8[256], poses (T N, 57).
    -> depth lists, seg lists (one (n_v, 3) float32 array per view, sweep order), both as the gen tools' .bin files hold them"""
    depth_lists, seg_lists = [], []
    lut = np.asarray(lut, np.uint8)
    for v in range(len(poses)):
        t = v // N
        keep, uvd = project(points[t], poses[v], H, W)
        cls = lut[np.asarray(labels[t], np.uint8)].astype(F32)
        depth_lists.append(np.ascontiguousarray(uvd[keep]))
        seg_lists.append(np.ascontiguousarray(np.stack([uvd[keep, 0], uvd[keep, 1], cls[keep]], 1)))
    return depth_lists, seg_lists


def offsets(lists):
    return np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ stage B
def view_labels(depth_list, seg_list, frame, H, W, fancy=False):
    """load_depth / load_seg_label / the gathers of get_rays for one view -> coor (n,2) f32, depth, seg, img (n,3) f32.
    fancy=True writes the map with one fancy assignment as the reference does (numpy keeps the last of repeated indices; the
    loop spells that out and is the definition here)"""
    coor = depth_list[:, :2].astype(np.int16)
    scoor = seg_list[:, :2].astype(np.int16)
    seg_map = np.zeros((H, W), F64)
    if fancy:
        seg_map[scoor[:, 1], scoor[:, 0]] = seg_list[:, 2]
    for k in range(0 if fancy else len(seg_list)):       # in list order: the last point of a pixel stays
        seg_map[scoor[k, 1], scoor[k, 0]] = seg_list[k, 2]
    seg = seg_map[coor[:, 1], coor[:, 0]].astype(F32)
    px = frame[coor[:, 1], coor[:, 0]].astype(F32)        # uint8 -> float32, exact
    img = ((px / F32(255.0)) - MEAN[None]) / STD[None]
    assert img.dtype == F32
    return coor.astype(F32), depth_list[:, 2].astype(F32), seg, img


def pts2ray(coor, depth, seg, img, c2w, K):
    """ray.py:34-56 in float32, products and sums in k_pts2ray's order"""
    c2w, K = np.asarray(c2w, F32), np.asarray(K, F32)
    d0 = ((coor[:, 0] + F32(0.5)) - K[0, 2]) / K[0, 0]
    d1 = ((coor[:, 1] + F32(0.5)) - K[1, 2]) / K[1, 1]
    d2 = np.ones_like(d0)
    rd = np.stack([(d0 * c2w[k, 0] + d1 * c2w[k, 1]) + d2 * c2w[k, 2] for k in range(3)], 1)
    nrm = np.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2])
    ro = np.broadcast_to(c2w[:3, 3][None], rd.shape)
    out = np.concatenate([coor, depth[:, None], seg[:, None], ro, rd, rd / nrm[:, None], img], 1)
    assert out.dtype == F32
    return out


def stage_b(depth_lists, seg_lists, frames, view_frame, c2w, K, H, W):
    """-> table (R, 16) float32, rows in view order then list order"""
    rows = []
    for v in range(len(depth_lists)):
        f = v if view_frame is None else int(view_frame[v])
        rows.append(pts2ray(*view_labels(depth_lists[v], seg_lists[v], frames[f], H, W), c2w[v], K[v]))
    return np.concatenate(rows, 0) if rows else np.zeros((0, 16), F32)


def class_counts(table, n_cls=17):
    return np.array([(table[:, 3] == F32(c)).sum() for c in range(n_cls)], np.int64)


def batch_balance(counts):
    """exp(0.005 * (class_nums.max() / class_nums - 1)) with class_nums float32; the exponential is the correctly rounded float32
    one (float64 exp, rounded), which the kernel computes the same way"""
    n = counts.astype(F32)
    with np.errstate(all='ignore'):
        arg = F32(0.005) * (n.max() / n - F32(1.0))
        return np.exp(arg.astype(F64)).astype(F32)


def weights(table, view_off, frame_ids, dynamic_class, balance_weight=None, weight_adj=0.3, weight_dyn=0.0, n_cls=17):
    """ray.py:93-112"""
    bw = batch_balance(class_counts(table, n_cls)) if balance_weight is None else np.asarray(balance_weight, F32)
    w = np.zeros(len(table), F32)
    for v in range(len(view_off) - 1):
        a, b = int(view_off[v]), int(view_off[v + 1])
        c = table[a:b, 3]
        wt = np.full(b - a, F32(1.0 if frame_ids[v] == 0 else weight_adj), F32)
        if frame_ids[v] != 0:
            wt[np.isin(c, np.asarray(dynamic_class, F32))] = F32(weight_dyn)
        w[a:b] = bw[np.clip(c.astype(np.int64), 0, n_cls - 1)] * wt
    return w


def sensor2keyegos_f64(infos, cam_names):
    """inverse(keyego2global) @ ego2global @ sensor2ego per view from the quaternions, all float64 (the reference rounds the
    4x4 poses to float32 first)"""
    def pose(r, t):
        M = np.eye(4)
        M[:3, :3] = quat_matrix(r)
        M[:3, 3] = t
        return M
    out = []
    for info in infos:
        for n in cam_names:
            cam, key = info['cams'][n], infos[0]['cams'][n]
            out.append(np.linalg.inv(pose(key['ego2global_rotation'], key['ego2global_translation'])) @
                       pose(cam['ego2global_rotation'], cam['ego2global_translation']) @
                       pose(cam['sensor2ego_rotation'], cam['sensor2ego_translation']))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------------------ synthetic samples
LUT = ((np.arange(256) * 7 + 3) % 17).astype(np.uint8)          # a stand-in lidarseg byte -> class table (all 17 classes)
CAM2EGO = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])      # camera (x right, y down, z ahead) -> ego


def synthetic_infos(seed, T, N, H, W, focal, scenes=None):
    """T info dicts of one drive at nuScenes magnitudes: the ego ~1e3 m from the map origin, moving ~4 m per frame; N cameras
    spread over the azimuth; the cameras' own ego poses a little off the lidar's (another timestamp)."""
    rs = np.random.RandomState(seed)
    base = np.array([1010.0 + 600 * rs.rand(), 640.0 + 500 * rs.rand(), 0.3 * rs.rand()])
    yaw0 = rs.uniform(-np.pi, np.pi)
    infos = []
    for t in range(T):
        yaw = yaw0 + 0.03 * t
        pos = base + 4.1 * t * np.array([np.cos(yaw0), np.sin(yaw0), 0.0]) + 0.01 * rs.randn(3)
        info = dict(scene_token='scene-%s' % (scenes[t] if scenes else 0), token='sample-%d-%d' % (seed, t),
                    lidar2ego_rotation=yaw_quat(-np.pi / 2 + 0.004, 0.002), lidar2ego_translation=[0.943713, 0.0, 1.84023],
                    ego2global_rotation=yaw_quat(yaw, 0.003 * rs.randn()), ego2global_translation=list(pos), cams={})
        for c in range(N):
            cyaw = 2 * np.pi * c / N + 0.02 * rs.randn()
            Rc = quat_matrix(yaw_quat(cyaw, 0.0)) @ CAM2EGO
            dpos = pos + np.array([0.25, 0.1, 0.0]) * rs.rand(3)
            info['cams']['CAM_%d' % c] = dict(
                data_path='samples/CAM_%d/%d_%d.jpg' % (c, seed, t),
                sensor2ego_rotation=rot_to_quat(Rc), sensor2ego_translation=[1.5 * np.cos(cyaw), 0.5 * np.sin(cyaw), 1.51],
                ego2global_rotation=yaw_quat(yaw + 0.002 * rs.randn(), 0.003 * rs.randn()), ego2global_translation=list(dpos),
                cam_intrinsic=[[focal, 0.0, W / 2 + 0.37], [0.0, focal, H / 2 - 0.21], [0.0, 0.0, 1.0]])
        infos.append(info)
    return infos


def synthetic_sweep(rs, P, border=None):
    """P points all around the lidar, 2 .. 50 m away (so some are behind every camera, some at depth <= 0).  border =
    (poses of the sweep's views, H, W, n): per view, n points placed 0.15 .. 0.9 px on either side of each of the four mask
    thresholds at 20 .. 40 m depth (back-projected through the ideal chain) replace the first rows."""
    r = rs.uniform(2.0, 50.0, P)
    az = rs.uniform(-np.pi, np.pi, P)
    pts = np.stack([r * np.cos(az), r * np.sin(az), rs.uniform(-2.2, 4.0, P), rs.uniform(0, 255, P), np.zeros(P)], 1)
    if border is not None:
        poses, H, W, n = border
        k = 0
        for pose in poses:
            Minv = np.linalg.inv(chain_ideal(pose))
            Kinv = np.linalg.inv(np.asarray(pose[48:57], F64).reshape(3, 3))
            for axis, thr in ((0, 1.0), (0, W - 1.0), (1, 1.0), (1, H - 1.0)):
                for _ in range(n):
                    uv = np.array([rs.uniform(3, W - 3), rs.uniform(3, H - 3)])
                    uv[axis] = thr + rs.choice([-1, 1]) * rs.uniform(0.15, 0.9)
                    d = rs.uniform(20.0, 40.0)
                    cam = Kinv @ np.array([uv[0] * d, uv[1] * d, d])
                    pts[k, :3] = Minv[:3, :3] @ cam + Minv[:3, 3]
                    k += 1
    return pts.astype(F32)


def synthetic_sample(seed, T=2, N=2, P=3001, H=48, W=80, focal=40.0, border=0, scenes=None, lengths=None):
    """-> dict(infos, cam_names, points [T], labels [T] uint8, frames (T N, H, W, 3) uint8, poses (T N, 57), H, W, N)"""
    rs = np.random.RandomState(seed + 1000)
    infos = synthetic_infos(seed, T, N, H, W, focal, scenes)
    names = list(infos[0]['cams'].keys())
    poses = view_poses(infos, names)
    points, labels = [], []
    for t in range(T):
        n = P if lengths is None else lengths[t]
        points.append(synthetic_sweep(rs, n, (poses[t * N:(t + 1) * N], H, W, border) if border else None))
        labels.append(rs.randint(0, 32, n).astype(np.uint8))
    frames = rs.randint(0, 256, (T * N, H, W, 3)).astype(np.uint8)
    return dict(infos=infos, cam_names=names, points=points, labels=labels, frames=frames, poses=poses, H=H, W=W, N=N)


def camera_tables(infos, cam_names):
    """c2w (V,4,4) float32 as the reference composes it (float32 poses, float64 products, float32) and K (V,3,3) float32"""
    def pose32(r, t):
        M = np.eye(4, dtype=F32)
        M[:3, :3] = quat_matrix(r)
        M[:3, 3] = np.asarray(t, F64)
        return M
    c2w, K = [], []
    for info in infos:
        for n in cam_names:
            cam, key = info['cams'][n], infos[0]['cams'][n]
            g = np.linalg.inv(pose32(key['ego2global_rotation'], key['ego2global_translation']).astype(F64))
            c2w.append((g @ pose32(cam['ego2global_rotation'], cam['ego2global_translation']).astype(F64) @
                        pose32(cam['sensor2ego_rotation'], cam['sensor2ego_translation']).astype(F64)).astype(F32))
            K.append(np.asarray(cam['cam_intrinsic'], F64).astype(F32))
    return np.stack(c2w), np.stack(K)
