"""numpy restatement of the depth supervision (csrc/pw_depth_sup.hip) and the accounting rule its tests use.

Two precisions side by side:
  * every DECISION (which pixel, kept or not, which depth, which bin) is restated in float32 in the reference's operation order
    -- `points.matmul(M.T)` as the k-ordered fma chain a BLAS sgemm runs on an FMA machine (fma32 below: the product of two
    float32 is exact in float64), then the rounded add of the translation, float32 divisions, rint -- and the winner of a pixel is
    the EXACT minimum;
  * the same projection in float64 gives every point's pre-rounding coordinates, which decide what may be EXCUSED: a float32
    pipeline cannot be asked to agree on a point that sits within 1e-3 px of a rounding threshold.
The loss (bce) is float64 throughout.  No torch, no reference code."""
import math

import numpy as np

f32 = np.float32
KEY_DIV = f32(100.0)


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _mm3(p, M, dtype):
    """rows of p (P,3) times M^T (M 3x3): float32 -> the sgemm chain, float64 -> plain"""
    if dtype == np.float64:
        return p.astype(np.float64) @ M.astype(np.float64).T
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    return fma32(z, M[None, :, 2], fma32(y, M[None, :, 1], x * M[None, :, 0]))


def project(points, l2i, post_rot, post_tran, dtype=f32):
    """loading.py:831-838 for one view: (P,3) columns (u, v, d) before the division by `downsample`"""
    p = points[:, :3].astype(dtype)
    l2i, post_rot, post_tran = l2i.astype(dtype), post_rot.astype(dtype), post_tran.astype(dtype)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        q = _mm3(p, l2i[:3, :3], dtype) + l2i[None, :3, 3]
        q = np.concatenate([q[:, :2] / q[:, 2:3], q[:, 2:3]], 1)
        return _mm3(q, post_rot, dtype) + post_tran[None]


def kept_pixels(uvd, h, w, ds, d0, d1):
    """points2depthmap's rounding and kept1 test in the dtype of uvd -> (kept mask, cx, cy as int64)"""
    dt = uvd.dtype.type
    with np.errstate(invalid='ignore'):
        cx, cy, d = np.rint(uvd[:, 0] / dt(ds)), np.rint(uvd[:, 1] / dt(ds)), uvd[:, 2]
        kept = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h) & (d < dt(f32(d1))) & (d >= dt(f32(d0)))
    cx, cy = np.where(kept, cx, 0).astype(np.int64), np.where(kept, cy, 0).astype(np.int64)
    return kept, cx, cy


def depth_maps(points, l2i, post_rot, post_tran, H, W, ds, d0, d1):
    """One sample.  Returns dict: maps (V,h,w) float32 exact minima (0 = nothing), cands: per view {flat pixel: sorted float32
    candidate depths}, uvd64 (V,P,3) float64 pre-rounding coordinates."""
    V, h, w = l2i.shape[0], H // ds, W // ds
    maps, cands, uvd64 = np.zeros((V, h, w), f32), [], []
    for v in range(V):
        uvd = project(points, l2i[v], post_rot[v], post_tran[v], f32)
        kept, cx, cy = kept_pixels(uvd, h, w, ds, d0, d1)
        flat, d = (cy * w + cx)[kept], uvd[kept, 2]
        order = np.lexsort((d, flat))
        flat, d = flat[order], d[order]
        first = np.ones(flat.shape[0], bool)
        first[1:] = flat[1:] != flat[:-1]
        maps[v].reshape(-1)[flat[first]] = d[first]
        starts = np.flatnonzero(first)
        cands.append({int(flat[s]): d[s:e] for s, e in zip(starts, list(starts[1:]) + [flat.shape[0]])})
        uvd64.append(project(points, l2i[v], post_rot[v], post_tran[v], np.float64))
    return dict(maps=maps, cands=cands, uvd64=np.stack(uvd64))


def bin_labels(m, d0, dstep, D):
    """view_transformer.py:757-771 on cell minima m (float32, 1e5 = nothing): int32 labels, -1 = the all-zero one-hot row"""
    sub = f32(float(d0) - float(dstep))
    g = (m.astype(f32) - sub) / f32(dstep)
    ok = (g < f32(D + 1)) & (g >= f32(0))
    return np.where(ok, g.astype(np.int64) - 1, -1).astype(np.int32)


def map_labels(gt, ds, d0, dstep, D):
    """get_downsampled_gt_depth on (V,H,W) -> (V,H/ds,W/ds) int32"""
    V, H, W = gt.shape
    g = gt.reshape(V, H // ds, ds, W // ds, ds).transpose(0, 1, 3, 2, 4).reshape(V, H // ds, W // ds, ds * ds)
    return bin_labels(np.where(g == 0, f32(1e5), g).min(-1), d0, dstep, D)


def near_threshold_mask(uvd64, h, w, ds, d0, d1, px_tol=1e-3, d_tol=1e-4):
    """(h,w) bool for one view: pixels touched by -- or next to one touched by -- a point whose float64 coordinate lies within
    px_tol (image pixels) of a rounding threshold (k + 0.5) ds, the image border thresholds being two of those, or whose depth
    is within d_tol relative of d0 or d1."""
    u, v, d = uvd64[:, 0], uvd64[:, 1], uvd64[:, 2]
    fin = np.isfinite(u) & np.isfinite(v) & np.isfinite(d)
    u, v, d = u[fin], v[fin], d[fin]

    def near(c):                                   # distance of c / ds to the nearest k + 0.5, in image pixels
        t = c / ds - 0.5
        return np.abs(t - np.rint(t)) * ds < px_tol
    d0, d1 = float(f32(d0)), float(f32(d1))
    inrange = (d > d0 * (1 - d_tol)) & (d < d1 * (1 + d_tol))
    hot = (((near(u) | near(v)) & inrange) | (np.abs(d - d0) <= d_tol * d0) | (np.abs(d - d1) <= d_tol * d1))
    mask = np.zeros((h, w), bool)
    cx, cy = np.rint(u[hot] / ds), np.rint(v[hot] / ds)
    for x, y in zip(cx, cy):
        if -2 < x < w + 1 and -2 < y < h + 1:
            mask[max(int(y) - 1, 0):int(y) + 2, max(int(x) - 1, 0):int(x) + 2] = True
    return mask


def key_tie_mask(cands, h, w):
    """(h,w) bool: multi-hit pixels whose two smallest candidates have the same float32 sort key rank + depth / 100
    (loading.py:778-779) -- the unstable argsort may keep either"""
    mask = np.zeros(h * w, bool)
    for flat, d in cands.items():
        if d.shape[0] > 1:
            k = f32(flat) + d[:2] / KEY_DIV
            mask[flat] = k[0] == k[1]
    return mask.reshape(h, w)


def account_maps(ref, R, h, w, ds, d0, d1):
    """The accounting rule.  ref (V,h,w): the map under test; R: depth_maps() of the same inputs.  Returns per view
    dict(excused, n_hit, n_excused, bad_single, bad_multi, bad_empty, not_candidate) -- n_excused counts EVERY excused pixel, the
    ones nothing lands on included (the 3 x 3 neighbourhood of a near-threshold point), n_hit the pixels something lands on; the
    bad_* are counts over NON-excused pixels, not_candidate over ALL pixels."""
    out = []
    for v in range(ref.shape[0]):
        exc = near_threshold_mask(R['uvd64'][v], h, w, ds, d0, d1) | key_tie_mask(R['cands'][v], h, w)
        want, got = R['maps'][v], ref[v]
        nhit = np.zeros(h * w, np.int64)
        for flat, d in R['cands'][v].items():
            nhit[flat] = d.shape[0]
        nhit = nhit.reshape(h, w)
        diff = (want.view(np.uint32) != got.view(np.uint32)) & ~exc
        notc = 0
        for flat in np.flatnonzero((got != want).reshape(-1)):
            c = R['cands'][v].get(int(flat))
            g = got.reshape(-1)[flat]
            notc += int(not ((c is not None and (c == g).any()) or (c is None and g == 0)))
        out.append(dict(excused=exc, n_hit=int((nhit > 0).sum()), n_excused=int(exc.sum()),
                        bad_single=int((diff & (nhit == 1)).sum()),
                        bad_multi=int((diff & (nhit > 1)).sum()), bad_empty=int((diff & (nhit == 0)).sum()), not_candidate=notc))
    return out


def excused_cells(exc, cell):
    h, w = exc.shape
    return exc.reshape(h // cell, cell, w // cell, cell).any((1, 3))


def bce(pred, labels, weight):
    """get_depth_loss in float64 on float32 predictions: pred (BN,D,h,w), labels (BN,h,w) -> (loss, d loss / d pred, n_fg)"""
    p = pred.astype(np.float64)
    BN, D = p.shape[:2]
    fg = labels >= 0
    y = np.zeros_like(p)
    bn, yy, xx = np.nonzero(fg)
    y[bn, labels[fg], yy, xx] = 1.0
    with np.errstate(divide='ignore'):
        lp, l1p = np.maximum(np.log(p), -100.0), np.maximum(np.log(1.0 - p), -100.0)
    elem = -(y * lp + (1.0 - y) * l1p) * fg[:, None]
    n = max(1, int(fg.sum()))
    grad = weight / n * (p - y) / np.maximum((1.0 - p) * p, 1e-12) * fg[:, None]
    return weight * elem.sum() / n, grad, int(fg.sum())


# ------------------------------------------------------------------------------------------------------- synthetic inputs
def _rot_z(a):
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])


def rot_to_quat(R):
    """(w, x, y, z) of a rotation matrix (trace branch chosen for conditioning)"""
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        return [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
    q = [0.0] * 4
    q[0], q[1 + i], q[1 + j], q[1 + k] = (R[k, j] - R[j, k]) / s, 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    return q


CAM_NAMES = ['CAM_FRONT_LEFT', 'CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_BACK_RIGHT', 'CAM_BACK', 'CAM_BACK_LEFT']


def synthetic_sweep(seed, n_beams=32, n_az=120, n_boxes=12, pts_per_box=60):
    """A lidar sweep in the lidar frame (sensor 1.84 m above the ground): ground returns on rings (beams at fixed elevations, so
    the far rings pass 45 m), returns on upright box faces, a few returns closer than 1 m and a sparse far wall.  (P,5) float32
    x y z intensity ring; all azimuths, so most points are behind any one camera."""
    rs = np.random.RandomState(seed)
    rows = []
    el = np.radians(np.linspace(-24.0, -1.6, n_beams))
    for b, e in enumerate(el):
        az = (np.arange(n_az) + rs.uniform(0, 1)) * (2 * math.pi / n_az) + rs.normal(0, 2e-3, n_az)
        r = 1.84 / math.tan(-e) * (1 + rs.normal(0, 4e-3, n_az))
        rows.append(np.stack([r * np.cos(az), r * np.sin(az), np.full(n_az, -1.84) + rs.normal(0, 0.02, n_az), rs.uniform(0, 1, n_az),
                              np.full(n_az, b)], 1))
    for _ in range(n_boxes):
        az0, r0, wdt, hgt = rs.uniform(0, 2 * math.pi), rs.uniform(4, 42), rs.uniform(1.5, 4.5), rs.uniform(1.2, 3.2)
        s, t = rs.uniform(-0.5, 0.5, pts_per_box) * wdt, rs.uniform(0, 1, pts_per_box) * hgt
        c = np.array([r0 * math.cos(az0), r0 * math.sin(az0)])
        tang = np.array([-math.sin(az0), math.cos(az0)])
        xy = c[None] + s[:, None] * tang[None]
        rows.append(np.concatenate([xy, (t - 1.84)[:, None], rs.uniform(0, 1, (pts_per_box, 1)), np.zeros((pts_per_box, 1))], 1))
    near = rs.uniform(-0.9, 0.9, (24, 3)) * [1, 1, 0.3] + [1.6, 0, -0.3]          # in front of the front camera, under 1 m from it
    far = np.stack([rs.uniform(46, 60, 80), rs.uniform(-30, 30, 80), rs.uniform(-1.5, 4, 80)], 1)
    for a in (near, far):
        rows.append(np.concatenate([a, rs.uniform(0, 1, (a.shape[0], 1)), np.zeros((a.shape[0], 1))], 1))
    pts = np.concatenate(rows, 0)
    return pts[rs.permutation(pts.shape[0])].astype(f32)


def image_aug(n_cams, H, W, resize, seed):
    """post_rots (N,3,3) / post_trans (N,3) of a resize + crop, with a horizontal flip on odd cameras and a small rotation about
    the crop centre on every third (the composition rule of the reference's image augmentation, restated)"""
    rs = np.random.RandomState(seed)
    prs, pts = [], []
    for c in range(n_cams):
        A, b = np.eye(2) * resize, np.zeros(2)
        newW, newH = int(1600 * resize), int(900 * resize)
        crop_x, crop_y = int((newW - W) * rs.uniform(0.3, 0.7)), newH - H
        b = b - np.array([crop_x, crop_y], np.float64)
        if c % 2 == 1:
            F, fb = np.array([[-1.0, 0], [0, 1]]), np.array([W, 0.0])
            A, b = F @ A, F @ b + fb
        if c % 3 == 0:
            a = math.radians(rs.uniform(-5.4, 5.4))
            Rm = np.array([[math.cos(a), math.sin(a)], [-math.sin(a), math.cos(a)]])
            ctr = np.array([W, H], np.float64) / 2
            A, b = Rm @ A, Rm @ (b - ctr) + ctr
        pr, pt = np.eye(3), np.zeros(3)
        pr[:2, :2], pt[:2] = A, b
        prs.append(pr)
        pts.append(pt)
    return np.stack(prs).astype(f32), np.stack(pts).astype(f32)


def synthetic_results(seed, H, W, resize, **sweep_kw):
    """The `results` dict PointToMultiViewDepth reads, as numpy: points, img_inputs pieces, cam_names, curr (quaternion poses:
    the 6-camera rig of preworld_amd.synth, a lidar mount, a global pose; the cameras' ego pose a few cm off the lidar's, as
    between two timestamps)."""
    from preworld_amd import synth as S
    rig = S.synthetic_rig(6, dtype=np.float64)
    ego_R, ego_t = _rot_z(math.radians(31.0)), np.array([412.5, 1103.25, 0.5])
    curr = dict(lidar2ego_rotation=rot_to_quat(_rot_z(math.radians(-1.5))), lidar2ego_translation=[0.94, 0.0, 1.84],
                ego2global_rotation=rot_to_quat(ego_R), ego2global_translation=list(ego_t), cams={})
    for i, name in enumerate(CAM_NAMES):
        s2e = rig['sensor2ego'][0, i]
        dR = _rot_z(math.radians(0.2 * (i - 2.5)))
        curr['cams'][name] = dict(sensor2ego_rotation=rot_to_quat(s2e[:3, :3]), sensor2ego_translation=list(s2e[:3, 3]),
                                  ego2global_rotation=rot_to_quat(dR @ ego_R),
                                  ego2global_translation=list(ego_t + ego_R @ np.array([0.05 * (i - 2.5), 0.01 * i, 0.0])))
    post_rots, post_trans = image_aug(6, H, W, resize, seed + 1)
    return dict(points=synthetic_sweep(seed, **sweep_kw), intrins=rig['intrin'][0].astype(f32), post_rots=post_rots,
                post_trans=post_trans, cam_names=list(CAM_NAMES), curr=curr, image_hw=(H, W))
