"""numpy (float32) restatement of what pw_render_views / pw_render_label_views define, for the tests: the pixel -> ray mapping
(mmdet3d/datasets/ray.py:34-45 as pts2ray calls it, :50), the sample positions and inner | cumdist mask of
nerf_head.py:32-55,197-199, and LABEL MODE as include/preworld_hip.h states it:

  same rays, same sample positions, same mask; a sample's voxel is floor(u + 0.5) per axis with u the continuous index of the
  align_corners=True mapping (outside the grid = miss); the first kept sample whose label is not empty_idx is the hit:
  cls = label, depth = (s_hit + 1e-7) radius with s = 1 - 1/(1+t), alphainv_last = 0; no hit: cls = empty_idx,
  depth = 1e-7 radius, alphainv_last = 1.

consts: the 27 floats of NerfHead.consts() (center[3], radius[3], bda[9], xyz_min[3], xyz_max[3], bg_len, act_shift, interval,
dist_thres, fast_thres, depth_scale)."""
import numpy as np

F = np.float32


def pixel_rays(K, c2w, hw, stride=1, origin=(0, 0)):
    """(V,H,W,9) float32 rows [rays_o, rays_d, viewdirs]: output pixel (i, j) looks through source pixel
    x = origin[0] + j stride, y = origin[1] + i stride, at its centre (+0.5)"""
    K, c2w = np.asarray(K, F), np.asarray(c2w, F)
    H, W = hw
    x = (origin[0] + np.arange(W) * stride).astype(F)[None, :] + np.zeros((H, 1), F)
    y = (origin[1] + np.arange(H) * stride).astype(F)[:, None] + np.zeros((1, W), F)
    out = np.zeros((K.shape[0], H, W, 9), F)
    for v in range(K.shape[0]):
        d0 = ((x + F(0.5)) - K[v, 0, 2]) / K[v, 0, 0]
        d1 = ((y + F(0.5)) - K[v, 1, 2]) / K[v, 1, 1]
        R = c2w[v, :3, :3]
        rd = np.stack([(d0 * R[k, 0] + d1 * R[k, 1]) + F(1) * R[k, 2] for k in range(3)], -1).astype(F)
        nrm = np.sqrt((rd[..., 0] * rd[..., 0] + rd[..., 1] * rd[..., 1]) + rd[..., 2] * rd[..., 2])
        out[v, ..., 0:3] = c2w[v, :3, 3]
        out[v, ..., 3:6] = rd
        out[v, ..., 6:9] = rd / nrm[..., None]
    return out


def sample_points(rays_o, rays_d, consts, t):
    """(R,S,3) float32 sample positions after contraction and bda, the (R,S) inner | cumdist mask, and (R,S) flags of samples whose
    mask decision is within 1e-6 of flipping (|norm - 1| or |cum - dist_thres|)"""
    c = np.asarray(consts, F)
    center, radius, bda, bg_len, thres = c[0:3], c[3:6], c[6:15].reshape(3, 3), c[21], c[24]
    t = np.asarray(t, F)
    o = (np.asarray(rays_o, F) - center) / radius
    rd = np.asarray(rays_d, F)
    nn = np.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2])
    d = rd / nn[:, None]
    q = o[:, None, :] + d[:, None, :] * t[None, :, None]                           # (R,S,3)
    norm = np.sqrt((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2])
    inner = norm <= F(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        sc = (F(1) + bg_len) - bg_len / norm
        qo = q / norm[..., None] * sc[..., None]
    q = np.where(inner[..., None], q, qo).astype(F)
    p = np.zeros_like(q)
    for k in range(3):
        p[..., k] = ((F(0) + bda[k, 0] * q[..., 0]) + bda[k, 1] * q[..., 1]) + bda[k, 2] * q[..., 2]
    e = p[:, 1:] - p[:, :-1]
    dist = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(F)
    mask = inner.copy()
    close = np.abs(norm - F(1)) < 1e-6
    cum = np.zeros(len(o), F)
    for s in range(1, len(t)):                                                     # ub360_utils_kernel.cu:13-32
        cum = (cum + dist[:, s - 1]).astype(F)
        over = cum > thres
        close[:, s] |= np.abs(cum - thres) < 1e-6
        cum = cum * (~over).astype(F)
        mask[:, s] |= over
    return p, mask, close


def voxel_index(p, consts, shape):
    """continuous voxel index u (…,3) of positions p for a grid of `shape` = (X,Y,Z): grid_sample's align_corners=True mapping"""
    c = np.asarray(consts, F)
    lo, hi = c[15:18], c[18:21]
    g = ((p - lo) / (hi - lo)) * F(2) - F(1)
    return (((g + F(1)) / F(2)) * (np.asarray(shape, F) - F(1))).astype(F)


def label_views(labels, rays_o, rays_d, consts, t, empty_idx=17, shift=None, flip_close=False):
    """LABEL MODE on R rays.  labels: uint8 (X,Y,Z).  Returns cls uint8 (R), depth float32 (R), alphainv_last float32 (R), the hit's
    sample index (R, -1 = none), and `fragile` (R): some sample up to the hit lies within 1e-4 voxel of a voxel face with another
    label behind it, or sits in a non-empty voxel within 1e-6 of the unit-sphere / cumdist decision -- there a float32 evaluation
    in another order may pick the neighbouring answer.  shift (3 floats, voxels) moves every continuous index and flip_close inverts
    the mask decision of the samples within 1e-6 of flipping: label_alternatives uses them to enumerate the neighbouring answers."""
    c = np.asarray(consts, F)
    t = np.asarray(t, F)
    p, mask, close = sample_points(rays_o, rays_d, consts, t)
    if flip_close:
        mask = mask ^ close
    u = voxel_index(p, consts, labels.shape) + F(0.5)
    if shift is not None:
        u = (u + np.asarray(shift, F)).astype(F)
    idx = np.floor(u)
    shape = np.asarray(labels.shape, F)
    inb = np.isfinite(u).all(-1) & (idx >= 0).all(-1) & (idx < shape).all(-1)
    ii = np.where(inb[..., None], idx, 0).astype(np.int64)
    lab = labels[ii[..., 0], ii[..., 1], ii[..., 2]]
    occ = mask & inb & (lab != empty_idx)
    any_hit = occ.any(1)
    first = np.where(any_hit, occ.argmax(1), -1)
    R = len(first)
    r = np.arange(R)
    s_hit = F(1) - F(1) / (F(1) + t[np.maximum(first, 0)])
    cls = np.where(any_hit, lab[r, np.maximum(first, 0)], empty_idx).astype(np.uint8)
    depth = ((np.where(any_hit, s_hit, F(0)).astype(F) + F(1e-7)) * c[26]).astype(F)
    last = np.where(any_hit, F(0), F(1)).astype(F)
    upto = np.arange(len(t))[None, :] <= np.where(any_hit, first, len(t))[:, None]
    # a sample within 1e-4 voxel of a face matters only if the voxel across that face holds another label (else both answers are
    # the same answer); one whose mask decision is within 1e-6 of flipping only if its voxel is not empty
    lab_e = np.where(inb, lab, empty_idx)
    near = np.abs(u - np.round(u)) < 1e-4                                          # (R,S,3)
    differs = near.sum(-1) >= 2
    for ax in range(3):
        alt = idx.copy()
        alt[..., ax] = np.where(u[..., ax] - idx[..., ax] < 0.5, idx[..., ax] - 1, idx[..., ax] + 1)
        ok = np.isfinite(u).all(-1) & (alt >= 0).all(-1) & (alt < shape).all(-1)
        ai = np.where(ok[..., None], alt, 0).astype(np.int64)
        alab = np.where(ok, labels[ai[..., 0], ai[..., 1], ai[..., 2]], empty_idx)
        differs |= near[..., ax] & (alab != lab_e)
    fragile = (((differs & mask) | (close & (lab_e != empty_idx))) & upto).any(1)
    return cls, depth, last, first, fragile


def clear_scene(seed):
    """The class-map scene: the geometry of synth.render_grids_mixed (ground slab + boxes, free space transparent) with a semantic
    field that has a clear per-voxel winner which is constant over large regions -- a ground voxel carries class (5 (x // 8) + 3 (y // 8)) % 17 (3.2 m tiles), a box voxel
    class 1 + (x // 25 + 3 (y // 25)) % 10, free space class 16 -- the winner at +6 over N(0, 0.3) noise on the other channels.
    A rendered pixel is then a near-tie only where a ray splits its weight evenly between two regions.
    Returns density (X,Y,Z), semantic (X,Y,Z,17), color (X,Y,Z,3) float32."""
    from preworld_amd import synth as S
    density, _, color = S.render_grids_mixed(seed)
    X, Y, Z = density.shape
    rs = np.random.RandomState(seed + 7)
    semantic = (rs.standard_normal((X, Y, Z, 17)) * 0.3).astype(F)
    xs, ys = np.meshgrid(np.arange(X), np.arange(Y), indexing='ij')
    win = np.broadcast_to((1 + (xs // 25 + 3 * (ys // 25)) % 10)[:, :, None], (X, Y, Z)).copy()
    win[:, :, :2] = ((5 * (xs // 8) + 3 * (ys // 8)) % 17)[:, :, None]
    win[density <= 8.5] = 16
    np.put_along_axis(semantic, win[..., None], F(6), -1)
    return density, semantic, color


def clear_rig():
    """two cameras pitched 30 deg down with a +-20 deg vertical field of view: every ray meets the ground slab or a box within ~10 m.
    Returns K (2,3,3), c2w (2,4,4) float32."""
    from preworld_amd import synth as S
    s2e = S.synthetic_rig(6, dtype=np.float64)['sensor2ego'][0]
    out = []
    for cam, pitch, yaw in ((1, 30.0, 15.0), (3, 33.0, -10.0)):
        p, y = np.radians(pitch), np.radians(yaw)
        Rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
        Ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
        a = s2e[cam].copy()
        a[:3, :3] = a[:3, :3] @ Ry @ Rx.T
        out.append(a)
    K = np.array([[[41.0, 0, 23.7], [0, 40.0, 16.2], [0, 0, 1]], [[44.5, 0, 21.3], [0, 43.0, 17.9], [0, 0, 1]]], F)
    return K, np.stack(out).astype(F)


def label_alternatives(labels, rays_o, rays_d, consts, t, empty_idx=17):
    """the neighbouring answers of a fragile pixel: (cls, depth, alphainv_last) with every continuous index moved by +-1e-4 voxel
    along one axis, and with the near-flipping mask decisions inverted.  Returns a list of 7 (cls, depth, last) triples."""
    out = []
    for ax in range(3):
        for sg in (-1e-4, 1e-4):
            sh = [0.0, 0.0, 0.0]
            sh[ax] = sg
            out.append(label_views(labels, rays_o, rays_d, consts, t, empty_idx, shift=sh)[:3])
    out.append(label_views(labels, rays_o, rays_d, consts, t, empty_idx, flip_close=True)[:3])
    return out
