"""Numpy restatement of the image side of the reference's PrepareImageInputs (mmdet3d/datasets/pipelines/loading.py:955-962
img_transform_core: PIL resize -> crop -> flip -> rotate; loading_traj_temporal.py:173-180 mmlabNormalize), vectorised, plus the
synthetic frames and info dicts the image-prep tests and tools/gen_golden_images.py share.

The uint8 stage restates Pillow's C (Resample.c precompute_coeffs / normalize_coeffs_8bpc / the 8 bpc passes, Geometry.c
affine_fixed, Image.rotate) in integers; tests/test_image_prep_cpu.py checks it byte for byte against the installed Pillow."""
import math

import numpy as np

PRECISION_BITS = 22
MEAN32 = np.array([123.675, 116.28, 103.53], np.float32)
STDINV32 = (1.0 / np.array([58.395, 57.12, 57.375], np.float32).astype(np.float64)).astype(np.float32)


def bicubic(x):
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def axis_table(n_in, n_out):
    """-> bounds (n_out, 2) int32 [first source index, tap count], coefs (n_out, ksize) int32.  n_in == n_out: PIL skips the
    pass, here the identity table."""
    if n_in == n_out:
        return (np.stack([np.arange(n_out), np.ones(n_out, np.int64)], 1).astype(np.int32),
                np.full((n_out, 1), 1 << PRECISION_BITS, np.int32))
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(n_out) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)
    hi = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    n = hi - lo
    w = np.zeros((n_out, ksize))
    ww = np.zeros(n_out)
    for k in range(ksize):                                   # the running sum in tap order, as the C loop forms it
        wk = np.where(k < n, bicubic((k + lo - center + 0.5) * ss), 0.0)
        w[:, k] = wk
        ww = ww + wk
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    q = w * float(1 << PRECISION_BITS)
    coefs = np.where(w < 0, np.trunc(-0.5 + q), np.trunc(0.5 + q)).astype(np.int32)
    return np.stack([lo, n], 1).astype(np.int32), coefs


def _pass(img, bounds, coefs, axis):
    """one 8 bpc pass along `axis` (0 rows, 1 columns) of img (H, W, 3) uint8"""
    n_in = img.shape[axis]
    acc = np.full((bounds.shape[0],) + tuple(s for i, s in enumerate(img.shape) if i != axis), 1 << (PRECISION_BITS - 1), np.int64)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    for k in range(coefs.shape[1]):
        idx = np.minimum(bounds[:, 0].astype(np.int64) + k, n_in - 1)
        c = np.where(k < bounds[:, 1], coefs[:, k], 0).astype(np.int64)
        acc += src[idx] * c[:, None, None]
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img, new_w, new_h):
    h, w = img.shape[:2]
    out = img
    if new_w != w:
        out = _pass(out, *axis_table(w, new_w), axis=1)      # horizontal first, rounded to uint8
    if new_h != h:
        out = _pass(out, *axis_table(h, new_h), axis=0)
    return out


def crop(img, box):
    x0, y0, x1, y1 = [int(v) for v in box]
    out = np.zeros((y1 - y0, x1 - x0, 3), np.uint8)
    h, w = img.shape[:2]
    xa, xb, ya, yb = max(x0, 0), min(x1, w), max(y0, 0), min(y1, h)
    if xa < xb and ya < yb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = img[ya:yb, xa:xb]
    return out


def rotation_fixed(angle, w, h):
    """the six 16.16 integers of PIL's Image.rotate(angle) (nearest, about the centre, no expand) on a w x h image"""
    t = -math.radians(angle % 360.0)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))
    return (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def rotate(img, angle):
    if angle % 360.0 == 0:
        return img
    h, w = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = rotation_fixed(angle, w, h)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    xin = (a2 + a1 * y + a0 * x) >> 16
    yin = (a5 + a4 * y + a3 * x) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def canvas(img, aug):
    """img (H, W, 3) uint8, aug = (resize_dims (newW, newH), crop box, flip, rotate): the reference's results['canvas'] entry"""
    dims, box, flip, angle = aug
    out = crop(resize(img, int(dims[0]), int(dims[1])), box)
    if flip:
        out = out[:, ::-1]
    return np.ascontiguousarray(rotate(out, float(angle)))


def normalize(cv):
    """(fH, fW, 3) uint8 -> (3, fH, fW) float32: the reference's to_rgb on an RGB array (plane 0 is blue), float32, no fma"""
    return np.ascontiguousarray(np.moveaxis((cv[..., ::-1].astype(np.float32) - MEAN32) * STDINV32, -1, 0))


def prepare(img, aug):
    cv = canvas(img, aug)
    return cv, normalize(cv)


def eval_aug(H, W, fH, fW, offset=0.0, angle=0.0, flip=0, crop_h=(0.0, 0.0)):
    """resize = fW / W + offset and the reference's test-time crop rule (loading.py:989-1000), with a rotation and a flip put in"""
    rs = float(fW) / float(W) + offset
    dims = (int(W * rs), int(H * rs))
    ch = int((1 - np.mean(crop_h)) * dims[1]) - fH
    cw = int(max(0, dims[0] - fW) / 2)
    return dims, (cw, ch, cw + fW, ch + fH), flip, angle


# (H, W, fH, fW, resize offset, angle, flip): the cases pinned against PIL
CASES = [(45, 80, 24, 64, 0, 0, 0), (45, 80, 24, 64, .07, 3.7, 1), (45, 80, 24, 64, -.05, -5.4, 0), (45, 80, 24, 64, .11, 5.4, 0),
         (90, 160, 48, 128, .11, 5.4, 1), (47, 83, 25, 67, .03, 2.25, 1), (47, 83, 25, 67, -.06, -.01, 0), (30, 40, 40, 64, 0, 0, 0),
         (30, 40, 40, 64, .2, 4.0, 1), (900, 1600, 512, 1408, 0, 0, 0)]


def synthetic_frames(seed, n, H, W):
    """n frames (H, W, 3) uint8: a diagonal gradient per channel plus strong noise, saturating at both ends so that the bicubic
    overshoot is clipped at 0 and at 255"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        g = np.stack([(x * (300.0 / W) + y * (40.0 / H)), (y * (330.0 / H) - 30.0 + 0 * x), ((x + y) * (280.0 / (W + H)) + 10.0 * i)], -1)
        out.append(np.clip(g - 20.0 + rs.normal(0, 45.0, (H, W, 3)) * (rs.uniform(0, 1, (H, W, 1)) < 0.5), 0, 255).astype(np.uint8))
    return out


CAM_NAMES = ['CAM_FRONT_LEFT', 'CAM_FRONT', 'CAM_FRONT_RIGHT', 'CAM_BACK_RIGHT', 'CAM_BACK', 'CAM_BACK_LEFT']


def _info(seed, step, k_scale):
    """one info dict (cams[name]: data_path, cam_intrinsic, sensor2ego_*, ego2global_*) of the synthetic 6-camera rig, the ego
    `step` frames along its track"""
    import _depth_np as DN
    from preworld_amd import synth as S
    rig = S.synthetic_rig(6, dtype=np.float64)
    yaw = math.radians(31.0 + 1.5 * step + seed)
    ego_R, ego_t = DN._rot_z(yaw), np.array([412.5 + 2.4 * step, 1103.25 - 0.7 * step, 0.5])
    cams = {}
    for i, name in enumerate(CAM_NAMES):
        s2e = rig['sensor2ego'][0, i]
        K = rig['intrin'][0, i].copy()
        K[:2] *= k_scale
        cams[name] = dict(data_path='synthetic/%s/%d_%d.jpg' % (name, seed, step), cam_intrinsic=K.tolist(),
                          sensor2ego_rotation=DN.rot_to_quat(s2e[:3, :3]), sensor2ego_translation=list(s2e[:3, 3]),
                          ego2global_rotation=DN.rot_to_quat(DN._rot_z(math.radians(0.2 * (i - 2.5))) @ ego_R),
                          ego2global_translation=list(ego_t + ego_R @ np.array([0.05 * (i - 2.5), 0.01 * i, 0.0])))
    return dict(cams=cams)


def synthetic_sample(seed, H, W, n_adj=1, k_scale=0.05):
    """The part of `results` PrepareImageInputs4DTraj reads: curr, adjacent, temporal_ann_infos[1..6] = {curr, adjacent}, and
    `frames`: 7 x 6 x (1 + n_adj) images in the order the reference opens files, keyed by data_path in `files`."""
    res = dict(curr=_info(seed, 0, k_scale), adjacent=[_info(seed, -1 - a, k_scale) for a in range(n_adj)], temporal_ann_infos={})
    for k in range(1, 7):
        res['temporal_ann_infos'][k] = dict(curr=_info(seed, k, k_scale), adjacent=[_info(seed, k - 1 - a, k_scale) for a in range(n_adj)])
    paths = []
    for d in [res] + [res['temporal_ann_infos'][k] for k in range(1, 7)]:
        for name in CAM_NAMES:
            paths.append(d['curr']['cams'][name]['data_path'])
            paths.extend(a['cams'][name]['data_path'] for a in d['adjacent'])
    uniq = sorted(set(paths))
    imgs = dict(zip(uniq, synthetic_frames(seed, len(uniq), H, W)))
    res['files'] = imgs
    res['frames'] = [imgs[p] for p in paths]
    return res


DATA_CONFIG = dict(cams=CAM_NAMES, Ncams=6, input_size=(24, 64), src_size=(45, 80), resize=(-0.06, 0.11), rot=(-5.4, 5.4), flip=True,
                   crop_h=(0.0, 0.0), resize_test=0.00)
