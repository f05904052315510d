"""TEST INFRASTRUCTURE ONLY.  Float64 yardstick of the dense camera-view renderer (k_render_views<0|1|2> in
preworld_amd/csrc/pw_render_views.hip) and the cases the CPU and GPU pins run (tests/test_render_views_ref64_cpu.py,
tests/test_gpu_render_views_ref64.py).

Above the harness line nothing is taken from oracle/, preworld_amd/ or the kernel.  The march itself is tests/_render_ref64.py's
`render64` (imported, not copied: its docstring states the decisions, margins and tie windows); this file adds what the view kernel
adds to it:

  pixel_rays64   mmdet3d/datasets/ray.py:34-45 as pts2ray calls it (:50): output pixel (i, j) of view v looks through the source
                 pixel (x0 + j stride, y0 + i stride) at its centre (+0.5); dirs = ((x - K02) / K00, (y - K12) / K11, 1), rays_d =
                 c2w[:3,:3] dirs, rays_o = c2w[:3,3].  The fp32 K and c2w widened to float64, everything after that in float64.
  views64        render64 on those rays, plus cls = the float64 argmax of the semantic sums, cls_margin = top minus second, and
                 opacity = 1 - alphainv_last (what min_opacity cuts).
  label_views64  LABEL MODE as include/preworld_hip.h states it: same rays, same sample positions, same inner | cumdist mask (all
                 from _render_ref64._geometry); a sample's voxel is floor(u + 0.5) per axis with u the align_corners=True
                 continuous index, outside the grid is a miss; the first kept sample whose label is not empty_idx is the hit:
                 cls = label, depth = (s_hit + 1e-7) radius, s = 1 - 1 / (1 + t), alphainv_last = 0; no hit: cls = empty_idx,
                 depth = 1e-7 radius, alphainv_last = 1.

FRAGILE PIXELS OF LABEL MODE.  A label pixel is `fragile` when some sample up to and including the hit
  (a) lies within FACE WINDOW of a voxel face (u + 0.5 within the window of an integer) whose far side holds a different label
      (outside the grid counts as empty_idx), or within the window of two faces at once (the diagonal neighbour), or
  (b) belongs to a ray that is a mask tie in _geometry's windows (NORM_TIE, the cumdist window) and sits in a non-empty voxel.
The face window, per axis, from fp32 rounding of u (ulp(1) = 2^-23), as the ray pin derived NORM_TIE:
  * the sample position p (after contraction and bda, |p| <= 1 + bg_len) is known to POS_ULPS = 8 ulp(1): the estimate the ray pin
    doubles into NORM_TIE for the same quantity (the norm of q moves by what q moves by); the pixel's ray direction adds four fp32
    roundings to the three of the ray pin, inside that doubling.  In voxels: POS_ULPS ulp(1) (n - 1) / (xyz_max - xyz_min).
  * u = (((p - lo) / (hi - lo)) 2 - 1 + 1) / 2 (n - 1) as the kernel's rv_index evaluates it: the subtraction, the division, the
    - 1 and the + 1 each round a value of magnitude <= 2 (the two powers of two are exact): 4 x ulp(1) / 2 in g, halved by / 2:
    ulp(1) (n - 1) in voxels; the product with n - 1 and the + 0.5 before the floor each round a value <= n: 2 x ulp(n) / 2.
  FACE WINDOW = (n - 1) ulp(1) (POS_ULPS / (hi - lo) + 1) + ulp(n).  It scales with n (with ulp(n) once n - 1 is factored), and on
  the grids used here it is 6.8e-6 (X = 11), 4.0e-6 (Y = 7) and 2.5e-5 (Z = 5, whose extent is 0.164) voxel: under the 1e-4 the
  fp32 restatement tests/_render_views_np.py uses, asserted for every case in the CPU test.  tests/test_render_views_ref64_cpu.py
  also asserts that restatement (fp32, other summation order) agrees with label_views64 off the fragile pixels of both: a window
  too narrow for fp32 arithmetic would show there, without a GPU.

EXCUSED PIXELS.  A soft-mode pixel is excused from the tight bound when the yardstick marks its ray `tie` (near-tie or mask-tie,
_render_ref64's docstring); at most TIE_CAP = 10 % of a case's pixels, from the float64 reference alone.  On a near-tie pixel that
is no mask tie the kernel may keep or drop samples of total weight <= W_TIE = 1.1e-3 (one sample at the alpha / weight cull, or
everything after an early stop at T < 1e-3 (1 + NEAR_TIE)), which moves
  depth by <= W_TIE radius (s < 1), semantic / colour by <= W_TIE max |grid channel| (a trilinear value is a convex combination
  of voxel values and zeros), alphainv_last by <= W_TIE (T_last changes by the dropped sample's weight times a product <= 1),
each on top of the 4 x floor of a non-excused pixel: `near_tie_bounds`.

METRIC AND FLOORS.  _render_ref64's: max |got - ref| / max |ref| per output over the non-excused pixels.  FLOORS holds, per case,
the error of the existing fp32 CPU checker -- tests/_render_views_np.pixel_rays (fp32) fed to oracle/torch_render.render on ONE
thread -- against the yardstick in that metric for depth, sem, color, alphainv_last, rounded up to two digits with the measured
value in the comment.  The GPU pins allow 4 x these; bf16 storage uses the same floors against the yardstick on the bf16-rounded
grid.  tests/test_render_views_ref64_cpu.py asserts every floor from both sides (<= floor, >= floor / 1.1).  No number comes from the kernel.

SEEDS.  See the comment above CASES."""
import collections
import functools

import numpy as np
import torch

import _render_ref64 as Y
from _render_ref64 import (BDA, F64, N_SEM, NORM_TIE, CUM_TIE_ENDS, CUM_TIE_STEP, TIE_CAP, ULP1, _geometry, bf16_round, pack,  # noqa: F401
                           render64, scene_mixed, standard_constants, table)

DEFAULT_LAYOUT = Y.DEFAULT_LAYOUT
OUTPUTS = ('depth', 'sem', 'color', 'alphainv_last')                   # the kernel's names; the yardstick calls sem `semantic`
REF_KEY = dict(depth='depth', sem='semantic', color='color', alphainv_last='alphainv_last')
W_TIE = 1.1e-3
POS_ULPS = 8
FACE_CAP = 1e-4                # the window of the fp32 restatement: the derived one must not exceed it
FRAGILE_CAP = 0.10
LABEL_DEPTH_ABS = 2 * ULP1     # x radius: label_depth_fp32


def _as64(a):
    return (a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(F64)


# ------------------------------------------------------------------------------------ the yardstick
def pixel_rays64(K, c2w, hw, stride=1, origin=(0, 0)):
    """K (V,3,3), c2w (V,4,4) float32, widened.  Returns rays_o, rays_d (V H W, 3) float64, view-major then row-major"""
    K, c2w = _as64(np.asarray(K, np.float32)), _as64(np.asarray(c2w, np.float32))
    H, W = hw
    x = (origin[0] + torch.arange(W, dtype=F64) * stride + 0.5)[None, :].expand(H, W)
    y = (origin[1] + torch.arange(H, dtype=F64) * stride + 0.5)[:, None].expand(H, W)
    ro, rd = [], []
    for v in range(K.shape[0]):
        dirs = torch.stack([(x - K[v, 0, 2]) / K[v, 0, 0], (y - K[v, 1, 2]) / K[v, 1, 1], torch.ones(H, W, dtype=F64)], -1)
        rd.append((dirs[..., None, :] * c2w[v, :3, :3]).sum(-1).reshape(-1, 3))
        ro.append(c2w[v, :3, 3].expand(H * W, 3))
    return torch.cat(ro).contiguous(), torch.cat(rd).contiguous()


def views64(K, c2w, hw, stride, origin, t, grid, consts, layout=DEFAULT_LAYOUT, fp32_alpha=False):
    """render64 on the pixels' rays; adds cls (int64), cls_margin, second (the runner-up class), opacity; all (V H W, ...)"""
    ro, rd = pixel_rays64(K, c2w, hw, stride, origin)
    ref = render64(ro, rd, t, grid, consts, layout, fp32_alpha=fp32_alpha)
    top2 = torch.topk(ref['semantic'], 2, dim=-1)
    # torch.topk does not promise the lowest index on exact float64 ties; argmax does not either: take the first maximum
    is_max = ref['semantic'] == top2.values[:, :1]
    ref['cls'] = is_max.to(torch.int64).argmax(-1)
    ref['second'] = torch.where(top2.indices[:, 0] == ref['cls'], top2.indices[:, 1], top2.indices[:, 0])
    ref['cls_margin'] = top2.values[:, 0] - top2.values[:, 1]
    ref['opacity'] = 1 - ref['alphainv_last']
    ref['rays_o'], ref['rays_d'] = ro, rd
    return ref


def face_window(consts, shape):
    """FACE WINDOW per axis, in voxels (module docstring)"""
    c = np.asarray(consts, np.float64)
    n = np.asarray(shape, np.float64)
    ulp_n = 2.0 ** (np.floor(np.log2(n)) - 23)
    return (n - 1) * ULP1 * (POS_ULPS / (c[18:21] - c[15:18]) + 1) + ulp_n


def label_views64(labels, rays, consts, t, empty_idx):
    """LABEL MODE in float64.  labels uint8 (X,Y,Z) numpy; rays = (rays_o, rays_d) float64 (R,3); consts (27) and t (S) the fp32 values
    the kernel reads.  Returns dict(cls int64 (R), depth, alphainv_last float64 (R), first int64 (R, -1 = no hit), fragile bool (R),
    mask (R,S))"""
    ro, rd = rays
    c, t64 = _as64(np.asarray(consts, np.float32)), _as64(np.asarray(t, np.float32))
    geo = _geometry(_as64(ro), _as64(rd), t64, c)
    lab_t = torch.from_numpy(np.ascontiguousarray(labels).astype(np.int64))
    shape = torch.tensor(labels.shape, dtype=F64)
    u = (geo['pts'] - c[15:18]) / (c[18:21] - c[15:18]) * (shape - 1) + 0.5             # (R,S,3): the voxel is floor(u)
    idx = torch.floor(u)

    def lookup(ix):
        ok = ((ix >= 0) & (ix < shape)).all(-1)
        ii = torch.where(ok[..., None], ix, torch.zeros_like(ix)).to(torch.int64)
        return torch.where(ok, lab_t[ii[..., 0], ii[..., 1], ii[..., 2]], torch.full(ok.shape, int(empty_idx), dtype=torch.int64))

    lab = lookup(idx)                                                                  # outside the grid: empty
    occ = geo['mask'] & (lab != empty_idx)
    R, S = occ.shape
    any_hit = occ.any(1)
    first = torch.where(any_hit, occ.to(torch.int64).argmax(1), torch.full((R,), -1, dtype=torch.int64))
    fs = first.clamp_min(0)
    r = torch.arange(R)
    s_hit = 1 - 1 / (1 + t64[fs])
    cls = torch.where(any_hit, lab[r, fs], torch.full((R,), int(empty_idx), dtype=torch.int64))
    depth = (torch.where(any_hit, s_hit, torch.zeros_like(s_hit)) + 1e-7) * c[26]
    last = torch.where(any_hit, torch.zeros(R, dtype=F64), torch.ones(R, dtype=F64))
    upto = torch.arange(S)[None, :] <= torch.where(any_hit, first, torch.full_like(first, S))[:, None]
    win = torch.from_numpy(face_window(consts, labels.shape))
    frac = u - idx
    near_lo, near_hi = frac <= win, (1 - frac) <= win                                   # (R,S,3)
    near = near_lo | near_hi
    differs = near.sum(-1) >= 2
    for ax in range(3):
        alt = idx.clone()
        alt[..., ax] = torch.where(near_lo[..., ax], idx[..., ax] - 1, idx[..., ax] + 1)
        differs |= near[..., ax] & (lookup(alt) != lab)
    face = differs & geo['mask']
    tie = geo['mask_tie'][:, None] & (lab != empty_idx)
    fragile = ((face | tie) & upto).any(1)
    return dict(cls=cls, depth=depth, alphainv_last=last, first=first, fragile=fragile, mask=geo['mask'])


def voxel_pixels(ref, t, consts, shape, voxel, sure_weight=1e-3):
    """which pixels of a views64 result read voxel (x, y, z) of a grid of `shape` = (X,Y,Z) into their semantic / colour sums.
    Returns (sure, maybe) bool (R): `sure` -- a kept sample of a non-tie pixel has the voxel among its in-bounds trilinear corners
    with a float64 weight >= sure_weight (each per-axis weight is then >= sure_weight: the sample is that far inside the cell, forty
    face windows, so an fp32 evaluation has the same corner set); `maybe` -- some MASKED sample lies within 1 + sure_weight voxels
    of it on every axis (a superset of every sample any evaluation could gather it for).  Pixels outside `maybe` cannot see the voxel."""
    X, Y_, Z = shape
    vx, vy, vz = voxel
    col = (vz * Y_ + vy) * X + vx
    A = ref['A']
    ii, vv = A.indices(), A.values()
    hit = (ii[1] == col) & (vv >= sure_weight)
    ray_id, step_id = torch.nonzero(ref['mask'], as_tuple=True)
    rows = ii[0][hit]
    R = ref['mask'].shape[0]
    sure = torch.zeros(R, dtype=torch.bool)
    keep = ref['kept'][ray_id[rows], step_id[rows]]
    sure[ray_id[rows][keep]] = True
    sure &= ~ref['tie']
    c = _as64(np.asarray(consts, np.float32))
    geo = _geometry(ref['rays_o'], ref['rays_d'], _as64(np.asarray(t, np.float32)), c)
    f = (geo['pts'] - c[15:18]) / (c[18:21] - c[15:18]) * (torch.tensor(shape, dtype=F64) - 1)
    close = ((f - torch.tensor(voxel, dtype=F64)).abs() < 1 + sure_weight).all(-1)
    maybe = (close & geo['mask']).any(1) | sure
    return sure, maybe


def label_depth_fp32(first, t, consts):
    """label mode's depth as ONE fp32 expression of the hit's table entry, ((1 - 1 / (1 + t[first])) + 1e-7) radius, every operation
    rounded to fp32 (first = -1: the miss value 1e-7 radius).  The float64 value of the same expression differs from it by up to
    LABEL_DEPTH_ABS = 2 ulp(1) radius: 1 / (1 + t) lies in [0.5, 1) for t <= 1 and the subtraction from 1 cancels, so s carries the
    absolute error of the two roundings before it (half an ulp(1) each, doubled), whatever its size -- 3e-6 of s at the first samples."""
    f = np.float32
    first = np.asarray(first)
    tt = np.asarray(t, f)[np.maximum(first, 0)]
    s = np.where(first >= 0, f(1) - f(1) / (f(1) + tt), f(0)).astype(f)
    return ((s + f(1e-7)) * np.asarray(consts, f)[26]).astype(f)


# ------------------------------------------------------------------------------------ metrics and bounds
def output_errors(got, ref, ok=None):
    """max |got - ref| / max |ref| per output of OUTPUTS over the pixels `ok` (default: the yardstick's non-tie pixels).  got: dict of
    arrays / tensors keyed by the kernel's names, any leading shape that flattens to the yardstick's pixel order"""
    ok = ~ref['tie'] if ok is None else ok
    err = {}
    for k in OUTPUTS:
        r = ref[REF_KEY[k]]
        g = _as64(got[k]).reshape(r.shape)
        e = (g[ok] - r[ok]).abs()
        err[k] = float(e.max() / r[ok].abs().max().clamp_min(1e-300)) if e.numel() else 0.0
    return err


def near_tie_bounds(name, grid, ref, pre=4.0):
    """absolute bound per output of OUTPUTS on a near-tie pixel that is no mask tie (module docstring): what samples of total weight
    W_TIE can move, plus the non-excused pixels' pre x floor x max |ref|.  grid: the packed grid the run read (bf16-rounded if so)"""
    _, _, c_sem, c_rgb = CASES[name]['layout']
    g = np.abs(np.asarray(grid, np.float64))
    one = dict(depth=W_TIE * float(standard_constants(BDA)[26]), sem=W_TIE * float(g[..., c_sem:c_sem + N_SEM].max()),
               color=W_TIE * float(g[..., c_rgb:c_rgb + 3].max()), alphainv_last=W_TIE)
    return {k: one[k] + pre * f * float(ref[REF_KEY[k]].abs().max()) for k, f in zip(OUTPUTS, FLOORS[name])}


# ------------------------------------------------------------------------------------ cases
HW, ORIGIN = (19, 37), (3, 2)      # 2 x 3 blocks of 16 x 16 with partial blocks and partial 8 x 8 tiles on both axes


def _c(scene, tab, rig='pair', grid=(11, 7, 5), seed=19, layout=DEFAULT_LAYOUT, hw=HW, origin=ORIGIN, stride=1, **kw):
    return dict(scene=scene, table=tab, rig=rig, grid=grid, seed=seed, layout=layout, hw=hw, origin=origin, stride=stride, **kw)


# name -> scene, sample table, rig, grid (X,Y,Z), grid seed, channel layout, output (H, W), source origin (x0, y0), stride, pitch.
# Rigs are in the harness (`rig`), all from the analytic six-camera rig with K's first two rows divided by 32 (39.6 px focal length):
# pair = cameras 0 and 1, one = camera 0, three = cameras 0, 1, 4 with three different K, outside = camera 1 moved to (48, 2, 1.5) m
# (normalised 1.23: outside the unit ball) looking outward, next to camera 1 in place; face = cameras 1 and 3 lifted to 9 m and 7.5 m,
# above the grid's top face (5.4 m), pitched down across it.  `pitch` (degrees down per camera) is 0 unless a case sets it.
# SEEDS, scanned on the CPU with the float64 reference alone.  Conditions: tie pixels <= TIE_CAP on the fp32 AND the bf16-rounded
# grid, and on `mixed` cases of >= 96 samples at least 10 % of the pixels terminate.  full417 / sub2 / clear keep the ray pin's grid
# seed 19 with the level cameras (6.7 % ties at full417 with 18 % terminating, 0 at sub2, 3.1 % on clear_winner with 16 classes in
# view).  At seed 19 the shorter tables terminate too few pixels (c5_96 6.7 %, dense128 3.6 %, ext448 8.5 %), so grid seeds 1..40 were
# scanned per case, level cameras first: seed 4 is the first that meets the conditions on c5_96 (3.1 % ties, 27 % terminate),
# dense128 (3.6 %, 16 %) and layout_one_wave (3.9 %, 13 %) and the third or fourth on ext448 (6.7 %, 30 %), three_views_stride3 (1.5 %,
# 40 %) and outside_ball (3.6 %, 17 %): those six share it.  tiny_grid takes seed 2 (the first with more than two classes in view:
# 1.7 %, 37 %).  Pitching the cameras down 18 .. 25 degrees was tried and dropped: the rays then cross the ground layer in a few samples
# and leave the grid with T between 0.17 and 0.24, the weight cull's tie band in empty space (13 % near-ties at full417).  across_face needs
# a pitch to meet the grid at all: pitches (0, 0, 0), (4, 6, 5), (8, 10, 9) degrees were scanned in that order and (8, 10, 9) with
# seed 10 is the first hit (2.8 % ties, 10.7 % terminate).  c5_96_plain keeps the ray pin's `plain` grid seed 3.
CASES = collections.OrderedDict([
    ('full417_mixed', _c('mixed', ('full', 417))),                                      # the reference's table
    ('c5_96_mixed', _c('mixed', ('c5', 96), seed=4)),                                           # the benchmarked table
    ('sub2_mixed', _c('mixed', ('sub', 2))),
    ('dense128_mixed', _c('mixed', ('dense', 128), seed=4)),
    ('ext448_mixed', _c('mixed', ('ext', 448), rig='one', seed=4)),                             # V = 1, the longest table
    ('c5_96_plain', _c('plain', ('c5', 96), seed=3)),                                   # transparent
    ('layout_one_wave', _c('mixed', ('c5', 96), seed=4, layout=(32, 5, 8, 27), hw=(8, 8), origin=(8, 5))),   # exactly one wave per view
    ('one_pixel', _c('mixed', ('full', 417), rig='one', seed=4, hw=(1, 1), origin=(23, 11))),
    ('tiny_grid_17x16', _c('mixed', ('c5', 96), grid=(3, 2, 2), seed=2, hw=(17, 16))),
    ('three_views_stride3', _c('mixed', ('c5', 96), rig='three', seed=4, hw=(7, 13), stride=3)),
    ('outside_ball', _c('mixed', ('c5', 96), rig='outside', seed=4)),
    ('across_face', _c('mixed', ('c5', 96), rig='face', seed=10, pitch=(8.0, 10.0, 9.0))),
    ('clear_winner', _c('clear', ('c5', 96))),
])
# label cases: the uint8 grid is thresholded from the mixed density of `seed` (occupied <=> density > 8.5, as the detectors decide)
LABEL_CASES = collections.OrderedDict([
    ('lab_mixed', _c('labels', ('full', 417), empty_idx=17, max_label=16, n_palette=18)),
    ('lab_empty0', _c('labels', ('c5', 96), rig='three', hw=(7, 13), stride=3, empty_idx=0, max_label=17, n_palette=18)),
    ('lab_255', _c('labels', ('dense', 128), rig='face', pitch=(8.0, 10.0, 9.0), empty_idx=17, max_label=255, n_palette=5)),
])

# min_opacity: the case and the two cuts; on it 54 % / 46 % of the pixels lie below / above 0.5 and 32 % / 68 % below / above 0.02
MIN_OPACITY = ('c5_96_mixed', (0.5, 0.02))
# non-finite attributes: the case, the voxel (x, y, z) that gets the NaNs (460 pixels surely read it, 861 cannot: voxel_pixels),
# the semantic channel (not 0: the kernel's running maximum starts from channel 0) and the colour channel
NAN_PROBE = ('c5_96_mixed', (7, 4, 2), 3, 1)

# Error of the fp32 CPU checker against the yardstick, one thread: depth, sem, color, alphainv_last.  Rounded up to two digits;
# measured value in the comment.
FLOORS = {
    'full417_mixed':        (3.0e-06, 1.2e-06, 1.9e-06, 6.2e-06),   # 2.958e-06 1.179e-06 1.859e-06 6.145e-06
    'c5_96_mixed':          (2.2e-06, 1.7e-06, 1.8e-06, 2.2e-06),   # 2.104e-06 1.689e-06 1.775e-06 2.197e-06
    'sub2_mixed':           (2.6e-06, 2.7e-06, 3.9e-06, 2.4e-06),   # 2.509e-06 2.675e-06 3.881e-06 2.340e-06
    'dense128_mixed':       (1.9e-06, 2.0e-06, 2.2e-06, 2.2e-06),   # 1.829e-06 1.998e-06 2.139e-06 2.175e-06
    'ext448_mixed':         (2.8e-06, 1.1e-06, 1.3e-06, 5.8e-06),   # 2.787e-06 1.093e-06 1.231e-06 5.729e-06
    'c5_96_plain':          (6.3e-03, 3.3e-03, 2.1e-03, 9.8e-07),   # 6.257e-03 3.274e-03 2.041e-03 9.795e-07
    'layout_one_wave':      (1.8e-06, 1.9e-06, 2.4e-06, 1.7e-06),   # 1.709e-06 1.861e-06 2.328e-06 1.677e-06
    'one_pixel':            (5.5e-07, 7.5e-07, 8.9e-07, 2.6e-05),   # 5.470e-07 7.496e-07 8.853e-07 2.583e-05
    'tiny_grid_17x16':      (6.9e-07, 3.8e-07, 4.1e-07, 9.4e-07),   # 6.850e-07 3.762e-07 4.065e-07 9.396e-07
    'three_views_stride3':  (1.9e-06, 1.5e-06, 1.8e-06, 2.1e-06),   # 1.840e-06 1.466e-06 1.748e-06 2.075e-06
    'outside_ball':         (3.6e-06, 2.3e-06, 3.0e-06, 3.3e-06),   # 3.581e-06 2.215e-06 2.947e-06 3.298e-06
    'across_face':          (3.5e-06, 4.5e-06, 1.8e-06, 3.3e-06),   # 3.441e-06 4.447e-06 1.703e-06 3.282e-06
    'clear_winner':         (2.4e-06, 3.4e-06, 3.9e-06, 2.5e-06),   # 2.348e-06 3.339e-06 3.821e-06 2.480e-06
}


# ------------------------------------------------------------------------------------ harness (project code from here on)
def rig(name, pitch=(0.0, 0.0, 0.0)):
    """K (V,3,3), c2w (V,4,4) float32 of a named rig; pitch: degrees down per camera slot (a case's `pitch`)"""
    from preworld_amd import synth
    r = synth.synthetic_rig(6, dtype=np.float64)
    s2e, K0 = r['sensor2ego'][0], r['intrin'][0, 0].copy()
    K0[:2] /= 32                                                # 39.6 px focal length, principal point (25.5, 15.4)

    def turned(cam, pitch, yaw, move=(0, 0, 0)):
        p, y = np.radians(pitch), np.radians(yaw)
        Rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
        Ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
        a = s2e[cam].copy()
        a[:3, :3] = a[:3, :3] @ Ry @ Rx.T
        a[:3, 3] += move
        return a

    def scaled(fx, fy, cx, cy):
        k = K0.copy()
        k[0, 0], k[1, 1], k[0, 2], k[1, 2] = fx, fy, cx, cy
        return k

    P = pitch
    if name == 'pair':
        K, c2w = [K0, K0], [turned(0, P[0], 0.0), turned(1, P[1], 8.0)]
    elif name == 'one':
        K, c2w = [K0], [turned(0, P[0], 0.0)]
    elif name == 'three':                                        # three different K and c2w: a wrong v * 9 or v * 16 shows
        K, c2w = ([K0, scaled(31.0, 33.0, 22.5, 14.0), scaled(45.0, 42.0, 27.0, 17.5)],
                  [turned(0, P[0], 0.0), turned(1, P[1], 8.0), turned(4, P[2], -10.0)])
    elif name == 'outside':                                      # (48, 2, 1.5) m: |o - center| / radius = 1.23; looking along +x
        K, c2w = [K0, scaled(36.0, 38.0, 24.0, 15.0)], [turned(1, P[0], 0.0, (46.5, 2.0, 0.0)), turned(1, P[1], 8.0)]
    elif name == 'face':                                         # 9 m up, above the grid's top face (5.4 m), looking down across it
        K, c2w = [K0, scaled(36.0, 38.0, 24.0, 15.0)], [turned(1, P[1], 10.0, (0.0, 0.0, 7.5)), turned(3, P[2], -15.0, (0.0, 0.0, 6.0))]
    else:
        raise KeyError(name)
    return np.stack(K).astype(np.float32), np.stack(c2w).astype(np.float32)


def clear_scene(seed, X, Y_, Z):
    """the class-map scene in the style of _render_views_np.clear_scene at any grid size: scene_mixed's density and colour, a
    semantic field whose winner is constant per region at +6 over N(0, 0.3): ground voxels (z = 0) carry class (5 x + 3 y) % 17,
    other occupied voxels 1 + (x + 3 y) % 10, free space 16"""
    density, _, color = scene_mixed(seed, X, Y_, Z)
    rs = np.random.RandomState(seed + 7)
    semantic = (rs.standard_normal((X, Y_, Z, N_SEM)) * 0.3).astype(np.float32)
    xs, ys = np.meshgrid(np.arange(X), np.arange(Y_), indexing='ij')
    win = np.broadcast_to((1 + (xs + 3 * ys) % 10)[:, :, None], (X, Y_, Z)).copy()
    win[:, :, 0] = (5 * xs + 3 * ys) % 17
    win[density <= 8.5] = 16
    np.put_along_axis(semantic, win[..., None], np.float32(6), -1)
    return density, semantic, color


def label_grid(name):
    """uint8 (X,Y,Z): occupied voxels of the mixed density carry a random label in the case's range that is not empty_idx"""
    case = LABEL_CASES[name]
    X, Y_, Z = case['grid']
    density = scene_mixed(case['seed'], X, Y_, Z)[0]
    rs = np.random.RandomState(case['seed'] + 1)
    e, hi = case['empty_idx'], case['max_label']
    if hi == 255:                                               # both sides of a 5-row palette's clamp, up to the largest uint8
        lab = np.array([0, 1, 2, 3, 4, 5, 16, 18, 100, 200, 254, 255])[rs.randint(0, 12, density.shape)]
    elif e > hi:
        lab = rs.randint(0, hi + 1, density.shape)
    else:                                                       # 0 .. hi with empty_idx skipped
        lab = rs.randint(0, hi, density.shape)
        lab = np.where(lab >= e, lab + 1, lab)
    return np.where(density > 8.5, lab, e).astype(np.uint8)


def _case(name):
    return CASES[name] if name in CASES else LABEL_CASES[name]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """a case's float32 inputs: K, c2w, t (S), packed grid (Z,Y,X,GC) or labels (X,Y,Z), consts (27)"""
    from preworld_amd import synth
    case = _case(name)
    X, Y_, Z = case['grid']
    K, c2w = rig(case['rig'], case.get('pitch', (0.0, 0.0, 0.0)))
    x = dict(K=K, c2w=c2w, t=table(case['table']), consts=standard_constants(BDA))
    if case['scene'] == 'labels':
        x['labels'] = label_grid(name)
        return x
    grids = {'mixed': scene_mixed, 'clear': clear_scene, 'plain': synth.render_grids}[case['scene']](case['seed'], X, Y_, Z)
    x['grid'] = pack(*grids, case['layout'], case['seed'])
    return x


@functools.lru_cache(maxsize=None)
def reference(name, bf16=False):
    """the yardstick on a soft case; bf16: on the bf16-rounded grid.  Shared by the tests: do not modify the result."""
    x, case = inputs(name), CASES[name]
    grid = bf16_round(x['grid']) if bf16 else x['grid']
    return views64(x['K'], x['c2w'], case['hw'], case['stride'], case['origin'], x['t'], grid, x['consts'], case['layout'])


@functools.lru_cache(maxsize=None)
def label_reference(name):
    x, case = inputs(name), LABEL_CASES[name]
    rays = pixel_rays64(x['K'], x['c2w'], case['hw'], case['stride'], case['origin'])
    return label_views64(x['labels'], rays, x['consts'], x['t'], case['empty_idx'])


def checker_fp32(name):
    """the existing fp32 CPU checker on a soft case: _render_views_np.pixel_rays (fp32) fed to oracle/torch_render.render on ONE
    thread.  Returns the outputs under the kernel's names plus the (R,S) sample mask."""
    import _render_views_np as RV
    from oracle import oracle as O
    from oracle import torch_render as TR
    x, case = inputs(name), CASES[name]
    rows = RV.pixel_rays(x['K'], x['c2w'], case['hw'], case['stride'], case['origin']).reshape(-1, 9)
    o, d = np.ascontiguousarray(rows[:, 0:3]), np.ascontiguousarray(rows[:, 3:6])
    consts = O.NerfConsts()
    consts.t_table = lambda: x['t']
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        grids = [torch.from_numpy(np.ascontiguousarray(a)) for a in Y.unpack(x['grid'], case['layout'])]
        out = TR.render(o, d, BDA, *grids, consts)
    finally:
        torch.set_num_threads(nt)
    res = O.render_one_scene(o, d, BDA, *[g.numpy() for g in grids], consts)
    return dict(depth=out['depth'], sem=out['semantic'], color=out['color'], alphainv_last=out['alphainv_last'],
                mask=torch.from_numpy(res['sample_mask'].astype(bool)))
