"""The LSS depth term of one fine-tune step at the training size (B = 2, 6 views, 512 x 1408, D = 88), three ways, in one process:

  (i)   the path of the parent commit: H2D copy of the dense (B,6,512,1408) gt_depth (pinned host memory) + get_depth_loss
        forward + backward (PyTorch: permute copies, one-hot, boolean-mask indexing, which synchronises);
  (ii)  the new path from a dense gt_depth: the same H2D copy + pw_depth_map_labels + pw_depth_bce_fwd / _bwd;
  (iii) the new path from the sweep: H2D copy of the points and the calibration + pw_lidar_depth_labels + pw_depth_bce_fwd / _bwd.

Each is timed wall-clock around `--iters` back-to-back steps, synchronised at both ends (path (i) also synchronises inside
every step, which is part of what it costs); the three are interleaved over `--rounds` rounds and the median round is reported with
the spread, so a drifting clock hits all three alike.  Prints one JSON line with the times and the bytes moved host -> device.

    python tools/bench_depth_sup.py [--iters 1000] [--rounds 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _depth_np as DN  # noqa: E402
from preworld_amd import modules, ops, synth as S, transforms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    dev, B, H, W, D = 'cuda:0', 2, 512, 1408, 88
    depth = S.GRID_CONFIG_FULL['depth']
    vt = modules.LSSViewTransformerBEVStereo(grid_config=S.GRID_CONFIG_FULL, input_size=(H, W), in_channels=16, out_channels=8,
                                             sid=False, collapse_z=False, loss_depth_weight=3.0, downsample=16,
                                             depthnet_cfg=dict(use_dcn=False, aspp_mid_channels=8, stereo=True, bias=5.0)).to(dev)
    Rs = [DN.synthetic_results(11 + b, H, W, 0.48, n_az=1000, n_boxes=30, pts_per_box=100) for b in range(B)]
    pts_h = torch.from_numpy(np.concatenate([r['points'] for r in Rs])).pin_memory()
    off_h = torch.tensor(np.cumsum([0] + [r['points'].shape[0] for r in Rs]), dtype=torch.int32).pin_memory()
    l2i_h = torch.stack([transforms.compose_lidar2img(r['curr'], r['cam_names'], r['intrins']) for r in Rs]).pin_memory()
    pr_h = torch.from_numpy(np.stack([r['post_rots'] for r in Rs])).pin_memory()
    pt_h = torch.from_numpy(np.stack([r['post_trans'] for r in Rs])).pin_memory()
    small = [pts_h, off_h, l2i_h, pr_h, pt_h]
    gt_h = ops.lidar_depth_maps(pts_h.to(dev), l2i_h.to(dev), pr_h.to(dev), pt_h.to(dev), (H, W), depth[:2],
                                offsets=off_h.to(dev)).cpu().pin_memory()
    logits = (torch.randn(B * 6, D, H // 16, W // 16, generator=torch.Generator().manual_seed(1)) * 2.0).to(dev).requires_grad_(True)

    def old():
        gt = gt_h.to(dev, non_blocking=True)
        loss = vt.get_depth_loss(gt, logits.softmax(1))
        return torch.autograd.grad(loss, logits)[0]

    def new_dense():
        gt = gt_h.to(dev, non_blocking=True)
        loss = vt.get_depth_loss_from_labels(vt.get_depth_labels(gt_depth=gt), logits.softmax(1))
        return torch.autograd.grad(loss, logits)[0]

    def new_points():
        p, o, l, r, t = [x.to(dev, non_blocking=True) for x in small]
        loss = vt.get_depth_loss_from_labels(vt.get_depth_labels(points=p, offsets=o, lidar2img=l, post_rots=r, post_trans=t),
                                             logits.softmax(1))
        return torch.autograd.grad(loss, logits)[0]
    paths = [('parent_dense_torch', old), ('new_from_dense', new_dense), ('new_from_points', new_points)]
    ref = old()
    for name, fn in paths:
        for _ in range(10):
            g = fn()
        assert float((g - ref).abs().max()) <= 4e-5 * float(ref.abs().max()), name
    times = {name: [] for name, _ in paths}
    for _ in range(a.rounds):
        for name, fn in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.iters * 1e3)
    nbytes = dict(parent_dense_torch=gt_h.numel() * 4, new_from_dense=gt_h.numel() * 4,
                  new_from_points=sum(x.numel() * x.element_size() for x in small))
    out = dict(bench='depth_supervision', B=B, views=6, image=[H, W], D=D, points=[r['points'].shape[0] for r in Rs], iters=a.iters,
               rounds=a.rounds)
    for name, _ in paths:
        t = sorted(times[name])
        out[name] = dict(ms_median=round(t[len(t) // 2], 4), ms_min=round(t[0], 4), ms_max=round(t[-1], 4), h2d_bytes=nbytes[name])
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
