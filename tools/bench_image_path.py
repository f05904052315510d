"""true image -> occupancy throughput of the C3 sample on one GPU.

images (6 cams x [key, adjacent, extra stereo reference], 3x512x1408) -> Swin-B + FPN_LSS + DepthNet with the stereo cost
volume (PyTorch-ROCm, fp32 like the reference; preworld_amd/image_encoder.py) -> the measured hot path of bench.py
(LSS pooling x2, voxel encoder, forecast, OccHead x7; hipGraph replay).  Random weights, synthetic images and rig.
Prints one JSON line; bench.py's `value` stays the hot-path number (the backbone is outside the path)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from preworld_amd import harness, image_encoder as IE, synth as S  # noqa: E402
from preworld_amd.pipeline import CapturedSample  # noqa: E402


class ImagePath:
    """the C3 sample's image -> occupancy path, built once: run(amp, attn, steps) times it with the image branch under bf16 autocast
    or not, the Swin blocks' window attention on the torch path or the fused HIP kernel (attn_impl, preworld_amd/image_encoder.py)
    and their Linears on torch or on the fused HIP GEMM (linear_impl)"""

    def __init__(self, dev='cuda:0'):
        T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        torch.manual_seed(0)
        self.branch = IE.ImageBranch(**IE.preworld_image_cfg()).to(dev).eval()
        self.n_par = sum(p.numel() for p in self.branch.parameters())
        net = harness.build_model(harness.model_cfg(S.GRID_CONFIG_FULL), S.synth_state_dict(0), dev)
        rigs = [S.synthetic_rig(6, dx=-2.5 * f) for f in range(3)]
        imgs = [torch.randn(1, 6, 3, 512, 1408, device=dev) for _ in range(3)]
        s2k = [T(r['sensor2ego']) for r in rigs]
        e2g = [torch.eye(4, device=dev).view(1, 1, 4, 4).repeat(1, 6, 1, 1) for _ in range(3)]
        intr, prot, ptran = [T(r['intrin']) for r in rigs], [T(r['post_rot']) for r in rigs], [T(r['post_tran']) for r in rigs]
        k2s = torch.eye(4, device=dev).view(1, 1, 4, 4).repeat(1, 6, 1, 1)
        k2s[..., 0, 3] = 2.5
        self.ego = T(S.ego_state(0))
        self.amp = 'none'
        bda = T(rigs[0]['bda'])

        def image_side():
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=self.amp == 'bf16'):
                return self.branch.frames_from_images(imgs, s2k, e2g, intr, prot, ptran, bda, [k2s, k2s, None])
        self.image_side = image_side
        self.cap = CapturedSample(net, self._f32(image_side()), self.ego, n_steps=6)

    @staticmethod
    def _f32(frames):
        frames = [{k: (v.float() if v.is_floating_point() else v) for k, v in f.items()} for f in frames]
        for f in frames:
            f['tran_feat']._pw_channels_last = True
        return frames

    def step(self):
        return self.cap.run(self._f32(self.image_side()), self.ego)

    def run(self, amp='none', attn='torch', steps=10, linear='torch', conv='torch'):
        self.amp = amp
        self.branch.img_backbone.set_linear_impl('torch')        # 'hip' Linears need a fused attention: switch in an order that holds
        self.branch.img_backbone.set_attn_impl(attn)
        self.branch.img_backbone.set_linear_impl(linear)
        self.branch.set_conv_impl(conv)                           # FPN_LSS and DepthNet: torch convolutions or the fused HIP implicit GEMM
        for _ in range(2):
            self.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.image_side()
        torch.cuda.synchronize()
        t_img = (time.perf_counter() - t0) / steps
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        torch.cuda.synchronize()
        t_all = (time.perf_counter() - t0) / steps
        return {'metric': 'image -> occupancy samples/s (C3, 1 GPU, serial)', 'value': round(1.0 / t_all, 2),
                'ms_per_sample': round(t_all * 1e3, 2), 'image_branch_ms': round(t_img * 1e3, 2),
                'voxel_path_ms': round((t_all - t_img) * 1e3, 2), 'image_branch_dtype': 'f32' if amp == 'none' else 'bf16 autocast',
                'window_attention': attn, 'block_linears': linear, 'neck_depthnet_convs': conv, 'image_branch_params': self.n_par,
                'images': '6 cams x (key + adjacent full backbone, extra reference stage 0), 3x512x1408',
                'data': 'synthetic, random weights'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--amp', choices=['none', 'bf16'], default='none', help='autocast for the PyTorch image branch only')
    ap.add_argument('--attn', choices=['torch', 'hip'], default='torch', help="the Swin blocks' window attention: torch ops or the fused HIP kernel")
    ap.add_argument('--linear', choices=['torch', 'hip'], default='torch',
                    help="the Swin blocks' Linears, LayerNorms, GELU and residuals: torch ops or the fused HIP GEMM (needs --attn hip)")
    ap.add_argument('--conv', choices=['torch', 'hip'], default='torch',
                    help="the stride-1 convolutions of FPN_LSS and DepthNet: torch ops or the fused HIP implicit GEMM (float32, not with --amp bf16)")
    a = ap.parse_args()
    print(json.dumps(ImagePath().run(a.amp, a.attn, a.steps, a.linear, a.conv)))


if __name__ == '__main__':
    main()
