"""FPN_LSS and DepthNet convolutions: the torch modules of preworld_amd/image_encoder.py against the fused HIP implicit GEMM
(conv_impl='hip', csrc/pw_conv2d.hip), alternating in one process.  float32, eval mode, no grad.

First the split of the image branch on the path as it stands (attn_impl='hip', linear_impl='hip', conv_impl='torch'): device events
in forward hooks around img_backbone, img_neck and depth_net over ImageBranch.frames_from_images of the C3 sample (the remainder is
the extra reference frame's stage-0 pass, the cost-volume inputs and the DepthNet tail).  Then each distinct convolution role at the
C3 shapes (6 cameras, 32 x 88 map): the torch ops the module runs today (conv, BatchNorm, ReLU, residual; NCHW) against one
ops.conv2d call (channels-last); then FPN_LSS and DepthNet whole; then, unless --no-e2e, image -> occupancy samples/s of
tools/bench_image_path.py with both.  Device events around batches of calls sized to --window seconds, after a warm-up; --rounds
repeats, old and new alternating inside every round; median and the min .. max spread are reported.  FLOPs are 2 M K N with
K = taps x Cin; the kernel EXECUTES 3 x 2 M Kp N, Kp = taps x Cin rounded up to 32 (three fp16 products per fp32 product).  Bytes are
algorithmic, from shapes: x read once, out written once, residual read once, the packed weight once.
Prints a markdown report (profiles/image_conv.md keeps one)."""
import argparse
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from preworld_amd import image_encoder as IE, ops  # noqa: E402
from bench_swin_attn import DEV, fmt, rounds  # noqa: E402

B, H, W = 6, 32, 88                          # one frame of the C3 sample: 6 cameras, 512 x 1408 / 16
# role, Cin, Cout, ksize, dilation, BatchNorm, conv bias, ReLU, residual, how many per frame
ROLES = [
    ('img_neck.conv[0]', 1536, 512, 3, 1, True, False, True, False, 1),
    ('3x3 512 -> 512 (neck conv[3], BasicBlock conv1)', 512, 512, 3, 1, True, False, True, False, 3),
    ('reduce_conv (bias + BN)', 512, 512, 3, 1, True, True, True, False, 1),
    ('BasicBlock conv2 + residual', 512, 512, 3, 1, True, False, True, True, 3),
    ('first BasicBlock conv1', 600, 512, 3, 1, True, False, True, False, 1),
    ('first BasicBlock downsample', 600, 512, 1, 1, False, True, False, False, 1),
    ('ASPP 1x1', 512, 96, 1, 1, True, False, True, False, 1),
    ('ASPP dilation 6', 512, 96, 3, 6, True, False, True, False, 1),
    ('ASPP dilation 12', 512, 96, 3, 12, True, False, True, False, 1),
    ('ASPP dilation 18', 512, 96, 3, 18, True, False, True, False, 1),
    ('ASPP.conv1', 480, 512, 1, 1, True, False, True, False, 1),
    ('last depth_conv layer', 512, 88, 1, 1, False, True, False, False, 1),
    ('context_conv', 512, 32, 1, 1, False, True, False, False, 1),
]


def split(a):
    from bench_image_path import ImagePath
    path = ImagePath(DEV)
    br = path.branch
    br.img_backbone.set_attn_impl('hip')
    br.img_backbone.set_linear_impl('hip')
    parts = {'img_backbone (two full Swin-B forwards)': br.img_backbone, 'img_neck': br.img_neck,
             'depth_net': br.img_view_transformer.depth_net}
    events = {k: [] for k in parts}
    hooks = []
    for k, m in parts.items():
        def pre(mod, args, k=k):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events[k].append([e])

        def post(mod, args, out, k=k):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events[k][-1].append(e)
        hooks += [m.register_forward_pre_hook(pre), m.register_forward_hook(post)]
    rows = {k: [] for k in list(parts) + ['everything else', 'image branch']}
    for r in range(a.rounds + 1):                          # the first round warms up
        for v in events.values():
            v.clear()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        path.image_side()
        e1.record()
        torch.cuda.synchronize()
        if r == 0:
            continue
        total, seen = e0.elapsed_time(e1), 0.0
        for k, v in events.items():
            t = sum(s.elapsed_time(e) for s, e in v)
            rows[k].append(t)
            seen += t
        rows['everything else'].append(total - seen)
        rows['image branch'].append(total)
    for h in hooks:
        h.remove()
    import statistics
    print('| image branch, f32, attn hip, Linears hip, torch convolutions | ms per sample |')
    print('|---|---|')
    for k, v in rows.items():
        print('| %s | %s |' % (k, fmt((statistics.median(v), min(v), max(v)))), flush=True)
    return path


def role_rows(a):
    print('\n| role (per frame: 6 x 32 x 88 pixels) | count | M x K x N | torch ms | hip ms | speed-up | hip TFLOP/s (2MKN) | executed TFLOP/s | hip GB/s |')
    print('|---|---|---|---|---|---|---|---|---|')
    M = B * H * W
    tot = {'torch': 0.0, 'hip': 0.0}
    for name, Cin, Cout, k, dil, has_bn, bias, relu, res, count in ROLES:
        torch.manual_seed(1)
        conv = nn.Conv2d(Cin, Cout, k, padding=dil * (k - 1) // 2, dilation=dil, bias=bias).to(DEV)
        bn = nn.BatchNorm2d(Cout).to(DEV).eval() if has_bn else None
        if bn is not None:
            with torch.no_grad():
                bn.running_mean.normal_(std=0.1)
                bn.running_var.uniform_(0.5, 1.5)
        x = torch.randn(B, Cin, H, W, device=DEV)
        r0 = torch.randn(B, Cout, H, W, device=DEV) if res else None
        xc = x.contiguous(memory_format=torch.channels_last)
        rc = None if r0 is None else r0.contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            pk = ops.conv2d_pack(conv, bn)

        def torch_f():
            with torch.no_grad():
                y = conv(x)
                if bn is not None:
                    y = bn(y)
                if r0 is not None:
                    y = y + r0
                return F.relu(y, inplace=True) if relu else y

        def hip_f():
            return ops.conv2d(xc, pk, dilation=dil, relu=relu, residual=rc)
        r = rounds({'torch': torch_f, 'hip': hip_f}, a.rounds, a.window)
        K, Kp = k * k * Cin, k * k * (-(-Cin // 32) * 32)
        tf = 2.0 * M * K * Cout / 1e12 / (r['hip'][0] * 1e-3)
        ex = 3 * 2.0 * M * Kp * Cout / 1e12 / (r['hip'][0] * 1e-3)
        gb = (M * Cin * 4 + M * Cout * 4 * (2 if res else 1) + Cout * Kp * 4) / 1e9 / (r['hip'][0] * 1e-3)
        for p in tot:
            tot[p] += count * r[p][0]
        print('| %s | %d | %d x %d x %d | %s | %s | %.2fx | %.0f | %.0f | %.0f |'
              % (name, count, M, K, Cout, fmt(r['torch']), fmt(r['hip']), r['torch'][0] / r['hip'][0], tf, ex, gb), flush=True)
        del conv, bn, x, xc, r0, rc, pk
        torch.cuda.empty_cache()
    print('| sum of medians x count | | | %.3f | %.3f | %.2fx | | | |' % (tot['torch'], tot['hip'], tot['torch'] / tot['hip']), flush=True)


def modules(a):
    print('\n| module, one frame (6 cameras) | torch ms | hip ms | speed-up |')
    print('|---|---|---|---|')
    cfg = IE.preworld_image_cfg()
    torch.manual_seed(0)
    neck = IE.FPN_LSS(**cfg['neck_cfg']).to(DEV).eval()
    feats = [torch.randn(B, 512, H, W, device=DEV), torch.randn(B, 1024, H // 2, W // 2, device=DEV)]
    dn = IE.DepthNet(512, 512, 32, 88, **cfg['depthnet_cfg']).to(DEV).eval()
    x, mlp = torch.randn(B, 512, H, W, device=DEV), torch.randn(1, B, 27, device=DEV)
    metas = dict(cv_feat_list=[None, None], downsample=16, cv_downsample=4)
    # a fixed random cost volume on the device stands for ops.stereo_cost_volume, which is the same kernel on both paths (the
    # module's own no-previous-frame branch builds its zeros on the host: 95 MB per call, more than the module itself takes)
    cv = torch.randn(B, 88, 4 * H, 4 * W, device=DEV)
    dn._cost_volume = lambda x, stereo_metas: cv

    def run(mod, impl, *args):
        def f():
            mod.set_conv_impl(impl)
            with torch.no_grad():
                return mod(*args)
        return f
    both = {'torch': 0.0, 'hip': 0.0}
    spread = 0.0
    for name, mod, args in (('FPN_LSS', neck, (feats,)), ('DepthNet (a given cost volume, through cost_volumn_net)', dn, (x, mlp, metas))):
        r = rounds({'torch': run(mod, 'torch', *args), 'hip': run(mod, 'hip', *args)}, a.rounds, a.window)
        print('| %s | %s | %s | %.2fx |' % (name, fmt(r['torch']), fmt(r['hip']), r['torch'][0] / r['hip'][0]), flush=True)
        for p in both:
            both[p] += r[p][0]
            spread += r[p][2] - r[p][1]
    print('| both | %.3f | %.3f | %.2fx (difference %.3f ms, spreads of the rounds add to %.3f ms) |'
          % (both['torch'], both['hip'], both['torch'] / both['hip'], both['torch'] - both['hip'], spread), flush=True)
    del neck, dn
    torch.cuda.empty_cache()


def end_to_end(a, path):
    print('\n| image -> occupancy (C3, 1 GPU, serial), f32, attn hip, Linears hip | convolutions | samples/s | ms per sample | image branch ms |')
    print('|---|---|---|---|---|')
    for _ in range(a.e2e_rounds):
        for conv in ('torch', 'hip'):
            r = path.run('none', 'hip', a.e2e_steps, 'hip', conv)
            print('| %s | %s | %.2f | %.2f | %.2f |' % (r['image_branch_dtype'], conv, r['value'], r['ms_per_sample'], r['image_branch_ms']), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.3, help='seconds of device time per timed batch')
    ap.add_argument('--e2e-steps', type=int, default=5)
    ap.add_argument('--e2e-rounds', type=int, default=3)
    ap.add_argument('--no-split', action='store_true')
    ap.add_argument('--no-roles', action='store_true')
    ap.add_argument('--no-modules', action='store_true')
    ap.add_argument('--no-e2e', action='store_true')
    a = ap.parse_args()
    assert a.rounds >= 3, 'at least 3 rounds'
    p = torch.cuda.get_device_properties(0)
    print('device: %s, %d CUs, torch %s, hip %s; times are ms as median (min .. max) of %d rounds, %.1f s of device time per timed batch\n'
          % (p.name, p.multi_processor_count, torch.__version__, torch.version.hip, a.rounds, a.window))
    path = None
    if not a.no_split:
        path = split(a)
    if not a.no_roles:
        role_rows(a)
    if not a.no_modules:
        modules(a)
    if not a.no_e2e:
        if path is None:
            from bench_image_path import ImagePath
            path = ImagePath(DEV)
        end_to_end(a, path)


if __name__ == '__main__':
    main()
