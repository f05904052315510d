"""Swin block Linears: the torch modules of preworld_amd/image_encoder.py against the fused HIP GEMM (linear_impl='hip',
csrc/pw_swin_linear.hip), alternating in one process.

Per real stage shape of the C3 sample (12 frames: 6 cameras x key + adjacent; window 12, head width 32) and dtype (fp32; bf16 =
the fp32 module under autocast): each of the four roles alone -- qkv = Linear(LN1(x)), x + proj(a), GELU(fc1(LN2(x))), x + fc2(h) --
as the torch ops the block runs today against one ops.swin_linear call, and the whole SwinBlock with attn_impl='hip' on both paths.
Device events around batches of calls sized to --window seconds, after a warm-up; --rounds repeats, old and new alternating inside
every round; median and the min .. max spread are reported.  FLOPs are 2 M K N (the kernel EXECUTES three times that in fp32 mode:
three fp16 products per fp32 product); bytes are algorithmic, from shapes: x read once, out written once, residual read once, the
weight once.

Then the whole Swin-B forward (6 x 3 x 512 x 1408) and, unless --no-e2e, image -> occupancy samples/s of tools/bench_image_path.py,
both dtypes, both paths.  Prints a markdown report (profiles/swin_linear.md keeps one)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from preworld_amd import image_encoder as IE, ops  # noqa: E402
from bench_swin_attn import DEV, FRAMES, STAGES, WS, fmt, rounds  # noqa: E402


def role_rows(a):
    print('| stage H x W x C | dtype | role | M x K x N | torch ms | hip ms | speed-up | hip TFLOP/s (2MKN) | executed TFLOP/s | hip GB/s |')
    print('|---|---|---|---|---|---|---|---|---|---|')
    for H, W, C, heads in STAGES:
        M = FRAMES * H * W
        for amp, dname in ((False, 'f32'), (True, 'bf16')):
            torch.manual_seed(1)
            blk = IE.SwinBlock(C, heads, 4 * C, WS, False, attn_impl='hip', linear_impl='hip').to(DEV).eval()
            m, fc1, fc2 = blk.attn.w_msa, blk.ffn.layers[0][0], blk.ffn.layers[1]
            dt = torch.bfloat16 if amp else torch.float32
            x = torch.randn(M, C, device=DEV)
            att = torch.randn(M, C, device=DEV, dtype=dt)
            hid = torch.randn(M, 4 * C, device=DEV, dtype=dt)
            with torch.no_grad():
                pq, pp, p1, p2 = blk._packed(dt)
            cast = lambda: torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp)
            roles = [
                ('qkv', C, 3 * C, lambda: m.qkv(blk.norm1(x)), lambda: ops.swin_linear(x, pq, ln=True), 4, dt.itemsize, 0),
                ('proj', C, C, lambda: m.proj(att) + x, lambda: ops.swin_linear(att, pp, residual=x), dt.itemsize, 4, 4),
                ('fc1', C, 4 * C, lambda: blk.ffn.layers[0](blk.norm2(x)), lambda: ops.swin_linear(x, p1, ln=True, act='gelu'), 4, dt.itemsize, 0),
                ('fc2', 4 * C, C, lambda: x + blk.ffn.layers[1](hid), lambda: ops.swin_linear(hid, p2, residual=x), dt.itemsize, 4, 4),
            ]
            for name, K, N, t_fn, h_fn, bx, bo, br in roles:
                def torch_f(t_fn=t_fn):
                    with torch.no_grad(), cast():
                        return t_fn()
                r = rounds({'torch': torch_f, 'hip': h_fn}, a.rounds, a.window)
                tf = 2.0 * M * K * N / 1e12 / (r['hip'][0] * 1e-3)
                gb = (M * K * bx + M * N * (bo + br) + N * K * (2 if amp else 4)) / 1e9 / (r['hip'][0] * 1e-3)
                print('| %d x %d x %d | %s | %s | %d x %d x %d | %s | %s | %.2fx | %.0f | %.0f | %.0f |'
                      % (H, W, C, dname, name, M, K, N, fmt(r['torch']), fmt(r['hip']), r['torch'][0] / r['hip'][0], tf, tf * (1 if amp else 3), gb),
                      flush=True)
            x3 = x.view(FRAMES, H * W, C)

            def block(impl):
                def f():
                    blk.set_linear_impl(impl)
                    with torch.no_grad(), cast():
                        return blk(x3, (H, W))
                return f
            r = rounds({'torch': block('torch'), 'hip': block('hip')}, a.rounds, a.window)
            print('| %d x %d x %d | %s | whole block (attn hip) | | %s | %s | %.2fx | | | |'
                  % (H, W, C, dname, fmt(r['torch']), fmt(r['hip']), r['torch'][0] / r['hip'][0]), flush=True)
            del blk, x, att, hid, pq, pp, p1, p2, roles
            torch.cuda.empty_cache()


def swin_b(a):
    print('\n| Swin-B forward, 6 x 3 x 512 x 1408, attn_impl=hip | torch Linears ms | hip Linears ms | speed-up |')
    print('|---|---|---|---|')
    torch.manual_seed(0)
    net = IE.SwinTransformer(**IE.preworld_image_cfg()['backbone_cfg'], attn_impl='hip').to(DEV).eval()
    x = torch.randn(6, 3, 512, 1408, device=DEV)
    for amp in (False, True):
        def run(impl):
            def f():
                net.set_linear_impl(impl)
                with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
                    return net(x)
            return f
        r = rounds({'torch': run('torch'), 'hip': run('hip')}, a.rounds, a.window)
        print('| %s | %s | %s | %.2fx |' % ('bf16 autocast' if amp else 'f32', fmt(r['torch']), fmt(r['hip']), r['torch'][0] / r['hip'][0]), flush=True)
    del net
    torch.cuda.empty_cache()


def end_to_end(a):
    from bench_image_path import ImagePath
    print('\n| image -> occupancy (C3, 1 GPU, serial), attn hip | Linears | samples/s | ms per sample | image branch ms |')
    print('|---|---|---|---|---|')
    path = ImagePath(DEV)
    for amp in ('none', 'bf16'):
        for _ in range(a.e2e_rounds):
            for lin in ('torch', 'hip'):
                r = path.run(amp, 'hip', a.e2e_steps, lin)
                print('| %s | %s | %.2f | %.2f | %.2f |' % (r['image_branch_dtype'], lin, r['value'], r['ms_per_sample'], r['image_branch_ms']), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.3, help='seconds of device time per timed batch')
    ap.add_argument('--e2e-steps', type=int, default=5)
    ap.add_argument('--e2e-rounds', type=int, default=2)
    ap.add_argument('--no-stages', action='store_true')
    ap.add_argument('--no-model', action='store_true')
    ap.add_argument('--no-e2e', action='store_true')
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print('device: %s, %d CUs, torch %s, hip %s; times are ms as median (min .. max) of %d rounds, %.1f s of device time per timed batch\n'
          % (p.name, p.multi_processor_count, torch.__version__, torch.version.hip, a.rounds, a.window))
    if not a.no_stages:
        role_rows(a)
    if not a.no_model:
        swin_b(a)
    if not a.no_e2e:
        end_to_end(a)


if __name__ == '__main__':
    main()
