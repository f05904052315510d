"""Swin window attention, forward + backward: the torch path of preworld_amd/image_encoder.py against the fused HIP kernels
(attn_impl='hip_grad': csrc/pw_swin_attn.hip forward, csrc/pw_swin_attn_bwd.hip backward), alternating in one process.

Per real stage shape of the C3 sample (12 frames, window 12, head width 32), shift 0 and 6, fp32 and bf16 autocast: one forward +
backward of ShiftWindowMSA (input and all parameters require grad) on both paths, the backward kernel alone on ready tensors, and
torch.cuda.max_memory_allocated of one forward + backward above what was resident before it.  Timing as tools/bench_swin_attn.py:
device events around batches sized to --window seconds, --rounds repeats, both paths alternating inside every round, median and
min .. max.  Bytes and FLOPs of the kernel are algorithmic, from shapes: qkv and dout read once, dqkv written once; the five
products of the gradient, 10 N^2 d per (window, head) (the kernel recomputes S and dP once more: it executes 14 N^2 d).

Then one Swin-B forward + backward (6 x 3 x 512 x 1408, loss = sum of squares of the outputs) on both paths, time and peak memory.
Prints a markdown report (profiles/swin_attention_backward.md keeps one)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_swin_attn import DEV, FRAMES, STAGES, WS, fmt, rounds  # noqa: E402
from preworld_amd import image_encoder as IE, ops  # noqa: E402


def peak_mb(fn):
    """MB that one call of fn allocates above what is resident before it"""
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def stage_rows(a):
    print('| stage H x W x C, heads | shift | dtype | torch fwd+bwd ms | hip_grad fwd+bwd ms | speed-up | backward kernel alone ms | kernel GB/s | kernel TFLOP/s | torch peak MB | hip_grad peak MB |')
    print('|---|---|---|---|---|---|---|---|---|---|---|')
    for H, W, C, heads in STAGES:
        for shift in (0, WS // 2):
            for amp, dname in ((False, 'f32'), (True, 'bf16 autocast')):
                torch.manual_seed(1)
                m = IE.ShiftWindowMSA(C, heads, WS, shift).to(DEV)
                with torch.no_grad():
                    m.w_msa.relative_position_bias_table.normal_(std=0.5)
                x = torch.randn(FRAMES, H * W, C, device=DEV, requires_grad=True)
                dy = torch.randn(FRAMES, H * W, C, device=DEV)
                dt = torch.bfloat16 if amp else torch.float32
                with torch.no_grad():
                    qkv = m.w_msa.qkv(x).to(dt)
                    pad = m.w_msa.qkv.bias.detach().to(dt)
                    table = m.w_msa.relative_position_bias_table.detach().float()
                    out = ops.swin_window_attention(qkv, pad, table, H, W, heads, WS, shift, m.w_msa.scale)
                    dout = torch.randn_like(out)

                def run(impl):
                    def f():
                        m.set_attn_impl(impl)
                        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
                            y = m(x, (H, W))
                        y.backward(dy.to(y.dtype))
                        x.grad = None
                        m.zero_grad(set_to_none=True)
                    return f

                def kernel():
                    return ops.swin_window_attention_backward(qkv, pad, table, out, dout, H, W, heads, WS, shift, m.w_msa.scale)
                r = rounds({'torch': run('torch'), 'hip': run('hip_grad'), 'kern': kernel}, a.rounds, a.window)
                mem = {k: peak_mb(run(k)) for k in ('torch', 'hip_grad')}
                m._mask_cache.clear()
                e = 2 if amp else 4
                nw = -(-H // WS) * -(-W // WS)
                gbytes = FRAMES * H * W * 7 * C * e / 1e9
                tflop = FRAMES * nw * heads * 10 * (WS * WS) ** 2 * (C // heads) / 1e12
                print('| %d x %d x %d, %d | %d | %s | %s | %s | %.2fx (%.2f .. %.2f) | %s | %.0f | %.1f | %.0f | %.0f |'
                      % (H, W, C, heads, shift, dname, fmt(r['torch']), fmt(r['hip']), r['torch'][0] / r['hip'][0],
                         r['torch'][1] / r['hip'][2], r['torch'][2] / r['hip'][1], fmt(r['kern']), gbytes / (r['kern'][0] * 1e-3),
                         tflop / (r['kern'][0] * 1e-3), mem['torch'], mem['hip_grad']), flush=True)
                del m, x, dy, qkv, out, dout
                torch.cuda.empty_cache()


def swin_b(a):
    print('\n| Swin-B forward + backward, 6 x 3 x 512 x 1408 | torch ms | hip_grad ms | speed-up | torch peak MB | hip_grad peak MB |')
    print('|---|---|---|---|---|---|')
    torch.manual_seed(0)
    net = IE.SwinTransformer(**IE.preworld_image_cfg()['backbone_cfg']).to(DEV).train()
    x = torch.randn(6, 3, 512, 1408, device=DEV)
    for amp in (False, True):
        def run(impl):
            def f():
                net.set_attn_impl(impl)
                with torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
                    outs = net(x)
                sum(o.float().square().sum() for o in outs).backward()
                net.zero_grad(set_to_none=True)
            return f
        r = rounds({'torch': run('torch'), 'hip': run('hip_grad')}, a.rounds, a.window)
        mem = {k: peak_mb(run(k)) for k in ('torch', 'hip_grad')}
        print('| %s | %s | %s | %.2fx (%.2f .. %.2f) | %.0f | %.0f |'
              % ('bf16 autocast' if amp else 'f32', fmt(r['torch']), fmt(r['hip']), r['torch'][0] / r['hip'][0],
                 r['torch'][1] / r['hip'][2], r['torch'][2] / r['hip'][1], mem['torch'], mem['hip_grad']), flush=True)
    del net
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.3, help='seconds of device time per timed batch')
    ap.add_argument('--no-stages', action='store_true')
    ap.add_argument('--no-model', action='store_true')
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print('device: %s, %d CUs, torch %s, hip %s; times are ms as median (min .. max) of %d rounds, %.1f s of device time per timed batch; '
          'a speed-up is median / median (lowest .. highest from the extremes of the rounds)\n'
          % (p.name, p.multi_processor_count, torch.__version__, torch.version.hip, a.rounds, a.window))
    if not a.no_stages:
        stage_rows(a)
    if not a.no_model:
        swin_b(a)


if __name__ == '__main__':
    main()
