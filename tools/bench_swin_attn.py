"""Swin window attention: the torch path of preworld_amd/image_encoder.py against the fused HIP kernel (attn_impl='hip',
csrc/pw_swin_attn.hip), alternating in one process.

Per real stage shape of the C3 sample (12 frames: 6 cameras x key + adjacent; window 12, head width 32), shift 0 and 6, fp32 and
bf16: ShiftWindowMSA as a whole on both paths, its two Linears alone on the un-padded tokens, and the kernel alone on a ready qkv.
"attention alone" of a path = its module time - the Linears' time: for the torch path that is pad, roll, partition, the qkv
permute, the expanded bias + mask, SDPA, reverse, roll back, crop (and the Linears' extra work on padded tokens, which only that
path has).  Device events around batches of calls sized to --window seconds, after a warm-up; --rounds repeats, old and new
alternating inside every round; median and the min .. max spread are reported.  Bytes and FLOPs are algorithmic, from shapes:
qkv read once + out written once, 4 N^2 d per (window, head).

Then the whole Swin-B forward (6 x 3 x 512 x 1408) and, unless --no-e2e, image -> occupancy samples/s of tools/bench_image_path.py,
both dtypes, both paths.  Prints a markdown report (profiles/swin_attention.md keeps one)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from preworld_amd import image_encoder as IE, ops  # noqa: E402

DEV = 'cuda:0'
STAGES = [(128, 352, 128, 4), (64, 176, 256, 8), (32, 88, 512, 16), (16, 44, 1024, 32)]      # H, W, C, heads
FRAMES, WS = 12, 12


def timed(fn, window):
    """ms per call: events around a batch sized to `window` seconds"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    n = max(3, int(window * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def rounds(fns, n_rounds, window):
    """{name: (median, min, max)} with the functions alternating inside every round"""
    for f in fns.values():          # warm-up: allocator, kernel selection, mask caches
        for _ in range(3):
            f()
    res = {k: [] for k in fns}
    for _ in range(n_rounds):
        for k, f in fns.items():
            res[k].append(timed(f, window))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


def fmt(t):
    return '%.3f (%.3f .. %.3f)' % t


def stage_rows(a):
    print('| stage H x W x C, heads | shift | dtype | torch module ms | hip module ms | Linears ms | torch attention ms | hip attention ms | kernel alone ms | speed-up of attention | kernel GB/s | kernel TFLOP/s |')
    print('|---|---|---|---|---|---|---|---|---|---|---|---|')
    for H, W, C, heads in STAGES:
        for shift in (0, WS // 2):
            for dt, dname in ((torch.float32, 'f32'), (torch.bfloat16, 'bf16')):
                torch.manual_seed(1)
                m = IE.ShiftWindowMSA(C, heads, WS, shift).to(DEV).eval()
                with torch.no_grad():
                    m.w_msa.relative_position_bias_table.normal_(std=0.5)
                m = m.to(dt)
                x = torch.randn(FRAMES, H * W, C, device=DEV, dtype=dt)
                with torch.no_grad():
                    qkv = m.w_msa.qkv(x)
                    pad = m.w_msa.qkv.bias.detach().clone()
                    table = m.w_msa.relative_position_bias_table.detach().float()
                    att = torch.randn(FRAMES, H * W, C, device=DEV, dtype=dt)

                def run(impl):
                    def f():
                        with torch.no_grad():
                            m.set_attn_impl(impl)
                            return m(x, (H, W))
                    return f

                def linears():
                    with torch.no_grad():
                        m.w_msa.qkv(x)
                        return m.w_msa.proj(att)

                def kernel():
                    return ops.swin_window_attention(qkv, pad, table, H, W, heads, WS, shift, m.w_msa.scale)
                r = rounds({'torch': run('torch'), 'hip': run('hip'), 'lin': linears, 'kern': kernel}, a.rounds, a.window)
                m._mask_cache.clear()
                e = 4 if dt == torch.float32 else 2
                nw = -(-H // WS) * -(-W // WS)
                gbytes = FRAMES * H * W * 4 * C * e / 1e9
                tflop = FRAMES * nw * heads * 4 * (WS * WS) ** 2 * (C // heads) / 1e12
                t_att, h_att = r['torch'][0] - r['lin'][0], r['hip'][0] - r['lin'][0]
                print('| %d x %d x %d, %d | %d | %s | %s | %s | %s | %.3f | %.3f | %s | %.2fx | %.0f | %.1f |'
                      % (H, W, C, heads, shift, dname, fmt(r['torch']), fmt(r['hip']), fmt(r['lin']), t_att, h_att, fmt(r['kern']),
                         t_att / h_att, gbytes / (r['kern'][0] * 1e-3), tflop / (r['kern'][0] * 1e-3)), flush=True)
                del m, x, qkv, att
                torch.cuda.empty_cache()


def swin_b(a):
    print('\n| Swin-B forward, 6 x 3 x 512 x 1408 | torch ms | hip ms | speed-up |')
    print('|---|---|---|---|')
    torch.manual_seed(0)
    net = IE.SwinTransformer(**IE.preworld_image_cfg()['backbone_cfg']).to(DEV).eval()
    x = torch.randn(6, 3, 512, 1408, device=DEV)
    for amp in (False, True):
        def run(impl):
            def f():
                net.set_attn_impl(impl)
                with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
                    return net(x)
            return f
        r = rounds({'torch': run('torch'), 'hip': run('hip')}, a.rounds, a.window)
        print('| %s | %s | %s | %.2fx |' % ('bf16 autocast' if amp else 'f32', fmt(r['torch']), fmt(r['hip']), r['torch'][0] / r['hip'][0]), flush=True)
    del net
    torch.cuda.empty_cache()


def end_to_end(a):
    from bench_image_path import ImagePath
    print('\n| image -> occupancy (C3, 1 GPU, serial) | attention | samples/s | ms per sample | image branch ms |')
    print('|---|---|---|---|---|')
    path = ImagePath(DEV)
    for amp in ('none', 'bf16'):
        for _ in range(a.e2e_rounds):
            for attn in ('torch', 'hip'):
                r = path.run(amp, attn, a.e2e_steps)
                print('| %s | %s | %.2f | %.2f | %.2f |' % (r['image_branch_dtype'], attn, r['value'], r['ms_per_sample'], r['image_branch_ms']), flush=True)


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
        stage_rows(a)
    if not a.no_model:
        swin_b(a)
    if not a.no_e2e:
        end_to_end(a)


if __name__ == '__main__':
    main()
