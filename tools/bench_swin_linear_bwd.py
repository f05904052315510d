"""Swin block Linears, backward: the torch modules of preworld_amd/image_encoder.py against the HIP gradient kernels
(linear_impl='hip_grad', csrc/pw_swin_linear_bwd.hip), float32, alternating in one process.  Both sides run attn_impl='hip_grad'.

Per real stage shape of the C3 sample (12 frames, window 12, head width 32) and role (qkv, proj, fc1, fc2), each piece of
include/preworld_hip_swin_linear_bwd.h against the torch ops it replaces, on ready tensors:
    (a) data gradient      ops.swin_linear_backward_data      against  g @ W
    (b) GELU gradient      ops.swin_linear_backward_gelu      against  gelu'(fc1(LN(x))) * dh recomputed by torch (fc1 only)
    (c) weight gradient    ops.swin_linear_backward_weight    against  g^T @ pro(x) and g.sum(0), pro(x) given to torch ready-made
    (d) LayerNorm gradient ops.swin_layernorm_backward        against  torch.ops.aten.native_layer_norm_backward (qkv, fc1 only)
with, for (c), 2 M K N FLOPs (the kernel executes three times that), algorithmic bytes (g and x read once, dW written once), the
split over M and the workspace.  Then one SwinBlock forward + backward per stage, and Swin-B forward + backward on 6 images with
peak memory.  Timing as tools/bench_swin_attn_bwd.py: device events around batches sized to --window seconds, --rounds repeats,
the two paths alternating inside every round, median and min .. max.  Prints a markdown report
(profiles/swin_linear_backward.md keeps one)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_swin_attn import DEV, FRAMES, STAGES, WS, fmt, rounds  # noqa: E402
from bench_swin_attn_bwd import peak_mb  # noqa: E402
from preworld_amd import _lib, image_encoder as IE, ops  # noqa: E402


def ratio(r, a, b):
    return '%.2fx (%.2f .. %.2f)' % (r[a][0] / r[b][0], r[a][1] / r[b][2], r[a][2] / r[b][1])


def piece_rows(a):
    print('| stage C | role | M x K x N | piece | torch ms | hip ms | speed-up | note |')
    print('|---|---|---|---|---|---|---|---|')
    for H, W, C, heads in STAGES:
        M = FRAMES * H * W
        torch.manual_seed(1)
        blk = IE.SwinBlock(C, heads, 4 * C, WS, False, attn_impl='hip_grad', linear_impl='hip_grad').to(DEV)
        m, fc1, fc2 = blk.attn.w_msa, blk.ffn.layers[0][0], blk.ffn.layers[1]
        with torch.no_grad():
            packs, packs_t = blk._packed(torch.float32), blk._packed_t()
        for (name, lin, norm), pk, pt in zip((('qkv', m.qkv, blk.norm1), ('proj', m.proj, None), ('fc1', fc1, blk.norm2), ('fc2', fc2, None)),
                                             packs, packs_t):
            N, K = lin.weight.shape
            x = torch.randn(M, K, device=DEV)
            g = torch.randn(M, N, device=DEV)
            w = lin.weight.detach()
            head = '| %d | %s | %d x %d x %d |' % (C, name, M, K, N)
            with torch.no_grad():
                xn = x if norm is None else norm(x)
                r = rounds({'torch': lambda: g @ w, 'hip': lambda: ops.swin_linear_backward_data(g, pt)}, a.rounds, a.window)
                print('%s (a) data | %s | %s | %s | |' % (head, fmt(r['torch']), fmt(r['hip']), ratio(r, 'torch', 'hip')), flush=True)
                if name == 'fc1':
                    def torch_gelu():
                        y = F.linear(norm(x), w, lin.bias)
                        return torch.ops.aten.gelu_backward(g, y)
                    r = rounds({'torch': torch_gelu, 'hip': lambda: ops.swin_linear_backward_gelu(x, pk, g, norm.eps)}, a.rounds, a.window)
                    print('%s (b) GELU | %s | %s | %s | torch recomputes LN and fc1 too; in training it reads the stored pre-activation |'
                          % (head, fmt(r['torch']), fmt(r['hip']), ratio(r, 'torch', 'hip')), flush=True)

                def torch_w():
                    return g.t() @ xn, g.sum(0)
                r = rounds({'torch': torch_w, 'hip': lambda: ops.swin_linear_backward_weight(g, x, pk, ln=norm is not None,
                                                                                             eps=norm.eps if norm is not None else 0.0)},
                           a.rounds, a.window)
                t = r['hip'][0] * 1e-3
                nbytes = _lib.call_size('pw_swin_linear_backward_weight_workspace_bytes', M, K, N, int(norm is not None))
                print('%s (c) weight + bias | %s | %s | %s | %.0f TFLOP/s (2MKN), %.0f executed, %.0f GB/s algorithmic; split %d, workspace %.1f MB |'
                      % (head, fmt(r['torch']), fmt(r['hip']), ratio(r, 'torch', 'hip'), 2.0 * M * K * N / 1e12 / t, 6.0 * M * K * N / 1e12 / t,
                         4.0 * (M * K + M * N + N * K) / 1e9 / t, -(-M // _lib.PW_SWIN_LINEAR_BWD['PW_SWIN_LINEAR_BWD_SPLIT_ROWS']), nbytes / 2 ** 20),
                      flush=True)
                if norm is not None:
                    dxn = torch.randn(M, K, device=DEV)
                    mean = x.mean(-1, keepdim=True)
                    rstd = (x.var(-1, unbiased=False, keepdim=True) + norm.eps).rsqrt()

                    def torch_ln():
                        return torch.ops.aten.native_layer_norm_backward(dxn, x, [K], mean, rstd, norm.weight, norm.bias, [True, True, True])
                    r = rounds({'torch': torch_ln, 'hip': lambda: ops.swin_layernorm_backward(dxn, x, norm.weight, eps=norm.eps)}, a.rounds, a.window)
                    print('%s (d) LayerNorm | %s | %s | %s | hip recomputes the statistics |' % (head, fmt(r['torch']), fmt(r['hip']), ratio(r, 'torch', 'hip')),
                          flush=True)
            del x, g, xn
            torch.cuda.empty_cache()
        del blk
        torch.cuda.empty_cache()


def block_rows(a):
    print('\n| SwinBlock forward + backward, H x W x C | torch Linears ms | hip_grad Linears ms | speed-up | torch peak MB | hip_grad peak MB |')
    print('|---|---|---|---|---|---|')
    for H, W, C, heads in STAGES:
        torch.manual_seed(1)
        blk = IE.SwinBlock(C, heads, 4 * C, WS, True, attn_impl='hip_grad').to(DEV)
        x = torch.randn(FRAMES, H * W, C, device=DEV, requires_grad=True)
        dy = torch.randn(FRAMES, H * W, C, device=DEV)

        def run(impl):
            def f():
                blk.set_linear_impl(impl)
                blk(x, (H, W)).backward(dy)
                x.grad = None
                blk.zero_grad(set_to_none=True)
            return f
        r = rounds({'torch': run('torch'), 'hip': run('hip_grad')}, a.rounds, a.window)
        mem = {k: peak_mb(run(k)) for k in ('torch', 'hip_grad')}
        print('| %d x %d x %d | %s | %s | %s | %.0f | %.0f |' % (H, W, C, fmt(r['torch']), fmt(r['hip']), ratio(r, 'torch', 'hip'), mem['torch'],
                                                               mem['hip_grad']), flush=True)
        del blk, x, dy
        torch.cuda.empty_cache()


def swin_b(a):
    print('\n| Swin-B forward + backward, 6 x 3 x 512 x 1408, f32 | torch Linears ms | hip_grad Linears ms | speed-up | torch peak MB | hip_grad peak MB |')
    print('|---|---|---|---|---|---|')
    torch.manual_seed(0)
    net = IE.SwinTransformer(**dict(IE.preworld_image_cfg()['backbone_cfg'], attn_impl='hip_grad')).to(DEV).train()
    x = torch.randn(6, 3, 512, 1408, device=DEV)

    def run(impl):
        def f():
            net.set_linear_impl(impl)
            sum(o.square().sum() for o in net(x)).backward()
            net.zero_grad(set_to_none=True)
        return f
    r = rounds({'torch': run('torch'), 'hip': run('hip_grad')}, a.rounds, a.window)
    mem = {k: peak_mb(run(k)) for k in ('torch', 'hip_grad')}
    print('| f32 | %s | %s | %s | %.0f | %.0f |' % (fmt(r['torch']), fmt(r['hip']), ratio(r, 'torch', 'hip'), mem['torch'], mem['hip_grad']), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.3, help='seconds of device time per timed batch')
    ap.add_argument('--no-pieces', action='store_true')
    ap.add_argument('--no-blocks', action='store_true')
    ap.add_argument('--no-model', action='store_true')
    a = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print('device: %s, %d CUs, torch %s, hip %s; times are ms as median (min .. max) of %d rounds, %.1f s of device time per timed batch; '
          'a speed-up is median / median (lowest .. highest from the extremes of the rounds)\n'
          % (p.name, p.multi_processor_count, torch.__version__, torch.version.hip, a.rounds, a.window))
    if not a.no_pieces:
        piece_rows(a)
    if not a.no_blocks:
        block_rows(a)
    if not a.no_model:
        swin_b(a)


if __name__ == '__main__':
    main()
