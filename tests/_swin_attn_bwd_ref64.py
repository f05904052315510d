"""The yardstick of the fused window attention's BACKWARD (pw_swin_window_attention_backward, ops.swin_window_attention_backward,
attn_impl='hip_grad'): float64 autograd straight through _swin_attn_ref64.swin_attn_ref64, the reference's own composition (pad, roll,
partition, slice-loop mask, table[index], explicit softmax) with qkv, pad_qkv and table as leaves.  Nothing here comes from the
kernel or from preworld_amd/image_encoder.py.

THE COTANGENT of a case is a seeded standard normal of the output's shape (bf16 cases: rounded to bf16).

THE CASES are a subset of _swin_attn_ref64.CASES (already the smallest maps at which the kernel can go wrong); together they cover
key tiles 1, 4 and 9, head widths 8, 16 and 32 and the NULL pad vector (tests/test_swin_attn_bwd_cpu.py asserts it).

THE BOUND.  Per case and per gradient (dqkv, dpad, dtable): max |g - g64| / max |g64| <= 4 x BWD_FLOORS[case][grad].  The floor is the
same figure for the backward of the EXISTING torch path (IE.ShiftWindowMSA 'torch', proj = identity) on the CPU in float32 (bf16 cases:
in bf16) fed the same qkv and cotangent: the QkvLookup.rows buffer of the harness is made a leaf, its row 0 collects dpad and the rest
is dqkv.  tests/test_swin_attn_bwd_cpu.py measures it and asserts the torch path stays under each entry (rounded up to two digits);
no floor is taken from the kernel.  The factor 4 is the forward's: device expf, summation order, matrix-core products.  No element is
excluded.  Where g64 is identically zero (dpad without padding; its q third always) the kernel's value must be exactly zero.

The module and toy-model floors at the bottom are float32 against float64 of the torch path on the CPU, measured by the same file."""
import contextlib
import functools

import numpy as np
import torch

import _swin_attn_ref64 as R

NAMES = ('tile_pad_s0', 'tile_pad_s6', 'tile_nopad_s0', 'tile_nopad_s6', 'one_window_nine_regions', 'ws7_no_bias', 'narrow_d8_s2',
         'narrow_d8_s0', 'narrow_d16_s2', 'many_heads_s6', 'peaked_s6', 'padded_keys_matter', 'range_2m12', 'range_2p8',
         'bf16_tile_pad_s6', 'bf16_tile_nopad_s0')
GRADS = ('dqkv', 'dtable', 'dpad')

# max |g_torch - g64| / max |g64| of the torch path's backward on the CPU (see the module docstring), rounded up to two digits;
# None: g64 is identically zero (no padded token, or no pad vector) and so must the gradient be
BWD_FLOORS = {
    'tile_pad_s0':               dict(dqkv=3.4e-07, dtable=1.5e-07, dpad=9.3e-07),          # measured 3.341e-07, 1.455e-07, 9.282e-07
    'tile_pad_s6':               dict(dqkv=3.2e-07, dtable=2.3e-07, dpad=5.0e-07),          # measured 3.182e-07, 2.223e-07, 4.953e-07
    'tile_nopad_s0':             dict(dqkv=5.1e-07, dtable=4.1e-07, dpad=None),             # measured 5.091e-07, 4.073e-07, 0
    'tile_nopad_s6':             dict(dqkv=4.1e-07, dtable=4.9e-07, dpad=None),             # measured 4.067e-07, 4.870e-07, 0
    'one_window_nine_regions':   dict(dqkv=3.6e-07, dtable=1.3e-07, dpad=None),             # measured 3.552e-07, 1.207e-07, 0
    'ws7_no_bias':               dict(dqkv=1.9e-07, dtable=1.7e-07),                        # measured 1.811e-07, 1.655e-07
    'narrow_d8_s2':              dict(dqkv=1.5e-07, dtable=2.4e-07, dpad=1.9e-07),          # measured 1.406e-07, 2.338e-07, 1.816e-07
    'narrow_d8_s0':              dict(dqkv=2.6e-07, dtable=1.3e-07, dpad=2.1e-07),          # measured 2.556e-07, 1.251e-07, 2.048e-07
    'narrow_d16_s2':             dict(dqkv=2.5e-07, dtable=1.6e-07, dpad=1.8e-07),          # measured 2.465e-07, 1.538e-07, 1.772e-07
    'many_heads_s6':             dict(dqkv=4.1e-07, dtable=3.3e-07, dpad=7.2e-07),          # measured 4.091e-07, 3.246e-07, 7.102e-07
    'peaked_s6':                 dict(dqkv=1.4e-06, dtable=1.3e-06, dpad=9.4e-07),          # measured 1.311e-06, 1.223e-06, 9.371e-07
    'padded_keys_matter':        dict(dqkv=5.6e-07, dtable=3.2e-07, dpad=5.0e-07),          # measured 5.560e-07, 3.126e-07, 4.960e-07
    'range_2m12':                dict(dqkv=2.6e-07, dtable=3.1e-07, dpad=4.1e-07),          # measured 2.514e-07, 3.002e-07, 4.028e-07
    'range_2p8':                 dict(dqkv=7.2e-03, dtable=7.7e+00, dpad=4.0e-03),          # measured 7.122e-03, 7.657e+00, 3.962e-03
    'bf16_tile_pad_s6':          dict(dqkv=2.1e-03, dtable=1.4e-02, dpad=7.3e-02),          # measured 2.072e-03, 1.367e-02, 7.204e-02
    'bf16_tile_nopad_s0':        dict(dqkv=2.6e-03, dtable=1.4e-02, dpad=None),             # measured 2.524e-03, 1.320e-02, 0
}

# ShiftWindowMSA(128, 4, 12, 6) with real Linears on a 13 x 25 map, B = 2 (module_case): float32 against float64 on the CPU, on one
# thread (_repeatable): the two weight gradients are GEMMs whose blocking would otherwise follow the core count
MODULE_FLOORS = {
    'x':                                     6.1e-07,      # measured 6.058e-07
    'w_msa.relative_position_bias_table':    5.4e-07,      # measured 5.323e-07
    'w_msa.qkv.weight':                      5.5e-07,      # measured 5.482e-07
    'w_msa.qkv.bias':                        3.1e-07,      # measured 3.044e-07
    'w_msa.proj.weight':                     4.8e-07,      # measured 4.796e-07
    'w_msa.proj.bias':                       1.1e-07,      # measured 1.089e-07
}

# the toy Swin (synth.small_swin_cfg, seeded weights), loss = sum of squares of the outputs: the largest float32-against-float64
# error max |g32 - g64| / max |g64| over its parameters on the CPU
TOY_FLOOR = 2.4e-06      # measured 2.354e-06


def padded(case):
    return case.H % case.ws != 0 or case.W % case.ws != 0


@functools.lru_cache(maxsize=None)
def cotangent(name):
    """float32 CPU tensor (B, H, W, C) whose values are representable in the case's dtype"""
    c = R.CASES[name]
    rs = np.random.RandomState(5000 + c.seed)
    g = torch.from_numpy(rs.standard_normal((c.B, c.H, c.W, c.heads * c.d)).astype(np.float32))
    return g.bfloat16().float() if c.dtype == 'bf16' else g


def _grads64(name):
    c = R.CASES[name]
    qkv, pad, table, scale = R.inputs(name)
    qkv = qkv.double().requires_grad_(True)
    pad = None if pad is None else pad.double().requires_grad_(True)
    table = table.double().requires_grad_(True)
    out = R.swin_attn_ref64(qkv, pad, table, c.heads, c.ws, c.shift, scale)
    (out * cotangent(name).double()).sum().backward()
    return dict(dqkv=qkv.grad, dtable=table.grad, dpad=None if pad is None else pad.grad)


@functools.lru_cache(maxsize=None)
def reference(name):
    """{'dqkv' (B, H, W, 3C), 'dtable' ((2 ws - 1)^2, heads), 'dpad' (3C) or None}: float64, computed once and shared (do not modify)"""
    return _grads64(name)


@contextlib.contextmanager
def _repeatable():
    """a CPU measurement that gives the same figure on every machine and run: one thread, so that a GEMM's blocking and every
    reduction's order do not follow the core count, and the backward of a lookup (rows[x], table[index]) adds duplicates in index
    order, not in the order the threads get to them"""
    was, threads = torch.are_deterministic_algorithms_enabled(), torch.get_num_threads()
    torch.use_deterministic_algorithms(True)
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)
        torch.use_deterministic_algorithms(was)


def torch_path_grads(name, dtype=None):
    """the same three gradients from the backward of the existing torch path on the CPU (float32, bf16 cases bf16, or `dtype`)"""
    c = R.CASES[name]
    m, x, hw = R.attention_module(name, 'torch', dtype=dtype)
    rows = m.w_msa.qkv.rows
    rows.requires_grad_(True)
    with _repeatable():
        out = m(x, hw).view(c.B, c.H, c.W, -1)
        (out * cotangent(name).to(out.dtype)).sum().backward()
    C3 = rows.shape[1]
    return dict(dqkv=rows.grad[1:].view(c.B, c.H, c.W, C3), dtable=m.w_msa.relative_position_bias_table.grad,
                dpad=rows.grad[0] if c.bias_pad else None)


def rel_err(g, g64):
    """max |g - g64| / max |g64| over every element; g64 == 0 everywhere: 0.0 if g is exactly zero, else inf"""
    scale = float(g64.abs().max())
    if scale == 0.0:
        return 0.0 if not bool(g.double().abs().max() > 0) else float('inf')
    return float((g.double() - g64).abs().max() / scale)


def check(name, got, say=None):
    """got: {'dqkv', 'dtable', 'dpad'} of a case against the yardstick under 4 x the floors; prints each figure before it asserts"""
    ref = reference(name)
    C = R.CASES[name].heads * R.CASES[name].d
    for k in GRADS:
        g64, g = ref[k], got[k]
        if g64 is None:
            assert g is None, (name, k)
            continue
        assert tuple(g.shape) == tuple(g64.shape), (name, k, tuple(g.shape))
        err, floor = rel_err(g.cpu(), g64), BWD_FLOORS[name][k]
        if say:
            print('%s %s: %s %.3e, bound %s' % (name, k, say, err, 'exactly 0' if floor is None else '%.3e (4 x floor %.1e)' % (4 * floor, floor)))
        if floor is None:
            assert float(g64.abs().max()) == 0.0 and err == 0.0, (name, k, err)
        else:
            assert err <= 4 * floor, (name, k, err)
    if ref['dpad'] is not None:                                   # a padded query has no output
        assert float(ref['dpad'][:C].abs().max()) == 0.0 and float(got['dpad'][:C].double().abs().max()) == 0.0, name


# ------------------------------------------------------------------------------------------ a module with real Linears
MODULE_CASE = dict(embed_dims=128, heads=4, ws=12, shift=6, H=13, W=25, B=2)
MODULE_GRADS = ('x', 'w_msa.relative_position_bias_table', 'w_msa.qkv.weight', 'w_msa.qkv.bias', 'w_msa.proj.weight', 'w_msa.proj.bias')


def module_case(attn_impl, dtype=torch.float32, device='cpu'):
    """(ShiftWindowMSA with seeded weights, input (B, H*W, C) requiring grad, hw_shape, cotangent)"""
    from preworld_amd import image_encoder as IE
    mc = MODULE_CASE
    g = torch.Generator().manual_seed(91)
    m = IE.ShiftWindowMSA(mc['embed_dims'], mc['heads'], mc['ws'], mc['shift'], attn_impl=attn_impl)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 if p.dim() == 2 and p.shape[1] == mc['heads'] else 0.1))
    x = torch.randn(mc['B'], mc['H'] * mc['W'], mc['embed_dims'], generator=g)
    dy = torch.randn(mc['B'], mc['H'] * mc['W'], mc['embed_dims'], generator=g)
    return m.to(device, dtype), x.to(device, dtype).requires_grad_(True), (mc['H'], mc['W']), dy.to(device, dtype)


def module_grads(attn_impl, dtype=torch.float32, device='cpu'):
    m, x, hw, dy = module_case(attn_impl, dtype, device)
    with _repeatable() if device == 'cpu' else contextlib.nullcontext():
        y = m(x, hw)
        (y * dy).sum().backward()
    grads = {'x': x.grad}
    grads.update({n: p.grad for n, p in m.named_parameters()})
    return m, y.detach(), grads


@functools.lru_cache(maxsize=None)
def module_reference():
    """float64 'torch' on the CPU, computed once"""
    return module_grads('torch', torch.float64)[2]


# ------------------------------------------------------------------------------------------ the toy Swin
def toy_grads(attn_impl, dtype=torch.float32, device='cpu'):
    """{parameter name: gradient} of sum(o^2 for o in outputs) of the toy Swin with its seeded weights"""
    from preworld_amd import image_encoder as IE, synth as S
    net = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl=attn_impl).eval()
    net.load_state_dict(S.seeded_module_state(net, 51), strict=False)
    net = net.to(device, dtype)
    x = torch.from_numpy(np.random.RandomState(52).standard_normal((2, 3, 64, 96)).astype(np.float32)).to(device, dtype)
    with _repeatable() if device == 'cpu' else contextlib.nullcontext():
        sum(o.square().sum() for o in net(x)).backward()
    return net, {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
