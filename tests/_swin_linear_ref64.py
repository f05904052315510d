"""The four Linears of the reference's SwinBlock (mmdet3d/models/backbones/swin.py:516-592; the FFN is mmcv's) with the LayerNorm in
front of them, the GELU and the residual additions behind them, and the whole block, restated in float64 torch -- the yardstick
pw_swin_linear (csrc/pw_swin_linear.hip, behind ops.swin_linear and SwinBlock(linear_impl='hip')) answers to.

A plain composition: mean, biased variance, (x - mean) / sqrt(var + eps) * gamma + beta; x W^T + b; 0.5 y (1 + erf(y / sqrt 2));
residual + y.  Nothing is folded, scaled or split here and nothing is borrowed from the kernel or from preworld_amd/image_encoder.py;
the block's attention is tests/_swin_attn_ref64.swin_attn_ref64.

THE CASES are the smallest shapes at which the kernel can still go wrong (see CASES).  Beyond the issue's table they hold six
`big_*` cases: the kernel has a 64 x 64 tile and a 128 x 128 one, and takes the large one only where ceil(M / 128) x
ceil(N / 128) >= 128 -- none of the table's shapes gets there, so without them the throughput kernel would run only inside the
model tests.  They have a row tail, a column tail (N = 528) and a K that ends in half a k chunk (48, 80).  In float32 a K above
1024 is summed in blocks of 1024 with a 128 x 64 throughput tile: k_deep_res takes that path with the small tile, big_deep_res
(K = 1040: one full block and half a chunk) with the large one.  Inputs are seeded; in
the bf16 cases every tensor the kernel reads as bf16 holds bf16 values, so the yardstick, the torch path and the kernel read the same
numbers.

THE BOUND.  Per case 4 x FLOORS[case], relative to max |out64|: the floor is max |out_torch - out64| / max |out64| of the EXISTING
torch modules on the CPU -- F.layer_norm, F.linear, F.gelu and the addition in float32, and the same calls under
torch.autocast('cpu', torch.bfloat16) for the bf16 cases -- measured by tests/test_swin_linear_cpu.py, which asserts that the torch
path stays under each entry (rounded up to two digits) and reaches at least half of it: never taken from the kernel.  The factor
covers a different summation order, the matrix-core products and the device's erf.  No element is excluded.

Nothing above the harness line calls project code."""
import collections
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import _swin_attn_ref64 as A

Case = collections.namedtuple('Case', 'role M K N dtype seed bias x_scale w_scale special')
# role: 'ln' = Linear(LayerNorm(x)); 'ln_gelu' = GELU(Linear(LayerNorm(x))); 'res' = residual + Linear(x)


def _c(role, M, K, N, dtype='f32', seed=0, bias=True, x_scale=1.0, w_scale=1.0, special=None):
    return Case(role, M, K, N, dtype, seed, bias, x_scale, w_scale, special)


CASES = collections.OrderedDict([
    ('qkv_tile', _c('ln', 128, 128, 384, seed=1)),                                   # exact tiles
    ('m_tail', _c('ln_gelu', 165, 128, 512, seed=2)),                                # row tail
    # the toy model's stage 0 at 24 * 2 + 5 rows: K of one k-step (half a chunk), N below a tile
    ('toy_narrow_qkv', _c('ln', 53, 16, 48, seed=3)),
    ('toy_narrow_proj', _c('res', 53, 16, 16, seed=4)),
    ('toy_narrow_fc1', _c('ln_gelu', 53, 16, 64, seed=5)),
    ('toy_narrow_fc2', _c('res', 53, 64, 16, seed=6)),
    ('k_deep_res', _c('res', 70, 4096, 1024, seed=7)),                               # longest accumulation (fc2, stage 3)
    ('wide_n_gelu', _c('ln_gelu', 70, 1024, 4096, seed=8)),                          # most column tiles
    ('rows_span', _c('res', 96, 256, 256, seed=9, special='rows_span')),             # row i scaled by 2^((i % 25) - 12)
    ('outlier_channel_res', _c('res', 96, 512, 512, seed=10, special='outlier')),    # one input channel 2^10 x the rest
    ('outlier_channel_ln', _c('ln', 96, 512, 512, seed=11, special='outlier')),
    ('range_2m12', _c('res', 96, 256, 256, seed=12, x_scale=2.0 ** -12)),            # x, bias and residual x 2^-12 / x 2^8
    ('range_2p8', _c('res', 96, 256, 256, seed=12, x_scale=2.0 ** 8)),
    ('degenerate_rows_ln', _c('ln', 64, 128, 128, seed=13, special='const_row')),    # a constant row: variance 0
    ('degenerate_rows_res', _c('res', 64, 128, 128, seed=14, special='zero_row')),   # an all-zero row: exponent 0
    ('gelu_tails', _c('ln_gelu', 64, 128, 512, seed=15, w_scale=2.0)),               # pre-activations span about +-8
    ('no_ln_bias_zero', _c('res', 64, 128, 128, seed=16, bias=False)),               # bias=None
    ('bf16_qkv_tile', _c('ln', 128, 128, 384, 'bf16', seed=1)),
    ('bf16_m_tail', _c('ln_gelu', 165, 128, 512, 'bf16', seed=2)),
    ('bf16_k_deep_res', _c('res', 70, 4096, 1024, 'bf16', seed=7)),
    # the 128 x 128 tile (see the module docstring): row tail, column tail, K ending in half a chunk
    ('big_ln', _c('ln', 5541, 128, 384, seed=17)),
    ('big_ln_gelu', _c('ln_gelu', 4133, 80, 528, seed=18)),
    ('big_res', _c('res', 4133, 48, 528, seed=19)),
    ('big_deep_res', _c('res', 2069, 1040, 1024, seed=20)),                          # 128 x 64 tile, sums in blocks of K = 1024
    ('bf16_big_ln', _c('ln', 5541, 128, 384, 'bf16', seed=17)),
    ('bf16_big_res', _c('res', 4133, 48, 528, 'bf16', seed=19)),
])
DEGENERATE_ROW = 3
EPS = 1e-5

# max |out_torch - out64| / max |out64| of the torch modules on the CPU (see the module docstring), rounded up to two digits
FLOORS = {
    'qkv_tile': 4.9e-07,                     # measured 4.864e-07
    'm_tail': 4.3e-07,                       # measured 4.287e-07
    'toy_narrow_qkv': 1.9e-07,               # measured 1.889e-07
    'toy_narrow_proj': 1.4e-07,              # measured 1.380e-07
    'toy_narrow_fc1': 2.5e-07,               # measured 2.471e-07
    'toy_narrow_fc2': 2.4e-07,               # measured 2.328e-07
    'k_deep_res': 2.5e-07,                   # measured 2.492e-07
    'wide_n_gelu': 4.8e-07,                  # measured 4.763e-07
    'rows_span': 6.1e-07,                    # measured 6.092e-07
    'outlier_channel_res': 9.5e-07,          # measured 9.428e-07
    'outlier_channel_ln': 1.2e-06,           # measured 1.105e-06
    'range_2m12': 3.8e-07,                   # measured 3.718e-07
    'range_2p8': 3.8e-07,                    # measured 3.718e-07
    'degenerate_rows_ln': 4.3e-07,           # measured 4.221e-07
    'degenerate_rows_res': 3.5e-07,          # measured 3.484e-07
    'gelu_tails': 4.8e-07,                   # measured 4.736e-07
    'no_ln_bias_zero': 3.3e-07,              # measured 3.299e-07
    'bf16_qkv_tile': 3.7e-03,                # measured 3.651e-03
    'bf16_m_tail': 4.4e-03,                  # measured 4.346e-03
    'bf16_k_deep_res': 2.3e-03,              # measured 2.202e-03
    'big_ln': 5.5e-07,                       # measured 5.428e-07
    'big_ln_gelu': 3.9e-07,                  # measured 3.878e-07
    'big_res': 2.7e-07,                      # measured 2.638e-07
    'big_deep_res': 4.4e-07,                 # measured 4.328e-07
    'bf16_big_ln': 3.8e-03,                  # measured 3.704e-03
    'bf16_big_res': 3.1e-03,                 # measured 3.098e-03
}

# SwinBlock cases of the GPU test (B, H, W, C, heads, ffn, ws, shifted): padded maps, shifted and unshifted; the floor is the torch
# block in float32 on the CPU against block_ref64, rounded up to two digits
BlockCase = collections.namedtuple('BlockCase', 'B H W C heads ffn ws shift seed')
BLOCK_CASES = collections.OrderedDict([
    ('toy_s0', BlockCase(2, 5, 9, 32, 2, 128, 4, False, 31)),
    ('toy_s2', BlockCase(2, 5, 9, 32, 2, 128, 4, True, 32)),
    ('tile_s0', BlockCase(1, 13, 25, 128, 4, 512, 12, False, 33)),
    ('tile_s6', BlockCase(1, 13, 25, 128, 4, 512, 12, True, 34)),
])
BLOCK_FLOORS = {
    'toy_s0': 1.3e-07,                       # measured 1.234e-07
    'toy_s2': 1.1e-07,                       # measured 1.024e-07
    'tile_s0': 1.2e-07,                      # measured 1.189e-07
    'tile_s6': 1.1e-07,                      # measured 1.072e-07
}
# the same block under torch.autocast('cpu', torch.bfloat16) against block_ref64
BLOCK_FLOORS_BF16 = {
    'tile_s6': 1.1e-03,                      # measured 1.098e-03
}

# the real-width model of tests/_swin_attn_ref64.MODEL_CFG under torch.autocast('cpu', torch.bfloat16) against the float64 model, per
# output map, rounded up to two digits (its float32 floors are MODEL_FLOORS there)
MODEL_FLOORS_BF16 = (7.9e-03, 8.8e-03, 9.9e-03, 8.7e-03)      # measured 7.810e-03, 8.765e-03, 9.897e-03, 8.617e-03


def torch_dtype(case):
    return torch.bfloat16 if case.dtype == 'bf16' else torch.float32


def _randn(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(x (M, K), weight (N, K), bias (N) or None, gamma, beta (K) or None, residual (M, N) or None): float32 CPU tensors.  In a
    bf16 case x of the 'res' role holds bf16 values (the kernel reads it as bf16); everything else is float32 in both modes, as under
    autocast."""
    c = CASES[name]
    rs = np.random.RandomState(2000 + c.seed)
    x = _randn(rs, c.M, c.K)
    w = _randn(rs, c.N, c.K) * (c.w_scale / math.sqrt(c.K))
    b = 0.1 * _randn(rs, c.N) if c.bias else None
    g = beta = res = None
    if c.role != 'res':
        g, beta = 1.0 + 0.1 * _randn(rs, c.K), 0.1 * _randn(rs, c.K)
    else:
        res = _randn(rs, c.M, c.N)
    if c.special == 'rows_span':
        x = x * torch.pow(2.0, (torch.arange(c.M) % 25 - 12).float()).view(-1, 1)
    elif c.special == 'outlier':
        x[:, 7] *= 2.0 ** 10
    elif c.special == 'const_row':
        x[DEGENERATE_ROW] = 0.75
    elif c.special == 'zero_row':
        x[DEGENERATE_ROW] = 0.0
    if c.x_scale != 1.0:                                   # exact: powers of two
        x = x * c.x_scale
        b = None if b is None else b * c.x_scale
        res = None if res is None else res * c.x_scale
    if c.dtype == 'bf16' and c.role == 'res':
        x = x.bfloat16().float()
    return dict(x=x, weight=w, bias=b, gamma=g, beta=beta, residual=res)


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def layer_norm64(x, gamma, beta, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)         # biased
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def gelu64(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def linear_ref64(role, x, weight, bias, gamma=None, beta=None, residual=None, eps=EPS):
    """one role in float64"""
    d = lambda t: None if t is None else t.double()
    x, weight, bias, gamma, beta, residual = d(x), d(weight), d(bias), d(gamma), d(beta), d(residual)
    if role != 'res':
        x = layer_norm64(x, gamma, beta, eps)
    y = x @ weight.t()
    if bias is not None:
        y = y + bias
    if role == 'ln_gelu':
        y = gelu64(y)
    if role == 'res':
        y = residual + y
    return y


def block_ref64(x, hw, sd, heads, ws, shift, eps=EPS):
    """SwinBlock.forward (swin.py:581-592) in float64 from the block's state dict `sd`: x (B, H*W, C) -> (B, H*W, C)"""
    p = {k: v.double() for k, v in sd.items()}
    x = x.double()
    B, L, C = x.shape
    H, W = hw
    identity = x
    t = layer_norm64(x, p['norm1.weight'], p['norm1.bias'], eps)
    qkv = t @ p['attn.w_msa.qkv.weight'].t() + p['attn.w_msa.qkv.bias']
    a = A.swin_attn_ref64(qkv.view(B, H, W, 3 * C), p['attn.w_msa.qkv.bias'], p['attn.w_msa.relative_position_bias_table'], heads, ws,
                          shift, float(C // heads) ** -0.5)
    x = a.view(B, L, C) @ p['attn.w_msa.proj.weight'].t() + p['attn.w_msa.proj.bias']
    x = x + identity
    identity = x
    t = layer_norm64(x, p['norm2.weight'], p['norm2.bias'], eps)
    t = gelu64(t @ p['ffn.layers.0.0.weight'].t() + p['ffn.layers.0.0.bias'])
    t = t @ p['ffn.layers.1.weight'].t() + p['ffn.layers.1.bias']
    return identity + t


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 output of a case, computed once and shared (do not modify)"""
    return linear_ref64(CASES[name].role, **inputs(name))


def rel_err(out, ref):
    """max |out - ref| / max |ref| over every element"""
    return float((out.double() - ref).abs().max() / ref.abs().max())


def torch_path(name, dtype=None):
    """the existing torch modules' arithmetic on a case, on the CPU: float32, or under autocast for the bf16 cases (dtype=float64:
    the same calls in double, to check the restatement)"""
    c = CASES[name]
    i = inputs(name)
    if dtype is not None:
        i = {k: None if v is None else v.to(dtype) for k, v in i.items()}

    def run():
        x = i['x']
        if c.dtype == 'bf16' and c.role == 'res' and dtype is None:
            x = x.bfloat16()
        if c.role != 'res':
            x = F.layer_norm(x, (c.K,), i['gamma'], i['beta'], EPS)
        y = F.linear(x, i['weight'], i['bias'])
        if c.role == 'ln_gelu':
            y = F.gelu(y)
        if c.role == 'res':
            y = i['residual'] + y
        return y
    with torch.no_grad():
        if c.dtype == 'bf16' and dtype is None:
            with torch.autocast('cpu', torch.bfloat16):
                return run()
        return run()


def out_dtype(case):
    return torch.bfloat16 if case.dtype == 'bf16' and case.role != 'res' else torch.float32


# ------------------------------------------------------------------------------------ harness (project code from here on)
def build_block(name, attn_impl='torch', linear_impl='torch', dtype=torch.float32):
    """(SwinBlock of a BLOCK_CASES entry with seeded parameters, its input (B, H*W, C), hw_shape)"""
    from preworld_amd import image_encoder as IE
    c = BLOCK_CASES[name]
    torch.manual_seed(c.seed)
    blk = IE.SwinBlock(c.C, c.heads, c.ffn, c.ws, c.shift, attn_impl=attn_impl, linear_impl=linear_impl).eval()
    g = torch.Generator().manual_seed(c.seed + 100)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if n.endswith('relative_position_bias_table'):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif n.startswith('norm'):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith('bias'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    x = torch.randn(c.B, c.H * c.W, c.C, generator=g)
    return blk.to(dtype), x.to(dtype), (c.H, c.W)


def build_model(attn_impl='torch', linear_impl='torch', dtype=torch.float32):
    """the real-width model of tests/_swin_attn_ref64.MODEL_CFG (same seeds, same weights) with a linear_impl"""
    net, x = A.build_model(attn_impl, dtype)
    if linear_impl != 'torch':
        net.set_linear_impl(linear_impl)
    return net, x
