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

THE UNIT.  The figure above divides by the tensor's largest element, so an error in a small row or column vanishes in it (dropping
x W^T from the 16 rows of rows_span whose scale is <= 2^-9 moves it to 5.0e-07 against a bound of 2.44e-06;
tests/test_swin_linear_cpu.py::test_the_unit_sees_what_the_tensor_maximum_hides).  Every case is therefore ALSO scored per element,
    q = |out - out64| / (U n),      U = 2^-24 (2^-9 for the bf16 cases),
where n is the float64 formula of the output with every product of leaves replaced by the product of their absolute values and every
addition or subtraction by an addition (as tests/_infer_ref64.py does on the voxel side):
    role res               n = |x| |W|^T + |b| + |residual|
    roles ln, ln_gelu      n_t = (|x| + |mean|) / sqrt(var + eps) * |gamma| + |beta|   (the cancellation in x - mean shows)
                           n_pre = n_t |W|^T + |b|
    after the GELU         n = |gelu'(y64)| n_pre + |gelu(y64)|,   y64 the float64 pre-activation
float32 cannot hold 1 + erf(y / sqrt 2) below 2^-25, so in the GELU's negative tail the torch path itself is thousands of these units
off (Q32 of gelu_tails is 2.2e5: the float32 result is an exact zero there) and 2 Q32 + 1 says little about the other elements of such
a case.  The 'ln_gelu' cases are therefore scored a second time against n_sum, the same n with the GELU's own sum taken as a sum,
    n_sum = |gelu'(y64)| n_pre + 0.5 |y64| (1 + |erf(y64 / sqrt 2)|),      max q <= 2 Q32_SUM[case] + 1,
which shows that cancellation as n_t shows the LayerNorm's; both bounds hold.
An element with n == 0 must be reproduced exactly.  The bound is max q <= 2 Q32[case] + 1 + FORMAT_TERM.get(case, 0): Q32 is the
worst q of the same torch path as above (float32, or autocast for bf16) on the CPU, rounded up to two digits, asserted by
tests/test_swin_linear_cpu.py like FLOORS; FORMAT_TERM holds a-priori terms only (profiles/image_gemm_units.md).  The cases
w_rows_span, w_rows_span_ln_gelu and x_and_w_span aim at the exponents the kernel takes per weight row and per token row: in
x_and_w_span the residual of element (i, n) carries both scales, so every element is judged at its own size.

Nothing above the harness line calls project code."""
import collections
import contextlib
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
    # the exponents (see THE UNIT): weight row n scaled by 2^((n % 25) - 12), alone and against spanned token rows
    ('w_rows_span', _c('res', 96, 256, 256, seed=21, special='w_rows_span')),
    ('w_rows_span_ln_gelu', _c('ln_gelu', 64, 128, 512, seed=22, special='w_rows_span')),
    ('x_and_w_span', _c('res', 96, 256, 256, seed=23, bias=False, special='x_and_w_span')),      # residual (i, n) scaled by both
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
    'w_rows_span': 3.6e-07,                  # measured 3.568e-07
    'w_rows_span_ln_gelu': 4.2e-07,          # measured 4.167e-07
    'x_and_w_span': 2.4e-07,                 # measured 2.364e-07
}

# worst q of the same torch path in the units of THE UNIT (2^-24 n; 2^-9 n for the bf16 cases), rounded up to two digits
U = 2.0 ** -24
Q32 = {
    'qkv_tile': 4.2,                         # measured 4.152, mean 0.295
    'm_tail': 2200.0,                        # measured 2128, mean 0.669
    'toy_narrow_qkv': 3.2,                   # measured 3.181, mean 0.349
    'toy_narrow_proj': 2.2,                  # measured 2.136, mean 0.311
    'toy_narrow_fc1': 610.0,                 # measured 605.3, mean 0.757
    'toy_narrow_fc2': 2.4,                   # measured 2.324, mean 0.277
    'k_deep_res': 0.8,                       # measured 0.7909, mean 0.113
    'wide_n_gelu': 740.0,                    # measured 730.3, mean 0.305
    'rows_span': 3.9,                        # measured 3.898, mean 0.309
    'outlier_channel_res': 27,               # measured 26.86, mean 2.596
    'outlier_channel_ln': 13,                # measured 12.43, mean 1.039
    'range_2m12': 3.5,                       # measured 3.486, mean 0.310
    'range_2p8': 3.5,                        # measured 3.486, mean 0.310
    'degenerate_rows_ln': 2.9,               # measured 2.843, mean 0.295
    'degenerate_rows_res': 3.7,              # measured 3.665, mean 0.312
    'gelu_tails': 220000.0,                  # measured 2.115e+05, mean 586.849
    'no_ln_bias_zero': 3.4,                  # measured 3.361, mean 0.305
    'bf16_qkv_tile': 0.9,                    # measured 0.8943, mean 0.135
    'bf16_m_tail': 0.98,                     # measured 0.9734, mean 0.152
    'bf16_k_deep_res': 0.17,                 # measured 0.1654, mean 0.023
    'big_ln': 5,                             # measured 4.963, mean 0.299
    'big_ln_gelu': 32000.0,                  # measured 3.19e+04, mean 0.723
    'big_res': 4.8,                          # measured 4.752, mean 0.300
    'big_deep_res': 2.3,                     # measured 2.295, mean 0.203
    'bf16_big_ln': 1.2,                      # measured 1.124, mean 0.134
    'bf16_big_res': 1.6,                     # measured 1.539, mean 0.177
    'w_rows_span': 3.9,                      # measured 3.876, mean 0.311
    'w_rows_span_ln_gelu': 170000.0,         # measured 1.66e+05, mean 451.924
    'x_and_w_span': 3.2,                     # measured 3.179, mean 0.313
}
# the 'ln_gelu' cases against n_sum (THE UNIT): worst q of the same torch path, rounded up to two digits
Q32_SUM = {
    'm_tail': 4.3,                           # measured 4.245, mean 0.245
    'toy_narrow_fc1': 2.6,                   # measured 2.55, mean 0.274
    'wide_n_gelu': 4.1,                      # measured 4.052, mean 0.182
    'gelu_tails': 4.6,                       # measured 4.518, mean 0.315
    'bf16_m_tail': 0.98,                     # measured 0.9734, mean 0.120
    'big_ln_gelu': 4.9,                      # measured 4.86, mean 0.243
    'w_rows_span_ln_gelu': 4.3,              # measured 4.235, mean 0.219
}
# a-priori terms of the format, in units of U n, for cases the kernel's path exceeds 2 Q32 + 1 on by construction; derivations in
# profiles/image_gemm_units.md.  Never fitted to a measured q
FORMAT_TERM = {}

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


def span(n):
    """the scale of row i of a *_span case: 2^((i % 25) - 12), exact in float32"""
    return torch.pow(2.0, (torch.arange(n) % 25 - 12).float())


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
        x = x * span(c.M).view(-1, 1)
    elif c.special == 'outlier':
        x[:, 7] *= 2.0 ** 10
    elif c.special == 'const_row':
        x[DEGENERATE_ROW] = 0.75
    elif c.special == 'zero_row':
        x[DEGENERATE_ROW] = 0.0
    elif c.special == 'w_rows_span':
        w = w * span(c.N).view(-1, 1)
    elif c.special == 'x_and_w_span':                      # every output element is a small row met by a small column, at its own size
        x, w = x * span(c.M).view(-1, 1), w * span(c.N).view(-1, 1)
        res = res * span(c.M).view(-1, 1) * span(c.N).view(1, -1)
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


# ------------------------------------------------------------------------------------------------------- the unit, per element
def gelu_grad64(y):
    """d/dy of gelu64: Phi(y) + y phi(y)"""
    return 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0))) + y * torch.exp(-0.5 * y * y) / math.sqrt(2.0 * math.pi)


def ln_normaliser64(x, gamma, beta, eps):
    """(n_xhat, n_t) of a LayerNorm in double: (|x| + |mean|) / sqrt(var + eps), and that times |gamma| plus |beta|"""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    n_xhat = (x.abs() + mean.abs()) / torch.sqrt(var + eps)
    return n_xhat, n_xhat * gamma.abs() + beta.abs()


def linear_normaliser64(role, x, weight, bias, gamma=None, beta=None, residual=None, eps=EPS, gelu_sum=False):
    """n of one role (THE UNIT): linear_ref64 with every product of leaves taken of absolute values and every sum as a sum; gelu_sum:
    the GELU's own sum 1 + erf likewise, as 1 + |erf| (n_sum of THE UNIT)"""
    d = lambda t: None if t is None else t.double()
    x, weight, bias, gamma, beta, residual = d(x), d(weight), d(bias), d(gamma), d(beta), d(residual)
    if role == 'res':
        n = x.abs() @ weight.abs().t()
    else:
        n = ln_normaliser64(x, gamma, beta, eps)[1] @ weight.abs().t()
    if bias is not None:
        n = n + bias.abs()
    if role == 'ln_gelu':
        y = layer_norm64(x, gamma, beta, eps) @ weight.t()
        y = y if bias is None else y + bias
        value = 0.5 * y.abs() * (1.0 + torch.erf(y / math.sqrt(2.0)).abs()) if gelu_sum else gelu64(y).abs()
        n = gelu_grad64(y).abs() * n + value
    if role == 'res':
        n = n + residual.abs()
    return n


@functools.lru_cache(maxsize=None)
def normaliser(name):
    """the float64 normaliser of a case, the shape of reference(name), computed once and shared (do not modify)"""
    return linear_normaliser64(CASES[name].role, **inputs(name))


@functools.lru_cache(maxsize=None)
def normaliser_sum(name):
    """n_sum of a 'ln_gelu' case (THE UNIT), computed once and shared (do not modify)"""
    assert CASES[name].role == 'ln_gelu', name
    return linear_normaliser64('ln_gelu', gelu_sum=True, **inputs(name))


def unit(name):
    return 2.0 ** -9 if CASES[name].dtype == 'bf16' else U


@contextlib.contextmanager
def one_thread():
    """a CPU measurement that gives the same figure on every machine: torch picks a GEMM's blocking, and so the order of its sums, by
    the thread count"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


def q_of(got, ref, n, u=U):
    """per-element q = |got - ref| / (u n) in double; where n == 0 the element must be reproduced exactly (q = inf otherwise); a NaN
    counts as inf"""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)
    return torch.where(n > 0, err / (u * n.clamp_min(1e-300)), torch.where(err > 0, torch.full_like(err, float('inf')), err))


def round11(t):
    """a float64 copy rounded to 11 significant bits: what an operand is without its lo plane"""
    m, e = torch.frexp(t.double())
    return torch.ldexp(torch.round(m * 2048.0) / 2048.0, e)


LOW_SCALE = 2.0 ** -9                  # the rows and columns of a *_span case with a scale up to this are its low-magnitude ones


def bound(name):
    return 2.0 * Q32[name] + 1.0 + FORMAT_TERM.get(name, 0.0)


def check_units(name, out, say):
    """a case's output in per-element units against bound(name); prints the figures before it asserts; returns (worst, mean) q"""
    q = q_of(out.cpu(), reference(name), normaliser(name), unit(name))
    worst, mean = float(q.max()), float(q.mean())
    print('%s: %s worst q %.3f, mean q %.3f, Q32 %.2f, bound %.2f (unit 2^%d n)' % (name, say, worst, mean, Q32[name], bound(name),
                                                                                 round(math.log2(unit(name)))))
    assert worst <= bound(name), (name, worst, bound(name))
    if CASES[name].role == 'ln_gelu':
        qs = q_of(out.cpu(), reference(name), normaliser_sum(name), unit(name))
        b = 2.0 * Q32_SUM[name] + 1.0
        print('%s: %s against n_sum worst q %.3f, mean q %.3f, Q32_SUM %.2f, bound %.2f' % (name, say, float(qs.max()), float(qs.mean()),
                                                                                          Q32_SUM[name], b))
        assert float(qs.max()) <= b, (name, float(qs.max()), b)
    return worst, mean


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
