"""The yardstick of the fused Swin Linears' BACKWARD (include/preworld_hip_swin_linear_bwd.h, ops.swin_linear_backward, ops.SwinLinear,
SwinBlock(linear_impl='hip_grad')): float64 autograd straight through _swin_linear_ref64.linear_ref64 / block_ref64 with x, weight,
bias, gamma, beta and residual as leaves.  Nothing here comes from the kernel or from preworld_amd/image_encoder.py.

THE COTANGENT of a case is a seeded standard normal of the output's shape (the cot_* cases reshape it, see below).

THE CASES are the float32 entries of _swin_linear_ref64.CASES -- already the smallest shapes that reach each tile, tail and
deep-accumulation path, its *_span cases included -- and six that only a backward can get wrong:
    long_m               role ln,       M = 20011, K = 16, N = 48   the split over M and the order of the partial sums
    cot_rows_span        role res,      96 x 256 x 256              cotangent row i scaled by 2^((i % 25) - 12): per-row exponents of
                                                                    the data gradient, per-column exponents of the weight gradient
    cot_outlier_column   role ln,       96 x 512 x 512              one output channel's cotangent 2^10 x the rest
    cot_zero_rows        role ln_gelu,  64 x 128 x 512              an all-zero cotangent row: exponent 0, an exact-zero dx row
    x_rows_span_wgrad    role res,      96 x 256 x 256              x row i scaled by 2^((i % 25) - 12), a plain cotangent: every column
                                                                    of x the weight gradient takes an exponent of spans 2^24
    x_cols_span_wgrad    role res,      96 x 256 x 256              x column k scaled by 2^((k % 25) - 12): small columns of dweight

THE BOUND.  Per case and per gradient (dx, dweight, dbias, dgamma, dbeta, dresidual):
    max |g - g64| / max |g64| <= 4 x BWD_FLOORS[case][grad]
The floor is the same figure for the float32 backward of the EXISTING torch modules (F.layer_norm, F.linear, F.gelu, the addition)
on the CPU, on one thread with deterministic algorithms (_swin_attn_bwd_ref64._repeatable); tests/test_swin_linear_bwd_cpu.py
measures it and asserts that the torch path stays under each entry (rounded up to two digits) and reaches at least half of it.  No
floor is taken from the kernel, no element is excluded, and dresidual must equal the cotangent exactly (its floor is None).

THE UNIT.  As in _swin_linear_ref64 (THE UNIT there) every gradient is ALSO scored per element, q = |g - g64| / (2^-24 n), with one
normaliser per gradient: the float64 formula of the gradient with products of absolute values and sums only.  With g the cotangent,
r = 1 / sqrt(var + eps), n_xhat = (|x| + |mean|) r, n_t = n_xhat |gamma| + |beta| and |g_pre| = |g| (role ln, res) or
|g| |gelu'(y64)| (role ln_gelu):
    dbias      sum_m |g_pre|                              dweight    |g_pre|^T n_t        (role res: |g|^T |x|)
    dx (res)   |g| |W|                                    dresidual  exactly the cotangent, not scored
    dt = g_pre W, the gradient of the LayerNorm's output:            n_dt = |g_pre| |W|
    dbeta  = sum_m dt                                                n = sum_m n_dt
    dgamma = sum_m dt xhat                                           n = sum_m n_dt n_xhat
    dxhat  = dt gamma                                                n_dxhat = n_dt |gamma|
    dx     = r (dxhat - mean_k dxhat - xhat mean_k(dxhat xhat))      n = r (n_dxhat + mean_k n_dxhat + n_xhat mean_k(n_dxhat n_xhat))
The bound is max q <= 2 Q32[case][grad] + 1 + FORMAT_TERM: Q32 is the worst q of the same float32 torch backward, asserted like
BWD_FLOORS.  An element with n == 0 (the dx row of an all-zero cotangent row) must be exactly zero."""
import collections
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import _swin_attn_bwd_ref64 as AB
import _swin_linear_ref64 as R

_repeatable = AB._repeatable
rel_err = AB.rel_err

NEW_CASES = collections.OrderedDict([
    ('long_m', R._c('ln', 20011, 16, 48, seed=41)),
    ('cot_rows_span', R._c('res', 96, 256, 256, seed=42, special='cot_rows_span')),
    ('cot_outlier_column', R._c('ln', 96, 512, 512, seed=43, special='cot_outlier_column')),
    ('cot_zero_rows', R._c('ln_gelu', 64, 128, 512, seed=44, special='cot_zero_rows')),
    ('x_rows_span_wgrad', R._c('res', 96, 256, 256, seed=45, special='x_rows_span')),
    ('x_cols_span_wgrad', R._c('res', 96, 256, 256, seed=46, special='x_cols_span')),
])
CASES = collections.OrderedDict([(k, c) for k, c in R.CASES.items() if c.dtype == 'f32'])
CASES.update(NEW_CASES)
GRADS = ('dx', 'dweight', 'dbias', 'dgamma', 'dbeta', 'dresidual')
LEAVES = dict(dx='x', dweight='weight', dbias='bias', dgamma='gamma', dbeta='beta', dresidual='residual')
OUTLIER_COLUMN, ZERO_ROW = 7, 3

# max |g_torch - g64| / max |g64| of the torch modules' float32 backward on the CPU (see the module docstring), rounded up to two
# digits, in the order dx, dweight, dbias, dgamma, dbeta; a gradient whose leaf the case does not have is absent
BWD_FLOORS = {
    'qkv_tile':                  dict(dx=6.3e-07, dweight=4.8e-07, dbias=8.0e-08, dgamma=3.4e-07, dbeta=4.2e-07),      # measured 6.231e-07, 4.737e-07, 7.974e-08, 3.347e-07, 4.110e-07
    'm_tail':                    dict(dx=5.9e-07, dweight=4.5e-07, dbias=1.8e-07, dgamma=3.8e-07, dbeta=3.9e-07),      # measured 5.844e-07, 4.493e-07, 1.759e-07, 3.727e-07, 3.886e-07
    'toy_narrow_qkv':            dict(dx=2.3e-07, dweight=2.8e-07, dbias=1.2e-07, dgamma=1.1e-07, dbeta=2.0e-07),      # measured 2.207e-07, 2.760e-07, 1.124e-07, 1.074e-07, 1.963e-07
    'toy_narrow_proj':           dict(dx=1.5e-07, dweight=1.7e-07, dbias=9.4e-08),      # measured 1.425e-07, 1.665e-07, 9.325e-08
    'toy_narrow_fc1':            dict(dx=4.1e-07, dweight=2.4e-07, dbias=1.3e-07, dgamma=1.9e-07, dbeta=2.0e-07),      # measured 4.031e-07, 2.371e-07, 1.232e-07, 1.808e-07, 1.916e-07
    'toy_narrow_fc2':            dict(dx=1.1e-07, dweight=2.0e-07, dbias=6.0e-08),      # measured 1.045e-07, 1.934e-07, 5.919e-08
    'k_deep_res':                dict(dx=5.3e-07, dweight=3.3e-07, dbias=1.2e-07),      # measured 5.265e-07, 3.291e-07, 1.123e-07
    'wide_n_gelu':               dict(dx=5.3e-07, dweight=4.0e-07, dbias=2.5e-07, dgamma=4.6e-07, dbeta=5.1e-07),      # measured 5.233e-07, 3.972e-07, 2.491e-07, 4.516e-07, 5.050e-07
    'rows_span':                 dict(dx=4.5e-07, dweight=3.5e-07, dbias=1.2e-07),      # measured 4.434e-07, 3.454e-07, 1.121e-07
    'outlier_channel_res':       dict(dx=6.1e-07, dweight=4.2e-07, dbias=9.9e-08),      # measured 6.024e-07, 4.104e-07, 9.870e-08
    'outlier_channel_ln':        dict(dx=4.0e-07, dweight=3.6e-07, dbias=9.4e-08, dgamma=1.4e-07, dbeta=3.4e-07),      # measured 3.972e-07, 3.522e-07, 9.338e-08, 1.341e-07, 3.328e-07
    'range_2m12':                dict(dx=5.1e-07, dweight=4.1e-07, dbias=8.0e-08),      # measured 5.042e-07, 4.080e-07, 7.932e-08
    'range_2p8':                 dict(dx=5.1e-07, dweight=4.1e-07, dbias=8.0e-08),      # measured 5.042e-07, 4.080e-07, 7.932e-08
    'degenerate_rows_ln':        dict(dx=3.3e-07, dweight=3.2e-07, dbias=7.9e-08, dgamma=3.1e-07, dbeta=2.4e-07),      # measured 3.267e-07, 3.180e-07, 7.871e-08, 3.072e-07, 2.384e-07
    'degenerate_rows_res':       dict(dx=4.4e-07, dweight=2.7e-07, dbias=7.6e-08),      # measured 4.319e-07, 2.623e-07, 7.590e-08
    'gelu_tails':                dict(dx=5.1e-07, dweight=4.7e-07, dbias=2.0e-07, dgamma=3.7e-07, dbeta=4.5e-07),      # measured 5.002e-07, 4.645e-07, 1.916e-07, 3.612e-07, 4.437e-07
    'no_ln_bias_zero':           dict(dx=4.3e-07, dweight=3.1e-07),      # measured 4.222e-07, 3.072e-07
    'big_ln':                    dict(dx=7.7e-07, dweight=4.3e-07, dbias=1.6e-07, dgamma=2.8e-06, dbeta=1.7e-06),      # measured 7.641e-07, 4.202e-07, 1.578e-07, 2.768e-06, 1.669e-06
    'big_ln_gelu':               dict(dx=5.4e-07, dweight=4.3e-07, dbias=2.4e-07, dgamma=1.8e-06, dbeta=1.8e-06),      # measured 5.314e-07, 4.297e-07, 2.325e-07, 1.757e-06, 1.740e-06
    'big_res':                   dict(dx=4.7e-07, dweight=4.4e-07, dbias=1.7e-07),      # measured 4.630e-07, 4.341e-07, 1.617e-07
    'big_deep_res':              dict(dx=5.6e-07, dweight=5.0e-07, dbias=1.6e-07),      # measured 5.564e-07, 4.990e-07, 1.572e-07
    'long_m':                    dict(dx=1.9e-07, dweight=4.2e-07, dbias=1.2e-07, dgamma=5.0e-06, dbeta=2.1e-06),      # measured 1.812e-07, 4.116e-07, 1.149e-07, 4.981e-06, 2.059e-06
    'cot_rows_span':             dict(dx=4.6e-07, dweight=4.9e-07, dbias=1.4e-07),      # measured 4.523e-07, 4.815e-07, 1.320e-07
    'cot_outlier_column':        dict(dx=1.3e-06, dweight=2.0e-07, dbias=3.3e-07, dgamma=2.6e-07, dbeta=1.9e-06),      # measured 1.277e-06, 1.939e-07, 3.296e-07, 2.504e-07, 1.823e-06
    'cot_zero_rows':             dict(dx=4.3e-07, dweight=3.4e-07, dbias=1.7e-07, dgamma=3.7e-07, dbeta=2.2e-07),      # measured 4.298e-07, 3.369e-07, 1.681e-07, 3.608e-07, 2.109e-07
    'w_rows_span':               dict(dx=5.0e-07, dweight=3.4e-07, dbias=1.2e-07),      # measured 4.986e-07, 3.305e-07, 1.120e-07
    'w_rows_span_ln_gelu':       dict(dx=5.2e-05, dweight=3.0e-05, dbias=2.1e-05, dgamma=2.4e-05, dbeta=1.2e-05),      # measured 5.189e-05, 2.994e-05, 2.037e-05, 2.310e-05, 1.184e-05
    'x_and_w_span':              dict(dx=4.4e-07, dweight=2.9e-07),      # measured 4.305e-07, 2.813e-07
    'x_rows_span_wgrad':         dict(dx=5.3e-07, dweight=3.5e-07, dbias=1.5e-07),      # measured 5.248e-07, 3.433e-07, 1.408e-07
    'x_cols_span_wgrad':         dict(dx=4.5e-07, dweight=2.9e-07, dbias=1.1e-07),      # measured 4.479e-07, 2.885e-07, 1.068e-07
}

# worst q of the same float32 backward in the units of THE UNIT (2^-24 n), rounded up to two digits, same order
Q32 = {
    'qkv_tile':                  dict(dx=1.7, dweight=4.1, dbias=0.48, dgamma=0.12, dbeta=0.17),      # measured 1.658, 4.012, 0.474, 0.1119, 0.1628
    'm_tail':                    dict(dx=1.6, dweight=4.6, dbias=1.1, dgamma=0.15, dbeta=0.12),      # measured 1.515, 4.538, 1.069, 0.1406, 0.1143
    'toy_narrow_qkv':            dict(dx=1.2, dweight=2.3, dbias=1.1, dgamma=0.16, dbeta=0.18),      # measured 1.164, 2.221, 1.031, 0.1552, 0.1739
    'toy_narrow_proj':           dict(dx=4, dweight=1.9, dbias=0.65),      # measured 3.927, 1.849, 0.65
    'toy_narrow_fc1':            dict(dx=1.4, dweight=2.3, dbias=1.2, dgamma=0.27, dbeta=0.28),      # measured 1.34, 2.3, 1.165, 0.2655, 0.2709
    'toy_narrow_fc2':            dict(dx=2.3, dweight=3, dbias=0.55),      # measured 2.282, 2.914, 0.5489
    'k_deep_res':                dict(dx=2.1, dweight=6.5, dbias=1.1),      # measured 2.002, 6.466, 1.087
    'wide_n_gelu':               dict(dx=0.53, dweight=12, dbias=3.6, dgamma=0.12, dbeta=0.098),      # measured 0.524, 11.97, 3.521, 0.1133, 0.09751
    'rows_span':                 dict(dx=3.7, dweight=9.1, dbias=0.67),      # measured 3.669, 9.015, 0.6609
    'outlier_channel_res':       dict(dx=2.8, dweight=5, dbias=0.72),      # measured 2.715, 4.988, 0.7153
    'outlier_channel_ln':        dict(dx=1.3, dweight=5.6, dbias=0.63, dgamma=0.25, dbeta=0.14),      # measured 1.251, 5.536, 0.6283, 0.245, 0.1343
    'range_2m12':                dict(dx=3.7, dweight=3.9, dbias=0.65),      # measured 3.608, 3.855, 0.6453
    'range_2p8':                 dict(dx=3.7, dweight=3.9, dbias=0.65),      # measured 3.608, 3.855, 0.6453
    'degenerate_rows_ln':        dict(dx=1.7, dweight=1.7, dbias=0.7, dgamma=0.034, dbeta=0.21),      # measured 1.683, 1.607, 0.6903, 0.03306, 0.2043
    'degenerate_rows_res':       dict(dx=4, dweight=3.6, dbias=0.67),      # measured 3.919, 3.507, 0.6671
    'gelu_tails':                dict(dx=1.3, dweight=5.8, dbias=2.6, dgamma=0.22, dbeta=0.21),      # measured 1.295, 5.752, 2.542, 0.215, 0.2016
    'no_ln_bias_zero':           dict(dx=3.4, dweight=3.4),      # measured 3.361, 3.374
    'big_ln':                    dict(dx=2.2, dweight=0.51, dbias=0.15, dgamma=0.16, dbeta=0.087),      # measured 2.102, 0.503, 0.1451, 0.1559, 0.08643
    'big_ln_gelu':               dict(dx=1.7, dweight=0.74, dbias=0.27, dgamma=0.089, dbeta=0.12),      # measured 1.639, 0.7382, 0.2612, 0.08821, 0.1185
    'big_res':                   dict(dx=2.7, dweight=0.75, dbias=0.17),      # measured 2.68, 0.7492, 0.1697
    'big_deep_res':              dict(dx=2.4, dweight=1.5, dbias=0.25),      # measured 2.389, 1.446, 0.2496
    'w_rows_span':               dict(dx=9.4, dweight=3.8, dbias=0.66),      # measured 9.359, 3.723, 0.6561
    'w_rows_span_ln_gelu':       dict(dx=450.0, dweight=670.0, dbias=210.0, dgamma=44, dbeta=18),      # measured 447, 664.3, 207.8, 43.62, 17.66
    'x_and_w_span':              dict(dx=9.5, dweight=11),      # measured 9.475, 10.97
    'long_m':                    dict(dx=2.1, dweight=0.22, dbias=0.045, dgamma=0.36, dbeta=0.16),      # measured 2.06, 0.2118, 0.0444, 0.3569, 0.1566
    'cot_rows_span':             dict(dx=4.7, dweight=11, dbias=2.1),      # measured 4.629, 10.42, 2.094
    'cot_outlier_column':        dict(dx=17, dweight=4, dbias=0.73, dgamma=2.6, dbeta=2),      # measured 16.27, 3.922, 0.722, 2.58, 1.94
    'cot_zero_rows':             dict(dx=1, dweight=4.7, dbias=2.1, dgamma=0.23, dbeta=0.18),      # measured 0.9965, 4.658, 2.041, 0.2218, 0.1785
    'x_rows_span_wgrad':         dict(dx=3.7, dweight=11, dbias=0.78),      # measured 3.622, 10.07, 0.7789
    'x_cols_span_wgrad':         dict(dx=3.5, dweight=3.7, dbias=0.69),      # measured 3.44, 3.665, 0.6887
}
# a-priori terms of the format per case and gradient, in units of 2^-24 n (profiles/image_gemm_units.md); never fitted to a measured q
FORMAT_TERM = {}

# SwinBlock (the BLOCK_CASES of _swin_linear_ref64): the torch block's float32 backward on the CPU against float64 autograd of
# block_ref64, per case and per gradient (x and every parameter), rounded up to two digits
BLOCK_BWD_FLOORS = {
    'toy_s0': {
        'attn.w_msa.proj.bias':                              1.1e-07,      # measured 1.081e-07
        'attn.w_msa.proj.weight':                            2.5e-07,      # measured 2.476e-07
        'attn.w_msa.qkv.bias':                               2.8e-07,      # measured 2.722e-07
        'attn.w_msa.qkv.weight':                             4.1e-07,      # measured 4.063e-07
        'attn.w_msa.relative_position_bias_table':           1.4e-07,      # measured 1.392e-07
        'ffn.layers.0.0.bias':                               1.5e-07,      # measured 1.437e-07
        'ffn.layers.0.0.weight':                             3.1e-07,      # measured 3.052e-07
        'ffn.layers.1.bias':                                 1.4e-07,      # measured 1.310e-07
        'ffn.layers.1.weight':                               3.8e-07,      # measured 3.763e-07
        'norm1.bias':                                        1.9e-07,      # measured 1.891e-07
        'norm1.weight':                                      2.7e-07,      # measured 2.694e-07
        'norm2.bias':                                        2.8e-07,      # measured 2.719e-07
        'norm2.weight':                                      2.2e-07,      # measured 2.143e-07
        'x':                                                 1.5e-07,      # measured 1.477e-07
    },
    'toy_s2': {
        'attn.w_msa.proj.bias':                              2.2e-07,      # measured 2.176e-07
        'attn.w_msa.proj.weight':                            2.8e-07,      # measured 2.785e-07
        'attn.w_msa.qkv.bias':                               2.0e-07,      # measured 1.970e-07
        'attn.w_msa.qkv.weight':                             2.6e-07,      # measured 2.510e-07
        'attn.w_msa.relative_position_bias_table':           2.4e-07,      # measured 2.375e-07
        'ffn.layers.0.0.bias':                               2.3e-07,      # measured 2.260e-07
        'ffn.layers.0.0.weight':                             3.1e-07,      # measured 3.077e-07
        'ffn.layers.1.bias':                                 7.3e-08,      # measured 7.293e-08
        'ffn.layers.1.weight':                               3.4e-07,      # measured 3.321e-07
        'norm1.bias':                                        3.4e-07,      # measured 3.369e-07
        'norm1.weight':                                      3.5e-07,      # measured 3.422e-07
        'norm2.bias':                                        5.4e-07,      # measured 5.370e-07
        'norm2.weight':                                      4.4e-07,      # measured 4.338e-07
        'x':                                                 8.7e-08,      # measured 8.693e-08
    },
    'tile_s0': {
        'attn.w_msa.proj.bias':                              1.6e-07,      # measured 1.549e-07
        'attn.w_msa.proj.weight':                            1.2e-06,      # measured 1.147e-06
        'attn.w_msa.qkv.bias':                               1.8e-07,      # measured 1.789e-07
        'attn.w_msa.qkv.weight':                             5.4e-07,      # measured 5.329e-07
        'attn.w_msa.relative_position_bias_table':           5.2e-07,      # measured 5.141e-07
        'ffn.layers.0.0.bias':                               3.1e-07,      # measured 3.094e-07
        'ffn.layers.0.0.weight':                             7.0e-07,      # measured 6.992e-07
        'ffn.layers.1.bias':                                 1.6e-07,      # measured 1.560e-07
        'ffn.layers.1.weight':                               9.9e-07,      # measured 9.829e-07
        'norm1.bias':                                        5.4e-07,      # measured 5.328e-07
        'norm1.weight':                                      5.4e-07,      # measured 5.306e-07
        'norm2.bias':                                        1.1e-06,      # measured 1.009e-06
        'norm2.weight':                                      1.1e-06,      # measured 1.068e-06
        'x':                                                 1.6e-07,      # measured 1.530e-07
    },
    'tile_s6': {
        'attn.w_msa.proj.bias':                              1.2e-07,      # measured 1.170e-07
        'attn.w_msa.proj.weight':                            2.9e-07,      # measured 2.890e-07
        'attn.w_msa.qkv.bias':                               2.5e-07,      # measured 2.433e-07
        'attn.w_msa.qkv.weight':                             3.6e-07,      # measured 3.569e-07
        'attn.w_msa.relative_position_bias_table':           3.9e-07,      # measured 3.862e-07
        'ffn.layers.0.0.bias':                               2.6e-07,      # measured 2.513e-07
        'ffn.layers.0.0.weight':                             8.3e-07,      # measured 8.260e-07
        'ffn.layers.1.bias':                                 1.2e-07,      # measured 1.166e-07
        'ffn.layers.1.weight':                               6.9e-07,      # measured 6.827e-07
        'norm1.bias':                                        5.0e-07,      # measured 4.999e-07
        'norm1.weight':                                      4.9e-07,      # measured 4.845e-07
        'norm2.bias':                                        5.4e-07,      # measured 5.343e-07
        'norm2.weight':                                      6.2e-07,      # measured 6.132e-07
        'x':                                                 1.3e-07,      # measured 1.265e-07
    },
}

# the toy Swin (synth.small_swin_cfg, seeded weights, loss = sum of squares of the outputs): _swin_attn_bwd_ref64.TOY_FLOOR, the largest
# float32-against-float64 error over its parameters on the CPU, measured by tests/test_swin_attn_bwd_cpu.py
TOY_FLOOR = AB.TOY_FLOOR


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(x, weight, bias, gamma, beta, residual) of a case: float32 CPU tensors, None where the case has none (do not modify)"""
    if name in R.CASES:
        return R.inputs(name)
    c = CASES[name]
    rs = np.random.RandomState(2000 + c.seed)
    x = R._randn(rs, c.M, c.K)
    w = R._randn(rs, c.N, c.K) / math.sqrt(c.K)
    b = 0.1 * R._randn(rs, c.N)
    g = beta = res = None
    if c.role != 'res':
        g, beta = 1.0 + 0.1 * R._randn(rs, c.K), 0.1 * R._randn(rs, c.K)
    else:
        res = R._randn(rs, c.M, c.N)
    if c.special == 'x_rows_span':
        x = x * R.span(c.M).view(-1, 1)
    elif c.special == 'x_cols_span':
        x = x * R.span(c.K).view(1, -1)
    return dict(x=x, weight=w, bias=b, gamma=g, beta=beta, residual=res)


@functools.lru_cache(maxsize=None)
def cotangent(name):
    """float32 CPU tensor (M, N) (do not modify)"""
    c = CASES[name]
    rs = np.random.RandomState(7000 + c.seed)
    g = R._randn(rs, c.M, c.N)
    if c.special == 'cot_rows_span':
        g = g * R.span(c.M).view(-1, 1)
    elif c.special == 'cot_outlier_column':
        g[:, OUTLIER_COLUMN] *= 2.0 ** 10
    elif c.special == 'cot_zero_rows':
        g[ZERO_ROW] = 0.0
    return g


def _leaves(name, dtype):
    return {k: None if v is None else v.detach().to(dtype).clone().requires_grad_(True) for k, v in inputs(name).items()}


def _collect(leaves):
    return {g: None if leaves[l] is None else leaves[l].grad for g, l in LEAVES.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """{gradient name: float64 tensor, or None where the case has no such leaf}, computed once and shared (do not modify)"""
    lv = _leaves(name, torch.float64)
    out = R.linear_ref64(CASES[name].role, **lv)
    (out * cotangent(name).double()).sum().backward()
    return _collect(lv)


def torch_path_grads(name, dtype=torch.float32):
    """the same gradients from the backward of the existing torch modules on the CPU, one thread, deterministic"""
    c = CASES[name]
    lv = _leaves(name, dtype)
    with _repeatable():
        x = lv['x']
        if c.role != 'res':
            x = F.layer_norm(x, (c.K,), lv['gamma'], lv['beta'], R.EPS)
        y = F.linear(x, lv['weight'], lv['bias'])
        if c.role == 'ln_gelu':
            y = F.gelu(y)
        if c.role == 'res':
            y = lv['residual'] + y
        (y * cotangent(name).to(dtype)).sum().backward()
    return _collect(lv)


def errors(name, got):
    """{gradient name: max |g - g64| / max |g64|} over the gradients the case has"""
    ref = reference(name)
    out = {}
    for k in GRADS:
        if ref[k] is None:
            assert got.get(k) is None, (name, k)
            continue
        assert got[k] is not None and tuple(got[k].shape) == tuple(ref[k].shape), (name, k)
        out[k] = rel_err(got[k].cpu(), ref[k])
    return out


def check(name, got, say=None):
    """got: {gradient name: tensor or None} of a case against the yardstick under 4 x the floors; prints each figure before it asserts"""
    errs = errors(name, got)
    for k, err in errs.items():
        if k == 'dresidual':
            if say:
                print('%s %s: %s %.3e, bound: exactly the cotangent' % (name, k, say, err))
            assert torch.equal(got[k].cpu(), cotangent(name)), (name, k)
            continue
        floor = BWD_FLOORS[name][k]
        if say:
            print('%s %s: %s %.3e, bound %.3e (4 x floor %.1e)' % (name, k, say, err, 4 * floor, floor))
        assert err <= 4 * floor, (name, k, err)
    return errs


# ------------------------------------------------------------------------------------------ the unit, per element
@functools.lru_cache(maxsize=None)
def normaliser(name):
    """{gradient name: float64 normaliser of reference(name)[gradient], or None}: every form is written out in the module docstring
    (THE UNIT); computed once and shared (do not modify)"""
    c = CASES[name]
    i = {k: None if v is None else v.double() for k, v in inputs(name).items()}
    x, W, g = i['x'], i['weight'], cotangent(name).double().abs()
    n = dict.fromkeys(GRADS)
    if c.role == 'res':
        n['dx'], n['dweight'] = g @ W.abs(), g.t() @ x.abs()
        n['dbias'] = None if i['bias'] is None else g.sum(0)
        return n
    gamma, beta = i['gamma'], i['beta']
    n_xhat, n_t = R.ln_normaliser64(x, gamma, beta, R.EPS)
    r = 1.0 / torch.sqrt(((x - x.mean(-1, keepdim=True)) ** 2).mean(-1, keepdim=True) + R.EPS)
    if c.role == 'ln_gelu':
        y = R.layer_norm64(x, gamma, beta, R.EPS) @ W.t()
        g = g * R.gelu_grad64(y if i['bias'] is None else y + i['bias']).abs()      # |g_pre|
    n['dweight'] = g.t() @ n_t
    n['dbias'] = None if i['bias'] is None else g.sum(0)
    n_dt = g @ W.abs()
    n['dbeta'], n['dgamma'] = n_dt.sum(0), (n_dt * n_xhat).sum(0)
    n_dxhat = n_dt * gamma.abs()
    n['dx'] = r * (n_dxhat + n_dxhat.mean(-1, keepdim=True) + n_xhat * (n_dxhat * n_xhat).mean(-1, keepdim=True))
    return n


def q_errors(name, got):
    """{gradient name: per-element q tensor} over the gradients the case has (dresidual: exactly the cotangent, not scored)"""
    ref, n = reference(name), normaliser(name)
    out = {}
    for k in GRADS:
        if ref[k] is None:
            assert got.get(k) is None, (name, k)
            continue
        assert got[k] is not None and tuple(got[k].shape) == tuple(ref[k].shape), (name, k)
        if k != 'dresidual':
            out[k] = R.q_of(got[k].cpu(), ref[k], n[k])
    return out


def bound(name, k):
    return 2.0 * Q32[name][k] + 1.0 + FORMAT_TERM.get(name, {}).get(k, 0.0)


def check_units(name, got, say):
    """got: {gradient name: tensor or None} of a case in per-element units under bound(name, gradient); prints every figure, then
    asserts; returns {gradient: (worst, mean) q}"""
    figures = {k: (float(q.max()), float(q.mean())) for k, q in q_errors(name, got).items()}
    for k, (worst, mean) in figures.items():
        print('%s %s: %s worst q %.3f, mean q %.3f, Q32 %.2f, bound %.2f' % (name, k, say, worst, mean, Q32[name][k], bound(name, k)))
    if reference(name)['dresidual'] is not None:
        print('%s dresidual: bound: exactly the cotangent' % name)
        assert torch.equal(got['dresidual'].cpu(), cotangent(name)), (name, 'dresidual')
    for k, (worst, mean) in figures.items():
        assert worst <= bound(name, k), (name, k, worst, bound(name, k))
    return figures


# ------------------------------------------------------------------------------------------ the block
def block_cotangent(name):
    c = R.BLOCK_CASES[name]
    g = torch.Generator().manual_seed(c.seed + 200)
    return torch.randn(c.B, c.H * c.W, c.C, generator=g)


@functools.lru_cache(maxsize=None)
def block_reference(name):
    """float64 autograd of block_ref64 with x and the block's parameters as leaves: {'x' or parameter name: gradient}"""
    c = R.BLOCK_CASES[name]
    blk, x, hw = R.build_block(name)
    sd = {k: v.detach().double().clone() for k, v in blk.state_dict().items()}
    names = [n for n, _ in blk.named_parameters()]
    for n in names:
        sd[n].requires_grad_(True)
    x = x.double().requires_grad_(True)
    y = R.block_ref64(x, hw, sd, c.heads, c.ws, c.ws // 2 if c.shift else 0)
    (y * block_cotangent(name).double()).sum().backward()
    grads = {n: sd[n].grad for n in names}
    grads['x'] = x.grad
    return grads


def block_grads(name, attn_impl='torch', linear_impl='torch', device='cpu', dtype=torch.float32):
    """(block, output, {'x' or parameter name: gradient}) of SwinBlock on a BLOCK_CASES entry"""
    import contextlib
    blk, x, hw = R.build_block(name, attn_impl, linear_impl, dtype)
    blk = blk.to(device)
    x = x.to(device).requires_grad_(True)
    with _repeatable() if device == 'cpu' else contextlib.nullcontext():
        y = blk(x, hw)
        (y * block_cotangent(name).to(device, dtype)).sum().backward()
    grads = {n: p.grad for n, p in blk.named_parameters()}
    grads['x'] = x.grad
    return blk, y.detach(), grads


def block_errors(name, grads):
    ref = block_reference(name)
    assert set(grads) == set(ref), name
    return {k: rel_err(grads[k].cpu(), ref[k]) for k in ref}


# ------------------------------------------------------------------------------------------ the toy Swin
def toy_grads(attn_impl, linear_impl, device):
    """{parameter name: gradient} of the toy Swin of _swin_attn_bwd_ref64.toy_grads (same seeds, weights and loss) with a linear_impl"""
    from preworld_amd import image_encoder as IE, synth as S
    net = IE.SwinTransformer(**S.small_swin_cfg(), attn_impl=attn_impl, linear_impl=linear_impl).eval()
    net.load_state_dict(S.seeded_module_state(net, 51), strict=False)
    net = net.to(device)
    x = torch.from_numpy(np.random.RandomState(52).standard_normal((2, 3, 64, 96)).astype(np.float32)).to(device)
    sum(o.square().sum() for o in net(x)).backward()
    return net, {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
