/*
 * preworld_hip_swin_linear_bwd.h -- the gradient of the Swin block Linears (preworld_hip_swin_linear.h) in the C ABI of
 * libpreworld_hip.so; included by preworld_hip.h, whose conventions hold: device pointers unless the name ends in _host, `stream`
 * last, 0 or a negative PW_E* code with a thread-local message.  Kept in a file of its own so that preworld_hip_swin_linear.h keeps
 * its four entry points (tests/test_swin_linear_cpu.py); preworld_amd/_lib.py parses it the same way and
 * tests/test_swin_linear_bwd_cpu.py holds it to the same rules.
 *
 * Float32 only (the split-fp16 mode PW_SWIN_F32 of the forward).  With y = pro(x) W^T + b, out = epi(y) and g the gradient of y:
 *   qkv   (mmdet3d/models/backbones/swin.py:583 norm1, :293 / :312 WindowMSA.qkv)   g = dout
 *   proj  (swin.py:295 / :341 WindowMSA.proj, :586 `x = x + identity`)              g = dout, d identity = dout
 *   fc1   (swin.py:589 norm2, :590 mmcv FFN: first Linear and GELU)                 g = dout o gelu'(y)
 *   fc2   (mmcv FFN.forward: second Linear and `identity + out`)                    g = dout, d identity = dout
 * and for every role  dx = g W  (through the LayerNorm's gradient where pro = LayerNorm),  dW = g^T pro(x),  db = column sums of g.
 * Every entry point is deterministic (no floating-point atomics: partial sums go to the workspace and a second launch adds them in a
 * fixed order, in double), does no host synchronisation (capturable) and refuses anything unsupported before any HIP call
 * (PW_EUNSUP for K, N; PW_EINVAL otherwise).  K and N as pw_swin_linear_packed_bytes: multiples of 16 in 16 .. 4096.  Workspaces
 * are 16-byte aligned; their contents before and after a call mean nothing.  Nothing is clamped: non-finite in, non-finite out.
 */
#ifndef PREWORLD_HIP_SWIN_LINEAR_BWD_H_
#define PREWORLD_HIP_SWIN_LINEAR_BWD_H_

#include <stddef.h>
#include <stdint.h>

#include "preworld_hip_swin_linear.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PW_SWIN_LINEAR_BWD_SPLIT_ROWS 1024     /* rows of M one workgroup of the weight gradient sums: split = ceil(M / 1024) */
#define PW_SWIN_LINEAR_BWD_COL_ROWS 512        /* rows of M one workgroup of a column-statistics launch covers */

/* Bytes of the TRANSPOSED packed operand of an (N, K) Linear (nn.Linear.weight, swin.py:293-295 and the FFN's two Linears): what
 * pw_swin_linear_packed_bytes gives for a (K, N) Linear in PW_SWIN_F32 mode; 0 if the shape is not supported. */
size_t pw_swin_linear_backward_packed_bytes(int K, int N);

/* weight (N, K) -> packed_t: W^T (K, N) in the layout pw_swin_linear reads, i.e. the columns of W (swin.py:293-295, FFN) as rows,
 * each split under the power of two of its own absmax; zero bias, no LayerNorm.  Two small launches. */
int pw_swin_linear_backward_pack(const float* weight, void* packed_t, int K, int N, void* stream);

/* Bytes of workspace of pw_swin_linear_backward_data and pw_swin_linear_backward_gelu: (M, 2) floats of row statistics
 * (the roles are listed at the top of this file). */
size_t pw_swin_linear_backward_rows_workspace_bytes(int64_t M);

/* dx (M, K) = g (M, N) W: the gradient of `x W^T` of all four Linears (swin.py:312, :341; the FFN's Linears) with respect to its
 * input -- for qkv and fc1 that input is the LayerNorm's output, see pw_swin_layernorm_backward.  It is the forward GEMM
 * (pw_swin_linear, identity prologue, no bias) with packed_t as its weight: g rows under their own power of two, the forward's tile
 * choice and, for N > 1024, its blocked accumulation.  Row m of dx depends on row m of g alone; an all-zero row gives exact zeros. */
int pw_swin_linear_backward_data(const float* g, const void* packed_t, float* dx, float* workspace, size_t workspace_bytes, int64_t M,
                                 int K, int N, void* stream);

/* dz (M, N) = dh o gelu'(LN(x) W^T + b), gelu'(y) = 0.5 (1 + erf(y / sqrt 2)) + y exp(-y^2 / 2) / sqrt(2 pi): the gradient of the
 * FFN's activation (swin.py:590; mmcv FFN, nn.GELU) with the pre-activation recomputed by the fc1 forward GEMM (LayerNorm prologue,
 * `packed` = the forward's pw_swin_linear_pack operand) and never stored.  dz may be dh itself. */
int pw_swin_linear_backward_gelu(const float* x, const void* packed, const float* dh, float* dz, float* workspace, size_t workspace_bytes,
                                 int64_t M, int K, int N, float eps, void* stream);

/* Bytes of workspace of pw_swin_linear_backward_weight; 0 if M, K or N is not supported.  From (M, K, N, ln) alone:
 * column-statistics partials of ceil(M / 512) row blocks, the scales, (M, 2) row statistics with ln, and ceil(M / 1024) partial
 * (N, K) products (roles: top of this file). */
size_t pw_swin_linear_backward_weight_workspace_bytes(int64_t M, int K, int N, int ln);

/* dweight (N, K) = g^T pro(x), dbias (N) = column sums of g, for g (M, N) and x (M, K): the parameter gradients of the four Linears
 * (swin.py:293-295, :312, :341; the FFN's Linears).  ln != 0: pro = LayerNorm (norm1 / norm2, swin.py:583 / :589) with gamma, beta and
 * the operand bound of `packed` (the forward's operand; NULL and unused with ln == 0), statistics recomputed; the normalised tensor
 * never exists in global memory.  dweight == NULL or dbias == NULL skips that gradient (not both).  Split-fp16 products: g under a
 * power of two per column, pro(x) under the pack-time LayerNorm bound or a power of two per column, all found on the device.  M is
 * split over workgroups of 1024 rows; partials are added in a fixed order in double. */
int pw_swin_linear_backward_weight(const float* g, const float* x, const void* packed, float* dweight, float* dbias, void* workspace,
                                   size_t workspace_bytes, int64_t M, int K, int N, int ln, float eps, void* stream);

/* Bytes of workspace of pw_swin_layernorm_backward: (M, 2) row statistics and the column partials of ceil(M / 512) row blocks
 * (norm1 / norm2, swin.py:583 / :589). */
size_t pw_swin_layernorm_backward_workspace_bytes(int64_t M, int K);

/* Gradient of xn = LayerNorm(x) over K (norm1 / norm2 of swin.py:583 / :589; biased variance, eps) for dxn (M, K):
 *   dx = dres + rstd (gamma dxn - mean_k(gamma dxn) - xhat mean_k(gamma dxn xhat)),  dgamma = column sums of dxn xhat,  dbeta = of dxn
 * dres (M, K) or NULL is the gradient the residual stream carries past the LayerNorm (`x + identity`, swin.py:586; FFN.forward's
 * identity), folded in so that no separate addition runs.  dx, or dgamma and dbeta together, may be NULL (not all); dx may be dxn. */
int pw_swin_layernorm_backward(const float* dxn, const float* x, const float* gamma, const float* dres, float* dx, float* dgamma,
                               float* dbeta, void* workspace, size_t workspace_bytes, int64_t M, int K, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PREWORLD_HIP_SWIN_LINEAR_BWD_H_ */
