/*
 * preworld_hip_swin_linear.h -- the Linears of a Swin block with LayerNorm, GELU and residual fused in, in the C ABI of
 * libpreworld_hip.so; included by preworld_hip.h, whose conventions hold: device pointers unless the name ends in _host, `stream`
 * last, 0 or a negative PW_E* code with a thread-local message.  Kept in a file of its own, like preworld_hip_swin.h, so that the
 * entry-point and pointer-parameter census of preworld_hip.h (tests/test_marshal_cpu.py) stays what it was; preworld_amd/_lib.py
 * parses it the same way and tests/test_swin_linear_cpu.py holds it to the same rules.
 *
 * One GEMM,  out (M, N) = epi( pro(x) (M, K) . W^T (K, N) + b ),  stands for the four Linears of SwinBlock.forward
 * (mmdet3d/models/backbones/swin.py:516-592, forward :581-592) together with what surrounds them:
 *   qkv   pro = LayerNorm (norm1, :583), epi = bias                 WindowMSA.qkv (:293, applied :312)
 *   proj  pro = identity,  epi = bias + residual                    WindowMSA.proj (:295, applied :341) and `x = x + identity` (:586)
 *   fc1   pro = LayerNorm (norm2, :589), epi = bias + GELU          first Linear and activation of mmcv's FFN (built :571, called :590;
 *                                                                   mmcv-full 1.6.0 mmcv/cnn/bricks/transformer.py, class FFN)
 *   fc2   pro = identity,  epi = bias + residual                    second Linear of mmcv's FFN and its `identity + out` (FFN.forward)
 */
#ifndef PREWORLD_HIP_SWIN_LINEAR_H_
#define PREWORLD_HIP_SWIN_LINEAR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* `dtype` is PW_SWIN_F32 or PW_SWIN_BF16 of preworld_hip_swin.h:
 *   PW_SWIN_F32   x, residual and out are float32.  Products are split-fp16 (three fp16 matrix-core products into fp32
 *                 accumulators, csrc/pw_h2.h) and keep fp32-level accuracy with no range state: the weight rows are split once at
 *                 pack time, each under its own power-of-two pre-scale; a LayerNorm operand is bounded by sqrt(K) max|gamma| +
 *                 max|beta|, so its power of two is fixed at pack time; any other x row is scaled by the power of two that puts its
 *                 own largest magnitude in [2^12, 2^13), found by the statistics launch and undone exactly in the epilogue (an all-zero row: 2^0;
 *                 a row holding Inf or NaN: 2^0, the row comes out non-finite and no other row is touched).
 *   PW_SWIN_BF16  autocast's data flow: the residual stream -- x of a LayerNorm prologue, residual, and out of a residual epilogue --
 *                 is float32; every other x and out is bfloat16.  Weights are rounded to bf16 at pack time, the LayerNorm output is
 *                 rounded to bf16 once, products are bf16 with fp32 accumulation, bias and GELU act on the fp32 accumulator and the
 *                 result is rounded once. */
#define PW_SWIN_LINEAR_EPI_BIAS 0        /* out = y,  y = pro(x) W^T + b */
#define PW_SWIN_LINEAR_EPI_GELU 1        /* out = 0.5 y (1 + erf(y / sqrt 2)): nn.GELU's default, not the tanh form */
#define PW_SWIN_LINEAR_EPI_RESIDUAL 2    /* out = residual + y (the operand order of FFN.forward) */
#define PW_SWIN_LINEAR_MIN_DIM 16
#define PW_SWIN_LINEAR_MAX_DIM 4096

/* Bytes of the packed operand of an (N, K) Linear (nn.Linear.weight as stored, swin.py:293-295 and the FFN's two Linears); 0 if the
 * shape or dtype is not supported: K % 16 == 0, N % 16 == 0, 16 <= K, N <= 4096. */
size_t pw_swin_linear_packed_bytes(int K, int N, int dtype);

/* weight (N, K), bias (N) or NULL (zeros: qkv_bias=False, swin.py:293), ln_weight / ln_bias (K) of the LayerNorm in front of the
 * Linear (norm1 / norm2, swin.py:557-570) or both NULL (gamma = 1, beta = 0) -> packed (pw_swin_linear_packed_bytes bytes, 16-byte
 * aligned).  gamma and beta are NOT folded into the weight and bias: the prologue applies them, so the packed bias is the Linear's
 * own.  Two small launches on `stream`, no host synchronisation: capturable. */
int pw_swin_linear_pack(const float* weight, const float* bias, const float* ln_weight, const float* ln_bias, void* packed, int K, int N,
                        int dtype, void* stream);

/* Bytes of workspace pw_swin_linear needs for M rows: (M, 2) floats of row statistics -- the LayerNorm's (mean, 1 / sigma) of
 * swin.py:583 / :589, or in PW_SWIN_F32 mode without it the row's powers of two -- and 0 where there are none (PW_SWIN_BF16 without ln). */
size_t pw_swin_linear_workspace_bytes(int64_t M, int ln, int dtype);

/* out (M, N) = epi(pro(x) W^T + b); the four roles and their reference lines are listed at the top of this file.  Two launches:
 * the row statistics into `workspace` (pw_swin_linear_workspace_bytes; may be NULL where that is 0), then the GEMM.
 *   ln != 0: pro = LayerNorm over K with the packed gamma / beta, float32 statistics, biased variance, `eps` (nn.LayerNorm)
 *   epi:     PW_SWIN_LINEAR_EPI_*; `residual` (M, N) float32 is required for _RESIDUAL and must be NULL otherwise
 *   x:       (M, K) float32; in PW_SWIN_BF16 mode without ln: bfloat16
 *   out:     (M, N) float32; in PW_SWIN_BF16 mode without a residual: bfloat16
 * Rows are independent: row m of out depends on row m of x and residual alone.  Deterministic (no atomics), no temporary in global
 * memory but the workspace, no host synchronisation: capturable.  Any M >= 1 with M x N tiles fitting one launch; K and N as
 * pw_swin_linear_packed_bytes.  Anything else is refused (PW_EUNSUP for K, N; PW_EINVAL otherwise) before any HIP call. */
int pw_swin_linear(const void* x, const void* packed, const float* residual, void* out, float* workspace, size_t workspace_bytes,
                   int64_t M, int K, int N, int ln, float eps, int epi, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PREWORLD_HIP_SWIN_LINEAR_H_ */
