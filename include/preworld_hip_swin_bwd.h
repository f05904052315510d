/*
 * preworld_hip_swin_bwd.h -- the backward of the Swin window attention (preworld_hip_swin.h) in the C ABI of libpreworld_hip.so;
 * included by preworld_hip.h, whose conventions hold: device pointers unless the name ends in _host, `stream` last, 0 or a negative
 * PW_E* code with a thread-local message.  Kept in a file of its own so that preworld_hip_swin.h stays its single entry point
 * (tests/test_swin_attn_cpu.py); preworld_amd/_lib.py parses it the same way and tests/test_swin_attn_bwd_cpu.py holds it to the
 * same rules.
 */
#ifndef PREWORLD_HIP_SWIN_BWD_H_
#define PREWORLD_HIP_SWIN_BWD_H_

#include <stddef.h>
#include <stdint.h>

#include "preworld_hip_swin.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PW_SWIN_BWD_PAD_SLOTS 64      /* floats per workgroup partial that hold the k and v gradient of its padded tokens (2 x 32) */

/* Gradient of pw_swin_window_attention (same layouts, same per-token statements, same supported range and dtype codes).  Per
 * (window, head) with S = scale q k^T + bias + mask, P = softmax(S), O = P v and the incoming dout:
 *   dv = P^T dout,  dP = dout v^T,  D_i = sum_b P_ib dP_ib (= dout_i . out_i),  dS = P o (dP - D),  dq = scale dS k,  dk = scale dS^T q
 *   dbias_table[(r_a - r_b + ws - 1)(2 ws - 1) + (c_a - c_b + ws - 1)][head] = sum of dS_ab over every window and batch entry
 *   dpad_qkv = sum of the dk, dv rows of all padded tokens (they are keys and values); its q third is exactly zero
 *   qkv (B, H, W, 3C), out and dout (B, H, W, C), dqkv (B, H, W, 3C): float32 (PW_SWIN_F32) or bfloat16 (PW_SWIN_BF16)
 *   pad_qkv (3C) in that dtype or NULL; bias_table, dbias_table ((2 ws - 1)^2, num_heads) and dpad_qkv (3C) float32
 * `out` is what the forward wrote for this qkv; nothing else is saved: logits, row maximum and row sum are recomputed as the forward
 * computes them.  This implementation forms D as sum_b P_ab dP_ab (the same number, out = P v) from registers it holds anyway, which
 * makes dS exactly zero where the softmax has saturated and keeps out's bf16 rounding out of D; `out` is checked and not read.
 * Every dqkv row is written exactly once with plain stores (every real token belongs to one window).  Products are fp32 on the
 * matrix cores for both dtypes (bf16 is a storage format here), all accumulation is fp32.
 * dbias_table == NULL skips the table gradient; dpad_qkv == NULL skips the pad gradient and is required when pad_qkv is NULL.
 * dbias_table and dpad_qkv are sums over workgroups: each (window, head) workgroup writes one partial of
 * (2 ws - 1)^2 + PW_SWIN_BWD_PAD_SLOTS floats into `workspace` and a second launch adds the partials in a fixed order -- no
 * floating-point atomics, two calls give the same bits.  The workspace must hold
 *   workspace_bytes >= 4 * B * ceil(H / ws) * ceil(W / ws) * num_heads * ((2 ws - 1)^2 + PW_SWIN_BWD_PAD_SLOTS)
 * bytes (4-byte aligned; its contents before and after the call mean nothing); when both dbias_table and dpad_qkv are NULL none is
 * needed and it may be NULL.  A smaller one is refused.  No host synchronisation: capturable.  Anything unsupported is refused
 * (PW_EUNSUP / PW_EINVAL) before any HIP call. */
int pw_swin_window_attention_backward(const void* qkv, const void* pad_qkv, const float* bias_table, const void* out, const void* dout,
                                      void* dqkv, float* dpad_qkv, float* dbias_table, void* workspace, int64_t workspace_bytes,
                                      int B, int H, int W, int C, int num_heads, int ws, int shift, float scale, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PREWORLD_HIP_SWIN_BWD_H_ */
