/*
 * preworld_hip_swin.h -- the image-side (Swin window attention) part of the C ABI of libpreworld_hip.so; included by preworld_hip.h,
 * whose conventions hold: device pointers unless the name ends in _host, `stream` last, 0 or a negative PW_E* code with a
 * thread-local message.  Kept in a file of its own so that the entry-point and pointer-parameter census of preworld_hip.h
 * (tests/test_marshal_cpu.py) stays what it was; preworld_amd/_lib.py parses it the same way and tests/test_swin_attn_cpu.py holds
 * it to the same rules.
 */
#ifndef PREWORLD_HIP_SWIN_H_
#define PREWORLD_HIP_SWIN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PW_SWIN_F32 0        /* qkv, pad_qkv and out are float32; exact-fp32 matrix-core products */
#define PW_SWIN_BF16 1       /* qkv, pad_qkv and out are bfloat16; bf16 products, fp32 logits, softmax and accumulation */
#define PW_SWIN_MAX_WS 12
#define PW_SWIN_MAX_HEAD_DIM 32

/* Shifted-window multi-head attention of one Swin block (mmdet3d/models/backbones/swin.py:244-513 from the qkv Linear's output to
 * the proj Linear's input) in one launch, stated per token so that no padded, rolled or window-ordered copy of the map exists:
 *   qkv  (B, H, W, 3C)  the qkv Linear applied to the UN-padded, UN-rolled tokens, last dim in the Linear's order [3][num_heads][d]
 *   out  (B, H, W, C)   last dim [num_heads][d]
 *   pad_qkv (3C) or NULL   what the Linear gives for a zero token (its bias in the activation dtype); NULL = zeros
 *   bias_table ((2 ws - 1)^2, num_heads) float32, the relative_position_bias_table parameter as stored
 * With Hp = ceil(H / ws) ws, Wp likewise: window (wi, wj) holds the shifted-frame positions i = wi ws + r, j = wj ws + c; the source
 * token of a position is ((i + shift) % Hp, (j + shift) % Wp); a source outside H x W is a padded token whose q, k, v are pad_qkv --
 * it DOES take part as key and value (the reference masks regions, not padding), its own query row is not computed and nothing
 * is written for it.  For shift > 0 the region of a position is 3 ((i >= Hp - ws) + (i >= Hp - shift)) + ((j >= Wp - ws) +
 * (j >= Wp - shift)) and pairs of different regions get the additive -100.  The bias of query a, key b is
 * table[(r_a - r_b + ws - 1)(2 ws - 1) + (c_a - c_b + ws - 1)][head], and
 *   out = softmax(q k^T scale + bias + mask) v   written at the source position.
 * No workspace, no index or mask tensor, no host synchronisation: capturable.  Supported: 2 <= ws <= PW_SWIN_MAX_WS, 0 <= shift < ws,
 * d = C / num_heads <= PW_SWIN_MAX_HEAD_DIM with d % 4 == 0; anything else is refused (PW_EUNSUP / PW_EINVAL) before any HIP call. */
int pw_swin_window_attention(const void* qkv, const void* pad_qkv, const float* bias_table, void* out, int B, int H, int W, int C,
                             int num_heads, int ws, int shift, float scale, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PREWORLD_HIP_SWIN_H_ */
