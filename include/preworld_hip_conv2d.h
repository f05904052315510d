/*
 * preworld_hip_conv2d.h -- the stride-1 2-D convolutions behind the image backbone (FPN_LSS and DepthNet) as one implicit GEMM with
 * eval-mode BatchNorm, bias, ReLU and the residual addition fused in, in the C ABI of libpreworld_hip.so; included by preworld_hip.h,
 * whose conventions hold: device pointers unless the name ends in _host, `stream` last, 0 or a negative PW_E* code with a
 * thread-local message.  Kept in a file of its own, like preworld_hip_swin_linear.h, so that the entry-point and pointer-parameter
 * census of preworld_hip.h (tests/test_marshal_cpu.py) stays what it was; preworld_amd/_lib.py parses it the same way and
 * tests/test_conv2d_cpu.py holds it to the same rules.
 *
 * One kernel over channels-last maps,
 *     out (B, H, W, Cout) = epi( scale[c] . sum_{taps, ci} x(b, h + dh d, w + dw d, ci) W[c, ci, tap] + shift[c] ),
 * stands for every stride-1 nn.Conv2d of
 *   FPN_LSS    mmdet3d/models/necks/lss_fpn.py:13-110           conv (:43: 3x3 conv, BN, ReLU, twice) and up2's convs (:64)
 *   DepthNet   mmdet3d/models/necks/view_transformer.py:322-638 reduce_conv (:487: 3x3 conv with bias, BN, ReLU), context_conv
 *              (:493: 1x1 with bias), the three BasicBlocks (:515-518; mmdet 2.24's ResNet block: 3x3 conv, BN, ReLU, 3x3 conv, BN,
 *              + identity or the 1x1 downsample with bias of :505, ReLU), ASPP (:322-426: 1x1 and three dilated 3x3 branches with BN
 *              and ReLU, conv1 + bn1 + ReLU over their concat) and the last 1x1 layer of depth_conv with bias (:535)
 * together with the BatchNorm2d, bias, ReLU and residual addition that follow it there.  Eval mode and forward only.
 */
#ifndef PREWORLD_HIP_CONV2D_H_
#define PREWORLD_HIP_CONV2D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* x, residual and out are float32.  Products are split-fp16 (three fp16 matrix-core products into fp32 accumulators, csrc/pw_h2.h)
 * and keep fp32-level accuracy with no range state: the weight rows are split once at pack time, each under its own power-of-two
 * pre-scale; x is scaled by ONE power of two per call, the one that puts the tensor's largest magnitude in [2^12, 2^13) (an
 * all-zero tensor: 2^0; a tensor holding Inf or NaN: 2^0), found by a small launch in front of the GEMM and undone exactly in
 * the epilogue.  A sum over more than 1024 products is taken in blocks of 1024. */
#define PW_CONV2D_EPI_NONE 0             /* out = y,  y = scale . acc + shift in float32 */
#define PW_CONV2D_EPI_RELU 1             /* out = max(y, 0) */
#define PW_CONV2D_EPI_RESIDUAL_RELU 2    /* out = max(y + residual, 0): BasicBlock's `out += identity; relu(out)` */
#define PW_CONV2D_MIN_DIM 4
#define PW_CONV2D_MAX_DIM 4096

/* Bytes of the packed operand of a (Cout, Cin, ksize, ksize) convolution (nn.Conv2d.weight as stored: lss_fpn.py:46-70,
 * view_transformer.py:322-638); 0 if the shape is not supported: ksize 1 or 3, Cin % 4 == 0, Cout % 4 == 0, 4 <= Cin, Cout <= 4096.
 * With CinP = Cin rounded up to 32 and CoutP = Cout rounded up to 64: 64 + 12 CoutP + 4 CoutP ksize^2 CinP. */
size_t pw_conv2d_packed_bytes(int Cin, int Cout, int ksize);

/* weight (Cout, Cin, ksize, ksize), bias (Cout) or NULL (zeros), and the eval-mode BatchNorm2d behind the convolution (lss_fpn.py:46-70,
 * view_transformer.py:322-638) as its raw parameters and running statistics bn_weight, bn_bias, bn_mean, bn_var (Cout) or all four
 * NULL -> packed (pw_conv2d_packed_bytes bytes, 16-byte aligned).  The launch computes on the device
 *     scale = bn_weight / sqrt(bn_var + bn_eps),  shift = bn_bias + (bias - bn_mean) scale      (no BatchNorm: scale = 1, shift = bias)
 * and writes the weight rows as split-fp16 planes in tap-major order with the k and n tails zero-filled.  One launch on `stream`, no
 * host synchronisation: capturable. */
int pw_conv2d_pack(const float* weight, const float* bias, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                   const float* bn_var, float bn_eps, void* packed, int Cin, int Cout, int ksize, void* stream);

/* Bytes of workspace pw_conv2d needs for a (B, H, W, .) map (lss_fpn.py:13-110, view_transformer.py:322-638 hold no such buffer: it is
 * this kernel's own): 256 partial maxima of |x|, 1024 bytes whatever the size; 0 if B, H or W is not positive. */
size_t pw_conv2d_workspace_bytes(int B, int H, int W);

/* out (B, H, W, Cout) = epi(scale . conv(x (B, H, W, Cin)) + shift) for one convolution of lss_fpn.py:13-110 or
 * view_transformer.py:322-638 (the roles are listed at the top of this file): ksize 1 or 3, stride 1, dilation >= 1, zero padding
 * dilation (ksize - 1) / 2, so the output is the size of the input.  Two launches: the partial maxima of |x| into `workspace`
 * (pw_conv2d_workspace_bytes, 4-byte aligned), then the implicit GEMM with M = B H W, N = Cout, K = ksize^2 Cin, whose A operand is
 * gathered by index arithmetic: a tap that leaves the map reads zero, and no unfolded or padded copy of x exists in global memory.
 *   epi:      PW_CONV2D_EPI_*; `residual` (B, H, W, Cout) is required for _RESIDUAL_RELU and must be NULL otherwise
 *   x, residual, out: channels-last float32, 16-byte aligned; out must not overlap x
 * Deterministic (no atomics), no temporary in global memory but the workspace, nothing survives the call, no host synchronisation:
 * capturable.  Cin, Cout and ksize as pw_conv2d_packed_bytes; B H W < 2^31 and B H W max(Cin, Cout) < 2^40.  Anything else is refused
 * (PW_EUNSUP for Cin, Cout, ksize; PW_EINVAL otherwise) before any HIP call. */
int pw_conv2d(const float* x, const void* packed, const float* residual, float* out, float* workspace, size_t workspace_bytes, int B,
              int H, int W, int Cin, int Cout, int ksize, int dilation, int epi, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PREWORLD_HIP_CONV2D_H_ */
