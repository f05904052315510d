// The Linears of a Swin block (include/preworld_hip_swin_linear.h) as one templated GEMM:
//     out (M, N) = epi( pro(x) (M, K) . W^T (K, N) + b )
// pro = identity or LayerNorm over K, epi = bias, bias + erf-GELU or bias + residual.  No normalised copy of x, no pre-GELU hidden
// tensor and no un-added proj / fc2 output exists in global memory.
//
// Orientation.  The product is computed TRANSPOSED, out^T = W . pro(x)^T, with v_mfma_f32_32x32x16_{f16,bf16}: the weight rows are the
// A operand, the token rows the B operand, so a lane of the 32x32 accumulator holds ONE token (column = lane & 31) and, per group of
// four registers, four CONSECUTIVE output channels: bias, GELU, residual and the store are 16-byte (bf16: 8-byte) accesses with no
// cross-lane step, and a non-finite token stays in its own column.
//
// Tiles.  A workgroup of 4 waves (2 x 2) owns BM = 64 TM tokens x BN = 64 TN channels, a wave TM x TN accumulator tiles; k advances
// in chunks of 64.  Both operands of a chunk sit in LDS as rows of 64 halves padded to 144 bytes: the 16-byte fragment reads of 16
// consecutive rows then start 36 banks apart and cover all 64 banks once (conflict-free ds_read_b128).  The next chunk's global loads
// are issued before the current chunk's MFMAs and land in registers; the transform (LayerNorm or row scale, split or rounding) runs
// when they are written to LDS.  TM = TN = 2 (128 x 128) is the throughput shape (128 x 64 for F32 with K > 1024, see DEEP);
// TM = TN = 1 (64 x 64) is taken when the large tile would leave CUs idle (small maps, the toy model).  Neighbouring workgroups
// share their token rows (the channel tile is the fast index), so x is read from HBM once and the packed weight lives in L2.
//
// PW_SWIN_F32: split-fp16, x w = hi_x hi_w + hi_x lo_w + lo_x hi_w (pw_h2.h), with no range slots: weight row n is packed as
// (hi, lo) of w 2^-e_n, e_n from the row's own absmax; a LayerNorm operand is scaled by the power of two that puts the pack-time bound
// sqrt(K) max|gamma| + max|beta| in [2^12, 2^13); any other row by the power of two of its OWN absmax, found by the
// statistics launch.  The epilogue multiplies by the two inverse powers: exact.  PW_SWIN_BF16: one bf16 plane per operand.
// Row statistics (mean and 1/sigma, two passes; or the power of two of the absmax) come from k_swin_linear_stats, a small launch in
// front of the GEMM that writes (M, 2) floats of caller-provided workspace.  Recomputing them in every workgroup was measured first:
// every column tile then reads its rows two more times before its first MFMA -- 24 column tiles for qkv of stage 3 -- and the
// LayerNorm roles ran at 0.6 of the rate of the others (profiles/swin_linear.md).
#include "pw_swin_linear_common.h"

PW_API size_t pw_swin_linear_packed_bytes(int K, int N, int dtype) {
  if (check_dims("pw_swin_linear_packed_bytes", K, N, dtype) != 0) return 0;
  return packed_bytes(K, N, dtype == PW_SWIN_BF16 ? 1 : 2);
}

PW_API int pw_swin_linear_pack(const float* weight, const float* bias, const float* ln_weight, const float* ln_bias, void* packed, int K,
                               int N, int dtype, void* stream) {
  PW_CHECK_ARG(weight && packed, "pw_swin_linear_pack: null pointer");
  const int rc = check_dims("pw_swin_linear_pack", K, N, dtype);
  if (rc != 0) return rc;
  PW_CHECK_ARG((ln_weight == nullptr) == (ln_bias == nullptr), "pw_swin_linear_pack: ln_weight and ln_bias come together or not at all");
  PW_CHECK_ARG(((uintptr_t)packed & 15) == 0 && (((uintptr_t)weight | (uintptr_t)bias | (uintptr_t)ln_weight | (uintptr_t)ln_bias) & 3) == 0,
               "pw_swin_linear_pack: packed must be 16-byte aligned, the float arrays 4-byte aligned");
  hipStream_t st = pw_stream(stream);
  if (dtype == PW_SWIN_BF16) {
    hipLaunchKernelGGL(k_swin_linear_pack_rows<true>, dim3(N), dim3(64), 0, st, weight, bias, packed, K, N);
    hipLaunchKernelGGL(k_swin_linear_pack_ln<true>, dim3(1), dim3(256), 0, st, ln_weight, ln_bias, packed, K, N);
  } else {
    hipLaunchKernelGGL(k_swin_linear_pack_rows<false>, dim3(N), dim3(64), 0, st, weight, bias, packed, K, N);
    hipLaunchKernelGGL(k_swin_linear_pack_ln<false>, dim3(1), dim3(256), 0, st, ln_weight, ln_bias, packed, K, N);
  }
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_swin_linear_pack_rows<%d>", (int)(dtype == PW_SWIN_BF16));
  return 0;
}

PW_API size_t pw_swin_linear_workspace_bytes(int64_t M, int ln, int dtype) {
  if (M < 1 || (dtype == PW_SWIN_BF16 && !ln)) return 0;
  return 8u * (size_t)M;
}

PW_API int pw_swin_linear(const void* x, const void* packed, const float* residual, void* out, float* workspace, size_t workspace_bytes,
                          int64_t M, int K, int N, int ln, float eps, int epi, int dtype, void* stream) {
  PW_CHECK_ARG(x && packed && out, "pw_swin_linear: null pointer");
  const int rc = check_dims("pw_swin_linear", K, N, dtype);
  if (rc != 0) return rc;
  PW_CHECK_ARG(M >= 1, "pw_swin_linear: M must be positive, got %lld", (long long)M);
  PW_CHECK_ARG(epi == EPI_BIAS || epi == EPI_GELU || epi == EPI_RES, "pw_swin_linear: epi must be a PW_SWIN_LINEAR_EPI_* value, got %d", epi);
  PW_CHECK_ARG((epi == EPI_RES) == (residual != nullptr), "pw_swin_linear: residual is required for PW_SWIN_LINEAR_EPI_RESIDUAL and must be NULL otherwise");
  PW_CHECK_ARG(!ln || (eps >= 0.f && eps < INFINITY), "pw_swin_linear: eps must be finite and non-negative");
  const bool bf = dtype == PW_SWIN_BF16;
  const size_t need = pw_swin_linear_workspace_bytes(M, ln, dtype);
  PW_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0),
               "pw_swin_linear: workspace of %zu bytes needed (8-byte aligned), got %zu", need, workspace_bytes);
  const uintptr_t xa = (bf && !ln) ? 7 : 15, oa = (bf && epi != EPI_RES) ? 7 : 15;      // four elements per access
  PW_CHECK_ARG(((uintptr_t)x & xa) == 0 && ((uintptr_t)out & oa) == 0 && ((uintptr_t)residual & 15) == 0 && ((uintptr_t)packed & 15) == 0,
               "pw_swin_linear: x, residual, out and packed must be aligned to four elements (packed: 16 bytes)");
  const bool ran = run_linear<false>(x, packed, residual, out, workspace, need != 0, M, K, N, ln != 0, eps, epi, bf, pw_stream(stream),
                                     "k_swin_linear<%d, %d, %d, %d, %d, %d>");
  PW_CHECK_ARG(ran, "pw_swin_linear: %lld rows do not fit one launch", (long long)M);
  PW_CHECK_LAUNCH();
  return 0;
}
