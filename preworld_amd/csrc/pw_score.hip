// ------------------------------------------------------------------------------------
// A22b  fused multi-horizon occupancy scoring (mmdet3d/datasets/occ_metrics.py:82-105 hist_info, :135-158 add_batch,
// :502-542 the temporal evaluate loop): ONE launch adds a sample's confusion counts for every horizon h < H <= 8 into
// counts[h][n_cl*n_cl + 4] --
//   [0, n_cl^2)       bincount(n_cl*gt + pred) over masked voxels with gt < n_cl (gt = 255 dropped), pred < n_cl
//   [n_cl^2, +4)      the binary 2x2 histogram [2*(gt != free) + (pred != free)], free = n_cl - 1, over masked voxels:
//                     gt = 255 counts as occupied there (the reference's `semantics_gt != 17` on the raw grid)
// The metric's per-sample path was 2 pw_confusion_hist launches + 4 elementwise ops + 3 host<->device copies per horizon.
//
// Shape: blockIdx.y = horizon, blockIdx.x = a >= 16 K-voxel share of it.  16-byte loads of pred / gt / mask; per-wave
// LDS histograms (the 18^2 bins are hit by LDS atomics, the binary bins are counted in registers and added once per
// thread); one 64-bit global atomic per non-zero bin per block.  Integer adds: exact in any order, bit-identical
// from run to run.  The pointer table travels by value in the kernel arguments (capturable, no device table).
// ------------------------------------------------------------------------------------
#include "pw_common.h"

namespace {
constexpr int OS_MAX_H = 8;
constexpr int OS_MAX_CL = 32;
constexpr int OS_THREADS = 256;
constexpr int OS_WAVES = OS_THREADS / PW_WAVE;
constexpr int64_t OS_VOX_PER_BLOCK = 16384;

struct OccScoreArgs {
  const uint8_t* pred[OS_MAX_H];
  const uint8_t* gt[OS_MAX_H];
  const uint8_t* mask[OS_MAX_H];      // nullptr: every voxel counts
};

struct BinCounts { unsigned tot, g1, p1, both; };

__device__ __forceinline__ void score_byte(unsigned p, unsigned g, unsigned m, unsigned n_cl, unsigned free_cl,
                                           unsigned* __restrict__ wh, BinCounts& b) {
  if (!m) return;
  if (g < n_cl && p < n_cl) atomicAdd(&wh[g * n_cl + p], 1u);
  const unsigned gb = g != free_cl, pb = p != free_cl;
  b.tot += 1u; b.g1 += gb; b.p1 += pb; b.both += gb & pb;
}

__device__ __forceinline__ void score_word(unsigned p, unsigned g, unsigned m, unsigned n_cl, unsigned free_cl,
                                           unsigned* __restrict__ wh, BinCounts& b) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    score_byte((p >> (8 * k)) & 0xffu, (g >> (8 * k)) & 0xffu, (m >> (8 * k)) & 0xffu, n_cl, free_cl, wh, b);
}

__global__ void __launch_bounds__(OS_THREADS)
k_occ_score(OccScoreArgs a, int64_t n, int n_cl, unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned lh[];                       // [OS_WAVES][nbins]
  const int h = blockIdx.y;
  const int nb = n_cl * n_cl, nbins = nb + 4;
  const unsigned ucl = (unsigned)n_cl, free_cl = (unsigned)(n_cl - 1);
  for (int k = threadIdx.x; k < OS_WAVES * nbins; k += blockDim.x) lh[k] = 0u;
  __syncthreads();
  unsigned* wh = lh + (threadIdx.x / PW_WAVE) * nbins;
  const uint8_t* __restrict__ pred = a.pred[h];
  const uint8_t* __restrict__ gt = a.gt[h];
  const uint8_t* __restrict__ mask = a.mask[h];
  BinCounts b = {0u, 0u, 0u, 0u};
  // 16-byte body when every row of this horizon is 16-byte aligned (the payload rows and torch allocations are)
  const bool aligned = ((((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)(mask ? mask : pred)) & 15) == 0);
  const int64_t n16 = aligned ? n / 16 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
    const uint4 p = reinterpret_cast<const uint4*>(pred)[i];
    const uint4 g = reinterpret_cast<const uint4*>(gt)[i];
    const uint4 m = mask ? reinterpret_cast<const uint4*>(mask)[i] : make_uint4(~0u, ~0u, ~0u, ~0u);
    score_word(p.x, g.x, m.x, ucl, free_cl, wh, b);
    score_word(p.y, g.y, m.y, ucl, free_cl, wh, b);
    score_word(p.z, g.z, m.z, ucl, free_cl, wh, b);
    score_word(p.w, g.w, m.w, ucl, free_cl, wh, b);
  }
  for (int64_t i = n16 * 16 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)     // the tail (< 16 voxels when aligned)
    score_byte(pred[i], gt[i], mask ? mask[i] : 1u, ucl, free_cl, wh, b);
  // binary 2x2: [gt free, pred free], [gt free, pred occ], [gt occ, pred free], [gt occ, pred occ]
  if (b.tot) {
    atomicAdd(&wh[nb + 0], b.tot - b.g1 - b.p1 + b.both);
    atomicAdd(&wh[nb + 1], b.p1 - b.both);
    atomicAdd(&wh[nb + 2], b.g1 - b.both);
    atomicAdd(&wh[nb + 3], b.both);
  }
  __syncthreads();
  unsigned long long* __restrict__ out = counts + (int64_t)h * nbins;
  for (int k = threadIdx.x; k < nbins; k += blockDim.x) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < OS_WAVES; ++w) s += lh[w * nbins + k];
    if (s) atomicAdd(&out[k], s);
  }
}
}  // namespace

PW_API int pw_occ_score(const uint8_t* const* pred_host, const uint8_t* const* gt_host, const uint8_t* const* mask_host,
                        int n_h, int64_t n, int n_cl, int64_t* counts, void* stream) {
  PW_CHECK_ARG(pred_host && gt_host && counts && n_h >= 1 && n_h <= OS_MAX_H && n >= 0 && n <= INT32_MAX && n_cl >= 2 &&
                   n_cl <= OS_MAX_CL, "pw_occ_score: bad arguments");
  OccScoreArgs a = {};
  for (int h = 0; h < n_h; ++h) {
    PW_CHECK_ARG(n == 0 || (pred_host[h] && gt_host[h]), "pw_occ_score: null pred / gt pointer of horizon %d", h);
    a.pred[h] = pred_host[h];
    a.gt[h] = gt_host[h];
    a.mask[h] = mask_host ? mask_host[h] : nullptr;
  }
  if (n == 0) return PW_OK;
  const int64_t want = pw_cdiv(n, OS_VOX_PER_BLOCK);
  const unsigned nbx = (unsigned)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
  const size_t lds = (size_t)OS_WAVES * (n_cl * n_cl + 4) * sizeof(unsigned);
  hipLaunchKernelGGL(k_occ_score, dim3(nbx, (unsigned)n_h), dim3(OS_THREADS), lds, pw_stream(stream), a, n, n_cl,
                     reinterpret_cast<unsigned long long*>(counts));
  PW_CHECK_LAUNCH();
  return PW_OK;
}
