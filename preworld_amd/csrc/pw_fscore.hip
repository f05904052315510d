// ------------------------------------------------------------------------------------
// A22c  occupancy F-score on the voxel lattice (mmdet3d/datasets/occ_metrics.py:322-410 Metric_FScore).  The reference turns
// the occupied voxels of gt and pred into centre points (voxel2points, :352-363) and queries two sklearn KDTrees for each
// point's nearest neighbour on the other side (:383-397).  With every point on one lattice, "a point of the other grid lies
// closer than t" holds exactly when the other grid is occupied at one of a fixed set of integer offsets (dx, dy, dz) with
// |(dx*vx, dy*vy, dz*vz)| < t; for a fixed (dx, dy) the admissible dz form one range |dz| <= m(dx, dy) (m = -1: none).  The
// host derives m (ops.fscore_offsets) and refuses thresholds that some lattice distance ties.  So the metric is a stencil:
//   * every (x, y) column becomes a Z-bit occupancy word (bit z: the voxel's value, 255 where the mask is 0, is not void);
//   * the other grid's words around the column are smeared along z by m(dx, dy) and OR-ed over the (dx, dy) window;
//   * popcount(own & dilated other) counts the hits.
// pw_occ_fscore adds counts[h] = {n_pred, n_pred_hit, n_gt, n_gt_hit} for up to 8 horizons in ONE launch.
//
// Shape: blockIdx.y = horizon, blockIdx.x = a 16 x 16 tile of (x, y) columns; the tile's words plus an rx / ry halo are built
// in LDS (one 16-byte load of pred / gt / mask per column at Z = 16, y fastest across a wave: 256 contiguous bytes per x row),
// then every thread scores one column.  Wave reduction, then at most 4 64-bit atomics per block: integer adds, exact in any
// order.  The pointers, the void set and both m tables travel by value in the kernel arguments (capturable, no device table).
//
// pw_occ_fscore_accumulate folds such count tables into float64 running totals with the reference's arithmetic (:399-408),
// one thread per horizon, samples in order; this file is compiled without FMA contraction so the totals are the same float64
// operations as the reference's Python.
// ------------------------------------------------------------------------------------
#include "pw_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int FS_MAX_H = 8;
constexpr int FS_MAX_Z = 64;
constexpr int FS_MAX_R = 7;
constexpr int FS_W = 2 * FS_MAX_R + 1;                 // the m tables are [FS_W][FS_W], centre at (FS_MAX_R, FS_MAX_R)
constexpr int FS_T = 16;                               // a tile is FS_T x FS_T columns, one per thread
constexpr int FS_THREADS = FS_T * FS_T;
constexpr int FS_WAVES = FS_THREADS / PW_WAVE;
constexpr int FS_P = FS_T + 2 * FS_MAX_R;              // LDS pitch (and rows) of the haloed tile

struct OccFscoreArgs {
  const uint8_t* pred[FS_MAX_H];
  const uint8_t* gt[FS_MAX_H];
  const uint8_t* mask[FS_MAX_H];                       // nullptr: every voxel counts
  uint32_t void_bits[8];                               // bit v: value v is not occupied
  int8_t m_acc[FS_W * FS_W];                           // [dx + 7][dy + 7]: gt within thr_acc of a pred voxel
  int8_t m_cmpl[FS_W * FS_W];                          // [dx + 7][dy + 7]: pred within thr_cmpl of a gt voxel
};

// bits z' with |z' - z| <= m for some set bit z of w (m <= 63); bits at or above Z are cleared by the caller
__device__ __forceinline__ uint64_t smear(uint64_t w, int m) {
  for (int r = 0; r < m;) {
    const int s = min(r + 1, m - r);                  // x covers [-r, r]: shifting by s <= 2r + 1 keeps it contiguous
    w |= (w << s) | (w >> s);
    r += s;
  }
  return w;
}

__device__ __forceinline__ uint64_t dilate(const uint64_t* __restrict__ lw, int c, const int8_t* __restrict__ mt, int rx, int ry) {
  uint64_t d = 0;
  for (int dx = -rx; dx <= rx; ++dx)
    for (int dy = -ry; dy <= ry; ++dy) {
      const int m = mt[(dx + FS_MAX_R) * FS_W + dy + FS_MAX_R];
      if (m >= 0) d |= smear(lw[c + dx * FS_P + dy], m);
    }
  return d;
}

__device__ __forceinline__ unsigned occ_bits(unsigned v, unsigned m, const uint8_t* __restrict__ lut) {
  // 4 bytes of a grid word -> 4 occupancy bits (masked voxels read as 255)
  unsigned b = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned x = ((m >> (8 * k)) & 0xffu) ? ((v >> (8 * k)) & 0xffu) : 255u;
    b |= (unsigned)lut[x] << k;
  }
  return b;
}

__global__ void __launch_bounds__(FS_THREADS)
k_occ_fscore(OccFscoreArgs a, int X, int Y, int Z, int rx, int ry, int tiles_y, unsigned long long* __restrict__ counts) {
  __shared__ uint64_t lp[FS_P * FS_P];
  __shared__ uint64_t lg[FS_P * FS_P];
  __shared__ uint8_t lut[256];                         // 1: occupied
  __shared__ int8_t lm[2][FS_W * FS_W];
  __shared__ unsigned red[FS_WAVES][4];
  const int tid = threadIdx.x, h = blockIdx.y;
  const int x0 = (int)(blockIdx.x / (unsigned)tiles_y) * FS_T, y0 = (int)(blockIdx.x % (unsigned)tiles_y) * FS_T;
  lut[tid] = (uint8_t)(((a.void_bits[tid >> 5] >> (tid & 31)) & 1u) ^ 1u);
  for (int k = tid; k < FS_W * FS_W; k += FS_THREADS) {
    lm[0][k] = a.m_acc[k];
    lm[1][k] = a.m_cmpl[k];
  }
  __syncthreads();

  const uint8_t* __restrict__ pred = a.pred[h];
  const uint8_t* __restrict__ gt = a.gt[h];
  const uint8_t* __restrict__ mask = a.mask[h];
  const bool vec = (Z & 15) == 0 && ((((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)(mask ? mask : pred)) & 15) == 0);
  // the haloed tile: columns x0 - rx .. x0 + 15 + rx, y0 - ry .. y0 + 15 + ry; outside the grid a column is empty
  const int hw = FS_T + 2 * ry, n_load = (FS_T + 2 * rx) * hw;
  for (int i = tid; i < n_load; i += FS_THREADS) {
    const int lx = i / hw, ly = i - lx * hw;
    const int gx = x0 - rx + lx, gy = y0 - ry + ly;
    uint64_t wp = 0, wg = 0;
    if (gx >= 0 && gx < X && gy >= 0 && gy < Y) {
      const int64_t base = ((int64_t)gx * Y + gy) * Z;
      if (vec) {
        for (int z = 0; z < Z; z += 16) {
          const uint4 p = *reinterpret_cast<const uint4*>(pred + base + z);
          const uint4 g = *reinterpret_cast<const uint4*>(gt + base + z);
          const uint4 m = mask ? *reinterpret_cast<const uint4*>(mask + base + z) : make_uint4(~0u, ~0u, ~0u, ~0u);
          const uint64_t bp = occ_bits(p.x, m.x, lut) | occ_bits(p.y, m.y, lut) << 4 | occ_bits(p.z, m.z, lut) << 8 |
                              occ_bits(p.w, m.w, lut) << 12;
          const uint64_t bg = occ_bits(g.x, m.x, lut) | occ_bits(g.y, m.y, lut) << 4 | occ_bits(g.z, m.z, lut) << 8 |
                              occ_bits(g.w, m.w, lut) << 12;
          wp |= bp << z;
          wg |= bg << z;
        }
      } else {
        for (int z = 0; z < Z; ++z) {
          const bool keep = !mask || mask[base + z];
          wp |= (uint64_t)lut[keep ? pred[base + z] : 255] << z;
          wg |= (uint64_t)lut[keep ? gt[base + z] : 255] << z;
        }
      }
    }
    lp[lx * FS_P + ly] = wp;
    lg[lx * FS_P + ly] = wg;
  }
  __syncthreads();

  // one column per thread, y fastest (the load order)
  const int tx = tid / FS_T, ty = tid % FS_T;
  unsigned c4[4] = {0u, 0u, 0u, 0u};                  // n_pred, n_pred_hit, n_gt, n_gt_hit
  if (x0 + tx < X && y0 + ty < Y) {
    const uint64_t zmask = Z == 64 ? ~0ull : ((1ull << Z) - 1ull);
    const int c = (tx + rx) * FS_P + ty + ry;
    const uint64_t p = lp[c], g = lg[c];
    const uint64_t near_gt = dilate(lg, c, lm[0], rx, ry) & zmask;
    const uint64_t near_pred = dilate(lp, c, lm[1], rx, ry) & zmask;
    c4[0] = __popcll(p);
    c4[1] = __popcll(p & near_gt);
    c4[2] = __popcll(g);
    c4[3] = __popcll(g & near_pred);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (int off = PW_WAVE / 2; off > 0; off >>= 1) c4[k] += __shfl_xor(c4[k], off);
  if ((tid & (PW_WAVE - 1)) == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) red[tid / PW_WAVE][k] = c4[k];
  __syncthreads();
  if (tid < 4) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < FS_WAVES; ++w) s += red[w][tid];
    if (s) atomicAdd(&counts[(int64_t)h * 4 + tid], s);
  }
}

// counts [n_s][n_h][4] -> totals [n_h][3] += (acc, cmpl, f) of every sample, in sample order (occ_metrics.py:380-408)
__global__ void k_occ_fscore_accumulate(const long long* __restrict__ counts, int n_s, int n_h, double* __restrict__ totals,
                                        long long* __restrict__ n_empty_gt) {
  const int h = threadIdx.x;
  if (h >= n_h) return;
  const double eps = 1e-8;
  double ta = totals[h * 3 + 0], tc = totals[h * 3 + 1], tf = totals[h * 3 + 2];
  long long ne = 0;
  for (int s = 0; s < n_s; ++s) {
    const long long* c = counts + ((int64_t)s * n_h + h) * 4;
    const long long np = c[0], nph = c[1], ng = c[2], ngh = c[3];
    double acc = 0.0, cmpl = 0.0, f = 0.0;
    if (np > 0 && ng == 0) {
      ne += 1;                                         // the reference raises here (KDTree of no points): counted as (0, 0, 0)
    } else if (np > 0) {
      acc = (double)nph / (double)np;                 // accuracy_mask.mean(): an exact integer sum over an integer count
      cmpl = (double)ngh / (double)ng;
      f = 2.0 / (1.0 / (acc + eps) + 1.0 / (cmpl + eps));
    }
    ta = ta + acc;
    tc = tc + cmpl;
    tf = tf + f;
  }
  totals[h * 3 + 0] = ta;
  totals[h * 3 + 1] = tc;
  totals[h * 3 + 2] = tf;
  if (ne) n_empty_gt[h] += ne;
}
}  // namespace

PW_API int pw_occ_fscore(const uint8_t* const* pred_host, const uint8_t* const* gt_host, const uint8_t* const* mask_host,
                         int n_h, int X, int Y, int Z, const uint32_t* void_bits, const int8_t* m_acc, const int8_t* m_cmpl,
                         int rx, int ry, int64_t* counts, void* stream) {
  PW_CHECK_ARG(n_h >= 1 && n_h <= FS_MAX_H, "pw_occ_fscore: 1 <= n_h <= %d horizons, got %d", FS_MAX_H, n_h);
  PW_CHECK_ARG(Z >= 0 && Z <= FS_MAX_Z, "pw_occ_fscore: Z = %d, at most %d voxels per column", Z, FS_MAX_Z);
  PW_CHECK_ARG(rx >= 0 && rx <= FS_MAX_R && ry >= 0 && ry <= FS_MAX_R,
               "pw_occ_fscore: neighbour window rx = %d, ry = %d, at most %d (a smaller threshold or larger voxels)", rx, ry,
               FS_MAX_R);
  PW_CHECK_ARG(pred_host && gt_host && void_bits && m_acc && m_cmpl && counts && X >= 0 && Y >= 0 &&
                   (int64_t)X * Y * Z <= INT32_MAX, "pw_occ_fscore: bad arguments");
  OccFscoreArgs a = {};
  for (int h = 0; h < n_h; ++h) {
    PW_CHECK_ARG(pred_host[h] && gt_host[h], "pw_occ_fscore: null pred / gt pointer of horizon %d", h);
    a.pred[h] = pred_host[h];
    a.gt[h] = gt_host[h];
    a.mask[h] = mask_host ? mask_host[h] : nullptr;
  }
  for (int k = 0; k < 8; ++k) a.void_bits[k] = void_bits[k];
  // the tables arrive as [2rx + 1][2ry + 1]; outside them no offset is admissible
  for (int k = 0; k < FS_W * FS_W; ++k) a.m_acc[k] = a.m_cmpl[k] = -1;
  for (int i = 0; i < 2 * rx + 1; ++i)
    for (int j = 0; j < 2 * ry + 1; ++j) {
      const int8_t ma = m_acc[i * (2 * ry + 1) + j], mc = m_cmpl[i * (2 * ry + 1) + j];
      PW_CHECK_ARG(ma >= -1 && ma <= 63 && mc >= -1 && mc <= 63, "pw_occ_fscore: m table entries must lie in [-1, 63]");
      a.m_acc[(i - rx + FS_MAX_R) * FS_W + j - ry + FS_MAX_R] = ma;
      a.m_cmpl[(i - rx + FS_MAX_R) * FS_W + j - ry + FS_MAX_R] = mc;
    }
  if ((int64_t)X * Y * Z == 0) return PW_OK;
  const int tiles_x = (int)pw_cdiv(X, FS_T), tiles_y = (int)pw_cdiv(Y, FS_T);
  hipLaunchKernelGGL(k_occ_fscore, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n_h), dim3(FS_THREADS), 0, pw_stream(stream), a,
                     X, Y, Z, rx, ry, tiles_y, reinterpret_cast<unsigned long long*>(counts));
  PW_CHECK_LAUNCH();
  return PW_OK;
}

PW_API int pw_occ_fscore_accumulate(const int64_t* counts, int n_s, int n_h, double* totals, int64_t* n_empty_gt, void* stream) {
  PW_CHECK_ARG(n_h >= 1 && n_h <= FS_MAX_H, "pw_occ_fscore_accumulate: 1 <= n_h <= %d horizons, got %d", FS_MAX_H, n_h);
  PW_CHECK_ARG(counts && totals && n_empty_gt && n_s >= 0, "pw_occ_fscore_accumulate: bad arguments");
  if (n_s == 0) return PW_OK;
  hipLaunchKernelGGL(k_occ_fscore_accumulate, dim3(1), dim3(PW_WAVE), 0, pw_stream(stream),
                     reinterpret_cast<const long long*>(counts), n_s, n_h, totals, reinterpret_cast<long long*>(n_empty_gt));
  PW_CHECK_LAUNCH();
  return PW_OK;
}
