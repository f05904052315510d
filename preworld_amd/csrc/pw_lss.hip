// Lift-Splat-Shoot voxel pooling for gfx950: geometry -> voxel ids -> stable segmented
// sort -> dense, write-once pooling.  Replaces (reference paths):
//   mmdet3d/models/necks/view_transformer.py:114-153  get_lidar_coor
//   mmdet3d/models/necks/view_transformer.py:203-261  voxel_pooling_prepare_v2
//   mmdet3d/ops/bev_pool_v2/src/bev_pool_cuda.cu:21-121  bev_pool_v2 fwd/bwd kernels
//
// This file is compiled with -ffp-contract=off: the geometry chain and the pooled sums
// follow exactly the op order of the test oracle (which is bit-identical to the
// reference's torch-CPU get_lidar_coor), so voxel ids AND pooled fp32 sums are
// bit-reproducible against the oracle.
//
// HBM-bound integer/byte work: no MFMA here.  Layout choices:
//   * points are never materialised as coordinates (17.8 MB in the reference) -- only the
//     int32 voxel id per frustum point (5.9 MB);
//   * the sort is a counting sort over the dense voxel range (histogram, exclusive scan,
//     atomic scatter, in-segment rank sort) -> deterministic ascending point order;
//   * pooling is voxel-driven: each group of C/4 lanes owns one voxel, walks its segment
//     with float4 gathers of feat, and writes the (Z,Y,X,C) row once (sum or zeros):
//     coalesced 1 KiB per wave-store, no memset pass, no permute pass.
#include "pw_lss_common.h"

// ------------------------------------------------------------------------------------
// camera matrices (closed-form 3x3 inverse, same op order as oracle inv3x3_f32)
// ------------------------------------------------------------------------------------
__global__ void k_camera_matrices(int BN, const float* __restrict__ s2e,
                                  const float* __restrict__ K, const float* __restrict__ pr,
                                  float* __restrict__ ipr, float* __restrict__ comb,
                                  float* __restrict__ tr) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= BN) return;
  lss_camera_matrix_one(c, s2e, K, pr, ipr, comb, tr);
}

PW_API int pw_lss_camera_matrices(int BN, const float* sensor2ego, const float* cam2imgs,
                                  const float* post_rots, float* inv_post_rot, float* combine,
                                  float* trans, void* stream) {
  PW_CHECK_ARG(BN > 0 && sensor2ego && cam2imgs && post_rots && inv_post_rot && combine && trans,
               "pw_lss_camera_matrices: bad arguments");
  hipLaunchKernelGGL(k_camera_matrices, dim3((BN + 63) / 64), dim3(64), 0, pw_stream(stream), BN,
                     sensor2ego, cam2imgs, post_rots, inv_post_rot, combine, trans);
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// ------------------------------------------------------------------------------------
// frustum point -> voxel id
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_voxel_index(int N, int64_t DHW, int64_t total, const float* __restrict__ frustum,
              const float* __restrict__ ipr, const float* __restrict__ ptr,
              const float* __restrict__ comb, const float* __restrict__ trn,
              const float* __restrict__ bda, GridParams gp, int32_t* __restrict__ vox,
              float* __restrict__ coor_out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  vox[i] = lss_voxel_of_point(i, N, DHW, frustum, ipr, ptr, comb, trn, bda, gp, coor_out);
}

PW_API int pw_lss_voxel_index(int B, int N, int D, int H, int W, const float* frustum,
                              const float* inv_post_rot, const float* post_trans,
                              const float* combine, const float* trans, const float* bda,
                              const float* lower3_host, const float* interval3_host, int gx,
                              int gy, int gz, int32_t* vox, float* coor_out, void* stream) {
  PW_CHECK_ARG(B > 0 && N > 0 && D > 0 && H > 0 && W > 0, "pw_lss_voxel_index: bad shape");
  PW_CHECK_ARG(frustum && inv_post_rot && post_trans && combine && trans && bda && vox &&
                   lower3_host && interval3_host,
               "pw_lss_voxel_index: null pointer");
  PW_CHECK_ARG((int64_t)B * gx * gy * gz < (int64_t)1 << 31, "pw_lss_voxel_index: grid too large");
  int64_t DHW = (int64_t)D * H * W, total = DHW * B * N;
  PW_CHECK_ARG(total < (int64_t)1 << 31, "pw_lss_voxel_index: too many frustum points");
  GridParams gp{lower3_host[0], lower3_host[1], lower3_host[2], interval3_host[0],
                interval3_host[1], interval3_host[2], gx, gy, gz};
  hipLaunchKernelGGL(k_voxel_index, dim3((unsigned)pw_cdiv(total, 256)), dim3(256), 0,
                     pw_stream(stream), N, DHW, total, frustum, inv_post_rot, post_trans, combine,
                     trans, bda, gp, vox, coor_out);
  pw_note_kernel("k_voxel_index");
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// ------------------------------------------------------------------------------------
// exclusive scan (int32), three passes, 2048-element tiles
// ------------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

__device__ __forceinline__ int wave_inclusive_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    int t = __shfl_up(v, off, 64);
    if (lane >= off) v += t;
  }
  return v;
}

// exclusive scan of one value per thread across a 256-thread block; returns exclusive
// prefix, *total = block sum.  lds: 4 ints.
__device__ __forceinline__ int block_exclusive_scan(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = wave_inclusive_scan(v);
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < SCAN_THREADS / 64; ++k) {
    int s = lds[k];
    if (k < w) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_reduce(const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ sums) {
  __shared__ int lds[4];
  int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  int s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k)
    if (base + k < n) s += in[base + k];
  int tot;
  block_exclusive_scan(s, lds, &tot);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_sums(int32_t* __restrict__ sums, int nb) {
  __shared__ int lds[4];
  int carry = 0;
  for (int base = 0; base < nb; base += SCAN_THREADS) {
    int i = base + threadIdx.x;
    int v = i < nb ? sums[i] : 0;
    int tot;
    int ex = block_exclusive_scan(v, lds, &tot);
    if (i < nb) sums[i] = carry + ex;
    carry += tot;
  }
}

// third pass of the 3-pass form (kept for reference sizes beyond SCAN_FUSED_MAX_BLOCKS tiles)
__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_apply(const int32_t* __restrict__ in, int64_t n, const int32_t* __restrict__ sums,
             int32_t* __restrict__ out) {
  __shared__ int lds[4];
  int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  int v[SCAN_ITEMS];
  int s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    v[k] = base + k < n ? in[base + k] : 0;
    s += v[k];
  }
  int tot;
  int ex = block_exclusive_scan(s, lds, &tot) + sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    if (base + k < n) out[base + k] = ex;
    ex += v[k];
  }
}

// two-pass form: every block of the apply pass adds up the totals of the tiles before it (nb <= a few thousand ints, L2-resident)
// instead of waiting for a one-block scan of the totals -- one launch and one dependent round trip less
constexpr int SCAN_FUSED_MAX_BLOCKS = 4096;
__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_apply_fused(const int32_t* __restrict__ in, int64_t n, const int32_t* __restrict__ tile_sums,
                   int32_t* __restrict__ out) {
  __shared__ int lds[4];
  int carry_part = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += SCAN_THREADS) carry_part += tile_sums[i];
  int carry;
  block_exclusive_scan(carry_part, lds, &carry);
  int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
  int v[SCAN_ITEMS];
  int s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    v[k] = base + k < n ? in[base + k] : 0;
    s += v[k];
  }
  int tot;
  int ex = block_exclusive_scan(s, lds, &tot) + carry;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    if (base + k < n) out[base + k] = ex;
    ex += v[k];
  }
}

static size_t scan_ws_bytes(int64_t n) { return pw_align_up((size_t)pw_cdiv(n, SCAN_TILE) * 4, 256); }
static int scan_exclusive_i32(const int32_t* in, int32_t* out, int64_t n, int32_t* sums, hipStream_t st);
// library-internal (pw_common.h): the same scan for other translation units (pw_render.hip's sorted backward)
size_t pw_scan_ws_bytes(int64_t n) { return scan_ws_bytes(n); }
int pw_scan_exclusive_i32(const int32_t* in, int32_t* out, int64_t n, int32_t* sums, hipStream_t st) {
  return scan_exclusive_i32(in, out, n, sums, st);
}

// out may alias in
static int scan_exclusive_i32(const int32_t* in, int32_t* out, int64_t n, int32_t* sums,
                              hipStream_t st) {
  int nb = (int)pw_cdiv(n, SCAN_TILE);
  hipLaunchKernelGGL(k_scan_reduce, dim3(nb), dim3(SCAN_THREADS), 0, st, in, n, sums);
  if (nb <= SCAN_FUSED_MAX_BLOCKS) {
    hipLaunchKernelGGL(k_scan_apply_fused, dim3(nb), dim3(SCAN_THREADS), 0, st, in, n, sums, out);
  } else {
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_THREADS), 0, st, sums, nb);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(SCAN_THREADS), 0, st, in, n, sums, out);
  }
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// ------------------------------------------------------------------------------------
// stable segmented (counting) sort
// ------------------------------------------------------------------------------------
// histogram with RETURNING atomics: the old counter value is this point's arrival rank inside
// its segment, so the scatter below needs no second round of atomics.
// Device-scope atomics execute below the per-XCD L2 on this part and sustain only ~19 G ops/s
// (measured: 0.88 M distinct-address atomics = 59 us, and hot addresses serialise on top), so the
// kernel is bound by how many it issues.  Consecutive lanes are consecutive pixels of one depth
// bin and therefore fall into the same voxel in runs (hundreds of lanes near the camera, ~2 at
// mid range, 1 far away): each run of equal keys inside a wave is served by ONE atomicAdd of the
// run length issued by its first lane; the other lanes take base + offset in the run.
__global__ void __launch_bounds__(256)
k_hist(const int32_t* __restrict__ keys, int64_t n, int32_t* __restrict__ count,
       int32_t* __restrict__ rank, int32_t* __restrict__ n_long) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n_long && i == 0) *n_long = 0;                 // consumed by k_scatter, two launches later
  const int lane = threadIdx.x & 63;
  const int k = i < n ? keys[i] : -1;
  const int kprev = __shfl_up(k, 1, 64);
  const unsigned long long heads = __ballot(lane == 0 || k != kprev);
  const unsigned long long upto = heads & (~0ull >> (63 - lane));           // heads at lanes <= mine
  const int start = 63 - __builtin_clzll(upto);
  const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
  const int end = above ? __builtin_ctzll(above) : 64;
  int base = 0;
  if (k >= 0 && lane == start) base = atomicAdd(&count[k], end - start);
  base = __shfl(base, start, 64);
  if (k >= 0) rank[i] = base + lane - start;
}

// scatter by (segment start + arrival rank); the first arrival of a long segment registers it
__global__ void __launch_bounds__(256)
k_scatter(const int32_t* __restrict__ keys, int64_t n, const int32_t* __restrict__ seg_start,
          const int32_t* __restrict__ rank, int32_t* __restrict__ tmp, int long_threshold,
          int32_t* __restrict__ long_list, int32_t* __restrict__ n_long) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int k = keys[i];
  if (k < 0) return;
  const int s = seg_start[k], r = rank[i];
  tmp[s + r] = (int32_t)i;
  if (long_list && r == 0 && seg_start[k + 1] - s > long_threshold) long_list[atomicAdd(n_long, 1)] = k;
}

// in-segment rank sort: the scatter order inside a segment is whatever the atomics gave;
// ids are distinct, so final position = number of smaller ids in the segment.  One thread per
// point for segments up to SORT_LONG entries (<= SORT_LONG loop trips); longer segments are
// sorted by whole blocks through LDS (k_sort_long).
// Optional by-product: order_aux[pos] = (id / aux_div) * aux_mod + id % aux_mod (LSS: the
// feat-pixel index, view_transformer.py:219-224, so pooling does no integer division).
constexpr int SORT_LONG = 64;
constexpr int SORT_LDS_MAX = 4096;          // ids per LDS pass of k_sort_long (16 KB)

__device__ __forceinline__ void emit_sorted(int32_t* order, int32_t* order_aux, int pos, int id,
                                            int aux_div, int aux_mod) {
  order[pos] = id;
  if (order_aux) order_aux[pos] = (id / aux_div) * aux_mod + id % aux_mod;
}

__global__ void __launch_bounds__(256)
k_ranksort(const int32_t* __restrict__ keys, const int32_t* __restrict__ seg_start,
           const int32_t* __restrict__ tmp, const int32_t* __restrict__ kept_ptr,
           int32_t* __restrict__ order, int aux_div, int aux_mod, int32_t* __restrict__ order_aux,
           int long_sorted_elsewhere) {
  int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= *kept_ptr) return;
  int id = tmp[pos];
  int k = keys[id];
  int s = seg_start[k], e = seg_start[k + 1];
  if (long_sorted_elsewhere && e - s > SORT_LONG) return;
  int r = 0;
  for (int j = s; j < e; ++j) r += tmp[j] < id;
  emit_sorted(order, order_aux, s + r, id, aux_div, aux_mod);
}

// long segments: one block per segment, ids staged in LDS, rank = #smaller ids (LDS broadcast
// reads, no global traffic in the O(n^2) part).  Segments beyond SORT_LDS_MAX ids are processed
// in LDS-sized passes (rank accumulates over passes).
__device__ __forceinline__ void sort_long_blocks(const int32_t* __restrict__ seg_start, const int32_t* __restrict__ tmp,
                                                 const int32_t* __restrict__ long_list, const int32_t* __restrict__ n_long,
                                                 int32_t* __restrict__ order, int aux_div, int aux_mod,
                                                 int32_t* __restrict__ order_aux, int32_t* ids, int first, int stride) {
  const int nl = *n_long;
  for (int li = first; li < nl; li += stride) {
    const int k = long_list[li];
    const int s = seg_start[k], n = seg_start[k + 1] - s;
    if (n <= SORT_LDS_MAX) {                              // the segment fits: stage once
      const int m16 = (n + 15) & ~15;                     // padded with INT_MAX: never "smaller"
      for (int j = threadIdx.x; j < m16; j += blockDim.x) ids[j] = j < n ? tmp[s + j] : 0x7fffffff;
      __syncthreads();
      for (int t = threadIdx.x; t < n; t += blockDim.x) {
        const int id = ids[t];
        emit_sorted(order, order_aux, s + count_smaller_lds(ids, m16, id), id, aux_div, aux_mod);
      }
    } else {
      for (int t0 = 0; t0 < n; t0 += blockDim.x) {        // elements owned by this block's threads
        const int t = t0 + threadIdx.x;
        const int id = t < n ? tmp[s + t] : 0;
        int r = 0;
        for (int p0 = 0; p0 < n; p0 += SORT_LDS_MAX) {    // LDS passes over the segment
          const int m = min(SORT_LDS_MAX, n - p0);
          const int m16 = (m + 15) & ~15;
          __syncthreads();
          for (int j = threadIdx.x; j < m16; j += blockDim.x) ids[j] = j < m ? tmp[s + p0 + j] : 0x7fffffff;
          __syncthreads();
          if (t < n) r += count_smaller_lds(ids, m16, id);
        }
        if (t < n) emit_sorted(order, order_aux, s + r, id, aux_div, aux_mod);
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256)
k_sort_long(const int32_t* __restrict__ seg_start, const int32_t* __restrict__ tmp,
            const int32_t* __restrict__ long_list, const int32_t* __restrict__ n_long,
            int32_t* __restrict__ order, int aux_div, int aux_mod, int32_t* __restrict__ order_aux) {
  extern __shared__ __attribute__((aligned(16))) int32_t ids[];
  sort_long_blocks(seg_start, tmp, long_list, n_long, order, aux_div, aux_mod, order_aux, ids, (int)blockIdx.x, (int)gridDim.x);
}

// k_ranksort and k_sort_long in ONE launch (they are independent: short segments by one thread per point, long ones by the first
// SORT_LONG_BLOCKS blocks through LDS): one launch and one drain / fill of the GPU less per frame
constexpr int SORT_LONG_BLOCKS = 512;
__global__ void __launch_bounds__(256)
k_ranksort_all(const int32_t* __restrict__ keys, const int32_t* __restrict__ seg_start, const int32_t* __restrict__ tmp,
               const int32_t* __restrict__ kept_ptr, const int32_t* __restrict__ long_list,
               const int32_t* __restrict__ n_long, int32_t* __restrict__ order, int aux_div, int aux_mod,
               int32_t* __restrict__ order_aux) {
  extern __shared__ __attribute__((aligned(16))) int32_t ids[];
  if ((int)blockIdx.x < SORT_LONG_BLOCKS) {
    sort_long_blocks(seg_start, tmp, long_list, n_long, order, aux_div, aux_mod, order_aux, ids, (int)blockIdx.x, SORT_LONG_BLOCKS);
    return;
  }
  const int64_t pos = (int64_t)(blockIdx.x - SORT_LONG_BLOCKS) * blockDim.x + threadIdx.x;
  if (pos >= *kept_ptr) return;
  const int id = tmp[pos];
  const int k = keys[id];
  const int s = seg_start[k], e = seg_start[k + 1];
  if (e - s > SORT_LONG) return;
  int r = 0;
  for (int j = s; j < e; ++j) r += tmp[j] < id;
  emit_sorted(order, order_aux, s + r, id, aux_div, aux_mod);
}

// zero-fill by a kernel, not hipMemsetAsync: a hipGraph that contains memset nodes faulted on replay
// ("write access to a read-only page") as soon as the process had allocated new device memory after
// the capture (ROCm 7.2; reproduced with this function alone, gone with the kernel)
__global__ void __launch_bounds__(256) k_zero_i32(int32_t* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

PW_API size_t pw_segment_sort_workspace_bytes(int64_t n, int64_t n_keys) {
  return pw_align_up((size_t)(n_keys + 1) * 4, 256)   // count
         + pw_align_up((size_t)n * 4, 256)            // arrival rank per point
         + pw_align_up((size_t)n * 4, 256)            // tmp
         + scan_ws_bytes(n_keys + 1);
}

PW_API int pw_segment_sort(int64_t n, int64_t n_keys, const int32_t* keys, void* workspace,
                           size_t workspace_bytes, int32_t* seg_start, int32_t* order, int aux_div,
                           int aux_mod, int32_t* order_aux, int long_threshold, int32_t* long_list,
                           int32_t* n_long, void* stream) {
  PW_CHECK_ARG(n > 0 && n_keys > 0 && keys && workspace && seg_start && order,
               "pw_segment_sort: bad arguments");
  PW_CHECK_ARG(n < ((int64_t)1 << 31) && n_keys < ((int64_t)1 << 31) - 1,
               "pw_segment_sort: sizes must fit int32");
  if (workspace_bytes < pw_segment_sort_workspace_bytes(n, n_keys)) {
    pw_set_error("pw_segment_sort: workspace too small (%zu < %zu)", workspace_bytes,
                 pw_segment_sort_workspace_bytes(n, n_keys));
    return PW_ENOSPC;
  }
  PW_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "pw_segment_sort: workspace must be 256-B aligned");
  PW_CHECK_ARG(!order_aux || (aux_div > 0 && aux_mod > 0), "pw_segment_sort: aux_div/aux_mod must be > 0");
  PW_CHECK_ARG(!long_list || (n_long && long_threshold > 0), "pw_segment_sort: long_list needs n_long and a threshold");
  hipStream_t st = pw_stream(stream);
  char* ws = (char*)workspace;
  int32_t* count = (int32_t*)ws;
  ws += pw_align_up((size_t)(n_keys + 1) * 4, 256);
  int32_t* rank = (int32_t*)ws;
  ws += pw_align_up((size_t)n * 4, 256);
  int32_t* tmp = (int32_t*)ws;
  ws += pw_align_up((size_t)n * 4, 256);
  int32_t* sums = (int32_t*)ws;
  hipLaunchKernelGGL(k_zero_i32, dim3((unsigned)pw_cdiv(n_keys + 1, 256)), dim3(256), 0, st, count, n_keys + 1);
  unsigned nbk = (unsigned)pw_cdiv(n, 256);
  hipLaunchKernelGGL(k_hist, dim3(nbk), dim3(256), 0, st, keys, n, count, rank, long_list ? n_long : (int32_t*)nullptr);
  int rc = scan_exclusive_i32(count, seg_start, n_keys + 1, sums, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_scatter, dim3(nbk), dim3(256), 0, st, keys, n, seg_start, rank, tmp,
                     long_threshold, long_list, n_long);
  // with a long list (threshold must be SORT_LONG) the long segments go to the LDS block sort
  const int split = (long_list && long_threshold == SORT_LONG) ? 1 : 0;
  if (split) {
    hipLaunchKernelGGL(k_ranksort_all, dim3(nbk + SORT_LONG_BLOCKS), dim3(256), SORT_LDS_MAX * 4, st, keys, seg_start, tmp,
                       seg_start + n_keys, long_list, n_long, order, aux_div, aux_mod, order_aux);
  } else {
    hipLaunchKernelGGL(k_ranksort, dim3(nbk), dim3(256), 0, st, keys, seg_start, tmp,
                       seg_start + n_keys, order, aux_div, aux_mod, order_aux, split);
  }
  pw_note_kernel("k_zero + k_hist + 2 scan + k_scatter + k_ranksort_all");
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// ------------------------------------------------------------------------------------
// expand to the reference's five rank tensors
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_nonempty_flags(const int32_t* __restrict__ seg_start, int64_t n_voxels, int32_t* __restrict__ flag) {
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v > n_voxels) return;
  flag[v] = v < n_voxels ? (seg_start[v + 1] > seg_start[v]) : 0;
}

__global__ void __launch_bounds__(256)
k_expand_ranks(const int32_t* __restrict__ seg_start, const int32_t* __restrict__ order,
               const int32_t* __restrict__ iv_index, int64_t n_voxels, int DHW, int HW,
               int32_t* __restrict__ ranks_bev, int32_t* __restrict__ ranks_depth,
               int32_t* __restrict__ ranks_feat, int32_t* __restrict__ interval_starts,
               int32_t* __restrict__ interval_lengths, int32_t* __restrict__ counts) {
  int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v == 0) {
    counts[0] = seg_start[n_voxels];
    counts[1] = iv_index[n_voxels];
  }
  if (v >= n_voxels) return;
  int s = seg_start[v], e = seg_start[v + 1];
  if (e == s) return;
  int iv = iv_index[v];
  interval_starts[iv] = s;
  interval_lengths[iv] = e - s;
  for (int pos = s; pos < e; ++pos) {
    int id = order[pos];
    ranks_bev[pos] = (int32_t)v;
    ranks_depth[pos] = id;
    ranks_feat[pos] = (id / DHW) * HW + id % HW;
  }
}

PW_API size_t pw_lss_ranks_workspace_bytes(int64_t n_voxels) {
  return pw_align_up((size_t)(n_voxels + 1) * 4, 256) + scan_ws_bytes(n_voxels + 1);
}

PW_API int pw_lss_ranks(int64_t n_voxels, const int32_t* seg_start, const int32_t* order, int D,
                        int HW, void* workspace, size_t workspace_bytes, int32_t* ranks_bev,
                        int32_t* ranks_depth, int32_t* ranks_feat, int32_t* interval_starts,
                        int32_t* interval_lengths, int32_t* counts, void* stream) {
  PW_CHECK_ARG(n_voxels > 0 && seg_start && order && workspace && ranks_bev && ranks_depth &&
                   ranks_feat && interval_starts && interval_lengths && counts && D > 0 && HW > 0,
               "pw_lss_ranks: bad arguments");
  if (workspace_bytes < pw_lss_ranks_workspace_bytes(n_voxels)) {
    pw_set_error("pw_lss_ranks: workspace too small");
    return PW_ENOSPC;
  }
  hipStream_t st = pw_stream(stream);
  int32_t* flag = (int32_t*)workspace;
  int32_t* sums = (int32_t*)((char*)workspace + pw_align_up((size_t)(n_voxels + 1) * 4, 256));
  unsigned nb = (unsigned)pw_cdiv(n_voxels + 1, 256);
  hipLaunchKernelGGL(k_nonempty_flags, dim3(nb), dim3(256), 0, st, seg_start, n_voxels, flag);
  int rc = scan_exclusive_i32(flag, flag, n_voxels + 1, sums, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_expand_ranks, dim3(nb), dim3(256), 0, st, seg_start, order, flag, n_voxels,
                     D * HW, HW, ranks_bev, ranks_depth, ranks_feat, interval_starts,
                     interval_lengths, counts);
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// ------------------------------------------------------------------------------------
// pooling kernels.  LPV = lanes per voxel = C/4 (float4 per lane); a wave owns 64/LPV voxels.
// Sequential fp32 accumulation in point order, mul and add NOT contracted: the summation ORDER is that of
// bev_pool_cuda.cu:37-41 and the result is bit-identical to the CPU checker of the test suite (also built without FMA contraction).
// Whether it is bit-identical to the reference's CUDA build depends on nvcc's own contraction choice there, which nothing here pins.
// ------------------------------------------------------------------------------------
constexpr int POOL_UNROLL = 8;

// dense, voxel-driven: writes every voxel row once.  order_feat[pos] is the feat-pixel index
// of sorted point pos.  Segments longer than long_threshold (a few hundred near-camera voxels
// hold up to ~1300 points) are taken by whole waves in the first LONG_BLOCKS blocks, which
// start first and run under the bulk sweep: 64 (pixel, depth) pairs are fetched in one
// coalesced go, then broadcast lane by lane so the sum keeps its sequential point order.
constexpr int LONG_BLOCKS = 128;    // x 4 waves
#ifndef PW_POOL_WAVES
#define PW_POOL_WAVES 5
#endif

template <int LPV>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PW_POOL_WAVES, 8)))
k_pool_dense(const float* __restrict__ depth, const float4* __restrict__ feat,
             const int32_t* __restrict__ seg_start, const int32_t* __restrict__ order,
             const int32_t* __restrict__ order_feat, int64_t n_voxels, int long_threshold,
             const int32_t* __restrict__ long_list, const int32_t* __restrict__ n_long,
             float4* __restrict__ out, int out_h2, int* __restrict__ out_rng) {
  const int lane = threadIdx.x & 63;
  const int sub = lane % LPV;
  const int e_out = out_h2 ? rng_exp(out_rng) : 0;
  const float omul = rng_pow2(-e_out);
  unsigned amax = 0u;
  const int long_blocks = long_list ? LONG_BLOCKS : 0;
  if ((int)blockIdx.x < long_blocks) {
    // Long segments: one wave per segment, 64 points per batch.  Lane L owns point base+L (its
    // pixel index and depth); lane group g gathers the feature rows of points u*8+g (u = 0..7,
    // 8 different rows per load instruction, 64 rows in flight), then every lane walks the 64
    // points IN ORDER, pulling its 4 channels of point p from lane (p%8)*8+sub with a ds_bpermute:
    // the data movement is parallel, the sum order stays the oracle's.
    const int nl = *n_long;
    const int grp = lane / LPV;
    constexpr int GROUPS = 64 / LPV;
    constexpr int NU = LPV < 16 ? LPV : 16;             // gathers in flight per lane
    constexpr int PB = NU * GROUPS;                     // points per batch (64 for LPV <= 16)
    for (int li = blockIdx.x * 4 + (threadIdx.x >> 6); li < nl; li += LONG_BLOCKS * 4) {
      const int64_t v = long_list[li];
      const int s = seg_start[v], e = seg_start[v + 1];
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      int idx = s + min(lane, e - s - 1);
      int my_pf = order_feat[idx];
      float my_d = depth[order[idx]];
      for (int base = s; base < e; base += PB) {
        const int n = min(PB, e - base);
        float4 f[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const int q = u * GROUPS + grp;
          const int pf = __shfl(my_pf, q, 64);
          f[u] = q < n ? feat[(int64_t)pf * LPV + sub] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float cur_d = my_d;
        if (base + PB < e) {                               // next batch's ids while this one sums
          idx = base + PB + min(lane, e - base - PB - 1);
          my_pf = order_feat[idx];
          my_d = depth[order[idx]];
        }
        {
#pragma unroll
          for (int u = 0; u < NU; ++u) {
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) {
              const int pidx = u * GROUPS + g;                // compile-time
              if (pidx < n) {                                // wave-uniform
                const int src = g * LPV + sub;
                float4 fv;
                fv.x = __shfl(f[u].x, src, 64);
                fv.y = __shfl(f[u].y, src, 64);
                fv.z = __shfl(f[u].z, src, 64);
                fv.w = __shfl(f[u].w, src, 64);
                const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur_d), pidx));
                fma4_nc(acc, fv, d);
              }
            }
          }
        }
      }
      if (lane < LPV) pool_store<LPV>(out, v, sub, acc, out_h2, omul, amax);     // every lane group holds the same sums
    }
    if (out_h2) rng_note(out_rng, amax, e_out);
    return;
  }
  // Dense sweep, software-pipelined over the voxels of one lane group.  A voxel costs a chain of
  // dependent loads (segment bounds -> point ids -> depth / feature row); run back to back that
  // chain (~3 memory latencies) times ~10 voxels per group was the whole kernel time.  Here the
  // bounds and the first LPV point ids of later voxels are requested while voxel v gathers (see
  // the pipeline note below), so one memory latency per voxel stays exposed.  Lane `sub` holds the (pixel, point id) pair of
  // point s+sub (one coalesced load per array per group instead of LPV clamped ones); pairs are
  // broadcast inside the lane group and only points that exist gather their feature row.
  // The sum order is still point order, one non-contracted multiply-add at a time (bit-exact).
  const int64_t gid = (int64_t)(blockIdx.x - long_blocks) * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)(gridDim.x - long_blocks) * blockDim.x / LPV;
  const int gbase = lane - sub;                     // first lane of this voxel's lane group
  // three-stage pipeline over the group's voxels v, v + stride, v + 2 stride: bounds are requested TWO voxels ahead, point ids ONE
  // voxel ahead (their bounds arrived an iteration ago), so an iteration exposes one memory latency (its gathers) instead of two
  // (bounds -> ids were back to back inside the iteration before)
  int64_t v = gid / LPV;
  int s = 0, e = 0, my_pf = 0, my_o = 0, sn = 0, en = 0;
  if (v < n_voxels) {
    s = seg_start[v];
    e = seg_start[v + 1];
    if (e > s) {
      const int j = min(s + sub, e - 1);
      my_pf = order_feat[j];
      my_o = order[j];
    }
    if (v + stride < n_voxels) { sn = seg_start[v + stride]; en = seg_start[v + stride + 1]; }
  }
  while (v < n_voxels) {
    const int64_t vn = v + stride, v2 = vn + stride;
    int s2 = 0, e2 = 0;
    if (v2 < n_voxels) { s2 = seg_start[v2]; e2 = seg_start[v2 + 1]; }
    int n_pf = 0, n_o = 0;
    if (en > sn) {
      const int j = min(sn + sub, en - 1);
      n_pf = order_feat[j];
      n_o = order[j];
    }
    const bool skip = long_list && e - s > long_threshold;   // summed by the long-segment blocks
    const int cnt = skip ? 0 : min(LPV, e - s);
    const float my_d = cnt > 0 ? depth[my_o] : 0.f;
    // most voxels hold 0-3 points: stop the unrolled per-point work at the largest count among the wave's voxels
    // (wave-uniform test; skipped iterations would only have shuffled and predicated-off)
    float4 f[LPV];
#pragma unroll
    for (int u = 0; u < LPV; ++u) f[u] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < LPV; ++u) {
      if (__ballot(u < cnt) == 0ull) break;
      const int pf = __shfl(my_pf, gbase + u, 64);
      if (u < cnt) f[u] = feat[(int64_t)pf * LPV + sub];
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < LPV; ++u) {
      if (__ballot(u < cnt) == 0ull) break;
      const float d = __shfl(my_d, gbase + u, 64);
      if (u < cnt) fma4_nc(acc, f[u], d);
    }
    if (!skip) {
      for (int i = s + LPV; i < e; i += LPV) {             // points LPV.. of a medium segment
        const int j = min(i + sub, e - 1);
        const int r_pf = order_feat[j];
        const float r_d = depth[order[j]];
        const int rc = min(LPV, e - i);
#pragma unroll
        for (int u = 0; u < LPV; ++u) {
          const int pf = __shfl(r_pf, gbase + u, 64);
          const float d = __shfl(r_d, gbase + u, 64);
          if (u < rc) fma4_nc(acc, feat[(int64_t)pf * LPV + sub], d);
        }
      }
      pool_store<LPV>(out, v, sub, acc, out_h2, omul, amax);
    }
    v = vn; s = sn; e = en; my_pf = n_pf; my_o = n_o; sn = s2; en = e2;
  }
  if (out_h2) rng_note(out_rng, amax, e_out);
}

// interval-driven (reference ABI): out pre-zeroed by the caller, assign per interval
template <int LPV>
__global__ void __launch_bounds__(256)
k_pool_intervals(const float* __restrict__ depth, const float4* __restrict__ feat,
                 const int32_t* __restrict__ ranks_depth, const int32_t* __restrict__ ranks_feat,
                 const int32_t* __restrict__ ranks_bev, const int32_t* __restrict__ istart,
                 const int32_t* __restrict__ ilen, int n_intervals, float4* __restrict__ out) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int sub = (int)(gid % LPV);
  const int64_t iv = gid / LPV;
  if (iv >= n_intervals) return;
  const int s = istart[iv], e = s + ilen[iv];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = s; i < e; i += POOL_UNROLL) {
    float d[POOL_UNROLL];
    float4 f[POOL_UNROLL];
#pragma unroll
    for (int u = 0; u < POOL_UNROLL; ++u) {
      int j = min(i + u, e - 1);
      d[u] = depth[ranks_depth[j]];
      f[u] = feat[(int64_t)ranks_feat[j] * LPV + sub];
    }
#pragma unroll
    for (int u = 0; u < POOL_UNROLL; ++u)
      if (i + u < e) fma4_nc(acc, f[u], d[u]);
  }
  out[(int64_t)ranks_bev[s] * LPV + sub] = acc;
}

// any channel count: one thread per (interval, channel) -- bev_pool_cuda.cu:21-48 shape
__global__ void __launch_bounds__(256)
k_pool_intervals_generic(int c, int n_intervals, const float* __restrict__ depth,
                         const float* __restrict__ feat, const int32_t* __restrict__ ranks_depth,
                         const int32_t* __restrict__ ranks_feat,
                         const int32_t* __restrict__ ranks_bev, const int32_t* __restrict__ istart,
                         const int32_t* __restrict__ ilen, float* __restrict__ out) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t iv = idx / c;
  int ch = (int)(idx % c);
  if (iv >= n_intervals) return;
  int s = istart[iv], len = ilen[iv];
  float psum = 0.f;
  for (int i = 0; i < len; ++i)
    psum = psum + feat[(int64_t)ranks_feat[s + i] * c + ch] * depth[ranks_depth[s + i]];
  out[(int64_t)ranks_bev[s] * c + ch] = psum;
}

__global__ void __launch_bounds__(256)
k_pool_dense_generic(int c, const float* __restrict__ depth, const float* __restrict__ feat,
                     const int32_t* __restrict__ seg_start, const int32_t* __restrict__ order,
                     const int32_t* __restrict__ order_feat, int64_t n_voxels,
                     float* __restrict__ out) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t v = idx / c;
  int ch = (int)(idx % c);
  if (v >= n_voxels) return;
  int s = seg_start[v], e = seg_start[v + 1];
  float psum = 0.f;
  for (int i = s; i < e; ++i)
    psum = psum + feat[(int64_t)order_feat[i] * c + ch] * depth[order[i]];
  out[v * c + ch] = psum;
}

static bool lpv_supported(int c) {
  if (c % 4) return false;
  int l = c / 4;
  return l == 1 || l == 2 || l == 4 || l == 8 || l == 16 || l == 32 || l == 64;
}

#define PW_DISPATCH_LPV(lpv, CALL)                                      \
  switch (lpv) {                                                        \
    case 1: { constexpr int L = 1; CALL; } break;                       \
    case 2: { constexpr int L = 2; CALL; } break;                       \
    case 4: { constexpr int L = 4; CALL; } break;                       \
    case 8: { constexpr int L = 8; CALL; } break;                       \
    case 16: { constexpr int L = 16; CALL; } break;                     \
    case 32: { constexpr int L = 32; CALL; } break;                     \
    default: { constexpr int L = 64; CALL; } break;                     \
  }

PW_API int pw_bev_pool_dense(const float* depth, const float* feat, const int32_t* seg_start,
                             const int32_t* order, const int32_t* order_feat, int64_t n_voxels,
                             int c, int long_threshold, const int32_t* long_list,
                             const int32_t* n_long, float* out, int out_h2, int32_t* out_rng, void* stream) {
  PW_CHECK_ARG(depth && feat && seg_start && order && order_feat && out && n_voxels > 0 && c > 0,
               "pw_bev_pool_dense: bad arguments");
  PW_CHECK_ARG(!out_h2 || (c % 32 == 0 && lpv_supported(c)), "pw_bev_pool_dense: h2 output needs C %% 32 == 0");
  PW_CHECK_ARG(!long_list || (n_long && long_threshold > 0), "pw_bev_pool_dense: long_list needs n_long");
  hipStream_t st = pw_stream(stream);
  if (lpv_supported(c) && ((uintptr_t)feat & 15) == 0 && ((uintptr_t)out & 15) == 0) {
    int lpv = c / 4;
    // memory-bound: cap the grid at ~8 blocks/CU x 256 CUs and grid-stride
    int64_t want = pw_cdiv(n_voxels * lpv, 256);
    const int cap = 2048;
    unsigned nb = (unsigned)(want < cap ? want : cap) + (long_list ? LONG_BLOCKS : 0);
    PW_DISPATCH_LPV(lpv, hipLaunchKernelGGL((k_pool_dense<L>), dim3(nb), dim3(256), 0, st, depth,
                                            (const float4*)feat, seg_start, order, order_feat,
                                            n_voxels, long_threshold, long_list, n_long,
                                            (float4*)out, out_h2, out_rng));
    pw_note_kernel("k_pool_dense<%d>", lpv);
  } else {
    PW_CHECK_ARG(!out_h2, "pw_bev_pool_dense: h2 output needs 16-byte aligned feat / out (the generic kernel writes fp32)");
    hipLaunchKernelGGL(k_pool_dense_generic, dim3((unsigned)pw_cdiv(n_voxels * c, 256)), dim3(256),
                       0, st, c, depth, feat, seg_start, order, order_feat, n_voxels, out);
    pw_note_kernel("k_pool_dense_generic");
  }
  PW_CHECK_LAUNCH();
  return PW_OK;
}

PW_API int pw_bev_pool_v2_forward(const float* depth, const float* feat, float* out,
                                  const int32_t* ranks_depth, const int32_t* ranks_feat,
                                  const int32_t* ranks_bev, const int32_t* interval_lengths,
                                  const int32_t* interval_starts, int c, int n_intervals,
                                  void* stream) {
  PW_CHECK_ARG(c > 0 && n_intervals >= 0, "pw_bev_pool_v2_forward: bad sizes");
  if (n_intervals == 0) return PW_OK;
  PW_CHECK_ARG(depth && feat && out && ranks_depth && ranks_feat && ranks_bev && interval_lengths &&
                   interval_starts,
               "pw_bev_pool_v2_forward: null pointer");
  hipStream_t st = pw_stream(stream);
  if (lpv_supported(c) && ((uintptr_t)feat & 15) == 0 && ((uintptr_t)out & 15) == 0) {
    int lpv = c / 4;
    unsigned nb = (unsigned)pw_cdiv((int64_t)n_intervals * lpv, 256);
    PW_DISPATCH_LPV(lpv, hipLaunchKernelGGL((k_pool_intervals<L>), dim3(nb), dim3(256), 0, st, depth,
                                            (const float4*)feat, ranks_depth, ranks_feat, ranks_bev,
                                            interval_starts, interval_lengths, n_intervals,
                                            (float4*)out));
  } else {
    hipLaunchKernelGGL(k_pool_intervals_generic,
                       dim3((unsigned)pw_cdiv((int64_t)n_intervals * c, 256)), dim3(256), 0, st, c,
                       n_intervals, depth, feat, ranks_depth, ranks_feat, ranks_bev,
                       interval_starts, interval_lengths, out);
  }
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// ------------------------------------------------------------------------------------
// backward (bev_pool_cuda.cu:67-121): intervals are per feat pixel
// ------------------------------------------------------------------------------------
template <int LPV>
__global__ void __launch_bounds__(256)
k_pool_bwd(const float4* __restrict__ out_grad, const float* __restrict__ depth,
           const float4* __restrict__ feat, const int32_t* __restrict__ ranks_depth,
           const int32_t* __restrict__ ranks_feat, const int32_t* __restrict__ ranks_bev,
           const int32_t* __restrict__ istart, const int32_t* __restrict__ ilen, int n_intervals,
           float* __restrict__ depth_grad, float4* __restrict__ feat_grad) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int sub = (int)(gid % LPV);
  const int64_t iv = gid / LPV;
  const bool active = iv < n_intervals;       // keep whole groups alive for the shuffles
  int s = 0, e = 0;
  if (active) { s = istart[iv]; e = s + ilen[iv]; }
  const int64_t pf = active ? ranks_feat[s] : 0;
  const float4 f = active ? feat[pf * LPV + sub] : make_float4(0, 0, 0, 0);
  float4 fg = make_float4(0.f, 0.f, 0.f, 0.f);
  // all lanes of a wave iterate to the wave-wide max length so shuffles stay convergent
  int len = e - s, maxlen = len;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, off, 64));
  for (int k = 0; k < maxlen; ++k) {
    const bool on = k < len;
    const int i = on ? s + k : max(e - 1, 0);
    float4 og = make_float4(0, 0, 0, 0);
    float d = 0.f;
    int rd = 0;
    if (on) {
      og = out_grad[(int64_t)ranks_bev[i] * LPV + sub];
      rd = ranks_depth[i];
      d = depth[rd];
    }
    float dot = ((og.x * f.x + og.y * f.y) + og.z * f.z) + og.w * f.w;
#pragma unroll
    for (int off = 1; off < LPV; off <<= 1) dot += __shfl_xor(dot, off, 64);
    if (on && sub == 0) depth_grad[rd] = dot;
    if (on) fma4_nc(fg, og, d);
  }
  if (active) feat_grad[pf * LPV + sub] = fg;
}

// tree_lpv > 0: a width k_pool_bwd<tree_lpv> serves, reached only because a pointer is not 16-byte aligned.  The dot product is
// then summed in that kernel's order -- four channels per lane, then the __shfl_xor butterfly, i.e. a balanced pairwise tree over
// the tree_lpv partial sums (built here with a binary-counter stack) -- so the result does not depend on where a buffer starts.
__global__ void __launch_bounds__(256)
k_pool_bwd_generic(int c, int tree_lpv, int n_intervals, const float* __restrict__ out_grad,
                   const float* __restrict__ depth, const float* __restrict__ feat,
                   const int32_t* __restrict__ ranks_depth, const int32_t* __restrict__ ranks_feat,
                   const int32_t* __restrict__ ranks_bev, const int32_t* __restrict__ istart,
                   const int32_t* __restrict__ ilen, float* __restrict__ depth_grad,
                   float* __restrict__ feat_grad) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_intervals) return;
  int s = istart[idx], len = ilen[idx];
  for (int i = 0; i < len; ++i) {
    const float* og = out_grad + (int64_t)ranks_bev[s + i] * c;
    const float* f = feat + (int64_t)ranks_feat[s + i] * c;
    float g = 0.f;
    if (tree_lpv > 0) {
      float stack[7];                                        // tree_lpv <= 64: at most 6 pending subtrees + the new leaf
      int top = 0;
      for (int j = 0; j < tree_lpv; ++j) {
        const float* a = og + 4 * j;
        const float* b = f + 4 * j;
        float p = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3];
        for (int bit = j; bit & 1; bit >>= 1) p = stack[--top] + p;
        stack[top++] = p;
      }
      g = stack[0];
    } else {
      for (int ch = 0; ch < c; ++ch) g = g + og[ch] * f[ch];
    }
    depth_grad[ranks_depth[s + i]] = g;
  }
  float* fg = feat_grad + (int64_t)ranks_feat[s] * c;
  for (int ch = 0; ch < c; ++ch) {
    float g = 0.f;
    for (int i = 0; i < len; ++i)
      g = g + out_grad[(int64_t)ranks_bev[s + i] * c + ch] * depth[ranks_depth[s + i]];
    fg[ch] = g;
  }
}

PW_API int pw_bev_pool_v2_backward(const float* out_grad, float* depth_grad, float* feat_grad,
                                   const float* depth, const float* feat,
                                   const int32_t* ranks_depth, const int32_t* ranks_feat,
                                   const int32_t* ranks_bev, const int32_t* interval_lengths,
                                   const int32_t* interval_starts, int c, int n_intervals,
                                   void* stream) {
  PW_CHECK_ARG(c > 0 && n_intervals >= 0, "pw_bev_pool_v2_backward: bad sizes");
  if (n_intervals == 0) return PW_OK;
  PW_CHECK_ARG(out_grad && depth_grad && feat_grad && depth && feat && ranks_depth && ranks_feat &&
                   ranks_bev && interval_lengths && interval_starts,
               "pw_bev_pool_v2_backward: null pointer");
  hipStream_t st = pw_stream(stream);
  if (lpv_supported(c) && c <= 256 && ((uintptr_t)feat & 15) == 0 &&
      ((uintptr_t)out_grad & 15) == 0 && ((uintptr_t)feat_grad & 15) == 0) {
    int lpv = c / 4;
    unsigned nb = (unsigned)pw_cdiv((int64_t)n_intervals * lpv, 256);
    PW_DISPATCH_LPV(lpv, hipLaunchKernelGGL((k_pool_bwd<L>), dim3(nb), dim3(256), 0, st,
                                            (const float4*)out_grad, depth, (const float4*)feat,
                                            ranks_depth, ranks_feat, ranks_bev, interval_starts,
                                            interval_lengths, n_intervals, depth_grad,
                                            (float4*)feat_grad));
  } else {
    const int tree_lpv = lpv_supported(c) && c <= 256 ? c / 4 : 0;      // misaligned buffers only: keep k_pool_bwd's sum order
    hipLaunchKernelGGL(k_pool_bwd_generic, dim3((unsigned)pw_cdiv(n_intervals, 256)), dim3(256), 0,
                       st, c, tree_lpv, n_intervals, out_grad, depth, feat, ranks_depth, ranks_feat,
                       ranks_bev, interval_starts, interval_lengths, depth_grad, feat_grad);
  }
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// ------------------------------------------------------------------------------------
// A22  occupancy confusion matrix (mmdet3d/datasets/occ_metrics.py:82-105: bincount(n_cl*gt+pred)
// over voxels with gt < n_cl, optionally restricted to mask_camera / mask_lidar).  Integer work:
// per-wave privatised LDS histograms, one global atomic per (bin, block).
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_confusion_hist(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                 const uint8_t* __restrict__ mask, int64_t n, int n_cl,
                 unsigned long long* __restrict__ hist) {
  extern __shared__ unsigned int lh[];
  const int nb = n_cl * n_cl;
  for (int k = threadIdx.x; k < nb; k += blockDim.x) lh[k] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (mask && !mask[i]) continue;
    const int g = gt[i], p = pred[i];
    if (g < n_cl && p < n_cl) atomicAdd(&lh[g * n_cl + p], 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nb; k += blockDim.x)
    if (lh[k]) atomicAdd(&hist[k], (unsigned long long)lh[k]);
}

PW_API int pw_confusion_hist(const uint8_t* pred, const uint8_t* gt, const uint8_t* mask, int64_t n,
                             int n_cl, int64_t* hist, void* stream) {
  PW_CHECK_ARG(pred && gt && hist && n >= 0 && n_cl > 0 && n_cl <= 64, "pw_confusion_hist: bad arguments");
  if (n == 0) return PW_OK;
  int64_t want = pw_cdiv(n, 256 * 16);
  unsigned nb = (unsigned)(want < 1024 ? (want < 1 ? 1 : want) : 1024);
  hipLaunchKernelGGL(k_confusion_hist, dim3(nb), dim3(256), (size_t)n_cl * n_cl * 4, pw_stream(stream),
                     pred, gt, mask, n, n_cl, reinterpret_cast<unsigned long long*>(hist));
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// ------------------------------------------------------------------------------------
// DepthNet tail (view_transformer.py:797-801 + :189): softmax over the D depth logits of each
// pixel and the channels-last copy of the context features, one thread per pixel.  Reads are
// coalesced over pixels (channel stride HW), the softmax keeps its D values in registers between
// the max / exp-sum / normalise sweeps when D <= 96 (one read of the logits), the context row
// leaves as float4 stores.  HBM: (D + C) * 4 B read and written per pixel.
// ------------------------------------------------------------------------------------
template <int DMAX>
__global__ void __launch_bounds__(256)
k_depthnet_tail(const float* __restrict__ x, int x_channels, int D, int C, int HW,
                float* __restrict__ depth, float4* __restrict__ feat_cl) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  const int bn = blockIdx.y;
  if (pix >= HW) return;
  const float* xp = x + ((size_t)bn * x_channels) * HW + pix;
  float* dp = depth + ((size_t)bn * D) * HW + pix;
  if (DMAX > 0) {
    float v[DMAX > 0 ? DMAX : 1];
    float m = -3.402823466e38f;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      v[d] = d < D ? xp[(size_t)d * HW] : -3.402823466e38f;
      m = fmaxf(m, v[d]);
    }
    float sum = 0.f;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      v[d] = d < D ? expf(v[d] - m) : 0.f;
      sum += v[d];
    }
#pragma unroll
    for (int d = 0; d < DMAX; ++d)
      if (d < D) dp[(size_t)d * HW] = v[d] / sum;
  } else {
    float m = -3.402823466e38f;
    for (int d = 0; d < D; ++d) m = fmaxf(m, xp[(size_t)d * HW]);
    float sum = 0.f;
    for (int d = 0; d < D; ++d) sum += expf(xp[(size_t)d * HW] - m);
    for (int d = 0; d < D; ++d) dp[(size_t)d * HW] = expf(xp[(size_t)d * HW] - m) / sum;
  }
  const float* cp = xp + (size_t)D * HW;
  float4* fo = feat_cl + ((size_t)bn * HW + pix) * (C / 4);
  for (int c = 0; c < C; c += 4)
    fo[c / 4] = make_float4(cp[(size_t)c * HW], cp[(size_t)(c + 1) * HW], cp[(size_t)(c + 2) * HW],
                            cp[(size_t)(c + 3) * HW]);
}

PW_API int pw_depthnet_tail(const float* x, int BN, int x_channels, int D, int C, int HW, float* depth,
                            float* feat_cl, void* stream) {
  PW_CHECK_ARG(x && depth && feat_cl, "pw_depthnet_tail: null pointer");
  PW_CHECK_ARG(BN > 0 && D > 0 && C > 0 && HW > 0 && x_channels >= D + C, "pw_depthnet_tail: bad shape");
  PW_CHECK_ARG(C % 4 == 0 && ((uintptr_t)feat_cl & 15) == 0, "pw_depthnet_tail: C must be a multiple of 4, feat_cl 16-B aligned");
  dim3 grid((unsigned)pw_cdiv(HW, 256), (unsigned)BN);
  hipStream_t st = pw_stream(stream);
  if (D <= 96)
    hipLaunchKernelGGL(k_depthnet_tail<96>, grid, dim3(256), 0, st, x, x_channels, D, C, HW, depth, (float4*)feat_cl);
  else
    hipLaunchKernelGGL(k_depthnet_tail<0>, grid, dim3(256), 0, st, x, x_channels, D, C, HW, depth, (float4*)feat_cl);
  PW_CHECK_LAUNCH();
  return PW_OK;
}
