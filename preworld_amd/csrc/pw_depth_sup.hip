// LSS depth supervision on the device: lidar sweep -> depth maps / depth labels, dense depth map -> labels, and the depth loss
// with its gradient.  Replaces, expression for expression,
//   mmdet3d/datasets/pipelines/loading.py:762-844          PointToMultiViewDepth (points2depthmap + the projection of __call__)
//   mmdet3d/models/necks/view_transformer.py:736-773       get_downsampled_gt_depth (sid=False)
//   mmdet3d/models/necks/view_transformer.py:775-789       get_depth_loss (F.binary_cross_entropy on the foreground cells)
// Built with -ffp-contract=off: the compiler fuses nothing, and the two places where the reference's arithmetic IS fused are
// written out with fmaf -- `points.matmul(M.T)` is a BLAS sgemm on the host, whose inner product over k = 0, 1, 2 is the chain
// fma(p2, m2, fma(p1, m1, p0 * m0)) on every FMA-capable CPU; the translation is a separate rounded add after it.
//
// The winner of a pixel (or a loss cell) is the EXACT minimum depth: depths that pass the range test are positive, so the order
// of their float bit patterns is the order of the values and an unsigned integer atomic min decides -- independent of the order
// in which the points arrive, hence deterministic.  (The reference sorts on float32(rank + depth / 100) with an unstable argsort;
// where two depths of one pixel round to the same key either may win.  INTEGRATION.md, "Depth supervision from the sweep".)
#include "pw_common.h"

#define PW_INF_BITS 0x7f800000u

namespace {

__global__ void __launch_bounds__(256) k_fill_u32(uint32_t* __restrict__ p, int64_t n, uint32_t v) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

// one thread = one point seen by one camera of its sample; blockIdx.y = camera
//   h, w   : size of the map the rounded pixel lives on (H / map_ds, W / map_ds)
//   cell   : 1 -> one slot per pixel; ds_loss -> one slot per cell x cell patch (slot row length w / cell)
__global__ void __launch_bounds__(256)
k_project_min(const float* __restrict__ pts, int64_t n_pts, int stride, const int32_t* __restrict__ offsets, int B, int N,
              const float* __restrict__ l2i, const float* __restrict__ prot, const float* __restrict__ ptran, int h, int w,
              float map_ds, int cell, float d0, float d1, uint32_t* __restrict__ slots) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pts) return;
  int b = 0;
  if (offsets) {
    if (i < offsets[0] || i >= offsets[B]) return;
    while (b + 1 < B && i >= offsets[b + 1]) ++b;
  }
  const int v = b * N + blockIdx.y;
  const float* p = pts + i * stride;
  const float px = p[0], py = p[1], pz = p[2];
  const float* M = l2i + (int64_t)v * 12;          // 3 x 4 row-major: [R | t]
  // points.matmul(R.T) + t   (loading.py:831-832)
  float x = fmaf(pz, M[2], fmaf(py, M[1], px * M[0])) + M[3];
  float y = fmaf(pz, M[6], fmaf(py, M[5], px * M[4])) + M[7];
  float z = fmaf(pz, M[10], fmaf(py, M[9], px * M[8])) + M[11];
  // cat([xy / z, z])   (:833-835)
  x = x / z;
  y = y / z;
  // points_img.matmul(post_rot.T) + post_tran   (:837-838) -- all three rows, the depth row included
  const float* R = prot + (int64_t)v * 9;
  const float* T = ptran + (int64_t)v * 3;
  const float u = fmaf(z, R[2], fmaf(y, R[1], x * R[0])) + T[0];
  const float q = fmaf(z, R[5], fmaf(y, R[4], x * R[3])) + T[1];
  const float d = fmaf(z, R[8], fmaf(y, R[7], x * R[6])) + T[2];
  // points2depthmap (:771-777): round half to even, then the kept1 test in float (NaN and inf fail it)
  const float cx = rintf(u / map_ds), cy = rintf(q / map_ds);
  if (!(cx >= 0.f && cx < (float)w && cy >= 0.f && cy < (float)h && d < d1 && d >= d0)) return;
  const int ix = (int)cx / cell, iy = (int)cy / cell;
  const int64_t slot = ((int64_t)v * (h / cell) + iy) * (w / cell) + ix;
  atomicMin(slots + slot, __float_as_uint(d));
}

// untouched slots (+inf bits) -> 0.0f; the rest already hold the depth's bits
__global__ void __launch_bounds__(256) k_finish_maps(uint32_t* __restrict__ slots, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && slots[i] == PW_INF_BITS) slots[i] = 0u;
}

// get_downsampled_gt_depth's binning (view_transformer.py:757-771) of one cell minimum m (1e5 = nothing there)
__device__ __forceinline__ int32_t bin_label(float m, float sub, float dstep, float Dp1) {
  const float g = (m - sub) / dstep;
  return (g < Dp1 && g >= 0.f) ? (int32_t)g - 1 : -1;
}

__global__ void __launch_bounds__(256)
k_finish_labels(int32_t* __restrict__ slots, int64_t n, float sub, float dstep, float Dp1) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t bits = (uint32_t)slots[i];
  slots[i] = bits == PW_INF_BITS ? -1 : bin_label(__uint_as_float(bits), sub, dstep, Dp1);
}

// one block = one row of cells of one view: every thread takes the column minima of the ds rows (coalesced along W), then the
// first w threads take the minimum over the ds columns of their cell
__global__ void __launch_bounds__(256)
k_map_labels(const float* __restrict__ maps, int H, int W, int ds, float sub, float dstep, float Dp1,
             int32_t* __restrict__ labels) {
  extern __shared__ float colmin[];
  const int h = H / ds, w = W / ds;
  const int v = blockIdx.x / h, cy = blockIdx.x % h;
  const float* src = maps + ((int64_t)v * H + (int64_t)cy * ds) * W;
  for (int x = threadIdx.x; x < w * ds; x += 256) {
    float m = 1e5f;
    for (int r = 0; r < ds; ++r) {
      float t = src[(int64_t)r * W + x];
      t = t == 0.f ? 1e5f : t;               // torch.where(gt == 0, 1e5, gt)
      m = t < m ? t : m;
    }
    colmin[x] = m;
  }
  __syncthreads();
  for (int cx = threadIdx.x; cx < w; cx += 256) {
    float m = colmin[cx * ds];
    for (int c = 1; c < ds; ++c) {
      const float t = colmin[cx * ds + c];
      m = t < m ? t : m;
    }
    labels[((int64_t)v * h + cy) * w + cx] = bin_label(m, sub, dstep, Dp1);
  }
}

// ---------------------------------------------------------------------------------------------------------------- the loss
// pred (BN, D, hw), labels (BN, hw).  A block is 64 consecutive cells (lanes, the contiguous dimension) x 4 slices of D
// (thread y takes d = y, y + 4, ...): every global access of a wave is one 256-byte row segment.
#define BCE_CELLS 64
#define BCE_SLICES 4

__device__ __forceinline__ float clamp_log(float p) {     // torch's binary_cross_entropy clamps each log at -100
  const float l = logf(p);
  return l < -100.f ? -100.f : l;
}

__global__ void __launch_bounds__(BCE_CELLS * BCE_SLICES)
k_bce_fwd(const float* __restrict__ pred, const int32_t* __restrict__ labels, int64_t n_cells, int D, int64_t hw,
          double* __restrict__ part_sum, int32_t* __restrict__ part_cnt) {
  __shared__ double s_sum[BCE_SLICES][BCE_CELLS];
  __shared__ int32_t s_cnt[BCE_CELLS];
  const int lane = threadIdx.x, sl = threadIdx.y;
  const int64_t cell = (int64_t)blockIdx.x * BCE_CELLS + lane;
  double acc = 0.0;
  int fg = 0;
  if (cell < n_cells) {
    const int k = labels[cell];
    if (k >= 0 && k < D) {
      fg = 1;
      const float* p = pred + (cell / hw) * (int64_t)D * hw + cell % hw;
      for (int d = sl; d < D; d += BCE_SLICES) {
        const float v = p[(int64_t)d * hw];
        acc += (double)-(d == k ? clamp_log(v) : clamp_log(1.f - v));
      }
    }
  }
  s_sum[sl][lane] = acc;
  if (sl == 0) s_cnt[lane] = fg;
  __syncthreads();
  if (sl == 0 && lane == 0) {                 // fixed order: slices of cell 0, then cell 1, ...
    double t = 0.0;
    int32_t c = 0;
    for (int l = 0; l < BCE_CELLS; ++l) {
      for (int s = 0; s < BCE_SLICES; ++s) t += s_sum[s][l];
      c += s_cnt[l];
    }
    part_sum[blockIdx.x] = t;
    part_cnt[blockIdx.x] = c;
  }
}

// one block: thread t sums partials t, t + 256, ... in that order, then thread 0 sums the 256 in order
__global__ void __launch_bounds__(256)
k_bce_finish(const double* __restrict__ part_sum, const int32_t* __restrict__ part_cnt, int n_part, float weight,
             float* __restrict__ loss, int32_t* __restrict__ n_fg) {
  __shared__ double s_sum[256];
  __shared__ int32_t s_cnt[256];
  double t = 0.0;
  int32_t c = 0;
  for (int i = threadIdx.x; i < n_part; i += 256) {
    t += part_sum[i];
    c += part_cnt[i];
  }
  s_sum[threadIdx.x] = t;
  s_cnt[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    int32_t n = 0;
    for (int i = 0; i < 256; ++i) {
      a += s_sum[i];
      n += s_cnt[i];
    }
    *n_fg = n;
    *loss = (float)((double)weight * (a / (double)(n > 1 ? n : 1)));
  }
}

__global__ void __launch_bounds__(BCE_CELLS * BCE_SLICES)
k_bce_bwd(const float* __restrict__ pred, const int32_t* __restrict__ labels, const float* __restrict__ grad_out,
          const int32_t* __restrict__ n_fg, float weight, int64_t n_cells, int D, int64_t hw, float* __restrict__ grad_pred) {
  const int lane = threadIdx.x, sl = threadIdx.y;
  const int64_t cell = (int64_t)blockIdx.x * BCE_CELLS + lane;
  if (cell >= n_cells) return;
  const int k = labels[cell];
  const bool fg = k >= 0 && k < D;
  const int n = *n_fg;
  const float coef = (*grad_out * weight) / (float)(n > 1 ? n : 1);
  const int64_t base = (cell / hw) * (int64_t)D * hw + cell % hw;
  for (int d = sl; d < D; d += BCE_SLICES) {
    const int64_t o = base + (int64_t)d * hw;
    float g = 0.f;
    if (fg) {
      const float v = pred[o];
      const float den = fmaxf((1.f - v) * v, 1e-12f);      // ATen binary_cross_entropy_backward, EPSILON = 1e-12
      g = coef * (v - (d == k ? 1.f : 0.f)) / den;
    }
    grad_pred[o] = g;
  }
}

int project(const float* points, int64_t n_points, int point_stride, const int32_t* offsets, int B, int N,
            const float* lidar2img, const float* post_rot, const float* post_tran, int h, int w, int map_ds, int cell,
            float d0, float d1, uint32_t* slots, int64_t n_slots, hipStream_t st) {
  PW_CHECK_ARG(n_slots < ((int64_t)1 << 40), "pw_lidar_depth_*: B N h w must stay under 2^40 (one thread per output element)");
  hipLaunchKernelGGL(k_fill_u32, dim3((unsigned)pw_cdiv(n_slots, 256)), dim3(256), 0, st, slots, n_slots, PW_INF_BITS);
  PW_CHECK_LAUNCH();
  if (n_points > 0) {
    hipLaunchKernelGGL(k_project_min, dim3((unsigned)pw_cdiv(n_points, 256), (unsigned)N), dim3(256), 0, st, points, n_points,
                       point_stride, offsets, B, N, lidar2img, post_rot, post_tran, h, w, (float)map_ds, cell, d0, d1, slots);
    PW_CHECK_LAUNCH();
  }
  pw_note_kernel("k_project_min");
  return PW_OK;
}

}  // namespace

#define CHECK_SWEEP(who)                                                                                                    \
  PW_CHECK_ARG((points || n_points == 0) && lidar2img && post_rot && post_tran, who ": null pointer");                      \
  PW_CHECK_ARG(n_points >= 0 && n_points < ((int64_t)1 << 31) && point_stride >= 3, who ": need 0 <= n_points < 2^31 and point_stride >= 3"); \
  PW_CHECK_ARG(B >= 1 && N >= 1 && N <= 65535 && (offsets || B == 1), who ": need B >= 1, 1 <= N <= 65535, offsets for B > 1"); \
  PW_CHECK_ARG(H > 0 && W > 0 && downsample >= 1, who ": bad image size or downsample");                                   \
  PW_CHECK_ARG(d0 > 0.f && d1 > d0, who ": the depth range must satisfy 0 < d0 < d1 (the minimum is taken on the bit pattern)")

PW_API int pw_lidar_depth_maps(const float* points, int64_t n_points, int point_stride, const int32_t* offsets, int B, int N,
                               const float* lidar2img, const float* post_rot, const float* post_tran, int H, int W,
                               int downsample, float d0, float d1, float* depth_maps, void* stream) {
  CHECK_SWEEP("pw_lidar_depth_maps");
  PW_CHECK_ARG(depth_maps, "pw_lidar_depth_maps: depth_maps is null");
  const int h = H / downsample, w = W / downsample;
  PW_CHECK_ARG(h > 0 && w > 0, "pw_lidar_depth_maps: downsample larger than the image");
  const int64_t n = (int64_t)B * N * h * w;
  hipStream_t st = pw_stream(stream);
  int rc = project(points, n_points, point_stride, offsets, B, N, lidar2img, post_rot, post_tran, h, w,
                   downsample, 1, d0, d1, reinterpret_cast<uint32_t*>(depth_maps), n, st);
  if (rc != PW_OK) return rc;
  hipLaunchKernelGGL(k_finish_maps, dim3((unsigned)pw_cdiv(n, 256)), dim3(256), 0, st, reinterpret_cast<uint32_t*>(depth_maps), n);
  PW_CHECK_LAUNCH();
  return PW_OK;
}

#define CHECK_BINS(who)                                                                                                     \
  PW_CHECK_ARG(dstep > 0.f && D >= 1, who ": need dstep > 0 and D >= 1")

PW_API int pw_lidar_depth_labels(const float* points, int64_t n_points, int point_stride, const int32_t* offsets, int B, int N,
                                 const float* lidar2img, const float* post_rot, const float* post_tran, int H, int W,
                                 int downsample, int loss_downsample, float d0, float d1, float dstep, int D, int32_t* labels,
                                 void* stream) {
  CHECK_SWEEP("pw_lidar_depth_labels");
  CHECK_BINS("pw_lidar_depth_labels");
  PW_CHECK_ARG(labels, "pw_lidar_depth_labels: labels is null");
  const int h = H / downsample, w = W / downsample;
  PW_CHECK_ARG(loss_downsample >= 1 && h > 0 && w > 0 && h % loss_downsample == 0 && w % loss_downsample == 0,
               "pw_lidar_depth_labels: loss_downsample must divide H / downsample and W / downsample");
  const int64_t n = (int64_t)B * N * (h / loss_downsample) * (w / loss_downsample);
  hipStream_t st = pw_stream(stream);
  int rc = project(points, n_points, point_stride, offsets, B, N, lidar2img, post_rot, post_tran, h, w,
                   downsample, loss_downsample, d0, d1, reinterpret_cast<uint32_t*>(labels), n, st);
  if (rc != PW_OK) return rc;
  hipLaunchKernelGGL(k_finish_labels, dim3((unsigned)pw_cdiv(n, 256)), dim3(256), 0, st, labels, n,
                     (float)((double)d0 - (double)dstep), dstep, (float)(D + 1));
  PW_CHECK_LAUNCH();
  return PW_OK;
}

PW_API int pw_depth_map_labels(const float* depth_maps, int n_views, int H, int W, int downsample, float d0, float dstep, int D,
                               int32_t* labels, void* stream) {
  PW_CHECK_ARG(depth_maps && labels, "pw_depth_map_labels: null pointer");
  CHECK_BINS("pw_depth_map_labels");
  PW_CHECK_ARG(n_views >= 1 && H > 0 && W > 0 && downsample >= 1 && H % downsample == 0 && W % downsample == 0,
               "pw_depth_map_labels: downsample must divide H and W");
  PW_CHECK_ARG(W <= 12288, "pw_depth_map_labels: W <= 12288 (one row of column minima is staged in LDS)");
  const int64_t blocks = (int64_t)n_views * (H / downsample);
  PW_CHECK_ARG(blocks < ((int64_t)1 << 31), "pw_depth_map_labels: too many cell rows");
  hipLaunchKernelGGL(k_map_labels, dim3((unsigned)blocks), dim3(256), (size_t)W * sizeof(float), pw_stream(stream), depth_maps,
                     H, W, downsample, (float)((double)d0 - (double)dstep), dstep, (float)(D + 1), labels);
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_map_labels");
  return PW_OK;
}

PW_API size_t pw_depth_bce_ws_bytes(int64_t n_cells) {
  if (n_cells <= 0) return 0;
  return (size_t)pw_cdiv(n_cells, BCE_CELLS) * (sizeof(double) + sizeof(int32_t));
}

PW_API int pw_depth_bce_fwd(const float* pred, const int32_t* labels, int BN, int D, int64_t hw, float weight, void* ws,
                            float* loss, int32_t* n_fg, void* stream) {
  PW_CHECK_ARG(pred && labels && ws && loss && n_fg, "pw_depth_bce_fwd: null pointer");
  PW_CHECK_ARG(BN >= 1 && D >= 1 && hw >= 1 && (int64_t)BN * hw < ((int64_t)1 << 31), "pw_depth_bce_fwd: bad shape");
  PW_CHECK_ARG(((uintptr_t)ws & 7) == 0, "pw_depth_bce_fwd: ws must be 8-byte aligned");
  const int64_t n_cells = (int64_t)BN * hw;
  const int n_part = (int)pw_cdiv(n_cells, BCE_CELLS);
  double* part_sum = reinterpret_cast<double*>(ws);
  int32_t* part_cnt = reinterpret_cast<int32_t*>(part_sum + n_part);
  hipStream_t st = pw_stream(stream);
  hipLaunchKernelGGL(k_bce_fwd, dim3((unsigned)n_part), dim3(BCE_CELLS, BCE_SLICES), 0, st, pred, labels, n_cells, D, hw,
                     part_sum, part_cnt);
  PW_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_bce_finish, dim3(1), dim3(256), 0, st, part_sum, part_cnt, n_part, weight, loss, n_fg);
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_bce_fwd");
  return PW_OK;
}

PW_API int pw_depth_bce_bwd(const float* pred, const int32_t* labels, const float* grad_out, const int32_t* n_fg, int BN, int D,
                            int64_t hw, float weight, float* grad_pred, void* stream) {
  PW_CHECK_ARG(pred && labels && grad_out && n_fg && grad_pred, "pw_depth_bce_bwd: null pointer");
  PW_CHECK_ARG(BN >= 1 && D >= 1 && hw >= 1 && (int64_t)BN * hw < ((int64_t)1 << 31), "pw_depth_bce_bwd: bad shape");
  const int64_t n_cells = (int64_t)BN * hw;
  hipLaunchKernelGGL(k_bce_bwd, dim3((unsigned)pw_cdiv(n_cells, BCE_CELLS)), dim3(BCE_CELLS, BCE_SLICES), 0, pw_stream(stream),
                     pred, labels, grad_out, n_fg, weight, n_cells, D, hw, grad_pred);
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_bce_bwd");
  return PW_OK;
}
