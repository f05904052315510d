// Dense camera views of one attribute grid for gfx950: pw_render_views / pw_render_label_views.
// Restates (reference paths):
//   mmdet3d/datasets/ray.py:34-45,50                       get_rays as pts2ray calls it (pixel centre = +0.5)
//   mmdet3d/models/nerf/nerf_head.py:32-55,165-269,331-353 sample_ray, render_one_scene, render_depth/semantic/color
//   mmdet3d/models/nerf/cuda/render_utils_kernel.cu:431-443,577-605   raw2alpha, alpha2weight (early stop at T < 1e-3)
//   mmdet3d/models/nerf/cuda/ub360_utils_kernel.cu:13-32   cumdist_thres
// The arithmetic per sample is pw_render.hip's (k_pts2ray + k_render_rays), expression for expression, so both kernels keep the
// same samples; this file is compiled with -ffp-contract=off like that one.  The per-sample code is restated here, not shared:
// pw_render.hip is untouched.
//
// Mapping: ONE LANE PER RAY, one wave per 8 x 8 pixel tile, four tiles (16 x 16 pixels) per block, blockIdx.z = view.
//  - the ray of output pixel (i, j) of view v is generated in registers from K[v], c2w[v] (device memory) and the source pixel
//    (x0 + j stride, y0 + i stride): no ray table;
//  - a lane walks its ray's samples in order, so the two recurrences of the reference (cumulative distance with reset,
//    transmittance with early stop) are plain scalar loops and the three compactions are branches; a lane whose ray has
//    terminated leaves the loop, the wave ends when its last ray has;
//  - at a given step the 64 rays of a tile are within a few voxels of each other, so their trilinear corners fall into few cache
//    lines (a packed voxel is 96 B, x-neighbours are adjacent).  No LDS staging.  Measured against the one-wave-per-ray route to
//    the same pixels: 4.8x to 6.5x faster (profiles/render_views.md); where the loads are served from was not measured;
//  - nothing per sample is written; a pixel leaves 1 .. 8 + 4 n_sem bytes.
// No lane reads another lane's registers, so a pixel's value does not depend on which tile, window, stride or launch it is in:
// sub-windows, strided renders and per-view launches are bit-identical to the crop of the full render.
//
// LABEL MODE (pw_render_label_views): instead of the packed grid, a uint8 label grid addressed through byte strides
// (label(x, y, z) = labels[x sx + y sy + z sz]).  Same rays, same sample positions, same inner | cumdist mask.  A sample's
// voxel is the one with the largest trilinear weight under the align_corners=True mapping of the soft path: floor(u + 0.5) per
// axis with u the continuous index ((p - xyz_min) / (xyz_max - xyz_min) (n - 1), evaluated as tri_setup does); outside
// [0, n) on any axis is a miss.  The first kept sample whose label is not empty_idx is the hit: cls = that label,
// depth = (s_hit + 1e-7) radius with s = 1 - 1 / (1 + t) (the soft formula with all the weight on one sample),
// alphainv_last = 0.  No hit: cls = empty_idx, depth = 1e-7 radius, alphainv_last = 1.
#include "pw_common.h"

namespace {
constexpr int RV_MAX_S = 448;     // the sample table pw_render_rays takes
constexpr int RV_NSEM = 17;
constexpr int RV_TILE = 8;        // pixels per tile edge: one wave = 8 x 8 rays

struct ViewArgs {
  const float* K;          // (V,3,3)
  const float* c2w;        // (V,4,4)
  const float* t;          // (S)
  const void* grid;        // packed (Z,Y,X,GC) fp32 / bf16, or the uint8 label grid
  float center[3], radius[3], bda[9], xyz_min[3], xyz_max[3];
  float bg_len, act_shift, interval, dist_thres, fast_thres, depth_scale, min_opacity;
  int V, H, W, x0, y0, stride, S, X, Y, Z, GC, c_sigma, c_sem, c_rgb;
  long long sx, sy, sz;    // label mode: byte strides
  int empty_idx, n_palette;
  float* out_depth;        // (V,H,W)
  uint8_t* out_cls;        // (V,H,W)
  float* out_sem;          // (V,H,W,17)
  float* out_color;        // (V,H,W,3)
  float* out_last;         // (V,H,W)
  uint8_t* out_rgb8;       // (V,H,W,3)
  const uint8_t* palette;  // (n_palette,3)
};

// continuous voxel index per axis: ATen grid_sampler_3d's unnormalisation (align_corners=True) after the reference's
// normalisation (nerf_head.py:209-211); the same expressions as tri_setup of pw_render.hip
__device__ __forceinline__ float rv_index(float p, float lo, float hi, int n) {
  const float g = ((p - lo) / (hi - lo)) * 2.f - 1.f;
  return ((g + 1.f) / 2.f) * (float)(n - 1);
}

template <bool BF16>
__device__ __forceinline__ float rv_grid_at(const void* grid, size_t idx) {
  if constexpr (BF16) return __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(grid)[idx] << 16);
  else return reinterpret_cast<const float*>(grid)[idx];
}

struct RvTri {
  int x0, y0, z0;
  float wx0, wx1, wy0, wy1, wz0, wz1;
};

__device__ __forceinline__ RvTri rv_tri(const ViewArgs& a, float px, float py, float pz) {
  RvTri t;
  const float fx = rv_index(px, a.xyz_min[0], a.xyz_max[0], a.X);
  const float fy = rv_index(py, a.xyz_min[1], a.xyz_max[1], a.Y);
  const float fz = rv_index(pz, a.xyz_min[2], a.xyz_max[2], a.Z);
  const float x0f = floorf(fx), y0f = floorf(fy), z0f = floorf(fz);
  // clamp the integer base far outside the grid so the bounds test cannot overflow
  t.x0 = (int)fminf(fmaxf(x0f, -2.f), (float)a.X + 1.f);
  t.y0 = (int)fminf(fmaxf(y0f, -2.f), (float)a.Y + 1.f);
  t.z0 = (int)fminf(fmaxf(z0f, -2.f), (float)a.Z + 1.f);
  t.wx1 = fx - x0f; t.wx0 = (x0f + 1.f) - fx;
  t.wy1 = fy - y0f; t.wy0 = (y0f + 1.f) - fy;
  t.wz1 = fz - z0f; t.wz0 = (z0f + 1.f) - fz;
  return t;
}

// the 8 corners in ATen's accumulation order (torch D = our X outermost, W = our Z innermost)
#define RV_FOR_CORNERS(t, BODY)                                                        \
  _Pragma("unroll") for (int cx = 0; cx < 2; ++cx)                                     \
  _Pragma("unroll") for (int cy = 0; cy < 2; ++cy)                                     \
  _Pragma("unroll") for (int cz = 0; cz < 2; ++cz) {                                   \
    const int xi = t.x0 + cx, yi = t.y0 + cy, zi = t.z0 + cz;                          \
    const float wgt = ((cz ? t.wz1 : t.wz0) * (cy ? t.wy1 : t.wy0)) * (cx ? t.wx1 : t.wx0); \
    const bool inb = (unsigned)xi < (unsigned)a.X && (unsigned)yi < (unsigned)a.Y &&  \
                     (unsigned)zi < (unsigned)a.Z;                                     \
    const size_t cbase = (((size_t)zi * a.Y + yi) * a.X + xi) * a.GC;                  \
    BODY                                                                               \
  }
}  // namespace

// MODE 0: packed fp32 grid, 1: packed bf16 grid, 2: uint8 label grid
template <int MODE>
__global__ void __launch_bounds__(256) k_render_views(ViewArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * (2 * RV_TILE) + (wave & 1) * RV_TILE + (lane & (RV_TILE - 1));
  const int i = blockIdx.y * (2 * RV_TILE) + (wave >> 1) * RV_TILE + (lane / RV_TILE);
  const int v = blockIdx.z;
  if (i >= a.H || j >= a.W) return;
  const size_t pix = ((size_t)v * a.H + i) * a.W + j;

  // ---- the pixel's ray: get_rays (ray.py:34-45) at the pixel centre, as k_pts2ray evaluates it
  const float* K = a.K + (size_t)v * 9;
  const float* c2w = a.c2w + (size_t)v * 16;
  const float x = (float)(a.x0 + j * a.stride), y = (float)(a.y0 + i * a.stride);
  const float d0 = ((x + 0.5f) - K[2]) / K[0];
  const float d1 = ((y + 0.5f) - K[5]) / K[4];
  float rd[3], o[3], d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) rd[k] = (d0 * c2w[k * 4 + 0] + d1 * c2w[k * 4 + 1]) + 1.f * c2w[k * 4 + 2];
  // ---- sample_ray (nerf_head.py:32-55): normalise
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = (c2w[k * 4 + 3] - a.center[k]) / a.radius[k];
  {
    float nn = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) nn += rd[k] * rd[k];
    nn = sqrtf(nn);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = rd[k] / nn;
  }

  float T_cum = 1.f, cum = 0.f, acc_d = 0.f;
  float acc_sem[RV_NSEM], acc_rgb[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < RV_NSEM; ++k) acc_sem[k] = 0.f;
  float ux = 0.f, uy = 0.f, uz = 0.f;          // the previous sample's position
  int hit = -1;                                // label mode: the hit's label
  float hit_s = 0.f;

  for (int s = 0; s < a.S; ++s) {
    const float ts = a.t[s];
    // march, contract, undo bda
    float q0 = o[0] + d[0] * ts, q1 = o[1] + d[1] * ts, q2 = o[2] + d[2] * ts;
    const float norm = sqrtf((q0 * q0 + q1 * q1) + q2 * q2);
    const bool inner = norm <= 1.f;
    if (!inner) {
      const float sc = (1.f + a.bg_len) - a.bg_len / norm;
      q0 = q0 / norm * sc; q1 = q1 / norm * sc; q2 = q2 / norm * sc;
    }
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float acc = 0.f;
      acc += a.bda[k * 3 + 0] * q0;
      acc += a.bda[k * 3 + 1] * q1;
      acc += a.bda[k * 3 + 2] * q2;
      r[k] = acc;
    }
    // cumdist_thres (ub360_utils_kernel.cu:13-32) on the distance to the previous sample (nerf_head.py:197-199)
    bool mask = inner;
    if (s > 0) {
      const float ex = r[0] - ux, ey = r[1] - uy, ez = r[2] - uz;
      cum += sqrtf((ex * ex + ey * ey) + ez * ez);
      const bool over = cum > a.dist_thres;
      cum *= (float)(!over);
      mask = mask || over;
    }
    ux = r[0]; uy = r[1]; uz = r[2];
    if (!mask) continue;

    if constexpr (MODE == 2) {
      const float fx = rv_index(r[0], a.xyz_min[0], a.xyz_max[0], a.X);
      const float fy = rv_index(r[1], a.xyz_min[1], a.xyz_max[1], a.Y);
      const float fz = rv_index(r[2], a.xyz_min[2], a.xyz_max[2], a.Z);
      const float xf = floorf(fx + 0.5f), yf = floorf(fy + 0.5f), zf = floorf(fz + 0.5f);
      if (xf >= 0.f && xf < (float)a.X && yf >= 0.f && yf < (float)a.Y && zf >= 0.f && zf < (float)a.Z) {
        const int lab = reinterpret_cast<const uint8_t*>(a.grid)[(long long)xf * a.sx + (long long)yf * a.sy + (long long)zf * a.sz];
        if (lab != a.empty_idx) {
          hit = lab;
          hit_s = 1.f - 1.f / (1.f + ts);
          break;
        }
      }
    } else {
      // density gather + raw2alpha
      const RvTri t3 = rv_tri(a, r[0], r[1], r[2]);
      float sig = 0.f;
      RV_FOR_CORNERS(t3, { if (inb) sig += rv_grid_at<MODE == 1>(a.grid, cbase + a.c_sigma) * wgt; })
      const float e = expf(sig + a.act_shift);
      const float al = 1.f - powf(1.f + e, -a.interval);
      if (!(al > a.fast_thres)) continue;
      // alpha2weight (render_utils_kernel.cu:577-605)
      const float wq = T_cum * al;
      T_cum = (float)((double)T_cum * (1. - (double)al));
      if (wq > a.fast_thres) {
        // render_depth/semantic/color (nerf_head.py:331-353)
        acc_d += wq * (1.f - 1.f / (1.f + ts));
        float sem[RV_NSEM], rgb[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < RV_NSEM; ++k) sem[k] = 0.f;
        RV_FOR_CORNERS(t3, {
          if (inb) {
            _Pragma("unroll") for (int k = 0; k < RV_NSEM; ++k) sem[k] += rv_grid_at<MODE == 1>(a.grid, cbase + a.c_sem + k) * wgt;
            _Pragma("unroll") for (int k = 0; k < 3; ++k) rgb[k] += rv_grid_at<MODE == 1>(a.grid, cbase + a.c_rgb + k) * wgt;
          }
        })
#pragma unroll
        for (int k = 0; k < RV_NSEM; ++k) acc_sem[k] += wq * sem[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) acc_rgb[k] += wq * rgb[k];
      }
      if ((double)T_cum < 1e-3) break;           // this ray is done; the wave goes on with the others
    }
  }

  int cls;
  float depth, last;
  if constexpr (MODE == 2) {
    cls = hit >= 0 ? hit : a.empty_idx;
    depth = ((hit >= 0 ? hit_s : 0.f) + 1e-7f) * a.depth_scale;
    last = hit >= 0 ? 0.f : 1.f;
  } else {
    depth = (acc_d + 1e-7f) * a.depth_scale;     // (+1e-7) * radius (nerf_head.py:337-338)
    last = T_cum;
    cls = 0;
    float best = acc_sem[0];
#pragma unroll
    for (int k = 1; k < RV_NSEM; ++k)
      if (acc_sem[k] > best) { best = acc_sem[k]; cls = k; }
    if (a.min_opacity > 0.f && 1.f - last < a.min_opacity) cls = RV_NSEM;
    if (a.out_sem) {
#pragma unroll
      for (int k = 0; k < RV_NSEM; ++k) a.out_sem[pix * RV_NSEM + k] = acc_sem[k];
    }
    if (a.out_color) {
#pragma unroll
      for (int k = 0; k < 3; ++k) a.out_color[pix * 3 + k] = acc_rgb[k];
    }
  }
  if (a.out_depth) a.out_depth[pix] = depth;
  if (a.out_last) a.out_last[pix] = last;
  if (a.out_cls) a.out_cls[pix] = (uint8_t)cls;
  if (a.out_rgb8) {
    const int pc = min(cls, a.n_palette - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) a.out_rgb8[pix * 3 + k] = a.palette[pc * 3 + k];
  }
}

static int rv_common(const char* who, ViewArgs& a, const float* K, const float* c2w, int n_views, int H, int W, int x0, int y0,
                     int stride, const float* t, int n_samples, int X, int Y, int Z, const float* consts_host) {
  PW_CHECK_ARG(K && c2w && t && consts_host, "%s: null pointer", who);
  PW_CHECK_ARG(n_views > 0 && n_views <= 65535 && H > 0 && W > 0 && stride > 0, "%s: bad view count / image size / stride (V=%d, H=%d, W=%d, stride=%d)",
               who, n_views, H, W, stride);
  PW_CHECK_ARG((int64_t)n_views * H * W < (1ll << 31) && pw_cdiv(H, 2 * RV_TILE) <= 65535, "%s: too many pixels for one launch", who);
  PW_CHECK_ARG(n_samples > 1 && n_samples <= RV_MAX_S, "%s: n_samples must be in [2, %d]", who, RV_MAX_S);
  PW_CHECK_ARG(X > 1 && Y > 1 && Z > 1, "%s: bad grid", who);
  PW_CHECK_ARG((((uintptr_t)K | (uintptr_t)c2w | (uintptr_t)t) & 3) == 0, "%s: K / c2w / t must be 4-B aligned", who);
  a.K = K; a.c2w = c2w; a.t = t;
  const float* c = consts_host;
  for (int i = 0; i < 3; ++i) { a.center[i] = c[i]; a.radius[i] = c[3 + i]; a.xyz_min[i] = c[15 + i]; a.xyz_max[i] = c[18 + i]; }
  for (int i = 0; i < 9; ++i) a.bda[i] = c[6 + i];
  a.bg_len = c[21]; a.act_shift = c[22]; a.interval = c[23]; a.dist_thres = c[24]; a.fast_thres = c[25];
  a.depth_scale = c[26];
  a.V = n_views; a.H = H; a.W = W; a.x0 = x0; a.y0 = y0; a.stride = stride; a.S = n_samples; a.X = X; a.Y = Y; a.Z = Z;
  return PW_OK;
}

static dim3 rv_blocks(const ViewArgs& a) {
  return dim3((unsigned)pw_cdiv(a.W, 2 * RV_TILE), (unsigned)pw_cdiv(a.H, 2 * RV_TILE), (unsigned)a.V);
}

PW_API int pw_render_views(const float* K, const float* c2w, int n_views, int H, int W, int x0, int y0, int stride,
                           const float* t, int n_samples, const float* grid, int X, int Y, int Z, int grid_channels,
                           int c_sigma, int c_sem, int n_sem, int c_rgb, const float* consts_host, float* out_depth,
                           uint8_t* out_cls, float* out_sem, float* out_color, float* out_last, uint8_t* out_rgb8,
                           const uint8_t* palette, float min_opacity, int grid_bf16, void* stream) {
  ViewArgs a = {};
  if (int rc = rv_common("pw_render_views", a, K, c2w, n_views, H, W, x0, y0, stride, t, n_samples, X, Y, Z, consts_host)) return rc;
  PW_CHECK_ARG(grid, "pw_render_views: null grid");
  PW_CHECK_ARG(out_depth || out_cls || out_sem || out_color || out_last || out_rgb8, "pw_render_views: no output requested (every output pointer is null)");
  PW_CHECK_ARG(n_sem == RV_NSEM, "pw_render_views: built for 17 semantic classes (got %d)", n_sem);
  PW_CHECK_ARG(grid_channels > 0 && c_sigma >= 0 && c_sigma < grid_channels && c_sem >= 0 && c_sem + n_sem <= grid_channels &&
                   c_rgb >= 0 && c_rgb + 3 <= grid_channels,
               "pw_render_views: channel offsets outside the packed grid (a uint8 label grid goes through pw_render_label_views)");
  PW_CHECK_ARG(((uintptr_t)grid & (grid_bf16 ? 1 : 3)) == 0 && (((uintptr_t)out_depth | (uintptr_t)out_sem | (uintptr_t)out_color | (uintptr_t)out_last) & 3) == 0,
               "pw_render_views: grid / float outputs must be aligned to their element size");
  PW_CHECK_ARG(!out_rgb8 || palette, "pw_render_views: rgb8 needs a palette of (n_sem + 1, 3) uint8");
  PW_CHECK_ARG(min_opacity >= 0.f && min_opacity <= 1.f, "pw_render_views: min_opacity must be in [0, 1]");
  a.grid = grid; a.GC = grid_channels; a.c_sigma = c_sigma; a.c_sem = c_sem; a.c_rgb = c_rgb;
  a.min_opacity = min_opacity; a.n_palette = n_sem + 1;
  a.out_depth = out_depth; a.out_cls = out_cls; a.out_sem = out_sem; a.out_color = out_color; a.out_last = out_last;
  a.out_rgb8 = out_rgb8; a.palette = palette;
  if (grid_bf16) hipLaunchKernelGGL(k_render_views<1>, rv_blocks(a), dim3(256), 0, pw_stream(stream), a);
  else hipLaunchKernelGGL(k_render_views<0>, rv_blocks(a), dim3(256), 0, pw_stream(stream), a);
  pw_note_kernel("k_render_views<%d>", grid_bf16 ? 1 : 0);
  PW_CHECK_LAUNCH();
  return PW_OK;
}

PW_API int pw_render_label_views(const float* K, const float* c2w, int n_views, int H, int W, int x0, int y0, int stride,
                                 const float* t, int n_samples, const uint8_t* labels, int X, int Y, int Z, int64_t stride_x,
                                 int64_t stride_y, int64_t stride_z, int empty_idx, const float* consts_host, float* out_depth,
                                 uint8_t* out_cls, float* out_last, uint8_t* out_rgb8, const uint8_t* palette, int n_palette,
                                 void* stream) {
  ViewArgs a = {};
  if (int rc = rv_common("pw_render_label_views", a, K, c2w, n_views, H, W, x0, y0, stride, t, n_samples, X, Y, Z, consts_host)) return rc;
  PW_CHECK_ARG(labels, "pw_render_label_views: null label grid");
  PW_CHECK_ARG(out_depth || out_cls || out_last || out_rgb8, "pw_render_label_views: no output requested (every output pointer is null)");
  PW_CHECK_ARG(stride_x > 0 && stride_y > 0 && stride_z > 0, "pw_render_label_views: byte strides must be positive");
  PW_CHECK_ARG(empty_idx >= 0 && empty_idx <= 255, "pw_render_label_views: empty_idx must be a uint8 value");
  PW_CHECK_ARG((((uintptr_t)out_depth | (uintptr_t)out_last) & 3) == 0, "pw_render_label_views: float outputs must be 4-B aligned");
  PW_CHECK_ARG(!out_rgb8 || (palette && n_palette > 0), "pw_render_label_views: rgb8 needs a palette of (n_palette, 3) uint8");
  a.grid = labels; a.sx = stride_x; a.sy = stride_y; a.sz = stride_z; a.empty_idx = empty_idx; a.n_palette = n_palette;
  a.out_depth = out_depth; a.out_cls = out_cls; a.out_last = out_last; a.out_rgb8 = out_rgb8; a.palette = palette;
  hipLaunchKernelGGL(k_render_views<2>, rv_blocks(a), dim3(256), 0, pw_stream(stream), a);
  pw_note_kernel("k_render_views<2>");
  PW_CHECK_LAUNCH();
  return PW_OK;
}
