// Pre-train ray supervision on the device: lidar sweeps with their lidarseg bytes + the staged uint8 frames -> the (R, 16) ray
// table and its weighted-ray-sampling weights.  Replaces
//   tools/gen_data/gen_depth_gt.py:17-76, gen_seg_gt_from_lidarseg.py:17-81     map_pointcloud_to_image (stage A)
//   mmdet3d/datasets/nuscenes_dataset_occ.py:48-66, 197-270                     load_depth, load_seg_label, get_rays (stage B)
//   mmdet3d/datasets/ray.py:34-56, 93-112                                        get_rays / pts2ray, the WRS weights
// Built with -ffp-contract=off.  The projection is the written sequence of roundings that tests/_ray_labels_np.py restates
// ("Ray supervision from the sweep"): the cloud is a float32 array, so each of the eight rigid sub-steps ends in
// a rounding to float32 -- a rotation is a float64 3x3 product ((r0 x + r1 y) + r2 z, then rounded), a translation a float32 add
// of the translation rounded to float32 -- and the pixel and the mask are float64.
//
// The seg label of a row is the label of the LAST point in sweep order that landed in its pixel (the reference writes a dense
// map by fancy assignment and reads it back).  Here a pixel's owner is the largest point index that hit it: an integer atomicMax
// on a 64-bit slot {view, pixel | point index} of an open-addressed table sized by the point count -- independent of the order
// in which the points arrive, hence deterministic.  Rows get their place from block counts and one single-block scan: no
// cross-block waiting, the same bits on every run.
#include "pw_common.h"

#define RL_BLOCK 256
static_assert(PW_WAVE == 64 && RL_BLOCK % PW_WAVE == 0, "block_rank ranks with one 64-bit ballot per wave: gfx950 runs wave64");
#define RL_POSE PW_RAY_POSE_DOUBLES      // doubles per view: R1 t1 R2 t2 | t3 R3 t4 R4 | K
#define RL_NONE 0xffffffffu

namespace {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------- stage A: one point
__device__ __forceinline__ void rot64(const double* __restrict__ R, float& x, float& y, float& z) {
  const double a = (double)x, b = (double)y, c = (double)z;
  x = (float)((R[0] * a + R[1] * b) + R[2] * c);
  y = (float)((R[3] * a + R[4] * b) + R[5] * c);
  z = (float)((R[6] * a + R[7] * b) + R[8] * c);
}

__device__ __forceinline__ void tran32(const double* __restrict__ t, float& x, float& y, float& z) {
  x = x + (float)t[0];
  y = y + (float)t[1];
  z = z + (float)t[2];
}

// -> kept; u, v the float32 pixel as the gen tools write it, d the depth
__device__ __forceinline__ bool project_point(const float* __restrict__ p, const double* __restrict__ P, int H, int W, float& u,
                                              float& v, float& d) {
  float x = p[0], y = p[1], z = p[2];
  rot64(P, x, y, z);             // lidar -> ego
  tran32(P + 9, x, y, z);
  rot64(P + 12, x, y, z);        // ego -> global
  tran32(P + 21, x, y, z);
  tran32(P + 24, x, y, z);       // global -> camera ego (-t, then R^T: both prepared on the host)
  rot64(P + 27, x, y, z);
  tran32(P + 36, x, y, z);       // camera ego -> camera
  rot64(P + 39, x, y, z);
  const double* K = P + 48;
  const double X = (double)x, Y = (double)y, Z = (double)z;
  const double pw = (K[6] * X + K[7] * Y) + K[8] * Z;
  const double pu = ((K[0] * X + K[1] * Y) + K[2] * Z) / pw;
  const double pv = ((K[3] * X + K[4] * Y) + K[5] * Z) / pw;
  d = z;
  u = (float)pu;
  v = (float)pv;
  return z > 0.f && pu > 1.0 && pu < (double)(W - 1) && pv > 1.0 && pv < (double)(H - 1);      // NaN fails
}

// ---------------------------------------------------------------------------------------------------- the owner table
__device__ __forceinline__ uint32_t rl_hash(uint32_t k) {
  k ^= k >> 16;
  k *= 0x85ebca6bu;
  k ^= k >> 13;
  k *= 0xc2b2ae35u;
  k ^= k >> 16;
  return k;
}

// slot = key << 32 | point index, key >= 1, 0 = empty.  A slot's key never changes once set, so the maximum over one key is
// taken by atomicMax on the whole word.
__device__ __forceinline__ void owner_insert(u64* __restrict__ slots, uint32_t mask, uint32_t key, uint32_t idx) {
  const u64 mine = ((u64)key << 32) | idx;
  uint32_t h = rl_hash(key) & mask;
  for (uint32_t n = 0; n <= mask; ++n) {
    u64 cur = __atomic_load_n(slots + h, __ATOMIC_RELAXED);
    if (cur == 0ull) {
      cur = atomicCAS(slots + h, 0ull, mine);
      if (cur == 0ull) return;
    }
    if ((uint32_t)(cur >> 32) == key) {
      atomicMax(slots + h, mine);
      return;
    }
    h = (h + 1) & mask;
  }
}

__device__ __forceinline__ uint32_t owner_find(const u64* __restrict__ slots, uint32_t mask, uint32_t key) {
  uint32_t h = rl_hash(key) & mask;
  for (uint32_t n = 0; n <= mask; ++n) {
    const u64 cur = slots[h];
    if (cur == 0ull) return RL_NONE;
    if ((uint32_t)(cur >> 32) == key) return (uint32_t)cur;
    h = (h + 1) & mask;
  }
  return RL_NONE;
}

__global__ void __launch_bounds__(RL_BLOCK) k_fill_u64(u64* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RL_BLOCK) p[i] = 0ull;
}

// ---------------------------------------------------------------------------------------------------- sweeps: count + owners
struct Sweep {
  const float* points;         // [T][Pmax][stride]
  const uint8_t* labels;       // [T][Pmax] or NULL (count pass)
  const int32_t* n_pts;        // [T] or NULL
  const double* pose;          // [T N][RL_POSE]
  int stride, N, Pmax, H, W;
};

__device__ __forceinline__ int sweep_len(const Sweep& s, int t) {
  if (!s.n_pts) return s.Pmax;
  const int n = s.n_pts[t];
  return n < 0 ? 0 : (n > s.Pmax ? s.Pmax : n);
}

// grid (blocks over Pmax, camera, frame); one thread = one point seen by one camera
__global__ void __launch_bounds__(RL_BLOCK)
k_sweep_count(Sweep s, u64* __restrict__ slots, uint32_t mask, int32_t* __restrict__ block_counts) {
  const int t = blockIdx.z, v = t * s.N + blockIdx.y;
  const int i = blockIdx.x * RL_BLOCK + threadIdx.x;
  int keep = 0;
  if (i < sweep_len(s, t)) {
    float u, q, d;
    if (project_point(s.points + ((int64_t)t * s.Pmax + i) * s.stride, s.pose + (int64_t)v * RL_POSE, s.H, s.W, u, q, d)) {
      const int px = (int)u, py = (int)q;                                   // 1 <= px <= W - 1, 1 <= py <= H - 1
      keep = 1;
      if (slots) owner_insert(slots, mask, (uint32_t)(((int64_t)v * s.H + py) * s.W + px) + 1u, (uint32_t)i);
    }
  }
  const int n = __syncthreads_count(keep);
  if (threadIdx.x == 0) block_counts[(int64_t)v * gridDim.x + blockIdx.x] = n;
}

// one block: exclusive scan of the n = V nblk block counts in place, the per-view row offsets and the total
__global__ void __launch_bounds__(RL_BLOCK)
k_scan_blocks(int32_t* __restrict__ counts, int n, int V, int nblk, int32_t* __restrict__ view_off) {
  __shared__ int32_t part[RL_BLOCK];
  const int chunk = (n + RL_BLOCK - 1) / RL_BLOCK;
  const int lo = min((int)threadIdx.x * chunk, n), hi = min(lo + chunk, n);
  int32_t s = 0;
  for (int j = lo; j < hi; ++j) s += counts[j];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t acc = 0;
    for (int k = 0; k < RL_BLOCK; ++k) {
      const int32_t c = part[k];
      part[k] = acc;
      acc += c;
    }
    view_off[V] = acc;
  }
  __syncthreads();
  int32_t acc = part[threadIdx.x];
  for (int j = lo; j < hi; ++j) {
    const int32_t c = counts[j];
    counts[j] = acc;
    acc += c;
  }
  __syncthreads();
  for (int v = threadIdx.x; v < V; v += RL_BLOCK) view_off[v] = counts[(int64_t)v * nblk];
}

// ---------------------------------------------------------------------------------------------------- one row of the table
struct Rows {
  const uint8_t* frames;       // element (f, y, x, ch) at f s_f + y s_y + x s_x + ch s_c
  int64_t s_f, s_y, s_x, s_c;
  int n_frames;
  const int32_t* view_frame;   // [V] or NULL (frame v)
  float mean[3], std[3];
  const float* c2w;            // [V][16]
  const float* K;              // [V][9]
  float4* rays;                // [capacity][4]
  int64_t capacity;
  u64* counts;                 // [n_cls]
  int n_cls;
};

// get_rays / pts2ray (ray.py:34-56) with k_pts2ray's expressions; label_img = (u8 / 255.0f - mean) / std
__device__ __forceinline__ void write_row(const Rows& r, int64_t row, int v, int px, int py, bool in_image, float depth, float seg) {
  const float x = (float)px, y = (float)py;
  const float* __restrict__ c2w = r.c2w + (int64_t)v * 16;
  const float* __restrict__ K = r.K + (int64_t)v * 9;
  const float d0 = ((x + 0.5f) - K[2]) / K[0];
  const float d1 = ((y + 0.5f) - K[5]) / K[4];
  const float d2 = 1.f;
  float rd[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) rd[k] = (d0 * c2w[k * 4 + 0] + d1 * c2w[k * 4 + 1]) + d2 * c2w[k * 4 + 2];
  const float nrm = sqrtf((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2]);
  float rgb[3] = {0.f, 0.f, 0.f};
  const int f = r.view_frame ? r.view_frame[v] : v;
  if (in_image && f >= 0 && f < r.n_frames) {
    const uint8_t* __restrict__ p = r.frames + f * r.s_f + py * r.s_y + px * r.s_x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = ((float)p[ch * r.s_c] / 255.0f - r.mean[ch]) / r.std[ch];
  }
  float4* __restrict__ o = r.rays + row * 4;
  o[0] = make_float4(x, y, depth, seg);
  o[1] = make_float4(c2w[3], c2w[7], c2w[11], rd[0]);
  o[2] = make_float4(rd[1], rd[2], rd[0] / nrm, rd[1] / nrm);
  o[3] = make_float4(rd[2] / nrm, rgb[0], rgb[1], rgb[2]);
}

// per-block class histogram in LDS, then one integer atomic per class and block (ray.py:94-97)
__device__ __forceinline__ void count_classes(const Rows& r, bool written, float seg, unsigned int* local) {
  if (threadIdx.x < 64) local[threadIdx.x] = 0u;
  __syncthreads();
  if (written) {
    const int ci = (int)seg;
    if (ci >= 0 && ci < r.n_cls && (float)ci == seg) atomicAdd(&local[ci], 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x < r.n_cls && local[threadIdx.x]) atomicAdd(&r.counts[threadIdx.x], (u64)local[threadIdx.x]);
}

// rank of this thread among the block's kept threads (threads in index order)
__device__ __forceinline__ int block_rank(int keep, int* wave_tot) {
  const u64 m = __ballot(keep);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int before = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[w] = __popcll(m);
  __syncthreads();
  int base = 0;
  for (int k = 0; k < w; ++k) base += wave_tot[k];
  return base + before;
}

// same grid as k_sweep_count; lists (stage A alone) and / or rows
__global__ void __launch_bounds__(RL_BLOCK)
k_sweep_emit(Sweep s, const uint8_t* __restrict__ lut, const int32_t* __restrict__ block_base, const u64* __restrict__ slots,
             uint32_t mask, float* __restrict__ depth_list, float* __restrict__ seg_list, int64_t list_capacity, Rows r,
             int want_rows) {
  __shared__ int wave_tot[RL_BLOCK / 64];
  __shared__ unsigned int local[64];
  const int t = blockIdx.z, v = t * s.N + blockIdx.y;
  const int i = blockIdx.x * RL_BLOCK + threadIdx.x;
  int keep = 0;
  float u = 0.f, q = 0.f, d = 0.f;
  if (i < sweep_len(s, t))
    keep = project_point(s.points + ((int64_t)t * s.Pmax + i) * s.stride, s.pose + (int64_t)v * RL_POSE, s.H, s.W, u, q, d);
  const int64_t row = (int64_t)block_base[(int64_t)v * gridDim.x + blockIdx.x] + block_rank(keep, wave_tot);
  if (keep && depth_list && row < list_capacity) {
    const float lab = (float)lut[s.labels[(int64_t)t * s.Pmax + i]];
    depth_list[row * 3 + 0] = u;
    depth_list[row * 3 + 1] = q;
    depth_list[row * 3 + 2] = d;
    seg_list[row * 3 + 0] = u;
    seg_list[row * 3 + 1] = q;
    seg_list[row * 3 + 2] = lab;
  }
  if (!want_rows) return;
  const bool written = keep && row < r.capacity;
  float seg = 0.f;
  if (written) {
    const int px = (int)u, py = (int)q;
    const uint32_t own = owner_find(slots, mask, (uint32_t)(((int64_t)v * s.H + py) * s.W + px) + 1u);
    if (own != RL_NONE && (int)own < s.Pmax) seg = (float)lut[s.labels[(int64_t)t * s.Pmax + own]];
    write_row(r, row, v, px, py, true, d, seg);
  }
  count_classes(r, written, seg, local);
}

// ---------------------------------------------------------------------------------------------------- lists mode
__device__ __forceinline__ int view_of_row(const int32_t* __restrict__ view_off, int V, int64_t i) {
  int lo = 0, hi = V;                       // largest v with view_off[v] <= i
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)view_off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// cam_depth[:, :2].astype(np.int16) (nuscenes_dataset_occ.py:54): truncation; a pixel outside the image owns nothing
__device__ __forceinline__ bool list_pixel(const float* __restrict__ e, int H, int W, int& px, int& py) {
  const float x = e[0], y = e[1];
  if (!(x > -1.f && x < (float)W && y > -1.f && y < (float)H)) return false;
  px = (int)x;
  py = (int)y;
  return px >= 0 && px < W && py >= 0 && py < H;
}

__global__ void __launch_bounds__(RL_BLOCK)
k_lists_owner(const float* __restrict__ seg_list, int64_t n, const int32_t* __restrict__ view_off, int V, int H, int W,
              u64* __restrict__ slots, uint32_t mask) {
  const int64_t i = (int64_t)blockIdx.x * RL_BLOCK + threadIdx.x;
  if (i >= n || i >= view_off[V] || i < view_off[0]) return;
  int px, py;
  if (!list_pixel(seg_list + i * 3, H, W, px, py)) return;
  const int v = view_of_row(view_off, V, i);
  owner_insert(slots, mask, (uint32_t)(((int64_t)v * H + py) * W + px) + 1u, (uint32_t)i);
}

__global__ void __launch_bounds__(RL_BLOCK)
k_lists_emit(const float* __restrict__ depth_list, const float* __restrict__ seg_list, int64_t n,
             const int32_t* __restrict__ view_off, int V, int H, int W, const u64* __restrict__ slots, uint32_t mask, Rows r) {
  __shared__ unsigned int local[64];
  const int64_t i = (int64_t)blockIdx.x * RL_BLOCK + threadIdx.x;
  const bool written = i < n && i < view_off[V] && i >= view_off[0] && i < r.capacity;
  float seg = 0.f;
  if (written) {
    const int v = view_of_row(view_off, V, i);
    const float* e = depth_list + i * 3;
    int px = 0, py = 0;
    const bool in_image = list_pixel(e, H, W, px, py);
    if (in_image) {
      const uint32_t own = owner_find(slots, mask, (uint32_t)(((int64_t)v * H + py) * W + px) + 1u);
      if (own != RL_NONE && (int64_t)own < n) seg = seg_list[(int64_t)own * 3 + 2];          // untouched pixels of the map are 0
    } else {
      px = (int)fminf(fmaxf(e[0], -32768.f), 32767.f);
      py = (int)fminf(fmaxf(e[1], -32768.f), 32767.f);
    }
    write_row(r, i, v, px, py, in_image, e[2], seg);
  }
  count_classes(r, written, seg, local);
}

// ---------------------------------------------------------------------------------------------------- weights (ray.py:93-112)
__global__ void __launch_bounds__(RL_BLOCK)
k_table_weights(float* __restrict__ rays, int64_t capacity, const int32_t* __restrict__ view_off, int V,
                const int32_t* __restrict__ frame_ids, const float* __restrict__ bw_in, const int64_t* __restrict__ counts,
                int n_cls, const int32_t* __restrict__ dyn, int n_dyn, float w_adj, float w_dyn, float* __restrict__ w) {
  __shared__ float bw[64];
  if ((int)threadIdx.x < n_cls) {
    if (bw_in) {
      bw[threadIdx.x] = bw_in[threadIdx.x];
    } else {                                           // exp(0.005 * (class_nums.max() / class_nums - 1)), class_nums float32
      int64_t mx = 0;
      for (int k = 0; k < n_cls; ++k) mx = counts[k] > mx ? counts[k] : mx;
      const float arg = 0.005f * ((float)mx / (float)counts[threadIdx.x] - 1.f);
      bw[threadIdx.x] = (float)exp((double)arg);       // the correctly rounded float32 exponential
    }
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * RL_BLOCK + threadIdx.x;
  if (i >= capacity) return;
  const int64_t n_rows = view_off[V];
  if (i >= n_rows || i < view_off[0]) {                 // past the table: weight 0 (never drawn), the row zeroed
    w[i] = 0.f;
    float4* __restrict__ o = reinterpret_cast<float4*>(rays) + i * 4;
    o[0] = o[1] = o[2] = o[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float c = rays[i * 16 + 3];
  float wt = 1.f;
  if (frame_ids[view_of_row(view_off, V, i)] != 0) {
    wt = w_adj;
    for (int k = 0; k < n_dyn; ++k)
      if ((float)dyn[k] == c) wt = w_dyn;
  }
  const int ci = min(max((int)c, 0), n_cls - 1);
  w[i] = bw[ci] * wt;
}

bool pow2(int64_t n) { return n >= 2 && (n & (n - 1)) == 0; }

int fill_slots(int64_t* slots, int64_t n_slots, hipStream_t st) {
  const int64_t want = pw_cdiv(n_slots, RL_BLOCK);
  hipLaunchKernelGGL(k_fill_u64, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(RL_BLOCK), 0, st, reinterpret_cast<u64*>(slots),
                     n_slots);
  PW_CHECK_LAUNCH();
  return PW_OK;
}

}  // namespace

#define CHECK_SWEEP(who)                                                                                                     \
  PW_CHECK_ARG(points && view_pose, who ": null pointer");                                                                   \
  PW_CHECK_ARG(point_stride >= 3 && T >= 1 && T <= 65535 && N >= 1 && N <= 65535 && Pmax >= 1,                               \
               who ": need point_stride >= 3, 1 <= T, N <= 65535 and Pmax >= 1");                                            \
  PW_CHECK_ARG((int64_t)T * N * Pmax < ((int64_t)1 << 31), who ": T N Pmax must stay under 2^31 (rows are int32)");           \
  PW_CHECK_ARG(H >= 3 && W >= 3 && H <= 32767 && W <= 32767 && (int64_t)T * N * H * W < 0xffffffffll,                        \
               who ": need 3 <= H, W <= 32767 (pixels are int16) and T N H W < 2^32 - 1 (the owner key)")

#define CHECK_SLOTS(who, items)                                                                                              \
  PW_CHECK_ARG(slots && pow2(n_slots) && n_slots <= ((int64_t)1 << 31) && n_slots > (items),                                 \
               who ": slots must hold a power of two of entries (at most 2^31), more than there are points to insert");      \
  PW_CHECK_ARG(((uintptr_t)slots & 7) == 0, who ": slots must be 8-byte aligned")

#define CHECK_ROWS(who)                                                                                                      \
  PW_CHECK_ARG(frames && mean_std_host && c2w && K && rays && counts, who ": null pointer");                                 \
  PW_CHECK_ARG(n_frames >= 1 && capacity >= 1 && capacity < ((int64_t)1 << 31) && n_cls >= 1 && n_cls <= 64,                 \
               who ": need n_frames >= 1, 1 <= capacity < 2^31 and 1 <= n_cls <= 64");                                       \
  PW_CHECK_ARG(((uintptr_t)rays & 15) == 0, who ": rays must be 16-byte aligned");                                           \
  PW_CHECK_ARG(s_f >= 0 && s_y >= 0 && s_x >= 0 && s_c >= 0, who ": frame strides must not be negative")

static Rows make_rows(const uint8_t* frames, int64_t s_f, int64_t s_y, int64_t s_x, int64_t s_c, int n_frames,
                      const int32_t* view_frame, const float* mean_std_host, const float* c2w, const float* K, int64_t capacity,
                      float* rays, int n_cls, int64_t* counts) {
  Rows r;
  r.frames = frames; r.s_f = s_f; r.s_y = s_y; r.s_x = s_x; r.s_c = s_c; r.n_frames = n_frames; r.view_frame = view_frame;
  for (int k = 0; k < 3; ++k) {
    r.mean[k] = mean_std_host ? mean_std_host[k] : 0.f;
    r.std[k] = mean_std_host ? mean_std_host[3 + k] : 1.f;
  }
  r.c2w = c2w; r.K = K; r.rays = reinterpret_cast<float4*>(rays); r.capacity = capacity;
  r.counts = reinterpret_cast<u64*>(counts); r.n_cls = n_cls;
  return r;
}

static Sweep make_sweep(const float* points, int point_stride, const uint8_t* labels, const int32_t* n_pts, int N, int Pmax,
                        const double* view_pose, int H, int W) {
  Sweep s;
  s.points = points; s.labels = labels; s.n_pts = n_pts; s.pose = view_pose; s.stride = point_stride; s.N = N; s.Pmax = Pmax;
  s.H = H; s.W = W;
  return s;
}

PW_API int pw_ray_sweep_count(const float* points, int point_stride, const int32_t* n_pts, int T, int N, int Pmax,
                              const double* view_pose, int H, int W, int64_t* slots, int64_t n_slots, int32_t* block_base,
                              int32_t* view_off, void* stream) {
  CHECK_SWEEP("pw_ray_sweep_count");
  if (slots || n_slots) {                       // slots NULL with n_slots 0: count and scan only, no owners (stage A alone)
    CHECK_SLOTS("pw_ray_sweep_count", (int64_t)T * N * Pmax);
  }
  PW_CHECK_ARG(block_base && view_off, "pw_ray_sweep_count: null pointer");
  const int nblk = (int)pw_cdiv(Pmax, RL_BLOCK);
  PW_CHECK_ARG((int64_t)T * N * nblk < ((int64_t)1 << 31), "pw_ray_sweep_count: too many blocks");
  hipStream_t st = pw_stream(stream);
  if (slots) {
    int rc = fill_slots(slots, n_slots, st);
    if (rc != PW_OK) return rc;
  }
  hipLaunchKernelGGL(k_sweep_count, dim3((unsigned)nblk, (unsigned)N, (unsigned)T), dim3(RL_BLOCK), 0, st,
                     make_sweep(points, point_stride, nullptr, n_pts, N, Pmax, view_pose, H, W), reinterpret_cast<u64*>(slots),
                     (uint32_t)(n_slots - 1), block_base);
  PW_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(RL_BLOCK), 0, st, block_base, T * N * nblk, T * N, nblk, view_off);
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_sweep_count");
  return PW_OK;
}

PW_API int pw_ray_sweep_lists(const float* points, int point_stride, const uint8_t* point_labels, const int32_t* n_pts, int T,
                              int N, int Pmax, const uint8_t* label_lut, const double* view_pose, int H, int W,
                              const int32_t* block_base, int64_t capacity, float* depth_list, float* seg_list, void* stream) {
  CHECK_SWEEP("pw_ray_sweep_lists");
  PW_CHECK_ARG(point_labels && label_lut && block_base && depth_list && seg_list, "pw_ray_sweep_lists: null pointer");
  PW_CHECK_ARG(capacity >= 1, "pw_ray_sweep_lists: capacity must be positive");
  const int nblk = (int)pw_cdiv(Pmax, RL_BLOCK);
  PW_CHECK_ARG((int64_t)T * N * nblk < ((int64_t)1 << 31), "pw_ray_sweep_lists: too many blocks");
  Rows none = make_rows(nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr);
  hipLaunchKernelGGL(k_sweep_emit, dim3((unsigned)nblk, (unsigned)N, (unsigned)T), dim3(RL_BLOCK), 0, pw_stream(stream),
                     make_sweep(points, point_stride, point_labels, n_pts, N, Pmax, view_pose, H, W), label_lut, block_base,
                     (const u64*)nullptr, 0u, depth_list, seg_list, capacity, none, 0);
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_sweep_emit");
  return PW_OK;
}

PW_API int pw_ray_sweep_table(const float* points, int point_stride, const uint8_t* point_labels, const int32_t* n_pts, int T,
                              int N, int Pmax, const uint8_t* label_lut, const double* view_pose, int H, int W,
                              const int64_t* slots, int64_t n_slots, const int32_t* block_base, const uint8_t* frames,
                              int64_t s_f, int64_t s_y, int64_t s_x, int64_t s_c, int n_frames, const int32_t* view_frame,
                              const float* mean_std_host, const float* c2w, const float* K, int64_t capacity, float* rays,
                              int n_cls, int64_t* counts, void* stream) {
  CHECK_SWEEP("pw_ray_sweep_table");
  CHECK_SLOTS("pw_ray_sweep_table", (int64_t)T * N * Pmax);
  PW_CHECK_ARG(point_labels && label_lut && block_base, "pw_ray_sweep_table: null pointer");
  CHECK_ROWS("pw_ray_sweep_table");
  const int nblk = (int)pw_cdiv(Pmax, RL_BLOCK);
  PW_CHECK_ARG((int64_t)T * N * nblk < ((int64_t)1 << 31), "pw_ray_sweep_table: too many blocks");
  hipLaunchKernelGGL(k_sweep_emit, dim3((unsigned)nblk, (unsigned)N, (unsigned)T), dim3(RL_BLOCK), 0, pw_stream(stream),
                     make_sweep(points, point_stride, point_labels, n_pts, N, Pmax, view_pose, H, W), label_lut, block_base,
                     reinterpret_cast<const u64*>(slots), (uint32_t)(n_slots - 1), (float*)nullptr, (float*)nullptr, (int64_t)0,
                     make_rows(frames, s_f, s_y, s_x, s_c, n_frames, view_frame, mean_std_host, c2w, K, capacity, rays, n_cls, counts),
                     1);
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_sweep_emit");
  return PW_OK;
}

PW_API int pw_ray_lists_table(const float* depth_list, const float* seg_list, int64_t n, const int32_t* view_off, int V, int H,
                              int W, int64_t* slots, int64_t n_slots, const uint8_t* frames, int64_t s_f, int64_t s_y,
                              int64_t s_x, int64_t s_c, int n_frames, const int32_t* view_frame, const float* mean_std_host,
                              const float* c2w, const float* K, int64_t capacity, float* rays, int n_cls, int64_t* counts,
                              void* stream) {
  PW_CHECK_ARG(depth_list && seg_list && view_off, "pw_ray_lists_table: null pointer");
  PW_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31) && V >= 1, "pw_ray_lists_table: need 1 <= n < 2^31 and V >= 1");
  PW_CHECK_ARG(H >= 1 && W >= 1 && H <= 32767 && W <= 32767 && (int64_t)V * H * W < 0xffffffffll,
               "pw_ray_lists_table: need 1 <= H, W <= 32767 (pixels are int16) and V H W < 2^32 - 1 (the owner key)");
  CHECK_SLOTS("pw_ray_lists_table", n);
  CHECK_ROWS("pw_ray_lists_table");
  hipStream_t st = pw_stream(stream);
  int rc = fill_slots(slots, n_slots, st);
  if (rc != PW_OK) return rc;
  const unsigned grid = (unsigned)pw_cdiv(n, RL_BLOCK);
  hipLaunchKernelGGL(k_lists_owner, dim3(grid), dim3(RL_BLOCK), 0, st, seg_list, n, view_off, V, H, W, reinterpret_cast<u64*>(slots),
                     (uint32_t)(n_slots - 1));
  PW_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_lists_emit, dim3(grid), dim3(RL_BLOCK), 0, st, depth_list, seg_list, n, view_off, V, H, W,
                     reinterpret_cast<const u64*>(slots), (uint32_t)(n_slots - 1),
                     make_rows(frames, s_f, s_y, s_x, s_c, n_frames, view_frame, mean_std_host, c2w, K, capacity, rays, n_cls, counts));
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_lists_emit");
  return PW_OK;
}

PW_API int pw_ray_table_weights(float* rays, int64_t capacity, const int32_t* view_off, int V, const int32_t* frame_ids,
                                const float* balance_weight, const int64_t* counts, int n_cls, const int32_t* dynamic_class,
                                int n_dyn, float weight_adj, float weight_dyn, float* weights, void* stream) {
  PW_CHECK_ARG(rays && view_off && frame_ids && weights && (balance_weight || counts), "pw_ray_table_weights: null pointer");
  PW_CHECK_ARG(capacity >= 1 && capacity < ((int64_t)1 << 31) && V >= 1 && n_cls >= 1 && n_cls <= 64,
               "pw_ray_table_weights: need 1 <= capacity < 2^31, V >= 1 and 1 <= n_cls <= 64");
  PW_CHECK_ARG(((uintptr_t)rays & 15) == 0, "pw_ray_table_weights: rays must be 16-byte aligned");
  PW_CHECK_ARG(n_dyn >= 0 && (n_dyn == 0 || dynamic_class), "pw_ray_table_weights: dynamic_class is null");
  hipLaunchKernelGGL(k_table_weights, dim3((unsigned)pw_cdiv(capacity, RL_BLOCK)), dim3(RL_BLOCK), 0, pw_stream(stream), rays,
                     capacity, view_off, V, frame_ids, balance_weight, counts, n_cls, dynamic_class, n_dyn, weight_adj, weight_dyn,
                     weights);
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_table_weights");
  return PW_OK;
}
