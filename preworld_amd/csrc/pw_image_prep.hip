// Camera frames to network input: PIL's resize (antialiased bicubic) -> crop -> flip -> rotate (nearest) and mmlabNormalize
// (mmdet3d/datasets/pipelines/loading_traj_temporal.py:173-180, 283-290) for all M frames of a call, gfx950.
//
// Bits.  Up to the uint8 image everything is integer arithmetic on host-built int32 tables (PIL's 22-bit coefficients, its 16.16
// affine), so the bytes do not depend on device floating point; the normalisation is one float subtract and one float multiply
// (this file is compiled with -ffp-contract=off).
//
// k_image_resize: one block per PW_IMAGE_PREP_TH x PW_IMAGE_PREP_TW (32 x 64) tile of the output image.  Only the rows and
// columns the crop keeps are computed.  Horizontal pass: for every source row the tile's band needs (the vertical taps of its
// first to its last row: about 32 scale + 2 support rows, 41 at the test-time 900 -> 792) and every tile column, the taps are
// read from global memory -- lane = column, so a wave reads one ~234-byte stretch of one source row, every byte of it several
// times but from L1 -- and the rounded RGB bytes go to LDS packed into one dword per pixel.  Vertical pass: a thread owns 4
// neighbouring output pixels of one row, reads its taps' dwords from LDS (one 128-bit read per tap when aligned), applies crop
// zero fill and flip, and stores three float4 (one per plane) plus 12 canvas bytes.  Unrotated images are finished here: ONE
// launch, no resized intermediate in global memory.  Images with a rotation store their uint8 window into the workspace instead
// and k_image_rotate gathers from it (nearest, closed form of PIL's running 16.16 sums: integer addition is associative).
//
// What bounds it.  HBM traffic: at the real size (12 frames 900 x 1600 -> 512 x 1408) 52 MB are read and 104 MB written and
// the arithmetic is ~21 integer MACs per horizontal and per vertical pixel, far under the VALU rate those bytes allow.  The
// band overlap makes a block re-read (41 - 32 scale) / 41 = 11 % of its source rows and 5 of 78 source columns, neighbours'
// data that sits in L2.  The horizontal pass reads bytes, not dwords: W * 3 need not be a multiple of 4 and the taps start at
// any byte.  That costs TA issue slots, not HBM bytes; profiles/image_prep.md has the measured share of the HBM rate.
#include "pw_common.h"

namespace {

constexpr int TH = PW_IMAGE_PREP_TH, TW = PW_IMAGE_PREP_TW, NP = PW_IMAGE_PREP_NPARAM;
constexpr int PREC = 22;                       // PIL: PRECISION_BITS = 32 - 8 - 2
constexpr int ROWS_LIMIT = 224;                // 224 * TW * 4 = 56 KiB of LDS

struct Norm {
  float mean[3];
  float stdinv[3];
};

struct Dst {
  float* out;        // (M,3,fH,fW)
  uint8_t* canvas;   // (M,fH,fW,3) or null
  int vec_out;       // float4 stores allowed (fW % 4 == 0, out 16-byte aligned)
  int vec_canvas;    // dword stores allowed
};

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// bytes of 4 neighbouring pixels (packed r | g << 8 | b << 16) as 3 dwords / 12 bytes of an (.., fW, 3) uint8 image
__device__ __forceinline__ void store_rgb4(uint8_t* base, int64_t pix, const uint32_t px[4], int n, bool vec) {
  uint8_t* p = base + pix * 3;
  if (vec && n == 4) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = (px[0] & 0xffffffu) | (px[1] << 24);
    q[1] = ((px[1] >> 8) & 0xffffu) | (px[2] << 16);
    q[2] = ((px[2] >> 16) & 0xffu) | (px[3] << 8);
  } else {
    for (int j = 0; j < n; ++j) {
      p[3 * j + 0] = (uint8_t)(px[j] & 255u);
      p[3 * j + 1] = (uint8_t)((px[j] >> 8) & 255u);
      p[3 * j + 2] = (uint8_t)((px[j] >> 16) & 255u);
    }
  }
}

// normalise and store n <= 4 neighbouring pixels of row oy starting at column ox of image m
__device__ __forceinline__ void emit(const Dst& d, const Norm& nm, int m, int fH, int fW, int oy, int ox, const uint32_t px[4],
                                     int n) {
  const int64_t pix = ((int64_t)m * fH + oy) * fW + ox;
  if (d.canvas) store_rgb4(d.canvas, pix, px, n, d.vec_canvas != 0);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // the reference's to_rgb on an RGB array: plane c takes byte 2 - c
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = ((float)((px[j] >> (8 * (2 - c))) & 255u) - nm.mean[c]) * nm.stdinv[c];
    float* o = d.out + (((int64_t)m * 3 + c) * fH + oy) * fW + ox;
    if (d.vec_out && n == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int j = 0; j < n; ++j) o[j] = v[j];
    }
  }
}

__device__ __forceinline__ bool table_ok(int off, int ks, int n_out, int64_t n_table) {
  return n_out > 0 && ks > 0 && off >= 0 && (int64_t)off + (int64_t)(2 + ks) * n_out <= n_table;
}

__global__ __launch_bounds__(256) void k_image_resize(const uint8_t* __restrict__ src, int H, int W, int fH, int fW,
                                                      const int32_t* __restrict__ params, const int32_t* __restrict__ tables,
                                                      int64_t n_table, int rows_max, uint8_t* __restrict__ inter, int vec_inter,
                                                      Dst dst, Norm nm) {
  extern __shared__ __align__(16) uint32_t tile[];   // [R][TW], r | g << 8 | b << 16 after the horizontal pass; read as uint4
  const int m = blockIdx.z;
  const int32_t* P = params + (int64_t)m * NP;
  const int newW = P[0], newH = P[1], x0 = P[2], y0 = P[3], flip = P[4], rot = P[5];
  const int hoff = P[12], hks = P[13], voff = P[14], vks = P[15];
  const bool ok = table_ok(hoff, hks, newW, n_table) && table_ok(voff, vks, newH, n_table);
  const int32_t* hb = tables + hoff;
  const int32_t* hk = hb + 2 * (int64_t)newW;
  const int32_t* vb = tables + voff;
  const int32_t* vk = vb + 2 * (int64_t)newH;

  const int oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;
  const int th = min(TH, fH - oy0), tw = min(TW, fW - ox0);
  const int cx0 = flip ? fW - ox0 - tw : ox0;  // left column of the tile in crop space (before the flip)
  const int ry_a = max(oy0 + y0, 0), ry_b = min(oy0 + th - 1 + y0, newH - 1);
  const int rx_a = max(cx0 + x0, 0), rx_b = min(cx0 + tw - 1 + x0, newW - 1);
  int srow_lo = 0, R = 0;
  if (ok && ry_a <= ry_b && rx_a <= rx_b) {
    srow_lo = min(max(vb[2 * ry_a], 0), H);
    const int srow_hi = min(max(vb[2 * ry_b] + vb[2 * ry_b + 1], 0), H);
    R = min(max(srow_hi - srow_lo, 0), rows_max);
  }

  // horizontal pass: source rows srow_lo .. srow_lo + R - 1, tile columns 0 .. TW - 1
  for (int idx = threadIdx.x; idx < R * TW; idx += 256) {
    const int r = idx / TW, c = idx % TW;
    const int rx = cx0 + c + x0;
    uint32_t packed = 0;
    if (c < tw && rx >= 0 && rx < newW) {
      const int lo = min(max(hb[2 * rx], 0), W);
      const int n = min(min(hb[2 * rx + 1], hks), W - lo);
      const int32_t* k = hk + (int64_t)rx * hks;
      const uint8_t* p = src + (((int64_t)m * H + srow_lo + r) * W + lo) * 3;
      int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
      for (int t = 0; t < n; ++t) {
        const int w = k[t];
        a0 += (int)p[3 * t + 0] * w;
        a1 += (int)p[3 * t + 1] * w;
        a2 += (int)p[3 * t + 2] * w;
      }
      packed = (uint32_t)clip8(a0) | ((uint32_t)clip8(a1) << 8) | ((uint32_t)clip8(a2) << 16);
    }
    tile[idx] = packed;
  }
  __syncthreads();

  // vertical pass + crop fill + flip + normalise: a unit is 4 neighbouring output pixels of one row
  for (int u = threadIdx.x; u < TH * (TW / 4); u += 256) {
    const int yy = u / (TW / 4), xq = u % (TW / 4);
    const int oy = oy0 + yy, ox = ox0 + 4 * xq;
    if (yy >= th || ox >= fW) continue;
    const int n_px = min(4, fW - ox);
    const int ry = oy + y0;
    uint32_t px[4] = {0u, 0u, 0u, 0u};
    if (ok && ry >= 0 && ry < newH && R > 0) {
      const int rel = vb[2 * ry] - srow_lo;
      int n = min(vb[2 * ry + 1], vks);
      if (rel < 0) n = 0;
      n = min(n, R - rel);
      const int32_t* k = vk + (int64_t)ry * vks;
      // crop-space columns of the unit, ascending: cmin .. cmin + 3 (relative to the tile); output pixel j reads
      // q[flip ? 3 - j : j]
      const int cmin = flip ? tw - 4 - 4 * xq : 4 * xq;
      int acc[4][3];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (PREC - 1);
      const bool aligned = cmin >= 0 && (cmin & 3) == 0;
      for (int t = 0; t < n; ++t) {
        const int w = k[t];
        const uint32_t* row = tile + (rel + t) * TW;
        uint32_t q[4];
        if (aligned) {
          const uint4 v = *reinterpret_cast<const uint4*>(row + cmin);
          q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) q[j] = (cmin + j >= 0 && cmin + j < TW) ? row[cmin + j] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[j][0] += (int)(q[j] & 255u) * w;
          acc[j][1] += (int)((q[j] >> 8) & 255u) * w;
          acc[j][2] += (int)((q[j] >> 16) & 255u) * w;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int qi = flip ? 3 - j : j;
        const int rx = cx0 + cmin + qi + x0;
        const bool in = cmin + qi >= 0 && cmin + qi < tw && rx >= 0 && rx < newW;
        px[j] = in ? ((uint32_t)clip8(acc[qi][0]) | ((uint32_t)clip8(acc[qi][1]) << 8) | ((uint32_t)clip8(acc[qi][2]) << 16)) : 0u;
      }
    }
    if (rot) {
      if (inter) store_rgb4(inter, ((int64_t)m * fH + oy) * fW + ox, px, n_px, vec_inter != 0);
    } else {
      emit(dst, nm, m, fH, fW, oy, ox, px, n_px);
    }
  }
}

// PIL's affine_fixed (nearest): output (x, y) <- input ((a2 + a1 y + a0 x) >> 16, (a5 + a4 y + a3 x) >> 16), 0 outside
__global__ __launch_bounds__(256) void k_image_rotate(const uint8_t* __restrict__ inter, int fH, int fW,
                                                      const int32_t* __restrict__ params, Dst dst, Norm nm) {
  const int m = blockIdx.y;
  const int32_t* P = params + (int64_t)m * NP;
  if (!P[5]) return;
  const int units_x = (fW + 3) / 4;
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= (int64_t)units_x * fH) return;
  const int oy = (int)(u / units_x), ox = 4 * (int)(u % units_x);
  const int n_px = min(4, fW - ox);
  const uint32_t a0 = (uint32_t)P[6], a1 = (uint32_t)P[7], a2 = (uint32_t)P[8];
  const uint32_t a3 = (uint32_t)P[9], a4 = (uint32_t)P[10], a5 = (uint32_t)P[11];
  uint32_t px[4] = {0u, 0u, 0u, 0u};
  for (int j = 0; j < n_px; ++j) {
    const uint32_t x = (uint32_t)(ox + j), y = (uint32_t)oy;
    const int xin = (int)(a2 + a1 * y + a0 * x) >> 16;    // wraps like PIL's int sums; the shift is arithmetic
    const int yin = (int)(a5 + a4 * y + a3 * x) >> 16;
    if (xin >= 0 && xin < fW && yin >= 0 && yin < fH) {
      const uint8_t* p = inter + (((int64_t)m * fH + yin) * fW + xin) * 3;
      px[j] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
  }
  emit(dst, nm, m, fH, fW, oy, ox, px, n_px);
}

}  // namespace

PW_API size_t pw_image_prep_ws_bytes(int M, int fH, int fW, int any_rot) {
  if (!any_rot || M <= 0 || fH <= 0 || fW <= 0) return 0;
  return pw_align_up((size_t)M * (size_t)fH * (size_t)fW * 3, 256);
}

PW_API int pw_image_prep(const uint8_t* src, int M, int H, int W, int fH, int fW, const int32_t* params, const int32_t* tables,
                         int64_t n_table, int rows_max, int any_rot, void* ws, float* out, uint8_t* canvas, int* launches_host,
                         void* stream) {
  PW_CHECK_ARG(src && params && tables && out, "pw_image_prep: null pointer");
  PW_CHECK_ARG(M >= 1 && M <= 65535, "pw_image_prep: need 1 <= M <= 65535 images");
  PW_CHECK_ARG(H >= 1 && W >= 1 && H <= 32767 && W <= 32767, "pw_image_prep: source size must be 1 .. 32767 (PIL's fixed-point range)");
  PW_CHECK_ARG(fH >= 1 && fW >= 1 && fH <= 32767 && fW <= 32767, "pw_image_prep: input_size must be 1 .. 32767");
  PW_CHECK_ARG(n_table >= 1 && n_table < ((int64_t)1 << 31), "pw_image_prep: need 1 <= n_table < 2^31");
  PW_CHECK_ARG(rows_max >= 1 && rows_max <= ROWS_LIMIT, "pw_image_prep: need 1 <= rows_max <= 224 (the band of source rows is staged in LDS)");
  PW_CHECK_ARG(!any_rot || ws, "pw_image_prep: a call with rotated images needs the workspace");
  PW_CHECK_ARG(((uintptr_t)out & 3) == 0, "pw_image_prep: out must be 4-byte aligned");
  hipStream_t st = pw_stream(stream);
  Norm nm;
  const float mean[3] = {123.675f, 116.28f, 103.53f}, stdv[3] = {58.395f, 57.12f, 57.375f};
  for (int c = 0; c < 3; ++c) {
    nm.mean[c] = mean[c];
    nm.stdinv[c] = (float)(1.0 / (double)stdv[c]);
  }
  Dst dst;
  dst.out = out;
  dst.canvas = canvas;
  dst.vec_out = (fW % 4 == 0) && ((uintptr_t)out & 15) == 0;
  dst.vec_canvas = (fW % 4 == 0) && ((uintptr_t)canvas & 3) == 0;
  uint8_t* inter = any_rot ? reinterpret_cast<uint8_t*>(ws) : nullptr;
  const int vec_inter = (fW % 4 == 0) && ((uintptr_t)inter & 3) == 0;
  int launches = 0;
  const dim3 grid((unsigned)pw_cdiv(fW, TW), (unsigned)pw_cdiv(fH, TH), (unsigned)M);
  hipLaunchKernelGGL(k_image_resize, grid, dim3(256), (size_t)rows_max * TW * sizeof(uint32_t), st, src, H, W, fH, fW, params,
                     tables, n_table, rows_max, inter, vec_inter, dst, nm);
  PW_CHECK_LAUNCH();
  ++launches;
  pw_note_kernel("k_image_resize");
  if (any_rot) {
    const int64_t units = pw_cdiv(fW, 4) * fH;
    hipLaunchKernelGGL(k_image_rotate, dim3((unsigned)pw_cdiv(units, 256), (unsigned)M), dim3(256), 0, st, inter, fH, fW, params,
                       dst, nm);
    pw_note_kernel("k_image_rotate");
    PW_CHECK_LAUNCH();
    ++launches;
  }
  if (launches_host) *launches_host = launches;
  return PW_OK;
}
