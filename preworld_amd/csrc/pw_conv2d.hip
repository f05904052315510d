// The stride-1 2-D convolutions of FPN_LSS and DepthNet (include/preworld_hip_conv2d.h) as one templated implicit GEMM over
// channels-last maps:
//     out (B, H, W, Cout) = epi( scale[c] . sum_{taps, ci} x(b, h + dh d, w + dw d, ci) W[c, ci, tap] + shift[c] )
// M = B H W pixels, N = Cout, K = taps x Cin.  It is k_swin_linear (pw_swin_linear_common.h: orientation, tiles, LDS layout, register
// staging, the blocked sum DEEP -- all described in pw_swin_linear.hip) with three changes:
//
// The A operand is gathered.  k runs tap-major, k = tap CinP + ci with CinP = Cin rounded up to 32 (XS), so the 32 consecutive k that
// the 8 threads of a pixel row stage in one pass belong to ONE tap: the tap and its (dh, dw) are wave-uniform scalars, and a thread's
// float4 is x[(m + dh d W + dw d) Cin + ci] or zero -- zero when the row is past M, ci is in the tail Cin .. CinP, or h + dh d / w + dw d
// leaves the map.  A tile of M rows may span row ends and image ends: (h, w) of each staged row are computed once from m, and the test
// is on them, so nothing wraps into the next row or image.  No unfolded or padded copy of x exists.
//
// One power of two per tensor.  A Linear's row scale does not carry over (an output pixel sums nine input pixels), so
// k_conv2d_absmax, a launch of 256 workgroups in front, writes 256 partial maxima of |x| (as bit patterns: a NaN or Inf is above every
// number) into the workspace and every wave of the GEMM folds them -- one 1 KB read -- into e = rng_ideal_exp: x 2^-e is split, the
// epilogue multiplies by 2^e.  Every workgroup writes its word on every call, so there is nothing to clear and nothing survives.
//
// The epilogue is y = (acc 2^e wscale[c]) scale[c] + shift[c] (the parenthesis is exact), then ReLU or + residual and ReLU.  scale and
// shift are the folded eval-mode BatchNorm and bias, computed by the pack launch.
//
// Packed operand: [64 B, zero][wscale CoutP f32][scale CoutP f32][shift CoutP f32][hi plane CoutP x Kp f16][lo plane CoutP x Kp f16],
// Kp = taps CinP, CoutP = Cout rounded up to 64; rows Cout .. CoutP and columns Cin .. CinP of every tap are zero, so weight loads
// need no channel mask; stores and the x gather are masked.
#include "pw_swin_linear_common.h"

namespace {

constexpr int C2_PART = 256;               // partial maxima = workgroups of k_conv2d_absmax = bytes / 4 of the workspace

__host__ __device__ inline int c2_cinp(int Cin) { return (Cin + XS - 1) / XS * XS; }
__host__ __device__ inline int c2_coutp(int Cout) { return (Cout + 63) / 64 * 64; }
__host__ __device__ inline size_t c2_packed_bytes(int Cin, int Cout, int ksize) {
  const size_t np = (size_t)c2_coutp(Cout), kp = (size_t)ksize * ksize * c2_cinp(Cin);
  return (size_t)HDR + 12u * np + 4u * np * kp;
}
struct C2Packed {
  const float* wscale;
  const float* scale;
  const float* shift;
  const unsigned short* plane[2];
};
__host__ __device__ inline C2Packed c2_view(const void* p, int Kp, int Np) {
  const char* c = static_cast<const char*>(p);
  C2Packed v;
  v.wscale = reinterpret_cast<const float*>(c + HDR);
  v.scale = v.wscale + Np;
  v.shift = v.scale + Np;
  v.plane[0] = reinterpret_cast<const unsigned short*>(v.shift + Np);
  v.plane[1] = v.plane[0] + (size_t)Np * Kp;
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- pack
// one wave per packed row n: the row's absmax -> exponent, (hi, lo) of w 2^-e in tap-major order, the undo scale, and the folded
// BatchNorm / bias; rows past Cout are zero
__global__ __launch_bounds__(64) void k_conv2d_pack(const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ g,
                                                    const float* __restrict__ b, const float* __restrict__ mean, const float* __restrict__ var,
                                                    float eps, void* packed, int Cin, int Cout, int T) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int CinP = c2_cinp(Cin), Kp = T * CinP, Np = c2_coutp(Cout);
  const C2Packed p = c2_view(packed, Kp, Np);
  unsigned short* hi = const_cast<unsigned short*>(p.plane[0]) + (size_t)n * Kp;
  unsigned short* lo = const_cast<unsigned short*>(p.plane[1]) + (size_t)n * Kp;
  if (n == 0 && lane < HDR / 4) reinterpret_cast<float*>(packed)[lane] = 0.f;      // every byte of the packed operand is defined
  if (n >= Cout) {
    for (int k = lane; k < Kp; k += 64) hi[k] = lo[k] = 0;
    if (lane == 0) {
      const_cast<float*>(p.wscale)[n] = 1.0f;
      const_cast<float*>(p.scale)[n] = 0.f;
      const_cast<float*>(p.shift)[n] = 0.f;
    }
    return;
  }
  const float* row = w + (size_t)n * Cin * T;         // (Cin, T) as stored
  unsigned bits = 0;
  for (int i = lane; i < Cin * T; i += 64) bits = max(bits, rng_absbits(row[i]));
  const int e = rng_ideal_exp(wave_umax_all(bits));
  const float down = rng_pow2(-e);
  for (int k = lane; k < Kp; k += 64) {
    const int t = k / CinP, ci = k - t * CinP;
    _Float16 h = (_Float16)0.f, l = (_Float16)0.f;
    if (ci < Cin) h2_split1(row[ci * T + t] * down, h, l);
    hi[k] = __builtin_bit_cast(unsigned short, h);
    lo[k] = __builtin_bit_cast(unsigned short, l);
  }
  if (lane == 0) {
    const float bv = bias ? bias[n] : 0.f;
    float sc = 1.0f, sh = bv;
    if (g) {                                          // one lane per row: in double, rounded once each
      const double s = (double)g[n] / sqrt((double)var[n] + (double)eps);
      sc = (float)s;
      sh = (float)((double)b[n] + ((double)bv - (double)mean[n]) * s);
    }
    const_cast<float*>(p.wscale)[n] = rng_pow2(e);
    const_cast<float*>(p.scale)[n] = sc;
    const_cast<float*>(p.shift)[n] = sh;
  }
}

// ---------------------------------------------------------------------------------------------------------------- |x| maxima
// C2_PART workgroups stride over the n4 float4 of x; each writes the bit pattern of its largest |x| (0 where it saw nothing)
__global__ __launch_bounds__(256) void k_conv2d_absmax(const float* __restrict__ x, int64_t n4, unsigned* __restrict__ part) {
  __shared__ unsigned sm[4];
  unsigned bits = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)C2_PART * 256) {
    const v4f v = *reinterpret_cast<const v4f*>(x + 4 * i);
    bits = max(max(bits, rng_absbits(v[0])), max(max(rng_absbits(v[1]), rng_absbits(v[2])), rng_absbits(v[3])));
  }
  bits = wave_umax_all(bits);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = bits;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = max(max(sm[0], sm[1]), max(sm[2], sm[3]));
}

// ---------------------------------------------------------------------------------------------------------------- GEMM
struct C2Args {
  const float* x;
  const void* packed;
  const float* residual;
  const unsigned* part;    // C2_PART partial maxima of |x| (k_conv2d_absmax)
  float* out;
  int M, H, W, Cin, Cout, T, dil, ntn;
};

enum { C2_NONE = PW_CONV2D_EPI_NONE, C2_RELU = PW_CONV2D_EPI_RELU, C2_RES = PW_CONV2D_EPI_RESIDUAL_RELU };

template <int EPI, int TM, int TN, bool DEEP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TM * TN >= 2 ? 2 : 1))) void k_conv2d(const C2Args a) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int RP = BM / 32;                         // pixel rows a thread stages per chunk: rows (tid >> 3) + 32 p
  constexpr int XH = BK / XS;                         // 32-wide k groups per chunk: each lies inside one tap
  constexpr int WL = BN * (BK / 8) / 256;             // 16-byte weight loads per thread, plane and chunk
  __shared__ __attribute__((aligned(16))) unsigned short sX[2][BM * LDS_ROW];
  __shared__ __attribute__((aligned(16))) unsigned short sW[2][BN * LDS_ROW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.M, H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout;
  const int CinP = c2_cinp(Cin), Kp = a.T * CinP, Np = c2_coutp(Cout);
  const unsigned bid = blockIdx.x;
  const int n0 = (int)(bid % (unsigned)a.ntn) * BN;
  const int m0 = (int)(bid / (unsigned)a.ntn) * BM;
  const C2Packed pk = c2_view(a.packed, Kp, Np);
  const int nch = (Kp + BK - 1) / BK;

  // ---- the tensor's power of two
  unsigned mx = 0;
#pragma unroll
  for (int i = 0; i < C2_PART / 64; ++i) mx = max(mx, a.part[lane + 64 * i]);
  const int ex = rng_ideal_exp(wave_umax_all(mx));
  const float a_scale = rng_pow2(-ex), a_undo = rng_pow2(ex);

  // ---- the pixel rows this thread stages
  const int xr = tid >> 3, xk = (tid & 7) * 4;
  int r_h[RP], r_w[RP];
  bool r_ok[RP];
#pragma unroll
  for (int p = 0; p < RP; ++p) {
    const int m = m0 + xr + 32 * p;
    r_ok[p] = m < M;
    const int q = m / W;
    r_w[p] = m - q * W;
    r_h[p] = q % H;
  }

  // ---- chunk staging
  v4f xreg[RP][XH];
  u4v wreg[2][WL];
  auto load_chunk = [&](int c) {
#pragma unroll
    for (int h = 0; h < XH; ++h) {
      const int kb = c * BK + XS * h;                 // wave-uniform: one tap per group
      const int tap = kb / CinP;
      const int ci = kb - tap * CinP + xk;
      int dh = 0, dw = 0;
      if (a.T == 9) {
        const int th = tap / 3;
        dh = (th - 1) * a.dil;
        dw = (tap - 3 * th - 1) * a.dil;
      }
      const bool kok = kb < Kp && ci < Cin;
      const int64_t doff = ((int64_t)dh * W + dw) * Cin + ci;
#pragma unroll
      for (int p = 0; p < RP; ++p) {
        const bool ok = r_ok[p] && kok && (unsigned)(r_h[p] + dh) < (unsigned)H && (unsigned)(r_w[p] + dw) < (unsigned)W;
        const int64_t off = (int64_t)(m0 + xr + 32 * p) * Cin + doff;
        xreg[p][h] = ok ? *reinterpret_cast<const v4f*>(a.x + off) : v4f{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int idx = tid + 256 * i, wr = idx >> 3, wk = c * BK + 8 * (idx & 7);
      const bool ok = n0 + wr < Np && wk < Kp;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
        wreg[pl][i] = ok ? *reinterpret_cast<const u4v*>(pk.plane[pl] + (size_t)(n0 + wr) * Kp + wk) : u4v{0u, 0u, 0u, 0u};
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int h = 0; h < XH; ++h)
#pragma unroll
      for (int p = 0; p < RP; ++p) {
        const int off = (xr + 32 * p) * LDS_ROW + XS * h + xk;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = xreg[p][h][e] * a_scale;      // a masked load is zero and stays zero
        u2 hi, lo;
        h2_split4(v, hi, lo);
        *reinterpret_cast<u2*>(&sX[0][off]) = hi;
        *reinterpret_cast<u2*>(&sX[1][off]) = lo;
      }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int idx = tid + 256 * i;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) *reinterpret_cast<u4v*>(&sW[pl][(idx >> 3) * LDS_ROW + 8 * (idx & 7)]) = wreg[pl][i];
    }
  };

  // ---- the wave's accumulator tiles: rows = channels (A operand), columns = pixels (B operand); DEEP as in k_swin_linear
  const int wm = wave & 1, wn = wave >> 1, lr = lane & 31, lg = lane >> 5;
  constexpr int FLUSH = DEEP_K / BK;
  constexpr int NTOT = DEEP ? TM : 1;
  v16f acc[TN][TM], tot[TN][NTOT];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn)
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        acc[tn][tm][e] = 0.f;
        if (tm < NTOT) tot[tn][tm][e] = 0.f;
      }

  load_chunk(0);
  for (int c = 0; c < nch; ++c) {
    __syncthreads();                                  // the previous chunk's fragment reads are done
    store_chunk();
    __syncthreads();
    if (c + 1 < nch) load_chunk(c + 1);
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      if (c * BK + 16 * ks >= Kp) break;              // Kp % 32 == 0: a k-step is whole or beyond the end
      u4v wf[2][TN], xf[2][TM];
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          wf[pl][tn] = *reinterpret_cast<const u4v*>(&sW[pl][(32 * TN * wn + 32 * tn + lr) * LDS_ROW + 16 * ks + 8 * lg]);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
          xf[pl][tm] = *reinterpret_cast<const u4v*>(&sX[pl][(32 * TM * wm + 32 * tm + lr) * LDS_ROW + 16 * ks + 8 * lg]);
      }
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
          const h8 wh = __builtin_bit_cast(h8, wf[0][tn]), wl = __builtin_bit_cast(h8, wf[1][tn]);
          const h8 xh = __builtin_bit_cast(h8, xf[0][tm]), xl = __builtin_bit_cast(h8, xf[1][tm]);
          acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh, acc[tn][tm], 0, 0, 0);
          acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl, acc[tn][tm], 0, 0, 0);
          acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh, acc[tn][tm], 0, 0, 0);
        }
    }
    if constexpr (DEEP) {
      if ((c & (FLUSH - 1)) == FLUSH - 1 || c + 1 == nch) {
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
          for (int tm = 0; tm < TM; ++tm) {
            tot[tn][tm] += acc[tn][tm];
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[tn][tm][e] = 0.f;
          }
      }
    }
  }

  // ---- epilogue: lane (lr, lg) holds pixel lr, channels 8 j + 4 lg + {0..3} of every tile
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int m = m0 + 32 * TM * wm + 32 * tm + lr;
    if (m >= M) continue;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + 32 * TN * wn + 32 * tn + 8 * j + 4 * lg;
        if (n >= Cout) continue;                      // Cout % 4 == 0: four channels are inside or outside together
        const v4f ws = *reinterpret_cast<const v4f*>(pk.wscale + n);
        const v4f sc = *reinterpret_cast<const v4f*>(pk.scale + n);
        const v4f sh = *reinterpret_cast<const v4f*>(pk.shift + n);
        const int64_t o = (int64_t)m * Cout + n;
        v4f r = {0.f, 0.f, 0.f, 0.f};
        if constexpr (EPI == C2_RES) r = *reinterpret_cast<const v4f*>(a.residual + o);
        v4f y;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float s = (DEEP ? tot[tn][DEEP ? tm : 0][4 * j + e] : acc[tn][tm][4 * j + e]) * (a_undo * ws[e]);
          y[e] = s * sc[e] + sh[e];
          if constexpr (EPI == C2_RES) y[e] += r[e];
          if constexpr (EPI != C2_NONE) y[e] = fmaxf(y[e], 0.f);
        }
        *reinterpret_cast<v4f*>(a.out + o) = y;
      }
  }
}

template <int EPI>
void c2_launch(const C2Args& a, bool large, bool deep, unsigned blocks, hipStream_t st) {
  if (deep) {
    if (large) hipLaunchKernelGGL((k_conv2d<EPI, 2, 1, true>), dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_conv2d<EPI, 1, 1, true>), dim3(blocks), dim3(256), 0, st, a);
  } else {
    if (large) hipLaunchKernelGGL((k_conv2d<EPI, 2, 2, false>), dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_conv2d<EPI, 1, 1, false>), dim3(blocks), dim3(256), 0, st, a);
  }
}

// 0, or PW_EUNSUP with the message set
int c2_check_dims(const char* fn, int Cin, int Cout, int ksize) {
  const int lo = PW_CONV2D_MIN_DIM, hi = PW_CONV2D_MAX_DIM;
  if ((ksize != 1 && ksize != 3) || Cin < lo || Cin > hi || Cin % 4 != 0 || Cout < lo || Cout > hi || Cout % 4 != 0) {
    pw_set_error("%s: Cin = %d, Cout = %d, ksize = %d not supported (ksize 1 or 3, channels multiples of 4 in %d .. %d)", fn, Cin, Cout,
                 ksize, lo, hi);
    return PW_EUNSUP;
  }
  return 0;
}

}  // namespace

PW_API size_t pw_conv2d_packed_bytes(int Cin, int Cout, int ksize) {
  if (c2_check_dims("pw_conv2d_packed_bytes", Cin, Cout, ksize) != 0) return 0;
  return c2_packed_bytes(Cin, Cout, ksize);
}

PW_API int pw_conv2d_pack(const float* weight, const float* bias, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                          const float* bn_var, float bn_eps, void* packed, int Cin, int Cout, int ksize, void* stream) {
  PW_CHECK_ARG(weight && packed, "pw_conv2d_pack: null pointer");
  const int rc = c2_check_dims("pw_conv2d_pack", Cin, Cout, ksize);
  if (rc != 0) return rc;
  const int nbn = (bn_weight != nullptr) + (bn_bias != nullptr) + (bn_mean != nullptr) + (bn_var != nullptr);
  PW_CHECK_ARG(nbn == 0 || nbn == 4, "pw_conv2d_pack: bn_weight, bn_bias, bn_mean and bn_var come together or not at all");
  PW_CHECK_ARG(nbn == 0 || (bn_eps >= 0.f && bn_eps < INFINITY), "pw_conv2d_pack: bn_eps must be finite and non-negative");
  PW_CHECK_ARG(((uintptr_t)packed & 15) == 0 &&
                   (((uintptr_t)weight | (uintptr_t)bias | (uintptr_t)bn_weight | (uintptr_t)bn_bias | (uintptr_t)bn_mean | (uintptr_t)bn_var) & 3) == 0,
               "pw_conv2d_pack: packed must be 16-byte aligned, the float arrays 4-byte aligned");
  hipLaunchKernelGGL(k_conv2d_pack, dim3(c2_coutp(Cout)), dim3(64), 0, pw_stream(stream), weight, bias, bn_weight, bn_bias, bn_mean, bn_var,
                     bn_eps, packed, Cin, Cout, ksize * ksize);
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_conv2d_pack");
  return 0;
}

PW_API size_t pw_conv2d_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  return 4u * (size_t)C2_PART;
}

PW_API int pw_conv2d(const float* x, const void* packed, const float* residual, float* out, float* workspace, size_t workspace_bytes, int B,
                     int H, int W, int Cin, int Cout, int ksize, int dilation, int epi, void* stream) {
  PW_CHECK_ARG(x && packed && out, "pw_conv2d: null pointer");
  const int rc = c2_check_dims("pw_conv2d", Cin, Cout, ksize);
  if (rc != 0) return rc;
  PW_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "pw_conv2d: B, H, W must be positive, got %d, %d, %d", B, H, W);
  const int64_t M64 = (int64_t)B * H * W;
  PW_CHECK_ARG(M64 < ((int64_t)1 << 31) - 128 && M64 * (Cin > Cout ? Cin : Cout) < ((int64_t)1 << 40),
               "pw_conv2d: a (%d, %d, %d) map with %d -> %d channels is too large", B, H, W, Cin, Cout);
  PW_CHECK_ARG(dilation >= 1 && dilation <= 4096, "pw_conv2d: dilation must be in 1 .. 4096, got %d", dilation);
  PW_CHECK_ARG(epi == C2_NONE || epi == C2_RELU || epi == C2_RES, "pw_conv2d: epi must be a PW_CONV2D_EPI_* value, got %d", epi);
  PW_CHECK_ARG((epi == C2_RES) == (residual != nullptr), "pw_conv2d: residual is required for PW_CONV2D_EPI_RESIDUAL_RELU and must be NULL otherwise");
  const size_t need = pw_conv2d_workspace_bytes(B, H, W);
  PW_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0,
               "pw_conv2d: workspace of %zu bytes needed (4-byte aligned), got %zu", need, workspace_bytes);
  PW_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)residual | (uintptr_t)packed) & 15) == 0,
               "pw_conv2d: x, residual, out and packed must be 16-byte aligned");
  PW_CHECK_ARG(x != out, "pw_conv2d: out must not be x (a pixel's neighbours are read after it is written)");
  const int M = (int)M64, Kp = ksize * ksize * c2_cinp(Cin);
  const bool large = pw_cdiv(M, 128) * pw_cdiv(Cout, 128) >= 128;
  const bool deep = Kp > DEEP_K;
  const int bm = large ? 128 : 64, bn = large && !deep ? 128 : 64;
  C2Args a;
  a.x = x; a.packed = packed; a.residual = residual; a.out = out;
  a.part = reinterpret_cast<const unsigned*>(workspace);
  a.M = M; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.T = ksize * ksize; a.dil = dilation;
  a.ntn = (int)pw_cdiv(Cout, bn);
  const int64_t blocks = pw_cdiv(M, bm) * a.ntn;
  PW_CHECK_ARG(blocks < ((int64_t)1 << 31), "pw_conv2d: %lld tiles do not fit one launch", (long long)blocks);
  hipStream_t st = pw_stream(stream);
  hipLaunchKernelGGL(k_conv2d_absmax, dim3(C2_PART), dim3(256), 0, st, x, M64 * Cin / 4, reinterpret_cast<unsigned*>(workspace));
  if (epi == C2_NONE) c2_launch<C2_NONE>(a, large, deep, (unsigned)blocks, st);
  else if (epi == C2_RELU) c2_launch<C2_RELU>(a, large, deep, (unsigned)blocks, st);
  else c2_launch<C2_RES>(a, large, deep, (unsigned)blocks, st);
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_conv2d<%d, %d, %d, %d>", epi, bm / 64, bn / 64, (int)deep);
  return 0;
}
