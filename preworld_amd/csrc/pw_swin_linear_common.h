// The GEMM template of the Swin block Linears, shared by pw_swin_linear.hip (forward) and pw_swin_linear_bwd.hip (the data and GELU
// gradients are the same GEMM with another operand or epilogue).  Layout, tiles and modes are described in pw_swin_linear.hip.
#ifndef PW_SWIN_LINEAR_COMMON_H_
#define PW_SWIN_LINEAR_COMMON_H_
#include "pw_h2.h"

namespace {

typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf4 __attribute__((ext_vector_type(4)));

constexpr int BK = 64;                 // k per chunk
constexpr int XS = 32;                 // k one pass of the 8 threads of a token row covers (4 each)
constexpr int LDS_ROW = 72;            // halves per LDS row: 64 + 8 of padding = 144 bytes
constexpr int DEEP_K = 1024;           // F32 mode: a longer K is summed in blocks of this many (k_swin_linear, DEEP)
constexpr int HDR = 64;                // bytes of the packed header: float a_scale, float a_unscale

// the packed operand: [HDR][wscale N f32][bias N f32][gamma K f32][beta K f32][planes x N x K 16-bit]
struct Packed {
  const float* hdr;
  const float* wscale;
  const float* bias;
  const float* gamma;
  const float* beta;
  const unsigned short* plane[2];
};
__host__ __device__ inline size_t packed_bytes(int K, int N, int planes) {
  return (size_t)HDR + 8u * (size_t)N + 8u * (size_t)K + (size_t)planes * 2u * (size_t)N * (size_t)K;
}
__host__ __device__ inline Packed packed_view(const void* p, int K, int N) {
  const char* c = static_cast<const char*>(p);
  Packed v;
  v.hdr = reinterpret_cast<const float*>(c);
  v.wscale = reinterpret_cast<const float*>(c + HDR);
  v.bias = v.wscale + N;
  v.gamma = v.bias + N;
  v.beta = v.gamma + K;
  v.plane[0] = reinterpret_cast<const unsigned short*>(v.beta + K);
  v.plane[1] = v.plane[0] + (size_t)N * K;
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
// the largest |bit pattern|: a NaN or Inf pattern is above every number, so it survives the maximum
__device__ __forceinline__ unsigned wave_umax_all(unsigned v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- pack
// one wave per weight row: absmax -> exponent, (hi, lo) of w 2^-e (bf16: the rounded weight), the undo scale and the bias
template <bool BF>
__global__ __launch_bounds__(64) void k_swin_linear_pack_rows(const float* __restrict__ w, const float* __restrict__ bias, void* packed,
                                                              int K, int N) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const Packed p = packed_view(packed, K, N);
  const float* row = w + (size_t)n * K;
  unsigned short* hi = const_cast<unsigned short*>(p.plane[0]) + (size_t)n * K;
  if constexpr (BF) {
    for (int k = lane; k < K; k += 64) hi[k] = __builtin_bit_cast(unsigned short, (__bf16)row[k]);
    if (lane == 0) const_cast<float*>(p.wscale)[n] = 1.0f;
  } else {
    unsigned short* lo = const_cast<unsigned short*>(p.plane[1]) + (size_t)n * K;
    unsigned bits = 0;
    for (int k = lane; k < K; k += 64) bits = max(bits, rng_absbits(row[k]));
    const int e = rng_ideal_exp(wave_umax_all(bits));
    const float down = rng_pow2(-e);
    for (int k = lane; k < K; k += 64) {
      _Float16 h, l;
      h2_split1(row[k] * down, h, l);
      hi[k] = __builtin_bit_cast(unsigned short, h);
      lo[k] = __builtin_bit_cast(unsigned short, l);
    }
    if (lane == 0) const_cast<float*>(p.wscale)[n] = rng_pow2(e);
  }
  if (lane == 0) const_cast<float*>(p.bias)[n] = bias ? bias[n] : 0.0f;
}

// one workgroup: gamma, beta (1, 0 without a LayerNorm) and the power of two of the LayerNorm operand's bound
template <bool BF>
__global__ __launch_bounds__(256) void k_swin_linear_pack_ln(const float* __restrict__ g, const float* __restrict__ b, void* packed, int K,
                                                             int N) {
  __shared__ float sm[8];
  const Packed p = packed_view(packed, K, N);
  float mg = 0.f, mb = 0.f;
  bool bad = false;
  for (int k = threadIdx.x; k < K; k += 256) {
    const float gv = g ? g[k] : 1.0f, bv = b ? b[k] : 0.0f;
    const_cast<float*>(p.gamma)[k] = gv;
    const_cast<float*>(p.beta)[k] = bv;
    mg = fmaxf(mg, fabsf(gv));
    mb = fmaxf(mb, fabsf(bv));
    bad |= !(fabsf(gv) < INFINITY) || !(fabsf(bv) < INFINITY);
  }
  mg = wave_max(mg);
  mb = wave_max(mb);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[wave] = mg;
    sm[4 + wave] = bad ? INFINITY : mb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mg = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    mb = fmaxf(fmaxf(sm[4], sm[5]), fmaxf(sm[6], sm[7]));
    // |x_hat| <= sqrt(K - 1) < sqrt(K) for the biased variance; a non-finite gamma or beta takes exponent 0 and propagates
    const float bound = sqrtf((float)K) * mg + mb;
    const int e = BF ? 0 : rng_ideal_exp(rng_absbits(bound));
    float* hdr = const_cast<float*>(p.hdr);
    hdr[0] = rng_pow2(-e);
    hdr[1] = rng_pow2(e);
    for (int i = 2; i < HDR / 4; ++i) hdr[i] = 0.f;      // every byte of the packed operand is defined
  }
}

// ---------------------------------------------------------------------------------------------------------------- row statistics
// LPR lanes per token row, 64 / LPR rows per wave.  LN: mean, then the biased variance around it (two passes: the second finds the
// row in cache), written as (mean, 1 / sqrt(var + eps)).  Otherwise: the row's absmax -> e = rng_ideal_exp, written as (2^-e, 2^e);
// e = 0 for an all-zero row and for a row holding Inf or NaN (its bit pattern is above every number's).
template <bool LN, int LPR>
__global__ __launch_bounds__(256) void k_swin_linear_stats(const float* __restrict__ x, float* __restrict__ stats, int64_t M, int K,
                                                           float eps) {
  const int sub = threadIdx.x % LPR;
  const int64_t m = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const bool ok = m < M;                              // no early return: the shuffles below take every lane of the wave
  const float* row = x + (ok ? m : 0) * K;
  float o0, o1;
  if constexpr (LN) {
    float s = 0.f;
    if (ok)
      for (int k = 4 * sub; k < K; k += 4 * LPR) {
        const v4f v = *reinterpret_cast<const v4f*>(row + k);
        s += (v[0] + v[1]) + (v[2] + v[3]);
      }
#pragma unroll
    for (int o = LPR / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)K;
    float q = 0.f;
    if (ok)
      for (int k = 4 * sub; k < K; k += 4 * LPR) {
        const v4f v = *reinterpret_cast<const v4f*>(row + k) - mean;
        q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
      }
#pragma unroll
    for (int o = LPR / 2; o >= 1; o >>= 1) q += __shfl_xor(q, o);
    o0 = mean;
    o1 = 1.0f / sqrtf(q / (float)K + eps);
  } else {
    unsigned bits = 0;
    if (ok)
      for (int k = 4 * sub; k < K; k += 4 * LPR) {
        const v4f v = *reinterpret_cast<const v4f*>(row + k);
        bits = max(max(bits, rng_absbits(v[0])), max(max(rng_absbits(v[1]), rng_absbits(v[2])), rng_absbits(v[3])));
      }
#pragma unroll
    for (int o = LPR / 2; o >= 1; o >>= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, o));
    const int e = rng_ideal_exp(bits);
    o0 = rng_pow2(-e);
    o1 = rng_pow2(e);
  }
  if (ok && sub == 0) *reinterpret_cast<h2_f2*>(stats + 2 * m) = h2_f2{o0, o1};
}

// ---------------------------------------------------------------------------------------------------------------- GEMM
struct LinArgs {
  const void* x;
  const void* packed;
  const float* residual;
  const float* stats;      // (M, 2): LayerNorm (mean, 1 / sigma); F32 mode without it (2^-e, 2^e) of the row; unused otherwise
  void* out;
  int64_t M;
  int K, N, ntn;
  float eps;
};

// EPI_DGELU is internal to the backward (pw_swin_linear_bwd.hip): out = residual o gelu'(y), `residual` being the hidden tensor's
// gradient; pw_swin_linear refuses it
enum { EPI_BIAS = PW_SWIN_LINEAR_EPI_BIAS, EPI_GELU = PW_SWIN_LINEAR_EPI_GELU, EPI_RES = PW_SWIN_LINEAR_EPI_RESIDUAL, EPI_DGELU = 3 };

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
// d/dy of gelu_erf: Phi(y) + y phi(y)
__device__ __forceinline__ float gelu_erf_grad(float v) {
  return 0.5f * (1.0f + erff(v * 0.70710678118654752440f)) + v * expf(-0.5f * v * v) * 0.39894228040143267794f;
}

// four consecutive k of one token row, as loaded: float4, or (BF16 mode without LayerNorm) four bf16 in two words
template <bool XBF>
struct XChunk;
template <>
struct XChunk<false> {
  v4f v;
  __device__ __forceinline__ void load(const void* x, int64_t off, bool ok) {
    v = ok ? *reinterpret_cast<const v4f*>(static_cast<const float*>(x) + off) : v4f{0.f, 0.f, 0.f, 0.f};
  }
};
template <>
struct XChunk<true> {
  u2 v;
  __device__ __forceinline__ void load(const void* x, int64_t off, bool ok) {
    v = ok ? *reinterpret_cast<const u2*>(static_cast<const unsigned short*>(x) + off) : u2{0u, 0u};
  }
};

// two workgroups per CU (one wave of each per SIMD) is what overlaps one workgroup's barriers and staging with the other's MFMAs:
// the large tiles are held to the 256 registers that allows
template <bool BF, bool LN, int EPI, int TM, int TN, bool DEEP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TM * TN >= 2 ? 2 : 1))) void k_swin_linear(const LinArgs a) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int PL = BF ? 1 : 2;                      // 16-bit planes per operand
  constexpr bool XBF = BF && !LN;                     // x is bfloat16
  constexpr bool OBF = BF && EPI != EPI_RES;          // out is bfloat16
  constexpr int RP = BM / 32;                         // token rows a thread stages per chunk: rows (tid >> 3) + 32 p
  constexpr int XH = BK / XS;                         // 4-element groups of one token row a thread stages per chunk
  constexpr int WL = BN * (BK / 8) / 256;             // 16-byte weight loads per thread, plane and chunk
  __shared__ __attribute__((aligned(16))) unsigned short sX[PL][BM * LDS_ROW];
  __shared__ __attribute__((aligned(16))) unsigned short sW[PL][BN * LDS_ROW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, N = a.N;
  const int64_t M = a.M;
  const unsigned bid = blockIdx.x;
  const int n0 = (int)(bid % (unsigned)a.ntn) * BN;
  const int64_t m0 = (int64_t)(bid / (unsigned)a.ntn) * BM;
  const Packed pk = packed_view(a.packed, K, N);
  const int nch = (K + BK - 1) / BK;

  // ---- the rows this thread stages, their statistics (k_swin_linear_stats)
  const int xr = tid >> 3, xk = (tid & 7) * 4;
  float r_mean[RP], r_mul[RP];                        // LN: mean, 1 / sigma; otherwise: -, the row's down-scale 2^-e
  bool r_ok[RP];
#pragma unroll
  for (int p = 0; p < RP; ++p) {
    const int64_t m = m0 + xr + 32 * p;
    r_ok[p] = m < M;
    r_mean[p] = 0.f;
    r_mul[p] = 1.f;
    if constexpr (LN || !BF) {
      if (r_ok[p]) {
        const h2_f2 st = *reinterpret_cast<const h2_f2*>(a.stats + 2 * m);
        r_mean[p] = LN ? st[0] : 0.f;
        r_mul[p] = LN ? st[1] : st[0];
      }
    }
  }
  const float a_scale = (LN && !BF) ? pk.hdr[0] : 1.0f;
  const float a_undo = (LN && !BF) ? pk.hdr[1] : 1.0f;

  // ---- chunk staging
  XChunk<XBF> xreg[RP][XH];
  u4v wreg[PL][WL];
  auto load_chunk = [&](int c) {
#pragma unroll
    for (int h = 0; h < XH; ++h) {
      const int k = c * BK + XS * h + xk;
#pragma unroll
      for (int p = 0; p < RP; ++p) xreg[p][h].load(a.x, (m0 + xr + 32 * p) * K + k, r_ok[p] && k < K);
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int idx = tid + 256 * i, wr = idx >> 3, wk = c * BK + 8 * (idx & 7);
      const bool ok = n0 + wr < N && wk < K;
#pragma unroll
      for (int pl = 0; pl < PL; ++pl)
        wreg[pl][i] = ok ? *reinterpret_cast<const u4v*>(pk.plane[pl] + (size_t)(n0 + wr) * K + wk) : u4v{0u, 0u, 0u, 0u};
    }
  };
  auto store_chunk = [&](int c) {
#pragma unroll
    for (int h = 0; h < XH; ++h) {
      const int k = c * BK + XS * h + xk;
      const bool kok = k < K;
      v4f g = {1.f, 1.f, 1.f, 1.f}, b = {0.f, 0.f, 0.f, 0.f};
      if constexpr (LN) {
        if (kok) {
          g = *reinterpret_cast<const v4f*>(pk.gamma + k);
          b = *reinterpret_cast<const v4f*>(pk.beta + k);
        }
      }
#pragma unroll
      for (int p = 0; p < RP; ++p) {
        const int off = (xr + 32 * p) * LDS_ROW + XS * h + xk;
        if constexpr (XBF) {
          *reinterpret_cast<u2*>(&sX[0][off]) = xreg[p][h].v;
        } else {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if constexpr (LN)
              v[e] = ((xreg[p][h].v[e] - r_mean[p]) * r_mul[p] * g[e] + b[e]) * a_scale;
            else
              v[e] = xreg[p][h].v[e] * r_mul[p];
            if (!(r_ok[p] && kok)) v[e] = 0.f;
          }
          if constexpr (BF) {
            const bf4 hv = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
            *reinterpret_cast<u2*>(&sX[0][off]) = __builtin_bit_cast(u2, hv);
          } else {
            u2 hi, lo;
            h2_split4(v, hi, lo);
            *reinterpret_cast<u2*>(&sX[0][off]) = hi;
            *reinterpret_cast<u2*>(&sX[PL - 1][off]) = lo;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int idx = tid + 256 * i;
#pragma unroll
      for (int pl = 0; pl < PL; ++pl) *reinterpret_cast<u4v*>(&sW[pl][(idx >> 3) * LDS_ROW + 8 * (idx & 7)]) = wreg[pl][i];
    }
  };

  // ---- the wave's accumulator tiles: rows = channels (A operand), columns = tokens (B operand)
  const int wm = wave & 1, wn = wave >> 1, lr = lane & 31, lg = lane >> 5;
  // DEEP (F32 mode, K > DEEP_K) sums in blocks of FLUSH chunks: the accumulator is rounded three times per k-step, and over
  // K = 4096 one chain of 768 roundings at the magnitude of the result costs more than the fp32 library GEMM's own error (measured:
  // 1.11e-6 of max |out| against a bound of 1.0e-6); a block's partial sum is small while it is rounded often, and the total is
  // rounded once per block.  The second accumulator set is why the DEEP throughput tile is 128 x 64.
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
    store_chunk(c);
    __syncthreads();
    if (c + 1 < nch) load_chunk(c + 1);
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      if (c * BK + 16 * ks >= K) break;               // K % 16 == 0: a k-step is whole or beyond the end
      u4v wf[PL][TN], xf[PL][TM];
#pragma unroll
      for (int pl = 0; pl < PL; ++pl) {
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
          if constexpr (BF) {
            acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, wf[0][tn]), __builtin_bit_cast(bf8, xf[0][tm]),
                                                                  acc[tn][tm], 0, 0, 0);
          } else {
            const h8 wh = __builtin_bit_cast(h8, wf[0][tn]), wl = __builtin_bit_cast(h8, wf[PL - 1][tn]);
            const h8 xh = __builtin_bit_cast(h8, xf[0][tm]), xl = __builtin_bit_cast(h8, xf[PL - 1][tm]);
            acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh, acc[tn][tm], 0, 0, 0);
            acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl, acc[tn][tm], 0, 0, 0);
            acc[tn][tm] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh, acc[tn][tm], 0, 0, 0);
          }
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

  // ---- epilogue: lane (lr, lg) holds token lr, channels 8 j + 4 lg + {0..3} of every tile
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int ml = 32 * TM * wm + 32 * tm + lr;
    const int64_t m = m0 + ml;
    if (m >= M) continue;
    float undo = a_undo;
    if constexpr (!LN && !BF) undo = a.stats[2 * m + 1];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + 32 * TN * wn + 32 * tn + 8 * j + 4 * lg;
        if (n >= N) continue;
        const v4f bias = *reinterpret_cast<const v4f*>(pk.bias + n);
        v4f ws = {1.f, 1.f, 1.f, 1.f};
        if constexpr (!BF) ws = *reinterpret_cast<const v4f*>(pk.wscale + n);
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          y[e] = (DEEP ? tot[tn][DEEP ? tm : 0][4 * j + e] : acc[tn][tm][4 * j + e]) * (undo * ws[e]) + bias[e];
          if constexpr (EPI == EPI_GELU) y[e] = gelu_erf(y[e]);
        }
        const int64_t o = m * N + n;
        if constexpr (EPI == EPI_RES) {
          const v4f r = *reinterpret_cast<const v4f*>(a.residual + o);
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = r[e] + y[e];
        }
        if constexpr (EPI == EPI_DGELU) {             // out may be `residual` itself: a lane reads its four values, then writes them
          const v4f r = *reinterpret_cast<const v4f*>(a.residual + o);
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = r[e] * gelu_erf_grad(y[e]);
        }
        if constexpr (OBF) {
          const bf4 h = {(__bf16)y[0], (__bf16)y[1], (__bf16)y[2], (__bf16)y[3]};
          *reinterpret_cast<u2*>(static_cast<unsigned short*>(a.out) + o) = __builtin_bit_cast(u2, h);
        } else {
          *reinterpret_cast<v4f*>(static_cast<float*>(a.out) + o) = v4f{y[0], y[1], y[2], y[3]};
        }
      }
  }
}

template <bool BF, bool LN, int EPI>
void launch_tile(const LinArgs& a, bool large, bool deep, unsigned blocks, hipStream_t st) {
  if constexpr (!BF) {
    if (deep) {
      if (large)
        hipLaunchKernelGGL((k_swin_linear<BF, LN, EPI, 2, 1, true>), dim3(blocks), dim3(256), 0, st, a);
      else
        hipLaunchKernelGGL((k_swin_linear<BF, LN, EPI, 1, 1, true>), dim3(blocks), dim3(256), 0, st, a);
      return;
    }
  }
  if (large)
    hipLaunchKernelGGL((k_swin_linear<BF, LN, EPI, 2, 2, false>), dim3(blocks), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((k_swin_linear<BF, LN, EPI, 1, 1, false>), dim3(blocks), dim3(256), 0, st, a);
}
template <bool BF, bool LN>
void launch_epi(const LinArgs& a, int epi, bool large, bool deep, unsigned blocks, hipStream_t st) {
  if (epi == EPI_BIAS) launch_tile<BF, LN, EPI_BIAS>(a, large, deep, blocks, st);
  else if (epi == EPI_GELU) launch_tile<BF, LN, EPI_GELU>(a, large, deep, blocks, st);
  else launch_tile<BF, LN, EPI_RES>(a, large, deep, blocks, st);
}

// The two launches of pw_swin_linear for a caller that has checked its arguments: the row statistics into `workspace` (where the mode
// has any), then the GEMM.  The 128 x 128 tile unless it would leave half of the 256 CUs without a workgroup.  BWD adds EPI_DGELU
// (float32, LayerNorm prologue), which only pw_swin_linear_bwd.hip instantiates.  False if the tiles do not fit one launch.
template <bool BWD>
bool run_linear(const void* x, const void* packed, const float* residual, void* out, float* workspace, bool stats, int64_t M, int K, int N,
                bool ln, float eps, int epi, bool bf, hipStream_t st, const char* note) {
  const int64_t big = pw_cdiv(M, 128) * pw_cdiv(N, 128);
  const bool large = big >= 128;
  const bool deep = !bf && K > DEEP_K;
  const int bm = large ? 128 : 64, bn = large && !deep ? 128 : 64;
  LinArgs a;
  a.x = x; a.packed = packed; a.residual = residual; a.out = out; a.stats = workspace;
  a.M = M; a.K = K; a.N = N; a.ntn = (int)pw_cdiv(N, bn);
  a.eps = eps;
  const int64_t blocks = pw_cdiv(M, bm) * a.ntn;
  if (!(blocks < ((int64_t)1 << 31) && M < ((int64_t)1 << 32))) return false;
  if (stats) {                                        // one lane group per row: 8 lanes for short rows, a wave for long ones
    const float* xf = static_cast<const float*>(x);
    if (K >= 512) {
      if (ln) hipLaunchKernelGGL((k_swin_linear_stats<true, 64>), dim3((unsigned)pw_cdiv(M, 4)), dim3(256), 0, st, xf, workspace, M, K, eps);
      else hipLaunchKernelGGL((k_swin_linear_stats<false, 64>), dim3((unsigned)pw_cdiv(M, 4)), dim3(256), 0, st, xf, workspace, M, K, eps);
    } else {
      if (ln) hipLaunchKernelGGL((k_swin_linear_stats<true, 8>), dim3((unsigned)pw_cdiv(M, 32)), dim3(256), 0, st, xf, workspace, M, K, eps);
      else hipLaunchKernelGGL((k_swin_linear_stats<false, 8>), dim3((unsigned)pw_cdiv(M, 32)), dim3(256), 0, st, xf, workspace, M, K, eps);
    }
  }
  if constexpr (BWD) {                                // float32 only: the GELU gradient, or the plain GEMM of the data gradient
    if (epi == EPI_DGELU) launch_tile<false, true, EPI_DGELU>(a, large, deep, (unsigned)blocks, st);
    else launch_tile<false, false, EPI_BIAS>(a, large, deep, (unsigned)blocks, st);
  } else if (bf) {
    if (ln) launch_epi<true, true>(a, epi, large, deep, (unsigned)blocks, st);
    else launch_epi<true, false>(a, epi, large, deep, (unsigned)blocks, st);
  } else {
    if (ln) launch_epi<false, true>(a, epi, large, deep, (unsigned)blocks, st);
    else launch_epi<false, false>(a, epi, large, deep, (unsigned)blocks, st);
  }
  if (note) pw_note_kernel(note, (int)bf, ln ? 1 : 0, epi, bm / 64, bn / 64, (int)deep);
  return true;
}

// shared by the entry points: 0, or PW_EUNSUP with the message set
int check_dims(const char* fn, int K, int N, int dtype) {
  if (dtype != PW_SWIN_F32 && dtype != PW_SWIN_BF16) {
    pw_set_error("%s: dtype must be PW_SWIN_F32 or PW_SWIN_BF16, got %d", fn, dtype);
    return PW_EINVAL;
  }
  const int lo = PW_SWIN_LINEAR_MIN_DIM, hi = PW_SWIN_LINEAR_MAX_DIM;
  if (K < lo || K > hi || K % 16 != 0 || N < lo || N > hi || N % 16 != 0) {
    pw_set_error("%s: K = %d, N = %d not supported (multiples of 16 in %d .. %d)", fn, K, N, lo, hi);
    return PW_EUNSUP;
  }
  return 0;
}

}  // namespace
#endif  // PW_SWIN_LINEAR_COMMON_H_
