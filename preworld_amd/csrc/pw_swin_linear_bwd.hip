// The gradient of the Swin block Linears (include/preworld_hip_swin_linear_bwd.h), float32 / split-fp16 only.
//
// Data gradient and GELU gradient are the FORWARD GEMM (pw_swin_linear_common.h): dx = g W is `x W^T` with W^T packed as the weight
// (k_swin_linear_pack_cols) and g as x; dz = dh o gelu'(y) is the fc1 forward with the epilogue EPI_DGELU.  No new GEMM kernel there.
//
// Weight gradient, dW (N, K) = g^T pro(x): the contraction runs over M and both operands are channels-last, so a fragment needs
// eight consecutive ROWS of one channel.  k_swin_wgrad transposes through LDS: a thread loads four consecutive channels of four
// consecutive rows (four 16-byte loads), scales, splits, and writes per channel the four rows as one 8-byte store per plane into a
// [channel][row] tile whose rows are padded like the forward's (144 bytes: conflict-free ds_read_b128 fragments).  A is pro(x)^T,
// B is g, so a lane of the accumulator holds one n and four consecutive k: 16-byte stores of the partial product.
// Scales cannot depend on m: g column n is scaled by the power of two of that column's absmax (k_swin_col_part / k_swin_col_reduce,
// which also give the bias gradient), pro(x) by the pack-time LayerNorm bound or by its own column's power of two.  M is split in
// blocks of PW_SWIN_LINEAR_BWD_SPLIT_ROWS rows (blockIdx.y), as the forward sums a long K in blocks of 1024; the partials are added
// in double in a fixed order by k_swin_wgrad_reduce, which also undoes the scales (exact).
//
// LayerNorm gradient: k_swin_ln_bwd_rows (one lane group per row, statistics from the forward's k_swin_linear_stats) and the column
// sums through the same partial / reduce pair.  Every column sum is accumulated in double.
#include "pw_swin_linear_common.h"

#include "../../include/preworld_hip_swin_linear_bwd.h"

namespace {

constexpr int SPLIT_ROWS = PW_SWIN_LINEAR_BWD_SPLIT_ROWS;
constexpr int COL_ROWS = PW_SWIN_LINEAR_BWD_COL_ROWS;
constexpr int MC = 64;                 // rows of M per chunk of k_swin_wgrad

// ---------------------------------------------------------------------------------------------------------------- transposed pack
// one wave per column k of W (N, K): absmax -> exponent, (hi, lo) of w 2^-e as row k of the (K, N) operand, the undo scale, bias 0
__global__ __launch_bounds__(64) void k_swin_linear_pack_cols(const float* __restrict__ w, void* packed_t, int K, int N) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const Packed p = packed_view(packed_t, N, K);       // an operand with N inputs and K outputs
  unsigned short* hi = const_cast<unsigned short*>(p.plane[0]) + (size_t)k * N;
  unsigned short* lo = const_cast<unsigned short*>(p.plane[1]) + (size_t)k * N;
  unsigned bits = 0;
  for (int n = lane; n < N; n += 64) bits = max(bits, rng_absbits(w[(size_t)n * K + k]));
  const int e = rng_ideal_exp(wave_umax_all(bits));
  const float down = rng_pow2(-e);
  for (int n = lane; n < N; n += 64) {
    _Float16 h, l;
    h2_split1(w[(size_t)n * K + k] * down, h, l);
    hi[n] = __builtin_bit_cast(unsigned short, h);
    lo[n] = __builtin_bit_cast(unsigned short, l);
  }
  if (lane == 0) {
    const_cast<float*>(p.wscale)[k] = rng_pow2(e);
    const_cast<float*>(p.bias)[k] = 0.0f;
  }
}

// ---------------------------------------------------------------------------------------------------------------- column sums
// A workgroup covers 64 columns x COL_ROWS rows: thread (col, sub) walks rows sub, sub + 4, .. and the four sub-sums are added in a
// fixed order.  Partials are doubles, (row block, column):
//   COL_G   p0 = the largest |bit pattern| of a (a NaN or Inf pattern is above every number), p1 = sum of a
//   COL_X   p0 = the largest |bit pattern| of a
//   COL_LN  p0 = sum of a xhat, p1 = sum of a, xhat = (x - mean) / sigma from `stats`
enum { COL_G = 0, COL_X = 1, COL_LN = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void k_swin_col_part(const float* __restrict__ a, const float* __restrict__ x, const float* __restrict__ stats,
                                                       double* __restrict__ p0, double* __restrict__ p1, int64_t M, int C) {
  __shared__ double s0[256], s1[256];
  const int tid = threadIdx.x, sub = tid >> 6;
  const int col = blockIdx.y * 64 + (tid & 63);
  const int64_t r0 = (int64_t)blockIdx.x * COL_ROWS;
  const int64_t r1 = r0 + COL_ROWS < M ? r0 + COL_ROWS : M;
  unsigned bits = 0;
  double u = 0.0, v = 0.0;
  if (col < C) {
    for (int64_t m = r0 + sub; m < r1; m += 4) {
      const float av = a[m * C + col];
      if constexpr (MODE == COL_LN) {
        const h2_f2 st = *reinterpret_cast<const h2_f2*>(stats + 2 * m);
        u += (double)(av * ((x[m * C + col] - st[0]) * st[1]));
        v += (double)av;
      } else {
        bits = max(bits, rng_absbits(av));
        if constexpr (MODE == COL_G) v += (double)av;
      }
    }
  }
  if constexpr (MODE != COL_LN) u = (double)bits;
  s0[tid] = u;
  s1[tid] = v;
  __syncthreads();
  if (sub == 0 && col < C) {
    const int64_t o = (int64_t)blockIdx.x * C + col;
    if constexpr (MODE == COL_LN) {
      p0[o] = (s0[tid] + s0[tid + 64]) + (s0[tid + 128] + s0[tid + 192]);
    } else {
      p0[o] = fmax(fmax(s0[tid], s0[tid + 64]), fmax(s0[tid + 128], s0[tid + 192]));
    }
    if constexpr (MODE != COL_X) p1[o] = (s1[tid] + s1[tid + 64]) + (s1[tid + 128] + s1[tid + 192]);
  }
}

// one thread per column adds (or maximises) the row blocks' partials in order.  COL_G / COL_X: scale[col] = (2^-e, 2^e) of the
// column's absmax, o1 = the bias gradient (or NULL); COL_LN: o0 = dgamma, o1 = dbeta.
template <int MODE>
__global__ __launch_bounds__(256) void k_swin_col_reduce(const double* __restrict__ p0, const double* __restrict__ p1, float* __restrict__ scale,
                                                         float* __restrict__ o0, float* __restrict__ o1, int64_t RB, int C) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= C) return;
  double u = 0.0, v = 0.0;
  const bool want1 = MODE != COL_X && (MODE == COL_LN || o1 != nullptr);
  for (int64_t r = 0; r < RB; ++r) {
    const double pu = p0[r * C + col];
    u = MODE == COL_LN ? u + pu : fmax(u, pu);
    if (want1) v += p1[r * C + col];
  }
  if constexpr (MODE == COL_LN) {
    o0[col] = (float)u;
    o1[col] = (float)v;
  } else {
    const int e = rng_ideal_exp((unsigned)u);
    *reinterpret_cast<h2_f2*>(scale + 2 * col) = h2_f2{rng_pow2(-e), rng_pow2(e)};
    if (want1) o1[col] = (float)v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- weight gradient
struct WArgs {
  const float* g;          // (M, N)
  const float* x;          // (M, K)
  const void* packed;      // LN: the forward's operand (gamma, beta, the bound's power of two)
  const float* stats;      // LN: (M, 2) mean, 1 / sigma
  const float* gscale;     // (N, 2): 2^-e, 2^e of the column
  const float* xscale;     // !LN: (K, 2)
  float* part;             // (split, N, K)
  int64_t M;
  int K, N, ntk;
};

template <bool LN, int T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(T >= 2 ? 2 : 1))) void k_swin_wgrad(const WArgs a) {
  constexpr int BT = 64 * T;                          // channels of either operand per workgroup
  __shared__ __attribute__((aligned(16))) unsigned short sX[2][BT * LDS_ROW];
  __shared__ __attribute__((aligned(16))) unsigned short sG[2][BT * LDS_ROW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, N = a.N;
  const int k0 = (int)(blockIdx.x % (unsigned)a.ntk) * BT, n0 = (int)(blockIdx.x / (unsigned)a.ntk) * BT;
  const int64_t mbeg = (int64_t)blockIdx.y * SPLIT_ROWS;
  const int64_t mend = mbeg + SPLIT_ROWS < a.M ? mbeg + SPLIT_ROWS : a.M;
  const int nch = (int)((mend - mbeg + MC - 1) / MC);

  // ---- staging: channels 64 h + 4 cg + {0..3}, rows 4 rg + {0..3} of the chunk
  const int cg = tid & 15, rg = tid >> 4;
  bool gok[T], xok[T];
  v4f gdown[T], xg[T];                                // the column's 2^-e of g and (without LayerNorm) of x
  Packed pk;
  float a_scale = 1.0f;
  if constexpr (LN) {
    pk = packed_view(a.packed, K, N);
    a_scale = pk.hdr[0];
  }
#pragma unroll
  for (int h = 0; h < T; ++h) {
    const int n = n0 + 64 * h + 4 * cg, k = k0 + 64 * h + 4 * cg;
    gok[h] = n < N;
    xok[h] = k < K;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      gdown[h][e] = gok[h] ? a.gscale[2 * (n + e)] : 0.f;
      xg[h][e] = !LN && xok[h] ? a.xscale[2 * (k + e)] : 0.f;
    }
  }
  v4f greg[T][4], xreg[T][4];
  h2_f2 sreg[4];
  bool rok[4];
  auto load_chunk = [&](int c) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t m = mbeg + (int64_t)c * MC + 4 * rg + r;
      rok[r] = m < mend;
      sreg[r] = h2_f2{0.f, 0.f};
      if constexpr (LN) {
        if (rok[r]) sreg[r] = *reinterpret_cast<const h2_f2*>(a.stats + 2 * m);
      }
#pragma unroll
      for (int h = 0; h < T; ++h) {
        const v4f z = {0.f, 0.f, 0.f, 0.f};
        greg[h][r] = rok[r] && gok[h] ? *reinterpret_cast<const v4f*>(a.g + m * N + (n0 + 64 * h + 4 * cg)) : z;
        xreg[h][r] = rok[r] && xok[h] ? *reinterpret_cast<const v4f*>(a.x + m * K + (k0 + 64 * h + 4 * cg)) : z;
      }
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int h = 0; h < T; ++h) {
      v4f ga = xg[h], be = {0.f, 0.f, 0.f, 0.f};      // LN: gamma and beta, re-read per chunk (cached) to stay inside 256 registers
      if constexpr (LN) {
        if (xok[h]) {
          ga = *reinterpret_cast<const v4f*>(pk.gamma + k0 + 64 * h + 4 * cg);
          be = *reinterpret_cast<const v4f*>(pk.beta + k0 + 64 * h + 4 * cg);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float gv[4], xv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gv[r] = greg[h][r][e] * gdown[h][e];
          if constexpr (LN)
            xv[r] = ((xreg[h][r][e] - sreg[r][0]) * sreg[r][1] * ga[e] + be[e]) * a_scale;
          else
            xv[r] = xreg[h][r][e] * ga[e];
          if (!(rok[r] && gok[h])) gv[r] = 0.f;
          if (!(rok[r] && xok[h])) xv[r] = 0.f;
        }
        const int off = (64 * h + 4 * cg + e) * LDS_ROW + 4 * rg;
        u2 hi, lo;
        h2_split4(gv, hi, lo);
        *reinterpret_cast<u2*>(&sG[0][off]) = hi;
        *reinterpret_cast<u2*>(&sG[1][off]) = lo;
        h2_split4(xv, hi, lo);
        *reinterpret_cast<u2*>(&sX[0][off]) = hi;
        *reinterpret_cast<u2*>(&sX[1][off]) = lo;
      }
    }
  };

  // ---- the wave's accumulator tiles: rows = k (A operand, pro(x)^T), columns = n (B operand, g)
  const int wk = wave & 1, wn = wave >> 1, lr = lane & 31, lg = lane >> 5;
  v16f acc[T][T];
#pragma unroll
  for (int tn = 0; tn < T; ++tn)
#pragma unroll
    for (int tk = 0; tk < T; ++tk)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[tn][tk][e] = 0.f;

  load_chunk(0);
  for (int c = 0; c < nch; ++c) {
    __syncthreads();                                  // the previous chunk's fragment reads are done
    store_chunk();
    __syncthreads();
    if (c + 1 < nch) load_chunk(c + 1);
#pragma unroll
    for (int ks = 0; ks < MC / 16; ++ks) {            // rows past the end of the split are zeros in LDS
      u4v xf[2][T], gf[2][T];
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int t = 0; t < T; ++t) {
          xf[pl][t] = *reinterpret_cast<const u4v*>(&sX[pl][(32 * T * wk + 32 * t + lr) * LDS_ROW + 16 * ks + 8 * lg]);
          gf[pl][t] = *reinterpret_cast<const u4v*>(&sG[pl][(32 * T * wn + 32 * t + lr) * LDS_ROW + 16 * ks + 8 * lg]);
        }
#pragma unroll
      for (int tn = 0; tn < T; ++tn)
#pragma unroll
        for (int tk = 0; tk < T; ++tk) {
          const h8 xh = __builtin_bit_cast(h8, xf[0][tk]), xl = __builtin_bit_cast(h8, xf[1][tk]);
          const h8 gh = __builtin_bit_cast(h8, gf[0][tn]), gl = __builtin_bit_cast(h8, gf[1][tn]);
          acc[tn][tk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, gh, acc[tn][tk], 0, 0, 0);
          acc[tn][tk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, gl, acc[tn][tk], 0, 0, 0);
          acc[tn][tk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, gh, acc[tn][tk], 0, 0, 0);
        }
    }
  }

  // ---- the partial product, still in scaled units: lane (lr, lg) holds n = lr, k = 8 j + 4 lg + {0..3} of every tile
  float* part = a.part + (size_t)blockIdx.y * (size_t)N * (size_t)K;
#pragma unroll
  for (int tn = 0; tn < T; ++tn) {
    const int n = n0 + 32 * T * wn + 32 * tn + lr;
    if (n >= N) continue;
#pragma unroll
    for (int tk = 0; tk < T; ++tk)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + 32 * T * wk + 32 * tk + 8 * j + 4 * lg;
        if (k >= K) continue;
        *reinterpret_cast<v4f*>(part + (size_t)n * K + k) =
            v4f{acc[tn][tk][4 * j], acc[tn][tk][4 * j + 1], acc[tn][tk][4 * j + 2], acc[tn][tk][4 * j + 3]};
      }
  }
}

// dW[n][k .. k+3] = (sum over the splits, in order, in double) 2^e_n 2^e_k
template <bool LN>
__global__ __launch_bounds__(256) void k_swin_wgrad_reduce(const float* __restrict__ part, const float* __restrict__ gscale,
                                                           const float* __restrict__ xscale, const void* packed, float* __restrict__ dw, int S,
                                                           int K, int N) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int kq = K / 4;
  if (i >= (int64_t)N * kq) return;
  const int n = (int)(i / kq), k = 4 * (int)(i % kq);
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int sp = 0; sp < S; ++sp) {
    const v4f p = *reinterpret_cast<const v4f*>(part + ((size_t)sp * N + n) * K + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += (double)p[e];
  }
  const float gu = gscale[2 * n + 1];
  v4f o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float xu;
    if constexpr (LN) xu = packed_view(packed, K, N).hdr[1];
    else xu = xscale[2 * (k + e) + 1];
    o[e] = (float)s[e] * (gu * xu);
  }
  *reinterpret_cast<v4f*>(dw + (size_t)n * K + k) = o;
}

// ---------------------------------------------------------------------------------------------------------------- LayerNorm gradient
// LPR lanes per row, statistics (mean, 1 / sigma) from k_swin_linear_stats<true>:
//   dx = dres + rstd (gamma dxn - mean_k(gamma dxn) - xhat mean_k(gamma dxn xhat));  dx may be dxn (a lane rewrites what it read)
template <int LPR>
__global__ __launch_bounds__(256) void k_swin_ln_bwd_rows(const float* dxn, const float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ dres, const float* __restrict__ stats, float* dx, int64_t M,
                                                          int K) {
  const int sub = threadIdx.x % LPR;
  const int64_t m = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const bool ok = m < M;                              // no early return: the shuffles below take every lane of the wave
  const int64_t base = (ok ? m : 0) * K;
  const h2_f2 st = *reinterpret_cast<const h2_f2*>(stats + 2 * (ok ? m : 0));
  float s1 = 0.f, s2 = 0.f;
  if (ok)
    for (int k = 4 * sub; k < K; k += 4 * LPR) {
      const v4f d = *reinterpret_cast<const v4f*>(dxn + base + k) * *reinterpret_cast<const v4f*>(gamma + k);
      const v4f xh = (*reinterpret_cast<const v4f*>(x + base + k) - st[0]) * st[1];
      s1 += (d[0] + d[1]) + (d[2] + d[3]);
      s2 += (d[0] * xh[0] + d[1] * xh[1]) + (d[2] * xh[2] + d[3] * xh[3]);
    }
#pragma unroll
  for (int o = LPR / 2; o >= 1; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  const float m1 = s1 / (float)K, m2 = s2 / (float)K;
  if (ok)
    for (int k = 4 * sub; k < K; k += 4 * LPR) {
      const v4f d = *reinterpret_cast<const v4f*>(dxn + base + k) * *reinterpret_cast<const v4f*>(gamma + k);
      const v4f xh = (*reinterpret_cast<const v4f*>(x + base + k) - st[0]) * st[1];
      v4f o = (d - m1 - xh * m2) * st[1];
      if (dres) o = *reinterpret_cast<const v4f*>(dres + base + k) + o;
      *reinterpret_cast<v4f*>(dx + base + k) = o;
    }
}

void launch_stats_ln(const float* x, float* stats, int64_t M, int K, float eps, hipStream_t st) {
  if (K >= 512) hipLaunchKernelGGL((k_swin_linear_stats<true, 64>), dim3((unsigned)pw_cdiv(M, 4)), dim3(256), 0, st, x, stats, M, K, eps);
  else hipLaunchKernelGGL((k_swin_linear_stats<true, 8>), dim3((unsigned)pw_cdiv(M, 32)), dim3(256), 0, st, x, stats, M, K, eps);
}

// ---------------------------------------------------------------------------------------------------------------- host
constexpr int64_t MAX_M = ((int64_t)1 << 32) - 1;     // and ceil(M / SPLIT_ROWS) <= 65535 for the weight gradient's grid

struct WLayout {
  size_t stats, pg0, pg1, px0, gscale, xscale, part, total;
  int64_t RB, S;
};
WLayout weight_layout(int64_t M, int K, int N, bool ln) {
  WLayout l;
  l.RB = pw_cdiv(M, COL_ROWS);
  l.S = pw_cdiv(M, SPLIT_ROWS);
  size_t off = 0;
  l.stats = off; off += ln ? pw_align_up(8u * (size_t)M, 16) : 0;
  l.pg0 = off; off += 8u * (size_t)l.RB * N;
  l.pg1 = off; off += 8u * (size_t)l.RB * N;
  l.px0 = off; off += ln ? 0 : 8u * (size_t)l.RB * K;
  l.gscale = off; off += 8u * (size_t)N;
  l.xscale = off; off += ln ? 0 : 8u * (size_t)K;
  l.part = off; off += 4u * (size_t)l.S * N * K;
  l.total = off;
  return l;
}
struct LnLayout {
  size_t stats, p0, p1, total;
  int64_t RB;
};
LnLayout ln_layout(int64_t M, int K) {
  LnLayout l;
  l.RB = pw_cdiv(M, COL_ROWS);
  size_t off = 0;
  l.stats = off; off += pw_align_up(8u * (size_t)M, 16);
  l.p0 = off; off += 8u * (size_t)l.RB * K;
  l.p1 = off; off += 8u * (size_t)l.RB * K;
  l.total = off;
  return l;
}
bool m_ok(int64_t M) { return M >= 1 && M <= MAX_M && pw_cdiv(M, SPLIT_ROWS) <= 65535; }

}  // namespace

PW_API size_t pw_swin_linear_backward_packed_bytes(int K, int N) {
  if (check_dims("pw_swin_linear_backward_packed_bytes", K, N, PW_SWIN_F32) != 0) return 0;
  return packed_bytes(N, K, 2);
}

PW_API int pw_swin_linear_backward_pack(const float* weight, void* packed_t, int K, int N, void* stream) {
  PW_CHECK_ARG(weight && packed_t, "pw_swin_linear_backward_pack: null pointer");
  const int rc = check_dims("pw_swin_linear_backward_pack", K, N, PW_SWIN_F32);
  if (rc != 0) return rc;
  PW_CHECK_ARG(((uintptr_t)packed_t & 15) == 0 && ((uintptr_t)weight & 3) == 0,
               "pw_swin_linear_backward_pack: packed_t must be 16-byte aligned, weight 4-byte aligned");
  hipStream_t st = pw_stream(stream);
  hipLaunchKernelGGL(k_swin_linear_pack_cols, dim3(K), dim3(64), 0, st, weight, packed_t, K, N);
  // header, gamma = 1, beta = 0 of an operand with N inputs and K outputs: every byte of the packed operand is defined
  hipLaunchKernelGGL(k_swin_linear_pack_ln<false>, dim3(1), dim3(256), 0, st, (const float*)nullptr, (const float*)nullptr, packed_t, N, K);
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_swin_linear_pack_cols");
  return 0;
}

PW_API size_t pw_swin_linear_backward_rows_workspace_bytes(int64_t M) { return M < 1 ? 0 : 8u * (size_t)M; }

PW_API int pw_swin_linear_backward_data(const float* g, const void* packed_t, float* dx, float* workspace, size_t workspace_bytes, int64_t M,
                                        int K, int N, void* stream) {
  PW_CHECK_ARG(g && packed_t && dx, "pw_swin_linear_backward_data: null pointer");
  const int rc = check_dims("pw_swin_linear_backward_data", K, N, PW_SWIN_F32);
  if (rc != 0) return rc;
  PW_CHECK_ARG(M >= 1 && M <= MAX_M, "pw_swin_linear_backward_data: M must be in 1 .. 2^32 - 1, got %lld", (long long)M);
  const size_t need = 8u * (size_t)M;
  PW_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0,
               "pw_swin_linear_backward_data: workspace of %zu bytes needed (16-byte aligned), got %zu", need, workspace_bytes);
  PW_CHECK_ARG((((uintptr_t)g | (uintptr_t)dx | (uintptr_t)packed_t) & 15) == 0,
               "pw_swin_linear_backward_data: g, dx and packed_t must be 16-byte aligned");
  // the forward GEMM with K and N exchanged: g (M, N) is its x, packed_t its weight, dx (M, K) its out
  const bool ran = run_linear<true>(g, packed_t, nullptr, dx, workspace, true, M, N, K, false, 0.f, EPI_BIAS, false, pw_stream(stream),
                                    "k_swin_linear<%d, %d, %d, %d, %d, %d>");
  PW_CHECK_ARG(ran, "pw_swin_linear_backward_data: %lld rows do not fit one launch", (long long)M);
  PW_CHECK_LAUNCH();
  return 0;
}

PW_API int pw_swin_linear_backward_gelu(const float* x, const void* packed, const float* dh, float* dz, float* workspace,
                                        size_t workspace_bytes, int64_t M, int K, int N, float eps, void* stream) {
  PW_CHECK_ARG(x && packed && dh && dz, "pw_swin_linear_backward_gelu: null pointer");
  const int rc = check_dims("pw_swin_linear_backward_gelu", K, N, PW_SWIN_F32);
  if (rc != 0) return rc;
  PW_CHECK_ARG(M >= 1 && M <= MAX_M, "pw_swin_linear_backward_gelu: M must be in 1 .. 2^32 - 1, got %lld", (long long)M);
  PW_CHECK_ARG(eps >= 0.f && eps < INFINITY, "pw_swin_linear_backward_gelu: eps must be finite and non-negative");
  const size_t need = 8u * (size_t)M;
  PW_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0,
               "pw_swin_linear_backward_gelu: workspace of %zu bytes needed (16-byte aligned), got %zu", need, workspace_bytes);
  PW_CHECK_ARG((((uintptr_t)x | (uintptr_t)dh | (uintptr_t)dz | (uintptr_t)packed) & 15) == 0,
               "pw_swin_linear_backward_gelu: x, dh, dz and packed must be 16-byte aligned");
  const bool ran = run_linear<true>(x, packed, dh, dz, workspace, true, M, K, N, true, eps, EPI_DGELU, false, pw_stream(stream),
                                    "k_swin_linear<%d, %d, %d, %d, %d, %d>");
  PW_CHECK_ARG(ran, "pw_swin_linear_backward_gelu: %lld rows do not fit one launch", (long long)M);
  PW_CHECK_LAUNCH();
  return 0;
}

PW_API size_t pw_swin_linear_backward_weight_workspace_bytes(int64_t M, int K, int N, int ln) {
  if (check_dims("pw_swin_linear_backward_weight_workspace_bytes", K, N, PW_SWIN_F32) != 0) return 0;
  if (!m_ok(M)) {
    pw_set_error("pw_swin_linear_backward_weight_workspace_bytes: M = %lld not supported", (long long)M);
    return 0;
  }
  return weight_layout(M, K, N, ln != 0).total;
}

PW_API int pw_swin_linear_backward_weight(const float* g, const float* x, const void* packed, float* dweight, float* dbias, void* workspace,
                                          size_t workspace_bytes, int64_t M, int K, int N, int ln, float eps, void* stream) {
  PW_CHECK_ARG(g && workspace, "pw_swin_linear_backward_weight: null pointer");
  PW_CHECK_ARG(dweight || dbias, "pw_swin_linear_backward_weight: dweight and dbias are both NULL");
  PW_CHECK_ARG(!dweight || (x && (!ln || packed)), "pw_swin_linear_backward_weight: dweight needs x, and with ln the packed operand");
  const int rc = check_dims("pw_swin_linear_backward_weight", K, N, PW_SWIN_F32);
  if (rc != 0) return rc;
  PW_CHECK_ARG(m_ok(M), "pw_swin_linear_backward_weight: M must be in 1 .. %lld, got %lld", (long long)65535 * SPLIT_ROWS, (long long)M);
  PW_CHECK_ARG(!ln || (eps >= 0.f && eps < INFINITY), "pw_swin_linear_backward_weight: eps must be finite and non-negative");
  const bool lnb = ln != 0;
  const WLayout l = weight_layout(M, K, N, lnb);
  PW_CHECK_ARG(workspace_bytes >= l.total && ((uintptr_t)workspace & 15) == 0,
               "pw_swin_linear_backward_weight: workspace of %zu bytes needed (16-byte aligned), got %zu", l.total, workspace_bytes);
  PW_CHECK_ARG((((uintptr_t)g | (uintptr_t)x | (uintptr_t)dweight | (uintptr_t)packed) & 15) == 0 && ((uintptr_t)dbias & 3) == 0,
               "pw_swin_linear_backward_weight: g, x, dweight and packed must be 16-byte aligned, dbias 4-byte aligned");
  char* w = static_cast<char*>(workspace);
  float* stats = reinterpret_cast<float*>(w + l.stats);
  double* pg0 = reinterpret_cast<double*>(w + l.pg0);
  double* pg1 = reinterpret_cast<double*>(w + l.pg1);
  double* px0 = reinterpret_cast<double*>(w + l.px0);
  float* gscale = reinterpret_cast<float*>(w + l.gscale);
  float* xscale = reinterpret_cast<float*>(w + l.xscale);
  float* part = reinterpret_cast<float*>(w + l.part);
  hipStream_t st = pw_stream(stream);
  // one pass over g: the columns' powers of two and the bias gradient
  hipLaunchKernelGGL(k_swin_col_part<COL_G>, dim3((unsigned)l.RB, (unsigned)pw_cdiv(N, 64)), dim3(256), 0, st, g, (const float*)nullptr,
                     (const float*)nullptr, pg0, pg1, M, N);
  hipLaunchKernelGGL(k_swin_col_reduce<COL_G>, dim3((unsigned)pw_cdiv(N, 256)), dim3(256), 0, st, pg0, pg1, gscale, (float*)nullptr, dbias, l.RB, N);
  if (dweight) {
    const bool large = K >= 128 && N >= 128;
    const int bt = large ? 128 : 64;
    WArgs a;
    a.g = g; a.x = x; a.packed = packed; a.stats = stats; a.gscale = gscale; a.xscale = xscale; a.part = part;
    a.M = M; a.K = K; a.N = N; a.ntk = (int)pw_cdiv(K, bt);
    const dim3 grid((unsigned)(a.ntk * pw_cdiv(N, bt)), (unsigned)l.S);
    if (lnb) {
      launch_stats_ln(x, stats, M, K, eps, st);
      if (large) hipLaunchKernelGGL((k_swin_wgrad<true, 2>), grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL((k_swin_wgrad<true, 1>), grid, dim3(256), 0, st, a);
      hipLaunchKernelGGL(k_swin_wgrad_reduce<true>, dim3((unsigned)pw_cdiv((int64_t)N * K / 4, 256)), dim3(256), 0, st, part, gscale, xscale,
                         packed, dweight, (int)l.S, K, N);
    } else {
      hipLaunchKernelGGL(k_swin_col_part<COL_X>, dim3((unsigned)l.RB, (unsigned)pw_cdiv(K, 64)), dim3(256), 0, st, x, (const float*)nullptr,
                         (const float*)nullptr, px0, (double*)nullptr, M, K);
      hipLaunchKernelGGL(k_swin_col_reduce<COL_X>, dim3((unsigned)pw_cdiv(K, 256)), dim3(256), 0, st, px0, (const double*)nullptr, xscale,
                         (float*)nullptr, (float*)nullptr, l.RB, K);
      if (large) hipLaunchKernelGGL((k_swin_wgrad<false, 2>), grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL((k_swin_wgrad<false, 1>), grid, dim3(256), 0, st, a);
      hipLaunchKernelGGL(k_swin_wgrad_reduce<false>, dim3((unsigned)pw_cdiv((int64_t)N * K / 4, 256)), dim3(256), 0, st, part, gscale, xscale,
                         packed, dweight, (int)l.S, K, N);
    }
    pw_note_kernel("k_swin_wgrad<%d, %d>", (int)lnb, bt / 64);
  } else {
    pw_note_kernel("k_swin_col_part<0>");
  }
  PW_CHECK_LAUNCH();
  return 0;
}

PW_API size_t pw_swin_layernorm_backward_workspace_bytes(int64_t M, int K) {
  if (check_dims("pw_swin_layernorm_backward_workspace_bytes", K, K, PW_SWIN_F32) != 0) return 0;
  if (M < 1 || M > MAX_M) {
    pw_set_error("pw_swin_layernorm_backward_workspace_bytes: M = %lld not supported", (long long)M);
    return 0;
  }
  return ln_layout(M, K).total;
}

PW_API int pw_swin_layernorm_backward(const float* dxn, const float* x, const float* gamma, const float* dres, float* dx, float* dgamma,
                                      float* dbeta, void* workspace, size_t workspace_bytes, int64_t M, int K, float eps, void* stream) {
  PW_CHECK_ARG(dxn && x && gamma && workspace, "pw_swin_layernorm_backward: null pointer");
  PW_CHECK_ARG(dx || dgamma, "pw_swin_layernorm_backward: dx, dgamma and dbeta are all NULL");
  PW_CHECK_ARG((dgamma == nullptr) == (dbeta == nullptr), "pw_swin_layernorm_backward: dgamma and dbeta come together or not at all");
  const int rc = check_dims("pw_swin_layernorm_backward", K, K, PW_SWIN_F32);
  if (rc != 0) return rc;
  PW_CHECK_ARG(M >= 1 && M <= MAX_M, "pw_swin_layernorm_backward: M must be in 1 .. 2^32 - 1, got %lld", (long long)M);
  PW_CHECK_ARG(eps >= 0.f && eps < INFINITY, "pw_swin_layernorm_backward: eps must be finite and non-negative");
  const LnLayout l = ln_layout(M, K);
  PW_CHECK_ARG(workspace_bytes >= l.total && ((uintptr_t)workspace & 15) == 0,
               "pw_swin_layernorm_backward: workspace of %zu bytes needed (16-byte aligned), got %zu", l.total, workspace_bytes);
  PW_CHECK_ARG((((uintptr_t)dxn | (uintptr_t)x | (uintptr_t)gamma | (uintptr_t)dres | (uintptr_t)dx) & 15) == 0 &&
                   (((uintptr_t)dgamma | (uintptr_t)dbeta) & 3) == 0,
               "pw_swin_layernorm_backward: dxn, x, gamma, dres and dx must be 16-byte aligned, dgamma and dbeta 4-byte aligned");
  char* w = static_cast<char*>(workspace);
  float* stats = reinterpret_cast<float*>(w + l.stats);
  double* p0 = reinterpret_cast<double*>(w + l.p0);
  double* p1 = reinterpret_cast<double*>(w + l.p1);
  hipStream_t st = pw_stream(stream);
  launch_stats_ln(x, stats, M, K, eps, st);
  if (dgamma) {                                       // before the rows: dx may overwrite dxn
    hipLaunchKernelGGL(k_swin_col_part<COL_LN>, dim3((unsigned)l.RB, (unsigned)pw_cdiv(K, 64)), dim3(256), 0, st, dxn, x, stats, p0, p1, M, K);
    hipLaunchKernelGGL(k_swin_col_reduce<COL_LN>, dim3((unsigned)pw_cdiv(K, 256)), dim3(256), 0, st, p0, p1, (float*)nullptr, dgamma, dbeta, l.RB, K);
  }
  if (dx) {
    if (K >= 512) hipLaunchKernelGGL((k_swin_ln_bwd_rows<64>), dim3((unsigned)pw_cdiv(M, 4)), dim3(256), 0, st, dxn, x, gamma, dres, stats, dx, M, K);
    else hipLaunchKernelGGL((k_swin_ln_bwd_rows<8>), dim3((unsigned)pw_cdiv(M, 32)), dim3(256), 0, st, dxn, x, gamma, dres, stats, dx, M, K);
  }
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_swin_ln_bwd_rows<%d>", K >= 512 ? 64 : 8);
  return 0;
}
