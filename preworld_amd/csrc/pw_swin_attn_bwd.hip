// Gradient of the Swin shifted-window attention (include/preworld_hip_swin_bwd.h): dqkv, dpad_qkv and dbias_table from qkv, out and
// dout, all in the UN-padded, UN-rolled (B, H, W, .) token layout of csrc/pw_swin_attn.hip.  Pad, roll, window partition, the
// relative-position index, the shift mask and their inverses are the index arithmetic of the forward (the header of
// preworld_hip_swin.h states them per token); nothing of size (N, N) and nothing in window order exists in global memory, and nothing
// but qkv is needed from the forward: logits, row maximum and row sum are recomputed with the forward's own expressions, and
// D = dout . out is formed as sum_b P_ab dP_ab in registers (`out` is checked and not read).
//
// One workgroup = one (window, head), NT = ceil(ws^2 / 16) waves, two phases over one pair of LDS arrays (fp32 whatever the storage
// dtype; 36-float rows so that 16-byte row reads and 4-byte column reads both spread over the banks):
//   phase A  LDS = K, V.  Wave s owns the queries 16 s .. 16 s + 15 in the forward's orientation: S^T = K Q^T puts a query's whole
//            row of logits into the registers of the lanes q, q + 16, q + 32, q + 48, and so does dP^T = V dout^T: m, l and D are
//            register work plus two cross-lane steps (kept in LDS for phase B), dS = P (dP - D) in registers is
//            already the B operand of dQ^T = K^T dS^T (A = a column of K per product).  Each dq row is stored once.
//   phase B  LDS = Q, dout.  Wave s owns the keys 16 s .. 16 s + 15: S = Q K^T and dP = dout V^T per query tile against the lane's
//            own k and v rows, P and dS from the m, l, D of phase A, then dV^T += dout^T P and dK^T += Q^T dS inside the wave.
//            Each dk, dv row of a real token is stored once; the rows of padded tokens are summed per workgroup in key order.
// Seven products instead of five, no cross-wave reduction of a matrix, no atomics.
//
// dbias_table: wave s adds its dS tiles into ITS OWN (2 ws - 1)^2 bins in LDS, one query (16 keys = 16 distinct bins) per step in a
// fixed order; LDS operations of one wave complete in issue order, so a step sees the sums of the steps before it.  The workgroup
// adds its waves' bins in wave order and writes one partial of (2 ws - 1)^2 + 64 floats (bins, then the k and v gradient of its
// padded tokens) to the workspace; k_swin_bwd_reduce adds the partials of one head in a fixed order (64 interleaved slices, then
// the slices).  Two calls give the same bits.
//
// Products are v_mfma_f32_16x16x4_f32 for both dtypes: bf16 is converted on the way into LDS / registers and rounded once on the
// store (a bf16-MFMA variant was not built).
#include "pw_common.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef __bf16 bf4 __attribute__((ext_vector_type(4)));

constexpr int DMAX = PW_SWIN_MAX_HEAD_DIM;
constexpr int TAB_MAX = (2 * PW_SWIN_MAX_WS - 1) * (2 * PW_SWIN_MAX_WS - 1);
constexpr int PADS = PW_SWIN_BWD_PAD_SLOTS;                                 // [k 0..31][v 0..31] of the padded tokens
constexpr unsigned KEY_PAD = 1u << 30;                                      // key word of a row beyond ws^2: no such key
constexpr int KS = 36;                                                      // LDS row stride in floats: 144 B
constexpr int RED_OUT = 16, RED_SLICES = 64;                                // k_swin_bwd_reduce: outputs per block, interleaved slices
static_assert(PADS == 2 * DMAX, "pad slots hold one k and one v row");

struct BwdArgs {
  const void* qkv;
  const void* pad;
  const float* table;
  const void* dout;
  void* dqkv;
  float* wsp;                        // partials, slot floats per workgroup; null: neither reduction is wanted
  int need_tab, need_pad, slot;
  int H, W, C, nH, d, ws, shift, Hp, Wp, nWh, nWw;
  float scale;
};

__device__ __forceinline__ int wrap(int v, int n) { return v >= n ? v - n : v; }

template <bool BF>
struct Fmt;
template <>
struct Fmt<false> {
  typedef float elem;
  static __device__ __forceinline__ v4f ld4(const float* p) { return *reinterpret_cast<const v4f*>(p); }
  static __device__ __forceinline__ void st4(float* p, v4f r) { *reinterpret_cast<v4f*>(p) = r; }
};
template <>
struct Fmt<true> {
  typedef unsigned short elem;
  static __device__ __forceinline__ v4f ld4(const unsigned short* p) {
    const u2v w = *reinterpret_cast<const u2v*>(p);
    return v4f{__uint_as_float(w[0] << 16), __uint_as_float(w[0] & 0xffff0000u), __uint_as_float(w[1] << 16),
               __uint_as_float(w[1] & 0xffff0000u)};
  }
  static __device__ __forceinline__ void st4(unsigned short* p, v4f r) {
    const bf4 h = {(__bf16)r[0], (__bf16)r[1], (__bf16)r[2], (__bf16)r[3]};
    *reinterpret_cast<u2v*>(p) = __builtin_bit_cast(u2v, h);
  }
};

template <bool BF, int NT>
__global__ __launch_bounds__(64 * NT) void k_swin_attn_bwd(const BwdArgs a) {
  typedef typename Fmt<BF>::elem E;
  typedef Fmt<BF> F;
  constexpr int NK = 16 * NT;                                   // rows: ws^2 rounded up to the tile
  constexpr int NTH = 64 * NT;
  __shared__ __attribute__((aligned(16))) float sAB[2 * NK * KS];
  __shared__ __attribute__((aligned(16))) unsigned sKey[NK];
  __shared__ __attribute__((aligned(16))) float sM[NK];
  __shared__ __attribute__((aligned(16))) float sInv[NK];
  __shared__ __attribute__((aligned(16))) float sD[NK];
  __shared__ float sTab[TAB_MAX];
  __shared__ float sBins[NT * TAB_MAX];
  float* const sA = sAB;                                        // phase A: K, phase B: Q
  float* const sB = sAB + NK * KS;                              // phase A: V, phase B: dout

  const int tid = threadIdx.x;
  const int ws = a.ws, N = ws * ws, d = a.d, C = a.C, shift = a.shift;
  const int tw = 2 * ws - 1, tw2 = tw * tw;
  const int64_t blk = blockIdx.x;
  unsigned bid = blockIdx.x;
  const int head = bid % a.nH;
  bid /= a.nH;
  const int wj = bid % a.nWw;
  bid /= a.nWw;
  const int wi = bid % a.nWh;
  const int b = bid / a.nWh;
  const int64_t HW = (int64_t)a.H * a.W;
  const E* qkv = static_cast<const E*>(a.qkv) + (int64_t)b * HW * 3 * C + head * d;
  const E* pad = a.pad ? static_cast<const E*>(a.pad) + head * d : nullptr;
  const E* doutp = static_cast<const E*>(a.dout) + (int64_t)b * HW * C + head * d;
  E* dqkv = static_cast<E*>(a.dqkv) + (int64_t)b * HW * 3 * C + head * d;

  // source token of window position n (< N), -1: a padded token
  auto token = [&](int r, int c) -> int64_t {
    const int si = wrap(wi * ws + r + shift, a.Hp), sj = wrap(wj * ws + c + shift, a.Wp);
    return si < a.H && sj < a.W ? (int64_t)si * a.W + sj : (int64_t)-1;
  };

  // ---- phase A staging: K, V, key words, the head's bias column; this workgroup's bins start at zero
  for (int idx = tid; idx < NK * (DMAX / 4); idx += NTH) {
    const int n = idx >> 3, c4 = (idx & 7) * 4;
    v4f kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
    unsigned key = KEY_PAD;
    if (n < N) {
      const int r = n / ws, c = n - r * ws;
      const int i = wi * ws + r, j = wj * ws + c;
      const int region = shift > 0 ? 3 * ((i >= a.Hp - ws) + (i >= a.Hp - shift)) + (j >= a.Wp - ws) + (j >= a.Wp - shift) : 0;
      key = (unsigned)r | (unsigned)c << 8 | (unsigned)region << 16;
      if (c4 < d) {
        const int64_t tok = token(r, c);
        if (tok >= 0) {
          const E* t = qkv + tok * 3 * C + c4;
          kv = F::ld4(t + C);
          vv = F::ld4(t + 2 * C);
        } else if (pad) {
          kv = F::ld4(pad + C + c4);
          vv = F::ld4(pad + 2 * C + c4);
        }
      }
    }
    *reinterpret_cast<v4f*>(&sA[n * KS + c4]) = kv;
    *reinterpret_cast<v4f*>(&sB[n * KS + c4]) = vv;
    if (c4 == 0) sKey[n] = key;
  }
  for (int idx = tid; idx < tw2; idx += NTH) sTab[idx] = a.table[(int64_t)idx * a.nH + head];
  if (a.need_tab)
    for (int idx = tid; idx < NT * tw2; idx += NTH) sBins[idx] = 0.f;
  __syncthreads();

  const int lane = tid & 63, s = tid >> 6, q = lane & 15, g = lane >> 4;
  const int row = 16 * s + q;                                   // phase A: this lane's query, phase B: this lane's key
  const unsigned rkey = sKey[row];
  const int rr = rkey & 0xff, rc = (rkey >> 8) & 0xff, rreg = (rkey >> 16) & 0xff;
  const bool isrow = row < N;
  const int64_t tok = isrow ? token(rr, rc) : (int64_t)-1;      // source token of the row, -1: padded token or no such row

  // ================================================================================================ phase A: wave = 16 queries
  {
    const E* qsrc = tok >= 0 ? qkv + tok * 3 * C : (isrow ? pad : nullptr);      // q of the query's token; null: zeros
    // k = g of the 16x16x4 product number (h, e) is channel 16 h + 4 g + e for both operands
    v4f qf[2], dof[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      qf[h] = v4f{0.f, 0.f, 0.f, 0.f};
      dof[h] = v4f{0.f, 0.f, 0.f, 0.f};
      const int c0 = 16 * h + 4 * g;
      if (c0 < d) {
        if (qsrc) qf[h] = F::ld4(qsrc + c0);
        if (tok >= 0) dof[h] = F::ld4(doutp + tok * C + c0);      // a padded query has no output: its dout, D and dS are zero
      }
    }

    v4f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      v4f kf[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) kf[t] = *reinterpret_cast<const v4f*>(&sA[(16 * t + q) * KS + 16 * h + 4 * g]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[t][e], qf[h][e], acc[t], 0, 0, 0);
    }

    // logits of query q against keys 16 t + 4 g + e, exactly as the forward forms them
    const int tbase = (rr + ws - 1) * tw + rc + ws - 1;
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const u4v kk = *reinterpret_cast<const u4v*>(&sKey[16 * t + 4 * g]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned key = kk[e];
        const int rb = key & 0xff, cb = (key >> 8) & 0xff, rgb = (key >> 16) & 0xff;
        float x = acc[t][e] * a.scale + sTab[tbase - rb * tw - cb];
        if (rgb != rreg) x += -100.0f;
        if (key & KEY_PAD) x = -INFINITY;
        acc[t][e] = x;
        mx = fmaxf(mx, x);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = __expf(acc[t][e] - mx);
        acc[t][e] = p;
        sum += p;
      }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;

    // dP^T = V dout^T, three key tiles (independent accumulators) at a time
    v4f dp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) dp[t] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t0 = 0; t0 < NT; t0 += 3)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        v4f vf[3];
#pragma unroll
        for (int t = t0; t < t0 + 3 && t < NT; ++t) vf[t - t0] = *reinterpret_cast<const v4f*>(&sB[(16 * t + q) * KS + 16 * h + 4 * g]);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int t = t0; t < t0 + 3 && t < NT; ++t) dp[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[t - t0][e], dof[h][e], dp[t], 0, 0, 0);
      }
    // D = dout . out, formed as sum_b P_ab dP_ab from these registers: the same number (out = P v), and where the softmax has
    // saturated (P one-hot) dP - D is exactly zero, as in the softmax backward of the torch path
    float D = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) D = fmaf(acc[t][e], dp[t][e], D);
    D += __shfl_xor(D, 16);
    D += __shfl_xor(D, 32);
    D *= inv;
    if (g == 0) {
      sM[row] = mx;
      sInv[row] = inv;
      sD[row] = D;
    }

    // dS = P (dP - D), dQ^T += K^T dS^T (rows = channels, the k index = keys as the tiles hold them)
    v4f o[2] = {v4f{0.f, 0.f, 0.f, 0.f}, v4f{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ds = acc[t][e] * inv * (dp[t][e] - D);
        const float* kcol = &sA[(16 * t + 4 * g + e) * KS + q];
        o[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(kcol[0], ds, o[0], 0, 0, 0);
        o[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(kcol[16], ds, o[1], 0, 0, 0);
      }
    }
    // lane (q, g) holds channels 16 dt + 4 g + {0..3} of dq of query q
    if (tok >= 0) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int c0 = 16 * dt + 4 * g;
        if (c0 < d) F::st4(dqkv + tok * 3 * C + c0, o[dt] * a.scale);
      }
    }
  }
  __syncthreads();

  // ================================================================================================ phase B: wave = 16 keys
  // staging: Q (a padded token's q is pad_qkv's, as in phase A, so that the recomputed logits are the same numbers) and dout
  for (int idx = tid; idx < NK * (DMAX / 4); idx += NTH) {
    const int n = idx >> 3, c4 = (idx & 7) * 4;
    v4f qv = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
    if (n < N && c4 < d) {
      const int r = n / ws, c = n - r * ws;
      const int64_t t = token(r, c);
      if (t >= 0) {
        qv = F::ld4(qkv + t * 3 * C + c4);
        dv = F::ld4(doutp + t * C + c4);
      } else if (pad) {
        qv = F::ld4(pad + c4);
      }
    }
    *reinterpret_cast<v4f*>(&sA[n * KS + c4]) = qv;
    *reinterpret_cast<v4f*>(&sB[n * KS + c4]) = dv;
  }
  __syncthreads();

  v4f ov[2] = {v4f{0.f, 0.f, 0.f, 0.f}, v4f{0.f, 0.f, 0.f, 0.f}};
  v4f ok[2] = {v4f{0.f, 0.f, 0.f, 0.f}, v4f{0.f, 0.f, 0.f, 0.f}};
  {
    const E* ksrc = tok >= 0 ? qkv + tok * 3 * C + C : (isrow && pad ? pad + C : nullptr);      // k of the key's token; v is C further
    v4f kf[2], vf[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      kf[h] = v4f{0.f, 0.f, 0.f, 0.f};
      vf[h] = v4f{0.f, 0.f, 0.f, 0.f};
      const int c0 = 16 * h + 4 * g;
      if (ksrc && c0 < d) {
        kf[h] = F::ld4(ksrc + c0);
        vf[h] = F::ld4(ksrc + C + c0);
      }
    }
    const int koff = rr * tw + rc - (ws - 1) * tw - (ws - 1);     // bin of (query a, this key) = r_a tw + c_a - koff
    volatile float* bins = sBins + s * tw2;
#pragma unroll 1
    for (int u = 0; u < NT; ++u) {
      // S = Q K^T and dP = dout V^T: rows = queries 16 u + 4 g + e, column = this lane's key
      v4f sacc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const v4f qa = *reinterpret_cast<const v4f*>(&sA[(16 * u + q) * KS + 16 * h + 4 * g]);
        const v4f da = *reinterpret_cast<const v4f*>(&sB[(16 * u + q) * KS + 16 * h + 4 * g]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sacc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[e], kf[h][e], sacc, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x4f32(da[e], vf[h][e], dp, 0, 0, 0);
        }
      }
      const u4v qk = *reinterpret_cast<const u4v*>(&sKey[16 * u + 4 * g]);
      const v4f m4 = *reinterpret_cast<const v4f*>(&sM[16 * u + 4 * g]);
      const v4f i4 = *reinterpret_cast<const v4f*>(&sInv[16 * u + 4 * g]);
      const v4f d4 = *reinterpret_cast<const v4f*>(&sD[16 * u + 4 * g]);
      v4f p, ds;
      int bin[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned key = qk[e];
        const int ra = key & 0xff, ca = (key >> 8) & 0xff, rga = (key >> 16) & 0xff;
        bin[e] = ra * tw + ca - koff;
        float x = sacc[e] * a.scale + sTab[bin[e]];
        if (rga != rreg) x += -100.0f;
        if (!isrow) x = -INFINITY;                                // no such key: P = 0
        p[e] = __expf(x - m4[e]) * i4[e];
        ds[e] = p[e] * (dp[e] - d4[e]);
      }
      // dV^T += dout^T P, dK^T += Q^T dS: rows = channels, the k index = queries in the order the tile holds them
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ar = (16 * u + 4 * g + e) * KS + q;
        ov[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(sB[ar], p[e], ov[0], 0, 0, 0);
        ov[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(sB[ar + 16], p[e], ov[1], 0, 0, 0);
        ok[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(sA[ar], ds[e], ok[0], 0, 0, 0);
        ok[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(sA[ar + 16], ds[e], ok[1], 0, 0, 0);
      }
      // the table gradient: one query group at a time, steps in the fixed order (u, gg, e).  The 16 active lanes of a step never
      // alias: they hold ONE query (16 u + 4 gg + e) against 16 distinct keys, and for a fixed query the bin r_a tw + c_a - koff is
      // one-to-one in the key.  Lanes of different groups hold different queries and can meet in a bin, hence one group at a time;
      // a later step reads what an earlier one wrote because LDS operations of one wave complete in issue order (volatile keeps
      // the compiler from reordering or merging them).
      if (a.need_tab) {
        for (int gg = 0; gg < 4; ++gg) {
          if (g == gg && isrow) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (16 * u + 4 * g + e < N) bins[bin[e]] = bins[bin[e]] + ds[e];
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
  }
  __syncthreads();                                                // every wave is done with Q and dout, every bin is final

  // lane (q, g) holds channels 16 dt + 4 g + {0..3} of dk and dv of key q
  if (tok >= 0) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int c0 = 16 * dt + 4 * g;
      if (c0 < d) {
        F::st4(dqkv + tok * 3 * C + C + c0, ok[dt] * a.scale);
        F::st4(dqkv + tok * 3 * C + 2 * C + c0, ov[dt]);
      }
    }
  }
  if (!a.wsp) return;
  float* part = a.wsp + blk * a.slot;
  if (a.need_tab) {
    for (int idx = tid; idx < tw2; idx += NTH) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < NT; ++w) v += sBins[w * tw2 + idx];
      part[idx] = v;
    }
  }
  if (a.need_pad) {
    // rows of the padded tokens, summed in key order; a window without padding (uniform over the workgroup) writes zeros
    bool any = false;
    for (int r = 0; r < ws; ++r) any |= wrap(wi * ws + r + shift, a.Hp) >= a.H || wrap(wj * ws + r + shift, a.Wp) >= a.W;
    if (any) {
      float* rows = sAB;                                          // [N][PADS], 16 NT x 64 <= 2 x 16 NT x 36 floats
      if (isrow) {
        const bool padded = tok < 0;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const int c0 = 16 * dt + 4 * g;
          const v4f z = {0.f, 0.f, 0.f, 0.f};
          *reinterpret_cast<v4f*>(&rows[row * PADS + c0]) = padded ? ok[dt] * a.scale : z;
          *reinterpret_cast<v4f*>(&rows[row * PADS + DMAX + c0]) = padded ? ov[dt] : z;
        }
      }
      __syncthreads();
      if (tid < PADS) {
        float v = 0.f;
        for (int n = 0; n < N; ++n) v += rows[n * PADS + tid];
        part[tw2 + tid] = v;
      }
    } else if (tid < PADS) {
      part[tw2 + tid] = 0.f;
    }
  }
}

// dbias_table[bin][head] and dpad_qkv[{k, v}][head][channel] = the sum of the workgroups' partials of one head in a fixed order:
// slice sl adds windows sl, sl + 64, ... in that order, then the 64 slices are added in slice order.  grid (ceil(slot / 16), nH).
__global__ __launch_bounds__(RED_OUT* RED_SLICES) void k_swin_bwd_reduce(const float* wsp, float* dtable, float* dpad, int64_t nwin, int nH,
                                                                          int slot, int tw2, int C, int d) {
  __shared__ float sRed[RED_SLICES][RED_OUT];
  const int o = threadIdx.x % RED_OUT, sl = threadIdx.x / RED_OUT;
  const int head = blockIdx.y, j = blockIdx.x * RED_OUT + o;
  const bool wanted = j < slot && (j < tw2 ? dtable != nullptr : dpad != nullptr);
  float v = 0.f;
  if (wanted)
    for (int64_t w = sl; w < nwin; w += RED_SLICES) v += wsp[(w * nH + head) * slot + j];
  sRed[sl][o] = v;
  __syncthreads();
  if (sl == 0 && wanted) {
    float t = 0.f;
    for (int i = 0; i < RED_SLICES; ++i) t += sRed[i][o];
    if (j < tw2) {
      dtable[(int64_t)j * nH + head] = t;
    } else {
      const int third = 1 + (j - tw2) / DMAX, ch = (j - tw2) % DMAX;
      if (ch < d) dpad[third * C + head * d + ch] = t;
    }
  }
  if (dpad && blockIdx.x == 0 && (int)threadIdx.x < d) dpad[head * d + threadIdx.x] = 0.f;      // padded queries have no output
}

template <bool BF>
int launch(const BwdArgs& a, int nt, int64_t blocks, hipStream_t st) {
  const dim3 grid((unsigned)blocks);
#define PW_SWIN_BWD_CASE(NT_)                                                          \
  case NT_:                                                                            \
    hipLaunchKernelGGL((k_swin_attn_bwd<BF, NT_>), grid, dim3(64 * NT_), 0, st, a);     \
    break;
  switch (nt) {
    PW_SWIN_BWD_CASE(1)
    PW_SWIN_BWD_CASE(2)
    PW_SWIN_BWD_CASE(3)
    PW_SWIN_BWD_CASE(4)
    PW_SWIN_BWD_CASE(6)
    PW_SWIN_BWD_CASE(7)
    PW_SWIN_BWD_CASE(8)
    PW_SWIN_BWD_CASE(9)
    default:
      pw_set_error("pw_swin_window_attention_backward: no kernel for %d key tiles", nt);
      return PW_EUNSUP;
  }
#undef PW_SWIN_BWD_CASE
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_swin_attn_bwd<%d, %d>", (int)BF, nt);
  return 0;
}

}  // namespace

PW_API int pw_swin_window_attention_backward(const void* qkv, const void* pad_qkv, const float* bias_table, const void* out, const void* dout,
                                             void* dqkv, float* dpad_qkv, float* dbias_table, void* workspace, int64_t workspace_bytes,
                                             int B, int H, int W, int C, int num_heads, int ws, int shift, float scale, int dtype,
                                             void* stream) {
  PW_CHECK_ARG(qkv && bias_table && out && dout && dqkv, "pw_swin_window_attention_backward: null pointer");
  PW_CHECK_ARG(dtype == PW_SWIN_F32 || dtype == PW_SWIN_BF16,
               "pw_swin_window_attention_backward: dtype must be PW_SWIN_F32 or PW_SWIN_BF16, got %d", dtype);
  PW_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1 && num_heads >= 1,
               "pw_swin_window_attention_backward: B, H, W, C, num_heads must be positive");
  PW_CHECK_ARG(H <= 32767 && W <= 32767, "pw_swin_window_attention_backward: H and W must be at most 32767");
  PW_CHECK_ARG(C % num_heads == 0, "pw_swin_window_attention_backward: C = %d is no multiple of num_heads = %d", C, num_heads);
  const int d = C / num_heads;
  if (ws < 2 || ws > PW_SWIN_MAX_WS || d > PW_SWIN_MAX_HEAD_DIM || d % 4 != 0) {
    pw_set_error("pw_swin_window_attention_backward: window %d, head width %d not supported (2 <= ws <= %d, head width <= %d and a multiple of 4)",
                 ws, d, PW_SWIN_MAX_WS, PW_SWIN_MAX_HEAD_DIM);
    return PW_EUNSUP;
  }
  PW_CHECK_ARG(shift >= 0 && shift < ws, "pw_swin_window_attention_backward: need 0 <= shift < ws, got shift = %d, ws = %d", shift, ws);
  PW_CHECK_ARG(pad_qkv || !dpad_qkv, "pw_swin_window_attention_backward: dpad_qkv given although pad_qkv is NULL");
  const uintptr_t align = dtype == PW_SWIN_F32 ? 15 : 7;               // four channels per load / store
  PW_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dqkv | (uintptr_t)pad_qkv) & align) == 0,
               "pw_swin_window_attention_backward: qkv, pad_qkv, out, dout and dqkv must be %d-byte aligned", (int)align + 1);
  PW_CHECK_ARG((((uintptr_t)bias_table | (uintptr_t)dpad_qkv | (uintptr_t)dbias_table | (uintptr_t)workspace) & 3) == 0,
               "pw_swin_window_attention_backward: bias_table, dpad_qkv, dbias_table and workspace must be 4-byte aligned");
  BwdArgs a;
  a.qkv = qkv; a.pad = pad_qkv; a.table = bias_table; a.dout = dout; a.dqkv = dqkv;
  a.H = H; a.W = W; a.C = C; a.nH = num_heads; a.d = d; a.ws = ws; a.shift = shift;
  a.nWh = (H + ws - 1) / ws; a.nWw = (W + ws - 1) / ws;
  a.Hp = a.nWh * ws; a.Wp = a.nWw * ws;
  a.scale = scale;
  const int tw2 = (2 * ws - 1) * (2 * ws - 1);
  a.slot = tw2 + PADS;
  a.need_tab = dbias_table != nullptr;
  a.need_pad = dpad_qkv != nullptr;
  const int64_t nwin = (int64_t)B * a.nWh * a.nWw;
  const int64_t blocks = nwin * num_heads;
  PW_CHECK_ARG(blocks < ((int64_t)1 << 31), "pw_swin_window_attention_backward: B x windows x heads = %lld does not fit one launch",
               (long long)blocks);
  const bool reduce = a.need_tab || a.need_pad;
  const int64_t need = reduce ? blocks * a.slot * (int64_t)sizeof(float) : 0;
  PW_CHECK_ARG(!reduce || (workspace && workspace_bytes >= need),
               "pw_swin_window_attention_backward: workspace of %lld bytes needed, got %lld%s", (long long)need, (long long)workspace_bytes,
               workspace ? "" : " (NULL)");
  a.wsp = reduce ? static_cast<float*>(workspace) : nullptr;
  const int nt = (ws * ws + 15) / 16;
  hipStream_t st = pw_stream(stream);
  const int rc = dtype == PW_SWIN_BF16 ? launch<true>(a, nt, blocks, st) : launch<false>(a, nt, blocks, st);
  if (rc != 0 || !reduce) return rc;
  hipLaunchKernelGGL(k_swin_bwd_reduce, dim3((unsigned)pw_cdiv(a.slot, RED_OUT), (unsigned)num_heads), dim3(RED_OUT * RED_SLICES), 0, st,
                     a.wsp, dbias_table, dpad_qkv, nwin, num_heads, a.slot, tw2, C, d);
  PW_CHECK_LAUNCH();
  return 0;
}
