// Swin shifted-window attention (include/preworld_hip_swin.h) as one kernel: softmax(q k^T scale + bias + mask) v per (window, head),
// read from and written to the UN-padded, UN-rolled (B, H, W, .) token map.  Pad, roll, window partition, the relative-position
// index, the shift mask and their inverses are index arithmetic here (the header states them per token); nothing of size (N, N) and
// nothing in window order exists in global memory.
//
// One workgroup = one (window, head), NT = ceil(ws^2 / 16) waves; heads of one window are neighbouring workgroups, so the 128-byte
// head slices of a token are read by workgroups that run together.  The workgroup gathers K (row-major, rows padded so that the
// 16-byte fragment reads spread over the banks) and V TRANSPOSED ([d][key]) into LDS, zero-filled up to 32 channels and up to the
// padded key count, plus the head's column of the bias table and one word (r, c, region) per key.  Wave s then owns the 16 queries
// 16 s .. 16 s + 15 and works in the transposed orientation:
//     S^T = K Q^T   16 x 16 tiles, key tile t: lane (q = lane & 15, g = lane >> 4) gets keys 16 t + 4 g + {0..3} of ITS query q
// so a query's whole row of logits sits in one lane's registers and the lanes q, q + 16, q + 32, q + 48: the softmax is register
// work plus two cross-lane steps, and the (unnormalised) probabilities are already the B operand of
//     O^T = V^T P^T
// with the k index of that product permuted the way the accumulator tiles hold the keys (A reads V^T from LDS in the same order).
// O^T leaves four consecutive channels of one token in a lane: one 16-byte (8-byte for bf16) store per lane and 16-channel tile.
//
// PW_SWIN_F32 uses the fp32-input MFMA (v_mfma_f32_16x16x4_f32): bit for bit an fp32 fmaf chain, so the fp32 contract holds with
// no operand split, no prescale and no range state (inputs scaled by 2^-12 or 2^8 give the same bits scaled); at 1/16 of the
// fp16 rate it is still faster than the block's qkv traffic at the real stage shapes (profiles/swin_attention.md).
// PW_SWIN_BF16 uses v_mfma_f32_16x16x32_bf16 with two stacked key tiles per P^T fragment; logits, softmax and sums are fp32.
#include "pw_common.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf4 __attribute__((ext_vector_type(4)));

constexpr int DMAX = PW_SWIN_MAX_HEAD_DIM;                                   // channels per head held in LDS (zero-filled above d)
constexpr int TAB_MAX = (2 * PW_SWIN_MAX_WS - 1) * (2 * PW_SWIN_MAX_WS - 1);
constexpr unsigned KEY_PAD = 1u << 30;                                      // key word of a row beyond ws^2: no such key

struct SwinArgs {
  const void* qkv;
  const void* pad;
  const float* table;
  void* out;
  int H, W, C, nH, d, ws, shift, Hp, Wp, nWh, nWw;
  float scale;
};

__device__ __forceinline__ int wrap(int v, int n) { return v >= n ? v - n : v; }

template <bool BF>
struct Fmt;
template <>
struct Fmt<false> {
  typedef float elem;
  typedef v4f chunk;                 // four channels
  static constexpr int KS = 36;      // K row stride in elements: 144 B, 16-byte aligned, rows 16 apart in banks
  static constexpr int VPAD = 4;
};
template <>
struct Fmt<true> {
  typedef unsigned short elem;
  typedef u2v chunk;
  static constexpr int KS = 40;      // 80 B
  static constexpr int VPAD = 8;
};

template <bool BF, int NT>
__global__ __launch_bounds__(64 * NT) void k_swin_attn(const SwinArgs a) {
  typedef typename Fmt<BF>::elem E;
  typedef typename Fmt<BF>::chunk Chunk;
  constexpr int NK = 16 * NT;                                   // key rows of K: ws^2 rounded up to the tile
  constexpr int NKV = BF ? 32 * ((NT + 1) / 2) : NK;            // key columns of V^T: the bf16 product takes two tiles per step
  constexpr int KS = Fmt<BF>::KS, VS = NKV + Fmt<BF>::VPAD;
  __shared__ __attribute__((aligned(16))) E sK[NK * KS];
  __shared__ __attribute__((aligned(16))) E sVt[DMAX * VS];
  __shared__ __attribute__((aligned(16))) unsigned sKey[NK];
  __shared__ float sTab[TAB_MAX];

  const int tid = threadIdx.x;
  const int ws = a.ws, N = ws * ws, d = a.d, C = a.C, shift = a.shift;
  unsigned bid = blockIdx.x;
  const int head = bid % a.nH;
  bid /= a.nH;
  const int wj = bid % a.nWw;
  bid /= a.nWw;
  const int wi = bid % a.nWh;
  const int b = bid / a.nWh;
  const E* qkv = static_cast<const E*>(a.qkv) + (int64_t)b * a.H * a.W * 3 * C + head * d;
  const E* pad = a.pad ? static_cast<const E*>(a.pad) + head * d : nullptr;

  // ---- K, V^T, key words and the head's bias column into LDS; every word that is read later is written here
  for (int idx = tid; idx < NKV * (DMAX / 4); idx += 64 * NT) {
    const int n = idx >> 3, c4 = (idx & 7) * 4;
    Chunk kv = {}, vv = {};
    unsigned key = KEY_PAD;
    if (n < N) {
      const int r = n / ws, c = n - r * ws;
      const int i = wi * ws + r, j = wj * ws + c;
      const int si = wrap(i + shift, a.Hp), sj = wrap(j + shift, a.Wp);
      const int region = shift > 0 ? 3 * ((i >= a.Hp - ws) + (i >= a.Hp - shift)) + (j >= a.Wp - ws) + (j >= a.Wp - shift) : 0;
      key = (unsigned)r | (unsigned)c << 8 | (unsigned)region << 16;
      if (c4 < d) {
        if (si < a.H && sj < a.W) {
          const E* t = qkv + ((int64_t)si * a.W + sj) * 3 * C + c4;
          kv = *reinterpret_cast<const Chunk*>(t + C);
          vv = *reinterpret_cast<const Chunk*>(t + 2 * C);
        } else if (pad) {
          kv = *reinterpret_cast<const Chunk*>(pad + C + c4);
          vv = *reinterpret_cast<const Chunk*>(pad + 2 * C + c4);
        }
      }
    }
    if (n < NK) {
      *reinterpret_cast<Chunk*>(&sK[n * KS + c4]) = kv;
      if (c4 == 0) sKey[n] = key;
    }
    if constexpr (BF) {
#pragma unroll
      for (int e = 0; e < 4; ++e) sVt[(c4 + e) * VS + n] = (unsigned short)(vv[e >> 1] >> (16 * (e & 1)));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) sVt[(c4 + e) * VS + n] = vv[e];
    }
  }
  for (int idx = tid; idx < (2 * ws - 1) * (2 * ws - 1); idx += 64 * NT) sTab[idx] = a.table[(int64_t)idx * a.nH + head];
  __syncthreads();

  // ---- this wave's 16 queries
  const int lane = tid & 63, s = tid >> 6, q = lane & 15, g = lane >> 4;
  const int qa = 16 * s + q;
  int ra = 0, ca = 0, rga = 0;
  int64_t tok = -1;                                             // source token of the query, -1: padded token or no such row
  bool qrow = qa < N;
  if (qrow) {
    const unsigned key = sKey[qa];
    ra = key & 0xff;
    ca = (key >> 8) & 0xff;
    rga = (key >> 16) & 0xff;
    const int si = wrap(wi * ws + ra + shift, a.Hp), sj = wrap(wj * ws + ca + shift, a.Wp);
    if (si < a.H && sj < a.W) tok = (int64_t)si * a.W + sj;
  }
  const E* qsrc = tok >= 0 ? qkv + tok * 3 * C : (qrow ? pad : nullptr);      // q of the query's token; null: zeros

  v4f acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};

  if constexpr (BF) {
    // k = 8 g + j of the 16x16x32 product is channel 8 g + j for both operands
    u2v q0 = {0u, 0u}, q1 = {0u, 0u};
    if (qsrc && 8 * g < d) q0 = *reinterpret_cast<const u2v*>(qsrc + 8 * g);
    if (qsrc && 8 * g + 4 < d) q1 = *reinterpret_cast<const u2v*>(qsrc + 8 * g + 4);
    const bf8 qf = __builtin_bit_cast(bf8, (u4v){q0[0], q0[1], q1[0], q1[1]});
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const bf8 kf = __builtin_bit_cast(bf8, *reinterpret_cast<const u4v*>(&sK[(16 * t + q) * KS + 8 * g]));
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, acc[t], 0, 0, 0);
    }
  } else {
    // k = g of the 16x16x4 product number (h, e) is channel 16 h + 4 g + e for both operands
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      v4f qf = {0.f, 0.f, 0.f, 0.f};
      if (qsrc && 16 * h + 4 * g < d) qf = *reinterpret_cast<const v4f*>(qsrc + 16 * h + 4 * g);
      v4f kf[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) kf[t] = *reinterpret_cast<const v4f*>(&sK[(16 * t + q) * KS + 16 * h + 4 * g]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[t][e], qf[e], acc[t], 0, 0, 0);
    }
  }

  // ---- logits of query q against keys 16 t + 4 g + e, softmax over the lane's registers and the four lanes of the query
  const int tw = 2 * ws - 1;
  const int tbase = (ra + ws - 1) * tw + ca + ws - 1;
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const u4v kk = *reinterpret_cast<const u4v*>(&sKey[16 * t + 4 * g]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned key = kk[e];
      const int rb = key & 0xff, cb = (key >> 8) & 0xff, rgb = (key >> 16) & 0xff;
      float x = acc[t][e] * a.scale + sTab[tbase - rb * tw - cb];
      if (rgb != rga) x += -100.0f;
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

  // ---- O^T = V^T P^T: rows = channels, the k index = keys in the order the accumulator tiles hold them
  v4f o[2] = {v4f{0.f, 0.f, 0.f, 0.f}, v4f{0.f, 0.f, 0.f, 0.f}};
  if constexpr (BF) {
#pragma unroll
    for (int tt = 0; tt < (NT + 1) / 2; ++tt) {
      bf8 pf;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pf[e] = (__bf16)acc[2 * tt][e];
        pf[4 + e] = 2 * tt + 1 < NT ? (__bf16)acc[2 * tt + 1 < NT ? 2 * tt + 1 : 0][e] : (__bf16)0.f;
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const E* row = &sVt[(16 * dt + q) * VS + 32 * tt + 4 * g];
        const u2v v0 = *reinterpret_cast<const u2v*>(row), v1 = *reinterpret_cast<const u2v*>(row + 16);
        const bf8 vf = __builtin_bit_cast(bf8, (u4v){v0[0], v0[1], v1[0], v1[1]});
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
      }
    }
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const v4f v0 = *reinterpret_cast<const v4f*>(&sVt[q * VS + 16 * t + 4 * g]);
      const v4f v1 = *reinterpret_cast<const v4f*>(&sVt[(16 + q) * VS + 16 * t + 4 * g]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0[e], acc[t][e], o[0], 0, 0, 0);
        o[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1[e], acc[t][e], o[1], 0, 0, 0);
      }
    }
  }

  // ---- lane (q, g) holds channels 16 dt + 4 g + {0..3} of query q
  if (tok < 0) return;
  const float inv = 1.0f / sum;
  E* dst = static_cast<E*>(a.out) + ((int64_t)b * a.H * a.W + tok) * C + head * d;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    const int c0 = 16 * dt + 4 * g;
    if (c0 >= d) continue;
    const v4f r = o[dt] * inv;
    if constexpr (BF) {
      const bf4 h = {(__bf16)r[0], (__bf16)r[1], (__bf16)r[2], (__bf16)r[3]};
      *reinterpret_cast<u2v*>(dst + c0) = __builtin_bit_cast(u2v, h);
    } else {
      *reinterpret_cast<v4f*>(dst + c0) = r;
    }
  }
}

template <bool BF>
int launch(const SwinArgs& a, int nt, int64_t blocks, hipStream_t st) {
  const dim3 grid((unsigned)blocks);
#define PW_SWIN_CASE(NT_)                                                            \
  case NT_:                                                                          \
    hipLaunchKernelGGL((k_swin_attn<BF, NT_>), grid, dim3(64 * NT_), 0, st, a);       \
    break;
  switch (nt) {
    PW_SWIN_CASE(1)
    PW_SWIN_CASE(2)
    PW_SWIN_CASE(3)
    PW_SWIN_CASE(4)
    PW_SWIN_CASE(6)
    PW_SWIN_CASE(7)
    PW_SWIN_CASE(8)
    PW_SWIN_CASE(9)
    default:
      pw_set_error("pw_swin_window_attention: no kernel for %d key tiles", nt);
      return PW_EUNSUP;
  }
#undef PW_SWIN_CASE
  PW_CHECK_LAUNCH();
  pw_note_kernel("k_swin_attn<%d, %d>", (int)BF, nt);
  return 0;
}

}  // namespace

PW_API int pw_swin_window_attention(const void* qkv, const void* pad_qkv, const float* bias_table, void* out, int B, int H, int W, int C,
                                    int num_heads, int ws, int shift, float scale, int dtype, void* stream) {
  PW_CHECK_ARG(qkv && bias_table && out, "pw_swin_window_attention: null pointer");
  PW_CHECK_ARG(dtype == PW_SWIN_F32 || dtype == PW_SWIN_BF16, "pw_swin_window_attention: dtype must be PW_SWIN_F32 or PW_SWIN_BF16, got %d", dtype);
  PW_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1 && num_heads >= 1, "pw_swin_window_attention: B, H, W, C, num_heads must be positive");
  PW_CHECK_ARG(H <= 32767 && W <= 32767, "pw_swin_window_attention: H and W must be at most 32767");
  PW_CHECK_ARG(C % num_heads == 0, "pw_swin_window_attention: C = %d is no multiple of num_heads = %d", C, num_heads);
  const int d = C / num_heads;
  if (ws < 2 || ws > PW_SWIN_MAX_WS || d > PW_SWIN_MAX_HEAD_DIM || d % 4 != 0) {
    pw_set_error("pw_swin_window_attention: window %d, head width %d not supported (2 <= ws <= %d, head width <= %d and a multiple of 4)",
                 ws, d, PW_SWIN_MAX_WS, PW_SWIN_MAX_HEAD_DIM);
    return PW_EUNSUP;
  }
  PW_CHECK_ARG(shift >= 0 && shift < ws, "pw_swin_window_attention: need 0 <= shift < ws, got shift = %d, ws = %d", shift, ws);
  const uintptr_t align = dtype == PW_SWIN_F32 ? 15 : 7;               // four channels per load / store
  PW_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)pad_qkv) & align) == 0 && ((uintptr_t)bias_table & 3) == 0,
               "pw_swin_window_attention: qkv, pad_qkv and out must be %d-byte aligned", (int)align + 1);
  SwinArgs a;
  a.qkv = qkv; a.pad = pad_qkv; a.table = bias_table; a.out = out;
  a.H = H; a.W = W; a.C = C; a.nH = num_heads; a.d = d; a.ws = ws; a.shift = shift;
  a.nWh = (H + ws - 1) / ws; a.nWw = (W + ws - 1) / ws;
  a.Hp = a.nWh * ws; a.Wp = a.nWw * ws;
  a.scale = scale;
  const int64_t blocks = (int64_t)B * a.nWh * a.nWw * num_heads;
  PW_CHECK_ARG(blocks < ((int64_t)1 << 31), "pw_swin_window_attention: B x windows x heads = %lld does not fit one launch", (long long)blocks);
  const int nt = (ws * ws + 15) / 16;
  hipStream_t st = pw_stream(stream);
  return dtype == PW_SWIN_BF16 ? launch<true>(a, nt, blocks, st) : launch<false>(a, nt, blocks, st);
}
