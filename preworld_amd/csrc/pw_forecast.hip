// State-conditioned temporal forecasting: the 6-step recursive decode of
// PreWorld4DTraj.simple_test (mmdet3d/models/detectors/preworld_temporal_traj.py:257-301,
// 329-368) as ONE kernel that keeps every voxel's 32-channel state in registers for all
// steps.  Modules replaced: plan_head (:121-127) and fusion_head (:128-132).
//
//   e      = plan_head(ego)                      21 -> 256 ReLU -> 256 ReLU -> 32   (per sample)
//   v_{k+1} = v_k + W2 softplus(W1[:, :32] v_k + (W1[:, 32:] e + b1)) + b2          (per voxel)
//
// The reference materialises repeat_interleave(e) (82 MB), cat (164 MB) and clone (82 MB) per
// step; here `W1[:, 32:] e + b1` is hoisted into a 128-vector c1 (e is voxel-invariant and the
// same for every step, :331-335) and the two GEMMs run on the exact-fp32 MFMA in TRANSPOSED
// form  D^T[feature][voxel] = W[feature][k] . V^T[k][voxel]  so that a lane always holds 16 of
// the 32 features of ONE voxel: rows (r&3) + 8*(r>>2) + 4*(lane>>5).  With the K index of the
// next GEMM enumerated in exactly that order, the D registers of one GEMM ARE the B operand of
// the next -- no LDS round trip, no shuffles, across all 6 steps:
//     v regs --W1a--> 4 x f32x16 hidden (softplus in place) --W2--> f32x16 + v  ->  v regs ...
// Weights are pre-packed per lane (pw_forecast_pack) and live in LDS (32 KB); c1/b2 enter as
// the MFMA C operand.  Each step's state is streamed out with 16-byte stores.
#include "pw_h2.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int C = 32;        // voxel feature width (out_dim)
constexpr int HID = 128;     // fusion_head hidden width (4*C)
constexpr int W1P = 4 * 4 * 64 * 4;   // packed W1a floats  [t][sq][lane][4]
constexpr int W2P = 4 * 4 * 64 * 4;   // packed W2  floats  [t][rq][lane][4]
}  // namespace

__device__ __forceinline__ int row_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// nn.Softplus(beta=1, threshold=20): x > 20 ? x : log1p(exp(x)), as
//     max(x, 0) + ln2 * log2(1 + exp2(-|x| * log2e))
// in SIX VALU instructions (v_mul with -|x| modifiers, v_exp, v_add, v_log, v_max, v_fma).
// Why so terse: on gfx950 the fp32-input MFMA runs on the SIMD's fp32 vector datapath, so every
// VALU instruction of ANY wave on the SIMD displaces matrix work (measured: 2.3k VALU per wave
// cost the conv kernel ~30% of its MFMA rate).  The libm log1pf(expf(x)) is ~100 instructions,
// a Cody-Waite + log1p-corrected version 21.
// Accuracy: the exp2 argument is <= 29 in magnitude where t matters, so its relative error
// (|arg| * 2^-24) stays below 2e-8 * t; rounding 1+t costs <= 6e-8 absolute.  Max abs error vs
// fp64 < 3e-7 over [-100, 100] (test_softplus_accuracy).  For x > 20 the correction term is
// < 2.1e-9 < half an ulp of x, so the threshold branch is the identity in fp32.
__device__ __forceinline__ float softplus_t20(float x) {
  const float t = __builtin_amdgcn_exp2f(-fabsf(x) * 1.44269504088896341f);
  return fmaf(__builtin_amdgcn_logf(1.f + t), 0.693147180559945309f, fmaxf(x, 0.f));
}

// ------------------------------------------------------------------------------------
// per-sample prologue: plan_head MLP and the hoisted ego term.  One block per sample.
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_forecast_prologue(const float* __restrict__ ego, int ego_dim, const float* __restrict__ w0,
                    const float* __restrict__ b0, const float* __restrict__ w2,
                    const float* __restrict__ b2, const float* __restrict__ w4,
                    const float* __restrict__ b4, const float* __restrict__ fw1,
                    const float* __restrict__ fb1, float* __restrict__ ego_feat,
                    float* __restrict__ c1, float* __restrict__ c1p) {
  __shared__ float h1[256], h2[256], e[C];
  const int t = threadIdx.x, s = blockIdx.x;
  const float* x = ego + (size_t)s * ego_dim;
  float acc = b0[t];
  for (int i = 0; i < ego_dim; ++i) acc += x[i] * w0[t * ego_dim + i];
  h1[t] = fmaxf(acc, 0.f);
  __syncthreads();
  acc = b2[t];
  for (int i = 0; i < 256; ++i) acc += h1[i] * w2[t * 256 + i];
  h2[t] = fmaxf(acc, 0.f);
  __syncthreads();
  if (t < C) {
    acc = b4[t];
    for (int i = 0; i < 256; ++i) acc += h2[i] * w4[t * 256 + i];
    e[t] = acc;
    ego_feat[(size_t)s * C + t] = acc;
  }
  __syncthreads();
  if (t < HID) {
    // cat order is [voxel_feats, ego_feats] (:339) -> ego weights are columns C..2C-1
    acc = fb1[t];
    for (int i = 0; i < C; ++i) acc += e[i] * fw1[t * 2 * C + C + i];
    c1[(size_t)s * HID + t] = acc;
    // D-register order for the main kernel: c1p[s][h][tile*16 + r] = c1[tile*32 + row_of(r,h)]
    const int tile = t >> 5, row = t & 31;
    const int h = (row >> 2) & 1, r = (row & 3) + 4 * (row >> 3);
    c1p[(size_t)s * HID + h * 64 + tile * 16 + r] = acc;
  }
}

// ------------------------------------------------------------------------------------
// weight packing into per-lane MFMA A-operand order (run once per weight update)
//   w1p[t][sq][lane][e] = W1[t*32 + (lane&31)][row_of(4*sq+e, lane>>5)]        (voxel part of W1)
//   w2p[t][rq][lane][e] = W2[lane&31][t*32 + row_of(4*rq+e, lane>>5)]
// ------------------------------------------------------------------------------------
__global__ void k_forecast_pack(const float* __restrict__ fw1, const float* __restrict__ fw2,
                                float* __restrict__ w1p, float* __restrict__ w2p) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= W1P) return;
  int e = idx & 3, lane = (idx >> 2) & 63, q = (idx >> 8) & 3, t = idx >> 10;
  int i = lane & 31, h = lane >> 5;
  int k = row_of(4 * q + e, h);
  w1p[idx] = fw1[(size_t)(t * 32 + i) * (2 * C) + k];
  w2p[idx] = fw2[(size_t)i * HID + t * 32 + k];
}

// ------------------------------------------------------------------------------------
// main kernel
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256, 4)
k_forecast(const float* __restrict__ v0, long long n_vox_per_sample, int n_samples,
           const float* __restrict__ w1p, const float* __restrict__ w2p,
           const float* __restrict__ c1p, const float* __restrict__ fb2, int n_steps,
           float* __restrict__ states /* [n_steps][n_samples*n_vox][C] */) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* l_w1 = lds;
  float* l_w2 = lds + W1P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, j = lane & 31;
  for (int k = tid; k < W1P / 4; k += 256) {
    reinterpret_cast<float4*>(l_w1)[k] = reinterpret_cast<const float4*>(w1p)[k];
    reinterpret_cast<float4*>(l_w2)[k] = reinterpret_cast<const float4*>(w2p)[k];
  }
  __syncthreads();

  const long long n_total = n_vox_per_sample * n_samples;
  const long long n_tiles = (n_total + 31) / 32;
  // b2 in D-register order for this lane half
  float b2r[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) b2r[s] = fb2[row_of(s, h)];

  for (long long tile = (long long)blockIdx.x * 4 + wave; tile < n_tiles;
       tile += (long long)gridDim.x * 4) {
    const long long m0 = tile * 32;
    long long m = m0 + j;
    const bool valid = m < n_total;
    if (!valid) m = n_total - 1;
    const int sample = (int)(m / n_vox_per_sample);
    const float* c1s = c1p + (size_t)sample * HID + h * 64;
    // this lane's 16 channels of its voxel: channel row_of(4q+e, h) = e + 8q + 4h
    float v[16];
    const float* src = v0 + (size_t)m * C + 4 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 t4 = *reinterpret_cast<const float4*>(src + 8 * q);
      v[4 * q + 0] = t4.x; v[4 * q + 1] = t4.y; v[4 * q + 2] = t4.z; v[4 * q + 3] = t4.w;
    }
    for (int step = 0; step < n_steps; ++step) {
      f32x16 o;
#pragma unroll
      for (int s = 0; s < 16; ++s) o[s] = b2r[s];
      // one 32-wide hidden tile at a time: GEMM1 tile -> softplus -> its K-slice of GEMM2,
      // so only 16 hidden registers are live; the loop stays rolled so that ~4 waves per SIMD
      // are resident and one wave's softplus (VALU) overlaps the others' MFMAs
#pragma unroll 1
      for (int t = 0; t < 4; ++t) {
        f32x16 hid;
        // C operand = hoisted ego term, already in D-register order
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 c4 = *reinterpret_cast<const float4*>(c1s + t * 16 + q * 4);
          hid[4 * q + 0] = c4.x; hid[4 * q + 1] = c4.y; hid[4 * q + 2] = c4.z; hid[4 * q + 3] = c4.w;
        }
#pragma unroll
        for (int sq = 0; sq < 4; ++sq) {
          const float4 a4 = *reinterpret_cast<const float4*>(l_w1 + ((t * 4 + sq) * 64 + lane) * 4);
          const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            hid = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], v[4 * sq + e], hid, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) hid[r] = softplus_t20(hid[r]);
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const float4 a4 = *reinterpret_cast<const float4*>(l_w2 + ((t * 4 + rq) * 64 + lane) * 4);
          const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            o = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], hid[4 * rq + e], o, 0, 0, 0);
        }
      }
#pragma unroll
      for (int s = 0; s < 16; ++s) v[s] = o[s] + v[s];   // residual connection (:342)
      if (valid) {
        float* dst = states + ((size_t)step * n_total + m) * C + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<float4*>(dst + 8 * q) =
              make_float4(v[4 * q + 0], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
      }
    }
  }
}

PW_API int pw_forecast_pack(const float* fusion_w1, const float* fusion_w2, float* w1p, float* w2p,
                            void* stream) {
  PW_CHECK_ARG(fusion_w1 && fusion_w2 && w1p && w2p, "pw_forecast_pack: null pointer");
  hipLaunchKernelGGL(k_forecast_pack, dim3(W1P / 256), dim3(256), 0, pw_stream(stream), fusion_w1,
                     fusion_w2, w1p, w2p);
  PW_CHECK_LAUNCH();
  return PW_OK;
}

PW_API int pw_forecast_prologue(const float* ego, int n_samples, int ego_dim, const float* plan_w0,
                                const float* plan_b0, const float* plan_w2, const float* plan_b2,
                                const float* plan_w4, const float* plan_b4, const float* fusion_w1,
                                const float* fusion_b1, float* ego_feat, float* c1, float* c1p,
                                void* stream) {
  PW_CHECK_ARG(ego && plan_w0 && plan_b0 && plan_w2 && plan_b2 && plan_w4 && plan_b4 && fusion_w1 &&
                   fusion_b1 && ego_feat && c1 && c1p,
               "pw_forecast_prologue: null pointer");
  PW_CHECK_ARG(n_samples > 0 && ego_dim > 0, "pw_forecast_prologue: bad sizes");
  hipLaunchKernelGGL(k_forecast_prologue, dim3(n_samples), dim3(256), 0, pw_stream(stream), ego,
                     ego_dim, plan_w0, plan_b0, plan_w2, plan_b2, plan_w4, plan_b4, fusion_w1,
                     fusion_b1, ego_feat, c1, c1p);
  PW_CHECK_LAUNCH();
  return PW_OK;
}

PW_API int pw_forecast_steps(const float* v0, int64_t n_vox_per_sample, int n_samples,
                             const float* w1p, const float* w2p, const float* c1p,
                             const float* fusion_b2, int n_steps, float* states, void* stream) {
  PW_CHECK_ARG(v0 && w1p && w2p && c1p && fusion_b2 && states, "pw_forecast_steps: null pointer");
  PW_CHECK_ARG(n_vox_per_sample > 0 && n_samples > 0 && n_steps > 0, "pw_forecast_steps: bad sizes");
  PW_CHECK_ARG((((uintptr_t)v0 | (uintptr_t)states | (uintptr_t)w1p | (uintptr_t)w2p) & 15) == 0,
               "pw_forecast_steps: pointers must be 16-B aligned");
  const size_t lds_bytes = (size_t)(W1P + W2P) * 4;   // 32 KB
  long long n_tiles = (n_vox_per_sample * n_samples + 31) / 32;
  long long want = (n_tiles + 3) / 4;
  // compute-bound on the fp32 MFMA: 4 blocks of 4 waves per CU saturate the 4 SIMDs
  unsigned nb = (unsigned)(want < 1280 ? want : 1280);   // 5 blocks x 256 CUs
  hipLaunchKernelGGL(k_forecast, dim3(nb), dim3(256), lds_bytes, pw_stream(stream), v0,
                     (long long)n_vox_per_sample, n_samples, w1p, w2p, c1p, fusion_b2, n_steps,
                     states);
  pw_note_kernel("k_forecast");
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// ------------------------------------------------------------------------------------
// The same recursion on the fp16 matrix cores with split-fp16 operands (pw_h2.h: x = hi + lo, three
// v_mfma_f32_32x32x16_f16 per product block, fp32 accumulate -- as accurate as an fp32 FMA chain at 5.3x the MFMA rate).
// Same transposed chain: block ks of the next GEMM's K index = accumulator registers 8 ks .. 8 ks + 7 of both lane
// halves, so a lane splits ITS OWN 8 registers into the 8 hi / 8 lo halves of its B fragment -- no LDS round trip, no
// shuffles.  Weights (A operand) are split and packed on the host (preworld_amd.ops.forecast_pack_h2):
//   w1p[t][ks][p][lane][e] = plane p of S1 * W1[t*32 + (lane&31)][row_of(8 ks + e, lane>>5)]
//   w2p[t][kb][p][lane][e] = plane p of S2 * W2[lane&31][t*32 + row_of(8 kb + e, lane>>5)]
// with power-of-two S1, S2 undone by inv1 / inv2 here.  With the MFMA time cut to ~1/5 the kernel is bound by its
// VALU work (softplus: 128 values per voxel and step, plus the splits).
// ------------------------------------------------------------------------------------
typedef _Float16 fh8 __attribute__((ext_vector_type(8)));
typedef _Float16 fh4 __attribute__((ext_vector_type(4)));
typedef float fv4 __attribute__((ext_vector_type(4)));
constexpr int WH2 = 4 * 2 * 2 * 64 * 4;     // floats per packed split matrix (16 KB)

// registers r0 .. r0+7 of an accumulator -> (8 hi halves, 8 lo halves); unsaturated, pair-wise like h2_split8 (pw_h2.h) so that the
// conversions become v_cvt_pk_f16_f32 and the residual a v_pk_add_f32: 7 instructions per 2 values instead of 10 (this kernel is
// VALU-bound: 80 splits per voxel and step)
__device__ __forceinline__ void split8(const float* x, fh8& hi, fh8& lo) {
  const float v[8] = {x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]};
  h8 a, b;
  h2_split8(v, a, b);
  hi = __builtin_bit_cast(fh8, a);
  lo = __builtin_bit_cast(fh8, b);
}

// split of 8 BOUNDED values (the hidden activations: at most 2^15 by construction, never Inf): hi = v_cvt_pk_f16_f32 per pair, lo =
// fp16(x - hi) as ONE v_fma_mixlo_f16 / v_fma_mixhi_f16 per value -- hi * -1 + x is exact in fp32 and rounded once into the fp16 half
// of the destination, the same bits as the convert-subtract-convert form of h2_split8, without its Inf guard (v_med3) and second
// convert: 1.5 instead of 3 VALU instructions per value in a kernel that is bound by them
__device__ __forceinline__ void split8_bounded(const float* x, fh8& hi, fh8& lo) {
  typedef _Float16 sh2 __attribute__((ext_vector_type(2)));
  typedef float sf2 __attribute__((ext_vector_type(2)));
  unsigned hp[4], lp[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const sf2 v = {x[2 * p], x[2 * p + 1]};
    hp[p] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, sh2));
    unsigned l;                              // (mixlo writes the low half, mixhi then the high half: no initialisation needed)
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(l) : "v"(hp[p]), "v"(v[0]));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l) : "v"(hp[p]), "v"(v[1]));
    lp[p] = l;
  }
  typedef unsigned su4 __attribute__((ext_vector_type(4)));
  hi = __builtin_bit_cast(fh8, su4{hp[0], hp[1], hp[2], hp[3]});
  lo = __builtin_bit_cast(fh8, su4{lp[0], lp[1], lp[2], lp[3]});
}

// softplus_t20(z) / 2^eh from zs = z / 2^eh:  max(zs, 0) + (ln2 / 2^eh) log2(1 + exp2(-|zs| 2^eh log2e)) -- the same six
// instructions, the hidden activations come out in the units they are split in (kexp = 2^eh log2e, kln = ln2 / 2^eh)
__device__ __forceinline__ float softplus_scaled(float zs, float kexp, float kln) {
  const float t = __builtin_amdgcn_exp2f(-fabsf(zs) * kexp);
  return fmaf(__builtin_amdgcn_logf(1.f + t), kln, fmaxf(zs, 0.f));
}

__global__ void __launch_bounds__(256, 2)
k_forecast_h2(const float* __restrict__ v0, long long n_vox_per_sample, int n_samples, const float* __restrict__ w1p,
              const float* __restrict__ w2p, float inv1, float inv2, const float* __restrict__ c1p,
              const float* __restrict__ fb2, int n_steps, float* __restrict__ states, int v0_h2, int out_h2,
              const int* __restrict__ v0_rng, int* __restrict__ st_rng, float w1_l1max) {
#ifdef PW_X_SKIP_FC             // ablation builds only
  return;
#endif
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* l_w1 = lds;
  float* l_w2 = lds + WH2;
  float* l_c1 = lds + 2 * WH2;               // the hoisted ego terms of all samples, in the hidden layer's units
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, j = lane & 31;
  // Range (pw_h2.h "Range").  The recursion runs in the units of the states' slot: u = v / 2^eu (eu = st_rng[0], calibrated by
  // the host from the largest state magnitude), so the split operand of every step sits in fp16's comfortable range whatever
  // the scale of the features.  The hidden activations softplus(z) are bounded A PRIORI, z <= ||W1a||_1 max|v| + max|c1|
  // with max|v| < 2^(16 + eu) (anything larger is Inf in h2 storage and flagged through the slot), and are computed directly in
  // units 2^eh that put this bound at 2^15.  All factors are powers of two folded into constants the loop already multiplies by.
  // (Loads first, uses behind the weight copy: the dependent chain costs no exposed latency.  Every wave derives the same eh.)
  const int e0 = v0_h2 ? rng_exp(v0_rng) : 0;
  const int eu = rng_exp(st_rng);
  unsigned cmb = 0u;
  for (int k = lane; k < n_samples * HID; k += 64) cmb = max(cmb, rng_absbits(c1p[k]));
  for (int k = tid; k < WH2 / 4; k += 256) {
    reinterpret_cast<float4*>(l_w1)[k] = reinterpret_cast<const float4*>(w1p)[k];
    reinterpret_cast<float4*>(l_w2)[k] = reinterpret_cast<const float4*>(w2p)[k];
  }
  int eh;
  {
    const float cmax = __uint_as_float(wave_umax(cmb));
    const float zb = fmaf(w1_l1max, rng_pow2(16 + eu), cmax + 1.f);
    int ex;
    (void)frexpf(zb, &ex);
    eh = __builtin_amdgcn_readfirstlane(ex) - 15;
    eh = eh < -100 ? -100 : (eh > 100 ? 100 : eh);
  }
  for (int k = tid; k < n_samples * HID; k += 256) l_c1[k] = c1p[k] * rng_pow2(-eh);
  __syncthreads();
  // wave-uniform constants, pinned to SGPRs (left in VGPRs they cost the kernel a wave of occupancy: 124 -> 160 VGPRs)
  auto uni_f = [](float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); };
  const float k_in = uni_f(rng_pow2(e0 - eu));                       // v0 as stored -> u
  const float k1 = uni_f(inv1 * rng_pow2(eu - eh));                  // (S1 W1a) u -> z / 2^eh
  const float k2 = uni_f(inv2 * rng_pow2(eh - eu));                  // (S2 W2) hs / 2^eh -> u
  const float kexp = uni_f(1.44269504088896341f * rng_pow2(eh)), kln = uni_f(0.693147180559945309f * rng_pow2(-eh));
  const float k_out = uni_f(rng_pow2(eu));                           // u -> true value (fp32 output)
  const long long n_total = n_vox_per_sample * n_samples;
  const long long n_tiles = (n_total + 31) / 32;
  float b2r[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) b2r[s] = fb2[row_of(s, h)] * rng_pow2(-eu);
  float amax = 0.f;
  unsigned lastbits = 0u;                    // |bits| of every voxel's last state: the non-finite ones `amax` cannot carry
  // A fragment (t, k-block, plane) of this lane: 16 bytes at ((t*2 + kb)*2 + p)*1024 + lane*16
  const char* a1 = reinterpret_cast<const char*>(l_w1) + lane * 16;
  const char* a2 = reinterpret_cast<const char*>(l_w2) + lane * 16;

  // TWO voxel tiles per wave and trip (round 4): the kernel is bound by its VALU work -- per hidden tile 16 softplus (two quarter-rate
  // transcendentals each) + 16 splits, ~1 050 issue cycles against 384 of MFMA -- and inside ONE tile everything is a dependent
  // chain MFMA -> softplus -> split -> MFMA.  With two independent tiles in the loop body one tile's softplus / split instructions
  // issue while the other tile's MFMAs execute.  The price is registers: the two-tile loop needs more than 168 (230 allocated under
  // this launch bound; bounds of 3 and 4 blocks per CU spill 96 and 312 bytes per lane), the 124 of the note above are the one-tile
  // loop -- more than two waves per SIMD are open to NU = 1 only (profiles/forecast_overlap.md).
  constexpr int NU = 2;
  const long long n_pairs = (n_tiles + NU - 1) / NU;
  for (long long pair = (long long)blockIdx.x * 4 + wave; pair < n_pairs; pair += (long long)gridDim.x * 4) {
    long long m[NU];
    bool valid[NU];
    const float* c1s[NU];
    float v[NU][16];
    fh8 vh[NU][2], vl[NU][2];               // split of the current state: GEMM operand of this step AND the h2 output of the last
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      m[u] = (pair * NU + u) * 32 + j;
      valid[u] = m[u] < n_total;
      if (!valid[u]) m[u] = n_total - 1;
      const int sample = (int)(m[u] / n_vox_per_sample);
      c1s[u] = l_c1 + (size_t)sample * HID + h * 64;
      if (v0_h2) {
        // h2 storage (pw_h2.h): channels 8 q + 4 h + 0..3 = the 8-byte group at slot 4 (q & 1) + 2 (q >> 1) + plane, byte 8 h
        const char* src = reinterpret_cast<const char*>(v0 + (size_t)m[u] * C) + 8 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int off = (4 * (q & 1) + 2 * (q >> 1)) * 16;
          const fh4 hi4 = *reinterpret_cast<const fh4*>(src + off), lo4 = *reinterpret_cast<const fh4*>(src + off + 16);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[u][4 * q + e] = ((float)hi4[e] + (float)lo4[e]) * k_in;
        }
      } else {
        const float* src = v0 + (size_t)m[u] * C + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float4 t4 = *reinterpret_cast<const float4*>(src + 8 * q);
          v[u][4 * q + 0] = t4.x * k_in; v[u][4 * q + 1] = t4.y * k_in; v[u][4 * q + 2] = t4.z * k_in; v[u][4 * q + 3] = t4.w * k_in;
        }
      }
      split8(v[u], vh[u][0], vl[u][0]);
      split8(v[u] + 8, vh[u][1], vl[u][1]);
    }
    for (int step = 0; step < n_steps; ++step) {
      f32x16 o[NU];
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int s = 0; s < 16; ++s) o[u][s] = 0.f;
#pragma unroll 1
      for (int t = 0; t < 4; ++t) {
        f32x16 hid[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int s = 0; s < 16; ++s) hid[u][s] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const fh8 wh = __builtin_bit_cast(fh8, *reinterpret_cast<const fv4*>(a1 + ((t * 2 + ks) * 2 + 0) * 1024));
          const fh8 wl = __builtin_bit_cast(fh8, *reinterpret_cast<const fv4*>(a1 + ((t * 2 + ks) * 2 + 1) * 1024));
#pragma unroll
          for (int u = 0; u < NU; ++u) {
            hid[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, vh[u][ks], hid[u], 0, 0, 0);
            hid[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, vh[u][ks], hid[u], 0, 0, 0);
            hid[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, vl[u][ks], hid[u], 0, 0, 0);
          }
        }
        fh8 hh[NU][2], hl[NU][2];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          float hs[16];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 c4 = *reinterpret_cast<const float4*>(c1s[u] + t * 16 + q * 4);
            hs[4 * q + 0] = softplus_scaled(fmaf(hid[u][4 * q + 0], k1, c4.x), kexp, kln);
            hs[4 * q + 1] = softplus_scaled(fmaf(hid[u][4 * q + 1], k1, c4.y), kexp, kln);
            hs[4 * q + 2] = softplus_scaled(fmaf(hid[u][4 * q + 2], k1, c4.z), kexp, kln);
            hs[4 * q + 3] = softplus_scaled(fmaf(hid[u][4 * q + 3], k1, c4.w), kexp, kln);
          }
#ifdef PW_X_FC_OLD_SPLIT                      // A/B builds only (tools/build_variant.py)
          split8(hs, hh[u][0], hl[u][0]);
          split8(hs + 8, hh[u][1], hl[u][1]);
#else
          split8_bounded(hs, hh[u][0], hl[u][0]);
          split8_bounded(hs + 8, hh[u][1], hl[u][1]);
#endif
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          const fh8 wh = __builtin_bit_cast(fh8, *reinterpret_cast<const fv4*>(a2 + ((t * 2 + kb) * 2 + 0) * 1024));
          const fh8 wl = __builtin_bit_cast(fh8, *reinterpret_cast<const fv4*>(a2 + ((t * 2 + kb) * 2 + 1) * 1024));
#pragma unroll
          for (int u = 0; u < NU; ++u) {
            o[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, hh[u][kb], o[u], 0, 0, 0);
            o[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, hh[u][kb], o[u], 0, 0, 0);
            o[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, hl[u][kb], o[u], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < NU; ++u) {
#pragma unroll
        for (int s = 0; s < 16; ++s) v[u][s] = fmaf(o[u][s], k2, b2r[s]) + v[u][s];   // + b2, residual connection (:342)
        split8(v[u], vh[u][0], vl[u][0]);
        split8(v[u] + 8, vh[u][1], vl[u][1]);
        if (valid[u]) {
#pragma unroll
          for (int s = 0; s < 16; ++s) amax = fmaxf(amax, fabsf(v[u][s]));
          if (out_h2) {
            // h2 storage: a 16-byte slot holds 8 channels of one plane, but this lane has only 4 of them (8 q + 4 h + e) and its
            // partner lane (l ^ 32, same voxel) the other 4.  One v_permlane32_swap per dword trades the pieces so that lane half
            // h ends up with both pieces of the slots of q = 2 h, 2 h + 1: four 16-byte stores like the fp32 layout.
            fh4 hi4[4], lo4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                hi4[q][e] = vh[u][q >> 1][4 * (q & 1) + e];
                lo4[q][e] = vl[u][q >> 1][4 * (q & 1) + e];
              }
            char* dst = reinterpret_cast<char*>(states + ((size_t)step * n_total + m[u]) * C);
#pragma unroll
            for (int qq = 0; qq < 2; ++qq)
#pragma unroll
              for (int p = 0; p < 2; ++p) {
                typedef unsigned fu2 __attribute__((ext_vector_type(2)));
                typedef unsigned fu4 __attribute__((ext_vector_type(4)));
                const fu2 a = __builtin_bit_cast(fu2, p ? lo4[qq] : hi4[qq]), b = __builtin_bit_cast(fu2, p ? lo4[qq + 2] : hi4[qq + 2]);
                const auto s0 = __builtin_amdgcn_permlane32_swap(a[0], b[0], false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(a[1], b[1], false, false);
                fu4 slot;
                slot[0] = s0[0]; slot[1] = s1[0]; slot[2] = s0[1]; slot[3] = s1[1];      // channels +0..3 | +4..7
                *reinterpret_cast<fu4*>(dst + (4 * qq + 2 * h + p) * 16) = slot;
              }
          } else {
            float* dst = states + ((size_t)step * n_total + m[u]) * C + 4 * h;
#pragma unroll
            for (int q = 0; q < 4; ++q)
              *reinterpret_cast<float4*>(dst + 8 * q) = make_float4(v[u][4 * q + 0] * k_out, v[u][4 * q + 1] * k_out, v[u][4 * q + 2] * k_out,
                                                                    v[u][4 * q + 3] * k_out);
          }
        }
      }
    }
    // v_max_f32 drops a NaN, so `amax` alone would leave a slot that looks healthy over states full of NaN (pw_h2.h: a NaN is recorded
    // as such).  NaN and Inf are sticky through the residual recursion: the LAST state of a voxel tells, once per trip instead of per step.
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (valid[u]) {
#pragma unroll
        for (int s = 0; s < 16; ++s) lastbits = max(lastbits, rng_absbits(v[u][s]));
      }
  }
  rng_note(st_rng, max(__float_as_uint(amax), lastbits), eu);
}

PW_API int pw_forecast_steps_h2(const float* v0, int64_t n_vox_per_sample, int n_samples, const float* w1p,
                                const float* w2p, float inv1, float inv2, const float* c1p, const float* fusion_b2,
                                int n_steps, float* states, int v0_h2, int out_h2, const int32_t* v0_rng, int32_t* states_rng,
                                float w1_l1max, void* stream) {
  PW_CHECK_ARG(v0 && w1p && w2p && c1p && fusion_b2 && states, "pw_forecast_steps_h2: null pointer");
  PW_CHECK_ARG(n_vox_per_sample > 0 && n_samples > 0 && n_samples <= 64 && n_steps > 0, "pw_forecast_steps_h2: bad sizes (<= 64 samples)");
  PW_CHECK_ARG(w1_l1max >= 0.f, "pw_forecast_steps_h2: w1_l1max = max row L1 norm of fusion_head.0.weight[:, :32]");
  PW_CHECK_ARG((((uintptr_t)v0 | (uintptr_t)states | (uintptr_t)w1p | (uintptr_t)w2p) & 15) == 0,
               "pw_forecast_steps_h2: pointers must be 16-B aligned");
  const size_t lds_bytes = (size_t)2 * WH2 * 4 + (size_t)n_samples * HID * 4;   // 32 KB + the scaled ego terms
  long long n_tiles = (n_vox_per_sample * n_samples + 31) / 32;
  long long want = ((n_tiles + 1) / 2 + 3) / 4;            // a wave takes two tiles per trip
  unsigned nb = (unsigned)(want < 512 ? want : 512);     // 2 resident blocks x 256 CUs, grid-stride: 10 000 tile pairs at C3 = 4.9 trips per wave
  hipLaunchKernelGGL(k_forecast_h2, dim3(nb), dim3(256), lds_bytes, pw_stream(stream), v0, (long long)n_vox_per_sample,
                     n_samples, w1p, w2p, inv1, inv2, c1p, fusion_b2, n_steps, states, v0_h2, out_h2, v0_rng, states_rng, w1_l1max);
  pw_note_kernel("k_forecast_h2");
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// ------------------------------------------------------------------------------------
// A12  attribute projection: density_mlp / semantic_mlp / color_mlp
// (mmdet3d/models/detectors/preworld_temporal_traj.py:81-104, used at :231-250 and in
// forward_train before the render head).  The three 32 -> 64 Softplus -> {2,17,3} MLPs run as
// one transposed MFMA chain: hidden = 192 rows (6 tiles), outputs = 32 rows of a block-
// diagonal second layer (22 used).  The result is written as ONE packed channels-last grid
//   [voxel][24] = { density_prob[0..1], semantic[0..16], color[0..2], 0, 0 }
// which is exactly what pw_render_rays gathers from (96 B per corner).
// ------------------------------------------------------------------------------------
constexpr int ATTR_TILES = 6;
constexpr int ATTR_WP = ATTR_TILES * 4 * 64 * 4;    // 6144 floats per packed matrix
constexpr int ATTR_GC = 24;

__global__ void __launch_bounds__(256, 3)
k_attr_mlp(const float* __restrict__ v0, long long n_vox, const float* __restrict__ w1p,
           const float* __restrict__ w2p, const float* __restrict__ b1p /* [2][96] */,
           const float* __restrict__ b2 /* [32] */, int final_softplus, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* l_w1 = lds;
  float* l_w2 = lds + ATTR_WP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, j = lane & 31;
  for (int k = tid; k < ATTR_WP / 4; k += 256) {
    reinterpret_cast<float4*>(l_w1)[k] = reinterpret_cast<const float4*>(w1p)[k];
    reinterpret_cast<float4*>(l_w2)[k] = reinterpret_cast<const float4*>(w2p)[k];
  }
  __syncthreads();
  float b2r[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) b2r[s] = b2[row_of(s, h)];
  const float* b1s = b1p + h * (ATTR_TILES * 16);
  const long long n_tiles = (n_vox + 31) / 32;
  for (long long tile = (long long)blockIdx.x * 4 + wave; tile < n_tiles;
       tile += (long long)gridDim.x * 4) {
    long long m = tile * 32 + j;
    const bool valid = m < n_vox;
    if (!valid) m = n_vox - 1;
    float v[16];
    const float* src = v0 + (size_t)m * C + 4 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 t4 = *reinterpret_cast<const float4*>(src + 8 * q);
      v[4 * q + 0] = t4.x; v[4 * q + 1] = t4.y; v[4 * q + 2] = t4.z; v[4 * q + 3] = t4.w;
    }
    f32x16 o;
#pragma unroll
    for (int s = 0; s < 16; ++s) o[s] = b2r[s];
#pragma unroll 1
    for (int t = 0; t < ATTR_TILES; ++t) {
      f32x16 hid;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 c4 = *reinterpret_cast<const float4*>(b1s + t * 16 + q * 4);
        hid[4 * q + 0] = c4.x; hid[4 * q + 1] = c4.y; hid[4 * q + 2] = c4.z; hid[4 * q + 3] = c4.w;
      }
#pragma unroll
      for (int sq = 0; sq < 4; ++sq) {
        const float4 a4 = *reinterpret_cast<const float4*>(l_w1 + ((t * 4 + sq) * 64 + lane) * 4);
        const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          hid = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], v[4 * sq + e], hid, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) hid[r] = softplus_t20(hid[r]);
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const float4 a4 = *reinterpret_cast<const float4*>(l_w2 + ((t * 4 + rq) * 64 + lane) * 4);
        const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], hid[4 * rq + e], o, 0, 0, 0);
      }
    }
    if (final_softplus && h == 0) {           // rows 0,1 = density_prob live in lane half 0, regs 0,1
      o[0] = softplus_t20(o[0]);
      o[1] = softplus_t20(o[1]);
    }
    if (valid) {
      float* dst = out + (size_t)m * ATTR_GC + 4 * h;
#pragma unroll
      for (int q = 0; q < 3; ++q)             // rows 8q+4h .. +3 for q = 0..2 cover channels 0..23
        *reinterpret_cast<float4*>(dst + 8 * q) =
            make_float4(o[4 * q + 0], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
  }
}

PW_API int pw_attr_mlp(const float* v0, int64_t n_vox, const float* w1p, const float* w2p,
                       const float* b1p, const float* b2, int final_softplus, float* out,
                       void* stream) {
  PW_CHECK_ARG(v0 && w1p && w2p && b1p && b2 && out && n_vox > 0, "pw_attr_mlp: bad arguments");
  PW_CHECK_ARG((((uintptr_t)v0 | (uintptr_t)out | (uintptr_t)w1p | (uintptr_t)w2p) & 15) == 0,
               "pw_attr_mlp: pointers must be 16-B aligned");
  const size_t lds_bytes = (size_t)ATTR_WP * 2 * 4;    // 48 KB
  long long want = ((n_vox + 31) / 32 + 3) / 4;
  unsigned nb = (unsigned)(want < 768 ? want : 768);    // 3 blocks x 256 CUs
  hipLaunchKernelGGL(k_attr_mlp, dim3(nb), dim3(256), lds_bytes, pw_stream(stream), v0,
                     (long long)n_vox, w1p, w2p, b1p, b2, final_softplus, out);
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// elementwise nn.Softplus(beta=1, threshold=20) with the same device function the fused
// kernels use (exposed for the attribute MLPs and for accuracy tests)
__global__ void k_softplus(const float* __restrict__ x, float* __restrict__ y, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = softplus_t20(x[i]);
}

PW_API int pw_softplus(const float* x, float* y, int64_t n, void* stream) {
  PW_CHECK_ARG(x && y && n > 0, "pw_softplus: bad arguments");
  hipLaunchKernelGGL(k_softplus, dim3((unsigned)pw_cdiv(n, 256)), dim3(256), 0, pw_stream(stream), x,
                     y, (long long)n);
  PW_CHECK_LAUNCH();
  return PW_OK;
}

// ------------------------------------------------------------------------------------
// A20  trajectory branch helpers (train-time only, tiny): global average pool + dense layers
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_global_avgpool(const float* __restrict__ x, int64_t n_vox, int C, float* __restrict__ y) {
  // block = one sample; thread = one channel (coalesced over channels), voxels in order
  const float* xb = x + (size_t)blockIdx.x * n_vox * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    for (int64_t v = 0; v < n_vox; ++v) s += xb[v * C + c];
    y[(size_t)blockIdx.x * C + c] = s / (float)n_vox;
  }
}

__global__ void __launch_bounds__(256)
k_linear_act(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
             float* __restrict__ y, int n_in, int n_out, int act) {
  const float* xr = x + (size_t)blockIdx.x * n_in;
  for (int o = threadIdx.x; o < n_out; o += blockDim.x) {
    float acc = b ? b[o] : 0.f;
    const float* wo = w + (size_t)o * n_in;
    for (int k = 0; k < n_in; ++k) acc += xr[k] * wo[k];
    if (act == 1) acc = fmaxf(acc, 0.f);
    else if (act == 2) acc = softplus_t20(acc);
    y[(size_t)blockIdx.x * n_out + o] = acc;
  }
}

PW_API int pw_global_avgpool_ndhwc(const float* x, int B, int64_t n_vox, int C, float* y, void* stream) {
  PW_CHECK_ARG(x && y && B > 0 && n_vox > 0 && C > 0, "pw_global_avgpool_ndhwc: bad arguments");
  hipLaunchKernelGGL(k_global_avgpool, dim3((unsigned)B), dim3(256), 0, pw_stream(stream), x, n_vox, C, y);
  PW_CHECK_LAUNCH();
  return PW_OK;
}

PW_API int pw_linear_act(const float* x, const float* w, const float* b, float* y, int rows, int n_in,
                         int n_out, int act, void* stream) {
  PW_CHECK_ARG(x && w && y && rows > 0 && n_in > 0 && n_out > 0, "pw_linear_act: bad arguments");
  PW_CHECK_ARG(act >= 0 && act <= 2, "pw_linear_act: act must be 0 (none), 1 (ReLU) or 2 (Softplus)");
  hipLaunchKernelGGL(k_linear_act, dim3((unsigned)rows), dim3(256), 0, pw_stream(stream), x, w, b, y, n_in,
                     n_out, act);
  PW_CHECK_LAUNCH();
  return PW_OK;
}
