// ------------------------------------------------------------------------------------
// The optimizer step in two launches: global gradient norm, clipped AdamW, EMA of the freshly written weights.
//
// Replaces, for the whole model at once:
//   torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2)     one vector_norm per tensor, a stack, a norm, a foreach mul
//   torch.optim.AdamW.step()  (torch/optim/adam.py _single_tensor_adam, decoupled_weight_decay=True -- the arithmetic restated
//                              here; the foreach path is the same operations over tensor lists)
//   ModelEMA.update           (mmdet3d/core/hook/ema.py:48-59: `v *= d; v += (1 - d) * msd[k]` per floating state-dict entry)
//
// Both kernels walk a device-resident plan (layout in include/preworld_hip_optim.h): a row per tensor, and a chunk table that cuts the
// rows into pieces of at most PW_OPTIM_CHUNK elements, so a 4 M-element weight and a 128-element bias both spread over the grid.
// A plan passed by value would not fit the kernel-argument space at this model's tensor count, and would bake the addresses into
// a captured graph; the plan in memory is replaced by one copy when an address changes.  Blocks of 256 grid-stride over the chunks
// (min(n_chunks, 2048) blocks: the memory-bound sizing); a chunk whose addresses are all 16-byte aligned at its first element moves
// float4s, any other chunk (a view that starts 4 bytes off, a head, a short tensor) goes element by element, still coalesced.
//
// Launch 1 (k_optim_sqnorm): every block sums g*g of its chunks in double (per thread in chunk order, then a fixed shuffle tree and
// a fixed order over the four waves) and STORES the partial to slab[blockIdx.x].  No atomics: the same plan gives the same bits.
// Launch 2 (k_optim_update): every block sums the live slab entries in one fixed order (<= 2048 doubles, L2-resident), forms the
// clipping coefficient, and derives the per-group scalars in double from the device-resident step counters and hyper-parameters:
// no value crosses to the host, so step() never synchronises, and a changed lr is one small upload, not a new plan or capture.
// The last block to draw a ticket advances the counters: every block has read them before it draws.
//
// This file is compiled with -ffp-contract=off (build.EXTRA): the fp32 update is the written sequence of roundings, which is
// what tests/_optim_ref64.py restates; a contracted p*(1 - lr wd) or addcdiv would still pass a tolerance, but no longer be that.
// ------------------------------------------------------------------------------------
#include "pw_common.h"

#include <math.h>
#include <string.h>

#pragma clang fp contract(off)

namespace {
constexpr int OP_THREADS = 256;
constexpr int OP_WAVES = OP_THREADS / PW_WAVE;
constexpr int64_t OP_MAGIC = 0x50574f5054494d31ll;        // "PWOPTIM1"
constexpr int64_t OP_MAX_NUMEL = (int64_t)1 << 40;

struct Row {
  uintptr_t a[5];                                          // p, g, m, v, e
  int64_t numel;
};

// ---- host: the layout --------------------------------------------------------------------------------------------------
inline uintptr_t addr_of(const float* const* tab, int i) { return tab ? reinterpret_cast<uintptr_t>(tab[i]) : 0; }

// pieces of one row: an optional scalar head up to the common 16-byte boundary, then near-equal pieces (multiples of 4 elements, so
// an aligned row stays aligned at every piece).  emit(start, count, vec) is called in element order.
template <class F>
void row_pieces(const Row& r, F emit) {
  if (r.numel == 0) return;
  uintptr_t any = 0;
  bool same = true;
  int mis = -1;
  for (int k = 0; k < 5; ++k) {
    if (!r.a[k]) continue;
    any |= r.a[k];
    const int mk = (int)(r.a[k] & 15);
    if (mis < 0) mis = mk;
    same = same && mk == mis;
  }
  int64_t start = 0;
  bool vec = (any & 15) == 0;
  if (!vec && same && (mis & 3) == 0) {                   // every address is the same number of floats past a boundary
    const int64_t head = (16 - mis) / 4;
    if (r.numel > head) {
      emit((int64_t)0, head, false);
      start = head;
      vec = true;
    }
  }
  const int64_t rest = r.numel - start;
  const int64_t k = pw_cdiv(rest, PW_OPTIM_CHUNK);
  const int64_t piece = pw_cdiv(pw_cdiv(rest, k), 4) * 4;  // <= PW_OPTIM_CHUNK: the chunk size is a multiple of 4
  for (int64_t s = 0; s < rest; s += piece) emit(start + s, rest - s < piece ? rest - s : piece, vec);
}

int read_rows(const char* fn, int n, const int64_t* numel, const float* const* p, const float* const* g, const float* const* m,
              const float* const* v, const float* const* e, Row* rows, int64_t* n_chunks) {
  int64_t nc = 0;
  for (int i = 0; i < n; ++i) {
    Row& r = rows[i];
    r.numel = numel[i];
    PW_CHECK_ARG(r.numel >= 0 && r.numel <= OP_MAX_NUMEL, "%s: numel[%d] = %lld must lie in [0, 2^40]", fn, i, (long long)r.numel);
    r.a[0] = addr_of(p, i), r.a[1] = addr_of(g, i), r.a[2] = addr_of(m, i), r.a[3] = addr_of(v, i), r.a[4] = addr_of(e, i);
    const int n_opt = (r.a[1] != 0) + (r.a[2] != 0) + (r.a[3] != 0);
    PW_CHECK_ARG(r.numel == 0 || r.a[0], "%s: row %d has no p", fn, i);
    PW_CHECK_ARG(n_opt == 0 || n_opt == 3, "%s: row %d needs g, m and v, or none of them (an EMA-only row)", fn, i);
    PW_CHECK_ARG(r.numel == 0 || n_opt == 3 || r.a[4], "%s: row %d has neither a gradient nor a shadow", fn, i);
    for (int k = 0; k < 5; ++k) PW_CHECK_ARG((r.a[k] & 3) == 0, "%s: row %d holds an address that is not 4-byte aligned", fn, i);
    row_pieces(r, [&](int64_t, int64_t, bool) { ++nc; });
  }
  *n_chunks = nc;
  return PW_OK;
}

inline int64_t plan_words(int64_t n_rows, int64_t n_chunks) {
  return PW_OPTIM_HEADER_WORDS + n_rows * PW_OPTIM_ROW_WORDS + n_chunks * PW_OPTIM_CHUNK_WORDS;
}

inline int64_t bits_of(double d) {
  int64_t b;
  memcpy(&b, &d, 8);
  return b;
}

// ---- device ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double bits_to_double(int64_t b) { return __longlong_as_double(b); }

// sum of one double per thread over the block in a fixed order; every thread gets the result
__device__ __forceinline__ double block_sum(double x, double* red) {
  for (int off = PW_WAVE / 2; off > 0; off >>= 1) x = x + __shfl_xor(x, off);
  __syncthreads();                                          // red may still be read from an earlier call
  if ((threadIdx.x & (PW_WAVE - 1)) == 0) red[threadIdx.x / PW_WAVE] = x;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < OP_WAVES; ++w) s = s + red[w];
  return s;
}

__global__ void __launch_bounds__(OP_THREADS)
k_optim_sqnorm(const int64_t* __restrict__ plan, int n_rows, int64_t n_chunks, double* __restrict__ slab) {
  __shared__ double red[OP_WAVES];
  const int64_t* __restrict__ rows = plan + PW_OPTIM_HEADER_WORDS;
  const int64_t* __restrict__ chunks = rows + (int64_t)n_rows * PW_OPTIM_ROW_WORDS;
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t w0 = chunks[c * PW_OPTIM_CHUNK_WORDS];
    const int64_t r = w0 & 0xffffffffll;
    if (r >= n_rows) continue;
    const float* __restrict__ g = reinterpret_cast<const float*>(rows[r * PW_OPTIM_ROW_WORDS + 1]);
    if (!g) continue;                                       // EMA-only row
    const int64_t start = chunks[c * PW_OPTIM_CHUNK_WORDS + 1];
    const int cnt = (int)chunks[c * PW_OPTIM_CHUNK_WORDS + 2];
    g += start;
    int done = 0;
    if ((w0 >> 32) & 1) {
      const int nv = cnt >> 2;
      for (int i = tid; i < nv; i += OP_THREADS) {
        const float4 x = reinterpret_cast<const float4*>(g)[i];
        acc = acc + (double)x.x * (double)x.x;
        acc = acc + (double)x.y * (double)x.y;
        acc = acc + (double)x.z * (double)x.z;
        acc = acc + (double)x.w * (double)x.w;
      }
      done = nv << 2;
    }
    for (int i = done + tid; i < cnt; i += OP_THREADS) acc = acc + (double)g[i] * (double)g[i];
  }
  const double s = block_sum(acc, red);
  if (tid == 0) slab[blockIdx.x] = s;
}

struct GroupK {                                            // per parameter group, formed once per block
  double lr, bc1;
  float omb1, b2, omb2, bc2s, eps;
};

struct ElemK {                                             // per chunk
  float coef, decay, omb1, b2, omb2, bc2s, eps, nstep, d, omd;
};

__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const ElemK& k) {
  const float gg = k.coef * g;
  p = p * k.decay;
  m = m + (gg - m) * k.omb1;
  v = v * k.b2 + (k.omb2 * gg) * gg;
  const float den = sqrtf(v) / k.bc2s + k.eps;
  p = p + (k.nstep * m) / den;
}

__device__ __forceinline__ float ema1(float e, float p, const ElemK& k) { return e * k.d + k.omd * p; }

__global__ void __launch_bounds__(OP_THREADS)
k_optim_update(const int64_t* __restrict__ plan, int n_rows, int64_t n_chunks, const double* __restrict__ hyper, int n_groups,
               const double* __restrict__ slab, int n_slab, int use_norm, int clip, int use_ema, int skip_nonfinite,
               int64_t* ctr, int64_t* ema_updates, double* norm_out) {
  __shared__ double red[OP_WAVES];
  __shared__ GroupK sg[PW_OPTIM_MAX_GROUPS];
  const int64_t* __restrict__ rows = plan + PW_OPTIM_HEADER_WORDS;
  const int64_t* __restrict__ chunks = rows + (int64_t)n_rows * PW_OPTIM_ROW_WORDS;
  const int tid = threadIdx.x;

  // the counters are read before this block draws its ticket; the block that draws the last ticket writes them
  const int64_t t = *reinterpret_cast<volatile int64_t*>(ctr) + 1;
  const int64_t u = use_ema ? *reinterpret_cast<volatile int64_t*>(ema_updates) + 1 : 0;

  double total = 0.0;
  float coef = 1.0f;
  if (use_norm) {
    double part = 0.0;
    for (int i = tid; i < n_slab; i += OP_THREADS) part = part + slab[i];
    total = sqrt(block_sum(part, red));
    if (clip) {
      const double c = hyper[0] / (total + 1e-6);
      coef = (float)(c > 1.0 ? 1.0 : c);                   // a NaN stays a NaN, as through torch.clamp(max=1.0)
    }
  }
  if (tid < n_groups) {
    const double* __restrict__ h = hyper + PW_OPTIM_HYPER_GLOBAL + tid * PW_OPTIM_HYPER_GROUP;
    const double b1 = h[1], b2 = h[2];
    GroupK k;
    k.lr = h[0];
    k.bc1 = 1.0 - pow(b1, (double)t);
    k.omb1 = (float)(1.0 - b1);
    k.b2 = (float)b2;
    k.omb2 = (float)(1.0 - b2);
    k.bc2s = (float)sqrt(1.0 - pow(b2, (double)t));
    k.eps = (float)h[3];
    sg[tid] = k;
  }
  __syncthreads();
  const bool skipped = skip_nonfinite && use_norm && !isfinite(total);
  float d = 0.0f, omd = 0.0f;
  if (use_ema) {
    const double dd = hyper[1] * (1.0 - exp(-(double)u / 2000.0));
    d = (float)dd;
    omd = (float)(1.0 - dd);
  }

  if (!skipped) {
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
      const int64_t w0 = chunks[c * PW_OPTIM_CHUNK_WORDS];
      const int64_t r = w0 & 0xffffffffll;
      if (r >= n_rows) continue;
      const int64_t* __restrict__ row = rows + r * PW_OPTIM_ROW_WORDS;
      const int64_t start = chunks[c * PW_OPTIM_CHUNK_WORDS + 1];
      const int cnt = (int)chunks[c * PW_OPTIM_CHUNK_WORDS + 2];
      const bool vec = (w0 >> 32) & 1;
      float* __restrict__ p = reinterpret_cast<float*>(row[0]) + start;
      float* __restrict__ e = (use_ema && row[4]) ? reinterpret_cast<float*>(row[4]) + start : nullptr;
      const int group = (int)row[8];
      const int nv = vec ? cnt >> 2 : 0;
      ElemK k;
      k.coef = coef, k.d = d, k.omd = omd;
      if ((row[9] & 1) || !row[1]) {                       // EMA only: p is read, e is blended
        if (!e) continue;
        for (int i = tid; i < nv; i += OP_THREADS) {
          const float4 pp = reinterpret_cast<const float4*>(p)[i];
          float4 ee = reinterpret_cast<float4*>(e)[i];
          ee.x = ema1(ee.x, pp.x, k), ee.y = ema1(ee.y, pp.y, k), ee.z = ema1(ee.z, pp.z, k), ee.w = ema1(ee.w, pp.w, k);
          reinterpret_cast<float4*>(e)[i] = ee;
        }
        for (int i = (nv << 2) + tid; i < cnt; i += OP_THREADS) e[i] = ema1(e[i], p[i], k);
        continue;
      }
      if (group < 0 || group >= n_groups) continue;
      const float* __restrict__ g = reinterpret_cast<const float*>(row[1]) + start;
      float* __restrict__ m = reinterpret_cast<float*>(row[2]) + start;
      float* __restrict__ v = reinterpret_cast<float*>(row[3]) + start;
      const GroupK gk = sg[group];
      const double lr = gk.lr * bits_to_double(row[7]);
      k.decay = (float)(1.0 - lr * bits_to_double(row[6]));
      k.nstep = (float)(-(lr / gk.bc1));
      k.omb1 = gk.omb1, k.b2 = gk.b2, k.omb2 = gk.omb2, k.bc2s = gk.bc2s, k.eps = gk.eps;
      for (int i = tid; i < nv; i += OP_THREADS) {
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 pp = reinterpret_cast<float4*>(p)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        adamw1(pp.x, gg.x, mm.x, vv.x, k);
        adamw1(pp.y, gg.y, mm.y, vv.y, k);
        adamw1(pp.z, gg.z, mm.z, vv.z, k);
        adamw1(pp.w, gg.w, mm.w, vv.w, k);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        if (e) {
          float4 ee = reinterpret_cast<float4*>(e)[i];
          ee.x = ema1(ee.x, pp.x, k), ee.y = ema1(ee.y, pp.y, k), ee.z = ema1(ee.z, pp.z, k), ee.w = ema1(ee.w, pp.w, k);
          reinterpret_cast<float4*>(e)[i] = ee;
        }
      }
      for (int i = (nv << 2) + tid; i < cnt; i += OP_THREADS) {
        float pp = p[i], mm = m[i], vv = v[i];
        adamw1(pp, g[i], mm, vv, k);
        p[i] = pp, m[i] = mm, v[i] = vv;
        if (e) e[i] = ema1(e[i], pp, k);
      }
    }
  }

  __syncthreads();
  if (tid == 0) {
    if (blockIdx.x == 0 && use_norm && norm_out) *norm_out = total;
    __threadfence();
    const unsigned long long ticket = atomicAdd(reinterpret_cast<unsigned long long*>(ctr + 2), 1ull);
    if (ticket == (unsigned long long)gridDim.x - 1ull) {
      ctr[2] = 0;
      if (skipped) {
        ctr[1] += 1;
      } else {
        if (plan[5] > 0) ctr[0] = t;                        // the plan has optimizer rows
        if (use_ema) ema_updates[0] = u;
      }
    }
  }
}

int check_plan_args(const char* fn, const int64_t* plan, int64_t plan_bytes, int n_rows, int64_t n_chunks) {
  PW_CHECK_ARG(plan, "%s: plan is NULL", fn);
  PW_CHECK_ARG(n_rows >= 0 && n_chunks >= 0 && n_chunks <= INT32_MAX, "%s: n_rows = %d, n_chunks = %lld must be >= 0", fn, n_rows,
               (long long)n_chunks);
  PW_CHECK_ARG(plan_bytes == plan_words(n_rows, n_chunks) * 8, "%s: plan_bytes = %lld, a plan of %d rows and %lld chunks has %lld", fn,
               (long long)plan_bytes, n_rows, (long long)n_chunks, (long long)plan_words(n_rows, n_chunks) * 8);
  PW_CHECK_ARG((reinterpret_cast<uintptr_t>(plan) & 7) == 0, "%s: plan must be 8-byte aligned", fn);
  return PW_OK;
}
}  // namespace

PW_API int pw_optim_grid(int64_t n_chunks) {
  PW_CHECK_ARG(n_chunks >= 0, "pw_optim_grid: n_chunks = %lld", (long long)n_chunks);
  return (int)(n_chunks < PW_OPTIM_MAX_BLOCKS ? n_chunks : PW_OPTIM_MAX_BLOCKS);
}

PW_API int64_t pw_optim_plan_bytes(int n, const int64_t* numel_host, const float* const* p, const float* const* g,
                                   const float* const* m, const float* const* v, const float* const* e) {
  PW_CHECK_ARG(n >= 0, "pw_optim_plan_bytes: n = %d", n);
  PW_CHECK_ARG(n == 0 || (numel_host && p), "pw_optim_plan_bytes: numel_host / p is NULL");
  Row* rows = n ? new Row[n] : nullptr;
  int64_t nc = 0;
  const int rc = read_rows("pw_optim_plan_bytes", n, numel_host, p, g, m, v, e, rows, &nc);
  delete[] rows;
  return rc == PW_OK ? plan_words(n, nc) * 8 : (int64_t)rc;
}

PW_API int pw_optim_plan_layout(int n, const int64_t* numel_host, const float* const* p, const float* const* g,
                                const float* const* m, const float* const* v, const float* const* e, const double* wd_host,
                                const double* lr_mul_host, const int32_t* group_host, int64_t* plan_host, int64_t plan_bytes,
                                int64_t* n_chunks_host) {
  PW_CHECK_ARG(n >= 0, "pw_optim_plan_layout: n = %d", n);
  PW_CHECK_ARG(plan_host && n_chunks_host, "pw_optim_plan_layout: plan_host / n_chunks_host is NULL");
  PW_CHECK_ARG(n == 0 || (numel_host && p && wd_host && lr_mul_host && group_host), "pw_optim_plan_layout: a host array is NULL");
  Row* rows = n ? new Row[n] : nullptr;
  int64_t nc = 0;
  int rc = read_rows("pw_optim_plan_layout", n, numel_host, p, g, m, v, e, rows, &nc);
  for (int i = 0; rc == PW_OK && i < n; ++i)
    if (group_host[i] < 0 || group_host[i] >= PW_OPTIM_MAX_GROUPS || !(wd_host[i] == wd_host[i]) || !(lr_mul_host[i] == lr_mul_host[i])) {
      pw_set_error("pw_optim_plan_layout: row %d: group %d must lie in [0, %d), weight_decay and lr multiplier must be numbers", i,
                   group_host[i], PW_OPTIM_MAX_GROUPS);
      rc = PW_EINVAL;
    }
  if (rc == PW_OK && (nc > INT32_MAX || plan_bytes != plan_words(n, nc) * 8)) {
    pw_set_error("pw_optim_plan_layout: plan_bytes = %lld, this plan has %lld (pw_optim_plan_bytes)", (long long)plan_bytes,
                 (long long)plan_words(n, nc) * 8);
    rc = PW_EINVAL;
  }
  if (rc != PW_OK) {
    delete[] rows;
    return rc;
  }
  int64_t* w = plan_host;
  int64_t n_opt = 0;
  for (int i = 0; i < n; ++i) n_opt += rows[i].a[1] != 0 && rows[i].numel > 0;
  w[0] = OP_MAGIC, w[1] = n, w[2] = nc, w[3] = PW_OPTIM_CHUNK, w[4] = plan_words(n, nc), w[5] = n_opt, w[6] = 0, w[7] = 0;
  w += PW_OPTIM_HEADER_WORDS;
  for (int i = 0; i < n; ++i, w += PW_OPTIM_ROW_WORDS) {
    for (int k = 0; k < 5; ++k) w[k] = (int64_t)rows[i].a[k];
    w[5] = rows[i].numel;
    w[6] = bits_of(wd_host[i]);
    w[7] = bits_of(lr_mul_host[i]);
    w[8] = group_host[i];
    w[9] = rows[i].a[1] ? 0 : 1;
  }
  for (int i = 0; i < n; ++i)
    row_pieces(rows[i], [&](int64_t start, int64_t count, bool vec) {
      w[0] = (int64_t)i | ((int64_t)(vec ? 1 : 0) << 32);
      w[1] = start;
      w[2] = count;
      w += PW_OPTIM_CHUNK_WORDS;
    });
  *n_chunks_host = nc;
  delete[] rows;
  return PW_OK;
}

PW_API int pw_optim_sqnorm(const int64_t* plan, int64_t plan_bytes, int n_rows, int64_t n_chunks, double* slab, void* stream) {
  if (int rc = check_plan_args("pw_optim_sqnorm", plan, plan_bytes, n_rows, n_chunks)) return rc;
  PW_CHECK_ARG(slab, "pw_optim_sqnorm: slab is NULL");
  if (n_chunks == 0) return PW_OK;
  const int grid = pw_optim_grid(n_chunks);
  hipLaunchKernelGGL(k_optim_sqnorm, dim3((unsigned)grid), dim3(OP_THREADS), 0, pw_stream(stream), plan, n_rows, n_chunks, slab);
  PW_CHECK_LAUNCH();
  return PW_OK;
}

PW_API int pw_optim_update(const int64_t* plan, int64_t plan_bytes, int n_rows, int64_t n_chunks, const double* hyper, int n_groups,
                           const double* slab, int use_norm, int clip, int use_ema, int skip_nonfinite, int64_t* ctr,
                           int64_t* ema_updates, double* norm_out, void* stream) {
  if (int rc = check_plan_args("pw_optim_update", plan, plan_bytes, n_rows, n_chunks)) return rc;
  PW_CHECK_ARG(hyper && ctr, "pw_optim_update: hyper / ctr is NULL");
  PW_CHECK_ARG(n_groups >= 0 && n_groups <= PW_OPTIM_MAX_GROUPS, "pw_optim_update: n_groups = %d, at most %d", n_groups,
               PW_OPTIM_MAX_GROUPS);
  PW_CHECK_ARG(!use_norm || (slab && norm_out), "pw_optim_update: use_norm needs slab and norm_out");
  PW_CHECK_ARG(use_norm || !(clip || skip_nonfinite), "pw_optim_update: clip / skip_nonfinite need use_norm (and launch 1)");
  PW_CHECK_ARG(!use_ema || ema_updates, "pw_optim_update: use_ema needs ema_updates");
  if (n_chunks == 0) return PW_OK;
  const int grid = pw_optim_grid(n_chunks);
  hipLaunchKernelGGL(k_optim_update, dim3((unsigned)grid), dim3(OP_THREADS), 0, pw_stream(stream), plan, n_rows, n_chunks, hyper, n_groups,
                     slab, grid, use_norm ? 1 : 0, clip ? 1 : 0, use_ema ? 1 : 0, skip_nonfinite ? 1 : 0, ctr, ema_updates, norm_out);
  PW_CHECK_LAUNCH();
  return PW_OK;
}
