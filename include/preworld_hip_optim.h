/*
 * preworld_hip_optim.h -- the optimizer-step part of the C ABI of libpreworld_hip.so; included by preworld_hip.h, whose
 * conventions hold: device pointers unless the name ends in _host, `stream` last, 0 or a negative PW_E* code with a thread-local message.
 * Kept in a file of its own so that the entry-point and pointer-parameter census of preworld_hip.h
 * (tests/test_marshal_cpu.py) stays what it was; preworld_amd/_lib.py parses both files the same way and
 * tests/test_optim_ref64_cpu.py holds this one to the same rules (every declaration parses, every pointer has a converter).
 */
#ifndef PREWORLD_HIP_OPTIM_H_
#define PREWORLD_HIP_OPTIM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * The optimizer step: gradient clipping by global L2 norm, AdamW and the EMA of the model in two launches with no host
 * synchronisation (capturable).  The kernels work from a device-resident PLAN: int64 words, laid out on the host by
 * pw_optim_plan_layout and uploaded by the caller with one copy.
 *   words [0, PW_OPTIM_HEADER_WORDS)      magic, n rows, n chunks, PW_OPTIM_CHUNK, total words, 0, 0, 0
 *   n rows of PW_OPTIM_ROW_WORDS          p, g, m (exp_avg), v (exp_avg_sq), e (EMA shadow or 0) as addresses; numel;
 *                                         weight_decay and lr multiplier (bit patterns of doubles); parameter group;
 *                                         flags (bit 0: EMA only -- p is only read, g / m / v are 0)
 *   n chunks of PW_OPTIM_CHUNK_WORDS      row | vector flag << 32; first element; element count (<= PW_OPTIM_CHUNK)
 * Every element of every row lies in exactly one chunk; a chunk carries the vector flag only if every non-null address of its
 * row is 16-byte aligned at the chunk's first element (a row whose addresses share one misalignment gets a scalar head chunk).
 * Blocks of 256 threads grid-stride over the chunks, pw_optim_grid(n_chunks) of them in both launches.
 * hyper: double[PW_OPTIM_HYPER_GLOBAL + PW_OPTIM_HYPER_GROUP * n_groups] on the device = max_norm, EMA decay, 0.., then per
 * parameter group lr, beta1, beta2, eps, 0..: read at every launch, so a changed lr needs no new plan.
 * ctr: int64[PW_OPTIM_CTR_WORDS] on the device = step count t, skipped steps, block ticket (0 between launches), 0. */
#define PW_OPTIM_CHUNK 8192
#define PW_OPTIM_MAX_BLOCKS 2048
#define PW_OPTIM_HEADER_WORDS 8
#define PW_OPTIM_ROW_WORDS 10
#define PW_OPTIM_CHUNK_WORDS 3
#define PW_OPTIM_HYPER_GLOBAL 8
#define PW_OPTIM_HYPER_GROUP 8
#define PW_OPTIM_MAX_GROUPS 64
#define PW_OPTIM_CTR_WORDS 4

/* blocks both launches use for a plan of n_chunks chunks (= live slab entries): min(n_chunks, PW_OPTIM_MAX_BLOCKS); -1: n_chunks < 0 */
int pw_optim_grid(int64_t n_chunks);

/* bytes of the plan pw_optim_plan_layout writes for these n tensors, or -1 (with the error message set) on a bad argument.  Pure host
 * arithmetic: the tables hold addresses that are looked at, never dereferenced.  numel_host int64[n]; p / g / m / v / e: n
 * addresses each, g / m / v entries 0 exactly for EMA-only rows, e entries 0 where there is no shadow (e itself may be NULL). */
int64_t pw_optim_plan_bytes(int n, const int64_t* numel_host, const float* const* p, const float* const* g, const float* const* m,
                            const float* const* v, const float* const* e);
/* lays the plan out into plan_host (plan_bytes = pw_optim_plan_bytes of the same arguments).  wd_host / lr_mul_host double[n],
 * group_host int32[n] in [0, PW_OPTIM_MAX_GROUPS).  n_chunks_host receives the chunk count.  Host only. */
int pw_optim_plan_layout(int n, const int64_t* numel_host, const float* const* p, const float* const* g, const float* const* m,
                         const float* const* v, const float* const* e, const double* wd_host, const double* lr_mul_host,
                         const int32_t* group_host, int64_t* plan_host, int64_t plan_bytes, int64_t* n_chunks_host);

/* Launch 1: slab[b] = sum over block b's chunks of g*g in double (fixed order inside a block: same bits on every run for one
 * plan); slab double[PW_OPTIM_MAX_BLOCKS].  With launch 2 this replaces torch.nn.utils.clip_grad_norm_(norm_type=2): one
 * vector_norm per tensor, a stack, a norm and a foreach multiply there. */
int pw_optim_sqnorm(const int64_t* plan, int64_t plan_bytes, int n_rows, int64_t n_chunks, double* slab, void* stream);

/* Launch 2.  use_norm != 0: total = sqrt(sum of the slab, fixed order) is written to norm_out, and with clip != 0
 * coef = min(1, max_norm / (total + 1e-6)) (clip_grad_norm_'s formula; a NaN total stays NaN) scales every gradient as it is READ --
 * the gradients in memory keep their values, unlike clip_grad_norm_.  Then per element in fp32, with t = ctr[0] + 1
 * (torch/optim/adam.py _single_tensor_adam with decoupled_weight_decay, what torch.optim.AdamW(foreach=False) runs):
 *   p *= 1 - lr wd;  m += (g' - m)(1 - b1);  v = v b2 + (1 - b2) g' g';  p += (-lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * and, where the row has a shadow (use_ema != 0), with u = ema_updates[0] + 1 (mmdet3d/core/hook/ema.py:48-59 ModelEMA.update):
 *   e = e d + (1 - d) p,  d = decay (1 - exp(-u / 2000))
 * EMA-only rows take only the last line.  The scalars are formed in double and rounded to float once, as torch's Python does.
 * The last block to finish advances ctr[0] (if the plan has optimizer rows) and ema_updates[0] (use_ema).
 * skip_nonfinite != 0 (needs use_norm): when total is not finite nothing is written but ctr[1] += 1.
 * norm_out (double[1]) may be NULL when use_norm == 0; ema_updates (int64[1]) may be NULL when use_ema == 0. */
int pw_optim_update(const int64_t* plan, int64_t plan_bytes, int n_rows, int64_t n_chunks, const double* hyper, int n_groups,
                    const double* slab, int use_norm, int clip, int use_ema, int skip_nonfinite, int64_t* ctr,
                    int64_t* ema_updates, double* norm_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PREWORLD_HIP_OPTIM_H_ */
