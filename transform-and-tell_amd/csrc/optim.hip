// Multi-tensor BertAdam over flat fp32 buffers (optimizer `bert_adam` of
// expt/nytimes/9_transformer_objects/config.yaml:126-149; update rule of
// pytorch_pretrained_bert.BertAdam - third-party, restated, parity unpinned):
//   per tensor:  g <- g * min(1, max_grad_norm / (||g||_2 + 1e-6))       (per-TENSOR clip)
//   m <- b1 m + (1-b1) g ;  v <- b2 v + (1-b2) g^2      (no bias correction)
//   p <- p - lr_t * ( m / (sqrt(v) + eps) + wd * p )
// Layout: every tensor starts at a multiple of CHUNK elements inside the flat
// buffers (zero padded), so a chunk belongs to exactly one tensor.  HBM-bound:
// 4 reads + 3 writes of fp32 per element.
#include "common.h"
#include "options.h"

#define OPT_CHUNK 1024
// MEASURED (MI355X, same box, round 5): on bare buffers of the decoder's size (tools/probes/stream_probe.hip, 176 M
// parameters, 34 B each) one chunk per iteration 1108 us = 5.66 TB/s, four chunks per iteration 1032 us, four chunks + non-
// temporal loads / stores 1003 us = 6.26 TB/s (a float4 copy on that box: 5.3-5.7 TB/s); decoder half of the step alone
// (tools/decoder_profile.py, TELL_ADAM_VAR = 0..4): 6.93 / 6.82 / 6.75 / 6.80 / 6.73 ms.
#define TELL_ADAM_DEFAULT 4
#include <stdlib.h>
#include <type_traits>

// partial[c] = sum of squares of (grad * grad_scale) over chunk c
// (wire != NULL: the gradient of this step is the bf16 buffer the data-parallel exchange left - read it as it is
//  instead of widening 2 B/param back into the fp32 buffer first)
__device__ __forceinline__ float4 load_grad4(const float* __restrict__ grad, const uint16_t* __restrict__ wire, long o) {
  if (wire) {
    const uint2 w = reinterpret_cast<const uint2*>(wire)[o];
    return make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                       __uint_as_float(w.y & 0xffff0000u));
  }
  return reinterpret_cast<const float4*>(grad)[o];
}
// U chunks per block iteration, every load of the iteration in flight before the first reduction (one chunk per iteration
// left a block with a single 16-byte load outstanding per thread between two barriers)
// One trip of one 256-thread block: chunks c0 .. c0 + U - 1 (those below n_chunks; none of them: two barriers and nothing
// else).  tid: the thread's index in the block; red: the block's own U x 4 floats of LDS.
template <int U>
__device__ __forceinline__ void sqsum_chunks_trip(const float* __restrict__ grad, const uint16_t* __restrict__ wire,
                                                  long n_chunks, float grad_scale, float* __restrict__ partial, long c0,
                                                  int tid, float (*red)[4]) {
  float4 g[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    g[u] = c0 + u < n_chunks ? load_grad4(grad, wire, (c0 + u) * OPT_CHUNK / 4 + tid) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    // Every multiply-add spelled out, none left to the compiler's contraction, which chose differently in the wide and the
    // narrow kernel.  This is the arithmetic the wide kernel always had: the first chunk of a trip unfused, the others as
    // one chain of multiply-adds that starts from y * y.
#pragma clang fp contract(off)
    float s;
    if (u == 0) s = ((g[u].x * g[u].x + g[u].y * g[u].y) + g[u].z * g[u].z) + g[u].w * g[u].w;
    else s = __builtin_fmaf(g[u].w, g[u].w, __builtin_fmaf(g[u].z, g[u].z, __builtin_fmaf(g[u].x, g[u].x, g[u].y * g[u].y)));
    s = (s * grad_scale) * grad_scale;
    s = wave_sum(s);
    if ((tid & 63) == 0) red[u][tid >> 6] = s;
  }
  __syncthreads();
  if (tid < U && c0 + tid < n_chunks) partial[c0 + tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
  __syncthreads();
}
template <int U>
__global__ __launch_bounds__(256) void sqsum_chunks_kernel(const float* __restrict__ grad, const uint16_t* __restrict__ wire,
                                                           long n_chunks, float grad_scale, float* __restrict__ partial) {
  __shared__ float red[U][4];
  for (long c0 = (long)blockIdx.x * U; c0 < n_chunks; c0 += (long)gridDim.x * U)
    sqsum_chunks_trip<U>(grad, wire, n_chunks, grad_scale, partial, c0, threadIdx.x, red);
}
// Narrow form (common.h): quarter q of a 1024-thread workgroup is virtual block vb0 + q of the wide launch's nvb.  The trip
// count is that of vb0, the largest of the four, and a quarter with nothing left (or with no virtual block at all) runs its
// trips past n_chunks: every thread reaches every barrier.
template <int U>
__global__ __launch_bounds__(1024) void sqsum_chunks_narrow_kernel(const float* __restrict__ grad,
                                                                   const uint16_t* __restrict__ wire, long n_chunks,
                                                                   float grad_scale, float* __restrict__ partial, long nvb) {
  __shared__ float red[4][U][4];
  const int q = tell_quarter(), tid = threadIdx.x & 255;
  for (long vb0 = (long)blockIdx.x * 4; vb0 < nvb; vb0 += (long)gridDim.x * 4)
    for (long c0 = vb0 * U; c0 < n_chunks; c0 += nvb * U)
      sqsum_chunks_trip<U>(grad, wire, n_chunks, grad_scale, partial, vb0 + q < nvb ? c0 + q * U : n_chunks, tid, red[q]);
}
// norms[t] = sqrt(sum of the tensor's chunk partials); one 256-thread block per tensor, four loads in flight per thread,
// partial sums folded in a fixed order (deterministic).  (One wave per tensor walked the 50 k chunks of the embedding
// table one dependent load at a time: 145 us.)
__global__ __launch_bounds__(256) void tensor_norms_kernel(const float* __restrict__ partial,
                                                           const long* __restrict__ chunk_begin,
                                                           int n_tensors, float* __restrict__ norms,
                                                           int* __restrict__ skip) {
  __shared__ float red[4];
  const int t = blockIdx.x, lane = threadIdx.x & 63;
  const long c0 = chunk_begin[t], c1 = chunk_begin[t + 1];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  long c = c0 + threadIdx.x;
  for (; c + 768 < c1; c += 1024) {
    s0 += partial[c]; s1 += partial[c + 256]; s2 += partial[c + 512]; s3 += partial[c + 768];
  }
  for (; c < c1; c += 256) s0 += partial[c];
  float s = wave_sum((s0 + s1) + (s2 + s3));
  if (lane == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = (red[0] + red[1]) + (red[2] + red[3]);
    norms[t] = sqrtf(s);
    if (skip && !(fabsf(s) <= 3.4e38f)) atomicOr(skip, 2);      // NaN / Inf gradient (apex O2 skips such steps)
  }
}
// skip[0] = 1 if the loss is NaN / Inf (callback_apex_trainer.py:225-227 skips the batch), else 0
__global__ void loss_flag_kernel(const float* __restrict__ loss, int* __restrict__ skip) {
  skip[0] = (fabsf(loss[0]) <= 3.4e38f) ? 0 : 1;
}
extern "C" int tell_loss_flag(const float* loss, int* skip, hipStream_t stream) {
  hipLaunchKernelGGL(loss_flag_kernel, dim3(1), dim3(1), 0, stream, loss, skip);
  return tell_check_launch("loss_flag");
}
// warmup_linear (pytorch_pretrained_bert WarmupLinearSchedule.get_lr_) evaluated on the device from a device step counter
// that only SUCCESSFUL updates advance: a batch skipped for a non-finite loss / gradient never reached optimizer.step()
// in the reference (callback_apex_trainer.py:225-227), so it must not cost a tick of the schedule either - and the host
// cannot know about the skip without a synchronisation.  t_total <= 0: constant learning rate.
__global__ void lr_schedule_kernel(const int* __restrict__ step, float lr, float warmup, float t_total,
                                   float* __restrict__ lr_dev) {
  double f = 1.0;
  if (t_total > 0.f) {
    const double x = (double)step[0] / (double)t_total, w = (double)warmup;
    f = x < w ? x / w : fmax((x - 1.0) / (w - 1.0), 0.0);
  }
  lr_dev[0] = (float)((double)lr * f);
}
// Parameter groups: up to TELL_ADAM_MAX_GROUPS rows of (lr_base, warmup, t_total, b1, b2, eps, wd,
// max_norm), handed to the kernels BY VALUE - 512 B of kernel arguments, so a replayed graph needs nothing of the host's -
// and tensor_group[t], the row of tensor t.  A chunk belongs to one tensor, hence to one row: everything read from the
// table is uniform across the workgroup.
#define TELL_ADAM_MAX_GROUPS 16
enum { HP_LR = 0, HP_WARMUP, HP_T_TOTAL, HP_B1, HP_B2, HP_EPS, HP_WD, HP_MAX_NORM, HP_COLS };
struct GroupTable {
  float row[TELL_ADAM_MAX_GROUPS][HP_COLS];
};
struct GroupArgs {
  const int* tensor_group;
  int n_groups;
  GroupTable hp;
};
// lr_dev[g] = lr_schedule_kernel's value for row g from the one shared step counter: one thread per group
__global__ void lr_schedule_groups_kernel(const int* __restrict__ step, GroupTable hp, int n_groups,
                                          float* __restrict__ lr_dev) {
  const int g = threadIdx.x;
  if (g >= n_groups) return;
  const float lr = hp.row[g][HP_LR], warmup = hp.row[g][HP_WARMUP], t_total = hp.row[g][HP_T_TOTAL];
  double f = 1.0;
  if (t_total > 0.f) {
    const double x = (double)step[0] / (double)t_total, w = (double)warmup;
    f = x < w ? x / w : fmax((x - 1.0) / (w - 1.0), 0.0);
  }
  lr_dev[g] = (float)((double)lr * f);
}
// Exponential moving average of the masters: this step's 1 - d_t from the same count of APPLIED
// updates n = *step (read before the update kernel increments it), d_t = min(decay, (1 + n) / (warm + n)) - the average
// follows the weights closely while there are few of them.  warm <= 0 or no device counter: d_t = decay.  In double from
// the fp32 arguments, like the learning rate above.  A skipped step leaves *step alone, so this schedule does not tick.
__global__ void ema_schedule_kernel(const int* __restrict__ step, float decay, float warm, float* __restrict__ omd_dev) {
  double d = (double)decay;
  if (step && warm > 0.f) {
    const double n = (double)step[0];
    d = fmin(d, (1.0 + n) / ((double)warm + n));
  }
  omd_dev[0] = (float)(1.0 - d);
}
// One pass over the flat buffers: BertAdam update of the fp32 masters, the bf16 working copy the next forward
// reads (shadow; no per-tensor cast kernels), and the zeroing of the gradient for the next step.
// U: chunks per block iteration (all 4 U loads of a thread in flight before the first use); NT: the streams nobody reads
// again soon (master, m, v, the zeroed gradient) go out with non-temporal stores and come in with non-temporal loads -
// the bf16 shadow, which the next forward pass reads, keeps the default policy.
// EMA (an EmaArgs as the one trailing argument): the same pass also moves the moving average e of the masters towards the
// fresh master p' it holds in a register, e' = fma(omd, p' - e, e) with omd = *omd_dev = 1 - d_t (ema_schedule_kernel): one
// more fp32 stream in and out (8 of 42 B per parameter), loaded with the other loads of the iteration and non-temporal
// where the master is.  A skipped step leaves e alone.  The switch is the presence of that argument and not a third
// `bool EMA` in the template list: without it an instantiation keeps its name (bertadam_update_kernel<4, true> - tests and
// the recorded profiles look for it), its kernel arguments and, instruction for instruction, its code; an unused pointer
// pair at the end of the argument list, or the body inlined into two wrapper kernels, changed the register allocation
// of all five.
// Groups (a GroupArgs as the last trailing argument, after the EmaArgs when both are there): lr, b1, b2, eps, wd and max_norm
// of a chunk come from the row of its tensor - lr from lr_dev[row] - instead of the scalar arguments, which are then not
// read.  The index loads go out with the iteration's other loads; an index outside the table counts as row 0.
struct EmaArgs {
  float* ema;
  const float* omd_dev;
};
// Narrow form (common.h; a NarrowArgs as the FIRST trailing argument): 1024-thread workgroups, each 256-thread quarter takes
// the wide launch's blocks quarter, quarter + 4 * gridDim.x, ... of nvb in turn and does with each what that block did.
// There is no barrier in this kernel, so the quarters need not keep step.  Like the other two switches it is the presence
// of an argument: the wide instantiations keep their names and their code.
struct NarrowArgs {
  long nvb;
};
template <typename T>
__device__ __forceinline__ const T* trailing_arg() { return nullptr; }
template <typename T, typename A, typename... R>
__device__ __forceinline__ const T* trailing_arg(const A& a, const R&... rest) {
  if constexpr (std::is_same<T, A>::value) return &a;
  else return trailing_arg<T>(rest...);
}
template <typename T, typename... Ts>
constexpr int count_of = (0 + ... + (std::is_same<T, Ts>::value ? 1 : 0));
template <int U, bool NT, typename... Ext>
__global__ __launch_bounds__((count_of<NarrowArgs, Ext...> == 1 ? 1024 : 256)) void bertadam_update_kernel(float* __restrict__ param,
                                                              float* __restrict__ grad,
                                                              float* __restrict__ m, float* __restrict__ v,
                                                              const int* __restrict__ chunk_tensor,
                                                              const float* __restrict__ norms, long n_chunks,
                                                              const float* __restrict__ lr_dev, float b1,
                                                              float b2, float eps, float wd, float max_norm,
                                                              float grad_scale, uint16_t* __restrict__ shadow,
                                                              int zero_grad, int* __restrict__ skip,
                                                              const uint16_t* __restrict__ wire,
                                                              int* __restrict__ step_dev,
                                                              const int* __restrict__ keep_grad, Ext... ext) {
  constexpr bool EMA = count_of<EmaArgs, Ext...> == 1, GROUPS = count_of<GroupArgs, Ext...> == 1;
  constexpr bool NARROW = count_of<NarrowArgs, Ext...> == 1;
  static_assert(sizeof...(Ext) == (NARROW ? 1 : 0) + (EMA ? 1 : 0) + (GROUPS ? 1 : 0),
                "the optional trailing arguments are one NarrowArgs, one EmaArgs, one GroupArgs, or several in that order");
  // the block of the wide launch this thread works as, the thread's index in it, and the number of such blocks
  const int tid = NARROW ? threadIdx.x & 255 : threadIdx.x;
  long vb = NARROW ? (long)blockIdx.x * 4 + tell_quarter() : blockIdx.x, nvb = gridDim.x;
  if constexpr (NARROW) nvb = trailing_arg<NarrowArgs>(ext...)->nvb;
  typedef __attribute__((ext_vector_type(4))) float f4;
  struct Hp { float lr, b1, b2, eps, wd, max_norm; };
  Hp one = {0.f, b1, b2, eps, wd, max_norm};
  if constexpr (!GROUPS) one.lr = *lr_dev;
  float* ema = nullptr;
  float omd = 0.f;
  // (the EMA-only forms keep the spelling they had, and the lookup below is compiled only with groups: taking a reference to
  //  the EmaArgs in trailing_arg gave those five other register numbers and another schedule - DESIGN.md section 32)
  if constexpr (EMA && !GROUPS && !NARROW) {
    const EmaArgs ea[] = {ext...};
    ema = ea[0].ema;
    omd = *ea[0].omd_dev;
  } else if constexpr (EMA) {
    const EmaArgs* ea = trailing_arg<EmaArgs>(ext...);
    ema = ea->ema;
    omd = *ea->omd_dev;
  }
  const GroupArgs* ga = nullptr;
  if constexpr (GROUPS) ga = trailing_arg<GroupArgs>(ext...);
  // keep_grad[t] != 0: tensor t's gradient is rewritten whole (beta = 0 stores) by its single producer in the next
  // backward pass - not zeroed here (4 B / parameter less to write, and the producer does not read it back)
  if (skip && skip[0] != 0) {      // non-finite loss or gradient: leave p, m, v and the shadow alone, only clear the gradient
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(skip + 1, 1);          // running count of skipped steps
    if (zero_grad)
      for (long c = vb; c < n_chunks; c += NARROW ? (long)gridDim.x * 4 : nvb)
        if (!keep_grad || !keep_grad[chunk_tensor[c]])
          reinterpret_cast<float4*>(grad)[c * OPT_CHUNK / 4 + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  if (step_dev && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(step_dev, 1);   // (nobody reads it inside this launch)
  auto ldf = [](const float* base, long o) __attribute__((always_inline)) {
    const f4* q = reinterpret_cast<const f4*>(base) + o;
    return NT ? __builtin_nontemporal_load(q) : *q;
  };
  auto stf = [](float* base, long o, f4 val) __attribute__((always_inline)) {
    f4* q = reinterpret_cast<f4*>(base) + o;
    if (NT) __builtin_nontemporal_store(val, q); else *q = val;
  };
  if (NARROW && vb >= nvb) return;
  do      // (wide: once)
  for (long c0 = vb * U; c0 < n_chunks; c0 += nvb * U) {
    f4 g[U], p[U], mm[U], vv[U], e[EMA ? U : 1];
    float coef[U];
    int tensor[U], group[GROUPS ? U : 1];
    Hp hp[GROUPS ? U : 1];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long c = c0 + u < n_chunks ? c0 + u : n_chunks - 1;               // (clamped: the tail repeats the last chunk's loads)
      const long o = c * OPT_CHUNK / 4 + tid;
      if (wire) { const float4 w = load_grad4(grad, wire, o); g[u] = f4{w.x, w.y, w.z, w.w}; }
      else g[u] = ldf(grad, o);
      p[u] = ldf(param, o); mm[u] = ldf(m, o); vv[u] = ldf(v, o);
      if constexpr (EMA) e[u] = ldf(ema, o);
      tensor[u] = chunk_tensor[c];
      if constexpr (GROUPS) group[u] = ga->tensor_group[tensor[u]];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (GROUPS) {
        const int gi = (unsigned)group[u] < (unsigned)ga->n_groups ? group[u] : 0;
        const float* row = ga->hp.row[gi];
        hp[u] = Hp{lr_dev[gi], row[HP_B1], row[HP_B2], row[HP_EPS], row[HP_WD], row[HP_MAX_NORM]};
      }
      const float max_norm = GROUPS ? hp[GROUPS ? u : 0].max_norm : one.max_norm;
      coef[u] = grad_scale;
      if (max_norm > 0.f) {
        const float cc = max_norm / (norms[tensor[u]] + 1e-6f);
        if (cc < 1.f) coef[u] *= cc;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (c0 + u >= n_chunks) break;
      const long o = (c0 + u) * OPT_CHUNK / 4 + tid;
      const Hp h = GROUPS ? hp[GROUPS ? u : 0] : one;
      const float lr = h.lr, b1 = h.b1, b2 = h.b2, eps = h.eps, wd = h.wd;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // Every multiply-add spelled out, none left to the compiler's contraction: written as plain expressions the
        // U = 1 instantiation fused m and v differently from the U = 2 / 4 ones (1 ulp apart in m, v and p on a few
        // percent of the elements).  This is the arithmetic the U = 2 / 4 instantiations - the default - always had.
#pragma clang fp contract(off)
        const float gg = g[u][k] * coef[u];
        mm[u][k] = __builtin_fmaf(1.f - b1, gg, b1 * mm[u][k]);
        const float g2 = ((1.f - b2) * gg) * gg;
        vv[u][k] = b2 * vv[u][k] + g2;
        p[u][k] = __builtin_fmaf(-lr, __builtin_fmaf(wd, p[u][k], mm[u][k] / (sqrtf(vv[u][k]) + eps)), p[u][k]);
        if constexpr (EMA) {             // (the difference rounded once, the multiply-add rounded once)
          const float d = p[u][k] - e[u][k];
          e[u][k] = __builtin_fmaf(omd, d, e[u][k]);
        }
      }
      stf(param, o, p[u]); stf(m, o, mm[u]); stf(v, o, vv[u]);
      if constexpr (EMA) stf(ema, o, e[u]);
      if (shadow) {
        uint2 sw;
        sw.x = (uint32_t)f2bf(p[u][0]) | ((uint32_t)f2bf(p[u][1]) << 16);
        sw.y = (uint32_t)f2bf(p[u][2]) | ((uint32_t)f2bf(p[u][3]) << 16);
        reinterpret_cast<uint2*>(shadow)[o] = sw;
      }
      if (zero_grad && !(keep_grad && keep_grad[tensor[u]])) stf(grad, o, f4{0.f, 0.f, 0.f, 0.f});
    }
  }
  while (NARROW && (vb += (long)gridDim.x * 4) < nvb);
}

// One pass that exchanges the masters with their moving average and rewrites the bf16 working copy from what is now in
// `param` (Trainer.ema_weights: evaluation with the averaged weights - values move, no pointer that a captured graph
// holds changes).  Applied twice it restores all three buffers bit for bit.  One float4 of each stream per thread and
// trip; both fp32 streams non-temporal (the next reader of the weights reads the shadow).
__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ param, float* __restrict__ ema,
                                                       uint16_t* __restrict__ shadow, long n4) {
  typedef __attribute__((ext_vector_type(4))) float f4;
  for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < n4; o += (long)gridDim.x * 256) {
    f4* pp = reinterpret_cast<f4*>(param) + o;
    f4* pe = reinterpret_cast<f4*>(ema) + o;
    const f4 p = __builtin_nontemporal_load(pp), e = __builtin_nontemporal_load(pe);
    __builtin_nontemporal_store(e, pp);
    __builtin_nontemporal_store(p, pe);
    if (shadow) {
      uint2 sw;
      sw.x = (uint32_t)f2bf(e[0]) | ((uint32_t)f2bf(e[1]) << 16);
      sw.y = (uint32_t)f2bf(e[2]) | ((uint32_t)f2bf(e[3]) << 16);
      reinterpret_cast<uint2*>(shadow)[o] = sw;
    }
  }
}
extern "C" int tell_ema_swap(float* param, float* ema, void* shadow_bf16, long n, hipStream_t stream) {
  TELL_REQUIRE(param && ema, "ema_swap: param and ema must not be NULL");
  TELL_REQUIRE(((uintptr_t)param & 15) == 0 && ((uintptr_t)ema & 15) == 0, "ema_swap: buffers must be 16-byte aligned");
  TELL_REQUIRE(((uintptr_t)shadow_bf16 & 7) == 0, "ema_swap: the bf16 shadow must be 8-byte aligned");
  TELL_REQUIRE(n >= 0 && n % OPT_CHUNK == 0, "ema_swap: n must be a whole number of chunks");
  if (n == 0) return TELL_OK;
  const long chunks = n / OPT_CHUNK;
  hipLaunchKernelGGL(ema_swap_kernel, dim3((int)(chunks < 8192 ? chunks : 8192)), dim3(256), 0, stream, param, ema,
                     (uint16_t*)shadow_bf16, n / 4);
  return tell_check_launch("ema_swap");
}

extern "C" int tell_opt_chunk(void) { return OPT_CHUNK; }

// workspace `partial`: n_chunks floats; `norms`: n_tensors floats
// keep_grad: device int32[n_tensors] or NULL - tensors whose gradient the zeroing leaves alone (see the kernel)
// EMA: tell_bertadam_step_ema - the moving average `ema` and the device scalar `omd_dev` join the update launch
// groups (host, may be NULL): tell_bertadam_step_groups - the table replaces b1 .. max_norm and lr_base .. t_total
struct AdamFixed {        // the update kernel's arguments before the optional trailing ones, in its order
  float *param, *grad, *m, *v;
  const int* chunk_tensor;
  const float* norms;
  long n_chunks;
  const float* lr_dev;
  float b1, b2, eps, wd, max_norm, grad_scale;
  uint16_t* shadow;
  int zero_grad;
  int* skip;
  const uint16_t* wire;
  int* step_dev;
  const int* keep_grad;
};
// g blocks of 256 threads, or (option bw_wgs = G > 0) the same g blocks walked by at most G workgroups of 1024
template <int U, bool NT, typename... Ext>
static void adam_launch(long G, int g, hipStream_t stream, const AdamFixed& f, Ext... ext) {
  if (G > 0) {
    void (*kern)(float*, float*, float*, float*, const int*, const float*, long, const float*, float, float, float, float, float,
                 float, uint16_t*, int, int*, const uint16_t*, int*, const int*, NarrowArgs, Ext...) =
        bertadam_update_kernel<U, NT, NarrowArgs, Ext...>;
    tell_launch_narrow(kern, tell_narrow_wgs(G, g), 1024, stream, f.param, f.grad, f.m, f.v, f.chunk_tensor, f.norms, f.n_chunks,
                       f.lr_dev, f.b1, f.b2, f.eps, f.wd, f.max_norm, f.grad_scale, f.shadow, f.zero_grad, f.skip, f.wire,
                       f.step_dev, f.keep_grad, NarrowArgs{g}, ext...);
  } else
    hipLaunchKernelGGL((bertadam_update_kernel<U, NT, Ext...>), dim3(g), dim3(256), 0, stream, f.param, f.grad, f.m, f.v,
                       f.chunk_tensor, f.norms, f.n_chunks, f.lr_dev, f.b1, f.b2, f.eps, f.wd, f.max_norm, f.grad_scale,
                       f.shadow, f.zero_grad, f.skip, f.wire, f.step_dev, f.keep_grad, ext...);
}
template <bool EMA>
static int bertadam_launch(float* param, float* grad, float* m, float* v, const int* chunk_tensor, const long* chunk_begin,
                           long n_chunks, int n_tensors, float* partial, float* norms, const float* lr_dev, float b1, float b2,
                           float eps, float wd, float max_norm, float grad_scale, void* shadow_bf16, int zero_grad, int* skip,
                           const void* grad_wire_bf16, int* step_dev, float lr_base, float warmup, float t_total,
                           const int* keep_grad, float* ema, float* omd_dev, float ema_decay, float ema_warm,
                           const GroupArgs* groups, hipStream_t stream) {
  if (n_chunks <= 0) return TELL_OK;
  if (EMA) {
    TELL_REQUIRE(ema && omd_dev, "bertadam: ema and ema_omd_dev must not be NULL");
    TELL_REQUIRE(((uintptr_t)ema & 15) == 0, "bertadam: ema must be 16-byte aligned");
    TELL_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, "bertadam: ema_decay must be in [0, 1)");      // (false for NaN)
    TELL_REQUIRE(ema_warm >= 0.f && ema_warm <= 3.4e38f, "bertadam: ema_warm must be finite and not negative");
  }
  // (every refusal before the first launch: a refused call writes nothing, *lr_dev included)
  TELL_REQUIRE(((uintptr_t)grad_wire_bf16 & 7) == 0 && ((uintptr_t)shadow_bf16 & 7) == 0,
               "bertadam: the bf16 gradient and the bf16 shadow must be 8-byte aligned");
  const uint16_t* wire = static_cast<const uint16_t*>(grad_wire_bf16);
  TELL_REQUIRE(((uintptr_t)param & 15) == 0 && ((uintptr_t)grad & 15) == 0 && ((uintptr_t)m & 15) == 0 &&
                   ((uintptr_t)v & 15) == 0,
               "bertadam: buffers must be 16-byte aligned");
  // eps = 0: the zero padding between tensors (m = v = 0) would become 0 / 0 in the master and the shadow
  if (groups) {      // the norm pass runs iff any row clips; it then covers every tensor, and so does its non-finite flag
    max_norm = 0.f;
    for (int i = 0; i < groups->n_groups; ++i) {
      TELL_REQUIRE(groups->hp.row[i][HP_EPS] > 0.f, "bertadam: eps must be positive in every group");
      if (groups->hp.row[i][HP_MAX_NORM] > 0.f) max_norm = groups->hp.row[i][HP_MAX_NORM];
    }
  } else {
    TELL_REQUIRE(eps > 0.f, "bertadam: eps must be positive");
  }
  if (step_dev) {    // device-side schedule: this step's learning rate from the count of updates applied so far
    if (groups)
      hipLaunchKernelGGL(lr_schedule_groups_kernel, dim3(1), dim3(TELL_ADAM_MAX_GROUPS), 0, stream, step_dev, groups->hp,
                         groups->n_groups, const_cast<float*>(lr_dev));
    else
      hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(1), 0, stream, step_dev, lr_base, warmup, t_total,
                         const_cast<float*>(lr_dev));
  }
  if (EMA) hipLaunchKernelGGL(ema_schedule_kernel, dim3(1), dim3(1), 0, stream, step_dev, ema_decay, ema_warm, omd_dev);
  // TELL_ADAM_VAR (A/B aid, read once): 0 = one chunk per iteration, default cache policy (the round-4 kernel's shape);
  // 1 = U 2; 2 = U 4; 3 = U 2 + non-temporal; 4 = U 4 + non-temporal.  tools/probes/stream_probe.hip has the same shapes
  // on bare buffers.
  const int var = tell_opt(OPT_ADAM_VAR) >= 0 ? (int)tell_opt(OPT_ADAM_VAR) : TELL_ADAM_DEFAULT;
  const int grid_env = tell_opt(OPT_ADAM_GRID) > 0 ? (int)tell_opt(OPT_ADAM_GRID) : 4096;
  const int U = (var == 1 || var == 3) ? 2 : (var == 2 || var == 4) ? 4 : 1;
  const long iters = (n_chunks + U - 1) / U;
  int g = iters < grid_env ? (int)iters : grid_env;
  const long G = tell_opt(OPT_BW_WGS);
  if (max_norm > 0.f) {
    const long it4 = (n_chunks + 3) / 4;
    const int gs = it4 < 4096 ? (int)it4 : 4096;
    if (G > 0)
      tell_launch_narrow(sqsum_chunks_narrow_kernel<4>, tell_narrow_wgs(G, gs), 1024, stream, grad, wire, n_chunks, grad_scale,
                         partial, (long)gs);
    else
      hipLaunchKernelGGL((sqsum_chunks_kernel<4>), dim3(gs), dim3(256), 0, stream, grad, wire, n_chunks, grad_scale, partial);
    hipLaunchKernelGGL(tensor_norms_kernel, dim3(n_tensors), dim3(256), 0, stream, partial, chunk_begin, n_tensors, norms, skip);
  }
  const AdamFixed f = {param, grad, m, v, chunk_tensor, norms, n_chunks, lr_dev, b1, b2, eps, wd, max_norm, grad_scale,
                       (uint16_t*)shadow_bf16, zero_grad, skip, wire, step_dev, keep_grad};
  // (with groups the scalar hyperparameters are not read: b1 .. max_norm arrive as 0 from tell_bertadam_step_groups, and
  //  max_norm, which the loop above set for the norm pass, goes to the kernel as 0 like them)
#define TELL_ADAM_LAUNCH(UU, NTT)                                                                          \
  do {                                                                                                     \
    AdamFixed fg = f;                                                                                      \
    fg.max_norm = 0.f;                                                                                     \
    if (EMA && groups) adam_launch<UU, NTT>(G, g, stream, fg, EmaArgs{ema, omd_dev}, *groups);             \
    else if (groups) adam_launch<UU, NTT>(G, g, stream, fg, *groups);                                      \
    else if (EMA) adam_launch<UU, NTT>(G, g, stream, f, EmaArgs{ema, omd_dev});                            \
    else adam_launch<UU, NTT>(G, g, stream, f);                                                            \
  } while (0)
  switch (var) {
    case 1: TELL_ADAM_LAUNCH(2, false); break;
    case 2: TELL_ADAM_LAUNCH(4, false); break;
    case 3: TELL_ADAM_LAUNCH(2, true); break;
    case 4: TELL_ADAM_LAUNCH(4, true); break;
    default: TELL_ADAM_LAUNCH(1, false); break;
  }
#undef TELL_ADAM_LAUNCH
  return tell_check_launch("bertadam_step");
}
extern "C" int tell_bertadam_step2(float* param, float* grad, float* m, float* v,
                                   const int* chunk_tensor, const long* chunk_begin, long n_chunks,
                                   int n_tensors, float* partial, float* norms, const float* lr_dev,
                                   float b1, float b2, float eps, float wd, float max_norm,
                                   float grad_scale, void* shadow_bf16, int zero_grad, int* skip,
                                   const void* grad_wire_bf16, int* step_dev, float lr_base, float warmup, float t_total,
                                   const int* keep_grad, hipStream_t stream) {
  return bertadam_launch<false>(param, grad, m, v, chunk_tensor, chunk_begin, n_chunks, n_tensors, partial, norms, lr_dev, b1,
                                b2, eps, wd, max_norm, grad_scale, shadow_bf16, zero_grad, skip, grad_wire_bf16, step_dev,
                                lr_base, warmup, t_total, keep_grad, nullptr, nullptr, 0.f, 0.f, nullptr, stream);
}
extern "C" int tell_bertadam_step_ema(float* param, float* grad, float* m, float* v,
                                      const int* chunk_tensor, const long* chunk_begin, long n_chunks,
                                      int n_tensors, float* partial, float* norms, const float* lr_dev,
                                      float b1, float b2, float eps, float wd, float max_norm,
                                      float grad_scale, void* shadow_bf16, int zero_grad, int* skip,
                                      const void* grad_wire_bf16, int* step_dev, float lr_base, float warmup, float t_total,
                                      const int* keep_grad, float* ema, float* ema_omd_dev, float ema_decay, float ema_warm,
                                      hipStream_t stream) {
  return bertadam_launch<true>(param, grad, m, v, chunk_tensor, chunk_begin, n_chunks, n_tensors, partial, norms, lr_dev, b1,
                               b2, eps, wd, max_norm, grad_scale, shadow_bf16, zero_grad, skip, grad_wire_bf16, step_dev,
                               lr_base, warmup, t_total, keep_grad, ema, ema_omd_dev, ema_decay, ema_warm, nullptr, stream);
}
extern "C" int tell_bertadam_step_groups(float* param, float* grad, float* m, float* v, const int* chunk_tensor,
                                         const long* chunk_begin, long n_chunks, int n_tensors, float* partial, float* norms,
                                         float* lr_dev, const int* tensor_group, const float* group_hp, int n_groups,
                                         float grad_scale, void* shadow_bf16, int zero_grad, int* skip,
                                         const void* grad_wire_bf16, int* step_dev, const int* keep_grad, float* ema,
                                         float* ema_omd_dev, float ema_decay, float ema_warm, hipStream_t stream) {
  if (n_chunks <= 0) return TELL_OK;
  TELL_REQUIRE(n_groups >= 1 && n_groups <= TELL_ADAM_MAX_GROUPS, "bertadam: n_groups must be in 1..16");
  TELL_REQUIRE(tensor_group && group_hp && lr_dev, "bertadam: tensor_group, group_hp and lr_dev must not be NULL");
  TELL_REQUIRE((ema == nullptr) == (ema_omd_dev == nullptr), "bertadam: ema and ema_omd_dev must be given together");
  GroupArgs ga = {};          // (rows past n_groups stay 0: the kernels never index them)
  ga.tensor_group = tensor_group;
  ga.n_groups = n_groups;
  for (int i = 0; i < n_groups * HP_COLS; ++i) ga.hp.row[i / HP_COLS][i % HP_COLS] = group_hp[i];
  if (ema)
    return bertadam_launch<true>(param, grad, m, v, chunk_tensor, chunk_begin, n_chunks, n_tensors, partial, norms, lr_dev,
                                 0.f, 0.f, 0.f, 0.f, 0.f, grad_scale, shadow_bf16, zero_grad, skip, grad_wire_bf16, step_dev,
                                 0.f, 0.f, 0.f, keep_grad, ema, ema_omd_dev, ema_decay, ema_warm, &ga, stream);
  return bertadam_launch<false>(param, grad, m, v, chunk_tensor, chunk_begin, n_chunks, n_tensors, partial, norms, lr_dev, 0.f,
                                0.f, 0.f, 0.f, 0.f, grad_scale, shadow_bf16, zero_grad, skip, grad_wire_bf16, step_dev, 0.f,
                                0.f, 0.f, keep_grad, nullptr, nullptr, 0.f, 0.f, &ga, stream);
}
extern "C" int tell_bertadam_step(float* param, float* grad, float* m, float* v,
                                  const int* chunk_tensor, const long* chunk_begin, long n_chunks,
                                  int n_tensors, float* partial, float* norms, const float* lr_dev,
                                  float b1, float b2, float eps, float wd, float max_norm,
                                  float grad_scale, void* shadow_bf16, int zero_grad, int* skip,
                                  const void* grad_wire_bf16, int* step_dev, float lr_base, float warmup, float t_total,
                                  hipStream_t stream) {
  return tell_bertadam_step2(param, grad, m, v, chunk_tensor, chunk_begin, n_chunks, n_tensors, partial, norms, lr_dev, b1, b2,
                             eps, wd, max_norm, grad_scale, shadow_bf16, zero_grad, skip, grad_wire_bf16, step_dev, lr_base,
                             warmup, t_total, nullptr, stream);
}

// fill n floats with a value (grad zeroing without a memset node per tensor)
__global__ void fill_kernel(float* __restrict__ x, long n, float value) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) x[i] = value;
}
extern "C" int tell_fill_f32(float* x, long n, float value, hipStream_t stream) {
  if (n <= 0) return TELL_OK;
  long g = (n + 1023) / 1024;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(fill_kernel, dim3((int)g), dim3(256), 0, stream, x, n, value);
  return tell_check_launch("fill_f32");
}
