// Copy-mechanism kernels of transformer_pointer / transformer_pointer_2 (include/tell_hip.h "copy mechanism").
//
//  * copy attention: the 16-head score-only attention of the decoder output over the article
//    (tell/modules/attention/multi_head.py:14-204 multi_head_attention_score_forward): bias_k and a zero key are
//    virtual columns S, S+1, key padding masks to -inf, fp32 softmax per head, dropout on the per-head weights, head
//    mean; the virtual columns are dropped and proper_mask < 1 columns zeroed.  Backward recomputes the per-head
//    probabilities from q, k and the saved log-sum-exp (there is no PV product).
//  * the fused copy loss: per batch row the context ids are deduplicated in LDS (duplicates summed in increasing
//    position order, as scatter_add_ does), p_target and Z = sum_{p>0} p + (V - n_pos) per entity row, per-entity-index
//    means reduced on the device; the backward writes dW directly.  No [B, T, V] tensor exists.
//  * the entity head: entity_fc (2 outputs) + cross entropy with ignore_index -1 against min(copy_mask, 1).
//  * causal entity attention: row t attends to keys s < t plus a zero slot (logit 0, value 0), i.e.
//    downsampled_single_head.py _mask_future_full + scalar_bias.py; one-query step form through pos0.
//  * the generation copy decision: one launch per step over the alive rows.
//
// All kernels are plain FMA code (no MFMA): the copy head is small next to the decoder it sits on.  Every launcher is
// asynchronous: no host synchronisation, no allocation.
#include "common.h"

namespace {

constexpr int NT = 256;           // threads per workgroup of the row kernels
constexpr int NW = NT / 64;
constexpr int MAX_S = 512;        // article positions a row kernel keeps in LDS
constexpr int RT = 4;             // query rows per copy-attention workgroup (K rows are read once per RT queries)

template <typename T> __device__ __forceinline__ float ld(const T* p) { return Elem<T>::ld(p); }
template <typename T> __device__ __forceinline__ void st(T* p, float v) { Elem<T>::st(p, v); }

// block-wide reductions over NT threads; `red` holds NW floats; every thread gets the result
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < NW; ++i) r = fmaxf(r, red[i]);
  return r;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < NW; ++i) r += red[i];
  return r;
}

// ------------------------------------------------------------------ copy attention, shared pieces
struct CopyAttnArgs {
  const void* q; const void* k; const void* bias_k; const uint8_t* mask; const int8_t* proper;
  int B, H, T, S, D; long q_st, q_sb, k_ss, k_sb;
  float p; uint32_t seed, salt; const uint32_t* step;
};

// logits of query rows t0 .. t0+RT-1, head h, into lg[r][0 .. S+1] (S, S+1: bias_k, zero key); masked keys -inf.
// qs[r][d] holds the (scaled) query rows of head h.
template <typename T>
__device__ void copy_logits(const CopyAttnArgs& a, int b, int h, int t0, const float (*qs)[64], float (*lg)[MAX_S + 2]) {
  const int S = a.S, D = a.D;
  for (int s = threadIdx.x; s < S + 2; s += NT) {
    float dot[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) dot[r] = 0.f;
    const bool masked = s < S && a.mask && a.mask[(long)b * S + s];
    if (s < S + 1 && !masked) {
      const T* kp = s < S ? static_cast<const T*>(a.k) + s * a.k_ss + b * a.k_sb + (long)h * D
                          : static_cast<const T*>(a.bias_k) + (long)h * D;
      for (int d = 0; d < D; ++d) {
        const float kv = ld(kp + d);
#pragma unroll
        for (int r = 0; r < RT; ++r) dot[r] += qs[r][d] * kv;
      }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) lg[r][s] = masked ? -INFINITY : dot[r];
  }
}

template <typename T>
__device__ void load_q_rows(const CopyAttnArgs& a, int b, int h, int t0, float (*qs)[64]) {
  for (int i = threadIdx.x; i < RT * 64; i += NT) {
    const int r = i / 64, d = i % 64, t = t0 + r;
    qs[r][d] = (t < a.T && d < a.D) ? ld(static_cast<const T*>(a.q) + t * a.q_st + b * a.q_sb + (long)h * a.D + d) : 0.f;
  }
}

// ------------------------------------------------------------------ copy attention forward
// grid (ceil(T / RT), B).  w [B, T, S] fp32 (head mean, proper-masked), lse [B, H, T].
template <typename T>
__global__ __launch_bounds__(NT) void copy_attn_fwd_kernel(CopyAttnArgs a, float* __restrict__ w, float* __restrict__ lse) {
  __shared__ float qs[RT][64];
  __shared__ float lg[RT][MAX_S + 2];
  __shared__ float red[NW];
  const int b = blockIdx.y, t0 = blockIdx.x * RT, S = a.S, H = a.H, S2 = S + 2;
  const uint32_t thr = tell_drop_threshold(a.p);
  const float inv_keep = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  const uint32_t salt = tell_step_salt(a.salt, a.step);
  float acc[RT][MAX_S / NT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int j = 0; j < MAX_S / NT; ++j) acc[r][j] = 0.f;
  for (int h = 0; h < H; ++h) {
    __syncthreads();
    load_q_rows<T>(a, b, h, t0, qs);
    __syncthreads();
    copy_logits<T>(a, b, h, t0, qs, lg);
    __syncthreads();
    for (int r = 0; r < RT; ++r) {
      const int t = t0 + r;
      if (t >= a.T) break;
      float m = -INFINITY;
      for (int s = threadIdx.x; s < S2; s += NT) m = fmaxf(m, lg[r][s]);
      m = block_max(m, red);                       // >= 0: the zero key is never masked
      float l = 0.f;
      for (int s = threadIdx.x; s < S2; s += NT) l += __expf(lg[r][s] - m);
      l = block_sum(l, red);
      const float lz = m + __logf(l);
      if (threadIdx.x == 0) lse[((long)b * H + h) * a.T + t] = lz;
      const uint64_t base = (((uint64_t)b * H + h) * a.T + t) * (uint64_t)S2;
#pragma unroll
      for (int j = 0; j < MAX_S / NT; ++j) {
        const int s = threadIdx.x + j * NT;
        if (s < S) {
          float pr = __expf(lg[r][s] - lz);
          if (thr) pr *= tell_keep(a.seed, salt, base + s, thr, inv_keep);
          acc[r][j] += pr;
        }
      }
    }
  }
  const float inv_h = 1.f / H;
  for (int r = 0; r < RT; ++r) {
    const int t = t0 + r;
    if (t >= a.T) break;
#pragma unroll
    for (int j = 0; j < MAX_S / NT; ++j) {
      const int s = threadIdx.x + j * NT;
      if (s < S) {
        const bool keep = !a.proper || a.proper[(long)b * S + s] >= 1;
        w[((long)b * a.T + t) * S + s] = keep ? acc[r][j] * inv_h : 0.f;
      }
    }
  }
}

// ------------------------------------------------------------------ copy attention backward, query side
// grid (ceil(T / RT), B).  dlogit[s] = P[s] (dP[s] - delta), dP[s] = keep[s] dW[s] / H for s < S (0 on the virtual
// columns); dq = sum_s dlogit[s] k[s] + dlogit[S] bias_k; delta [B, H, T] is kept for the key side;
// dbk_rows [B * T, E] fp32 gets dlogit[S] q (the caller sums the rows).
template <typename T>
__global__ __launch_bounds__(NT) void copy_attn_bwd_q_kernel(CopyAttnArgs a, const float* __restrict__ lse,
                                                             const float* __restrict__ dw, void* __restrict__ dq,
                                                             float* __restrict__ delta, float* __restrict__ dbk_rows) {
  __shared__ float qs[RT][64];
  __shared__ float lg[RT][MAX_S + 2];
  __shared__ float part[NW][64];
  __shared__ float red[NW];
  const int b = blockIdx.y, t0 = blockIdx.x * RT, S = a.S, H = a.H, S2 = S + 2, D = a.D;
  const uint32_t thr = tell_drop_threshold(a.p);
  const float inv_keep = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  const uint32_t salt = tell_step_salt(a.salt, a.step);
  const float inv_h = 1.f / H;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int h = 0; h < H; ++h) {
    __syncthreads();
    load_q_rows<T>(a, b, h, t0, qs);
    __syncthreads();
    copy_logits<T>(a, b, h, t0, qs, lg);
    __syncthreads();
    for (int r = 0; r < RT; ++r) {
      const int t = t0 + r;
      if (t >= a.T) break;
      const float lz = lse[((long)b * H + h) * a.T + t];
      const uint64_t base = (((uint64_t)b * H + h) * a.T + t) * (uint64_t)S2;
      float dsum = 0.f;
      for (int s = threadIdx.x; s < S2; s += NT) {
        const float pr = __expf(lg[r][s] - lz);
        float dp = 0.f;
        if (s < S && (!a.proper || a.proper[(long)b * S + s] >= 1)) {
          dp = dw[((long)b * a.T + t) * S + s] * inv_h;
          if (thr) dp *= tell_keep(a.seed, salt, base + s, thr, inv_keep);
        }
        lg[r][s] = pr;                         // probability; dP kept beside it below
        dsum += pr * dp;
      }
      const float dl_delta = block_sum(dsum, red);
      if (threadIdx.x == 0) delta[((long)b * H + h) * a.T + t] = dl_delta;
      // dlogit in place of the probabilities
      for (int s = threadIdx.x; s < S2; s += NT) {
        float dp = 0.f;
        if (s < S && (!a.proper || a.proper[(long)b * S + s] >= 1)) {
          dp = dw[((long)b * a.T + t) * S + s] * inv_h;
          if (thr) dp *= tell_keep(a.seed, salt, base + s, thr, inv_keep);
        }
        lg[r][s] = lg[r][s] * (dp - dl_delta);
      }
      __syncthreads();
      // dq[d] = sum_s dlogit[s] k[s][d]: wave wv takes s = wv, wv + NW, ...; lane d
      float accd = 0.f;
      if (lane < D) {
        for (int s = wv; s < S; s += NW) {
          const float g = lg[r][s];
          if (g != 0.f) accd += g * ld(static_cast<const T*>(a.k) + s * a.k_ss + b * a.k_sb + (long)h * D + lane);
        }
        if (wv == 0 && a.bias_k) accd += lg[r][S] * ld(static_cast<const T*>(a.bias_k) + (long)h * D + lane);
      }
      part[wv][lane] = accd;
      __syncthreads();
      if (wv == 0 && lane < D) {
        float sum = 0.f;
        for (int i = 0; i < NW; ++i) sum += part[i][lane];
        st(static_cast<T*>(dq) + t * a.q_st + b * a.q_sb + (long)h * D + lane, sum);
        if (dbk_rows) dbk_rows[((long)b * a.T + t) * (H * D) + (long)h * D + lane] = lg[r][S] * qs[r][lane];
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------ copy attention backward, key side
// grid (ceil(S / NW), B): wave wv owns key s = blockIdx.x * NW + wv, lane d; loops heads and query rows.
template <typename T>
__global__ __launch_bounds__(NT) void copy_attn_bwd_k_kernel(CopyAttnArgs a, const float* __restrict__ lse,
                                                             const float* __restrict__ dw,
                                                             const float* __restrict__ delta, void* __restrict__ dk) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, s = blockIdx.x * NW + (threadIdx.x >> 6);
  if (s >= a.S) return;                                  // whole waves leave: no block barrier below
  const int S = a.S, H = a.H, S2 = S + 2, D = a.D;
  T* dkp = static_cast<T*>(dk) + s * a.k_ss + b * a.k_sb;
  const bool masked = a.mask && a.mask[(long)b * S + s];
  const bool prop = !a.proper || a.proper[(long)b * S + s] >= 1;
  const uint32_t thr = tell_drop_threshold(a.p);
  const float inv_keep = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  const uint32_t salt = tell_step_salt(a.salt, a.step);
  const float inv_h = 1.f / H;
  for (int h = 0; h < H; ++h) {
    float acc = 0.f;
    const float kd = lane < D ? ld(static_cast<const T*>(a.k) + s * a.k_ss + b * a.k_sb + (long)h * D + lane) : 0.f;
    if (!masked) {
      for (int t = 0; t < a.T; ++t) {
        const float qd = lane < D ? ld(static_cast<const T*>(a.q) + t * a.q_st + b * a.q_sb + (long)h * D + lane) : 0.f;
        const float dot = wave_sum(qd * kd);
        const long row = ((long)b * H + h) * a.T + t;
        const float pr = __expf(dot - lse[row]);
        float dp = 0.f;
        if (prop) {
          dp = dw[((long)b * a.T + t) * S + s] * inv_h;
          if (thr) dp *= tell_keep(a.seed, salt, (uint64_t)row * S2 + s, thr, inv_keep);
        }
        acc += pr * (dp - delta[row]) * qd;
      }
    }
    if (lane < D) st(dkp + (long)h * D + lane, acc);
  }
}

// ------------------------------------------------------------------ fused copy loss
// Per batch row b: LDS copy of the context ids, nxt[s] = the next position holding the same id (-1 at the end of a
// chain), head[s] = 1 at the first occurrence.  The thread of a chain head sums the weights along the chain in
// increasing position order.
__device__ void dedupe_row(const long* __restrict__ ids, int S, int* sid, int* nxt, uint8_t* head) {
  for (int s = threadIdx.x; s < S; s += NT) sid[s] = (int)ids[s];
  __syncthreads();
  for (int s = threadIdx.x; s < S; s += NT) {
    const int v = sid[s];
    int n = -1;
    for (int j = s + 1; j < S; ++j)
      if (sid[j] == v) { n = j; break; }
    nxt[s] = n;
    bool first = true;
    for (int j = 0; j < s; ++j)
      if (sid[j] == v) { first = false; break; }
    head[s] = first;
  }
  __syncthreads();
}

// grid B.  term [B, T]: the row's loss term (entity rows), p_t [B, T], z [B, T] (variant 2).
__global__ __launch_bounds__(NT) void copy_loss_rows_kernel(const float* __restrict__ w, const long* __restrict__ ctx,
                                                            const long* __restrict__ tgt, long tgt_sb,
                                                            const long* __restrict__ cmask, long cm_sb,
                                                            const int* __restrict__ vcount, int variant, int T, int S,
                                                            float* __restrict__ term, float* __restrict__ pt,
                                                            float* __restrict__ zz) {
  __shared__ int sid[MAX_S];
  __shared__ int nxt[MAX_S];
  __shared__ uint8_t head[MAX_S];
  __shared__ float ws[MAX_S];
  __shared__ float red[NW];
  __shared__ float ptarget;
  const int b = blockIdx.x;
  dedupe_row(ctx + (long)b * S, S, sid, nxt, head);
  const float V = vcount ? (float)*vcount : 0.f;
  for (int t = 0; t < T; ++t) {
    const long cm = cmask[(long)b * cm_sb + t];
    const long o = (long)b * T + t;
    if (cm < 1) {
      if (threadIdx.x == 0) { term[o] = 0.f; pt[o] = 0.f; zz[o] = 0.f; }
      continue;
    }
    const int target = (int)tgt[(long)b * tgt_sb + t];
    for (int s = threadIdx.x; s < S; s += NT) ws[s] = w[o * S + s];
    if (threadIdx.x == 0) ptarget = 0.f;
    __syncthreads();
    float npos = 0.f, zsum = 0.f;
    for (int s = threadIdx.x; s < S; s += NT) {
      if (!head[s]) continue;
      float p = 0.f;
      for (int j = s; j >= 0; j = nxt[j]) p += ws[j];
      if (sid[s] == target) ptarget = p;
      if (p > 0.f) { npos += 1.f; zsum += p; }
    }
    npos = block_sum(npos, red);
    zsum = block_sum(zsum, red);                 // (its barriers also publish ptarget)
    if (threadIdx.x == 0) {
      const float p = ptarget;
      const float lp = p > 0.f ? logf(p) : 0.f;
      const float z = zsum + (V - npos);
      // V < 0: an id outside the vocabulary (the reference's index_copy_ fails there) - the loss becomes NaN
      term[o] = variant == 2 ? (V < 0.f ? NAN : -lp + logf(z)) : -lp;
      pt[o] = p;
      zz[o] = z;
    }
    __syncthreads();
  }
}

// one workgroup: loss = sum_{i = 1 .. max index} mean over rows with copy_mask == i of term (an index without rows
// gives the mean of nothing, NaN, as the reference's loop does); scale[r] = 1 / count of the row's index.
__global__ __launch_bounds__(NT) void copy_loss_reduce_kernel(const float* __restrict__ term,
                                                              const long* __restrict__ cmask, long cm_sb, int B, int T,
                                                              float* __restrict__ loss, float* __restrict__ scale) {
  __shared__ float red[NW];
  const int N = B * T;
  float mx = 0.f;
  for (int r = threadIdx.x; r < N; r += NT) mx = fmaxf(mx, (float)cmask[(long)(r / T) * cm_sb + r % T]);
  const long maxidx = (long)block_max(mx, red);
  float total = 0.f;
  for (long i = 1; i <= maxidx; ++i) {
    float s = 0.f, c = 0.f;
    for (int r = threadIdx.x; r < N; r += NT)
      if (cmask[(long)(r / T) * cm_sb + r % T] == i) { s += term[r]; c += 1.f; }
    s = block_sum(s, red);
    c = block_sum(c, red);
    total += s / c;
    for (int r = threadIdx.x; r < N; r += NT)
      if (cmask[(long)(r / T) * cm_sb + r % T] == i) scale[r] = 1.f / c;
  }
  for (int r = threadIdx.x; r < N; r += NT)
    if (cmask[(long)(r / T) * cm_sb + r % T] < 1) scale[r] = 0.f;
  if (threadIdx.x == 0) *loss = total;
}

// grid (T, B): dW of one row.  variant 1: -g / p_t on the target's positions (p_t > 0);
// variant 2: g (1 / Z on positions whose id has p > 0, - 1 / p_t on the target's positions).
__global__ __launch_bounds__(NT) void copy_loss_bwd_kernel(const float* __restrict__ dloss, const float* __restrict__ w,
                                                           const long* __restrict__ ctx, const long* __restrict__ tgt,
                                                           long tgt_sb, const long* __restrict__ cmask, long cm_sb,
                                                           const float* __restrict__ pt, const float* __restrict__ zz,
                                                           const float* __restrict__ scale, int variant, int T, int S,
                                                           float* __restrict__ dw) {
  __shared__ int sid[MAX_S];
  __shared__ float ws[MAX_S];
  const int t = blockIdx.x, b = blockIdx.y;
  const long o = (long)b * T + t;
  float* out = dw + o * S;
  const long cm = cmask[(long)b * cm_sb + t];
  if (cm < 1) {
    for (int s = threadIdx.x; s < S; s += NT) out[s] = 0.f;
    return;
  }
  const float g = *dloss * scale[o];
  const int target = (int)tgt[(long)b * tgt_sb + t];
  const float p = pt[o];
  const float gt = p > 0.f ? -g / p : 0.f;
  if (variant != 2) {
    for (int s = threadIdx.x; s < S; s += NT) out[s] = (int)ctx[(long)b * S + s] == target ? gt : 0.f;
    return;
  }
  for (int s = threadIdx.x; s < S; s += NT) {
    sid[s] = (int)ctx[(long)b * S + s];
    ws[s] = w[o * S + s];
  }
  __syncthreads();
  const float gz = g / zz[o];
  for (int s = threadIdx.x; s < S; s += NT) {
    const int v = sid[s];
    bool pos = false;
    for (int j = 0; j < S && !pos; ++j) pos = sid[j] == v && ws[j] > 0.f;
    out[s] = (pos ? gz : 0.f) + (v == target ? gt : 0.f);
  }
}

// vocabulary bitmap of cat(context_ids, targets) -> the number of distinct ids V (variant 2's reduced vocabulary)
__global__ void vocab_mark_kernel(const long* __restrict__ ctx, long n_ctx, const long* __restrict__ tgt, int B, int T,
                                  long tgt_sb, int vocab, uint32_t* __restrict__ bits) {
  const long n = n_ctx + (long)B * T;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long v = i < n_ctx ? ctx[i] : tgt[((i - n_ctx) / T) * tgt_sb + (i - n_ctx) % T];
    if (v >= 0 && v < vocab) atomicOr(&bits[v >> 5], 1u << (v & 31));
    else atomicOr(&bits[(vocab + 31) / 32], 1u);              // the flag word after the bitmap: an id out of range
  }
}
__global__ __launch_bounds__(NT) void vocab_count_kernel(const uint32_t* __restrict__ bits, int words, int* __restrict__ count) {
  __shared__ float red[NW];
  float c = 0.f;
  for (int i = threadIdx.x; i < words; i += NT) c += (float)__popc(bits[i]);
  c = block_sum(c, red);
  if (threadIdx.x == 0) *count = bits[words] ? -1 : (int)c;
}

// ------------------------------------------------------------------ entity head: entity_fc + cross entropy
// grid N = T * B rows (x row of (t, b) at t * x_st + b * x_sb), one wave each.  logits [B, T, 2] fp32.
template <typename T>
__global__ __launch_bounds__(64) void entity_logits_kernel(const T* __restrict__ x, long x_st, long x_sb,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           int B, int Tn, int E, float* __restrict__ logits) {
  const int r = blockIdx.x, t = r / B, b = r % B, lane = threadIdx.x;
  const T* xp = x + t * x_st + b * x_sb;
  float a0 = 0.f, a1 = 0.f;
  for (int e = lane; e < E; e += 64) {
    const float xv = ld(xp + e);
    a0 += xv * w[e];
    a1 += xv * w[E + e];
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  if (lane == 0) {
    logits[((long)b * Tn + t) * 2] = a0 + (bias ? bias[0] : 0.f);
    logits[((long)b * Tn + t) * 2 + 1] = a1 + (bias ? bias[1] : 0.f);
  }
}
// one workgroup: mean cross entropy over rows with copy_mask != -1, target min(copy_mask, 1); *nvalid for backward
__global__ __launch_bounds__(NT) void entity_ce_kernel(const float* __restrict__ logits, const long* __restrict__ cmask,
                                                       long cm_sb, int B, int Tn, float* __restrict__ loss,
                                                       float* __restrict__ nvalid) {
  __shared__ float red[NW];
  float s = 0.f, c = 0.f;
  for (int r = threadIdx.x; r < B * Tn; r += NT) {
    const long cm = cmask[(long)(r / Tn) * cm_sb + r % Tn];
    if (cm == -1) continue;
    const float l0 = logits[2 * r], l1 = logits[2 * r + 1];
    const float m = fmaxf(l0, l1);
    const float lz = m + logf(expf(l0 - m) + expf(l1 - m));
    s += lz - (cm >= 1 ? l1 : l0);
    c += 1.f;
  }
  s = block_sum(s, red);
  c = block_sum(c, red);
  if (threadIdx.x == 0) { *loss = s / c; *nvalid = c; }
}
// grid N rows, one wave each: dlogit = g / n (softmax - onehot); dx = dlogit W
template <typename T>
__global__ __launch_bounds__(64) void entity_dx_kernel(const float* __restrict__ dloss, const float* __restrict__ nvalid,
                                                       const float* __restrict__ logits, const long* __restrict__ cmask,
                                                       long cm_sb, const float* __restrict__ w, int B, int Tn, int E,
                                                       T* __restrict__ dx, long dx_st, long dx_sb,
                                                       float* __restrict__ dlogits) {
  const int r = blockIdx.x, t = r / B, b = r % B, lane = threadIdx.x;
  const long o = (long)b * Tn + t;
  const long cm = cmask[(long)b * cm_sb + t];
  float d0 = 0.f, d1 = 0.f;
  if (cm != -1) {
    const float l0 = logits[2 * o], l1 = logits[2 * o + 1];
    const float m = fmaxf(l0, l1);
    const float e0 = expf(l0 - m), e1 = expf(l1 - m), inv = 1.f / (e0 + e1);
    const float g = *dloss / *nvalid;
    d0 = g * (e0 * inv - (cm >= 1 ? 0.f : 1.f));
    d1 = g * (e1 * inv - (cm >= 1 ? 1.f : 0.f));
  }
  if (lane == 0) { dlogits[2 * o] = d0; dlogits[2 * o + 1] = d1; }
  T* dp = dx + t * dx_st + b * dx_sb;
  for (int e = lane; e < E; e += 64) st(dp + e, d0 * w[e] + d1 * w[E + e]);
}
// grid ceil(E / 64): dW[c][e] = sum_r dlogit[r][c] x[r][e] (fp32 [2, E], assigned), db[c] += sum_r dlogit[r][c]
template <typename T>
__global__ __launch_bounds__(NT) void entity_dw_kernel(const float* __restrict__ dlogits, const T* __restrict__ x,
                                                       long x_st, long x_sb, int B, int Tn, int E,
                                                       float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float part[NW][2][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, e = blockIdx.x * 64 + lane;
  float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
  for (int r = g; r < B * Tn; r += NW) {
    const int t = r / B, b = r % B;
    const long o = (long)b * Tn + t;
    const float d0 = dlogits[2 * o], d1 = dlogits[2 * o + 1];
    b0 += d0;
    b1 += d1;
    if (e < E) {
      const float xv = ld(x + t * x_st + b * x_sb + e);
      a0 += d0 * xv;
      a1 += d1 * xv;
    }
  }
  part[g][0][lane] = a0;
  part[g][1][lane] = a1;
  __syncthreads();
  if (g == 0 && e < E) {
    float s0 = 0.f, s1 = 0.f;
    for (int i = 0; i < NW; ++i) { s0 += part[i][0][lane]; s1 += part[i][1][lane]; }
    dw[e] = s0;
    dw[E + e] = s1;
  }
  __syncthreads();
  if (blockIdx.x == 0 && db) {
    part[g][0][lane] = lane == 0 ? b0 : 0.f;
    part[g][1][lane] = lane == 0 ? b1 : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
      float s0 = 0.f, s1 = 0.f;
      for (int i = 0; i < NW; ++i) { s0 += part[i][0][0]; s1 += part[i][1][0]; }
      db[0] += s0;
      db[1] += s1;
    }
  }
}

// ------------------------------------------------------------------ causal entity attention
// One wave per (query row, b, h), lane d (D = 64).  Query i sits at position pos0 + i and sees keys s < pos0 + i,
// plus the zero slot (logit 0, value 0) as the first term of the online softmax.
struct CausalArgs {
  const void* q; const void* k; const void* v; void* out; float* lse;
  int B, H, Tq, S, D, pos0; long q_st, q_sb, k_ss, k_sb, v_ss, v_sb, o_st, o_sb; float scale;
};
template <typename T>
__global__ __launch_bounds__(64) void causal_fwd_kernel(CausalArgs a) {
  const int i = blockIdx.x, b = blockIdx.y / a.H, h = blockIdx.y % a.H, d = threadIdx.x;
  const long hd = (long)h * a.D + d;
  const float qd = ld(static_cast<const T*>(a.q) + i * a.q_st + b * a.q_sb + hd) * a.scale;
  const int n = min(a.pos0 + i, a.S);
  float m = 0.f, l = 1.f, acc = 0.f;                 // the zero slot
  for (int s = 0; s < n; ++s) {
    const float dot = wave_sum(qd * ld(static_cast<const T*>(a.k) + s * a.k_ss + b * a.k_sb + hd));
    const float vd = ld(static_cast<const T*>(a.v) + s * a.v_ss + b * a.v_sb + hd);
    if (dot > m) {
      const float c = __expf(m - dot);
      l = l * c + 1.f;
      acc = acc * c + vd;
      m = dot;
    } else {
      const float e = __expf(dot - m);
      l += e;
      acc += e * vd;
    }
  }
  st(static_cast<T*>(a.out) + i * a.o_st + b * a.o_sb + hd, acc / l);
  if (d == 0) a.lse[((long)b * a.H + h) * a.Tq + i] = m + __logf(l);
}
// dq and delta = dout . out (per (b, h, query)); Tq = S, pos0 = 0 (training)
template <typename T>
__global__ __launch_bounds__(64) void causal_bwd_q_kernel(CausalArgs a, const void* dout, void* dq,
                                                          float* __restrict__ delta) {
  const int i = blockIdx.x, b = blockIdx.y / a.H, h = blockIdx.y % a.H, d = threadIdx.x;
  const long hd = (long)h * a.D + d;
  const long qo = i * a.q_st + b * a.q_sb + hd, oo = i * a.o_st + b * a.o_sb + hd;
  const float qd = ld(static_cast<const T*>(a.q) + qo) * a.scale;
  const float gd = ld(static_cast<const T*>(dout) + oo);
  const float dl = wave_sum(gd * ld(static_cast<const T*>(a.out) + oo));
  const long row = ((long)b * a.H + h) * a.Tq + i;
  const float lz = a.lse[row];
  float acc = 0.f;
  for (int s = 0; s < min(a.pos0 + i, a.S); ++s) {
    const float kd = ld(static_cast<const T*>(a.k) + s * a.k_ss + b * a.k_sb + hd);
    const float vd = ld(static_cast<const T*>(a.v) + s * a.v_ss + b * a.v_sb + hd);
    const float pr = __expf(wave_sum(qd * kd) - lz);
    const float dp = wave_sum(gd * vd);
    acc += pr * (dp - dl) * kd;
  }
  st(static_cast<T*>(dq) + qo, acc * a.scale);
  if (d == 0) delta[row] = dl;
}
// dk, dv of key s: the queries i with pos0 + i > s (dk, dv share k's / v's strides)
template <typename T>
__global__ __launch_bounds__(64) void causal_bwd_kv_kernel(CausalArgs a, const void* dout, const float* __restrict__ delta,
                                                           void* dk, void* dv) {
  const int s = blockIdx.x, b = blockIdx.y / a.H, h = blockIdx.y % a.H, d = threadIdx.x;
  const long hd = (long)h * a.D + d;
  const float kd = ld(static_cast<const T*>(a.k) + s * a.k_ss + b * a.k_sb + hd);
  const float vd = ld(static_cast<const T*>(a.v) + s * a.v_ss + b * a.v_sb + hd);
  float ak = 0.f, av = 0.f;
  for (int i = max(s + 1 - a.pos0, 0); i < a.Tq; ++i) {
    const long row = ((long)b * a.H + h) * a.Tq + i;
    const float qd = ld(static_cast<const T*>(a.q) + i * a.q_st + b * a.q_sb + hd) * a.scale;
    const float gd = ld(static_cast<const T*>(dout) + i * a.o_st + b * a.o_sb + hd);
    const float pr = __expf(wave_sum(qd * kd) - a.lse[row]);
    const float dp = wave_sum(gd * vd);
    ak += pr * (dp - delta[row]) * qd;
    av += pr * gd;
  }
  st(static_cast<T*>(dk) + s * a.k_ss + b * a.k_sb + hd, ak);          // (qd carries the scale)
  st(static_cast<T*>(dv) + s * a.v_ss + b * a.v_sb + hd, av);
}

// ------------------------------------------------------------------ generation: the copy decision of one step
// grid Ba (alive rows), rows[i] = the row's original batch row.  One-query copy attention over the article keys
// (projected once per batch), proper mask, per-id sums (chain walk in position order), arg-max with ties to the lower
// id, the 1e-6 rule, the has-copied check against hist[row, 0 .. n_hist), the entity arg-max (ties to index 0).
template <typename T>
__global__ __launch_bounds__(NT) void copy_step_kernel(const T* __restrict__ q, long q_sb, const T* __restrict__ k,
                                                       long k_ss, long k_sb, const T* __restrict__ bias_k,
                                                       const uint8_t* __restrict__ mask, const int8_t* __restrict__ proper,
                                                       const long* __restrict__ ctx, const int* __restrict__ rows,
                                                       const float* __restrict__ ent, const long* __restrict__ gen,
                                                       long* __restrict__ hist, int hist_len, int n_hist, int H, int S,
                                                       int D, long* __restrict__ tok, uint8_t* __restrict__ copy,
                                                       float* __restrict__ prob) {
  __shared__ float qs[64];
  __shared__ float lg[MAX_S + 2];
  __shared__ float wsum[MAX_S];
  __shared__ int sid[MAX_S];
  __shared__ int nxt[MAX_S];
  __shared__ uint8_t head[MAX_S];
  __shared__ float red[NW];
  __shared__ float bestp[NT];
  __shared__ int bestid[NT];
  const int i = blockIdx.x, b = rows[i], S2 = S + 2;
  for (int s = threadIdx.x; s < S; s += NT) wsum[s] = 0.f;
  for (int h = 0; h < H; ++h) {
    __syncthreads();
    if (threadIdx.x < 64) qs[threadIdx.x] = threadIdx.x < D ? ld(q + i * q_sb + (long)h * D + threadIdx.x) : 0.f;
    __syncthreads();
    for (int s = threadIdx.x; s < S2; s += NT) {
      const bool masked = s < S && mask && mask[(long)b * S + s];
      float dot = 0.f;
      if (s < S + 1 && !masked) {
        const T* kp = s < S ? k + s * k_ss + b * k_sb + (long)h * D : bias_k + (long)h * D;
        for (int d = 0; d < D; ++d) dot += qs[d] * ld(kp + d);
      }
      lg[s] = masked ? -INFINITY : dot;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int s = threadIdx.x; s < S2; s += NT) m = fmaxf(m, lg[s]);
    m = block_max(m, red);
    float l = 0.f;
    for (int s = threadIdx.x; s < S2; s += NT) l += __expf(lg[s] - m);
    l = block_sum(l, red);
    const float lz = m + __logf(l);
    for (int s = threadIdx.x; s < S; s += NT) wsum[s] += __expf(lg[s] - lz);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < S; s += NT) {
    const bool keep = !proper || proper[(long)b * S + s] >= 1;
    wsum[s] = keep ? wsum[s] / H : 0.f;
  }
  dedupe_row(ctx + (long)b * S, S, sid, nxt, head);       // (its barriers publish wsum)
  float bp = -1.f;
  int bi = 0x7fffffff;
  for (int s = threadIdx.x; s < S; s += NT) {
    if (!head[s]) continue;
    float p = 0.f;
    for (int j = s; j >= 0; j = nxt[j]) p += wsum[j];
    if (p > bp || (p == bp && sid[s] < bi)) { bp = p; bi = sid[s]; }
  }
  bestp[threadIdx.x] = bp;
  bestid[threadIdx.x] = bi;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const float p2 = bestp[threadIdx.x + o];
      const int i2 = bestid[threadIdx.x + o];
      if (p2 > bestp[threadIdx.x] || (p2 == bestp[threadIdx.x] && i2 < bestid[threadIdx.x])) {
        bestp[threadIdx.x] = p2;
        bestid[threadIdx.x] = i2;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float p = bestp[0];
    const long id = bestid[0] == 0x7fffffff ? 0 : bestid[0];
    const bool empty = p < 1e-6f;
    if (empty) p = 1e-6f;
    bool should = ent[2 * i + 1] > ent[2 * i] && !empty;
    for (int j = 0; j < n_hist && should; ++j)
      if (hist[(long)b * hist_len + j] == id) should = false;
    hist[(long)b * hist_len + n_hist] = should ? id : -1;
    tok[i] = should ? id : gen[i];
    copy[i] = should;
    prob[i] = p;
  }
}

}  // namespace

// ------------------------------------------------------------------ C ABI
#define TELL_DISPATCH(dtype, KERNEL, grid, block, ...)                                              \
  do {                                                                                              \
    if ((dtype) == TELL_BF16) hipLaunchKernelGGL((KERNEL<uint16_t>), grid, block, 0, stream, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<float>), grid, block, 0, stream, __VA_ARGS__);                  \
  } while (0)

static int copy_args(CopyAttnArgs& a, const void* q, const void* k, const void* bias_k, const uint8_t* mask,
                     const int8_t* proper, int B, int H, int T, int S, int D, long q_st, long q_sb, long k_ss,
                     long k_sb, float p, uint32_t seed, uint32_t salt, int dtype) {
  TELL_REQUIRE(D > 0 && D <= 64, "copy_attn: head_dim must be <= 64");
  TELL_REQUIRE(B > 0 && H > 0 && T > 0 && S >= 0 && S <= MAX_S, "copy_attn: bad sizes (S <= 512)");
  TELL_REQUIRE(bias_k != nullptr, "copy_attn: bias_k is required");
  TELL_REQUIRE(p >= 0.f && p < 1.f, "copy_attn: dropout p must be in [0,1)");
  TELL_REQUIRE(dtype == TELL_F32 || dtype == TELL_BF16, "copy_attn: bad dtype");
  a = CopyAttnArgs{q, k, bias_k, mask, proper, B, H, T, S, D, q_st, q_sb, k_ss, k_sb, p, seed, salt, g_tell_rng_step};
  return TELL_OK;
}

extern "C" int tell_copy_attn_fwd(const void* q, const void* k, const void* bias_k, const uint8_t* mask,
                                  const int8_t* proper, float* w, float* lse, int B, int H, int T, int S, int D,
                                  long q_st, long q_sb, long k_ss, long k_sb, float p, uint32_t seed, uint32_t salt,
                                  int dtype, hipStream_t stream) {
  CopyAttnArgs a;
  int rc = copy_args(a, q, k, bias_k, mask, proper, B, H, T, S, D, q_st, q_sb, k_ss, k_sb, p, seed, salt, dtype);
  if (rc) return rc;
  TELL_DISPATCH(dtype, copy_attn_fwd_kernel, dim3((T + RT - 1) / RT, B), dim3(NT), a, w, lse);
  return tell_check_launch("copy_attn_fwd");
}

extern "C" int tell_copy_attn_bwd(const void* q, const void* k, const void* bias_k, const uint8_t* mask,
                                  const int8_t* proper, const float* lse, const float* dw, void* dq, void* dk,
                                  float* dbias_k_rows, float* delta, int B, int H, int T, int S, int D, long q_st,
                                  long q_sb, long k_ss, long k_sb, float p, uint32_t seed, uint32_t salt, int dtype,
                                  hipStream_t stream) {
  CopyAttnArgs a;
  int rc = copy_args(a, q, k, bias_k, mask, proper, B, H, T, S, D, q_st, q_sb, k_ss, k_sb, p, seed, salt, dtype);
  if (rc) return rc;
  TELL_DISPATCH(dtype, copy_attn_bwd_q_kernel, dim3((T + RT - 1) / RT, B), dim3(NT), a, lse, dw, dq, delta,
                dbias_k_rows);
  if (S > 0) TELL_DISPATCH(dtype, copy_attn_bwd_k_kernel, dim3((S + NW - 1) / NW, B), dim3(NT), a, lse, dw, delta, dk);
  return tell_check_launch("copy_attn_bwd");
}

extern "C" int tell_copy_vocab_count(const long* ctx_ids, long n_ctx, const long* targets, int B, int T, long tgt_sb,
                                     int vocab, uint32_t* bitmap, int* count, hipStream_t stream) {
  TELL_REQUIRE(vocab > 0 && B >= 0 && T >= 0 && n_ctx >= 0, "copy_vocab_count: bad sizes");
  const int words = (vocab + 31) / 32;
  if (hipMemsetAsync(bitmap, 0, (size_t)(words + 1) * 4, stream) != hipSuccess) return tell_check_launch("copy_vocab_count");
  const long n = n_ctx + (long)B * T;
  if (n > 0)
    hipLaunchKernelGGL(vocab_mark_kernel, dim3((unsigned)min((n + 255) / 256, 1024L)), dim3(256), 0, stream, ctx_ids,
                       n_ctx, targets, B, T, tgt_sb, vocab, bitmap);
  hipLaunchKernelGGL(vocab_count_kernel, dim3(1), dim3(NT), 0, stream, bitmap, words, count);
  return tell_check_launch("copy_vocab_count");
}

extern "C" int tell_copy_loss_fwd(const float* w, const long* ctx_ids, const long* targets, long tgt_sb,
                                  const long* copy_mask, long cm_sb, const int* vcount, int variant, int B, int T,
                                  int S, float* term, float* p_target, float* z, float* scale, float* loss,
                                  hipStream_t stream) {
  TELL_REQUIRE(B > 0 && T > 0 && S >= 0 && S <= MAX_S, "copy_loss: bad sizes (S <= 512)");
  TELL_REQUIRE(variant == 1 || variant == 2, "copy_loss: variant must be 1 or 2");
  TELL_REQUIRE(variant == 1 || vcount != nullptr, "copy_loss: variant 2 needs the vocabulary count");
  hipLaunchKernelGGL(copy_loss_rows_kernel, dim3(B), dim3(NT), 0, stream, w, ctx_ids, targets, tgt_sb, copy_mask,
                     cm_sb, vcount, variant, T, S, term, p_target, z);
  hipLaunchKernelGGL(copy_loss_reduce_kernel, dim3(1), dim3(NT), 0, stream, term, copy_mask, cm_sb, B, T, loss, scale);
  return tell_check_launch("copy_loss_fwd");
}

extern "C" int tell_copy_loss_bwd(const float* dloss, const float* w, const long* ctx_ids, const long* targets,
                                  long tgt_sb, const long* copy_mask, long cm_sb, const float* p_target, const float* z,
                                  const float* scale, int variant, int B, int T, int S, float* dw, hipStream_t stream) {
  TELL_REQUIRE(B > 0 && T > 0 && S >= 0 && S <= MAX_S, "copy_loss_bwd: bad sizes (S <= 512)");
  if (S == 0) return TELL_OK;
  hipLaunchKernelGGL(copy_loss_bwd_kernel, dim3(T, B), dim3(NT), 0, stream, dloss, w, ctx_ids, targets, tgt_sb,
                     copy_mask, cm_sb, p_target, z, scale, variant, T, S, dw);
  return tell_check_launch("copy_loss_bwd");
}

extern "C" int tell_entity_head_fwd(const void* x, long x_st, long x_sb, const float* w, const float* bias,
                                    const long* copy_mask, long cm_sb, int B, int T, int E, float* logits, float* loss,
                                    float* nvalid, int dtype, hipStream_t stream) {
  TELL_REQUIRE(B > 0 && T > 0 && E > 0, "entity_head: bad sizes");
  if (dtype == TELL_BF16)
    hipLaunchKernelGGL(entity_logits_kernel<uint16_t>, dim3(B * T), dim3(64), 0, stream, (const uint16_t*)x, x_st, x_sb,
                       w, bias, B, T, E, logits);
  else
    hipLaunchKernelGGL(entity_logits_kernel<float>, dim3(B * T), dim3(64), 0, stream, (const float*)x, x_st, x_sb, w,
                       bias, B, T, E, logits);
  hipLaunchKernelGGL(entity_ce_kernel, dim3(1), dim3(NT), 0, stream, logits, copy_mask, cm_sb, B, T, loss, nvalid);
  return tell_check_launch("entity_head_fwd");
}

extern "C" int tell_entity_logits(const void* x, long x_st, long x_sb, const float* w, const float* bias, int B, int T,
                                  int E, float* logits, int dtype, hipStream_t stream) {
  TELL_REQUIRE(B > 0 && T > 0 && E > 0, "entity_logits: bad sizes");
  if (dtype == TELL_BF16)
    hipLaunchKernelGGL(entity_logits_kernel<uint16_t>, dim3(B * T), dim3(64), 0, stream, (const uint16_t*)x, x_st, x_sb,
                       w, bias, B, T, E, logits);
  else
    hipLaunchKernelGGL(entity_logits_kernel<float>, dim3(B * T), dim3(64), 0, stream, (const float*)x, x_st, x_sb, w,
                       bias, B, T, E, logits);
  return tell_check_launch("entity_logits");
}

extern "C" int tell_entity_head_bwd(const float* dloss, const float* nvalid, const float* logits, const long* copy_mask,
                                    long cm_sb, const void* x, long x_st, long x_sb, const float* w, void* dx,
                                    long dx_st, long dx_sb, float* dlogits, float* dw, float* dbias, int B, int T,
                                    int E, int dtype, hipStream_t stream) {
  TELL_REQUIRE(B > 0 && T > 0 && E > 0, "entity_head_bwd: bad sizes");
  if (dtype == TELL_BF16) {
    hipLaunchKernelGGL(entity_dx_kernel<uint16_t>, dim3(B * T), dim3(64), 0, stream, dloss, nvalid, logits, copy_mask,
                       cm_sb, w, B, T, E, (uint16_t*)dx, dx_st, dx_sb, dlogits);
    hipLaunchKernelGGL(entity_dw_kernel<uint16_t>, dim3((E + 63) / 64), dim3(NT), 0, stream, dlogits,
                       (const uint16_t*)x, x_st, x_sb, B, T, E, dw, dbias);
  } else {
    hipLaunchKernelGGL(entity_dx_kernel<float>, dim3(B * T), dim3(64), 0, stream, dloss, nvalid, logits, copy_mask,
                       cm_sb, w, B, T, E, (float*)dx, dx_st, dx_sb, dlogits);
    hipLaunchKernelGGL(entity_dw_kernel<float>, dim3((E + 63) / 64), dim3(NT), 0, stream, dlogits, (const float*)x,
                       x_st, x_sb, B, T, E, dw, dbias);
  }
  return tell_check_launch("entity_head_bwd");
}

static int causal_args(CausalArgs& a, const void* q, const void* k, const void* v, void* out, float* lse, int B, int H,
                       int Tq, int S, int D, int pos0, long q_st, long q_sb, long k_ss, long k_sb, long v_ss,
                       long v_sb, long o_st, long o_sb, float scale, int dtype) {
  TELL_REQUIRE(D == 64, "causal_attn: head_dim must be 64");
  TELL_REQUIRE(B > 0 && H > 0 && Tq > 0 && S >= 0 && pos0 >= 0, "causal_attn: bad sizes");
  TELL_REQUIRE(dtype == TELL_F32 || dtype == TELL_BF16, "causal_attn: bad dtype");
  a = CausalArgs{q, k, v, out, lse, B, H, Tq, S, D, pos0, q_st, q_sb, k_ss, k_sb, v_ss, v_sb, o_st, o_sb, scale};
  return TELL_OK;
}

extern "C" int tell_causal_attn_fwd(const void* q, const void* k, const void* v, void* out, float* lse, int B, int H,
                                    int Tq, int S, int D, int pos0, long q_st, long q_sb, long k_ss, long k_sb,
                                    long v_ss, long v_sb, long o_st, long o_sb, float scale, int dtype,
                                    hipStream_t stream) {
  CausalArgs a;
  int rc = causal_args(a, q, k, v, out, lse, B, H, Tq, S, D, pos0, q_st, q_sb, k_ss, k_sb, v_ss, v_sb, o_st, o_sb, scale,
                       dtype);
  if (rc) return rc;
  TELL_DISPATCH(dtype, causal_fwd_kernel, dim3(Tq, B * H), dim3(64), a);
  return tell_check_launch("causal_attn_fwd");
}

extern "C" int tell_causal_attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                                    const float* lse, void* dq, void* dk, void* dv, float* delta, int B, int H, int T,
                                    int D, long q_st, long q_sb, long k_ss, long k_sb, long v_ss, long v_sb, long o_st,
                                    long o_sb, float scale, int dtype, hipStream_t stream) {
  CausalArgs a;
  int rc = causal_args(a, q, k, v, const_cast<void*>(out), const_cast<float*>(lse), B, H, T, T, D, 0, q_st, q_sb, k_ss,
                       k_sb, v_ss, v_sb, o_st, o_sb, scale, dtype);
  if (rc) return rc;
  TELL_DISPATCH(dtype, causal_bwd_q_kernel, dim3(T, B * H), dim3(64), a, dout, dq, delta);
  TELL_DISPATCH(dtype, causal_bwd_kv_kernel, dim3(T, B * H), dim3(64), a, dout, (const float*)delta, dk, dv);
  return tell_check_launch("causal_attn_bwd");
}

extern "C" int tell_copy_step(const void* q, long q_sb, const void* k, long k_ss, long k_sb, const void* bias_k,
                              const uint8_t* mask, const int8_t* proper, const long* ctx_ids, const int* rows,
                              const float* entity_logits, const long* gen_tok, long* hist, int hist_len, int n_hist,
                              int Ba, int H, int S, int D, long* tok, uint8_t* copied, float* prob, int dtype,
                              hipStream_t stream) {
  TELL_REQUIRE(D > 0 && D <= 64 && H > 0 && S >= 0 && S <= MAX_S, "copy_step: bad sizes (D <= 64, S <= 512)");
  TELL_REQUIRE(n_hist >= 0 && n_hist < hist_len, "copy_step: history is full");
  TELL_REQUIRE(bias_k != nullptr, "copy_step: bias_k is required");
  if (Ba <= 0) return TELL_OK;
  if (dtype == TELL_BF16)
    hipLaunchKernelGGL(copy_step_kernel<uint16_t>, dim3(Ba), dim3(NT), 0, stream, (const uint16_t*)q, q_sb,
                       (const uint16_t*)k, k_ss, k_sb, (const uint16_t*)bias_k, mask, proper, ctx_ids, rows,
                       entity_logits, gen_tok, hist, hist_len, n_hist, H, S, D, tok, copied, prob);
  else
    hipLaunchKernelGGL(copy_step_kernel<float>, dim3(Ba), dim3(NT), 0, stream, (const float*)q, q_sb, (const float*)k,
                       k_ss, k_sb, (const float*)bias_k, mask, proper, ctx_ids, rows, entity_logits, gen_tok, hist,
                       hist_len, n_hist, H, S, D, tok, copied, prob);
  return tell_check_launch("copy_step");
}
