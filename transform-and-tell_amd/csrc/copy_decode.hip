// The copy models' decode step on static shapes (include/tell_hip.h "copy mechanism, cached generation"; DESIGN.md
// section 27): the two kernels that end a step of transformer_pointer / transformer_pointer_2 when the step is issued over a
// batch that keeps its shape - no row map, no growing history, the step index from the host or from the device counter of
// a captured step (*step_dev + 1, the convention of tell_greedy_update).
//
//  * tell_entity_attn_step: the one-query causal entity attention of step p over a static K/V history [L, B, H*64]: one
//    wave per (row, head) writes row p of both histories from this step's projections and attends to rows 0 .. p-1 plus the
//    zero slot - slot p is never read at step p, so appending and attending need no ordering.  The loop is the online
//    softmax of causal_fwd_kernel (csrc/copy.hip), restated here because that file's kernels are private to it.
//  * tell_copy_decide: tell_copy_step for a static batch, head-parallel.  Launch 1, grid (row, head): the head's
//    probabilities over the article into an fp32 scratch [B, H, S]; a key's D-wide head slice is read by 64 / VEC adjacent
//    lanes in 16-byte pieces, so a wave instruction reads whole 128-byte segments.  Launch 2, grid rows: heads summed in
//    ascending order, proper mask, per-id chains, arg-max, the rules and the stores of copy_step_kernel.
//    The arithmetic of a key does not depend on its position s (the same pieces, the same butterfly, the same exp), so
//    byte-identical key rows get bit-equal weights.
//  * tell_copy_decide_hyp: tell_copy_decide for n hypotheses per image, rows r = b n + j over the
//    keys, masks and ids of B images.  Launch 1, grid (image, head, chunk of HYP_CHUNK hypotheses): every key slice is
//    loaded once per workgroup and multiplied with the chunk's queries; per row the arithmetic of copy_probs_kernel, so its
//    outputs are that kernel's over the n-times repeated keys, bit for bit.  Launch 2 is tell_copy_decide's with r / n as
//    the row of proper and ctx_ids.
//
// Plain FMA code; every launcher is asynchronous: no host synchronisation, no allocation.
#include "common.h"

namespace {

constexpr int NT = 256;           // threads per workgroup
constexpr int NW = NT / 64;
constexpr int MAX_S = 512;        // article positions a workgroup keeps in LDS
constexpr int MAX_HYP = 16;       // hypotheses per image (tell_sample_rank's limit)
constexpr int HYP_CHUNK = 4;      // ... of which one workgroup of copy_probs_hyp_kernel serves this many

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

// ------------------------------------------------------------------ entity attention of one step
// grid B * H, one wave each, lane d (D = 64).  p: the step; row p of the histories <- k_new / v_new (p < L), the query sees
// rows s < min(p, L) and the zero slot (logit 0, value 0) as the first term of the online softmax.
template <typename T>
__global__ __launch_bounds__(64) void entity_attn_step_kernel(const T* __restrict__ q, long q_sb, const T* __restrict__ kn,
                                                              long kn_sb, const T* __restrict__ vn, long vn_sb,
                                                              T* k_hist, T* v_hist, long h_ss, long h_sb,
                                                              T* __restrict__ out, long o_sb, int H, int L, float scale,
                                                              int step, const int* __restrict__ step_dev) {
  const int p = step_dev ? *step_dev + 1 : step;
  const int b = blockIdx.x / H, h = blockIdx.x % H, d = threadIdx.x;
  const long hd = (long)h * 64 + d;
  if (p >= 0 && p < L) {                                       // (a raw 2- or 4-byte copy: bit for bit)
    k_hist[p * h_ss + b * h_sb + hd] = kn[b * kn_sb + hd];
    v_hist[p * h_ss + b * h_sb + hd] = vn[b * vn_sb + hd];
  }
  const float qd = ld(q + b * q_sb + hd) * scale;
  const int n = min(max(p, 0), L);
  float m = 0.f, l = 1.f, acc = 0.f;                           // the zero slot
  for (int s = 0; s < n; ++s) {
    const float dot = wave_sum(qd * ld(k_hist + s * h_ss + b * h_sb + hd));
    const float vd = ld(v_hist + s * h_ss + b * h_sb + hd);
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
  st(out + b * o_sb + hd, acc / l);
}

// ------------------------------------------------------------------ copy decision, launch 1: per-head probabilities
// grid (B, H).  LPK = 64 / VEC lanes share a key: lane g of the group holds elements g VEC .. g VEC + VEC - 1 of the head
// slice (zero beyond D) - one 16-byte load when `vec` (every base and stride a multiple of 16 bytes, D a multiple of VEC),
// element loads otherwise, the same products either way - multiplies them with its piece of the query in element order and
// the group adds its partial sums by an xor butterfly.  Column S is bias_k, column S + 1 the zero key.
template <typename T>
__global__ __launch_bounds__(NT) void copy_probs_kernel(const T* __restrict__ q, long q_sb, const T* __restrict__ k, long k_ss,
                                                        long k_sb, const T* __restrict__ bias_k,
                                                        const uint8_t* __restrict__ mask,
                                                        const uint8_t* __restrict__ finished, int H, int S, int D, int vec,
                                                        float* __restrict__ scratch) {
  constexpr int VEC = Elem<T>::VEC, LPK = 64 / VEC, KPP = NT / LPK, UNR = 4;
  __shared__ float lg[MAX_S + 2];
  __shared__ float red[NW];
  const int b = blockIdx.x, h = blockIdx.y, S2 = S + 2;
  if (finished && finished[b]) return;                         // (the whole workgroup: no barrier is left half-way)
  const int g = threadIdx.x % LPK, slot = threadIdx.x / LPK, d0 = g * VEC;
  float qv[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) qv[j] = d0 + j < D ? ld(q + b * q_sb + (long)h * D + d0 + j) : 0.f;
  // UNR keys per thread and trip: their loads are issued together (a masked key is loaded like any other - it lies inside
  // the article's rows - and its logit replaced afterwards), then the products
  for (int s0 = 0; s0 < S2; s0 += KPP * UNR) {
    float kv[UNR][VEC];
    bool masked[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int s = s0 + u * KPP + slot;
      masked[u] = s < S && mask && mask[(long)b * S + s];
#pragma unroll
      for (int j = 0; j < VEC; ++j) kv[u][j] = 0.f;
      if (s <= S && d0 < D) {
        const T* kp = (s < S ? k + s * k_ss + b * k_sb : bias_k) + (long)h * D + d0;
        if (vec) {
          unpack16(*reinterpret_cast<const uint4*>(kp), kv[u], kp);
        } else {
#pragma unroll
          for (int j = 0; j < VEC; ++j)
            if (d0 + j < D) kv[u][j] = ld(kp + j);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int s = s0 + u * KPP + slot;
      float part = 0.f;
#pragma unroll
      for (int j = 0; j < VEC; ++j) part += qv[j] * kv[u][j];
#pragma unroll
      for (int o = LPK / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
      if (g == 0 && s < S2) lg[s] = masked[u] ? -INFINITY : part;
    }
  }
  __syncthreads();
  float m = -INFINITY;
  for (int s = threadIdx.x; s < S2; s += NT) m = fmaxf(m, lg[s]);
  m = block_max(m, red);                                       // >= 0: the zero key is never masked
  float l = 0.f;
  for (int s = threadIdx.x; s < S2; s += NT) l += __expf(lg[s] - m);
  l = block_sum(l, red);
  const float lz = m + __logf(l);
  float* out = scratch + ((long)b * H + h) * S;
  for (int s = threadIdx.x; s < S; s += NT) out[s] = __expf(lg[s] - lz);
}

// block-wide reductions of CH values at once: per value the order of block_max / block_sum (wave reduction, then the waves
// in ascending order), one pair of barriers for all of them; `red` holds CH * NW floats
template <int CH>
__device__ __forceinline__ void block_max_n(float (&v)[CH], float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < CH; ++c) v[c] = wave_max(v[c]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < CH; ++c) red[c * NW + w] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    float r = red[c * NW];
    for (int i = 1; i < NW; ++i) r = fmaxf(r, red[c * NW + i]);
    v[c] = r;
  }
}
template <int CH>
__device__ __forceinline__ void block_sum_n(float (&v)[CH], float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < CH; ++c) v[c] = wave_sum(v[c]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < CH; ++c) red[c * NW + w] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    float r = red[c * NW];
    for (int i = 1; i < NW; ++i) r += red[c * NW + i];
    v[c] = r;
  }
}

// ------------------------------------------------------------------ copy decision for n hypotheses per image, launch 1
// grid (B images, H, chunks of CH hypotheses).  copy_probs_kernel with CH queries against one pass over the image's keys:
// hypothesis j of image b is row r = b n + j of q / finished / scratch, the keys and the mask are image b's.  A key's head
// slice is loaded once per workgroup and multiplied with the CH queries the lanes keep in registers; per row the arithmetic
// is copy_probs_kernel's, term by term (the lane pieces in element order, the xor butterfly, the strided partial sums of
// the 256 threads, wave reduction, waves in ascending order, __expf(lg - lz)), so row r gets the bits copy_probs_kernel
// gives it over the n-times repeated keys.  A finished hypothesis, or a slot past n in the last chunk, is `dead`: its query
// is not loaded (zeros take its place in the products) and nothing is stored for it.
template <typename T, int CH>
__global__ __launch_bounds__(NT) void copy_probs_hyp_kernel(const T* __restrict__ q, long q_sb, const T* __restrict__ k,
                                                            long k_ss, long k_sb, const T* __restrict__ bias_k,
                                                            const uint8_t* __restrict__ mask,
                                                            const uint8_t* __restrict__ finished, int n, int H, int S, int D,
                                                            int vec, float* __restrict__ scratch) {
  constexpr int VEC = Elem<T>::VEC, LPK = 64 / VEC, KPP = NT / LPK, UNR = 4;
  __shared__ float lg[CH][MAX_S + 2];
  __shared__ float red[CH * NW];
  const int b = blockIdx.x, h = blockIdx.y, j0 = blockIdx.z * CH, S2 = S + 2;
  const long r0 = (long)b * n + j0;
  bool live[CH];
  bool any = false;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    live[c] = j0 + c < n && !(finished && finished[r0 + c]);
    any = any || live[c];
  }
  if (!any) return;                                            // (the whole workgroup, in front of every barrier and load)
  const int g = threadIdx.x % LPK, slot = threadIdx.x / LPK, d0 = g * VEC;
  float qv[CH][VEC];
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      qv[c][j] = live[c] && d0 + j < D ? ld(q + (r0 + c) * q_sb + (long)h * D + d0 + j) : 0.f;
  for (int s0 = 0; s0 < S2; s0 += KPP * UNR) {
    float kv[UNR][VEC];
    bool masked[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int s = s0 + u * KPP + slot;
      masked[u] = s < S && mask && mask[(long)b * S + s];
#pragma unroll
      for (int j = 0; j < VEC; ++j) kv[u][j] = 0.f;
      if (s <= S && d0 < D) {
        const T* kp = (s < S ? k + s * k_ss + b * k_sb : bias_k) + (long)h * D + d0;
        if (vec) {
          unpack16(*reinterpret_cast<const uint4*>(kp), kv[u], kp);
        } else {
#pragma unroll
          for (int j = 0; j < VEC; ++j)
            if (d0 + j < D) kv[u][j] = ld(kp + j);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int s = s0 + u * KPP + slot;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        float part = 0.f;
#pragma unroll
        for (int j = 0; j < VEC; ++j) part += qv[c][j] * kv[u][j];
#pragma unroll
        for (int o = LPK / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        if (g == 0 && s < S2) lg[c][s] = masked[u] ? -INFINITY : part;
      }
    }
  }
  __syncthreads();
  float m[CH], l[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    m[c] = -INFINITY;
    for (int s = threadIdx.x; s < S2; s += NT) m[c] = fmaxf(m[c], lg[c][s]);
  }
  block_max_n<CH>(m, red);                                     // >= 0: the zero key is never masked
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    l[c] = 0.f;
    for (int s = threadIdx.x; s < S2; s += NT) l[c] += __expf(lg[c][s] - m[c]);
  }
  block_sum_n<CH>(l, red);
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (!live[c]) continue;                                    // (the same in every thread; no barrier behind it)
    const float lz = m[c] + __logf(l[c]);
    float* out = scratch + ((r0 + c) * H + h) * S;
    for (int s = threadIdx.x; s < S; s += NT) out[s] = __expf(lg[c][s] - lz);
  }
}

// nxt[s] = the next position holding the same id (-1 at the end of a chain), head[s] = 1 at the first occurrence - what
// dedupe_row of csrc/copy.hip computes, by another route: a thread finds the PREVIOUS occurrence of its position's id (the
// last match of one walk over the positions in front of it, no data-dependent exit: every lane reads the same sid[j], an
// LDS broadcast, and the loop pipelines), which makes it a head or the successor of that occurrence.  Thread i takes
// positions i and S - 1 - i, so every wave walks about S positions.
__device__ void dedupe_row(const long* __restrict__ ids, int S, int* sid, int* nxt, uint8_t* head) {
  for (int s = threadIdx.x; s < S; s += NT) {
    sid[s] = (int)ids[s];
    nxt[s] = -1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (S + 1) / 2; i += NT) {
    const int sa = i, sb = S - 1 - i;                          // sa <= sb
    const int va = sid[sa], vb = sid[sb];
    int pa = -1, pb = -1;
#pragma unroll 4
    for (int j = 0; j < sa; ++j) {
      const int x = sid[j];
      pa = x == va ? j : pa;
      pb = x == vb ? j : pb;
    }
#pragma unroll 4
    for (int j = sa; j < sb; ++j) pb = sid[j] == vb ? j : pb;
    head[sa] = pa < 0;
    if (pa >= 0) nxt[pa] = sa;                                 // (a position is the predecessor of one position at most)
    if (sb != sa) {
      head[sb] = pb < 0;
      if (pb >= 0) nxt[pb] = sb;
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------ copy decision, launch 2: the row's decision
// grid rows (n rows per image; tell_copy_decide: n = 1).  Head mean (heads added in ascending order), proper mask, per-id sums along the chains in position order, arg-max
// with ties to the lower id, the 1e-6 rule, the has-copied check against hist[b, 0 .. p], the entity arg-max (ties to
// index 0); stores of an unfinished row: tok[b], hist[b, p + 1], copied[b, p + 1], prob[b, p].
__global__ __launch_bounds__(NT) void copy_finish_kernel(const float* __restrict__ scratch, const int8_t* __restrict__ proper,
                                                         const long* __restrict__ ctx, const float* __restrict__ ent,
                                                         const int* __restrict__ gen, const uint8_t* __restrict__ finished,
                                                         int* __restrict__ hist, long ld_hist, uint8_t* __restrict__ copied,
                                                         long ld_copied, float* __restrict__ prob, long ld_prob, int L,
                                                         int step, const int* __restrict__ step_dev, int H, int S,
                                                         int n, int* __restrict__ tok) {
  __shared__ float wsum[MAX_S];
  __shared__ int sid[MAX_S];
  __shared__ int nxt[MAX_S];
  __shared__ uint8_t head[MAX_S];
  __shared__ float bestp[NT];
  __shared__ int bestid[NT];
  const int p = step_dev ? *step_dev + 1 : step;
  const int b = blockIdx.x;
  const long img = b / n;                                      // proper / ctx: one row per image, n rows (hypotheses) each
  if (p < 0 || p >= L || (finished && finished[b])) return;    // (the whole workgroup)
  for (int s = threadIdx.x; s < S; s += NT) {
    float w = 0.f;
    for (int h = 0; h < H; ++h) w += scratch[((long)b * H + h) * S + s];
    const bool keep = !proper || proper[img * S + s] >= 1;
    wsum[s] = keep ? w / H : 0.f;
  }
  dedupe_row(ctx + img * S, S, sid, nxt, head);                   // (its barriers publish wsum)
  float bp = -1.f;
  int bi = 0x7fffffff;
  for (int s = threadIdx.x; s < S; s += NT) {
    if (!head[s]) continue;
    float pr = 0.f;
    for (int j = s; j >= 0; j = nxt[j]) pr += wsum[j];
    if (pr > bp || (pr == bp && sid[s] < bi)) { bp = pr; bi = sid[s]; }
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
  const int id = bestid[0] == 0x7fffffff ? 0 : bestid[0];
  int seen = 0;                                                // the has-copied check, all threads (one thread walking
  for (int j = threadIdx.x; j <= p; j += NT)                   // the history waits for a load per step taken so far)
    seen |= hist[(long)b * ld_hist + j] == id;
  seen = __syncthreads_or(seen);
  if (threadIdx.x == 0) {
    float pr = bestp[0];
    const bool empty = pr < 1e-6f;
    if (empty) pr = 1e-6f;
    const bool should = ent[2 * b + 1] > ent[2 * b] && !empty && !seen;
    hist[(long)b * ld_hist + p + 1] = should ? id : -1;
    copied[(long)b * ld_copied + p + 1] = should;
    prob[(long)b * ld_prob + p] = pr;
    tok[b] = should ? id : gen[b];
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" int tell_entity_attn_step(const void* q, long q_sb, const void* k_new, long kn_sb, const void* v_new, long vn_sb,
                                     void* k_hist, void* v_hist, long h_ss, long h_sb, void* out, long o_sb, int B, int H,
                                     int D, int L, float scale, int step, const int* step_dev, int dtype,
                                     hipStream_t stream) {
  TELL_REQUIRE(D == 64, "entity_attn_step: head_dim must be 64");
  TELL_REQUIRE(B > 0 && H > 0 && L > 0, "entity_attn_step: bad sizes");
  TELL_REQUIRE(dtype == TELL_F32 || dtype == TELL_BF16, "entity_attn_step: bad dtype");
  TELL_REQUIRE(q && k_new && v_new && k_hist && v_hist && out, "entity_attn_step: null pointer");
  TELL_REQUIRE(step_dev != nullptr || (step >= 0 && step < L), "entity_attn_step: the history is full (0 <= step < L)");
  if (dtype == TELL_BF16)
    hipLaunchKernelGGL(entity_attn_step_kernel<uint16_t>, dim3(B * H), dim3(64), 0, stream, (const uint16_t*)q, q_sb,
                       (const uint16_t*)k_new, kn_sb, (const uint16_t*)v_new, vn_sb, (uint16_t*)k_hist, (uint16_t*)v_hist,
                       h_ss, h_sb, (uint16_t*)out, o_sb, H, L, scale, step, step_dev);
  else
    hipLaunchKernelGGL(entity_attn_step_kernel<float>, dim3(B * H), dim3(64), 0, stream, (const float*)q, q_sb,
                       (const float*)k_new, kn_sb, (const float*)v_new, vn_sb, (float*)k_hist, (float*)v_hist, h_ss, h_sb,
                       (float*)out, o_sb, H, L, scale, step, step_dev);
  return tell_check_launch("entity_attn_step");
}

extern "C" int tell_copy_decide(const void* q, long q_sb, const void* k, long k_ss, long k_sb, const void* bias_k,
                                const uint8_t* mask, const int8_t* proper, const long* ctx_ids, const float* entity_logits,
                                const int* gen_tok, const uint8_t* finished, int* hist, long ld_hist, uint8_t* copied,
                                long ld_copied, float* prob, long ld_prob, int L, int step, const int* step_dev, int B, int H,
                                int S, int D, float* scratch, int* tok, int dtype, hipStream_t stream) {
  TELL_REQUIRE(D > 0 && D <= 64 && H > 0 && S >= 0 && S <= MAX_S, "copy_decide: bad sizes (D <= 64, S <= 512)");
  TELL_REQUIRE(bias_k != nullptr, "copy_decide: bias_k is required");
  TELL_REQUIRE(dtype == TELL_F32 || dtype == TELL_BF16, "copy_decide: bad dtype");
  TELL_REQUIRE(L > 0 && ld_hist >= L + 1 && ld_copied >= L + 1 && ld_prob >= L, "copy_decide: hist / copied [B, L + 1], prob [B, L]");
  TELL_REQUIRE(step_dev != nullptr || (step >= 0 && step < L), "copy_decide: the history is full (0 <= step < L)");
  TELL_REQUIRE(q && entity_logits && gen_tok && hist && copied && prob && tok && (S == 0 || (k && ctx_ids && scratch)),
               "copy_decide: null pointer");
  if (B <= 0) return TELL_OK;
  const long es = dtype == TELL_BF16 ? 2 : 4, vecn = 16 / es;
  const int vec = aligned16(k) && aligned16(bias_k) && (k_ss * es) % 16 == 0 && (k_sb * es) % 16 == 0 && D % vecn == 0;
  if (S > 0) {
    if (dtype == TELL_BF16)
      hipLaunchKernelGGL(copy_probs_kernel<uint16_t>, dim3(B, H), dim3(NT), 0, stream, (const uint16_t*)q, q_sb,
                         (const uint16_t*)k, k_ss, k_sb, (const uint16_t*)bias_k, mask, finished, H, S, D, vec, scratch);
    else
      hipLaunchKernelGGL(copy_probs_kernel<float>, dim3(B, H), dim3(NT), 0, stream, (const float*)q, q_sb, (const float*)k,
                         k_ss, k_sb, (const float*)bias_k, mask, finished, H, S, D, vec, scratch);
  }
  hipLaunchKernelGGL(copy_finish_kernel, dim3(B), dim3(NT), 0, stream, (const float*)scratch, proper, ctx_ids, entity_logits,
                     gen_tok, finished, hist, ld_hist, copied, ld_copied, prob, ld_prob, L, step, step_dev, H, S, 1, tok);
  return tell_check_launch("copy_decide");
}

namespace {

template <typename T, int CH>
void launch_probs_hyp(const void* q, long q_sb, const void* k, long k_ss, long k_sb, const void* bias_k, const uint8_t* mask,
                      const uint8_t* finished, int B, int n, int H, int S, int D, int vec, float* scratch,
                      hipStream_t stream) {
  hipLaunchKernelGGL((copy_probs_hyp_kernel<T, CH>), dim3(B, H, (n + CH - 1) / CH), dim3(NT), 0, stream, (const T*)q, q_sb,
                     (const T*)k, k_ss, k_sb, (const T*)bias_k, mask, finished, n, H, S, D, vec, scratch);
}

template <typename T>
void launch_probs_hyp(const void* q, long q_sb, const void* k, long k_ss, long k_sb, const void* bias_k, const uint8_t* mask,
                      const uint8_t* finished, int B, int n, int H, int S, int D, int vec, float* scratch,
                      hipStream_t stream) {
  // the chunk: HYP_CHUNK hypotheses of an image per workgroup, all n of them when there are fewer
  switch (n < HYP_CHUNK ? n : HYP_CHUNK) {
    case 1: launch_probs_hyp<T, 1>(q, q_sb, k, k_ss, k_sb, bias_k, mask, finished, B, n, H, S, D, vec, scratch, stream); break;
    case 2: launch_probs_hyp<T, 2>(q, q_sb, k, k_ss, k_sb, bias_k, mask, finished, B, n, H, S, D, vec, scratch, stream); break;
    case 3: launch_probs_hyp<T, 3>(q, q_sb, k, k_ss, k_sb, bias_k, mask, finished, B, n, H, S, D, vec, scratch, stream); break;
    default: launch_probs_hyp<T, 4>(q, q_sb, k, k_ss, k_sb, bias_k, mask, finished, B, n, H, S, D, vec, scratch, stream);
  }
}

}  // namespace

extern "C" int tell_copy_decide_hyp(const void* q, long q_sb, const void* k, long k_ss, long k_sb, const void* bias_k,
                                    const uint8_t* mask, const int8_t* proper, const long* ctx_ids,
                                    const float* entity_logits, const int* gen_tok, const uint8_t* finished, int* hist,
                                    long ld_hist, uint8_t* copied, long ld_copied, float* prob, long ld_prob, int L, int step,
                                    const int* step_dev, int B, int per_image, int H, int S, int D, float* scratch, int* tok,
                                    int dtype, hipStream_t stream) {
  TELL_REQUIRE(D > 0 && D <= 64 && H > 0 && S >= 0 && S <= MAX_S, "copy_decide_hyp: bad sizes (D <= 64, S <= 512)");
  TELL_REQUIRE(per_image >= 1 && per_image <= MAX_HYP, "copy_decide_hyp: per_image must be in 1..16");
  TELL_REQUIRE(bias_k != nullptr, "copy_decide_hyp: bias_k is required");
  TELL_REQUIRE(dtype == TELL_F32 || dtype == TELL_BF16, "copy_decide_hyp: bad dtype");
  TELL_REQUIRE(L > 0 && ld_hist >= L + 1 && ld_copied >= L + 1 && ld_prob >= L,
               "copy_decide_hyp: hist / copied [R, L + 1], prob [R, L]");
  TELL_REQUIRE(step_dev != nullptr || (step >= 0 && step < L), "copy_decide_hyp: the history is full (0 <= step < L)");
  TELL_REQUIRE(q && entity_logits && gen_tok && hist && copied && prob && tok && (S == 0 || (k && ctx_ids && scratch)),
               "copy_decide_hyp: null pointer");
  if (B <= 0) return TELL_OK;
  const long es = dtype == TELL_BF16 ? 2 : 4, vecn = 16 / es;
  const int vec = aligned16(k) && aligned16(bias_k) && (k_ss * es) % 16 == 0 && (k_sb * es) % 16 == 0 && D % vecn == 0;
  if (S > 0) {
    if (dtype == TELL_BF16)
      launch_probs_hyp<uint16_t>(q, q_sb, k, k_ss, k_sb, bias_k, mask, finished, B, per_image, H, S, D, vec, scratch, stream);
    else
      launch_probs_hyp<float>(q, q_sb, k, k_ss, k_sb, bias_k, mask, finished, B, per_image, H, S, D, vec, scratch, stream);
  }
  hipLaunchKernelGGL(copy_finish_kernel, dim3(B * per_image), dim3(NT), 0, stream, (const float*)scratch, proper, ctx_ids,
                     entity_logits, gen_tok, finished, hist, ld_hist, copied, ld_copied, prob, ld_prob, L, step, step_dev, H, S,
                     per_image, tok);
  return tell_check_launch("copy_decide_hyp");
}
