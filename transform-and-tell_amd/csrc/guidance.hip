// Context guidance: the pick of a decode step whose batch holds every caption twice - conditional row r
// and, pair_offset rows further down the same logit buffers, its partner decoded with some contexts dropped.
//
//   lp_c(v), lp_u(v)   the full adaptive-softmax log-probs of the two rows, with the arithmetic of the plain pick kernels
//                      (adaptive.hip: logit - lse_head; a tail token adds head_lsm[c0 + i] - lse_tail)
//   d = lp_c - lp_u;  t = (gamma - 1) * d;  s = lp_c + t        three fp32 operations rounded one by one, never an FMA
//   L = log sum_v exp(s(v))  (max-shifted);  g = s - L
//
// Candidates are ranked by s (value descending, lower id first on ties) and reported as g; both rows of a pair receive the
// same k candidates.  gamma = 1 or u == c makes t a zero, so s is lp_c bit for bit and the tokens are those of
// tell_adaptive_logprob_topk: each form below reduces a row in the order of its plain counterpart (register form:
// logprob_regs_kernel, streaming form: logprob_topk_body), and reduces u with the very code that reduces c.
// gamma is read from device memory: a captured step serves every gamma.
#include "common.h"
#include "options.h"
#include "logits_args.h"

namespace {

struct GuideArgs {
  const float* head; long ld_head; int head_n;        // head_n = c0 + n_tails
  const float* tail[3]; long ld_tail[3]; int tail_n[3];
  int n_tails, c0, rows, k;
  long pair_offset;
  const float* gamma;
  float* s_rows; long ld_s;                            // optional fp32 [rows, vocab]
  int* tokens; float* lps;                             // [rows + pair_offset.., k]
};

typedef float f4 __attribute__((ext_vector_type(4)));
__device__ constexpr int G_CAP[4] = {2, 4, 8, 2};      // float4 per thread and segment: the capacity of logprob_regs_kernel
__device__ constexpr int G_OFF[4] = {0, 2, 6, 14};
// (so the launcher asks logits_regs() of logits_args.h, the plain launchers' own predicate, whether a row fits)
static_assert(LOGITS_REGS_CAP[0] == G_CAP[0] * 1024 * 4 && LOGITS_REGS_CAP[1] == G_CAP[1] * 1024 * 4 &&
              LOGITS_REGS_CAP[2] == G_CAP[2] * 1024 * 4 && LOGITS_REGS_CAP[3] == G_CAP[3] * 1024 * 4,
              "LOGITS_REGS_CAP (logits_args.h) must follow G_CAP");
__device__ constexpr int G_SEG[16] = {0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3};   // the segment of register chunk c

// The thread index as a value the compiler knows nothing about: every phase of the register form derives its element
// indices and bounds tests from its own copy, so the tests of one phase are not kept alive (64 lane masks) for the next.
__device__ __forceinline__ int opaque_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t & 1023;                                     // (the range keeps the loads in base + 32-bit offset form)
}

__device__ __forceinline__ bool better(float v, int j, float w, int m) { return v > w || (v == w && j < m); }

// s of one element from the two log-probs (the three roundings of the definition)
__device__ __forceinline__ float guided_s(float lpc, float lpu, float gm1) {
#pragma clang fp contract(off)
  const float d = lpc - lpu;
  const float t = gm1 * d;
  return lpc + t;
}

template <int K>
struct Best {
  float tv[K]; int ti[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int q = 0; q < K; ++q) { tv[q] = -INFINITY; ti[q] = 0x7fffffff; }
  }
  __device__ __forceinline__ void consider(float v, int j) {
    if (!better(v, j, tv[K - 1], ti[K - 1])) return;
    tv[K - 1] = v; ti[K - 1] = j;
#pragma unroll
    for (int q = K - 1; q > 0; --q)
      if (better(tv[q], ti[q], tv[q - 1], ti[q - 1])) {
        const float fv = tv[q]; tv[q] = tv[q - 1]; tv[q - 1] = fv;
        const int fi = ti[q]; ti[q] = ti[q - 1]; ti[q - 1] = fi;
      }
  }
  __device__ __forceinline__ void advance() {
#pragma unroll
    for (int q = 0; q < K - 1; ++q) { tv[q] = tv[q + 1]; ti[q] = ti[q + 1]; }
    tv[K - 1] = -INFINITY; ti[K - 1] = 0x7fffffff;
  }
};

// pop the block-wide best k times (lowest index wins ties); entry r of both rows of the pair = (token, s - L)
template <int K, int WAVES>
__device__ __forceinline__ void pop_pair(Best<K>& b, const GuideArgs& p, int i, float L, float* best_v, int* best_i, int* win_i) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = 0; r < p.k; ++r) {
    float bv = b.tv[0]; int bi = b.ti[0];
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();                                   // previous round's win_i / best_* consumed
    if (lane == 0) { best_v[wave] = bv; best_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < WAVES; ++w)
        if (better(best_v[w], best_i[w], bv, bi)) { bv = best_v[w]; bi = best_i[w]; }
      const float g = bv - L;
      const long a = (long)i * p.k + r, c = ((long)i + p.pair_offset) * p.k + r;
      p.tokens[a] = bi; p.lps[a] = g;
      p.tokens[c] = bi; p.lps[c] = g;
      *win_i = bi;
    }
    __syncthreads();
    if (b.ti[0] == *win_i) b.advance();                // the owner of the winner advances its list
  }
}

// ------------------------------------------------------------------ register form
// One 1024-thread workgroup per pair, 64 registers of row per thread - two rows do not fit, so: (1) u into the registers,
// its four log-sum-exps reduced, (2) c into the registers, its four reduced by the same code, (3) u read again (from L2)
// element by element while the registers are overwritten with s, (4) max, sum-exp and the k-best pop over the registers.
__device__ __forceinline__ void load_row(f4 (&x)[16], const float* const (&rowp)[4], const int (&n)[4]) {
  const int tid = opaque_tid();
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int q = 0; q < G_CAP[s]; ++q) {
      const int j = (q * 1024 + tid) * 4;
      // (the launcher takes this form only where a row can be read in whole float4: ld >= n rounded up to 4)
      f4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (j < n[s]) v = *reinterpret_cast<const f4*>(rowp[s] + j);
      v.y = j + 1 < n[s] ? v.y : -INFINITY;
      v.z = j + 2 < n[s] ? v.z : -INFINITY;
      v.w = j + 3 < n[s] ? v.w : -INFINITY;
      x[G_OFF[s] + q] = v;
    }
}
// the four (max, sum-exp) of the row in registers, in the order of logprob_regs_kernel -> lse of the head, and per tail the
// offset its logits take: (head[c0 + s - 1] - lse_head) - lse_tail
__device__ __forceinline__ void reduce_row(const f4 (&x)[16], const float* hrow, int c0, int nseg, float (*red)[16],
                                           float& lse_h, float (&off)[3]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float mx[4], sm[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < G_CAP[s]; ++q) {
      const f4 v = x[G_OFF[s] + q];
      m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    m = wave_max(m);
    if (lane == 0) red[s][wave] = m;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float m = red[s][0];
#pragma unroll
    for (int w = 1; w < 16; ++w) m = fmaxf(m, red[s][w]);
    mx[s] = m;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float t = 0.f;
    if (s < nseg) {
#pragma unroll
      for (int q = 0; q < G_CAP[s]; ++q) {
        const f4 v = x[G_OFF[s] + q];
        t += (__expf(v.x - mx[s]) + __expf(v.y - mx[s])) + (__expf(v.z - mx[s]) + __expf(v.w - mx[s]));
      }
    }
    t = wave_sum(t);
    if (lane == 0) red[s][wave] = t;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[s][w];
    sm[s] = t;
  }
  __syncthreads();                                     // red is written again by the next reduction
  lse_h = mx[0] + __logf(sm[0]);
#pragma unroll
  for (int s = 1; s < 4; ++s)
    off[s - 1] = s < nseg ? (hrow[c0 + s - 1] - lse_h) - (mx[s] + __logf(sm[s])) : 0.f;
}

template <int K>
__global__ __launch_bounds__(1024) void guided_regs_kernel(GuideArgs p) {
  __shared__ float red[4][16];
  __shared__ float best_v[16];
  __shared__ int best_i[16];
  __shared__ int win_i;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nseg = 1 + p.n_tails;
  const long iu = (long)i + p.pair_offset;
  const float* rc[4]; const float* ru[4]; int n[4];
  rc[0] = p.head + (long)i * p.ld_head; ru[0] = p.head + iu * p.ld_head; n[0] = p.head_n;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    rc[c + 1] = c < p.n_tails ? p.tail[c] + (long)i * p.ld_tail[c] : rc[0];
    ru[c + 1] = c < p.n_tails ? p.tail[c] + iu * p.ld_tail[c] : ru[0];
    n[c + 1] = c < p.n_tails ? p.tail_n[c] : 0;
  }
  const float gm1 = *p.gamma - 1.f;
  f4 x[16];
  float lse_u, off_u[3], lse_c, off_c[3];
  load_row(x, ru, n);
  reduce_row(x, ru[0], p.c0, nseg, red, lse_u, off_u);
  __builtin_amdgcn_sched_barrier(0);                   // (c's loads stay behind u's reduction: one row in registers at a time)
  load_row(x, rc, n);
  reduce_row(x, rc[0], p.c0, nseg, red, lse_c, off_c);
  __builtin_amdgcn_sched_barrier(0);
  // registers <- s; everything outside the vocabulary (the head's cluster logits, a segment's padding) <- -inf.  The 16
  // float4 of u are requested two chunks ahead of their use and no further (scheduling barriers): all sixteen in flight
  // beside the sixteen of c is what does not fit.
  float* srow = p.s_rows ? p.s_rows + (long)i * p.ld_s : nullptr;
  int sbase[4];
  sbase[0] = 0; sbase[1] = p.c0;
#pragma unroll
  for (int s = 2; s < 4; ++s) sbase[s] = sbase[s - 1] + n[s - 1];
  const int tid_u = opaque_tid(), tid_s = opaque_tid();
  auto load_u = [&](int c) {
    const int s = G_SEG[c], j = ((c - G_OFF[s]) * 1024 + tid_u) * 4;
    f4 u = {0.f, 0.f, 0.f, 0.f};
    if (j < n[s]) u = *reinterpret_cast<const f4*>(ru[s] + j);   // (elements behind the segment's end are never used)
    return u;
  };
  float m = -INFINITY;
  f4 ua = load_u(0), ub = load_u(1);
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const int s = G_SEG[c], j = ((c - G_OFF[s]) * 1024 + tid_s) * 4;
    const f4 u = ua;
    ua = ub;
    if (c + 2 < 16) ub = load_u(c + 2);
    // (head: logit - lse, the plain kernels' subtraction; a tail: logit + offset, their addition)
    const float ac = s == 0 ? -lse_c : off_c[s > 0 ? s - 1 : 0];
    const float au = s == 0 ? -lse_u : off_u[s > 0 ? s - 1 : 0];
    f4 v = x[c];
    // (load_row left -inf in every register element behind its segment's end; the head's cluster logits go by index)
    const bool ok0 = s == 0 ? j < p.c0 : v.x > -INFINITY, ok1 = s == 0 ? j + 1 < p.c0 : v.y > -INFINITY;
    const bool ok2 = s == 0 ? j + 2 < p.c0 : v.z > -INFINITY, ok3 = s == 0 ? j + 3 < p.c0 : v.w > -INFINITY;
    v.x = ok0 ? guided_s(s == 0 ? v.x - lse_c : v.x + ac, s == 0 ? u.x - lse_u : u.x + au, gm1) : -INFINITY;
    v.y = ok1 ? guided_s(s == 0 ? v.y - lse_c : v.y + ac, s == 0 ? u.y - lse_u : u.y + au, gm1) : -INFINITY;
    v.z = ok2 ? guided_s(s == 0 ? v.z - lse_c : v.z + ac, s == 0 ? u.z - lse_u : u.z + au, gm1) : -INFINITY;
    v.w = ok3 ? guided_s(s == 0 ? v.w - lse_c : v.w + ac, s == 0 ? u.w - lse_u : u.w + au, gm1) : -INFINITY;
    x[c] = v;
    m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    if (srow) {
      if (ok0) srow[sbase[s] + j] = v.x;
      if (ok1) srow[sbase[s] + j + 1] = v.y;
      if (ok2) srow[sbase[s] + j + 2] = v.z;
      if (ok3) srow[sbase[s] + j + 3] = v.w;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  // L over the whole vocabulary
  m = wave_max(m);
  if (lane == 0) red[0][wave] = m;
  __syncthreads();
  m = red[0][0];
#pragma unroll
  for (int w = 1; w < 16; ++w) m = fmaxf(m, red[0][w]);
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const f4 v = x[q];
    t += (__expf(v.x - m) + __expf(v.y - m)) + (__expf(v.z - m) + __expf(v.w - m));
  }
  t = wave_sum(t);
  if (lane == 0) red[0][wave] = t;
  __syncthreads();
  t = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) t += red[0][w];
  const float L = m + __logf(t);
  // every thread's K best of its registers, then the pop
  Best<K> b;
  b.clear();
  const int tid_k = opaque_tid();
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const int s = G_SEG[c], j = ((c - G_OFF[s]) * 1024 + tid_k) * 4;
    const f4 v = x[c];
    // (an element outside the vocabulary holds -inf and never enters a list: a row has more than k finite scores)
    if (v.x > -INFINITY) b.consider(v.x, sbase[s] + j);
    if (v.y > -INFINITY) b.consider(v.y, sbase[s] + j + 1);
    if (v.z > -INFINITY) b.consider(v.z, sbase[s] + j + 2);
    if (v.w > -INFINITY) b.consider(v.w, sbase[s] + j + 3);
  }
  pop_pair<K, 16>(b, p, i, L, best_v, best_i, &win_i);
}

// ------------------------------------------------------------------ streaming form
// Any row (unaligned, larger than the register capacity) and option argmax_regs = 0.  256 threads per pair; the rows are read
// from memory in every pass: the log-sum-exps of u and of c in the order of logprob_topk_body, then s -> maximum and every
// thread's k best (and s_rows), then s again -> sum-exp.
struct RowLse { float lse_h; float off[3]; };
__device__ __forceinline__ float blk_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < 4; ++w) r = fmaxf(r, red[w]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ float blk_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int w = 0; w < 4; ++w) r += red[w];
  __syncthreads();
  return r;
}
__device__ __forceinline__ RowLse stream_lse(const GuideArgs& p, long row, float* red) {
  RowLse o;
  const float* hrow = p.head + row * p.ld_head;
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < p.head_n; j += 256) mx = fmaxf(mx, hrow[j]);
  mx = blk_max(mx, red);
  float s = 0.f;
  for (int j = threadIdx.x; j < p.head_n; j += 256) s += __expf(hrow[j] - mx);
  s = blk_sum(s, red);
  o.lse_h = mx + __logf(s);
  for (int c = 0; c < 3; ++c) {
    o.off[c] = 0.f;
    if (c < p.n_tails) {
      const float* trow = p.tail[c] + row * p.ld_tail[c];
      const int n = p.tail_n[c];
      float m2 = -INFINITY;
      for (int j = threadIdx.x; j < n; j += 256) m2 = fmaxf(m2, trow[j]);
      m2 = blk_max(m2, red);
      float s2 = 0.f;
      for (int j = threadIdx.x; j < n; j += 256) s2 += __expf(trow[j] - m2);
      s2 = blk_sum(s2, red);
      o.off[c] = (hrow[p.c0 + c] - o.lse_h) - (m2 + __logf(s2));
    }
  }
  return o;
}

template <int K>
__global__ __launch_bounds__(256) void guided_stream_kernel(GuideArgs p) {
  __shared__ float red[4];
  __shared__ float best_v[4];
  __shared__ int best_i[4];
  __shared__ int win_i;
  const int i = blockIdx.x;
  const long iu = (long)i + p.pair_offset;
  const float gm1 = *p.gamma - 1.f;
  const RowLse lu = stream_lse(p, iu, red);
  const RowLse lc = stream_lse(p, (long)i, red);
  float* srow = p.s_rows ? p.s_rows + (long)i * p.ld_s : nullptr;
  Best<K> b;
  b.clear();
  float m = -INFINITY;
  {
    const float* hc = p.head + (long)i * p.ld_head;
    const float* hu = p.head + iu * p.ld_head;
    for (int j = threadIdx.x; j < p.c0; j += 256) {
      const float s = guided_s(hc[j] - lc.lse_h, hu[j] - lu.lse_h, gm1);
      if (srow) srow[j] = s;
      m = fmaxf(m, s);
      b.consider(s, j);
    }
    int base = p.c0;
    for (int c = 0; c < p.n_tails; ++c) {
      const float* tc = p.tail[c] + (long)i * p.ld_tail[c];
      const float* tu = p.tail[c] + iu * p.ld_tail[c];
      const int n = p.tail_n[c];
      for (int j = threadIdx.x; j < n; j += 256) {
        const float s = guided_s(tc[j] + lc.off[c], tu[j] + lu.off[c], gm1);
        if (srow) srow[base + j] = s;
        m = fmaxf(m, s);
        b.consider(s, base + j);
      }
      base += n;
    }
  }
  m = blk_max(m, red);
  float t = 0.f;
  {
    const float* hc = p.head + (long)i * p.ld_head;
    const float* hu = p.head + iu * p.ld_head;
    for (int j = threadIdx.x; j < p.c0; j += 256) t += __expf(guided_s(hc[j] - lc.lse_h, hu[j] - lu.lse_h, gm1) - m);
    for (int c = 0; c < p.n_tails; ++c) {
      const float* tc = p.tail[c] + (long)i * p.ld_tail[c];
      const float* tu = p.tail[c] + iu * p.ld_tail[c];
      const int n = p.tail_n[c];
      for (int j = threadIdx.x; j < n; j += 256) t += __expf(guided_s(tc[j] + lc.off[c], tu[j] + lu.off[c], gm1) - m);
    }
  }
  t = blk_sum(t, red);
  const float L = m + __logf(t);
  pop_pair<K, 4>(b, p, i, L, best_v, best_i, &win_i);
}

}  // namespace

extern "C" int tell_adaptive_logprob_topk_guided(const float* head, long ld_head, int c0, int n_tails, const float* tail0,
                                                 long ld0, int n0, const float* tail1, long ld1, int n1, const float* tail2,
                                                 long ld2, int n2, int rows, long pair_offset, int k, const float* gamma_dev,
                                                 float* s_rows, long ld_s, int* tokens, float* lps, hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_topk_guided: up to 3 tails");
  TELL_REQUIRE(k >= 1 && k <= 8, "logprob_topk_guided: 1 <= k <= 8");
  TELL_REQUIRE(head && tokens && lps && gamma_dev, "logprob_topk_guided: head, gamma_dev, tokens and lps [rows + pair_offset, k]");
  TELL_REQUIRE(pair_offset >= rows && pair_offset >= 1, "logprob_topk_guided: pair_offset >= rows (the partners lie behind the conditional rows)");
  TELL_REQUIRE(c0 >= 1 && (n_tails < 1 || (tail0 && n0 >= 1)) && (n_tails < 2 || (tail1 && n1 >= 1)) &&
               (n_tails < 3 || (tail2 && n2 >= 1)), "logprob_topk_guided: c0 >= 1 and every tail non-empty");
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  TELL_REQUIRE(!s_rows || ld_s >= logits_vocab(lg), "logprob_topk_guided: s_rows fp32 [rows, ld_s >= vocab]");
  if (rows <= 0) return TELL_OK;
  GuideArgs p;
  p.head = head; p.ld_head = ld_head; p.head_n = c0 + n_tails; p.c0 = c0; p.n_tails = n_tails; p.rows = rows; p.k = k;
  for (int i = 0; i < 3; ++i) { p.tail[i] = lg.tail[i]; p.ld_tail[i] = lg.ld[i]; p.tail_n[i] = lg.n[i]; }
  p.pair_offset = pair_offset; p.gamma = gamma_dev; p.s_rows = s_rows; p.ld_s = ld_s; p.tokens = tokens; p.lps = lps;
  // (the register form reads whole float4 of a row: the last one may reach into the row's padding)
  bool whole = ld_head >= ((p.head_n + 3) & ~3);
  for (int i = 0; i < n_tails; ++i) whole = whole && lg.ld[i] >= ((lg.n[i] + 3) & ~3);
  if (logits_regs(lg) && whole) {
    if (k == 1) hipLaunchKernelGGL((guided_regs_kernel<1>), dim3(rows), dim3(1024), 0, stream, p);
    else if (k <= 4) hipLaunchKernelGGL((guided_regs_kernel<4>), dim3(rows), dim3(1024), 0, stream, p);
    else hipLaunchKernelGGL((guided_regs_kernel<8>), dim3(rows), dim3(1024), 0, stream, p);
    return tell_check_launch("logprob_topk_guided (registers)");
  }
  if (k == 1) hipLaunchKernelGGL((guided_stream_kernel<1>), dim3(rows), dim3(256), 0, stream, p);
  else if (k <= 4) hipLaunchKernelGGL((guided_stream_kernel<4>), dim3(rows), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((guided_stream_kernel<8>), dim3(rows), dim3(256), 0, stream, p);
  return tell_check_launch("logprob_topk_guided");
}
