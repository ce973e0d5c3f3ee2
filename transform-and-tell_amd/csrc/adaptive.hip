// Adaptive input embedding + adaptive softmax helpers with STATIC shapes
// (tell/modules/token_embedders/adaptive.py:61-76, tell/modules/softmax.py:144-222,
//  tell/modules/criteria/adaptive_loss.py:27-73).
//
// The reference uses boolean masks / nonzero() / index_select with host syncs.
// Here a single-workgroup partition kernel builds, on the device, ascending
// compacted row lists per vocabulary band; the band GEMMs then run over a
// fixed-capacity buffer with a device-side row count (gemm_nt's m_dev), so the
// whole step has no data-dependent launch and no host synchronisation.
#include "common.h"
#include "options.h"
#include "logits_args.h"

#define MAX_BANDS 4

struct PartitionArgs {
  const long* ids;      // [N] int64 token ids
  int N, n_bands;
  int cut[MAX_BANDS];   // upper bounds: band b = [cut[b-1], cut[b])
  int pad_idx;          // ids == pad_idx are not counted in n_valid
  int* band_rows;       // [n_bands][N]  ascending row indices of each band
  int* band_local;      // [n_bands][N]  id - band_lo of those rows
  int* band_count;      // [n_bands]
  int* slot;            // [N]  b*N + position of the row inside its band list
  int* head_target;     // [N]  id (band 0) or cut[0] + b - 1 (softmax.py:158)
  int* n_valid;         // [1]  number of ids != pad_idx (adaptive_loss.py:62-65)
};

__global__ __launch_bounds__(1024) void partition_kernel(PartitionArgs p) {
  __shared__ int wave_tot[16];
  __shared__ int base_s;
  __shared__ int valid_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) valid_s = 0;
  for (int b = 0; b < p.n_bands; ++b) {
    const int lo = b == 0 ? 0 : p.cut[b - 1], hi = p.cut[b];
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int start = 0; start < p.N; start += 1024) {
      const int i = start + tid;
      long id = i < p.N ? p.ids[i] : -1;
      const bool flag = i < p.N && id >= lo && id < hi;
      const unsigned long long bal = __ballot(flag);
      const int wpre = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wave_tot[wave] = __popcll(bal);
      __syncthreads();
      int off = base_s, tot = 0;
      for (int w = 0; w < 16; ++w) { if (w < wave) off += wave_tot[w]; tot += wave_tot[w]; }
      if (flag) {
        const int j = off + wpre;
        p.band_rows[(long)b * p.N + j] = i;
        p.band_local[(long)b * p.N + j] = (int)(id - lo);
        if (p.slot) p.slot[i] = b * p.N + j;
        if (p.head_target) p.head_target[i] = b == 0 ? (int)id : p.cut[0] + b - 1;
      }
      if (b == 0 && p.n_valid) {
        const unsigned long long vb = __ballot(i < p.N && id != p.pad_idx);
        if (lane == 0) atomicAdd(&valid_s, __popcll(vb));
      }
      __syncthreads();
      if (tid == 0) base_s += tot;
      __syncthreads();
    }
    if (tid == 0) p.band_count[b] = base_s;
  }
  __syncthreads();
  if (tid == 0 && p.n_valid) *p.n_valid = valid_s;
}

extern "C" int tell_adaptive_partition(const long* ids, int N, const int* cutoffs, int n_bands, int pad_idx,
                                       int* band_rows, int* band_local, int* band_count, int* slot,
                                       int* head_target, int* n_valid, hipStream_t stream) {
  TELL_REQUIRE(n_bands >= 1 && n_bands <= MAX_BANDS, "partition: 1..4 bands");
  if (N <= 0) return TELL_OK;
  PartitionArgs p;
  p.ids = ids; p.N = N; p.n_bands = n_bands; p.pad_idx = pad_idx;
  for (int b = 0; b < MAX_BANDS; ++b) p.cut[b] = b < n_bands ? cutoffs[b] : 0;
  p.band_rows = band_rows; p.band_local = band_local; p.band_count = band_count; p.slot = slot;
  p.head_target = head_target; p.n_valid = n_valid;
  hipLaunchKernelGGL(partition_kernel, dim3(1), dim3(1024), 0, stream, p);
  return tell_check_launch("adaptive_partition");
}

// ------------------------------------------------------------------ embedding finalize
// out[row(n)] = scale * band_out[slot[n]] + pos_table[position(n)]
//   position (positional.py:231-268, right padding): pad -> pad_idx, else pad_idx + 1 + t + start_pos
//   row(n): n = b*T + t  ->  t*B + b when `tbc` (decoder layout) else n
template <typename T>
__global__ __launch_bounds__(256) void embed_finalize_kernel(const T* __restrict__ band_out,
                                                             const int* __restrict__ slot,
                                                             const long* __restrict__ ids,
                                                             const float* __restrict__ pos_table,
                                                             int pos_rows, T* __restrict__ out, int Bn,
                                                             int Tn, int E, float scale, int pos_pad,
                                                             int start_pos, int tbc,
                                                             const uint32_t* __restrict__ step) {
  // inside a captured decode step the position offset advances with the graph's device counter (common.h)
  if (step) start_pos += (int)*step;
  const int n = blockIdx.x;
  const int b = n / Tn, t = n % Tn;
  const long id = ids[n];
  int pos = id == pos_pad ? pos_pad : pos_pad + 1 + t + start_pos;
  if (pos >= pos_rows) pos = pos_rows - 1;       // host guarantees the table is large enough
  const T* src = band_out + (long)slot[n] * E;
  const float* pr = pos_table + (long)pos * E;
  T* dst = out + (long)(tbc ? t * Bn + b : n) * E;
  for (int c = threadIdx.x; c < E; c += 256) Elem<T>::st(dst + c, scale * Elem<T>::ld(src + c) + pr[c]);
}
extern "C" int tell_embed_finalize(const void* band_out, const int* slot, const long* ids,
                                   const float* pos_table, int pos_rows, void* out, int B, int T, int E,
                                   float scale, int pos_pad, int start_pos, int tbc, int dtype,
                                   hipStream_t stream) {
  if (B * T <= 0) return TELL_OK;
  if (dtype == TELL_BF16) hipLaunchKernelGGL((embed_finalize_kernel<uint16_t>), dim3(B * T), dim3(256), 0, stream, (const uint16_t*)band_out, slot, ids, pos_table, pos_rows, (uint16_t*)out, B, T, E, scale, pos_pad, start_pos, tbc, g_tell_pos_step);
  else hipLaunchKernelGGL((embed_finalize_kernel<float>), dim3(B * T), dim3(256), 0, stream, (const float*)band_out, slot, ids, pos_table, pos_rows, (float*)out, B, T, E, scale, pos_pad, start_pos, tbc, g_tell_pos_step);
  return tell_check_launch("embed_finalize");
}

// backward of finalize: dband[slot[n]] = scale * dout[row(n)]
template <typename T>
__global__ __launch_bounds__(256) void embed_finalize_bwd_kernel(const T* __restrict__ dout,
                                                                 const int* __restrict__ slot,
                                                                 T* __restrict__ dband, int Bn, int Tn,
                                                                 int E, float scale, int tbc) {
  const int n = blockIdx.x;
  const int b = n / Tn, t = n % Tn;
  const T* src = dout + (long)(tbc ? t * Bn + b : n) * E;
  T* dst = dband + (long)slot[n] * E;
  for (int c = threadIdx.x; c < E; c += 256) Elem<T>::st(dst + c, scale * Elem<T>::ld(src + c));
}
extern "C" int tell_embed_finalize_bwd(const void* dout, const int* slot, void* dband, int B, int T, int E,
                                       float scale, int tbc, int dtype, hipStream_t stream) {
  if (B * T <= 0) return TELL_OK;
  if (dtype == TELL_BF16) hipLaunchKernelGGL((embed_finalize_bwd_kernel<uint16_t>), dim3(B * T), dim3(256), 0, stream, (const uint16_t*)dout, slot, (uint16_t*)dband, B, T, E, scale, tbc);
  else hipLaunchKernelGGL((embed_finalize_bwd_kernel<float>), dim3(B * T), dim3(256), 0, stream, (const float*)dout, slot, (float*)dband, B, T, E, scale, tbc);
  return tell_check_launch("embed_finalize_bwd");
}

// gradient of the band table: demb[local[j]] += drows[j]; local row `padding_idx` receives nothing
// (nn.Embedding(padding_idx), adaptive.py:42).
// Round 6: DETERMINISTIC - a segmented sum by table row instead of fp32 atomics.  (With atomics the order in which the
// duplicates of a token met in a table row depended on workgroup scheduling: two otherwise identical trainers differed by
// 1-3e-6 of the loss after a few steps, and a test tolerance had to follow.)  The workgroup of the FIRST band row that
// names a table row is that row's only writer: it lists the later band rows with the same id in increasing order (a block
// scan over 1024 candidates at a time), adds them up in that order and adds the sum to the gradient row once.
template <typename T>
__global__ __launch_bounds__(256) void embed_table_grad_kernel(const T* __restrict__ drows, long ld,
                                                               const int* __restrict__ local,
                                                               const int* __restrict__ count_dev, int cap,
                                                               float* __restrict__ demb, int dim,
                                                               int padding_idx) {
  __shared__ int s_wave[4];
  __shared__ int s_list[1024];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = *count_dev;
  if (n > cap) n = cap;
  for (int j = blockIdx.x; j < n; j += gridDim.x) {
    const int row = local[j];
    if (row == padding_idx) continue;                          // (uniform)
    int dup = 0;
    for (int i = tid; i < j; i += 256) dup |= (local[i] == row) ? 1 : 0;
    if (__syncthreads_or(dup)) continue;                       // an earlier band row owns this table row (uniform)
    for (int c0 = 0; c0 < dim; c0 += 1024) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int base = j; base < n; base += 1024) {
        // ordered list of the band rows base .. base + 1023 that name `row`: thread t owns candidates 4t .. 4t + 3
        int hit[4], cnt = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = base + tid * 4 + e;
          hit[e] = (i < n && local[i] == row) ? 1 : 0;
          cnt += hit[e];
        }
        int incl = cnt;                                        // inclusive scan over the wave, then over the 4 waves
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int v = __shfl_up(incl, o, 64);
          if (lane >= o) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int off = incl - cnt;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (hit[e]) s_list[off++] = base + tid * 4 + e;
        __syncthreads();
        for (int m = 0; m < total; ++m) {
          const T* src = drows + (long)s_list[m] * ld + c0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = tid + q * 256;
            if (c0 + c < dim) acc[q] += Elem<T>::ld(src + c);
          }
        }
        __syncthreads();                                       // (s_list / s_wave are rewritten by the next chunk)
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + tid + q * 256;
        if (c < dim) demb[(long)row * dim + c] += acc[q];
      }
    }
  }
}
extern "C" int tell_embed_table_grad(const void* drows, long ld, const int* local, const int* count_dev,
                                     int cap, float* demb, int dim, int padding_idx, int dtype,
                                     hipStream_t stream) {
  if (cap <= 0) return TELL_OK;
  int g = cap < 1024 ? cap : 1024;
  if (dtype == TELL_BF16) hipLaunchKernelGGL((embed_table_grad_kernel<uint16_t>), dim3(g), dim3(256), 0, stream, (const uint16_t*)drows, ld, local, count_dev, cap, demb, dim, padding_idx);
  else hipLaunchKernelGGL((embed_table_grad_kernel<float>), dim3(g), dim3(256), 0, stream, (const float*)drows, ld, local, count_dev, cap, demb, dim, padding_idx);
  return tell_check_launch("embed_table_grad");
}

// ------------------------------------------------------------------ cross entropy over one cluster
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = fmaxf(r, red[w]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += red[w];
  __syncthreads();
  return r;
}

// per row i (< *m_dev): lse[i] = logsumexp(logits[i,:]); loss[i] = lse - logits[i,tgt] unless tgt == ignore
// target of compacted row i is targets[row_idx ? row_idx[i] : i]
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ logits, long ld, int M, int V,
                                                     const int* __restrict__ targets,
                                                     const int* __restrict__ row_idx,
                                                     const int* __restrict__ m_dev, int ignore_index,
                                                     float* __restrict__ lse, float* __restrict__ loss) {
  __shared__ float red[4];
  int Me = M;
  if (m_dev) { int md = *m_dev; Me = md < M ? md : M; }
  const int i = blockIdx.x;
  if (i >= Me) { if (threadIdx.x == 0) { loss[i] = 0.f; lse[i] = 0.f; } return; }
  const float* row = logits + (long)i * ld;
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < V; j += 256) mx = fmaxf(mx, row[j]);
  mx = block_max(mx, red);
  float s = 0.f;
  for (int j = threadIdx.x; j < V; j += 256) s += __expf(row[j] - mx);
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const float l = mx + __logf(s);
    const int tg = targets[row_idx ? row_idx[i] : i];
    lse[i] = l;
    loss[i] = tg == ignore_index ? 0.f : l - row[tg];
  }
}
// dlogits[i,j] = (softmax - onehot) * g,  g = *gscale (device scalar), 0 for ignored rows
template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, long ld, int M, int V,
                                                     const int* __restrict__ targets,
                                                     const int* __restrict__ row_idx,
                                                     const int* __restrict__ m_dev, int ignore_index,
                                                     const float* __restrict__ lse,
                                                     const float* __restrict__ gscale, T* __restrict__ dlogits,
                                                     long ld_d) {
  int Me = M;
  if (m_dev) { int md = *m_dev; Me = md < M ? md : M; }
  const int i = blockIdx.x;
  if (i >= Me) return;
  const int tg = targets[row_idx ? row_idx[i] : i];
  const float g = tg == ignore_index ? 0.f : *gscale;
  const float l = lse[i];
  const float* row = logits + (long)i * ld;
  T* d = dlogits + (long)i * ld_d;
  for (int j = threadIdx.x; j < V; j += 256)
    Elem<T>::st(d + j, (__expf(row[j] - l) - (j == tg ? 1.f : 0.f)) * g);
}
extern "C" int tell_ce_fwd(const float* logits, long ld, int M, int V, const int* targets, const int* row_idx,
                           const int* m_dev, int ignore_index, float* lse, float* loss, hipStream_t stream) {
  if (M <= 0) return TELL_OK;
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(M), dim3(256), 0, stream, logits, ld, M, V, targets, row_idx, m_dev, ignore_index, lse, loss);
  return tell_check_launch("ce_fwd");
}
extern "C" int tell_ce_bwd(const float* logits, long ld, int M, int V, const int* targets, const int* row_idx,
                           const int* m_dev, int ignore_index, const float* lse, const float* gscale,
                           void* dlogits, long ld_d, int dtype, hipStream_t stream) {
  if (M <= 0) return TELL_OK;
  if (dtype == TELL_BF16) hipLaunchKernelGGL((ce_bwd_kernel<uint16_t>), dim3(M), dim3(256), 0, stream, logits, ld, M, V, targets, row_idx, m_dev, ignore_index, lse, gscale, (uint16_t*)dlogits, ld_d);
  else hipLaunchKernelGGL((ce_bwd_kernel<float>), dim3(M), dim3(256), 0, stream, logits, ld, M, V, targets, row_idx, m_dev, ignore_index, lse, gscale, (float*)dlogits, ld_d);
  return tell_check_launch("ce_bwd");
}

// ---- per-row weights (tell_ce_fwd_weighted / tell_ce_bwd_weighted, include/tell_hip.h): the weight of compacted row i is
// w[w_idx ? w_idx[i] : i].  The reductions are those of ce_fwd_kernel statement for statement, so lse keeps its bits and
// loss is one fp32 multiply away; backward forms *gscale * weight once per row and then is ce_bwd_kernel's loop.
__global__ __launch_bounds__(256) void ce_fwd_weighted_kernel(const float* __restrict__ logits, long ld, int M, int V,
                                                              const int* __restrict__ targets,
                                                              const int* __restrict__ row_idx,
                                                              const int* __restrict__ m_dev, int ignore_index,
                                                              const float* __restrict__ w,
                                                              const int* __restrict__ w_idx,
                                                              float* __restrict__ lse, float* __restrict__ loss) {
  __shared__ float red[4];
  int Me = M;
  if (m_dev) { int md = *m_dev; Me = md < M ? md : M; }
  const int i = blockIdx.x;
  if (i >= Me) { if (threadIdx.x == 0) { loss[i] = 0.f; lse[i] = 0.f; } return; }
  const float* row = logits + (long)i * ld;
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < V; j += 256) mx = fmaxf(mx, row[j]);
  mx = block_max(mx, red);
  float s = 0.f;
  for (int j = threadIdx.x; j < V; j += 256) s += __expf(row[j] - mx);
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const float l = mx + __logf(s);
    const int tg = targets[row_idx ? row_idx[i] : i];
    lse[i] = l;
    if (tg == ignore_index) {
      loss[i] = 0.f;
    } else {
      const float nll = l - row[tg];
      loss[i] = w[w_idx ? w_idx[i] : i] * nll;
    }
  }
}
template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_weighted_kernel(const float* __restrict__ logits, long ld, int M, int V,
                                                              const int* __restrict__ targets,
                                                              const int* __restrict__ row_idx,
                                                              const int* __restrict__ m_dev, int ignore_index,
                                                              const float* __restrict__ w,
                                                              const int* __restrict__ w_idx,
                                                              const float* __restrict__ lse,
                                                              const float* __restrict__ gscale, T* __restrict__ dlogits,
                                                              long ld_d) {
  int Me = M;
  if (m_dev) { int md = *m_dev; Me = md < M ? md : M; }
  const int i = blockIdx.x;
  if (i >= Me) return;
  const int tg = targets[row_idx ? row_idx[i] : i];
  const float g = tg == ignore_index ? 0.f : *gscale * w[w_idx ? w_idx[i] : i];
  const float l = lse[i];
  const float* row = logits + (long)i * ld;
  T* d = dlogits + (long)i * ld_d;
  for (int j = threadIdx.x; j < V; j += 256)
    Elem<T>::st(d + j, (__expf(row[j] - l) - (j == tg ? 1.f : 0.f)) * g);
}
extern "C" int tell_ce_fwd_weighted(const float* logits, long ld, int M, int V, const int* targets, const int* row_idx,
                                    const int* m_dev, int ignore_index, const float* w, const int* w_idx, float* lse,
                                    float* loss, hipStream_t stream) {
  TELL_REQUIRE(w, "ce_fwd_weighted: w fp32 [rows] expected (tell_ce_fwd is the call without weights)");
  if (M <= 0) return TELL_OK;
  hipLaunchKernelGGL(ce_fwd_weighted_kernel, dim3(M), dim3(256), 0, stream, logits, ld, M, V, targets, row_idx, m_dev, ignore_index, w, w_idx, lse, loss);
  return tell_check_launch("ce_fwd_weighted");
}
extern "C" int tell_ce_bwd_weighted(const float* logits, long ld, int M, int V, const int* targets, const int* row_idx,
                                    const int* m_dev, int ignore_index, const float* w, const int* w_idx,
                                    const float* lse, const float* gscale, void* dlogits, long ld_d, int dtype,
                                    hipStream_t stream) {
  TELL_REQUIRE(w, "ce_bwd_weighted: w fp32 [rows] expected (tell_ce_bwd is the call without weights)");
  if (M <= 0) return TELL_OK;
  if (dtype == TELL_BF16) hipLaunchKernelGGL((ce_bwd_weighted_kernel<uint16_t>), dim3(M), dim3(256), 0, stream, logits, ld, M, V, targets, row_idx, m_dev, ignore_index, w, w_idx, lse, gscale, (uint16_t*)dlogits, ld_d);
  else hipLaunchKernelGGL((ce_bwd_weighted_kernel<float>), dim3(M), dim3(256), 0, stream, logits, ld, M, V, targets, row_idx, m_dev, ignore_index, w, w_idx, lse, gscale, (float*)dlogits, ld_d);
  return tell_check_launch("ce_bwd_weighted");
}

// deterministic sum of n (< = *m_dev if given) floats -> out[0] (+= if accumulate)
__global__ __launch_bounds__(1024) void sum_kernel(const float* __restrict__ x, int n,
                                                   const int* __restrict__ m_dev, float* __restrict__ out,
                                                   int accumulate) {
  __shared__ float red[16];
  if (m_dev) { int md = *m_dev; n = md < n ? md : n; }
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) s += x[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += red[w];
    out[0] = accumulate ? out[0] + t : t;
  }
}
extern "C" int tell_sum_f32(const float* x, int n, const int* m_dev, float* out, int accumulate,
                            hipStream_t stream) {
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(1024), 0, stream, x, n, m_dev, out, accumulate);
  return tell_check_launch("sum_f32");
}

// ------------------------------------------------------------------ generation head (softmax.py:193-222 + topk(1))
// One workgroup per row: log-softmax of the head and of every tail, combined
// log-probs  lp(w) = head_lsm[w]  (w < c0)   |   tail_lsm_i[w - cut_i] + head_lsm[c0 + i];
// writes argmax token + its log-prob and, optionally, the full log-prob row.
struct LogProbArgs {
  const float* head; long ld_head; int head_n;    // head_n = c0 + n_tails
  const float* tail[3]; long ld_tail[3]; int tail_n[3];
  int n_tails, c0, rows;
  float* log_probs; long ld_lp;                   // optional [rows, vocab]
  int* token; float* token_lp;
};
// (1024 threads per row, 4 loads in flight per thread: with 256 threads and one load at a time the 50 k logits of a row
//  took 87 us of dependent latency - 8 % of a decode step)
__global__ __launch_bounds__(1024) void logprob_argmax_kernel(LogProbArgs p) {
  __shared__ float red[16];
  __shared__ float best_v[16];
  __shared__ int best_i[16];
  const int i = blockIdx.x;
  const float* hrow = p.head + (long)i * p.ld_head;
  float mx = -INFINITY;
#pragma unroll 4
  for (int j = threadIdx.x; j < p.head_n; j += 1024) mx = fmaxf(mx, hrow[j]);
  mx = block_max(mx, red);
  float s = 0.f;
#pragma unroll 4
  for (int j = threadIdx.x; j < p.head_n; j += 1024) s += __expf(hrow[j] - mx);
  s = block_sum(s, red);
  const float lse_h = mx + __logf(s);
  float bv = -INFINITY; int bi = 0x7fffffff;
  float* lp = p.log_probs ? p.log_probs + (long)i * p.ld_lp : nullptr;
#pragma unroll 4
  for (int j = threadIdx.x; j < p.c0; j += 1024) {
    const float v = hrow[j] - lse_h;
    if (lp) lp[j] = v;
    if (v > bv || (v == bv && j < bi)) { bv = v; bi = j; }
  }
  int base = p.c0;
  for (int c = 0; c < p.n_tails; ++c) {
    const float* trow = p.tail[c] + (long)i * p.ld_tail[c];
    const int n = p.tail_n[c];
    float m2 = -INFINITY;
  #pragma unroll 4
  for (int j = threadIdx.x; j < n; j += 1024) m2 = fmaxf(m2, trow[j]);
    m2 = block_max(m2, red);
    float s2 = 0.f;
  #pragma unroll 4
  for (int j = threadIdx.x; j < n; j += 1024) s2 += __expf(trow[j] - m2);
    s2 = block_sum(s2, red);
    const float off = (hrow[p.c0 + c] - lse_h) - (m2 + __logf(s2));
  #pragma unroll 4
  for (int j = threadIdx.x; j < n; j += 1024) {
      const float v = trow[j] + off;
      if (lp) lp[base + j] = v;
      if (v > bv || (v == bv && base + j < bi)) { bv = v; bi = base + j; }
    }
    base += n;
  }
  // block arg-max (lowest index wins ties)
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { best_v[threadIdx.x >> 6] = bv; best_i[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w)
      if (best_v[w] > bv || (best_v[w] == bv && best_i[w] < bi)) { bv = best_v[w]; bi = best_i[w]; }
    if (p.token) p.token[i] = bi;
    if (p.token_lp) p.token_lp[i] = bv;
  }
}
// The same arg-max with every logit of the row in registers: all loads of a row are requested at once (the three-pass
// form above is a chain of ~36 dependent load groups per row: 33 us of a 600 us decode step), the max / sum-exp /
// arg-max passes then run over registers.  Same comparisons as above (v = logit - lse, lowest index wins a tie).
// Capacity (float4 per thread x 1024 threads): head 2 (8192 logits), tails 4 / 8 / 2 (16384 / 32768 / 8192); rows start
// on 16 bytes.  64 of the 128 registers a 1024-thread workgroup leaves each thread.
__device__ constexpr int LPF_CAP[4] = {2, 4, 8, 2};
__device__ constexpr int LPF_OFF[4] = {0, 2, 6, 14};
// (the launchers' side of the capacity, logits_regs() in logits_args.h: LPF_CAP[i] * 1024 threads * 4 floats)
static_assert(LOGITS_REGS_CAP[0] == LPF_CAP[0] * 1024 * 4 && LOGITS_REGS_CAP[1] == LPF_CAP[1] * 1024 * 4 &&
              LOGITS_REGS_CAP[2] == LPF_CAP[2] * 1024 * 4 && LOGITS_REGS_CAP[3] == LPF_CAP[3] * 1024 * 4,
              "LOGITS_REGS_CAP (logits_args.h) must follow LPF_CAP");
// K = 1: arg-max (token, token_lp); K = 4 / 8: every thread keeps its K best while scanning its registers, the block pops
// the global best k times (beam search: tokens / lps [rows, k], best first).
// BAN (tell_adaptive_logprob_topk_banned): the row's ban list (ban[i][0 .. n_ban[i])) becomes a bitmap over the vocabulary
// in LDS; a banned token never enters a thread's candidate list.  The test sits behind consider()'s "beats my K-th best"
// return, which few elements pass, and a row without bans skips the bitmap altogether; maxima, sums and log-probs are
// those of the whole row either way.  BAN = false is the kernel as it was.
struct BanArgs { const int* ban; long ld_ban; const int* n_ban; int vocab; };
extern __shared__ unsigned ban_bits[];
template <int THREADS>
__device__ __forceinline__ void ban_stage(const BanArgs& ba, int row, int nb) {
  const int words = (ba.vocab + 31) >> 5;
  for (int w = threadIdx.x; w < words; w += THREADS) ban_bits[w] = 0u;
  __syncthreads();
  for (int e = threadIdx.x; e < nb; e += THREADS) {
    const int t = ba.ban[(long)row * ba.ld_ban + e];
    if (t >= 0 && t < ba.vocab) atomicOr(&ban_bits[t >> 5], 1u << (t & 31));
  }
  __syncthreads();
}
// PEN (tell_adaptive_logprob_topk_penalised / _sample_penalised, include/tell_hip.h): the row's token list (tok / cnt
// [i][0 .. n_pen[i]): the distinct tokens of its history with their counts, tell_decode_token_counts) becomes the same bitmap
// plus, behind it in LDS, the list itself: the token and sub[count] of up to 256 entries.  A listed token's score is
// s = min(lp, 0) * theta - sub[count], two fp32 operations rounded one by one; s <= lp, so the "beats my K-th best" return on
// the unpenalised value stays valid and only the few elements that pass it test their bit.  n_pen[i] == 0 stages nothing.
struct PenArgs { const int* tok; const int* cnt; long ld; const int* n_pen; const float* sub; int n_sub; float theta; int vocab; };
struct NoPen {};
__device__ __forceinline__ NoPen pen_pick() { return NoPen{}; }
__device__ __forceinline__ const PenArgs& pen_pick(const PenArgs& a) { return a; }
// STA (tell_adaptive_logprob_stats, include/tell_hip.h): the K = 4 / 8 top-k form also counts the chosen
// token's rank and sums the entropy terms while the row is in registers; outputs [slots, rows(, n)].
struct StatsArgs {
  const int* chosen; long ld_chosen; const uint8_t* finished;
  int n, slots, step; const int* step_dev; int pad;
  int* alt_tok; float* alt_lp; int* rank; float* entropy; float* chosen_lp;
};
// the trailing argument of the top-k kernels: the ban list, or with PEN the penalty list, or with STA the statistics' arguments
template <bool PEN, bool MSK = false, bool STA = false> struct ListOf { typedef BanArgs type; };
template <> struct ListOf<true, false> { typedef PenArgs type; };
template <> struct ListOf<false, false, true> { typedef StatsArgs type; };
// the slot of this step (`step`, or *step_dev + 1: the convention of tell_adaptive_logprob_forced), -1: nothing is written
__device__ __forceinline__ int stats_slot(const StatsArgs& a) {
  const int s = a.step_dev ? *a.step_dev + 1 : a.step;
  return s < 0 || s >= a.slots ? -1 : s;
}
__device__ __forceinline__ void stats_neutral(const StatsArgs& a, long so) {      // a finished row: pad, 0, -1, 0, 0
  for (int q = 0; q < a.n; ++q) { a.alt_tok[so * a.n + q] = a.pad; a.alt_lp[so * a.n + q] = 0.f; }
  a.rank[so] = -1; a.entropy[so] = 0.f; a.chosen_lp[so] = 0.f;
}
// token t -> its segment (0 = head, c + 1 = tail c) and offset there; -1: outside the vocabulary
__device__ __forceinline__ int stats_locate(const LogProbArgs& p, int t, int& local) {
  local = t;
  if (t < 0) return -1;
  if (t < p.c0) return 0;
  int base = p.c0;
  for (int c = 0; c < p.n_tails; ++c) {
    if (t < base + p.tail_n[c]) { local = t - base; return c + 1; }
    base += p.tail_n[c];
  }
  return -1;
}
__device__ __forceinline__ float stats_term(float e, float d) { return e > 0.f ? e * d : 0.f; }   // (padding: 0 * -inf)
// a wave-uniform value into a scalar register: the row's 64 VGPRs leave no room for the maxima, sums and offsets
__device__ __forceinline__ float stats_uni(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
#define PEN_MAX_LIST 256
__device__ __forceinline__ int pen_count(const PenArgs& pa, int row) {
  const int np = pa.n_pen[row];
  const int cap = pa.ld < PEN_MAX_LIST ? (int)pa.ld : PEN_MAX_LIST;
  return np < 0 ? 0 : (np > cap ? cap : np);
}
__device__ __forceinline__ int pen_count(const NoPen&, int) { return 0; }
__device__ __forceinline__ int pen_count(const BanArgs&, int) { return 0; }
template <int THREADS>
__device__ __forceinline__ void pen_stage(const PenArgs& pa, int row, int np) {
  const int words = (pa.vocab + 31) >> 5;
  int* lt = reinterpret_cast<int*>(ban_bits + words);
  float* ls = reinterpret_cast<float*>(ban_bits + words + PEN_MAX_LIST);
  for (int w = threadIdx.x; w < words; w += THREADS) ban_bits[w] = 0u;
  __syncthreads();
  for (int e = threadIdx.x; e < np; e += THREADS) {
    const int t = pa.tok[(long)row * pa.ld + e];
    int c = pa.cnt[(long)row * pa.ld + e];
    c = c < 0 ? 0 : (c > pa.n_sub - 1 ? pa.n_sub - 1 : c);
    const bool ok = t >= 0 && t < pa.vocab;
    lt[e] = ok ? t : -1;
    ls[e] = pa.sub[c];
    if (ok) atomicOr(&ban_bits[t >> 5], 1u << (t & 31));
  }
  __syncthreads();
}
template <int THREADS> __device__ __forceinline__ void pen_stage(const NoPen&, int, int) {}
template <int THREADS> __device__ __forceinline__ void pen_stage(const BanArgs&, int, int) {}
__device__ __forceinline__ bool pen_bit(int j) { return (ban_bits[j >> 5] >> (j & 31)) & 1u; }
// token j has its bit set: its entry in the staged list -> s (the multiply and the subtract are not contracted)
__device__ __forceinline__ float pen_score(const PenArgs& pa, int np, int j, float lp) {
#pragma clang fp contract(off)
  const int words = (pa.vocab + 31) >> 5;
  const int* lt = reinterpret_cast<const int*>(ban_bits + words);
  const float* ls = reinterpret_cast<const float*>(ban_bits + words + PEN_MAX_LIST);
  float sv = 0.f;
  for (int e = 0; e < np; ++e)
    if (lt[e] == j) { sv = ls[e]; break; }
  const float m = fminf(lp, 0.f) * pa.theta;
  return m - sv;
}
__device__ __forceinline__ float pen_score(const NoPen&, int, int, float lp) { return lp; }
__device__ __forceinline__ float pen_score(const BanArgs&, int, int, float lp) { return lp; }
// MSK (tell_adaptive_logprob_topk_masked / _sample_masked, include/tell_hip.h): the BAN bitmap from memory - the workgroup copies
// row `i / per` of `mask` (uint32 [rows / per, ld_mask], tell_decode_vocab_mask) into ban_bits instead of zeroing it, then ORs
// the row's optional ban list in (ban == NULL or n_ban == NULL: none).  A token whose bit is set never enters a candidate list
// (top-k) or gets the key of an element outside the row (the sampler); every other log-prob is the whole row's.
struct MaskArgs { const unsigned* mask; long ld_mask; int per; const int* ban; long ld_ban; const int* n_ban; int vocab; };
__device__ __forceinline__ const MaskArgs& pen_pick(const MaskArgs& a) { return a; }
template <> struct ListOf<false, true> { typedef MaskArgs type; };
template <class... P> struct IsMask { static constexpr bool value = false; };
template <> struct IsMask<MaskArgs> { static constexpr bool value = true; };
template <int THREADS>
__device__ __forceinline__ void mask_stage(const MaskArgs& ma, int row) {
  const int words = (ma.vocab + 31) >> 5;
  const unsigned* m = ma.mask + (long)(row / ma.per) * ma.ld_mask;
  int nb = 0;                                          // (uniform over the workgroup)
  if (ma.ban && ma.n_ban) { nb = ma.n_ban[row]; nb = nb < 0 ? 0 : (nb > (int)ma.ld_ban ? (int)ma.ld_ban : nb); }
  for (int w = threadIdx.x; w < words; w += THREADS) ban_bits[w] = m[w];
  __syncthreads();
  for (int e = threadIdx.x; e < nb; e += THREADS) {
    const int t = ma.ban[(long)row * ma.ld_ban + e];
    if (t >= 0 && t < ma.vocab) atomicOr(&ban_bits[t >> 5], 1u << (t & 31));
  }
  __syncthreads();
}
// (the register-resident kernel takes `ba` as a trailing argument that BAN = false never reads: its code stays the kernel's
//  own, not an inlined body - this is the launch every greedy and beam step ends with)
template <int K, bool BAN, bool PEN = false, bool MSK = false, bool STA = false>
__global__ __launch_bounds__(1024) void logprob_regs_kernel(LogProbArgs p, int k, int* __restrict__ tokens,
                                                            float* __restrict__ lps, typename ListOf<PEN, MSK, STA>::type ba) {
  __shared__ float red[4][16];
  __shared__ float best_v[16];
  __shared__ int best_i[16];
  __shared__ int win_i;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nseg = 1 + p.n_tails;
  const float* rowp[4]; int n[4];
  rowp[0] = p.head + (long)i * p.ld_head; n[0] = p.head_n;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    rowp[c + 1] = c < p.n_tails ? p.tail[c] + (long)i * p.ld_tail[c] : rowp[0];
    n[c + 1] = c < p.n_tails ? p.tail_n[c] : 0;
  }
  [[maybe_unused]] long so = 0;                        // STA: (slot, row) in the [slots, rows] outputs
  if constexpr (STA) {                                 // (uniform over the workgroup; a row that leaves requests no logit)
    const int slot = stats_slot(ba);
    if (slot < 0) return;
    so = (long)slot * p.rows + i;
    if (ba.finished && ba.finished[i]) { if (tid == 0) stats_neutral(ba, so); return; }
    k = ba.n; tokens = ba.alt_tok + (long)slot * p.rows * k; lps = ba.alt_lp + (long)slot * p.rows * k;
  }
  int nb = 0;                                          // (requested before the row: its wait does not cover the row's loads)
  if constexpr (BAN) { nb = ba.n_ban[i]; nb = nb < 0 ? 0 : (nb > (int)ba.ld_ban ? (int)ba.ld_ban : nb); }
  if constexpr (PEN) nb = pen_count(ba, i);
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 x[16];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int q = 0; q < LPF_CAP[s]; ++q) {
      const int j = (q * 1024 + tid) * 4;
      f4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (j + 3 < n[s]) v = *reinterpret_cast<const f4*>(rowp[s] + j);
      else if (j < n[s]) {
        v.x = rowp[s][j];
        if (j + 1 < n[s]) v.y = rowp[s][j + 1];
        if (j + 2 < n[s]) v.z = rowp[s][j + 2];
      }
      x[LPF_OFF[s] + q] = v;
    }
  if constexpr (BAN) { if (nb > 0) ban_stage<1024>(ba, i, nb); }   // (nb is uniform over the workgroup)
  if constexpr (PEN) { if (nb > 0) pen_stage<1024>(ba, i, nb); }
  if constexpr (MSK) mask_stage<1024>(ba, i);
  float mx[4], sm[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < LPF_CAP[s]; ++q) {
      const f4 v = x[LPF_OFF[s] + q];
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
    mx[s] = STA ? stats_uni(m) : m;
  }
  __syncthreads();
  [[maybe_unused]] float us[4] = {0.f, 0.f, 0.f, 0.f};  // STA: this wave's sum of exp(x - m) * (x - m), paired like the sum of exp(x - m)
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float t = 0.f;
    [[maybe_unused]] float u = 0.f;
    if (s < nseg) {
#pragma unroll
      for (int q = 0; q < LPF_CAP[s]; ++q) {
        const f4 v = x[LPF_OFF[s] + q];
        if constexpr (STA) {
          const f4 d = {v.x - mx[s], v.y - mx[s], v.z - mx[s], v.w - mx[s]};
          const f4 e = {__expf(d.x), __expf(d.y), __expf(d.z), __expf(d.w)};
          t += (e.x + e.y) + (e.z + e.w);
          u += (stats_term(e.x, d.x) + stats_term(e.y, d.y)) + (stats_term(e.z, d.z) + stats_term(e.w, d.w));
        } else {
          t += (__expf(v.x - mx[s]) + __expf(v.y - mx[s])) + (__expf(v.z - mx[s]) + __expf(v.w - mx[s]));
        }
      }
    }
    t = wave_sum(t);
    if (lane == 0) red[s][wave] = t;
    if constexpr (STA) us[s] = stats_uni(wave_sum(u));
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[s][w];
    sm[s] = STA ? stats_uni(t) : t;
  }
  const float lse_h = STA ? stats_uni(mx[0] + __logf(sm[0])) : mx[0] + __logf(sm[0]);
  float tv[K]; int ti[K];
#pragma unroll
  for (int q = 0; q < K; ++q) { tv[q] = -INFINITY; ti[q] = 0x7fffffff; }
  auto better = [](float v, int j, float w, int m) { return v > w || (v == w && j < m); };
  [[maybe_unused]] int ch = 0, ch_seg = -1, cnt = 0;   // STA: the chosen token, its segment, how many tokens come before it
  [[maybe_unused]] float ch_lp = 0.f;
  if constexpr (STA) {
    __syncthreads();                                   // (red: the sums are consumed; thread 0 adds the waves' u at the end)
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (lane == 0) red[s][wave] = us[s];
    ch = ba.chosen[(long)i * ba.ld_chosen];
    int local;
    ch_seg = stats_locate(p, ch, local);
    if (ch_seg == 0) ch_lp = rowp[0][local] - lse_h;   // (the expressions of the scan below, on the same operands)
#pragma unroll
    for (int s = 1; s < 4; ++s)
      if (s == ch_seg) ch_lp = rowp[s][local] + ((rowp[0][p.c0 + s - 1] - lse_h) - (mx[s] + __logf(sm[s])));
    ch_lp = stats_uni(ch_lp);
    // the rank count is a scan of its own, before the candidate lists exist (they would not fit next to it): the log-probs
    // of the scan below, compared with the chosen token's
    if (ch_seg >= 0) {
#pragma unroll
      for (int q = 0; q < LPF_CAP[0]; ++q) {
        const int j = (q * 1024 + tid) * 4;
        cnt += (j < p.c0 && better(x[q].x - lse_h, j, ch_lp, ch)) + (j + 1 < p.c0 && better(x[q].y - lse_h, j + 1, ch_lp, ch)) +
               (j + 2 < p.c0 && better(x[q].z - lse_h, j + 2, ch_lp, ch)) + (j + 3 < p.c0 && better(x[q].w - lse_h, j + 3, ch_lp, ch));
      }
      int base = p.c0;
#pragma unroll
      for (int s = 1; s < 4; ++s) {
        if (s < nseg) {
          const float off = (rowp[0][p.c0 + s - 1] - lse_h) - (mx[s] + __logf(sm[s]));
#pragma unroll
          for (int q = 0; q < LPF_CAP[s]; ++q) {
            const int j = (q * 1024 + tid) * 4;
            const f4 v = x[LPF_OFF[s] + q];
            cnt += (j < n[s] && better(v.x + off, base + j, ch_lp, ch)) + (j + 1 < n[s] && better(v.y + off, base + j + 1, ch_lp, ch)) +
                   (j + 2 < n[s] && better(v.z + off, base + j + 2, ch_lp, ch)) + (j + 3 < n[s] && better(v.w + off, base + j + 3, ch_lp, ch));
          }
          base += n[s];
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    cnt = __builtin_amdgcn_readfirstlane(cnt);         // (this wave's count)
  }
  auto consider = [&](float v, int j) {
    if (!better(v, j, tv[K - 1], ti[K - 1])) return;
    if (BAN && nb > 0 && ((ban_bits[j >> 5] >> (j & 31)) & 1u)) return;
    if constexpr (MSK) { if (pen_bit(j)) return; }
    if constexpr (PEN) {
      if (nb > 0 && pen_bit(j)) {
        v = pen_score(ba, nb, j, v);
        if (!better(v, j, tv[K - 1], ti[K - 1])) return;
      }
    }
    tv[K - 1] = v; ti[K - 1] = j;
#pragma unroll
    for (int q = K - 1; q > 0; --q)
      if (better(tv[q], ti[q], tv[q - 1], ti[q - 1])) {
        const float fv = tv[q]; tv[q] = tv[q - 1]; tv[q - 1] = fv;
        const int fi = ti[q]; ti[q] = ti[q - 1]; ti[q - 1] = fi;
      }
  };
#pragma unroll
  for (int q = 0; q < LPF_CAP[0]; ++q) {
    const int j = (q * 1024 + tid) * 4;
    if (j < p.c0) consider(x[q].x - lse_h, j);
    if (j + 1 < p.c0) consider(x[q].y - lse_h, j + 1);
    if (j + 2 < p.c0) consider(x[q].z - lse_h, j + 2);
    if (j + 3 < p.c0) consider(x[q].w - lse_h, j + 3);
  }
  int base = p.c0;
#pragma unroll
  for (int s = 1; s < 4; ++s) {
    if (s < nseg) {
      const float off = (rowp[0][p.c0 + s - 1] - lse_h) - (mx[s] + __logf(sm[s]));
#pragma unroll
      for (int q = 0; q < LPF_CAP[s]; ++q) {
        const int j = (q * 1024 + tid) * 4;
        const f4 v = x[LPF_OFF[s] + q];
        if (j < n[s]) consider(v.x + off, base + j);
        if (j + 1 < n[s]) consider(v.y + off, base + j + 1);
        if (j + 2 < n[s]) consider(v.z + off, base + j + 2);
        if (j + 3 < n[s]) consider(v.w + off, base + j + 3);
      }
      base += n[s];
    }
  }
  if constexpr (STA) {                                 // rank: a thread's count, the wave (above), then the waves
    if (lane == 0) best_i[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
      int total = 0;
      for (int w = 0; w < 16; ++w) total += best_i[w];
      float ut[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        ut[s] = 0.f;
        for (int w = 0; w < 16; ++w) ut[s] += red[s][w];
      }
      float H = __logf(sm[0]) - ut[0] / sm[0];         // chain rule: the head, then every tail weighted by its cluster
#pragma unroll
      for (int s = 1; s < 4; ++s)
        if (s < nseg) H += __expf(rowp[0][p.c0 + s - 1] - lse_h) * (__logf(sm[s]) - ut[s] / sm[s]);
      ba.rank[so] = ch_seg >= 0 ? total : -1;
      ba.chosen_lp[so] = ch_seg >= 0 ? ch_lp : 0.f;
      ba.entropy[so] = H;
    }
  }
  for (int r = 0; r < k; ++r) {                       // pop the block-wide best k times (lowest index wins ties)
    float bv = tv[0]; int bi = ti[0];
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();                                   // previous round's win_i / best_* consumed
    if (lane == 0) { best_v[wave] = bv; best_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 16; ++w)
        if (better(best_v[w], best_i[w], bv, bi)) { bv = best_v[w]; bi = best_i[w]; }
      if (K == 1) {
        if (p.token) p.token[i] = bi;
        if (p.token_lp) p.token_lp[i] = bv;
      } else {
        tokens[(long)i * k + r] = bi;
        lps[(long)i * k + r] = bv;
      }
      win_i = bi;
    }
    if (K == 1) break;
    __syncthreads();
    if (ti[0] == win_i) {                              // the owner of the winner advances its list
#pragma unroll
      for (int q = 0; q < K - 1; ++q) { tv[q] = tv[q + 1]; ti[q] = ti[q + 1]; }
      tv[K - 1] = -INFINITY; ti[K - 1] = 0x7fffffff;
    }
  }
}

// Top-k variant for beam search: per row the k best (log-prob, token) pairs of the adaptive softmax, sorted best
// first, without materialising [rows, vocab] (a beam of k only ever needs each hypothesis' own k best tokens).
// Every thread keeps its k best in registers while streaming the row; the block then pops the global best k times.
template <int K, bool BAN, bool PEN = false, bool MSK = false>
__device__ __forceinline__ void logprob_topk_body(const LogProbArgs& p, int k, int* __restrict__ tokens,
                                                  float* __restrict__ lps, const typename ListOf<PEN, MSK>::type& ba) {
  __shared__ float red[4];
  __shared__ float best_v[4];
  __shared__ int best_i[4];
  __shared__ int win_i;
  const int i = blockIdx.x;
  const float* hrow = p.head + (long)i * p.ld_head;
  float tv[K]; int ti[K];
#pragma unroll
  for (int q = 0; q < K; ++q) { tv[q] = -INFINITY; ti[q] = 0x7fffffff; }
  auto better = [](float v, int j, float w, int m) { return v > w || (v == w && j < m); };
  int nb = 0;
  if constexpr (BAN) {
    nb = ba.n_ban[i]; nb = nb < 0 ? 0 : (nb > (int)ba.ld_ban ? (int)ba.ld_ban : nb);
    if (nb > 0) ban_stage<256>(ba, i, nb);             // (nb is uniform over the workgroup)
  }
  if constexpr (PEN) {
    nb = pen_count(ba, i);
    if (nb > 0) pen_stage<256>(ba, i, nb);
  }
  if constexpr (MSK) mask_stage<256>(ba, i);
  auto push = [&](float v, int j) {
    if (!better(v, j, tv[K - 1], ti[K - 1])) return;
    if (BAN && nb > 0 && ((ban_bits[j >> 5] >> (j & 31)) & 1u)) return;
    if constexpr (MSK) { if (pen_bit(j)) return; }
    if constexpr (PEN) {
      if (nb > 0 && pen_bit(j)) {
        v = pen_score(ba, nb, j, v);
        if (!better(v, j, tv[K - 1], ti[K - 1])) return;
      }
    }
    tv[K - 1] = v; ti[K - 1] = j;
#pragma unroll
    for (int q = K - 1; q > 0; --q)
      if (better(tv[q], ti[q], tv[q - 1], ti[q - 1])) {
        const float fv = tv[q]; tv[q] = tv[q - 1]; tv[q - 1] = fv;
        const int fi = ti[q]; ti[q] = ti[q - 1]; ti[q - 1] = fi;
      }
  };
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < p.head_n; j += 256) mx = fmaxf(mx, hrow[j]);
  mx = block_max(mx, red);
  float s = 0.f;
  for (int j = threadIdx.x; j < p.head_n; j += 256) s += __expf(hrow[j] - mx);
  s = block_sum(s, red);
  const float lse_h = mx + __logf(s);
  for (int j = threadIdx.x; j < p.c0; j += 256) push(hrow[j] - lse_h, j);
  int base = p.c0;
  for (int c = 0; c < p.n_tails; ++c) {
    const float* trow = p.tail[c] + (long)i * p.ld_tail[c];
    const int n = p.tail_n[c];
    float m2 = -INFINITY;
    for (int j = threadIdx.x; j < n; j += 256) m2 = fmaxf(m2, trow[j]);
    m2 = block_max(m2, red);
    float s2 = 0.f;
    for (int j = threadIdx.x; j < n; j += 256) s2 += __expf(trow[j] - m2);
    s2 = block_sum(s2, red);
    const float off = (hrow[p.c0 + c] - lse_h) - (m2 + __logf(s2));
    for (int j = threadIdx.x; j < n; j += 256) push(trow[j] + off, base + j);
    base += n;
  }
  for (int r = 0; r < k; ++r) {                       // pop the block-wide best k times
    float bv = tv[0]; int bi = ti[0];
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();                                   // previous round's win_i / best_* consumed
    if ((threadIdx.x & 63) == 0) { best_v[threadIdx.x >> 6] = bv; best_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; ++w)
        if (better(best_v[w], best_i[w], bv, bi)) { bv = best_v[w]; bi = best_i[w]; }
      tokens[(long)i * k + r] = bi;
      lps[(long)i * k + r] = bv;
      win_i = bi;
    }
    __syncthreads();
    if (ti[0] == win_i) {                              // the owner of the winner advances its list
#pragma unroll
      for (int q = 0; q < K - 1; ++q) { tv[q] = tv[q + 1]; ti[q] = ti[q + 1]; }
      tv[K - 1] = -INFINITY; ti[K - 1] = 0x7fffffff;
    }
  }
}
template <int K>
__global__ __launch_bounds__(256) void logprob_topk_kernel(LogProbArgs p, int k, int* __restrict__ tokens,
                                                           float* __restrict__ lps) {
  logprob_topk_body<K, false>(p, k, tokens, lps, BanArgs{nullptr, 0, nullptr, 0});
}
template <int K>
__global__ __launch_bounds__(256) void logprob_topk_banned_kernel(LogProbArgs p, int k, int* __restrict__ tokens,
                                                                  float* __restrict__ lps, BanArgs ba) {
  logprob_topk_body<K, true>(p, k, tokens, lps, ba);
}
template <int K>
__global__ __launch_bounds__(256) void logprob_topk_penalised_kernel(LogProbArgs p, int k, int* __restrict__ tokens,
                                                                     float* __restrict__ lps, PenArgs pa) {
  logprob_topk_body<K, false, true>(p, k, tokens, lps, pa);
}
template <int K>
__global__ __launch_bounds__(256) void logprob_topk_masked_kernel(LogProbArgs p, int k, int* __restrict__ tokens,
                                                                  float* __restrict__ lps, MaskArgs ma) {
  logprob_topk_body<K, false, false, true>(p, k, tokens, lps, ma);
}
// What every launcher below builds from its Logits (logits_args.h): the kernels' view of them ...
static LogProbArgs logprob_args(const Logits& lg, float* log_probs = nullptr, long ld_lp = 0, int* token = nullptr,
                                float* token_lp = nullptr) {
  LogProbArgs p;
  p.head = lg.head; p.ld_head = lg.ld_head; p.head_n = lg.c0 + lg.n_tails; p.c0 = lg.c0; p.n_tails = lg.n_tails; p.rows = lg.rows;
  for (int i = 0; i < 3; ++i) { p.tail[i] = lg.tail[i]; p.ld_tail[i] = lg.ld[i]; p.tail_n[i] = lg.n[i]; }
  p.log_probs = log_probs; p.ld_lp = ld_lp; p.token = token; p.token_lp = token_lp;
  return p;
}
// ... and the LDS bytes of the bitmap over the vocabulary (ban_bits).
static size_t bitmap_lds(int vocab) { return (size_t)((vocab + 31) >> 5) * sizeof(unsigned); }
extern "C" int tell_adaptive_logprob_topk(const float* head, long ld_head, int c0, int n_tails,
                                          const float* tail0, long ld0, int n0, const float* tail1, long ld1,
                                          int n1, const float* tail2, long ld2, int n2, int rows, int k,
                                          int* tokens, float* lps, hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_topk: up to 3 tails");
  TELL_REQUIRE(k >= 1 && k <= 8, "logprob_topk: 1 <= k <= 8");
  if (rows <= 0) return TELL_OK;
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  const LogProbArgs p = logprob_args(lg);
  if (logits_regs(lg)) {
    if (k <= 4) hipLaunchKernelGGL((logprob_regs_kernel<4, false>), dim3(rows), dim3(1024), 0, stream, p, k, tokens, lps, BanArgs{});
    else hipLaunchKernelGGL((logprob_regs_kernel<8, false>), dim3(rows), dim3(1024), 0, stream, p, k, tokens, lps, BanArgs{});
    return tell_check_launch("logprob_topk (registers)");
  }
  if (k <= 4) hipLaunchKernelGGL((logprob_topk_kernel<4>), dim3(rows), dim3(256), 0, stream, p, k, tokens, lps);
  else hipLaunchKernelGGL((logprob_topk_kernel<8>), dim3(rows), dim3(256), 0, stream, p, k, tokens, lps);
  return tell_check_launch("logprob_topk");
}

// tell_adaptive_logprob_topk with a ban list per row (include/tell_hip.h): ban int32 [rows, ld_ban], n_ban int32 [rows].
extern "C" int tell_adaptive_logprob_topk_banned(const float* head, long ld_head, int c0, int n_tails,
                                                 const float* tail0, long ld0, int n0, const float* tail1, long ld1,
                                                 int n1, const float* tail2, long ld2, int n2, int rows, int k,
                                                 const int* ban, long ld_ban, const int* n_ban, int* tokens, float* lps,
                                                 hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_topk_banned: up to 3 tails");
  TELL_REQUIRE(k >= 1 && k <= 8, "logprob_topk_banned: 1 <= k <= 8");
  TELL_REQUIRE(ban && n_ban && ld_ban >= 1, "logprob_topk_banned: ban [rows, ld_ban] and n_ban [rows]");
  if (rows <= 0) return TELL_OK;
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  const LogProbArgs p = logprob_args(lg);
  const BanArgs ba{ban, ld_ban, n_ban, (int)logits_vocab(lg)};
  TELL_REQUIRE(ba.vocab > 0 && ba.vocab <= (1 << 18), "logprob_topk_banned: vocab <= 2^18 (the ban bitmap: 32 KB of LDS)");
  const size_t lds = bitmap_lds(ba.vocab);
  if (logits_regs(lg)) {
    if (k <= 4) hipLaunchKernelGGL((logprob_regs_kernel<4, true>), dim3(rows), dim3(1024), lds, stream, p, k, tokens, lps, ba);
    else hipLaunchKernelGGL((logprob_regs_kernel<8, true>), dim3(rows), dim3(1024), lds, stream, p, k, tokens, lps, ba);
    return tell_check_launch("logprob_topk_banned (registers)");
  }
  if (k <= 4) hipLaunchKernelGGL((logprob_topk_banned_kernel<4>), dim3(rows), dim3(256), lds, stream, p, k, tokens, lps, ba);
  else hipLaunchKernelGGL((logprob_topk_banned_kernel<8>), dim3(rows), dim3(256), lds, stream, p, k, tokens, lps, ba);
  return tell_check_launch("logprob_topk_banned");
}

// tell_adaptive_logprob_topk over penalised scores (include/tell_hip.h): pen_tok / pen_cnt int32 [rows, ld_pen], n_pen int32
// [rows] (tell_decode_token_counts), sub fp32 [n_sub] on the device.
static int pen_args(PenArgs& pa, const Logits& lg, const int* pen_tok, const int* pen_cnt, long ld_pen, const int* n_pen,
                    float theta, const float* sub, int n_sub) {
  TELL_REQUIRE(pen_tok && pen_cnt && n_pen && ld_pen >= 1, "logprob penalised: pen_tok / pen_cnt [rows, ld_pen] and n_pen [rows]");
  TELL_REQUIRE(sub && n_sub >= 1, "logprob penalised: sub fp32 [n_sub >= 1]");
  TELL_REQUIRE(theta >= 1.f && theta < INFINITY, "logprob penalised: theta finite and >= 1");
  pa.tok = pen_tok; pa.cnt = pen_cnt; pa.ld = ld_pen; pa.n_pen = n_pen; pa.sub = sub; pa.n_sub = n_sub; pa.theta = theta;
  pa.vocab = (int)logits_vocab(lg);
  TELL_REQUIRE(pa.vocab > 0 && pa.vocab <= (1 << 18), "logprob penalised: vocab <= 2^18 (the bitmap: 32 KB of LDS)");
  return TELL_OK;
}
static size_t pen_lds(const PenArgs& pa) { return bitmap_lds(pa.vocab) + 2 * PEN_MAX_LIST * sizeof(unsigned); }
extern "C" int tell_adaptive_logprob_topk_penalised(const float* head, long ld_head, int c0, int n_tails,
                                                    const float* tail0, long ld0, int n0, const float* tail1, long ld1,
                                                    int n1, const float* tail2, long ld2, int n2, int rows, int k,
                                                    const int* pen_tok, const int* pen_cnt, long ld_pen, const int* n_pen,
                                                    float theta, const float* sub, int n_sub, int* tokens, float* lps,
                                                    hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_topk_penalised: up to 3 tails");
  TELL_REQUIRE(k >= 1 && k <= 8, "logprob_topk_penalised: 1 <= k <= 8");
  TELL_REQUIRE(tokens && lps, "logprob_topk_penalised: tokens and lps [rows, k]");
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  PenArgs pa;
  const int rc = pen_args(pa, lg, pen_tok, pen_cnt, ld_pen, n_pen, theta, sub, n_sub);
  if (rc != TELL_OK) return rc;
  if (rows <= 0) return TELL_OK;
  const LogProbArgs p = logprob_args(lg);
  const size_t lds = pen_lds(pa);
  if (logits_regs(lg)) {
    if (k == 1) {                                            // the arg-max form: its winner goes to token / token_lp
      hipLaunchKernelGGL((logprob_regs_kernel<1, false, true>), dim3(rows), dim3(1024), lds, stream,
                         logprob_args(lg, nullptr, 0, tokens, lps), 1, tokens, lps, pa);
    } else if (k <= 4) hipLaunchKernelGGL((logprob_regs_kernel<4, false, true>), dim3(rows), dim3(1024), lds, stream, p, k, tokens, lps, pa);
    else hipLaunchKernelGGL((logprob_regs_kernel<8, false, true>), dim3(rows), dim3(1024), lds, stream, p, k, tokens, lps, pa);
    return tell_check_launch("logprob_topk_penalised (registers)");
  }
  if (k <= 4) hipLaunchKernelGGL((logprob_topk_penalised_kernel<4>), dim3(rows), dim3(256), lds, stream, p, k, tokens, lps, pa);
  else hipLaunchKernelGGL((logprob_topk_penalised_kernel<8>), dim3(rows), dim3(256), lds, stream, p, k, tokens, lps, pa);
  return tell_check_launch("logprob_topk_penalised");
}

// tell_adaptive_logprob_topk under a vocabulary mask (include/tell_hip.h): mask uint32 [rows / per, ld_mask >= words], row r
// reads mask row r / per; ban / n_ban as tell_adaptive_logprob_topk_banned or NULL.
static int mask_args(MaskArgs& ma, const Logits& lg, const uint32_t* mask, long ld_mask, int per, const int* ban, long ld_ban,
                     const int* n_ban) {
  ma.vocab = (int)logits_vocab(lg);
  TELL_REQUIRE(ma.vocab > 0 && ma.vocab <= (1 << 18), "logprob masked: vocab <= 2^18 (the bitmap: 32 KB of LDS)");
  TELL_REQUIRE(mask && ld_mask >= (ma.vocab + 31) / 32, "logprob masked: mask uint32 [rows / per, ld_mask >= words]");
  TELL_REQUIRE(per >= 1 && lg.rows % per == 0, "logprob masked: rows must be a multiple of per >= 1");
  TELL_REQUIRE(!ban || ld_ban >= 1, "logprob masked: ban [rows, ld_ban >= 1]");
  ma.mask = mask; ma.ld_mask = ld_mask; ma.per = per; ma.ban = ban; ma.ld_ban = ld_ban; ma.n_ban = n_ban;
  return TELL_OK;
}
extern "C" int tell_adaptive_logprob_topk_masked(const float* head, long ld_head, int c0, int n_tails, const float* tail0,
                                                 long ld0, int n0, const float* tail1, long ld1, int n1, const float* tail2,
                                                 long ld2, int n2, int rows, int k, const uint32_t* mask, long ld_mask, int per,
                                                 const int* ban, long ld_ban, const int* n_ban, int* tokens, float* lps,
                                                 hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_topk_masked: up to 3 tails");
  TELL_REQUIRE(k >= 1 && k <= 8, "logprob_topk_masked: 1 <= k <= 8");
  TELL_REQUIRE(tokens && lps, "logprob_topk_masked: tokens and lps [rows, k]");
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  MaskArgs ma;
  const int rc = mask_args(ma, lg, mask, ld_mask, per, ban, ld_ban, n_ban);
  if (rc != TELL_OK) return rc;
  if (rows <= 0) return TELL_OK;
  const LogProbArgs p = logprob_args(lg);
  const size_t lds = bitmap_lds(ma.vocab);
  if (logits_regs(lg)) {
    if (k <= 4) hipLaunchKernelGGL((logprob_regs_kernel<4, false, false, true>), dim3(rows), dim3(1024), lds, stream, p, k, tokens, lps, ma);
    else hipLaunchKernelGGL((logprob_regs_kernel<8, false, false, true>), dim3(rows), dim3(1024), lds, stream, p, k, tokens, lps, ma);
    return tell_check_launch("logprob_topk_masked (registers)");
  }
  if (k <= 4) hipLaunchKernelGGL((logprob_topk_masked_kernel<4>), dim3(rows), dim3(256), lds, stream, p, k, tokens, lps, ma);
  else hipLaunchKernelGGL((logprob_topk_masked_kernel<8>), dim3(rows), dim3(256), lds, stream, p, k, tokens, lps, ma);
  return tell_check_launch("logprob_topk_masked");
}

extern "C" int tell_adaptive_logprob_argmax(const float* head, long ld_head, int c0, int n_tails,
                                            const float* tail0, long ld0, int n0, const float* tail1,
                                            long ld1, int n1, const float* tail2, long ld2, int n2,
                                            int rows, float* log_probs, long ld_lp, int* token,
                                            float* token_lp, hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_argmax: up to 3 tails");
  if (rows <= 0) return TELL_OK;
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  const LogProbArgs p = logprob_args(lg, log_probs, ld_lp, token, token_lp);
  if (!log_probs && logits_regs(lg)) {                       // (the register form does not write the full rows)
    hipLaunchKernelGGL((logprob_regs_kernel<1, false>), dim3(rows), dim3(1024), 0, stream, p, 1, (int*)nullptr, (float*)nullptr,
                       BanArgs{});
    return tell_check_launch("logprob_argmax (registers)");
  }
  hipLaunchKernelGGL(logprob_argmax_kernel, dim3(rows), dim3(1024), 0, stream, p);
  return tell_check_launch("logprob_argmax");
}

// ------------------------------------------------------------------ forced tokens (caption completion)
// Runs BEHIND the mode's pick kernel, over the tokens / lps [rows, k] it has just written.  A row whose sample still has
// prefix left at this step (i < plen[sample]) gets tokens[r][0] = prefix[sample][i] and lps[r][0] = that token's log-prob
// exactly as the arg-max kernels write it; entries 1 .. k - 1 become (-inf, pad).  Every other row leaves before a single
// logit is requested.  One 1024-thread workgroup per row; only the head and the forced token's own tail are reduced, with
// the reductions of logprob_regs_kernel (REGS) / logprob_argmax_kernel (streaming): same grouping, same order, same bits.
struct ForcedArgs {
  const long* prefix; long ld_prefix; int P;
  const int* plen; int n_samples;
  const int* row_ids; int beams;
  int step; const int* step_dev;
  int pad, k;
  int* tokens; float* lps;
};
// log-sum-exp of one register-resident segment: logprob_regs_kernel's loads, per-thread pairing, wave and cross-wave order
template <int S>
__device__ __forceinline__ float forced_lse_regs(const float* __restrict__ row, int n, float* red) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  f4 x[LPF_CAP[S]];
#pragma unroll
  for (int q = 0; q < LPF_CAP[S]; ++q) {
    const int j = (q * 1024 + tid) * 4;
    f4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (j + 3 < n) v = *reinterpret_cast<const f4*>(row + j);
    else if (j < n) {
      v.x = row[j];
      if (j + 1 < n) v.y = row[j + 1];
      if (j + 2 < n) v.z = row[j + 2];
    }
    x[q] = v;
  }
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < LPF_CAP[S]; ++q) m = fmaxf(fmaxf(m, fmaxf(x[q].x, x[q].y)), fmaxf(x[q].z, x[q].w));
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  float mx = red[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) mx = fmaxf(mx, red[w]);
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < LPF_CAP[S]; ++q)
    t += (__expf(x[q].x - mx) + __expf(x[q].y - mx)) + (__expf(x[q].z - mx) + __expf(x[q].w - mx));
  t = wave_sum(t);
  if (lane == 0) red[wave] = t;
  __syncthreads();
  float sm = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) sm += red[w];
  __syncthreads();
  return mx + __logf(sm);
}
// ... and of a streamed one: logprob_argmax_kernel's two passes
__device__ __forceinline__ float forced_lse_stream(const float* __restrict__ row, int n, float* red) {
  float mx = -INFINITY;
#pragma unroll 4
  for (int j = threadIdx.x; j < n; j += 1024) mx = fmaxf(mx, row[j]);
  mx = block_max(mx, red);
  float s = 0.f;
#pragma unroll 4
  for (int j = threadIdx.x; j < n; j += 1024) s += __expf(row[j] - mx);
  s = block_sum(s, red);
  return mx + __logf(s);
}
template <bool REGS>
__global__ __launch_bounds__(1024) void logprob_forced_kernel(LogProbArgs p, ForcedArgs a) {
  __shared__ float red[16];
  const int r = blockIdx.x;
  // (uniform over the workgroup: everything below depends on the row alone)
  const int row = a.row_ids ? a.row_ids[r] : r;
  const int sample = row / a.beams;
  if (row < 0 || sample >= a.n_samples) return;
  const int i = a.step_dev ? *a.step_dev + 1 : a.step;
  int pl = a.plen[sample];
  pl = pl > a.P ? a.P : pl;
  if (i < 0 || i >= pl) return;                              // a free row: the pick stands, no logit is read
  const long t = a.prefix[(long)sample * a.ld_prefix + i];
  const float* hrow = p.head + (long)r * p.ld_head;
  // the forced token's segment: 0 = head, c + 1 = tail c at offset `local`
  int seg = -1, local = 0;
  if (t >= 0 && t < p.c0) { seg = 0; local = (int)t; }
  else if (t >= p.c0) {
    long base = p.c0;
    for (int c = 0; c < p.n_tails; ++c) {
      if (t < base + p.tail_n[c]) { seg = c + 1; local = (int)(t - base); break; }
      base += p.tail_n[c];
    }
  }
  float lp = -INFINITY;
  int tok = a.pad;                                           // (an id outside the vocabulary: the host check refuses it)
  if (seg >= 0) {
    const float lse_h = REGS ? forced_lse_regs<0>(hrow, p.head_n, red) : forced_lse_stream(hrow, p.head_n, red);
    tok = (int)t;
    if (seg == 0) lp = hrow[local] - lse_h;
    else {
      const int c = seg - 1;
      const float* trow = p.tail[c] + (long)r * p.ld_tail[c];
      const int n = p.tail_n[c];
      float lse_t;
      if (!REGS) lse_t = forced_lse_stream(trow, n, red);
      else if (c == 0) lse_t = forced_lse_regs<1>(trow, n, red);
      else if (c == 1) lse_t = forced_lse_regs<2>(trow, n, red);
      else lse_t = forced_lse_regs<3>(trow, n, red);
      const float off = (hrow[p.c0 + c] - lse_h) - lse_t;
      lp = trow[local] + off;
    }
  }
  if (threadIdx.x == 0) {
    a.tokens[(long)r * a.k] = tok;
    a.lps[(long)r * a.k] = lp;
    for (int q = 1; q < a.k; ++q) { a.tokens[(long)r * a.k + q] = a.pad; a.lps[(long)r * a.k + q] = -INFINITY; }
  }
}
extern "C" int tell_adaptive_logprob_forced(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                            int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                            int rows, int k, const long* prefix, long ld_prefix, int P, const int* plen,
                                            int n_samples, const int* row_ids, int beams, int step, const int* step_dev,
                                            int pad, int* tokens, float* lps, hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_forced: up to 3 tails");
  TELL_REQUIRE(k >= 1 && k <= 8, "logprob_forced: 1 <= k <= 8");
  TELL_REQUIRE(prefix && plen && P >= 1 && ld_prefix >= P && n_samples >= 1, "logprob_forced: prefix [n_samples, P] and plen [n_samples]");
  TELL_REQUIRE(beams >= 1 && (row_ids || (long)n_samples * beams >= rows), "logprob_forced: rows / beams exceeds n_samples");
  TELL_REQUIRE(step_dev || step >= 0, "logprob_forced: step >= 0");
  TELL_REQUIRE(tokens && lps, "logprob_forced: tokens and lps [rows, k]");
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  TELL_REQUIRE(pad >= 0 && pad < (int)logits_vocab(lg), "logprob_forced: pad must be a token of the vocabulary (it is the next step's input of a filler hypothesis)");
  if (rows <= 0) return TELL_OK;
  const LogProbArgs p = logprob_args(lg);
  ForcedArgs a;
  a.prefix = prefix; a.ld_prefix = ld_prefix; a.P = P; a.plen = plen; a.n_samples = n_samples; a.row_ids = row_ids;
  a.beams = beams; a.step = step; a.step_dev = step_dev; a.pad = pad; a.k = k; a.tokens = tokens; a.lps = lps;
  if (logits_regs(lg)) {
    hipLaunchKernelGGL((logprob_forced_kernel<true>), dim3(rows), dim3(1024), 0, stream, p, a);
    return tell_check_launch("logprob_forced (registers)");
  }
  hipLaunchKernelGGL((logprob_forced_kernel<false>), dim3(rows), dim3(1024), 0, stream, p, a);
  return tell_check_launch("logprob_forced");
}

// ------------------------------------------------------------------ per-token statistics
// Runs BEHIND the step's pick (and forced) launch over the same logits: the n best tokens of the model's own distribution,
// the rank and log-prob of the token the step took (chosen[r][0]) and the row's entropy, into slot `step` of static buffers.
// Register form: logprob_regs_kernel<8, ..., STA> above - the K = 8 top-k kernel itself, so the alternatives are its bits.
// Streaming form (below): logprob_topk_body<8> writes the alternatives - the streaming top-k kernel's own code, hence ITS 256
// threads and sum order -, then the same two passes per cluster once more with the entropy sum riding on the second, then one
// pass that counts the rank.  Three more reads of the row than the register form: this is the fall-back for rows that do not
// fit LPF_CAP or do not start on 16 bytes.
__device__ __forceinline__ void stats_cluster_stream(const float* __restrict__ row, int n, float* red, float& lse, float& H) {
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < n; j += 256) mx = fmaxf(mx, row[j]);
  mx = block_max(mx, red);
  float s = 0.f, u = 0.f;
  for (int j = threadIdx.x; j < n; j += 256) {
    const float d = row[j] - mx, e = __expf(d);
    s += e;
    u += stats_term(e, d);
  }
  s = block_sum(s, red);
  u = block_sum(u, red);
  lse = mx + __logf(s);
  H = __logf(s) - u / s;
}
__global__ __launch_bounds__(256) void logprob_stats_stream_kernel(LogProbArgs p, StatsArgs a) {
  __shared__ float red[4];
  __shared__ int cnt_w[4];
  const int i = blockIdx.x;
  const int slot = stats_slot(a);                              // (uniform over the workgroup, like everything up to the body)
  if (slot < 0) return;
  const long so = (long)slot * p.rows + i;
  if (a.finished && a.finished[i]) { if (threadIdx.x == 0) stats_neutral(a, so); return; }
  logprob_topk_body<8, false>(p, a.n, a.alt_tok + (long)slot * p.rows * a.n, a.alt_lp + (long)slot * p.rows * a.n,
                              BanArgs{nullptr, 0, nullptr, 0});
  __syncthreads();
  const float* hrow = p.head + (long)i * p.ld_head;
  float lse_h, H, off[3] = {0.f, 0.f, 0.f};
  stats_cluster_stream(hrow, p.head_n, red, lse_h, H);
  for (int c = 0; c < p.n_tails; ++c) {
    float lse_t, H_t;
    stats_cluster_stream(p.tail[c] + (long)i * p.ld_tail[c], p.tail_n[c], red, lse_t, H_t);
    off[c] = (hrow[p.c0 + c] - lse_h) - lse_t;
    H += __expf(hrow[p.c0 + c] - lse_h) * H_t;
  }
  const int ch = a.chosen[(long)i * a.ld_chosen];
  int local;
  const int seg = stats_locate(p, ch, local);
  float ch_lp = 0.f;
  if (seg == 0) ch_lp = hrow[local] - lse_h;
  else if (seg > 0) ch_lp = p.tail[seg - 1][(long)i * p.ld_tail[seg - 1] + local] + off[seg - 1];
  int cnt = 0;
  if (seg >= 0) {
    auto before = [&](float v, int j) { return v > ch_lp || (v == ch_lp && j < ch); };
    for (int j = threadIdx.x; j < p.c0; j += 256) cnt += before(hrow[j] - lse_h, j) ? 1 : 0;
    int base = p.c0;
    for (int c = 0; c < p.n_tails; ++c) {
      const float* trow = p.tail[c] + (long)i * p.ld_tail[c];
      for (int j = threadIdx.x; j < p.tail_n[c]; j += 256) cnt += before(trow[j] + off[c], base + j) ? 1 : 0;
      base += p.tail_n[c];
    }
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) cnt_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    a.rank[so] = seg >= 0 ? (cnt_w[0] + cnt_w[1]) + (cnt_w[2] + cnt_w[3]) : -1;
    a.chosen_lp[so] = seg >= 0 ? ch_lp : 0.f;
    a.entropy[so] = H;
  }
}
extern "C" int tell_adaptive_logprob_stats(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                           int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                           int rows, const int* chosen, long ld_chosen, const uint8_t* finished, int n,
                                           int slots, int step, const int* step_dev, int pad, int* alt_tok, float* alt_lp,
                                           int* rank, float* entropy, float* chosen_lp, hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_stats: up to 3 tails");
  TELL_REQUIRE(n >= 1 && n <= 8, "logprob_stats: 1 <= n <= 8 alternatives");
  TELL_REQUIRE(rows >= 1, "logprob_stats: rows >= 1");
  TELL_REQUIRE(chosen && ld_chosen >= 1, "logprob_stats: chosen int32 [rows, ld_chosen >= 1]");
  TELL_REQUIRE(slots >= 1 && (step_dev || (step >= 0 && step < slots)), "logprob_stats: 0 <= step < slots");
  TELL_REQUIRE(alt_tok && alt_lp && rank && entropy && chosen_lp,
               "logprob_stats: alt_tok / alt_lp [slots, rows, n] and rank / entropy / chosen_lp [slots, rows]");
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  const LogProbArgs p = logprob_args(lg);
  StatsArgs a;
  a.chosen = chosen; a.ld_chosen = ld_chosen; a.finished = finished; a.n = n; a.slots = slots; a.step = step;
  a.step_dev = step_dev; a.pad = pad; a.alt_tok = alt_tok; a.alt_lp = alt_lp; a.rank = rank; a.entropy = entropy;
  a.chosen_lp = chosen_lp;
  if (logits_regs(lg)) {
    // (K as tell_adaptive_logprob_topk picks it for k = n: the alternatives come from the same instantiation's code)
    if (n <= 4) hipLaunchKernelGGL((logprob_regs_kernel<4, false, false, false, true>), dim3(rows), dim3(1024), 0, stream, p, n,
                                   (int*)nullptr, (float*)nullptr, a);
    else hipLaunchKernelGGL((logprob_regs_kernel<8, false, false, false, true>), dim3(rows), dim3(1024), 0, stream, p, n,
                            (int*)nullptr, (float*)nullptr, a);
    return tell_check_launch("logprob_stats (registers)");
  }
  hipLaunchKernelGGL(logprob_stats_stream_kernel, dim3(rows), dim3(256), 0, stream, p, a);
  return tell_check_launch("logprob_stats");
}

// ------------------------------------------------------------------ top-k sampling with a temperature
// transformer_faces_objects.py:443-470 with sampling_topk = k: lprobs.topk(k), / T, torch.multinomial.  Per row, exactly
// (include/tell_hip.h, DESIGN.md "Top-k sampling"): the k largest log-probs of the full adaptive softmax (value descending,
// lower token id first on ties; the log-probs are those of the arg-max kernels), the uniform u of (seed, row, step)
// (common.h tell_sample_u), the pick of tell_sample_pick; out: the token and its log-prob WITHOUT the temperature (the
// bookkeeping launch divides).  One 1024-thread workgroup per row.
//
// The exact top-k is a radix select on order-preserving 32-bit keys (0 = not a token: padding, cluster columns):
//  1. tau = the k-th largest of the 1024 per-thread maxima (4 passes of 8 bits over one key per thread).  The k threads
//     that own the k largest maxima hold k elements >= tau, so every element of the top k is >= tau;
//  2. the k-th largest key K over the elements >= tau (4 passes; typically a few times k elements take part, so the LDS
//     histogram atomics stay few), and how many elements tie at K;
//  3. only if more elements tie at K than the top k takes: the lowest token ids among the ties (3 passes over the ids);
//  4. the k winners are compacted into LDS, ranked (value, id) by k threads, and thread 0 draws.
// Every pass walks the row's elements through `each` - the registers of the row (logprob_sample_regs_kernel) or the
// logits in memory (logprob_sample_stream_kernel) - so the register form never reads the row twice.
struct SampleArgs {
  int k; float inv_temp;
  const uint32_t* seed_dev; const int* row_ids; int step; const int* step_dev;
  int* tokens; float* lps;
  float topp; int* nuc_size; uint32_t* nuc_key;       // the nucleus entry point only (tell_adaptive_logprob_nucleus)
  float* typ_c;                                       // tell_adaptive_logprob_typical only (topp: its tau; min-p: log_minp)
};
struct SampleSmem {
  int hist[256];
  uint32_t cand_key[64]; int cand_idx[64];
  float sort_v[64]; int sort_i[64];
  int sel, above, count, n_cand;
  uint32_t ref;                       // the filter's reference value, read from LDS in every pass (see sample_radix_select)
};
__device__ __forceinline__ uint32_t lp_key(float v) {          // order-preserving: larger float -> larger key
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_lp(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// ---- nucleus (top-p) over k candidates sorted best first (tell_adaptive_logprob_nucleus with k > 0, tell_nucleus_candidates)
// steps 1-2: w_j = exp((lp_j - lp_0) * inv_temp) summed in candidate order; -> n, the shortest prefix with c_n >= p * total
__device__ __forceinline__ int nucleus_prefix(const float* lp, int k, float inv_temp, float p) {
  const float l0 = lp[0];
  float tot = 0.f;
  for (int j = 0; j < k; ++j) tot += expf((lp[j] - l0) * inv_temp);
  const float target = p * tot;
  float c = 0.f;
  for (int j = 0; j < k; ++j) {
    c += expf((lp[j] - l0) * inv_temp);
    if (c >= target) return j + 1;
  }
  return k;
}
// step 3: order[0..n) lists the members by ascending token id; the first whose running weight exceeds u * sum (the last if none)
__device__ __forceinline__ int nucleus_draw(const float* lp, const int* order, int n, float inv_temp, float u) {
  const float l0 = lp[0];
  float sum = 0.f;
  for (int r = 0; r < n; ++r) sum += expf((lp[order[r]] - l0) * inv_temp);
  const float t = u * sum;
  float c = 0.f;
  for (int r = 0; r < n; ++r) {
    c += expf((lp[order[r]] - l0) * inv_temp);
    if (t < c) return order[r];
  }
  return order[n - 1];
}
__device__ __forceinline__ float sample_args_u(const SampleArgs& a, int row) {
  const uint32_t r = a.row_ids ? (uint32_t)a.row_ids[row] : (uint32_t)row;
  const uint32_t step = a.step_dev ? (uint32_t)(*a.step_dev + 1) : (uint32_t)a.step;     // (captured: the counter holds i - 1)
  return tell_sample_u(*a.seed_dev, r, step);
}
// the workgroup's form over candidates ranked in LDS: thread 0 cuts the prefix, n threads rank the members by id, thread 0 draws
__device__ __forceinline__ void nucleus_candidates_block(const float* sort_v, const int* sort_i, int* order, int* n_s, int row,
                                                         const SampleArgs& a) {
  const int tid = threadIdx.x;
  if (tid == 0) *n_s = nucleus_prefix(sort_v, a.k, a.inv_temp, a.topp);
  __syncthreads();
  const int n = *n_s;
  if (tid < n) {
    const int mi = sort_i[tid];
    int r = 0;
    for (int j = 0; j < n; ++j) r += sort_i[j] < mi ? 1 : 0;
    order[r] = tid;
  }
  __syncthreads();
  if (tid == 0) {
    const int j = nucleus_draw(sort_v, order, n, a.inv_temp, sample_args_u(a, row));
    a.tokens[row] = sort_i[j];
    a.lps[row] = sort_v[j];
    if (a.nuc_size) a.nuc_size[row] = n;
    if (a.nuc_key) a.nuc_key[row] = lp_key(sort_v[n - 1]);
  }
}
// one radix pass's decision (hist complete after the first barrier): the digit whose bin holds the need-th largest of the
// counted values, how many lie in the bins above it and how many in the bin itself.  Wave 0 decides, everyone reads.
__device__ __forceinline__ void sample_radix_decide(SampleSmem& sm, int need, int& d, int& above, int& count) {
  __syncthreads();
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const int h[4] = {sm.hist[4 * lane], sm.hist[4 * lane + 1], sm.hist[4 * lane + 2], sm.hist[4 * lane + 3]};
    const int tot = h[0] + h[1] + h[2] + h[3];
    int suf = tot;                                            // sum over lanes >= lane (higher digits)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_down(suf, o, 64);
      if (lane + o < 64) suf += v;
    }
    int cum = suf - tot;
#pragma unroll
    for (int b = 3; b >= 0; --b) {
      if (cum < need && cum + h[b] >= need) { sm.sel = 4 * lane + b; sm.above = cum; sm.count = h[b]; }
      cum += h[b];
    }
  }
  __syncthreads();
  d = sm.sel; above = sm.above; count = sm.count;
}
// the need-th largest value v among the elements for which val(key, idx, ref, v) holds, digits from bit top_shift + 7 down
// (higher bits of v must be equal for all participants); on return need = how many elements equal to the result it takes,
// count = how many there are.  ref = sm.ref, loaded after each pass's barrier: a filter on a register value would be
// loop-invariant, and the compiler hoists the 64 per-element masks / values of the register form out of the pass loop
// (54 VGPRs and 117 SGPRs spilled); the caller sets sm.ref before the call.
template <class Each, class Val>
__device__ __forceinline__ uint32_t sample_radix_select(const Each& each, const Val& val, int top_shift, int& need, int& count,
                                                        SampleSmem& sm) {
  uint32_t pre = 0, msk = 0;
  for (int sh = top_shift; sh >= 0; sh -= 8) {
    if (threadIdx.x < 256) sm.hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t ref = sm.ref;
    each([&](uint32_t key, int idx) {
      uint32_t v;
      if (val(key, idx, ref, v) && (v & msk) == pre) atomicAdd(&sm.hist[(v >> sh) & 255], 1);
    });
    int d, above;
    sample_radix_decide(sm, need, d, above, count);
    pre |= (uint32_t)d << sh;
    msk |= 0xFFu << sh;
    need -= above;
  }
  return pre;
}
// each_ties: the same elements with the same keys, for the tie pass (3) only - the register form hands in a walk over memory
// there, because ids kept live through the pass loop spill half of its registers
template <bool NUC, class Each, class EachTies>
__device__ __forceinline__ void sample_row(const Each& each, const EachTies& each_ties, uint32_t thread_max, int row,
                                           const SampleArgs& a, SampleSmem& sm) {
  const int tid = threadIdx.x, k = a.k;
  int need = k, count = 0;
  // 1. tau: the k-th largest per-thread maximum
  const uint32_t tau = sample_radix_select([&](auto f) { f(thread_max, 0); },
                                          [](uint32_t key, int, uint32_t, uint32_t& v) { v = key; return true; }, 24, need,
                                          count, sm);
  // 2. the k-th largest key
  need = k;
  if (tid == 0) sm.ref = tau;
  const uint32_t kth = sample_radix_select(
      each, [](uint32_t key, int, uint32_t ref, uint32_t& v) { v = key; return key >= ref; }, 24, need, count, sm);
  // 3. more ties at kth than places left: the `need` lowest ids among them (largest 0xFFFFFF - id; `key ^ ref` is 0 for a
  //    participant and keeps the value inside the pass)
  int last = 0xFFFFFF;
  if (count > need) {                                         // (uniform)
    if (tid == 0) sm.ref = kth;
    const uint32_t inv = sample_radix_select(
        each_ties,
        [](uint32_t key, int idx, uint32_t ref, uint32_t& v) {
          v = (key ^ ref) | (0xFFFFFFu - (uint32_t)idx);
          return key == ref;
        },
        16, need, count, sm);
    last = 0xFFFFFF - (int)inv;
  }
  // 4. compact the k winners, rank them, draw
  if (tid == 0) sm.n_cand = 0;
  __syncthreads();
  each([&](uint32_t key, int idx) {
    if (key > kth || (key == kth && idx <= last)) {
      const int s = atomicAdd(&sm.n_cand, 1);
      if (s < 64) { sm.cand_key[s] = key; sm.cand_idx[s] = idx; }
    }
  });
  __syncthreads();
  if (tid < k) {
    const uint32_t mk = sm.cand_key[tid];
    const int mi = sm.cand_idx[tid];
    int rank = 0;
    for (int j = 0; j < k; ++j) {
      const uint32_t ok = sm.cand_key[j];
      rank += (ok > mk || (ok == mk && sm.cand_idx[j] < mi)) ? 1 : 0;
    }
    sm.sort_v[rank] = key_lp(mk);
    sm.sort_i[rank] = mi;
  }
  __syncthreads();
  if (NUC) {                                                  // top-k cut, then the nucleus over the k candidates (below)
    nucleus_candidates_block(sm.sort_v, sm.sort_i, sm.cand_idx, &sm.n_cand, row, a);
    return;
  }
  if (tid == 0) {
    const uint32_t r = a.row_ids ? (uint32_t)a.row_ids[row] : (uint32_t)row;
    const uint32_t step = a.step_dev ? (uint32_t)(*a.step_dev + 1) : (uint32_t)a.step;   // (captured: the counter holds i - 1)
    const float u = tell_sample_u(*a.seed_dev, r, step);
    const int j = tell_sample_pick(sm.sort_v, k, a.inv_temp, u);
    a.tokens[row] = sm.sort_i[j];
    a.lps[row] = sm.sort_v[j];
  }
}
// The register-resident form: loads, maxima, sums and log-probs exactly as logprob_regs_kernel (so k = 1 is its arg-max bit
// for bit), then the log-probs become keys in place and every pass of the select runs over registers.  Same capacity and
// alignment rules.
// PEN (tell_adaptive_logprob_sample_penalised): the penalty list is staged like the top-k kernels' (pen_stage) and a listed
// token's log-prob becomes its score where the keys are formed - one bit test per element; the select, sample_row, is untouched.
// (the list arguments are a parameter pack that is empty without PEN: the unpenalised instantiations keep their signature,
//  their kernel-argument layout and with them their code)
template <bool NUC, bool PEN = false, class... P>
__global__ __launch_bounds__(1024) void logprob_sample_regs_kernel(LogProbArgs p, SampleArgs a, P... pa_) {
  const auto& pa = pen_pick(pa_...);
  __shared__ float red[4][16];
  __shared__ SampleSmem sm;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nseg = 1 + p.n_tails;
  const float* rowp[4]; int n[4];
  rowp[0] = p.head + (long)i * p.ld_head; n[0] = p.head_n;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    rowp[c + 1] = c < p.n_tails ? p.tail[c] + (long)i * p.ld_tail[c] : rowp[0];
    n[c + 1] = c < p.n_tails ? p.tail_n[c] : 0;
  }
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 x[16];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int q = 0; q < LPF_CAP[s]; ++q) {
      const int j = (q * 1024 + tid) * 4;
      f4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (j + 3 < n[s]) v = *reinterpret_cast<const f4*>(rowp[s] + j);
      else if (j < n[s]) {
        v.x = rowp[s][j];
        if (j + 1 < n[s]) v.y = rowp[s][j + 1];
        if (j + 2 < n[s]) v.z = rowp[s][j + 2];
      }
      x[LPF_OFF[s] + q] = v;
    }
  int np = 0;
  if constexpr (PEN) {
    np = pen_count(pa, i);
    if (np > 0) pen_stage<1024>(pa, i, np);              // (np is uniform over the workgroup)
  }
  // MSK (tell_adaptive_logprob_sample_masked): the mask row is staged like the top-k kernels' (mask_stage) and a masked token's
  // key becomes 0, the key of an element outside the row, where the keys are formed (in: the element is a token of the row)
  constexpr bool MSK = IsMask<P...>::value;
  if constexpr (MSK) mask_stage<1024>(pa, i);
  // a listed token's log-prob -> its score (in: the element is a token of the row)
  auto pen = [&](float l, int idx, bool in) {
    if constexpr (PEN) {
      if (np > 0 && in && pen_bit(idx)) return pen_score(pa, np, idx, l);
    }
    return l;
  };
  float mx[4], sm_[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < LPF_CAP[s]; ++q) {
      const f4 v = x[LPF_OFF[s] + q];
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
      for (int q = 0; q < LPF_CAP[s]; ++q) {
        const f4 v = x[LPF_OFF[s] + q];
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
    sm_[s] = t;
  }
  const float lse_h = mx[0] + __logf(sm_[0]);
  float off[4];
  int base[4];
  off[0] = -lse_h; base[0] = 0;
  base[1] = p.c0;
#pragma unroll
  for (int s = 1; s < 4; ++s) {
    off[s] = s < nseg ? (rowp[0][p.c0 + s - 1] - lse_h) - (mx[s] + __logf(sm_[s])) : 0.f;
    if (s < 3) base[s + 1] = base[s] + n[s];
  }
  const int lim[4] = {p.c0, n[1], n[2], n[3]};               // (segments past n_tails have n = 0)
  uint32_t key[64];
  uint32_t tmax = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int q = 0; q < LPF_CAP[s]; ++q) {
      const int j = (q * 1024 + tid) * 4, e0 = (LPF_OFF[s] + q) * 4;
      const f4 v = x[LPF_OFF[s] + q];
      // head: v - lse_h (the argmax kernels' `x - lse_h`); tails: v + off
      const float l0 = s == 0 ? v.x - lse_h : v.x + off[s], l1 = s == 0 ? v.y - lse_h : v.y + off[s];
      const float l2 = s == 0 ? v.z - lse_h : v.z + off[s], l3 = s == 0 ? v.w - lse_h : v.w + off[s];
      key[e0] = j < lim[s] ? lp_key(pen(l0, base[s] + j, j < lim[s])) : 0u;
      key[e0 + 1] = j + 1 < lim[s] ? lp_key(pen(l1, base[s] + j + 1, j + 1 < lim[s])) : 0u;
      key[e0 + 2] = j + 2 < lim[s] ? lp_key(pen(l2, base[s] + j + 2, j + 2 < lim[s])) : 0u;
      key[e0 + 3] = j + 3 < lim[s] ? lp_key(pen(l3, base[s] + j + 3, j + 3 < lim[s])) : 0u;
      if constexpr (!MSK) tmax = max(tmax, max(max(key[e0], key[e0 + 1]), max(key[e0 + 2], key[e0 + 3])));
    }
  if constexpr (MSK) {                                        // (a pass of its own: the logits are dead by now)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int q = 0; q < LPF_CAP[s]; ++q) {
        const int j = (q * 1024 + tid) * 4, e0 = (LPF_OFF[s] + q) * 4;
        if (j < lim[s]) {                                     // (4 consecutive ids: at most two words of the bitmap)
          const int t0 = base[s] + j;
          const unsigned w0 = ban_bits[t0 >> 5], w1 = ban_bits[min(t0 + 3, pa.vocab - 1) >> 5];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int t = t0 + e;
            const unsigned w = (t >> 5) == (t0 >> 5) ? w0 : w1;
            if (j + e < lim[s] && ((w >> (t & 31)) & 1u)) key[e0 + e] = 0u;
          }
        }
        tmax = max(tmax, max(max(key[e0], key[e0 + 1]), max(key[e0 + 2], key[e0 + 3])));
      }
  }
  auto each = [&](auto f) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int q = 0; q < LPF_CAP[s]; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) f(key[(LPF_OFF[s] + q) * 4 + e], base[s] + (q * 1024 + tid) * 4 + e);
  };
  auto each_mem = [&](auto f) {                               // (the same keys: the same operations on the same logits)
    for (int j = tid; j < p.c0; j += 1024) f(lp_key(pen(rowp[0][j] - lse_h, j, true)), j);
    for (int s = 1; s < nseg; ++s)
      for (int j = tid; j < n[s]; j += 1024) f(lp_key(pen(rowp[s][j] + off[s], base[s] + j, true)), base[s] + j);
  };
  if constexpr (MSK) {                                        // (the tie pass over memory: the same keys, masked alike)
    auto each_mem_masked = [&](auto f) {
      each_mem([&](uint32_t key_, int idx) { f(pen_bit(idx) ? 0u : key_, idx); });
    };
    sample_row<NUC>(each, each_mem_masked, tmax, i, a, sm);
  } else {
    sample_row<NUC>(each, each_mem, tmax, i, a, sm);
  }
}
// Any row: the log-probs with the arithmetic of logprob_argmax_kernel (the three-pass form; its full-row output is what the
// tests take top-k of), read from memory in every pass of the select.
template <bool NUC, bool PEN = false, class... P>
__global__ __launch_bounds__(1024) void logprob_sample_stream_kernel(LogProbArgs p, SampleArgs a, P... pa_) {
  const auto& pa = pen_pick(pa_...);
  __shared__ float red[16];
  __shared__ SampleSmem sm;
  const int i = blockIdx.x, tid = threadIdx.x;
  const float* hrow = p.head + (long)i * p.ld_head;
  float mx = -INFINITY;
#pragma unroll 4
  for (int j = tid; j < p.head_n; j += 1024) mx = fmaxf(mx, hrow[j]);
  mx = block_max(mx, red);
  float s = 0.f;
#pragma unroll 4
  for (int j = tid; j < p.head_n; j += 1024) s += __expf(hrow[j] - mx);
  s = block_sum(s, red);
  const float lse_h = mx + __logf(s);
  float off[3] = {0.f, 0.f, 0.f};
  for (int c = 0; c < p.n_tails; ++c) {
    const float* trow = p.tail[c] + (long)i * p.ld_tail[c];
    const int n = p.tail_n[c];
    float m2 = -INFINITY;
#pragma unroll 4
    for (int j = tid; j < n; j += 1024) m2 = fmaxf(m2, trow[j]);
    m2 = block_max(m2, red);
    float s2 = 0.f;
#pragma unroll 4
    for (int j = tid; j < n; j += 1024) s2 += __expf(trow[j] - m2);
    s2 = block_sum(s2, red);
    off[c] = (hrow[p.c0 + c] - lse_h) - (m2 + __logf(s2));
  }
  if constexpr (IsMask<P...>::value) {                        // masked: a set bit -> the key of an element outside the row
    mask_stage<1024>(pa, i);
    auto msk = [&](uint32_t key, int idx) { return pen_bit(idx) ? 0u : key; };
    auto each = [&](auto f) {
      for (int j = tid; j < p.c0; j += 1024) f(msk(lp_key(hrow[j] - lse_h), j), j);
      int base = p.c0;
      for (int c = 0; c < p.n_tails; ++c) {
        const float* trow = p.tail[c] + (long)i * p.ld_tail[c];
        for (int j = tid; j < p.tail_n[c]; j += 1024) f(msk(lp_key(trow[j] + off[c]), base + j), base + j);
        base += p.tail_n[c];
      }
    };
    uint32_t tmax = 0;
    each([&](uint32_t key, int) { tmax = max(tmax, key); });
    sample_row<NUC>(each, each, tmax, i, a, sm);
  } else if constexpr (!PEN) {                                // (the unpenalised kernel: the code it always was)
    auto each = [&](auto f) {
      for (int j = tid; j < p.c0; j += 1024) f(lp_key(hrow[j] - lse_h), j);
      int base = p.c0;
      for (int c = 0; c < p.n_tails; ++c) {
        const float* trow = p.tail[c] + (long)i * p.ld_tail[c];
        for (int j = tid; j < p.tail_n[c]; j += 1024) f(lp_key(trow[j] + off[c]), base + j);
        base += p.tail_n[c];
      }
    };
    uint32_t tmax = 0;
    each([&](uint32_t key, int) { tmax = max(tmax, key); });
    sample_row<NUC>(each, each, tmax, i, a, sm);
  } else {
    const int np = pen_count(pa, i);
    if (np > 0) pen_stage<1024>(pa, i, np);                   // (np is uniform over the workgroup)
    auto pen = [&](float l, int idx) { return np > 0 && pen_bit(idx) ? pen_score(pa, np, idx, l) : l; };
    auto each = [&](auto f) {
      for (int j = tid; j < p.c0; j += 1024) f(lp_key(pen(hrow[j] - lse_h, j)), j);
      int base = p.c0;
      for (int c = 0; c < p.n_tails; ++c) {
        const float* trow = p.tail[c] + (long)i * p.ld_tail[c];
        for (int j = tid; j < p.tail_n[c]; j += 1024) f(lp_key(pen(trow[j] + off[c], base + j)), base + j);
        base += p.tail_n[c];
      }
    };
    uint32_t tmax = 0;
    each([&](uint32_t key, int) { tmax = max(tmax, key); });
    sample_row<NUC>(each, each, tmax, i, a, sm);
  }
}
// The draw's arguments with every rule's field defined (topp = 0, nuc_size / nuc_key / typ_c = NULL): a launcher sets the
// fields of its own rule only.
static SampleArgs sample_args(int k, float inv_temp, const uint32_t* seed_dev, const int* row_ids, int step, const int* step_dev,
                              int* tokens, float* lps) {
  SampleArgs a{};
  a.k = k; a.inv_temp = inv_temp; a.seed_dev = seed_dev; a.row_ids = row_ids; a.step = step; a.step_dev = step_dev;
  a.tokens = tokens; a.lps = lps;
  return a;
}
extern "C" int tell_adaptive_logprob_sample(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                            int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                            int rows, int k, float inv_temp, const uint32_t* seed_dev, const int* row_ids,
                                            int step, const int* step_dev, int* tokens, float* lps, hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_sample: up to 3 tails");
  TELL_REQUIRE(k >= 1 && k <= 64, "logprob_sample: 1 <= k <= 64");
  TELL_REQUIRE(inv_temp > 0.f, "logprob_sample: inv_temp > 0");
  TELL_REQUIRE(seed_dev && tokens && lps, "logprob_sample: seed_dev, tokens and lps are required");
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  const long vocab = logits_vocab(lg);
  TELL_REQUIRE(vocab >= k && vocab < (1L << 24), "logprob_sample: k <= vocab < 2^24");
  if (rows <= 0) return TELL_OK;
  const LogProbArgs p = logprob_args(lg);
  const SampleArgs a = sample_args(k, inv_temp, seed_dev, row_ids, step, step_dev, tokens, lps);
  if (logits_regs(lg)) {
    hipLaunchKernelGGL(logprob_sample_regs_kernel<false>, dim3(rows), dim3(1024), 0, stream, p, a);
    return tell_check_launch("logprob_sample (registers)");
  }
  hipLaunchKernelGGL(logprob_sample_stream_kernel<false>, dim3(rows), dim3(1024), 0, stream, p, a);
  return tell_check_launch("logprob_sample");
}

// tell_adaptive_logprob_sample over penalised scores (include/tell_hip.h): the arguments of tell_adaptive_logprob_sample
// plus the penalty list of tell_adaptive_logprob_topk_penalised.
extern "C" int tell_adaptive_logprob_sample_penalised(const float* head, long ld_head, int c0, int n_tails, const float* tail0,
                                                      long ld0, int n0, const float* tail1, long ld1, int n1, const float* tail2,
                                                      long ld2, int n2, int rows, int k, float inv_temp, const uint32_t* seed_dev,
                                                      const int* row_ids, int step, const int* step_dev, const int* pen_tok,
                                                      const int* pen_cnt, long ld_pen, const int* n_pen, float theta,
                                                      const float* sub, int n_sub, int* tokens, float* lps, hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_sample_penalised: up to 3 tails");
  TELL_REQUIRE(k >= 1 && k <= 64, "logprob_sample_penalised: 1 <= k <= 64");
  TELL_REQUIRE(inv_temp > 0.f, "logprob_sample_penalised: inv_temp > 0");
  TELL_REQUIRE(seed_dev && tokens && lps, "logprob_sample_penalised: seed_dev, tokens and lps are required");
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  PenArgs pa;
  const int rc = pen_args(pa, lg, pen_tok, pen_cnt, ld_pen, n_pen, theta, sub, n_sub);
  if (rc != TELL_OK) return rc;
  TELL_REQUIRE(pa.vocab >= k, "logprob_sample_penalised: k <= vocab");
  if (rows <= 0) return TELL_OK;
  const LogProbArgs p = logprob_args(lg);
  const SampleArgs a = sample_args(k, inv_temp, seed_dev, row_ids, step, step_dev, tokens, lps);
  const size_t lds = pen_lds(pa);
  if (logits_regs(lg)) {
    hipLaunchKernelGGL((logprob_sample_regs_kernel<false, true>), dim3(rows), dim3(1024), lds, stream, p, a, pa);
    return tell_check_launch("logprob_sample_penalised (registers)");
  }
  hipLaunchKernelGGL((logprob_sample_stream_kernel<false, true>), dim3(rows), dim3(1024), lds, stream, p, a, pa);
  return tell_check_launch("logprob_sample_penalised");
}

// tell_adaptive_logprob_sample under a vocabulary mask (include/tell_hip.h): the arguments of tell_adaptive_logprob_sample plus
// the mask of tell_adaptive_logprob_topk_masked (no ban list).
extern "C" int tell_adaptive_logprob_sample_masked(const float* head, long ld_head, int c0, int n_tails, const float* tail0,
                                                   long ld0, int n0, const float* tail1, long ld1, int n1, const float* tail2,
                                                   long ld2, int n2, int rows, int k, float inv_temp, const uint32_t* seed_dev,
                                                   const int* row_ids, int step, const int* step_dev, const uint32_t* mask,
                                                   long ld_mask, int per, int* tokens, float* lps, hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_sample_masked: up to 3 tails");
  TELL_REQUIRE(k >= 1 && k <= 64, "logprob_sample_masked: 1 <= k <= 64");
  TELL_REQUIRE(inv_temp > 0.f, "logprob_sample_masked: inv_temp > 0");
  TELL_REQUIRE(seed_dev && tokens && lps, "logprob_sample_masked: seed_dev, tokens and lps are required");
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  MaskArgs ma;
  const int rc = mask_args(ma, lg, mask, ld_mask, per, nullptr, 0, nullptr);
  if (rc != TELL_OK) return rc;
  TELL_REQUIRE(ma.vocab >= k, "logprob_sample_masked: k <= vocab");
  if (rows <= 0) return TELL_OK;
  const LogProbArgs p = logprob_args(lg);
  const SampleArgs a = sample_args(k, inv_temp, seed_dev, row_ids, step, step_dev, tokens, lps);
  const size_t lds = bitmap_lds(ma.vocab);
  if (logits_regs(lg)) {
    hipLaunchKernelGGL((logprob_sample_regs_kernel<false, false>), dim3(rows), dim3(1024), lds, stream, p, a, ma);
    return tell_check_launch("logprob_sample_masked (registers)");
  }
  hipLaunchKernelGGL((logprob_sample_stream_kernel<false, false>), dim3(rows), dim3(1024), lds, stream, p, a, ma);
  return tell_check_launch("logprob_sample_masked");
}

// steps 2-5 of the sampling semantics on given candidates (sorted best first): one thread per row
__global__ __launch_bounds__(256) void sample_candidates_kernel(const int* __restrict__ cand_tokens,
                                                                const float* __restrict__ cand_lps, int rows, SampleArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const uint32_t row = a.row_ids ? (uint32_t)a.row_ids[r] : (uint32_t)r;
  const uint32_t step = a.step_dev ? (uint32_t)(*a.step_dev + 1) : (uint32_t)a.step;
  const float u = tell_sample_u(*a.seed_dev, row, step);
  const int j = tell_sample_pick(cand_lps + (long)r * a.k, a.k, a.inv_temp, u);
  a.tokens[r] = cand_tokens[(long)r * a.k + j];
  a.lps[r] = cand_lps[(long)r * a.k + j];
}
extern "C" int tell_sample_candidates(const int* cand_tokens, const float* cand_lps, int rows, int k, float inv_temp,
                                      const uint32_t* seed_dev, const int* row_ids, int step, const int* step_dev, int* tokens,
                                      float* lps, hipStream_t stream) {
  TELL_REQUIRE(k >= 1 && k <= 64, "sample_candidates: 1 <= k <= 64");
  TELL_REQUIRE(inv_temp > 0.f, "sample_candidates: inv_temp > 0");
  TELL_REQUIRE(seed_dev && cand_tokens && cand_lps && tokens && lps, "sample_candidates: null pointer");
  if (rows <= 0) return TELL_OK;
  SampleArgs a;
  a.k = k; a.inv_temp = inv_temp; a.seed_dev = seed_dev; a.row_ids = row_ids; a.step = step; a.step_dev = step_dev;
  a.tokens = tokens; a.lps = lps; a.topp = 0.f; a.nuc_size = nullptr; a.nuc_key = nullptr;
  hipLaunchKernelGGL(sample_candidates_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, cand_tokens, cand_lps, rows, a);
  return tell_check_launch("sample_candidates");
}

// ------------------------------------------------------------------ nucleus (top-p) sampling with a temperature
// include/tell_hip.h tell_adaptive_logprob_nucleus, DESIGN.md section 14.  Per row, with the log-probs and keys of the top-k
// sampler above: weights w = exp((lp - lp_max) * inv_temp); the nucleus is the shortest prefix, by (value descending, id
// ascending), whose weight reaches p * total; the pick is the first member IN TOKEN-ID ORDER whose running weight exceeds
// u * (nucleus weight).  No sort: the boundary is the key tau with mass(key > tau) < p * total <= mass(key >= tau), found by
// a threshold search over weight-mass histograms -
//  1. one pass over a coarse, well spread digit (quarter nats below the maximum after the temperature, nuc_coarse: monotone
//     in the key).  The raw key's top byte would put the whole vocabulary into two or three exponent bins, i.e. 50 000 LDS
//     atomics on three addresses;
//  2. the crossing coarse bin is a key range klo .. khi (one pass of min / max); then passes of 8 key bits over the elements
//     of that range (typically a few hundred), skipping every byte that klo and khi share;
//  3. one pass in id order: `m`, the number of keys equal to tau that the prefix takes, go to the lowest ids (block-wide
//     prefix count, only when not all of them enter), and the running weight is a block-wide fp32 prefix sum in a fixed
//     order (thread, wave, workgroup, chunk), from which every thread tests its own elements.
// The histogram masses are 64-bit FIXED-POINT sums (weight * 2^44, truncated) added with integer LDS atomics: integer
// addition is associative, so a bin's mass does not depend on the order in which lanes arrive - no atomics on floats, and
// the same row gives the same tau in any batch, eager or captured.  A weight below 2^-44 of the maximum counts as zero
// (5.7e-14: below what fp32 sums of the other weights resolve); 2^19 tokens of weight 1 still fit 63 bits.
// Every pass walks the row through `each` (registers or memory); `sweep` hands out the id-ordered chunks of pass 3.
#define NUC_FX 17592186044416.f                                 // 2^44
struct NucleusSmem {
  unsigned long long hist[256];
  unsigned long long need, above, bucket;                       // a pass's decision: target left, mass above the bin, the bin's mass
  float wtot[2][16];
  int ttot[2][16];
  int sel;
  uint32_t klo, khi;                                            // the keys of the crossing coarse bin span klo .. khi
  float ref_max;                                                // the row's maximum log-prob, re-read in every pass (see nucleus_row)
  int best, last, cnt;
  uint32_t tau;                                                 // the typical rule's boundary key, re-read in its id passes
};
__device__ __forceinline__ float nuc_weight(uint32_t key, float lmax, float inv_temp) {
  return __expf((key_lp(key) - lmax) * inv_temp);
}
__device__ __forceinline__ unsigned long long nuc_fx(float w) { return (unsigned long long)(w * NUC_FX); }
// 255 - quarter nats below the maximum (after the temperature), clamped: larger key -> larger or equal digit
__device__ __forceinline__ int nuc_coarse(uint32_t key, float lmax, float inv_temp) {
  return 255 - (int)fminf((lmax - key_lp(key)) * inv_temp * 4.f, 255.f);
}
// What a rule (nucleus, locally typical, min-p: DESIGN.md sections 14 and 19) makes of the 32-bit word a row element is held
// as (0 = not a token) and of the row's reference value `ref` (NucleusSmem::ref_max): the search key (larger = better), the
// weight, the coarse digit (monotone in the key) and the key as reported.  KIND picks the membership test of nucleus_draw_row.
struct NucleusRule {                                            // word = lp_key(lp); ref = the row's maximum log-prob
  static constexpr int KIND = 0;
  static __device__ __forceinline__ uint32_t cmp(uint32_t w) { return w; }
  static __device__ __forceinline__ float weight(uint32_t w, float ref, float inv_temp) { return nuc_weight(w, ref, inv_temp); }
  static __device__ __forceinline__ int coarse(uint32_t w, float ref, float inv_temp) { return nuc_coarse(w, ref, inv_temp); }
  static __device__ __forceinline__ uint32_t report(uint32_t tau) { return tau; }
};
// word = typ_word(x), x = a + c the token's surprise relative to the entropy (a = (lp - lp_max) * inv_temp, c = ref): bit 31
// the sign of x, bits 0..30 the inverted bits of d = |x| - a non-negative float orders as its bit pattern, inverted the
// smaller d is the larger key, and no d gives 0.  The weight exp(a) is recovered as exp(x - c).
__device__ __forceinline__ uint32_t typ_word(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) | (~u & 0x7fffffffu);
}
// a = (lp - lmax) * inv_temp and x = a + c, each operation rounded on its own: contraction is switched off here (the
// __fmul_rn / __fadd_rn of this toolchain are plain operators, which the compiler fuses into an FMA like any others), so
// that numpy float32 restates a and x bit for bit
__device__ __forceinline__ float typ_a(float lp, float lmax, float inv_temp) {
#pragma clang fp contract(off)
  const float s = lp - lmax;
  return s * inv_temp;
}
__device__ __forceinline__ float typ_x(float lp, float lmax, float inv_temp, float c) {
#pragma clang fp contract(off)
  const float s = lp - lmax;
  const float a = s * inv_temp;
  return a + c;
}
struct TypicalRule {
  static constexpr int KIND = 1;
  static __device__ __forceinline__ uint32_t cmp(uint32_t w) { return w & 0x7fffffffu; }
  static __device__ __forceinline__ float weight(uint32_t w, float ref, float) {
    return __expf(__uint_as_float((w & 0x80000000u) | (~w & 0x7fffffffu)) - ref);
  }
  static __device__ __forceinline__ int coarse(uint32_t w, float, float) {      // 255 - quarter nats of d, clamped
    return 255 - (int)fminf(__uint_as_float(~w & 0x7fffffffu) * 4.f, 255.f);
  }
  static __device__ __forceinline__ uint32_t report(uint32_t tau) { return tau | 0x80000000u; }     // ~bits(d)
};
struct MinpRule : NucleusRule {                                 // words and weights of the nucleus; tau = the bits of log_minp
  static constexpr int KIND = 2;
};
// hist complete after the first barrier; bins taken from 255 down: the bin in which the running mass reaches the target.
// topp > 0 (the first pass): the target is set here, ceil(topp * total mass), at least 1.  Wave 0 decides, everyone reads.
__device__ __forceinline__ void nucleus_decide(NucleusSmem& sm, float topp) {
  __syncthreads();
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const unsigned long long h[4] = {sm.hist[4 * lane], sm.hist[4 * lane + 1], sm.hist[4 * lane + 2], sm.hist[4 * lane + 3]};
    const unsigned long long tot = h[0] + h[1] + h[2] + h[3];
    unsigned long long suf = tot;                              // sum over lanes >= lane (higher digits)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long v = __shfl_down(suf, o, 64);
      if (lane + o < 64) suf += v;
    }
    unsigned long long need = sm.need;
    if (topp > 0.f) {
      const unsigned long long all = __shfl(suf, 0, 64);
      need = (unsigned long long)ceil((double)topp * (double)all);
      need = need < 1 ? 1 : (need > all ? all : need);
    }
    unsigned long long cum = suf - tot;
#pragma unroll
    for (int b = 3; b >= 0; --b) {
      if (cum < need && cum + h[b] >= need) { sm.sel = 4 * lane + b; sm.above = cum; sm.bucket = h[b]; sm.need = need - cum; }
      cum += h[b];
    }
  }
  __syncthreads();
}
// the row's maximum key from the threads' maxima; leaves hist zeroed and best / last / cnt / klo / khi reset (one barrier)
__device__ __forceinline__ uint32_t nucleus_row_max(uint32_t thread_max, NucleusSmem& sm) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t kmax = thread_max;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
  if (lane == 0) sm.ttot[0][wave] = (int)kmax;
  if (tid < 256) sm.hist[tid] = 0;
  if (tid == 0) { sm.best = 0x7fffffff; sm.last = -1; sm.cnt = 0; sm.klo = 0xFFFFFFFFu; sm.khi = 0u; }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 16; ++w) kmax = max(kmax, (uint32_t)sm.ttot[0][w]);
  return kmax;
}
// 3. id order, shared by the rules.  Members by KIND - nucleus: key > tau, and of the keys equal to tau all (!cut) or the m
// lowest ids; typical: the same on Rule::cmp with the ties up to id_cut; min-p: (lp - ref) * inv_temp >= the float whose bits
// tau holds.  The pick is the first member whose running weight exceeds t; lp_of(word, id) is its untempered log-prob.
template <class Rule, class Sweep, class LpOf>
__device__ __forceinline__ void nucleus_draw_row(const Sweep& sweep, const LpOf& lp_of, uint32_t tau, bool cut, int m, int id_cut,
                                                 float t, int row, const SampleArgs& a, NucleusSmem& sm) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv_temp = a.inv_temp;
  const float lmax = sm.ref_max;
  float carry = 0.f;
  int tie_carry = 0, par = 0;
  int best = 0x7fffffff, last = -1, cnt = 0;
  uint32_t best_key = 0, last_key = 0;
  sweep([&](uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3, int id0) {
    const uint32_t k[4] = {k0, k1, k2, k3};
    bool mem[4];
    if constexpr (Rule::KIND == 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) mem[e] = Rule::cmp(k[e]) > tau || (Rule::cmp(k[e]) == tau && id0 + e <= id_cut);
    } else if constexpr (Rule::KIND == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) mem[e] = k[e] != 0u && typ_a(key_lp(k[e]), lmax, inv_temp) >= __uint_as_float(tau);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) mem[e] = k[e] > tau || (!cut && k[e] == tau);
    }
    if (Rule::KIND == 0 && cut) {
      int tc = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) tc += k[e] == tau ? 1 : 0;
      int incl = tc;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      if (lane == 63) sm.ttot[par][wave] = incl;
      __syncthreads();
      int rank = tie_carry + incl - tc;
#pragma unroll
      for (int w = 0; w < 16; ++w) {
        const int v = sm.ttot[par][w];
        if (w < wave) rank += v;
        tie_carry += v;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k[e] == tau) { mem[e] = rank < m; ++rank; }
    }
    float s[4];
    float run = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      run += mem[e] ? Rule::weight(k[e], lmax, inv_temp) : 0.f;
      s[e] = run;
    }
    float incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.f;
    if (lane == 63) sm.wtot[par][wave] = incl;
    __syncthreads();
    float off = carry, c = carry;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      if (w == wave) off = c;
      c += sm.wtot[par][w];
    }
    carry = c;
    const float base = off + excl;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (mem[e]) {
        if (best == 0x7fffffff && base + s[e] > t) { best = id0 + e; best_key = k[e]; }
        last = id0 + e; last_key = k[e];
        ++cnt;
      }
    par ^= 1;
  });
  int wb = best, wl = last, wc = cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    wb = min(wb, __shfl_xor(wb, o, 64));
    wl = max(wl, __shfl_xor(wl, o, 64));
    wc += __shfl_xor(wc, o, 64);
  }
  if (lane == 0) { atomicMin(&sm.best, wb); atomicMax(&sm.last, wl); atomicAdd(&sm.cnt, wc); }
  __syncthreads();
  const int pick = sm.best != 0x7fffffff ? sm.best : sm.last;   // (no running sum above t: rounding at the top end - the last member)
  if (best == pick) { a.tokens[row] = pick; a.lps[row] = lp_of(best_key, pick); }
  else if (sm.best == 0x7fffffff && last == pick) { a.tokens[row] = pick; a.lps[row] = lp_of(last_key, pick); }
  if (tid == 0) {
    if (a.nuc_size) a.nuc_size[row] = sm.cnt;
    if (Rule::KIND != 2 && a.nuc_key) a.nuc_key[row] = Rule::report(tau);
  }
}
// steps 1-3 after nucleus_row_max: `ref` is the rule's reference value (the maximum log-prob; the typical rule's c), a.topp
// the share of the total mass to reach.  `each` hands out (word, token id) - the id is only read by the typical rule.
template <class Rule, class Each, class Sweep, class LpOf>
__device__ __forceinline__ void nucleus_search_row(const Each& each, const Sweep& sweep, const LpOf& lp_of, float ref, int row,
                                                   const SampleArgs& a, NucleusSmem& sm) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv_temp = a.inv_temp;
  // 1. the coarse digit over the whole row
  {
    const float lmax = ref;
    if (tid == 0) sm.ref_max = lmax;
    each([&](uint32_t key, int) {
      const unsigned long long fx = key ? nuc_fx(Rule::weight(key, lmax, inv_temp)) : 0ull;
      if (fx) atomicAdd(&sm.hist[Rule::coarse(key, lmax, inv_temp)], fx);        // (a peaked row: most of the vocabulary is 0)
    });
  }
  nucleus_decide(sm, a.topp);
  unsigned long long above = sm.above;
  // the crossing coarse bin is a key range (the digit is monotone in the key): klo .. khi, the bin's smallest and largest key
  {
    const int g = sm.sel;
    const float lmax = sm.ref_max;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    each([&](uint32_t key, int) {
      if (key && Rule::coarse(key, lmax, inv_temp) == g) { lo = min(lo, Rule::cmp(key)); hi = max(hi, Rule::cmp(key)); }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
      hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, 64));
    }
    if (lane == 0) { atomicMin(&sm.klo, lo); atomicMax(&sm.khi, hi); }
    __syncthreads();
  }
  // 2. the key's bytes inside that range.  A byte that klo and khi share (with all bytes above it) is the same in every
  //    participant: its pass is skipped - typically the top byte (a quarter nat rarely spans two exponents), often
  //    the next.  klo / khi / ref_max are re-read from LDS in every pass: filters and weights computed from register values
  //    are loop-invariant, and the compiler would keep 64 of each per thread of the register form live across the passes
  //    (293 VGPRs spilled).
  uint32_t pre = 0, msk = 0;
  for (int sh = 24; sh >= 0; sh -= 8) {
    if (((sm.klo ^ sm.khi) >> sh) == 0) {                        // (uniform)
      pre |= sm.klo & (0xFFu << sh);
      msk |= 0xFFu << sh;
      continue;
    }
    if (tid < 256) sm.hist[tid] = 0;
    __syncthreads();
    const uint32_t klo = sm.klo, khi = sm.khi;
    const float lmax = sm.ref_max;
    each([&](uint32_t word, int) {
      const uint32_t key = Rule::cmp(word);
      if (key >= klo && key <= khi && (key & msk) == pre) {
        const unsigned long long fx = nuc_fx(Rule::weight(word, lmax, inv_temp));
        if (fx) atomicAdd(&sm.hist[(key >> sh) & 255], fx);
      }
    });
    nucleus_decide(sm, 0.f);
    pre |= (uint32_t)sm.sel << sh;
    msk |= 0xFFu << sh;
    above += sm.above;
  }
  const uint32_t tau = pre;
  if constexpr (Rule::KIND == 1) {
    // the tokens at distance tau need not weigh the same (x = +d and x = -d), so the ties are not counted off: when there
    // are several, the mass target left inside them picks the id up to which they enter - three more passes, over the
    // digits of 2^19 - 1 - id (lower ids first), with the same masses and the same decision
    if (tid == 0) sm.tau = tau;
    int tc = 0;
    each([&](uint32_t word, int) { tc += Rule::cmp(word) == tau ? 1 : 0; });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tc += __shfl_xor(tc, o, 64);
    if (lane == 0) sm.ttot[0][wave] = tc;
    __syncthreads();
    int ties = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) ties += sm.ttot[0][w];
    unsigned long long mass = above + sm.bucket;
    int id_cut = 0x7fffffff;
    if (ties > 1) {                                             // (uniform)
      mass = above;
      uint32_t ipre = 0, imsk = 0;
      for (int sh = 16; sh >= 0; sh -= 8) {
        if (tid < 256) sm.hist[tid] = 0;
        __syncthreads();
        const uint32_t tv = sm.tau;
        const float c = sm.ref_max;
        each([&](uint32_t word, int id) {
          const uint32_t inv = 0x7FFFFu - (uint32_t)id;
          if (Rule::cmp(word) == tv && (inv & imsk) == ipre) {
            const unsigned long long fx = nuc_fx(Rule::weight(word, c, inv_temp));
            if (fx) atomicAdd(&sm.hist[(inv >> sh) & 255], fx);
          }
        });
        nucleus_decide(sm, 0.f);
        ipre |= (uint32_t)sm.sel << sh;
        imsk |= 0xFFu << sh;
        mass += sm.above;
      }
      mass += sm.bucket;                                        // (the last bin holds one token: the last tie to enter)
      id_cut = 0x7FFFF - (int)ipre;
    }
    const float t = sample_args_u(a, row) * ((float)mass * (1.f / NUC_FX));
    nucleus_draw_row<Rule>(sweep, lp_of, tau, false, 0, id_cut, t, row, a, sm);
  } else {
    // tau = pre: `ties` keys equal it, the prefix takes the m lowest ids of them
    const float lmax = sm.ref_max;
    const unsigned long long fx_tau = nuc_fx(Rule::weight(tau, lmax, inv_temp));   // (> 0: its bin reached a target >= 1)
    const int ties = (int)(sm.bucket / fx_tau);
    int m = (int)((sm.need + fx_tau - 1) / fx_tau);
    m = m > ties ? ties : m;
    const bool cut = m < ties;                                   // (uniform)
    const float t = sample_args_u(a, row) * ((float)(above + (unsigned long long)m * fx_tau) * (1.f / NUC_FX));
    nucleus_draw_row<Rule>(sweep, lp_of, tau, cut, m, 0, t, row, a, sm);
  }
}
template <class Each, class Sweep>
__device__ __forceinline__ void nucleus_row(const Each& each, const Sweep& sweep, uint32_t thread_max, int row,
                                            const SampleArgs& a, NucleusSmem& sm) {
  const uint32_t kmax = nucleus_row_max(thread_max, sm);
  nucleus_search_row<NucleusRule>(each, sweep, [](uint32_t key, int) { return key_lp(key); }, key_lp(kmax), row, a, sm);
}
// min-p (tell_adaptive_logprob_minp): the maximum, the members' mass, the id-order draw; a.topp is log_minp
template <class Each, class Sweep>
__device__ __forceinline__ void minp_row(const Each& each, const Sweep& sweep, uint32_t thread_max, int row,
                                         const SampleArgs& a, NucleusSmem& sm) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float lmax = key_lp(nucleus_row_max(thread_max, sm));
  if (tid == 0) sm.ref_max = lmax;                              // (the draw re-reads it: see nucleus_search_row, 2.)
  const float inv_temp = a.inv_temp, thr = a.topp;
  unsigned long long mass = 0;
  each([&](uint32_t key, int) {
    if (key && typ_a(key_lp(key), lmax, inv_temp) >= thr) mass += nuc_fx(nuc_weight(key, lmax, inv_temp));
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mass += __shfl_xor(mass, o, 64);
  if (lane == 0) sm.hist[wave] = mass;
  __syncthreads();
  unsigned long long all = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) all += sm.hist[w];               // (>= 2^44: the best token weighs 1)
  const float t = sample_args_u(a, row) * ((float)all * (1.f / NUC_FX));
  nucleus_draw_row<MinpRule>(sweep, [](uint32_t key, int) { return key_lp(key); }, __float_as_uint(thr), false, 0, 0, t, row,
                             a, sm);
}
// locally typical (tell_adaptive_logprob_typical), after nucleus_row_max: W and S over the row's lp keys in a fixed order,
// -> c.  red: 2 x 16 floats.
template <class Each>
__device__ __forceinline__ float typical_c(const Each& each, float lmax, float inv_temp, float (*red)[16]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float W = 0.f, S = 0.f;
  each([&](uint32_t key, int) {
    if (key) {
      const float x = typ_a(key_lp(key), lmax, inv_temp), w = __expf(x);
      W += w;
      S += w * x;
    }
  });
  W = wave_sum(W);
  S = wave_sum(S);
  if (lane == 0) { red[0][wave] = W; red[1][wave] = S; }
  __syncthreads();
  W = 0.f; S = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) { W += red[0][w]; S += red[1][w]; }
  return S < 0.f ? -S / W : 0.f;
}
// The register-resident form: loads, maxima, sums and log-probs exactly as logprob_regs_kernel / logprob_sample_regs_kernel
// (a tiny p is the register arg-max bit for bit); every pass runs over registers, the logits cross HBM once.
// RULE 0: the nucleus; 1: locally typical - the lp keys are overwritten with the words of TypicalRule, and the picking
// thread recovers lp from its one logit in memory with the arithmetic that formed the key; 2: min-p.
template <int RULE>
__global__ __launch_bounds__(1024) void logprob_nucleus_regs_kernel(LogProbArgs p, SampleArgs a) {
  __shared__ float red[4][16];
  __shared__ NucleusSmem sm;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nseg = 1 + p.n_tails;
  const float* rowp[4]; int n[4];
  rowp[0] = p.head + (long)i * p.ld_head; n[0] = p.head_n;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    rowp[c + 1] = c < p.n_tails ? p.tail[c] + (long)i * p.ld_tail[c] : rowp[0];
    n[c + 1] = c < p.n_tails ? p.tail_n[c] : 0;
  }
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 x[16];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int q = 0; q < LPF_CAP[s]; ++q) {
      const int j = (q * 1024 + tid) * 4;
      f4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (j + 3 < n[s]) v = *reinterpret_cast<const f4*>(rowp[s] + j);
      else if (j < n[s]) {
        v.x = rowp[s][j];
        if (j + 1 < n[s]) v.y = rowp[s][j + 1];
        if (j + 2 < n[s]) v.z = rowp[s][j + 2];
      }
      x[LPF_OFF[s] + q] = v;
    }
  float mx[4], sm_[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < LPF_CAP[s]; ++q) {
      const f4 v = x[LPF_OFF[s] + q];
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
      for (int q = 0; q < LPF_CAP[s]; ++q) {
        const f4 v = x[LPF_OFF[s] + q];
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
    sm_[s] = t;
  }
  const float lse_h = mx[0] + __logf(sm_[0]);
  float off[4];
  int base[4];
  off[0] = -lse_h; base[0] = 0;
  base[1] = p.c0;
#pragma unroll
  for (int s = 1; s < 4; ++s) {
    off[s] = s < nseg ? (rowp[0][p.c0 + s - 1] - lse_h) - (mx[s] + __logf(sm_[s])) : 0.f;
    if (s < 3) base[s + 1] = base[s] + n[s];
  }
  const int lim[4] = {p.c0, n[1], n[2], n[3]};               // (segments past n_tails have n = 0)
  uint32_t key[64];
  uint32_t tmax = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int q = 0; q < LPF_CAP[s]; ++q) {
      const int j = (q * 1024 + tid) * 4, e0 = (LPF_OFF[s] + q) * 4;
      const f4 v = x[LPF_OFF[s] + q];
      const float l0 = s == 0 ? v.x - lse_h : v.x + off[s], l1 = s == 0 ? v.y - lse_h : v.y + off[s];
      const float l2 = s == 0 ? v.z - lse_h : v.z + off[s], l3 = s == 0 ? v.w - lse_h : v.w + off[s];
      key[e0] = j < lim[s] ? lp_key(l0) : 0u;
      key[e0 + 1] = j + 1 < lim[s] ? lp_key(l1) : 0u;
      key[e0 + 2] = j + 2 < lim[s] ? lp_key(l2) : 0u;
      key[e0 + 3] = j + 3 < lim[s] ? lp_key(l3) : 0u;
      tmax = max(tmax, max(max(key[e0], key[e0 + 1]), max(key[e0 + 2], key[e0 + 3])));
    }
  auto each = [&](auto f) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int q = 0; q < LPF_CAP[s]; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) f(key[(LPF_OFF[s] + q) * 4 + e], base[s] + (q * 1024 + tid) * 4 + e);
  };
  auto sweep = [&](auto chunk) {                              // chunk (s, q): ids base[s] + q * 4096 .. + 4095, four per thread
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int q = 0; q < LPF_CAP[s]; ++q)
        if (q * 4096 < lim[s]) {                              // (uniform)
          const int e0 = (LPF_OFF[s] + q) * 4;
          chunk(key[e0], key[e0 + 1], key[e0 + 2], key[e0 + 3], base[s] + (q * 1024 + tid) * 4);
        }
  };
  if constexpr (RULE == 0) nucleus_row(each, sweep, tmax, i, a, sm);
  else if constexpr (RULE == 2) minp_row(each, sweep, tmax, i, a, sm);
  else {
    const float lmax = key_lp(nucleus_row_max(tmax, sm));
    if (tid == 0) sm.ref_max = lmax;
    const float c = typical_c(each, lmax, a.inv_temp, red);
    const float lm2 = sm.ref_max;                             // (from LDS: the a of typical_c must not stay live, see nucleus_search_row)
#pragma unroll
    for (int e = 0; e < 64; ++e) key[e] = key[e] ? typ_word(typ_x(key_lp(key[e]), lm2, a.inv_temp, c)) : 0u;
    if (tid == 0 && a.typ_c) a.typ_c[i] = c;
    __syncthreads();
    auto lp_of = [&](uint32_t, int id) {
      float v = rowp[0][id < p.c0 ? id : 0] - lse_h;
#pragma unroll
      for (int s = 1; s < 4; ++s)
        if (id >= base[s] && id < base[s] + n[s]) v = rowp[s][id - base[s]] + off[s];
      return v;
    };
    nucleus_search_row<TypicalRule>(each, sweep, lp_of, c, i, a, sm);
  }
}
// Any row: the log-probs with the arithmetic of logprob_argmax_kernel, read from memory in every pass (a chunk of pass 3 is
// 1024 consecutive ids, one per thread).
template <int RULE>
__global__ __launch_bounds__(1024) void logprob_nucleus_stream_kernel(LogProbArgs p, SampleArgs a) {
  __shared__ float red[16];
  __shared__ NucleusSmem sm;
  const int i = blockIdx.x, tid = threadIdx.x;
  const float* hrow = p.head + (long)i * p.ld_head;
  float mx = -INFINITY;
#pragma unroll 4
  for (int j = tid; j < p.head_n; j += 1024) mx = fmaxf(mx, hrow[j]);
  mx = block_max(mx, red);
  float s = 0.f;
#pragma unroll 4
  for (int j = tid; j < p.head_n; j += 1024) s += __expf(hrow[j] - mx);
  s = block_sum(s, red);
  const float lse_h = mx + __logf(s);
  float off[3] = {0.f, 0.f, 0.f};
  for (int c = 0; c < p.n_tails; ++c) {
    const float* trow = p.tail[c] + (long)i * p.ld_tail[c];
    const int n = p.tail_n[c];
    float m2 = -INFINITY;
#pragma unroll 4
    for (int j = tid; j < n; j += 1024) m2 = fmaxf(m2, trow[j]);
    m2 = block_max(m2, red);
    float s2 = 0.f;
#pragma unroll 4
    for (int j = tid; j < n; j += 1024) s2 += __expf(trow[j] - m2);
    s2 = block_sum(s2, red);
    off[c] = (hrow[p.c0 + c] - lse_h) - (m2 + __logf(s2));
  }
  auto each = [&](auto f) {
    for (int j = tid; j < p.c0; j += 1024) f(lp_key(hrow[j] - lse_h), j);
    int base = p.c0;
    for (int c = 0; c < p.n_tails; ++c) {
      const float* trow = p.tail[c] + (long)i * p.ld_tail[c];
      for (int j = tid; j < p.tail_n[c]; j += 1024) f(lp_key(trow[j] + off[c]), base + j);
      base += p.tail_n[c];
    }
  };
  auto sweep = [&](auto chunk) {
    for (int j0 = 0; j0 < p.c0; j0 += 1024) {
      const int j = j0 + tid;
      chunk(j < p.c0 ? lp_key(hrow[j] - lse_h) : 0u, 0u, 0u, 0u, j);
    }
    int base = p.c0;
    for (int c = 0; c < p.n_tails; ++c) {
      const float* trow = p.tail[c] + (long)i * p.ld_tail[c];
      const int n = p.tail_n[c];
      for (int j0 = 0; j0 < n; j0 += 1024) {
        const int j = j0 + tid;
        chunk(j < n ? lp_key(trow[j] + off[c]) : 0u, 0u, 0u, 0u, base + j);
      }
      base += n;
    }
  };
  uint32_t tmax = 0;
  each([&](uint32_t key, int) { tmax = max(tmax, key); });
  if constexpr (RULE == 0) nucleus_row(each, sweep, tmax, i, a, sm);
  else if constexpr (RULE == 2) minp_row(each, sweep, tmax, i, a, sm);
  else {
    __shared__ float red2[2][16];
    const float lmax = key_lp(nucleus_row_max(tmax, sm)), inv_temp = a.inv_temp;
    const float c = typical_c(each, lmax, inv_temp, red2);
    if (tid == 0 && a.typ_c) a.typ_c[i] = c;
    auto word = [&](uint32_t key) { return key ? typ_word(typ_x(key_lp(key), lmax, inv_temp, c)) : 0u; };
    auto each_t = [&](auto f) { each([&](uint32_t key, int id) { f(word(key), id); }); };
    auto sweep_t = [&](auto chunk) {
      sweep([&](uint32_t k0, uint32_t, uint32_t, uint32_t, int id0) { chunk(word(k0), 0u, 0u, 0u, id0); });
    };
    auto lp_of = [&](uint32_t, int id) {
      if (id < p.c0) return hrow[id] - lse_h;
      float v = 0.f;
      int base = p.c0;
      for (int c2 = 0; c2 < p.n_tails; ++c2) {
        if (id >= base && id < base + p.tail_n[c2]) v = (p.tail[c2] + (long)i * p.ld_tail[c2])[id - base] + off[c2];
        base += p.tail_n[c2];
      }
      return v;
    };
    nucleus_search_row<TypicalRule>(each_t, sweep_t, lp_of, c, i, a, sm);
  }
}
extern "C" int tell_adaptive_logprob_nucleus(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                             int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                             int rows, int k, float inv_temp, float p, const uint32_t* seed_dev,
                                             const int* row_ids, int step, const int* step_dev, int* tokens, float* lps,
                                             int* nuc_size, uint32_t* nuc_key, hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_nucleus: up to 3 tails");
  TELL_REQUIRE(k == 0 || (k >= 2 && k <= 64), "logprob_nucleus: k = 0 (no top-k cut) or 2 <= k <= 64");
  TELL_REQUIRE(inv_temp > 0.f, "logprob_nucleus: inv_temp > 0");
  TELL_REQUIRE(p > 0.f && p <= 1.f, "logprob_nucleus: 0 < p <= 1");
  TELL_REQUIRE(seed_dev && tokens && lps, "logprob_nucleus: seed_dev, tokens and lps are required");
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  const long vocab = logits_vocab(lg);
  TELL_REQUIRE(vocab >= 1 && vocab >= k && vocab < (1L << 19), "logprob_nucleus: k <= vocab < 2^19");
  if (rows <= 0) return TELL_OK;
  const LogProbArgs q = logprob_args(lg);
  SampleArgs a = sample_args(k, inv_temp, seed_dev, row_ids, step, step_dev, tokens, lps);
  a.topp = p; a.nuc_size = nuc_size; a.nuc_key = nuc_key;
  const bool regs = logits_regs(lg);
  if (k > 0) {                                                // the top-k sampler's selection, then the nucleus of the k
    if (regs) hipLaunchKernelGGL(logprob_sample_regs_kernel<true>, dim3(rows), dim3(1024), 0, stream, q, a);
    else hipLaunchKernelGGL(logprob_sample_stream_kernel<true>, dim3(rows), dim3(1024), 0, stream, q, a);
    return tell_check_launch("logprob_nucleus (top-k)");
  }
  if (regs) hipLaunchKernelGGL(logprob_nucleus_regs_kernel<0>, dim3(rows), dim3(1024), 0, stream, q, a);
  else hipLaunchKernelGGL(logprob_nucleus_stream_kernel<0>, dim3(rows), dim3(1024), 0, stream, q, a);
  return tell_check_launch("logprob_nucleus");
}

// ------------------------------------------------------------------ min-p and locally typical sampling
// include/tell_hip.h tell_adaptive_logprob_minp / _typical: the nucleus kernels under another rule (RULE 2 / 1 above).
template <int RULE>
static int truncation_launch(const char* what, const Logits& lg, SampleArgs a, hipStream_t stream) {
  const LogProbArgs q = logprob_args(lg);
  if (logits_regs(lg)) hipLaunchKernelGGL(logprob_nucleus_regs_kernel<RULE>, dim3(lg.rows), dim3(1024), 0, stream, q, a);
  else hipLaunchKernelGGL(logprob_nucleus_stream_kernel<RULE>, dim3(lg.rows), dim3(1024), 0, stream, q, a);
  return tell_check_launch(what);
}
extern "C" int tell_adaptive_logprob_minp(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                          int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                          int rows, float inv_temp, float log_minp, const uint32_t* seed_dev,
                                          const int* row_ids, int step, const int* step_dev, int* tokens, float* lps,
                                          int* nuc_size, hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_minp: up to 3 tails");
  TELL_REQUIRE(inv_temp > 0.f, "logprob_minp: inv_temp > 0");
  TELL_REQUIRE(log_minp <= 0.f, "logprob_minp: log_minp = log(m) with 0 < m <= 1");
  TELL_REQUIRE(seed_dev && tokens && lps, "logprob_minp: seed_dev, tokens and lps are required");
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  const long vocab = logits_vocab(lg);
  TELL_REQUIRE(vocab >= 1 && vocab < (1L << 19), "logprob_minp: 1 <= vocab < 2^19");
  if (rows <= 0) return TELL_OK;
  SampleArgs a = sample_args(0, inv_temp, seed_dev, row_ids, step, step_dev, tokens, lps);
  a.topp = log_minp; a.nuc_size = nuc_size;
  return truncation_launch<2>("logprob_minp", lg, a, stream);
}
extern "C" int tell_adaptive_logprob_typical(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0,
                                             int n0, const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2,
                                             int rows, float inv_temp, float tau, const uint32_t* seed_dev,
                                             const int* row_ids, int step, const int* step_dev, int* tokens, float* lps,
                                             int* nuc_size, uint32_t* nuc_key, float* typ_c, hipStream_t stream) {
  TELL_REQUIRE(n_tails >= 0 && n_tails <= 3, "logprob_typical: up to 3 tails");
  TELL_REQUIRE(inv_temp > 0.f, "logprob_typical: inv_temp > 0");
  TELL_REQUIRE(tau > 0.f && tau <= 1.f, "logprob_typical: 0 < tau <= 1");
  TELL_REQUIRE(seed_dev && tokens && lps, "logprob_typical: seed_dev, tokens and lps are required");
  const Logits lg = logits_of(head, ld_head, c0, n_tails, tail0, ld0, n0, tail1, ld1, n1, tail2, ld2, n2, rows);
  const long vocab = logits_vocab(lg);
  TELL_REQUIRE(vocab >= 1 && vocab < (1L << 19), "logprob_typical: 1 <= vocab < 2^19");
  if (rows <= 0) return TELL_OK;
  SampleArgs a = sample_args(0, inv_temp, seed_dev, row_ids, step, step_dev, tokens, lps);
  a.topp = tau; a.nuc_size = nuc_size; a.nuc_key = nuc_key; a.typ_c = typ_c;
  return truncation_launch<1>("logprob_typical", lg, a, stream);
}

// the nucleus of given candidates (sorted best first, as tell_sample_candidates takes them): one thread per row
__global__ __launch_bounds__(256) void nucleus_candidates_kernel(const int* __restrict__ cand_tokens,
                                                                 const float* __restrict__ cand_lps, int rows, SampleArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float* lp = cand_lps + (long)r * a.k;
  const int* id = cand_tokens + (long)r * a.k;
  const int n = nucleus_prefix(lp, a.k, a.inv_temp, a.topp);
  int order[64];                                              // the members by ascending id (insertion sort, n <= 64)
  for (int j = 0; j < n; ++j) {
    int q = j;
    while (q > 0 && id[order[q - 1]] > id[j]) { order[q] = order[q - 1]; --q; }
    order[q] = j;
  }
  const int j = nucleus_draw(lp, order, n, a.inv_temp, sample_args_u(a, r));
  a.tokens[r] = id[j];
  a.lps[r] = lp[j];
}
extern "C" int tell_nucleus_candidates(const int* cand_tokens, const float* cand_lps, int rows, int k, float inv_temp, float p,
                                       const uint32_t* seed_dev, const int* row_ids, int step, const int* step_dev,
                                       int* tokens, float* lps, hipStream_t stream) {
  TELL_REQUIRE(k >= 1 && k <= 64, "nucleus_candidates: 1 <= k <= 64");
  TELL_REQUIRE(inv_temp > 0.f, "nucleus_candidates: inv_temp > 0");
  TELL_REQUIRE(p > 0.f && p <= 1.f, "nucleus_candidates: 0 < p <= 1");
  TELL_REQUIRE(seed_dev && cand_tokens && cand_lps && tokens && lps, "nucleus_candidates: null pointer");
  if (rows <= 0) return TELL_OK;
  SampleArgs a;
  a.k = k; a.inv_temp = inv_temp; a.seed_dev = seed_dev; a.row_ids = row_ids; a.step = step; a.step_dev = step_dev;
  a.tokens = tokens; a.lps = lps; a.topp = p; a.nuc_size = nullptr; a.nuc_key = nullptr;
  hipLaunchKernelGGL(nucleus_candidates_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, cand_tokens, cand_lps, rows, a);
  return tell_check_launch("nucleus_candidates");
}

// ------------------------------------------------------------------ greedy generation: one step's bookkeeping
// What the loop of transformer_faces_objects.py:443-494 does per token after the arg-max, for all rows at once: a row
// that has not finished records token and log-prob (divided by the sampling temperature), a row that emits EOS now is
// marked finished and remembers the step; every row's token becomes the next step's input (finished rows keep decoding
// into the void - the batch keeps its shape - and their outputs stay padding).  Sixteen elementwise ATen launches per
// generated token before.
__global__ void greedy_update_kernel(const int* __restrict__ tok, const float* __restrict__ lp,
                                     uint8_t* __restrict__ finished, long* __restrict__ ids, long ld_ids,
                                     float* __restrict__ lps, long ld_lps, long* __restrict__ done_step,
                                     long* __restrict__ cur, int B, int i_host, int eos, float inv_temp, int* counter,
                                     const int* step_dev) {
  const int i = step_dev ? *step_dev + 1 : i_host;             // (in a captured step: the registered counter holds i - 1)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (counter && b == 0) *counter = i;       // position offset of the NEXT replay of a step graph captured at step 1: (i + 1) - 1
  if (b >= B) return;
  const bool fin = finished[b] != 0;
  const int t = tok[b];
  if (!fin) {
    ids[(long)b * ld_ids + i + 1] = t;
    lps[(long)b * ld_lps + i] = lp[b] * inv_temp;
    if (t == eos) { done_step[b] = i + 1; finished[b] = 1; }
  }
  cur[b] = t;
}
// tok int32 [B], lp fp32 [B], finished uint8 [B], ids int64 [B, ld_ids], lps fp32 [B, ld_lps], done_step int64 [B],
// cur int64 [B] (the next step's input tokens); i = index of the step that produced tok; counter (optional): the device
// int32 a captured decode step reads as its position offset - set to i (saves the per-step fill launch in front of the graph)
extern "C" int tell_greedy_update(const int* tok, const float* lp, uint8_t* finished, long* ids, long ld_ids, float* lps,
                                  long ld_lps, long* done_step, long* cur, int B, int i, int eos, float inv_temp, int* counter,
                                  const int* step_dev, hipStream_t stream) {
  if (B <= 0) return TELL_OK;
  hipLaunchKernelGGL(greedy_update_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, tok, lp, finished, ids, ld_ids, lps,
                     ld_lps, done_step, cur, B, i, eos, inv_temp, counter, step_dev);
  return tell_check_launch("greedy_update");
}
