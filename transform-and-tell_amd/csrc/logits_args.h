// Host side of the launchers over the adaptive-softmax logits (adaptive.hip, guidance.hip): the thirteen leading parameters
// of every tell_adaptive_logprob_* entry point (include/tell_hip.h) as one value, and what every launcher derives from them.
#pragma once
#include "common.h"
#include "options.h"

struct Logits {
  const float* head; long ld_head; int c0, n_tails;   // head: fp32 [rows, c0 + n_tails]
  const float* tail[3]; long ld[3]; int n[3];          // n[i] = 0 for i >= n_tails, whatever the caller sent
  int rows;
};
static inline Logits logits_of(const float* head, long ld_head, int c0, int n_tails, const float* tail0, long ld0, int n0,
                               const float* tail1, long ld1, int n1, const float* tail2, long ld2, int n2, int rows) {
  return Logits{head, ld_head, c0, n_tails, {tail0, tail1, tail2}, {ld0, ld1, ld2},
                {n_tails > 0 ? n0 : 0, n_tails > 1 ? n1 : 0, n_tails > 2 ? n2 : 0}, rows};
}
static inline long logits_vocab(const Logits& lg) { return (long)lg.c0 + lg.n[0] + lg.n[1] + lg.n[2]; }

// Logits per segment (head with its cluster columns, tails 0 .. 2) that the register-resident kernels hold: float4 per thread
// x 1024 threads x 4 floats, i.e. LPF_CAP[i] * 1024 * 4 (adaptive.hip) = G_CAP[i] * 1024 * 4 (guidance.hip); both files assert it.
constexpr int LOGITS_REGS_CAP[4] = {2 * 4096, 4 * 4096, 8 * 4096, 2 * 4096};
// The register form may run: option argmax_regs (an A/B aid, and the tests' way to the streaming form), the head and every
// present tail start on 16 bytes with a pitch of whole float4, and every segment fits.
static inline bool logits_regs(const Logits& lg) {
  if (tell_opt(OPT_ARGMAX_REGS) == 0) return false;
  if (lg.ld_head % 4 != 0 || (uintptr_t)lg.head % 16 != 0 || lg.c0 + lg.n_tails > LOGITS_REGS_CAP[0]) return false;
  for (int i = 0; i < lg.n_tails; ++i)
    if (lg.ld[i] % 4 != 0 || (uintptr_t)lg.tail[i] % 16 != 0 || lg.n[i] > LOGITS_REGS_CAP[i + 1]) return false;
  return true;
}
