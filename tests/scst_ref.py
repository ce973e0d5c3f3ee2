"""Self-critical sequence training restated on the host for the tests: the reward and advantage of
tell_caption_reward by brute force in numpy (written apart from the package's own caption_reward_definition, which the host
test holds to this one), the cases its GPU test runs, and the weighted loss sum_r sum_t w_rt * -log p(y_rt) / n_valid in
float64."""
import math

import numpy as np

PAD, EOS = 1, 2
F32 = np.float32


def cut(row, limit, pad=PAD, eos=EOS):
    """row[1 ..] up to, and excluding, the first eos or pad, at most `limit` tokens"""
    out = []
    for t in list(row)[1:1 + limit]:
        if int(t) in (int(eos), int(pad)):
            break
        out.append(int(t))
    return out


def clipped_matches(h, r, k):
    """|H_k n R_k| of two token lists: every distinct k-gram of h counts min(its count in h, its count in r)"""
    hg = [tuple(h[i:i + k]) for i in range(len(h) - k + 1)]
    rg = [tuple(r[i:i + k]) for i in range(len(r) - k + 1)]
    return sum(min(hg.count(g), rg.count(g)) for g in set(hg))


def positions(t, K):
    return sum(max(len(t) - k + 1, 0) for k in range(1, K + 1))


def leave_one_out(reward):
    """adv[b, j] = reward[b, j] - s / (n - 1), s = the other rewards of the image added in ascending j in ONE fp32 accumulator"""
    reward = np.asarray(reward, F32)
    B, n = reward.shape
    adv = np.zeros((B, n), F32)
    for b in range(B):
        for j in range(n):
            s = F32(0.0)
            for e in range(n):
                if e != j:
                    s = F32(s + reward[b, e])
            adv[b, j] = F32(reward[b, j] - F32(s / F32(n - 1)))
    return adv


def reward(ids, ref, n, steps, ref_steps, K, baseline=None, pad=PAD, eos=EOS):
    """-> reward fp32 [B, n], adv fp32 [B, n], counts int32 [B * n, 3] = (match, th, tr)"""
    ids, ref = np.asarray(ids), np.asarray(ref)
    R = ids.shape[0]
    B = R // n
    rew, counts = np.zeros(R, F32), np.zeros((R, 3), np.int32)
    for r in range(R):
        h, g = cut(ids[r], steps, pad, eos), cut(ref[r // n], ref_steps, pad, eos)
        match = sum(clipped_matches(h, g, k) for k in range(1, K + 1))
        th, tr = positions(h, K), positions(g, K)
        counts[r] = (match, th, tr)
        rew[r] = F32(match) / F32(max(th, tr)) if max(th, tr) else F32(0.0)
    rew = rew.reshape(B, n)
    if baseline is not None:
        adv = (rew - np.asarray(baseline, F32).reshape(B, 1)).astype(F32)
    elif n > 1:
        adv = leave_one_out(rew)
    else:
        adv = rew.copy()
    return rew, adv, counts


# ---------------------------------------------------------------- the cases of the kernel test
CASE_B = 3
CASE_N = (1, 2, 5, 16)
CASE_STEPS = (1, 7, 64, 256)
ALPHABET = (3, 4, 5, 6, 7, 8)            # six ids: n-grams repeat, inside a row and between hypothesis and reference


def _row(rng, width, limit, kind):
    """one row [width]: <s>, `limit` tokens of the alphabet, ended as `kind` says; behind the end: other tokens, eos and pad"""
    row = np.empty(width, np.int64)
    row[0] = 0
    row[1:] = rng.choice(ALPHABET + (PAD, EOS), size=width - 1)          # what lies behind the cut is never read as a token
    body = rng.choice(ALPHABET, size=limit)
    if kind == 'run':                                                    # one token repeated: every count is clipped
        body[:] = ALPHABET[0]
    row[1:1 + limit] = body
    length = {'full': limit, 'run': limit, 'empty': 0, 'one': min(1, limit), 'short': min(3, limit),
              'any': int(rng.randint(0, limit + 1))}[kind]
    if length < limit:
        row[1 + length] = EOS if rng.randint(2) else PAD
    return row


def case(n, steps, seed=0):
    """ids int64 [B * n, ld_ids > steps + 1], ref int64 [B, ld_ref > ref_steps + 1], ref_steps: rows that never end, empty
    rows, rows shorter than the highest order, a reference longer and shorter than the hypotheses, a hypothesis that IS the
    reference (reward 1), runs of one token"""
    rng = np.random.RandomState(1000 * n + steps + seed)
    ref_steps = {1: 4, 7: 5, 64: 64, 256: 256}[steps]
    ld_ids, ld_ref = steps + 1 + 3, ref_steps + 1 + 2
    kinds = ['full', 'empty', 'one', 'short', 'any', 'run']
    ref = np.stack([_row(rng, ld_ref, ref_steps, k) for k in ('any', 'full', 'run')][:CASE_B])
    ids = np.stack([_row(rng, ld_ids, steps, kinds[(r + r // n) % len(kinds)]) for r in range(CASE_B * n)])
    m = min(steps, ref_steps)                                            # hypothesis 0 of image 1 repeats its reference
    ids[n, 1:1 + m] = ref[1, 1:1 + m]
    if steps > ref_steps:
        ids[n, 1 + m] = EOS
    return ids, ref, ref_steps


# ---------------------------------------------------------------- the weighted loss in float64
def weighted_bits(log_probs, targets, weights, pad=PAD):
    """log_probs [R, T, V], targets int [R, T], weights [R, T] -> (sum_rt w_rt * -log p(y_rt) over the non-pad targets,
    divided by their number and by ln 2; their number), float64"""
    lp, tg, w = np.asarray(log_probs, np.float64), np.asarray(targets), np.asarray(weights, np.float64)
    live = tg != pad
    nll = -np.take_along_axis(lp, tg[..., None], axis=-1)[..., 0]
    n_valid = int(live.sum())
    return float((w * nll)[live].sum() / n_valid / math.log(2)), n_valid
