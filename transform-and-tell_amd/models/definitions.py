"""The host definitions of the generation and reward kernels (include/tell_hip.h), in numpy / torch on the CPU: what the
kernels are tested against, and what serves hypotheses that live on the CPU."""
import math

import torch

from .gen_options import RANK_BY


def caption_reward_definition(ids, ref, n, steps, ref_steps, pad, eos, max_order=4, baseline=None):
    """The contract of tell_caption_reward (include/tell_hip.h) in numpy on the host - what the kernel is tested against and
    what scores hypotheses that live on the CPU.  ids [B * n, > steps], ref [B, > ref_steps], baseline fp32 [B] or None.
    -> dict: reward, adv fp32 [B, n]; counts int32 [B * n, 3] = (match, th, tr)."""
    from collections import Counter
    import numpy as np
    ids, ref = np.asarray(ids), np.asarray(ref)
    n, steps, ref_steps, K = int(n), int(steps), int(ref_steps), int(max_order)
    R = ids.shape[0]
    B = R // n

    def cut(row, L):
        out = []
        for t in row[1:1 + L]:
            if int(t) == int(eos) or int(t) == int(pad):
                break
            out.append(int(t))
        return tuple(out)

    def grams(t):
        return [Counter(zip(*[t[i:] for i in range(k)])) for k in range(1, K + 1)]

    def total(t):
        return sum(max(len(t) - k + 1, 0) for k in range(1, K + 1))
    reward, counts = np.zeros(R, dtype=np.float32), np.zeros((R, 3), dtype=np.int32)
    for b in range(B):
        rt_ = cut(ref[b], ref_steps)
        rg, tr = grams(rt_), total(rt_)
        for j in range(n):
            h = cut(ids[b * n + j], steps)
            match = sum(sum((a & c).values()) for a, c in zip(grams(h), rg))
            th = total(h)
            den = max(th, tr)
            counts[b * n + j] = (match, th, tr)
            reward[b * n + j] = np.float32(match) / np.float32(den) if den else np.float32(0.0)
    reward = reward.reshape(B, n)
    return {'reward': reward, 'adv': advantage_definition(reward, baseline), 'counts': counts}


def advantage_definition(reward, baseline=None):
    """reward fp32 [B, n] -> adv fp32 [B, n] by tell_caption_reward's rule: minus baseline[b] when given; else, for n > 1,
    minus the leave-one-out mean s / (n - 1), s summed over the OTHER rewards in ascending j in one fp32 accumulator; else
    the reward itself."""
    import numpy as np
    reward = np.asarray(reward, dtype=np.float32)
    B, n = reward.shape
    adv = np.zeros((B, n), dtype=np.float32)
    for b in range(B):
        for j in range(n):
            if baseline is not None:
                base = np.float32(np.asarray(baseline, dtype=np.float32).reshape(-1)[b])
            elif n > 1:
                s = np.float32(0.0)
                for e in range(n):
                    if e != j:
                        s = np.float32(s + reward[b, e])
                base = np.float32(s / np.float32(n - 1))
            else:
                base = np.float32(0.0)
            adv[b, j] = np.float32(reward[b, j] - base)
    return adv


def sample_rank_definition(ids, lps, done_step, n, steps, eos, rule, inv_norm=None):
    """The contract of tell_sample_rank (include/tell_hip.h) in numpy on the host - what the kernel is tested against and what
    ranks hypotheses that live on the CPU.  ids [B * n, > steps], lps [B * n, >= steps], done_step [B * n]; rule 'draw' /
    'score' / 'consensus' (or 0 / 1 / 2); inv_norm fp32 [>= steps + 1] or None.
    -> dict of [B, n] arrays: len int32, score fp32 (sequential fp32 sum, one fp32 multiply), dup uint8, cons fp32, order int32."""
    import functools
    from collections import Counter
    import numpy as np
    ids, done = np.asarray(ids), np.asarray(done_step).reshape(-1)
    lps = np.asarray(lps, dtype=np.float32)
    rule = RANK_BY.index(rule) if isinstance(rule, str) else int(rule)
    n, steps = int(n), int(steps)
    R = ids.shape[0]
    B = R // n
    ln = np.clip(done, 0, steps).astype(np.int32)
    score = np.zeros(R, dtype=np.float32)
    with np.errstate(all='ignore'):
        for r in range(R):
            acc = np.float32(0.0)
            for p in range(int(ln[r])):
                acc = np.float32(acc + lps[r, p])
            if inv_norm is not None:
                acc = np.float32(acc * np.float32(inv_norm[int(ln[r])]))
            score[r] = acc
    dup, cons, order = np.zeros(R, dtype=np.uint8), np.zeros(R, dtype=np.float32), np.zeros(R, dtype=np.int32)
    for b in range(B):
        toks = [tuple(int(t) for t in ids[b * n + j, 1:1 + int(ln[b * n + j])]) for j in range(n)]
        big = []
        for j, t in enumerate(toks):
            dup[b * n + j] = any(toks[e] == t for e in range(j))
            g = t[:-1] if t and t[-1] == int(eos) else t
            big.append(Counter(zip(g, g[1:])))
        for i in range(n):
            acc = np.float32(0.0)
            for j in range(n):
                if j == i:
                    continue
                den = sum(big[i].values()) + sum(big[j].values())
                inter = sum((big[i] & big[j]).values())
                acc = np.float32(acc + (np.float32(2 * inter) / np.float32(den) if den else np.float32(0.0)))
            cons[b * n + i] = np.float32(acc / np.float32(n - 1)) if n > 1 else np.float32(0.0)
        sc = score[b * n:(b + 1) * n]
        key = (cons if rule == 2 else score)[b * n:(b + 1) * n].copy()
        key[np.isnan(key)] = -np.inf
        dp = dup[b * n:(b + 1) * n]

        def cmp(e, j):                              # < 0: e ranks before j
            if dp[e] != dp[j]:
                return -1 if dp[e] < dp[j] else 1
            if key[e] > key[j] or key[e] < key[j]:
                return -1 if key[e] > key[j] else 1
            if rule == 2 and (sc[e] > sc[j] or sc[e] < sc[j]):
                return -1 if sc[e] > sc[j] else 1
            return -1 if e < j else 1
        order[b * n:(b + 1) * n] = list(range(n)) if rule == 0 else sorted(range(n), key=functools.cmp_to_key(cmp))
    return {k_: v_.reshape(B, n) for k_, v_ in (('len', ln), ('score', score), ('dup', dup), ('cons', cons), ('order', order))}


def nucleus_definition(lp, temp, topp, topk=0, u=None):
    """The definition of nucleus sampling (include/tell_hip.h tell_adaptive_logprob_nucleus, steps 1-4) on one row of
    log-probs, in fp64 on the CPU - what the kernel is tested against.  lp: [V] log-probs; temp = T; topp = p; topk = 0 or
    the size of the top-k cut; u in [0, 1) or None.
    -> dict: members (token ids of the nucleus, ascending), boundary (the smallest member log-prob), margin
    (|cum - p * total| / total at the boundary: the smaller of the distances by which the prefix reaches p * total and by
    which the prefix without its last member misses it), cdf (running weight of the members in id order, normalised),
    token (the pick for u, or None)."""
    import numpy as np
    lp = np.asarray(lp, dtype=np.float64).reshape(-1)
    p = float(topp)
    order = np.lexsort((np.arange(lp.size), -lp))             # value descending, lower id first on ties
    if topk:
        order = order[:int(topk)]
    w = np.exp((lp[order] - lp[order[0]]) / float(temp))
    cum = np.cumsum(w)
    total = cum[-1]
    n = min(int(np.searchsorted(cum, p * total, side='left')) + 1, order.size)
    members = np.sort(order[:n])
    margin = min(cum[n - 1] - p * total, p * total - (cum[n - 2] if n > 1 else 0.0)) / total
    wm = np.exp((lp[members] - lp[order[0]]) / float(temp))
    run = np.cumsum(wm)
    out = {'members': members, 'boundary': float(lp[order[n - 1]]), 'margin': float(abs(margin)), 'cdf': run / run[-1],
           'token': None}
    if u is not None:
        hit = np.nonzero(run > float(u) * run[-1])[0]
        out['token'] = int(members[hit[0]] if hit.size else members[-1])
    return out


def token_stats_definition(lp_full, chosen, n):
    """The definition of the per-token statistics (include/tell_hip.h tell_adaptive_logprob_stats) on
    one full row of log-probs, in torch on the CPU and in the row's own dtype - what the kernel and the generators are tested
    against.  lp_full: [V] log-probs of the model's own distribution; chosen: the token the step took; n alternatives.
    -> dict: alt_ids int64 [n] / alt_log_probs [n] (value descending, lower id first on ties; (0x7fffffff, -inf) past the
    vocabulary), token_rank (#{t: lp_t > lp_c or (lp_t == lp_c and t < c)}; -1 for a token outside the vocabulary),
    token_entropy (-sum p log p in nats, terms with p = 0 dropped), token_model_lp (lp_c; 0 outside the vocabulary)."""
    lp = torch.as_tensor(lp_full).detach().cpu().reshape(-1)
    V, n, c = lp.numel(), int(n), int(chosen)
    order = torch.sort(-lp, stable=True).indices               # (stable: equal values keep id order)
    alt = order[:n]
    alt_ids = torch.full((n,), 0x7fffffff, dtype=torch.long)
    alt_lp = torch.full((n,), float('-inf'), dtype=lp.dtype)
    alt_ids[:alt.numel()] = alt
    alt_lp[:alt.numel()] = lp[alt]
    p = lp.exp()
    ent = -(torch.where(p > 0, p * lp, torch.zeros_like(lp))).sum()
    if 0 <= c < V:
        ids = torch.arange(V)
        rank = int(((lp > lp[c]) | ((lp == lp[c]) & (ids < c))).sum())
        lp_c = lp[c].clone()
    else:
        rank, lp_c = -1, lp.new_zeros(())
    return {'alt_ids': alt_ids, 'alt_log_probs': alt_lp, 'token_rank': rank, 'token_entropy': ent, 'token_model_lp': lp_c}


def _id_order_draw(out, members, wm, u):
    import numpy as np
    run = np.cumsum(wm)
    out['cdf'] = run / run[-1]
    out['token'] = None
    if u is not None:
        hit = np.nonzero(run > float(u) * run[-1])[0]
        out['token'] = int(members[hit[0]] if hit.size else members[-1])
    return out


def minp_definition(lp, temp, minp, u=None):
    """The definition of min-p sampling (include/tell_hip.h tell_adaptive_logprob_minp) on one row of log-probs.  The member
    set is the kernel's float32 statement - a = (lp - max lp) * float32(1 / T), one fp32 subtract and one fp32 multiply; member
    iff a >= float32(log(m)) - so lp is taken as fp32; the weights of the draw are fp64.
    -> dict: members (ascending ids), a (fp32 [V]), threshold (float32(log m)), cdf (running weight of the members in id order,
    normalised), token (the pick for u, or None)."""
    import numpy as np
    lp32 = np.asarray(lp, dtype=np.float32).reshape(-1)
    a = (lp32 - lp32.max()) * np.float32(1.0 / float(temp))
    thr = np.float32(math.log(float(minp)))
    members = np.nonzero(a >= thr)[0]
    lp64 = lp32.astype(np.float64)
    wm = np.exp((lp64[members] - lp64.max()) / float(temp))
    return _id_order_draw({'members': members, 'a': a, 'threshold': thr}, members, wm, u)


def typical_definition(lp, temp, tau, c=None, u=None):
    """The definition of locally typical sampling (include/tell_hip.h tell_adaptive_logprob_typical) on one row of log-probs:
    a = (lp - max lp) / T, w = exp(a), c = -(sum w a) / (sum w), d = |a + c|; the members are the shortest prefix of the order
    (d ascending, lower id first on ties) whose weight reaches tau * (total weight).  Mass sums in fp64.  c = None: everything
    in fp64.  c given (the kernel's fp32 c): the ORDER is taken from the kernel's fp32 d = |(lp - max lp) * float32(1 / T) + c|
    (fp32 subtract, multiply, add), so that only the masses differ from the kernel's.
    -> dict: members (ascending ids), order (all ids, best first), c (the fp64 c), boundary (d of the worst member), key
    (~bits of float32(boundary): the kernel's nuc_key), margin (as nucleus_definition's, relative to the total weight), cdf,
    token."""
    import numpy as np
    lp64 = np.asarray(lp, dtype=np.float64).reshape(-1)
    a = (lp64 - lp64.max()) / float(temp)
    w = np.exp(a)
    total = w.sum()
    c64 = -float((w * a).sum() / total)
    if c is None:
        d = np.abs(a + c64)
    else:
        lp32 = np.asarray(lp, dtype=np.float32).reshape(-1)
        d = np.abs((lp32 - lp32.max()) * np.float32(1.0 / float(temp)) + np.float32(c))
        assert d.dtype == np.float32
    order = np.lexsort((np.arange(d.size), d))
    cum = np.cumsum(w[order])
    target = float(tau) * cum[-1]
    n = min(int(np.searchsorted(cum, target, side='left')) + 1, order.size)
    members = np.sort(order[:n])
    margin = min(cum[n - 1] - target, target - (cum[n - 2] if n > 1 else 0.0)) / cum[-1]
    bound = d[order[n - 1]]
    out = {'members': members, 'order': order, 'c': c64, 'boundary': float(bound), 'margin': float(abs(margin)),
           'key': int(~np.array([bound], dtype=np.float32).view(np.uint32)[0] & np.uint32(0xFFFFFFFF))}
    return _id_order_draw(out, members, w[members], u)
