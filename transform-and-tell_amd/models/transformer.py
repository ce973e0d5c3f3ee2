"""tell/models/transformer_faces_objects.py:23-517 and tell/models/transformer_flattened.py:24-443
on the MI355X path (training forward + loss, greedy generation)."""
import math
import os
from collections import defaultdict, namedtuple

import torch
import torch.nn as nn

from .. import graphs, ops, streams
from ..common.registrable import Registrable
from .stepper import TOKEN_STATS_REFUSALS, DecodeStepper

_OVERLAP = os.environ.get('TELL_ENCODER_OVERLAP', '1') != '0'
# where the PREFETCHED ResNet pass of the next batch is enqueued: 'own' = its side stream (three streams share the chip),
# 'main' = the training stream, in front of the decoder step of the current batch (two streams: RoBERTa against ResNet +
# decoder back to back - 4.3 + 6.7 ms against 11.2 ms alone).  MEASURED in round 6: tools/step_timeline.py, DESIGN.md.
_RESNET_STREAM = os.environ.get('TELL_RESNET_STREAM', 'own')
def _side_stream(device, name='resnet'):
    return streams.get(name, device)


class EncodedBatch:
    """Outputs of the frozen encoders for one batch (CaptionModel.encode), possibly still in flight on the
    encoder streams."""

    def __init__(self):
        self.stack = self.x_image = self.article_mask = None
        self.events = []
        self.static = False      # stack / x_image are graph-owned static buffers (stable addresses across steps)
        self.slots = []          # (graph slot, generation at production): a later replay of the slot overwrites the data

    def stale(self):
        """True when a graph replay issued after this batch was encoded has reused one of its output buffers."""
        return any(s.get('generation') != g for s, g in self.slots)

    def wait(self):
        """Join the producing streams into the current stream (idempotent)."""
        if self.events:
            cur = torch.cuda.current_stream()
            for ev in self.events:
                cur.wait_event(ev)
            self.events = []
            for t in (self.x_image, self.article_mask, self.stack):
                for u in (t if isinstance(t, (list, tuple)) else (t,)):
                    if torch.is_tensor(u) and u.is_cuda:
                        u.record_stream(cur)


class Model(nn.Module, Registrable):
    """Stand-in for allennlp.models.Model (forward(**batch) -> dict with 'loss')."""

    def __init__(self, vocab=None):
        super().__init__()
        self.vocab = vocab

    def get_metrics(self, reset=False):
        return {}

    def decode(self, output_dict):
        return output_dict


MAX_SAMPLING_TOPK = 64          # tell_adaptive_logprob_sample's exact top-k


def check_sampling(sampling_topk, sampling_temp, sampling_topp=None, sampling_minp=None, sampling_typical=None):
    """The caption models' `sampling_topk` / `sampling_temp` (transformer_faces_objects.py:38-55): top-k sampling with a
    temperature, 1 <= k <= 64 (k = 1: the arg-max token) and T > 0.  -> (k, T); ValueError otherwise.
    With `sampling_topp` = p (nucleus sampling, 0 < p <= 1): k is 0 (no top-k cut) or 2..64 -> (k, T, p).
    With `sampling_minp` = m (min-p, 0 < m <= 1) or `sampling_typical` = tau (locally typical sampling, 0 < tau <= 1;
    DESIGN.md section 19): at most one of the three, and sampling_topk must be 0 -> (0, T, m, 'minp') / (0, T, tau, 'typical')."""
    rules = [(n, v) for n, v in (('sampling_topp', sampling_topp), ('sampling_minp', sampling_minp),
                                 ('sampling_typical', sampling_typical)) if v is not None]
    if len(rules) > 1:
        raise ValueError('%s do not combine: one truncation rule per model' % ' and '.join('%s=%r' % r for r in rules))
    if sampling_minp is not None or sampling_typical is not None:
        name, v = rules[0]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < float(v) <= 1.0:
            raise ValueError('%s must be a number with 0 < %s <= 1, or None (got %r)'
                             % (name, 'm' if name == 'sampling_minp' else 'tau', v))
        k = sampling_topk
        if isinstance(k, bool) or not isinstance(k, (int, float)) or k != 0:
            raise ValueError('with %s, sampling_topk must be 0: the rule takes no top-k cut (got sampling_topk=%r)' % (name, k))
        _, temp = check_sampling(2, sampling_temp)
        return 0, temp, float(v), name[len('sampling_'):]
    if sampling_topp is not None:
        p = sampling_topp
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 < float(p) <= 1.0:
            raise ValueError('sampling_topp must be a number with 0 < p <= 1, or None (got %r)' % (p,))
        k = sampling_topk
        if not isinstance(k, bool) and isinstance(k, (int, float)) and k == 1:
            raise ValueError('sampling_topk=1 (the arg-max token) and sampling_topp=%r do not combine: pass sampling_topk=0 '
                             'for a nucleus without a top-k cut' % (p,))
        if isinstance(k, bool) or not isinstance(k, (int, float)) or int(k) != k or \
                not (int(k) == 0 or 2 <= int(k) <= MAX_SAMPLING_TOPK):
            raise ValueError('with sampling_topp, sampling_topk must be 0 (no top-k cut) or an integer in 2..%d (got %r)'
                             % (MAX_SAMPLING_TOPK, k))
        _, temp = check_sampling(2, sampling_temp)
        return int(k), temp, float(p)
    if isinstance(sampling_topk, bool) or not isinstance(sampling_topk, (int, float)) or int(sampling_topk) != sampling_topk \
            or not 1 <= int(sampling_topk) <= MAX_SAMPLING_TOPK:
        raise ValueError('sampling_topk must be an integer in 1..%d (got %r)' % (MAX_SAMPLING_TOPK, sampling_topk))
    if isinstance(sampling_temp, bool) or not isinstance(sampling_temp, (int, float)) or not float(sampling_temp) > 0.0 \
            or float(sampling_temp) == float('inf'):
        raise ValueError('sampling_temp must be a finite number > 0 (got %r)' % (sampling_temp,))
    return int(sampling_topk), float(sampling_temp)


MAX_NO_REPEAT_NGRAM = 8         # tell_decode_ban_list's longest n-gram
DEFAULT_GEN_LEN = 100           # `_generate`'s gen_len: what the constructor checks min_len against


def check_beam_options(beam_len_penalty=0.0, no_repeat_ngram_size=0, min_len=0, gen_len=DEFAULT_GEN_LEN):
    """The search options of the cached generators: `beam_len_penalty` alpha >= 0 (score =
    sum of log-probs * len ** -alpha; beam search), `no_repeat_ngram_size` 0 (off) or 1..8, `min_len` 0..gen_len - 1 (no
    </s> before that step) - the last two for greedy and beam search.  -> (alpha, n, min_len); ValueError otherwise."""
    a = beam_len_penalty
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not 0.0 <= float(a) < float('inf'):
        raise ValueError('beam_len_penalty must be a finite number >= 0 (got %r)' % (a,))
    n = no_repeat_ngram_size
    if isinstance(n, bool) or not isinstance(n, (int, float)) or int(n) != n or not 0 <= int(n) <= MAX_NO_REPEAT_NGRAM:
        raise ValueError('no_repeat_ngram_size must be 0 (off) or an integer in 1..%d (got %r)' % (MAX_NO_REPEAT_NGRAM, n))
    m = min_len
    if isinstance(m, bool) or not isinstance(m, (int, float)) or int(m) != m or not 0 <= int(m) <= int(gen_len) - 1:
        raise ValueError('min_len must be an integer in 0..%d (gen_len - 1; got %r)' % (int(gen_len) - 1, m))
    return float(a), int(n), int(m)


PENALTY_KEYS = ('repetition_penalty', 'presence_penalty', 'frequency_penalty')


def check_penalties(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0):
    """The soft repetition controls of the cached generators: `repetition_penalty` theta, finite and
    >= 1; `presence_penalty` alpha and `frequency_penalty` beta, finite and >= 0.  A token that the caption already holds
    c >= 1 times scores min(lp, 0) * theta - (alpha + beta * c) instead of its log-prob lp.  -> (theta, alpha, beta);
    ValueError naming the option otherwise."""
    out = []
    for name, v, lo in zip(PENALTY_KEYS, (repetition_penalty, presence_penalty, frequency_penalty), (1.0, 0.0, 0.0)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo <= float(v) < float('inf'):
            raise ValueError('%s must be a finite number >= %g (got %r)' % (name, lo, v))
        out.append(float(v))
    return tuple(out)


MIN_ALLOWED_TOKENS = MAX_SAMPLING_TOPK       # every row of a vocabulary mask keeps that many tokens: a pick has k real candidates


def check_mask_keys(suppress_tokens=(), ground_names=False):
    """The constructor / config keys of the vocabulary masks: `suppress_tokens`, a list of token ids
    that no caption may contain (folded into the banned set), and `ground_names`, a bool (generate(ground=True)).
    -> (tuple of ids, bool); ValueError naming the key otherwise."""
    st = suppress_tokens
    if st is None:
        st = ()
    if isinstance(st, (str, bytes)) or not isinstance(st, (list, tuple)) or \
            any(isinstance(t, bool) or not isinstance(t, int) or t < 0 for t in st):
        raise ValueError('suppress_tokens must be a list of token ids >= 0 (got %r)' % (suppress_tokens,))
    if not isinstance(ground_names, bool):
        raise ValueError('ground_names must be a bool (got %r)' % (ground_names,))
    return tuple(sorted(set(int(t) for t in st))), ground_names


GUIDANCE_CONTEXTS = ('image', 'article', 'faces', 'obj')


def check_guidance(guidance_scale=1.0, guidance_drop=('image',)):
    """The keys of context guidance: `guidance_scale` gamma, a finite number >= 0 (1.0: off), and
    `guidance_drop`, a non-empty list of context names out of image / article / faces / obj - the contexts the unconditional
    pass decodes without.  -> (gamma, names in the order above)."""
    g = guidance_scale
    if isinstance(g, bool) or not isinstance(g, (int, float)) or not math.isfinite(g) or g < 0:
        raise ValueError('guidance_scale must be a finite number >= 0 (got %r)' % (guidance_scale,))
    d = (guidance_drop,) if isinstance(guidance_drop, str) else guidance_drop
    if not isinstance(d, (list, tuple)) or not d or any(not isinstance(n, str) for n in d):
        raise ValueError('guidance_drop must be a non-empty list of context names out of %s (got %r)'
                         % (' / '.join(GUIDANCE_CONTEXTS), guidance_drop))
    unknown = [n for n in d if n not in GUIDANCE_CONTEXTS]
    if unknown:
        raise ValueError('guidance_drop: unknown context %s (the contexts are %s)'
                         % (' / '.join(repr(n) for n in unknown), ' / '.join(GUIDANCE_CONTEXTS)))
    return float(g), tuple(n for n in GUIDANCE_CONTEXTS if n in d)


def guided_batch(caption_ids, contexts, drop):
    """The batch of a guided decode: images B .. 2B - 1 are copies of 0 .. B - 1 whose dropped contexts
    have an all-masked key-padding mask - they attend to the bias key and the zero key only.  Contexts are [S, B, E] views of
    [B, S, E] storage and stay that; masks are [B, S].  -> (caption_ids [2B, T], contexts)."""
    for n in drop:
        if n not in contexts or n + '_mask' not in contexts:
            raise ValueError('guidance_drop: the decoder has no context %r (it has %s)'
                             % (n, ' / '.join(k for k in contexts if not k.endswith('_mask'))))
    out = {}
    for k, v in contexts.items():
        if not torch.is_tensor(v):
            out[k] = v
        elif k.endswith('_mask'):
            twin = torch.ones_like(v) if k[:-5] in drop else v
            out[k] = torch.cat([v, twin], 0)
        else:
            out[k] = torch.cat([v.transpose(0, 1), v.transpose(0, 1)], 0).transpose(0, 1)
    return torch.cat([caption_ids, caption_ids], 0), out


def check_vocab_mask(banned, ground, vocab_size, batch_size, eos=2, suppress=()):
    """generate(banned=, ground=).  banned: bool [V] or [B, V], True = the token may not be generated;
    ground: bool [V], the grounded class - its tokens may be generated only if they occur in the row's own article; `suppress`:
    ids folded into the banned set (the model's `suppress_tokens`).  </s> may not be banned (it is never in the class: the mask
    kernel clears it), and every row must keep at least 64 allowed tokens - the sampler's largest k, so every pick has k real
    candidates; for `ground` that is counted on the class's complement, for `banned` it is one reduction and one sync per call.
    -> (deny bool [1 or B, V] or None, cls bool [V] or None); ValueError naming the option otherwise."""
    V, B = int(vocab_size), int(batch_size)
    cls = deny = None
    if ground is not None:
        if not torch.is_tensor(ground) or ground.dtype != torch.bool or tuple(ground.shape) != (V,):
            raise ValueError('ground must be a bool tensor [%d] (the grounded class) or True (got %s)' % (
                V, '%s %s' % (ground.dtype, tuple(ground.shape)) if torch.is_tensor(ground) else repr(ground)))
        cls = ground.clone()
        if 0 <= int(eos) < V:
            cls[int(eos)] = False
        if V - int(cls.sum()) < MIN_ALLOWED_TOKENS:
            raise ValueError('ground: the class leaves %d tokens outside it, at least %d must stay allowed'
                             % (V - int(cls.sum()), MIN_ALLOWED_TOKENS))
    if banned is not None:
        if not torch.is_tensor(banned) or banned.dtype != torch.bool or banned.dim() not in (1, 2) or \
                banned.shape[-1] != V or (banned.dim() == 2 and banned.shape[0] != B):
            raise ValueError('banned must be a bool tensor [%d] or [%d, %d] (got %s)' % (
                V, B, V, '%s %s' % (banned.dtype, tuple(banned.shape)) if torch.is_tensor(banned) else repr(banned)))
        deny = banned.view(1, V) if banned.dim() == 1 else banned
        if 0 <= int(eos) < V and bool(deny[:, int(eos)].any()):
            raise ValueError('banned: </s> (%d) may not be banned - a caption could never end' % int(eos))
    sup = [int(t) for t in suppress]
    if sup:
        if max(sup) >= V:
            raise ValueError('suppress_tokens: token ids must lie in 0..%d (got %d)' % (V - 1, max(sup)))
        if int(eos) in sup:
            raise ValueError('suppress_tokens: </s> (%d) may not be suppressed - a caption could never end' % int(eos))
        dev = deny.device if deny is not None else (cls.device if cls is not None else 'cpu')
        deny = deny.clone() if deny is not None else torch.zeros(1, V, dtype=torch.bool, device=dev)
        deny[:, torch.tensor(sup, dtype=torch.long, device=deny.device)] = True
    if deny is not None:
        gone = deny if cls is None else (deny | cls.to(deny.device).view(1, V))
        left = V - int(gone.sum(1).max())                    # (the one reduction and sync of the non-default path)
        if left < MIN_ALLOWED_TOKENS:
            raise ValueError('%s: a row keeps %d allowed tokens, at least %d must stay allowed'
                             % ('banned' if banned is not None else 'suppress_tokens', left, MIN_ALLOWED_TOKENS))
    return deny, cls


def check_prefix(prefix, batch_size, vocab_size, gen_len=DEFAULT_GEN_LEN, pad=1, eos=2):
    """The forced caption prefix of the cached generators: int64 [B, P], the caption tokens AFTER <s>,
    right-padded with `pad`; plen[r] = the number of leading non-pad tokens (0: the row decodes freely).  </s> may only be
    the last token of a row's prefix, ids lie in 0..vocab_size - 1, P <= gen_len, B = batch_size.
    -> (prefix int64 [B, P] on the CPU, plen int32 [B]), or None for prefix = None; ValueError otherwise."""
    if prefix is None:
        return None
    if not torch.is_tensor(prefix) or prefix.dtype != torch.long or prefix.dim() != 2:
        raise ValueError('prefix must be an int64 tensor [B, P] of the caption tokens after <s> (got %s)' % (
            '%s %s' % (prefix.dtype, tuple(prefix.shape)) if torch.is_tensor(prefix) else type(prefix).__name__))
    B, P = prefix.shape
    if B != int(batch_size):
        raise ValueError('prefix has %d rows, the batch has %d' % (B, int(batch_size)))
    if P > int(gen_len):
        raise ValueError('prefix is %d tokens wide, generation stops after gen_len = %d' % (P, int(gen_len)))
    pf = prefix.detach().cpu().contiguous()
    real = pf != int(pad)
    plen = real.sum(1)
    if P and not bool((real == (torch.arange(P).unsqueeze(0) < plen.unsqueeze(1))).all()):
        raise ValueError('prefix: a token follows a pad (rows are right-padded with %d)' % int(pad))
    if P and bool((real & ((pf < 0) | (pf >= int(vocab_size)))).any()):
        raise ValueError('prefix: token ids must lie in 0..%d' % (int(vocab_size) - 1))
    if P and bool(((pf == int(eos)) & real & (torch.arange(P).unsqueeze(0) != (plen - 1).unsqueeze(1))).any()):
        raise ValueError('prefix: </s> (%d) may only be the last token of a row\'s prefix' % int(eos))
    return pf, plen.to(torch.int32)


def encode_prefix(texts, bpe=None, pad=1):
    """Caption starts as a `prefix` tensor: every string is encoded as the indexer encodes a caption
    (data/indexers.RobertaTokenIndexer.encode) without <s> and without the closing </s>; '' or None gives a free row.
    bpe: a RobertaBPE (default: the installed roberta-base files).  -> int64 [len(texts), P] right-padded with `pad`."""
    from ..data.indexers import RobertaTokenIndexer
    indexer = RobertaTokenIndexer(bpe=bpe, padding_value=pad)
    rows = [indexer.encode(t)[0][1:-1] if t else [] for t in texts]
    P = max([len(r) for r in rows] + [1])
    out = torch.full((len(rows), P), int(pad), dtype=torch.long)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(r, dtype=torch.long)
    return out


def inv_norm_table(alpha, L):
    """The length-penalty table of tell_beam_update_norm: fp32 [L + 1], [0] = 1, [l] = float32(float64(l) ** -alpha)."""
    import numpy as np
    t = np.ones(int(L) + 1, dtype=np.float32)
    t[1:] = (np.arange(1, int(L) + 1, dtype=np.float64) ** -float(alpha)).astype(np.float32)
    return torch.from_numpy(t)


MAX_N_SAMPLES = 16              # tell_sample_rank's hypotheses per image
RANK_BY = ('draw', 'score', 'consensus')


def check_n_samples(n_samples=1, rank_by='score', rank_len_penalty=0.0):
    """generate(n_samples=, rank_by=, rank_len_penalty=): n an integer in 1..16, the rank rule one of
    'draw' / 'score' / 'consensus', alpha a finite number >= 0 (score = sum of log-probs * len ** -alpha, as beam_len_penalty).
    -> (n, rule, alpha); ValueError otherwise."""
    n = n_samples
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_N_SAMPLES:
        raise ValueError('n_samples must be an integer in 1..%d (got %r)' % (MAX_N_SAMPLES, n))
    if not isinstance(rank_by, str) or rank_by not in RANK_BY:
        raise ValueError('rank_by must be one of %s (got %r)' % (', '.join(repr(r) for r in RANK_BY), rank_by))
    a = rank_len_penalty
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not 0.0 <= float(a) < float('inf'):
        raise ValueError('rank_len_penalty must be a finite number >= 0 (got %r)' % (a,))
    return n, rank_by, float(a)


def check_per_image(per_image, caption_rows, images):
    """forward(per_image=n): n a positive integer with caption_rows == images * n -> n; ValueError otherwise."""
    n = per_image
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError('per_image must be a positive integer (got %r)' % (n,))
    if caption_rows != images * n:
        raise ValueError('per_image=%d: %d images need %d captions (got %d)' % (n, images, images * n, caption_rows))
    return n


def check_caption_weights(w, target_ids):
    """forward(caption_weights=w): fp32 [rows] or [rows, T] on the device of the targets [rows, T] -> fp32 [rows, T]
    contiguous and detached; ValueError otherwise."""
    rows, T = target_ids.shape
    if not torch.is_tensor(w) or w.dtype != torch.float32 or w.device != target_ids.device or \
            tuple(w.shape) not in ((rows,), (rows, T)):
        raise ValueError('caption_weights must be an fp32 tensor [%d] or [%d, %d] on the device of the captions (got %s)'
                         % (rows, rows, T, (tuple(w.shape), w.dtype, str(w.device)) if torch.is_tensor(w)
                            else type(w).__name__))
    w = w.detach()
    return (w.unsqueeze(1).expand(rows, T) if w.dim() == 1 else w).contiguous()


def refuse_weighted_forward(model, caption_weights=None, per_image=1):
    """The models outside the weighted / per-image training pass (copy, GloVe, LSTM) say so by name."""
    if caption_weights is not None or per_image != 1:
        raise ValueError('%s does not take caption_weights / per_image: the weighted training pass (self-critical '
                         'training) covers the transformer_faces_objects family only' % type(model).__name__)


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


class DecodeInfo(list):
    """Third result of the cached generators without attention maps: the empty list it always was, carrying what
    `generate` reports beside the best hypothesis - scores [B] (beam: the normalised score of hypothesis 0) and, with
    n_best > 1, nbest = (ids [B, n, L], log_probs [B, n, L - 1], scores [B, n]), best first; with n_samples > 1, samples =
    the '*_samples' / 'sample_index' / 'duplicate' entries of the output dict, in rank order."""
    scores = None
    nbest = None
    samples = None
    token_stats = None             # generate(token_stats=n): the five per-token arrays of the output dict (first rank)


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


TOKEN_STATS_KEYS = ('alt_ids', 'alt_log_probs', 'token_rank', 'token_entropy', 'token_model_lp')


def check_token_stats(token_stats=0):
    """generate(token_stats=n): n alternatives per token, 0 (off) .. 8 (the K of the top-k kernels) -> int."""
    if isinstance(token_stats, bool) or not isinstance(token_stats, int) or not 0 <= token_stats <= 8:
        raise ValueError('token_stats must be an integer in 0..8 (alternatives per token; 0: off), got %r' % (token_stats,))
    return token_stats


def token_stats_neutral(B, steps, n, pad, device=None):
    """What positions behind a row's </s> hold: alt_ids = pad, alt_log_probs = 0, token_rank = -1, token_entropy = 0,
    token_model_lp = 0 - the five arrays of generate(token_stats=n) filled with them."""
    return {'alt_ids': torch.full((B, steps, n), int(pad), dtype=torch.long, device=device),
            'alt_log_probs': torch.zeros(B, steps, n, dtype=torch.float32, device=device),
            'token_rank': torch.full((B, steps), -1, dtype=torch.long, device=device),
            'token_entropy': torch.zeros(B, steps, dtype=torch.float32, device=device),
            'token_model_lp': torch.zeros(B, steps, dtype=torch.float32, device=device)}


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


def draw_seed():
    """The seed of one batch's sampled decode: 31 bits from torch's default CPU generator (torch.manual_seed makes the
    captions reproducible)."""
    return int(torch.randint(0, 1 << 31, (1,)).item())


def set_sampling(model, sampling_topk, sampling_temp, sampling_topp=None, sampling_minp=None, sampling_typical=None):
    """check_sampling, kept on the model: sampling_topk / _temp / _topp / _minp / _typical."""
    model.sampling_topk, model.sampling_temp = check_sampling(sampling_topk, sampling_temp, sampling_topp, sampling_minp,
                                                              sampling_typical)[:2]
    model.sampling_topp = None if sampling_topp is None else float(sampling_topp)
    model.sampling_minp = None if sampling_minp is None else float(sampling_minp)
    model.sampling_typical = None if sampling_typical is None else float(sampling_typical)


class AttnMaps(namedtuple('AttnMaps', 'maps steps')):
    """Third result of the cached generator with attention=True (without: the empty list it always was).
    maps: {context name: fp32 [B, steps, n_layers, S + 2]} on the device; steps: [B] long, the row's `done_step` - the
    number of decode steps it took part in, the one that produced its </s> included."""
    __slots__ = ()


class AttnMapsStats(AttnMaps):
    """AttnMaps of a generation that also kept per-token statistics (attention=True, token_stats=n): .token_stats as DecodeInfo's."""
    token_stats = None


class CaptionModel(Model):
    USE_FACES_OBJECTS = False
    EVAL_ATTENTION = True        # forward() in evaluate mode honours `eval_attention` (commands/evaluate.py attention_maps=True)
    EXTRA_CONTEXTS = ()          # which of ('faces', 'obj') the model feeds to its decoder

    def __init__(self, vocab, decoder, criterion, evaluate_mode=False, attention_dim=1024, hidden_size=1024,
                 dropout=0.1, vocab_size=50264, model_name='roberta-base', namespace='bpe', index='roberta',
                 padding_value=1, use_context=True, sampling_topk=1, sampling_temp=1.0, weigh_bert=False,
                 initializer=None, resnet=None, roberta=None, n_bert_layers=25, sampling_topp=None,
                 beam_len_penalty=0.0, no_repeat_ngram_size=0, min_len=0, sampling_minp=None, sampling_typical=None,
                 repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, suppress_tokens=(),
                 ground_names=False, guidance_scale=1.0, guidance_drop=('image',)):
        super().__init__(vocab)
        self.decoder, self.criterion = decoder, criterion
        self.index, self.namespace = index, namespace
        if resnet is None:
            from .resnet import resnet152
            resnet = resnet152()
        if roberta is None:
            from .roberta import roberta_large
            roberta = roberta_large()
        self.resnet, self.roberta = resnet, roberta
        self.use_context = use_context
        self.padding_idx = padding_value
        self.evaluate_mode = evaluate_mode
        set_sampling(self, sampling_topk, sampling_temp, sampling_topp, sampling_minp, sampling_typical)
        self.beam_len_penalty, self.no_repeat_ngram_size, self.min_len = check_beam_options(
            beam_len_penalty, no_repeat_ngram_size, min_len)
        self._check_options()
        self._check_truncation()
        self.repetition_penalty, self.presence_penalty, self.frequency_penalty = check_penalties(
            repetition_penalty, presence_penalty, frequency_penalty)
        self._check_penalties()
        self.suppress_tokens, self.ground_names = check_mask_keys(suppress_tokens, ground_names)
        self._check_mask_options()
        self.guidance_scale, self.guidance_drop = check_guidance(guidance_scale, guidance_drop)
        self._check_guidance()
        self.weigh_bert = weigh_bert
        if weigh_bert:
            self.bert_weight = nn.Parameter(torch.rand(n_bert_layers))      # nn.init.uniform_, :57-59
        self.n_batches = 0
        self.n_samples = 0
        self.sample_history = defaultdict(float)
        # captured encoder / decode graphs bake in the addresses of working copies of the weights: anything that can
        # re-home those copies (a checkpoint load, a trainer re-flagging requires_grad) drops the captures
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.reset_graphs())

    def _sampling(self):
        """-> (k, T) when generation samples (sampling_topk > 1), None for the arg-max decode (sampling_topk = 1);
        (k, T, p) with nucleus sampling (sampling_topp = p; k = 0: no top-k cut); (0, T, m, 'minp') with sampling_minp = m and
        (0, T, tau, 'typical') with sampling_typical = tau."""
        k = int(self.sampling_topk)
        for rule in ('minp', 'typical'):
            v = getattr(self, 'sampling_' + rule, None)
            if v is not None:
                return (0, float(self.sampling_temp), float(v), rule)
        p = getattr(self, 'sampling_topp', None)
        if p is not None:
            return (k, float(self.sampling_temp), float(p))
        return (k, float(self.sampling_temp)) if k > 1 else None

    def _truncation(self):
        """-> 'sampling_minp=0.1' / 'sampling_typical=0.9' when one of the two rules is set, else None."""
        for name in ('sampling_minp', 'sampling_typical'):
            if getattr(self, name, None) is not None:
                return '%s=%r' % (name, getattr(self, name))
        return None

    def _check_truncation(self):
        """sampling_minp / sampling_typical: the cached DynamicConv generator only."""
        what = self._truncation()
        if what and (not self.SEARCH_OPTIONS or not hasattr(getattr(self, 'decoder', None), 'project_contexts')):
            raise ValueError('%s: %s has a decode step with its own decision launch (LSTM decoders, copy models); min-p and '
                             'typical sampling cover the cached DynamicConv generator only' % (what, type(self).__name__))

    def _check_beam(self, beam_size):
        if int(beam_size) > 1 and self._truncation():
            raise ValueError('beam search (beam_size %d) and %s do not combine' % (int(beam_size), self._truncation()))
        if int(beam_size) > 1 and getattr(self, 'sampling_topp', None) is not None:
            raise ValueError('beam search (beam_size %d) and nucleus sampling (sampling_topp %r) do not combine'
                             % (int(beam_size), self.sampling_topp))
        if int(beam_size) > 1 and self._sampling() is not None:
            raise ValueError('beam search (beam_size %d) and top-k sampling (sampling_topk %d) do not combine: the reference '
                             'samples without a beam' % (int(beam_size), int(self.sampling_topk)))

    SEARCH_OPTIONS = True        # the class decodes through the cached generator below (False: the options are refused)

    def _search_options(self, gen_len=DEFAULT_GEN_LEN):
        """-> (alpha, n, min_len) of the model's attributes, checked; None when all three are at their defaults."""
        opts = check_beam_options(getattr(self, 'beam_len_penalty', 0.0), getattr(self, 'no_repeat_ngram_size', 0),
                                  getattr(self, 'min_len', 0), gen_len)
        return None if opts == (0.0, 0, 0) else opts

    def _check_options(self, beam_size=1, attention=False, n_best=1, gen_len=DEFAULT_GEN_LEN):
        """What the search options and n_best combine with: the arg-max / beam decode of the cached DynamicConv generator -
        no sampling, no attention maps, not the LSTM decoders nor the copy models."""
        if isinstance(n_best, bool) or not isinstance(n_best, int) or not 1 <= n_best <= max(int(beam_size), 1):
            raise ValueError('n_best must be an integer in 1..beam_size (got n_best=%r with beam_size=%d)'
                             % (n_best, int(beam_size)))
        opts = self._search_options(gen_len)
        used = [name for name, v in zip(('beam_len_penalty', 'no_repeat_ngram_size', 'min_len'), opts or ()) if v]
        if n_best > 1:
            used.append('n_best')
        if not used:
            return None
        what = ' / '.join('%s=%r' % (u, n_best if u == 'n_best' else getattr(self, u)) for u in used)
        if self._truncation():
            raise ValueError('%s and %s do not combine: the search options apply to the arg-max and beam decodes'
                             % (what, self._truncation()))
        if getattr(self, 'sampling_topp', None) is not None or int(getattr(self, 'sampling_topk', 1)) > 1:
            raise ValueError('%s and sampling (sampling_topk %r, sampling_topp %r) do not combine: the search options '
                             'apply to the arg-max and beam decodes' % (what, self.sampling_topk, self.sampling_topp))
        if attention:
            raise ValueError('%s and attention=True do not combine: attention maps are exported without search options'
                             % what)
        if not self.SEARCH_OPTIONS or not hasattr(getattr(self, 'decoder', None), 'project_contexts'):
            raise ValueError('%s: %s has a decode step with its own decision launch (LSTM decoders, copy models); the '
                             'search options cover the cached DynamicConv generator only' % (what, type(self).__name__))
        return opts

    def _penalties(self):
        """-> (theta, alpha, beta) of the model's attributes, checked; None when all three are at their defaults."""
        pen = check_penalties(getattr(self, 'repetition_penalty', 1.0), getattr(self, 'presence_penalty', 0.0),
                              getattr(self, 'frequency_penalty', 0.0))
        return None if pen == (1.0, 0.0, 0.0) else pen

    def _check_penalties(self, attention=False):
        """What the penalties combine with: the arg-max, beam and top-k sampling decodes of the cached
        DynamicConv generator - no truncation rule, no ban options, no attention maps, not the LSTM decoders nor the copy
        models.  -> (theta, alpha, beta) or None."""
        pen = self._penalties()
        if pen is None:
            return None
        what = ' / '.join('%s=%r' % (k_, v) for k_, v, d in zip(PENALTY_KEYS, pen, (1.0, 0.0, 0.0)) if v != d)
        for name in ('sampling_topp', 'sampling_minp', 'sampling_typical'):
            if getattr(self, name, None) is not None:
                raise ValueError('%s and %s=%r do not combine: the penalties cover the arg-max, beam and top-k sampling decodes'
                                 % (what, name, getattr(self, name)))
        for name in ('no_repeat_ngram_size', 'min_len'):
            if getattr(self, name, 0):
                raise ValueError('%s and %s=%r do not combine: one list per pick launch' % (what, name, getattr(self, name)))
        if attention:
            raise ValueError('%s and attention=True do not combine: attention maps are exported without penalties' % what)
        if not self.SEARCH_OPTIONS or not hasattr(getattr(self, 'decoder', None), 'project_contexts'):
            raise ValueError('%s: %s has a decode step with its own decision launch (LSTM decoders, copy models); the '
                             'penalties cover the cached DynamicConv generator only' % (what, type(self).__name__))
        return pen

    def _mask_options(self, banned=None, ground=None):
        """-> the names of the vocabulary-mask options in force ('banned', 'ground', 'suppress_tokens', 'ground_names'), the
        call's arguments and the model's attributes alike; empty: nothing set."""
        st, gn = check_mask_keys(getattr(self, 'suppress_tokens', ()), getattr(self, 'ground_names', False))
        used = []
        if banned is not None:
            used.append('banned')
        if ground is not None and ground is not False:
            used.append('ground')
        if st:
            used.append('suppress_tokens')
        if gn and 'ground' not in used:
            used.append('ground_names')
        return used

    def _check_mask_options(self, banned=None, ground=None, attention=False):
        """What a vocabulary mask combines with: the arg-max, beam and top-k sampling decodes of the
        cached DynamicConv generator, with or without the search options, n_samples and a prefix - no truncation rule, no
        penalties, no attention maps, not the LSTM decoders nor the copy models.  -> the option names in force (may be empty)."""
        used = self._mask_options(banned, ground)
        if not used:
            return used
        what = ' / '.join(used)
        for name in ('sampling_topp', 'sampling_minp', 'sampling_typical'):
            if getattr(self, name, None) is not None:
                raise ValueError('%s and %s=%r do not combine: a vocabulary mask covers the arg-max, beam and top-k sampling '
                                 'decodes' % (what, name, getattr(self, name)))
        if self._penalties() is not None:
            pen = ' / '.join('%s=%r' % (k_, v) for k_, v, d in zip(PENALTY_KEYS, self._penalties(), (1.0, 0.0, 0.0)) if v != d)
            raise ValueError('%s and %s do not combine: the penalties\' bitmap means "listed", not "banned"' % (what, pen))
        if attention:
            raise ValueError('%s and attention=True do not combine: attention maps are exported without a vocabulary mask' % what)
        if not self.SEARCH_OPTIONS or not hasattr(getattr(self, 'decoder', None), 'project_contexts'):
            raise ValueError('%s: %s has a decode step with its own decision launch (LSTM decoders, copy models); vocabulary '
                             'masks cover the cached DynamicConv generator only' % (what, type(self).__name__))
        return used

    def _check_guidance(self, guidance=None, guidance_drop=None, attention=False, prefix=None, n_samples=1, banned=None,
                        ground=None):
        """Context guidance of one call: the arguments, or where they are None the model's
        `guidance_scale` / `guidance_drop`, checked (check_guidance; every name a context of this decoder).  -> None for
        gamma = 1.0 (off: the call of before), else (drop, gamma) after what guidance combines with: the arg-max and beam decodes
        of the cached DynamicConv generator with beam_len_penalty and n_best - no sampling rule, no no_repeat_ngram_size /
        min_len, no penalties, no vocabulary mask, no prefix, no n_samples, no attention maps, not the LSTM decoders nor the
        copy models."""
        gamma, drop = check_guidance(getattr(self, 'guidance_scale', 1.0) if guidance is None else guidance,
                                     getattr(self, 'guidance_drop', ('image',)) if guidance_drop is None else guidance_drop)
        layers = getattr(getattr(self, 'decoder', None), 'layers', None)
        have = getattr(layers[0], 'context_names', None) if layers is not None and len(layers) else None
        if have is not None and (gamma != 1.0 or guidance_drop is not None):   # (the default drop of a model that is off: unread)
            for n in drop:
                if n not in have:
                    raise ValueError('guidance_drop: the decoder has no context %r (it has %s)' % (n, ' / '.join(have)))
        if gamma == 1.0:
            return None
        what = 'guidance=%r' % gamma
        if not self.SEARCH_OPTIONS or not hasattr(getattr(self, 'decoder', None), 'project_contexts'):
            raise ValueError('%s: %s has a decode step with its own decision launch (LSTM decoders, copy models); context '
                             'guidance covers the cached DynamicConv generator only' % (what, type(self).__name__))
        if int(getattr(self, 'sampling_topk', 1)) > 1:
            raise ValueError('%s and sampling_topk=%r do not combine: guidance covers the arg-max and beam decodes'
                             % (what, self.sampling_topk))
        for name in ('sampling_topp', 'sampling_minp', 'sampling_typical'):
            if getattr(self, name, None) is not None:
                raise ValueError('%s and %s=%r do not combine: guidance covers the arg-max and beam decodes'
                                 % (what, name, getattr(self, name)))
        for name in ('no_repeat_ngram_size', 'min_len'):
            if getattr(self, name, 0):
                raise ValueError('%s and %s=%r do not combine: the guided pick takes no ban list' % (what, name, getattr(self, name)))
        if self._penalties() is not None:
            pen = ' / '.join('%s=%r' % (k_, v) for k_, v, d in zip(PENALTY_KEYS, self._penalties(), (1.0, 0.0, 0.0)) if v != d)
            raise ValueError('%s and %s do not combine: the guided pick takes no penalty list' % (what, pen))
        used = self._mask_options(banned, ground)
        if used:
            raise ValueError('%s and %s do not combine: the guided pick takes no vocabulary mask' % (what, ' / '.join(used)))
        if prefix is not None:
            raise ValueError('%s and prefix do not combine: a forced token has no guided log-prob' % what)
        if isinstance(n_samples, int) and n_samples > 1:
            raise ValueError('%s and n_samples=%d do not combine: guidance covers the arg-max and beam decodes' % (what, n_samples))
        if attention:
            raise ValueError('%s and attention=True do not combine: attention maps are exported without guidance' % what)
        return drop, gamma

    def name_tokens(self):
        """The grounded class of generate(ground=True): data.bpe.capitalised_tokens over the installed roberta-base vocabulary -
        bool [vocab], the BPE pieces that start a capitalised word (per token, not per word: continuation pieces are
        unconstrained).  Cached; FileNotFoundError when the vocabulary files are absent."""
        cls = self.__dict__.get('_name_tokens')
        if cls is None:
            from ..data.bpe import RobertaBPE, capitalised_tokens
            from ..data.indexers import bpe_directory
            cls = capitalised_tokens(RobertaBPE(bpe_directory()))
            V = int(self.decoder.adaptive_softmax.vocab_size)
            full = torch.zeros(V, dtype=torch.bool)
            full[:min(V, cls.numel())] = cls[:V]
            cls = self.__dict__['_name_tokens'] = full
        return cls

    def _vocab_mask(self, context, banned=None, ground=None, attention=False, eos=2):
        """The vocabulary mask of one caption batch, from generate's arguments and the model's `suppress_tokens` /
        `ground_names`: -> None when nothing is set (the default path reads nothing of the batch), else (ctx_ids int64 [B, S] -
        the article ids context[self.index] -, cls_bits int32 [words] or None, deny8 uint8 [1 or B, V] or None), what
        DecodeStepper.set_mask takes.  check_vocab_mask and _check_mask_options apply."""
        used = self._check_mask_options(banned, ground, attention)
        if not used:
            return None
        ctx_ids = context[self.index]
        if ground is True or (ground is None and 'ground_names' in used):
            ground = self.name_tokens()
        if ground is False:
            ground = None
        V = int(self.decoder.adaptive_softmax.vocab_size)
        deny, cls = check_vocab_mask(banned, ground, V, ctx_ids.shape[0], eos,
                                     suppress=getattr(self, 'suppress_tokens', ()) or ())
        dev = ctx_ids.device
        cls_bits = None if cls is None else ops.pack_mask_bits(cls).to(dev)
        deny8 = None if deny is None else deny.to(device=dev, dtype=torch.uint8).contiguous()
        return ctx_ids, cls_bits, deny8

    def _check_prefix(self, prefix, batch_size, gen_len=DEFAULT_GEN_LEN, eos=2):
        """generate(prefix=...): check_prefix against this model; the cached DynamicConv generators only - the LSTM decoders
        and the copy models end their decode step in a decision launch of their own.  -> (prefix, plen) or None."""
        if prefix is None:
            return None
        if not self.SEARCH_OPTIONS or not hasattr(getattr(self, 'decoder', None), 'project_contexts'):
            raise ValueError('prefix: %s has a decode step with its own decision launch (LSTM decoders, copy models such as '
                             'transformer_pointer / transformer_pointer_2); a forced prefix is out of scope there: it covers '
                             'the cached DynamicConv generator only' % type(self).__name__)
        return check_prefix(prefix, batch_size, self.decoder.adaptive_softmax.vocab_size, gen_len, self.padding_idx, eos)

    CACHED_N_SAMPLES = False       # a model with a decision launch of its own that still decodes n hypotheses per image

    def _check_n_samples(self, n_samples=1, rank_by='score', rank_len_penalty=0.0, beam_size=1, attention=False,
                         forward=False, cached=False):
        """generate(n_samples=n): check_n_samples, and for n > 1 what it combines with - a sampling
        decode of the cached DynamicConv generator, one seed per call; no beam search (n_best is the beam's own form), no
        attention maps, not forward=True, not the arg-max decode, not the LSTM decoders nor the copy models - except, with
        cached=True (the call decodes through the cached step), a copy model that samples (CACHED_N_SAMPLES, DESIGN.md
        section 28).  -> (n, rule, alpha), or None for n = 1."""
        n, rule, alpha = check_n_samples(n_samples, rank_by, rank_len_penalty)
        if n == 1:
            return None
        if int(beam_size) > 1:
            raise ValueError('n_samples=%d and beam search (beam_size %d) do not combine: n_best is the beam\'s own form'
                             % (n, int(beam_size)))
        if attention:
            raise ValueError('n_samples=%d and attention=True do not combine: attention maps are exported for one hypothesis '
                             'per sample' % n)
        if forward:
            raise ValueError('n_samples goes with generate, not with forward=True')
        has_cache = hasattr(getattr(self, 'decoder', None), 'project_contexts')
        if not has_cache or not (self.SEARCH_OPTIONS or (cached and self.CACHED_N_SAMPLES and self._sampling() is not None)):
            raise ValueError('n_samples=%d: %s has a decode step with its own decision launch (LSTM decoders, copy models); '
                             'several samples per image cover the cached DynamicConv generator only' % (n, type(self).__name__))
        if self._sampling() is None:
            raise ValueError('n_samples=%d needs a sampling model (sampling_topk > 1, sampling_topp, sampling_minp or '
                             'sampling_typical): the arg-max decode (sampling_topk 1) would give %d identical captions' % (n, n))
        return n, rule, alpha

    def _check_token_stats(self, token_stats=0, beam_size=1, n_best=1, guide=None):
        """generate(token_stats=n): check_token_stats, and for n > 0 what it combines with - the greedy
        and sampling decodes of the cached DynamicConv generator; no beam search, no guidance, no LSTM decoder.  -> n."""
        n = check_token_stats(token_stats)
        if not n:
            return 0
        if int(beam_size) > 1 or int(n_best) > 1:
            raise ValueError('token_stats=%d: %s' % (n, TOKEN_STATS_REFUSALS['beam']))
        if guide is not None:
            raise ValueError('token_stats=%d: %s' % (n, TOKEN_STATS_REFUSALS['guide']))
        if not hasattr(getattr(self, 'decoder', None), 'project_contexts'):
            raise ValueError('token_stats=%d: %s' % (n, TOKEN_STATS_REFUSALS['lstm']))
        return n

    def _check_attention(self, beam_size=1):
        """generate(attention=True): what the attention-map export covers - the DynamicConv decoders, one hypothesis per
        sample (greedy, top-k, nucleus)."""
        if int(beam_size) > 1:
            raise ValueError('attention=True: attention maps are exported for greedy / top-k / nucleus generation only, not '
                             'for beam search (beam_size %d): the slots would have to follow the surviving hypotheses'
                             % int(beam_size))
        if not hasattr(self.decoder, 'project_contexts'):
            raise ValueError('attention=True: %s is an LSTM decoder; attention maps are exported for the DynamicConv '
                             'decoders only (its dot attention is not covered)' % type(self.decoder).__name__)

    @staticmethod
    def _attn_output(out, attns):
        """'attns' (+ 'attn_steps') of an output dict from a generator's third result: an AttnMaps, or the plain list."""
        if isinstance(attns, AttnMaps):
            out['attns'], out['attn_steps'] = attns.maps, attns.steps
        else:
            out['attns'] = [] if isinstance(attns, DecodeInfo) else attns
        if torch.is_tensor(out.get('log_probs')):
            # 'scores': the hypothesis' score - the (tempered) log-prob sum; beam search: normalised by beam_len_penalty
            info = attns if isinstance(attns, DecodeInfo) else None
            out['scores'] = info.scores if info is not None and info.scores is not None else out['log_probs'].sum(-1)
            if info is not None and info.nbest is not None:
                out['gen_ids_nbest'], out['log_probs_nbest'], out['scores_nbest'] = info.nbest
            if info is not None and info.samples is not None:
                out.update(info.samples)
        if getattr(attns, 'token_stats', None) is not None:
            out.update(attns.token_stats)
        return out

    def reset_graphs(self):
        """Forget every captured hipGraph of this model (encoders, decode steps); they are re-recorded on next use."""
        for k in ('_resnet_graph', '_roberta_graph'):
            g = self.__dict__.get(k)
            if g is not None:
                g.reset()
        self.__dict__.pop('_decode_graphs', None)
        self.__dict__.pop('_decode_graphs_stamp', None)

    def set_capture_after(self, n):
        """Sightings of an input shape before the encoder graphs capture it (graphs.CAPTURE_AFTER by default)."""
        self.__dict__['_capture_after'] = n
        self.reset_graphs()
        for k in ('_resnet_graph', '_roberta_graph'):
            self.__dict__.pop(k, None)

    def _run_resnet(self, image, slot=None):
        """The frozen trunk as one hipGraph replay per step (graphs.GraphedCall); eager for the first call."""
        from .resnet import ResNetFeatureExtractor
        if not isinstance(self.resnet, ResNetFeatureExtractor):      # a user-supplied trunk: no assumptions
            return self.resnet(image)
        g = self.__dict__.get('_resnet_graph')
        if g is None:
            g = self.__dict__['_resnet_graph'] = graphs.GraphedCall(self.resnet, 'resnet152',
                                                                    capture_after=self.__dict__.get('_capture_after'))
        w = self.resnet.conv1.weight                 # a reloaded / moved / re-typed trunk must not replay stale pointers
        from .resnet import stats_epoch
        # (eval captures bake in weights folded with the running statistics: a train-mode pass in between retires them)
        return g(image, key=(self.resnet.training, ops.rt.compute_dtype(), w._version, w.data_ptr(),
                             0 if self.resnet.training else stats_epoch()), slot=slot)

    def _run_roberta(self, article_ids, slot=None):
        """RoBERTa-large (~170 launches, dropout active in train mode) as one hipGraph replay per step."""
        from .roberta import RobertaEncoder
        if not isinstance(self.roberta, RobertaEncoder):
            return self.roberta.extract_features(article_ids, return_all_hiddens=True)
        g = self.__dict__.get('_roberta_graph')
        if g is None:
            g = self.__dict__['_roberta_graph'] = graphs.GraphedCall(
                lambda ids: self.roberta.extract_features(ids, return_all_hiddens=True), 'roberta-large', rng=True,
                capture_after=self.__dict__.get('_capture_after'))
        w = self.roberta.model.decoder.sentence_encoder.layers[0].fc1.weight
        return g(article_ids, key=(self.roberta.training, ops.rt.compute_dtype(), w._version, w.data_ptr()), slot=slot)

    # ---- frozen encoders -------------------------------------------------------------
    def encode(self, context, image, ahead=False):
        """ResNet-152 + RoBERTa-large on one batch (transformer_faces_objects.py:335-353) -> EncodedBatch.

        The two encoders are independent and read no trainable weight.  ahead=False: RoBERTa runs on the current
        stream, ResNet's many small launches on a side stream underneath RoBERTa's chip-filling GEMMs
        (TELL_ENCODER_OVERLAP=0 serialises them).  ahead=True: both run on their own streams and the call returns
        at once - the trainer uses it to encode batch N+1 underneath the latency-bound decoder forward /
        backward / optimizer of batch N; `EncodedBatch.wait()` joins them into the consumer's stream."""
        with torch.no_grad():
            main = torch.cuda.current_stream()
            article_ids = context[self.index]
            enc = EncodedBatch()
            # both encoder graphs replay into the buffer set of this call's parity: consecutive batches never share a
            # buffer, and the addresses the decoder step graph is keyed on depend on the parity alone (graphs.py)
            par = self.__dict__['_enc_parity'] = self.__dict__.get('_enc_parity', -1) + 1
            if ahead:
                rs = _side_stream(image.device, 'roberta')
                is_ = main if _RESNET_STREAM == 'main' else _side_stream(image.device, 'resnet')
                start = torch.cuda.Event()
                start.record(main)
                rs.wait_event(start)
                if is_ is not main:
                    is_.wait_event(start)
                with torch.cuda.stream(rs), ops.hip.bound_stream():
                    enc.article_mask = self._pad_mask(article_ids)                      # :347
                    enc.stack = self._run_roberta(article_ids, par)
                    article_ids.record_stream(rs)
                    enc.events.append(torch.cuda.Event())
                    enc.events[-1].record(rs)
                with torch.cuda.stream(is_), ops.hip.bound_stream():
                    enc.x_image = self._run_resnet(image, par)
                    image.record_stream(is_)
                    enc.events.append(torch.cuda.Event())
                    enc.events[-1].record(is_)
                enc.static = self._encoders_replayed()
                self._note_slots(enc)
                return enc
            side = _side_stream(image.device, 'resnet') if _OVERLAP else None
            enc.article_mask = self._pad_mask(article_ids)                              # :347
            if side is not None:
                start = torch.cuda.Event()
                start.record(main)
            # RoBERTa is issued FIRST: its ~300 launches keep the main stream busy for ~10 ms of GPU time
            # while the host is still issuing ResNet's small launches onto the side stream.
            enc.stack = self._run_roberta(article_ids, par)                                   # [L,B,S,E]
            if side is not None:
                side.wait_event(start)
                with torch.cuda.stream(side), ops.hip.bound_stream():
                    enc.x_image = self._run_resnet(image, par)             # [B,49,2048] (NHWC == :335-341)
                    enc.events.append(torch.cuda.Event())
                    enc.events[-1].record(side)
            else:
                enc.x_image = self._run_resnet(image, par)
            enc.static = self._encoders_replayed()
            self._note_slots(enc)
            return enc

    def _encoders_replayed(self):
        return all(getattr(self.__dict__.get(k), 'last_replayed', False) for k in ('_resnet_graph', '_roberta_graph'))

    def _note_slots(self, enc):
        for k in ('_resnet_graph', '_roberta_graph'):
            g = self.__dict__.get(k)
            if g is not None and getattr(g, 'last_replayed', False):
                enc.slots.append((g.last_slot, g.last_slot['generation']))

    def _pad_mask(self, ids):
        """Key-padding mask of the article (:347).  On the GPU as the uint8 the attention kernels read - produced once,
        inside the encoder graph - instead of a bool that every decoder call converts."""
        m = ids == self.padding_idx
        return m.to(torch.uint8) if ids.is_cuda else m

    def _no_mask(self, B, P, device):
        """The all-visible mask of the image regions (:371): a constant, built once per shape."""
        cache = self.__dict__.setdefault('_no_mask_cache', {})
        key = (B, P, str(device))
        if key not in cache:
            cache[key] = torch.zeros(B, P, dtype=torch.uint8 if torch.device(device).type == 'cuda' else torch.bool,
                                     device=device)
        return cache[key]

    # ---- :311-397 -----------------------------------------------------------------
    def _forward(self, context, image, caption, face_embeds=None, obj_embeds=None, encoded=None, per_image=1):
        """per_image = n: `caption` holds n captions for each of the B images (caption b * n + j belongs to image b); every
        context and its mask is repeated n times along the batch axis AFTER the encoders and the layer mix - one encode for
        the n captions, and autograd sums the mix's gradient over them."""
        dtype = ops.rt.compute_dtype()
        cap = caption[self.index]
        plain = type(per_image) is int and per_image == 1                  # (the default reads nothing more of the batch)
        n_per = 1 if plain else check_per_image(per_image, cap.shape[0], image.shape[0])
        target_ids = cap[:, 1:].contiguous()                               # :321-328
        caption_ids = cap[:, :-1].contiguous()
        caption[self.index] = caption_ids                                  # :329

        enc = encoded if encoded is not None else self.encode(context, image)   # frozen encoders (config :150-152)
        enc.wait()
        stack, x_image, article_mask = enc.stack, enc.x_image, enc.article_mask
        B, P, _ = x_image.shape
        ops.rt.wait_weight_update()      # everything below reads trainable weights (the encoders above do not)
        if self.weigh_bert:
            x_article = ops.mix_layers(stack, self.bert_weight)            # :355-364
        else:
            x_article = stack[-1]
        if n_per > 1:
            B = B * n_per
            x_image, x_article, article_mask = (t.repeat_interleave(n_per, dim=0) for t in (x_image, x_article, article_mask))
            face_embeds, obj_embeds = (None if t is None else t.repeat_interleave(n_per, dim=0)
                                       for t in (face_embeds, obj_embeds))
        contexts = {
            'image': x_image.transpose(0, 1),
            'image_mask': self._no_mask(B, P, image.device),                  # :371
            'article': x_article.transpose(0, 1),
            'article_mask': article_mask,
        }
        if self.EXTRA_CONTEXTS:                                            # :373-379
            for key, emb in (('faces', face_embeds), ('obj', obj_embeds)):
                if key not in self.EXTRA_CONTEXTS:
                    continue
                Bf, n, dim = emb.shape
                if n == 0 or dim == 0:
                    contexts[key] = emb.new_zeros(n, Bf, dim).to(dtype)
                    contexts[key + '_mask'] = torch.zeros(Bf, n, dtype=torch.bool, device=emb.device)
                    continue
                clean = torch.empty(Bf, n, dim, dtype=dtype, device=emb.device)
                mask = torch.empty(Bf, n, dtype=torch.uint8, device=emb.device)
                ops.call('tell_nan_rows', emb.float().contiguous(), Bf * n, dim, clean, ops.hip.dt(dtype), mask)
                contexts[key] = clean.transpose(0, 1)
                contexts[key + '_mask'] = mask if mask.is_cuda else mask.bool()    # (uint8 is what the kernels read)
        return caption_ids, target_ids, contexts

    # ---- :67-140 ------------------------------------------------------------------
    def forward(self, context, image, caption, face_embeds=None, obj_embeds=None, metadata=None, names=None,
                attn_idx=None, encoded=None, caption_weights=None, per_image=1):
        """encoded: optional EncodedBatch of THIS batch produced earlier by `encode(..., ahead=True)`.
        caption_weights: fp32 [rows] or [rows, T] on the captions' device, T = caption length - 1 - the
        loss becomes sum_r sum_t w_rt * -log p(y_rt) over the number of non-pad targets (still bits per token) and every
        token's gradient carries its weight; not differentiated.  A per-row advantage (Trainer.train_self_critical), a mask
        that keeps a forced prefix out of the loss, a weight on entity tokens.  None: exactly the call of before.
        per_image = n: the batch holds B images and B * n captions, caption b * n + j for image b: one pass of the encoders
        and of the layer mix, their outputs repeated n times for the decoder.  1: exactly the call of before."""
        if not hasattr(getattr(self, 'decoder', None), 'project_contexts'):          # an LSTM decoder behind this class
            refuse_weighted_forward(self, caption_weights, per_image)
        output_dict, caption_ids, contexts = self._forward_loss(context, image, caption, face_embeds, obj_embeds, encoded,
                                                                caption_weights, per_image)
        if not self.training and self.evaluate_mode:                       # :92-116
            # (eval_attention: commands/evaluate.py's opt-in - the captions come with their attention maps)
            vm = self._vocab_mask(context, attention=bool(getattr(self, 'eval_attention', False)))
            guide = self._check_guidance(attention=bool(getattr(self, 'eval_attention', False)))
            _, gen_ids, attns = self._generate(caption_ids, contexts, beam_size=getattr(self, 'eval_beam_size', 1),
                                               **({'attention': True} if getattr(self, 'eval_attention', False) else {}),
                                               **({'vmask': vm} if vm is not None else {}),
                                               **({'guide': guide} if guide is not None else {}))
            self._forward_generated(output_dict, gen_ids, attns, metadata)
        self.n_samples += caption_ids.shape[0]
        self.n_batches += 1
        return output_dict

    def _forward_loss(self, context, image, caption, face_embeds=None, obj_embeds=None, encoded=None, caption_weights=None,
                      per_image=1):
        """:67-88 - encoders, teacher-forced decoder pass, loss in bits per token -> (output_dict, caption_ids, contexts)."""
        caption_ids, target_ids, contexts = self._forward(context, image, caption, face_embeds, obj_embeds, encoded,
                                                          per_image)
        decoder_out = self.decoder(caption, contexts)
        if caption_weights is None:
            loss_sum, sample_size = self.criterion(self.decoder.adaptive_softmax, decoder_out, target_ids)
        else:
            loss_sum, sample_size = self.criterion(self.decoder.adaptive_softmax, decoder_out, target_ids,
                                                   row_weight=check_caption_weights(caption_weights, target_ids))
        loss = ops.loss_bits(loss_sum, sample_size)                        # :85-88, bits per token
        return {'loss': loss, 'sample_size': sample_size.reshape(())}, caption_ids, contexts

    def _forward_generated(self, output_dict, gen_ids, attns, metadata):
        """:92-116 - what evaluate mode adds to the output once the captions are decoded: ids, text, per-sample BLEU."""
        ids_cpu = gen_ids.cpu()
        output_dict['gen_ids'] = ids_cpu.numpy()
        self._attn_output(output_dict, attns)
        gen_texts = [self.detokenize(x[x > 1]) for x in ids_cpu]        # :96 "we ignore <s> and <pad>"
        output_dict['generations'] = gen_texts
        if metadata is not None:
            captions = [m.get('caption') or '' for m in metadata]
            output_dict['captions'] = captions
            output_dict['metadata'] = metadata
            import re
            from ..metrics import BleuScorer
            gens = [re.sub(r'[^\w\s]', '', t) for t in gen_texts]       # :105-106 remove punctuation
            refs = [re.sub(r'[^\w\s]', '', t) for t in captions]
            for gen, ref in zip(gens, refs):                            # :108-116
                scorer = BleuScorer(n=4)
                scorer += (gen, [ref])
                score, _ = scorer.compute_score(option='closest')
                for k in range(4):
                    self.sample_history['bleu-%d' % (k + 1)] += score[k] * 100

    def detokenize(self, ids):
        """`self.roberta.decode(ids)` of the reference (:96): BPE ids -> text.  Uses the encoder's own `decode` when it
        has one (a fairseq hub model), else the byte-level BPE of the data plane when its files are installed
        (data/indexers.bpe_directory), else the ids themselves as space-separated words (synthetic data has no text)."""
        dec = getattr(self.roberta, 'decode', None)
        if callable(dec):
            try:
                return dec(ids)
            except Exception:                                   # noqa: BLE001 - fall through to the local tokenizer
                pass
        bpe = self.__dict__.get('_bpe')
        if bpe is None:
            from ..data.bpe import RobertaBPE
            from ..data.indexers import bpe_directory
            try:
                bpe = RobertaBPE(bpe_directory())
            except FileNotFoundError:
                bpe = False
            self.__dict__['_bpe'] = bpe
        if bpe:
            return bpe.decode(ids)
        return ' '.join(str(int(i)) for i in ids if int(i) != 2)

    def generate(self, context, image, caption, face_embeds=None, obj_embeds=None, metadata=None, names=None,
                 attn_idx=None, beam_size=1, encoded=None, attention=False, n_best=1, prefix=None, n_samples=1,
                 rank_by='score', rank_len_penalty=0.0, banned=None, ground=None, guidance=None, guidance_drop=None,
                 token_stats=0):
        """encoded: optional EncodedBatch of THIS batch produced earlier by `encode(..., ahead=True)`.
        token_stats = n (0..8; per-token statistics): every step of the cached generator also leaves, for
        the token it took, the n best tokens of the MODEL'S OWN distribution (no temperature, penalty, mask), the token's rank in
        it (0 = the arg-max), its log-prob and the distribution's entropy in nats - one more launch behind the pick, inside the
        captured step.  Adds, with steps = gen_ids.shape[1] - 1: 'alt_ids' int64 [B, steps, n], 'alt_log_probs' fp32 [B, steps,
        n], 'token_rank' int64 [B, steps], 'token_entropy' fp32 [B, steps], 'token_model_lp' fp32 [B, steps]; positions behind a
        row's </s> hold pad, 0, -1, 0, 0.  With n_samples > 1 also their '_samples' forms [B, n_samples, steps, ...] in rank
        order (the plain keys are the first rank).  Greedy and every sampling rule, with the search options, penalties, masks,
        a prefix and attention maps; refused for beam search / n_best and guidance.  0: exactly the call of before.
        guidance = gamma / guidance_drop = names (context guidance; None: the model's `guidance_scale` /
        `guidance_drop`): every step is decoded twice in one static batch - with all contexts, and with the contexts in
        `guidance_drop` (out of image / article / faces / obj) fully masked - and the pick follows
        s = lp_c + (gamma - 1) * (lp_c - lp_u), reported as the normalised log-prob s - logsumexp(s): gamma > 1 rewards the
        tokens the dropped contexts made more likely, 0 <= gamma < 1 interpolates towards the decode without them.  Greedy and
        beam search (with beam_len_penalty and n_best); 'log_probs' / 'scores' then hold the guided log-probs.  gamma = 1.0:
        exactly the call of before.
        banned / ground (vocabulary masks): banned - bool [V] or [B, V] - lists tokens no caption (of
        that row) may contain; ground - bool [V], or True for `name_tokens()`, the BPE pieces that start a capitalised word -
        is a class of tokens that may be generated only if they occur in the row's own article context[index] (the class is per
        token, not per word: continuation pieces are unconstrained).  The model's `suppress_tokens` joins `banned`,
        `ground_names` means ground=True.  A masked token is never picked - greedy, beam search (with its search options and
        n_best) and top-k sampling (with n_samples), with or without a prefix; every reported log-prob is the model's own
        (nothing is renormalised), </s> is always allowed, a forced prefix token still wins.  None / None with the model's keys
        at their defaults: exactly the call of before.
        n_samples = n (2..16; a sampling model): n draws per image from ONE pass of the encoders and ONE
        cached context - row b * n + j of the decode step is draw j of image b, keyed (seed, b * n + j, step): under the same
        torch.manual_seed the draws of the batch with every image repeated n times.  Adds 'gen_ids_samples' [B, n, L],
        'log_probs_samples' [B, n, L - 1], 'scores_samples' [B, n] in rank order, 'sample_index' [B, n] (the draw in every rank
        slot) and 'duplicate' [B, n] bool (an earlier draw of the image has the same tokens); 'gen_ids' / 'log_probs' /
        'scores' are the first rank.  rank_by: 'draw' (draw order, duplicates flagged only), 'score' (sum of the recorded
        log-probs * len ** -rank_len_penalty, best first) or 'consensus' (mean bigram overlap with the other draws); with the
        last two every duplicate ranks behind every non-duplicate (tell_sample_rank).  A prefix row is shared by the n
        hypotheses of its image.  n_samples = 1: exactly the call of before.
        prefix (caption completion): int64 [B, P], the tokens every caption starts with after <s>,
        right-padded with padding_idx (`check_prefix`; `encode_prefix` builds it from strings).  Row r's first plen[r] steps take
        the prefix token instead of the model's pick - inside the decode step, every mode of the cached generators - and
        report the model's log-prob of it; 'gen_ids' is <s>, the prefix, the generated rest, 'log_probs' has one entry per
        step (forced steps: the teacher-forced log-probs), 'prefix_len' [B] is plen.  None: exactly the launches of before.
        'scores' [B]: the score of every caption (sum of its log-probs; beam search with `beam_len_penalty` alpha: * len ** -alpha).
        With `repetition_penalty` / `presence_penalty` / `frequency_penalty` set every pick is taken over
        penalised scores s = min(lp, 0) * theta - (alpha + beta * count) for the tokens the caption already holds, and
        'log_probs' / 'scores' (and their n-best forms) then hold THOSE SCORES, not log-probs - the convention of the
        generators that introduced these penalties; forced prefix steps still report the model's own log-prob.
        n_best = n (2..beam_size): also 'gen_ids_nbest' [B, n, L], 'log_probs_nbest' [B, n, L - 1], 'scores_nbest' [B, n] - the
        n best hypotheses of the beam, best first ('gen_ids' / 'log_probs' stay hypothesis 0).
        attention=True (greedy / top-k / nucleus, DynamicConv decoders): 'attns' is a dict name -> fp32 device tensor
        [B, steps, n_layers, S_name + 2] of head-averaged attention weights, one row per generated token and decoder layer
        (steps = gen_ids.shape[1] - 1; columns: the S context positions, the learned bias_k key, the zero key), and
        'attn_steps' [B] is the number of steps a row took part in, THE STEP THAT PRODUCED ITS </s> INCLUDED (= the column of
        </s> in gen_ids; `steps` for a row that never ended): maps[b, :attn_steps[b] - 1] are the steps of the words of an ended
        row, maps[b, attn_steps[b]:] what the static batch computed after it.  The tokens and log-probs are bit for bit those of attention=False.  `caption_attention` turns the maps into the
        reference's per-word view.  Default: 'attns' is [] on the cached generators."""
        if attention:
            self._check_attention(beam_size)
        self._check_options(beam_size, attention, n_best)
        ns = self._check_n_samples(n_samples, rank_by, rank_len_penalty, beam_size, attention)
        # (prefix=None reads nothing of the batch here: the default path is the path of before)
        pfx = None if prefix is None else self._check_prefix(prefix, caption[self.index].shape[0])
        vm = self._vocab_mask(context, banned, ground, attention)
        guide = self._check_guidance(guidance, guidance_drop, attention, prefix, n_samples, banned, ground)
        ts = self._check_token_stats(token_stats, beam_size, n_best, guide)
        caption_ids, _, contexts = self._forward(context, image, caption, face_embeds, obj_embeds, encoded)
        log_probs, gen_ids, attns = self._generate(caption_ids, contexts, attn_idx, beam_size=beam_size, attention=attention,
                                                   **({'n_best': n_best} if n_best != 1 else {}),
                                                   **({'token_stats': ts} if ts else {}),
                                                   **({'guide': guide} if guide is not None else {}),
                                                   **({'samples': ns} if ns is not None else {}),
                                                   **({'vmask': vm} if vm is not None else {}),
                                                   prefix=pfx)
        out = self._attn_output({'gen_ids': gen_ids, 'log_probs': log_probs}, attns)
        if pfx is not None:
            out['prefix_len'] = pfx[1].to(gen_ids.device, torch.long)
        return out

    @torch.no_grad()
    def score_captions(self, batch, token_stats=0):
        """token_stats = n (1..8): also the five per-token arrays of generate(token_stats=n) for the batch's own captions -
        'alt_ids' / 'alt_log_probs' [B, T - 1, n], 'token_rank' / 'token_entropy' / 'token_model_lp' [B, T - 1]: where the model
        ranks every reference token, what it would have preferred and how flat its distribution was; neutral values (pad, 0,
        -1, 0, 0) behind a row's </s>.  They come from the same launch as generate's (the forced-prefix path).
        How likely the model finds the batch's OWN captions: the caption after <s>, its </s> included, is forced token by
        token through the greedy cached generator (generate(prefix=...)).  -> {'log_probs' [B, T - 1]: the teacher-forced
        log-prob of every caption token (0 behind a row's </s>), 'scores' [B]: their sum, 'prefix_len' [B]: tokens scored}.
        The captions may be at most gen_len (100) tokens long."""
        cap = batch['caption'][self.index]
        prefix = cap[:, 1:].contiguous()
        f = {k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()
             if k in ('context', 'image', 'caption', 'face_embeds', 'obj_embeds', 'encoded')}
        n_ts = check_token_stats(token_stats)
        out = self.generate(**f, prefix=prefix, **({'token_stats': n_ts} if n_ts else {}))
        plen = out['prefix_len']
        lp = out['log_probs']
        T = prefix.shape[1]
        full = lp.new_zeros(lp.shape[0], T)
        n = min(T, lp.shape[1])
        full[:, :n] = lp[:, :n]
        live = torch.arange(T, device=lp.device).unsqueeze(0) < plen.unsqueeze(1)
        full = full * live
        res = {'log_probs': full, 'scores': full.sum(1), 'prefix_len': plen}
        if n_ts:
            neutral = token_stats_neutral(lp.shape[0], T, n_ts, self.padding_idx, lp.device)
            for k_ in TOKEN_STATS_KEYS:
                t = neutral[k_]
                t[:, :n] = out[k_][:, :n]
                keep = live if t.dim() == 2 else live.unsqueeze(-1)
                res[k_] = torch.where(keep, t, token_stats_neutral(1, 1, n_ts, self.padding_idx, lp.device)[k_])
        return res

    def caption_confidence(self, batch, gen, bpe=None):
        """The word-level view of `gen = generate(**batch, token_stats=n)` (attention_maps.caption_confidence)."""
        from .attention_maps import caption_confidence
        return caption_confidence(self, batch, gen, bpe=bpe)

    def caption_attention(self, batch, gen, bpe=None):
        """The reference's per-word attention view of `gen = generate(**batch, attention=True)` (attention_maps.py)."""
        from .attention_maps import caption_attention
        return caption_attention(self, batch, gen, bpe=bpe)

    def lanes_usable(self):
        """Whether `generate_lanes` has a decode loop to interleave: the K/V-cached static-batch generator on a GPU."""
        return (self.fast_generation and hasattr(self.decoder, 'project_contexts')
                and next(self.parameters()).is_cuda)

    @torch.no_grad()
    def generate_lanes(self, batches, beam_size=1, lanes=2, forward=False, attention=False, n_best=1, n_samples=1,
                       rank_by='score', rank_len_penalty=0.0, banned=None, ground=None, guidance=None, guidance_drop=None,
                       token_stats=0):
        """Captions for a sequence of batches with `lanes` decode loops IN FLIGHT TOGETHER, each on its own stream with its
        own DecodeStepper - captured step, static buffers and counters (_decode_stepper(lane=)): a decode step is a chain of ~40 dependent
        launches that each fill the chip for a few microseconds and then wait on memory - at 12-27 % of the HBM roofline a second
        chain fits beside the first.  The host alternates the lanes' graph replays (one replay per lane and token).  The
        encoders of a group of batches run first (eval mode: no randomness, results identical to `generate`).
        Yields (batch, output) in order.  forward=True: the outputs of `forward` in evaluate mode (loss + captions + per-sample
        BLEU bookkeeping: what commands/evaluate.py consumes) instead of `generate`'s; beam_size then is `eval_beam_size`.
        n_samples / rank_by / rank_len_penalty: as `generate` - every lane decodes the n hypotheses of its batch's images.
        banned (bool [V]) / ground (bool [V] or True): the shared forms of `generate`'s vocabulary masks, applied to every batch
        (each row grounded in its own article).
        guidance / guidance_drop: as `generate` - every lane decodes its batch and the batch's unconditional twin.
        token_stats: refused here (0 only); `generate` keeps the per-token statistics."""
        if check_token_stats(token_stats):
            raise ValueError('token_stats=%d: %s' % (token_stats, TOKEN_STATS_REFUSALS['lanes']))
        if banned is not None and (not torch.is_tensor(banned) or banned.dim() != 1):
            raise ValueError('generate_lanes takes the shared form of banned: a bool tensor [V]')
        ns = self._check_n_samples(n_samples, rank_by, rank_len_penalty, beam_size, attention, forward)
        guide = self._check_guidance(guidance, guidance_drop, attention, None, n_samples, banned, ground)
        if forward and (guidance is not None or guidance_drop is not None):   # (forward=True decodes under the model's keys)
            raise ValueError('guidance / guidance_drop as arguments go with generate, not with forward=True')
        gkw = {'guide': guide} if guide is not None else {}
        if attention:
            if forward:
                raise ValueError('attention=True goes with generate, not with forward=True')
            self._check_attention(beam_size)
        if forward:
            beam_size = getattr(self, 'eval_beam_size', 1)
            if getattr(self, 'eval_attention', False) and not self.training and self.evaluate_mode:
                self._check_attention(beam_size)
                attention = True
            if self.training or not self.evaluate_mode or not self.lanes_usable():
                yield from self.generate_stream(batches, forward=True)  # nothing to decode / no static-batch decode loop
                return
        self._check_beam(beam_size)
        self._check_options(beam_size, attention, n_best)
        self._check_penalties(attention)
        it = iter(batches)
        main = torch.cuda.current_stream()
        lane_streams = [streams.get('decode_lane_%d' % i) for i in range(lanes)]
        while True:
            group = []
            for _ in range(lanes):
                b = next(it, None)
                if b is not None:
                    group.append(b)
            if not group:
                return
            gens, outs, heads, thirds, plens = [], [None] * len(group), [], [None] * len(group), []
            for ln, b in enumerate(group):
                f = {k: v for k, v in b.items() if k in ('context', 'image', 'caption', 'face_embeds', 'obj_embeds')}
                if forward:
                    od, caption_ids, contexts = self._forward_loss(**f)
                    heads.append((od, b.get('metadata'), caption_ids.shape[0]))
                else:
                    caption_ids, _, contexts = self._forward(**f)
                # (sampling: the batch's seed is drawn here, in batch order - the draws of `generate` batch by batch)
                seed = draw_seed() if self._sampling() is not None else None
                if b.get('prefix') is not None and forward:
                    raise ValueError('prefix goes with generate, not with forward=True')
                pfx = self._check_prefix(b.get('prefix'), caption_ids.shape[0])
                if guide is not None and pfx is not None:
                    self._check_guidance(guidance, guidance_drop, prefix=pfx)
                plens.append(pfx[1] if pfx is not None else None)
                vm = self._vocab_mask(b['context'], banned, ground, attention)
                vkw = {'vmask': vm} if vm is not None else {}
                ev = torch.cuda.Event()
                ev.record(main)
                lane_streams[ln].wait_event(ev)
                with torch.cuda.stream(lane_streams[ln]), ops.hip.bound_stream():
                    g = (self._beam_steps(caption_ids, contexts, int(beam_size), lane=ln, n_best=n_best, prefix=pfx, **vkw, **gkw)
                         if beam_size > 1 else
                         self._greedy_steps(caption_ids, contexts, lane=ln, seed=seed, attention=attention, prefix=pfx,
                                            **({'n': ns[0], 'rank': ns[1:]} if ns is not None else {}), **vkw, **gkw))
                gens.append(g)
            live = list(range(len(group)))
            while live:
                for ln in list(live):
                    with torch.cuda.stream(lane_streams[ln]), ops.hip.bound_stream():
                        try:
                            next(gens[ln])
                        except StopIteration as done:
                            lp, ids, attns = done.value
                            outs[ln] = self._attn_output({'gen_ids': ids, 'log_probs': lp}, attns)
                            if plens[ln] is not None:
                                outs[ln]['prefix_len'] = plens[ln].to(ids.device, torch.long)
                            thirds[ln] = attns
                            live.remove(ln)
            for ln in range(len(group)):
                ev = torch.cuda.Event()
                ev.record(lane_streams[ln])
                main.wait_event(ev)
            for ln, (b, o) in enumerate(zip(group, outs)):
                if forward:
                    od, metadata, n = heads[ln]
                    self._forward_generated(od, o['gen_ids'], thirds[ln], metadata)
                    self.n_samples += n
                    self.n_batches += 1
                    o = od
                yield b, o

    def generate_stream(self, batches, beam_size=1, forward=False, attention=False, n_best=1, token_stats=0):
        """Captions for a sequence of batches (the test-set loop of tell/commands/evaluate.py:118-160) with the frozen
        encoders of batch N+1 launched on their own streams BEFORE the decode loop of batch N is issued - the trainer's
        schedule applied to generation.  Numerics are those of `generate` / `forward` batch by batch: the encoders read
        nothing the decode loop writes, and consecutive batches' encoder outputs live in different buffer sets.

        MEASURED (MI355X, full model, 32 captions x 100 steps): 534 -> 544 captions/s greedy, 375 -> 381 beam 4 - not the
        25 % the two legs' sum promises.  A decode step is ~44 dependent launches of 5-20 us whose workgroups fill the
        chip for one round each; every one of them queues behind a wave of 100-us GEMM workgroups of the encoders, so
        the two mostly take turns.  Giving the decode chain compute units of its own (hipExtStreamCreateWithCUMask
        streams - hipGraph replays launched on them DO keep the mask, tools/probes/cumask_probe.hip) was built and
        measured: 64 / 128 CUs for the chain -> 260 / 416 captions/s - the chain's kernels are one round of
        latency-bound workgroups on 256 CUs and become two / four rounds on fewer (profiles/r05_cu_partition.txt); not
        kept.  What moves generation throughput is the batch (the iterator's knob): 544 / 747 / 939 captions/s greedy at
        32 / 64 / 128 captions per batch.

        batches: any iterable of batch dicts (keys of `forward`); forward=True yields `self(**batch)` (evaluate mode:
        loss + generation + metrics) instead of `generate(**batch)`.  Yields (batch, output_dict) in order.
        token_stats: refused here (0 only); `generate` keeps the per-token statistics."""
        if check_token_stats(token_stats):
            raise ValueError('token_stats=%d: %s' % (token_stats, TOKEN_STATS_REFUSALS['lanes']))
        if attention:
            if forward:
                raise ValueError('attention=True goes with generate, not with forward=True')
            self._check_attention(beam_size)
        gen_kw = {'attention': True} if attention else {}
        if n_best != 1:
            if forward:
                raise ValueError('n_best goes with generate, not with forward=True')
            gen_kw['n_best'] = n_best
        it = iter(batches)
        cur = next(it, None)
        enc = None
        while cur is not None:
            nxt = next(it, None)
            ahead = None
            can = hasattr(self, 'encode') and torch.is_tensor(cur.get('image')) and cur['image'].is_cuda
            if can and enc is None:
                enc = self.encode(cur['context'], cur['image'])
            if can and nxt is not None and torch.is_tensor(nxt.get('image')) and nxt['image'].is_cuda:
                ahead = self.encode(nxt['context'], nxt['image'], ahead=True)
            if enc is not None and enc.stale():
                enc = self.encode(cur['context'], cur['image'])
            extra = {'encoded': enc} if enc is not None else {}
            if forward and cur.get('prefix') is not None:
                raise ValueError('prefix goes with generate, not with forward=True')
            out = self(**{k_: v_ for k_, v_ in cur.items() if k_ != 'prefix'}, **extra) if forward else self.generate(**cur, beam_size=beam_size, **extra, **gen_kw)
            yield cur, out
            cur, enc = nxt, ahead

    # ---- :399-494 -----------------------------------------------------------------
    fast_generation = True      # projected-K/V cache + static batch; False = the reference's control flow

    def _generate(self, caption_ids, contexts, attn_idx=None, gen_len=100, eos=2, beam_size=1, attention=False, n_best=1,
                  prefix=None, samples=None, vmask=None, guide=None, token_stats=0):
        opts = self._check_options(beam_size, attention, n_best, gen_len)
        # (n, as checked by _check_token_stats: lives in the cached greedy / sampling generator, like `opts`)
        skw = {'stats': self._check_token_stats(token_stats, beam_size, n_best, guide)} if token_stats else {}
        if guide is not None:                 # (drop, gamma) of _check_guidance: lives in the cached generators, like `opts`
            self._check_guidance(guide[1], guide[0], attention, prefix, samples[0] if samples is not None else 1,
                                 True if vmask is not None else None)
            self._check_beam(beam_size)
            if beam_size > 1:
                return self._generate_beam(caption_ids, contexts, beam_size, gen_len, eos, n_best=n_best, guide=guide)
            return self._generate_cached(caption_ids, contexts, gen_len, eos, guide=guide)
        if self._check_penalties(attention) is not None:      # (the penalties live in the cached generators, like `opts`)
            opts = opts or (0.0, 0, 0)
        if prefix is not None:                # (prefix, plen) of _check_prefix: lives in the cached generators, like `opts`
            self._check_prefix(prefix[0], caption_ids.shape[0], gen_len, eos)
        if vmask is not None:                 # (ctx_ids, cls_bits, deny8) of _vocab_mask: lives in the cached generators
            self._check_mask_options(True, None, attention)
            if not hasattr(self.decoder, 'project_contexts'):
                raise ValueError('vocabulary masks cover the cached DynamicConv generator only')
            self._check_beam(beam_size)
            vkw = {'vmask': vmask}
            if beam_size > 1:
                return self._generate_beam(caption_ids, contexts, beam_size, gen_len, eos, n_best=n_best, prefix=prefix, **vkw)
            return self._generate_cached(caption_ids, contexts, gen_len, eos, prefix=prefix, samples=samples, **vkw, **skw)
        if attention:
            # attention maps: always the cached static-batch generator (fast_generation = False is the reference's control
            # flow with the legacy need_attn export, which stays what it is)
            self._check_attention(beam_size)
            return self._generate_cached(caption_ids, contexts, gen_len, eos, attention=True, prefix=prefix, **skw)
        if not hasattr(self.decoder, 'project_contexts'):
            # a recurrent decoder behind this model class (expt/*/3_lstm_roberta: `lstm_decoder_flattened`): greedy
            # decode that carries the LSTM state.  (The reference's loop feeds such a decoder only the last token with
            # an incremental_state its LSTMDecoder ignores, i.e. every step restarts from the initial state -
            # transformer_flattened.py:_generate with decoder_flattened_lstm.py:131-152; not reproduced.)
            from .baseline_glove import BaselineGloveModel
            lps, ids = BaselineGloveModel._generate(self, caption_ids, contexts, gen_len, eos)
            return lps, ids, []
        self._check_beam(beam_size)
        if beam_size > 1:
            return self._generate_beam(caption_ids, contexts, beam_size, gen_len, eos, n_best=n_best, prefix=prefix)
        if samples is not None:
            return self._generate_cached(caption_ids, contexts, gen_len, eos, prefix=prefix, samples=samples, **skw)
        if self.fast_generation or opts is not None or prefix is not None or skw:  # (the search options live in the cached generator)
            return self._generate_cached(caption_ids, contexts, gen_len, eos, prefix=prefix, **skw)
        return self._generate_reference_flow(caption_ids, contexts, attn_idx, gen_len, eos)

    @staticmethod
    def _drive(gen):
        """Run a decode generator (one `yield` per issued step) to its result."""
        try:
            while True:
                next(gen)
        except StopIteration as done:
            return done.value

    @torch.no_grad()
    def _generate_cached(self, caption_ids, contexts, gen_len=100, eos=2, check_every=8, lane=0, attention=False, prefix=None,
                         samples=None, vmask=None, guide=None, stats=0):
        # (prefix only when given: a stand-in for _greedy_steps without that parameter keeps working - tests/test_attn_maps_host.py)
        return self._drive(self._greedy_steps(caption_ids, contexts, gen_len, eos, check_every, lane, attention=attention,
                                              **({'prefix': prefix} if prefix is not None else {}),
                                              **({'n': samples[0], 'rank': samples[1:]} if samples is not None else {}),
                                              **({'vmask': vmask} if vmask is not None else {}),
                                              **({'guide': guide} if guide is not None else {}),
                                              **({'stats': stats} if stats else {})))

    def _greedy_steps(self, caption_ids, contexts, gen_len=100, eos=2, check_every=8, lane=0, seed=None, attention=False,
                      prefix=None, n=1, rank=('score', 0.0), vmask=None, guide=None, stats=0):
        """A generator: yields after every issued decode step (generate_lanes interleaves two of these on two streams), returns
        (log_probs, ids, []).  Same greedy decode, restructured for the GPU: (1) context K/V projected once per caption,
        (2) the batch keeps its shape - finished rows are masked instead of compacted, so there is no
        per-step gather of the contexts and no per-step host synchronisation (the all-finished test
        runs every `check_every` steps), (3) fused arg-max over the adaptive softmax.  Rows are
        independent, so every row sees exactly the arithmetic of the reference flow: token ids are
        identical, pad=1 after EOS, output length = 1 + steps until the last row finished.
        sampling_topk > 1: the head's last launch draws from the top k instead (tell_adaptive_logprob_sample), keyed on
        (seed, row, step) - `seed` (default: drawn now, draw_seed) goes into the stepper's device word before the first step.
        attention=True: every step also leaves its head-averaged attention weights in the stepper's sink (step.attn, one slot
        per step); the third result is then an AttnMaps (maps {name: [B, steps, n_layers, S + 2] fp32}, steps [B]) instead of [].
        prefix = (tokens int64 [B, P], plen int32 [B]) of check_prefix: the stepper's forcing table is filled before the first step
        and the head of every step ends in one more launch (tell_adaptive_logprob_forced); the bookkeeping is untouched - it
        books a forced token exactly as a picked one.
        With penalties set (_penalties()): the head counts every row's tokens (step.pen_source over `ids`) and picks - arg-max or
        top-k draw - over the penalised scores, which is what `log_probs` then holds.
        n > 1 (a sampling model; generate(n_samples=n)): R = B * n rows are resident, hypothesis j of image b in row b * n + j -
        cur, ids, lps, done_step and fin8 are R rows tall, the contexts, masks, projected K/V and the prefix stay at width B (as
        _beam_steps hands them to the stepper), one seed, row r draws with (seed, r, step).  Behind the loop one launch
        (tell_sample_rank, rank = (rule, alpha)) scores, de-duplicates and ranks the n hypotheses of every image: the results
        are the first rank's, the third a DecodeInfo with .scores and .samples.
        vmask = (ctx_ids, cls_bits, deny8) of _vocab_mask: the stepper's bitmap - one row per image - is built before the first
        step (step.set_mask) and every pick is the masked one; the bookkeeping is untouched.
        guide = (drop, gamma) of _check_guidance: the batch is decoded with its unconditional twin behind
        it (guided_batch: 2 * images rows), every pick is the guided arg-max - one token and one normalised log-prob for both
        rows of a pair - the bookkeeping runs over all rows unchanged and the results are the first half.
        stats = n_alt in 1..8 (generate(token_stats=)): every head ends in tell_adaptive_logprob_stats,
        which reads the finished flags as they stand BEFORE the step's bookkeeping (step.stats_source) and writes slot = step of
        the stepper's sink; behind the loop the slots become the five [rows, steps(, n_alt)] arrays, carried as .token_stats of
        the third result (a DecodeInfo, or an AttnMapsStats with attention=True)."""
        dec = self.decoder
        n = int(n)
        stats = int(stats)
        if stats and guide is not None:
            raise ValueError('token_stats=%d: %s' % (stats, TOKEN_STATS_REFUSALS['guide']))
        if guide is not None:
            self._check_guidance(guide[1], guide[0], attention, prefix, n, True if vmask is not None else None)
            cond = caption_ids.shape[0]
            caption_ids, contexts = guided_batch(caption_ids, contexts, guide[0])
        images = caption_ids.shape[0]
        B = images * n                                           # decode rows
        dev = caption_ids.device
        kv = dec.project_contexts(contexts)
        sampling = self._sampling()
        opts = self._check_options(1, attention, 1, gen_len)
        # greedy: the bans apply (no_repeat_ngram_size, min_len); the length penalty ranks hypotheses and there is one
        ban = (opts[1], opts[2], int(eos)) if opts is not None and (opts[1] or opts[2]) else None
        pen = self._check_penalties(attention)
        step = self._decode_stepper(B, kv, contexts, gen_len, lane=lane, sample=sampling, attention=attention, ban=ban,
                                    prefix=prefix is not None, **({'pen': pen} if pen is not None else {}),
                                    **({'hyp': n} if n > 1 else {}), **({'mask': True} if vmask is not None else {}),
                                    **({'guide': guide[0]} if guide is not None else {}), **({'stats': stats} if stats else {}))
        if guide is not None:
            step.set_guidance(guide[1])
        if prefix is not None:
            step.set_prefix(*prefix)
        if vmask is not None:
            step.set_mask(*vmask, eos=int(eos))
        if sampling is not None:
            step.seed.fill_(draw_seed() if seed is None else int(seed))
        cur = caption_ids[:, 0:1].contiguous() if n == 1 else caption_ids[:, 0:1].repeat_interleave(n, dim=0).contiguous()
        finished = cur[:, 0] == eos
        fused = caption_ids.is_cuda and step.static              # one bookkeeping launch per token (tell_greedy_update)
        if fused:
            # the histories live in STATIC buffers of the stepper (the bookkeeping launch is part of the captured step)
            bk = step.book('greedy', lambda: dict(
                ids=torch.empty(B, gen_len + 1, dtype=torch.long, device=dev),
                lps=torch.empty(B, gen_len, dtype=torch.float32, device=dev),
                done_step=torch.empty(B, dtype=torch.long, device=dev), fin8=torch.empty(B, dtype=torch.uint8, device=dev)))
            ids, lps, done_step, fin8 = bk['ids'], bk['lps'], bk['done_step'], bk['fin8']
            ids.fill_(self.padding_idx)
            lps.zero_()
            done_step.fill_(gen_len)
            if ban is not None:
                step.ban_source(ids, fin8)
            if pen is not None:
                step.pen_source(ids, fin8)
            if stats:
                step.stats_source(fin8)
        else:
            ids = torch.full((B, gen_len + 1), self.padding_idx, dtype=torch.long, device=dev)
            lps = torch.zeros(B, gen_len, dtype=torch.float32, device=dev)
            done_step = torch.full((B,), gen_len, dtype=torch.long, device=dev)   # steps this row took part in
        ids[:, 0] = cur[:, 0]
        done_step[finished] = 0
        steps = gen_len
        if fused:
            fin8.copy_(finished)
            step.cur.copy_(cur)
            inv_temp = 1.0 / float(self.sampling_temp)

            def book(out, i, step_dev):
                # the step's LAST launch: inside the captured step it takes the step index from the device counter
                # (step_dev), eagerly from the host; either way it leaves the next step's position offset behind
                tok, lp = out
                ops.call('tell_greedy_update', tok.reshape(B), lp.reshape(B), fin8, ids, ids.stride(0), lps, lps.stride(0),
                         done_step, step.cur, B, int(i), int(eos), inv_temp, step.counter_out, step_dev)
            yield from step.steps(gen_len, check_every, book, fin8)
        for i in range(0 if fused else gen_len):
            if ban is not None:
                step.ban_source(ids, finished.to(torch.uint8))
            if pen is not None:
                step.pen_source(ids, finished.to(torch.uint8))
            if stats:
                step.stats_source(finished.to(torch.uint8))
            tok, lp = step(i, cur)
            yield i
            tok = tok.long().view(B)
            lp = lp.view(B) / self.sampling_temp
            ids[:, i + 1] = torch.where(finished, ids[:, i + 1], tok)
            lps[:, i] = torch.where(finished, lps[:, i], lp)
            newly = (~finished) & (tok == eos)
            done_step = torch.where(newly, torch.full_like(done_step, i + 1), done_step)
            finished = finished | newly
            cur = tok.view(B, 1)
            if (i + 1) % check_every == 0 and bool(finished.all()):
                break
        steps = int(done_step.max())                                          # one sync at the end
        steps = max(steps, 1)
        ts = self._token_stats_arrays(step.stats, steps) if stats else None
        if n > 1:
            return self._rank_samples(ids, lps, done_step, images, n, steps, gen_len, eos, rank,
                                      **({'stats': ts} if ts is not None else {}))
        attns = []
        if ts is not None:
            attns = DecodeInfo()
            attns.token_stats = ts
        if attention:
            # slot i of a layer's buffer = step i (the token at ids[:, i + 1]); copied out: the buffers belong to the stepper
            bufs = step.attn.bufs
            attns = (AttnMapsStats if ts is not None else AttnMaps)(
                {n: torch.stack([lb[n][:steps] for lb in bufs], 0).permute(2, 1, 0, 3).contiguous() for n in bufs[0]},
                done_step.clamp(max=steps).clone())
            if ts is not None:
                attns.token_stats = ts
        if guide is not None:                                                 # (the unconditional twins took the same decisions)
            return lps[:cond, :steps].clone(), ids[:cond, :steps + 1].clone(), attns
        if fused:                                                             # (the static buffers belong to the stepper)
            return lps[:, :steps].clone(), ids[:, :steps + 1].clone(), attns
        return lps[:, :steps], ids[:, :steps + 1], attns

    @staticmethod
    def _token_stats_arrays(sink, steps):
        """The first `steps` slots of a decode.StatsSink [slots, rows(, n)] -> the five arrays of generate(token_stats=n),
        [rows, steps(, n)] (copies: the buffers belong to the stepper)."""
        return {'alt_ids': sink.alt_tok[:steps].permute(1, 0, 2).long().contiguous(),
                'alt_log_probs': sink.alt_lp[:steps].permute(1, 0, 2).contiguous(),
                'token_rank': sink.rank[:steps].t().long().contiguous(),
                'token_entropy': sink.entropy[:steps].t().contiguous(),
                'token_model_lp': sink.chosen_lp[:steps].t().contiguous()}

    def _rank_samples(self, ids, lps, done_step, B, n, steps, gen_len, eos, rank, stats=None):
        """The end of _greedy_steps with n > 1 hypotheses per image: ids [B * n, gen_len + 1], lps [B * n, gen_len], done_step
        [B * n] of the decode loop -> (log_probs [B, steps], ids [B, steps + 1] of the first rank, DecodeInfo).  One launch
        (tell_sample_rank; hypotheses on the CPU: its host definition), then the gathers by its order."""
        rule, alpha = rank
        inv_norm = inv_norm_table(alpha, gen_len).to(ids.device) if alpha else None
        if ids.is_cuda:
            order, score, dup = ops.sample_rank(ids, lps, done_step, B, n, steps, self.padding_idx, eos, rule, inv_norm=inv_norm)[:3]
        else:
            d = sample_rank_definition(ids.numpy(), lps.numpy(), done_step.numpy(), n, steps, eos, rule,
                                       None if inv_norm is None else inv_norm.numpy())
            order, score, dup = (torch.from_numpy(d[k_]) for k_ in ('order', 'score', 'dup'))
        order = order.long()

        def ranked(t):                                            # [B * n, W] -> [B, n, W] in rank order (a new tensor)
            t = t.reshape(B, n, -1)
            return t.gather(1, order.unsqueeze(-1).expand(-1, -1, t.shape[-1]))
        info = DecodeInfo()
        info.samples = {'gen_ids_samples': ranked(ids[:, :steps + 1]), 'log_probs_samples': ranked(lps[:, :steps]),
                        'scores_samples': score.gather(1, order), 'sample_index': order,
                        'duplicate': dup.gather(1, order).bool()}
        info.scores = info.samples['scores_samples'][:, 0].contiguous()
        if stats is not None:                                     # the per-token statistics of every draw, in rank order too
            for k_, t in stats.items():
                t = t.reshape(B, n, *t.shape[1:])
                info.samples[k_ + '_samples'] = t.gather(1, order.view(B, n, *([1] * (t.dim() - 2))).expand_as(t))
            info.token_stats = {k_: info.samples[k_ + '_samples'][:, 0].contiguous() for k_ in stats}
        return (info.samples['log_probs_samples'][:, 0].contiguous(), info.samples['gen_ids_samples'][:, 0].contiguous(), info)

    def _decode_stepper(self, B, kv, contexts, gen_len, topk=0, lane=0, sample=None, attention=False, ban=None, opts=None,
                        prefix=False, pen=None, hyp=1, mask=False, guide=None, hidden=False, stats=0):
        """-> the DecodeStepper (models/stepper.py) of the cached greedy / beam generators for this caption batch: a view over
        the cache entry of its signature in `_decode_graphs` (static buffers, captured graphs), or the eager step."""
        return DecodeStepper(self, B, kv, contexts, gen_len, topk=topk, lane=lane, sample=sample, attention=attention, ban=ban,
                             opts=opts, prefix=prefix, pen=pen, **({'hyp': hyp} if hyp != 1 else {}),
                             **({'mask': True} if mask else {}), **({'guide': guide} if guide is not None else {}),
                             **({'hidden': True} if hidden else {}), **({'stats': stats} if stats else {}))

    @torch.no_grad()
    def _generate_beam(self, caption_ids, contexts, beam_size, gen_len=100, eos=2, check_every=8, lane=0, n_best=1, prefix=None,
                       vmask=None, guide=None):
        return self._drive(self._beam_steps(caption_ids, contexts, beam_size, gen_len, eos, check_every, lane, n_best, prefix=prefix,
                                            **({'vmask': vmask} if vmask is not None else {}),
                                            **({'guide': guide} if guide is not None else {})))

    def _beam_steps(self, caption_ids, contexts, beam_size, gen_len=100, eos=2, check_every=8, lane=0, n_best=1, prefix=None,
                    vmask=None, guide=None):
        """A generator like _greedy_steps.  Beam search on the cached static-shape generator (SURVEY 8-f1 / BASELINE config 5; the reference itself
        only samples top-1, transformer_faces_objects.py:443-464).  B*K rows (row = b*K + j) stay resident; the
        projected K/V of the static contexts are computed once per caption and replicated per beam; the DynamicConv
        input buffers are reordered by parent with the reference's `reorder_incremental_state` contract
        (dynamic.py:338-342).  Score = sum of token log-probs (no length penalty); a finished hypothesis keeps its
        score and is extended with pad only.  -> (log_probs [B,steps], ids [B,steps+1] of the best hypothesis, []).
        With search options: `beam_len_penalty` alpha ranks the candidates by sum * len ** -alpha (len:
        generated tokens, </s> included; frozen when a hypothesis ends), `no_repeat_ngram_size` / `min_len` ban tokens per
        hypothesis before its K best are taken.  The third result is a DecodeInfo (an empty list) with .scores [B] and, for
        n_best = n > 1, .nbest = (ids [B,n,steps+1], log_probs [B,n,steps], scores [B,n]).
        prefix = (tokens, plen) of check_prefix: during a sample's forced steps every hypothesis' candidate list is the forced
        token and K - 1 fillers (-inf, pad), so only slot 0 stays live - as at step 0 - and the beam opens at the first free
        step; the bookkeeping is untouched.
        With penalties set (_penalties()): every hypothesis' K best are taken over its penalised scores (step.pen_source over
        `seqs`), and `cum`, the log_probs and the scores accumulate those scores.
        vmask = (ctx_ids, cls_bits, deny8) of _vocab_mask: the K hypotheses of a sample share its row of the stepper's bitmap
        (step.set_mask) and every hypothesis' K best are taken under it - with a ban list, in the same launch.
        guide = (drop, gamma) of _check_guidance: samples B .. 2B - 1 are the unconditional twins
        (guided_batch), hypothesis row r's partner is row r + B * K; every pair's K candidates come from the guided pick and are
        the same for both rows, so tell_beam_update takes the same decisions in both halves; the results are the first half."""
        dec = self.decoder
        if guide is not None:
            self._check_guidance(guide[1], guide[0], False, prefix, 1, True if vmask is not None else None)
            cond = caption_ids.shape[0]
            caption_ids, contexts = guided_batch(caption_ids, contexts, guide[0])
        B, K = caption_ids.shape[0], int(beam_size)
        dev = caption_ids.device
        pad = self.padding_idx
        opts = self._check_options(K, False, n_best, gen_len)
        alpha = opts[0] if opts is not None else 0.0
        ban = (opts[1], opts[2], int(eos)) if opts is not None and (opts[1] or opts[2]) else None
        rep = lambda t, dim: t.repeat_interleave(K, dim=dim).contiguous()           # noqa: E731
        # contexts, masks and projected K/V stay at batch B: the attention modules present the K hypotheses of a
        # sample as K query positions of that sample (modules/attention.py), nothing is replicated per beam
        ctx = {k_: v_ for k_, v_ in contexts.items() if torch.is_tensor(v_)}
        kv = dec.project_contexts(contexts)
        pen = self._check_penalties()
        step = self._decode_stepper(B * K, kv, ctx, gen_len, topk=K, lane=lane, ban=ban,
                                    opts=(opts + (int(eos),)) if opts is not None else None, prefix=prefix is not None,
                                    **({'pen': pen} if pen is not None else {}), **({'mask': True} if vmask is not None else {}),
                                    **({'guide': guide[0]} if guide is not None else {}))
        if guide is not None:
            step.set_guidance(guide[1])
        if prefix is not None:
            step.set_prefix(*prefix)
        if vmask is not None:
            step.set_mask(*vmask, eos=int(eos))
        cur = rep(caption_ids[:, 0:1], 0)
        finished = (cur[:, 0] == eos).view(B, K)
        fused = caption_ids.is_cuda and step.static and K <= 8 and gen_len + 1 <= 256
        if fused:
            bk = step.book('beam', lambda: dict(
                cum=torch.empty(B, K, dtype=torch.float32, device=dev), fin8=torch.empty(B, K, dtype=torch.uint8, device=dev),
                seqs=torch.empty(B, K, gen_len + 1, dtype=torch.long, device=dev),
                lps=torch.empty(B, K, gen_len, dtype=torch.float32, device=dev),
                rows=torch.empty(B * K, dtype=torch.long, device=dev)))
            cum, fin8, seqs, lps, rows = bk['cum'], bk['fin8'], bk['seqs'], bk['lps'], bk['rows']
            cum.fill_(float('-inf'))
            seqs.fill_(pad)
            lps.zero_()
            if alpha:
                nb = step.book('beam_norm', lambda: dict(len=torch.empty(B, K, dtype=torch.int32, device=dev),
                                                         inv_norm=torch.empty(gen_len + 2, dtype=torch.float32, device=dev)))
                hyp_len, inv_norm = nb['len'], nb['inv_norm']
                hyp_len.zero_()
                inv_norm.copy_(inv_norm_table(alpha, gen_len + 1))
        else:
            cum = torch.full((B, K), float('-inf'), dtype=torch.float32, device=dev)
            seqs = torch.full((B, K, gen_len + 1), pad, dtype=torch.long, device=dev)
            lps = torch.zeros(B, K, gen_len, dtype=torch.float32, device=dev)
            if alpha:
                hyp_len = torch.zeros(B, K, dtype=torch.long, device=dev)
                inv_norm = inv_norm_table(alpha, gen_len + 1).to(dev)
        cum[:, 0] = 0.0                                     # all K rows start identical: only hypothesis 0 counts
        seqs[:, :, 0] = cur.view(B, K)
        base = (torch.arange(B, device=dev) * K).view(B, 1)
        n_steps = gen_len
        if fused:
            # one bookkeeping launch per token (tell_beam_update: candidate scores, top-K per sample, histories gathered
            # by parent, next inputs; ring buffers: it also composes the ancestor table with this step's parents - no row
            # of any layer's DynamicConv buffer is moved) - the LAST launch of the captured step where the stepper allows
            fin8.copy_(finished)
            step.cur.copy_(cur)
            ring = step.back is not None
            inv_temp = 1.0 / float(self.sampling_temp)

            if ban is not None:
                step.ban_source(seqs.view(B * K, gen_len + 1), fin8.view(B * K))
            if pen is not None:
                step.pen_source(seqs.view(B * K, gen_len + 1), fin8.view(B * K))

            def book(out, i, step_dev):
                tk, lp = out
                if alpha:
                    ops.call('tell_beam_update_norm', tk, lp, cum, fin8, seqs, lps, step.cur, rows, hyp_len, inv_norm, B, K,
                             gen_len + 1, int(i), int(pad), int(eos), inv_temp, step.back, step.back.shape[0] if ring else 0,
                             step.counter_out, step_dev)
                    return
                ops.call('tell_beam_update', tk, lp, cum, fin8, seqs, lps, step.cur, rows, B, K, gen_len + 1, int(i), int(pad),
                         int(eos), inv_temp, step.back, step.back.shape[0] if ring else 0, step.counter_out, step_dev)

            def host_book(out, i):
                # (time-ordered buffers - fp32 parity mode: the bookkeeping stays a host-side launch and one more launch
                #  re-orders every layer's rows by parent)
                book(out, i, None)
                step.reorder(rows, K)
            # (multi-step replays need the bookkeeping inside the captured step: ring buffers only)
            n_steps = yield from step.steps(gen_len, check_every, book if ring else None, fin8, multi=ring,
                                            after=None if ring else host_book)
        for i in range(0 if fused else gen_len):
            # each hypothesis contributes its own K best tokens (the best K of K x V always lie among them)
            if ban is not None:
                step.ban_source(seqs.view(B * K, -1).contiguous(), finished.to(torch.uint8).view(B * K).contiguous())
            if pen is not None:
                step.pen_source(seqs.view(B * K, -1).contiguous(), finished.to(torch.uint8).view(B * K).contiguous())
            tk, lp = step(i, cur)
            tk, lp = tk.view(B, K, K).long(), lp.view(B, K, K) / self.sampling_temp
            # a finished hypothesis has ONE continuation: pad, at no cost
            fin = finished.unsqueeze(-1)
            first = torch.zeros(K, dtype=torch.bool, device=dev)
            first[0] = True
            lp = torch.where(fin, torch.where(first, torch.zeros_like(lp), torch.full_like(lp, float('-inf'))), lp)
            tk = torch.where(fin, torch.full_like(tk, pad), tk)
            raw = (cum.unsqueeze(-1) + lp).view(B, K * K)
            if alpha:
                # candidates of a live hypothesis have i + 1 tokens, a finished one keeps its length; one fp32 multiply
                cand_len = torch.where(finished, hyp_len, torch.full_like(hyp_len, i + 1)).unsqueeze(-1).expand(B, K, K)
                score = raw * inv_norm[cand_len.reshape(B, K * K)]
                score = torch.where(torch.isnan(score), torch.full_like(score, float('-inf')), score)
                # (the lowest candidate index wins a tie: a stable descending sort)
                idx = torch.sort(score, dim=1, descending=True, stable=True)[1][:, :K]
                top = raw.gather(1, idx)
                hyp_len = cand_len.reshape(B, K * K).gather(1, idx)
            else:
                top, idx = raw.topk(K, dim=1)                                       # sorted, best first
            parent = idx // K
            tok = tk.view(B, K * K).gather(1, idx)
            rows = (base + parent).view(-1)
            was_finished = finished.gather(1, parent)
            tok = torch.where(was_finished, torch.full_like(tok, pad), tok)
            seqs = seqs.view(B * K, -1).index_select(0, rows).view(B, K, -1)
            lps = lps.view(B * K, -1).index_select(0, rows).view(B, K, -1)
            seqs[:, :, i + 1] = tok
            lps[:, :, i] = torch.where(was_finished, torch.zeros_like(top), top - cum.gather(1, parent))
            finished = was_finished | (tok == eos)
            cum = top
            step.reorder(rows)
            cur = tok.view(B * K, 1)
            yield i
            if (i + 1) % check_every == 0 and bool(finished.all()):
                n_steps = i + 1
                break
        best = seqs[:, 0]                                    # topk keeps hypotheses sorted by score
        n_best = int(n_best)
        # one sync: length of the longest best caption (n_best > 1: of the longest of the n best)
        steps = int((best[:, 1:] != pad).sum(1).max()) if n_best == 1 else int((seqs[:, :n_best, 1:] != pad).sum(2).max())
        steps = max(min(steps, n_steps), 1)
        info = DecodeInfo()
        scores = cum * inv_norm[hyp_len.long()] if alpha else cum      # (the multiply the ranking used)
        if guide is not None:                                # (the unconditional twins took the same decisions)
            seqs, lps, scores, best = seqs[:cond], lps[:cond], scores[:cond], best[:cond]
        info.scores = scores[:, 0].clone()
        if n_best > 1:
            info.nbest = (seqs[:, :n_best, :steps + 1].clone(), lps[:, :n_best, :steps].clone(), scores[:, :n_best].clone())
        if fused:                                            # (the static buffers belong to the stepper)
            return lps[:, 0, :steps].clone(), best[:, :steps + 1].clone(), info
        return lps[:, 0, :steps], best[:, :steps + 1], info

    @torch.no_grad()
    def _generate_reference_flow(self, caption_ids, contexts, attn_idx=None, gen_len=100, eos=2):
        """Greedy decoding with the reference's semantics (finished rows leave the batch, pad=1 after
        EOS, loop ends when no row is active).  The arg-max over the 50 265-way adaptive softmax is
        fused (no [B, vocab] log-prob tensor).  sampling_topk > 1: the fused top-k draw keyed on the alive rows' ORIGINAL
        batch rows, so the captions equal the cached flow's under the same seed."""
        state = {}
        B = caption_ids.shape[0]
        dev = caption_ids.device
        sampling = self._sampling()
        if sampling is not None:
            seed_word = torch.full((1,), draw_seed(), dtype=torch.int32, device=dev)
        seed = caption_ids[:, 0:1]
        alive = seed[:, -1] != eos
        keep = alive
        cur = seed
        log_probs, paths, attns = [], [seed], []
        names = [k for k in contexts if not k.endswith('_mask') and not k.startswith('_')]
        for i in range(gen_len):
            self.decoder.filter_incremental_state(state, keep)                      # :417
            ctx_i = {}
            for n in names:                                                         # :420-431
                ctx_i[n] = contexts[n][:, alive]
                ctx_i[n + '_mask'] = contexts[n + '_mask'][alive]
            dec_out = self.decoder({self.index: cur[:, -1:]}, ctx_i, incremental_state=state)
            attns.append(dec_out[1]['attn'])
            if sampling is None:
                tok, lp = self.decoder.adaptive_softmax.greedy(dec_out[0][:, -1:])  # :443-464
            else:                                                                   # :443-470, topk + multinomial
                rows = alive.nonzero().squeeze(1).to(torch.int32)
                tok, lp = self.decoder.adaptive_softmax.sample(dec_out[0][:, -1:], sampling[0], sampling[1], seed_word, i,
                                                               row_ids=rows, **({'topp': sampling[2]} if len(sampling) > 2 else {}),
                                                               **({'rule': sampling[3]} if len(sampling) > 3 else {}))
            sel_ix = tok.long()
            sel_lp = lp / self.sampling_temp
            full_lp = sel_lp.new_zeros(B, 1)
            full_lp[alive] = sel_lp
            full_ix = sel_ix.new_full((B, 1), self.padding_idx)
            full_ix[alive] = sel_ix
            log_probs.append(full_lp)
            paths.append(full_ix)
            keep = sel_ix.squeeze(-1) != eos                                        # :476-483
            alive = alive.clone()
            alive[alive.nonzero().squeeze(1)[~keep]] = False
            cur = torch.cat([cur, sel_ix], dim=1)[keep]
            if int(keep.sum()) == 0:                                                # :485
                break
        return torch.cat(log_probs, dim=-1), torch.cat(paths, dim=-1), attns

    def get_metrics(self, reset=False):                                             # :504-517
        metrics = {'_n_batches': self.n_batches, '_n_samples': self.n_samples}
        for key, value in self.sample_history.items():
            metrics[key] = value / max(self.n_samples, 1)
        if reset:
            self.n_batches = 0
            self.n_samples = 0
            self.sample_history = defaultdict(float)
        return metrics


@Model.register('transformer_faces_objects')
class TransformerFacesObjectModel(CaptionModel):
    """tell/models/transformer_faces_objects.py:22-23"""
    USE_FACES_OBJECTS = True
    EXTRA_CONTEXTS = ('faces', 'obj')


@Model.register('transformer_faces')
class TransformerFacesModel(CaptionModel):
    """tell/models/transformer_faces.py:21-22 (expt/*/8_transformer_faces): image + article + faces, driven by
    `dynamic_conv_decoder_faces_parallel`; the faces+objects forward without `obj_embeds`."""
    USE_FACES_OBJECTS = True
    EXTRA_CONTEXTS = ('faces',)


@Model.register('transformer_flattened')
class TransformerFlattenedModel(CaptionModel):
    """tell/models/transformer_flattened.py:23-24 (also drives `dynamic_conv_decoder_flattened_no_image`)"""
    USE_FACES_OBJECTS = False
    EXTRA_CONTEXTS = ()
