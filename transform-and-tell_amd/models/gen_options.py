"""The options of caption generation: the pure validators of every key and argument (`check_*`), what the generators hand
back beside the captions (DecodeInfo, AttnMaps), and DecodePlan - the options of ONE decode call, checked in one place - with
the table of what does not combine with what."""
import math
from collections import namedtuple
from typing import NamedTuple, Optional

import torch

from .stepper import TOKEN_STATS_REFUSALS

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


class DecodeInfo(list):
    """Third result of the cached generators without attention maps: the empty list it always was, carrying what
    `generate` reports beside the best hypothesis - scores [B] (beam: the normalised score of hypothesis 0) and, with
    n_best > 1, nbest = (ids [B, n, L], log_probs [B, n, L - 1], scores [B, n]), best first; with n_samples > 1, samples =
    the '*_samples' / 'sample_index' / 'duplicate' entries of the output dict, in rank order."""
    scores = None
    nbest = None
    samples = None
    token_stats = None             # generate(token_stats=n): the five per-token arrays of the output dict (first rank)


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


def draw_seed():
    """The seed of one batch's sampled decode: 31 bits from torch's default CPU generator (torch.manual_seed makes the
    captions reproducible)."""
    return int(torch.randint(0, 1 << 31, (1,)).item())


class AttnMaps(namedtuple('AttnMaps', 'maps steps')):
    """Third result of the cached generator with attention=True (without: the empty list it always was).
    maps: {context name: fp32 [B, steps, n_layers, S + 2]} on the device; steps: [B] long, the row's `done_step` - the
    number of decode steps it took part in, the one that produced its </s> included."""
    __slots__ = ()


class AttnMapsStats(AttnMaps):
    """AttnMaps of a generation that also kept per-token statistics (attention=True, token_stats=n): .token_stats as DecodeInfo's."""
    token_stats = None


# ---- what does not combine with what --------------------------------------------------------------------------------------
# option -> ((partner, reason), ...) in the order its refusals are tested: with `partner` set (OptionChecks._stated) the
# refusal reads '<option> and <partner> do not combine: <reason>'; partner None is the refusal of a model whose decode step
# ends in a decision launch of its own (OptionChecks._cached_only; `reason` is then what covers the cached generator only).
_TRUNCATIONS = ('sampling_topp', 'sampling_minp', 'sampling_typical')
_BANS = ('no_repeat_ngram_size', 'min_len')
_SEARCH = 'the search options apply to the arg-max and beam decodes'
_GUIDED = 'guidance covers the arg-max and beam decodes'
COMBINES = {
    'search': (('truncation', _SEARCH), ('sampling', _SEARCH),
               ('attention', 'attention maps are exported without search options'), (None, 'the search options cover')),
    'penalties': tuple((n, 'the penalties cover the arg-max, beam and top-k sampling decodes') for n in _TRUNCATIONS)
    + tuple((n, 'one list per pick launch') for n in _BANS)
    + (('attention', 'attention maps are exported without penalties'), (None, 'the penalties cover')),
    'mask': tuple((n, 'a vocabulary mask covers the arg-max, beam and top-k sampling decodes') for n in _TRUNCATIONS)
    + (('penalties', 'the penalties\' bitmap means "listed", not "banned"'),
       ('attention', 'attention maps are exported without a vocabulary mask'), (None, 'vocabulary masks cover')),
    'guidance': ((None, 'context guidance covers'), ('sampling_topk', _GUIDED)) + tuple((n, _GUIDED) for n in _TRUNCATIONS)
    + tuple((n, 'the guided pick takes no ban list') for n in _BANS)
    + (('penalties', 'the guided pick takes no penalty list'), ('mask', 'the guided pick takes no vocabulary mask'),
       ('prefix', 'a forced token has no guided log-prob'), ('n_samples', _GUIDED),
       ('attention', 'attention maps are exported without guidance')),
    'n_samples': (('beam', 'n_best is the beam\'s own form'),
                  ('attention', 'attention maps are exported for one hypothesis per sample')),
}


class DecodePlan(NamedTuple):
    """The options of one decode call, each field the checked value the generators take (CaptionModel._plan builds one from
    generate's arguments): prefix = (tokens, plen) of check_prefix, samples = (n, rule, alpha) of check_n_samples, vmask =
    (ctx_ids, cls_bits, deny8) of _vocab_mask, guide = (drop, gamma) of _check_guidance, stats = n of check_token_stats.
    The sampling rule, the search options and the penalties are keys of the model: `resolve` reads them.  DecodePlan() is the
    call without options - the route, the stepper's arguments and the graph-cache signature of the plain decode."""
    beam_size: int = 1
    n_best: int = 1
    attention: bool = False
    prefix: Optional[tuple] = None
    samples: Optional[tuple] = None
    vmask: Optional[tuple] = None
    guide: Optional[tuple] = None
    stats: int = 0

    def options(self):
        """-> {field: value} of the fields that are off their defaults (empty: the plain decode)."""
        return {k: v for k, v in self._asdict().items() if v is not None and v != self._field_defaults[k]}

    def keywords(self):
        """options() under the names of `_generate`'s keywords (`stats` is its `token_stats`)."""
        kw = self.options()
        if 'stats' in kw:
            kw['token_stats'] = kw.pop('stats')
        return kw

    def resolve(self, model, gen_len=DEFAULT_GEN_LEN, eos=2, rows=None):
        """Checks the plan against `model` - what its options do not combine with, the keys of the model included - and reads
        the model's own options once.  rows: the batch's captions, to re-check a prefix handed in as a raw tuple (None: not
        re-checked).  -> (sample, opts, ban, pen): _sampling(), the search options (alpha, n, min_len) or None, the ban list's
        (n, min_len, eos) or None, the penalties (theta, alpha, beta) or None."""
        opts = model._check_options(self.beam_size, self.attention, self.n_best, gen_len)
        model._check_token_stats(self.stats, self.beam_size, self.n_best, self.guide)
        if self.guide is not None:
            model._check_guidance(self.guide[1], self.guide[0], self.attention, self.prefix,
                                  self.samples[0] if self.samples is not None else 1, True if self.vmask is not None else None)
        pen = model._check_penalties(self.attention)
        if self.prefix is not None and rows is not None:
            model._check_prefix(self.prefix[0], rows, gen_len, eos)
        if self.vmask is not None:
            model._check_mask_options(True, None, self.attention)
        if self.attention:
            model._check_attention(self.beam_size)
        ban = (opts[1], opts[2], int(eos)) if opts is not None and (opts[1] or opts[2]) else None
        return model._sampling(), opts, ban, pen


class OptionChecks:
    """What a caption model knows about its generation options (a mix-in of CaptionModel): the model's own keys as the
    generators take them (_sampling, _search_options, _penalties), the checks of every option against COMBINES - each returns
    the checked value, or None / 0 for an option that is off - and `_plan`, which runs them in one fixed order."""
    SEARCH_OPTIONS = True        # the class decodes through the cached generator (False: the options are refused)
    CACHED_N_SAMPLES = False     # a model with a decision launch of its own that still decodes n hypotheses per image

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

    def _search_options(self, gen_len=DEFAULT_GEN_LEN):
        """-> (alpha, n, min_len) of the model's attributes, checked; None when all three are at their defaults."""
        opts = check_beam_options(getattr(self, 'beam_len_penalty', 0.0), getattr(self, 'no_repeat_ngram_size', 0),
                                  getattr(self, 'min_len', 0), gen_len)
        return None if opts == (0.0, 0, 0) else opts

    def _penalties(self):
        """-> (theta, alpha, beta) of the model's attributes, checked; None when all three are at their defaults."""
        pen = check_penalties(getattr(self, 'repetition_penalty', 1.0), getattr(self, 'presence_penalty', 0.0),
                              getattr(self, 'frequency_penalty', 0.0))
        return None if pen == (1.0, 0.0, 0.0) else pen

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

    # ---- the table's two kinds of refusal ---------------------------------------------------------------------------
    def _cached_only(self, what, scope, also=False, models='copy models'):
        """Refuses `what` on a model whose decode step ends in a decision launch of its own - an LSTM decoder, or a class
        without SEARCH_OPTIONS unless `also` holds: `scope` ('the penalties cover', ...) the cached generator only."""
        if not hasattr(getattr(self, 'decoder', None), 'project_contexts') or not (self.SEARCH_OPTIONS or also):
            raise ValueError('%s: %s has a decode step with its own decision launch (LSTM decoders, %s); %s the cached '
                             'DynamicConv generator only' % (what, type(self).__name__, models, scope))

    def _stated(self, name, call):
        """How a refusal spells partner `name` of COMBINES when it is set - a key of the model, or an argument in `call` -
        else None."""
        if name in _TRUNCATIONS + _BANS + ('sampling_topk',):
            v = getattr(self, name, None)
            on = v is not None if name in _TRUNCATIONS else int(v or 0) > (1 if name == 'sampling_topk' else 0)
            return '%s=%r' % (name, v) if on else None
        if name == 'truncation':
            return self._truncation()
        if name == 'sampling':
            on = getattr(self, 'sampling_topp', None) is not None or int(getattr(self, 'sampling_topk', 1)) > 1
            return 'sampling (sampling_topk %r, sampling_topp %r)' % (self.sampling_topk, self.sampling_topp) if on else None
        if name == 'penalties':
            pen = self._penalties()
            return pen and ' / '.join('%s=%r' % (k_, v) for k_, v, d in zip(PENALTY_KEYS, pen, (1.0, 0.0, 0.0)) if v != d)
        if name == 'mask':
            return ' / '.join(self._mask_options(call.get('banned'), call.get('ground'))) or None
        if name == 'attention':
            return 'attention=True' if call.get('attention') else None
        if name == 'prefix':
            return 'prefix' if call.get('prefix') is not None else None
        if name == 'n_samples':
            n = call.get('n_samples', 1)
            return 'n_samples=%d' % n if isinstance(n, int) and n > 1 else None
        if name == 'beam':
            return 'beam search (beam_size %d)' % int(call['beam_size']) if int(call.get('beam_size', 1)) > 1 else None
        raise KeyError(name)

    def _refuse(self, option, what, **call):
        """Raises the first refusal of COMBINES[option] that applies to `what` (the option as set) under the model's keys and
        the arguments in `call`."""
        for partner, reason in COMBINES[option]:
            if partner is None:
                self._cached_only(what, reason)
            elif self._stated(partner, call):
                raise ValueError('%s and %s do not combine: %s' % (what, self._stated(partner, call), reason))

    # ---- one check per option -----------------------------------------------------------------------------------------
    def _check_truncation(self):
        """sampling_minp / sampling_typical: the cached DynamicConv generator only."""
        if self._truncation():
            self._cached_only(self._truncation(), 'min-p and typical sampling cover')

    def _check_beam(self, beam_size):
        if int(beam_size) > 1 and self._truncation():
            raise ValueError('beam search (beam_size %d) and %s do not combine' % (int(beam_size), self._truncation()))
        if int(beam_size) > 1 and getattr(self, 'sampling_topp', None) is not None:
            raise ValueError('beam search (beam_size %d) and nucleus sampling (sampling_topp %r) do not combine'
                             % (int(beam_size), self.sampling_topp))
        if int(beam_size) > 1 and self._sampling() is not None:
            raise ValueError('beam search (beam_size %d) and top-k sampling (sampling_topk %d) do not combine: the reference '
                             'samples without a beam' % (int(beam_size), int(self.sampling_topk)))

    def _check_options(self, beam_size=1, attention=False, n_best=1, gen_len=DEFAULT_GEN_LEN):
        """The search options and n_best: the arg-max / beam decode of the cached DynamicConv generator.
        -> (alpha, n, min_len), or None when nothing is set."""
        if isinstance(n_best, bool) or not isinstance(n_best, int) or not 1 <= n_best <= max(int(beam_size), 1):
            raise ValueError('n_best must be an integer in 1..beam_size (got n_best=%r with beam_size=%d)'
                             % (n_best, int(beam_size)))
        opts = self._search_options(gen_len)
        used = [name for name, v in zip(('beam_len_penalty', 'no_repeat_ngram_size', 'min_len'), opts or ()) if v]
        if n_best > 1:
            used.append('n_best')
        if not used:
            return None
        self._refuse('search', ' / '.join('%s=%r' % (u, n_best if u == 'n_best' else getattr(self, u)) for u in used),
                     attention=attention)
        return opts

    def _check_penalties(self, attention=False):
        """The penalties: the arg-max, beam and top-k sampling decodes of the cached DynamicConv
        generator.  -> (theta, alpha, beta) or None."""
        pen = self._penalties()
        if pen is not None:
            self._refuse('penalties', self._stated('penalties', {}), attention=attention)
        return pen

    def _check_mask_options(self, banned=None, ground=None, attention=False):
        """A vocabulary mask: the arg-max, beam and top-k sampling decodes of the cached DynamicConv
        generator, with or without the search options, n_samples and a prefix.  -> the option names in force (may be empty)."""
        used = self._mask_options(banned, ground)
        if used:
            self._refuse('mask', ' / '.join(used), attention=attention)
        return used

    def _check_guidance(self, guidance=None, guidance_drop=None, attention=False, prefix=None, n_samples=1, banned=None,
                        ground=None):
        """Context guidance of one call: the arguments, or where they are None the model's
        `guidance_scale` / `guidance_drop`, checked (check_guidance; every name a context of this decoder).  -> None for
        gamma = 1.0 (off: the call of before), else (drop, gamma): the arg-max and beam decodes of the cached DynamicConv
        generator with beam_len_penalty and n_best."""
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
        self._refuse('guidance', 'guidance=%r' % gamma, attention=attention, prefix=prefix, n_samples=n_samples, banned=banned,
                     ground=ground)
        return drop, gamma

    def _check_prefix(self, prefix, batch_size, gen_len=DEFAULT_GEN_LEN, eos=2):
        """generate(prefix=...): check_prefix against this model; the cached DynamicConv generators only - the LSTM decoders
        and the copy models end their decode step in a decision launch of their own.  -> (prefix, plen) or None."""
        if prefix is None:
            return None
        self._cached_only('prefix', 'a forced prefix is out of scope there: it covers',
                          models='copy models such as transformer_pointer / transformer_pointer_2')
        return check_prefix(prefix, batch_size, self.decoder.adaptive_softmax.vocab_size, gen_len, self.padding_idx, eos)

    def _check_n_samples(self, n_samples=1, rank_by='score', rank_len_penalty=0.0, beam_size=1, attention=False,
                         forward=False, cached=False):
        """generate(n_samples=n): check_n_samples, and for n > 1 a sampling decode of the cached
        DynamicConv generator, one seed per call, not forward=True - or, with cached=True (the call decodes through the cached
        step), a copy model that samples (CACHED_N_SAMPLES).  -> (n, rule, alpha), or None for n = 1."""
        n, rule, alpha = check_n_samples(n_samples, rank_by, rank_len_penalty)
        if n == 1:
            return None
        self._refuse('n_samples', 'n_samples=%d' % n, beam_size=beam_size, attention=attention)
        if forward:
            raise ValueError('n_samples goes with generate, not with forward=True')
        self._cached_only('n_samples=%d' % n, 'several samples per image cover',
                          also=cached and self.CACHED_N_SAMPLES and self._sampling() is not None)
        if self._sampling() is None:
            raise ValueError('n_samples=%d needs a sampling model (sampling_topk > 1, sampling_topp, sampling_minp or '
                             'sampling_typical): the arg-max decode (sampling_topk 1) would give %d identical captions' % (n, n))
        return n, rule, alpha

    def _check_token_stats(self, token_stats=0, beam_size=1, n_best=1, guide=None):
        """generate(token_stats=n): check_token_stats, and for n > 0 the greedy and sampling decodes of
        the cached DynamicConv generator; TOKEN_STATS_REFUSALS words every refusal.  -> n."""
        n = check_token_stats(token_stats)
        for on, why in ((int(beam_size) > 1 or int(n_best) > 1, 'beam'), (guide is not None, 'guide'),
                        (not hasattr(getattr(self, 'decoder', None), 'project_contexts'), 'lstm')):
            if n and on:
                raise ValueError('token_stats=%d: %s' % (n, TOKEN_STATS_REFUSALS[why]))
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

    def _plan(self, beam_size=1, attention=False, n_best=1, prefix=None, n_samples=1, rank_by='score', rank_len_penalty=0.0,
              banned=None, ground=None, guidance=None, guidance_drop=None, token_stats=0, context=None, batch_size=None):
        """The DecodePlan of generate's arguments, every option checked once, in one fixed order: attention, search options /
        n_best, n_samples, prefix, vocabulary mask, guidance, token_stats.  context: the batch's `context` (the article ids a
        class is grounded in; None - generate_lanes: the mask is checked and built batch by batch); batch_size: its captions,
        for the prefix.  Nothing set: DecodePlan(), and nothing of the batch is read."""
        if attention:
            self._check_attention(beam_size)
        self._check_options(beam_size, attention, n_best)
        ns = self._check_n_samples(n_samples, rank_by, rank_len_penalty, beam_size, attention)
        pfx = None if prefix is None else self._check_prefix(prefix, batch_size)
        vm = None if context is None else self._vocab_mask(context, banned, ground, attention)
        guide = self._check_guidance(guidance, guidance_drop, attention, prefix, n_samples, banned, ground)
        ts = self._check_token_stats(token_stats, beam_size, n_best, guide)
        return DecodePlan(beam_size, n_best, bool(attention), pfx, ns, vm, guide, ts)
