"""float64 reference of tell_adaptive_logprob_stats (csrc/adaptive.hip), the bounds its fp32 outputs are
held to, and the case table that tests/test_token_stats_host.py and tests/test_gpu_token_stats.py both walk.  numpy only.

Reference (per row, all float64): the full log-probs of the adaptive softmax, the top n with ties to the lower id, the rank
of the chosen token  #{t: lp_t > lp_c or (lp_t == lp_c and t < c)}  and the entropy in nats, computed twice - directly,
-sum p log p, and by the chain rule  H_head + sum_i p(cluster i) H_tail_i  - which agree to 1e-12.

Bounds, derived from the kernel's arithmetic with eps = 2^-24 (an fp32 operation is off by eps relative; __expf rounds and
scales its argument, so exp(d) is off by (|d| + 4) eps relative on a given d - the model of tests/copy_ref.py; __logf is
off by 3 eps (|log s| + 1) absolute - v_log_f32 times ln 2, the model of tests/ln_ref.py; a sum of g same-sign terms is off
by g eps relative, g = the depth of the kernel's order: the longest per-thread chain, 6 wave steps, up to 16 waves):

  one cluster of n logits x, m = max x, d = x - m (off by eps |d|), e = exp(d) (off by (2 |d| + 4) eps e):
    s = sum e            ds <= eps (A + g s),          A = sum e (2 |d| + 4)
    u = sum e d          du <= eps (B + g |u|),        B = sum e |d| (2 |d| + 6)
    lse = m + log s      dlse <= ds / s + 3 eps (|log s| + 1) + eps |lse|
    H_c = log s - u / s  dH_c <= (ds / s) (1 + |u| / s) + du / s + eps |u| / s + 3 eps (|log s| + 1) + eps |H_c|
  row: w_i = exp(a_i), a_i = head[c0 + i] - lse_h (off by dlse_h + eps |a_i|), so dw_i <= w_i (dlse_h + (2 |a_i| + 4) eps)
    H = H_head + sum_i w_i H_i    dH <= dH_head + sum_i (w_i dH_i + H_i dw_i + 2 eps w_i H_i) + n_tails eps |H|
  a log-prob: head  lp = x - lse_h:  dlp <= dlse_h + eps |lp|
              tail  lp = x + ((h - lse_h) - lse_i):  dlp <= dlse_h + dlse_i + eps (|h - lse_h| + |off| + |lp|)

bound_entropy(...) is  c * dH  per row with ONE leading constant c; the derived bound must hold at c = 1 (it over-counts:
every error is taken at its worst sign), and C_ENTROPY pins c at the smallest power of two >= 8 x the largest ratio
|H_gpu - H_64| / dH observed on the MI355X over the whole grid of tests/test_gpu_token_stats.py (MEASURED_ENTROPY_RATIO)."""
import functools

import numpy as np

EPS = 2.0 ** -24
THREADS_MIN = 256                 # the streaming form's workgroup: the longest per-thread chains
MEASURED_ENTROPY_RATIO = 0.08835  # MI355X, the 'tie' case (both forms); next: 'unaligned' 0.05607


def pin(ratio):
    """the smallest power of two >= 8 x ratio"""
    return 2.0 ** int(np.ceil(np.log2(8.0 * ratio)))


C_ENTROPY = pin(MEASURED_ENTROPY_RATIO)   # = 1: the pinned bound is the derived one


# name, c0, tails, layout ('aligned': rows start on 16 bytes; 'odd': a leading dimension that breaks that; 'sliced': column
# slices of ONE buffer, head_step's composed layout), content ('randn', 'tie', 'spike', 'uniform'), seed
CASES = (
    dict(name='tiny', c0=5, tails=(3,), layout='aligned', content='randn', seed=11),
    dict(name='unaligned', c0=37, tails=(61, 130, 29), layout='odd', content='randn', seed=12),
    dict(name='head8192', c0=8191, tails=(64,), layout='aligned', content='randn', seed=13),        # head_n = 8192: registers
    dict(name='head8193', c0=8192, tails=(64,), layout='aligned', content='randn', seed=14),        # head_n = 8193: streaming
    dict(name='expt', c0=5000, tails=(15000, 30265), layout='aligned', content='randn', seed=21),   # cutoffs (5000, 20000)
    dict(name='expt_sliced', c0=5000, tails=(15000, 30265), layout='sliced', content='randn', seed=29),
    dict(name='no_tails', c0=300, tails=(), layout='aligned', content='randn', seed=17),
    dict(name='tie', c0=64, tails=(32,), layout='aligned', content='tie', seed=18),
    dict(name='spike', c0=100, tails=(50,), layout='aligned', content='spike', seed=19),
    dict(name='uniform', c0=128, tails=(), layout='aligned', content='uniform', seed=20),
)
# (the seeds of the two expt cases were picked so that EVERY row of every row count passes the gap condition of
#  tests/test_token_stats_host.py; seeds 15 and 16 each had one row whose chosen tail token lay within 2 d_lp of another)
ROWS = (1, 5, 33)
ALTS = (1, 4, 8)
TIE_CONTENT = ('tie', 'uniform')


def vocab(case):
    return case['c0'] + sum(case['tails'])


@functools.lru_cache(maxsize=None)
def logits(name, rows):
    """-> (head fp32 [rows, c0 + n_tails], [tail fp32 [rows, n_i]]) of a case: made once, never written to."""
    case = next(c for c in CASES if c['name'] == name)
    g = np.random.default_rng(case['seed'] * 1000 + rows)
    c0, tails = case['c0'], case['tails']
    hn = c0 + len(tails)
    kind = case['content']
    if kind == 'randn':
        head = (g.standard_normal((rows, hn)) * 3.0).astype(np.float32)
        tl = [(g.standard_normal((rows, n)) * 2.0).astype(np.float32) for n in tails]
    elif kind == 'tie':
        # integer logits inside the head with duplicates: 0..9 over 64 tokens; the tail's cluster logit is far below, so every
        # tail token lies below every head token and the ties are the head's alone
        head = g.integers(0, 10, (rows, hn)).astype(np.float32)
        head[:, c0:] = -40.0
        tl = [g.integers(0, 4, (rows, n)).astype(np.float32) for n in tails]
    elif kind == 'spike':
        head = (g.standard_normal((rows, hn)) * 1.0).astype(np.float32)
        head[np.arange(rows), g.integers(0, c0, rows)] += 60.0
        tl = [(g.standard_normal((rows, n)) * 1.0).astype(np.float32) for n in tails]
    else:                                                   # uniform: H = log V exactly in float64
        head = np.full((rows, hn), 1.5, dtype=np.float32)
        tl = []
    for a in [head] + tl:
        a.setflags(write=False)
    return head, tl


def cluster(x):
    """x float64 [rows, n] -> dict of the cluster's float64 quantities and error terms (module docstring)."""
    n = x.shape[1]
    m = x.max(1, keepdims=True)
    d = x - m
    e = np.exp(d)
    s = e.sum(1)
    u = (e * d).sum(1)
    g = -(-n // THREADS_MIN) + 6 + 16
    A = (e * (2 * np.abs(d) + 4)).sum(1)
    B = (e * np.abs(d) * (2 * np.abs(d) + 6)).sum(1)
    ds = EPS * (A + g * s)
    du = EPS * (B + g * np.abs(u))
    logs = np.log(s)
    lse = m[:, 0] + logs
    H = logs - u / s
    dlse = ds / s + 3 * EPS * (np.abs(logs) + 1) + EPS * np.abs(lse)
    dH = (ds / s) * (1 + np.abs(u) / s) + du / s + EPS * np.abs(u) / s + 3 * EPS * (np.abs(logs) + 1) + EPS * np.abs(H)
    return dict(lse=lse, H=H, dlse=dlse, dH=dH, lsm=x - lse[:, None])


@functools.lru_cache(maxsize=None)
def reference(name, rows):
    """-> dict: lp float64 [rows, V], entropy (chain rule), entropy_direct, d_entropy (the derived bound at c = 1), d_lp [rows]
    (the largest fp32 error bound of a log-prob of the row)."""
    case = next(c for c in CASES if c['name'] == name)
    head, tl = logits(name, rows)
    c0 = case['c0']
    h = cluster(head.astype(np.float64))
    parts = [h['lsm'][:, :c0]]
    H, dH = h['H'].copy(), h['dH'].copy()
    d_lp = h['dlse'] + EPS * np.abs(h['lsm'][:, :c0]).max(1)
    for i, t in enumerate(tl):
        c = cluster(t.astype(np.float64))
        a = h['lsm'][:, c0 + i]                              # log p(cluster i)
        w = np.exp(a)
        dw = w * (h['dlse'] + (2 * np.abs(a) + 4) * EPS)
        H += w * c['H']
        dH += w * c['dH'] + c['H'] * dw + 2 * EPS * w * c['H']
        lp_t = c['lsm'] + a[:, None]
        off = a - c['lse']
        parts.append(lp_t)
        d_lp = np.maximum(d_lp, h['dlse'] + c['dlse'] + EPS * (np.abs(a) + np.abs(off) + np.abs(lp_t).max(1)))
    dH += len(tl) * EPS * np.abs(H)
    lp = np.concatenate(parts, 1)
    p = np.exp(lp)
    direct = -(np.where(p > 0, p * lp, 0.0)).sum(1)
    for a in (lp, H, dH, d_lp, direct):
        a.setflags(write=False)
    return dict(lp=lp, entropy=H, entropy_direct=direct, d_entropy=dH, d_lp=d_lp)


def bound_entropy(name, rows, c=None):
    """the entropy bound of every row: c * dH (module docstring)"""
    return (C_ENTROPY if c is None else c) * reference(name, rows)['d_entropy']


def top_n(lp, n):
    """lp float64 [V] -> (ids [n], values [n]): value descending, lower id first; (0x7fffffff, -inf) past the vocabulary."""
    order = np.lexsort((np.arange(lp.size), -lp))[:n]
    ids = np.full(n, 0x7fffffff, dtype=np.int64)
    val = np.full(n, -np.inf)
    ids[:order.size], val[:order.size] = order, lp[order]
    return ids, val


def rank_of(lp, c):
    if not 0 <= c < lp.size:
        return -1
    return int(((lp > lp[c]) | ((lp == lp[c]) & (np.arange(lp.size) < c))).sum())


def chosen_kinds(case):
    """What the rows of a case choose, cycling: the arg-max, the 3rd best, one token of every tail (its best), one token
    outside the vocabulary.  The tie table: the first, a middle and the last member of the largest tied group, then the rest."""
    kinds = ['argmax', 'third'] + ['tail%d' % i for i in range(len(case['tails']))] + ['outside']
    if case['content'] in TIE_CONTENT:
        kinds = ['tie_first', 'tie_middle', 'tie_last'] + kinds
    return kinds


@functools.lru_cache(maxsize=None)
def chosen(name, rows):
    """-> (tokens int32 [rows], kinds [rows]) on the float64 log-probs of the case."""
    case = next(c for c in CASES if c['name'] == name)
    lp = reference(name, rows)['lp']
    kinds = chosen_kinds(case)
    V, c0 = lp.shape[1], case['c0']
    out, used = [], []
    for r in range(rows):
        kind = kinds[r % len(kinds)]
        order = np.lexsort((np.arange(V), -lp[r]))
        if kind == 'argmax':
            t = order[0]
        elif kind == 'third':
            t = order[min(2, V - 1)]
        elif kind.startswith('tail'):
            i = int(kind[4:])
            lo = c0 + sum(case['tails'][:i])
            t = lo + int(np.argmax(lp[r, lo:lo + case['tails'][i]]))
        elif kind == 'outside':
            t = V + 7 if r % 2 else -3
        else:                                               # the largest group of exactly equal log-probs (float64 and fp32 agree:
            vals, counts = np.unique(lp[r], return_counts=True)   # equal logits of one cluster)
            grp = np.flatnonzero(lp[r] == vals[np.argmax(counts)])
            t = {'tie_first': grp[0], 'tie_middle': grp[len(grp) // 2], 'tie_last': grp[-1]}[kind]
        out.append(int(t))
        used.append(kind)
    return np.asarray(out, dtype=np.int32), tuple(used)


def gap(name, rows):
    """per row: the smallest |lp_t - lp_c| over the tokens t != c whose log-prob differs from lp_c (float64); inf for a chosen
    token outside the vocabulary.  A row whose gap exceeds 2 * d_lp admits one rank only: no fp32 error within the bound can
    reorder c against a token with a different log-prob."""
    lp = reference(name, rows)['lp']
    tok, _ = chosen(name, rows)
    out = np.full(rows, np.inf)
    for r in range(rows):
        c = int(tok[r])
        if 0 <= c < lp.shape[1]:
            d = np.abs(lp[r] - lp[r, c])
            d = d[d > 0]
            out[r] = d.min() if d.size else np.inf
    return out


# --------------------------------------------------------------------------- the small fp32 model of the score_captions tests
# The model of the package's smoke run (vocabulary 600, width 64, cutoffs (100, 300); stand-in encoders), a batch of its own
# captions, and the teacher-forced reference: the layer-by-layer forward with FULL log-probs.  The GPU test holds
# score_captions(token_stats=4) to it at SCORE_RTOL / SCORE_ATOL (section 27's tolerance for two fp32 paths); a rank is held
# to the interval the reference admits at that tolerance, and the host test shows - on the CPU oracle alone - that the interval
# is a single value for at least 90 % of the batch's tokens.
SCORE_KW = dict(vocab_size=600, dim=64, heads=4, ffn=128, cutoff=(100, 300))
SCORE_RTOL, SCORE_ATOL = 1e-4, 5e-4
SCORE_SHARPEN = 6.0
SCORE_BATCH = dict(B=6, article_len=24, caption_len=12, faces_objects=True, vocab=600, cutoffs=(100, 300), seed=41,
                   variable=True)


def score_encoders(nhwc):
    """(resnet, roberta) stand-ins, deterministic; nhwc: the package's layout ([B, 49, 2048]) or the oracle's ([B, 2048, 7, 7])"""
    import torch

    class TinyRoberta(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(3)
            self.register_buffer('tab', torch.randn(3, 64, 1024, generator=g) * 0.5)

        def extract_features(self, ids, return_all_hiddens=False):
            out = self.tab[:, ids % 64]
            if out.is_cuda:
                import tell_amd
                out = out.to(tell_amd.compute_dtype())
            return out if (return_all_hiddens and out.is_cuda) else (list(out) if return_all_hiddens else out[-1])

    class TinyResnet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(4)
            self.register_buffer('proj', torch.randn(2048, 3, generator=g) * 0.3)

        def forward(self, image):
            f = torch.relu(torch.einsum('oc,bchw->bohw', self.proj, torch.nn.functional.avg_pool2d(image, 32)))
            if not nhwc:
                return f
            import tell_amd
            return f.permute(0, 2, 3, 1).reshape(f.shape[0], 49, 2048).to(tell_amd.compute_dtype()).contiguous()
    return TinyResnet(), TinyRoberta()


def score_model():
    """the package's model (on the CPU, fp32, eval; the caller moves it) under a fixed seed"""
    import torch
    from tell_amd.build import build_model
    torch.manual_seed(0)
    model = build_model('faces_objects', *score_encoders(True), n_bert_layers=3, **SCORE_KW).eval()
    # a freshly initialised width-64 model spreads its 600 log-probs over less than one nat: spacing ~1e-3, the size of the
    # tolerance.  The output tables (tied to the input embeddings) are scaled so that the distribution has a shape to rank in.
    with torch.no_grad():
        for p in model.decoder.adaptive_softmax.parameters():
            p.mul_(SCORE_SHARPEN)
    return model


def rank_interval(lp, c, rtol=SCORE_RTOL, atol=SCORE_ATOL):
    """The ranks of token c that log-probs within atol + rtol |lp| of `lp` [V] admit: every token whose log-prob may have
    moved across lp_c by two such errors may or may not count.  -> (lo, hi)."""
    lp = np.asarray(lp, dtype=np.float64)
    tol = atol + rtol * np.abs(lp)
    ids = np.arange(lp.size)
    sure = (lp - tol > lp[c] + tol[c])
    may = (lp + tol >= lp[c] - tol[c]) & (ids != c)
    return int(sure.sum()), int(may.sum())
