"""CPU checks of the launchers over the adaptive-softmax logits (csrc/adaptive.hip, csrc/guidance.hip; ops.py, decode.py):

1. every refusal of the fourteen tell_adaptive_logprob_* entry points - return code and the text of tell_last_error() -
   and TELL_OK for rows = 0 where an entry point returns early.  Nothing is launched: a refusal returns before the first HIP
   call.  The table below was written from the launchers' source; host code between a signature and its launch may be
   rearranged, what it refuses and with which words may not.
2. the launches of the Python head - ops.adaptive_log_probs and both layouts of decode.head_step - for every pick the
   generators take: which entry points, in which order, with which arguments (tensors as dtype / shape / stride / offset).
   tests/golden/logprob_pick_calls.json holds the recording; TELL_RECORD_PICK_CALLS=1 writes it anew instead of comparing."""
import ctypes
import json
import math
import os

import pytest
import torch

import tell_amd  # noqa: F401
from tell_amd import decode, hip, ops
from tell_amd import runtime as rt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'logprob_pick_calls.json')
TELL_OK, TELL_ERR_ARG = 0, -1

# --------------------------------------------------------------------------- 1. the refusals of the C entry points
_BUF = (ctypes.c_char * 256)()
P = ctypes.addressof(_BUF)                                  # a valid host address; no entry point below gets to read it
INF = float('inf')
# head [rows, 8 + 0]: a vocabulary of 8 tokens and no tail (the sizes of absent tails must not count: n0 = 1000)
LOGITS = dict(head=P, ld_head=8, c0=8, n_tails=0, tail0=None, ld0=0, n0=1000, tail1=None, ld1=0, n1=0, tail2=None, ld2=0, n2=0,
              rows=0)
OUT = dict(tokens=P, lps=P)
DRAW = dict(k=4, inv_temp=1.0, seed_dev=P, row_ids=None, step=0, step_dev=None, **OUT)
PEN = dict(pen_tok=P, pen_cnt=P, ld_pen=4, n_pen=P, theta=1.5, sub=P, n_sub=2)
MASK = dict(mask=P, ld_mask=1, per=1)
BIG = (1 << 18) + 1


def _tails(who):
    return [(dict(n_tails=4), who + ': up to 3 tails'), (dict(n_tails=-1), who + ': up to 3 tails')]


def _k8(who):
    return [(dict(k=0), who + ': 1 <= k <= 8'), (dict(k=9), who + ': 1 <= k <= 8')]


def _draw(who, kmsg=': 1 <= k <= 64'):
    return _tails(who) + [(dict(k=0), who + kmsg), (dict(k=65), who + kmsg), (dict(inv_temp=0.0), who + ': inv_temp > 0'),
                          (dict(seed_dev=None), who + ': seed_dev, tokens and lps are required'),
                          (dict(tokens=None), who + ': seed_dev, tokens and lps are required'),
                          (dict(lps=None), who + ': seed_dev, tokens and lps are required')]


_PEN_REFUSALS = [
    (dict(pen_tok=None), 'logprob penalised: pen_tok / pen_cnt [rows, ld_pen] and n_pen [rows]'),
    (dict(pen_cnt=None), 'logprob penalised: pen_tok / pen_cnt [rows, ld_pen] and n_pen [rows]'),
    (dict(n_pen=None), 'logprob penalised: pen_tok / pen_cnt [rows, ld_pen] and n_pen [rows]'),
    (dict(ld_pen=0), 'logprob penalised: pen_tok / pen_cnt [rows, ld_pen] and n_pen [rows]'),
    (dict(sub=None), 'logprob penalised: sub fp32 [n_sub >= 1]'),
    (dict(n_sub=0), 'logprob penalised: sub fp32 [n_sub >= 1]'),
    (dict(theta=0.5), 'logprob penalised: theta finite and >= 1'),
    (dict(theta=INF), 'logprob penalised: theta finite and >= 1'),
    (dict(c0=0), 'logprob penalised: vocab <= 2^18 (the bitmap: 32 KB of LDS)'),
    (dict(c0=BIG), 'logprob penalised: vocab <= 2^18 (the bitmap: 32 KB of LDS)'),
    (dict(c0=1 << 17, n_tails=1, tail0=P, ld0=BIG, n0=BIG - (1 << 17)), 'logprob penalised: vocab <= 2^18 (the bitmap: 32 KB of LDS)'),
]
_MASK_REFUSALS = [
    (dict(c0=0), 'logprob masked: vocab <= 2^18 (the bitmap: 32 KB of LDS)'),
    (dict(c0=BIG, ld_mask=1 << 14), 'logprob masked: vocab <= 2^18 (the bitmap: 32 KB of LDS)'),
    (dict(mask=None), 'logprob masked: mask uint32 [rows / per, ld_mask >= words]'),
    (dict(ld_mask=0), 'logprob masked: mask uint32 [rows / per, ld_mask >= words]'),
    (dict(c0=33), 'logprob masked: mask uint32 [rows / per, ld_mask >= words]'),      # two words, ld_mask = 1
    (dict(per=0), 'logprob masked: rows must be a multiple of per >= 1'),
    (dict(rows=3, per=2), 'logprob masked: rows must be a multiple of per >= 1'),
]
_FORCED_PAD = ('logprob_forced: pad must be a token of the vocabulary (it is the next step\'s input of a filler hypothesis)')
_STATS_OUT = ('logprob_stats: alt_tok / alt_lp [slots, rows, n] and rank / entropy / chosen_lp [slots, rows]')

# entry point -> (the arguments behind `rows` of a call that is let through, rows = 0 returns TELL_OK?, [(changes, text)])
REFUSALS = {
    'tell_adaptive_logprob_topk': (dict(k=4, **OUT), True, _tails('logprob_topk') + _k8('logprob_topk')),
    'tell_adaptive_logprob_topk_banned': (dict(k=4, ban=P, ld_ban=2, n_ban=P, **OUT), True, _tails('logprob_topk_banned') + _k8(
        'logprob_topk_banned') + [
        (dict(ban=None), 'logprob_topk_banned: ban [rows, ld_ban] and n_ban [rows]'),
        (dict(n_ban=None), 'logprob_topk_banned: ban [rows, ld_ban] and n_ban [rows]'),
        (dict(ld_ban=0), 'logprob_topk_banned: ban [rows, ld_ban] and n_ban [rows]'),
        # (this one stands behind the early return: rows = 1, refused before the launch)
        (dict(rows=1, c0=0), 'logprob_topk_banned: vocab <= 2^18 (the ban bitmap: 32 KB of LDS)'),
        (dict(rows=1, c0=BIG), 'logprob_topk_banned: vocab <= 2^18 (the ban bitmap: 32 KB of LDS)')]),
    'tell_adaptive_logprob_topk_penalised': (dict(k=4, **PEN, **OUT), True, _tails('logprob_topk_penalised') + _k8(
        'logprob_topk_penalised') + [(dict(tokens=None), 'logprob_topk_penalised: tokens and lps [rows, k]'),
                                     (dict(lps=None), 'logprob_topk_penalised: tokens and lps [rows, k]')] + _PEN_REFUSALS),
    'tell_adaptive_logprob_topk_masked': (dict(k=4, **MASK, ban=None, ld_ban=0, n_ban=None, **OUT), True, _tails(
        'logprob_topk_masked') + _k8('logprob_topk_masked') + [
        (dict(tokens=None), 'logprob_topk_masked: tokens and lps [rows, k]'),
        (dict(lps=None), 'logprob_topk_masked: tokens and lps [rows, k]')] + _MASK_REFUSALS + [
        (dict(ban=P, ld_ban=0), 'logprob masked: ban [rows, ld_ban >= 1]')]),
    'tell_adaptive_logprob_topk_guided': (dict(pair_offset=1, k=4, gamma_dev=P, s_rows=None, ld_s=0, **OUT), True, _tails(
        'logprob_topk_guided') + _k8('logprob_topk_guided') + [
        (dict(head=None), 'logprob_topk_guided: head, gamma_dev, tokens and lps [rows + pair_offset, k]'),
        (dict(gamma_dev=None), 'logprob_topk_guided: head, gamma_dev, tokens and lps [rows + pair_offset, k]'),
        (dict(tokens=None), 'logprob_topk_guided: head, gamma_dev, tokens and lps [rows + pair_offset, k]'),
        (dict(lps=None), 'logprob_topk_guided: head, gamma_dev, tokens and lps [rows + pair_offset, k]'),
        (dict(pair_offset=0), 'logprob_topk_guided: pair_offset >= rows (the partners lie behind the conditional rows)'),
        (dict(rows=2), 'logprob_topk_guided: pair_offset >= rows (the partners lie behind the conditional rows)'),
        (dict(c0=0), 'logprob_topk_guided: c0 >= 1 and every tail non-empty'),
        (dict(n_tails=1), 'logprob_topk_guided: c0 >= 1 and every tail non-empty'),
        (dict(n_tails=2, tail0=P, tail1=P, n1=0), 'logprob_topk_guided: c0 >= 1 and every tail non-empty'),
        (dict(n_tails=3, tail0=P, tail1=P, n1=8, tail2=P, n2=0), 'logprob_topk_guided: c0 >= 1 and every tail non-empty'),
        (dict(s_rows=P, ld_s=7), 'logprob_topk_guided: s_rows fp32 [rows, ld_s >= vocab]'),
        (dict(s_rows=P, ld_s=1007, n_tails=1, tail0=P), 'logprob_topk_guided: s_rows fp32 [rows, ld_s >= vocab]')]),
    'tell_adaptive_logprob_argmax': (dict(log_probs=None, ld_lp=0, token=P, token_lp=P), True, _tails('logprob_argmax')),
    'tell_adaptive_logprob_forced': (dict(k=4, prefix=P, ld_prefix=3, P=3, plen=P, n_samples=2, row_ids=None, beams=1, step=0,
                                          step_dev=None, pad=1, **OUT), True, _tails('logprob_forced') + _k8('logprob_forced') + [
        (dict(prefix=None), 'logprob_forced: prefix [n_samples, P] and plen [n_samples]'),
        (dict(plen=None), 'logprob_forced: prefix [n_samples, P] and plen [n_samples]'),
        (dict(P=0), 'logprob_forced: prefix [n_samples, P] and plen [n_samples]'),
        (dict(ld_prefix=2), 'logprob_forced: prefix [n_samples, P] and plen [n_samples]'),
        (dict(n_samples=0), 'logprob_forced: prefix [n_samples, P] and plen [n_samples]'),
        (dict(beams=0), 'logprob_forced: rows / beams exceeds n_samples'),
        (dict(rows=5, beams=2), 'logprob_forced: rows / beams exceeds n_samples'),
        (dict(step=-1), 'logprob_forced: step >= 0'),
        (dict(tokens=None), 'logprob_forced: tokens and lps [rows, k]'),
        (dict(lps=None), 'logprob_forced: tokens and lps [rows, k]'),
        (dict(pad=-1), _FORCED_PAD), (dict(pad=8), _FORCED_PAD)]),
    'tell_adaptive_logprob_stats': (dict(chosen=P, ld_chosen=1, finished=None, n=4, slots=2, step=0, step_dev=None, pad=1,
                                         alt_tok=P, alt_lp=P, rank=P, entropy=P, chosen_lp=P), False, [
        (dict(rows=1, n_tails=4), 'logprob_stats: up to 3 tails'),
        (dict(rows=1, n=0), 'logprob_stats: 1 <= n <= 8 alternatives'), (dict(rows=1, n=9), 'logprob_stats: 1 <= n <= 8 alternatives'),
        (dict(rows=0), 'logprob_stats: rows >= 1'),
        (dict(rows=1, chosen=None), 'logprob_stats: chosen int32 [rows, ld_chosen >= 1]'),
        (dict(rows=1, ld_chosen=0), 'logprob_stats: chosen int32 [rows, ld_chosen >= 1]'),
        (dict(rows=1, slots=0), 'logprob_stats: 0 <= step < slots'), (dict(rows=1, step=2), 'logprob_stats: 0 <= step < slots'),
        (dict(rows=1, step=-1), 'logprob_stats: 0 <= step < slots')] + [
        (dict(rows=1, **{name: None}), _STATS_OUT) for name in ('alt_tok', 'alt_lp', 'rank', 'entropy', 'chosen_lp')]),
    'tell_adaptive_logprob_sample': (dict(DRAW), True, _draw('logprob_sample') + [
        (dict(k=9), 'logprob_sample: k <= vocab < 2^24'), (dict(c0=1 << 24), 'logprob_sample: k <= vocab < 2^24')]),
    'tell_adaptive_logprob_sample_penalised': (dict({k_: v for k_, v in DRAW.items() if k_ not in OUT}, **PEN, **OUT), True, _draw(
        'logprob_sample_penalised') + _PEN_REFUSALS + [(dict(k=9), 'logprob_sample_penalised: k <= vocab')]),
    'tell_adaptive_logprob_sample_masked': (dict({k_: v for k_, v in DRAW.items() if k_ not in OUT}, **MASK, **OUT), True, _draw(
        'logprob_sample_masked') + _MASK_REFUSALS + [(dict(k=9), 'logprob_sample_masked: k <= vocab')]),
    'tell_adaptive_logprob_nucleus': (dict(k=0, inv_temp=1.0, p=0.9, seed_dev=P, row_ids=None, step=0, step_dev=None, **OUT,
                                           nuc_size=None, nuc_key=None), True, _tails('logprob_nucleus') + [
        (dict(k=1), 'logprob_nucleus: k = 0 (no top-k cut) or 2 <= k <= 64'),
        (dict(k=65), 'logprob_nucleus: k = 0 (no top-k cut) or 2 <= k <= 64'),
        (dict(inv_temp=-1.0), 'logprob_nucleus: inv_temp > 0'),
        (dict(p=0.0), 'logprob_nucleus: 0 < p <= 1'), (dict(p=1.5), 'logprob_nucleus: 0 < p <= 1'),
        (dict(seed_dev=None), 'logprob_nucleus: seed_dev, tokens and lps are required'),
        (dict(lps=None), 'logprob_nucleus: seed_dev, tokens and lps are required'),
        (dict(c0=0), 'logprob_nucleus: k <= vocab < 2^19'), (dict(k=9), 'logprob_nucleus: k <= vocab < 2^19'),
        (dict(c0=1 << 19), 'logprob_nucleus: k <= vocab < 2^19')]),
    'tell_adaptive_logprob_minp': (dict(inv_temp=1.0, log_minp=math.log(0.1), seed_dev=P, row_ids=None, step=0, step_dev=None, **OUT,
                                        nuc_size=None), True, _tails('logprob_minp') + [
        (dict(inv_temp=0.0), 'logprob_minp: inv_temp > 0'),
        (dict(log_minp=0.1), 'logprob_minp: log_minp = log(m) with 0 < m <= 1'),
        (dict(seed_dev=None), 'logprob_minp: seed_dev, tokens and lps are required'),
        (dict(tokens=None), 'logprob_minp: seed_dev, tokens and lps are required'),
        (dict(c0=0), 'logprob_minp: 1 <= vocab < 2^19'), (dict(c0=1 << 19), 'logprob_minp: 1 <= vocab < 2^19')]),
    'tell_adaptive_logprob_typical': (dict(inv_temp=1.0, tau=0.9, seed_dev=P, row_ids=None, step=0, step_dev=None, **OUT,
                                           nuc_size=None, nuc_key=None, typ_c=None), True, _tails('logprob_typical') + [
        (dict(inv_temp=0.0), 'logprob_typical: inv_temp > 0'),
        (dict(tau=0.0), 'logprob_typical: 0 < tau <= 1'), (dict(tau=1.5), 'logprob_typical: 0 < tau <= 1'),
        (dict(seed_dev=None), 'logprob_typical: seed_dev, tokens and lps are required'),
        (dict(lps=None), 'logprob_typical: seed_dev, tokens and lps are required'),
        (dict(c0=0), 'logprob_typical: 1 <= vocab < 2^19'), (dict(c0=1 << 19), 'logprob_typical: 1 <= vocab < 2^19')]),
}


def test_the_table_names_every_launcher_over_the_logits():
    declared = {n for n in hip.parse_header() if n.startswith('tell_adaptive_logprob_')}
    assert declared == set(REFUSALS) and len(declared) == 14


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_refusals_keep_their_code_and_text(name):
    if not os.path.exists(hip.LIB_PATH):
        pytest.fail('%s is not built' % hip.LIB_PATH)
    lib = hip.lib()
    fn, argnames = getattr(lib, name), hip.parse_header()[name][2]
    rest, early_ok, refusals = REFUSALS[name]
    good = dict(LOGITS, **rest, stream=None)
    assert set(good) == set(argnames), set(good) ^ set(argnames)
    if early_ok:                                            # (rows = 0: nothing to do, and nothing launched)
        assert fn(*[good[a] for a in argnames]) == TELL_OK
        assert fn(*[dict(good, rows=-1)[a] for a in argnames]) == TELL_OK
    for changes, text in refusals:
        assert set(changes) <= set(good), changes
        args = dict(good, **changes)
        assert fn(*[args[a] for a in argnames]) == TELL_ERR_ARG, (name, changes)
        assert lib.tell_last_error().decode() == text, (name, changes)


# --------------------------------------------------------------------------- 2. the launches of the Python head
N, C0, NT, H = 4, 8, (16, 16), 256                          # cutoffs (8, 24, 40): a head of 8 tokens + 2 clusters, two tails of 16
CUTOFFS = [C0, C0 + NT[0], C0 + NT[0] + NT[1]]
VOCAB = CUTOFFS[-1]


def _norm(a):
    if torch.is_tensor(a):                                  # e.g. 'float32[4, 16]/[44, 1]+28'
        return '%s%s/%s+%d' % (str(a.dtype)[6:], list(a.shape), list(a.stride()), a.storage_offset())
    assert a is None or isinstance(a, (int, float)), type(a)
    return a


def _calls(issued):
    """[(entry point, arguments)] -> {'logits': the thirteen leading arguments (head .. n2), which every launch over the logits
    of one head shares, 'calls': [[entry point, rows and the arguments behind it ...] ...]}; any other launch is kept whole."""
    over = [c for c in issued if c[0].startswith('tell_adaptive_logprob_')]
    logits = over[0][1:14] if over else None
    assert all(c[1:14] == logits for c in over), 'one head, one set of logits'
    return {'logits': logits, 'calls': [[c[0]] + (c[14:] if c in over else c[1:]) for c in issued]}


def _picks():
    """name -> the keyword arguments of one pick (without force / stats), and whether force / stats may join it"""
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)                                  # noqa: E731
    seed, cnt = i32(1), i32(1)
    ban = (i32(N, 3), i32(N))
    pen = (1.2, torch.zeros(4), i32(N, 5), i32(N, 5), i32(N))
    mask = (i32(N, 2), 1)
    mask2 = (i32(N // 2, 3)[:, :2], 2)                      # one mask row per two launch rows, rows longer than the words
    draw = (8, 1.25, seed, None, 3)
    return {
        'argmax': (dict(), True),
        'top4': (dict(topk=4), True),
        'top4_ban': (dict(topk=4, ban=ban), True),
        'top4_pen': (dict(topk=4, pen=pen), True),
        'top4_mask': (dict(topk=4, mask=mask), True),
        'top1_mask_per2': (dict(topk=1, mask=mask2), True),
        'top4_mask_ban': (dict(topk=4, mask=mask, ban=ban), True),
        'top4_guide': (dict(topk=4, guide=(N // 2, torch.ones(1))), False),
        'top8': (dict(topk=8), True),
        'draw': (dict(sample=draw), True),
        'draw_rows_counter': (dict(sample=(8, 1.25, seed, i32(N), cnt)), True),          # row_ids and a device step counter
        'draw_pen': (dict(sample=draw, pen=pen), True),
        'draw_mask': (dict(sample=draw, mask=mask), True),
        'nucleus': (dict(sample=(0, 1.25, seed, None, 3, 0.9)), True),
        'nucleus_top8': (dict(sample=(8, 1.25, seed, None, 3, 0.9)), True),
        'minp': (dict(sample=(0, 1.25, seed, None, 3, 0.1, 'minp')), True),
        'typical': (dict(sample=(0, 1.25, seed, None, 3, 0.9, 'typical')), True),
    }


def _force(step):
    return (torch.zeros(N, 3, dtype=torch.long), torch.zeros(N, dtype=torch.int32), None, 1, step, 1)


def _variants(kw, joins):
    yield 'plain', kw
    if joins:
        cnt = torch.zeros(1, dtype=torch.int32)
        yield 'force', dict(kw, force=_force(3))
        yield 'stats', dict(kw, stats=decode.StatsSink(4, 6, N, 1, 'cpu').at(3))
        yield 'force_stats', dict(kw, force=_force(cnt), stats=decode.StatsSink(8, 6, N, 1, 'cpu').at(cnt))


def _weights(dtype, E):
    g = torch.Generator().manual_seed(0)
    w = lambda r, c: torch.randn(r, c, generator=g).to(dtype)                             # noqa: E731
    tails = []
    for n in NT:
        tails += [w(H, E), w(n, H)]
    return w(C0, E), w(len(NT), E), tails


def _record(monkeypatch):
    """-> {driver/pick/variant: [[entry point, normalised arguments ...], ...]} with every launch replaced by a note of it."""
    issued = []
    note = lambda name, *a: issued.append([name] + [_norm(x) for x in a])                # noqa: E731
    monkeypatch.setattr(ops, 'call', note)
    monkeypatch.setattr(decode, 'call', note)
    monkeypatch.setattr(ops, 'gemm', lambda a, b, out=None, out_dtype=None, **kw: out if out is not None else torch.empty(
        a.shape[0], b.shape[0], dtype=out_dtype or a.dtype))
    monkeypatch.setattr(ops, 'gemm_grouped', lambda problems: None)
    monkeypatch.setattr(decode, '_skinny', lambda *a, **kw: None)
    monkeypatch.setattr(decode, 'ENABLED', True)
    out = {}

    def run(driver, fn):
        for pick, (kw, joins) in _picks().items():
            for variant, kw2 in _variants(kw, joins):
                del issued[:]
                res = fn(**kw2)
                assert len(res) == 3
                out['%s/%s/%s' % (driver, pick, variant)] = _calls(issued)
    ops.clear_weight_cache()
    try:
        monkeypatch.setitem(rt._state, 'dtype', torch.float32)
        emb0, cls, tails = _weights(torch.float32, 32)
        x = torch.zeros(N, 32)
        run('adaptive_log_probs', lambda **kw: ops.adaptive_log_probs(x, CUTOFFS, emb0, cls, tails, **kw))
        del issued[:]
        res = ops.adaptive_log_probs(x, CUTOFFS, emb0, cls, tails, want_full=True)
        assert tuple(res[2].shape) == (N, VOCAB)
        out['adaptive_log_probs/argmax_full/plain'] = _calls(issued)
        monkeypatch.setitem(rt._state, 'dtype', torch.bfloat16)
        emb0, cls, tails = _weights(torch.bfloat16, 1024)
        xb = torch.zeros(N, 1024, dtype=torch.bfloat16)
        for composed in (True, False):
            monkeypatch.setattr(decode, 'HEAD_COMPOSED', composed)
            ops.clear_weight_cache()
            run('head_step_' + ('composed' if composed else 'skinny'),
                lambda **kw: decode.head_step(xb, CUTOFFS, emb0, cls, tails, **kw))
            # ... and ops.adaptive_log_probs hands such rows to head_step with everything it was given
            del issued[:]
            pk = _picks()
            ops.adaptive_log_probs(xb, CUTOFFS, emb0, cls, tails, force=_force(3), stats=decode.StatsSink(4, 6, N, 1, 'cpu').at(3),
                                   **pk['top4_mask_ban'][0])
            ops.adaptive_log_probs(xb, CUTOFFS, emb0, cls, tails, **pk['draw_pen'][0])
            ops.adaptive_log_probs(xb, CUTOFFS, emb0, cls, tails, **pk['top4_guide'][0])
            out['adaptive_log_probs_to_head_step_%s' % ('composed' if composed else 'skinny')] = _calls(issued)
    finally:
        ops.clear_weight_cache()
    return out


def test_the_head_issues_the_recorded_launches(monkeypatch):
    got = json.loads(json.dumps(_record(monkeypatch)))      # (tuples -> lists, as the file holds them)
    if os.environ.get('TELL_RECORD_PICK_CALLS') == '1':
        with open(GOLDEN, 'w') as f:
            json.dump(got, f, indent=None, separators=(',', ':'), sort_keys=True)
            f.write('\n')
    want = json.load(open(GOLDEN))
    assert set(got) == set(want)
    for key in sorted(want):
        assert got[key] == want[key], key
    names = {c[0] for head in want.values() for c in head['calls']}
    assert names >= set(REFUSALS), 'every launcher over the logits is reached: %s' % sorted(set(REFUSALS) - names)


def test_the_head_refuses_what_does_not_combine(monkeypatch):
    monkeypatch.setattr(ops, 'call', lambda name, *a: None)
    monkeypatch.setattr(decode, 'call', lambda name, *a: None)
    monkeypatch.setattr(ops, 'gemm', lambda a, b, out=None, out_dtype=None, **kw: out if out is not None else torch.empty(
        a.shape[0], b.shape[0], dtype=out_dtype or a.dtype))
    monkeypatch.setattr(ops, 'gemm_grouped', lambda problems: None)
    monkeypatch.setattr(decode, '_skinny', lambda *a, **kw: None)
    pk = {k_: v[0] for k_, v in _picks().items()}
    ban, pen, mask = pk['top4_ban']['ban'], pk['top4_pen']['pen'], pk['top4_mask']['mask']
    guide, stats = pk['top4_guide']['guide'], decode.StatsSink(4, 6, N, 1, 'cpu').at(3)
    G, P_, M, B = 'guidance goes with', 'penalties go with', 'a vocabulary mask goes with', 'a ban list goes with'
    draw, nucleus = pk['draw']['sample'], pk['nucleus']['sample']
    both = [(dict(guide=guide), G), (dict(guide=guide, topk=4, ban=ban), G), (dict(guide=guide, topk=4, pen=pen), G),
            (dict(guide=guide, topk=4, mask=mask), G), (dict(guide=guide, topk=4, force=_force(3)), G),
            (dict(guide=guide, topk=4, stats=stats), G), (dict(guide=guide, topk=4, sample=draw), G),
            (dict(pen=pen), P_), (dict(mask=mask), M), (dict(ban=ban), B),
            (dict(topk=4, mask=mask, pen=pen), M), (dict(sample=draw, mask=mask, pen=pen), M), (dict(topk=4, ban=ban, pen=pen), P_),
            (dict(sample=nucleus, pen=pen), P_), (dict(sample=pk['minp']['sample'], pen=pen), P_),
            (dict(sample=nucleus, mask=mask), M), (dict(sample=pk['typical']['sample'], mask=mask), M),
            # (head_step's rule; adaptive_log_probs used to ignore the list where it did not hand the rows to head_step)
            (dict(sample=draw, ban=ban), B)]
    full = [(dict(pen=pen, topk=4), P_), (dict(mask=mask, topk=4), M), (dict(force=_force(3)), 'forced tokens go with'),
            (dict(stats=stats), 'token statistics go with'), (dict(guide=guide, topk=4), G)]
    ops.clear_weight_cache()
    try:
        monkeypatch.setitem(rt._state, 'dtype', torch.float32)
        emb0, cls, tails = _weights(torch.float32, 32)
        x = torch.zeros(N, 32)
        for kw, why in both:
            with pytest.raises(ValueError, match='^adaptive_log_probs: ' + why):
                ops.adaptive_log_probs(x, CUTOFFS, emb0, cls, tails, **kw)
        for kw, why in full:
            with pytest.raises(ValueError, match='^adaptive_log_probs: ' + why):
                ops.adaptive_log_probs(x, CUTOFFS, emb0, cls, tails, want_full=True, **kw)
        # with the full rows a draw is not taken, so what only a draw rules out is let through as it always was
        for kw in (dict(sample=nucleus), dict(sample=draw, topk=4, ban=ban)):
            assert len(ops.adaptive_log_probs(x, CUTOFFS, emb0, cls, tails, want_full=True, **kw)) == 3
        monkeypatch.setitem(rt._state, 'dtype', torch.bfloat16)
        emb0, cls, tails = _weights(torch.bfloat16, 1024)
        xb = torch.zeros(N, 1024, dtype=torch.bfloat16)
        for composed in (True, False):
            monkeypatch.setattr(decode, 'HEAD_COMPOSED', composed)
            for kw, why in both:
                with pytest.raises(ValueError, match='^head_step: ' + why):
                    decode.head_step(xb, CUTOFFS, emb0, cls, tails, **kw)
    finally:
        ops.clear_weight_cache()
