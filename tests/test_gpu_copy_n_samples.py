"""Several sampled captions per image for the copy models on the GPU: tell_copy_decide_hyp through the C
ABI, bit for bit against tell_copy_decide over the batch with every image's keys repeated n times - every operand a view in a
buffer of sentinels (tests/guarded.py) - and generate(cached=True, n_samples=n) against the n-times repeated batch.
Run on the MI355X box:  python -m pytest tests/test_gpu_copy_n_samples.py -m gpu -s"""
import numpy as np
import pytest
import torch

import copy_decode_cases as cdc
import copy_hyp_cases as chc
import copy_ref as ref
from guarded import Guard
from test_gpu_copy_decode import (BF16, COPIED_FILL, F32, I8, I32, I64, PROB_FILL, TOK_FILL, U8, Decide, _batch, _gen,  # noqa: F401
                                  _gpu, _launch_by_launch, _model, declined, dev, intact, ptr, tdt, within)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- tell_copy_decide_hyp
class DecideHyp(Decide):
    """the operands of one tell_copy_decide_hyp launch over a hypothesis batch of tests/copy_hyp_cases.py: k, mask, proper and
    ctx one row per image, everything else R = B * n rows tall; the views, strides and fills of Decide"""

    def __init__(self, h, dtype, layout):
        td = tdt(dtype)
        S, B, E = h['k'].shape
        n = h['n']
        R = B * n
        self.x, self.images, self.n, self.B, self.S, self.E, self.H, self.L, self.td = h, B, n, R, S, E, h['H'], h['L'], td
        self.q = Guard((R, E), td, (E + 8, 1), dev(h['q'], td))
        if layout == 'bse':
            self.k = Guard((S, B, E), td, (E, S * E, 1), dev(h['k'], td))
        else:
            self.k = Guard((S, B, E), td, (B * 2 * E, 2 * E, 1), dev(h['k'], td), off=E)
        self.bk = Guard((E,), td, fill=dev(h['bias_k'], td))
        self.mask = None if h['mask'] is None else Guard((B, S), U8, fill=h['mask'])
        self.proper = None if h['proper'] is None else Guard((B, S), I8, fill=h['proper'])
        self.ctx = Guard((B, S), I64, fill=h['ctx'])
        self.ent, self.gen = Guard((R, 2), F32, fill=h['ent']), Guard((R,), I32, fill=h['gen'])
        self.fin = Guard((R,), U8, fill=h['fin'])
        self.scratch = Guard((R, self.H, S), F32)
        self.fresh()

    def args(self, step, step_dev, **kw):
        a = Decide.args(self, step, step_dev, **kw)
        # (..., step, step_dev, B, H, S, D, scratch, tok, dtype) -> (..., step, step_dev, images, per_image, H, S, D, ...)
        return a[:21] + (self.images, kw.get('n', self.n)) + a[22:]


_CASES = chc.cases()


@pytest.mark.parametrize('layout', ['bse', 'half'])
@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('case', [c[0] for c in _CASES])
def test_copy_decide_hyp(case, dtype, layout):
    from tell_amd import hip
    x = dict(cdc.cases())[case](dtype)
    base = cdc.expected(x)                                               # float64, rows of the case itself
    p, L, B = x['p'], x['L'], len(x['fin'])
    for n in chc.N_HYP:
        tag = '%s %s %s n=%d' % (case, dtype, layout, n)
        h = dict(_CASES)[case](dtype, n)
        R = B * n
        # the yardstick: tell_copy_decide on the expanded batch (keys [S, R, E])
        want = Decide(chc.expand(h), dtype, layout)
        hip.call('tell_copy_decide', *want.args(p, None))
        intact(*want.guards())
        d = DecideHyp(h, dtype, layout)
        assert d.args(p, None)[21:23] == (B, n) and len(d.args(p, None)) == len(want.args(p, None)) + 1
        hip.call('tell_copy_decide_hyp', *d.args(p, None))
        intact(*d.guards())
        by_host = d.outputs()
        # bit for bit, prob included; the whole allocations: finished rows, untouched columns and the gaps as well
        for name, a, b_ in zip(('hist', 'copied', 'prob', 'tok'), want.outputs(), by_host):
            assert torch.equal(a, b_), tag + ': ' + name
        fin = torch.from_numpy(h['fin']).bool()
        live = (~fin).nonzero().flatten().tolist()
        assert live and d.tok.t[fin].tolist() == [TOK_FILL] * int(fin.sum()), tag
        assert (d.prob.t[fin] == PROB_FILL).all() and (d.copied.t[fin] == COPIED_FILL).all(), tag
        assert torch.equal(d.hist.t[fin].cpu(), dev(h['hist'], I32)[fin]), tag
        assert (d.prob.t[live, p] != PROB_FILL).all() and (d.copied.t[live, p + 1] <= 1).all(), tag
        if x['k'].shape[0]:                                              # (no scratch at S = 0)
            sc = d.scratch.t.cpu()
            assert (sc[fin] == d.scratch.sentinel).all(), tag + ': a finished row wrote its scratch'
        # hypothesis (b, 0) is case row b: the float64 reference within the pinned bound
        r = base['r']
        for i, b in enumerate(base['rows']):
            if h['fin'][b * n]:
                continue
            within('prob', d.prob.t[b * n, p], np.reshape(r['prob'][i], ()), r['S_prob'][i], 'float32', r['gam'][i],
                   tag + ' row (%d, 0)' % b)
            assert int(d.tok.t[b * n]) == base['tok'][b] and bool(d.copied.t[b * n, p + 1]) == base['copied'][b], tag
            assert d.hist.t[b * n].tolist() == base['hist'][b].tolist(), tag
        # the step from the device counter: the same bytes
        d.fresh()
        counter = Guard((1,), I32, fill=np.array([p - 1]))
        hip.call('tell_copy_decide_hyp', *d.args(12345, counter.t))
        intact(counter, *d.guards())
        for a, b_ in zip(by_host, d.outputs()):
            assert torch.equal(a, b_), tag + ': step_dev'
        # a counter past the history: nothing is written
        d.fresh()
        before = d.outputs()
        counter.t.fill_(L - 1)
        hip.call('tell_copy_decide_hyp', *d.args(0, counter.t))
        intact(counter, *d.guards())
        for a, b_ in zip(before, d.outputs()):
            assert torch.equal(a, b_), tag + ': p >= L'
        assert R == d.B


def test_declined_calls_write_nothing():
    h = dict(_CASES)['step_S20']('float32', 3)
    d = DecideHyp(h, 'float32', 'bse')
    before = d.outputs()
    for kw, step in ((dict(S=513), 0), (dict(D=65), 0), (dict(bk=None), 0), (dict(dt=2), 0), ({}, d.L), ({}, -1), (dict(n=0), 0),
                     (dict(n=17), 0), (dict(n=-3), 0)):
        assert declined('tell_copy_decide_hyp', *d.args(step, None, **kw)) != 0, (kw, step)
    torch.cuda.synchronize()
    assert d.scratch.untouched()
    for a, b_ in zip(before, d.outputs()):
        assert torch.equal(a, b_)
    intact(*d.guards())


def test_ops_copy_decide_per_image_issues_the_new_entry_point():
    from test_gpu_beam_options import _Spy
    from tell_amd import hip, ops
    h = dict(_CASES)['X37']('float32', 5)
    S, B, E = h['k'].shape
    R, L, H, p = B * 5, h['L'], h['H'], h['p']
    c = lambda a, dt: dev(a, dt).cuda()                                                 # noqa: E731
    mk = lambda: dict(hist=c(h['hist'], I32), copied=torch.zeros(R, L + 1, dtype=U8, device='cuda'),         # noqa: E731
                      prob=torch.zeros(R, L, device='cuda'), tok=torch.zeros(R, dtype=I32, device='cuda'))
    kw = dict(q=c(h['q'], F32), k=c(h['k'], F32), bias_k=c(h['bias_k'], F32).view(1, 1, E), mask=c(h['mask'], U8),
              proper=c(h['proper'], I8), ctx_ids=c(h['ctx'], I64), entity_logits=c(h['ent'], F32), gen_tok=c(h['gen'], I32),
              finished=c(h['fin'], U8), step=p, H=H, scratch=torch.zeros(R, H, S, device='cuda'))
    got = mk()
    with _Spy() as spy:
        ops.copy_decide(**kw, **got, per_image=5)
    assert 'tell_copy_decide_hyp' in spy.names and 'tell_copy_decide' not in spy.names
    want = mk()
    hip.call('tell_copy_decide', kw['q'], E, kw['k'].repeat_interleave(5, dim=1).contiguous(), R * E, E, kw['bias_k'].view(E),
             kw['mask'].repeat_interleave(5, 0), kw['proper'].repeat_interleave(5, 0), kw['ctx_ids'].repeat_interleave(5, 0),
             kw['entity_logits'], kw['gen_tok'], kw['finished'], want['hist'], L + 1, want['copied'], L + 1, want['prob'], L, L, p,
             None, R, H, S, E // H, torch.zeros(R, H, S, device='cuda'), want['tok'], hip.dt(F32))
    for k_ in got:
        assert torch.equal(got[k_], want[k_]), k_
    with pytest.raises(ValueError, match='mask'):
        ops.copy_decide(**dict(kw, mask=kw['mask'].repeat_interleave(5, 0)), **mk(), per_image=5)
    with pytest.raises(ValueError, match='per_image'):
        ops.copy_decide(**kw, **mk(), per_image=17)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the generators
N_FP32 = 3
TENSOR_KEYS = ('gen_ids', 'log_probs', 'should_copy', 'copy_probs', 'scores', 'gen_ids_samples', 'log_probs_samples', 'scores_samples',
               'sample_index', 'duplicate', 'should_copy_samples', 'copy_probs_samples')
TEXT_KEYS = ('generations', 'copied_texts', 'generations_samples', 'copied_texts_samples')


def _sampler(dtype, **kw):
    """the small model of tests/test_gpu_copy_decode.py drawing from the nucleus: sampling_topp 0.9, T 0.8"""
    return _model(dtype, sampling_topk=0, sampling_topp=0.9, sampling_temp=0.8, **kw)


def _hyp_entries(model, n):
    return {sig: h for sig, h in model.__dict__.get('_decode_graphs', {}).items() if ('hyp', n) in sig and ('hidden',) in sig}


def _same(a, b):
    return all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in TENSOR_KEYS) and all(a[k] == b[k] for k in TEXT_KEYS)


def _pad(t, w, v):
    return torch.cat([t, t.new_full((t.shape[0], w - t.shape[1]), v)], 1)


def test_n_samples_draws_the_repeated_batch_fp32():
    import tell_amd
    from test_gpu_n_samples import _repeat
    model, batch, n = _sampler(F32), _batch(), N_FP32
    B = batch['image'].shape[0]
    R = B * n
    keep = tell_amd.graphs.ENABLED

    def run(seed, graphed=True, b=None, **kw):
        tell_amd.graphs.ENABLED = graphed
        try:
            torch.manual_seed(seed)
            return _gen(model, batch if b is None else b, cached=True, **kw)
        finally:
            tell_amd.graphs.ENABLED = keep
    # ---- n_samples = 1 is the plain call: the same outputs, the same keys, the same graph signatures
    plain = run(123)
    sigs = set(model.__dict__['_decode_graphs'])
    one = run(123, n_samples=1, rank_by='consensus', rank_len_penalty=0.7)
    assert set(one) == set(plain)
    assert all(torch.equal(one[k], plain[k]) for k in ('gen_ids', 'log_probs', 'should_copy', 'copy_probs'))
    assert set(model.__dict__['_decode_graphs']) == sigs and not any(('hyp', n) in sig for sig in sigs)

    # ---- a seed under which the repeated batch agrees with itself, captured against graphs disabled (one with no
    #      differing row if the list has one)
    def against(rep, draw):
        """-> the rows of the draw that differ from the repeated batch in ids or copy flags; the others within the bounds"""
        L = draw['gen_ids_samples'].shape[2]
        W = max(L, rep['gen_ids'].shape[1])
        pairs = [(draw['gen_ids_samples'].reshape(R, L), rep['gen_ids'], W, 1), (draw['should_copy_samples'].reshape(R, L), rep['should_copy'], W, False),
                 (draw['log_probs_samples'].reshape(R, L - 1), rep['log_probs'], W - 1, 0.0),
                 (draw['copy_probs_samples'].reshape(R, L - 1), rep['copy_probs'], W - 1, 0.0)]
        (ids, r_ids), (sc, r_sc), (lps, r_lps), (cps, r_cps) = [(_pad(a, w, v).cpu(), _pad(b_, w, v).cpu()) for a, b_, w, v in pairs]
        differ = [r for r in range(R) if not (torch.equal(ids[r], r_ids[r]) and torch.equal(sc[r], r_sc[r]))]
        same = [r for r in range(R) if r not in differ]
        torch.testing.assert_close(lps[same], r_lps[same], rtol=1e-4, atol=5e-4)
        torch.testing.assert_close(cps[same], r_cps[same], rtol=1e-4, atol=5e-4)
        return differ
    chosen = None
    for seed in (123, 124, 125, 126, 127):
        a, b_ = run(seed, b=_repeat(batch, n)), run(seed, graphed=False, b=_repeat(batch, n))
        if not (a['gen_ids'].shape == b_['gen_ids'].shape and torch.equal(a['gen_ids'], b_['gen_ids'])
                and torch.equal(a['should_copy'], b_['should_copy'])):
            continue
        draw = run(seed, n_samples=n, rank_by='draw')
        differ = against(a, draw)
        print('\nseed %d: rows that differ from the repeated batch: %s of %d' % (seed, differ, R))
        if chosen is None or not differ:
            chosen = (seed, a, draw, differ)
        if not differ:
            break
    assert chosen is not None, 'no seed in 123..127 under which the repeated batch agrees captured / graphs disabled'
    seed, rep, draw, differ = chosen
    assert len(differ) <= 1, differ                                     # (a draw on a bucket boundary)
    # ---- the form
    assert set(draw) == set(plain) | set(TENSOR_KEYS) | set(TEXT_KEYS)
    L = draw['gen_ids_samples'].shape[2]
    assert draw['gen_ids_samples'].shape == (B, n, L) and draw['log_probs_samples'].shape == (B, n, L - 1)
    assert draw['should_copy_samples'].shape == (B, n, L) and draw['should_copy_samples'].dtype == torch.bool
    assert draw['copy_probs_samples'].shape == (B, n, L - 1) and draw['copy_probs_samples'].dtype == torch.float32
    assert draw['scores_samples'].shape == (B, n) and draw['duplicate'].shape == (B, n) and draw['duplicate'].dtype == torch.bool
    assert draw['sample_index'].dtype == torch.long and draw['sample_index'].tolist() == [list(range(n))] * B
    assert [len(x) for x in draw['generations_samples']] == [n] * B == [len(x) for x in draw['copied_texts_samples']]
    ids = draw['gen_ids_samples'].reshape(R, L).cpu()
    assert any(len({tuple(ids[b * n + j].tolist()) for j in range(n)}) > 1 for b in range(B))   # not n copies of one caption
    assert bool(draw['should_copy_samples'][:, :, 0].all()) and int(draw['should_copy_samples'][:, :, 1:].sum()) > 0
    # ---- the flows agree; a seed is a seed
    assert _same(run(seed, n_samples=n, rank_by='draw'), draw)
    assert _same(run(seed, graphed=False, n_samples=n, rank_by='draw'), draw), 'graphs disabled'
    other = run(seed + 100, n_samples=n, rank_by='draw')
    assert other['gen_ids_samples'].shape != draw['gen_ids_samples'].shape or \
        not torch.equal(other['gen_ids_samples'], draw['gen_ids_samples'])
    hs = _hyp_entries(model, n)
    assert len(hs) == 1 and all(h['graph'] not in (None, False) for h in hs.values()), [h.get('error') for h in hs.values()]
    # ---- rank order: a permutation of the draws applied to every `_samples` key alike, duplicates last
    for rule, alpha in (('score', 0.0), ('score', 0.7), ('consensus', 0.0)):
        out = run(seed, n_samples=n, rank_by=rule, rank_len_penalty=alpha)
        idx = out['sample_index']
        assert idx.sort(1).values.tolist() == [list(range(n))] * B
        pick = lambda t: t.gather(1, idx.view(B, n, *[1] * (t.dim() - 2)).expand(-1, -1, *t.shape[2:]))   # noqa: E731
        for k_ in ('gen_ids_samples', 'log_probs_samples', 'should_copy_samples', 'copy_probs_samples', 'duplicate'):
            assert torch.equal(out[k_], pick(draw[k_])), (rule, alpha, k_)
        for k_ in ('generations_samples', 'copied_texts_samples'):
            assert out[k_] == [[draw[k_][b][j] for j in idx[b].tolist()] for b in range(B)], (rule, alpha, k_)
        for first, many in (('gen_ids', 'gen_ids_samples'), ('log_probs', 'log_probs_samples'), ('should_copy', 'should_copy_samples'),
                            ('copy_probs', 'copy_probs_samples'), ('scores', 'scores_samples')):
            assert torch.equal(out[first], out[many][:, 0]), (rule, alpha, first)
        assert out['generations'] == [x[0] for x in out['generations_samples']]
        assert out['copied_texts'] == [x[0] for x in out['copied_texts_samples']]
        dup, sc = out['duplicate'].cpu(), out['scores_samples'].cpu()
        for b in range(B):
            k = int((~dup[b]).sum())
            assert not dup[b, :k].any() and dup[b, k:].all()                           # duplicates behind the others
            if rule == 'score':
                assert (sc[b, 1:k] <= sc[b, :k - 1]).all(), sc[b]
        if alpha == 0.0:
            assert torch.equal(out['scores_samples'], pick(draw['scores_samples']))
    assert torch.equal(draw['gen_ids'], draw['gen_ids_samples'][:, 0])


def test_n_samples_bf16_captured_against_launch_by_launch():
    from test_gpu_beam_options import _Spy
    model, batch, other, n = _sampler(BF16), _batch(), _batch(S=40), 4

    def gen(b, **kw):
        torch.manual_seed(11)
        return _gen(model, b, cached=True, n_samples=n, rank_by='draw', **kw)
    # ---- the same launches issued one by one over the same static buffers
    from tell_amd.models import stepper as stepper_mod
    from test_gpu_copy_decode import _NoCapture
    keep = stepper_mod.graphs
    model.reset_graphs()
    try:
        stepper_mod.graphs = _NoCapture()
        with _Spy() as spy_flat:
            flat = gen(batch)
        hs = _hyp_entries(model, n)
        assert hs and all(h['graph'] is False for h in hs.values())
    finally:
        stepper_mod.graphs = keep
        model.reset_graphs()
    assert 'tell_copy_decide_hyp' in spy_flat.names and 'tell_entity_attn_step' in spy_flat.names
    assert 'tell_copy_decide' not in spy_flat.names and 'tell_copy_step' not in spy_flat.names
    captured = gen(batch)
    hs = _hyp_entries(model, n)
    assert len(hs) == 1 and all(h['graph'] not in (None, False) for h in hs.values()), [h.get('error') for h in hs.values()]
    assert _same(captured, flat)
    # ---- a batch of another article length: its own signature; then the first again, replayed without a new capture
    first = next(iter(hs.values()))
    graph_before = first['graph']
    second = gen(other)
    assert len(_hyp_entries(model, n)) == 2 and second['gen_ids_samples'].shape[:2] == (4, n)
    with _Spy() as spy_replay:
        again = gen(batch)
    assert next(iter(_hyp_entries(model, n).values()))['graph'] is graph_before
    assert _same(again, captured)
    assert first.get('graph_has_post'), 'the tail is not part of the captured step'
    for name in ('tell_copy_decide_hyp', 'tell_copy_decide', 'tell_entity_attn_step', 'tell_greedy_update', 'tell_copy_step'):
        assert name not in spy_replay.names, name
    # ---- the copy invariants on every hypothesis: a copied id lies at a proper position of its own image's article,
    #      no id is copied twice in a row's history
    ids, sc = captured['gen_ids_samples'], captured['should_copy_samples']
    assert ids.shape == sc.shape and bool(sc[:, :, 0].all()) and ids.shape[2] >= 2
    assert int(sc[:, :, 1:].sum()) > 0, 'no hypothesis copies'
    ctx, proper = batch['context']['roberta'], batch['context']['roberta_proper_masks']
    for b in range(ids.shape[0]):
        allowed = set(ctx[b][proper[b] >= 1].tolist())
        for j in range(n):
            row = ids[b, j, 1:][sc[b, j, 1:]].tolist()
            assert len(row) == len(set(row)) and set(row) <= allowed, (b, j, row)
    assert any(len({tuple(ids[b, j].tolist()) for j in range(n)}) > 1 for b in range(ids.shape[0]))


def test_n_samples_bf16_multi_step_replays_against_launch_by_launch():
    """no </s> in the articles: the rows decode past the first all-finished test, from where eight steps go as one replay"""
    from tell_amd.models import stepper as stepper_mod
    from test_gpu_copy_decode import _NoCapture
    model, batch, n = _sampler(BF16, bias=False), _batch(eos=False), 2

    def gen():
        torch.manual_seed(7)
        return _gen(model, batch, cached=True, n_samples=n, rank_by='draw')
    keep = stepper_mod.graphs
    model.reset_graphs()
    try:
        stepper_mod.graphs = _NoCapture()
        flat = gen()
    finally:
        stepper_mod.graphs = keep
        model.reset_graphs()
    captured = gen()
    steps = captured['gen_ids_samples'].shape[2] - 1
    print('\nbf16 B=4 n=%d, no planted </s>: %d steps' % (n, steps))
    h, = _hyp_entries(model, n).values()
    assert h['graph'] not in (None, False), h.get('error')
    if steps > 16:
        assert h.get(('multi', 8)) not in (None, False), h.get('multi_error')
    assert _same(captured, flat)


def test_n_samples_1_records_no_new_signature_and_issues_the_entry_point_of_before():
    from test_gpu_beam_options import _Spy
    model, batch = _sampler(BF16), _batch()
    torch.manual_seed(3)
    plain = _gen(model, batch, cached=True)
    sigs = set(model.__dict__['_decode_graphs'])
    torch.manual_seed(3)
    one = _gen(model, batch, cached=True, n_samples=1)
    assert set(one) == set(plain) and set(model.__dict__['_decode_graphs']) == sigs
    assert all(torch.equal(one[k], plain[k]) for k in ('gen_ids', 'log_probs', 'should_copy', 'copy_probs'))
    _, spy = _launch_by_launch(model, batch)
    assert 'tell_copy_decide' in spy.names and 'tell_copy_decide_hyp' not in spy.names
