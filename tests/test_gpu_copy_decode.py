"""The copy models' cached generation on the GPU: the two kernels of csrc/copy_decode.hip through the C
ABI against the float64 reference and the pinned bounds of tests/copy_ref.py - every operand a view in a buffer of sentinels
(tests/guarded.py) - and generate(cached=True) against the eager generator of the pointer models.
Run on the MI355X box:  python -m pytest tests/test_gpu_copy_decode.py -m gpu -s"""
import numpy as np
import pytest
import torch

import copy_decode_cases as cdc
import copy_ref as ref
from guarded import SENTINEL, Guard

pytestmark = pytest.mark.gpu

F32, BF16, I64, I32, U8, I8 = torch.float32, torch.bfloat16, torch.int64, torch.int32, torch.uint8, torch.int8
COPIED_FILL, PROB_FILL, TOK_FILL = 7, 0.25, -3


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    prev = tell_amd.compute_dtype()
    yield
    tell_amd.set_compute_dtype(prev)
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                  # a device fault: every later launch of this process would fail the same way
        pytest.exit('GPU error, nothing more is launched: %s' % err, 3)


def tdt(dtype):
    return getattr(torch, dtype)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def intact(*guards):
    torch.cuda.synchronize()
    for i, g in enumerate(guards):
        assert g is None or g.intact(), 'store outside view %d of the launch' % i


def ptr(g):
    return None if g is None else g.t


def within(out, got, want, S, stored, gam, tag):
    """element-wise bound of copy_ref with the pinned constant of `out`; the figure is printed before it is judged"""
    got = ref.np64(got).reshape(np.shape(want))
    want = np.asarray(want, np.float64)
    S = np.broadcast_to(np.asarray(S, np.float64), want.shape)
    r = ref.ratio(got, want, S, stored, gam)
    print('ratio %-6s %-44s %.6f   c = %s' % (out, tag, r, ref.C[out]))
    assert np.isfinite(got).all(), (out, tag)
    err, b = np.abs(got - want), ref.bound(out, want, S, stored, gam)
    assert (err <= b).all(), '%s %s: worst error %.3g at bound %.3g (ratio %.3f, c = %g)' % (
        out, tag, err.max(), b.reshape(-1)[err.argmax()], r, ref.C[out])


def declined(name, *args):
    from tell_amd import hip
    try:
        return hip.call_rc(name, *args)
    except RuntimeError as err:
        assert name in str(err)
        return -1


# ---------------------------------------------------------------- tell_copy_decide
class Decide:
    """the operands of one tell_copy_decide launch, every one a guarded view; k stored [B,S,E] ('bse') or as the second
    half of a fused [S,B,2E] projection ('half')"""

    def __init__(self, x, dtype, layout):
        td = tdt(dtype)
        S, B, E = x['k'].shape
        self.x, self.B, self.S, self.E, self.H, self.L, self.td = x, B, S, E, x['H'], x['L'], td
        self.q = Guard((B, E), td, (E + 8, 1), dev(x['q'], td))
        if layout == 'bse':
            self.k = Guard((S, B, E), td, (E, S * E, 1), dev(x['k'], td))
        else:
            self.k = Guard((S, B, E), td, (B * 2 * E, 2 * E, 1), dev(x['k'], td), off=E)
        self.bk = Guard((E,), td, fill=dev(x['bias_k'], td))
        self.mask = None if x['mask'] is None else Guard((B, S), U8, fill=x['mask'])
        self.proper = None if x['proper'] is None else Guard((B, S), I8, fill=x['proper'])
        self.ctx = Guard((B, S), I64, fill=x['ctx'])
        self.ent, self.gen = Guard((B, 2), F32, fill=x['ent']), Guard((B,), I32, fill=x['gen'])
        self.fin = Guard((B,), U8, fill=x['fin'])
        self.scratch = Guard((B, self.H, S), F32)
        self.fresh()

    def fresh(self):
        B, L = self.B, self.L
        self.hist = Guard((B, L + 1), I32, (L + 3, 1), fill=self.x['hist'])
        self.copied = Guard((B, L + 1), U8, (L + 5, 1), fill=np.full((B, L + 1), COPIED_FILL))
        self.prob = Guard((B, L), F32, (L + 2, 1), fill=np.full((B, L), PROB_FILL))
        self.tok = Guard((B,), I32, fill=np.full(B, TOK_FILL))

    def args(self, step, step_dev, **kw):
        from tell_amd import hip
        g = lambda name: kw.get(name, getattr(self, name))                 # noqa: E731
        return (self.q.t, self.E + 8, self.k.t, self.k.strides[0], self.k.strides[1], ptr(g('bk')), ptr(self.mask), ptr(self.proper),
                self.ctx.t, self.ent.t, self.gen.t, self.fin.t, self.hist.t, self.L + 3, self.copied.t, self.L + 5, self.prob.t,
                self.L + 2, self.L, step, step_dev, self.B, self.H, kw.get('S', self.S), kw.get('D', self.E // self.H),
                self.scratch.t, self.tok.t, kw.get('dt', hip.dt(self.td)))

    def guards(self):
        return (self.q, self.k, self.bk, self.mask, self.proper, self.ctx, self.ent, self.gen, self.fin, self.scratch, self.hist,
                self.copied, self.prob, self.tok)

    def outputs(self):
        return [g.buf.clone() for g in (self.hist, self.copied, self.prob, self.tok)]


_CASES = cdc.cases()


@pytest.mark.parametrize('layout', ['bse', 'half'])
@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('case', [c[1] for c in _CASES], ids=[c[0] for c in _CASES])
def test_copy_decide(case, dtype, layout, request):
    from tell_amd import hip
    tag = '%s %s %s' % (request.node.callspec.id, dtype, layout)
    x = case(dtype)
    e = cdc.expected(x)
    r, p, B, L = e['r'], x['p'], len(x['fin']), x['L']
    d = Decide(x, dtype, layout)
    hip.call('tell_copy_decide', *d.args(p, None))
    intact(*d.guards())
    by_host = d.outputs()
    # prob first (its figure is printed), then the discrete outputs
    for i, b in enumerate(e['rows']):
        within('prob', d.prob.t[b, p], np.reshape(r['prob'][i], ()), r['S_prob'][i], 'float32', r['gam'][i], tag + ' row %d' % b)
    want_tok = [TOK_FILL if t is None else t for t in e['tok']]
    assert d.tok.t.tolist() == want_tok, tag
    assert d.hist.t.cpu().numpy().tolist() == e['hist'].tolist(), tag + ': hist (only column p + 1 of the unfinished rows)'
    want_cp = np.full((B, L + 1), COPIED_FILL)
    for b in e['rows']:
        want_cp[b, p + 1] = int(e['copied'][b])
    assert d.copied.t.cpu().numpy().tolist() == want_cp.tolist(), tag
    got_prob = d.prob.t.cpu().numpy()
    keep = np.ones((B, L), bool)
    keep[e['rows'], p] = False
    assert (got_prob[keep] == np.float32(PROB_FILL)).all(), tag + ': prob outside column p of the unfinished rows'
    if x['k'].shape[0] == 0:
        assert all(float(got_prob[b, p]) == float(np.float32(1e-6)) for b in e['rows'])
        assert [want_tok[b] for b in e['rows']] == [int(x['gen'][b]) for b in e['rows']]
    # the step from the device counter: the same bytes
    d.fresh()
    counter = Guard((1,), I32, fill=np.array([p - 1]))
    hip.call('tell_copy_decide', *d.args(12345, counter.t))
    intact(counter, *d.guards())
    for a, b_ in zip(by_host, d.outputs()):
        assert torch.equal(a, b_), tag + ': step_dev'
    # a counter past the history: nothing is written
    d.fresh()
    before = d.outputs()
    counter.t.fill_(L - 1)
    hip.call('tell_copy_decide', *d.args(0, counter.t))
    intact(counter, *d.guards())
    for a, b_ in zip(before, d.outputs()):
        assert torch.equal(a, b_), tag + ': p >= L'


# ---------------------------------------------------------------- tell_entity_attn_step
@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('p', [0, 1, 5, 7])
def test_entity_attn_step(p, dtype):
    from tell_amd import hip
    L, B, H = 8, 2, 2
    E, td = H * 64, tdt(dtype)
    tag = 'entity_attn_step p=%d %s' % (p, dtype)
    g = ref._gen(600 + p)
    q, kn, vn = (ref._round(ref._randn(g, B, E) * 0.5, dtype) for _ in range(3))
    kh, vh = (ref._round(ref._randn(g, L, B, E) * 0.5, dtype) for _ in range(2))
    # rows from p on: zero keys (logit 0, a weight that counts) with sentinel values - a read of them would show in out
    kh[p:], vh[p:] = 0.0, SENTINEL
    f = ref.causal(q[None], kh[:p], vh[:p], ref.C_SCALE, p, p, H)
    mk = lambda: (Guard((B, E), td, (E + 8, 1), dev(q, td)), Guard((B, E), td, (E + 16, 1), dev(kn, td)),        # noqa: E731
                  Guard((B, E), td, (E + 24, 1), dev(vn, td)), Guard((L, B, E), td, (B * (E + 8), E + 8, 1), dev(kh, td)),
                  Guard((L, B, E), td, (B * (E + 8), E + 8, 1), dev(vh, td)), Guard((B, E), td, (E + 32, 1)))
    outs = []
    for form in ('host', 'device'):
        gq, gkn, gvn, gkh, gvh, gout = mk()
        counter = Guard((1,), I32, fill=np.array([p - 1]))
        step, step_dev = (p, None) if form == 'host' else (4321, counter.t)
        hip.call('tell_entity_attn_step', gq.t, E + 8, gkn.t, E + 16, gvn.t, E + 24, gkh.t, gvh.t, B * (E + 8), E + 8, gout.t,
                 E + 32, B, H, 64, L, ref.C_SCALE, step, step_dev, hip.dt(td))
        intact(gq, gkn, gvn, gkh, gvh, gout, counter)
        want_k, want_v = dev(kh, td), dev(vh, td)
        want_k[p], want_v[p] = dev(kn, td), dev(vn, td)
        assert torch.equal(gkh.t.cpu(), want_k) and torch.equal(gvh.t.cpu(), want_v), tag + ': row p appended, no other row touched'
        outs.append(gout.buf.clone())
    assert torch.equal(outs[0], outs[1]), tag + ': step_dev'
    if p == 0:
        assert not bool(gout.t.any()), tag
    within('c_out', gout.t, f['out'][0], f['S_out'][0], dtype, ref.causal_gamma('c_out', f, f['n'], 1), tag)


def test_entity_attn_step_is_the_causal_step_kernel_bit_for_bit():
    """the definition: tell_causal_attn_fwd(Tq = 1, pos0 = p, S = p) over the same history"""
    from tell_amd import hip
    L, B, H, p = 8, 2, 2, 5
    E = H * 64
    for td in (F32, BF16):
        g = ref._gen(31)
        q, kn, vn = (ref._randn(g, B, E).to(td).cuda() for _ in range(3))
        kh, vh = (ref._randn(g, L, B, E).to(td).cuda() for _ in range(2))
        want, lse = torch.empty(1, B, E, dtype=td, device='cuda'), torch.empty(B, H, 1, dtype=F32, device='cuda')
        hip.call('tell_causal_attn_fwd', q, kh, vh, want, lse, B, H, 1, p, 64, p, B * E, E, B * E, E, B * E, E, B * E, E,
                 ref.C_SCALE, hip.dt(td))
        got = torch.empty(B, E, dtype=td, device='cuda')
        hip.call('tell_entity_attn_step', q, E, kn, E, vn, E, kh, vh, B * E, E, got, E, B, H, 64, L, ref.C_SCALE, p, None, hip.dt(td))
        assert torch.equal(got, want[0])


# ---------------------------------------------------------------- declined calls
def test_declined_calls_write_nothing():
    from tell_amd import hip
    case = dict(cdc.cases())['step_S20']
    d = Decide(case('float32'), 'float32', 'bse')
    before = d.outputs()
    for kw, step in ((dict(S=513), 0), (dict(D=65), 0), (dict(bk=None), 0), (dict(dt=2), 0), ({}, d.L), ({}, -1)):
        assert declined('tell_copy_decide', *d.args(step, None, **kw)) != 0, (kw, step)
    L, B, H = 8, 2, 2
    E = H * 64
    bufs = [Guard((L * B * E,), F32) for _ in range(6)]
    a = [g.t for g in bufs]
    attn = lambda D=64, step=0, dt=0: declined('tell_entity_attn_step', a[0], E, a[1], E, a[2], E, a[3], a[4], B * E, E, a[5], E,    # noqa: E731
                                               B, H, D, L, 0.125, step, None, dt)
    assert attn(D=32) != 0 and attn(step=L) != 0 and attn(step=-1) != 0 and attn(dt=2) != 0
    torch.cuda.synchronize()
    assert all(g.untouched() for g in bufs) and d.scratch.untouched()
    for x, y in zip(before, d.outputs()):
        assert torch.equal(x, y)
    intact(*d.guards())


def test_ops_wrappers_check_shapes():
    from tell_amd import ops
    B, S, H, E, L = 2, 6, 2, 128, 3
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device='cuda')                     # noqa: E731
    kw = dict(q=z(B, E), k=z(S, B, E), bias_k=z(1, 1, E), mask=z(B, S, dt=U8), proper=z(B, S, dt=I8), ctx_ids=z(B, S, dt=I64),
              entity_logits=z(B, 2), gen_tok=z(B, dt=I32), finished=z(B, dt=U8), hist=z(B, L + 1, dt=I32), copied=z(B, L + 1, dt=U8),
              prob=z(B, L), step=0, H=H, scratch=z(B, H, S), tok=z(B, dt=I32))
    ops.copy_decide(**kw)
    for name, bad in (('proper', z(B, S - 1, dt=I8)), ('mask', z(B, S + 1, dt=U8)), ('ctx_ids', z(B, S - 2, dt=I64)),
                      ('hist', z(B, L, dt=I32)), ('scratch', z(B, H, S + 1)), ('gen_tok', z(B, dt=I64))):
        with pytest.raises(ValueError, match=name):
            ops.copy_decide(**dict(kw, **{name: bad}))
    with pytest.raises(ValueError, match='k_hist'):
        ops.entity_attn_step(z(B, E), z(B, E), z(B, E), z(L, B + 1, E), z(L, B, E), H, 0.125, 0)
    with pytest.raises(RuntimeError, match='tell_entity_attn_step'):
        ops.entity_attn_step(z(B, E), z(B, E), z(B, E), z(L, B, E), z(L, B, E), H, 0.125, L)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the generators
def _batch(S=24, eos=True):
    """the tiny batch of tests/test_gpu_pointer.py at B = 4.  eos: the only proper positions of row b are those of b decoy ids
    - six, five and four positions - and three of </s> (id 2).  The copy attention of an untrained model is close to uniform
    over the article, so an id's probability is close to its number of positions over S + 2 and the most probable id - the only
    one a step can copy - leads the runner-up by about one position's weight (1 / 26 of the total), far above what bf16
    rounding of the decoder's output moves.  A model that copies whenever it can copies </s> in row 0, which ends at step 1,
    and the first decoy in rows 1 - 3, once (it stays the most probable id and is in the history from then on); those rows
    decode on with the generator's tokens."""
    from test_gpu_pointer import _pointer_batch
    batch = _pointer_batch(B=4, S=S)
    if eos:
        ids, proper = batch['context']['roberta'], batch['context']['roberta_proper_masks']
        proper[:] = 0
        for b in range(4):
            at = 0
            for tok, n in [(300 + j, 6 - j) for j in range(b)] + [(2, 3)]:
                ids[b, at:at + n], proper[b, at:at + n] = tok, 1
                at += n
    return batch


def _model(dtype, bias=True, **kw):
    import tell_amd
    from test_gpu_pointer import _Resnet, _Roberta
    from tell_amd.build import build_model
    tell_amd.set_compute_dtype(dtype)
    torch.manual_seed(0)
    model = build_model('pointer', _Resnet(), _Roberta(), n_bert_layers=3, vocab_size=600, dim=1024, heads=16, ffn=256,
                        kernels=(3,), cutoff=(100, 300), **kw).cuda().eval()
    if bias:
        with torch.no_grad():
            model.entity_fc.bias.data = torch.tensor([-5., 5.], device='cuda')          # copy whenever something is copyable
    return model


def _gen(model, batch, **kw):
    with torch.no_grad():
        out = model.generate({k: v.clone() for k, v in batch['context'].items()}, batch['image'],
                             {k: v.clone() for k, v in batch['caption'].items()}, batch['face_embeds'], **kw)
    torch.cuda.synchronize()
    return out


def _ends(out, eos=2):
    ids = out['gen_ids']
    return [int((row == eos).nonzero()[0]) if bool((row == eos).any()) else ids.shape[1] for row in ids]


def _non_vacuous(eager):
    sc = eager['should_copy'][:, 1:]
    assert int((sc.sum(1) > 0).sum()) >= 3, 'fewer than three rows copy on the eager path: %s' % sc.sum(1).tolist()
    assert len(set(_ends(eager))) > 1, 'every row ends at the same step on the eager path: %s' % _ends(eager)


def _same_form(cached, eager):
    for k in ('gen_ids', 'log_probs', 'should_copy', 'copy_probs'):
        assert cached[k].shape == eager[k].shape and cached[k].dtype == eager[k].dtype, k


@pytest.mark.parametrize('bias', [True, False], ids=['bias_-5_5', 'bias_as_built'])
def test_cached_generation_matches_the_eager_generator_fp32(bias):
    model, batch = _model(F32, bias), _batch()
    eager = _gen(model, batch)
    if bias:
        _non_vacuous(eager)
    cached = _gen(model, batch, cached=True)
    _same_form(cached, eager)
    assert torch.equal(cached['gen_ids'], eager['gen_ids'])
    assert torch.equal(cached['should_copy'], eager['should_copy'])
    torch.testing.assert_close(cached['log_probs'], eager['log_probs'], rtol=1e-4, atol=5e-4)
    torch.testing.assert_close(cached['copy_probs'], eager['copy_probs'], rtol=1e-4, atol=5e-4)
    assert cached['copied_texts'] == eager['copied_texts'] and cached['generations'] == eager['generations']
    again = _gen(model, batch, cached=True)                                  # the replayed capture
    assert torch.equal(again['gen_ids'], cached['gen_ids']) and torch.equal(again['copy_probs'], cached['copy_probs'])


def test_cached_generation_with_graphs_disabled_fp32():
    """no static stepper (tell_amd.graphs.ENABLED off): the same launches one by one over buffers of the call"""
    import tell_amd
    model, batch = _model(F32), _batch()
    eager = _gen(model, batch)
    keep = tell_amd.graphs.ENABLED
    model.reset_graphs()
    try:
        tell_amd.graphs.ENABLED = False
        cached = _gen(model, batch, cached=True)
        assert not model.__dict__.get('_decode_graphs')
    finally:
        tell_amd.graphs.ENABLED = keep
    _same_form(cached, eager)
    assert torch.equal(cached['gen_ids'], eager['gen_ids']) and torch.equal(cached['should_copy'], eager['should_copy'])
    torch.testing.assert_close(cached['log_probs'], eager['log_probs'], rtol=1e-4, atol=5e-4)
    torch.testing.assert_close(cached['copy_probs'], eager['copy_probs'], rtol=1e-4, atol=5e-4)


def test_cached_generation_draws_the_eager_nucleus_fp32():
    model, batch = _model(F32, bias=False, sampling_topk=0, sampling_topp=0.9), _batch()       # (the entity head as built: not every token a copy)
    torch.manual_seed(5)
    eager = _gen(model, batch)
    torch.manual_seed(5)
    cached = _gen(model, batch, cached=True)
    greedy = _gen(_model(F32, bias=False), batch)
    assert torch.equal(cached['gen_ids'], eager['gen_ids']) and torch.equal(cached['should_copy'], eager['should_copy'])
    n = min(greedy['gen_ids'].shape[1], eager['gen_ids'].shape[1])
    assert not torch.equal(greedy['gen_ids'][:, :n], eager['gen_ids'][:, :n]), 'the nucleus draw never left the arg-max'


def test_cached_generation_divides_the_log_probs_by_the_temperature_fp32():
    model, batch = _model(F32), _batch()
    one = _gen(model, batch, cached=True)
    model.sampling_temp = 2.0
    two = _gen(model, batch, cached=True)
    assert torch.equal(two['gen_ids'], one['gen_ids'])
    torch.testing.assert_close(two['log_probs'], one['log_probs'] / 2.0)


def test_forward_in_evaluate_mode_takes_the_cached_path_fp32():
    batch = _batch()
    texts = []
    for cached in (False, True):
        model = _model(F32, cached_generation=cached)
        model.evaluate_mode = True
        with torch.no_grad():
            out = model(**{k: ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in batch.items()})
        torch.cuda.synchronize()
        texts.append(out['copied_texts'])
        assert len(out['copied_texts']) == 4
    assert texts[0] == texts[1]


class _NoCapture:
    """The stepper's view of tell_amd.graphs with captures refused: every step is issued launch by launch."""

    def __getattr__(self, name):
        import tell_amd
        return getattr(tell_amd.graphs, name)

    @staticmethod
    def capture(*a, **kw):
        raise RuntimeError('capture refused by the test')


def _pointer_entries(model):
    return {sig: h for sig, h in model.__dict__.get('_decode_graphs', {}).items() if ('hidden',) in sig}


def _launch_by_launch(model, batch):
    """generate(cached=True) over the same static buffers with every capture refused -> (result, the entry points issued)"""
    from tell_amd.models import stepper as stepper_mod
    from test_gpu_beam_options import _Spy
    keep = stepper_mod.graphs
    model.reset_graphs()
    try:
        stepper_mod.graphs = _NoCapture()
        with _Spy() as spy:
            flat = _gen(model, batch, cached=True)
        hs = _pointer_entries(model)
        assert hs and all(h['graph'] is False for h in hs.values())
    finally:
        stepper_mod.graphs = keep
        model.reset_graphs()
    return flat, spy


def test_cached_generation_bf16_multi_step_replays_against_launch_by_launch():
    """no </s> in the articles: the rows decode past the first all-finished test, from where eight steps go as one replay"""
    model, batch = _model(BF16, bias=False), _batch(eos=False)
    flat, _ = _launch_by_launch(model, batch)
    captured = _gen(model, batch, cached=True)
    steps = captured['gen_ids'].shape[1] - 1
    print('\nbf16 B=4, no planted </s>: %d steps' % steps)
    h, = _pointer_entries(model).values()
    assert h['graph'] not in (None, False), h.get('error')
    if steps > 16:
        assert h.get(('multi', 8)) not in (None, False), h.get('multi_error')
    for k in ('gen_ids', 'should_copy', 'copy_probs', 'log_probs'):
        assert torch.equal(captured[k], flat[k]), k


def test_cached_generation_bf16_captured_against_launch_by_launch():
    from test_gpu_beam_options import _Spy
    model, batch, other = _model(BF16), _batch(), _batch(S=40)
    eager = _gen(model, batch)
    _non_vacuous(eager)
    flat, spy_flat = _launch_by_launch(model, batch)
    assert 'tell_copy_decide' in spy_flat.names and 'tell_entity_attn_step' in spy_flat.names
    assert 'tell_copy_step' not in spy_flat.names
    captured = _gen(model, batch, cached=True)
    hs = _pointer_entries(model)
    assert len(hs) == 1 and all(h['graph'] not in (None, False) for h in hs.values()), [h.get('error') for h in hs.values()]
    for k in ('gen_ids', 'should_copy', 'copy_probs', 'log_probs'):
        assert torch.equal(captured[k], flat[k]), k
    # a batch of another article length: its own signature; then the first one again, replayed without a new capture
    first = next(iter(hs.values()))
    graph_before = first['graph']
    second = _gen(model, other, cached=True)
    assert len(_pointer_entries(model)) == 2 and second['gen_ids'].shape[0] == 4
    with _Spy() as spy_replay:
        again = _gen(model, batch, cached=True)
    assert next(iter(_pointer_entries(model).values()))['graph'] is graph_before
    for k in ('gen_ids', 'should_copy', 'copy_probs', 'log_probs'):
        assert torch.equal(again[k], captured[k]), k
    # a token is one graph replay: the tail and the bookkeeping are part of the captured step, so a run over a recorded
    # signature issues none of the step's entry points from the host
    assert first.get('graph_has_post'), 'the tail is not part of the captured step'
    assert again['gen_ids'].shape[1] - 1 > 2
    for name in ('tell_copy_decide', 'tell_entity_attn_step', 'tell_greedy_update', 'tell_copy_step', 'tell_entity_logits'):
        assert name not in spy_replay.names, name
    # the invariants of test_pointer_generation_runs_and_records_copies
    ids, sc = captured['gen_ids'], captured['should_copy']
    assert ids.shape == sc.shape and bool(sc[:, 0].all()) and ids.shape[1] >= 2
    assert ids[:, 1:][sc[:, 1:]].numel() > 0
    ctx = batch['context']['roberta']
    for b in range(ids.shape[0]):
        row = ids[b, 1:][sc[b, 1:]].tolist()
        assert len(row) == len(set(row)) and set(row) <= set(ctx[b].tolist())
    n = min(ids.shape[1], eager['gen_ids'].shape[1])
    agree = float((ids[:, :n] == eager['gen_ids'][:, :n]).float().mean())
    print('\nbf16 B=4: cached against eager pointer generation: position-wise agreement %.3f over %d positions' % (agree, 4 * n))
    assert agree >= 0.8                # (tests/test_gpu_fullsize.py's gate on two bf16 launch sequences of one model)


def test_defaults_issue_the_launches_they_always_did():
    from test_gpu_beam_options import _Spy
    model, batch = _model(F32), _batch()
    with _Spy() as spy:
        _gen(model, batch)
    assert 'tell_copy_step' in spy.names
    assert 'tell_copy_decide' not in spy.names and 'tell_entity_attn_step' not in spy.names
    assert not _pointer_entries(model)
    with _Spy() as spy:
        _gen(model, batch, cached=True)
    assert 'tell_copy_step' not in spy.names and 'tell_copy_decide' in spy.names
