"""The moving average of the weights on the device: tell_bertadam_step_ema and tell_ema_swap through
the C ABI against tests/optim_ema_ref.py and against tell_bertadam_step2 itself, every buffer between guard bands
(tests/guarded.py); then the trainer's surface - ema_weights(), ema_state_dict(), the checkpoint round trip - on the tiny
decoder of tests/test_gpu_train.py, eager and through the captured step.
Nothing here has a tolerance: given the master p' that the step has just written, the average is one fp32 subtraction and
one fused multiply-add deep, and everything else is compared with what tell_bertadam_step2 writes from the same inputs.
Run on the MI355X box:  python -m pytest tests/test_gpu_optim_ema.py -m gpu"""
import warnings

import numpy as np
import pytest
import torch

import optim_ema_ref as ema
import optim_ref as ref
from guarded import DEV, Guard
from test_gpu_optim import BF16, F32, I32, VARIANTS, Step, bf16_tensor, bits, exact_want, plus_zero, same
from test_gpu_train import KW, _no_dropout, _Res, _Rob

pytestmark = pytest.mark.gpu

OMD_FILL = 7777.0                  # what *ema_omd_dev holds before a launch
_DATA = {}


@pytest.fixture(autouse=True)
def _gpu(monkeypatch):
    import tell_amd
    tell_amd.hip.require_gpu()
    monkeypatch.setenv('TELL_STEP_GRAPH_STRICT', '1')       # a failed capture fails the test instead of going eager
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                  # a device fault: every later launch of this process would fail the same way
        pytest.exit('GPU error, nothing more is launched: %s' % err, 3)
    finally:
        tell_amd.set_compute_dtype(torch.float32)


def data(c):
    if c['id'] not in _DATA:
        d = ref.make_case(c)
        d['e'] = ema.make_e(d['p'], d['lay'].real, c['seed'])
        _DATA[c['id']] = d
    return _DATA[c['id']]


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


class EmaStep(Step):
    """test_gpu_optim.Step plus the two buffers of tell_bertadam_step_ema"""

    def __init__(self, lay, p, g, m, v, e, **kw):
        super().__init__(lay, p, g, m, v, **kw)
        self.ema = Guard((lay.total,), F32, fill=f32(e))
        self.omd = Guard((1,), F32, fill=torch.tensor([OMD_FILL]))

    def guards(self):
        return Step.guards(self) + [self.ema, self.omd]

    def run_ema(self, hp, decay, warm, grad_scale=1.0, max_norm=0.0, zero_grad=0, lr_base=0.0, warmup=-1.0, t_total=-1.0,
                var=None, grid=None, **over):
        """over: param / wire / ema / omd replace the buffer handed to the library (None: NULL)"""
        from tell_amd import hip
        ptr = lambda x: None if x is None else x.t                                # noqa: E731
        opts = {}
        if var is not None:
            opts['adam_var'] = var
        if grid is not None:
            opts['adam_grid'] = grid
        args = [over.get('param', self.param.t), self.grad.t, self.m.t, self.v.t, self.chunk_tensor, self.chunk_begin,
                self.lay.n_chunks, self.lay.n_tensors, self.partial.t, self.norms.t, self.lr.t, float(hp['b1']),
                float(hp['b2']), float(hp['eps']), float(hp['wd']), float(max_norm), float(grad_scale), ptr(self.shadow),
                int(zero_grad), ptr(self.skip), over.get('wire', ptr(self.wire)), ptr(self.step), float(lr_base),
                float(warmup), float(t_total), ptr(self.keep), over.get('ema', self.ema.t), over.get('omd', self.omd.t),
                float(decay), float(warm)]
        with hip.options(**opts):
            hip.call('tell_bertadam_step_ema', *args)
        torch.cuda.synchronize()

    def read(self):
        out = Step.read(self)
        out['e'] = self.ema.t.cpu().numpy()
        out['omd'] = self.omd.t.cpu().numpy()[0]
        return out


def as_bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32 if t.dtype == F32 else t.dtype)


def check_e(got, e0, n, decay, warm, tag):
    """omd is (float32)(1 - d_t) bit for bit, and e' is the kernel's two roundings from the DEVICE's own master and omd"""
    same(np.array([got['omd']]), np.array([ema.omd_at(n, decay, warm)]), tag + ' omd')
    same(got['e'], ema.ema_step(e0, got['p'], got['omd']), tag + ' e')


# ---------------------------------------------------------------- the same step as tell_bertadam_step2
@pytest.mark.parametrize('grid', [1, 3, None])
@pytest.mark.parametrize('var', sorted(VARIANTS))
def test_everything_but_the_average_is_what_step2_writes(var, grid):
    """every case of the random table (fp32 and wire gradients) x keep_grad on / off x zero_grad 0 / 1: the buffers that
    tell_bertadam_step2 has - guard bands included - are equal to its own on cloned inputs; the average is right too"""
    decay, warm = 0.9, 10.0
    for c in ref.CASES:
        d = data(c)
        lay = d['lay']
        args, g = ref.step_args(c, d, 0)
        keeps = (None, d['keep'] if d['keep'] is not None and d['keep'].any() else
                 (np.arange(lay.n_tensors) % 2).astype(np.int32) * 7)
        for keep in keeps:
            for zero_grad in (0, 1):
                kw = dict(shadow=c['shadow'], wire=args.get('wire'), keep=keep, step=args['step'], skip=(0, 4))
                run = (d['hp'], args['grad_scale'], args['max_norm'], zero_grad, args['lr_base'], args['warmup'],
                       args['t_total'])
                a = Step(lay, d['p'], g, d['m'], d['v'], **kw)
                a.run(*run, var=var, grid=grid)
                b = EmaStep(lay, d['p'], g, d['m'], d['v'], d['e'], **kw)
                b.run_ema(d['hp'], decay, warm, *run[1:], var=var, grid=grid)
                tag = '%s var %d grid %s keep %s zero_grad %d' % (c['id'], var, grid, keep is not None, zero_grad)
                assert a.intact() and b.intact(), tag
                ga, gb = a.guards(), Step.guards(b)
                assert len(ga) == len(gb) >= 9
                for x, y in zip(ga, gb):
                    assert torch.equal(as_bits(x.buf), as_bits(y.buf)), tag
                got = b.read()
                assert got['step'] == args['step'] + 1 and got['skip'] == (0, 4), tag
                check_e(got, d['e'], args['step'], decay, warm, tag)
                plus_zero(got['e'], ~lay.real, tag + ' e')
                assert (bits(got['e']) != bits(d['e']))[lay.real].mean() > 0.5, tag           # it did move


# ---------------------------------------------------------------- the schedule and the bits of the average
@pytest.mark.parametrize('decay,warm,n', ema.SCHEDULE)
def test_average_and_schedule_bit_for_bit(decay, warm, n):
    """n = None: step_dev NULL, the caller's learning rate - the warm-up then plays no part"""
    c = ref.BY_ID['normal-clip0.5']
    d = data(c)
    args, g = ref.step_args(c, d, 0)
    for var, grid in ((None, None), (0, 3)):
        s = EmaStep(d['lay'], d['p'], g, d['m'], d['v'], d['e'], keep=d['keep'], step=n, lr=None if n is not None else 0.03125)
        s.run_ema(d['hp'], decay, warm, args['grad_scale'], args['max_norm'], 1, 1e-2, 0.2, 10.0, var=var, grid=grid)
        got = s.read()
        tag = 'decay %g warm %g n %s var %s' % (decay, warm, n, var)
        assert s.intact() and got['step'] == (None if n is None else n + 1), tag
        check_e(got, d['e'], n, decay, warm, tag)
        if n is None:
            assert got['lr'] == 0.03125
        if warm == 0.0 or n is None or n >= 10 ** 5:
            same(np.array([got['omd']]), np.array([np.float32(1.0 - float(np.float32(decay)))]), tag + ' constant decay')
        same(got['shadow'], ref.bf16_rne(got['p']), tag + ' shadow')
        plus_zero(got['e'], ~d['lay'].real, tag)


# ---------------------------------------------------------------- exact lane
@pytest.mark.parametrize('grid', [1, 2, 3, 4096])
@pytest.mark.parametrize('var', sorted(VARIANTS))
def test_exact_lane_every_launch_shape(var, grid):
    """optim_ref.exact_case with decay 1/2 and 3/4 and small integers in e: e' is exact in any association, so it is the
    float64 step plus the float64 average, rounded to fp32 (tests/test_optim_ema_host.py shows that this is exact)"""
    for k in range(len(ref.EXACT_LAYOUTS)):
        d, want, w32 = exact_want(k)
        lay = d['lay']
        e0 = ema.exact_e(lay)
        for decay in (0.5, 0.75):
            s = EmaStep(lay, d['p'], d['g'], d['m'], d['v'], e0, lr=ref.EXACT_LR, skip=(0, 3))
            s.run_ema(d['hp'], decay, 0.0, max_norm=ref.EXACT_MAX_NORM, zero_grad=1, var=var, grid=grid)
            got = s.read()
            tag = 'var %d grid %d layout %d decay %g' % (var, grid, k, decay)
            for key in ('p', 'm', 'v', 'norms'):
                same(got[key], w32[key], '%s %s' % (tag, key))
            same(got['shadow'], want['shadow'], tag + ' shadow')
            same(got['g'], want['grad'], tag + ' grad')
            e64 = e0.astype(np.float64) + (1.0 - decay) * (w32['p'].astype(np.float64) - e0.astype(np.float64))
            same(got['e'], e64.astype(np.float32), tag + ' e')
            same(np.array([got['omd']]), np.array([np.float32(1.0 - decay)]), tag + ' omd')
            for key in ('p', 'm', 'v', 'g', 'shadow', 'e'):
                plus_zero(got[key], ~lay.real, '%s %s' % (tag, key))
            assert got['skip'] == (0, 3) and got['lr'] == ref.EXACT_LR and s.intact(), tag


# ---------------------------------------------------------------- variants
@pytest.mark.parametrize('cid', ['heavy-clip0.5-keepmixed', 'wire-gs8-heavy-clip0.1', 'gs3-noclip'])
def test_variants_are_bit_identical_in_the_average(cid):
    c = ref.BY_ID[cid]
    d = data(c)
    args, g = ref.step_args(c, d, 0)
    first = None
    for var in sorted(VARIANTS):
        for grid in (3, 4096):
            s = EmaStep(d['lay'], d['p'], g, d['m'], d['v'], d['e'], shadow=True, wire=args.get('wire'), keep=d['keep'],
                        step=args['step'])
            s.run_ema(d['hp'], 0.9999, 10.0, args['grad_scale'], args['max_norm'], args['zero_grad'], args['lr_base'],
                      args['warmup'], args['t_total'], var=var, grid=grid)
            got = s.read()
            assert s.intact()
            if first is None:
                first = got
            for key in ('e', 'p', 'm', 'v', 'g', 'shadow', 'norms', 'partial'):
                same(got[key], first[key], '%s var %d grid %d %s' % (cid, var, grid, key))
            assert got['omd'] == first['omd']


# ---------------------------------------------------------------- a skipped step
@pytest.mark.parametrize('var,grid', [(0, 3), (3, 1), (4, None)])
def test_three_steps_with_the_middle_one_skipped(var, grid):
    """skip[0] = 1 for the second launch: the average, the masters and the counter stay, the gradient is cleared as today,
    and the third step uses the decay of n = 1 - the schedule did not tick"""
    c = ref.BY_ID['three-steps']
    d = data(c)
    lay = d['lay']
    decay, warm = 0.9, 10.0
    s = EmaStep(lay, d['p'], d['grads'][0], d['m'], d['v'], d['e'], keep=d['keep'], step=0, skip=(0, 0))
    run = lambda: s.run_ema(d['hp'], decay, warm, c['grad_scale'], c['max_norm'], 1, c['lr'], c['warmup'],   # noqa: E731
                            c['t_total'], var=var, grid=grid)
    run()
    one = s.read()
    assert one['step'] == 1 and one['skip'] == (0, 0)
    check_e(one, d['e'], 0, decay, warm, 'first')
    s.grad.t.copy_(f32(d['grads'][1]))
    s.skip.t.copy_(torch.tensor([1, 0], dtype=I32))
    run()
    two = s.read()
    assert two['step'] == 1 and two['skip'] == (1, 1) and s.intact()
    for key in ('e', 'p', 'm', 'v', 'shadow'):
        same(two[key], one[key], 'skipped ' + key)
    want_g = np.array(d['grads'][1], dtype=np.float32)
    want_g[np.repeat(d['keep'][lay.chunk_tensor] == 0, ref.CHUNK)] = 0.0
    same(two['g'], want_g, 'skipped grad')
    same(np.array([two['omd']]), np.array([ema.omd_at(1, decay, warm)]), 'skipped omd')      # (scratch: written, unused)
    s.grad.t.copy_(f32(d['grads'][2]))
    s.skip.t.copy_(torch.tensor([0, 1], dtype=I32))
    run()
    three = s.read()
    assert three['step'] == 2 and three['skip'] == (0, 1) and s.intact()
    check_e(three, one['e'], 1, decay, warm, 'third')
    assert ema.omd_at(1, decay, warm) != ema.omd_at(2, decay, warm)
    assert (bits(three['e']) != bits(one['e']))[lay.real].mean() > 0.5


# ---------------------------------------------------------------- refusals
REFUSALS = ['ema_null', 'omd_null', 'ema_misaligned', 'decay_one', 'decay_negative', 'decay_nan', 'decay_inf',
            'warm_negative', 'warm_inf', 'warm_nan', 'wire', 'param', 'eps']


@pytest.mark.parametrize('what', REFUSALS)
def test_refusals_write_nothing(what):
    c = ref.BY_ID['wire-clip0.5']
    d = data(c)
    args, g = ref.step_args(c, d, 0)
    s = EmaStep(d['lay'], d['p'], g, d['m'], d['v'], d['e'], wire=args['wire'], keep=d['keep'], step=args['step'],
                skip=(0, 5))
    snap = s.snapshot()
    assert len(snap) == 14
    hp, decay, warm, over = d['hp'], 0.9, 10.0, {}
    if what == 'ema_null':
        over['ema'] = None
    elif what == 'omd_null':
        over['omd'] = None
    elif what == 'ema_misaligned':
        over['ema'] = s.ema.buf[s.ema.lo + 1:]                # 4 bytes off
    elif what.startswith('decay_'):
        decay = {'one': 1.0, 'negative': -0.125, 'nan': float('nan'), 'inf': float('inf')}[what[6:]]
    elif what.startswith('warm_'):
        warm = {'negative': -1.0, 'inf': float('inf'), 'nan': float('nan')}[what[5:]]
    elif what == 'wire':
        over['wire'] = s.wire.buf[s.wire.lo + 1:]             # 2 bytes off
    elif what == 'param':
        over['param'] = s.param.buf[s.param.lo + 1:]
    else:
        hp = dict(hp, eps=0.0)
    with pytest.raises(RuntimeError, match='bertadam'):
        s.run_ema(hp, decay, warm, args['grad_scale'], args['max_norm'], 1, args['lr_base'], args['warmup'],
                  args['t_total'], **over)
    torch.cuda.synchronize()
    assert s.unchanged(snap)
    assert float(s.lr.t.item()) == 7777.0 and float(s.omd.t.item()) == OMD_FILL and int(s.step.t.item()) == args['step']


# ---------------------------------------------------------------- tell_ema_swap
def _swap_buffers(chunks, shadow=True):
    n = chunks * ref.CHUNK
    rng = np.random.default_rng(chunks)
    p = (rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    e = (rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    ties = ref.make_case(ref.BY_ID['ties-lr0'])['p'][:24]          # bf16 ties, +-max, subnormals, 0
    e[:24], p[n - 24:] = ties, -ties
    e[24:28] = [0.0, -0.0, 1.0, -1.0]
    P, E = Guard((n,), F32, fill=f32(p)), Guard((n,), F32, fill=f32(e))
    S = Guard((n,), BF16, fill=bf16_tensor(ref.bf16_rne(p))) if shadow else None
    return n, p, e, P, E, S


def _read16(S):
    return bits(S.t.view(torch.int16).cpu().numpy())


@pytest.mark.parametrize('shadow', [True, False])
@pytest.mark.parametrize('chunks', [1, 30])
def test_ema_swap_exchanges_and_applied_twice_restores(chunks, shadow):
    from tell_amd import hip
    n, p, e, P, E, S = _swap_buffers(chunks, shadow)
    hip.call('tell_ema_swap', P.t, E.t, S.t if shadow else None, n)
    torch.cuda.synchronize()
    same(P.t.cpu().numpy(), e, 'param <- ema')
    same(E.t.cpu().numpy(), p, 'ema <- param')
    if shadow:
        same(_read16(S), ref.bf16_rne(e), 'shadow')
        assert (ref.bf16_rne(e) != ref.bf16_rne(p)).mean() > 0.9
    hip.call('tell_ema_swap', P.t, E.t, S.t if shadow else None, n)
    torch.cuda.synchronize()
    same(P.t.cpu().numpy(), p, 'param back')
    same(E.t.cpu().numpy(), e, 'ema back')
    if shadow:
        same(_read16(S), ref.bf16_rne(p), 'shadow back')
    assert P.intact() and E.intact() and (S is None or S.intact())


@pytest.mark.parametrize('what', ['param', 'ema', 'shadow', 'n_minus_one', 'n_1023', 'n_negative', 'param_null', 'ema_null'])
def test_ema_swap_refusals_write_nothing(what):
    from tell_amd import hip
    n, p, e, P, E, S = _swap_buffers(2)
    snap = [x.buf.clone() for x in (P, E, S)]
    a = [P.t, E.t, S.t, n]
    if what == 'param':
        a[0] = P.buf[P.lo + 1:]
    elif what == 'ema':
        a[1] = E.buf[E.lo + 2:]
    elif what == 'shadow':
        a[2] = S.buf[S.lo + 1:]
    elif what == 'param_null':
        a[0] = None
    elif what == 'ema_null':
        a[1] = None
    else:
        a[3] = {'n_minus_one': n - 1, 'n_1023': 1023, 'n_negative': -ref.CHUNK}[what]
    with pytest.raises(RuntimeError, match='ema_swap'):
        hip.call('tell_ema_swap', *a)
    torch.cuda.synchronize()
    assert all(torch.equal(as_bits(x.buf), as_bits(y)) for x, y in zip((P, E, S), snap))
    hip.call('tell_ema_swap', P.t, E.t, S.t, 0)                        # n = 0: nothing to do, no error
    torch.cuda.synchronize()
    assert all(torch.equal(as_bits(x.buf), as_bits(y)) for x, y in zip((P, E, S), snap))


# ---------------------------------------------------------------- the trainer
OCFG = dict(lr=5e-3, warmup=0.5, t_total=12, b1=0.9, b2=0.98, e=1e-6, weight_decay=1e-5, max_grad_norm=0.1)


def _dev(b):
    return {k: ({kk: vv.to(DEV) for kk, vv in v.items()} if isinstance(v, dict) else v.to(DEV)) for k, v in b.items()}


def _clone(x):
    return {k: (dict(v) if isinstance(v, dict) else v.clone()) for k, v in x.items()}


def _model(seed=0):
    from tell_amd.build import build_model
    torch.manual_seed(seed)
    m = build_model('faces_objects', _Res(True), _Rob(1024), n_bert_layers=3, **KW)
    _no_dropout(m)
    return m


def _batch(seed=61):
    from tell_amd.data import synthetic_batch
    return _dev(synthetic_batch(B=3, article_len=20, caption_len=9, faces_objects=True, vocab=600, cutoffs=(100, 300),
                                seed=seed))


def _trainer(dtype, graph, model=None, **ocfg):
    import tell_amd
    from tell_amd.training import Trainer
    tell_amd.set_compute_dtype(dtype)
    tr = Trainer(model if model is not None else _model(), dict(OCFG, **ocfg), device=DEV, capture_after=1)
    if not graph:
        tr.step_graph = None
    return tr


def _np(t):
    return t.detach().cpu().numpy()


def _state(tr):
    f = tr.flat
    return f.flat.clone(), f.ema.clone(), f.shadow.view(torch.int16).clone()


def _same_state(tr, st):
    f = tr.flat
    return torch.equal(as_bits(f.flat), as_bits(st[0])) and torch.equal(as_bits(f.ema), as_bits(st[1])) and \
        torch.equal(f.shadow.view(torch.int16), st[2])


@pytest.mark.parametrize('graph', [False, True])
def test_trainer_average_follows_the_definition(graph):
    """four steps, eager and through the captured step: after each one flat.ema is the reference recursion over the masters
    read back from the device - whatever the two paths make of the gradients"""
    tr = _trainer(torch.float32, graph, ema_decay=0.9, ema_warmup=10)
    assert tr.optimizer.ema_decay == 0.9 and tr.optimizer.ema_warmup == 10
    batch = _batch()
    e = _np(tr.flat.ema)
    same(e, _np(tr.flat.flat), 'initial average')
    real = np.zeros(tr.flat.total, dtype=bool)
    for o, p in zip(tr.flat.offsets, tr.flat.params):
        real[o:o + p.numel()] = True
    p_old = e
    for n in range(4):
        loss = tr.train_one_batch(_clone(batch))
        assert torch.isfinite(loss)
        omd = _np(tr.flat.ema_omd)[0]
        same(np.array([omd]), np.array([ema.omd_at(n, 0.9, 10.0)]), 'omd step %d' % n)
        p_new = _np(tr.flat.flat)
        e_new = ema.ema_step(e, p_new, omd)
        print('step %d: |m| %.3e, largest norm %.3e, lr %.3e, masters moved %.3f, average moved %.3f, skipped %d' % (
            n, float(tr.flat.m.abs().max()), float(tr.flat.norms.max()), float(tr.optimizer.lr_dev), (bits(p_new) != bits(p_old))[real].mean(), (bits(e_new) != bits(e))[real].mean(),
            tr.skipped_steps()))
        p_old = p_new
        same(_np(tr.flat.ema), e_new, 'average after step %d' % n)
        if n > 0:               # (step 0 has the learning rate 0 of the warm-up's start, and the average starts AT the weights)
            assert (bits(e_new) != bits(e))[real].mean() > 0.5
        plus_zero(e_new, ~real, 'padding')
        e = e_new
    assert tr.skipped_steps() == 0 and tr.optimizer.applied_steps() == 4
    if graph:
        assert tr.step_graph.replays == 3 and [x['state'] for x in tr.step_graph.entries.values()] == ['ready']
    else:
        assert tr.step_graph is None


def _generate(model, batch):
    model.eval()
    try:
        with torch.no_grad():
            out = model.generate(**_clone(batch))
        return out['gen_ids'].clone(), out['log_probs'].clone()
    finally:
        model.train()


def test_ema_weights_context():
    """bf16; decay 1/2 and one large step make the average differ from the weights by half that step"""
    from tell_amd import graphs
    tr = _trainer(torch.bfloat16, True, ema_decay=0.5, ema_warmup=0, lr=5e-2, warmup=-1, t_total=-1, max_grad_norm=1.0)
    model, batch = tr.model, _batch(9)
    tr.train_one_batch(_clone(batch))                       # eager, then captured
    tr.train_one_batch(_clone(batch))                       # the first replay
    assert tr.step_graph.replays == 1
    torch.cuda.synchronize()
    before = _state(tr)
    gap = float((tr.flat.flat - tr.flat.ema).abs().max())
    assert gap > 1e-2, gap
    ids_out, lp_out = _generate(model, batch)
    model.eval()
    with torch.no_grad():
        loss_out = float(model(**_clone(batch))['loss'])
    model.train()

    with tr.ema_weights() as inside:
        assert inside is tr and tr.optimizer.ema_swapped
        assert torch.equal(as_bits(tr.flat.flat), as_bits(before[1])) and torch.equal(as_bits(tr.flat.ema), as_bits(before[0]))
        same(bits(_np(tr.flat.shadow.view(torch.int16))), ref.bf16_rne(_np(before[1])), 'shadow inside')
        sd_in = {k: v.detach().clone() for k, v in model.state_dict().items()}
        model.eval()
        with torch.no_grad():
            loss_in = float(model(**_clone(batch))['loss'])
        model.train()
        ids_in, lp_in = _generate(model, batch)
        was = graphs.ENABLED
        graphs.ENABLED = False
        try:
            ids_in_eager, lp_in_eager = _generate(model, batch)
        finally:
            graphs.ENABLED = was
        with pytest.raises(RuntimeError, match='ema_weights'):
            tr.train_one_batch(_clone(batch))
        with pytest.raises(RuntimeError, match='ema_weights'):
            tr.optimizer.step()
        with pytest.raises(RuntimeError, match='nest'):
            with tr.ema_weights():
                pass
        assert tr.optimizer.ema_swapped                      # the refused inner context did not swap anything back
    torch.cuda.synchronize()
    assert not tr.optimizer.ema_swapped and _same_state(tr, before)

    # the forward pass really saw other weights - only then do different captions mean anything
    print('loss outside %.6f inside %.6f, largest |p - e| %.4f' % (loss_out, loss_in, gap))
    assert abs(loss_in - loss_out) > 1e-3 * abs(loss_out), (loss_in, loss_out)
    assert not torch.equal(lp_in, lp_out)
    assert not (torch.equal(ids_in, ids_out) and torch.equal(lp_in, lp_out))

    # ema_state_dict(): the state dict seen inside, detached from the flat buffer
    esd = tr.ema_state_dict()
    assert _same_state(tr, before) and set(esd) == set(sd_in)
    for k in esd:
        assert torch.equal(esd[k], sd_in[k]), k
    assert all(v.data_ptr() != p.data_ptr() for v in esd.values() for p in tr.flat.params[:3])

    # a second model, freshly built and loaded from it, generates the same captions bit for bit
    other = _model(seed=5).to(DEV)
    if hasattr(other, 'set_capture_after'):
        other.set_capture_after(1)
    other.load_state_dict(esd)
    for enabled, want in ((True, (ids_in, lp_in)), (False, (ids_in_eager, lp_in_eager))):
        was = graphs.ENABLED
        graphs.ENABLED = enabled
        try:
            ids2, lp2 = _generate(other, batch)
        finally:
            graphs.ENABLED = was
        print('graphs %s: largest log-prob difference to the second model %.3e' %
              (enabled, float((lp2.float() - want[1].float()).abs().max())))
        assert torch.equal(ids2, want[0]) and torch.equal(lp2, want[1]), enabled

    # an exception inside still restores the buffers
    with pytest.raises(KeyError):
        with tr.ema_weights():
            raise KeyError('inside')
    torch.cuda.synchronize()
    assert not tr.optimizer.ema_swapped and _same_state(tr, before)

    # training goes on: a replay of the graph captured before, no new capture, the average continues per the definition
    e0 = _np(tr.flat.ema)
    tr.train_one_batch(_clone(batch))
    assert tr.step_graph.replays == 2 and [x['state'] for x in tr.step_graph.entries.values()] == ['ready']
    same(_np(tr.flat.ema), ema.ema_step(e0, _np(tr.flat.flat), ema.omd_at(2, 0.5, 0.0)), 'average after the context')
    assert tr.optimizer.applied_steps() == 3


def test_ema_weights_needs_the_option():
    tr = _trainer(torch.float32, False)
    assert tr.flat.ema is None and tr.flat.ema_omd is None and set(tr.optimizer.state_dict()) == {'step', 'm', 'v'}
    with pytest.raises(ValueError, match='ema_decay'):
        with tr.ema_weights():
            pass
    with pytest.raises(ValueError, match='ema_decay'):
        tr.ema_state_dict()
    from tell_amd.training import Trainer
    with pytest.raises(ValueError, match='ema_decay.*1.5'):
        Trainer(_model(), dict(OCFG, type='bert_adam', ema_decay=1.5), device=DEV)
    tr.train_one_batch(_clone(_batch()))                    # and the step without the option still runs


def test_checkpoint_round_trip(monkeypatch):
    """save the optimizer state (with 'ema') and the model weights after two steps; a fresh trainer loaded from them takes
    the third step to the same masters and the same average, bit for bit.  (Gradient stores off on both sides: the fresh
    trainer's first step would otherwise be its observing one.)"""
    monkeypatch.setenv('TELL_GRAD_STORE', '0')
    batch = _batch()
    a = _trainer(torch.float32, False, ema_decay=0.9, ema_warmup=10)
    for _ in range(2):
        a.train_one_batch(_clone(batch))
    osd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.optimizer.state_dict().items()}
    msd = {k: v.detach().clone() for k, v in a.model.state_dict().items()}
    assert set(osd) == {'step', 'm', 'v', 'ema'} and osd['step'] == 2
    assert not torch.equal(osd['ema'], a.flat.flat)
    a.train_one_batch(_clone(batch))

    b = _trainer(torch.float32, False, model=_model(seed=7), ema_decay=0.9, ema_warmup=10)
    b.model.load_state_dict(msd)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        b.optimizer.load_state_dict(osd)
    assert torch.equal(b.flat.ema, osd['ema']) and torch.equal(b.flat.flat, a.flat.flat) is False
    b.train_one_batch(_clone(batch))
    torch.cuda.synchronize()
    assert torch.equal(as_bits(b.flat.flat), as_bits(a.flat.flat))
    assert torch.equal(as_bits(b.flat.ema), as_bits(a.flat.ema))
    assert b.optimizer.applied_steps() == a.optimizer.applied_steps() == 3
    same(_np(b.flat.ema_omd), np.array([ema.omd_at(2, 0.9, 10.0)]), 'omd after the reload')

    # a state without 'ema': the average restarts from the loaded weights, one warning
    c = _trainer(torch.float32, False, model=_model(seed=8), ema_decay=0.9, ema_warmup=10)
    c.model.load_state_dict(msd)
    old = {k: v for k, v in osd.items() if k != 'ema'}
    with pytest.warns(UserWarning, match="no 'ema'") as rec:
        c.optimizer.load_state_dict(old)
        c.optimizer.load_state_dict(old)
    assert len(rec) == 1
    assert torch.equal(as_bits(c.flat.ema), as_bits(c.flat.flat)) and torch.equal(c.flat.flat, osd['ema']) is False
    loaded = c.model.state_dict()
    for k, v in msd.items():
        assert torch.equal(loaded[k], v), k
