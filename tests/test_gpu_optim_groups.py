"""BertAdam's parameter groups on the device: tell_bertadam_step_groups through the C ABI, every
buffer between guard bands (tests/guarded.py).  The claim is conformance: within every chunk of every tensor of group g the
grouped call writes bit for bit what tell_bertadam_step2 (tell_bertadam_step_ema with an average) writes when called with
row g's eight values - so the expectation is tests/optim_groups_ref.grouped() driven with a function that runs that call
on the device, one run per group on copies, and nothing here has a tolerance except the one-step-deep comparison with
float64, which keeps the constants of tests/optim_ref.py.  Then the trainer on the tiny decoder of tests/test_gpu_train.py,
eager and through the captured step.
Run on the MI355X box:  python -m pytest tests/test_gpu_optim_groups.py -m gpu"""
import ctypes
import gc

import numpy as np
import pytest
import torch

import optim_ema_ref as ema
import optim_groups_ref as grp
import optim_ref as ref
from guarded import DEV, Guard
from test_gpu_optim import BF16, F32, I32, VARIANTS, WS_FILL, Step, bits, hold, kernel_names, plus_zero, same
from test_gpu_optim_ema import OMD_FILL, EmaStep, _batch, _clone, _model, _np, f32

pytestmark = pytest.mark.gpu

DECAY, WARM = 0.9, 10.0
_CASES = {}


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


def case(cid):
    if cid not in _CASES:
        c, d, kw, g = grp.case_kw(cid)
        d['e'] = ema.make_e(d['p'], d['lay'].real, c['seed'])
        _CASES[cid] = (c, d, kw, g)
    return _CASES[cid]


# ---------------------------------------------------------------- the two sides of the comparison
def device_step(p, g, m, v, lay, hp, grad_scale=1.0, max_norm=0.0, zero_grad=0, keep_grad=None, skip=None, wire=None,
                step=None, lr=None, lr_base=0.0, warmup=-1.0, t_total=-1.0, e=None, shadow=True, var=None, grid=None):
    """optim_ref.emulate's signature and result, computed by tell_bertadam_step2 (e given: tell_bertadam_step_ema with
    DECAY, WARM) on guarded copies - what optim_groups_ref.grouped() loops over, one run per group"""
    kw = dict(shadow=shadow, wire=wire, keep=keep_grad, skip=skip, step=step, lr=lr)
    if e is None:
        s = Step(lay, p, g, m, v, **kw)
        s.run(hp, grad_scale, max_norm, zero_grad, lr_base, warmup, t_total, var=var, grid=grid)
    else:
        s = EmaStep(lay, p, g, m, v, e, **kw)
        s.run_ema(hp, DECAY, WARM, grad_scale, max_norm, zero_grad, lr_base, warmup, t_total, var=var, grid=grid)
    assert s.intact()
    got = s.read()
    return dict(p=got['p'], m=got['m'], v=got['v'], shadow=got['shadow'], grad=got['g'], e=got.get('e'), omd=got.get('omd'),
                norms=got['norms'] if max_norm > 0 else None, partial=got['partial'], lr=got['lr'], step=got['step'],
                skip=got['skip'], applied=got['skip'] is None or got['skip'][0] == 0, aux=None)


def memo(fn, store):
    """one device run per distinct row, shared by the assignments that use it"""
    def run(p, g, m, v, lay, hp, **kw):
        key = (tuple(sorted(hp.items())), kw['max_norm'], kw.get('lr_base'), kw.get('warmup'), kw.get('t_total'), kw.get('lr'))
        if key not in store:
            store[key] = fn(p, g, m, v, lay, hp, **kw)
        return store[key]
    return run


class GroupStep(Step):
    """test_gpu_optim.Step with what tell_bertadam_step_groups adds: n_groups learning rates, tensor_group, the host table,
    and the two buffers of the average when there is one"""

    def __init__(self, lay, p, g, m, v, rows, tensor_group, e=None, lrs=None, **kw):
        super().__init__(lay, p, g, m, v, **kw)
        n = len(rows)
        self.lr = Guard((n,), F32, fill=torch.full((n,), WS_FILL) if lrs is None else f32(lrs))
        self.tg = Guard((lay.n_tensors,), I32, fill=torch.tensor(list(tensor_group), dtype=I32))
        self.ema = Guard((lay.total,), F32, fill=f32(e)) if e is not None else None
        self.omd = Guard((1,), F32, fill=torch.tensor([OMD_FILL])) if e is not None else None
        self.n_groups = n
        self.table = (ctypes.c_float * (8 * n))(*grp.table(rows).reshape(-1).tolist())

    def guards(self):
        return Step.guards(self) + [x for x in (self.tg, self.ema, self.omd) if x is not None]

    def run_groups(self, grad_scale=1.0, zero_grad=0, decay=DECAY, warm=WARM, var=None, grid=None, **over):
        """over: param / wire / lr / tg / table / n_groups / ema / omd / n_chunks replace what is handed to the library"""
        from tell_amd import hip
        ptr = lambda x: None if x is None else x.t                                # noqa: E731
        opts = {}
        if var is not None:
            opts['adam_var'] = var
        if grid is not None:
            opts['adam_grid'] = grid
        args = [over.get('param', self.param.t), self.grad.t, self.m.t, self.v.t, self.chunk_tensor, self.chunk_begin,
                over.get('n_chunks', self.lay.n_chunks), self.lay.n_tensors, self.partial.t, self.norms.t,
                over.get('lr', self.lr.t), over.get('tg', self.tg.t), over.get('table', self.table),
                over.get('n_groups', self.n_groups), float(grad_scale), ptr(self.shadow), int(zero_grad), ptr(self.skip),
                over.get('wire', ptr(self.wire)), ptr(self.step), ptr(self.keep), over.get('ema', ptr(self.ema)),
                over.get('omd', ptr(self.omd)), float(decay), float(warm)]
        with hip.options(**opts):
            hip.call('tell_bertadam_step_groups', *args)
        torch.cuda.synchronize()

    def read(self):
        out = dict(p=self.param.t.cpu().numpy(), g=self.grad.t.cpu().numpy(), m=self.m.t.cpu().numpy(),
                   v=self.v.t.cpu().numpy(), norms=self.norms.t.cpu().numpy(), lr=[float(x) for x in self.lr.t.tolist()],
                   partial=self.partial.t.cpu().numpy())
        out['shadow'] = bits(self.shadow.t.view(torch.int16).cpu().numpy()) if self.shadow is not None else None
        out['step'] = int(self.step.t.item()) if self.step is not None else None
        out['skip'] = tuple(self.skip.t.tolist()) if self.skip is not None else None
        out['e'] = self.ema.t.cpu().numpy() if self.ema is not None else None
        out['omd'] = float(self.omd.t.item()) if self.omd is not None else None
        return out


def check(got, want, lay, rows, tag):
    """every buffer bit for bit, no element excluded; norms and partial whenever some row clips"""
    for key in ('p', 'm', 'v', 'shadow', 'e'):
        if want.get(key) is None:
            assert got[key] is None, (tag, key)
            continue
        same(got[key], want[key], '%s %s' % (tag, key))
        plus_zero(got[key], ~lay.real, '%s %s' % (tag, key))
    same(got['g'], want['grad'], tag + ' grad')
    assert got['lr'] == [float(x) for x in want['lr']], (tag, got['lr'], want['lr'])
    assert got['step'] == want['step'] and got['skip'] == want['skip'], (tag, got['step'], got['skip'])
    if any(np.float32(r['max_norm']) > 0 for r in rows):
        same(got['norms'], want['norms'], tag + ' norms')
        same(got['partial'], want['partial'], tag + ' partial')
    else:                                                   # no row clips: the norm pass does not run
        assert (got['norms'] == WS_FILL).all() and (got['partial'] == WS_FILL).all(), tag
    if want.get('omd') is not None:
        assert got['omd'] == want['omd'], tag


# ---------------------------------------------------------------- the conformance claim
@pytest.mark.parametrize('grid', [1, 3, None])
@pytest.mark.parametrize('var', sorted(VARIANTS))
def test_every_tensor_is_what_step2_writes_with_its_groups_row(var, grid):
    """the four assignments x the four cases (fp32 gradient with shadow; mixed keep_grad; the bf16 wire gradient without
    shadow and without zeroing; a gradient scale) x with / without the average, on this launch shape"""
    for cid in grp.CASE_IDS:
        c, d, kw, g = case(cid)
        lay = d['lay']
        for avg in (False, True):
            e = d['e'] if avg else None
            per_row = memo(device_step, {})
            for aname, (tg, rows) in grp.ASSIGNMENTS.items():
                tag = '%s %s avg %d var %d grid %s' % (cid, aname, avg, var, grid)
                want = grp.grouped(per_row, d['p'], g, d['m'], d['v'], lay, rows, tg, skip=(0, 4), e=e, shadow=c['shadow'],
                                   var=var, grid=grid, **kw)
                s = GroupStep(lay, d['p'], g, d['m'], d['v'], rows, tg, e=e, shadow=c['shadow'], wire=kw.get('wire'),
                              keep=kw['keep_grad'], step=kw['step'], skip=(0, 4))
                s.run_groups(kw['grad_scale'], kw['zero_grad'], var=var, grid=grid)
                assert s.intact(), tag
                got = s.read()
                check(got, want, lay, rows, tag)
                assert got['step'] == kw['step'] + 1 and got['skip'] == (0, 4), tag
                for key in ('p', 'm', 'v'):
                    assert (bits(got[key]) != bits(d[key]))[lay.real].mean() > 0.5, (tag, key)           # it did move
                if len(rows) > 1:       # and the groups did matter: another group's run differs on this group's elements
                    eg = np.asarray(tg)[lay.tensor_of_elem()]
                    row0 = rows[0]
                    other = per_row(d['p'], g, d['m'], d['v'], lay, dict(b1=row0['b1'], b2=row0['b2'], eps=row0['eps'],
                                                                          wd=row0['wd']),
                                    max_norm=row0['max_norm'], step=kw['step'], lr_base=row0['lr'], warmup=row0['warmup'],
                                    t_total=row0['t_total'])
                    assert (bits(got['m']) != bits(other['m']))[lay.real & (eg != 0)].mean() > 0.5, tag


@pytest.mark.parametrize('avg', [False, True])
def test_one_group_is_step2_bit_for_bit_in_every_buffer(avg):
    """n_groups = 1: every buffer tell_bertadam_step2 / _ema has, guard bands included, on every case of the random table"""
    for c in ref.CASES:
        cid = c['id']
        d = ref.make_case(c)
        lay = d['lay']
        args, g = ref.step_args(c, d, 0)
        e = ema.make_e(d['p'], lay.real, c['seed']) if avg else None
        row = dict(lr=args['lr_base'], warmup=args['warmup'], t_total=args['t_total'], b1=d['hp']['b1'], b2=d['hp']['b2'],
                   eps=d['hp']['eps'], wd=d['hp']['wd'], max_norm=args['max_norm'])
        kw = dict(shadow=c['shadow'], wire=args.get('wire'), keep=d['keep'], step=args['step'], skip=(0, 4))
        for var, grid in ((None, None), (0, 3)):
            if avg:
                a = EmaStep(lay, d['p'], g, d['m'], d['v'], e, **kw)
                a.run_ema(d['hp'], DECAY, WARM, args['grad_scale'], args['max_norm'], args['zero_grad'], args['lr_base'],
                          args['warmup'], args['t_total'], var=var, grid=grid)
            else:
                a = Step(lay, d['p'], g, d['m'], d['v'], **kw)
                a.run(d['hp'], args['grad_scale'], args['max_norm'], args['zero_grad'], args['lr_base'], args['warmup'],
                      args['t_total'], var=var, grid=grid)
            b = GroupStep(lay, d['p'], g, d['m'], d['v'], [row], [0] * lay.n_tensors, e=e, **kw)
            b.run_groups(args['grad_scale'], args['zero_grad'], var=var, grid=grid)
            assert a.intact() and b.intact(), cid
            ga = Step.guards(a) + ([a.ema, a.omd] if avg else [])
            gb = Step.guards(b) + ([b.ema, b.omd] if avg else [])
            assert len(ga) == len(gb) >= 9
            for x, y in zip(ga, gb):
                view = (lambda t: t.view(torch.int16 if t.dtype == BF16 else torch.int32 if t.dtype == F32 else t.dtype))
                assert torch.equal(view(x.buf), view(y.buf)), (cid, var, grid)


# ---------------------------------------------------------------- exact lane
@pytest.mark.parametrize('grid', [1, 3, None])
@pytest.mark.parametrize('var', sorted(VARIANTS))
def test_exact_lane_is_the_closed_form(var, grid):
    """optim_ref's exact layouts with the four rows of powers of two: p', m, v of every element by the closed form of its
    own row (tests/test_optim_groups_host.py shows it exact in fp32), the average with decay 1/2, the caller's lr_dev"""
    lrs = [r['lr'] for r in grp.EXACT_ROWS]
    for k in range(len(ref.EXACT_LAYOUTS)):
        d = ref.exact_case(k)
        lay, tg = d['lay'], grp.exact_groups(k)
        closed = grp.exact_closed_form(k)
        for avg in (False, True):
            e0 = ema.exact_e(lay) if avg else None
            s = GroupStep(lay, d['p'], d['g'], d['m'], d['v'], grp.EXACT_ROWS, tg, e=e0, lrs=lrs, skip=(0, 3))
            s.run_groups(zero_grad=1, decay=0.5, warm=0.0, var=var, grid=grid)
            got = s.read()
            tag = 'var %d grid %s layout %d avg %d' % (var, grid, k, avg)
            for key in ('p', 'm', 'v'):
                same(got[key], closed[key].astype(np.float32), '%s %s' % (tag, key))
            same(got['norms'], d['norms'].astype(np.float32), tag + ' norms')
            same(got['shadow'], ref.bf16_rne(closed['p'].astype(np.float32)), tag + ' shadow')
            same(got['g'], np.zeros(lay.total, dtype=np.float32), tag + ' grad')
            if avg:
                e64 = e0.astype(np.float64) + 0.5 * (closed['p'] - e0.astype(np.float64))
                same(got['e'], e64.astype(np.float32), tag + ' e')
            for key in ('p', 'm', 'v', 'g', 'shadow') + (('e',) if avg else ()):
                plus_zero(got[key], ~lay.real, '%s %s' % (tag, key))
            assert got['skip'] == (0, 3) and got['lr'] == lrs and s.intact(), tag


# ---------------------------------------------------------------- one step deep against float64
@pytest.mark.parametrize('aname', sorted(grp.ASSIGNMENTS))
def test_one_step_deep_against_float64(aname):
    """optim_ref.C unchanged: the arithmetic is bertadam_update_kernel's, so its pinned constants apply"""
    tg, rows = grp.ASSIGNMENTS[aname]
    for cid in grp.CASE_IDS:
        c, d, kw, g = case(cid)
        lay = d['lay']
        s = GroupStep(lay, d['p'], g, d['m'], d['v'], rows, tg, shadow=c['shadow'], wire=kw.get('wire'), keep=kw['keep_grad'],
                      step=kw['step'])
        s.run_groups(kw['grad_scale'], kw['zero_grad'])
        got = s.read()
        want = grp.grouped(ref.step, d['p'], g, d['m'], d['v'], lay, rows, tg, p_dev=got['p'], **kw)
        tag = '%s %s' % (cid, aname)
        assert want['applied'] and s.intact(), tag
        for kind, r in ref.ratios(got, want).items():
            hold(kind, tag, r)
        for gi, row in enumerate(rows):
            hold('lr', '%s group %d' % (tag, gi), ref.lr_ratio(got['lr'][gi], want['lr'][gi], row['lr']))
        if c['shadow']:
            same(got['shadow'], want['shadow'], tag + ' shadow')
        same(got['g'], want['grad'], tag + ' grad')


# ---------------------------------------------------------------- the skip is global
def _three_steps():
    c = ref.BY_ID['three-steps']
    d = ref.make_case(c)
    d['e'] = ema.make_e(d['p'], d['lay'].real, c['seed'])
    return c, d


@pytest.mark.parametrize('var,grid,avg', [(0, 3, False), (3, 1, True), (4, None, True)])
def test_three_steps_the_middle_one_skipped_for_all_groups(var, grid, avg):
    """a NaN in a tensor of the group that does not clip, found by the norm pass another group asks for: nobody moves,
    step_dev and every lr_dev[g] do not tick, the gradient is cleared as today; the third step goes on from n = 1"""
    c, d = _three_steps()
    lay = d['lay']
    tg, rows = grp.ASSIGNMENTS['three']
    assert rows[tg[3]]['max_norm'] == 0 and rows[1]['max_norm'] > 0
    e = d['e'] if avg else None
    s = GroupStep(lay, d['p'], d['grads'][0], d['m'], d['v'], rows, tg, e=e, keep=d['keep'], step=0, skip=(0, 0))
    run = lambda: s.run_groups(c['grad_scale'], 1, var=var, grid=grid)                # noqa: E731
    kw = dict(grad_scale=c['grad_scale'], zero_grad=1, keep_grad=d['keep'], skip=(0, 0), e=e, var=var, grid=grid)
    run()
    one = s.read()
    check(one, grp.grouped(device_step, d['p'], d['grads'][0], d['m'], d['v'], lay, rows, tg, step=0, **kw), lay, rows, 'first')
    assert one['step'] == 1 and one['skip'] == (0, 0)
    bad = np.array(d['grads'][1], dtype=np.float32)
    bad[int(lay.offsets[3]) + 1] = np.nan
    s.grad.t.copy_(f32(bad))
    run()
    two = s.read()
    assert two['step'] == 1 and two['skip'] == (2, 1) and s.intact()
    for key in ('p', 'm', 'v', 'shadow') + (('e',) if avg else ()):
        same(two[key], one[key], 'skipped ' + key)
    want_g = bad.copy()
    want_g[np.repeat(d['keep'][lay.chunk_tensor] == 0, ref.CHUNK)] = 0.0
    same(two['g'], want_g, 'skipped grad')
    assert two['lr'] != one['lr'] and two['lr'][2] == 0.0     # the schedule of n = 1; the third launch writes it again
    s.grad.t.copy_(f32(d['grads'][2]))
    s.skip.t.copy_(torch.tensor([0, 1], dtype=I32))
    run()
    three = s.read()
    want = grp.grouped(device_step, one['p'], d['grads'][2], one['m'], one['v'], lay, rows, tg, step=1,
                       **dict(kw, skip=(0, 1), e=one['e']))
    check(three, want, lay, rows, 'third')
    assert three['step'] == 2 and three['skip'] == (0, 1) and three['lr'] == two['lr'] and s.intact()


def test_without_a_clipping_group_a_nan_is_not_looked_for():
    """as tell_bertadam_step2 with max_norm <= 0 does not: the step is applied, the NaN lands in its element"""
    c, d = _three_steps()
    lay = d['lay']
    tg, rows = grp.ASSIGNMENTS['three']
    rows = [dict(r, max_norm=0.0) for r in rows]
    bad = np.array(d['grads'][0], dtype=np.float32)
    at = int(lay.offsets[3]) + 1
    bad[at] = np.nan
    s = GroupStep(lay, d['p'], bad, d['m'], d['v'], rows, tg, keep=d['keep'], step=0, skip=(0, 0))
    s.run_groups(c['grad_scale'], 1)
    got = s.read()
    want = grp.grouped(device_step, d['p'], bad, d['m'], d['v'], lay, rows, tg, step=0, grad_scale=c['grad_scale'],
                       zero_grad=1, keep_grad=d['keep'], skip=(0, 0))
    check(got, want, lay, rows, 'no clip')
    assert got['step'] == 1 and got['skip'] == (0, 0) and s.intact()
    assert np.isnan(got['p'][at]) and np.isnan(got['p']).sum() == 1


# ---------------------------------------------------------------- refusals
REFUSALS = ['n_groups_0', 'n_groups_17', 'n_groups_negative', 'tensor_group_null', 'table_null', 'lr_null', 'eps_zero',
            'eps_negative', 'eps_nan', 'ema_only', 'omd_only', 'ema_misaligned', 'decay_one', 'decay_nan', 'warm_negative',
            'wire', 'param']


@pytest.mark.parametrize('what', REFUSALS)
def test_refusals_write_nothing(what):
    c, d, kw, g = case('wire-gs8-heavy-clip0.1')
    tg, rows = grp.ASSIGNMENTS['three']
    lay = d['lay']
    s = GroupStep(lay, d['p'], g, d['m'], d['v'], rows, tg, e=d['e'], wire=kw['wire'], step=kw['step'], skip=(0, 5),
                  keep=(np.arange(lay.n_tensors) % 2).astype(np.int32))
    snap = s.snapshot()
    assert len(snap) == 15
    over, decay, warm = {}, DECAY, WARM
    if what.startswith('n_groups_'):
        over['n_groups'] = {'0': 0, '17': 17, 'negative': -1}[what[9:]]
        if what == 'n_groups_17':                           # (a table long enough: the refusal must not depend on reading it)
            over['table'] = (ctypes.c_float * (8 * 17))(*(grp.table(grp.ROWS).reshape(-1).tolist() + [1.0] * 8))
    elif what == 'tensor_group_null':
        over['tg'] = None
    elif what == 'table_null':
        over['table'] = None
    elif what == 'lr_null':
        over['lr'] = None
    elif what.startswith('eps_'):                           # in the LAST row: every row is looked at
        bad = [dict(r) for r in rows]
        bad[2]['eps'] = {'zero': 0.0, 'negative': -1e-6, 'nan': float('nan')}[what[4:]]
        over['table'] = (ctypes.c_float * 24)(*grp.table(bad).reshape(-1).tolist())
    elif what == 'ema_only':
        over['omd'] = None
    elif what == 'omd_only':
        over['ema'] = None
    elif what == 'ema_misaligned':
        over['ema'] = s.ema.buf[s.ema.lo + 1:]                # 4 bytes off
    elif what.startswith('decay_'):
        decay = {'one': 1.0, 'nan': float('nan')}[what[6:]]
    elif what == 'warm_negative':
        warm = -1.0
    elif what == 'wire':
        over['wire'] = s.wire.buf[s.wire.lo + 1:]             # 2 bytes off
    else:
        over['param'] = s.param.buf[s.param.lo + 1:]
    with pytest.raises(RuntimeError, match='bertadam'):
        s.run_groups(kw['grad_scale'], 1, decay=decay, warm=warm, **over)
    torch.cuda.synchronize()
    assert s.unchanged(snap)
    assert s.lr.t.tolist() == [WS_FILL] * 3 and float(s.omd.t.item()) == OMD_FILL and int(s.step.t.item()) == kw['step']


def test_no_chunks_is_ok_and_writes_nothing_and_no_average_ignores_its_scalars():
    c, d, kw, g = case('normal-clip0.5')
    tg, rows = grp.ASSIGNMENTS['three']
    s = GroupStep(d['lay'], d['p'], g, d['m'], d['v'], rows, tg, e=d['e'], keep=d['keep'], step=kw['step'], skip=(0, 5))
    snap = s.snapshot()
    s.run_groups(kw['grad_scale'], 1, n_chunks=0)
    assert s.unchanged(snap)
    # ema and ema_omd_dev NULL together: no average, and ema_decay / ema_warm are not looked at
    a = GroupStep(d['lay'], d['p'], g, d['m'], d['v'], rows, tg, keep=d['keep'], step=kw['step'], skip=(0, 5))
    a.run_groups(kw['grad_scale'], 1, decay=float('nan'), warm=-1.0)
    b = GroupStep(d['lay'], d['p'], g, d['m'], d['v'], rows, tg, keep=d['keep'], step=kw['step'], skip=(0, 5))
    b.run_groups(kw['grad_scale'], 1, decay=0.0, warm=0.0)
    ga, gb = a.read(), b.read()
    for key in ('p', 'm', 'v', 'g', 'shadow', 'norms'):
        same(ga[key], gb[key], key)
    assert ga['step'] == kw['step'] + 1 and a.intact() and b.intact()


# ---------------------------------------------------------------- an index outside the table
@pytest.mark.parametrize('var', [0, 4])
def test_a_group_index_outside_the_table_counts_as_group_zero(var):
    c, d, kw, g = case('heavy-clip0.5-keepmixed')
    lay = d['lay']
    tg, rows = grp.ASSIGNMENTS['three']
    wild = list(tg)
    wild[0], wild[4], wild[6] = 99, -1, 3                    # 21 chunks, 3 chunks, the last chunk; 3 = n_groups itself
    clean = [0 if t in (0, 4, 6) else x for t, x in enumerate(tg)]
    runs = []
    for groups in (wild, clean):
        s = GroupStep(lay, d['p'], g, d['m'], d['v'], rows, groups, e=d['e'], keep=d['keep'], step=kw['step'], skip=(0, 0))
        s.run_groups(kw['grad_scale'], 1, var=var, grid=3)
        assert s.intact()
        runs.append(s.read())
    for key in ('p', 'm', 'v', 'g', 'shadow', 'e', 'norms'):
        same(runs[0][key], runs[1][key], key)
    assert runs[0]['lr'] == runs[1]['lr'] and runs[0]['step'] == kw['step'] + 1
    want = grp.grouped(device_step, d['p'], g, d['m'], d['v'], lay, rows, wild, e=d['e'], skip=(0, 0), var=var, grid=3,
                       **dict(kw, zero_grad=1))
    check(runs[0], want, lay, rows, 'index 99')


# ---------------------------------------------------------------- launches by name; a captured launch
@pytest.mark.parametrize('var,avg', [(4, False), (0, True), (3, True)])
def test_launched_kernels_by_name(var, avg):
    c, d, kw, g = case('normal-clip0.5')
    tg, rows = grp.ASSIGNMENTS['alternating']
    s = GroupStep(d['lay'], d['p'], g, d['m'], d['v'], rows, tg, e=d['e'] if avg else None, step=kw['step'])
    names = kernel_names(lambda: s.run_groups(kw['grad_scale'], 1, var=var))
    mine = sorted(n for n in names if 'kernel' in n)
    update = 'bertadam_update_kernel' + VARIANTS[var][:-1] + (',EmaArgs,GroupArgs>' if avg else ',GroupArgs>')
    assert any(update in n for n in names), mine
    assert sum('bertadam_update_kernel' in n for n in names) == 1, mine                 # ONE update launch for all groups
    assert sum('sqsum_chunks_kernel' in n for n in names) == 1 and sum('tensor_norms_kernel' in n for n in names) == 1, mine
    assert any('lr_schedule_groups_kernel' in n for n in names), mine
    assert not any('lr_schedule_kernel' in n for n in names), mine
    assert any('ema_schedule_kernel' in n for n in names) == avg, mine


def test_a_captured_launch_replays_with_nothing_of_the_hosts_alive():
    """the table travels by value: captured once, the host array freed, replayed on fresh gradients"""
    from tell_amd import hip
    c, d = _three_steps()
    lay = d['lay']
    tg, rows = grp.ASSIGNMENTS['seven']
    s = GroupStep(lay, d['p'], d['grads'][0], d['m'], d['v'], rows, tg, e=d['e'], keep=d['keep'], step=0, skip=(0, 0))
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    state0 = [x.buf.clone() for x in s.guards()]
    with torch.cuda.stream(side):
        s.run_groups(c['grad_scale'], 1)                    # warm, eager
        for x, b in zip(s.guards(), state0):
            x.buf.copy_(b)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            hip.call('tell_bertadam_step_groups', s.param.t, s.grad.t, s.m.t, s.v.t, s.chunk_tensor, s.chunk_begin,
                     lay.n_chunks, lay.n_tensors, s.partial.t, s.norms.t, s.lr.t, s.tg.t, s.table, s.n_groups,
                     float(c['grad_scale']), s.shadow.t, 1, s.skip.t, None, s.step.t, s.keep.t, s.ema.t, s.omd.t, DECAY, WARM)
    for i in range(len(s.table)):
        s.table[i] = float('nan')
    s.table = None
    gc.collect()
    kw = dict(grad_scale=c['grad_scale'], zero_grad=1, keep_grad=d['keep'], skip=(0, 0))
    p, m, v, e = d['p'], d['m'], d['v'], d['e']
    for n in range(2):
        s.grad.t.copy_(f32(d['grads'][n]))
        graph.replay()
        torch.cuda.synchronize()
        got = s.read()
        want = grp.grouped(device_step, p, d['grads'][n], m, v, lay, rows, tg, step=n, e=e, **kw)
        check(got, want, lay, rows, 'replay %d' % n)
        assert got['step'] == n + 1 and s.intact()
        p, m, v, e = got['p'], got['m'], got['v'], got['e']


# ---------------------------------------------------------------- the trainer
OCFG = dict(lr=5e-3, warmup=0.5, t_total=12, b1=0.9, b2=0.98, e=1e-6, weight_decay=1e-2, max_grad_norm=0.1)
# no weight decay on biases and normalisation gains, a tenth of the learning rate for the embedder
GROUPS = [[['bias', 'norm'], {'weight_decay': 0}], [['^decoder.embedder'], {'lr': 5e-4}]]


def _trainer(graph, groups, defer=False, **ocfg):
    import tell_amd
    from tell_amd.training import Trainer
    tell_amd.set_compute_dtype(torch.float32)
    tr = Trainer(_model(), dict(OCFG, parameter_groups=groups, **ocfg), device=DEV, capture_after=1)
    if not graph:
        tr.step_graph = None
    tr.defer_update = defer
    return tr


def _recorded(monkeypatch):
    """the entry points BertAdam.launch calls (and only those: the reference runs of this file call the library too)"""
    import tell_amd.training.optimizers as opt
    rec, inside = [], [False]
    real_call, real_launch = opt.hip.call, opt.BertAdam.launch

    def call(name, *args):
        if inside[0]:
            rec.append(name)
        return real_call(name, *args)

    def launch(self, *args, **kw):
        inside[0] = True
        try:
            return real_launch(self, *args, **kw)
        finally:
            inside[0] = False
    monkeypatch.setattr(opt.hip, 'call', call)
    monkeypatch.setattr(opt.BertAdam, 'launch', launch)
    return rec


@pytest.mark.parametrize('avg', [False, True])
@pytest.mark.parametrize('graph', [False, True])
def test_trainer_groups_follow_the_definition(graph, avg, monkeypatch):
    """two steps, eager and through the captured step.  A second trainer of the same model stops after backward
    (defer_update): from the masters, moments and gradients read back from it the reference loop - optim_groups_ref.grouped
    over tell_bertadam_step2 runs with each group's row - gives the masters it must have after its own grouped step, bit
    for bit; and the trainer under test, which runs the whole step (inside the graph when captured), has the same masters.
    (Gradient stores off: both trainers then zero and accumulate every gradient alike.)"""
    monkeypatch.setenv('TELL_GRAD_STORE', '0')
    rec = _recorded(monkeypatch)
    extra = dict(ema_decay=DECAY, ema_warmup=WARM) if avg else {}
    tr = _trainer(graph, GROUPS, **extra)
    rf = _trainer(graph, GROUPS, defer=True, **extra)
    opt, f = rf.optimizer, rf.flat
    assert len(opt.groups) == 3 and [len(g['names']) > 0 for g in opt.groups] == [True] * 3
    assert opt.groups[0]['weight_decay'] == 0 and opt.groups[1]['lr'] == 5e-4 and opt.groups[2]['lr'] == 5e-3
    assert any(n.endswith('bias') for n in opt.groups[0]['names']) and all('embedder' in n for n in opt.groups[1]['names'])
    assert f.tensor_group.tolist() == tr.flat.tensor_group.tolist() == grp.resolve(f.names, dict(OCFG), GROUPS)[1]
    rows = [grp.row_of(g) for g in opt.groups]
    tg = f.tensor_group.tolist()
    lay = ref.Layout([p.numel() for p in f.params])
    assert lay.total == f.total and np.array_equal(lay.chunk_tensor, _np(f.chunk_tensor))
    batch = _batch()
    for n in range(2):
        loss = rf.train_one_batch(_clone(batch))
        assert torch.isfinite(loss)
        torch.cuda.synchronize()
        p, g, m, v = (_np(x).copy() for x in (f.flat, f.grad, f.m, f.v))
        e = _np(f.ema).copy() if avg else None
        assert float(np.abs(g).max()) > 0 and opt.applied_steps() == n
        want = grp.grouped(device_step, p, g, m, v, lay, rows, tg, step=n, grad_scale=1.0, zero_grad=1, skip=(0, 0), e=e)
        opt.step(grad_scale=1.0, zero_grad=True, skip=rf.skip)
        torch.cuda.synchronize()
        tag = 'step %d' % n
        for key, t in (('p', f.flat), ('m', f.m), ('v', f.v)) + ((('e', f.ema),) if avg else ()):
            same(_np(t), want[key], '%s reference trainer %s' % (tag, key))
        same(bits(_np(f.shadow.view(torch.int16))), want['shadow'], tag + ' shadow')
        assert [float(x) for x in opt.lr_dev.tolist()] == [float(x) for x in want['lr']] and float(f.grad.abs().max()) == 0.0
        for gi in range(3):
            assert abs(float(opt.lr_dev[gi]) - opt.current_lr(n, group=gi)) <= 1e-6 * opt.groups[gi]['lr']
        if n > 0:               # (step 0 has the learning rate 0 of the warm-up's start)
            real = lay.real
            assert (bits(want['p']) != bits(p))[real].mean() > 0.5
        # the trainer under test: the whole step in one call
        loss_t = tr.train_one_batch(_clone(batch))
        torch.cuda.synchronize()
        assert float(loss_t) == float(loss)
        for key, a, b in (('p', tr.flat.flat, f.flat), ('m', tr.flat.m, f.m), ('v', tr.flat.v, f.v)):
            same(_np(a), _np(b), '%s trainer %s' % (tag, key))
        if avg:
            same(_np(tr.flat.ema), _np(f.ema), tag + ' trainer e')
    assert tr.optimizer.applied_steps() == 2 and tr.skipped_steps() == 0
    assert set(rec) == {'tell_bertadam_step_groups'} and 3 <= len(rec) <= 4      # (a replay issues no call)
    if graph:
        assert tr.step_graph.replays == 1 and [x['state'] for x in tr.step_graph.entries.values()] == ['ready']
    else:
        assert tr.step_graph is None


def test_default_config_records_no_grouped_launch(monkeypatch):
    """the groups of the shipped configs carry `{}`: the launch of the parent commit, and its bits"""
    rec = _recorded(monkeypatch)
    shipped = [[['^decoder.embedder'], {}], [['^decoder.layers.0'], {}], [['^decoder.layers.1'], {}],
               [['^decoder.layers.2'], {}], [['^decoder.layers.3'], {}], [['^decoder.adaptive_softmax'], {}]]
    a, b = _trainer(False, shipped), _trainer(False, None)
    assert len(a.optimizer.groups) == 1 and a.flat.tensor_group is None and a.optimizer.lr_dev.shape == (1,)
    batch = _batch()
    for _ in range(2):
        a.train_one_batch(_clone(batch))
        b.train_one_batch(_clone(batch))
    torch.cuda.synchronize()
    assert rec == ['tell_bertadam_step2'] * 4
    same(_np(a.flat.flat), _np(b.flat.flat), 'masters')
