"""The BertAdam step kernels through the C ABI (csrc/optim.hip: tell_bertadam_step2 / tell_bertadam_step, tell_loss_flag,
tell_fill_f32) against tests/optim_ref.py:
  * exact lane: inputs on which fp32 arithmetic is exact in any association - parameters, m, v, shadow, gradient and norms
    BIT FOR BIT on every launch shape (adam_var 0..4 x adam_grid 1 / 2 / 3 / 4096 x layouts of 1..13 chunks);
  * random lane: one step deep against the float64 step, to the bounds c_n / c_m / c_v / c_p / c_lr of optim_ref.py; the bf16
    shadow is the round-to-nearest-even of the device's own master bit for bit;
  * the two norm kernels at every trip count of their loops, one case with a second grid-stride trip of the sum of squares;
  * skip semantics, the schedule, the small entry points, the refusals.
Every buffer the library sees sits between guard bands (tests/guarded.py).  The last test is the GPU half of the wrapper
classes (BertAdam.state_dict / load_state_dict).
Run on the MI355X box:  python -m pytest tests/test_gpu_optim.py -m gpu   (-s prints every ratio the constants are pinned from)"""
import numpy as np
import pytest
import torch

import optim_ref as ref
from guarded import DEV, Guard

pytestmark = pytest.mark.gpu

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
WS_FILL = 7777.0                   # what partial / norms / lr_dev hold before a launch: a slot read unwritten shows
VARIANTS = {0: '<1,false>', 1: '<2,false>', 2: '<4,false>', 3: '<2,true>', 4: '<4,true>'}
_R = {}                            # kind -> {tag: largest ratio}
_DATA = {}


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                  # a device fault: every later launch of this process would fail the same way
        pytest.exit('GPU error, nothing more is launched: %s' % err, 3)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for kind in sorted(_R):
        tag = max(_R[kind], key=_R[kind].get)
        print('\nlargest %-3s ratio over %4d checks: %.4f  (%s)' % (kind, len(_R[kind]), _R[kind][tag], tag))


def hold(kind, tag, ratio):
    """record, print, assert: every inexact quantity goes through here"""
    _R.setdefault(kind, {})[tag] = max(_R.get(kind, {}).get(tag, 0.0), ratio)
    print('%-3s %-70s %.4f' % (kind, tag, ratio))
    assert ratio <= ref.C[kind], '%s %s: ratio %.4f above %g' % (kind, tag, ratio, ref.C[kind])


def hold_all(tag, got, want, lr_base=None):
    for k, r in ref.ratios(got, want).items():
        hold(k, tag, r)
    if lr_base is not None:
        hold('lr', tag, ref.lr_ratio(got['lr'], want['lr'], lr_base))


def data(c):
    if c['id'] not in _DATA:
        _DATA[c['id']] = ref.make_case(c)
    return _DATA[c['id']]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want, tag):
    """bit for bit (stricter than torch.equal: it tells -0 from +0)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, '%s: %d of %d differ, first at %d: got %r want %r' % (tag, bad.size, got.size, bad[0],
                                                                              got[bad[0]], want[bad[0]])


def plus_zero(a, where, tag):
    assert not bits(a)[where].any(), '%s: padding is not +0' % tag


def bf16_tensor(h):
    return torch.from_numpy(np.ascontiguousarray(h, dtype=np.uint16).view(np.int16)).view(BF16)


class Step:
    """the device side of one call: every buffer a Guard, sized exactly as include/tell_hip.h documents"""

    def __init__(self, lay, p, g, m, v, shadow=True, wire=None, keep=None, skip=None, step=None, lr=None, shadow_fill=None,
                 device_arrays=False):
        t = (lambda a: a) if device_arrays else (lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        n, T = lay.total, lay.n_tensors
        self.lay = lay
        self.param, self.grad = Guard((n,), F32, fill=t(p)), Guard((n,), F32, fill=t(g))
        self.m, self.v = Guard((n,), F32, fill=t(m)), Guard((n,), F32, fill=t(v))
        self.shadow = Guard((n,), BF16, fill=None if shadow_fill is None else bf16_tensor(shadow_fill)) if shadow else None
        self.wire = Guard((n,), BF16, fill=bf16_tensor(wire)) if wire is not None else None
        self.partial = Guard((lay.n_chunks,), F32, fill=torch.full((lay.n_chunks,), WS_FILL))
        self.norms = Guard((T,), F32, fill=torch.full((T,), WS_FILL))
        self.lr = Guard((1,), F32, fill=torch.tensor([WS_FILL if lr is None else lr]))
        self.step = Guard((1,), I32, fill=torch.tensor([step], dtype=I32)) if step is not None else None
        self.skip = Guard((2,), I32, fill=torch.tensor(list(skip), dtype=I32)) if skip is not None else None
        self.keep = Guard((T,), I32, fill=torch.from_numpy(np.asarray(keep, dtype=np.int32))) if keep is not None else None
        self.chunk_tensor = torch.from_numpy(lay.chunk_tensor).to(DEV)
        self.chunk_begin = torch.from_numpy(lay.chunk_begin).to(DEV)

    def guards(self):
        return [x for x in (self.param, self.grad, self.m, self.v, self.shadow, self.wire, self.partial, self.norms,
                            self.lr, self.step, self.skip, self.keep) if x is not None]

    def run(self, hp, grad_scale=1.0, max_norm=0.0, zero_grad=0, lr_base=0.0, warmup=-1.0, t_total=-1.0, var=None,
            grid=None, entry='tell_bertadam_step2', param=None, grad=None, wire=None, n_chunks=None):
        from tell_amd import hip
        ptr = lambda x: None if x is None else x.t                                # noqa: E731
        opts = {}
        if var is not None:
            opts['adam_var'] = var
        if grid is not None:
            opts['adam_grid'] = grid
        args = [self.param.t if param is None else param, self.grad.t if grad is None else grad, self.m.t, self.v.t,
                self.chunk_tensor, self.chunk_begin, self.lay.n_chunks if n_chunks is None else n_chunks,
                self.lay.n_tensors, self.partial.t, self.norms.t, self.lr.t, float(hp['b1']), float(hp['b2']),
                float(hp['eps']), float(hp['wd']), float(max_norm), float(grad_scale), ptr(self.shadow), int(zero_grad),
                ptr(self.skip), ptr(self.wire) if wire is None else wire, ptr(self.step), float(lr_base), float(warmup),
                float(t_total)]
        if entry == 'tell_bertadam_step2':
            args.append(ptr(self.keep))
        with hip.options(**opts):
            hip.call(entry, *args)
        torch.cuda.synchronize()

    def read(self):
        out = dict(p=self.param.t.cpu().numpy(), g=self.grad.t.cpu().numpy(), m=self.m.t.cpu().numpy(),
                   v=self.v.t.cpu().numpy(), norms=self.norms.t.cpu().numpy(), lr=float(self.lr.t.item()),
                   partial=self.partial.t.cpu().numpy())
        out['shadow'] = bits(self.shadow.t.view(torch.int16).cpu().numpy()) if self.shadow is not None else None
        out['step'] = int(self.step.t.item()) if self.step is not None else None
        out['skip'] = tuple(self.skip.t.tolist()) if self.skip is not None else None
        return out

    def snapshot(self):
        return [x.buf.clone() for x in self.guards()]

    def unchanged(self, snap):
        return all(torch.equal(x.buf.view(torch.int16 if x.buf.dtype == BF16 else x.buf.dtype),
                               s.view(torch.int16 if s.dtype == BF16 else s.dtype)) for x, s in zip(self.guards(), snap))

    def intact(self):
        return all(x.intact() for x in self.guards())


def kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name.replace(' ', '') for e in prof.events()}


# ---------------------------------------------------------------- exact lane
EXACT_KW = dict(max_norm=ref.EXACT_MAX_NORM, zero_grad=1)


def exact_want(k):
    key = ('exact', k)
    if key not in _DATA:
        d = ref.exact_case(k)
        want = ref.step(d['p'], d['g'], d['m'], d['v'], d['lay'], d['hp'], lr=ref.EXACT_LR, **EXACT_KW)
        _DATA[key] = (d, want, ref.to_f32(want))
    return _DATA[key]


def check_exact(k, tag, **run):
    d, want, w32 = exact_want(k)
    lay = d['lay']
    s = Step(lay, d['p'], d['g'], d['m'], d['v'], lr=ref.EXACT_LR, skip=(0, 3))
    s.run(d['hp'], **dict(EXACT_KW, **run))
    got = s.read()
    for key in ('p', 'm', 'v', 'norms'):
        same(got[key], w32[key], '%s %s' % (tag, key))
    same(got['shadow'], want['shadow'], tag + ' shadow')
    same(got['g'], want['grad'], tag + ' grad')
    pad = ~lay.real
    for key in ('p', 'm', 'v', 'g', 'shadow'):
        plus_zero(got[key], pad, '%s %s' % (tag, key))
    assert got['skip'] == (0, 3) and got['lr'] == ref.EXACT_LR and s.intact(), tag
    # the sums of squares per chunk are exact as well: every slot written, none twice with another value
    sq = (d['g'].astype(np.float64) ** 2).reshape(-1, ref.CHUNK).sum(1)
    same(got['partial'], sq.astype(np.float32), tag + ' partial')


@pytest.mark.parametrize('grid', [1, 2, 3, 4096])
@pytest.mark.parametrize('var', sorted(VARIANTS))
def test_exact_lane_every_launch_shape(var, grid):
    for k in range(len(ref.EXACT_LAYOUTS)):
        check_exact(k, 'var %d grid %d layout %d' % (var, grid, k), var=var, grid=grid)


def test_exact_lane_default_shape_and_forwarding_entry_point():
    """no option set: the built-in default (variant 4, 4096 blocks); tell_bertadam_step forwards with keep_grad = NULL"""
    for k in (4, 9):
        check_exact(k, 'default layout %d' % k)
        check_exact(k, 'tell_bertadam_step layout %d' % k, entry='tell_bertadam_step')


@pytest.mark.parametrize('var', sorted(VARIANTS))
def test_launched_kernels_by_name(var):
    d, want, w32 = exact_want(9)
    s = Step(d['lay'], d['p'], d['g'], d['m'], d['v'], step=0)
    names = kernel_names(lambda: s.run(d['hp'], lr_base=ref.EXACT_LR, var=var, **EXACT_KW))
    mine = sorted(n for n in names if 'kernel' in n)
    assert any('bertadam_update_kernel' + VARIANTS[var] in n for n in names), mine
    assert sum('bertadam_update_kernel' in n for n in names) == 1, mine
    for w in ('sqsum_chunks_kernel<4>', 'tensor_norms_kernel', 'lr_schedule_kernel'):
        assert any(w in n for n in names), (w, mine)
    same(s.read()['p'], w32['p'], 'profiled run')


@pytest.mark.parametrize('cid', ['heavy-clip0.5-keepmixed', 'wire-gs8-heavy-clip0.1', 'gs3-noclip'])
def test_variants_are_bit_identical_on_random_input(cid):
    c = ref.BY_ID[cid]
    d = data(c)
    args, g = ref.step_args(c, d, 0)
    first = None
    for var in sorted(VARIANTS):
        for grid in (3, 4096):
            s = Step(d['lay'], d['p'], g, d['m'], d['v'], shadow=True, wire=args.get('wire'), keep=d['keep'],
                     step=args['step'])
            s.run(d['hp'], args['grad_scale'], args['max_norm'], args['zero_grad'], args['lr_base'], args['warmup'],
                  args['t_total'], var=var, grid=grid)
            got = s.read()
            assert s.intact()
            if first is None:
                first = got
            for key in ('p', 'm', 'v', 'g', 'shadow', 'norms', 'partial'):
                same(got[key], first[key], '%s var %d grid %d %s' % (cid, var, grid, key))


# ---------------------------------------------------------------- random lane
@pytest.mark.parametrize('cid', [c['id'] for c in ref.CASES])
def test_random_lane_one_step_deep(cid):
    c = ref.BY_ID[cid]
    d = data(c)
    lay, pad = d['lay'], ~d['lay'].real
    p, m, v = d['p'], d['m'], d['v']
    with_skip = len(cid) % 2 == 0                       # half of the cases pass skip = {0, 4}, the others NULL
    for i in range(c['steps']):
        args, g = ref.step_args(c, d, i)
        s = Step(lay, p, g, m, v, shadow=c['shadow'], wire=args.get('wire'), keep=d['keep'], step=args['step'],
                 skip=(0, 4) if with_skip else None)
        s.run(d['hp'], args['grad_scale'], args['max_norm'], args['zero_grad'], args['lr_base'], args['warmup'],
              args['t_total'])
        got = s.read()
        want = ref.step(p, g, m, v, lay, d['hp'], p_dev=got['p'], skip=(0, 4) if with_skip else None, **args)
        tag = '%s step %d' % (cid, i)
        assert want['applied'] and s.intact(), tag
        hold_all(tag, got, want, c['lr'])
        if c['shadow']:
            same(got['shadow'], want['shadow'], tag + ' shadow')
            plus_zero(got['shadow'], pad, tag + ' shadow')
        same(got['g'], want['grad'], tag + ' grad')
        for key in ('p', 'm', 'v'):
            plus_zero(got[key], pad, '%s %s' % (tag, key))
        if want['norms'] is None:
            assert (got['norms'] == WS_FILL).all() and (got['partial'] == WS_FILL).all(), tag
        assert got['step'] == want['step'] and got['skip'] == want['skip'], tag
        if want['lr'] == 0.0:
            same(got['p'], p, tag + ' lr 0')
        emu = ref.emulate(p, g, m, v, lay, d['hp'], fused=True, **args)       # (reported, not asserted: section 30)
        print('    elements that differ from the fp32 emulation: ' +
              ', '.join('%s %d' % (k, (bits(got[k]) != bits(emu[k])).sum()) for k in ('p', 'm', 'v')))
        p, m, v = got['p'], got['m'], got['v']


def test_wire_gradient_equals_its_widened_fp32_gradient():
    """the same values through load_grad4's wire branch and through the fp32 buffer: the same bits out"""
    out = {}
    for cid in ('wire-clip0.5', 'wire-clip0.5-widened'):
        c = ref.BY_ID[cid]
        d = data(c)
        args, g = ref.step_args(c, d, 0)
        s = Step(d['lay'], d['p'], g, d['m'], d['v'], wire=args.get('wire'), keep=d['keep'], step=args['step'])
        s.run(d['hp'], args['grad_scale'], args['max_norm'], args['zero_grad'], args['lr_base'], args['warmup'],
              args['t_total'])
        out[cid] = s.read()
        assert s.intact()
    a, b = out['wire-clip0.5'], out['wire-clip0.5-widened']
    for key in ('p', 'm', 'v', 'shadow', 'norms', 'partial'):
        same(a[key], b[key], key)
    kept = np.repeat(d['keep'][d['lay'].chunk_tensor] != 0, ref.CHUNK) & d['lay'].real
    assert (a['g'][kept] == ref.DECOY).all() and not a['g'][~kept].any()       # the decoy: zeroed or kept, never read


# ---------------------------------------------------------------- norm kernels
def _norm_case(chunks):
    """one tensor; gradients in chosen chunks only - the first, the last, and both sides of every trip boundary of
    tensor_norms_kernel (256-stride tail, 1024-stride unrolled trips)"""
    lay = ref.Layout([chunks * ref.CHUNK - 3])
    rng = np.random.default_rng(chunks)
    chosen = sorted({x for x in (0, 1, 254, 255, 256, 257, 511, 512, 767, 768, 769, 1023, 1024, 1025, 1279, 1280,
                                 1536, 1791, 1792, 1793, 2047, 2048, chunks - 2, chunks - 1) if 0 <= x < chunks})
    g = np.zeros(lay.total, dtype=np.float32)
    for x in chosen:
        g[x * ref.CHUNK:(x + 1) * ref.CHUNK] = rng.standard_normal(ref.CHUNK) * 0.02
    g[~lay.real] = 0.0
    p = lay.scatter([rng.standard_normal(lay.sizes[0])])
    m = (0.01 * p).astype(np.float32)
    v = (m * m).astype(np.float32)
    return lay, p, g, m, v, chosen


@pytest.mark.parametrize('chunks', [1, 255, 256, 257, 769, 1023, 1024, 1025, 1300, 2100])
def test_tensor_norms_every_trip_count(chunks):
    """2100: the only size with TWO unrolled trips (c + 768 < c1 again at c = 1024 + thread for threads below 308), so that
    each of the four accumulators has to carry a non-zero sum from one trip into the next"""
    lay, p, g, m, v, chosen = _norm_case(chunks)
    kw = dict(grad_scale=0.5, max_norm=0.1, zero_grad=0, step=3, lr_base=1e-2, warmup=0.2, t_total=10.0)
    s = Step(lay, p, g, m, v, step=3, skip=(0, 0))
    s.run(ref.HP, 0.5, 0.1, 0, 1e-2, 0.2, 10.0)
    got = s.read()
    want = ref.step(p, g, m, v, lay, ref.HP, p_dev=got['p'], skip=(0, 0), **kw)
    assert s.intact() and got['skip'] == (0, 0) and want['norms'][0] > 0.1
    hold_all('norms %d chunks' % chunks, got, want, 1e-2)
    # each chosen chunk carries 1 / len(chosen) of the sum: a dropped one is orders of magnitude outside c_n
    assert 1.0 / (2 * len(chosen)) / ref.U24 > 1000 * ref.C['n']
    sq = (g.astype(np.float64) * 0.5) ** 2
    part = sq.reshape(-1, ref.CHUNK).sum(1)
    assert np.abs(got['partial'] - part).max() <= ref.C['n'] * 2 * ref.U24 * part.max()
    same(got['shadow'], want['shadow'], 'shadow')


def test_sum_of_squares_second_grid_stride_trip():
    """16 385 + 3 chunks: the smallest layout in which sqsum_chunks_kernel<4> (4096 blocks x 4 chunks) takes a second trip;
    gradients only in the chunks of that trip.  The float64 reference runs on a sample of chunks that holds all of them."""
    big = ref.Layout([16385 * ref.CHUNK - 1, 3 * ref.CHUNK - 5])
    assert big.n_chunks == 4096 * 4 + 4
    n = big.total
    idx = torch.arange(n, device=DEV)
    real = torch.from_numpy(big.real).to(DEV)
    p = (((idx * 7) % 33 - 16).float() * 0.125) * real
    m = p * 0.01
    v = m * m
    g = torch.zeros(n, device=DEV)
    rng = np.random.default_rng(7)
    tail = (rng.standard_normal(4 * ref.CHUNK) * 0.05).astype(np.float32)
    tail[~big.real[16384 * ref.CHUNK:]] = 0.0
    g[16384 * ref.CHUNK:] = torch.from_numpy(tail).to(DEV)
    s = Step(big, p, g, m, v, step=3, skip=(0, 0), device_arrays=True)
    del p, m, v, g, idx
    sample = [0, 1, 5, 4095, 4096, 8191, 12288, 16380, 16383, 16384, 16385, 16386, 16387]
    el = (torch.tensor(sample, device=DEV)[:, None] * ref.CHUNK + torch.arange(ref.CHUNK, device=DEV)[None]).reshape(-1)

    def take():
        return {k: x.t[el].cpu().numpy() for k, x in (('p', s.param), ('g', s.grad), ('m', s.m), ('v', s.v))}
    before = take()
    s.run(ref.HP, 1.0, 0.1, 1, 1e-2, 0.2, 10.0)
    after = take()
    after['norms'] = s.norms.t.cpu().numpy()
    mini = ref.Layout([10 * ref.CHUNK, 3 * ref.CHUNK])      # the sample as a layout of its own: the same tensors' norms
    want = ref.step(before['p'], before['g'], before['m'], before['v'], mini, ref.HP, p_dev=after['p'], skip=(0, 0),
                    grad_scale=1.0, max_norm=0.1, zero_grad=1, step=3, lr_base=1e-2, warmup=0.2, t_total=10.0)
    assert want['norms'].min() > 0.1
    hold_all('second trip', after, want)
    same(s.shadow.t[el].view(torch.int16).cpu().numpy().view(np.uint16), want['shadow'], 'shadow')
    assert not after['g'].any() and not bool(s.grad.t.any())
    part = s.partial.t.cpu().numpy()
    assert not part[:16384].any() and (part[16384:] > 0).all()
    assert tuple(s.skip.t.tolist()) == (0, 0) and int(s.step.t.item()) == 4 and s.intact()


# ---------------------------------------------------------------- skip semantics
SKIP_CASE = 'heavy-clip0.5-keepmixed'


def _skip_state(c, g=None, wire=None, skip=(0, 5), shadow_fill=True):
    d = data(c)
    args, g0 = ref.step_args(c, d, 0)
    g = g0 if g is None else g
    fill = ref.bf16_rne(d['p']) ^ 1 if shadow_fill else None        # a shadow that is NOT the rounding of the master
    s = Step(d['lay'], d['p'], g, d['m'], d['v'], wire=wire if wire is not None else args.get('wire'), keep=d['keep'],
             step=args['step'], skip=skip, shadow_fill=fill)
    return s, d, args, g, fill


def _assert_skipped(s, d, args, g, fill, got, skip0, zero_grad, tag):
    for key in ('p', 'm', 'v'):
        same(got[key], d[key], '%s %s' % (tag, key))
    same(got['shadow'], fill, tag + ' shadow')
    assert got['step'] == args['step'] and got['skip'] == (skip0, 6) and s.intact(), (tag, got['step'], got['skip'])
    want = np.array(g, dtype=np.float32)
    if zero_grad:
        want[np.repeat(d['keep'][d['lay'].chunk_tensor] == 0, ref.CHUNK)] = 0.0
    same(got['g'], want, tag + ' grad')
    hold('lr', tag, ref.lr_ratio(got['lr'], ref.schedule(args['step'], args['lr_base'], args['warmup'], args['t_total']),
                                 args['lr_base']))


def test_skip_zero_applies_the_step():
    c = ref.BY_ID[SKIP_CASE]
    s, d, args, g, fill = _skip_state(c)
    s.run(d['hp'], args['grad_scale'], args['max_norm'], 1, args['lr_base'], args['warmup'], args['t_total'])
    got = s.read()
    assert got['step'] == args['step'] + 1 and got['skip'] == (0, 5) and s.intact()
    same(got['shadow'], ref.bf16_rne(got['p']), 'shadow')
    assert (bits(got['p']) != bits(d['p'])).any()


@pytest.mark.parametrize('zero_grad', [0, 1])
@pytest.mark.parametrize('preset', [1, 2, 3])
def test_preset_skip_leaves_the_state_alone(preset, zero_grad):
    c = ref.BY_ID[SKIP_CASE]
    for var, grid in ((0, 3), (3, 4096), (4, 2), (None, None)):
        s, d, args, g, fill = _skip_state(c, skip=(preset, 5))
        s.run(d['hp'], args['grad_scale'], args['max_norm'], zero_grad, args['lr_base'], args['warmup'], args['t_total'],
              var=var, grid=grid)
        _assert_skipped(s, d, args, g, fill, s.read(), preset, zero_grad, 'preset %d var %s grid %s' % (preset, var, grid))


def _positions(lay):
    """an element of the first chunk, the last real element (last chunk), and one in the other chunk of the clamped tail
    group of U = 4 (30 chunks: the group 28, 29)"""
    assert lay.n_chunks == 30
    return {'first': 3, 'last': int(lay.offsets[-1]) + lay.sizes[-1] - 1, 'tail': 28 * ref.CHUNK}


@pytest.mark.parametrize('where', ['first', 'last', 'tail'])
@pytest.mark.parametrize('kind', ['fp32', 'wire'])
@pytest.mark.parametrize('bad', ['nan', 'inf', '-inf'])
def test_non_finite_gradient_sets_bit_two_and_nothing_else_changes(bad, kind, where):
    c = ref.BY_ID[SKIP_CASE]
    d = data(c)
    at = _positions(d['lay'])[where]
    g = ref.step_args(c, d, 0)[1].copy()
    wire = None
    if kind == 'wire':
        wire = ref.bf16_rne(g)
        wire[at] = {'nan': 0x7fc0, 'inf': 0x7f80, '-inf': 0xff80}[bad]
        g = np.where(d['lay'].real, ref.DECOY, 0.0).astype(np.float32)
    else:
        g[at] = float(bad)
    s, d, args, g, fill = _skip_state(c, g=g, wire=wire)
    s.run(d['hp'], args['grad_scale'], args['max_norm'], 1, args['lr_base'], args['warmup'], args['t_total'])
    _assert_skipped(s, d, args, g, fill, s.read(), 2, 1, '%s %s %s' % (bad, kind, where))


@pytest.mark.parametrize('how', ['one-square', 'tensor-sum'])
def test_overflowing_sum_of_squares_skips_the_step(how):
    """PINNED: a finite gradient whose scaled sum of squares leaves fp32 is treated as non-finite (include/tell_hip.h).
    one-square: 3e19^2 is already Inf; tensor-sum: four chunks with one 1.5e19 each - every square (2.25e38) and every chunk
    partial is finite, their sum in tensor_norms_kernel is not."""
    c = ref.BY_ID[SKIP_CASE]
    d = data(c)
    g = ref.step_args(c, d, 0)[1].copy()
    if how == 'one-square':
        g[5] = 3e19
    else:
        g[[5, 1024 + 5, 2048 + 5, 3072 + 5]] = 1.5e19
    s, d, args, g, fill = _skip_state(c, g=g)
    s.run(d['hp'], args['grad_scale'], args['max_norm'], 1, args['lr_base'], args['warmup'], args['t_total'])
    got = s.read()
    _assert_skipped(s, d, args, g, fill, got, 2, 1, how)
    assert np.isinf(got['norms'][0]) and np.isfinite(got['norms'][1:]).all()
    if how == 'tensor-sum':
        assert np.isfinite(got['partial']).all()
    want = ref.step(d['p'], g, d['m'], d['v'], d['lay'], d['hp'], skip=(0, 5), **dict(args, zero_grad=1))
    assert want['skip'] == (2, 6) and not want['applied']              # the float64 reference applies the same limit


def test_without_clipping_a_nan_gradient_is_not_inspected():
    """DOCUMENTED LIMIT (include/tell_hip.h): max_norm <= 0 launches no norm pass - the NaN goes into p, m, v of ITS element"""
    c = ref.BY_ID['gs3-noclip']
    d = data(c)
    args, g = ref.step_args(c, d, 0)
    g = g.copy()
    g[7] = np.nan
    s = Step(d['lay'], d['p'], g, d['m'], d['v'], keep=d['keep'], step=args['step'], skip=(0, 5))
    s.run(d['hp'], args['grad_scale'], 0.0, 0, args['lr_base'], args['warmup'], args['t_total'])
    got = s.read()
    assert got['skip'] == (0, 5) and got['step'] == args['step'] + 1 and s.intact()
    for key in ('p', 'm', 'v'):
        assert np.isnan(got[key][7]) and np.isnan(got[key]).sum() == 1, key
    assert (got['norms'] == WS_FILL).all()


# ---------------------------------------------------------------- schedule, small entry points, refusals
SCHEDULE = [(0.5, 4.0, s) for s in (0, 1, 2, 3, 4, 9)] + [(0.2, 10.0, s) for s in (0, 1, 2, 9, 10, 15)] + \
    [(0.2, -1.0, 7), (0.2, 0.0, 7), (-1.0, 10.0, 0), (-1.0, 10.0, 5), (-1.0, 10.0, 10)]


@pytest.mark.parametrize('warmup,t_total,step', SCHEDULE)
def test_schedule_on_the_device(warmup, t_total, step):
    c = ref.BY_ID['normal-clip0.5']
    d = data(c)
    args = dict(ref.step_args(c, d, 0)[0], step=step, warmup=warmup, t_total=t_total, lr_base=0.01)
    g = d['grads'][0]
    s = Step(d['lay'], d['p'], g, d['m'], d['v'], keep=d['keep'], step=step)
    s.run(d['hp'], args['grad_scale'], args['max_norm'], args['zero_grad'], 0.01, warmup, t_total)
    got = s.read()
    want = ref.step(d['p'], g, d['m'], d['v'], d['lay'], d['hp'], p_dev=got['p'], **args)
    tag = 'schedule warmup %g t_total %g step %d' % (warmup, t_total, step)
    hold_all(tag, got, want, 0.01)
    assert got['step'] == step + 1 and s.intact()
    if want['lr'] == 0.0:
        assert got['lr'] == 0.0
        same(got['p'], d['p'], tag + ' p')
    if (warmup, t_total) == (0.5, 4.0):                                      # exact in fp32
        assert got['lr'] == float(np.float32(0.01) * np.float32({0: 0, 1: 0.5, 2: 1, 3: 0.5}.get(step, 0))), tag


def test_without_step_dev_the_callers_lr_is_used_untouched():
    c = ref.BY_ID['normal-clip0.5']
    d = data(c)
    args, g = ref.step_args(c, d, 0)
    s = Step(d['lay'], d['p'], g, d['m'], d['v'], keep=d['keep'], lr=0.03125)
    s.run(d['hp'], args['grad_scale'], args['max_norm'], args['zero_grad'], 0.5, 0.2, 10.0)     # (schedule arguments ignored)
    got = s.read()
    want = ref.step(d['p'], g, d['m'], d['v'], d['lay'], d['hp'], p_dev=got['p'],
                    **dict(args, step=None, lr=0.03125))
    assert got['lr'] == 0.03125 and s.intact()
    hold_all('lr from the caller', got, want)


@pytest.mark.parametrize('loss,flag', [(float('nan'), 1), (float('inf'), 1), (float('-inf'), 1), (3.4e38, 0), (0.0, 0)])
def test_loss_flag(loss, flag):
    from tell_amd import hip
    for preset in (0, 1, 2, 9):
        skip = Guard((2,), I32, fill=torch.tensor([preset, 5], dtype=I32))
        x = Guard((1,), F32, fill=torch.tensor([loss]))
        hip.call('tell_loss_flag', x.t, skip.t)
        torch.cuda.synchronize()
        assert skip.t.tolist() == [flag, 5] and skip.intact() and x.intact()


@pytest.mark.parametrize('n', [0, 1, 1023, 1025, 4096 * 1024 + 7])
def test_fill_f32(n):
    from tell_amd import hip
    tail = 5                                                  # the view is longer than n: its tail is guarded too
    y = Guard((n + tail,), F32)
    hip.call('tell_fill_f32', y.t, n, 2.5)
    torch.cuda.synchronize()
    assert bool((y.t[:n] == 2.5).all()) and bool((y.t[n:] == y.sentinel).all()) and y.intact()
    if n == 0:
        assert y.untouched()


@pytest.mark.parametrize('what', ['wire', 'param', 'grad', 'eps', 'n_chunks'])
def test_refusals_write_nothing(what):
    """a misaligned bf16 gradient, misaligned fp32 buffers and eps = 0 are errors; n_chunks = 0 is a no-op: none of them
    launches anything - not even the schedule kernel, which used to run before the checks and rewrite *lr_dev"""
    c = ref.BY_ID['wire-clip0.5']
    d = data(c)
    args, g = ref.step_args(c, d, 0)
    s = Step(d['lay'], d['p'], g, d['m'], d['v'], wire=args['wire'], keep=d['keep'], step=args['step'], skip=(0, 5))
    snap = s.snapshot()
    hp, kw = d['hp'], {}
    if what == 'wire':
        kw['wire'] = s.wire.buf[s.wire.lo + 1:]               # 2 bytes off
    elif what == 'param':
        kw['param'] = s.param.buf[s.param.lo + 1:]            # 4 bytes off
    elif what == 'grad':
        kw['grad'] = s.grad.buf[s.grad.lo + 2:]               # 8 bytes off
    elif what == 'eps':
        hp = dict(hp, eps=0.0)
    else:
        kw['n_chunks'] = 0
    run = lambda: s.run(hp, args['grad_scale'], args['max_norm'], 1, args['lr_base'], args['warmup'], args['t_total'], **kw)  # noqa: E731
    if what == 'n_chunks':
        run()
    else:
        with pytest.raises(RuntimeError, match='bertadam'):
            run()
    torch.cuda.synchronize()
    assert s.unchanged(snap)


# ---------------------------------------------------------------- the wrapper classes
def test_bertadam_state_dict_round_trip():
    """three steps, the second skipped; save; load into fresh objects holding the same weights; the fourth step is
    bit-equal to the uninterrupted run's and uses the same learning rate; the saved step is the APPLIED count"""
    from tell_amd.training.optimizers import BertAdam, FlatParams
    torch.manual_seed(0)
    shapes = [(30, 70), (5,), (1024,), (2049,)]
    init = [torch.randn(*sh) for sh in shapes]
    grads = [[torch.randn(*sh).to(DEV) for sh in shapes] for _ in range(4)]
    cfg = dict(lr=1e-2, warmup=0.2, t_total=10, b1=0.9, b2=0.98, e=1e-6, weight_decay=1e-2, max_grad_norm=0.5)

    def fresh(weights):
        ps = [torch.nn.Parameter(w.detach().clone()) for w in weights]
        flat = FlatParams([('p%d' % i, p) for i, p in enumerate(ps)], DEV)
        return ps, flat, BertAdam(flat, **cfg)

    def run(ps, opt, i):
        for p, g in zip(ps, grads[i]):
            p.grad.copy_(g)
        opt.step(zero_grad=True, skip=torch.tensor([1 if i == 1 else 0, 0], dtype=I32, device=DEV))

    ps_a, flat_a, opt_a = fresh(init)
    for i in range(4):
        run(ps_a, opt_a, i)
    ps_b, flat_b, opt_b = fresh(init)
    for i in range(3):
        run(ps_b, opt_b, i)
    sd = {k: (x.clone() if torch.is_tensor(x) else x) for k, x in opt_b.state_dict().items()}
    assert sd['step'] == 2 and opt_b.step_count == 3
    ps_c, flat_c, opt_c = fresh([p.detach().cpu() for p in ps_b])
    opt_c.load_state_dict(sd)
    assert opt_c.applied_steps() == 2 and opt_c.step_count == 2
    run(ps_c, opt_c, 3)
    torch.cuda.synchronize()
    assert opt_c.applied_steps() == opt_a.applied_steps() == 3
    assert torch.equal(opt_c.lr_dev, opt_a.lr_dev) and abs(float(opt_c.lr_dev) - opt_c.current_lr(2)) < 1e-8
    for a, b in ((flat_a.flat, flat_c.flat), (flat_a.m, flat_c.m), (flat_a.v, flat_c.v), (flat_a.grad, flat_c.grad)):
        assert torch.equal(a, b)
    assert torch.equal(flat_a.shadow.view(torch.int16), flat_c.shadow.view(torch.int16))
    assert not torch.equal(flat_a.flat, flat_b.flat)
