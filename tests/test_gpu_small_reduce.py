"""The reducing small kernels of the training step (csrc/elementwise.hip, csrc/multi.hip, csrc/lstm.hip) through the C ABI,
element by element against the float64 reference and the bounds of tests/small_ref.py: weight norm
(tell_wn_rowscale, tell_wn_weight, tell_wn_backward, tell_wn_weight_multi, tell_wn_backward_multi, tell_wn_backward_multi2), the
RoBERTa layer mix (tell_mix_fwd, tell_mix_bwd, tell_mix_wgrad), column sums (tell_colsum, tell_colsum_multi), the LSTM pieces
(tell_lstm_cell_fwd / _bwd, tell_dot_attn_fwd / _bwd, tell_tanh_fwd / _bwd) and, bit for bit, the transposes (tell_transpose,
tell_transpose_multi).  Every operand and every output is a view inside a buffer of sentinels
(tests/guarded.py): after each launch every guard band and every row gap is intact, and every read-only operand is bit for
bit what was put in.  Mix and multi weight norm run with bw_wgs 0 and 13.
Run on the MI355X box:  python -m pytest tests/test_gpu_small_reduce.py -m gpu -s   (-s prints the ratios c is pinned from and
the time of the whole file)"""
import time

import numpy as np
import pytest
import torch

import small_ref as ref
from guarded import Guard

pytestmark = pytest.mark.gpu

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
TD = {'float32': F32, 'bfloat16': BF16}
INTS = {'int32': I32, 'int64': torch.int64, 'uint8': torch.uint8}
OUTS = ('bfloat16', 'float32')
BW = (0, 13)
_RATIOS, _UNPINNED = {}, {}


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    _UNPINNED.clear()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                  # a device fault: every later launch of this process would fail the same way
        pytest.exit('GPU error, nothing more is launched: %s' % err, 3)


@pytest.fixture(scope='module', autouse=True)
def _report():
    t0 = time.time()
    yield
    for k in sorted(_RATIOS):
        print('\nlargest (|got - ref| - u_out |ref|) / (gamma 2^-24 S)  %-12s %.6f   c = %s' % (k, _RATIOS[k], ref.C.get(k)))
    print('\n%s: %.1f s' % (__name__, time.time() - t0))


class In:
    """a read-only operand: a Guard holding `a` (numpy, already rounded to its storage type), checked bit for bit afterwards"""

    def __init__(self, a, dtype, strides=None, off=0):
        self.a = np.ascontiguousarray(a, {'int32': np.int32, 'int64': np.int64, 'uint8': np.uint8}.get(dtype, np.float32))
        self.g = Guard(self.a.shape, INTS.get(dtype) or TD[dtype], strides, torch.from_numpy(self.a), off)
        self.t = self.g.t

    def intact(self):
        return self.g.intact() and ref.same_bits(host(self.g), self.a)


def out_guard(shape, dtype, fill=None, strides=None, off=0):
    fill = None if fill is None else torch.from_numpy(np.ascontiguousarray(fill, np.float32))
    return Guard(shape, TD[dtype], strides, fill, off)


def host(g):
    """a Guard's (or tensor's) view as fp32 numpy"""
    t = g.t if hasattr(g, 't') else g
    return t.float().cpu().numpy()


def intact(*guards):
    torch.cuda.synchronize()
    for i, g in enumerate(guards):
        assert g is None or g.intact(), 'operand %d of the launch: written outside its view, or a read-only operand changed' % i


def check(got, o, tag):
    """`got` (Guard, tensor or numpy) against the Out `o`: exact and derived-bound outputs at once, a measured group against
    its pinned constant - or, not pinned yet, recorded for settle()"""
    got = got if isinstance(got, np.ndarray) else host(got)
    assert got.shape == np.shape(o.value), tag
    if o.group in ('exact', None):
        bad = ref.failures(got, o)
        assert bad == 0, '%s: %d of %d elements %s' % (tag, bad, got.size, 'differ' if o.group else 'outside the derived bound')
        return
    rt = ref.ratio(got, o)
    _RATIOS[o.group] = max(_RATIOS.get(o.group, 0.0), rt)
    print('ratio %-12s %-52s %.6f' % (o.group, tag, rt))
    if o.group not in ref.C:
        _UNPINNED[o.group] = max(_UNPINNED.get(o.group, 0.0), rt)
        assert np.isfinite(got[np.isfinite(np.asarray(o.value, np.float64))]).all(), tag
        return
    bad = ref.failures(got, o)
    assert bad == 0, '%s %s: %d of %d outside the bound (ratio %.4f, c = %g)' % (o.group, tag, bad, got.size, rt, ref.C[o.group])


def settle():
    """until c is pinned the test fails with the measured ratio in its message"""
    assert not _UNPINNED, 'constant not pinned yet, largest ratios of this case: %s' % \
        ', '.join('%s %.6f' % kv for kv in sorted(_UNPINNED.items()))


def ids(table):
    return [c['id'] for c in table]


# ---------------------------------------------------------------- weight norm
class WN:
    """the guarded operands of one tensor: g, v, dW read-only; w, norms, scale fresh; dg, dv prefilled"""

    def __init__(self, case, out):
        x, rows, cols = ref.wn_inputs(case), case['rows'], case['cols']
        self.case, self.rows, self.cols = case, rows, cols
        self.g, self.v = In(x['g'], 'float32'), In(x['v'], 'float32')
        self.dW = In(x['dW'], 'float32', off=1 if case['off'] == 'dW' else 0)
        self.w = out_guard((rows, cols), out)
        self.norms, self.scale = out_guard((rows,), 'float32'), out_guard((rows,), 'float32')
        self.fresh_grads()

    def fresh_grads(self):
        x = ref.wn_inputs(self.case)
        self.dg = out_guard((self.rows,), 'float32', x['dg0'])
        self.dv = out_guard((self.rows, self.cols), 'float32', x['dv0'], off=1 if self.case['off'] == 'dv' else 0)

    def all(self):
        return [self.g, self.v, self.dW, self.w, self.norms, self.scale, self.dg, self.dv]


@pytest.mark.parametrize('out', OUTS)
@pytest.mark.parametrize('case', ref.WN, ids=ids(ref.WN))
def test_weight_norm(case, out):
    """tell_wn_rowscale, tell_wn_weight, then the backward on the forward's own norms: tell_wn_backward (accumulate) or
    tell_wn_backward_multi2 with one tensor (store), the multi entry points with bw_wgs 0 and 13"""
    from tell_amd import hip
    from tell_amd.decode import _ints, _ptrs
    t = WN(case, out)
    rows, cols = t.rows, t.cols
    hip.call('tell_wn_rowscale', t.g.t, t.v.t, rows, cols, t.scale.t, t.norms.t)
    intact(*t.all())
    assert t.w.untouched()
    want = ref.wn_case(case, out)
    check(t.norms, want['norms'], '%s rowscale norms' % case['id'])
    check(t.scale, want['scale'], '%s rowscale scale' % case['id'])
    first = host(t.norms)
    t.norms = out_guard((rows,), 'float32')
    hip.call('tell_wn_weight', t.g.t, t.v.t, rows, cols, t.w.t, hip.dt(TD[out]), t.norms.t)
    intact(*t.all())
    check(t.norms, want['norms'], '%s weight norms' % case['id'])
    check(t.w, want['w'], '%s w %s' % (case['id'], out))
    if ref.wn_path(cols) == 'scalar':
        assert ref.same_bits(first, host(t.norms)), 'the scalar norm loop of tell_wn_weight is tell_wn_rowscale\'s'
    norms = host(t.norms)
    want = ref.wn_case(case, out, norms=norms)
    seen = []
    for entry, bw in [('single', 0)] * (not case['store']) + [('multi', b) for b in BW]:
        t.fresh_grads()
        if entry == 'single':
            hip.call('tell_wn_backward', t.dW.t, t.g.t, t.v.t, t.norms.t, rows, cols, t.dg.t, t.dv.t)
        else:
            args = (1, _ptrs([t.dW.t]), _ptrs([t.g.t]), _ptrs([t.v.t]), _ptrs([t.norms.t]), _ints([rows]), _ints([cols]),
                    _ptrs([t.dg.t]), _ptrs([t.dv.t]))
            with hip.options(bw_wgs=bw):
                if case['store']:
                    hip.call('tell_wn_backward_multi2', *args, _ints([1]))
                else:
                    hip.call('tell_wn_backward_multi', *args)
        intact(*t.all())
        assert ref.same_bits(host(t.norms), norms)
        tag = '%s %s bw_wgs %d' % (case['id'], entry, bw)
        check(t.dg, want['dg'], tag + ' dg')
        check(t.dv, want['dv'], tag + ' dv')
        seen.append((host(t.dg), host(t.dv)))
    for a in seen[1:]:
        assert ref.same_bits(a[0], seen[0][0]) and ref.same_bits(a[1], seen[0][1]), 'the entry points disagree'
    settle()


@pytest.mark.parametrize('bw', BW)
@pytest.mark.parametrize('out', OUTS)
@pytest.mark.parametrize('pattern', sorted(ref.WN_MULTI_STORE))
def test_weight_norm_multi(pattern, out, bw):
    """36 tensors: a launch of 32 and one of 4; `store` set where a tensor's global and per-launch indices disagree"""
    from tell_amd import hip
    from tell_amd.decode import _ints, _ptrs
    n = ref.WN_MULTI_N
    ts = [WN(ref.wn_multi_case(j), out) for j in range(n)]
    rows, cols = _ints([t.rows for t in ts]), _ints([t.cols for t in ts])
    every = [g for t in ts for g in t.all()]
    with hip.options(bw_wgs=bw):
        hip.call('tell_wn_weight_multi', n, _ptrs([t.g.t for t in ts]), _ptrs([t.v.t for t in ts]), _ptrs([t.w.t for t in ts]),
                 _ptrs([t.norms.t for t in ts]), rows, cols, hip.dt(TD[out]))
        intact(*every)
        norms = [host(t.norms) for t in ts]
        hip.call('tell_wn_backward_multi2', n, _ptrs([t.dW.t for t in ts]), _ptrs([t.g.t for t in ts]),
                 _ptrs([t.v.t for t in ts]), _ptrs([t.norms.t for t in ts]), rows, cols, _ptrs([t.dg.t for t in ts]),
                 _ptrs([t.dv.t for t in ts]),
                 _ints([int(j in ref.WN_MULTI_STORE[pattern]) for j in range(n)]))
        intact(*every)
    want = ref.wn_multi(pattern, out, norms=norms)
    for j, (t, r) in enumerate(zip(ts, want)):
        assert t.scale.untouched() and ref.same_bits(host(t.norms), norms[j])
        for k in ('norms', 'w', 'dg', 'dv'):
            check(getattr(t, k), r[k], 'multi %s tensor %d %s bw_wgs %d %s' % (pattern, j, out, bw, k))
    settle()


# ---------------------------------------------------------------- RoBERTa layer mix
def mix_operands(case):
    x, dty = ref.mix_inputs(case), ref.mix_dtype(case)
    return (In(x['H'], dty, off=1 if case['kind'] == 'bf16_off' else 0), In(x['dout'], dty), In(x['w'], 'float32'), dty)


@pytest.mark.parametrize('bw', BW)
@pytest.mark.parametrize('case', ref.MIX, ids=ids(ref.MIX))
def test_mix_forward_and_backward(case, bw):
    from tell_amd import hip
    H, dout, w, dty = mix_operands(case)
    L, n = case['L'], case['n']
    out = out_guard((n,), dty)
    with hip.options(bw_wgs=bw):
        hip.call('tell_mix_fwd', H.t, w.t, L, n, out.t, hip.dt(TD[dty]))
        intact(H, dout, w, out)
        check(out, ref.mix_case(case, 1)['out'], '%s bw_wgs %d out' % (case['id'], bw))
        for nb in ref.MIX_BLOCKS:
            partial = out_guard((nb, L), 'float32')
            hip.call('tell_mix_bwd', H.t, dout.t, L, n, partial.t, nb, hip.dt(TD[dty]))
            intact(H, dout, w, partial)
            check(partial, ref.mix_case(case, nb)['partial'], '%s bw_wgs %d blocks %d partial' % (case['id'], bw, nb))
    settle()


@pytest.mark.parametrize('case', ref.MIX_WGRAD, ids=ids(ref.MIX_WGRAD))
def test_mix_wgrad(case):
    """the logit gradient from the partials tell_mix_bwd itself wrote (checked on their own first), gw prefilled"""
    from tell_amd import hip
    src, nb = ref.mix_wgrad_source(), case['nb']
    H, dout, w, dty = mix_operands(src)
    L, n = src['L'], src['n']
    partial = out_guard((nb, L), 'float32')
    hip.call('tell_mix_bwd', H.t, dout.t, L, n, partial.t, nb, hip.dt(TD[dty]))
    intact(H, dout, w, partial)
    check(partial, ref.mix_case(src, nb)['partial'], 'wgrad source blocks %d partial' % nb)
    p = host(partial)
    gw0 = ref.mix_inputs(src)['gw0']
    gw = out_guard((L,), 'float32', gw0)
    hip.call('tell_mix_wgrad', partial.t, nb, L, w.t, gw.t)
    intact(w, partial, gw)
    assert ref.same_bits(host(partial), p)
    check(gw, ref.mix_wgrad(p, ref.mix_inputs(src)['w'], gw0)['gw'], 'wgrad blocks %d' % nb)
    settle()


# ---------------------------------------------------------------- column sums
@pytest.mark.parametrize('case', ref.COLSUM, ids=ids(ref.COLSUM))
def test_colsum(case):
    from tell_amd import hip
    x, rows, Cc = ref.colsum_inputs(case), case['rows'], case['C']
    ld, nch = Cc + case['pad'], ref.colsum_chunks(rows)
    assert nch == hip.lib().tell_colsum_chunks(rows)
    src = In(x['x'], case['dtype'], (ld, 1))
    out = out_guard((Cc,), 'float32', x['out0'])
    m = None if case['m'] is None else In(np.array([case['m']]), 'int32')
    ws = out_guard((nch * Cc,), 'float32')
    hip.call('tell_colsum', src.t, ld, rows, Cc, hip.dt(TD[case['dtype']]), out.t, case['acc'], None if m is None else m.t,
             case['scale'], ws.t)
    intact(src, out, m, ws)
    assert nch > 1 or ws.untouched(), 'a single chunk goes straight to out'
    check(out, ref.colsum_case(case)['out'], case['id'])
    settle()


def test_colsum_multi():
    """50 jobs (48 + 2): every row count around the 4-way unrolled walk, widths around a 64-column block, the three kinds of
    split between dst0 and dst1 (a null pointer for the empty side), ld > width, both destinations prefilled"""
    from tell_amd import hip
    from tell_amd.decode import _ints, _longs, _ptrs
    jobs, xs = [ref.csm_job(j) for j in range(ref.CSM_N)], ref.csm_inputs()
    src = [In(x['x'], 'float32', (job['ld'], 1)) for job, x in zip(jobs, xs)]
    d0 = [out_guard((job['w0'],), 'float32', x['d0'][:job['w0']]) if job['w0'] else None for job, x in zip(jobs, xs)]
    d1 = [out_guard((job['width'] - job['w0'],), 'float32', x['d0'][job['w0']:]) if job['w0'] < job['width'] else None
          for job, x in zip(jobs, xs)]
    hip.call('tell_colsum_multi', ref.CSM_N, _ptrs([s.t for s in src]), _longs([job['ld'] for job in jobs]),
             _ints([job['rows'] for job in jobs]), _ints([job['width'] for job in jobs]), _ints([job['w0'] for job in jobs]),
             _ptrs([None if g is None else g.t for g in d0]), _ptrs([None if g is None else g.t for g in d1]))
    intact(*(src + d0 + d1))
    for j, o in enumerate(ref.colsum_multi()):
        got = np.concatenate([host(g) for g in (d0[j], d1[j]) if g is not None])
        check(got, o, 'colsum_multi job %d %s' % (j, jobs[j]))
    settle()


# ---------------------------------------------------------------- transposes (exact)
@pytest.mark.parametrize('case', ref.TR, ids=ids(ref.TR))
def test_transpose(case):
    """every leading dimension padded: the gaps keep the sentinel; a null dst_t / dst_plain / row_scale"""
    from tell_amd import hip
    x, rows, cols = ref.tr_inputs(case), case['rows'], case['cols']
    s, d = case['types']
    src = In(x['src'], s, (cols + 3, 1))
    sc = None if x['scale'] is None else In(x['scale'], 'float32')
    dt_ = out_guard((cols, rows), d, strides=(rows + 5, 1)) if case['outs'] in ('both', 't') else None
    dp = out_guard((rows, cols), d, strides=(cols + 2, 1)) if case['outs'] in ('both', 'plain') else None
    hip.call('tell_transpose', src.t, cols + 3, hip.dt(TD[s]), None if dt_ is None else dt_.t, rows + 5,
             None if dp is None else dp.t, cols + 2, hip.dt(TD[d]), None if sc is None else sc.t, rows, cols)
    intact(src, sc, dt_, dp)
    want = ref.tr_case(case)
    for k, g in (('t', dt_), ('plain', dp)):
        if g is not None:
            check(g, want[k], '%s %s' % (case['id'], k))


def test_transpose_multi():
    """50 jobs (48 + 2) of bf16, leading dimensions padded to multiples of 8"""
    from tell_amd import hip
    from tell_amd.decode import _ints, _longs, _ptrs
    xs = ref.trm_inputs()
    up8 = lambda v: (v + 7) // 8 * 8                                                              # noqa: E731
    ls = [up8(x.shape[1]) + 8 * (j % 2) for j, x in enumerate(xs)]
    ldd = [up8(x.shape[0]) + 8 * (j % 3 == 0) for j, x in enumerate(xs)]
    src = [In(x, 'bfloat16', (l, 1)) for x, l in zip(xs, ls)]
    dst = [out_guard(x.shape[::-1], 'bfloat16', strides=(l, 1)) for x, l in zip(xs, ldd)]
    hip.call('tell_transpose_multi', ref.TRM_N, _ptrs([s.t for s in src]), _longs(ls), _ptrs([g.t for g in dst]), _longs(ldd),
             _ints([x.shape[0] for x in xs]), _ints([x.shape[1] for x in xs]))
    intact(*(src + dst))
    for j, o in enumerate(ref.transpose_multi()):
        check(dst[j], o, 'transpose_multi job %d %s' % (j, xs[j].shape))


# ---------------------------------------------------------------- LSTM pieces
@pytest.mark.parametrize('dty', OUTS)
@pytest.mark.parametrize('case', ref.LSTM, ids=ids(ref.LSTM))
def test_lstm_cell(case, dty):
    """the forward, then the backward on the gates and the cell state the forward itself stored; dh or dc a null pointer"""
    from tell_amd import hip
    x, B, H = ref.lstm_inputs(case, dty), case['B'], case['H']
    g1, g2, cp = In(x['g1'], dty), In(x['g2'], dty), In(x['c_prev'], dty)
    h, c, gates = out_guard((B, H), dty), out_guard((B, H), dty), out_guard((B, 4 * H), 'float32')
    code = hip.dt(TD[dty])
    hip.call('tell_lstm_cell_fwd', g1.t, g2.t, cp.t, h.t, c.t, gates.t, B, H, code)
    intact(g1, g2, cp, h, c, gates)
    want = ref.lstm_case(case, dty)
    for k, g in (('h', h), ('c', c), ('gates', gates)):
        check(g, want[k], '%s %s %s' % (case['id'], dty, k))
    gk, ck = host(gates), host(c)
    want = ref.lstm_case(case, dty, gates=gk, c=ck)
    dh = None if case['null'] == 'dh' else In(x['dh'], dty)
    dc = None if case['null'] == 'dc' else In(x['dc'], dty)
    dgates, dcp = out_guard((B, 4 * H), dty), out_guard((B, H), dty)
    hip.call('tell_lstm_cell_bwd', None if dh is None else dh.t, None if dc is None else dc.t, gates.t, c.t, cp.t, dgates.t,
             dcp.t, B, H, code)
    intact(dh, dc, gates, c, cp, dgates, dcp)
    assert ref.same_bits(host(gates), gk) and ref.same_bits(host(c), ck)
    check(dgates, want['dgates'], '%s %s dgates' % (case['id'], dty))
    check(dcp, want['dc_prev'], '%s %s dc_prev' % (case['id'], dty))
    settle()


@pytest.mark.parametrize('dty', OUTS)
@pytest.mark.parametrize('n', ref.TANH_N)
def test_tanh(n, dty):
    from tell_amd import hip
    r = ref._rng('tanh', n)
    x, dy = In(ref.store(r.standard_normal(n) * 2, dty), dty), In(ref.store(r.standard_normal(n), dty), dty)
    y, dx = out_guard((n,), dty), out_guard((n,), dty)
    hip.call('tell_tanh_fwd', x.t, y.t, n, hip.dt(TD[dty]))
    intact(x, y)
    check(y, ref.tanh_fwd(x.a, dty)['y'], 'tanh n %d %s' % (n, dty))
    yk = host(y)
    hip.call('tell_tanh_bwd', dy.t, y.t, dx.t, n, hip.dt(TD[dty]))
    intact(dy, y, dx)
    assert ref.same_bits(host(y), yk)
    check(dx, ref.tanh_bwd(dy.a, yk, dty)['dx'], 'tanh_bwd n %d %s' % (n, dty))
    settle()


@pytest.mark.parametrize('dty', OUTS)
@pytest.mark.parametrize('case', ref.DA, ids=ids(ref.DA))
def test_dot_attention(case, dty):
    """forward, then the backward on the probabilities the forward stored.  A fully masked row is NaN in probs, ctx, dx and
    dsrc (softmax of all -inf); every other row stays in bound"""
    from tell_amd import hip
    x, L, B, D = ref.da_inputs(case, dty), case['L'], case['B'], case['D']
    strides = {'lbd': (B * D, D, 1), 'bld': (D, L * D, 1), 'padded': (B * (D + 3), D + 3, 1)}[case['lay']]
    src, q, dctx = In(x['src'], dty, strides), In(x['x'], dty), In(x['dctx'], dty)
    mask = None if x['mask'] is None else In(x['mask'], 'uint8')
    ctx, probs = out_guard((B, D), dty), out_guard((L, B), 'float32')
    code = hip.dt(TD[dty])
    hip.call('tell_dot_attn_fwd', src.t, strides[0], strides[1], q.t, None if mask is None else mask.t, ctx.t, probs.t,
             L, B, D, code)
    intact(src, q, mask, ctx, probs)
    want = ref.da_case(case, dty)
    check(probs, want['probs'], '%s %s probs' % (case['id'], dty))
    check(ctx, want['ctx'], '%s %s ctx' % (case['id'], dty))
    pk = host(probs)
    assert np.array_equal(np.isnan(pk), np.isnan(np.asarray(want['probs'].value)))
    want = ref.da_case(case, dty, probs=pk)
    dx = out_guard((B, D), dty)
    dsrc = out_guard((L, B, D), dty) if case['dsrc'] else None
    hip.call('tell_dot_attn_bwd', src.t, strides[0], strides[1], probs.t, dctx.t, q.t, dx.t, None if dsrc is None else dsrc.t,
             L, B, D, code)
    intact(src, q, dctx, probs, dx, dsrc)
    assert ref.same_bits(host(probs), pk)
    check(dx, want['dx'], '%s %s dx' % (case['id'], dty))
    if dsrc is not None:
        check(dsrc, want['dsrc'], '%s %s dsrc' % (case['id'], dty))
    settle()


# ---------------------------------------------------------------- refusals
def test_refused_calls_launch_nothing():
    """mix with L = 0 or L = 65, dot attention with L = 1025 and an unaligned weight-norm forward: the binding's error, every
    output untouched"""
    from tell_amd import hip
    case = ref.MIX[1]
    H, dout, w, dty = mix_operands(case)
    out, partial, gw = out_guard((case['n'],), dty), out_guard((3, 64), 'float32'), out_guard((64,), 'float32')
    for L in (0, 65):
        for name, args in (('tell_mix_fwd', (H.t, w.t, L, case['n'], out.t, hip.dt(TD[dty]))),
                           ('tell_mix_bwd', (H.t, dout.t, L, case['n'], partial.t, 3, hip.dt(TD[dty]))),
                           ('tell_mix_wgrad', (partial.t, 3, L, w.t, gw.t))):
            with pytest.raises(RuntimeError, match=name):
                hip.call(name, *args)
    t = WN(ref.WN[4], 'float32')
    w_off = out_guard((t.rows, t.cols), 'float32', off=1)
    with pytest.raises(RuntimeError, match='tell_wn_weight'):
        hip.call('tell_wn_weight', t.g.t, t.v.t, t.rows, t.cols, w_off.t, hip.dt(F32), t.norms.t)
    z = In(np.zeros((1025, 1, 8), np.float32), 'float32')
    ctx, probs, dsrc = out_guard((1, 8), 'float32'), out_guard((1025, 1), 'float32'), out_guard((1025, 1, 8), 'float32')
    with pytest.raises(RuntimeError, match='tell_dot_attn_fwd'):
        hip.call('tell_dot_attn_fwd', z.t, 8, 8, z.t, None, ctx.t, probs.t, 1025, 1, 8, hip.dt(F32))
    with pytest.raises(RuntimeError, match='tell_dot_attn_bwd'):
        hip.call('tell_dot_attn_bwd', z.t, 8, 8, z.t, z.t, z.t, ctx.t, dsrc.t, 1025, 1, 8, hip.dt(F32))
    torch.cuda.synchronize()
    assert out.untouched() and partial.untouched() and gw.untouched() and w_off.untouched() and t.norms.untouched()
    assert ctx.untouched() and probs.untouched() and dsrc.untouched()
