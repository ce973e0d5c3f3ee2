"""DynamicConv training kernels (csrc/dynconv.hip) through the C ABI, every launch path of tell_dynconv_fwd /
tell_dynconv_bwd and the fused tell_dynconv_block_fwd, element by element against the float64 reference and the bounds
of tests/dynconv_ref.py.  Every output is a view inside a buffer of sentinels, so a store
outside the tensor shows without anything running out of range.
Run on the MI355X box:  python -m pytest tests/test_gpu_dynconv.py -m gpu   (-s prints the error ratios c is pinned from)"""
import numpy as np
import pytest
import torch

import dynconv_ref as ref

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16]
P = [0.0, 0.1]
SENTINEL = -65536.0          # exact in both types, far from anything the kernels produce
PAD = 64                     # elements on each side of a view: keeps the view's 16-byte alignment
SEED, SALT = ref.SEED, ref.SALT

LDS_SHAPE = (33, 2, 3, 31, 64)       # LDS-tiled forward and backward, second pass of the tap staging
ROW_SHAPE = (41, 3, 3, 33, 64)       # wave-per-row forward and backward (K > 32), 369 waves
LDS_FWD_SHAPE = (65, 2, 3, 31, 64)   # LDS-tiled forward, wave-per-row backward

_RATIOS = {}


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    for k in sorted(_RATIOS):
        print('\nlargest (|got - ref| - u_out |ref|) / (gamma 2^-24 S)  %-22s %.4f' % (k, _RATIOS[k]))


def _name(dtype):
    return str(dtype).split('.')[-1]


class Guarded:
    """a tensor that is a view inside a larger allocation filled with SENTINEL; off: extra elements in front of the
    view (off = 1 takes the view off its 16-byte alignment)"""

    def __init__(self, shape, dtype, off=0, fill=None):
        self.n = int(np.prod(shape))
        self.lo = PAD + off
        self.buf = torch.full((self.n + 2 * PAD + off,), SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[self.lo:self.lo + self.n].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.lo + self.n:] == SENTINEL).all())


def fwd(shape, dtype, p, x, lg, lds=True, off=0, with_taps=True, salt=SALT):
    """tell_dynconv_fwd on CPU tensors x, lg (already rounded to dtype) -> y, taps (device tensors; taps None if not
    asked for); the guard bands are checked here"""
    from tell_amd import hip
    T, B, H, K, R = shape
    xg = Guarded(x.shape, dtype, off, x)
    lgd = lg.to(DEV)
    y = Guarded((T, B, H * R), dtype, off)
    taps = Guarded((T, B, H, K), torch.float32)
    with hip.options(dynconv_lds=int(lds)):
        hip.call('tell_dynconv_fwd', xg.t, lgd, y.t, taps.t if with_taps else None, T, B, H, K, R, p, SEED, salt,
                 hip.dt(dtype))
    torch.cuda.synchronize()
    assert y.intact() and taps.intact() and xg.intact(), 'store outside y / taps'
    if not with_taps:
        assert bool((taps.t == SENTINEL).all())
    return y.t, (taps.t if with_taps else None)


def bwd(shape, dtype, p, x, dy, taps, lds=True, off=0, dx0=None, salt=SALT):
    """tell_dynconv_bwd -> dlogits, dx (device tensors); dx0 given: dx preset to it and dx_accumulate = 1"""
    from tell_amd import hip
    T, B, H, K, R = shape
    xg = Guarded(x.shape, dtype, off, x)
    dyg = Guarded(dy.shape, dtype, off, dy)
    dl = Guarded((T, B, H * K), dtype)
    dx = Guarded((T, B, H * R), dtype, off, dx0)
    tg = Guarded((T, B, H, K), torch.float32, 0, taps)
    with hip.options(dynconv_lds=int(lds)):
        hip.call('tell_dynconv_bwd', xg.t, dyg.t, tg.t, dx.t, int(dx0 is not None), dl.t, T, B, H, K, R, p, SEED, salt,
                 hip.dt(dtype))
    torch.cuda.synchronize()
    assert dl.intact() and dx.intact() and xg.intact() and dyg.intact() and tg.intact(), 'store outside dlogits / dx'
    return dl.t, dx.t


def check(out, got, want, S, stored, gam, tag, group='grid'):
    """element-wise bound of dynconv_ref; the ratio c is pinned from is recorded and printed"""
    got = ref.np64(got).reshape(want.shape)
    assert np.isfinite(got).all(), out
    r = ref.ratio(got, want, S, stored, gam)
    _RATIOS[group + ' ' + out] = max(_RATIOS.get(group + ' ' + out, 0.0), r)
    print('ratio %-8s %-44s %.4f' % (out, tag, r))
    err, b = np.abs(got - want), ref.bound(out, want, S, stored, gam)
    bad = err > b
    assert not bad.any(), '%s %s: %d of %d outside the bound, worst error %.3g at bound %.3g (ratio %.3f, c = %g)' % (
        out, tag, bad.sum(), bad.size, err[bad].max(), b[bad][err[bad].argmax()], r, ref.C[out])


_FWD_REF = {}


def case(shape, dtype, p, scale=1.0):
    """inputs and the float64 forward reference of a case, computed once and shared"""
    key = (shape, dtype, p, scale)
    if key not in _FWD_REF:
        T, B, H, K, R = shape
        x, lg, dy, dx0 = ref.case_inputs(T, B, H, K, R, dtype, scale)
        keep = ref.keep_factors(SEED, SALT, T, B, H, K, p)
        y, A, w = ref.forward(ref.np64(x), ref.np64(lg), H, K, keep)
        _FWD_REF[key] = dict(x=x, lg=lg, dy=dy, dx0=dx0, keep=keep, y=y, A=A, w=w, D=ref.logit_spread(ref.np64(lg), H, K))
    return _FWD_REF[key]


def run_and_check(shape, dtype, p, lds=True, off=0, accumulate=False, scale=1.0, group='grid'):
    T, B, H, K, R = shape
    c = case(shape, dtype, p, scale)
    n = _name(dtype)
    tag = '%s %s p=%.1f%s%s%s' % (shape, n, p, '' if lds else ' lds=0', ' off=%d' % off if off else '',
                                  ' acc' if accumulate else '')
    y, taps = fwd(shape, dtype, p, c['x'], c['lg'], lds, off)
    check('y', y, c['y'], c['A'], n, ref.gamma('y', K, R, c['D']), tag, group)
    check('taps', taps, c['w'], c['w'], 'float32', ref.gamma('taps', K, R, c['D']), tag, group)
    dx0 = c['dx0'] if accumulate else None
    dl, dx = bwd(shape, dtype, p, c['x'], c['dy'], taps, lds, off, dx0)
    # backward judged on the kernel's own fp32 taps
    rdl, rdx, S_dl, S_dx = ref.backward(ref.np64(c['x']), ref.np64(c['dy']), ref.np64(taps), c['keep'],
                                        None if dx0 is None else ref.np64(dx0))
    check('dlogits', dl, rdl, S_dl, n, ref.gamma('dlogits', K, R), tag, group)
    check('dx', dx, rdx, S_dx, n, ref.gamma('dx', K, R), tag, group)
    return dict(y=y, taps=taps, dl=dl, dx=dx)


# ---------------------------------------------------------------- 3.1 the grid
@pytest.mark.parametrize('p', P)
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@pytest.mark.parametrize('shape', ref.GRID, ids=str)
def test_grid_against_float64(shape, dtype, p):
    """whichever kernels the dispatchers pick for the shape: y, taps, dlogits, dx inside the bounds"""
    run_and_check(shape, dtype, p)


@pytest.mark.parametrize('p', P)
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@pytest.mark.parametrize('shape', ref.GRID_LDS + ref.GRID_LDS_FWD, ids=str)
def test_forced_wave_per_row_path(shape, dtype, p):
    """dynconv_lds = 0 sends the shapes of the LDS-tiled kernels through the wave-per-row kernels: same bounds, taps
    that agree with the tiled path within the taps bound, DropConnect zeros at the same places"""
    T, B, H, K, R = shape
    row = run_and_check(shape, dtype, p, lds=False)
    c = case(shape, dtype, p)
    y, taps = fwd(shape, dtype, p, c['x'], c['lg'], lds=True)
    dl, dx = bwd(shape, dtype, p, c['x'], c['dy'], taps, lds=True)
    diff = np.abs(ref.np64(taps) - ref.np64(row['taps']))
    assert (diff <= ref.bound('taps', c['w'], c['w'], 'float32', ref.gamma('taps', K, R, c['D']))).all()
    assert torch.equal(y == 0, row['y'] == 0) and torch.equal(dx == 0, row['dx'] == 0)
    if K == 1 and p > 0:                     # one tap: y is zero exactly where that tap was dropped
        dropped = torch.from_numpy(c['keep'] == 0).to(DEV).view(T, B, H, 1).expand(T, B, H, R).reshape(T, B, H * R)
        x0 = c['x'].to(DEV) == 0
        for yy in (y, row['y']):
            assert torch.equal((yy == 0) | x0, dropped | x0)


# ---------------------------------------------------------------- 3.2 corners of the ABI
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@pytest.mark.parametrize('shape', [LDS_SHAPE, LDS_FWD_SHAPE], ids=['lds', 'wave_per_row'])
def test_dx_accumulate(shape, dtype):
    """dx_accumulate = 1 on both backward paths: dx preset to random values, reference dx0 + the sum"""
    run_and_check(shape, dtype, 0.1, accumulate=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@pytest.mark.parametrize('shape', [LDS_SHAPE, ROW_SHAPE], ids=['lds', 'wave_per_row'])
def test_inference_forward_without_taps(shape, dtype):
    """taps = NULL: the same y, bit for bit, and nothing written where the taps would have gone"""
    c = case(shape, dtype, 0.1)
    y1, _ = fwd(shape, dtype, 0.1, c['x'], c['lg'])
    y0, none = fwd(shape, dtype, 0.1, c['x'], c['lg'], with_taps=False)
    assert none is None and torch.equal(y0, y1)


@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@pytest.mark.parametrize('shape', [LDS_SHAPE, (64, 2, 3, 32, 64)], ids=str)
def test_buffers_off_16_byte_alignment(shape, dtype):
    """x, y, dy, dx one element into a larger allocation: the tiled kernels' 16-byte loads do not apply, the
    dispatchers take the wave-per-row kernels, and the results meet the same bounds"""
    run_and_check(shape, dtype, 0.1, off=1)


def test_empty_problem_writes_nothing():
    from tell_amd import hip
    for T, B, H in ((0, 2, 3), (4, 0, 3), (4, 2, 0)):
        bufs = [Guarded((8,), torch.float32) for _ in range(7)]
        for g in bufs:
            g.t.fill_(SENTINEL)
        x, lg, y, taps, dy, dx, dl = (g.t for g in bufs)
        hip.call('tell_dynconv_fwd', x, lg, y, taps, T, B, H, 3, 64, 0.1, SEED, SALT, hip.F32)
        hip.call('tell_dynconv_bwd', x, dy, taps, dx, 0, dl, T, B, H, 3, 64, 0.1, SEED, SALT, hip.F32)
        torch.cuda.synchronize()
        assert all(bool((g.buf == SENTINEL).all()) for g in bufs)


@pytest.mark.parametrize('K,p', [(0, 0.1), (65, 0.1), (3, 1.0)])
def test_rejected_arguments_raise(K, p):
    from tell_amd import hip
    T, B, H, R = 2, 2, 2, 64
    bufs = [Guarded((T * B * H * 65,), torch.float32) for _ in range(7)]
    x, lg, y, taps, dy, dx, dl = (g.t for g in bufs)
    with pytest.raises(RuntimeError, match='dynconv'):
        hip.call('tell_dynconv_fwd', x, lg, y, taps, T, B, H, K, R, p, SEED, SALT, hip.F32)
    with pytest.raises(RuntimeError, match='dynconv'):
        hip.call('tell_dynconv_bwd', x, dy, taps, dx, 0, dl, T, B, H, K, R, p, SEED, SALT, hip.F32)
    torch.cuda.synchronize()
    assert all(bool((g.buf == SENTINEL).all()) for g in bufs)


# ---------------------------------------------------------------- 3.4 exact properties
EXACT = pytest.mark.parametrize('shape', [LDS_SHAPE, ROW_SHAPE], ids=['lds', 'wave_per_row'])


def _all(shape, dtype, p, x, lg, dy):
    y, taps = fwd(shape, dtype, p, x, lg)
    dl, dx = bwd(shape, dtype, p, x, dy, taps)
    return y, taps, dl, dx


@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@EXACT
def test_two_runs_are_bit_identical(shape, dtype):
    c = case(shape, dtype, 0.1)
    a = _all(shape, dtype, 0.1, c['x'], c['lg'], c['dy'])
    b = _all(shape, dtype, 0.1, c['x'], c['lg'], c['dy'])
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@EXACT
def test_causality(shape, dtype):
    """rows t >= t0 of x and the logits do not reach y[:t0], taps[:t0]; rows t < t0 of dy do not reach dx[t0:],
    dlogits[t0:]"""
    T, B, H, K, R = shape
    c = case(shape, dtype, 0.1)
    t0 = T // 2 + 1
    g = torch.Generator().manual_seed(5)
    x2, lg2, dy2 = c['x'].clone(), c['lg'].clone(), c['dy'].clone()
    x2[t0:] = torch.randn(x2[t0:].shape, generator=g).to(dtype)
    lg2[t0:] = torch.randn(lg2[t0:].shape, generator=g).to(dtype)
    dy2[:t0] = torch.randn(dy2[:t0].shape, generator=g).to(dtype)
    y, taps = fwd(shape, dtype, 0.1, c['x'], c['lg'])
    y2, taps2 = fwd(shape, dtype, 0.1, x2, lg2)
    assert torch.equal(y[:t0], y2[:t0]) and torch.equal(taps[:t0], taps2[:t0])
    assert not torch.equal(y[t0:], y2[t0:])
    dl, dx = bwd(shape, dtype, 0.1, c['x'], c['dy'], taps)
    dl2, dx2 = bwd(shape, dtype, 0.1, c['x'], dy2, taps)
    assert torch.equal(dx[t0:], dx2[t0:]) and torch.equal(dl[t0:], dl2[t0:])
    assert not torch.equal(dx[:t0], dx2[:t0])


@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@EXACT
def test_batch_columns_permute(shape, dtype):
    """p = 0: the batch columns do not see each other, so permuting them permutes every output"""
    T, B, H, K, R = shape
    c = case(shape, dtype, 0.0)
    perm = torch.tensor([(b + 1) % B for b in range(B)])
    a = _all(shape, dtype, 0.0, c['x'], c['lg'], c['dy'])
    b = _all(shape, dtype, 0.0, c['x'][:, perm].contiguous(), c['lg'][:, perm].contiguous(),
             c['dy'][:, perm].contiguous())
    assert all(torch.equal(u[:, perm.to(DEV)], v) for u, v in zip(a, b))


# ---------------------------------------------------------------- 3.5 softmax range
@pytest.mark.parametrize('p', P)
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@EXACT
def test_nearly_one_hot_taps(shape, dtype, p):
    """logits x 30: rows spread over D ~ 200, most taps underflow; finite and inside the bounds (gamma carries D)"""
    assert case(shape, dtype, p, 30.0)['D'] > 100
    run_and_check(shape, dtype, p, scale=30.0, group='range')


@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@EXACT
def test_minus_infinity_logits_give_an_exact_one_hot(shape, dtype):
    T, B, H, K, R = shape
    c = case(shape, dtype, 0.0)
    g = torch.Generator().manual_seed(6)
    hot = torch.randint(0, K, (T, B, H, 1), generator=g)
    lg = torch.full((T, B, H, K), float('-inf')).scatter_(3, hot, torch.randn(T, B, H, 1, generator=g)).to(dtype)
    y, taps = fwd(shape, dtype, 0.0, c['x'], lg.view(T, B, H * K))
    one_hot = torch.zeros(T, B, H, K).scatter_(3, hot, 1.0)
    assert torch.equal(taps.cpu(), one_hot)
    want = ref.forward(ref.np64(c['x']), None, H, K, None, taps=one_hot.double().numpy())[0]
    assert np.array_equal(ref.np64(y), want)              # y[t] is x[t - (K-1) + k], or 0 before the start


# ---------------------------------------------------------------- 3.6 the fused conv-block forward and its backward
@pytest.mark.parametrize('p', P)
@pytest.mark.parametrize('T,B,K', [(1, 1, 31), (32, 9, 31), (31, 8, 3), (32, 1, 1)])
def test_block_forward_then_backward(T, B, K, p):
    """tell_dynconv_block_fwd (E = 1024, H = 16, bf16), then tell_dynconv_bwd on the taps it wrote - the chain
    blocks.py runs in training.  gl bit-equal to tell_glu_fwd; taps against the float64 softmax of the float64 logits
    gl W^T with the error of an fp32 dot product of E terms in front of the softmax; y on the kernel's own taps."""
    from tell_amd import hip
    E, H, R = 1024, 16, 64
    shape = (T, B, H, K, R)
    g = torch.Generator().manual_seed(T * 100 + K)
    h1 = torch.randn(T * B, 2 * E, generator=g).bfloat16().to(DEV)
    wt = (torch.randn(H * K, E, generator=g) * 0.05).bfloat16().to(DEV)
    dy = torch.randn(T, B, E, generator=g).bfloat16()
    gl = Guarded((T * B, E), torch.bfloat16)
    y = Guarded((T * B, E), torch.bfloat16)
    taps = Guarded((T, B, H, K), torch.float32)
    assert hip.call_rc('tell_dynconv_block_fwd', h1, wt, gl.t, y.t, taps.t, T, B, H, K, p, SEED, SALT) == 0
    torch.cuda.synchronize()
    assert gl.intact() and y.intact() and taps.intact()
    gl_ref = torch.empty_like(gl.t)
    hip.call('tell_glu_fwd', h1, gl_ref, T * B, E, hip.BF16)
    assert torch.equal(gl.t, gl_ref)
    tag = 'block T=%d B=%d K=%d p=%.1f' % (T, B, K, p)
    x64, w64 = ref.np64(gl.t).reshape(T, B, E), ref.np64(wt)
    lg64 = x64 @ w64.T
    w_ref, D = ref.softmax_taps(lg64, H, K), ref.logit_spread(lg64, H, K)
    mag = (np.abs(x64) @ np.abs(w64).T).reshape(T, B, H, K).max(-1, keepdims=True)
    c_t = ref.C['taps']
    got = ref.np64(taps.t)
    rel = 2 * c_t * (E + 8) * ref.EPS * mag + c_t * (K + 8 + D) * ref.EPS
    err = np.abs(got - w_ref)
    ok = rel * w_ref > 0
    r = float(((err - ref.EPS * w_ref - ref.TINY)[ok] / (rel * w_ref / c_t)[ok]).max())
    _RATIOS['block taps'] = max(_RATIOS.get('block taps', 0.0), r)
    print('ratio %-8s %-44s %.4f' % ('taps', tag, r))
    assert (err <= ref.EPS * w_ref + rel * w_ref + ref.TINY).all(), (err.max(), r)
    keep = ref.keep_factors(SEED, SALT, T, B, H, K, p)
    y_ref, A, _ = ref.forward(x64, None, H, K, keep, taps=got)
    check('y', y.t, y_ref, A, 'bfloat16', ref.gamma('y', K, R), tag, 'block')
    dl, dx = bwd(shape, torch.bfloat16, p, gl.t.view(T, B, E), dy, taps.t)
    rdl, rdx, S_dl, S_dx = ref.backward(x64, ref.np64(dy), got, keep)
    check('dlogits', dl, rdl, S_dl, 'bfloat16', ref.gamma('dlogits', K, R), tag, 'block')
    check('dx', dx, rdx, S_dx, 'bfloat16', ref.gamma('dx', K, R), tag, 'block')
