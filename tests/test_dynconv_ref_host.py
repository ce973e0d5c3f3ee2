"""Host checks of tests/dynconv_ref.py, the float64 DynamicConv reference and the element-wise bounds that
tests/test_gpu_dynconv.py holds the kernels to: the reference reproduces what the REFERENCE project produced (golden
fixtures), a float32 emulation of the kernels' arithmetic sits inside the bounds at c = 1 on every grid shape, and the
bounds are tight enough to throw out the classic index mistakes (a dropped tap, a dropped source row, a DropConnect
factor missing or applied at the wrong place)."""
import numpy as np
import pytest
import torch

import dynconv_ref as ref

DTYPES = [torch.float32, torch.bfloat16]
P = [0.0, 0.1]


def _name(dtype):
    return str(dtype).split('.')[-1]


def _round(a, dtype):
    """float32 array -> values as stored in `dtype`, float64"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).double().numpy()


@pytest.mark.parametrize('K,T', [(3, 6), (7, 4), (31, 12), (15, 40)])
def test_reference_reproduces_the_golden_fixtures(golden, K, T):
    import seeded
    fx = golden('dynconv_K%d_T%d' % (K, T))
    W = ref.np64(fx['sd']['weight_linear.weight'])
    x, gy = ref.np64(fx['in']['x']), ref.np64(fx['in']['gy'])
    H, C = 4, x.shape[-1]
    y, A, w = ref.forward(x, x @ W.T, H, K)
    dl, dx, S_dl, S_dx = ref.backward(x, gy, w)
    xf, n = x.reshape(-1, C), x.shape[0] * x.shape[1]
    got = {'y': y, 'gx': dx + dl @ W, 'g_weight': dl.reshape(-1, H * K).T @ xf}
    # The stored values are fp32 results of fp32 arithmetic: rtol 1e-5 of the value, plus the absolute error of a sum
    # of n terms in fp32, n 2^-24 sum|terms| - an element that is small because its terms cancel is no more exact
    # than its terms (pure rtol fails on 0.6 % of y, by at most 6e-8).
    err = {'y': (K + 8) * ref.EPS * A, 'gx': (K + 8 + H * K) * ref.EPS * (S_dx + S_dl @ np.abs(W)),
           'g_weight': (n + K + C) * ref.EPS * (S_dl.reshape(-1, H * K).T @ np.abs(xf))}
    for key, g in got.items():
        e = err[key]
        if key in fx.get('out', {}):
            want = ref.np64(fx['out'][key])
        else:
            want, g, e = ref.np64(fx['sub'][key]), seeded.subsample(g), seeded.subsample(e)
        assert g.shape == want.shape, key
        assert (np.abs(g - want) <= 1e-5 * np.abs(want) + e).all(), (key, np.abs(g - want).max())


def emulate(x, lg, dy, H, K, keep, dtype):
    """the kernels' arithmetic in float32: max-subtracted exp, sequential sums, one rounding to the stored type"""
    f = np.float32
    T, B, C = x.shape
    Rw = C // H
    lgr = lg.astype(f).reshape(T, B, H, K)
    e = np.exp(lgr - lgr.max(-1, keepdims=True)).astype(f)
    w = (e / np.cumsum(e, -1, dtype=f)[..., -1:]).astype(f)
    kp = np.ones_like(w) if keep is None else keep.astype(f)
    wd = (w * kp).astype(f)
    xp = ref._padded(x, H, K).astype(f)
    dyr = dy.astype(f).reshape(T, B, H, Rw)
    y = np.zeros((T, B, H, Rw), f)
    dw = np.zeros_like(w)
    for k in range(K):
        y = (y + wd[..., k, None] * xp[k:k + T]).astype(f)
        dw[..., k] = np.cumsum(dyr * xp[k:k + T], -1, dtype=f)[..., -1]
    dw = (dw * kp).astype(f)
    dot = np.cumsum(w * dw, -1, dtype=f)[..., -1:]
    dl = (w * (dw - dot)).astype(f)
    dx = np.zeros((T, B, H, Rw), f)
    for j in range(min(K, T)):
        dx[:T - j] = (dx[:T - j] + (w[j:, :, :, K - 1 - j, None] * kp[j:, :, :, K - 1 - j, None]) * dyr[j:]).astype(f)
    return (_round(y.reshape(T, B, C), dtype), w.astype(np.float64), _round(dl.reshape(T, B, H * K), dtype),
            _round(dx.reshape(T, B, C), dtype))


_CASES = {}


def case(shape, dtype, p):
    """inputs and float64 reference of one grid shape, computed once"""
    key = (shape, dtype, p)
    if key not in _CASES:
        T, B, H, K, Rw = shape
        x, lg, dy, _ = (ref.np64(t) for t in ref.case_inputs(T, B, H, K, Rw, dtype))
        keep = ref.keep_factors(ref.SEED, ref.SALT, T, B, H, K, p)
        y, A, w = ref.forward(x, lg, H, K, keep)
        dl, dx, S_dl, S_dx = ref.backward(x, dy, w, keep)
        _CASES[key] = dict(x=x, lg=lg, dy=dy, keep=keep, y=y, A=A, w=w, dl=dl, dx=dx, S_dl=S_dl, S_dx=S_dx,
                           D=ref.logit_spread(lg, H, K))
    return _CASES[key]


@pytest.mark.parametrize('p', P)
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@pytest.mark.parametrize('shape', ref.GRID, ids=str)
def test_float32_emulation_inside_the_bounds_at_c_1(shape, dtype, p):
    T, B, H, K, Rw = shape
    c = case(shape, dtype, p)
    n = _name(dtype)
    y, w, dl, dx = emulate(c['x'], c['lg'], c['dy'], H, K, c['keep'], dtype)
    assert (np.abs(y - c['y']) <= ref.bound('y', c['y'], c['A'], n, ref.gamma('y', K, Rw, c['D']), c=1)).all()
    assert (np.abs(w - c['w']) <= ref.bound('taps', c['w'], c['w'], 'float32', ref.gamma('taps', K, Rw, c['D']), c=1)).all()
    # backward on the emulation's own taps, as the GPU tests do with the kernel's
    rdl, rdx, S_dl, S_dx = ref.backward(c['x'], c['dy'], w, c['keep'])
    assert (np.abs(dl - rdl) <= ref.bound('dlogits', rdl, S_dl, n, ref.gamma('dlogits', K, Rw), c=1)).all()
    assert (np.abs(dx - rdx) <= ref.bound('dx', rdx, S_dx, n, ref.gamma('dx', K, Rw), c=1)).all()


R64_T_GE_K = [s for s in ref.GRID if s[4] == 64 and s[0] >= s[3]]


@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
@pytest.mark.parametrize('shape', R64_T_GE_K, ids=str)
@pytest.mark.parametrize('mutant', ref.MUTANTS)
def test_bounds_throw_out_the_mutants(mutant, shape, dtype):
    """more than half of the outputs a mutant changes leave the bound (pinned c), after rounding to the stored type.
    The two DropConnect mutants change nothing at p = 0, so they run at p = 0.1 only; the index mutants at both."""
    T, B, H, K, Rw = shape
    n = _name(dtype)
    for p in ([0.1] if mutant in ('dx_no_keep', 'keep_late') else P):
        c = case(shape, dtype, p)
        if mutant == 'k_lo':
            out, good, S = 'y', c['y'], c['A']
            bad = ref.forward(c['x'], c['lg'], H, K, c['keep'], mutant=mutant)[0]
        else:
            out = 'dlogits' if mutant == 'keep_late' else 'dx'
            good, S = (c['dl'], c['S_dl']) if out == 'dlogits' else (c['dx'], c['S_dx'])
            bdl, bdx, _, _ = ref.backward(c['x'], c['dy'], c['w'], c['keep'], mutant=mutant)
            bad = bdl if out == 'dlogits' else bdx
        # (a row whose keeps are all equal gives the same dlogits under 'keep_late' up to float64 rounding: not affected)
        affected = np.abs(bad - good) > 2.0 ** -40 * S
        if not affected.any():                 # K = 1: the softmax backward of a single tap is zero either way
            assert K == 1 and mutant == 'keep_late'
            continue
        stored = _round(bad, dtype)
        outside = np.abs(stored - good) > ref.bound(out, good, S, n, ref.gamma(out, K, Rw, c['D']))
        frac = (outside & affected).sum() / affected.sum()
        print('%s %s %s p=%.1f: %.1f %% of %d affected outputs leave the bound' % (mutant, shape, n, p, 100 * frac,
                                                                                 affected.sum()))
        assert frac > 0.5, frac
