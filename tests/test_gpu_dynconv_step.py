"""The DynamicConv step kernel (csrc/decode.hip: dynconv_step_kernel<R, NK, HAS_BACK, KB>) through the C ABI: every (C, R)
pair the launcher can select, every tap bucket at both edges, step sequences from a zeroed ring, an ancestor table, a large
step index, and the same steps through the registered device step counter - y element by element against the float64
reference and the bound of tests/decode_ref.py, the ring bit for bit.  Every operand and output is a
view inside a buffer of sentinels (tests/guarded.py); rows >= M of y do not exist, so a store of a dead row shows in the guards.
Run on the MI355X box:  python -m pytest tests/test_gpu_dynconv_step.py -m gpu -s   (-s prints the ratio c is pinned from and
the time of the whole file)"""
import time

import numpy as np
import pytest
import torch

import decode_ref as ref
from guarded import DEV, Guard

pytestmark = pytest.mark.gpu

BF16, I32 = torch.bfloat16, torch.int32
_RATIOS, _UNPINNED = {}, {}
COUNTER_BASE = 1 << 20                   # what the device counter holds beyond the step index (t_host is then negative)


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    _UNPINNED.clear()
    yield
    tell_amd.hip.call('tell_set_pos_step_ptr', None)          # the counter never stays registered
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
    print('\ntests/test_gpu_dynconv_step.py: %.1f s' % (time.time() - t0))


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def bits(t):
    return t.contiguous().view(torch.int16)


def check(got, r, gam, tag):
    got, want, S = ref.np64(got), r['y'], r['S_y']
    assert np.isfinite(got).all(), tag
    rt = ref.ratio(got, want, S, 'bfloat16', gam)
    _RATIOS['dcs_y'] = max(_RATIOS.get('dcs_y', 0.0), rt)
    if 'dcs_y' not in ref.C:
        _UNPINNED['dcs_y'] = max(_UNPINNED.get('dcs_y', 0.0), rt)
        return rt
    err, b = np.abs(got - want), ref.bound('dcs_y', want, S, 'bfloat16', gam)
    bad = err > b
    assert not bad.any(), 'dcs_y %s: %d of %d outside the bound, worst error %.3g at bound %.3g (ratio %.3f, c = %g)' % (
        tag, bad.sum(), bad.size, err[bad].max(), b[bad][err[bad].argmax()], rt, ref.C['dcs_y'])
    return rt


@pytest.mark.parametrize('counter', ['host', 'device'])
@pytest.mark.parametrize('case', ref.DCS, ids=[c['id'] for c in ref.DCS])
def test_dynconv_step(case, counter):
    from tell_amd import hip
    Cc, H, M, K = case['C'], case['H'], case['M'], case['K']
    assert ref.dynconv_rule(M, H) == case['R']
    x, want = ref.dcs_inputs(case), ref.dcs_run(case)
    base = dev(x['base'], BF16).to(DEV)
    wt = Guard((H * K, Cc), BF16, fill=dev(x['wt'], BF16))
    ring = Guard((K, M, Cc), BF16, fill=torch.zeros(K, M, Cc))
    back = Guard((K - 1, M), I32, fill=x['back'])
    xg = Guard((M, Cc), BF16, fill=base)
    expect = torch.zeros(K, M, Cc, dtype=BF16, device=DEV)
    word = torch.zeros(1, dtype=I32, device=DEV)
    if counter == 'device':
        hip.call('tell_set_pos_step_ptr', word)
    worst = 0.0
    for i, ((t, hb), perm, r) in enumerate(zip(ref.dcs_steps(case), x['perms'], want)):
        xg.t.copy_(base[torch.from_numpy(perm).to(DEV)])
        t_host = t
        if counter == 'device':
            word.fill_(COUNTER_BASE + t)
            t_host = -COUNTER_BASE
        expect[t % K] = xg.t
        ys = []
        for _ in range(2):                                    # (the plane a step writes is the one plane it does not read)
            y = Guard((M, Cc), BF16)
            hip.call('tell_dynconv_step', xg.t, ring.t, wt.t, y.t, M, Cc, H, K, t_host, back.t if hb else None)
            torch.cuda.synchronize()
            assert xg.intact() and ring.intact() and wt.intact() and back.intact() and y.intact(), \
                '%s step %d: a store outside a view' % (case['id'], i)
            assert torch.equal(bits(ring.t), bits(expect)), '%s step %d (t = %d): the ring' % (case['id'], i, t)
            ys.append(y)
        assert torch.equal(bits(ys[0].t), bits(ys[1].t)), '%s step %d: the second launch differs' % (case['id'], i)
        worst = max(worst, check(ys[0].t, r, ref.dcs_gamma(r, Cc, K), '%s %s step %d (t = %d)' % (case['id'], counter, i, t)))
    print('ratio %-12s %-44s %.6f' % ('dcs_y', '%s %s' % (case['id'], counter), worst))
    assert not _UNPINNED, 'constant not pinned yet, largest ratio of this case: dcs_y %.6f' % _UNPINNED['dcs_y']


def test_refused_calls_launch_nothing():
    """K = 1, K = 33, C = 768, and a negative step index without a registered counter"""
    from tell_amd import hip
    M = 4
    big = [Guard((33 * M * 2048,), BF16) for _ in range(4)]
    x, ring, wt, y = (g.t for g in big)

    def refused(Cc=1024, K=3, t=0):
        try:
            return hip.call_rc('tell_dynconv_step', x, ring, wt, y, M, Cc, Cc // 64, K, t, None)
        except RuntimeError as err:
            assert 'tell_dynconv_step' in str(err)
            return -1
    assert refused(K=1) != 0 and refused(K=33) != 0 and refused(Cc=768) != 0 and refused(t=-1) != 0
    torch.cuda.synchronize()
    assert all(g.untouched() for g in big)
