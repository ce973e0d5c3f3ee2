"""The narrow launch form of the step's bandwidth-bound kernels (option bw_wgs): BertAdam in all its
entry points and template variants, its norm pass, the RoBERTa layer mix forward and backward and the two multi weight-norm
launches write, with bw_wgs = 1 / 8 / 13 / 64, bit for bit what they write with bw_wgs = 0.  Nothing here has a tolerance:
a narrow workgroup walks the wide launch's 256-thread blocks, so every reduction sees the same elements in the same order.
The wide launch itself is held to float64 by the kernels' own test files (BertAdam: tests/test_gpu_optim.py; mix and weight
norm: tests/test_gpu_small_reduce.py).
Run on the MI355X box:  python -m pytest tests/test_gpu_narrow_launch.py -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import optim_ema_ref as ema
import optim_groups_ref as grp
import optim_ref as ref
from guarded import DEV, Guard
from test_gpu_optim import BF16, F32, VARIANTS, Step
from test_gpu_optim_ema import EmaStep
from test_gpu_optim_groups import GroupStep

pytestmark = pytest.mark.gpu

WGS = (1, 8, 13, 64)
LAYOUTS = (0, 4, 9)                 # optim_ref.EXACT_LAYOUTS of 1, 5 and 13 chunks
DECAY, WARM = 0.9, 10.0
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


def as_bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()]) if t.is_floating_point() else t


def same_buffers(a, b, tag):
    """two lists of Guards: every allocation equal bit for bit, guard bands included"""
    assert len(a) == len(b) and len(a) > 0, tag
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(as_bits(x.buf), as_bits(y.buf)), '%s: buffer %d differs' % (tag, i)
        assert x.intact() and y.intact(), '%s: buffer %d written outside its view' % (tag, i)


# ---------------------------------------------------------------- BertAdam and its norm pass
def adam_case(k):
    """layout k of the exact lane with dense random state: every chunk partial and every norm is a sum whose order shows"""
    if k not in _DATA:
        lay = ref.Layout(ref.EXACT_LAYOUTS[k][0])
        rng = np.random.default_rng(100 + k)
        dense = lambda scale: np.where(lay.real, rng.standard_normal(lay.total) * scale, 0.0).astype(np.float32)   # noqa: E731
        p, g, m = dense(0.5), dense(0.3), dense(0.01)
        v = (dense(0.01) ** 2).astype(np.float32)
        _DATA[k] = dict(lay=lay, p=p, g=g, m=m, v=v, e=ema.make_e(p, lay.real, k),
                        wire=ref.bf16_rne(g), keep=(np.arange(lay.n_tensors) % 2).astype(np.int32))
    return _DATA[k]


def run_adam(entry, d, wgs, var, grid, wire=False, skip=(0, 4)):
    """one call of `entry` on fresh guarded copies with bw_wgs = wgs; max_norm 0.05 clips (the norm pass runs)"""
    from tell_amd import hip
    lay = d['lay']
    kw = dict(shadow=True, wire=d['wire'] if wire else None, keep=d['keep'], step=3, skip=skip)
    run = dict(grad_scale=0.5, zero_grad=1, var=var, grid=grid)
    with hip.options(bw_wgs=wgs):
        if entry == 'step2':
            s = Step(lay, d['p'], d['g'], d['m'], d['v'], **kw)
            s.run(ref.HP, max_norm=0.05, lr_base=1e-2, warmup=0.2, t_total=10.0, **run)
        elif entry == 'ema':
            s = EmaStep(lay, d['p'], d['g'], d['m'], d['v'], d['e'], **kw)
            s.run_ema(ref.HP, DECAY, WARM, max_norm=0.05, lr_base=1e-2, warmup=0.2, t_total=10.0, **run)
        else:                                        # two groups, tensors alternating; with and without the average
            tg = [t % 2 for t in range(lay.n_tensors)]
            s = GroupStep(lay, d['p'], d['g'], d['m'], d['v'], grp.ROWS[:2], tg, e=d['e'] if entry == 'groups_ema' else None,
                          **kw)
            s.run_groups(**run)
    return s


@pytest.mark.parametrize('entry', ['step2', 'ema', 'groups', 'groups_ema'])
@pytest.mark.parametrize('var', sorted(VARIANTS))
def test_bertadam_and_norm_pass_are_the_wide_launch_bit_for_bit(var, entry):
    """every buffer of the call (masters, m, v, shadow, gradient, average, chunk partials, norms, lr, counters) on the 1-,
    5- and 13-chunk layouts, with the default grid and with 3 blocks (several trips per block), fp32 and wire gradient"""
    for k in LAYOUTS:
        d = adam_case(k)
        for grid in (None, 3):
            for wire in (False, True):
                wide = run_adam(entry, d, 0, var, grid, wire)
                assert int(wide.step.t.item()) == 4 and wide.intact()          # (an update was applied)
                for wgs in WGS:
                    narrow = run_adam(entry, d, wgs, var, grid, wire)
                    same_buffers(narrow.guards(), wide.guards(), '%s layout %d var %d grid %s wire %d bw_wgs %d'
                                 % (entry, k, var, grid, wire, wgs))


@pytest.mark.parametrize('entry', ['step2', 'groups_ema'])
def test_bertadam_skipped_step(entry):
    """skip[0] != 0: nothing but the gradient's zeroing and the skip count, in both forms alike"""
    d = adam_case(9)
    wide = run_adam(entry, d, 0, None, None, skip=(1, 4))
    assert tuple(wide.skip.t.tolist()) == (1, 5) and int(wide.step.t.item()) == 3
    for wgs in WGS:
        same_buffers(run_adam(entry, d, wgs, None, None, skip=(1, 4)).guards(), wide.guards(), '%s bw_wgs %d' % (entry, wgs))


def test_norm_pass_second_trip():
    """4096 x 4 + 4 chunks: the wide norm pass takes a second trip in its first block only; in the narrow form the other
    quarters of that workgroup run the trip empty to keep its barriers whole"""
    from tell_amd import hip
    big = ref.Layout([16385 * ref.CHUNK - 1, 3 * ref.CHUNK - 5])
    real = torch.from_numpy(big.real).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(11)
    g = torch.randn(big.total, device=DEV, generator=gen) * 0.05 * real
    p = torch.randn(big.total, device=DEV, generator=gen) * 0.5 * real
    m, v = p * 0.01, (p * 0.01) ** 2
    out = {}
    for wgs in (0, 1, 64):
        s = Step(big, p, g, m, v, step=3, skip=(0, 0), device_arrays=True)
        with hip.options(bw_wgs=wgs):
            s.run(ref.HP, 1.0, 0.1, 1, 1e-2, 0.2, 10.0)
        assert s.intact()
        out[wgs] = [as_bits(x.t).clone() for x in (s.partial, s.norms, s.param, s.m, s.v, s.shadow, s.grad)]
        del s
    assert bool((out[0][0].view(F32) > 0).all())
    for wgs in (1, 64):
        for i, (x, y) in enumerate(zip(out[wgs], out[0])):
            assert torch.equal(x, y), (wgs, i)


# ---------------------------------------------------------------- RoBERTa layer mix
MIX_L = 25
MIX_N = (2047, 2048, 5 * 2048 + 8 * 37)   # one element short of a 16-byte vector (the element-wise kernels); exactly one
#                                           256-thread block of 8-element vectors; five blocks and a ragged sixth


def mix_inputs(n, dtype):
    key = ('mix', n, dtype)
    if key not in _DATA:
        gen = torch.Generator().manual_seed(n)
        _DATA[key] = (torch.randn(MIX_L, n, generator=gen).to(dtype), torch.randn(n, generator=gen).to(dtype),
                      torch.randn(MIX_L, generator=gen))
    return _DATA[key]


@pytest.mark.parametrize('dtype', [BF16, F32])
@pytest.mark.parametrize('n', MIX_N)
def test_mix_forward_and_backward_are_the_wide_launch_bit_for_bit(n, dtype):
    from tell_amd import hip
    H0, d0, w0 = mix_inputs(n, dtype)
    code = hip.dt(dtype)

    def run(wgs, nb):
        H, dout, w = Guard((MIX_L, n), dtype, fill=H0), Guard((n,), dtype, fill=d0), Guard((MIX_L,), F32, fill=w0)
        out, partial = Guard((n,), dtype), Guard((nb, MIX_L), F32)
        with hip.options(bw_wgs=wgs):
            hip.call('tell_mix_fwd', H.t, w.t, MIX_L, n, out.t, code)
            hip.call('tell_mix_bwd', H.t, dout.t, MIX_L, n, partial.t, nb, code)
        torch.cuda.synchronize()
        return [H, dout, w, out, partial]

    for nb in (1, 3, 7):                         # 7 blocks: more than the five-and-a-bit of work; 3: several trips per block
        wide = run(0, nb)
        assert not bool((wide[3].t == wide[3].sentinel).any())
        for wgs in WGS:
            same_buffers(run(wgs, nb), wide, 'n %d %s blocks %d bw_wgs %d' % (n, dtype, nb, wgs))


# ---------------------------------------------------------------- weight norm over many tensors
WN_SHAPES = ((1, 8), (7, 1024), (64, 4096))


def wn_inputs():
    if 'wn' not in _DATA:
        gen = torch.Generator().manual_seed(5)
        _DATA['wn'] = [(torch.randn(r, generator=gen), torch.randn(r, c, generator=gen), torch.randn(r, c, generator=gen),
                        torch.randn(r, generator=gen), torch.randn(r, c, generator=gen)) for r, c in WN_SHAPES]
    return _DATA['wn']


def _ptrs(guards):
    return (ctypes.c_void_p * len(guards))(*[x.t.data_ptr() for x in guards])


def _ints(values):
    return (ctypes.c_int * len(values))(*values)


@pytest.mark.parametrize('out_dtype', [BF16, F32])
def test_wn_weight_multi_is_the_wide_launch_bit_for_bit(out_dtype):
    from tell_amd import hip
    rows, cols = _ints([r for r, _ in WN_SHAPES]), _ints([c for _, c in WN_SHAPES])

    def run(wgs):
        g = [Guard((r,), F32, fill=x[0]) for (r, c), x in zip(WN_SHAPES, wn_inputs())]
        v = [Guard((r, c), F32, fill=x[1]) for (r, c), x in zip(WN_SHAPES, wn_inputs())]
        w = [Guard((r, c), out_dtype) for r, c in WN_SHAPES]
        norms = [Guard((r,), F32) for r, _ in WN_SHAPES]
        with hip.options(bw_wgs=wgs):
            hip.call('tell_wn_weight_multi', len(WN_SHAPES), _ptrs(g), _ptrs(v), _ptrs(w), _ptrs(norms), rows, cols,
                     hip.dt(out_dtype))
        torch.cuda.synchronize()
        return g + v + w + norms

    wide = run(0)
    assert all(bool((x.t > 0).all()) for x in wide[-len(WN_SHAPES):])
    for wgs in WGS:
        same_buffers(run(wgs), wide, '%s bw_wgs %d' % (out_dtype, wgs))


def test_wn_backward_multi_is_the_wide_launch_bit_for_bit():
    """dg / dv stored for tensors 0 and 2, accumulated into what they held for tensor 1"""
    from tell_amd import hip
    rows, cols, store = _ints([r for r, _ in WN_SHAPES]), _ints([c for _, c in WN_SHAPES]), _ints([1, 0, 1])

    def run(wgs):
        mk = lambda i, shape: [Guard(shape(r, c), F32, fill=x[i]) for (r, c), x in zip(WN_SHAPES, wn_inputs())]   # noqa: E731
        g, v, dW = mk(0, lambda r, c: (r,)), mk(1, lambda r, c: (r, c)), mk(2, lambda r, c: (r, c))
        dg, dv = mk(3, lambda r, c: (r,)), mk(4, lambda r, c: (r, c))
        norms = [Guard((r,), F32, fill=x[1].norm(dim=1)) for (r, c), x in zip(WN_SHAPES, wn_inputs())]
        with hip.options(bw_wgs=wgs):
            hip.call('tell_wn_backward_multi2', len(WN_SHAPES), _ptrs(dW), _ptrs(g), _ptrs(v), _ptrs(norms), rows, cols,
                     _ptrs(dg), _ptrs(dv), store)
        torch.cuda.synchronize()
        return g + v + dW + norms + dg + dv

    wide = run(0)
    for wgs in WGS:
        same_buffers(run(wgs), wide, 'bw_wgs %d' % wgs)
