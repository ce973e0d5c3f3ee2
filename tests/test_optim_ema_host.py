"""CPU half of the moving average of the weights: tests/optim_ema_ref.py proved against exact
rational arithmetic and against its own MUTANTS, the declared ABI of the two new entry points, and the host wrapper
(training/optimizers.py) with hip.call recorded instead of run."""
import inspect
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

import optim_ema_ref as ema
import optim_ref as ref


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- the schedule
def test_decay_schedule_by_direct_formulas():
    assert ema.decay_at(0, 0.9, 10.0) == 0.1 and ema.decay_at(1, 0.9, 10.0) == 2.0 / 11.0
    assert ema.decay_at(9, 0.9, 10.0) == 10.0 / 19.0 and ema.decay_at(10, 0.9, 10.0) == 11.0 / 20.0
    d9 = float(np.float32(0.9))
    assert ema.decay_at(80, 0.9, 10.0) == d9 < 0.9 + 1e-7 and ema.decay_at(79, 0.9, 10.0) == 80.0 / 89.0 < d9
    assert ema.decay_at(10 ** 5, 0.9, 10.0) == d9 and ema.decay_at(10 ** 5, 0.9999, 10.0) == float(np.float32(0.9999))
    for n in ema.STEPS_N + (None,):
        assert ema.decay_at(n, 0.9, 0.0) == d9 and ema.decay_at(n, 0.9, -1.0) == d9       # no warm-up
    assert ema.decay_at(None, 0.9, 10.0) == d9                                             # no device counter
    assert ema.decay_at(0, 0.9, 0.5) == d9                          # (1 + n) / (warm + n) > 1 for warm < 1: the cap holds
    assert ema.omd_at(0, 0.5, 0.0) == np.float32(0.5) and ema.omd_at(3, 0.75, 0.0) == np.float32(0.25)
    assert ema.omd_at(0, 0.9, 10.0) == np.float32(0.9) and ema.omd_at(0, 0.9, 10.0).dtype == np.float32
    # 1 - d_t is rounded once, from the float64 difference - not computed in fp32
    assert ema.omd_at(None, 0.9, 0.0) == np.float32(1.0 - d9) != np.float32(0.1)
    ds = [ema.decay_at(n, 0.9999, 10.0) for n in range(0, 200000, 997)]
    assert all(a <= b for a, b in zip(ds, ds[1:])) and ds[0] == 0.1 and ds[-1] == float(np.float32(0.9999))


# ---------------------------------------------------------------- one rounding
def exact_fma32(a, b, c):
    """a * b + c in rational arithmetic, rounded to the nearest fp32, ties to even (finite, in range)"""
    x = Fraction(float(np.float32(a))) * Fraction(float(np.float32(b))) + Fraction(float(np.float32(c)))
    r = np.float32(float(x))                                   # within an ulp: look at it and both neighbours
    cand = sorted({float(r), float(np.nextafter(r, np.float32(np.inf))), float(np.nextafter(r, np.float32(-np.inf)))})
    best = min(cand, key=lambda y: (abs(Fraction(y) - x), int(np.float32(y).view(np.uint32)) & 1))
    return np.float32(best)


def test_fma32_rounds_once_on_the_double_rounding_trap():
    for e, p_new, omd, want, twice in ema.TRAPS:
        e32, p32, o32 = np.float32(e), np.float32(p_new), np.float32(omd)
        assert float(e32) == e and float(p32) == p_new and float(o32) == omd             # the inputs are fp32 numbers
        d = p32 - e32
        exact = exact_fma32(o32, d, e32)
        assert float(exact) == want != twice
        got = ema.ema_step(np.array([e32]), np.array([p32]), o32)
        assert got.dtype == np.float32 and float(got[0]) == want
        naive = ref._fma(o32, d, e32)                          # product and sum in float64, then fp32: two roundings
        assert float(naive) == twice, 'optim_ref._fma rounds once here - the trap is not one'
        # the float64 sum really is the fp32 tie
        s = float(o32) * float(d) + float(e32)
        lo, hi = sorted((want, twice))
        assert s == (lo + hi) / 2


def test_fma32_equals_rational_arithmetic_on_random_operands():
    rng = np.random.default_rng(11)
    n = 3000
    a = rng.random(n).astype(np.float32)                                              # 1 - d_t
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32)
    b = (rng.standard_normal(n) * np.abs(c) * 10.0 ** rng.integers(-8, 2, n)).astype(np.float32)
    # a share of near-ties: b chosen so that a * b is close to half an ulp of c
    half = (np.spacing(np.abs(c)) / 2).astype(np.float32)
    b[::3] = (half[::3] / a[::3]).astype(np.float32)
    b[::7] = 0.0
    got = ema.fma32(a, b, c)
    want = np.array([exact_fma32(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(bits(got), bits(want))
    # the plain fp32 expression (product rounded, then the sum) is a different function: the fused form is observable
    assert (bits((a * b + c).astype(np.float32)) != bits(want)).any()


def test_ema_step_special_values():
    z = np.zeros(4, dtype=np.float32)
    out = ema.ema_step(z, z, np.float32(0.1))
    assert not bits(out).any()                                                         # the padding stays +0
    e = np.array([1.5, -2.25, 3.0e38, 1e-40], dtype=np.float32)
    assert np.array_equal(bits(ema.ema_step(e, e, np.float32(0.3))), bits(e))          # p' = e: nothing moves
    p = np.array([4.0, 8.0, -3.0e38, 0.0], dtype=np.float32)
    keep = np.array([True, True, False, True])
    assert np.array_equal(bits(ema.ema_step(e[keep], p[keep], np.float32(0.0))), bits(e[keep]))      # 1 - d_t = 0
    out = ema.ema_step(e[:2], p[:2], np.float32(0.5))
    assert list(out) == [2.75, 2.875]
    # the fp32 difference overflows, as it does in the kernel: -Inf, and 0 x -Inf is NaN
    assert ema.ema_step(e[2:3], p[2:3], np.float32(0.5))[0] == -np.inf and np.isnan(ema.ema_step(e[2:3], p[2:3], np.float32(0.0))[0])


# ---------------------------------------------------------------- mutants
def table():
    """the random case table of tests/optim_ref.py with the masters before and after three float64 steps"""
    out = []
    for cid in ('normal-clip0.5', 'ties-lr0', 'three-steps'):
        c = ref.BY_ID[cid]
        d = ref.make_case(c)
        lay = d['lay']
        p, m, v = d['p'], d['m'], d['v']
        steps = []
        for i in range(3):
            args, g = ref.step_args(c, d, min(i, c['steps'] - 1))
            got = ref.emulate(p, g, m, v, lay, d['hp'], fused=True, **dict(args, step=c['step0'] + 2 * i + 1))
            steps.append((p, got['p'], False))
            p, m, v = got['p'], got['m'], got['v']
        out.append((cid, lay, ema.make_e(d['p'], lay.real, len(cid)), steps))
    return out


_TABLE = []


def rejected_by(mutant):
    """the first (case, decay, warm, n, skip pattern) on which a bit-for-bit comparison tells the mutant from run()"""
    if not _TABLE:
        _TABLE.extend(table())
    for cid, lay, e0, steps in _TABLE:
        for decay, warm, n in ema.SCHEDULE:
            for pattern in ((False, False, False), (False, True, False)):
                seq = [(a, b, s) for (a, b, _), s in zip(steps, pattern)]
                want, n_want = ema.run(e0, seq, n, decay, warm)
                got, n_got = ema.run(e0, seq, n, decay, warm, mutant=mutant)
                if n_got != n_want or any(not np.array_equal(bits(x), bits(y)) for x, y in zip(got, want)):
                    return cid, decay, warm, n, pattern
    return None


CAUGHT_BY = {
    'ema_of_old_p': ('normal-clip0.5', 0.9, 10.0, 0, (False, False, False)),
    'decay_swapped': ('normal-clip0.5', 0.9, 10.0, 0, (False, False, False)),
    'n_off_by_one': ('normal-clip0.5', 0.9, 10.0, 0, (False, False, False)),
    'skip_ticks': ('normal-clip0.5', 0.9, 10.0, 0, (False, True, False)),
    'warmup_ignored': ('normal-clip0.5', 0.9, 10.0, 0, (False, False, False)),
    'unfused': ('normal-clip0.5', 0.9, 10.0, 0, (False, False, False)),
}


@pytest.mark.parametrize('name', ema.MUTANTS)
def test_mutant_is_rejected(name):
    assert rejected_by(name) == CAUGHT_BY[name]


def test_mutants_differ_only_where_they_should():
    if not _TABLE:
        _TABLE.extend(table())
    cid, lay, e0, steps = _TABLE[0]
    # the unmutated run against itself; the schedule mutants are invisible once the warm-up is over or switched off
    for mutant in (None, 'n_off_by_one', 'warmup_ignored', 'skip_ticks'):
        seq = [(a, b, s) for (a, b, _), s in zip(steps, (False, True, False))]
        want, n_want = ema.run(e0, seq, 10 ** 5, 0.9, 0.0)
        got, n_got = ema.run(e0, seq, 10 ** 5, 0.9, 0.0, mutant=mutant)
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, want))
        assert (n_got == n_want) == (mutant != 'skip_ticks')
    # a skipped step: e and n untouched, the step after it uses the decay of the SAME n
    seq = [(steps[0][0], steps[0][1], True), (steps[1][0], steps[1][1], False)]
    out, n = ema.run(e0, seq, 1, 0.9, 10.0)
    assert n == 2 and np.array_equal(bits(out[0]), bits(e0))
    assert np.array_equal(bits(out[1]), bits(ema.ema_step(e0, steps[1][1], ema.omd_at(1, 0.9, 10.0))))
    # the padding stays +0 through every step
    out, _ = ema.run(e0, steps, 0, 0.9, 10.0)
    assert all(not bits(x)[~lay.real].any() for x in out)
    # the unfused form differs on SOME elements only: most roundings agree
    got, _ = ema.run(e0, steps[:1], 0, 0.9, 10.0, mutant='unfused')
    diff = bits(got[0]) != bits(out[0])
    assert 0 < diff.sum() < diff.size


def test_exact_lane_is_exact_for_the_average():
    """decay 1/2 and 3/4, e small integers, p' a multiple of 2^-7 below 64: e' = e + (1 - d)(p' - e) is a multiple of 2^-9 -
    exact in fp32 in any association, so the float64 formula rounded to fp32 is what every kernel variant must give"""
    for k in range(len(ref.EXACT_LAYOUTS)):
        d = ref.exact_case(k)
        want = ref.step(d['p'], d['g'], d['m'], d['v'], d['lay'], d['hp'], max_norm=ref.EXACT_MAX_NORM, zero_grad=1,
                        lr=ref.EXACT_LR)
        e0 = ema.exact_e(d['lay'])
        p32 = ref.to_f32(want)['p']              # (the float64 master carries the reference's 1e-6 of the clip: section 30)
        for decay in (0.5, 0.75):
            e64 = e0.astype(np.float64) + (1.0 - decay) * (p32.astype(np.float64) - e0.astype(np.float64))
            assert np.array_equal(e64 * 512, np.round(e64 * 512)) and np.abs(e64).max() < 64
            got = ema.ema_step(e0, p32, ema.omd_at(0, decay, 0.0))
            assert np.array_equal(bits(got), bits(e64.astype(np.float32)))
            unfused = (np.float32(decay) * e0 + np.float32(1 - decay) * p32).astype(np.float32)
            assert np.array_equal(bits(unfused), bits(got))
            assert not bits(got)[~d['lay'].real].any()


# ---------------------------------------------------------------- the declared ABI
STEP2_ARGS = ['param', 'grad', 'm', 'v', 'chunk_tensor', 'chunk_begin', 'n_chunks', 'n_tensors', 'partial', 'norms',
              'lr_dev', 'b1', 'b2', 'eps', 'wd', 'max_norm', 'grad_scale', 'shadow_bf16', 'zero_grad', 'skip',
              'grad_wire_bf16', 'step_dev', 'lr_base', 'warmup', 't_total', 'keep_grad']


def test_header_declares_the_new_entry_points():
    import ctypes
    import tell_amd
    protos = tell_amd.hip.parse_header()
    res, types, names = protos['tell_bertadam_step2']
    assert names == STEP2_ARGS + ['stream']
    res_e, types_e, names_e = protos['tell_bertadam_step_ema']
    assert res_e is ctypes.c_int
    assert names_e == STEP2_ARGS + ['ema', 'ema_omd_dev', 'ema_decay', 'ema_warm', 'stream']
    assert types_e == types[:-1] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_void_p]
    res_s, types_s, names_s = protos['tell_ema_swap']
    assert res_s is ctypes.c_int and names_s == ['param', 'ema', 'shadow_bf16', 'n', 'stream']
    assert types_s == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    lib = tell_amd.hip.lib()
    assert hasattr(lib, 'tell_bertadam_step_ema') and hasattr(lib, 'tell_ema_swap')


# ---------------------------------------------------------------- the host wrapper, hip.call recorded
def _flat(device='cpu'):
    from tell_amd.training.optimizers import FlatParams
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(*s)) for s in [(30, 70), (5,), (1025,)]]
    return ps, FlatParams([('p%d' % i, p) for i, p in enumerate(ps)], device)


@pytest.fixture
def calls(monkeypatch):
    import tell_amd
    import tell_amd.ops                      # noqa: F401 - (it binds hip.call by name when first imported: not under the patch)
    import tell_amd.training.optimizers      # noqa: F401
    rec = []
    monkeypatch.setattr(tell_amd.hip, 'call', lambda name, *args: rec.append((name, args)))
    return rec


CFG = dict(lr=1e-2, warmup=0.2, t_total=10, b1=0.9, b2=0.98, e=1e-6, weight_decay=1e-2, max_grad_norm=0.5)


def test_without_ema_decay_nothing_changes(calls):
    from tell_amd.training.optimizers import BertAdam
    ps, flat = _flat()
    opt = BertAdam(flat, **CFG)
    assert flat.ema is None and flat.ema_omd is None and opt.ema_decay is None
    skip = torch.zeros(2, dtype=torch.int32)
    opt.launch(grad_scale=0.5, zero_grad=True, skip=skip)
    assert len(calls) == 1
    name, args = calls[0]
    f = flat
    want = (f.flat, f.grad, f.m, f.v, f.chunk_tensor, f.chunk_begin, f.n_chunks, 3, f.partial, f.norms, opt.lr_dev, 0.9,
            0.98, 1e-6, 1e-2, 0.5, 0.5, None, 1, skip, None, opt.step_dev, 1e-2, 0.2, 10.0, None)
    assert name == 'tell_bertadam_step2' and len(args) == len(want) == len(STEP2_ARGS)
    assert all((a is b) if (torch.is_tensor(a) or torch.is_tensor(b)) else (a == b and type(a) is type(b))
               for a, b in zip(args, want)), args
    assert set(opt.state_dict()) == {'step', 'm', 'v'}
    with pytest.raises(ValueError, match='ema_decay'):
        opt.reset_ema()


def test_with_ema_decay_the_new_entry_point_gets_the_buffers_in_the_declared_order(calls):
    import tell_amd
    from tell_amd.training.optimizers import BertAdam
    ps, flat = _flat()
    before = flat.flat.clone()
    opt = BertAdam(flat, ema_decay=0.9, **CFG)
    assert opt.ema_warmup == 10.0
    assert flat.ema.dtype == torch.float32 and flat.ema.shape == flat.flat.shape and torch.equal(flat.ema, before)
    assert flat.ema.data_ptr() != flat.flat.data_ptr() and flat.ema_omd.shape == (1,) and flat.ema_omd.dtype == torch.float32
    opt.launch(zero_grad=False)
    name, args = calls[-1]
    names = tell_amd.hip.parse_header()['tell_bertadam_step_ema'][2]
    assert name == 'tell_bertadam_step_ema' and len(args) == len(names) - 1             # (hip.call adds the stream)
    got = dict(zip(names, args))
    f = flat
    for key, t in (('param', f.flat), ('grad', f.grad), ('m', f.m), ('v', f.v), ('chunk_tensor', f.chunk_tensor),
                   ('chunk_begin', f.chunk_begin), ('partial', f.partial), ('norms', f.norms), ('lr_dev', opt.lr_dev),
                   ('step_dev', opt.step_dev), ('ema', f.ema), ('ema_omd_dev', f.ema_omd)):
        assert got[key] is t, key
    assert got['ema_decay'] == 0.9 and got['ema_warm'] == 10.0 and type(got['ema_warm']) is float
    assert got['keep_grad'] is None and got['zero_grad'] == 0 and got['n_chunks'] == f.n_chunks
    assert set(opt.state_dict()) == {'step', 'm', 'v', 'ema'} and opt.state_dict()['ema'] is f.ema
    flat.flat.add_(1.0)
    opt.reset_ema()
    assert torch.equal(flat.ema, flat.flat)
    opt2 = BertAdam(_flat()[1], ema_decay=0, ema_warmup=0, **CFG)                      # the ends of both ranges
    opt2.launch()
    assert calls[-1][1][-2:] == (0.0, 0.0)
    # the masters sit in the EMA buffer while the trainer has them exchanged: no update then
    opt.ema_swapped = True
    n = len(calls)
    with pytest.raises(RuntimeError, match='ema_weights'):
        opt.launch()
    with pytest.raises(RuntimeError, match='ema_weights'):
        opt.step()
    assert len(calls) == n


@pytest.mark.parametrize('key,value', [('ema_decay', 1.0), ('ema_decay', -0.1), ('ema_decay', float('nan')),
                                       ('ema_decay', float('inf')), ('ema_decay', '0.9'), ('ema_decay', True),
                                       ('ema_warmup', -1.0), ('ema_warmup', float('inf')), ('ema_warmup', float('nan')),
                                       ('ema_warmup', None)])
def test_bad_values_name_the_key_and_the_value(key, value):
    from tell_amd.training.optimizers import BertAdam
    kw = dict(CFG, ema_decay=0.9)
    kw[key] = value
    flat = _flat()[1]
    with pytest.raises(ValueError) as err:
        BertAdam(flat, **kw)
    assert key in str(err.value) and repr(value) in str(err.value)
    assert flat.ema is None


def test_ema_warmup_is_not_looked_at_without_ema_decay():
    from tell_amd.training.optimizers import BertAdam
    assert BertAdam(_flat()[1], ema_warmup=-5, **CFG).ema_decay is None
    sig = inspect.signature(BertAdam.__init__).parameters
    assert sig['ema_decay'].default is None and sig['ema_warmup'].default == 10.0


def test_state_dict_with_and_without_the_average():
    from tell_amd.training.optimizers import BertAdam
    flat_a = _flat()[1]
    a = BertAdam(flat_a, ema_decay=0.9, **CFG)
    flat_a.ema.mul_(0.5)
    flat_a.m.add_(1.0)
    sd = {k: (x.clone() if torch.is_tensor(x) else x) for k, x in a.state_dict().items()}
    sd['step'] = 4
    # with 'ema' into an optimizer with the feature: restored
    flat_b = _flat()[1]
    b = BertAdam(flat_b, ema_decay=0.9, **CFG)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        b.load_state_dict(sd)
    assert torch.equal(flat_b.ema, flat_a.ema) and torch.equal(flat_b.m, flat_a.m) and b.applied_steps() == 4
    # without 'ema': the average restarts from the loaded weights, one warning however often it happens
    old = {k: v for k, v in sd.items() if k != 'ema'}
    flat_b.flat.add_(2.0)
    with pytest.warns(UserWarning, match="no 'ema'") as rec:
        b.load_state_dict(old)
        b.load_state_dict(old)
    assert len(rec) == 1 and torch.equal(flat_b.ema, flat_b.flat)
    # with 'ema' into an optimizer without the feature: ignored, one warning
    flat_c = _flat()[1]
    c = BertAdam(flat_c, **CFG)
    with pytest.warns(UserWarning, match='ignored') as rec:
        c.load_state_dict(sd)
        c.load_state_dict(sd)
    assert len(rec) == 1 and flat_c.ema is None and torch.equal(flat_c.m, flat_a.m) and set(c.state_dict()) == {'step', 'm', 'v'}
