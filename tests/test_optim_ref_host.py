"""tests/optim_ref.py proved on the CPU: the float64 step against oracle/optim.py and direct
formulas, the fp32 emulation of the kernels inside every bound at the pinned constants, the exact lane exact (fused and
unfused), and the MUTANTS - deliberately wrong variants that the comparisons of tests/test_gpu_optim.py must reject.
The last test is the CPU half of the wrapper classes: the FlatParams layout (it needs the built library only)."""
import numpy as np
import pytest
import torch

import optim_ref as ref

BY_ID = ref.BY_ID
IDS = [c['id'] for c in ref.CASES]
_DATA = {}


def data(c):
    if c['id'] not in _DATA:
        _DATA[c['id']] = ref.make_case(c)
    return _DATA[c['id']]


def first_step(c, fn=ref.step, **kw):
    d = data(c)
    args, g = ref.step_args(c, d, 0)
    args.update(kw)
    return fn(d['p'], g, d['m'], d['v'], d['lay'], d['hp'], **args), d, g


# ---------------------------------------------------------------- a. the reference against independent formulations
@pytest.mark.parametrize('cid', IDS)
def test_reference_equals_the_oracle_in_float64(cid):
    from oracle.optim import BertAdam as OAdam
    c = BY_ID[cid]
    out, d, g = first_step(c)
    lay, hp = d['lay'], d['hp']
    f = lambda x: float(np.float32(x))                                       # noqa: E731
    wire = ref.step_args(c, d, 0)[0].get('wire')
    src = ref.bf16_widen(wire) if wire is not None else g
    params = []
    for o, n in zip(lay.offsets, lay.sizes):
        q = torch.nn.Parameter(torch.from_numpy(d['p'][o:o + n].astype(np.float64)))
        q.grad = torch.from_numpy(src[o:o + n].astype(np.float64) * np.float64(np.float32(c['grad_scale'])))
        params.append(q)
    opt = OAdam(params, lr=f(c['lr']), warmup=f(c['warmup']), t_total=f(c['t_total']), b1=f(hp['b1']), b2=f(hp['b2']),
                e=f(hp['eps']), weight_decay=f(hp['wd']), max_grad_norm=f(c['max_norm']))
    for q, o, n in zip(params, lay.offsets, lay.sizes):
        st = opt.state[id(q)]
        st['step'] = c['step0']
        st['m'] = torch.from_numpy(d['m'][o:o + n].astype(np.float64))
        st['v'] = torch.from_numpy(d['v'][o:o + n].astype(np.float64))
    opt.step()
    for t, (q, o, n) in enumerate(zip(params, lay.offsets, lay.sizes)):
        st = opt.state[id(q)]
        np.testing.assert_allclose(out['p'][o:o + n], q.detach().numpy(), rtol=1e-10, atol=0)
        np.testing.assert_allclose(out['m'][o:o + n], st['m'].numpy(), rtol=1e-10, atol=0)
        np.testing.assert_allclose(out['v'][o:o + n], st['v'].numpy(), rtol=1e-10, atol=0)
        if out['norms'] is not None:
            np.testing.assert_allclose(out['norms'][t], float(q.grad.norm()), rtol=1e-12)
    assert out['step'] == c['step0'] + 1 and out['applied']
    pad = ~lay.real                                          # the padding stays +0
    for k in ('p', 'm', 'v'):
        assert not out[k][pad].any() and not np.signbit(out[k][pad]).any()


def test_schedule_is_warmup_linear():
    from oracle.optim import warmup_linear
    from tell_amd.training.optimizers import warmup_linear as wl2
    for warm, tt in ((0.5, 4.0), (0.2, 10.0), (0.05, 437600.0)):
        w = float(np.float32(warm))
        for s in (0, 1, 2, 3, int(tt) - 1, int(tt), int(tt) + 5):
            want = float(np.float32(1e-2)) * warmup_linear(s / tt, w)
            assert ref.schedule(s, 1e-2, warm, tt) == want == float(np.float32(1e-2)) * wl2(s / tt, w)
    assert ref.schedule(0, 1e-2, 0.5, 4.0) == 0.0 and ref.schedule(4, 1e-2, 0.5, 4.0) == 0.0
    assert ref.schedule(2, 0.25, 0.5, 4.0) == 0.25 and ref.schedule(9, 0.25, 0.5, 4.0) == 0.0
    for tt in (-1.0, 0.0):                                   # constant rate
        assert ref.schedule(7, 0.25, 0.2, tt) == 0.25
    assert ref.schedule(0, 0.25, -1.0, 10.0) == 0.125 and ref.schedule(5, 0.25, -1.0, 10.0) == 0.0625   # (1 - x) / 2


def test_bf16_helpers_against_torch():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-30, 30, 4096),
                        data(BY_ID['ties-lr0'])['p'][:64]]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(ref.bf16_rne(x).view(np.int16), want.view(torch.int16).numpy())
    assert np.array_equal(ref.bf16_widen(ref.bf16_rne(x)), want.float().numpy())
    tie = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=np.float32)
    assert list(ref.bf16_rne(tie)) == [0x3f80, 0x3f82] and list(ref.bf16_trunc(tie)) == [0x3f80, 0x3f81]


def test_wire_gradient_is_the_widened_gradient():
    a, d, _ = first_step(BY_ID['wire-clip0.5'])
    b, _, g = first_step(BY_ID['wire-clip0.5-widened'])
    for k in ('p', 'm', 'v', 'norms'):
        assert np.array_equal(a[k], b[k])
    assert a['grad'].any() and not a['grad'][np.repeat(d['keep'][d['lay'].chunk_tensor] == 0, ref.CHUNK)].any()
    h = np.array([0x3f80, 0xc000, 0x0000, 0x4040], dtype=np.uint16)              # 1, -2, 0, 3: element 0 is the LOW half-word
    assert list(ref.bf16_widen(h)) == [1.0, -2.0, 0.0, 3.0]


@pytest.mark.parametrize('preset', [1, 2, 3])
@pytest.mark.parametrize('zero_grad', [0, 1])
def test_skip_path_by_direct_formulas(preset, zero_grad):
    c = BY_ID['heavy-clip0.5-keepmixed']
    out, d, g = first_step(c, skip=(preset, 5), zero_grad=zero_grad)
    assert not out['applied'] and out['skip'] == (preset, 6) and out['step'] == c['step0'] and out['shadow'] is None
    for k in ('p', 'm', 'v'):
        assert np.array_equal(out[k], d[k].astype(np.float64))
    kept = np.repeat(d['keep'][d['lay'].chunk_tensor] != 0, ref.CHUNK)
    want = g.copy()
    if zero_grad:
        want[~kept] = 0.0
    assert np.array_equal(out['grad'], want) and want[kept].any()
    assert out['lr'] == ref.schedule(c['step0'], c['lr'], c['warmup'], c['t_total'])


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf, 3e19])
def test_non_finite_gradient_sets_bit_two(bad):
    """3e19: finite, but 64 of them square-sum past fp32 - flagged like Inf (F32_LIMIT is on the SUM of squares)"""
    c = BY_ID['normal-clip0.5']
    d = data(c)
    args, g = ref.step_args(c, d, 0)
    g = g.copy()
    g[d['lay'].offsets[2]:d['lay'].offsets[2] + (64 if bad == 3e19 else 1)] = bad
    for fn in (ref.step, ref.emulate):
        out = fn(d['p'], g, d['m'], d['v'], d['lay'], d['hp'], **dict(args, skip=(0, 0)))
        assert out['skip'] == (2, 1) and not out['applied'] and out['step'] == c['step0']
        out = fn(d['p'], g, d['m'], d['v'], d['lay'], d['hp'], **dict(args, skip=(0, 0), max_norm=0.0))
        assert out['skip'] == (0, 0) and out['applied']           # never inspected without clipping (tell_hip.h: limit)


# ---------------------------------------------------------------- b. the emulation inside the bounds
def run_steps(c, fn, **kw):
    """teacher-forced: the reference restarts each step from the state `fn` left -> [(got, ref)]"""
    d = data(c)
    p, m, v = d['p'], d['m'], d['v']
    out = []
    for i in range(c['steps']):
        args, g = ref.step_args(c, d, i)
        got = fn(p, g, m, v, d['lay'], d['hp'], **dict(args, **kw))
        want = ref.step(p, g, m, v, d['lay'], d['hp'], p_dev=got['p'], **args)
        out.append((got, want))
        p, m, v = got['p'], got['m'], got['v']
    return out


EMU_RATIOS = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for k in sorted(EMU_RATIOS):                                # (-s: the emulation's column of the constants table)
        print('\nemulation: largest ratio %s %.4f  (%s)' % ((k,) + EMU_RATIOS[k]))


@pytest.mark.parametrize('fused', [False, True], ids=['unfused', 'fused'])
@pytest.mark.parametrize('cid', IDS)
def test_emulation_is_inside_every_bound(cid, fused):
    c = BY_ID[cid]
    for i, (got, want) in enumerate(run_steps(c, ref.emulate, fused=fused)):
        r = ref.ratios(got, want)
        r['lr'] = ref.lr_ratio(got['lr'], want['lr'], c['lr'])
        for k, x in r.items():
            k = '%-2s %s' % (k, 'as the kernel fuses' if fused else 'nothing fused')
            if x > EMU_RATIOS.get(k, (0.0, ''))[0]:
                EMU_RATIOS[k] = (x, cid)
        print(cid, 'step', i, 'fused' if fused else 'unfused', {k: round(x, 3) for k, x in r.items()})
        assert ref.inside(r), r
        assert np.array_equal(got['shadow'], want['shadow']) and np.array_equal(got['grad'], want['grad'])
        assert got['step'] == want['step']
        pad = ~data(c)['lay'].real
        for k in ('p', 'm', 'v'):
            assert not got[k][pad].any() and not np.signbit(got[k][pad]).any()


@pytest.mark.parametrize('chunks', [1, 255, 257, 769, 1025, 1300, 2100])
def test_emulated_tensor_norms_loop_structure(chunks):
    """emu_norms walks tensor_norms_kernel's two loops: every partial is counted exactly once (integers: exact in any
    order), also with a neighbour tensor on either side, and random partials stay inside c_n"""
    begin = np.array([0, 3, 3 + chunks, 3 + chunks + 2])
    ints = np.arange(1, begin[-1] + 1, dtype=np.float32)
    norms, sums = ref.emu_norms(ints, begin)
    assert [float(s) for s in sums] == [float(ints[a:b].astype(np.float64).sum()) for a, b in zip(begin[:-1], begin[1:])]
    part = np.random.default_rng(chunks).random(begin[-1]).astype(np.float32)
    norms, sums = ref.emu_norms(part, begin)
    want = np.sqrt([part[a:b].astype(np.float64).sum() for a, b in zip(begin[:-1], begin[1:])])
    assert (np.abs(norms - want) / (ref.U24 * want)).max() <= ref.C['n']


def test_bounds_are_tight_enough_to_mean_something():
    """one fp32 ulp of relative error on every element is far outside: the constants are not a blank cheque"""
    c = BY_ID['normal-clip0.5']
    want, d, g = first_step(c)
    for k, fn in (('m', ref.m_ratio), ('v', ref.v_ratio), ('p', ref.p_ratio)):
        assert fn(want[k] * (1 + 64 * ref.U24), want) > 4 * ref.C[k]
        assert fn(want[k], want) == 0.0
    assert ref.norms_ratio(want['norms'] * (1 + 64 * ref.U24), want) > 4 * ref.C['n']


# ---------------------------------------------------------------- c. mutants
def differs(mut, want, c):
    """does the comparison the GPU test makes tell `mut` from the reference `want`?"""
    if mut['applied'] != want['applied'] or mut['step'] != want['step'] or mut['skip'] != want['skip']:
        return True
    if not np.array_equal(mut['grad'], want['grad']):
        return True
    if ref.lr_ratio(mut['lr'], want['lr'], c['lr']) > ref.C['lr']:
        return True
    if not want['applied']:
        return False
    if not np.array_equal(mut['shadow'], want['shadow']):
        return True
    return not ref.inside(ref.ratios(mut, want))


def mutant_caught_by(name):
    for c in ref.CASES:
        d = data(c)
        args, g = ref.step_args(c, d, 0)
        state = (d['p'], g, d['m'], d['v'], d['lay'], d['hp'])
        if name.startswith('skip_'):
            args = dict(args, skip=(1, 0))
        want = ref.step(*state, **args)
        if name == 'tail_chunk_dropped':
            mut = ref.emulate(*state, U=4, mutant=name, **args)
            want = ref.step(*state, p_dev=mut['p'], **args)
        else:
            mut = ref.step(*state, mutant=name, **args)
            if name != 'shadow_trunc' and mut['applied']:              # the shadow is judged against the mutant's own master
                mut['shadow'] = ref.bf16_rne(mut['p'].astype(np.float32))
                want = dict(want, shadow=mut['shadow'])
        if differs(mut, want, c):
            return c['id']
    return None


# the first case of the table that rejects each mutant
CAUGHT_BY = {
    'global_norm': 'normal-clip0.5', 'norm_unscaled': 'gs8-clip0.5', 'neighbour_norm': 'normal-clip0.5',
    'v_unclipped': 'normal-clip0.5', 'sqrt_inside': 'normal-clip0.5', 'bias_correction': 'normal-clip0.5',
    'wd_after': 'normal-clip0.5', 'schedule_next': 'normal-clip0.5', 'wire_swapped': 'wire-clip0.5',
    'shadow_trunc': 'normal-clip0.5', 'tail_chunk_dropped': 'normal-clip0.5', 'skip_advances': 'normal-clip0.5',
    'skip_ignores_keep': 'heavy-clip0.5-keepmixed',
}


@pytest.mark.parametrize('name', ref.MUTANTS)
def test_mutant_is_caught(name):
    assert mutant_caught_by(name) == CAUGHT_BY[name]


def test_grad_scale_moves_one_tensor_across_the_threshold():
    """what makes `norm_unscaled` visible as a clip DECISION, not only as a coefficient"""
    a, d, _ = first_step(BY_ID['normal-clip0.5'])
    b, _, _ = first_step(BY_ID['gs8-clip0.5'])
    assert a['norms'][5] > 0.5 > b['norms'][5] > 0.1
    n = a['norms']
    assert (n > 0.5).sum() >= 3 and (n < 0.5).sum() >= 3 and n[2] / n[1] > 1e4 and n[2] / n[3] > 1e3


def test_no_mutant_hides_in_an_unmutated_run():
    c = BY_ID['normal-clip0.5']
    want, d, g = first_step(c)
    assert not differs(first_step(c)[0], want, c)


# ---------------------------------------------------------------- d. the exact lane
@pytest.mark.parametrize('k', range(len(ref.EXACT_LAYOUTS)))
def test_exact_lane_is_exact_in_fp32(k):
    d = ref.exact_case(k)
    lay = d['lay']
    kw = dict(max_norm=ref.EXACT_MAX_NORM, zero_grad=1, lr=ref.EXACT_LR)
    want = ref.step(d['p'], d['g'], d['m'], d['v'], lay, d['hp'], **kw)
    w32 = ref.to_f32(want)
    assert np.array_equal(want['norms'], d['norms'])
    assert all((n == 0 or (n >= 32 and np.log2(n) % 1 == 0)) for n in d['norms'])
    for fused in (False, True):
        got = ref.emulate(d['p'], d['g'], d['m'], d['v'], lay, d['hp'], fused=fused, **kw)
        for key in ('p', 'm', 'v', 'norms'):
            assert np.array_equal(got[key].view(np.uint32), w32[key].view(np.uint32)), (key, fused)
        assert np.array_equal(got['shadow'], want['shadow'])
        assert np.array_equal(got['shadow'], ref.bf16_rne(w32['p']))
    nz = d['g'] != 0                                             # |u| = 1/2 wherever there is a gradient, m = g'/2, v = g'^2/4
    assert np.array_equal(np.abs(w32['m'][nz]), np.full(nz.sum(), 16.0, np.float32))
    assert np.array_equal(w32['v'][nz], np.full(nz.sum(), 256.0, np.float32))
    assert np.array_equal(w32['p'] * 128, np.round(w32['p'] * 128)) and np.abs(w32['p']).max() < 64
    assert not want['grad'].any()


def test_exact_lane_covers_what_it_claims():
    chunks = sorted(ref.Layout(s).n_chunks for s, _ in ref.EXACT_LAYOUTS)
    assert chunks == [1, 2, 3, 4, 5, 7, 8, 9, 11, 13]
    assert {len(s) for s, _ in ref.EXACT_LAYOUTS} == {1, 2, 3, 4, 5}
    assert {n for s, _ in ref.EXACT_LAYOUTS for n in s} == {1, 5, 1023, 1024, 1025, 2049}
    spec = [x for _, sp in ref.EXACT_LAYOUTS for x in sp]
    assert any(j > 0 for _, j in spec) and any(j == 0 and c4 == 3 for c4, j in spec) and any(c4 is None for c4, _ in spec)
    for U in (1, 2, 4):
        assert {n % U for n in chunks} == set(range(U))


# ---------------------------------------------------------------- FlatParams layout (CPU; the built library only)
def test_flat_params_layout():
    from tell_amd.training.optimizers import FlatParams
    torch.manual_seed(0)
    shapes = [(30, 70), (5,), (1024,), (33, 1), (2049,)]
    ps = [torch.nn.Parameter(torch.randn(*s)) for s in shapes]
    frozen = torch.nn.Parameter(torch.randn(7), requires_grad=False)
    before = [p.detach().clone() for p in ps]
    named = [('a', ps[0]), ('frozen', frozen), ('b', ps[1]), ('a_again', ps[0]), ('c', ps[2]), ('d', ps[3]), ('e', ps[4])]
    flat = FlatParams(named, 'cpu')
    assert flat.names == ['a', 'b', 'c', 'd', 'e'] and all(a is b for a, b in zip(flat.params, ps))
    lay = ref.Layout([p.numel() for p in ps])
    assert flat.chunk == ref.CHUNK and flat.total == lay.total and flat.n_chunks == lay.n_chunks
    assert flat.offsets == list(lay.offsets) and all(o % flat.chunk == 0 for o in flat.offsets)
    assert np.array_equal(flat.chunk_tensor.numpy(), lay.chunk_tensor) and flat.chunk_tensor.dtype == torch.int32
    assert np.array_equal(flat.chunk_begin.numpy(), lay.chunk_begin) and flat.chunk_begin.dtype == torch.int64
    assert flat.numel() == sum(lay.sizes) and flat.keep_grad.numel() == 5 and flat.norms.numel() == 5
    assert flat.partial.numel() == lay.n_chunks and flat.shadow is None
    for p, b, o in zip(ps, before, flat.offsets):
        n = p.numel()
        assert torch.equal(p.data, b) and p.data.data_ptr() == flat.flat[o:].data_ptr()
        assert p.grad.data_ptr() == flat.grad[o:].data_ptr() and p.grad.shape == p.shape
        flat.grad[o:o + n] = 2.0                             # aliasing, both ways
        p.data.mul_(0).add_(3.0)
        assert bool((p.grad == 2.0).all()) and bool((flat.flat[o:o + n] == 3.0).all())
    real = torch.from_numpy(lay.real)
    for buf in (flat.flat, flat.grad, flat.m, flat.v):
        assert not buf[~real].any()
    assert frozen.grad is None and frozen.numel() == 7
