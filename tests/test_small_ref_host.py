"""tests/small_ref.py on the CPU: the fp32 emulation of every kernel stays inside every bound at
c = 1 on every case of every table, every mutant breaks a bound or an exact comparison on a case that names it, every
dispatch path the entry points have is reached by a case, and no case is in a table without a path or a mutant that needs
it."""
import numpy as np
import pytest

import small_ref as ref

F32, F64 = np.float32, np.float64
OUTS = ('bfloat16', 'float32')


def stored(outs):
    """what a kernel computing `outs` would leave in memory"""
    return {k: ref.store(o.value, o.dtype) for k, o in outs.items()}


def broken(got, want, pinned=False):
    """{output: elements outside what the reference allows} (only the outputs with any).  Measured groups: at c = 1 (the
    emulation), or - pinned, for a mutant - at the larger of 1 and the pinned constant, the bound the GPU test uses"""
    assert set(got) == set(want)
    c = lambda o: None if o.group in (None, 'exact') else (max(1.0, ref.C.get(o.group, 0.0)) if pinned else 1.0)   # noqa: E731
    bad = {k: ref.failures(got[k], want[k], c(want[k])) for k in want}
    return {k: v for k, v in bad.items() if v}


# ---------------------------------------------------------------- one (reference, emulation, mutant) triple per family
def wn_runs(case, mutant=None):
    for out in OUTS:
        emu = ref.wn_case(case, out, F32)
        norms = emu['norms'].value.astype(np.float32)
        want = ref.wn_case(case, out, F64, norms=norms)
        yield want, stored(emu if mutant is None else ref.wn_case(case, out, F64, mutant, norms))


def wn_multi_runs(pattern, mutant=None):
    for out in OUTS:
        emu = ref.wn_multi(pattern, out, F32)
        norms = [e['norms'].value.astype(np.float32) for e in emu]
        want = ref.wn_multi(pattern, out, F64, norms=norms)
        got = emu if mutant is None else ref.wn_multi(pattern, out, F64, mutant, norms)
        yield ({'%d.%s' % (j, k): o for j, r in enumerate(want) for k, o in r.items()},
               stored({'%d.%s' % (j, k): o for j, r in enumerate(got) for k, o in r.items()}))


def mix_runs(case, mutant=None):
    for nb in ref.MIX_BLOCKS:
        yield ref.mix_case(case, nb), stored(ref.mix_case(case, nb, F32 if mutant is None else F64, mutant))


def wgrad_runs(case, mutant=None):
    big = ref.mix_wgrad_source()
    x = ref.mix_inputs(big)
    partial = ref.store(ref.mix_case(big, case['nb'], F32)['partial'].value, 'float32')
    got = ref.mix_wgrad(partial, x['w'], x['gw0'], F32 if mutant is None else F64, mutant)
    yield ref.mix_wgrad(partial, x['w'], x['gw0']), stored(got)


def lstm_runs(case, mutant=None):
    for dty in OUTS:
        emu = ref.lstm_case(case, dty, F32)
        gates, c = ref.store(emu['gates'].value, 'float32'), ref.store(emu['c'].value, dty)
        yield (ref.lstm_case(case, dty, F64, None, gates, c),
               stored(emu if mutant is None else ref.lstm_case(case, dty, F64, mutant, gates, c)))


def tanh_runs(case, mutant=None):
    for dty in OUTS:
        r = ref._rng('tanh', case['n'])
        x, dy = ref.store(r.standard_normal(case['n']) * 2, dty), ref.store(r.standard_normal(case['n']), dty)
        emu = ref.tanh_fwd(x, dty, F32)
        y = ref.store(emu['y'].value, dty)
        want, got = ref.tanh_fwd(x, dty), emu
        want.update(ref.tanh_bwd(dy, y, dty))
        got.update(ref.tanh_bwd(dy, y, dty, F32))
        yield want, stored(got)


def da_runs(case, mutant=None):
    for dty in OUTS:
        emu = ref.da_case(case, dty, F32)
        probs = ref.store(emu['probs'].value, 'float32')
        got = emu if mutant is None else ref.da_case(case, dty, F64, mutant, probs)
        yield ref.da_case(case, dty, F64, None, probs), stored(got)


def colsum_runs(case, mutant=None):
    yield ref.colsum_case(case), stored(ref.colsum_case(case, F32 if mutant is None else F64, mutant))


def csm_runs(case, mutant=None):
    name = lambda outs: {'job%d' % j: o for j, o in enumerate(outs)}                              # noqa: E731
    yield name(ref.colsum_multi()), stored(name(ref.colsum_multi(F32 if mutant is None else F64, mutant)))


def tr_runs(case, mutant=None):
    yield ref.tr_case(case), stored(ref.tr_case(case, mutant))


def trm_runs(case, mutant=None):
    name = lambda outs: {'job%d' % j: o for j, o in enumerate(outs)}                              # noqa: E731
    yield name(ref.transpose_multi()), stored(name(ref.transpose_multi(mutant)))


def pw_runs(case, mutant=None):
    yield ref.pw_case(case), stored(ref.pw_case(case, F32 if mutant is None else F64, mutant))


FAMILIES = {
    'wn': (ref.WN, wn_runs, ref.wn_paths),
    'wn_multi': ([dict(id=p, mutants=ref.WN_MUTANTS[-2:]) for p in ref.WN_MULTI_STORE],
                 lambda case, mutant=None: wn_multi_runs(case['id'], mutant), lambda case: {'wn_multi:store:' + case['id']}),
    'mix': (ref.MIX, mix_runs, ref.mix_paths),
    'mix_wgrad': (ref.MIX_WGRAD, wgrad_runs, lambda case: {'mix_wgrad:blocks%d' % case['nb']}),
    'colsum': (ref.COLSUM, colsum_runs, ref.colsum_paths),
    'colsum_multi': ([dict(id='all', mutants=ref.CSM_MUTANTS)], csm_runs, lambda case: ref.csm_paths()),
    'transpose': (ref.TR, tr_runs, ref.tr_paths),
    'transpose_multi': ([dict(id='all', mutants=ref.TR_MUTANTS[-2:])], trm_runs, lambda case: ref.trm_paths()),
    'lstm': (ref.LSTM, lstm_runs, ref.lstm_paths),
    'tanh': ([dict(id='n%d' % n, n=n, mutants=()) for n in ref.TANH_N], tanh_runs,
             lambda case: {'tanh:' + ('single_element' if case['n'] == 1 else
                                      ('below' if case['n'] < 256 else ('at' if case['n'] == 256 else 'above')))}),
    'dot_attn': (ref.DA, da_runs, ref.da_paths),
    'pointwise': (ref.PW, pw_runs, ref.pw_paths),
}
CASES = [(f, c) for f, (cases, _, _) in FAMILIES.items() for c in cases]
IDS = ['%s-%s' % (f, c['id']) for f, c in CASES]


@pytest.mark.parametrize('fam,case', CASES, ids=IDS)
def test_fp32_emulation_is_inside_every_bound_at_c_1(fam, case):
    for want, got in FAMILIES[fam][1](case):
        assert not broken(got, want), (fam, case['id'])


@pytest.mark.parametrize('fam,case', [fc for fc in CASES if fc[1]['mutants']],
                         ids=[i for i, fc in zip(IDS, CASES) if fc[1]['mutants']])
def test_every_mutant_is_caught_on_the_case_that_names_it(fam, case):
    for mutant in case['mutants']:
        assert mutant in ref.MUTANTS
        caught = any(broken(got, want, pinned=True) for want, got in FAMILIES[fam][1](case, mutant))
        assert caught, '%s survives %s %s' % (mutant, fam, case['id'])


def test_every_mutant_is_named_by_a_case():
    named = {m for _, c in CASES for m in c['mutants']}
    assert named == set(ref.MUTANTS), set(ref.MUTANTS) ^ named
    assert len(set(ref.MUTANTS)) == len(ref.MUTANTS)


PATHS = {
    'wn_fwd:reg', 'wn_fwd:vec4', 'wn_fwd:scalar', 'wn_bwd:reg', 'wn_bwd:vec4', 'wn_bwd:scalar', 'wn_bwd:scalar:misaligned',
    'wn_bwd:store', 'wn_bwd:accumulate', 'wn_rows%4=0', 'wn_rows%4=1', 'wn_rows%4=3', 'wn_multi:store:late',
    'wn_multi:store:early', 'mix:vec:bfloat16', 'mix:scalar:n%8', 'mix:scalar:misaligned', 'mix:scalar:L>32',
    'mix:scalar:float32', 'mix:logits:equal', 'mix:logits:spread', 'mix:logits:random', 'mix:blocks>work',
    'mix:several_trips', 'mix:ragged_tail', 'mix:whole_blocks', 'mix_wgrad:blocks1', 'mix_wgrad:blocks16',
    'mix_wgrad:blocks17', 'mix_wgrad:blocks40', 'colsum:direct', 'colsum:finish', 'colsum:finish:128x129',
    'colsum:m_dev:null', 'colsum:m_dev:zero', 'colsum:m_dev:inside', 'colsum:m_dev:edge', 'colsum:m_dev:above',
    'colsum:bfloat16', 'colsum:float32', 'colsum:acc0', 'colsum:acc1', 'colsum:rows0', 'colsum:C%64=0', 'colsum:C%64=1',
    'colsum:C%64=63', 'colsum:C%64=8', 'colsum:ld>C', 'colsum:ld=C', 'csm:launch0', 'csm:launch1', 'csm:w0:zero',
    'csm:w0:width', 'csm:w0:mid%64=1', 'tr:float32->float32', 'tr:float32->bfloat16', 'tr:bfloat16->bfloat16',
    'tr:bfloat16->float32', 'tr:scaled', 'tr:unscaled', 'tr:outs:t', 'tr:outs:plain', 'tr:outs:both', 'trm:launch0',
    'trm:launch1', 'trm:load:none+tail', 'trm:load:vec', 'trm:load:vec+tail', 'trm:store:none+tail', 'trm:store:vec',
    'trm:store:vec+tail', 'trm:tiles1', 'trm:tiles6', 'trm:tiles4', 'scale_cast:n%4=0', 'scale_cast:n%4=1',
    'scale_cast:n%4=2', 'scale_cast:n%4=3', 'scale_cast:scale:null', 'scale_cast:scale:device', 'scale_cast:float32',
    'scale_cast:bfloat16', 'sum_n:inputs1', 'sum_n:inputs8', 'lstm:null:None', 'lstm:null:dh', 'lstm:null:dc',
    'lstm:one_block', 'lstm:ragged_last_block', 'tanh:below', 'tanh:at', 'tanh:above', 'tanh:single_element', 'da:lay:lbd',
    'da:lay:bld', 'da:lay:padded', 'da:mask:none', 'da:mask:ragged', 'da:mask:one', 'da:mask:row0', 'da:dsrc:0', 'da:dsrc:1',
    'glu:C1', 'glu:C5', 'glu:C64', 'glu:below', 'glu:at', 'glu:above', 'glu:float32', 'glu:bfloat16', 'gelu:below', 'gelu:at',
    'gelu:above', 'loss_bits', 'embed:E>256', 'embed:float32', 'embed:bfloat16', 'mask_rows:second_trip', 'mask_rows:float32',
    'mask_rows:bfloat16', 'tr:row_tiles:one_ragged', 'tr:row_tiles:whole', 'tr:row_tiles:several_ragged',
    'tr:col_tiles:one_ragged', 'tr:col_tiles:whole', 'tr:col_tiles:several_ragged', 'da:keys:<4:ragged',
    'da:keys:one_trip:whole', 'da:keys:one_trip:ragged', 'da:keys:several_trips:ragged', 'da:keys:several_trips:whole',
    'da:lanes:partial', 'da:lanes:whole', 'da:lanes:ragged', 'da:D>256', 'da:D<=256', 'da:one_block', 'da:several_blocks',
    'csm:walk:groups_empty', 'csm:walk:remainder_only', 'csm:walk:unrolled_for_some', 'csm:walk:unrolled',
    'csm:walk:unrolled+remainder', 'csm:cols:partial', 'csm:cols:whole', 'csm:cols:ragged', 'nan_rows:lanes:partial',
    'nan_rows:lanes:two_trips', 'nan_rows:lanes:several_trips', 'embed:one_token', 'embed:partial_wave', 'embed:one_wave',
    'embed:two_waves', 'embed:all_waves', 'glu:grid_capped',
}
SIZES = ('below', 'at', 'above', 'grid_capped', 'float32', 'bfloat16')
PATHS |= {'%s:%s' % (op, s) for op in ('dropout', 'dropout_add') for s in SIZES + ('p0', 'p0.1', 'p0.999')}
PATHS |= {'%s:%s' % (op, s) for op in ('cast', 'axpy', 'relu_bwd', 'sum_n') for s in SIZES}
PATHS |= {'%s:count:%s' % (op, s) for op in ('gather', 'scatter') for s in ('null', 'zero', 'below', 'above')}


def test_every_dispatch_path_is_reached_and_every_case_is_needed():
    """the paths are named by functions of small_ref that restate the entry points' dispatch conditions; a case stays in its
    table only if it names a mutant or reaches a path that no earlier case of the table reaches"""
    seen = set()
    for fam, (cases, _, paths) in FAMILIES.items():
        for case in cases:
            p = paths(case)
            assert case['mutants'] or (p - seen), 'case %s %s is not needed' % (fam, case['id'])
            seen |= p
    assert PATHS <= seen, sorted(PATHS - seen)


def test_the_multi_tables_make_a_second_launch():
    assert ref.WN_MULTI_N > 32 and ref.CSM_N > 48 and ref.TRM_N > 48
    for pat in ref.WN_MULTI_STORE.values():                       # a store bit whose global and per-launch indices disagree
        assert any(j >= 32 and (j - 32) not in pat for j in pat) or any(j < 4 and (j + 32) not in pat for j in pat)


def test_pinned_constants():
    """four times the measured ratio, rounded up to a power of two; 2^-10 where the ratio never left u_out |ref|"""
    for k, v in ref.MEASURED.items():
        assert k in ref.GROUPS
        assert ref.C[k] == (2.0 ** -10 if v <= 0 else 2.0 ** np.ceil(np.log2(4 * v)))
    assert set(ref.MEASURED) <= set(ref.GROUPS)
