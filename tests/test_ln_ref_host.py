"""tests/ln_ref.py on the CPU: the fp32 emulation of every LayerNorm kernel stays inside every bound at
c = 1 on every case of every table, every mutant breaks a bound or an exact comparison on a case that names it, every dispatch
path the entry points have is reached by a case, and no case is in a table without a path or a mutant that needs it."""
import numpy as np
import pytest

import ln_ref as ref

F32, F64 = np.float32, np.float64


def stored(outs):
    """what a kernel computing `outs` would leave in memory"""
    return {k: ref.store(o.value, o.dtype) for k, o in outs.items()}


def broken(got, want, pinned=False):
    """{output: elements outside what the reference allows}: at c = 1 (the emulation), or - pinned, for a mutant - at the
    larger of 1 and the pinned constant, the bound the GPU test uses"""
    assert set(got) == set(want)
    c = lambda o: max(1.0, ref.C.get(o.group, 0.0)) if pinned else 1.0                          # noqa: E731
    bad = {k: ref.failures(got[k], want[k], c(want[k])) for k in want}
    return {k: v for k, v in bad.items() if v}


def _runs(fn, case, mutant):
    """the reference on the statistics the emulated forward stored, against the emulation or a mutant"""
    emu = fn(case, F32)
    stats = None
    if 'mean' in emu:
        stats = (ref.store(emu['mean'].value, 'float32'), ref.store(emu['rstd'].value, 'float32'))
    want = fn(case, F64, None, stats)
    got = emu if mutant is None else fn(case, F32 if mutant in ref.FP32_MUTANTS else F64, mutant, stats)
    return want, stored(got)


def ln_runs(case, mutant=None):
    yield _runs(ref.ln_case, case, mutant)


def cat_runs(case, mutant=None):
    yield _runs(ref.cat_case, case, mutant)


def rows_runs(case, mutant=None):
    yield ref.rows_case(case), stored(ref.rows_case(case, F32 if mutant is None else F64, mutant))


FAMILIES = {
    'ln': (ref.LN, ln_runs, ref.ln_paths),
    'cat': (ref.CAT, cat_runs, ref.cat_paths),
    'rows': (ref.ROWS, rows_runs, ref.rows_paths),
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
    'fwd:generic:ragged', 'fwd:generic:nch3', 'fwd:generic:nch>4', 'fwd:generic:ld', 'fwd:generic:ptr_x', 'fwd:generic:ptr_res',
    'fwd:generic:ptr_y', 'fwd:vec:nch1', 'fwd:vec:nch2', 'fwd:vec:nch4', 'fwd:rows2',
    'bwd:generic:ragged', 'bwd:generic:nch3', 'bwd:generic:nch>4:lds64k', 'bwd:generic:bf16_nch4:lds64k', 'bwd:generic:ld',
    'bwd:generic:ptr_x', 'bwd:generic:ptr_res', 'bwd:generic:ptr_dy', 'bwd:generic:ptr_dx', 'bwd:generic:ptr_dres',
    'bwd:vec:nch1', 'bwd:vec:nch2', 'bwd:vec:nch4',
    'ln:float32', 'ln:bfloat16', 'ln:res', 'ln:no_res', 'ln:p0', 'ln:dropout', 'ln:eps', 'ln:eps_small', 'ln:ld>C', 'ln:ld=C',
    'ln:last_block:1_rows', 'ln:last_block:2_rows', 'ln:last_block:3_rows', 'ln:last_block:4_rows', 'ln:one_block',
    'ln:several_blocks', 'ln:option:None', 'ln:option:0', 'ln:option:-1',
    'bwd:outs:both', 'bwd:outs:dx', 'bwd:outs:dres', 'bwd:dres_acc0', 'bwd:dres_acc1', 'bwd:dparam_acc0', 'bwd:dparam_acc1',
    'bwd:dgamma_null', 'finish:groups_empty', 'finish:remainder_only', 'finish:unrolled_for_some', 'finish:unrolled',
    'finish:unrolled+remainder',
    'cat:nch1', 'cat:nch2', 'cat:n=1', 'cat:n', 'cat:n=max', 'cat:ld_y>nC', 'cat:ld_y=nC', 'cat:p0', 'cat:dropout',
    'cat:salts:equal', 'cat:salts:distinct', 'cat:dx_null', 'cat:dx_all', 'cat:dres_null', 'cat:dres', 'cat:dgamma_null',
    'cat:finish', 'cat:last_block:1_rows', 'cat:last_block:4_rows', 'cat:one_block', 'cat:several_blocks',
    'cat:finish:groups_empty', 'cat:finish:unrolled_for_some',
    'rows:float4_per_thread:1', 'rows:float4_per_thread:2', 'rows:float4_per_thread:3', 'rows:float4_per_thread:4',
    'rows:ld_x>C', 'rows:ld_x=C', 'rows:ld_y>C', 'rows:ld_y=C', 'rows:stats_null', 'rows:stats', 'rows:one_row',
    'rows:several_rows',
}


def test_every_dispatch_path_is_reached_and_every_case_is_needed():
    """the paths are named by functions of ln_ref that restate the launchers' dispatch conditions; a case stays in its table
    only if it names a mutant or reaches a path that no earlier case of the table reaches"""
    seen = set()
    for fam, (cases, _, paths) in FAMILIES.items():
        for case in cases:
            p = paths(case)
            assert case['mutants'] or (p - seen), 'case %s %s is not needed' % (fam, case['id'])
            seen |= p
    assert PATHS <= seen, sorted(PATHS - seen)


def test_the_demotions_name_their_cause_and_the_row_threshold_its_path():
    by = {c['id']: c for c in ref.LN}
    assert ref.ln_fwd_path(by['d_ld1028']) == 'fwd:generic:ld' and ref.ln_bwd_path(by['d_ld1028']) == 'bwd:generic:ld'
    for who in ('x', 'res', 'y'):
        assert ref.ln_fwd_path(by['d_%s_off' % who]) == 'fwd:generic:ptr_' + who
    for who in ('dy', 'dx', 'dres'):
        assert ref.ln_fwd_path(by['d_%s_off' % who]).startswith('fwd:vec')
        assert ref.ln_bwd_path(by['d_%s_off' % who]) == 'bwd:generic:ptr_' + who
    assert ref.ln_bwd_path(by['d_y_off']).startswith('bwd:vec')
    assert ref.ln_fwd_path(by['v_ld1032']) == 'fwd:vec:nch2' and ref.ln_bwd_path(by['v_ld1032']) == 'bwd:vec:nch2'
    assert ref.ln_fwd_path(by['v_bf16_2048']) == 'fwd:vec:nch4'
    assert ref.ln_bwd_path(by['v_bf16_2048']) == 'bwd:generic:bf16_nch4:lds64k'
    assert ref.ln_fwd_path(by['r2_4095']) == 'fwd:vec:nch2' and ref.ln_fwd_path(by['r2_4096_var0']) == 'fwd:vec:nch2'
    for k in ('r2_4096', 'r2_4097_p', 'r2_4097_nores'):
        assert ref.ln_fwd_path(by[k]) == 'fwd:rows2'
    assert [ref.finish_walk(nb) for nb in (1, 15, 16, 17, 48, 49, 64, 65, 113)] == [
        'groups_empty', 'groups_empty', 'remainder_only', 'remainder_only', 'remainder_only', 'unrolled_for_some', 'unrolled',
        'unrolled+remainder', 'unrolled+remainder']


def test_pinned_constants():
    """four times the measured ratio, rounded up to a power of two; 2^-10 where the ratio never left u_out |ref|.  A measured
    ratio above 1 would mean an error the derived gamma does not count: a finding, not a number to pin over"""
    for k, v in ref.MEASURED.items():
        assert k in ref.GROUPS and v <= 1.0
        assert ref.C[k] == (2.0 ** -10 if v <= 0 else 2.0 ** np.ceil(np.log2(4 * v)))
