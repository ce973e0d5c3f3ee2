"""tests/adaptive_ref.py on the CPU: the fp32 emulation of every kernel stays inside every bound at
c = 1 on every case of every table and equals the reference bit for bit where the output is exact, every mutant breaks a
bound or an exact comparison on a case that names it, every path the launchers and kernels have is reached by a case, no
case is in a table without a path or a mutant that needs it, no judged element of the cross entropy is skipped, and each
family agrees with torch on the CPU in float64."""
import numpy as np
import pytest
import torch

import adaptive_ref as ref

F32, F64 = np.float32, np.float64
OUTS = ('bfloat16', 'float32')


def stored(outs):
    """what a kernel computing `outs` would leave in memory"""
    return {k: ref.store(o.value, o.dtype) for k, o in outs.items()}


def broken(got, want, pinned=False):
    """{output: elements outside what the reference allows}.  Measured groups: at c = 1 (the emulation), or - pinned, for a
    mutant - at the larger of 1 and the pinned constant, the bound the GPU test uses"""
    assert set(got) == set(want)
    c = lambda o: None if o.group in (None, 'exact') else (max(1.0, ref.C.get(o.group, 0.0)) if pinned else 1.0)   # noqa: E731
    bad = {k: ref.failures(got[k], want[k], c(want[k])) for k in want}
    return {k: v for k, v in bad.items() if v}


def part_runs(case, mutant=None):
    yield ref.part_case(case), stored(ref.part_case(case, mutant))


def typed_runs(fn):
    def runs(case, mutant=None):
        for dty in OUTS:
            yield fn(case, dty), stored(fn(case, dty, F32 if mutant is None else F64, mutant))
    return runs


def ce_runs(case, mutant=None):
    for dty in OUTS:
        emu = ref.ce_case(case, dty, F32)
        lse = ref.store(emu['lse'].value, 'float32')
        yield ref.ce_case(case, dty, F64, None, lse), stored(emu if mutant is None else ref.ce_case(case, dty, F64, mutant, lse))


def plain_runs(fn):
    def runs(case, mutant=None):
        yield fn(case), stored(fn(case, F32 if mutant is None else F64, mutant))
    return runs


FAMILIES = {
    'partition': (ref.PART, part_runs, ref.part_paths),
    'finalize': (ref.FIN, typed_runs(ref.fin_case), ref.fin_paths),
    'table_grad': (ref.TG, typed_runs(ref.tg_case), ref.tg_paths),
    'ce': (ref.CE, ce_runs, ref.ce_paths),
    'sum': (ref.SUM, plain_runs(ref.sum_case), ref.sum_paths),
    'step': (ref.STEP, plain_runs(ref.step_case), ref.step_paths),
}
CASES = [(f, c) for f, (cases, _, _) in FAMILIES.items() for c in cases]
IDS = ['%s-%s' % (f, c['id']) for f, c in CASES]


@pytest.mark.parametrize('fam,case', CASES, ids=IDS)
def test_fp32_emulation_is_inside_every_bound_at_c_1_and_exact_where_the_output_is(fam, case):
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


def test_the_order_of_the_duplicates_is_held_by_the_exact_comparison():
    """adding a table row's band rows in decreasing order stays inside the float64 bound (k = m) and breaks demb_bits"""
    case = next(c for c in ref.TG if 'tg_decreasing_order' in c['mutants'])
    want, got = ref.tg_case(case, 'float32'), stored(ref.tg_case(case, 'float32', F64, 'tg_decreasing_order'))
    assert ref.failures(got['demb_bits'], want['demb_bits']) > 0
    assert ref.failures(got['demb'], want['demb']) == 0


PATHS = {
    'part:refused:bands0', 'part:refused:bands5', 'part:N<=0', 'part:bands1', 'part:bands2', 'part:bands3', 'part:bands4',
    'part:chunks:one', 'part:chunks:carried', 'part:last_chunk:whole', 'part:last_chunk:partial_wave', 'part:last_chunk:ragged',
    'part:pad_idx:-1', 'part:pad_idx:token', 'part:null:none', 'part:null:slot', 'part:null:head_target', 'part:null:n_valid',
    'part:pads:none', 'part:pads:some', 'part:pads:all', 'part:ids:outside_every_band', 'part:band:empty',
    'part:band:owns_a_chunk', 'part:band:second_chunk_only', 'part:ballot:mixed', 'part:ballot:full',
    'fin:E<256', 'fin:E=256', 'fin:E%256=0', 'fin:E>256:ragged', 'fin:tbc0', 'fin:tbc1', 'fin:B1', 'fin:B>1', 'fin:T1', 'fin:T>1',
    'fin:scale:one', 'fin:scale:sqrt', 'fin:start_pos:0', 'fin:start_pos:>0', 'fin:clamped', 'fin:in_table',
    'tg:grid:cap', 'tg:grid:clamped', 'tg:c0:one_trip', 'tg:c0:second_trip', 'tg:dim%256=0', 'tg:dim<256', 'tg:dim%256:ragged',
    'tg:ld>dim', 'tg:ld=dim', 'tg:count:zero', 'tg:count:one', 'tg:count:inside', 'tg:count:equal', 'tg:count:above',
    'tg:padding_idx:-1', 'tg:padding_idx:row', 'tg:duplicates', 'tg:owner_not_row0', 'tg:list_crosses_chunk',
    'tg:list_longer_than_chunk', 'tg:padding_row_inside_run',
    'ce:trips:partial', 'ce:trips:one', 'ce:trips:two_ragged', 'ce:trips:many_ragged', 'ce:m_dev:null', 'ce:m_dev:zero',
    'ce:m_dev:inside', 'ce:m_dev:equal', 'ce:m_dev:above', 'ce:row_idx:null', 'ce:row_idx:perm', 'ce:logits:random',
    'ce:logits:spread', 'ce:logits:equal', 'ce:logits:offset', 'ce:logits:dominated', 'ce:logits:neginf', 'ce:gscale:one',
    'ce:gscale:1/37', 'ce:gscale:zero', 'ce:ld>V', 'ce:ld=V', 'ce:rows:one', 'ce:rows:several', 'ce:ignored_target:head',
    'ce:ignored_target:tail', 'ce:target:first', 'ce:target:last',
    'sum:n:zero', 'sum:n:one', 'sum:n:partial_wave', 'sum:n:ragged', 'sum:n:one_trip', 'sum:n:second_trip:one_thread',
    'sum:n:many_trips', 'sum:m_dev:null', 'sum:m_dev:zero', 'sum:m_dev:below', 'sum:m_dev:above', 'sum:acc0', 'sum:acc1',
    'sum:cancel', 'sum:plain',
    'step:bands1', 'step:bands3', 'step:bands4', 'step:ktot:one_trip', 'step:ktot:second_trip', 'step:E:ragged',
    'step:E:whole_trip', 'step:E:second_trip', 'step:counter:none', 'step:counter:registered', 'step:id:pad',
    'step:id:outside_every_band', 'step:pos:clamped', 'step:band_not_at_column0',
}


def test_every_path_is_reached_and_every_case_is_needed():
    """the paths are named by functions of adaptive_ref that restate the launchers' and the kernels' branch conditions; a
    case stays in its table only if it names a mutant or reaches a path that no earlier case of the table reaches"""
    seen = set()
    for fam, (cases, _, paths) in FAMILIES.items():
        for case in cases:
            p = paths(case)
            assert case['mutants'] or (p - seen), 'case %s %s is not needed' % (fam, case['id'])
            seen |= p
    assert PATHS <= seen, sorted(PATHS - seen)


def test_the_tables_hold_the_shapes_the_kernels_branch_on():
    assert {c['N'] for c in ref.PART} >= {1, 63, 64, 65, 1023, 1024, 1025, 2049, 3000}
    assert {(c['B'], c['T']) for c in ref.FIN} == {(1, 1), (1, 7), (5, 1), (3, 4)}
    assert {c['E'] for c in ref.FIN} == {1, 255, 256, 257, 1024}
    assert {c['dim'] for c in ref.TG} >= {1, 255, 256, 1023, 1024, 1025, 1300}
    assert {c['cap'] for c in ref.TG} == {1, 5, 1024, 1100, 2100}
    assert {c['V'] for c in ref.CE} == {1, 2, 255, 256, 257, 600, 5002, 8195} and {c['M'] for c in ref.CE} == {1, 3, 70}
    assert next(c for c in ref.CE if c['V'] == 5002)['ld'] == 5004
    assert {c['n'] for c in ref.SUM} == {0, 1, 63, 1023, 1024, 1025, 5000}
    assert {c['E'] for c in ref.STEP} == {4, 1020, 1024, 1028} and {ref.step_bands(c)[4] for c in ref.STEP} == {88, 2056}
    case = next(c for c in ref.TG if c['pat'] == 'pairs')         # the pairs sit inside the count, 1023 / 1024 / 1025 apart
    local = ref.tg_inputs(case, 'float32')['local']
    for first, dist in ref.TG_PAIRS:
        assert first + dist < case['count'] and local[first] == local[first + dist]
        assert (local[:case['count']] == local[first]).sum() == 2


@pytest.mark.parametrize('case', ref.CE, ids=[c['id'] for c in ref.CE])
def test_no_judged_element_of_the_cross_entropy_is_skipped(case):
    """every reference value is finite; ratio() skips nothing of lse and loss among the live rows, and of dlogits only what is
    zero by definition (an ignored row, gscale = 0, the probability of a -inf logit) - compared against zero instead"""
    x, M = ref.ce_inputs(case), case['M']
    live = np.arange(M) < (M if case['m'] is None else min(case['m'], M))
    for dty in OUTS:
        want = ref.ce_case(case, dty)
        for o in want.values():
            assert np.isfinite(np.asarray(o.value, F64)).all()
        assert not ref.skipped(want['lse']).any() and not ref.skipped(want['loss']).any()
        zero = (ref.ce_zero_rows(case)[:, None] | np.isneginf(x['logits'])) & live[:, None]
        assert np.array_equal(ref.skipped(want['dlogits']), zero)
        assert (np.asarray(want['dlogits'].value)[zero] == 0).all()
    tg = x['targets']
    assert (tg >= 0).all() and (tg < case['V']).all() and (case['V'] == 1 or ref.CE_IGNORE < case['V'])
    assert x['row_idx'] is None or sorted(x['row_idx']) == list(range(M))
    assert np.isfinite(x['logits'][np.arange(M), ref.ce_targets(tg, x['row_idx'], M)]).all()


def test_every_index_of_every_case_and_mutant_is_in_range():
    for case in ref.PART:
        for mutant in (None,) + case['mutants']:
            o, N = ref.part_case(case, mutant), max(case['N'], 1)
            for k, top in (('rows', N), ('slot', max(case['nb'], 1) * N)):
                if k in o:
                    v = o[k].value[o[k].value != ref.SENTINEL]
                    assert ((v >= 0) & (v < top)).all()
    for case in ref.FIN:
        x = ref.fin_inputs(case, 'float32')
        assert sorted(set(x['slot'])) == sorted(x['slot']) and x['slot'].max() < 3 * case['B'] * case['T']
        assert ref.FIN_PAD + 1 + case['T'] - 1 + case['start'] < ref.FIN_TABLE_ROWS
    for case in ref.TG:
        x = ref.tg_inputs(case, 'float32')
        assert x['local'].min() >= 0 and x['local'].max() < x['demb0'].shape[0] and x['drows'].shape[0] >= case['count']
    for case in ref.STEP:
        lo, hi, dim, off, ktot = ref.step_bands(case)
        assert all(o + d <= ktot and o % 8 == 0 and d % 8 == 0 for o, d in zip(off, dim)) and ktot % 8 == 0


# ---------------------------------------------------------------- one cross-check per family against torch in float64
def test_partition_against_torch():
    case = next(c for c in ref.PART if c['N'] == 3000)
    ids, cut, N = torch.from_numpy(ref.part_inputs(case)['ids']), ref.part_cut(case), case['N']
    o = ref.part_case(case)
    for b in range(case['nb']):
        lo = 0 if b == 0 else cut[b - 1]
        rows = torch.nonzero((ids >= lo) & (ids < cut[b])).flatten()
        assert o['count'].value[b] == rows.numel()
        assert np.array_equal(o['rows'].value[b, :rows.numel()], rows.numpy())
        assert np.array_equal(o['local'].value[b, :rows.numel()], (ids[rows] - lo).numpy())
        assert (o['rows'].value[b, rows.numel():] == ref.SENTINEL).all()
        assert np.array_equal(o['slot'].value[rows.numpy()], b * N + np.arange(rows.numel()))
    assert o['n_valid'].value[0] == int((ids != case['pad']).sum())
    outside = ((ids < 0) | (ids >= cut[-1])).numpy()
    assert outside.any() and (o['slot'].value[outside] == ref.SENTINEL).all() and (o['head_target'].value[~outside] >= 0).all()


def test_finalize_against_torch():
    case = next(c for c in ref.FIN if c['id'] == 'b3_t4_e257_tbc')
    x, B, T, E = ref.fin_inputs(case, 'float32'), case['B'], case['T'], case['E']
    t64 = lambda a: torch.from_numpy(np.asarray(a, F64))                                   # noqa: E731
    ids = torch.from_numpy(x['ids']).reshape(B, T)
    pos = torch.where(ids == ref.FIN_PAD, ref.FIN_PAD, ref.FIN_PAD + 1 + torch.arange(T)[None, :] + case['start'])
    emb = t64(x['band_out'])[torch.from_numpy(x['slot']).long()].reshape(B, T, E)
    want = (float(np.float32(ref.fin_scale(case))) * emb + t64(x['pos_table'])[pos]).transpose(0, 1).reshape(B * T, E)
    got = ref.fin_case(case, 'float32')
    assert np.abs(got['out'].value - want.numpy()).max() < 1e-12
    back = torch.zeros(3 * B * T, E, dtype=torch.float64)
    back[torch.from_numpy(x['slot']).long()] = float(np.float32(ref.fin_scale(case))) * \
        t64(x['dout']).reshape(T, B, E).transpose(0, 1).reshape(B * T, E)
    named = ~got['dband'].exact_at
    assert np.abs(got['dband'].value - back.numpy())[named].max() < 1e-12
    assert ref.same_bits(got['dband'].value[~named], x['dband0'][~named])


def test_table_grad_against_index_add():
    for case in ref.TG:
        x = ref.tg_inputs(case, 'float32')
        n = min(case['count'], case['cap'])
        local, d = torch.from_numpy(x['local'][:n]).long(), torch.from_numpy(np.asarray(x['drows'][:n], F64))
        keep = local != case['pad']
        want = torch.from_numpy(np.asarray(x['demb0'], F64)).index_add_(0, local[keep], d[keep])
        assert np.abs(ref.tg_case(case, 'float32')['demb'].value - want.numpy()).max() < 1e-10, case['id']


def test_cross_entropy_against_torch():
    for case in ref.CE:
        x, M = ref.ce_inputs(case), case['M']
        Me = M if case['m'] is None else min(case['m'], M)
        tg = ref.ce_targets(x['targets'], x['row_idx'], M)
        logits = torch.from_numpy(np.asarray(x['logits'], F64)).requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(tg).long(), ignore_index=ref.CE_IGNORE,
                                                 reduction='none')
        want = ref.ce_fwd(x['logits'], x['targets'], x['row_idx'], case['m'], ref.CE_IGNORE)
        assert np.abs(want['loss'].value - loss.detach().numpy())[:Me].max(initial=0) < 1e-9, case['id']
        assert np.abs(want['lse'].value - torch.logsumexp(logits, 1).detach().numpy())[:Me].max(initial=0) < 1e-9
        assert (want['loss'].value[Me:] == 0).all() and (want['lse'].value[Me:] == 0).all()
        g = ref.CE_G[case['g']]
        (loss[:Me].sum() * g).backward()
        back = ref.ce_bwd(x['logits'], x['targets'], x['row_idx'], case['m'], ref.CE_IGNORE, want['lse'].value, g, 'float32')
        assert np.abs(back['dlogits'].value - logits.grad.numpy())[:Me].max(initial=0) < 1e-9, case['id']
        assert (back['dlogits'].value[Me:] == ref.SENTINEL).all()


def test_sum_against_torch():
    for case in ref.SUM:
        x = ref.sum_inputs(case)
        ne = case['n'] if case['m'] is None else min(case['n'], case['m'])
        want = float(torch.from_numpy(np.asarray(x['x'][:ne], F64)).sum()) + (x['out0'] if case['acc'] else 0.0)
        assert abs(float(ref.sum_case(case)['out'].value[0]) - want) < 1e-9, case['id']


def test_step_embedding_against_torch():
    for case in ref.STEP:
        x, (lo, hi, dim, off, ktot) = ref.step_inputs(case), ref.step_bands(case)
        got = ref.step_case(case)
        ids = torch.from_numpy(x['ids'])
        cat = torch.zeros(case['M'], ktot, dtype=torch.float64)
        for b in range(case['nb']):
            rows = torch.nonzero((ids >= lo[b]) & (ids < hi[b])).flatten()
            emb = torch.nn.functional.embedding(ids[rows] - lo[b], torch.from_numpy(np.asarray(x['tables'][b], F64)))
            cat[rows, off[b]:off[b] + dim[b]] = emb
        assert np.array_equal(got['cat'].value, cat.numpy())
        pos = torch.where(ids == ref.STEP_PAD, ref.STEP_PAD, ref.STEP_PAD + 1 + case['start'] + (case['step'] or 0))
        pos = pos.clamp(max=ref.STEP_POS_ROWS - 1)
        prow = torch.from_numpy(x['pos_table'])[pos]
        assert np.array_equal(got['pos_out'].value, prow.numpy())
        known = (ids >= 0) & (ids < hi[-1])
        emb = torch.from_numpy(np.asarray(x['table'], F64))[ids.clamp(0, hi[-1] - 1)] * known[:, None]
        assert np.abs(got['out'].value - (emb + prow.double()).numpy()).max() < 1e-12


def test_pinned_constants():
    """four times the measured ratio, rounded up to a power of two; 2^-10 where the ratio never left u_out |ref|"""
    for k, v in ref.MEASURED.items():
        assert k in ref.GROUPS
        assert ref.C[k] == (2.0 ** -10 if v <= 0 else 2.0 ** np.ceil(np.log2(4 * v)))
