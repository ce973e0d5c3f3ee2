"""tests/attn_ref.py on the CPU: the float64 reference against an independent torch float64
formulation, the fp32 emulation of every attention path inside every bound at c = 1 on every case, every mutant outside a bound
or an exact comparison on the cases that name it and inside on the cases that say it must not show, every dispatch path reached,
no case without a reason, no element outside a comparison, and the coverage facts the tables promise."""
import numpy as np
import pytest
import torch

import attn_ref as ref

F32, F64 = np.float32, np.float64
ALL = ref.CASES + ref.AVG
IDS = [c['id'] for c in ALL]


def emulated_forward(case):
    return ref.cached(('attn_emu', case['id']), lambda: ref.attn_fwd_tiled(case, F32))


def broken(got, want, pinned=False):
    """{output: elements outside what the reference allows}: at c = 1 (the emulation), or - pinned, for a mutant - at the larger
    of 1 and the pinned constant"""
    bad = {}
    for k, o in want.items():
        if isinstance(o, ref.Out):
            c = max(1.0, ref.C.get(o.group, 0.0)) if pinned else 1.0
            n = ref.failures(got[k], o, c)
            if n:
                bad[k] = n
    return bad


def runs(case, mutant=None):
    """-> (want, got) pairs of one case: the forward; the backward on what the emulated forward stored; the weights"""
    if case in ref.AVG:
        lse = emulated_forward(case)['lse']
        want = ref.avg_weights(case, lse)
        if mutant is None:
            got = ref.avg_weights(case, lse, F32)
        elif mutant in ref.W_MUTANTS:
            got = ref.avg_weights(case, lse, F64, mutant)
        else:                                        # a key mutant: the forward that made lse is the wrong one
            pr_lse = ref.store(ref.attn_fwd(case, mutant)['lse'].value, 'float32')
            got = ref.avg_weights(case, pr_lse)
        yield {'w': want}, {'w': ref.store(got.value, 'float32')}
        return
    emu = emulated_forward(case)
    fwd_mut = mutant is not None and mutant not in ref.BWD_MUTANTS
    if mutant is None or fwd_mut:
        want = ref.fwd_case(case)
        if mutant is None:
            got = emu
        elif mutant in ref.TILED_MUTANTS:
            got = ref.attn_fwd_tiled(case, ref.TILED_MUTANTS[mutant], mutant)
        else:
            got = ref.stored(ref.attn_fwd(case, mutant))
        yield {k: want[k] for k in ('out', 'lse')}, got
    if case['bwd'] and (mutant is None or not fwd_mut or mutant in ref.KEY_MUTANTS + ref.DROP_MUTANTS):
        if mutant in ('dropout_scales_lse',):
            return
        want = ref.attn_bwd(case, emu['out'], emu['lse'])
        if mutant is None:
            got = ref.attn_bwd_tiled(case, emu['out'], emu['lse'], F32)
        else:
            got = ref.stored(ref.attn_bwd(case, emu['out'], emu['lse'], mutant))
        yield want, got


@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_fp32_emulation_is_inside_every_bound_at_c_1(case):
    for want, got in runs(case):
        assert not broken(got, want), case['id']


@pytest.mark.parametrize('case', [c for c in ALL if c['mutants'] or c['not_caught']],
                         ids=[c['id'] for c in ALL if c['mutants'] or c['not_caught']])
def test_every_mutant_is_caught_on_the_cases_that_name_it_and_not_where_it_must_not_show(case):
    for mutant in case['mutants']:
        assert mutant in ref.MUTANTS
        assert any(broken(got, want, pinned=True) for want, got in runs(case, mutant)), '%s survives %s' % (mutant, case['id'])
    for mutant in case['not_caught']:
        assert mutant in ref.MUTANTS
        assert not any(broken(got, want, pinned=True) for want, got in runs(case, mutant)), '%s shows on %s' % (mutant, case['id'])


def _bias_key_masked(c):
    m = ref.key_mask(c)
    return bool(c['bias'] and m is not None and m[1:, 0].any())


def _masks_differ(c):
    m = ref.key_mask(c)
    return m is not None and bool((m != np.roll(m, -1, 0)).any())


# the class of cases on which a mutant must NOT show, as a condition on the case (St, QB, kernel); every case of the class is run
SILENT_ON = {
    'drop_last_key': lambda c, St, QB, k: c['S'] == St and c['mask'] in ('ragged', 'sample0', 'first_only') and c['S'] > 1,
    'tail_key_live': lambda c, St, QB, k: St % 32 == 0,
    'no_zero_key': lambda c, St, QB, k: not c['zero'],
    'bias_v_as_bias_k': lambda c, St, QB, k: not c['bias'],
    'bias_masked': lambda c, St, QB, k: not _bias_key_masked(c),
    'mask_of_other_sample': lambda c, St, QB, k: not _masks_differ(c),
    'head_swap': lambda c, St, QB, k: c['H'] == 1,
    'drop_second_tile64': lambda c, St, QB, k: St <= 64,
    'drop_odd_tile': lambda c, St, QB, k: k != 'self',
    'ksplit_wave3_lost': lambda c, St, QB, k: QB > 1 or St <= 96,
    'no_rescale': lambda c, St, QB, k: c['profile'] == 'descending' and c['mask'] == 'tile64',
    'lazy_max_never_moves': lambda c, St, QB, k: k != 'self' or c['profile'] in ('step7.9', 'descending'),
    'keep_pair_swapped': lambda c, St, QB, k: St % 2 == 1 or not c['p'],
    'keep_quad_rotated': lambda c, St, QB, k: St % 4 != 0 or k not in ('reg', 'self') or not c['p'],
    'keep_index_without_head': lambda c, St, QB, k: not c['p'],
    'dropout_scales_lse': lambda c, St, QB, k: not c['p'],
    'bwd_delta_without_keep': lambda c, St, QB, k: not c['p'],
    'bwd_dk_last_qblock_only': lambda c, St, QB, k: QB == 1,
    'bwd_second_wave_lost': lambda c, St, QB, k: ref.bwd_shape(c)[1] == 1 or St <= 32,
    'dbias_not_summed_over_t': lambda c, St, QB, k: not c['bias'] or c['Tq'] == 1,
    'dv_from_undropped_p': lambda c, St, QB, k: not c['p'],
    'avg_w_not_divided_by_H': lambda c, St, QB, k: c['H'] == 1,
}


def silent_class(mutant):
    table = ref.AVG if mutant in ref.W_MUTANTS else ALL
    if mutant in ref.BWD_MUTANTS:
        table = [c for c in ref.CASES if c['bwd']]
    return [c for c in table if SILENT_ON[mutant](c, *ref.sizes(c), ref.fwd_kernel(c)[0])]


@pytest.mark.parametrize('mutant', sorted(SILENT_ON))
def test_a_mutant_stays_inside_every_bound_on_every_case_of_its_silent_class(mutant):
    """not a property of the table: the mutant is run on every case of the class and must leave no bound and no exact comparison"""
    cases = silent_class(mutant)
    assert cases, mutant
    for c in cases:
        assert mutant not in c['mutants'], (mutant, c['id'])
        assert not any(broken(got, want, pinned=True) for want, got in runs(c, mutant)), '%s shows on %s' % (mutant, c['id'])


def test_lse_base2_moves_lse_and_nothing_else():
    """the one mutant without a silent class of cases: on every case out (and, through the stored lse, nothing else of the forward)
    stays inside its bound while lse leaves it wherever a row's lse is not 0 or +inf"""
    for c in ref.CASES:
        for want, got in runs(c, 'lse_base2'):
            assert set(broken(got, want, pinned=True)) <= {'lse'}, c['id']


def test_every_mutant_is_named_by_a_case_and_has_a_class_that_must_not_catch_it():
    named = {m for c in ALL for m in c['mutants']}
    assert named == set(ref.MUTANTS), set(ref.MUTANTS) ^ named
    assert len(set(ref.MUTANTS)) == len(ref.MUTANTS)
    assert set(SILENT_ON) == set(ref.MUTANTS) - {'lse_base2'}
    silent = {m for c in ALL for m in c['not_caught']}
    assert silent == set(SILENT_ON), silent ^ set(SILENT_ON)          # each also has a NAMED case that must not notice
    for c in ALL:
        for m in c['not_caught']:
            assert c in silent_class(m), (m, c['id'])
    by = {c['id']: c for c in ALL}
    # one backward launch shape per NW that has a second wave
    nws = {ref.bwd_shape(c)[0] for c in ALL if 'bwd_second_wave_lost' in c['mutants']}
    assert {'bwd_bf16_nw2', 'bwd_bf16_nw4', 'bwd_f32'} <= nws
    # the classes that must not notice, stated as conditions on the case
    for c in ALL:
        St, QB = ref.sizes(c)
        kern = ref.fwd_kernel(c)[0]
        for m in c['mutants']:
            assert not (m == 'keep_pair_swapped' and St % 2), c['id']
            assert not (m == 'keep_quad_rotated' and (St % 4 or kern not in ('reg', 'self'))), c['id']
            assert not (m == 'drop_second_tile64' and St <= 64), c['id']
            assert not (m == 'drop_odd_tile' and kern != 'self'), c['id']
            assert not (m == 'bwd_dk_last_qblock_only' and QB == 1), c['id']
            assert not (m == 'lazy_max_never_moves' and c['profile'] not in ('staircase', 'jump', 'cliff')), c['id']
            assert not (m == 'tail_key_live' and St % 32 == 0), c['id']
            assert not (m == 'ksplit_wave3_lost' and (QB > 1 or St <= 96)), c['id']
            assert not (m in ref.DROP_MUTANTS and not c['p']), c['id']
    assert by['s97_s128_79']['not_caught'] == ('lazy_max_never_moves',)


PATHS = {
    'fwd_bf16:ksplit:nkt<nw:nodrop', 'fwd_bf16:ksplit:nkt<nw:pair', 'fwd_bf16:ksplit:nkt<nw:single', 'fwd_bf16:ksplit:nkt>=nw:pair',
    'fwd_bf16:ksplit:nkt>=nw:single', 'fwd_bf16:ksplit:nkt>=nw:nodrop', 'fwd_bf16:qblocks:nodrop', 'fwd_bf16:qblocks:pair',
    'fwd_bf16:qblocks:single', 'fwd_f32:ksplit:nkt<nw:nodrop', 'fwd_f32:ksplit:nkt>=nw:single', 'fwd_f32:qblocks:single',
    'fwd_f32:qblocks:nodrop', 'fwd_bf16_d16:ksplit:nkt<nw:single', 'fwd_bf16_d16:qblocks:nodrop', 'fwd_f32_d16:qblocks:single',
    'fwd_f32_d16:ksplit:nkt<nw:pair',
    'reg:occ2:quad', 'reg:occ2:pair', 'reg:occ2:single', 'reg:occ2:nodrop', 'reg:occ3:quad', 'reg:occ3:nodrop',
    'tile64_f32:single', 'tile64_f32:nodrop', 'tile64_f32:pair', 'tile64_bf16:pair', 'tile64_bf16:nodrop', 'tile64_bf16:single',
    'self:regs:quad', 'self:regs:nodrop', 'self:dma:quad', 'self:dma:nodrop',
    'bwd_bf16_nw1:qb1:nodrop:dbias_two', 'bwd_bf16_nw1:qb1:pair:dbias_one', 'bwd_bf16_nw1:qb1:single:dbias_none',
    'bwd_bf16_nw1:qb1:pair:dbias_none', 'bwd_bf16_nw2:qb1:single:dbias_one', 'bwd_bf16_nw2:qb1:pair:dbias_none',
    'bwd_bf16_nw4:qb1:single:dbias_two', 'bwd_bf16_nw2:qb>1:nodrop:dbias_two', 'bwd_bf16_nw2:qb>1:single:dbias_none',
    'bwd_bf16_nw2:qb>1:pair:dbias_one', 'bwd_bf16_nw4:qb>1:pair:dbias_none', 'bwd_bf16_nw2:qb>1:pair:dbias_none',
    'bwd_bf16_nw4:qb>1:single:dbias_two', 'bwd_bf16_d16:qb1:single:dbias_one', 'bwd_bf16_d16:qb>1:nodrop:dbias_none',
    'bwd_f32_d16:qb>1:single:dbias_two', 'bwd_f32_d16:qb1:pair:dbias_none', 'bwd_f32:qb1:nodrop:dbias_none',
    'bwd_f32:qb1:single:dbias_none', 'bwd_f32:qb>1:single:dbias_one', 'bwd_f32:qb>1:nodrop:dbias_none',
    'bwd_bf16_nw2:qb1:nodrop:dbias_none', 'bwd_f32:qb>1:single:dbias_two',
}


def test_every_dispatch_path_is_reached_and_every_case_is_needed():
    """the paths are named by fwd_path / bwd_path, which restate the launchers' dispatch conditions and read no table; a case stays
    only if it names a mutant or reaches a path no earlier case reaches"""
    seen = set()
    for case in ref.CASES:
        kern, shape = ref.fwd_kernel(case)[0], ref.bwd_shape(case)[0] if case['bwd'] else None
        p = ref.paths(case)
        # a mutant counts once per kernel (or backward launch shape) it is caught or silent on
        p |= {(m, shape if m in ref.BWD_MUTANTS else kern) for m in case['mutants']} | {('silent', m) for m in case['not_caught']}
        assert p - seen, 'case %s is not needed: no new path, and no mutant on a kernel that no earlier case has' % case['id']
        seen |= p
    assert PATHS <= seen, sorted(PATHS - seen)
    every = {ref.fwd_path(c) for c in ref.CASES} | {ref.bwd_path(c) for c in ref.CASES if c['bwd']}
    assert every == PATHS, sorted(every ^ PATHS)
    # PATHS is the set the tables reach, not the product of what the functions can return: the components are crossed only where
    # a kernel treats them together.  Each component is reached on every kernel / launch shape that has it:
    fw = {tuple(ref.fwd_path(c).split(':')) for c in ref.CASES}
    for kern in ('fwd_bf16', 'fwd_f32'):
        assert {(f[1], f[-1]) for f in fw if f[0] == kern} >= {('ksplit', 'nodrop'), ('qblocks', 'nodrop')}
        assert {f[-1] for f in fw if f[0] == kern} >= {'nodrop', 'single'} and {f[2] for f in fw if f[0] == kern and f[1] == 'ksplit'} == \
            {'nkt<nw', 'nkt>=nw'}
    assert {f[-1] for f in fw if f[0] == 'fwd_bf16'} == {'nodrop', 'pair', 'single'}
    assert {f[-1] for f in fw if f[0] == 'reg'} == {'nodrop', 'quad', 'pair', 'single'} and {f[1] for f in fw if f[0] == 'reg'} == {'occ2', 'occ3'}
    assert {f[1:] for f in fw if f[0] == 'self'} == {(a, b) for a in ('regs', 'dma') for b in ('quad', 'nodrop')}
    for kern in ('tile64_f32', 'tile64_bf16'):
        assert {f[-1] for f in fw if f[0] == kern} == {'nodrop', 'pair', 'single'}
    bw = {tuple(ref.bwd_path(c).split(':')) for c in ref.CASES if c['bwd']}
    for shape in ref.BWD_SHAPES:
        mine = {b[1:] for b in bw if b[0] == shape}
        assert {m[1] for m in mine} & {'pair', 'single'}, shape                       # every launch shape runs with dropout
        if not shape.endswith('d16') and shape != 'bwd_bf16_nw1':
            assert {m[0] for m in mine} == {'qb1', 'qb>1'}, shape
    assert {b[2] for b in bw} == {'nodrop', 'pair', 'single'} and {b[3] for b in bw} == {'dbias_one', 'dbias_two', 'dbias_none'}
    kernels = {ref.fwd_kernel(c)[0] for c in ref.CASES}
    assert kernels == set(ref.FWD_KERNELS)
    assert {ref.bwd_shape(c)[0] for c in ref.CASES if c['bwd']} == set(ref.BWD_SHAPES)


def test_the_dispatch_conditions():
    by = ref.BY_ID
    assert ref.fwd_kernel(by['s128_s128'])[0] == 'self' and ref.fwd_kernel(by['s128_s128'], dict(attn_self=0))[0] == 'reg'
    assert ref.fwd_kernel(by['s128_s128'], dict(attn_tile64=1))[0] == 'tile64_bf16'
    assert ref.fwd_kernel(by['r160_s130'])[0] == 'reg'                   # by S % 64 alone
    assert ref.fwd_kernel(by['r128_s64_b'])[0] == 'reg'                  # by the bias row alone
    assert ref.fwd_kernel(by['q96_s193'])[0] == 'fwd_bf16' and ref.fwd_kernel(by['r127_s257'])[0] == 'reg'    # QB 3 | 4
    assert ref.fwd_path(by['s97_s192_dma']) == 'self:dma:quad'
    shapes = {st: ref.bwd_shape(ref._c('x', 'bf16', 32, st))[0] for st in (31, 32, 33, 128, 129)}
    assert shapes == {31: 'bwd_bf16_nw1', 32: 'bwd_bf16_nw1', 33: 'bwd_bf16_nw2', 128: 'bwd_bf16_nw2', 129: 'bwd_bf16_nw4'}
    # the edges 32 | 33 and 128 | 129 of S_total occur on both sides, the virtual keys making the difference at 32 | 33
    st = {c['id']: ref.sizes(c)[0] for c in ref.CASES if c['bwd'] and c['dtype'] == 'bfloat16' and c['D'] == 64}
    assert st['k32_s31_z'] == 32 and st['k32_s31_bz'] == 33 and st['k1_s128'] == 128 and st['k31_s127_bz'] == 129
    assert {1, 2, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 193, 256, 257} <= {ref.sizes(c)[0] for c in ref.CASES}
    assert {1, 31, 32, 33, 64, 95, 96, 97, 127, 128, 129, 160} <= {c['Tq'] for c in ref.CASES}
    for kern in ('reg', 'fwd_bf16'):                                    # every walk with and without dropout
        got = {(ref.sizes(c)[0] % 4 if ref.sizes(c)[0] % 2 == 0 else 1, bool(c['p'])) for c in ref.CASES if ref.fwd_kernel(c)[0] == kern}
        assert {(0, True), (2, True), (1, True), (0, False), (2, False), (1, False)} <= got, (kern, got)
    # every layout on every forward kernel family and every backward launch shape family (the two D = 16 instantiations count as
    # one family each); a case in a non-dense layout also launches the dense one, for the bit comparison
    other = set(ref.LAYOUTS) - {'dense'}
    fams = {}
    for c in ref.CASES:
        fams.setdefault(ref.family(ref.fwd_kernel(c)[0]), set()).add(c['layout'])
        if c['bwd']:
            fams.setdefault(ref.family(ref.bwd_shape(c)[0]), set()).add(c['layout'])
    assert len(fams) == 7 + 5 and all(other <= v for v in fams.values()), {k: sorted(other - v) for k, v in fams.items() if other - v}
    for kern in ('fwd_bf16', 'reg', 'tile64_f32'):                      # the four virtual-key forms on every kernel that takes them
        got = {(c['bias'], c['zero']) for c in ref.CASES if ref.fwd_kernel(c)[0] == kern}
        assert len(got) == 4, (kern, got)


def torch_forward(case, keep):
    """softmax / logsumexp over the concatenated keys, the dropped-probability formulation, in torch float64 with autograd"""
    x = ref.inputs(case)
    B, H, Tq, S, D = case['B'], case['H'], case['Tq'], case['S'], case['D']
    t = lambda a: torch.tensor(np.asarray(a, F64), requires_grad=True)                          # noqa: E731
    q, k, v = t(x['q']), t(x['k']), t(x['v'])
    leaves = dict(q=q, k=k, v=v)
    ks, vs = [k], [v]
    neg = torch.zeros(B, 1, 1, S, dtype=torch.float64)
    if x['mask'] is not None:
        neg = neg.masked_fill(torch.tensor(x['mask'].astype(bool))[:, None, None, :], float('-inf'))
    cols = [neg]
    if case['bias']:
        bk, bv = t(x['bk']), t(x['bv'])
        leaves.update(bk=bk, bv=bv)
        ks.append(bk[None, :, None, :].expand(B, H, 1, D))
        vs.append(bv[None, :, None, :].expand(B, H, 1, D))
        cols.append(torch.zeros(B, 1, 1, 1, dtype=torch.float64))
    if case['zero']:
        ks.append(torch.zeros(B, H, 1, D, dtype=torch.float64))
        vs.append(torch.zeros(B, H, 1, D, dtype=torch.float64))
        cols.append(torch.zeros(B, 1, 1, 1, dtype=torch.float64))
    K, V = torch.cat(ks, 2), torch.cat(vs, 2)
    s = q @ K.transpose(-1, -2) + torch.cat(cols, -1)
    dead = torch.isinf(s).all(-1, keepdim=True)
    prob = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    lse = torch.logsumexp(s, -1).masked_fill(dead[..., 0], float('inf'))
    if keep is not None:
        prob = prob * torch.tensor(np.asarray(keep, F64)) / (1.0 - float(np.float32(case['p'])))
    return prob @ V, lse, leaves


@pytest.mark.parametrize('case', ref.CASES, ids=[c['id'] for c in ref.CASES])
def test_float64_reference_equals_a_torch_formulation(case):
    keep = ref.keep_of(case)
    out, lse, leaves = torch_forward(case, keep)
    want = ref.fwd_case(case)
    # (atol: an element that cancels to nothing keeps the float64 rounding of its 257 terms of size <= |v|, 257 x 2^-53 x 4)
    np.testing.assert_allclose(out.detach().numpy(), want['out'].value, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(lse.detach().numpy(), want['lse'].value, rtol=1e-10)
    if not case['bwd']:
        return
    x = ref.inputs(case)
    out.backward(torch.tensor(np.asarray(x['dout'], F64)))
    got = ref.attn_bwd(case, out.detach().numpy(), lse.detach().numpy())          # out and lse recomputed, not stored
    B, H, D = case['B'], case['H'], case['D']
    # (atol: dP - delta cancels on a key that holds all of a row's weight - 2^-52 of the largest operand stays)
    tol = lambda g: 1e-12 * max(1.0, float(np.abs(g).max(initial=0.0)))                                   # noqa: E731
    for k, leaf in (('dq', 'q'), ('dk', 'k'), ('dv', 'v')):
        g = leaves[leaf].grad.numpy()
        np.testing.assert_allclose(got[k].value, g, rtol=1e-10, atol=tol(g), err_msg=k)
    if case['bias']:
        for k, leaf in (('dbias_k', 'bk'), ('dbias_v', 'bv')):
            g = leaves[leaf].grad.numpy()
            np.testing.assert_allclose(got[k].value.reshape(B, H, D).sum(0), g, rtol=1e-10, atol=tol(g))


@pytest.mark.parametrize('case', ref.AVG, ids=[c['id'] for c in ref.AVG])
def test_average_weights_equal_the_head_mean_of_the_softmax(case):
    f = ref.fwd_case(case)
    lse = np.where(f['dead'], 0.0, f['lse'].value)
    w = ref.avg_weights(case, lse)
    want = np.where(f['dead'][..., None], 0.0, f['w1']).mean(1)
    np.testing.assert_allclose(np.where(np.broadcast_to(f['dead'].any(1)[..., None], want.shape), want, w.value), want, rtol=1e-10,
                               atol=1e-300)
    assert w.value.shape == (case['B'], case['Tq'], ref.sizes(case)[0])
    assert {ref.sizes(c)[0] for c in ref.AVG} == {1, 255, 256, 257} and {c['H'] for c in ref.AVG} == {1, 3}


def test_no_element_is_left_out_of_a_comparison():
    """every element of every output is bounded (finite reference, finite positive bound) or compared for equality"""
    for case in ALL:
        for want, _ in runs(case):
            for k, o in want.items():
                if not isinstance(o, ref.Out):
                    continue
                v = np.asarray(o.value, F64)
                ex = np.zeros(v.shape, bool) if o.exact_at is None else np.broadcast_to(o.exact_at, v.shape)
                S = np.broadcast_to(np.asarray(o.S, F64), v.shape)
                assert (np.isfinite(v) & np.isfinite(S) | ex).all(), (case['id'], k)
                bogus = np.full(v.shape, ref.SENTINEL, F32)
                assert ref.failures(bogus, o, 1.0) == v.size, (case['id'], k)


def test_coverage_facts():
    by = ref.BY_ID
    # an exact-zero row exists, on every forward kernel family that takes a mask
    zero_rows = {ref.fwd_kernel(c)[0] for c in ref.CASES if ref.fwd_case(c)['dead'].any()}
    assert {'fwd_bf16', 'reg', 'self', 'tile64_f32', 'fwd_f32'} <= zero_rows, zero_rows
    # the staircase moves the lazy maximum twice (the first tile and the third) and leaves a probability above e^5 in between
    moves, top = ref.lazy_moves(by['s128_s256_stair'])
    assert moves >= 1 and top > np.exp(5.0) and top <= np.exp(ref.THR), (moves, top)
    moves, top = ref.lazy_moves(by['s97_s128_79'])
    assert moves == 0 and np.exp(7.0) < top <= np.exp(ref.THR), (moves, top)
    moves, top = ref.lazy_moves(by['s128_s256_onerow'])
    assert moves >= 1
    moves, top = ref.lazy_moves(by['s128_s128_cliff'])          # 64 keys ahead by 86: 64 e^86 is not an fp32 number
    assert moves == 1 and top <= np.exp(ref.THR) and 64 * np.exp(86.0) > np.finfo(F32).max
    # the jump: live keys whose probability is exactly 0 in fp32
    for cid in ('s128_s192_jump', 'k32_s257_jump', 't128_s128_bf16', 'f32_q64_s64_jump'):
        f = ref.fwd_case(by[cid])
        live = np.isfinite(f['scores'])
        assert (live & (f['w1'].astype(F32) == 0)).any(), cid
    # every dropout case drops and keeps an element of its last key tile and of its last query row
    for c in ref.CASES:
        if not c['p']:
            continue
        keep = ref.keep_of(c)
        St = ref.sizes(c)[0]
        kt = 32 if ref.fwd_kernel(c)[0].startswith('fwd') else 64
        for part in (keep[..., (St - 1) // kt * kt:], keep[:, :, -1]):
            assert (part == 0).any() and (part == 1).any(), c['id']


def test_pinned_constants():
    """four times the measured ratio, rounded up to a power of two; 2^-10 where the ratio never left the first terms.  A
    measured ratio above 1 would mean an error the derived gamma does not count: a finding, not a number to pin over"""
    for k, v in ref.MEASURED.items():
        assert k in ref.GROUPS and v <= 1.0
        assert ref.C[k] == (2.0 ** -10 if v <= 0 else 2.0 ** np.ceil(np.log2(4 * v)))
