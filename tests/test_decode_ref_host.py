"""tests/decode_ref.py judged without a GPU: the float64 reference against an independent formulation
(torch.softmax in float64); an fp32 emulation of every case (the same formulas with every product, exp2 / exp and sequential
sum rounded to fp32; the packed path with its probabilities rounded to bf16) inside the bounds at c = 1, so the gammas and
the derived packed term are not too small; nineteen mutants of the reference, each of which must break a bound - at the
stored dtype and the pinned c - on a named case of the table; the coverage facts of the table as conditions on its inputs;
and decode.PackedKV.fill on the CPU against an independent indexing of the fragment-order layout."""
import types

import numpy as np
import pytest
import torch

import decode_ref as ref

F64 = torch.float64


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(F64)


def outside(out, got, want, S, dtype, gam, c, extra=0.0):
    """does any element of got leave the bound around want; where the reference is not finite (lse2 = -inf of a row without
    keys) got must be equal.  No element is left out."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and not np.isnan(want).any() and not (want == np.inf).any()
    inf = ~np.isfinite(want)
    if not np.array_equal(got[inf], want[inf]):
        return True
    b = np.broadcast_to(ref.bound(out, np.where(inf, 0.0, want), S, dtype, gam, c, extra), want.shape)
    return bool((np.abs(got[~inf] - want[~inf]) > b[~inf]).any())


def attn_outputs(L, beams, path, dt=np.float64, mutant=None):
    """[(output name, context, value, S, stored dtype, gamma, additive term)] of one launch; gamma from the float64 reference"""
    res, want = ref.launch_ref(L, beams, path, dt, mutant), ref.launch_ref(L, beams, path)
    outs = []
    for c, (r, w) in enumerate(zip(res, want)):
        if path == 'packed':
            outs.append(('pk_out', c, r['out'], w['S_out'], 'bfloat16', ref.attn_gamma('out', w), ref.PK_PROB * w['S_out']))
        else:
            outs.append(('ad_out_nq%d' % ref.nq_of(beams), c, r['out'], w['S_out'], 'bfloat16', ref.attn_gamma('out', w), 0.0))
            if beams == 1:
                outs.append(('ad_lse2', c, r['lse2'], w['S_lse'], 'float32', ref.attn_gamma('lse', w), 0.0))
    return outs


def attn_grid():
    return [(L, beams, path) for L in ref.ATTN for beams in ref.launch_beams(L) for path in ('valu', 'packed')]


# ---------------------------------------------------------------- the reference against torch
@pytest.mark.parametrize('L', ref.ATTN, ids=[L['id'] for L in ref.ATTN])
def test_attention_reference_against_torch_softmax(L):
    beams, Bs, H = L['wide'], L.get('samples', 3), L['H']
    for path in ('valu', 'packed'):
        virt = ref.virt_of(L, path)
        for S, x, r in zip(L['S'], ref.attn_inputs(L), ref.launch_ref(L, beams, path)):
            q = tt(x['q'][:, :beams]).reshape(Bs, beams, H, 64)
            k, v = (tt(x[n]).reshape(S, Bs, H, 64) for n in ('k', 'v'))
            keys = [k] + ([tt(x['bias_k']).reshape(1, 1, H, 64).expand(1, Bs, H, 64)] if 'k' in virt else []) + \
                ([torch.zeros(1, Bs, H, 64, dtype=F64)] if 'z' in virt else [])
            vals = [v] + ([(tt(x['bias_v']) if 'v' in virt else torch.zeros(H * 64, dtype=F64)).reshape(1, 1, H, 64)
                           .expand(1, Bs, H, 64)] if 'k' in virt else []) + ([torch.zeros(1, Bs, H, 64, dtype=F64)] if 'z' in virt else [])
            kx, vx = torch.cat(keys), torch.cat(vals)
            lg = torch.einsum('bjhd,sbhd->bjhs', q, kx)
            if x['mask'] is not None:
                dead = torch.cat([torch.from_numpy(x['mask']).bool(), torch.zeros(Bs, kx.shape[0] - S, dtype=torch.bool)], 1)
                lg = lg.masked_fill(dead[:, None, None, :], -np.inf)
            none = torch.isinf(lg).all(-1)
            out = torch.einsum('bjhs,sbhd->bjhd', torch.softmax(lg.masked_fill(none[..., None], 0.0), -1), vx)
            out = out.masked_fill(none[..., None], 0.0).reshape(Bs * beams, H * 64).numpy()
            lse2 = (torch.logsumexp(lg, -1) / np.log(2.0)).reshape(Bs * beams, H).numpy()
            assert np.allclose(r['out'], out, rtol=1e-10, atol=1e-12), (L['id'], path, S)
            assert np.array_equal(np.isinf(r['lse2']), none.reshape(Bs * beams, H).numpy())
            fin = np.isfinite(r['lse2'])
            assert np.allclose(r['lse2'][fin], lse2[fin], rtol=1e-10, atol=1e-12) and (r['lse2'][~fin] == -np.inf).all()
            assert not np.signbit(r['out'][np.repeat(~fin, 64, -1)]).any() and not r['out'][np.repeat(~fin, 64, -1)].any()


@pytest.mark.parametrize('case', ref.DCS, ids=[c['id'] for c in ref.DCS])
def test_dynconv_step_reference_against_torch(case):
    """the window of a step rebuilt from the list of past inputs (no ring): step s of hypothesis lineage"""
    x, H, K, Cc, M = ref.dcs_inputs(case), case['H'], case['K'], case['C'], case['M']
    wt = tt(x['wt'])
    hist = {}                                                     # step index -> input rows
    for (t, hb), perm, r in zip(ref.dcs_steps(case), x['perms'], ref.dcs_run(case)):
        xt = tt(x['base'][perm])
        taps = torch.softmax((xt @ wt.t()).reshape(M, H, K), -1)
        win = []
        for j in range(K - 1, 0, -1):
            # what the ring holds for "j steps ago": the latest step s <= t - 1 with s = t - j mod K, if it was ever written
            s = max([s for s in hist if s < t and (s - (t - j)) % K == 0], default=None)
            rows = hist[s] if s is not None else torch.zeros(M, Cc, dtype=F64)
            win.append(rows[torch.from_numpy(x['back'][j - 1]).long()] if hb else rows)
        win.append(xt)
        y = sum(taps[..., i].repeat_interleave(64, -1) * w for i, w in enumerate(win))
        assert np.allclose(r['y'], y.numpy(), rtol=1e-10, atol=1e-12), (case['id'], t)
        hist[t] = xt
        if case.get('taps') == 'equal':
            assert np.allclose(taps.numpy(), 1.0 / K, rtol=1e-12)
        if case.get('taps') == 'peaked':
            assert float(taps.max(-1).values.min()) > 1 - 1e-9


# ---------------------------------------------------------------- fp32 emulation at c = 1
@pytest.mark.parametrize('L', ref.ATTN, ids=[L['id'] for L in ref.ATTN])
def test_fp32_emulation_attention(L):
    for beams in ref.launch_beams(L):
        for path in ('valu', 'packed'):
            want, emu = attn_outputs(L, beams, path), attn_outputs(L, beams, path, np.float32)
            for (o, c, w, S, _, gam, extra), (_, _, g, _, _, _, _) in zip(want, emu):
                assert not outside(o, g, w, S, 'float32', gam, 1.0, extra), \
                    '%s beams %d %s context %d %s: fp32 emulation outside the bound at c = 1 (ratio %.3f)' % (
                        L['id'], beams, path, c, o, ref.ratio(g, w, S, 'float32', gam, extra))


def test_packed_probability_term_is_needed():
    """without the derived 2^-8 S_out term the packed emulation (probabilities rounded to bf16) leaves the bound at c = 1:
    the term is what covers that rounding, not gamma and not c"""
    L = next(L for L in ref.ATTN if L['id'] == 'S62_63')
    want, emu = attn_outputs(L, L['wide'], 'packed'), attn_outputs(L, L['wide'], 'packed', np.float32)
    assert any(outside(o, g, w, S, 'float32', gam, 1.0, 0.0) for (o, _, w, S, _, gam, _), (_, _, g, _, _, _, _) in zip(want, emu))


@pytest.mark.parametrize('case', ref.DCS, ids=[c['id'] for c in ref.DCS])
def test_fp32_emulation_dynconv_step(case):
    for i, (w, g) in enumerate(zip(ref.dcs_run(case), ref.dcs_run(case, np.float32))):
        gam = ref.dcs_gamma(w, case['C'], case['K'])
        assert not outside('dcs_y', g['y'], w['y'], w['S_y'], 'float32', gam, 1.0), \
            '%s step %d: ratio %.3f' % (case['id'], i, ref.ratio(g['y'], w['y'], w['S_y'], 'float32', gam))


def test_dynconv_step_ring_takes_exactly_one_plane():
    case = ref.DCS[8]
    x, K, M, Cc = ref.dcs_inputs(case), case['K'], case['M'], case['C']
    ring = np.random.default_rng(3).standard_normal((K, M, Cc))
    for t in (0, 1, K, 1000 + K):
        for dt in (np.float64, np.float32):
            before = ring.copy()
            r = ref.dynconv_step(x['base'], ring, x['wt'], t, x['back'], case['H'], K, dt)
            assert np.array_equal(ring, before) and np.array_equal(r['ring'][t % K], x['base'])
            others = [k for k in range(K) if k != t % K]
            assert np.array_equal(r['ring'][others], before[others])


# ---------------------------------------------------------------- mutants
def _c(o):
    return max(ref.C.get(o, 1.0), 1.0)


@pytest.mark.parametrize('mutant', ref.ATTN_MUTANTS + ref.PK_MUTANTS)
def test_attention_mutants_break_a_bound(mutant):
    """each wrong-answer variant leaves the bound of the STORED dtype (at the pinned c, at least 1) on a named case"""
    broken = []
    both = ('mask_by_row', 'cache_by_row', 'first_q_for_all', 'drop_last_key', 'no_rescale', 'ctx_swap')
    paths = ('packed',) if mutant in ref.PK_MUTANTS else (('valu', 'packed') if mutant in both else ('valu',))
    for L, beams, path in attn_grid():
        if path not in paths:
            continue
        want, got = attn_outputs(L, beams, path), attn_outputs(L, beams, path, mutant=mutant)
        for (o, c, w, S, dtype, gam, extra), (_, _, g, _, _, _, _) in zip(want, got):
            if outside(o, g, w, S, dtype, gam, _c(o), extra):
                broken.append((L['id'], beams, path, c, o))
    print('\n%s breaks: %s' % (mutant, broken))
    assert broken, mutant
    ids = {b[0] for b in broken}
    where = {(b[0], b[3]) for b in broken}
    if mutant == 'drop_wave3':
        assert where <= {('S16_25', 3), ('S30_33', 0), ('S30_33', 1), ('S30_33', 2), ('unmasked', 0)} and ('S30_33', 1) in where
    if mutant == 'drop_second_trip':
        assert ids <= {'S0_129', 'S257', 'S2048', 'ascending', 'peaked'} and {'S0_129', 'S257', 'S2048'} <= ids
    if mutant == 'pk_block_round_robin':
        assert ids <= {'S0_129', 'S126_128', 'S257', 'S2048', 'ascending', 'peaked', 'unmasked'} and 'S126_128' in ids
    if mutant == 'tail_key_live':
        assert ('S7_8_9', 2) in where and not any(L['S'][c] % 8 == 0 for L in ref.ATTN for c in range(len(L['S']))
                                                   if (L['id'], c) in where)
    if mutant == 'no_rescale':
        assert 'ascending' in ids
    if mutant == 'ctx_swap':
        assert all(b[3] in (1, 2) for b in broken)
    if mutant in ('mask_by_row', 'cache_by_row', 'first_q_for_all'):
        assert all(b[1] > 1 for b in broken) and {b[2] for b in broken} == {'valu', 'packed'}
        assert {ref.nq_of(b[1]) for b in broken if b[2] == 'valu'} == {2, 4}
    if mutant == 'lse_natural':
        assert all(b[4] == 'ad_lse2' for b in broken)
    if mutant in ('no_zero_key', 'bias_v_as_bias_k'):
        assert {ref.nq_of(b[1]) for b in broken} == {1, 2, 4}


@pytest.mark.parametrize('mutant', ref.DCS_MUTANTS)
def test_dynconv_step_mutants_break_a_bound(mutant):
    broken = []
    for case in ref.DCS:
        for i, (w, g) in enumerate(zip(ref.dcs_run(case), ref.dcs_run(case, mutant=mutant))):
            if outside('dcs_y', g['y'], w['y'], w['S_y'], 'bfloat16', ref.dcs_gamma(w, case['C'], case['K']), _c('dcs_y')):
                broken.append((case['id'], i))
    print('\n%s breaks: %s' % (mutant, broken))
    assert broken, mutant
    ids = {b[0] for b in broken}
    by_id = {c['id']: c for c in ref.DCS}
    if mutant == 'dcs_back_ignored':
        assert all(ref.dcs_steps(by_id[c])[i][1] for c, i in broken) and len(ids) >= 9
    if mutant == 'dcs_second_tile_lost':
        assert ids == {c['id'] for c in ref.DCS if c['K'] > 16}
    if mutant == 'dcs_softmax_over_32':
        assert not any(by_id[c]['K'] == 32 for c in ids) and len(ids) >= 9
    if mutant in ('dcs_tap_reversed', 'dcs_plane_off_by_one'):
        assert len(ids) >= 9 and any(i == len(ref.dcs_steps(by_id[c])) - 1 for c, i in broken)   # ... and at the large t


# ---------------------------------------------------------------- coverage facts, as conditions on the inputs
def test_attention_table_covers_what_it_claims():
    S_all = sorted({S for L in ref.ATTN for S in L['S']})
    assert S_all == [0, 1, 7, 8, 9, 16, 17, 24, 25, 30, 31, 32, 33, 62, 63, 126, 127, 128, 129, 257, 2048]
    assert {b for L in ref.ATTN for b in ref.launch_beams(L)} == set(ref.BEAMS)
    assert {L['H'] for L in ref.ATTN if L['id'] != 'S2048'} == {1, 3, 16}
    assert {len(L['S']) for L in ref.ATTN} == {1, 2, 3, 4}
    assert {L['virt'] for L in ref.ATTN} == {'kvz', 'k', 'z', 'none'} and {L['klay'] for L in ref.ATTN} == {'row', 'head', 'inter'}
    assert {m for L in ref.ATTN for m in L['masks']} == {'none', 'ragged', 's0', 'last', 'first'}
    assert any(L.get('qwide') for L in ref.ATTN) and any(L.get('owide') for L in ref.ATTN)
    assert any(0 in L['S'] and 129 in L['S'] for L in ref.ATTN)
    assert all(min(L['S']) > 0 for L in ref.ATTN if L['virt'] == 'none')          # (no keys at all is a refusal)
    by_id = {L['id']: L for L in ref.ATTN}
    assert by_id['S2048'].get('samples') == 2 and by_id['S2048']['H'] == 2
    zero_rows = 0
    for L in ref.ATTN:
        for beams in ref.launch_beams(L):
            for S, r in zip(L['S'], ref.launch_ref(L, beams)):
                zero_rows += int((~r['has']).sum())
                if S >= 129:                     # a (row, head) whose largest score lies in the second trip or later
                    am = np.where(np.isfinite(r['s2'][..., :S]), r['s2'][..., :S], -np.inf).argmax(-1)
                    assert (am[r['has']] >= 128).any(), (L['id'], S)
    assert zero_rows > 0
    for S, r in zip(by_id['ascending']['S'], ref.launch_ref(by_id['ascending'], 2)):
        last = (S - 1) // 128 * 128
        assert (r['s2'][..., last:S].max(-1) > r['s2'][..., :last].max(-1)).any()     # the running maximum moves in the last trip
    for path in ('valu', 'packed'):
        for r in ref.launch_ref(by_id['peaked'], 4, path, np.float32):
            assert (r['w'] == 0).any() and np.isfinite(r['out']).all()                # live keys of probability exactly 0 in fp32
        for r in ref.launch_ref(by_id['peaked'], 4, path):
            top2 = np.sort(np.where(np.isnan(r['w']), -np.inf, r['s2']), -1)[..., -2:]
            assert ((top2[..., 1] - top2[..., 0])[r['has']] > 150).any()
    for L in ref.ATTN:                           # inputs are bf16 values
        for x in ref.attn_inputs(L):
            for n in ('q', 'k', 'v', 'bias_k', 'bias_v'):
                t = torch.from_numpy(np.ascontiguousarray(x[n]))
                assert torch.equal(t.to(torch.bfloat16).double(), t)


def test_dynconv_table_covers_what_it_claims():
    assert all(ref.dynconv_rule(c['M'], c['H']) == c['R'] and c['M'] % c['R'] and c['C'] == c['H'] * 64 for c in ref.DCS)
    assert {(c['C'], c['R']) for c in ref.DCS} == {(C, R) for C in (512, 1024, 2048) for R in (4, 8, 16)}
    Ks = {c['K'] for c in ref.DCS}
    assert Ks == {2, 3, 4, 5, 8, 9, 16, 17, 31, 32}
    assert {ref.dynconv_bucket(K) for K in Ks} == {4, 8, 16, 32}
    assert {2, 4, 5, 8, 9, 16, 17, 32} <= Ks                                       # both edges of every bucket
    assert {c.get('taps', 'plain') for c in ref.DCS} == {'plain', 'peaked', 'equal'}
    for c in ref.DCS:
        st = ref.dcs_steps(c)
        assert [t for t, _ in st[:c['K'] + 3]] == list(range(c['K'] + 3)) and st[-2][1] and st[-1][0] == 1000 + c['K']
        x = ref.dcs_inputs(c)
        assert (x['back'] != np.arange(c['M'])).any() and x['back'].shape == (c['K'] - 1, c['M'])


# ---------------------------------------------------------------- PackedKV.fill on the CPU
@pytest.mark.parametrize('S', [0, 1, 30, 31, 62, 63, 127])
def test_packed_kv_fill_layout(S):
    """kc and vt unpacked with an indexing written from the layout comment in csrc/decode.hip, not from fill's permutes"""
    try:
        from tell_amd import decode
    except Exception as err:                                     # noqa: BLE001
        pytest.skip('tell_amd cannot be imported here: %s' % err)
    Bc, H = 2, 3
    E = H * 64
    g = torch.Generator().manual_seed(50 + S)
    bf = torch.bfloat16
    k, v = torch.randn(S, Bc, E, generator=g).to(bf), torch.randn(S, Bc, E, generator=g).to(bf)
    mod = types.SimpleNamespace(num_heads=H, bias_k=torch.randn(1, 1, E, generator=g).to(bf),
                                bias_v=torch.randn(1, 1, E, generator=g).to(bf))
    mask = (torch.rand(Bc, S, generator=g) < 0.3).to(torch.uint8)
    pk = decode.PackedKV(mod, S, Bc, 'cpu')
    pk.fill(k, v, mask)
    Sp = pk.Sp
    assert Sp % 32 == 0 and Sp - 32 < S + 2 <= Sp
    kc = pk.kc.float().numpy().reshape(Bc, H, Sp // 16, 2, 64, 8)
    vt = pk.vt.float().numpy().reshape(Bc, H, Sp // 32, 4, 64, 8)
    lane = np.arange(64)
    knat, vnat = np.zeros((Bc, H, Sp, 64), np.float32), np.zeros((Bc, H, Sp, 64), np.float32)
    for tile in range(Sp // 16):
        for c in range(2):
            for e in range(8):
                knat[:, :, tile * 16 + (lane & 15), c * 32 + (lane >> 4) * 8 + e] = kc[:, :, tile, c, lane, e]
    for blk in range(Sp // 32):
        for rt in range(4):
            for j in range(8):
                key = blk * 32 + (4 * (lane >> 4) + j if j < 4 else 16 + 4 * (lane >> 4) + j - 4)
                vnat[:, :, key, rt * 16 + (lane & 15)] = vt[:, :, blk, rt, lane, j]
    want_k, want_v = (t.float().numpy().reshape(S, Bc, H, 64).transpose(1, 2, 0, 3) for t in (k, v))
    assert np.array_equal(knat[:, :, :S], want_k) and np.array_equal(vnat[:, :, :S], want_v)
    for b in range(Bc):
        assert np.array_equal(knat[b, :, S], mod.bias_k.float().numpy().reshape(H, 64))
        assert np.array_equal(vnat[b, :, S], mod.bias_v.float().numpy().reshape(H, 64))
    assert not knat[:, :, S + 1:].any() and not vnat[:, :, S + 1:].any()
    m = pk.mask.numpy()
    assert np.array_equal(m[:, :S], mask.numpy()) and not m[:, S:S + 2].any() and (m[:, S + 2:] == 1).all()
    pk.fill(k, v, None)
    assert not pk.mask.numpy()[:, :S + 2].any() and (pk.mask.numpy()[:, S + 2:] == 1).all()
