"""The copy-mechanism kernels (csrc/copy.hip) through the C ABI, every entry point in both dtypes, element by element
against the float64 reference and the bounds of tests/copy_ref.py.  Every operand and every output
is a view inside a buffer of sentinels (tests/guarded.py): after each launch the guard bands and the row gaps of all of
them are intact.  Discrete outputs (tokens, copy flags, the history column, the vocabulary count, where NaN sits, the
exact zeros) must be equal.
Run on the MI355X box:  python -m pytest tests/test_gpu_copy.py -m gpu -s   (-s prints the ratios c is pinned from and the
time of the whole file)"""
import time

import numpy as np
import pytest
import torch

import copy_ref as ref
from guarded import DEV, SENTINEL, Guard

pytestmark = pytest.mark.gpu

F32, BF16, I64, I32, U8, I8 = torch.float32, torch.bfloat16, torch.int64, torch.int32, torch.uint8, torch.int8
SEED, SALT = ref.SEED, ref.SALT
_RATIOS, _UNPINNED = {}, {}


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    tell_amd.hip.call('tell_set_rng_step_ptr', None)     # tell_step_salt would fold in a step the reference does not know
    _UNPINNED.clear()
    yield
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
    print('\ntests/test_gpu_copy.py: %.1f s' % (time.time() - t0))


def tdt(dtype):
    return getattr(torch, dtype)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def check(out, got, want, S, stored, gam, tag):
    """element-wise bound of copy_ref; NaN must sit where the reference has it; the ratio c is pinned from is recorded"""
    got = ref.np64(got).reshape(np.shape(want))
    want = np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s %s: NaN in other places' % (out, tag)
    ok = ~np.isnan(want)
    assert np.isfinite(got[ok]).all(), (out, tag)
    S = np.broadcast_to(np.asarray(S, np.float64), want.shape)
    r = ref.ratio(got[ok], want[ok], S[ok], stored, gam)
    _RATIOS[out] = max(_RATIOS.get(out, 0.0), r)
    print('ratio %-12s %-40s %.6f' % (out, tag, r))
    if out not in ref.C:
        _UNPINNED[out] = max(_UNPINNED.get(out, 0.0), r)
        return
    err, b = np.abs(got - want)[ok], ref.bound(out, want[ok], S[ok], stored, gam)
    bad = err > b
    assert not bad.any(), '%s %s: %d of %d outside the bound, worst error %.3g at bound %.3g (ratio %.3f, c = %g)' % (
        out, tag, bad.sum(), bad.size, err[bad].max(), b[bad][err[bad].argmax()], r, ref.C[out])


def settle():
    """until c is pinned the test fails with the measured ratio in its message"""
    assert not _UNPINNED, 'constant not pinned yet, largest ratios of this case: %s' % \
        ', '.join('%s %.4f' % kv for kv in sorted(_UNPINNED.items()))


def intact(*guards):
    torch.cuda.synchronize()
    for i, g in enumerate(guards):
        assert g is None or g.intact(), 'store outside view %d of the launch' % i


def ptr(g):
    return None if g is None else g.t


def declined(name, *args):
    """the return code of a call the library declines (a negative code arrives as the RuntimeError of hip.call_rc)"""
    from tell_amd import hip
    try:
        return hip.call_rc(name, *args)
    except RuntimeError as err:
        assert name in str(err)
        return -1


# ---------------------------------------------------------------- copy attention
def attn_buffers(case, dtype, x):
    """q, k (and the like-strided dq, dk) laid out as the case says"""
    B, H, T, S, D = case['shape']
    E, td, lay = H * D, tdt(dtype), case['layout']
    qs = (B * 3 * E, 3 * E, 1) if lay == 'q_third' else None
    ks, koff = None, 0
    if lay == 'k_half':
        ks, koff = (B * 2 * E, 2 * E, 1), E
    if lay == 'k_bse':
        ks = (E, S * E, 1)
    mk = lambda shape, st, off, fill: Guard(shape, td, st, None if fill is None else dev(fill, td), off)   # noqa: E731
    q, dq = mk((T, B, E), qs, 0, x['q']), mk((T, B, E), qs, 0, None)
    k = mk((S, B, E), ks, koff, x['k'])
    dk = mk((S, B, E), ks, koff, None) if S else mk((1, B, E), None, 0, None)
    return q, k, dq, dk


@pytest.mark.parametrize('p', ref.P_DROP)
@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('case', ref.ATTN, ids=[c['id'] for c in ref.ATTN])
def test_copy_attention(case, dtype, p):
    from tell_amd import hip
    B, H, T, S, D = case['shape']
    E, td = H * D, tdt(dtype)
    tag = 'attn %s %s p=%.1f' % (case['id'], dtype, p)
    x = ref.attn_inputs(case, dtype)
    keep, f = ref.attn_ref(case, dtype, p)
    q, k, dq, dk = attn_buffers(case, dtype, x)
    bk = Guard((E,), td, fill=dev(x['bias_k'], td))
    mask = None if x['mask'] is None else Guard((B, S), U8, fill=x['mask'])
    proper = None if x['proper'] is None else Guard((B, S), I8, fill=x['proper'])
    w, lse = Guard((B, T, S), F32), Guard((B, H, T), F32)
    strides = (q.strides[0], q.strides[1], k.strides[0], k.strides[1])
    hip.call('tell_copy_attn_fwd', q.t, k.t, bk.t, ptr(mask), ptr(proper), w.t, lse.t, B, H, T, S, D, *strides, p, SEED, SALT,
             hip.dt(td))
    intact(q, k, bk, mask, proper, w, lse)
    g = lambda o, st: ref.attn_gamma(o, st, H, T, S, D)                                       # noqa: E731
    check('w', w.t, f['w'], f['S_w'], 'float32', g('w', f), tag)
    check('lse', lse.t, f['lse'], f['S_lse'], 'float32', g('lse', f), tag)
    assert torch.equal(w.t == 0, dev(f['w'] == 0, torch.bool).to(DEV)), tag + ': the exact zeros of w'
    dw = Guard((B, T, S), F32, fill=dev(x['dw'], F32))
    dbk, delta = Guard((B * T, E), F32), Guard((B, H, T), F32)
    hip.call('tell_copy_attn_bwd', q.t, k.t, bk.t, ptr(mask), ptr(proper), lse.t, dw.t, dq.t, dk.t, dbk.t, delta.t, B, H, T, S, D,
             *strides, p, SEED, SALT, hip.dt(td))
    intact(q, k, bk, mask, proper, lse, dw, dq, dk, dbk, delta)
    b = ref.copy_attn_bwd(x['q'], x['k'], x['bias_k'], x['mask'], x['proper'], H, keep, ref.np64(lse.t), x['dw'])
    check('delta', delta.t, b['delta'], b['S_delta'], 'float32', g('delta', b), tag)
    check('dq', dq.t, b['dq'], b['S_dq'], dtype, g('dq', b), tag)
    check('dbk', dbk.t, b['dbk'], b['S_dbk'], 'float32', g('dbk', b), tag)
    if S:
        check('dk', dk.t, b['dk'], b['S_dk'], dtype, g('dk', b), tag)
    else:
        assert dk.untouched(), 'S = 0: the key side is not launched'
    if case['mask'] == 'padrow':
        assert not bool(w.t[1].any()) and not bool(dk.t[:, 1].any()), tag + ': a fully padded row gives exact zeros'
    settle()


# ---------------------------------------------------------------- copy loss
@pytest.mark.parametrize('variant', [1, 2])
@pytest.mark.parametrize('case', ref.LOSS, ids=[c['id'] for c in ref.LOSS])
def test_copy_loss(case, variant):
    from tell_amd import hip
    B, T, S = case['shape']
    tag = 'loss %s v%d' % (case['id'], variant)
    x = ref.loss_inputs(case)
    tgt_sb, cm_sb = T + x['tgt_pad'], T + x['cm_pad']
    w = Guard((B, T, S), F32, fill=dev(x['w'], F32))
    ctx = Guard((B, S), I64, fill=x['ctx'])
    tgt, cm = Guard((B, T), I64, (tgt_sb, 1), x['tgt']), Guard((B, T), I64, (cm_sb, 1), x['cm'])
    words = (case['vocab'] + 31) // 32
    bitmap, count = Guard((words + 1,), I32), Guard((1,), I32)
    hip.call('tell_copy_vocab_count', ctx.t, B * S, tgt.t, B, T, tgt_sb, case['vocab'], bitmap.t, count.t)
    intact(ctx, tgt, bitmap, count)
    V = ref.vocab_count(x['ctx'], x['tgt'], case['vocab'])
    assert int(count.t) == V, tag
    ids = np.concatenate([x['ctx'].reshape(-1), x['tgt'].reshape(-1)])
    legal = ids[(ids >= 0) & (ids < case['vocab'])]
    bits = np.zeros(words * 32, np.int64)
    bits[legal] = 1
    want_words = (bits.reshape(words, 32) << np.arange(32)).sum(1).astype(np.uint32).astype(np.int32)
    assert bitmap.t[:words].cpu().numpy().tolist() == want_words.tolist(), tag + ': the bitmap'
    assert int(bitmap.t[words]) == int(len(legal) != len(ids)), tag + ': the flag word'
    outs = {n: Guard((B, T), F32) for n in ('term', 'p_target', 'z', 'scale')}
    loss = Guard((1,), F32)
    hip.call('tell_copy_loss_fwd', w.t, ctx.t, tgt.t, tgt_sb, cm.t, cm_sb, count.t if variant == 2 else None, variant, B, T, S,
             outs['term'].t, outs['p_target'].t, outs['z'].t, outs['scale'].t, loss.t)
    intact(w, ctx, tgt, cm, count, loss, *outs.values())
    r = ref.copy_loss(x['w'], x['ctx'], x['tgt'], x['cm'], variant, V)
    g = lambda o: ref.loss_gamma(o, r['n'], B, T, S, r['top'])                                # noqa: E731
    for n in ('p_target', 'z', 'term', 'scale'):
        check(n, outs[n].t, r[n], r['S_' + n], 'float32', g(n), tag)
    check('loss', loss.t, np.reshape(r['loss'], (1,)), r['S_loss'], 'float32', g('loss'), tag)
    if case['kind'] == 'gap' or (V < 0 and variant == 2):
        assert bool(torch.isnan(loss.t).all()), tag
    for n in ('term', 'p_target', 'z', 'scale'):
        assert not bool(outs[n].t[dev(x['cm'] < 1, torch.bool).to(DEV)].any()), tag + ': rows without an entity are 0'
    dloss = Guard((1,), F32, fill=torch.tensor([0.37]))
    dw = Guard((B, T, S), F32)
    hip.call('tell_copy_loss_bwd', dloss.t, w.t, ctx.t, tgt.t, tgt_sb, cm.t, cm_sb, outs['p_target'].t, outs['z'].t,
             outs['scale'].t, variant, B, T, S, dw.t)
    intact(dloss, w, ctx, tgt, cm, dw, *outs.values())
    check('loss_dw', dw.t, r['dw'], r['S_dw'], 'float32', g('loss_dw'), tag)
    assert torch.equal(dw.t == 0, dev(r['dw'] == 0, torch.bool).to(DEV)), tag + ': the exact zeros of dw'
    settle()


# ---------------------------------------------------------------- entity head
@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('case', ref.ENT, ids=[c['id'] for c in ref.ENT])
def test_entity_head(case, dtype):
    from tell_amd import hip
    B, T, E = case['shape']
    td = tdt(dtype)
    tag = 'entity %s %s' % (case['id'], dtype)
    x = ref.ent_inputs(case, dtype)
    xs, dxs = (B * (E + 8), E + 8, 1), (B * (E + 24), E + 24, 1)           # x and dx inside wider buffers, dx_st != x_st
    xg, dx = Guard((T, B, E), td, xs, dev(x['x'], td)), Guard((T, B, E), td, dxs)
    wg, bias = Guard((2, E), F32, fill=dev(x['w'], F32)), Guard((2,), F32, fill=dev(x['bias'], F32))
    cm = Guard((B, T), I64, (T + 5, 1), x['cm'])
    logits, loss, nvalid = Guard((B, T, 2), F32), Guard((1,), F32), Guard((1,), F32)
    hip.call('tell_entity_head_fwd', xg.t, xs[0], xs[1], wg.t, bias.t, cm.t, T + 5, B, T, E, logits.t, loss.t, nvalid.t,
             hip.dt(td))
    intact(xg, wg, bias, cm, logits, loss, nvalid)
    r = ref.entity_head(x['x'], x['w'], x['bias'], x['cm'], logits=ref.np64(logits.t), dbias0=x['dbias0'])
    g = lambda o: ref.ent_gamma(o, B, T, E)                                                    # noqa: E731
    check('ent_logits', logits.t, r['logits'], r['S_logits'], 'float32', g('ent_logits'), tag)
    check('ent_loss', loss.t, np.reshape(r['loss'], (1,)), r['S_loss'], 'float32', g('ent_loss'), tag)
    assert float(nvalid.t) == r['nvalid'], tag
    dloss = Guard((1,), F32, fill=torch.tensor([0.37]))
    dlogits, dw = Guard((B, T, 2), F32), Guard((2, E), F32)                # dw is assigned: preset to sentinels
    db = Guard((2,), F32, fill=dev(x['dbias0'], F32))                      # dbias is accumulated: preset to non-zero values
    hip.call('tell_entity_head_bwd', dloss.t, nvalid.t, logits.t, cm.t, T + 5, xg.t, xs[0], xs[1], wg.t, dx.t, dxs[0], dxs[1],
             dlogits.t, dw.t, db.t, B, T, E, hip.dt(td))
    intact(dloss, nvalid, logits, cm, xg, wg, dx, dlogits, dw, db)
    if case['cm'] == 'ignored':
        assert bool(torch.isnan(loss.t).all()) and not bool(dx.t.any()) and not bool(dlogits.t.any()) and not bool(dw.t.any())
        assert db.t.tolist() == x['dbias0'].tolist()
        return
    check('ent_dlogits', dlogits.t, r['dlogits'], r['S_dlogits'], 'float32', g('ent_dlogits'), tag)
    check('ent_dx', dx.t, r['dx'], r['S_dx'], dtype, g('ent_dx'), tag)
    check('ent_dw', dw.t, r['dw'], r['S_dw'], 'float32', g('ent_dw'), tag)
    check('ent_db', db.t, r['dbias'], r['S_dbias'], 'float32', g('ent_db'), tag)
    assert not bool(dlogits.t[dev(x['cm'] == -1, torch.bool).to(DEV)].any()), tag + ': ignored rows have no gradient'
    settle()


@pytest.mark.parametrize('dtype', ref.DTYPES)
def test_entity_logits_of_one_step(dtype):
    """tell_entity_logits with T = 1 (the generation step), with and without a bias"""
    from tell_amd import hip
    case = ref.ENT_LOGITS
    B, T, E = case['shape']
    td = tdt(dtype)
    x = ref.ent_inputs(case, dtype)
    xs = (B * (E + 8), E + 8, 1)
    xg = Guard((T, B, E), td, xs, dev(x['x'], td))
    wg, bias = Guard((2, E), F32, fill=dev(x['w'], F32)), Guard((2,), F32, fill=dev(x['bias'], F32))
    for bg, bv in ((bias, x['bias']), (None, np.zeros(2))):
        logits = Guard((B, T, 2), F32)
        hip.call('tell_entity_logits', xg.t, xs[0], xs[1], wg.t, ptr(bg), B, T, E, logits.t, hip.dt(td))
        intact(xg, wg, bias, logits)
        r = ref.entity_head(x['x'], x['w'], bv, x['cm'])
        check('ent_logits', logits.t, r['logits'], r['S_logits'], 'float32', ref.ent_gamma('ent_logits', B, T, E),
              'logits_T1 %s' % dtype)
    settle()


# ---------------------------------------------------------------- causal entity attention
@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('case', ref.CAUSAL, ids=[c['id'] for c in ref.CAUSAL])
def test_causal_training(case, dtype):
    """q, k, v are the three thirds of one [T,B,3E] buffer (dq, dk, dv of another), out and dout have a stride of their own"""
    from tell_amd import hip
    B, H, T = case['shape']
    E, td = H * 64, tdt(dtype)
    tag = 'causal %s %s' % (case['id'], dtype)
    x = ref.causal_inputs(case, dtype)
    qkv = Guard((T, B, 3 * E), td, fill=dev(np.concatenate([x['q'], x['k'], x['v']], -1), td))
    q, k, v = (qkv.t[..., i * E:(i + 1) * E] for i in range(3))
    os_ = (B * (E + 16), E + 16, 1)
    out, lse = Guard((T, B, E), td, os_), Guard((B, H, T), F32)
    st = (B * 3 * E, 3 * E) * 3 + os_[:2]
    hip.call('tell_causal_attn_fwd', q, k, v, out.t, lse.t, B, H, T, T, 64, 0, *st, ref.C_SCALE, hip.dt(td))
    intact(qkv, out, lse)
    f = ref.causal(x['q'], x['k'], x['v'], ref.C_SCALE, 0, T, H)
    g = lambda o, s: ref.causal_gamma(o, s, f['n'], T)                                         # noqa: E731
    check('c_out', out.t, f['out'], f['S_out'], dtype, g('c_out', f), tag)
    check('c_lse', lse.t, f['lse'], f['S_lse'], 'float32', g('c_lse', f), tag)
    assert not bool(out.t[0].any()) and not bool(lse.t[..., 0].any()), tag + ': row 0 sees the zero slot alone'
    dout = Guard((T, B, E), td, os_, dev(x['dout'], td))
    dqkv, delta = Guard((T, B, 3 * E), td), Guard((B, H, T), F32)
    dq, dk, dv = (dqkv.t[..., i * E:(i + 1) * E] for i in range(3))
    hip.call('tell_causal_attn_bwd', q, k, v, out.t, dout.t, lse.t, dq, dk, dv, delta.t, B, H, T, 64, *st, ref.C_SCALE, hip.dt(td))
    intact(qkv, out, dout, lse, dqkv, delta)
    b = ref.causal_bwd(x['q'], x['k'], x['v'], ref.np64(out.t), x['dout'], ref.np64(lse.t), ref.C_SCALE, H)
    check('c_delta', delta.t, b['delta'], b['S_delta'], 'float32', g('c_delta', b), tag)
    for n, t in (('dq', dq), ('dk', dk), ('dv', dv)):
        check('c_' + n, t, b[n], b['S_' + n], dtype, g('c_' + n, b), tag)
    assert not bool(dk[-1].any()) and not bool(dv[-1].any()), tag + ': nobody sees the last key'
    settle()


@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('case', ref.CAUSAL_STEP, ids=[c['id'] for c in ref.CAUSAL_STEP])
def test_causal_step_forms(case, dtype):
    """(Tq, pos0, S); in (3, 5, 6) min(pos0 + i, S) clamps.  Two rows follow the S rows of k and v inside the allocation:
    zero keys (logit 0, a weight that counts) with sentinel values - a read past row S would show in out"""
    from tell_amd import hip
    Tq, pos0, S = case['form']
    B, H = 2, 2
    E, td = H * 64, tdt(dtype)
    tag = 'causal %s %s' % (case['id'], dtype)
    x = ref.causal_inputs(case, dtype)
    q = Guard((Tq, B, E), td, fill=dev(x['q'], td))
    k = Guard((S + 2, B, E), td, fill=dev(np.concatenate([x['k'], np.zeros((2, B, E))]), td))
    v = Guard((S + 2, B, E), td, fill=dev(np.concatenate([x['v'], np.full((2, B, E), SENTINEL)]), td))
    out, lse = Guard((Tq, B, E), td, (B * (E + 16), E + 16, 1)), Guard((B, H, Tq), F32)
    hip.call('tell_causal_attn_fwd', q.t, k.t, v.t, out.t, lse.t, B, H, Tq, S, 64, pos0, B * E, E, B * E, E, B * E, E,
             B * (E + 16), E + 16, ref.C_SCALE, hip.dt(td))
    intact(q, k, v, out, lse)
    f = ref.causal(x['q'], x['k'], x['v'], ref.C_SCALE, pos0, S, H)
    check('c_out', out.t, f['out'], f['S_out'], dtype, ref.causal_gamma('c_out', f, f['n'], Tq), tag)
    check('c_lse', lse.t, f['lse'], f['S_lse'], 'float32', ref.causal_gamma('c_lse', f, f['n'], Tq), tag)
    settle()


# ---------------------------------------------------------------- the copy decision of one generation step
@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('case', ref.STEP, ids=[c['id'] for c in ref.STEP])
def test_copy_step(case, dtype):
    from tell_amd import hip
    Ba, B, H, S, D = case['shape']
    E, td = H * D, tdt(dtype)
    tag = 'step %s %s' % (case['id'], dtype)
    x = ref.step_inputs(case, dtype)
    r = ref.copy_step(**x)
    q = Guard((Ba, E), td, (E + 8, 1), dev(x['q'], td))
    k = Guard((S, B, E), td, (E, S * E, 1), dev(x['k'], td))                  # stored [B,S,E]
    bk = Guard((E,), td, fill=dev(x['bias_k'], td))
    mask = None if x['mask'] is None else Guard((B, S), U8, fill=x['mask'])
    proper = None if x['proper'] is None else Guard((B, S), I8, fill=x['proper'])
    ctx, rows = Guard((B, S), I64, fill=x['ctx']), Guard((Ba,), I32, fill=x['rows'])
    ent, gen = Guard((Ba, 2), F32, fill=x['ent']), Guard((Ba,), I64, fill=x['gen'])
    hist = Guard((B, ref.HIST_LEN), I64, fill=x['hist'])
    tok, copied, prob = Guard((Ba,), I64), Guard((Ba,), U8), Guard((Ba,), F32)
    hip.call('tell_copy_step', q.t, E + 8, k.t, k.strides[0], k.strides[1], bk.t, ptr(mask), ptr(proper), ctx.t, rows.t, ent.t,
             gen.t, hist.t, ref.HIST_LEN, x['n_hist'], Ba, H, S, D, tok.t, copied.t, prob.t, hip.dt(td))
    intact(q, k, bk, mask, proper, ctx, rows, ent, gen, hist, tok, copied, prob)
    judged = np.ones(Ba, bool)
    if not case.get('tie'):                      # the condition on the inputs (asserted on the host for the whole table)
        judged = r['gap'] > 2 * ref.step_bound(r, c=max(ref.C.get('prob', 1.0), 1.0))
        assert judged.all(), tag
    for i in range(Ba):
        check('prob', prob.t[i], np.reshape(r['prob'][i], ()), r['S_prob'][i], 'float32', r['gam'][i], tag)
    assert tok.t.tolist() == r['tok'].tolist() and copied.t.bool().tolist() == r['copied'].tolist(), tag
    want_hist = x['hist'].copy()
    want_hist[:, x['n_hist']] = r['hist_col']
    assert hist.t.cpu().numpy().tolist() == want_hist.tolist(), tag + ': hist (only column n_hist of the alive rows is written)'
    if S == 0:
        assert prob.t.tolist() == [float(np.float32(1e-6))] * Ba and tok.t.tolist() == x['gen'].tolist()
    settle()


# ---------------------------------------------------------------- declined calls
def test_declined_calls_write_nothing():
    from tell_amd import hip
    B, H, T, S, D = 2, 2, 3, 8, 64
    E = H * D
    big = [Guard((4 * 520 * 130,), F32) for _ in range(12)]
    a = [g.t for g in big]
    i8 = Guard((B * 520,), I64)
    # q k bk mask proper w lse | lse dw dq dk dbk delta
    fwd = lambda **kw: declined('tell_copy_attn_fwd', a[0], a[1], kw.get('bk', a[2]), None, None, a[3], a[4], B, H, T,       # noqa: E731
                                kw.get('S', S), kw.get('D', D), B * E, E, B * E, E, kw.get('p', 0.1), SEED, SALT, kw.get('dt', 0))
    bwd = lambda **kw: declined('tell_copy_attn_bwd', a[0], a[1], kw.get('bk', a[2]), None, None, a[4], a[3], a[5], a[6], a[7],  # noqa: E731
                                a[8], B, H, T, kw.get('S', S), kw.get('D', D), B * E, E, B * E, E, kw.get('p', 0.1), SEED, SALT,
                                kw.get('dt', 0))
    for kw in (dict(D=65), dict(S=513), dict(p=1.0), dict(bk=None), dict(dt=2)):
        assert fwd(**kw) != 0 and bwd(**kw) != 0, kw
    loss = lambda variant, vc: declined('tell_copy_loss_fwd', a[0], i8.t, i8.t, T, i8.t, T, vc, variant, B, T, S, a[1], a[2],  # noqa: E731
                                        a[3], a[4], a[5])
    assert loss(3, None) != 0 and loss(2, None) != 0
    assert declined('tell_causal_attn_fwd', a[0], a[1], a[2], a[3], a[4], B, H, T, T, 32, 0, B * E, E, B * E, E, B * E, E, B * E, E,
                    0.125, 0) != 0
    assert declined('tell_causal_attn_bwd', a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], B, H, T, 32, B * E, E,
                    B * E, E, B * E, E, B * E, E, 0.125, 0) != 0
    step = lambda n_hist, Ba: declined('tell_copy_step', a[0], E, a[1], B * E, E, a[2], None, None, i8.t, i8.t, a[3], i8.t, i8.t,  # noqa: E731
                                       4, n_hist, Ba, H, S, D, i8.t, i8.t, a[4], 0)
    assert step(4, 2) != 0                       # n_hist == hist_len: the history is full
    assert step(1, 0) == 0                       # no alive row: OK, nothing launched
    torch.cuda.synchronize()
    assert all(g.untouched() for g in big) and i8.untouched()


# ---------------------------------------------------------------- through ops: the stride handling of the autograd functions
@pytest.fixture
def fp32_masters():
    import tell_amd
    prev = tell_amd.compute_dtype()
    tell_amd.set_compute_dtype(torch.float32)        # bf16 operands are then cast explicitly, not taken from the weight cache
    yield
    tell_amd.set_compute_dtype(prev)


def test_ops_copy_attention_bf16_on_sliced_projections(fp32_masters):
    """q the first third of a [T,B,3E] buffer, k the second half of [S,B,2E]: CopyAttnFn.backward makes the non-dense
    operands dense and the gradients arrive in the buffers' slices"""
    from tell_amd import ops
    case = dict(id='ops', shape=(2, 2, 5, 65, 64), mask='tail', proper='mixed', layout='dense')
    B, H, T, S, D = case['shape']
    E = H * D
    x = ref.attn_inputs(case, 'bfloat16')
    qb = torch.zeros(T, B, 3 * E, dtype=BF16, device=DEV)
    kb = torch.zeros(S, B, 2 * E, dtype=BF16, device=DEV)
    qb[..., :E], kb[..., E:] = dev(x['q'], BF16).to(DEV), dev(x['k'], BF16).to(DEV)
    qb.requires_grad_()
    kb.requires_grad_()
    w = ops.copy_attention(qb[..., :E], kb[..., E:], dev(x['bias_k'], BF16).to(DEV), dev(x['mask'], U8).to(DEV),
                           dev(x['proper'], I8).to(DEV), H)
    f = ref.copy_attn_fwd(x['q'], x['k'], x['bias_k'], x['mask'], x['proper'], H)
    g = lambda o, st: ref.attn_gamma(o, st, H, T, S, D)                                       # noqa: E731
    check('w', w.detach(), f['w'], f['S_w'], 'float32', g('w', f), 'ops.copy_attention')
    w.backward(dev(x['dw'], F32).to(DEV))
    torch.cuda.synchronize()
    # the backward is judged on the float64 lse here (the kernel's is not handed out): its own 16 + gP on top
    b = ref.copy_attn_bwd(x['q'], x['k'], x['bias_k'], x['mask'], x['proper'], H, None, f['lse'], x['dw'])
    extra = ref.attn_gamma('lse', f, H, T, S, D)
    check('dq', qb.grad[..., :E], b['dq'], b['S_dq'], 'bfloat16', g('dq', b) + extra, 'ops.copy_attention')
    check('dk', kb.grad[..., E:], b['dk'], b['S_dk'], 'bfloat16', g('dk', b) + extra, 'ops.copy_attention')
    assert not bool(qb.grad[..., E:].any()) and not bool(kb.grad[..., :E].any())
    settle()


def test_ops_causal_attention_on_a_fused_projection(fp32_masters):
    """q, k, v the thirds of one [T,B,3E] projection (non-dense): CausalAttnFn.backward's stride handling"""
    from tell_amd import ops
    case = ref.CAUSAL[2]
    B, H, T = case['shape']
    E = H * 64
    x = ref.causal_inputs(case, 'bfloat16')
    qkv = dev(np.concatenate([x['q'], x['k'], x['v']], -1), BF16).to(DEV).requires_grad_()
    out = ops.causal_attention(qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:], H, ref.C_SCALE)
    f = ref.causal(x['q'], x['k'], x['v'], ref.C_SCALE, 0, T, H)
    check('c_out', out.detach(), f['out'], f['S_out'], 'bfloat16', ref.causal_gamma('c_out', f, f['n'], T), 'ops.causal_attention')
    out.backward(dev(x['dout'], BF16).to(DEV))
    torch.cuda.synchronize()
    b = ref.causal_bwd(x['q'], x['k'], x['v'], ref.np64(out.detach()), x['dout'], f['lse'], ref.C_SCALE, H)
    extra = ref.causal_gamma('c_lse', f, f['n'], T)
    for i, n in enumerate(('dq', 'dk', 'dv')):
        check('c_' + n, qkv.grad[..., i * E:(i + 1) * E], b[n], b['S_' + n], 'bfloat16',
              ref.causal_gamma('c_' + n, b, f['n'], T) + extra, 'ops.causal_attention')
    settle()
