"""tests/copy_ref.py judged without a GPU: the float64 reference against an independent
formulation (torch.softmax, scatter_add, cross_entropy in float64, autograd for every gradient) over the whole case
table at rtol 1e-10; vocab_count against len(unique); an fp32 emulation of each op (the same formulas with every product,
exp and sequential sum rounded to fp32) inside the bounds at c = 1, so the gammas are not too small; eight mutants of the
reference, each of which must break a bound somewhere on the table; the tie-gap condition of the copy-step cases and the
rounding of the inputs."""
import math

import numpy as np
import pytest
import torch

import copy_ref as ref

F64 = torch.float64
RTOL = 1e-10


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(F64)


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    scale = np.abs(want[ok]).max() if ok.any() and want[ok].size else 0.0
    assert np.allclose(got[ok], want[ok], rtol=RTOL, atol=RTOL * max(scale, 1e-300)), \
        (what, float(np.abs(got[ok] - want[ok]).max()))


def outside(out, got, want, S, dtype, gam, c=1.0):
    """does any element of got leave the bound around want (a NaN pattern that differs counts)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return True
    ok = ~np.isnan(want)
    return bool((np.abs(got - want)[ok] > np.broadcast_to(ref.bound(out, want, S, dtype, gam, c), want.shape)[ok]).any())


# ---------------------------------------------------------------- independent formulations (torch float64 + autograd)
def torch_copy_attn(q, k, bk, mask, proper, H, keep):
    T, B, E = q.shape
    S, D = k.shape[0], E // H
    qh = q.reshape(T, B, H, D).permute(1, 2, 0, 3)
    kx = torch.cat([k, bk.reshape(1, 1, E).expand(1, B, E), torch.zeros(1, B, E, dtype=F64)])
    lg = qh @ kx.reshape(S + 2, B, H, D).permute(1, 2, 3, 0)
    if mask is not None:
        m = torch.cat([torch.from_numpy(mask).bool(), torch.zeros(B, 2, dtype=torch.bool)], 1)
        lg = lg.masked_fill(m[:, None, None, :], -math.inf)
    P = torch.softmax(lg, -1)
    if keep is not None:
        P = P * tt(keep)
    w = P.mean(1)[:, :, :S]
    if proper is not None:
        w = w.masked_fill((torch.from_numpy(proper) < 1)[:, None, :], 0.0)
    return w, torch.logsumexp(lg, -1)


@pytest.mark.parametrize('p', ref.P_DROP)
@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('case', ref.ATTN, ids=[c['id'] for c in ref.ATTN])
def test_copy_attention_against_autograd(case, dtype, p):
    B, H, T, S, D = case['shape']
    x = ref.attn_inputs(case, dtype)
    keep, f = ref.attn_ref(case, dtype, p)
    q, k, bk = (tt(x[n]).requires_grad_() for n in ('q', 'k', 'bias_k'))
    w, lse = torch_copy_attn(q, k, bk, x['mask'], x['proper'], H, keep)
    close(f['w'], w.detach().numpy(), 'w')
    close(f['lse'], lse.detach().numpy(), 'lse')
    w.backward(tt(x['dw']))
    b = ref.copy_attn_bwd(x['q'], x['k'], x['bias_k'], x['mask'], x['proper'], H, keep, f['lse'], x['dw'])
    close(b['dq'], q.grad.numpy(), 'dq')
    close(b['dk'], k.grad.numpy(), 'dk')
    close(b['dbk'].sum(0), bk.grad.numpy(), 'dbias_k')
    if case['mask'] == 'padrow':                       # a fully padded batch row: exact zeros, lse of the virtual columns
        assert not f['w'][1].any() and not b['dk'][:, 1].any()
        q1 = x['q'][:, 1].reshape(T, H, D)
        v = (q1 * x['bias_k'].reshape(1, H, D)).sum(-1)                       # [T,H]
        close(f['lse'][1], np.logaddexp(v, 0.0).T, 'lse of a padded row')
    if case['id'] == 'spread60':
        assert 45 < f['spread'] < 90


def torch_copy_loss(w, ctx, tgt, cm, variant):
    """pointer_loss as the model states it: unique, scatter_add, a loop over the entity indices"""
    B, T, S = w.shape
    ids = torch.cat([torch.from_numpy(ctx), torch.from_numpy(tgt)], 1)
    uniq = ids.unique()
    V = len(uniq)
    remap = {int(v): i for i, v in enumerate(uniq.tolist())}
    cidx = torch.tensor([[remap[int(v)] for v in row] for row in ctx], dtype=torch.long).reshape(B, S)
    tidx = torch.tensor([[remap[int(v)] for v in row] for row in tgt], dtype=torch.long)
    probs = w.new_zeros(B, T, V).scatter_add(2, cidx.unsqueeze(1).expand(B, T, S), w)
    lprobs = torch.where(probs > 0, torch.log(probs.clamp_min(1e-300)), torch.zeros_like(probs)).view(B * T, V)
    nt = tidx.reshape(-1, 1)
    cmt = torch.from_numpy(cm)
    loss = w.new_zeros(())
    for i in range(1, int(cmt.max()) + 1):
        sel = (cmt == i).view(-1)
        if variant == 1:
            loss = loss + (-lprobs[sel].gather(-1, nt[sel])).mean()
        else:
            loss = loss + torch.nn.functional.cross_entropy(lprobs[sel], nt[sel].squeeze(1))
    return loss, probs, V


@pytest.mark.parametrize('variant', [1, 2])
@pytest.mark.parametrize('case', ref.LOSS, ids=[c['id'] for c in ref.LOSS])
def test_copy_loss_against_autograd(case, variant):
    B, T, S = case['shape']
    x = ref.loss_inputs(case)
    V = ref.vocab_count(x['ctx'], x['tgt'], case['vocab'])
    ids = np.concatenate([x['ctx'].reshape(-1), x['tgt'].reshape(-1)])
    legal = bool(((ids >= 0) & (ids < case['vocab'])).all())
    assert V == (len(np.unique(ids)) if legal else -1)
    assert (case['kind'] in ('oov', 'negative')) == (not legal)
    r = ref.copy_loss(x['w'], x['ctx'], x['tgt'], x['cm'], variant, V)
    w = tt(x['w']).requires_grad_()
    loss, probs, Vt = torch_copy_loss(w, x['ctx'], x['tgt'], x['cm'], variant)
    if case['kind'] == 'gap':
        assert math.isnan(float(loss)) and math.isnan(float(r['loss']))
        return
    if not legal and variant == 2:
        assert math.isnan(float(r['loss'])) and np.isnan(r['term'][x['cm'] >= 1]).all()
        assert np.isfinite(r['dw']).all()
        return
    close(r['loss'], loss.detach().numpy(), 'loss')
    (loss * 0.37).backward()
    close(r['dw'], w.grad.numpy(), 'dw')
    ent = x['cm'] >= 1
    pr = probs.detach().numpy()
    tcol = np.searchsorted(np.unique(ids), x['tgt'])
    close(r['p_target'], np.where(ent, np.take_along_axis(pr, tcol[..., None], -1)[..., 0], 0.0), 'p_target')
    if variant == 2:                                     # Z = sum_{p>0} p + V - n_pos over the V columns
        close(r['z'], np.where(ent, pr.sum(-1) + (pr <= 0).sum(-1), 0.0), 'z')
    if case['id'] == 'rich':
        assert r['p_target'][0, 2] == 0 and r['p_target'][1, 4] == 0 and r['top'] == 5
        assert not r['dw'][x['cm'] < 1].any() and (x['cm'] == -1).any() and (x['cm'] == 0).any()
    if case['id'] == 'S512_equal':
        assert r['n'] == 512
    if case['id'] == 'S257':
        assert r['n'] >= 3 and (x['ctx'][:, [0, 255, 256]] == 50).all()


@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('case', ref.ENT + [ref.ENT_LOGITS], ids=[c['id'] for c in ref.ENT + [ref.ENT_LOGITS]])
def test_entity_head_against_autograd(case, dtype):
    B, T, E = case['shape']
    x = ref.ent_inputs(case, dtype)
    r = ref.entity_head(x['x'], x['w'], x['bias'], x['cm'], dbias0=x['dbias0'])
    xt, wt, bt = (tt(x[n]).requires_grad_() for n in ('x', 'w', 'bias'))
    lg = xt.transpose(0, 1) @ wt.t() + bt
    close(r['logits'], lg.detach().numpy(), 'logits')
    tgt = torch.from_numpy(np.minimum(x['cm'], 1))
    assert r['nvalid'] == int((x['cm'] != -1).sum())
    if case['cm'] == 'ignored':
        assert math.isnan(float(r['loss'])) and not r['dx'].any() and not r['dlogits'].any()
        return
    loss = torch.nn.functional.cross_entropy(lg.reshape(-1, 2), tgt.reshape(-1), ignore_index=-1)
    close(r['loss'], loss.detach().numpy(), 'loss')
    lg.retain_grad()
    (loss * 0.37).backward()
    close(r['dlogits'], lg.grad.numpy(), 'dlogits')
    close(r['dx'], xt.grad.numpy(), 'dx')
    close(r['dw'], wt.grad.numpy(), 'dw')
    close(r['dbias'], bt.grad.numpy() + x['dbias0'], 'dbias')


def torch_causal(q, k, v, scale, pos0, S, H):
    Tq, B, E = q.shape
    D = E // H
    qh = q.reshape(Tq, B, H, D).permute(1, 2, 0, 3) * scale
    kh, vh = (t[:S].reshape(S, B, H, D).permute(1, 2, 0, 3) for t in (k, v))
    lg = qh @ kh.transpose(-1, -2)
    hide = torch.arange(S)[None, :] >= (pos0 + torch.arange(Tq))[:, None]
    lg = torch.cat([torch.zeros(B, H, Tq, 1, dtype=F64), lg.masked_fill(hide, -math.inf)], -1)
    out = torch.softmax(lg, -1)[..., 1:] @ vh
    return out.permute(2, 0, 1, 3).reshape(Tq, B, E), torch.logsumexp(lg, -1)


@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('case', ref.CAUSAL + ref.CAUSAL_STEP, ids=[c['id'] for c in ref.CAUSAL + ref.CAUSAL_STEP])
def test_causal_against_autograd(case, dtype):
    x = ref.causal_inputs(case, dtype)
    Tq, B, E = x['q'].shape
    H = E // 64
    pos0, S = (case['form'][1:] if 'form' in case else (0, Tq))
    f = ref.causal(x['q'], x['k'], x['v'], ref.C_SCALE, pos0, S, H)
    q, k, v = (tt(x[n]).requires_grad_() for n in ('q', 'k', 'v'))
    out, lse = torch_causal(q, k, v, ref.C_SCALE, pos0, S, H)
    close(f['out'], out.detach().numpy(), 'out')
    close(f['lse'], lse.detach().numpy(), 'lse')
    if 'form' in case:
        return
    assert not f['out'][0].any() and not f['lse'][..., 0].any()               # row 0: the zero slot alone
    out.backward(tt(x['dout']))
    b = ref.causal_bwd(x['q'], x['k'], x['v'], f['out'], x['dout'], f['lse'], ref.C_SCALE, H)
    for n, t in (('dq', q), ('dk', k), ('dv', v)):
        close(b[n], t.grad.numpy(), n)
    assert not b['dk'][-1].any() and not b['dv'][-1].any()                   # nobody sees the last key
    if case.get('order'):
        lg = np.einsum('tbhd,sbhd->bhts', (x['q'] * ref.C_SCALE).reshape(Tq, B, H, 64), x['k'].reshape(Tq, B, H, 64))
        d = np.diff(lg[:, :, -1, :], axis=-1) * case['order']
        assert (d > 0).all() and 40 < np.abs(lg).max() < 90


def torch_copy_step(x):
    """softmax + scatter_add over a dense id axis; ties to the lower id by arg-max over ids in increasing order"""
    q, k = tt(x['q']), tt(x['k'])
    Ba, E = q.shape
    S, B = k.shape[0], k.shape[1]
    H = x['H']
    tok, cop, prob = [], [], []
    col = x['hist'][:, x['n_hist']].copy()
    for i, b in enumerate(x['rows'].tolist()):
        w, _ = torch_copy_attn(q[i].reshape(1, 1, E), k[:, b:b + 1], tt(x['bias_k']),
                               None if x['mask'] is None else x['mask'][b:b + 1],
                               None if x['proper'] is None else x['proper'][b:b + 1], H, None)
        sums = torch.zeros(2000, dtype=F64).scatter_add(0, torch.from_numpy(x['ctx'][b]).long(), w[0, 0])
        present = torch.zeros(2000, dtype=torch.bool)
        present[torch.from_numpy(x['ctx'][b]).long()] = True
        sums = torch.where(present, sums, torch.full_like(sums, -1.0))
        bid = int(sums.argmax()) if S else 0                                   # the first (lowest) id of the largest sum
        top = float(sums.max()) if S else -1.0
        empty = top < float(np.float32(1e-6))
        should = bool(x['ent'][i][1] > x['ent'][i][0]) and not empty and bid not in x['hist'][b, :x['n_hist']].tolist()
        col[b] = bid if should else -1
        tok.append(bid if should else int(x['gen'][i]))
        cop.append(should)
        prob.append(float(np.float32(1e-6)) if empty else top)
    return tok, cop, prob, col


@pytest.mark.parametrize('dtype', ref.DTYPES)
@pytest.mark.parametrize('case', ref.STEP, ids=[c['id'] for c in ref.STEP])
def test_copy_step_against_scatter_add(case, dtype):
    x = ref.step_inputs(case, dtype)
    r = ref.copy_step(**x)
    tok, cop, prob, col = torch_copy_step(x)
    if not case.get('tie'):                                  # (an exact tie of two float64 sums in another order may not tie)
        assert r['tok'].tolist() == tok and r['copied'].tolist() == cop and r['hist_col'].tolist() == col.tolist()
    close(r['prob'], np.array(prob), 'prob')
    assert sorted(x['rows'].tolist()) != x['rows'].tolist() and len(set(x['rows'].tolist())) == len(x['rows'])
    S = case['shape'][3]
    if S == 0:
        assert r['prob'].tolist() == [float(np.float32(1e-6))] * 3 and not r['copied'].any() and r['tok'].tolist() == [11, 12, 13]
    if case.get('tie'):
        assert (r['gap'] == 0).all() and r['tok'].tolist() == [80, 80, 80] and r['copied'].all()
        assert np.array_equal(x['k'][2], x['k'][9])
    if case.get('ent_tie'):
        assert r['copied'].tolist() == [True, False, True]
    if case.get('in_hist'):
        assert r['copied'].tolist() == [False, True, True] and r['tok'][0] == 11
    if case.get('last_hist'):
        assert x['n_hist'] == ref.HIST_LEN - 1


def test_tie_gap_condition():
    """a non-tie case is in the table only if its best-to-second gap exceeds twice the bound of prob (at c = 1, or the
    pinned c); at most one alive row in ten may fail that and is then not judged on its token"""
    n = dropped = 0
    for case in ref.STEP:
        if case.get('tie'):
            continue
        for dtype in ref.DTYPES:
            r = ref.copy_step(**ref.step_inputs(case, dtype))
            b = ref.step_bound(r, c=max(ref.C.get('prob', 1.0), 1.0))
            n += len(b)
            dropped += int((r['gap'] <= 2 * b).sum())
    assert dropped * 10 <= n, (dropped, n)
    assert dropped == 0, 'pick other seeds: %d of %d rows inside twice the bound' % (dropped, n)


def test_inputs_are_rounded_to_the_compute_dtype():
    def representable(a, dtype):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return torch.equal(t.to(getattr(torch, dtype)).double(), t)
    for dtype in ref.DTYPES:
        x = ref.attn_inputs(ref.ATTN[4], dtype)
        assert all(representable(x[n], dtype) for n in ('q', 'k', 'bias_k'))
        x = ref.causal_inputs(ref.CAUSAL[4], dtype)
        assert all(representable(x[n], dtype) for n in ('q', 'k', 'v', 'dout'))
        x = ref.step_inputs(ref.STEP[6], dtype)
        assert all(representable(x[n], dtype) for n in ('q', 'k', 'bias_k'))
        assert representable(ref.ent_inputs(ref.ENT[3], dtype)['x'], dtype)
    assert not representable(ref.attn_inputs(ref.ATTN[4], 'float32')['q'], 'bfloat16')
    assert representable(ref.loss_inputs(ref.LOSS[2])['w'], 'float32')


# ---------------------------------------------------------------- fp32 emulation and mutants, op by op
def attn_outputs(case, dtype, p, dt=np.float64, mutant=None, lse=None):
    """every output of a copy-attention case with its S and gamma: [(name, value, S, gamma)]; the backward on `lse`"""
    B, H, T, S, D = case['shape']
    x = ref.attn_inputs(case, dtype)
    keep = ref.keep_factors(ref.SEED, ref.SALT, B, H, T, S, p, mutant)
    f = ref.copy_attn_fwd(x['q'], x['k'], x['bias_k'], x['mask'], x['proper'], H, keep, dt, mutant)
    lse = f['lse'] if lse is None else lse
    b = ref.copy_attn_bwd(x['q'], x['k'], x['bias_k'], x['mask'], x['proper'], H, keep, lse, x['dw'], dt, mutant)
    g = lambda o, st: ref.attn_gamma(o, st, H, T, S, D)                                      # noqa: E731
    return [('w', f['w'], f['S_w'], g('w', f)), ('lse', f['lse'], f['S_lse'], g('lse', f))] + \
        [(o, b[o], b['S_' + o], g(o, b)) for o in ('delta', 'dq', 'dk', 'dbk')], lse


def loss_outputs(case, variant, dt=np.float64, mutant=None):
    B, T, S = case['shape']
    x = ref.loss_inputs(case)
    V = ref.vocab_count(x['ctx'], x['tgt'], case['vocab'])
    r = ref.copy_loss(x['w'], x['ctx'], x['tgt'], x['cm'], variant, V, dt=dt, mutant=mutant)
    g = lambda o: ref.loss_gamma(o, r['n'], B, T, S, r['top'])                               # noqa: E731
    return [(o, r[o], r['S_' + o], g(o)) for o in ('p_target', 'z', 'term', 'scale', 'loss')] + \
        [('loss_dw', r['dw'], r['S_dw'], g('loss_dw'))]


def ent_outputs(case, dtype, dt=np.float64, mutant=None, logits=None):
    B, T, E = case['shape']
    x = ref.ent_inputs(case, dtype)
    r = ref.entity_head(x['x'], x['w'], x['bias'], x['cm'], logits=logits, dbias0=x['dbias0'], dt=dt, mutant=mutant)
    names = dict(ent_logits='logits', ent_loss='loss', ent_dlogits='dlogits', ent_dx='dx', ent_dw='dw', ent_db='dbias')
    return [(o, r[n], r['S_' + n], ref.ent_gamma(o, B, T, E)) for o, n in names.items()], r['logits']


def causal_outputs(case, dtype, dt=np.float64, mutant=None, given=None):
    x = ref.causal_inputs(case, dtype)
    Tq, B, E = x['q'].shape
    H = E // 64
    pos0, S = (case['form'][1:] if 'form' in case else (0, Tq))
    f = ref.causal(x['q'], x['k'], x['v'], ref.C_SCALE, pos0, S, H, dt, mutant)
    outs = [('c_out', f['out'], f['S_out'], ref.causal_gamma('c_out', f, f['n'], Tq)),
            ('c_lse', f['lse'], f['S_lse'], ref.causal_gamma('c_lse', f, f['n'], Tq))]
    if 'form' not in case:
        out, lse = given if given is not None else (f['out'], f['lse'])
        b = ref.causal_bwd(x['q'], x['k'], x['v'], out, x['dout'], lse, ref.C_SCALE, H, dt, mutant)
        outs += [('c_' + o, b[o], b['S_' + o], ref.causal_gamma('c_' + o, b, f['n'], Tq)) for o in ('delta', 'dq', 'dk', 'dv')]
    return outs, (f['out'], f['lse'])


def _emulated(ref_outs, emu_outs, tag):
    for (o, want, S, gam), (_, got, _, _) in zip(ref_outs, emu_outs):
        assert not outside(o, got, want, S, 'float32', gam, 1.0), \
            '%s %s: fp32 emulation outside the bound at c = 1 (ratio %.3f)' % (tag, o, ref.ratio(got, want, S, 'float32', gam))


@pytest.mark.parametrize('case', ref.ATTN, ids=[c['id'] for c in ref.ATTN])
def test_fp32_emulation_copy_attention(case):
    for dtype in ref.DTYPES:
        emu, lse = attn_outputs(case, dtype, 0.1, np.float32)
        want, _ = attn_outputs(case, dtype, 0.1, np.float64, lse=lse)        # the backward on the emulation's own lse
        _emulated(want, emu, case['id'])


def test_fp32_emulation_of_the_other_ops():
    for case in ref.LOSS:
        for variant in (1, 2):
            _emulated(loss_outputs(case, variant), loss_outputs(case, variant, np.float32), 'loss ' + case['id'])
    for case in ref.ENT:
        emu, logits = ent_outputs(case, 'bfloat16', np.float32)
        _emulated(ent_outputs(case, 'bfloat16', logits=logits)[0], emu, 'entity ' + case['id'])   # backward on its logits
    for case in ref.CAUSAL + ref.CAUSAL_STEP:
        emu, given = causal_outputs(case, 'float32', np.float32)
        want, _ = causal_outputs(case, 'float32', np.float64, given=given)
        _emulated(want, emu, 'causal ' + case['id'])
    for case in ref.STEP:
        x = ref.step_inputs(case, 'float32')
        want, emu = ref.copy_step(**x), ref.copy_step(dt=np.float32, **x)
        assert (np.abs(emu['prob'] - want['prob']) <= ref.step_bound(want, c=1.0)).all(), case['id']
        if not case.get('tie'):
            assert emu['tok'].tolist() == want['tok'].tolist()


def _breaks(ref_outs, mut_outs, c):
    return [o for (o, want, S, gam), (_, got, _, _) in zip(ref_outs, mut_outs)
            if outside(o, got, want, S, 'float32', gam, max(ref.C.get(o, 1.0), c))]


@pytest.mark.parametrize('mutant', ref.MUTANTS)
def test_mutants_of_the_reference_break_a_bound(mutant):
    """each wrong-answer variant leaves the bound (taken at the pinned c, at least 1) on at least one case of the table"""
    broken = []
    if mutant in ('keep_row', 'proper_gt1', 'dq_no_bias', 'drop_col_256'):
        for case in ref.ATTN:
            want, lse = attn_outputs(case, 'float32', 0.1)
            got, _ = attn_outputs(case, 'float32', 0.1, mutant=mutant, lse=lse)
            broken += [(case['id'], o) for o in _breaks(want, got, 1.0)]
    if mutant in ('causal_sees_self', 'causal_scale_once'):
        for case in ref.CAUSAL + ref.CAUSAL_STEP:
            want, given = causal_outputs(case, 'float32')
            got, _ = causal_outputs(case, 'float32', mutant=mutant, given=given)
            broken += [(case['id'], o) for o in _breaks(want, got, 1.0)]
    if mutant == 'chain_drop_last':
        for case in ref.LOSS:
            broken += [(case['id'], o) for o in _breaks(loss_outputs(case, 2), loss_outputs(case, 2, mutant=mutant), 1.0)]
    if mutant in ('chain_drop_last', 'tie_high', 'proper_gt1', 'drop_col_256'):
        for case in ref.STEP:
            x = ref.step_inputs(case, 'float32')
            want, got = ref.copy_step(**x), ref.copy_step(mutant=mutant, **x)
            if got['tok'].tolist() != want['tok'].tolist() or \
                    (np.abs(got['prob'] - want['prob']) > ref.step_bound(want, c=max(ref.C.get('prob', 1.0), 1.0))).any():
                broken.append((case['id'], 'step'))
    assert broken, mutant
    if mutant == 'tie_high':
        assert broken == [('tie', 'step')]
    if mutant == 'drop_col_256':
        assert {c for c, _ in broken} >= {'S257', 'S300', 'S511', 'S512', 'D48'} and not any(c == 'S256' for c, _ in broken)
