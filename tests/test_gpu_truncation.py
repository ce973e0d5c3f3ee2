"""GPU: min-p and locally typical sampling with a temperature (include/tell_hip.h tell_adaptive_logprob_minp / _typical,
DESIGN.md section 19) through the C ABI - member sets, sizes and picks against tell_amd.models.transformer.minp_definition /
typical_definition - and through the caption models' decode loops.

Min-p is a float32 statement (one subtract, one multiply, one comparison), so its member sets are checked exactly and no row
is skipped.  The streaming forms have the arithmetic of the full-row arg-max kernel, whose rows the tests restate; the
register form reduces lse in another order, so its log-probs may differ from those rows by 2 ulp of the largest |logit|
(test_gpu_nucleus): there a token within that distance of the threshold may fall on either side - the size is bracketed by
the two restatements (they coincide unless such a token exists), and every reported log-prob is held against the threshold
with the register arg-max kernel's maximum, exactly.

The typical rule weighs tokens in fp32 where the definition sums in fp64: the skip rule and BOUND of test_gpu_nucleus apply
(margin at the boundary, distance of u to a CDF edge; at most 5 % of the rows skipped under each rule)."""
import math

import numpy as np
import pytest
import torch

from test_gpu_nucleus import BOUND, C0, TAILS, V, _golden_nucleus_model, _nucleus
from test_gpu_sampling import DEV, _Rows, _alive, _clone

pytestmark = pytest.mark.gpu

TINY = (37, (61, 103))                                        # tail sizes not divisible by 4; register form
FORMS = ('regs', 'option', 'unaligned', 'tiny')               # register-resident | streaming by option | by alignment | tiny
TEMPS = (0.7, 1.0, 1.3)
MINP = (0.02, 0.1, 0.5, 1.0)
TAUS = (0.2, 0.9, 0.95)
# the exactness rows of the typical rule.  A CPU restatement of that test (these generators and seeds, the definition with
# float32(its own c)) skips 2 of 144 rows at N = 4 and 36 of 1152 at N = 32 (1.4 % / 3.1 %) at the boundary, 0 / 10 at a CDF edge
TYPICAL_SEEDS = {4: 40, 32: 96}


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    yield
    torch.cuda.synchronize()


def _rows(form, N, seed, head=1.0, tail=1.0, **kw):
    c0, tails = TINY if form == 'tiny' else (C0, TAILS)
    X = _Rows(N, c0, tails, seed=seed, shift=1 if form == 'unaligned' else 0, **kw)
    X.head.mul_(head)
    for t, _ in X.tl:
        t.mul_(tail)
    return X


def _opts(form):
    import tell_amd
    return tell_amd.hip.options(argmax_regs=0 if form == 'option' else 1)


def _draw_args(X, seed, step, row_ids, step_dev, N):
    N = X.N if N is None else N
    tok = torch.empty(N, dtype=torch.int32, device=DEV)
    lp = torch.empty(N, dtype=torch.float32, device=DEV)
    size = torch.empty(N, dtype=torch.int32, device=DEV)
    seed_dev = torch.tensor([seed], dtype=torch.int32, device=DEV)
    rid = None if row_ids is None else torch.as_tensor(row_ids, dtype=torch.int32).to(DEV)
    cnt = torch.tensor([step - 1], dtype=torch.int32, device=DEV) if step_dev else None
    return N, tok, lp, size, (seed_dev, rid, 0 if step_dev else step, cnt, tok, lp, size)


def _minp(X, inv_temp, m, seed, step, row_ids=None, step_dev=False, N=None):
    from tell_amd.hip import call
    N, tok, lp, size, draw = _draw_args(X, seed, step, row_ids, step_dev, N)
    call('tell_adaptive_logprob_minp', *X.args(), N, inv_temp, math.log(m), *draw)
    return tok.cpu().numpy(), lp.cpu().numpy(), size.cpu().numpy()


def _typical(X, inv_temp, tau, seed, step, row_ids=None, step_dev=False, N=None):
    from tell_amd.hip import call
    N, tok, lp, size, draw = _draw_args(X, seed, step, row_ids, step_dev, N)
    key = torch.empty(N, dtype=torch.int32, device=DEV)
    c = torch.empty(N, dtype=torch.float32, device=DEV)
    call('tell_adaptive_logprob_typical', *X.args(), N, inv_temp, tau, *draw, key, c)
    return tok.cpu().numpy(), lp.cpu().numpy(), size.cpu().numpy(), key.cpu().numpy().view(np.uint32), c.cpu().numpy()


def _key_d(key):
    return (~np.asarray(key, dtype=np.uint32)).view(np.float32)


def _u(seed, row, step):
    from tell_amd import rng
    return float(rng.sample_uniform(seed, row, step))


def _near(u, cdf):
    return float(np.min(np.abs(u - np.r_[0.0, cdf])))


# ---------------------------------------------------------------------------------------------------- min-p, exactly
@pytest.mark.parametrize('N', [4, 32])
def test_minp_members_are_exact(N):
    """nuc_size and the member set against the float32 restatement, m in {0.02, 0.1, 0.5, 1}, T in {0.7, 1, 1.3}, peaked rows
    (head x 5, tails x 5: sets of a few tokens) and flat rows (sets of tens of tokens), all four forms; no row is skipped.
    The reported log-prob is the full-row value of the token (bitwise in the streaming forms) and satisfies the threshold
    with the arg-max kernel's maximum, bitwise; the token is the definition's away from the CDF edges."""
    from tell_amd.models.transformer import minp_definition
    rows_seen = ambiguous = skipped_u = 0
    sizes = []
    for fi, form in enumerate(FORMS):
        for kind, scale in (('peaked', 5.0), ('flat', 1.0)):
            X = _rows(form, N, seed=11 * N + fi + (100 if kind == 'flat' else 0), head=scale, tail=scale, ties=kind == 'flat')
            full, _, _ = X.full()
            stream = form in ('option', 'unaligned')
            tol = 0.0 if stream else 2.0 ** -22 * float(X.head.abs().max())
            with _opts(form):
                _, am_lp = X.argmax()
                for mi, m in enumerate(MINP):
                    for ti, T in enumerate(TEMPS):
                        inv_temp = float(np.float32(1.0 / T))
                        seed, step = 4000 + 100 * mi + ti, 3 + 7 * ti + mi
                        rid = (np.arange(N) * 37 + (1 << 20)) if ti == 1 else None
                        tok, lp, size = _minp(X, inv_temp, m, seed, step, row_ids=rid, step_dev=ti == 2)
                        for r in range(N):
                            rows_seen += 1
                            u = _u(seed, int(rid[r]) if rid is not None else r, step)
                            d = minp_definition(full[r], 1.0 / inv_temp, m, u)
                            a, thr = d['a'], d['threshold']
                            eps = np.float32(2.0 * tol * inv_temp * (1 + 2.0 ** -20))
                            lo = int(((a >= thr + eps) | (a == 0)).sum())        # (a = 0, the best tokens: members in any form)
                            hi = int((a >= thr - eps).sum())
                            sizes.append(len(d['members']))
                            print('form %s %s N %d m %.2f T %.1f row %d: size %d / %d [%d, %d] token %d / %d'
                                  % (form, kind, N, m, T, r, size[r], len(d['members']), lo, hi, tok[r], d['token']))
                            assert lo <= size[r] <= hi, (form, kind, m, T, r, size[r], lo, hi)
                            if lo == hi:
                                assert size[r] == len(d['members'])
                            else:
                                ambiguous += 1
                            # the reported lp against the threshold, with the kernel's own maximum: bitwise
                            assert (np.float32(lp[r]) - np.float32(am_lp[r])) * np.float32(inv_temp) >= thr, (form, m, T, r)
                            assert a[tok[r]] >= thr - eps, (form, kind, m, T, r, tok[r])
                            if stream:
                                assert tok[r] in d['members'] and lp[r] == full[r, tok[r]], (form, m, T, r)
                            else:
                                assert abs(float(lp[r]) - float(full[r, tok[r]])) <= tol, (form, m, T, r)
                            if m == 1.0:                      # the arg-max ties: the arg-max kernel's value, bit for bit
                                assert lp[r] == am_lp[r], (form, T, r)
                            if lo != hi or _near(u, d['cdf']) < BOUND:
                                skipped_u += 1
                                continue
                            assert tok[r] == d['token'], (form, kind, m, T, r, tok[r], d['token'])
    print('rows %d, a token within the register form\'s rounding of the threshold %d, u at a CDF edge %d, sizes up to %d'
          % (rows_seen, ambiguous, skipped_u, max(sizes)))
    assert max(sizes) >= 30 and min(sizes) == 1
    assert ambiguous <= 0.01 * rows_seen and skipped_u <= 0.05 * rows_seen


@pytest.mark.parametrize('form', FORMS)
def test_minp_member_set_by_many_draws(form):
    """The member set recovered by drawing: 4 flat rows, m = 0.1, T = 1.3, 256 steps - every drawn token is a member of the
    restatement, and the draws reach every member that holds at least 2 % of the set's mass (miss chance < 1e-2 each)."""
    from tell_amd.models.transformer import minp_definition
    X = _rows(form, 4, seed=61)
    full, _, _ = X.full()
    inv_temp = float(np.float32(1.0 / 1.3))
    tol = 0.0 if form in ('option', 'unaligned') else 2.0 ** -22 * float(X.head.abs().max())
    seen = [set() for _ in range(4)]
    with _opts(form):
        for step in range(1, 257):
            tok, _, size = _minp(X, inv_temp, 0.1, 99, step)
            for r in range(4):
                seen[r].add(int(tok[r]))
    for r in range(4):
        d = minp_definition(full[r], 1.0 / inv_temp, 0.1)
        wide = set(np.nonzero(d['a'] >= d['threshold'] - np.float32(2.1 * tol * inv_temp))[0].tolist())
        prob = np.diff(np.r_[0.0, d['cdf']])
        heavy = set(d['members'][prob >= 0.02].tolist())
        print('form %s row %d: %d members, %d drawn, %d heavy' % (form, r, len(d['members']), len(seen[r]), len(heavy)))
        assert seen[r] <= wide and heavy <= seen[r] and len(d['members']) >= (2 if form == 'tiny' else 5)


def test_minp_with_a_tiny_m_is_the_whole_row_nucleus():
    """m = 1e-300 (log m = -691: every token a member, also on the peaked rows, whose lightest tokens lie 250 nats under the
    best) draws what tell_adaptive_logprob_nucleus(k = 0, p = 1) draws, token for token, under
    the CDF-edge rule: the two walk the same members in id order, but the nucleus leaves out tokens lighter than 2^-44 of
    the best one, which min-p keeps - a running sum may differ in its last bits, so a row may differ where u is within BOUND
    of a CDF edge (a flat row of 50 265 members has edges everywhere: the rule bounds the rows that DIFFER, at most 5 %)."""
    from tell_amd.models.transformer import nucleus_definition
    differ = rows = 0
    for form in FORMS[:3]:
        for scale in (1.0, 5.0):
            X = _rows(form, 32, seed=71, head=scale, tail=scale)
            full, _, _ = X.full()
            with _opts(form):
                for T in TEMPS:
                    inv_temp = float(np.float32(1.0 / T))
                    a = _minp(X, inv_temp, 1e-300, 123, 6)
                    b = _nucleus(X, 0, inv_temp, 1.0, 123, 6)
                    assert (a[2] == V).all()
                    for r in range(32):
                        rows += 1
                        if a[0][r] == b[0][r]:
                            assert a[1][r] == b[1][r], (form, T, r)
                            continue
                        differ += 1
                        d = nucleus_definition(full[r], 1.0 / inv_temp, 1.0, 0, _u(123, r, 6))
                        assert _near(_u(123, r, 6), d['cdf']) < BOUND, (form, scale, T, r, a[0][r], b[0][r])
    print('rows %d, of which min-p and the whole-row nucleus differ on %d' % (rows, differ))
    assert differ <= 0.05 * rows


# ---------------------------------------------------------------------------------------------------- typical
@pytest.mark.parametrize('N', [4, 32])
def test_typical_membership_and_pick_are_exact(N):
    """typ_c against the fp64 c within rtol = BOUND; given the kernel's c, nuc_size and the boundary key equal
    typical_definition's on every row whose mass margin at the boundary is at least BOUND, and the pick equals the
    definition's on every such row whose u is at least BOUND from a CDF edge; at most 5 % of the rows are skipped under each
    rule.  Peaked rows (head x 15, tails x 10), tau in {0.2, 0.9, 0.95}, T in {0.7, 1, 1.3}, all four forms; host step,
    device step, original-row ids.  Measured on MI355X: see the print at the end (DESIGN.md section 19 quotes it)."""
    from tell_amd.models.transformer import typical_definition
    rows_seen = skipped_m = kept = skipped_u = 0
    c_err = 0.0
    for fi, form in enumerate(FORMS):
        X = _rows(form, N, seed=TYPICAL_SEEDS[N] + fi, head=5.0, tail=5.0)
        full, _, _ = X.full()
        stream = form in ('option', 'unaligned')
        tol = 0.0 if stream else 2.0 ** -22 * float(X.head.abs().max())
        with _opts(form):
            for pi, tau in enumerate(TAUS):
                for ti, T in enumerate(TEMPS):
                    inv_temp = float(np.float32(1.0 / T))
                    seed, step = 9000 + 100 * pi + ti, 2 + 13 * ti + pi
                    rid = (np.arange(N) * 37 + (1 << 20)) if ti == 1 else None
                    tok, lp, size, key, c = _typical(X, inv_temp, tau, seed, step, row_ids=rid, step_dev=ti == 2)
                    for r in range(N):
                        rows_seen += 1
                        u = _u(seed, int(rid[r]) if rid is not None else r, step)
                        d = typical_definition(full[r], 1.0 / inv_temp, float(np.float32(tau)), c=c[r], u=u)
                        near = _near(u, d['cdf'])
                        err = abs(float(c[r]) - d['c']) / d['c']
                        c_err = max(c_err, err)
                        print('form %s N %d tau %.2f T %.1f row %d: c %.6f / %.6f (%.1e) size %d / %d margin %.3e near %.3e '
                              'token %d / %d' % (form, N, tau, T, r, c[r], d['c'], err, size[r], len(d['members']), d['margin'],
                                                 near, tok[r], d['token']))
                        assert c[r] >= 0.0 and err <= BOUND, (form, tau, T, r, c[r], d['c'])
                        if d['margin'] < BOUND:
                            skipped_m += 1
                            continue
                        assert size[r] == len(d['members']), (form, tau, T, r, size[r], len(d['members']))
                        if stream:
                            assert int(key[r]) == d['key'], (form, tau, T, r, hex(int(key[r])), hex(d['key']))
                        else:                                 # (d moves with the register form's log-probs: 2 roundings of tol)
                            assert abs(float(_key_d(key[r])) - d['boundary']) <= 2.1 * tol * inv_temp, (form, tau, T, r)
                        kept += 1
                        if near < BOUND:
                            skipped_u += 1
                            continue
                        assert tok[r] == d['token'], (form, tau, T, r, tok[r], d['token'])
                        assert abs(float(lp[r]) - float(full[r, tok[r]])) <= tol, (form, tau, T, r, lp[r], full[r, tok[r]])
    print('rows %d, skipped at the boundary %d, kept %d, skipped at a CDF edge %d; max relative error of typ_c %.2e (BOUND %.2e)'
          % (rows_seen, skipped_m, kept, skipped_u, c_err, BOUND))
    assert skipped_m <= 0.05 * rows_seen, (skipped_m, rows_seen)
    assert skipped_u <= 0.05 * kept, (skipped_u, kept)


@pytest.mark.parametrize('form', FORMS)
def test_typical_size_on_flat_rows(form):
    """Flat rows (typical sets of hundreds to thousands of tokens), nothing skipped: the size lies between the definition's
    sizes for the targets tau - BOUND and tau + BOUND (given the kernel's c), the token is a member of the larger set and
    reports its own untempered log-prob."""
    from tell_amd.models.transformer import typical_definition
    X = _rows(form, 8, seed=91, ties=True)
    full, _, _ = X.full()
    with _opts(form):
        for tau, T in ((0.2, 0.7), (0.9, 1.0), (0.95, 1.3)):
            inv_temp = float(np.float32(1.0 / T))
            tok, lp, size, key, c = _typical(X, inv_temp, tau, 99, 4)
            for r in range(X.N):
                lo = typical_definition(full[r], 1.0 / inv_temp, max(tau - BOUND, 1e-9), c=c[r])
                hi = typical_definition(full[r], 1.0 / inv_temp, min(tau + BOUND, 1.0), c=c[r])
                print('form %s tau %.2f T %.1f row %d: size %d in [%d, %d]' % (form, tau, T, r, size[r], len(lo['members']),
                                                                                len(hi['members'])))
                assert abs(float(c[r]) - lo['c']) <= BOUND * lo['c']
                assert len(lo['members']) <= size[r] <= len(hi['members']), (form, tau, T, r)
                assert tok[r] in hi['members']
                assert abs(float(lp[r]) - float(full[r, tok[r]])) <= 2e-6 * max(1.0, abs(float(lp[r])))


def test_typical_ties_at_the_boundary_enter_in_id_order():
    """Ten equally heavy head tokens (8.9 % of the mass each) over a flat rest: they tie at the smallest distance, and the cut
    goes through them - tau = 0.5 / 0.6 / 0.85 take the 6 / 7 / 9 lowest ids (margins of 1 % and more).  Sizes, keys and, over
    64 steps, the drawn tokens against the definition; both forms."""
    from tell_amd.models.transformer import typical_definition
    c0, tails = TINY
    heavy = [3, 7, 8, 12, 20, 21, 25, 30, 33, 36]
    X = _Rows(2, c0, tails, seed=1)
    X.head.zero_()
    for t, _ in X.tl:
        t.zero_()
    X.head[:, heavy] = 5.0
    full, _, _ = X.full()
    for form in ('regs', 'option'):
        with _opts(form):
            for tau, n in ((0.5, 6), (0.6, 7), (0.85, 9)):
                seen = set()
                for step in range(1, 65):
                    tok, lp, size, key, c = _typical(X, 1.0, tau, 5, step)
                    seen.update(tok.tolist())
                    for r in range(2):
                        d = typical_definition(full[r], 1.0, float(np.float32(tau)), c=c[r])
                        assert d['margin'] >= BOUND and d['members'].tolist() == heavy[:n]
                        assert size[r] == n and abs(float(lp[r]) - float(full[r, tok[r]])) <= 1e-5, (form, tau, step, r)
                        assert abs(float(_key_d(key[r])) - d['boundary']) <= 1e-5
                assert seen == set(heavy[:n]), (form, tau, sorted(seen))


# ---------------------------------------------------------------------------------------------------- both rules
@pytest.mark.parametrize('rule', ['minp', 'typical'])
def test_truncation_frequencies(rule):
    """One fixed, moderately flat distribution, 8192 rows x 3 steps = 24 576 draws (min-p: m = 0.02, T = 1; typical: tau = 0.9,
    T = 1): chi-square of the token counts against the definition's member distribution below the p ~ 1e-4 quantile (the
    acceptance level of test_nucleus_frequencies; seeded: it passes or it does not); no token outside the member set is drawn."""
    from tell_amd.models.transformer import minp_definition, typical_definition
    X = _Rows(8192, C0, TAILS, seed=5, replicate=True)
    full, _, _ = _Rows(1, C0, TAILS, seed=5, replicate=True).full()
    toks = []
    for step in (1, 2, 3):
        if rule == 'minp':
            tok, lp, size = _minp(X, 1.0, 0.02, 31337, step)
        else:
            tok, lp, size, key, c = _typical(X, 1.0, 0.9, 31337, step)
            assert (key == key[0]).all() and (c == c[0]).all()
        assert (size == size[0]).all()
        np.testing.assert_allclose(lp, full[0, tok], rtol=1e-6, atol=2e-6)
        toks.append(tok)
    n = int(size[0])
    if rule == 'minp':
        d = minp_definition(full[0], 1.0, 0.02)
        lo = int((d['a'] >= d['threshold'] + np.float32(1e-5)).sum())       # (register form: see the module's note)
        hi = int((d['a'] >= d['threshold'] - np.float32(1e-5)).sum())
        assert lo <= n <= hi and (lo != hi or n == len(d['members']))
        members = np.sort(np.argsort(-d['a'], kind='stable')[:n])
    else:
        d = typical_definition(full[0], 1.0, float(np.float32(0.9)), c=c[0])
        if d['margin'] >= BOUND:
            assert n == len(d['members'])
        assert abs(n - len(d['members'])) <= 1
        members = np.sort(d['order'][:n])
    row = full[0].astype(np.float64)
    prob = np.exp(row[members] - row.max())
    prob /= prob.sum()
    tok = np.concatenate(toks)
    assert len(tok) >= 20000 and np.isin(tok, members).all()
    cnt = np.bincount(np.searchsorted(members, tok), minlength=len(members)).astype(np.float64)
    exp = prob * len(tok)
    big = exp >= 5
    o = np.r_[cnt[big], cnt[~big].sum()]
    e = np.r_[exp[big], exp[~big].sum()]
    chi2 = ((o - e) ** 2 / np.maximum(e, 1e-12)).sum()
    dof = len(o) - 1
    print('%s: %d members, %d bins, chi2 %.1f' % (rule, len(members), len(o), chi2))
    assert dof >= 20
    assert chi2 < dof + 3.72 * np.sqrt(2 * dof) + 8, (chi2, dof)


@pytest.mark.parametrize('rule', ['minp', 'typical'])
def test_truncation_kernel_determinism(rule):
    """Host step against the device counter of a captured step, inside a hipGraph against eager, 32 rows against the same rows
    inside 128, and compacted rows with their original ids against the full batch: bitwise, every output."""
    import tell_amd
    from tell_amd.hip import call
    X = _Rows(128, C0, TAILS, seed=29)
    sel = np.array([5, 17, 18, 40, 77, 100, 127])
    Y = _Rows(len(sel), C0, TAILS, seed=1)
    Y.head.copy_(X.head[sel])
    for (ty, _), (tx, _) in zip(Y.tl, X.tl):
        ty.copy_(tx[sel])
    value = 0.1 if rule == 'minp' else 0.9
    run_rule = _minp if rule == 'minp' else _typical
    name = 'tell_adaptive_logprob_' + rule
    for form in ('regs', 'option'):
        with _opts(form):
            a = run_rule(X, 1.0, value, 77, 12)
            b = run_rule(X, 1.0, value, 77, 12, step_dev=True)
            c = run_rule(X, 1.0, value, 77, 12, N=32)
            y = run_rule(Y, 1.0, value, 77, 12, row_ids=sel)
            for x0, x1, x2, x3 in zip(a, b, c, y):
                assert np.array_equal(x0, x1) and np.array_equal(x0[:32], x2) and np.array_equal(x0[sel], x3), form
            tok = torch.empty(128, dtype=torch.int32, device=DEV)
            lp = torch.empty(128, dtype=torch.float32, device=DEV)
            seed = torch.tensor([77], dtype=torch.int32, device=DEV)
            cnt = torch.tensor([11], dtype=torch.int32, device=DEV)
            args = X.args()
            par = math.log(value) if rule == 'minp' else value
            extra = (None,) if rule == 'minp' else (None, None, None)
            run = lambda: call(name, *args, 128, 1.0, par, seed, None, 0, cnt, tok, lp, *extra)       # noqa: E731
            run()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                with tell_amd.hip.bound_stream():
                    run()
            tok.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(tok.cpu().numpy(), a[0]) and np.array_equal(lp.cpu().numpy(), a[1]), form
            cnt.fill_(12)                                       # the next step: other draws from the same graph
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(tok.cpu().numpy(), run_rule(X, 1.0, value, 77, 13)[0])
            assert not np.array_equal(tok.cpu().numpy(), a[0])


def test_entry_points_refuse_bad_arguments():
    from tell_amd.hip import call
    X = _Rows(2, *TINY, seed=1)
    _, tok, lp, size, draw = _draw_args(X, 1, 1, None, False, None)
    for bad in (0.5, float('nan')):
        with pytest.raises(RuntimeError, match='log_minp'):
            call('tell_adaptive_logprob_minp', *X.args(), 2, 1.0, bad, *draw)
    for bad in (0.0, 1.5, -0.1, float('nan')):
        with pytest.raises(RuntimeError, match='tau'):
            call('tell_adaptive_logprob_typical', *X.args(), 2, 1.0, bad, *draw, None, None)
    for name, extra in (('tell_adaptive_logprob_minp', ()), ('tell_adaptive_logprob_typical', (None, None))):
        with pytest.raises(RuntimeError, match='inv_temp'):
            call(name, *X.args(), 2, 0.0, -1.0 if 'minp' in name else 0.5, *draw, *extra)


# ---------------------------------------------------------------------------------------------------- the models
RULES = {'minp': dict(sampling_minp=0.1), 'typical': dict(sampling_typical=0.9)}


@pytest.mark.parametrize('rule', sorted(RULES))
def test_golden_faces_objects_truncation_flows(golden, rule):
    """transformer_faces_objects with sampling_minp = 0.1 / sampling_typical = 0.9 (fp32 golden weights): captions finish; the
    cached flow (eager first step + captured replays), the same flow with graphs off and the reference's control flow give
    the same ids under one seed, captured == eager bit for bit; another seed gives other captions; the capture is keyed by the
    rule; teacher-forcing the model on the sampled prefix, every token lies in the definition's member set of its step (the
    teacher-forced log-probs come from other kernels than the decode step's: a token that only enters the set widened by
    that difference counts as skipped, at most 5 %); prefix= rows start with their prefix; attention=True returns the maps."""
    import tell_amd
    from tell_amd.models.transformer import minp_definition, typical_definition
    T = 0.9
    value = list(RULES[rule].values())[0]
    model, batch = _golden_nucleus_model(golden, 'faces_objects', sampling_topk=0, sampling_temp=T, **RULES[rule])
    outs = []
    keep = tell_amd.graphs.ENABLED
    try:
        for fast, graphed in ((True, True), (True, True), (True, False), (False, True)):
            model.fast_generation, tell_amd.graphs.ENABLED = fast, graphed
            torch.manual_seed(123)
            outs.append(model.generate(**batch()))
    finally:
        tell_amd.graphs.ENABLED = keep
    sigs = list(model.__dict__.get('_decode_graphs', {}).items())
    assert sigs and all(h['graph'] not in (None, False) for _, h in sigs), [h.get('error') for _, h in sigs]
    assert all((rule, 0, T, value) in sig for sig, _ in sigs)
    ids = outs[0]['gen_ids'].cpu()
    for o in outs[1:]:
        assert torch.equal(o['gen_ids'].cpu(), ids)
    assert torch.equal(outs[1]['log_probs'], outs[2]['log_probs']) and torch.equal(outs[0]['log_probs'], outs[1]['log_probs'])
    assert ids.shape[1] > 2
    alive = _alive(ids)
    assert ((ids == 2).any(1) | (ids.shape[1] >= 100)).all()               # every caption ends in </s> (or at gen_len)
    torch.manual_seed(124)
    model.fast_generation = True
    assert not torch.equal(model.generate(**batch())['gen_ids'].cpu(), ids)
    with torch.no_grad():
        b = batch()
        _, _, ctx = model._forward(b['context'], b['image'], b['caption'], b.get('face_embeds'), b.get('obj_embeds'))
        out = model.decoder({'roberta': ids[:, :-1].to(DEV)}, ctx)
        lp = model.decoder.get_normalized_probs((out[0], None), log_probs=True).float().cpu()
    got = outs[0]['log_probs'].cpu()
    seen = skipped = 0
    for bi in range(ids.shape[0]):
        for t in range(ids.shape[1] - 1):
            if not alive[bi, t]:
                continue
            seen += 1
            token = int(ids[bi, t + 1])
            assert abs(float(got[bi, t]) - float(lp[bi, t, token]) / T) <= 2e-4
            row = lp[bi, t].numpy()
            if rule == 'minp':
                d = minp_definition(row, T, value)
                inside = token in d['members']
                wide = d['a'][token] >= d['threshold'] - np.float32(1e-3)       # (2e-4 on two log-probs, / T)
            else:
                inside = token in typical_definition(row, T, value)['members']
                wide = token in typical_definition(row, T, min(1.0, value + 2 * BOUND))['members']
            assert inside or wide, (bi, t, token)
            skipped += 0 if inside else 1
    print('%s: %d tokens, %d only in the widened set' % (rule, seen, skipped))
    assert skipped <= 0.05 * seen
    with pytest.raises(ValueError, match='sampling_' + rule):
        model.generate(**batch(), beam_size=2)
    # a forced prefix (the first tokens of the sampled captions; row 0 free), and the attention maps
    P = 3
    pfx = ids[:, 1:1 + P].clone()
    pfx[0] = 1
    for r in range(1, pfx.shape[0]):                           # (a prefix stops at </s>, and at a sampled pad id)
        stop = ((pfx[r] == 2).nonzero().flatten() + 1).tolist() + (pfx[r] == 1).nonzero().flatten().tolist() + [P]
        pfx[r, min(stop):] = 1
    plens = (pfx != 1).sum(1).tolist()
    assert plens[0] == 0 and max(plens) >= 2, plens
    torch.manual_seed(123)
    forced = model.generate(**batch(), prefix=pfx.to(DEV))
    fid = forced['gen_ids'].cpu()
    assert forced['prefix_len'].tolist() == plens
    for r, n in enumerate(plens):
        assert torch.equal(fid[r, 1:1 + n], pfx[r, :n]), r
    torch.manual_seed(123)
    am = model.generate(**batch(), attention=True)
    assert torch.equal(am['gen_ids'].cpu(), ids)
    B = ids.shape[0]
    assert am['attn_steps'].shape == (B,) and am['attns']
    for name, maps in am['attns'].items():
        assert maps.dim() == 4 and maps.shape[0] == B and maps.shape[1] >= int(am['attn_steps'].max()), (name, tuple(maps.shape))
        assert torch.isfinite(maps).all()


def test_transformer_glove_takes_the_rules(golden):
    """TransformerGloveModel decodes through the same cached generator: both rules generate, repeat under one seed and differ
    across seeds (golden weights, T = 1.5)."""
    import tell_amd
    from tell_amd.build import build_decoder
    from tell_amd.models import TransformerGloveModel
    from tell_amd.modules import AdaptiveLoss
    from test_gpu_decoder import DEC_KW, _PoolResnet
    tell_amd.set_compute_dtype(torch.float32)
    fx = golden('model_transformer_glove')
    ins = fx['in']
    batch = lambda: dict(image=ins['image'].to(DEV), caption={'roberta': ins['caption'].to(DEV)},   # noqa: E731
                         context_vectors=ins['context_vectors'].to(DEV))
    for rule, opt in sorted(RULES.items()):
        model = TransformerGloveModel(None, build_decoder('flattened', article_dim=300, **DEC_KW), AdaptiveLoss(1), vocab_size=600,
                                      resnet=_PoolResnet(), sampling_topk=0, sampling_temp=1.5, **opt).eval()
        own = model.state_dict()
        model.load_state_dict({k: v for k, v in fx['sd'].items() if k in own}, strict=False)
        model.to(DEV)
        torch.manual_seed(7)
        a = model.generate(**batch())
        torch.manual_seed(7)
        b = model.generate(**batch())
        assert torch.equal(a['gen_ids'], b['gen_ids']) and torch.equal(a['log_probs'], b['log_probs']), rule
        assert a['gen_ids'].shape[1] > 2
        torch.manual_seed(8)
        c = model.generate(**batch())
        assert c['gen_ids'].shape != a['gen_ids'].shape or not torch.equal(c['gen_ids'], a['gen_ids']), rule


def test_fullsize_truncation_lanes_and_captured_steps():
    """Full-size faces_objects in bf16 with sampling_minp = 0.1, then sampling_typical = 0.9: the single-step and multi-step
    graphs are recorded under the rule's key; one seed gives one result, another seed another; generate_lanes equals
    `generate` batch by batch under one torch seed."""
    import tell_amd
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    try:
        torch.manual_seed(0)
        model = build_model('faces_objects', sampling_topk=0, sampling_minp=0.1).to(DEV).eval()
        batches = [synthetic_batch(4, 64, 9, True, seed=81 + i, device=DEV) for i in range(3)]

        def gen(seed, b):
            torch.manual_seed(seed)
            out = model.generate(**_clone(b))
            torch.cuda.synchronize()
            return out['gen_ids'].cpu(), out['log_probs'].cpu()
        for rule, value in (('minp', 0.1), ('typical', 0.9)):
            model.sampling_minp, model.sampling_typical = (value, None) if rule == 'minp' else (None, value)
            a, a2 = gen(11, batches[0]), gen(11, batches[0])
            assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1]), rule
            assert not torch.equal(gen(12, batches[0])[0], a[0]), rule
            hs = [(sig, h) for sig, h in model.__dict__['_decode_graphs'].items() if (rule, 0, 1.0, value) in sig]
            assert hs and all(h['graph'] not in (None, False) for _, h in hs), [h.get('error') for _, h in hs]
            assert any(any(isinstance(k, tuple) and k[0] == 'multi' and v for k, v in h.items()) for _, h in hs), rule
            torch.manual_seed(21)
            alone = [model.generate(**_clone(b)) for b in batches]
            torch.cuda.synchronize()
            torch.manual_seed(21)
            seen = 0
            for i, (_, out) in enumerate(model.generate_lanes((_clone(b) for b in batches), lanes=2)):
                torch.cuda.synchronize()
                assert torch.equal(out['gen_ids'], alone[i]['gen_ids']), (rule, i)
                assert torch.equal(out['log_probs'], alone[i]['log_probs']), (rule, i)
                seen += 1
            assert seen == len(batches)
    finally:
        tell_amd.set_compute_dtype(torch.float32)
