"""GPU: nucleus (top-p) sampling with a temperature (include/tell_hip.h tell_adaptive_logprob_nucleus)
through the C ABI on the full 50 265-token head - membership and pick against the fp64 definition
(tell_amd.models.transformer.nucleus_definition) - and through the caption models' decode loops.

The skip rule of the exactness tests.  The kernel weighs tokens in fp32 where the definition uses fp64, so the boundary may
legitimately move by a token when the cumulative weight passes within rounding of p * total, and the pick when u * sum
passes within rounding of a running sum.  BOUND = V * 2^-24 (V = 50 265 summed terms: 3.0e-3, relative to the total) is
the fp32 summation bound of a sum over the vocabulary; rows whose margin at the boundary (resp. distance of u to a CDF
edge) is below it are skipped, and AT MOST 5 % of the rows may be skipped (asserted, separately for both).  The bound asks
for peaked rows (a boundary token must hold far more than 0.3 % of the mass), so the exactness rows scale the logits up
(`_peaked`); flat rows with nuclei of thousands of tokens are covered by test_nucleus_size_on_flat_rows and the chi-square."""
import numpy as np
import pytest
import torch

from test_gpu_sampling import DEV, LAYOUTS, _Rows, _alive, _clone

pytestmark = pytest.mark.gpu

C0, TAILS = LAYOUTS['build_model']                             # the configs' cutoffs (5000, 20000) over 50 265 tokens
V = C0 + sum(TAILS)
BOUND = V * 2.0 ** -24
P_VALUES = (0.3, 0.9, 0.95)
FORMS = ('regs', 'option', 'unaligned')                        # register-resident | streaming by option | streaming (rows off 16 bytes)


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    yield
    torch.cuda.synchronize()


def _peaked(N, seed, shift=0, head=5.0, tail=5.0):
    """Rows whose distribution is peaked enough for the skip rule: randn * 15 in the head (and its cluster columns),
    randn * 10 in the tails - nuclei of a few tokens."""
    X = _Rows(N, C0, TAILS, seed=seed, shift=shift)
    X.head.mul_(head)
    for t, _ in X.tl:
        t.mul_(tail)
    return X


def _key_lp(key):
    key = np.asarray(key, dtype=np.uint32)
    bits = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7FFFFFFF), ~key)
    return bits.astype(np.uint32).view(np.float32)


def _nucleus(X, k, inv_temp, p, seed, step, row_ids=None, step_dev=False, N=None):
    from tell_amd.hip import call
    N = X.N if N is None else N
    tok = torch.empty(N, dtype=torch.int32, device=DEV)
    lp = torch.empty(N, dtype=torch.float32, device=DEV)
    size = torch.empty(N, dtype=torch.int32, device=DEV)
    key = torch.empty(N, dtype=torch.int32, device=DEV)
    seed_dev = torch.tensor([seed], dtype=torch.int32, device=DEV)
    rid = None if row_ids is None else torch.as_tensor(row_ids, dtype=torch.int32).to(DEV)
    cnt = torch.tensor([step - 1], dtype=torch.int32, device=DEV) if step_dev else None
    call('tell_adaptive_logprob_nucleus', *X.args(), N, k, inv_temp, p, seed_dev, rid, 0 if step_dev else step, cnt, tok, lp,
         size, key)
    return tok.cpu().numpy(), lp.cpu().numpy(), size.cpu().numpy(), _key_lp(key.cpu().numpy().view(np.uint32))


def _definition(full, inv_temp, p, k, seed, rows, step):
    from tell_amd import rng
    from tell_amd.models.transformer import nucleus_definition
    T = 1.0 / float(np.float32(inv_temp))
    out = []
    for r in range(full.shape[0]):
        u = float(rng.sample_uniform(seed, rows[r], step))
        d = nucleus_definition(full[r], T, float(np.float32(p)), k, u)
        d['near'] = float(np.min(np.abs(u - np.r_[0.0, d['cdf']])))
        out.append(d)
    return out


@pytest.mark.parametrize('N', [32, 128])
def test_nucleus_membership_and_pick_are_exact(N):
    """Nucleus size and threshold equal the fp64 definition's on every row whose boundary margin is at least BOUND, and
    the token equals the definition's on every such row whose u is at least BOUND from a CDF edge; at most 5 % of the rows
    are skipped by either rule.  p in {0.3, 0.9, 0.95}, T in {0.7, 1, 1.3}; register form, streaming form by option and
    by alignment; host step, device step, original-row ids.  The reported log-prob is the untempered lp of the token."""
    import tell_amd
    rows_seen = skipped_m = kept = skipped_u = 0
    for form in FORMS:
        X = _peaked(N, seed=3 * N + len(form), shift=1 if form == 'unaligned' else 0)
        full, _, _ = X.full()
        # the register form reduces lse in another order than the full-row kernel: lp = logit - lse may differ by 2 ulp of
        # the largest |logit| (lse is of that size); the streaming forms have the full-row kernel's arithmetic
        tol = 2.0 ** -22 * float(X.head.abs().max()) if form == 'regs' else 0.0
        with tell_amd.hip.options(argmax_regs=0 if form == 'option' else 1):
            for pi, p in enumerate(P_VALUES):
                for ti, T in enumerate((0.7, 1.0, 1.3)):
                    inv_temp = float(np.float32(1.0 / T))
                    seed, step = 7000 + 100 * pi + ti, 2 + 13 * ti + pi
                    rid = (np.arange(N) * 37 + (1 << 20)) if ti == 1 else None
                    tok, lp, size, thr = _nucleus(X, 0, inv_temp, p, seed, step, row_ids=rid, step_dev=ti == 2)
                    want = _definition(full, inv_temp, p, 0, seed, rid if rid is not None else np.arange(N), step)
                    for r, d in enumerate(want):
                        rows_seen += 1
                        print('form %s N %d p %.2f T %.1f row %d: size %d / %d margin %.3e near %.3e token %d / %d'
                              % (form, N, p, T, r, size[r], len(d['members']), d['margin'], d['near'], tok[r], d['token']))
                        if d['margin'] < BOUND:
                            skipped_m += 1
                            continue
                        assert size[r] == len(d['members']), (form, p, T, r, size[r], len(d['members']))
                        assert abs(float(thr[r]) - d['boundary']) <= tol, (form, p, T, r, thr[r], d['boundary'])
                        kept += 1
                        if d['near'] < BOUND:
                            skipped_u += 1
                            continue
                        assert tok[r] == d['token'], (form, p, T, r, tok[r], d['token'])
                        assert abs(float(lp[r]) - float(full[r, tok[r]])) <= tol, (form, p, T, r, lp[r], full[r, tok[r]])
    print('rows %d, skipped at the boundary %d, kept %d, skipped at a CDF edge %d' % (rows_seen, skipped_m, kept, skipped_u))
    assert skipped_m <= 0.05 * rows_seen, (skipped_m, rows_seen)
    assert skipped_u <= 0.05 * kept, (skipped_u, kept)


@pytest.mark.parametrize('form', FORMS)
def test_nucleus_size_on_flat_rows(form):
    """Rows as flat as the top-k tests' (nuclei of hundreds to tens of thousands of tokens): no row is skipped - the size
    must lie between the definition's sizes for p * total -/+ BOUND * total, and every token must be a member of the
    larger of the two with its own untempered log-prob."""
    import tell_amd
    X = _Rows(32, C0, TAILS, seed=91, shift=1 if form == 'unaligned' else 0, ties=True)
    full, _, _ = X.full()
    ids = np.arange(V)
    with tell_amd.hip.options(argmax_regs=0 if form == 'option' else 1):
        for p, T in ((0.3, 0.6), (0.9, 0.8), (0.95, 1.0)):
            inv_temp = float(np.float32(1.0 / T))
            tok, lp, size, thr = _nucleus(X, 0, inv_temp, p, 99, 4)
            for r in range(X.N):
                row = full[r].astype(np.float64)
                order = np.lexsort((ids, -row))
                cum = np.cumsum(np.exp((row[order] - row[order[0]]) * float(np.float32(inv_temp))))
                lo = int(np.searchsorted(cum, (p - BOUND) * cum[-1], side='left')) + 1
                hi = min(int(np.searchsorted(cum, (p + BOUND) * cum[-1], side='left')) + 1, V)
                print('form %s p %.2f T %.1f row %d: size %d in [%d, %d]' % (form, p, T, r, size[r], lo, hi))
                assert lo <= size[r] <= hi, (form, p, T, r, size[r], lo, hi)
                assert tok[r] in order[:hi]
                assert abs(float(lp[r]) - float(full[r, tok[r]])) <= 2e-6 * max(1.0, abs(float(lp[r])))
                assert abs(float(thr[r]) - row[order[size[r] - 1]]) <= 2e-6 * abs(row[order[size[r] - 1]])


def test_nucleus_ends():
    """A tiny p is tell_adaptive_logprob_argmax bit for bit; k = 8, p = 1 only returns members of tell_adaptive_logprob_topk's
    set; k > 0 with a p follows the definition on the k candidates."""
    import tell_amd
    for form in FORMS:
        X = _Rows(128, C0, TAILS, seed=17, shift=1 if form == 'unaligned' else 0, ties=True)
        full, _, _ = X.full()
        with tell_amd.hip.options(argmax_regs=0 if form == 'option' else 1):
            am_tok, am_lp = X.argmax()
            for p in (1e-7, 1e-4):
                tok, lp, size, _ = _nucleus(X, 0, 1.25, p, 5, 9)
                assert np.array_equal(tok, am_tok) and np.array_equal(lp, am_lp), form
                assert (size == 1).all()
            top8 = X.topk(8)
            seen = set()
            for step in range(1, 9):
                tok, lp, size, _ = _nucleus(X, 8, 0.5, 1.0, 11, step)
                assert all(tok[r] in top8[r] for r in range(X.N)), form
                assert (size == 8).all()
                seen.update(int(np.nonzero(top8[r] == tok[r])[0][0]) for r in range(X.N))
            assert len(seen) >= 6                               # (T = 2 over 1024 draws: not only the best candidate)
            inv_temp = float(np.float32(1 / 1.5))
            tok, lp, size, thr = _nucleus(X, 20, inv_temp, 0.6, 23, 3)
            want = _definition(full, inv_temp, 0.6, 20, 23, np.arange(X.N), 3)
            ok = np.array([d['margin'] >= BOUND for d in want])
            assert ok.mean() > 0.5
            for r, d in enumerate(want):
                if ok[r]:
                    assert size[r] == len(d['members']), (form, r)
                    if d['near'] >= BOUND:
                        assert tok[r] == d['token'], (form, r)


def test_nucleus_frequencies():
    """One fixed distribution, 8192 rows x 3 steps = 24 576 draws at p = 0.9, T = 0.7: chi-square of the token counts against
    the fp64 nucleus probabilities below the p ~ 1e-4 quantile (seeded: it passes or it does not); every draw is a member and
    reports the member's untempered log-prob."""
    from tell_amd.models.transformer import nucleus_definition
    X = _Rows(8192, C0, TAILS, seed=5, replicate=True)
    full, _, _ = _Rows(1, C0, TAILS, seed=5, replicate=True).full()
    inv_temp = float(np.float32(1 / 0.7))
    d = nucleus_definition(full[0], 1.0 / inv_temp, float(np.float32(0.9)), 0)
    toks = []
    for step in (1, 2, 3):
        tok, lp, size, _ = _nucleus(X, 0, inv_temp, 0.9, 31337, step)
        assert (size == size[0]).all()
        np.testing.assert_allclose(lp, full[0, tok], rtol=1e-6, atol=2e-6)
        toks.append(tok)
    n = int(size[0])
    if d['margin'] >= BOUND:                                    # (else the boundary may sit one token off: the skip rule)
        assert n == len(d['members'])
    assert abs(n - len(d['members'])) <= 1
    row = full[0].astype(np.float64)
    members = np.sort(np.lexsort((np.arange(V), -row))[:n])     # the fp64 probabilities of the n best tokens, in id order
    prob = np.exp((row[members] - row.max()) * inv_temp)
    prob /= prob.sum()
    tok = np.concatenate(toks)
    assert len(tok) >= 20000 and np.isin(tok, members).all()
    cnt = np.bincount(np.searchsorted(members, tok), minlength=len(members)).astype(np.float64)
    exp = prob * len(tok)
    big = exp >= 5                                              # (bins with fewer than 5 expected draws pooled)
    o = np.r_[cnt[big], cnt[~big].sum()]
    e = np.r_[exp[big], exp[~big].sum()]
    chi2 = ((o - e) ** 2 / np.maximum(e, 1e-12)).sum()
    dof = len(o) - 1
    print('nucleus of %d tokens, %d bins, chi2 %.1f' % (len(members), len(o), chi2))
    assert dof >= 20
    assert chi2 < dof + 3.72 * np.sqrt(2 * dof) + 8, (chi2, dof)   # ~ the p = 1e-4 quantile of chi2(dof)


def test_nucleus_kernel_determinism():
    """Host step against the device counter of a captured step, inside a hipGraph against eager, and 32 rows against the
    same rows inside 128: the same tokens, log-probs, sizes and thresholds."""
    import tell_amd
    from tell_amd.hip import call
    X = _Rows(128, C0, TAILS, seed=29)
    for form in ('regs', 'option'):
        with tell_amd.hip.options(argmax_regs=0 if form == 'option' else 1):
            a = _nucleus(X, 0, 1.0, 0.9, 77, 12)
            b = _nucleus(X, 0, 1.0, 0.9, 77, 12, step_dev=True)
            c = _nucleus(X, 0, 1.0, 0.9, 77, 12, N=32)
            for x, y, z in zip(a, b, c):
                assert np.array_equal(x, y) and np.array_equal(x[:32], z), form
            tok = torch.empty(128, dtype=torch.int32, device=DEV)
            lp = torch.empty(128, dtype=torch.float32, device=DEV)
            seed = torch.tensor([77], dtype=torch.int32, device=DEV)
            cnt = torch.tensor([11], dtype=torch.int32, device=DEV)
            args = X.args()
            run = lambda: call('tell_adaptive_logprob_nucleus', *args, 128, 0, 1.0, 0.9, seed, None, 0, cnt, tok, lp,  # noqa: E731
                               None, None)
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
            assert np.array_equal(tok.cpu().numpy(), _nucleus(X, 0, 1.0, 0.9, 77, 13)[0])
            assert not np.array_equal(tok.cpu().numpy(), a[0])


def test_nucleus_candidates_kernel():
    """tell_nucleus_candidates against the definition on given sorted candidates (rows away from the rounding cases)."""
    from tell_amd import rng
    from tell_amd.hip import call
    from tell_amd.models.transformer import nucleus_definition
    g = torch.Generator().manual_seed(3)
    R, k = 300, 20
    lps = torch.sort(torch.randn(R, k, generator=g) * 2, dim=1, descending=True).values
    toks = torch.stack([torch.randperm(50000, generator=g)[:k] for _ in range(R)]).to(torch.int32)
    out_t = torch.empty(R, dtype=torch.int32, device=DEV)
    out_l = torch.empty(R, dtype=torch.float32, device=DEV)
    seed = torch.tensor([77], dtype=torch.int32, device=DEV)
    inv_temp = float(np.float32(1 / 0.7))
    call('tell_nucleus_candidates', toks.to(DEV), lps.to(DEV), R, k, inv_temp, 0.8, seed, None, 11, None, out_t, out_l)
    checked = 0
    for r in range(R):
        row = np.full(50000, -1e9)
        row[toks[r].numpy()] = lps[r].numpy()
        u = float(rng.sample_uniform(77, r, 11))
        d = nucleus_definition(row, 1.0 / inv_temp, float(np.float32(0.8)), k, u)
        if d['margin'] < 1e-4 or np.min(np.abs(u - np.r_[0.0, d['cdf']])) < 1e-4:       # k * 2^-24 = 1.2e-6 and a safety factor
            continue
        checked += 1
        assert int(out_t[r]) == d['token']
        assert float(out_l[r]) == float(lps[r][toks[r].tolist().index(d['token'])])
    assert checked > 0.95 * R


# ---------------------------------------------------------------------------------------------------- the models
def _golden_nucleus_model(golden, kind, **sampling):
    import tell_amd
    from tell_amd.build import build_model
    from test_gpu_decoder import DEC_KW, _PoolResnet, _TableRoberta
    tell_amd.set_compute_dtype(torch.float32)
    fx = golden('model_' + kind)
    art_dim = 64 if kind == 'flattened' else 1024
    model = build_model(kind, _PoolResnet(), _TableRoberta(art_dim), article_dim=art_dim, **sampling, **DEC_KW).eval()
    own = model.state_dict()
    model.load_state_dict({k: v for k, v in fx['sd'].items() if k in own}, strict=False)
    model.to(DEV)
    ins = fx['in']

    def batch():
        b = dict(context={'roberta': ins['article_ids'].to(DEV)}, image=ins['image'].to(DEV),
                 caption={'roberta': ins['caption_ids'].to(DEV)})
        if kind == 'faces_objects':
            f, o = ins['face_embeds'].clone(), ins['obj_embeds'].clone()
            for i in range(f.shape[0]):
                f[i, int(ins['n_faces'][i]):] = float('nan')
                o[i, int(ins['n_objs'][i]):] = float('nan')
            b.update(face_embeds=f.to(DEV), obj_embeds=o.to(DEV))
        return b
    return model, batch


def test_golden_faces_objects_nucleus_flows(golden):
    """transformer_faces_objects with sampling_topk = 0, sampling_topp = 0.9 (fp32 golden weights): captions finish; the cached
    flow (eager first step + captured replays), the same flow with graphs off and the reference's control flow give the same
    ids under one seed, captured == eager bit for bit; another seed gives other captions; the capture is keyed as a nucleus
    step; teacher-forcing the model on the sampled prefix, every token is inside the fp64 nucleus (+ BOUND) of its step."""
    import tell_amd
    from tell_amd.models.transformer import nucleus_definition
    T, P = 0.9, 0.9
    model, batch = _golden_nucleus_model(golden, 'faces_objects', sampling_topk=0, sampling_topp=P, sampling_temp=T)
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
    assert all(('nucleus', 0, T, P) in sig for sig, _ in sigs)
    ids = outs[0]['gen_ids'].cpu()
    for o in outs[1:]:
        assert torch.equal(o['gen_ids'].cpu(), ids)
    assert torch.equal(outs[1]['log_probs'], outs[2]['log_probs'])
    assert ids.shape[1] > 2
    alive = _alive(ids)
    torch.manual_seed(124)
    model.fast_generation = True
    assert not torch.equal(model.generate(**batch())['gen_ids'].cpu(), ids)
    with torch.no_grad():
        b = batch()
        _, _, ctx = model._forward(b['context'], b['image'], b['caption'], b.get('face_embeds'), b.get('obj_embeds'))
        out = model.decoder({'roberta': ids[:, :-1].to(DEV)}, ctx)
        lp = model.decoder.get_normalized_probs((out[0], None), log_probs=True).float().cpu()
    got = outs[0]['log_probs'].cpu()
    for bi in range(ids.shape[0]):
        for t in range(ids.shape[1] - 1):
            if alive[bi, t]:
                d = nucleus_definition(lp[bi, t].numpy(), T, min(1.0, P + 1e-3))
                assert int(ids[bi, t + 1]) in d['members'], (bi, t)
                assert abs(float(got[bi, t]) - float(lp[bi, t, ids[bi, t + 1]]) / T) <= 2e-4
    with pytest.raises(ValueError):
        model.generate(**batch(), beam_size=2)


def test_pointer_model_nucleus_generation():
    """transformer_pointer with sampling_topk = 0, sampling_topp = 0.9: generates, finishes, repeats under one seed and differs
    across seeds."""
    import tell_amd
    from tell_amd.build import build_model
    from test_gpu_pointer import _Resnet, _Roberta, _pointer_batch
    tell_amd.set_compute_dtype(torch.float32)
    try:
        torch.manual_seed(0)
        model = build_model('pointer', _Resnet(), _Roberta(), n_bert_layers=3, vocab_size=600, dim=1024, heads=16, ffn=256,
                            kernels=(3,), cutoff=(100, 300), sampling_topk=0, sampling_topp=0.9).cuda().eval()
        batch = _pointer_batch(B=4)
        gen = lambda: model.generate(batch['context'], batch['image'], batch['caption'], batch['face_embeds'])   # noqa: E731
        torch.manual_seed(7)
        a = gen()
        torch.manual_seed(7)
        b = gen()
        assert torch.equal(a['gen_ids'], b['gen_ids']) and torch.equal(a['log_probs'], b['log_probs'])
        assert a['gen_ids'].shape == a['should_copy'].shape and a['gen_ids'].shape[1] >= 2
        assert len(a['generations']) == 4
        torch.manual_seed(8)
        c = gen()
        assert c['gen_ids'].shape != a['gen_ids'].shape or not torch.equal(c['gen_ids'], a['gen_ids'])
    finally:
        tell_amd.set_compute_dtype(torch.float32)


@pytest.fixture(scope='module')
def fullsize_nucleus():
    import tell_amd
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects', sampling_topk=0, sampling_topp=0.9).to(DEV).eval()
    batches = [synthetic_batch(4, 64, 9, True, seed=81 + i, device=DEV) for i in range(3)]
    yield model, batches
    tell_amd.set_compute_dtype(torch.float32)


def test_fullsize_nucleus_lanes_and_captured_steps(fullsize_nucleus):
    """Full-size faces_objects in bf16 with sampling_topk = 0, sampling_topp = 0.9: the single-step and multi-step graphs are
    recorded under the nucleus key; one seed gives one result, another seed another; generate_lanes equals `generate` batch
    by batch under one torch seed."""
    model, batches = fullsize_nucleus

    def gen(seed, b):
        torch.manual_seed(seed)
        out = model.generate(**_clone(b))
        torch.cuda.synchronize()
        return out['gen_ids'].cpu(), out['log_probs'].cpu()
    a, a2 = gen(11, batches[0]), gen(11, batches[0])
    assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])
    assert not torch.equal(gen(12, batches[0])[0], a[0])
    hs = [(sig, h) for sig, h in model.__dict__['_decode_graphs'].items() if ('nucleus', 0, 1.0, 0.9) in sig]
    assert hs and all(h['graph'] not in (None, False) for _, h in hs), [h.get('error') for _, h in hs]
    torch.manual_seed(21)
    alone = [model.generate(**_clone(b)) for b in batches]
    torch.cuda.synchronize()
    torch.manual_seed(21)
    seen = 0
    for i, (_, out) in enumerate(model.generate_lanes((_clone(b) for b in batches), lanes=2)):
        torch.cuda.synchronize()
        assert torch.equal(out['gen_ids'], alone[i]['gen_ids']), i
        assert torch.equal(out['log_probs'], alone[i]['log_probs']), i
        seen += 1
    assert seen == len(batches)


@pytest.mark.parametrize('topk', [0, 5])
def test_lstm_baseline_nucleus(golden, topk):
    """BaselineGloveModel with sampling_topp = 0.9 (k = 0: the nucleus kernel over the full log-prob row; k = 5: the nucleus of
    the five best, tell_nucleus_candidates): one seed gives one result, and every sampled token is a member of the fp64
    nucleus (+ BOUND) of its teacher-forced log-probs."""
    import tell_amd
    from tell_amd.build import build_embedder
    from tell_amd.models import BaselineGloveModel, LSTMDecoder
    from tell_amd.models.transformer import nucleus_definition
    from tell_amd.modules import AdaptiveLoss
    from test_gpu_decoder import _PoolResnet
    tell_amd.set_compute_dtype(torch.float32)
    fx = golden('model_baseline_glove')
    dec = LSTMDecoder(None, build_embedder(600, 64, (100, 300), 512), num_layers=2, hidden_size=48, dropout=0.1,
                      share_decoder_input_output_embed=True, vocab_size=600, adaptive_softmax_cutoff=[100, 300],
                      tie_adaptive_weights=True, adaptive_softmax_dropout=0, tie_adaptive_proj=False,
                      adaptive_softmax_factor=1, article_embed_size=300, image_embed_size=2048)
    model = BaselineGloveModel(None, dec, AdaptiveLoss(1), resnet=_PoolResnet(), sampling_topk=topk, sampling_topp=0.9,
                               sampling_temp=0.7).eval()
    own = model.state_dict()
    model.load_state_dict({k: v for k, v in fx['sd'].items() if k in own}, strict=False)
    model.to(DEV)
    ins = fx['in']
    batch = lambda: dict(image=ins['image'].to(DEV), caption={'roberta': ins['caption'].to(DEV)},   # noqa: E731
                         context_vectors=ins['context_vectors'].to(DEV))
    torch.manual_seed(5)
    a = model.generate(**batch())
    torch.manual_seed(5)
    b = model.generate(**batch())
    ids = a['gen_ids']
    assert torch.equal(ids, b['gen_ids']) and torch.equal(a['log_probs'], b['log_probs'])
    with torch.no_grad():
        bb = batch()
        _, _, contexts = model._forward(model._vectors(bb['context_vectors'], None), bb['image'], bb['caption'])
        state, lps = {}, []
        for t in range(ids.shape[1] - 1):
            out = model.decoder({'roberta': ids[:, t:t + 1]}, contexts, incremental_state=state)
            lps.append(model.decoder.get_normalized_probs((out[0][:, -1:], None), log_probs=True).squeeze(1).float())
        lp = torch.stack(lps, 1).cpu()
    alive = _alive(ids.cpu())
    got = a['log_probs'].cpu()
    for bi in range(ids.shape[0]):
        for t in range(ids.shape[1] - 1):
            if alive[bi, t]:
                d = nucleus_definition(lp[bi, t].numpy(), 0.7, min(1.0, 0.9 + BOUND), topk)
                assert int(ids[bi, t + 1]) in d['members'], (bi, t)
                assert abs(float(got[bi, t]) - float(lp[bi, t, ids[bi, t + 1]]) / 0.7) <= 1e-4
