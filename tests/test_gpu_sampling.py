"""GPU: top-k sampling with a temperature (include/tell_hip.h tell_adaptive_logprob_sample / tell_sample_candidates) through
the C ABI - exact against a numpy restatement of the semantics - and through the caption models' decode loops."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    yield
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the kernel, exactly
LAYOUTS = {
    'build_model': (5000, (15000, 30265)),                    # the full-size adaptive softmax (cutoffs 5000, 20000)
    'three_tails': (4000, (12000, 24000, 8000)),
}


class _Rows:
    """Random logits of N rows in the adaptive layout: fp32 head [N, c0 + n_tails] and tails, rows on 16 bytes (or not:
    shift=1 starts every buffer one float later, which the register kernel does not take)."""

    def __init__(self, N, c0, tails, seed, shift=0, ties=False, replicate=False):
        g = torch.Generator().manual_seed(seed)
        nt = len(tails)
        self.c0, self.tails, self.N, self.nt = c0, tails, N, nt

        def buf(n, scale):
            ld = -(-(n + shift) // 4) * 4
            t = (torch.randn(1 if replicate else N, ld, generator=g) * scale).expand(N, ld).contiguous()
            return t.to(DEV), ld
        self.head, self.ld_head = buf(c0 + nt, 3.0)
        self.tl = [buf(n, 2.0) for n in tails]
        if ties:                                              # row 0: eight exactly equal head logits at the top
            self.head[0, shift + 17:shift + 17 + 8 * 97:97] = self.head[0, shift:shift + c0].max() + 1.0
        self.shift = shift

    def args(self):
        s = self.shift
        h = self.head[:, s:]
        tl = [(t[:, s:], ld, n) for (t, ld), n in zip(self.tl, self.tails)] + [(None, 0, 0)] * (3 - self.nt)
        out = [h, self.ld_head, self.c0, self.nt]
        for t, ld, n in tl:
            out += [t, ld, n]
        return out

    def full(self):
        """-> (log-prob rows [N, vocab] of tell_adaptive_logprob_argmax, arg-max token, lp) - the streaming arg-max kernel."""
        from tell_amd.hip import call
        V = self.c0 + sum(self.tails)
        lp = torch.empty(self.N, V, dtype=torch.float32, device=DEV)
        tok = torch.empty(self.N, dtype=torch.int32, device=DEV)
        tlp = torch.empty(self.N, dtype=torch.float32, device=DEV)
        call('tell_adaptive_logprob_argmax', *self.args(), self.N, lp, V, tok, tlp)
        return lp.cpu().numpy(), tok.cpu().numpy(), tlp.cpu().numpy()

    def argmax(self):
        from tell_amd.hip import call
        tok = torch.empty(self.N, dtype=torch.int32, device=DEV)
        tlp = torch.empty(self.N, dtype=torch.float32, device=DEV)
        call('tell_adaptive_logprob_argmax', *self.args(), self.N, None, 0, tok, tlp)
        return tok.cpu().numpy(), tlp.cpu().numpy()

    def topk(self, k):
        from tell_amd.hip import call
        tok = torch.empty(self.N, k, dtype=torch.int32, device=DEV)
        lps = torch.empty(self.N, k, dtype=torch.float32, device=DEV)
        call('tell_adaptive_logprob_topk', *self.args(), self.N, k, tok, lps)
        return tok.cpu().numpy()

    def sample(self, k, inv_temp, seed, step, row_ids=None, step_dev=False):
        from tell_amd.hip import call
        tok = torch.empty(self.N, dtype=torch.int32, device=DEV)
        lp = torch.empty(self.N, dtype=torch.float32, device=DEV)
        seed_dev = torch.tensor([seed], dtype=torch.int32, device=DEV)
        rid = None if row_ids is None else torch.as_tensor(row_ids, dtype=torch.int32).to(DEV)
        cnt = torch.tensor([step - 1], dtype=torch.int32, device=DEV) if step_dev else None
        call('tell_adaptive_logprob_sample', *self.args(), self.N, k, inv_temp, seed_dev, rid, 0 if step_dev else step, cnt,
             tok, lp)
        return tok.cpu().numpy(), lp.cpu().numpy()


def _order(full):
    """Per row the 64 best token ids: value descending, lower id first on ties."""
    ids = np.arange(full.shape[1])
    return np.stack([np.lexsort((ids, -r))[:64] for r in full])


def _expect(full, order, k, inv_temp, seed, rows, step):
    from tell_amd import rng
    tok, lp, near = [], [], []
    for r in range(full.shape[0]):
        cand = full[r, order[r, :k]]
        u = rng.sample_uniform(seed, rows[r], step)
        j = rng.sample_pick(cand, inv_temp, u)
        tok.append(order[r, j])
        lp.append(cand[j])
        w = np.exp((cand - cand[0]) * np.float32(inv_temp)).astype(np.float32)
        c = np.add.accumulate(w, dtype=np.float32).astype(np.float64)
        t = float(np.float32(u) * np.float32(c[-1]))
        near.append(np.min(np.abs(t - c)) <= 1e-5 * c[-1])
    return np.array(tok), np.array(lp, dtype=np.float32), np.array(near)


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_sample_kernel_is_exact(layout):
    """tokens and log-probs equal the semantics restated in numpy over the full log-prob row of the arg-max kernel, for
    N in {1, 7, 32, 224}, k in {1, 2, 8, 50, 64}, T in {0.5, 1, 1.7}; the register form and the streaming form (option
    argmax_regs = 0, and unaligned rows); a row with exact ties; host and device step; original-row ids.  Only rows whose
    u * c_{k-1} lies within 1e-5 (relative) of a CDF edge may disagree, at most one per 1000 rows."""
    import tell_amd
    c0, tails = LAYOUTS[layout]
    rows_seen, disagree = 0, []
    for form in ('regs', 'option', 'unaligned'):
        for N in (1, 7, 32, 224):
            X = _Rows(N, c0, tails, seed=N + 7 * len(tails), shift=1 if form == 'unaligned' else 0, ties=True)
            full, _, _ = X.full()
            order = _order(full)
            with tell_amd.hip.options(argmax_regs=0 if form == 'option' else 1):
                am_tok, am_lp = X.argmax()
                for k in (1, 2, 8, 50, 64):
                    if k <= 8:                               # the candidate set is tell_adaptive_logprob_topk's
                        assert np.array_equal(X.topk(k), order[:, :k]), (form, N, k)
                    for ti, T in enumerate((0.5, 1.0, 1.7)):
                        inv_temp = float(np.float32(1.0 / T))
                        seed, step = 1000 * k + 17 * N + ti, 3 + ti * 40
                        rid = (np.arange(N) * 37 + (1 << 20)) if ti == 1 else None
                        got_tok, got_lp = X.sample(k, inv_temp, seed, step, row_ids=rid, step_dev=ti == 2)
                        want_tok, want_lp, near = _expect(full, order, k, inv_temp, seed,
                                                          rid if rid is not None else np.arange(N), step)
                        if k == 1:                          # the arg-max kernel's result, bit for bit
                            assert np.array_equal(got_tok, am_tok) and np.array_equal(got_lp, am_lp), (form, N)
                        rows_seen += N
                        bad = np.nonzero(got_tok != want_tok)[0]
                        for r in bad:
                            assert near[r], (form, N, k, T, r, got_tok[r], want_tok[r])
                            disagree.append((form, N, k, T, int(r)))
                        ok = got_tok == want_tok
                        if form == 'regs':                  # (lse reduced in another order than the full-row kernel's)
                            np.testing.assert_allclose(got_lp[ok], want_lp[ok], rtol=1e-6, atol=2e-6)
                        else:                               # the streaming form has the full-row kernel's arithmetic
                            assert np.array_equal(got_lp[ok], want_lp[ok]), (form, N, k, T)
    assert len(disagree) <= max(1, rows_seen // 1000), disagree


def test_sample_kernel_distribution():
    """One logit row replicated over 8192 rows, k = 50, T = 0.8: the counts of the drawn tokens against
    softmax(topk(lp) / T) - chi2 at p ~ 1e-4."""
    c0, tails = LAYOUTS['build_model']
    X = _Rows(8192, c0, tails, seed=5, replicate=True)
    full, _, _ = _Rows(1, c0, tails, seed=5, replicate=True).full()        # (the same row)
    order = _order(full)[0, :50]
    tok, lp = X.sample(50, float(np.float32(1 / 0.8)), seed=424242, step=9)
    assert np.isin(tok, order).all()
    p = np.exp((full[0, order].astype(np.float64) - full[0, order[0]]) / 0.8)
    p /= p.sum()
    cnt = np.array([(tok == t).sum() for t in order], dtype=np.float64)
    exp = p * len(tok)
    big = exp >= 5                                             # (bins with fewer than 5 expected draws pooled)
    o = np.r_[cnt[big], cnt[~big].sum()]
    e = np.r_[exp[big], exp[~big].sum()]
    chi2 = ((o - e) ** 2 / np.maximum(e, 1e-12)).sum()
    dof = len(o) - 1
    assert chi2 < dof + 3.72 * np.sqrt(2 * dof) + 8, (chi2, dof)  # ~ the p = 1e-4 quantile for 10..50 dof
    np.testing.assert_allclose(lp, full[0, tok], rtol=1e-6, atol=2e-6)


def test_sample_candidates_kernel():
    """tell_sample_candidates: steps 2-5 of the semantics on given sorted candidates."""
    from tell_amd import rng
    from tell_amd.hip import call
    g = torch.Generator().manual_seed(3)
    R, k = 300, 20
    lps = torch.sort(torch.randn(R, k, generator=g) * 2, dim=1, descending=True).values
    toks = torch.randint(0, 50000, (R, k), generator=g, dtype=torch.int32)
    out_t = torch.empty(R, dtype=torch.int32, device=DEV)
    out_l = torch.empty(R, dtype=torch.float32, device=DEV)
    seed = torch.tensor([77], dtype=torch.int32, device=DEV)
    cnt = torch.tensor([10], dtype=torch.int32, device=DEV)
    for step_dev in (None, cnt):
        call('tell_sample_candidates', toks.to(DEV), lps.to(DEV), R, k, float(np.float32(1 / 0.7)), seed, None, 11, step_dev,
             out_t, out_l)
        for r in range(R):
            j = rng.sample_pick(lps[r].numpy(), np.float32(1 / 0.7), rng.sample_uniform(77, r, 11))
            assert int(out_t[r]) == int(toks[r, j]) and float(out_l[r]) == float(lps[r, j])


# ---------------------------------------------------------------------------------------------------- the models
def _golden_model(golden, kind, topk, temp):
    import tell_amd
    from tell_amd.build import build_model
    from test_gpu_decoder import DEC_KW, _PoolResnet, _TableRoberta
    tell_amd.set_compute_dtype(torch.float32)
    fx = golden('model_' + kind)
    art_dim = 64 if kind == 'flattened' else 1024
    model = build_model(kind, _PoolResnet(), _TableRoberta(art_dim), article_dim=art_dim, sampling_topk=topk,
                        sampling_temp=temp, **DEC_KW).eval()
    own = model.state_dict()
    model.load_state_dict({k: v for k, v in fx['sd'].items() if k in own}, strict=False)
    model.to(DEV)
    ins = fx['in']

    def batch(dev=DEV):
        b = dict(context={'roberta': ins['article_ids'].to(dev)}, image=ins['image'].to(dev),
                 caption={'roberta': ins['caption_ids'].to(dev)})
        if kind == 'faces_objects':
            f, o = ins['face_embeds'].clone(), ins['obj_embeds'].clone()
            for i in range(f.shape[0]):
                f[i, int(ins['n_faces'][i]):] = float('nan')
                o[i, int(ins['n_objs'][i]):] = float('nan')
            b.update(face_embeds=f.to(dev), obj_embeds=o.to(dev))
        return b
    return model, fx, batch


def _alive(ids, eos=2):
    """[B, steps] mask of the positions a row still decodes (up to and including its </s>)."""
    gen = ids[:, 1:]
    done_before = torch.cumsum((gen == eos).long(), dim=1) - (gen == eos).long()
    return done_before == 0


@pytest.mark.parametrize('kind', ['flattened', 'faces_objects'])
def test_golden_model_sampling_fp32(golden, kind):
    """sampling_topk = 5, T = 0.8 on the fp32 golden models: the cached flow (eager first step + capture, then all replays),
    the same flow with graphs off and the reference's control flow give the same ids under one seed; teacher-forcing the fp32 CPU oracle on the sampled
    prefix puts every sampled token inside its top 5 (near-ties allowed) and every reported log-prob is the oracle's lp / T."""
    from oracle.build import build_model as obuild
    from test_gpu_decoder import DEC_KW
    from test_oracle_golden import _PoolResnet as OResnet, _TableRoberta as ORoberta
    T = 0.8
    model, fx, batch = _golden_model(golden, kind, 5, T)
    import tell_amd
    outs = []
    keep = tell_amd.graphs.ENABLED
    try:
        for fast, graphed in ((True, True), (True, True), (True, False), (False, True)):
            model.fast_generation, tell_amd.graphs.ENABLED = fast, graphed
            torch.manual_seed(123)
            outs.append(model.generate(**batch()))
    finally:
        tell_amd.graphs.ENABLED = keep
    hs = list(model.__dict__.get('_decode_graphs', {}).values())
    assert hs and all(h['graph'] not in (None, False) for h in hs), [h.get('error') for h in hs]
    ids = outs[0]['gen_ids'].cpu()
    for o in outs[1:]:
        assert torch.equal(o['gen_ids'].cpu(), ids)
    assert torch.equal(outs[1]['log_probs'], outs[2]['log_probs'])      # captured == eager, bit for bit
    assert ids.shape[1] > 2
    torch.manual_seed(124)
    model.fast_generation = True
    other = model.generate(**batch())['gen_ids'].cpu()
    assert not torch.equal(other, ids)                          # a different seed, other captions
    # the fp32 CPU oracle, teacher-forced on the sampled prefix
    art_dim = 64 if kind == 'flattened' else 1024
    cpu = obuild(kind, OResnet(), ORoberta(art_dim), article_dim=art_dim, **DEC_KW).eval()
    own = cpu.state_dict()
    cpu.load_state_dict({k: v for k, v in fx['sd'].items() if k in own}, strict=False)
    with torch.no_grad():
        b = batch('cpu')
        _, _, ctx = cpu._forward(b['context'], b['image'], b['caption'], b.get('face_embeds'), b.get('obj_embeds'))
        out = cpu.decoder({'roberta': ids[:, :-1]}, ctx)
        lp = cpu.decoder.get_normalized_probs((out[0], None), log_probs=True).float()       # [B, steps, V]
    alive = _alive(ids)
    tok = ids[:, 1:]
    fifth = lp.topk(5, dim=-1).values[..., -1]
    lp_tok = lp.gather(2, tok.unsqueeze(-1)).squeeze(-1)
    assert (lp_tok >= fifth - 1e-4)[alive].all()
    for o in outs:
        got = o['log_probs'].cpu()
        assert torch.allclose(got[alive], (lp_tok / T)[alive], atol=2e-4, rtol=0), (got - lp_tok / T)[alive].abs().max()


@pytest.fixture(scope='module')
def fullsize():
    import tell_amd
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects', sampling_topk=20, sampling_temp=0.9).to(DEV).eval()
    batches = [synthetic_batch(4, 64, 9, True, seed=81 + i, device=DEV) for i in range(3)]
    yield model, batches
    tell_amd.set_compute_dtype(torch.float32)


def _clone(b):
    return {k: (dict(v) if isinstance(v, dict) else v.clone()) for k, v in b.items()}


def test_fullsize_captured_sampling_step(fullsize):
    """Full-size faces_objects model in bf16 with sampling_topk = 20: same seed -> same ids and lps; another seed -> other
    ids; the single-step and the multi-step graphs are recorded (and keyed on the sampling mode); multi-step replays and one
    step per replay agree bit for bit.  (Graphs off, this model decodes layer by layer - other bf16 rounding points, so
    the eager comparison is test_golden_model_sampling_fp32's.)"""
    import tell_amd
    from tell_amd.models import stepper as tr
    model, batches = fullsize
    b = batches[0]

    def gen(seed):
        torch.manual_seed(seed)
        out = model.generate(**_clone(b))
        torch.cuda.synchronize()
        return out['gen_ids'].cpu(), out['log_probs'].cpu()
    keep_multi = tr.MULTI_STEP_GRAPHS
    try:
        tr.MULTI_STEP_GRAPHS = True
        a = gen(11)
        a2 = gen(11)
        assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])
        assert a[0].shape[1] > 16                               # (random weights: long captions, multi-step replays)
        assert not torch.equal(gen(12)[0], a[0])
        hs = [(sig, h) for sig, h in model.__dict__['_decode_graphs'].items() if ('sample', 20, 0.9) in sig]
        assert hs and all(h['graph'] not in (None, False) for _, h in hs), [h.get('error') for _, h in hs]
        assert all(h.get(('multi', 8)) for _, h in hs), [h.get('multi_error') for _, h in hs]
        tr.MULTI_STEP_GRAPHS = False
        model.__dict__['_decode_graphs'].clear()
        s = gen(11)
        assert torch.equal(s[0], a[0]) and torch.equal(s[1], a[1])
        hs = [h for sig, h in model.__dict__['_decode_graphs'].items() if ('sample', 20, 0.9) in sig]
        assert hs and all(h['graph'] not in (None, False) for h in hs)
    finally:
        tr.MULTI_STEP_GRAPHS = keep_multi


def test_fullsize_sampling_lanes_equal_batch_by_batch(fullsize):
    """generate_lanes draws the seeds of its batches in batch order: under one torch seed its captions are those of
    `generate` called batch by batch."""
    model, batches = fullsize
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
    with pytest.raises(ValueError):
        model.generate(**_clone(batches[0]), beam_size=2)


def test_lstm_baseline_sampling(golden):
    """BaselineGloveModel with sampling_topk = 5: every sampled token lies in the top 5 of its teacher-forced log-probs,
    the same seed gives the same ids."""
    import tell_amd
    from tell_amd.build import build_embedder
    from tell_amd.models import BaselineGloveModel, LSTMDecoder
    from tell_amd.modules import AdaptiveLoss
    from test_gpu_decoder import _PoolResnet
    tell_amd.set_compute_dtype(torch.float32)
    fx = golden('model_baseline_glove')
    dec = LSTMDecoder(None, build_embedder(600, 64, (100, 300), 512), num_layers=2, hidden_size=48, dropout=0.1,
                      share_decoder_input_output_embed=True, vocab_size=600, adaptive_softmax_cutoff=[100, 300],
                      tie_adaptive_weights=True, adaptive_softmax_dropout=0, tie_adaptive_proj=False,
                      adaptive_softmax_factor=1, article_embed_size=300, image_embed_size=2048)
    model = BaselineGloveModel(None, dec, AdaptiveLoss(1), resnet=_PoolResnet(), sampling_topk=5, sampling_temp=0.7).eval()
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
        state = {}
        lps = []
        for t in range(ids.shape[1] - 1):                     # the decoder carries its LSTM state, like _generate
            out = model.decoder({'roberta': ids[:, t:t + 1]}, contexts, incremental_state=state)
            lps.append(model.decoder.get_normalized_probs((out[0][:, -1:], None), log_probs=True).squeeze(1).float())
        lp = torch.stack(lps, 1)
    alive = _alive(ids.cpu()).to(DEV)
    tok = ids[:, 1:]
    fifth = lp.topk(5, dim=-1).values[..., -1]
    lp_tok = lp.gather(2, tok.unsqueeze(-1)).squeeze(-1)
    assert (lp_tok >= fifth - 1e-5)[alive].all()
    assert torch.allclose(a['log_probs'][alive], (lp_tok / 0.7)[alive], atol=1e-4, rtol=0)
