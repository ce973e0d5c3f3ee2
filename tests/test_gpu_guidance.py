"""Context guidance on the MI355X: tell_adaptive_logprob_topk_guided against the plain definition of
tests/test_guidance_host.py (guided_rows), the fp32 generators against greedy_guided / beam_search_guided on the oracle at
full size, the fused captured bf16 path at the bench batch, and the defaults, which must change nothing."""
import numpy as np
import pytest
import torch

from test_gpu_beam_options import _clone, _Spy
from test_gpu_sampling import LAYOUTS, _Rows
from test_guidance_host import (FP32_ALPHA, FP32_B, FP32_CASES, FP32_GEN, beam_search_guided, fullsize_oracle, greedy_guided,
                                guided_rows)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NEW = 'tell_adaptive_logprob_topk_guided'
PLAIN_PICKS = {'tell_adaptive_logprob_argmax', 'tell_adaptive_logprob_topk', 'tell_adaptive_logprob_topk_banned',
               'tell_adaptive_logprob_topk_penalised', 'tell_adaptive_logprob_topk_masked', 'tell_adaptive_logprob_sample',
               'tell_adaptive_logprob_nucleus', 'tell_adaptive_logprob_forced'}
GAMMAS = (0.0, 1.0, 1.5, 3.0, 7.5)
# |lps - (s_rows[token] - L)| with L the float64 log-sum-exp of the device's own s_rows: the largest value measured over every
# case below is 6.5e-6 (register form, three_tails, 32 pairs); the bound is four times that, rounded up to one digit, and may
# never pass 1e-4 (a reported probability off by more than 0.01 %)
L_BOUND = 3e-5
assert L_BOUND <= 1e-4


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    yield
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- 1. the kernel, through the C ABI
def _t(x):
    """The bound tests/test_gpu_nucleus.py holds a reported log-prob to."""
    return 1e-6 * np.abs(x) + 2e-6


class _Pairs:
    """R pairs in N = 2 R + 1 logit rows: conditional rows 0 .. R - 1, a row that belongs to no pair, partners R + 1 .. 2 R
    (pair_offset = R + 1).  ties: row 0 and its partner hold exactly equal logits at eight head tokens."""

    def __init__(self, R, c0, tails, seed, shift=0, twin=False):
        self.R, self.off, self.V = R, R + 1, c0 + sum(tails)
        X = self.X = _Rows(2 * R + 1, c0, tails, seed, shift=shift, ties=True)
        pos = slice(shift + 17, shift + 17 + 8 * 97, 97)
        X.head[self.off, pos] = 0.25                                      # ... so that s ties there as lp_c does
        if twin:                                                          # u a copy of c
            for t in [X.head] + [t for t, _ in X.tl]:
                t[self.off:] = t[:R]
        self.full = X.full()[0]
        self.lp_c, self.lp_u = self.full[:R], self.full[self.off:]

    def launch(self, k, gamma_dev, want_s=True):
        from tell_amd.hip import call
        N = 2 * self.R + 1
        tok = torch.full((N, k), -7, dtype=torch.int32, device=DEV)
        lps = torch.full((N, k), -7.0, dtype=torch.float32, device=DEV)
        s = torch.full((self.R, self.V + 3), -7.0, dtype=torch.float32, device=DEV) if want_s else None
        call(NEW, *self.X.args(), self.R, self.off, k, gamma_dev, s, self.V + 3 if want_s else 0, tok, lps)
        torch.cuda.synchronize()
        if want_s:
            assert bool((s[:, self.V:] == -7.0).all())                    # nothing behind the vocabulary
            s = s[:, :self.V].cpu().numpy()
        return tok.cpu().numpy(), lps.cpu().numpy(), s


def _check_pairs(P, form, worst):
    """(a) - (d) and the gamma = 1 half of (e) for one set of pairs, every gamma and k."""
    R, off = P.R, P.off
    ids = np.arange(P.V)
    gamma_dev = torch.zeros(1, dtype=torch.float32, device=DEV)
    lc, lu = P.lp_c.astype(np.float64), P.lp_u.astype(np.float64)
    for gamma in GAMMAS:
        gamma_dev.fill_(gamma)
        a = abs(gamma - 1.0)
        want = lc + (gamma - 1.0) * (lc - lu)
        E = (1 + a) * _t(lc) + a * _t(lu) + 2.0 ** -22 * (np.abs(lc) + a * np.abs(lc - lu))
        tok8, lps8, s = P.launch(8, gamma_dev)
        err = np.abs(s.astype(np.float64) - want)
        assert (err <= E).all(), (form, R, gamma, float((err / E).max()))                            # (a)
        order = np.stack([np.lexsort((ids, -row))[:8] for row in s])
        s64 = s.astype(np.float64)
        mx = s64.max(1, keepdims=True)
        L = (mx + np.log(np.exp(s64 - mx).sum(1, keepdims=True)))[:, 0]
        for k in (1, 4, 8):
            tok, lps, s_k = (tok8, lps8, s) if k == 8 else P.launch(k, gamma_dev)
            assert np.array_equal(s_k.view(np.uint32), s.view(np.uint32)), (form, R, gamma, k)
            assert np.array_equal(tok[:R], order[:, :k]), (form, R, gamma, k)                        # (b)
            got = lps[:R].astype(np.float64)
            ref = np.take_along_axis(s64, tok[:R].astype(np.int64), 1) - L[:, None]
            worst.append(float(np.abs(got - ref).max()))
            assert worst[-1] <= L_BOUND, (form, R, gamma, k, worst[-1])                              # (c)
            assert np.array_equal(tok[off:], tok[:R]) and np.array_equal(lps[off:].view(np.uint32), lps[:R].view(np.uint32))  # (d)
            assert (tok[R] == -7).all() and (lps[R] == -7.0).all()                                   # the row of no pair: untouched
            tok_n, lps_n, _ = P.launch(k, gamma_dev, want_s=False)                                   # s_rows = NULL: the same pick
            assert np.array_equal(tok_n, tok) and np.array_equal(lps_n.view(np.uint32), lps.view(np.uint32))
            if gamma == 1.0:                                                                          # (e)
                assert np.array_equal(tok[:R], P.X.topk(k)[:R]), (form, R, k)
        if form != 'small':                                                                           # the planted ties are ties,
            assert len(set(s[0, 17:17 + 8 * 97:97].tolist())) == 1                                    # and at gamma = 1 the row's top
            assert gamma != 1.0 or sorted(order[0].tolist()) == list(range(17, 17 + 8 * 97, 97))
        # the host restatement, on the device's arithmetic: fp32 s within two ulps of rounding lp to fp32 first
        s_host, _, _ = guided_rows(P.lp_c, P.lp_u, gamma)
        assert (np.abs(s_host.astype(np.float64) - want) <= E).all()


@pytest.mark.parametrize('R', [1, 3, 32])
@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_guided_pick_register_form(layout, R):
    """s_rows against the float64 formula within E, tokens exactly the k best of the device's own s_rows (lower id first on the
    planted ties), lps = s - L within L_BOUND, both rows of a pair identical, gamma = 1 the tokens of tell_adaptive_logprob_topk -
    k in {1, 4, 8}, gamma in {0, 1, 1.5, 3, 7.5}."""
    c0, tails = LAYOUTS[layout]
    worst = []
    _check_pairs(_Pairs(R, c0, tails, seed=11 * R + len(tails)), 'regs', worst)
    print('\nregister form %s R=%d: max |lps - (s - L)| %.2e' % (layout, R, max(worst)))


@pytest.mark.parametrize('how', ['unaligned', 'option'])
@pytest.mark.parametrize('shape', ['37+5', '130+61+7+3', 'build_model'])
def test_guided_pick_streaming_form(shape, how):
    """The same properties on the streaming form: rows that do not start on 16 bytes, and option argmax_regs = 0; small odd
    shapes (one and three tails) and the full-size layout."""
    import tell_amd
    c0, tails = {'37+5': (37, (5,)), '130+61+7+3': (130, (61, 7, 3)), 'build_model': LAYOUTS['build_model']}[shape]
    small = shape != 'build_model'
    worst = []
    with tell_amd.hip.options(argmax_regs=0 if how == 'option' else 1):
        for R in ((1, 3, 5) if small else (3,)):
            _check_pairs(_Pairs(R, c0, tails, seed=7 * R + len(tails), shift=1 if how == 'unaligned' else 0),
                         'small' if small else 'stream', worst)
    print('\nstreaming form %s (%s): max |lps - (s - L)| %.2e' % (shape, how, max(worst)))


@pytest.mark.parametrize('shape', ['37+5', '130+61+7+3'])
def test_guided_pick_register_form_on_small_odd_rows(shape):
    """Aligned small rows take the register form: segments that end inside a float4, and threads without any element."""
    c0, tails = {'37+5': (37, (5,)), '130+61+7+3': (130, (61, 7, 3))}[shape]
    worst = []
    for R in (1, 4):
        _check_pairs(_Pairs(R, c0, tails, seed=3 * R + len(tails)), 'small', worst)
    print('\nregister form %s: max |lps - (s - L)| %.2e' % (shape, max(worst)))


@pytest.mark.parametrize('regs', [1, 0])
def test_a_copy_as_partner_is_the_plain_topk_and_gamma_is_read_from_the_device(regs):
    """(e) u a copy of c at gamma = 3: d is an exact zero, s is lp_c bit for bit, the tokens are tell_adaptive_logprob_topk's.
    (f) a host change of gamma between two launches - eager, and between two replays of one captured launch - is picked up."""
    import tell_amd
    from tell_amd.hip import call
    c0, tails = LAYOUTS['build_model']
    with tell_amd.hip.options(argmax_regs=regs):
        P = _Pairs(3, c0, tails, seed=21, twin=True)
        gamma_dev = torch.full((1,), 3.0, dtype=torch.float32, device=DEV)
        for k in (1, 4, 8):
            tok, lps, s = P.launch(k, gamma_dev)
            assert np.array_equal(tok[:3], P.X.topk(k)[:3]), (regs, k)
            np.testing.assert_allclose(s, P.lp_c, rtol=1e-6, atol=2e-6)
        Q = _Pairs(3, c0, tails, seed=22)
        got = {}
        for gamma in (1.5, 3.0, 1.5):
            gamma_dev.fill_(gamma)
            tok, lps, s = Q.launch(4, gamma_dev)
            if gamma in got:
                assert np.array_equal(got[gamma][0], tok) and np.array_equal(got[gamma][1], s)
            got[gamma] = (tok, s)
            want, _, _ = guided_rows(Q.lp_c, Q.lp_u, gamma)
            np.testing.assert_allclose(s, want, rtol=0, atol=1e-4)
        assert not np.array_equal(got[1.5][1], got[3.0][1])
        # one captured launch, two gammas
        N = 2 * Q.R + 1
        tok = torch.zeros(N, 4, dtype=torch.int32, device=DEV)
        lps = torch.zeros(N, 4, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call(NEW, *Q.X.args(), Q.R, Q.off, 4, gamma_dev, None, 0, tok, lps)
        for gamma in (3.0, 1.5):
            gamma_dev.fill_(gamma)
            g.replay()
            torch.cuda.synchronize()
            t = tok.cpu().numpy()
            assert np.array_equal(t[:Q.R], got[gamma][0][:Q.R]) and np.array_equal(t[Q.off:], t[:Q.R]), gamma


def test_the_launcher_refuses_bad_arguments():
    from tell_amd.hip import call
    P = _Pairs(2, 37, (5,), seed=1)
    gamma = torch.ones(1, dtype=torch.float32, device=DEV)
    tok = torch.zeros(5, 4, dtype=torch.int32, device=DEV)
    lps = torch.zeros(5, 4, dtype=torch.float32, device=DEV)
    s = torch.zeros(2, 42, dtype=torch.float32, device=DEV)
    for bad, what in ((dict(k=0), 'k <= 8'), (dict(k=9), 'k <= 8'), (dict(off=1), 'pair_offset'), (dict(gamma=None), 'gamma_dev'),
                      (dict(ld_s=41), 's_rows')):
        a = dict(k=4, off=3, gamma=gamma, ld_s=42)
        a.update(bad)
        with pytest.raises(RuntimeError, match=what):
            call(NEW, *P.X.args(), 2, a['off'], a['k'], a['gamma'], s, a['ld_s'], tok, lps)


# --------------------------------------------------------------------------- 2. / 3. fp32, full-size decoder
@pytest.fixture(scope='module')
def fp32_models():
    import tell_amd
    from tell_amd.build import build_decoder
    from tell_amd.models.transformer import CaptionModel
    from test_gpu_fullsize import _to_dev
    om, sd, ctx, start = fullsize_oracle()
    tell_amd.set_compute_dtype(torch.float32)
    dec = build_decoder('faces_objects')
    dec.load_state_dict(sd)
    dec.to(DEV).eval()
    m = CaptionModel.__new__(CaptionModel)
    torch.nn.Module.__init__(m)
    m.decoder, m.padding_idx, m.index, m.sampling_topk, m.sampling_temp = dec, 1, 'roberta', 1, 1.0
    m.training = False
    return om, m, ctx, start, _to_dev(ctx, torch.float32)


def _same(got, want):
    got = got.cpu()
    n = min(got.shape[-1], want.shape[-1])
    assert torch.equal(got[..., :n], want[..., :n]), (got, want)
    assert (got[..., n:] == 1).all() and (want[..., n:] == 1).all()


@pytest.mark.parametrize('case', range(len(FP32_CASES)))
def test_full_size_generators_under_guidance_match_the_definition_fp32(fp32_models, case):
    """B = 4, 12 steps, sharpened </s>: the cached fp32 generators (the layer-by-layer path, through the same head) against
    greedy_guided, and beam 4 with n_best = 4 and a length penalty against beam_search_guided - identical ids, scores within
    section 16's rtol 1e-4 / atol 5e-4; the pick is the guided one, and it changes the captions."""
    import tell_amd
    om, m, ctx, start, dctx = fp32_models
    tell_amd.set_compute_dtype(torch.float32)
    drop, gamma = FP32_CASES[case]
    GEN = FP32_GEN
    c = lambda: {k: v.clone() for k, v in ctx.items()}       # noqa: E731
    with torch.no_grad():
        _, plain_ids, _ = m._generate_cached(start.to(DEV), dctx, gen_len=GEN, eos=2)
        want_ids, want_sc = greedy_guided(om, start, c(), drop, gamma, gen_len=GEN)
        with _Spy() as spy:
            lp, got, _ = m._generate_cached(start.to(DEV), dctx, gen_len=GEN, eos=2, guide=(drop, gamma))
        assert NEW in spy.names and not PLAIN_PICKS & set(spy.names)
        assert got.shape[0] == FP32_B and lp.shape[0] == FP32_B
        _same(got, want_ids)
        print('\nfp32 greedy %s gamma %.1f: scores %s vs definition %s' % ('+'.join(drop), gamma, lp.sum(1).cpu().tolist(),
                                                                          want_sc.tolist()))
        assert torch.allclose(lp.sum(1).cpu(), want_sc, rtol=1e-4, atol=5e-4)
        n = min(got.shape[1], plain_ids.shape[1])
        assert got.shape != plain_ids.shape or not torch.equal(got[:, :n], plain_ids[:, :n])       # guidance changes a caption
        want_b, want_sc = beam_search_guided(om, start, c(), drop, gamma, 4, gen_len=GEN, alpha=FP32_ALPHA)
        m.beam_len_penalty = FP32_ALPHA
        try:
            with _Spy() as spy:
                lp, got, info = m._generate_beam(start.to(DEV), dctx, 4, gen_len=GEN, eos=2, n_best=4, guide=(drop, gamma))
        finally:
            m.beam_len_penalty = 0.0
        assert NEW in spy.names and not PLAIN_PICKS & set(spy.names)
        ids_n, lps_n, sc_n = info.nbest
        assert ids_n.shape[0] == FP32_B and sc_n.shape == (FP32_B, 4)
        print('fp32 beam 4 %s gamma %.1f: scores %s vs definition %s' % ('+'.join(drop), gamma, sc_n.cpu().tolist(), want_sc.tolist()))
        _same(ids_n, want_b)
        _same(got, want_b[:, 0])
        assert torch.allclose(sc_n.cpu(), want_sc, rtol=1e-4, atol=5e-4), (sc_n, want_sc)
        assert torch.allclose(info.scores.cpu(), want_sc[:, 0], rtol=1e-4, atol=5e-4)


def test_nothing_to_drop_changes_nothing_fp32(fp32_models):
    """A batch whose faces context is fully masked already, drop = ('faces',), gamma = 3: the twin rows see what the
    conditional rows see, d is zero up to the two rows' rounding, and the captions are the unguided ones."""
    import tell_amd
    om, m, ctx, start, dctx = fp32_models
    tell_amd.set_compute_dtype(torch.float32)
    dctx = dict(dctx, faces_mask=torch.ones_like(dctx['faces_mask']))
    with torch.no_grad():
        lp0, ids0, _ = m._generate_cached(start.to(DEV), dctx, gen_len=FP32_GEN, eos=2)
        lp1, ids1, _ = m._generate_cached(start.to(DEV), dctx, gen_len=FP32_GEN, eos=2, guide=(('faces',), 3.0))
        assert torch.equal(ids0, ids1)
        assert torch.allclose(lp1, lp0, rtol=1e-4, atol=5e-4)
        _, b0, i0 = m._generate_beam(start.to(DEV), dctx, 4, gen_len=FP32_GEN, eos=2)
        _, b1, i1 = m._generate_beam(start.to(DEV), dctx, 4, gen_len=FP32_GEN, eos=2, guide=(('faces',), 3.0))
        assert torch.equal(b0, b1)
        assert torch.allclose(i1.scores, i0.scores, rtol=1e-4, atol=5e-4)


# --------------------------------------------------------------------------- 4. bf16, the fused captured path
BF16_EOS_FACTOR = 12.0


@pytest.fixture(scope='module')
def fullsize():
    import tell_amd
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    from test_gpu_fullsize import _sharpened_eos
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    plain = build_model('faces_objects')
    sd = _sharpened_eos(plain.state_dict(), BF16_EOS_FACTOR)
    plain.load_state_dict(sd)
    plain.to(DEV).eval()
    batches = [synthetic_batch(32, 64, 9, True, seed=91, device=DEV), synthetic_batch(32, 64, 9, True, seed=93, device=DEV),
               synthetic_batch(4, 64, 9, True, seed=92, device=DEV)]
    yield plain, batches
    tell_amd.set_compute_dtype(torch.float32)


def _guide_graphs(model):
    return [h for sig, h in model.__dict__['_decode_graphs'].items() if any(isinstance(e, tuple) and e[:1] == ('guide',) for e in sig)]


class _NoCapture:
    """The stepper's view of tell_amd.graphs with captures refused: every step is issued launch by launch."""

    def __getattr__(self, name):
        import tell_amd
        return getattr(tell_amd.graphs, name)

    @staticmethod
    def capture(*a, **kw):
        raise RuntimeError('capture refused by the test')


def _eager(model, run):
    from tell_amd.models import stepper as stepper_mod
    keep = stepper_mod.graphs
    model.__dict__.pop('_decode_graphs', None)
    try:
        stepper_mod.graphs = _NoCapture()
        with _Spy() as spy:
            out = run()
        torch.cuda.synchronize()
        hs = _guide_graphs(model)
        assert hs and all(h['graph'] is False for h in hs)              # every step of this run was issued eagerly
    finally:
        stepper_mod.graphs = keep
        model.__dict__.pop('_decode_graphs', None)
    return out, spy


@pytest.mark.parametrize('mode', ['greedy', 'beam4'])
def test_fused_bf16_path_under_guidance_at_the_bench_batch(fullsize, mode):
    """32 captions (64 images in the static batch; beam 4: 256 rows): the captured step against the same step issued launch by
    launch - identical ids -, a second batch and a second gamma through the same graph, and gamma = 0 against a plain generate
    on the batch whose image mask is all-masked."""
    plain, batches = fullsize
    b, b2 = batches[0], batches[1]
    kw = {'greedy': {}, 'beam4': dict(beam_size=4, n_best=4)}[mode]
    keys = ('gen_ids', 'log_probs', 'scores') + {'greedy': (), 'beam4': ('gen_ids_nbest', 'log_probs_nbest', 'scores_nbest')}[mode]
    with torch.no_grad():
        plain.reset_graphs()
        free = plain.generate(**_clone(b), **kw)
        out = plain.generate(**_clone(b), **kw, guidance=3.0)
        torch.cuda.synchronize()
        hs = _guide_graphs(plain)
        assert len(hs) == 1 and hs[0]['graph'] not in (None, False), [h.get('error') for h in hs]
        assert any(('guide', ('image',)) == e for sig in plain.__dict__['_decode_graphs'] for e in sig if isinstance(e, tuple))
        graph = hs[0]['graph']
        assert out['gen_ids'].shape[0] == 32
        n = min(out['gen_ids'].shape[1], free['gen_ids'].shape[1])
        assert out['gen_ids'].shape != free['gen_ids'].shape or not torch.equal(out['gen_ids'][:, :n], free['gen_ids'][:, :n])
        # a second batch, then another gamma: the same entry, the same graph
        two = plain.generate(**_clone(b2), **kw, guidance=3.0)
        other = plain.generate(**_clone(b), **kw, guidance=1.5)
        again = plain.generate(**_clone(b), **kw, guidance=3.0)
        zero = plain.generate(**_clone(b), **kw, guidance=0.0)
        torch.cuda.synchronize()
        hs = _guide_graphs(plain)
        assert len(hs) == 1 and hs[0]['graph'] is graph
        for key in keys:
            assert torch.equal(again[key], out[key]), (mode, key)
        assert two['gen_ids'].shape[0] == 32 and other['gen_ids'].shape[0] == 32

        def run():
            return plain.generate(**_clone(b), **kw, guidance=3.0)
        eager, spy = _eager(plain, run)
        assert NEW in spy.names and not PLAIN_PICKS & set(spy.names)
        for key in keys:                                                    # captured and launch by launch: identical
            assert torch.equal(eager[key], out[key]), (mode, key)
        # gamma = 0: s ~ lp_u, the decode without the image - against a plain generate whose image mask is all-masked
        keep = plain._no_mask
        try:
            plain._no_mask = lambda B, P, device: torch.ones_like(keep(B, P, device))
            blind = plain.generate(**_clone(b), **kw)
        finally:
            plain._no_mask = keep
        torch.cuda.synchronize()
    n = min(zero['gen_ids'].shape[1], blind['gen_ids'].shape[1])
    agree = float((zero['gen_ids'][:, :n] == blind['gen_ids'][:, :n]).float().mean())
    print('\nbf16 B=32 %s: gamma = 0 against the plain decode without the image: position-wise agreement %.3f over %d positions'
          % (mode, agree, 32 * n))
    assert agree >= 0.8                # (tests/test_gpu_fullsize.py's gate on two bf16 launch sequences of one model)


def test_defaults_change_nothing_on_the_fused_path(fullsize):
    """A model built with the keys at their defaults and called with guidance=None / 1.0 against one built and called without
    them: the same tensors, the same graph keys, and - warm steps, captures and bookkeeping - the same sequence of entry
    points, the guided pick not among them."""
    from tell_amd.build import build_model
    plain, batches = fullsize
    keyed = build_model('faces_objects', resnet=plain.resnet, roberta=plain.roberta, guidance_scale=1.0, guidance_drop=['image', 'obj'])
    keyed.load_state_dict(plain.state_dict())
    keyed.to(DEV).eval()
    assert keyed.guidance_drop == ('image', 'obj')
    b = batches[2]
    with torch.no_grad():
        for K in (4, 1):
            for gkw in (dict(guidance=None), dict(guidance=1.0, guidance_drop=['article'])):
                plain.generate(**_clone(b), beam_size=K)                  # (working weights cached on both sides first)
                keyed.generate(**_clone(b), beam_size=K)
                plain.reset_graphs()
                keyed.reset_graphs()
                with _Spy() as sa:
                    a = plain.generate(**_clone(b), beam_size=K)
                with _Spy() as sk:
                    k_ = keyed.generate(**_clone(b), beam_size=K, **gkw)
                torch.cuda.synchronize()
                assert torch.equal(a['gen_ids'], k_['gen_ids']) and torch.equal(a['log_probs'], k_['log_probs'])
                assert torch.equal(a['scores'], k_['scores'])
                pk = [s_[:5] + s_[6:] for s_ in plain.__dict__['_decode_graphs']]     # (all but the position table's address)
                kk = [s_[:5] + s_[6:] for s_ in keyed.__dict__['_decode_graphs']]
                assert pk == kk and not _guide_graphs(keyed)
                assert all(h['graph'] not in (None, False) for h in keyed.__dict__['_decode_graphs'].values())
                assert all('gamma' not in h for h in keyed.__dict__['_decode_graphs'].values())
                assert sa.names == sk.names and len(sa.names) > 100
                assert NEW not in sk.names
                assert ('tell_beam_update' if K > 1 else 'tell_greedy_update') in sk.names


@pytest.mark.parametrize('K', [1, 4])
def test_generate_lanes_takes_the_same_arguments(fullsize, K):
    """Two lanes in flight, each with its batch and the batch's twin: the captions of `generate` with the same arguments."""
    plain, batches = fullsize
    b = batches[2]
    kw = dict(beam_size=K, n_best=K) if K > 1 else {}
    with torch.no_grad():
        want = plain.generate(**_clone(b), **kw, guidance=3.0, guidance_drop=['image', 'obj'])
        free = plain.generate(**_clone(b), **kw)
        outs = list(plain.generate_lanes([_clone(b), _clone(b)], guidance=3.0, guidance_drop=['image', 'obj'], **kw))
        torch.cuda.synchronize()
    assert len(outs) == 2
    for _, o in outs:
        assert torch.equal(o['gen_ids'], want['gen_ids']) and torch.equal(o['scores'], want['scores'])
    n = min(want['gen_ids'].shape[1], free['gen_ids'].shape[1])
    assert want['gen_ids'].shape != free['gen_ids'].shape or not torch.equal(want['gen_ids'][:, :n], free['gen_ids'][:, :n])
    with pytest.raises(ValueError, match='guidance.*forward'):
        list(plain.generate_lanes([_clone(b)], forward=True, guidance=3.0))
