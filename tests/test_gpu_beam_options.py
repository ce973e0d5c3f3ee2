"""Search options of the cached generators on the MI355X: the three entry points against the plain
definitions of tests/test_beam_options_host.py (ban_set, beam_update_norm, beam_search_opts), the fp32 generators against
the prefix-re-decoding definition at full size, and the invariants of the fused captured bf16 path at the bench batch."""
import numpy as np
import pytest
import torch

from test_beam_options_host import (ban_set, beam_search_opts, beam_update_norm, eos_before, inv_norm, repeats_ngram)

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# --------------------------------------------------------------------------- 1. tell_decode_ban_list
def test_ban_list_kernel_matches_ban_set():
    from tell_amd.hip import call
    rows, L, eos = 37, 40, 2
    g = torch.Generator().manual_seed(5)
    hist = torch.randint(3, 8, (rows, L), generator=g)               # five tokens: every n-gram repeats often
    hist[:, 0] = 0
    hist[3, 1:] = torch.arange(100, 100 + L - 1)                      # a row without any repeat
    hist[4, 1:] = 9                                                   # one token over and over
    hist[5, 10:15] = hist[5, 30:35] = torch.tensor([50, 51, 52, 53, 54])   # a planted 5-gram
    fin = torch.zeros(rows, dtype=torch.uint8)
    fin[[1, 8, 20]] = 1
    d_hist = torch.full((rows, L + 3), -7, dtype=torch.long)          # (a leading dimension wider than L)
    d_hist[:, :L] = hist
    d_hist, d_fin = d_hist.to(DEV), fin.to(DEV)
    for n in (1, 2, 3, 5):
        for min_len in (0, 10):
            for step in (0, 1, 2, 3, 4, 7, 20, 34, L - 1):
                got = []
                for dev_form in (False, True):
                    ban = torch.full((rows, L + 1), -1, dtype=torch.int32, device=DEV)
                    n_ban = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
                    sd = torch.tensor([step - 1], dtype=torch.int32, device=DEV) if dev_form else None
                    call('tell_decode_ban_list', d_hist, d_hist.stride(0), L, d_fin, rows, 12345 if dev_form else step, sd, n,
                         min_len, eos, ban, ban.stride(0), n_ban)
                    got.append((ban.cpu().numpy(), n_ban.cpu().numpy()))
                for ban, n_ban in got:
                    for r in range(rows):
                        want = set() if fin[r] else ban_set(hist[r].tolist(), step, n, min_len, eos)
                        assert 0 <= n_ban[r] <= L + 1
                        assert set(ban[r, :n_ban[r]].tolist()) == want, (n, min_len, step, r)
                        assert (ban[r, n_ban[r]:] == -1).all()        # nothing written behind the list
                assert np.array_equal(got[0][1], got[1][1])           # `step` and `step_dev` forms agree
                for r in range(rows):
                    assert sorted(got[0][0][r, :got[0][1][r]]) == sorted(got[1][0][r, :got[1][1][r]])


# --------------------------------------------------------------------------- 2. tell_adaptive_logprob_topk_banned
C0, TAILS = 5000, (15000, 30265)                                      # the full-size adaptive softmax: head 5002 columns


def _rows(N, seed):
    g = torch.Generator().manual_seed(seed)

    def buf(n, scale):
        ld = -(-n // 4) * 4
        return (torch.randn(N, ld, generator=g) * scale).to(DEV), ld
    head, ld_h = buf(C0 + len(TAILS), 3.0)
    tl = [buf(n, 2.0) for n in TAILS]
    head[0, 17:17 + 8 * 97:97] = head[0, :C0].max() + 1.0             # row 0: eight exactly equal logits at the top
    args = [head, ld_h, C0, len(TAILS)]
    for (t, ld), n in zip(tl, TAILS):
        args += [t, ld, n]
    return args + [None, 0, 0]


@pytest.mark.parametrize('regs', [1, 0])
@pytest.mark.parametrize('k', [1, 4, 8])
def test_banned_topk_kernel(k, regs):
    """Register (argmax_regs = 1) and streaming forms.  n_ban = 0: bitwise tell_adaptive_logprob_topk.  With bans: the
    tokens are the top k of the masked row (the full log-prob row of tell_adaptive_logprob_argmax, value descending, lower
    id first); the log-probs are bitwise those the unbanned kernel reports for the same tokens (wherever it reports them:
    its k = 8 list) and the full row's otherwise."""
    from tell_amd import hip
    from tell_amd.hip import call
    N, V = 12, C0 + sum(TAILS)
    args = _rows(N, 7)
    with hip.options(argmax_regs=regs):
        def plain(kk):
            tok = torch.empty(N, kk, dtype=torch.int32, device=DEV)
            lps = torch.empty(N, kk, dtype=torch.float32, device=DEV)
            call('tell_adaptive_logprob_topk', *args, N, kk, tok, lps)
            return tok.cpu().numpy(), lps.cpu().numpy()

        def banned(ban, n_ban):
            tok = torch.full((N, k), -5, dtype=torch.int32, device=DEV)
            lps = torch.zeros(N, k, dtype=torch.float32, device=DEV)
            call('tell_adaptive_logprob_topk_banned', *args, N, k, ban, ban.stride(0), n_ban, tok, lps)
            return tok.cpu().numpy(), lps.cpu().numpy()
        p_tok, p_lp = plain(k)
        LDB = 64
        ban = torch.randint(0, V, (N, LDB), dtype=torch.int32).to(DEV)   # (garbage behind n_ban must not matter)
        t, l = banned(ban, torch.zeros(N, dtype=torch.int32, device=DEV))
        assert np.array_equal(t, p_tok) and np.array_equal(l.view(np.int32), p_lp.view(np.int32))
        full = torch.empty(N, V, dtype=torch.float32, device=DEV)
        call('tell_adaptive_logprob_argmax', *args, N, full, V, torch.empty(N, dtype=torch.int32, device=DEV),
             torch.empty(N, dtype=torch.float32, device=DEV))
        full = full.cpu().numpy()
        top8_tok, top8_lp = plain(8)
        rng = np.random.default_rng(3)
        bans = []
        for r in range(N):
            order = np.lexsort((np.arange(V), -full[r]))
            b = [int(order[0])]                                          # the arg-max
            b += [int(np.argmax(full[r, :C0])), C0 + int(np.argmax(full[r, C0:C0 + TAILS[0]])),
                  C0 + TAILS[0] + int(np.argmax(full[r, C0 + TAILS[0]:]))]      # the best token of every cluster
            b += [int(order[2]), int(order[2]), int(order[0])]             # duplicates
            b += rng.integers(0, V, r).tolist()                          # r tokens anywhere
            if r == 0:
                b = [17, 17 + 2 * 97, 17]                                # the tie of row 0 straddles k: members 1, 3, 4, 5, ..
            if r == 1:
                b = []                                                   # a row without bans beside rows with
            if r == 2:
                b = [int(t_) for t_ in order[:20]]                       # the whole top 20
            bans.append(b)
        n_ban = torch.tensor([len(b) for b in bans], dtype=torch.int32)
        for r, b in enumerate(bans):
            ban[r, :len(b)] = torch.tensor(b, dtype=torch.int32, device=DEV) if b else ban[r, :0]
        t, l = banned(ban, n_ban.to(DEV))
        for r in range(N):
            masked = full[r].copy()
            masked[bans[r]] = -np.inf
            want = np.lexsort((np.arange(V), -masked))[:k]
            assert np.array_equal(t[r], want), (r, t[r], want)
            for q in range(k):
                hit = np.nonzero(top8_tok[r] == t[r, q])[0]
                if hit.size:
                    assert l[r, q].view(np.int32) == top8_lp[r, hit[0]].view(np.int32), (r, q)
                else:
                    assert abs(l[r, q] - full[r, t[r, q]]) <= 4e-6, (r, q)
        assert np.array_equal(t[1], p_tok[1]) and np.array_equal(l[1].view(np.int32), p_lp[1].view(np.int32))
        assert list(t[0]) == [17 + 97 * m for m in (1, 3, 4, 5, 6, 7)][:k] + [int(x) for x in t[0][6:]]


# --------------------------------------------------------------------------- 3. tell_beam_update_norm
@pytest.mark.parametrize('K', [2, 4, 8])
def test_beam_update_norm_kernel_matches_the_numpy_definition(K):
    """Several steps with finished and live hypotheses, an ancestor table and tied scores (log-probs on a grid of 1/4);
    everything the launch writes is compared exactly.  1 / T is a power of two here, so that lp * (1 / T) is exact and the
    sum cum + lp * (1 / T) has one rounding whether or not the compiler contracts it into a fused multiply-add."""
    from tell_amd import ops
    B, L, pad, eos, NB = 6, 14, 1, 2, 5
    for alpha, inv_temp, grid in ((1.0, 1.0, True), (0.7, 0.5, False), (2.0, 2.0, True)):
        rng = np.random.default_rng(K * 10 + int(alpha * 10))
        table = inv_norm(alpha, L)
        cum = np.full((B, K), -np.inf, np.float32)
        cum[:, 0] = 0
        fin = np.zeros((B, K), bool)
        seqs = np.full((B, K, L), pad, np.int64)
        seqs[:, :, 0] = 0
        lps = np.zeros((B, K, L - 1), np.float32)
        length = np.zeros((B, K), np.int32)
        back = np.tile(np.arange(B * K, dtype=np.int32), (NB, 1))
        d = dict(cum=torch.from_numpy(cum).to(DEV), fin=torch.from_numpy(fin).to(DEV, torch.uint8),
                 seqs=torch.from_numpy(seqs).to(DEV), lps=torch.from_numpy(lps).to(DEV),
                 len=torch.from_numpy(length).to(DEV), back=torch.from_numpy(back).to(DEV),
                 cur=torch.zeros(B * K, dtype=torch.long, device=DEV), rows=torch.zeros(B * K, dtype=torch.long, device=DEV),
                 table=torch.from_numpy(table).to(DEV), counter=torch.full((1,), -3, dtype=torch.int32, device=DEV))
        mixed = 0                                  # steps whose INPUT had finished and live hypotheses side by side
        for step in range(L - 1):
            mixed += bool(fin.any() and not fin.all())
            lp = -np.sort(rng.random((B, K, K)).astype(np.float32) * 4, -1)
            if grid:
                lp = np.round(lp * 4) / 4
            tk = rng.integers(3, 60, (B, K, K)).astype(np.int32)
            tk[rng.random((B, K, K)) < 0.06] = eos
            want = beam_update_norm(tk, lp, cum, fin, seqs, lps, length, table, step, pad, eos, inv_temp, back)
            ops.call('tell_beam_update_norm', torch.from_numpy(tk).to(DEV), torch.from_numpy(lp).to(DEV), d['cum'], d['fin'],
                     d['seqs'], d['lps'], d['cur'], d['rows'], d['len'], d['table'], B, K, L, step, pad, eos, inv_temp,
                     d['back'], NB, d['counter'], None)
            cum, fin, seqs, lps, length, back = (want[k_] for k_ in ('cum', 'finished', 'seqs', 'lps', 'len', 'back'))
            assert int(d['counter']) == step
            assert np.array_equal(d['cum'].cpu().numpy().view(np.int32), cum.view(np.int32)), (alpha, step)
            assert np.array_equal(d['len'].cpu().numpy(), length), (alpha, step)
            assert np.array_equal(d['fin'].cpu().numpy().astype(bool), fin), (alpha, step)
            assert np.array_equal(d['seqs'].cpu().numpy(), seqs), (alpha, step)
            assert np.array_equal(d['lps'].cpu().numpy().view(np.int32), lps.view(np.int32)), (alpha, step)
            assert np.array_equal(d['cur'].cpu().numpy(), want['cur']) and np.array_equal(d['rows'].cpu().numpy(), want['rows'])
            assert np.array_equal(d['back'].cpu().numpy(), back), (alpha, step)
        assert mixed >= 3, mixed                   # (at K = 2 every hypothesis may have ended by the last step)


@pytest.mark.parametrize('K', [2, 4, 8])
def test_beam_update_norm_with_the_all_ones_table_is_beam_update(K):
    from tell_amd import ops
    B, L, pad, eos, NB = 5, 12, 1, 2, 4
    g = torch.Generator().manual_seed(K)

    def state():
        cum = torch.full((B, K), float('-inf'), device=DEV)
        cum[:, 0] = 0.0
        return dict(cum=cum, fin=torch.zeros(B, K, dtype=torch.uint8, device=DEV),
                    seqs=torch.full((B, K, L), pad, dtype=torch.long, device=DEV), lps=torch.zeros(B, K, L - 1, device=DEV),
                    cur=torch.zeros(B * K, dtype=torch.long, device=DEV), rows=torch.zeros(B * K, dtype=torch.long, device=DEV),
                    back=torch.arange(B * K, dtype=torch.int32, device=DEV).repeat(NB, 1).contiguous())
    a, b = state(), state()
    length = torch.zeros(B, K, dtype=torch.int32, device=DEV)
    ones = torch.ones(L + 1, device=DEV)
    for step in range(L - 1):
        top = torch.log_softmax(torch.randn(B, K, 50, generator=g), -1).topk(K, dim=-1)
        tk = top.indices.to(DEV, torch.int32).contiguous()
        tk[tk == 7] = eos
        lp = top.values.to(DEV).contiguous()
        ops.call('tell_beam_update', tk, lp, a['cum'], a['fin'], a['seqs'], a['lps'], a['cur'], a['rows'], B, K, L, step, pad, eos,
                 1.0 / 0.7, a['back'], NB, None, None)
        ops.call('tell_beam_update_norm', tk, lp, b['cum'], b['fin'], b['seqs'], b['lps'], b['cur'], b['rows'], length, ones, B, K,
                 L, step, pad, eos, 1.0 / 0.7, b['back'], NB, None, None)
        for key in a:
            x, y = a[key], b[key]
            if x.dtype == torch.float32:
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), (key, step)
    assert bool(a['fin'].any())


# --------------------------------------------------------------------------- 4. fp32, full-size decoder
FP32_GEN, FP32_EOS_FACTOR, FP32_SEED, FP32_ALPHA_MOVES = 16, 14.0, 43, 1.5


def test_full_size_generators_with_options_match_the_definition_fp32():
    """Setup of test_full_size_beam4_matches_oracle_definition_fp32 (BB = 2; K = 4, 2 and greedy): the cached fp32
    generators with (alpha, n, min_len) = (1.0, 3, 4) and each option alone against beam_search_opts - identical token
    ids (all K hypotheses, through n_best = K), scores within the rtol 1e-4 / atol 5e-4 of the existing beam test.
    Non-vacuity (checked on the oracle, asserted here): the unconstrained run repeats a 3-gram and has an </s> before
    step 4 in at least one row each, and alpha = 1.5 changes the best hypothesis of at least one row (alpha = 1 does not
    on this input: the three-token hypothesis still wins), so that case runs too at K = 4."""
    import tell_amd
    from oracle.build import build_decoder as obuild
    from tell_amd.build import build_decoder
    from test_gpu_fullsize import _inputs_batch, _oracle, _sharpened_eos, _shell_models, _to_dev
    BB, GEN = 2, FP32_GEN
    o = _oracle('faces_objects')
    sd = _sharpened_eos(o['sd'], FP32_EOS_FACTOR)
    ref = obuild('faces_objects').eval()
    ref.load_state_dict({k: v for k, v in sd.items() if k in ref.state_dict()}, strict=False)
    ctx, start = _inputs_batch(BB, seed=FP32_SEED)
    tell_amd.set_compute_dtype(torch.float32)
    dec = build_decoder('faces_objects')
    dec.load_state_dict(sd)
    dec.to(DEV).eval()
    om, m = _shell_models(ref, dec)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    c = lambda: {k: v.clone() for k, v in ctx.items()}       # noqa: E731
    dctx = _to_dev(ctx, torch.float32)

    def same(got, want):
        got = got.cpu()
        n = min(got.shape[-1], want.shape[-1])
        assert torch.equal(got[..., :n], want[..., :n]), (got, want)
        assert (got[..., n:] == 1).all() and (want[..., n:] == 1).all()
    with torch.no_grad():
        plain, _ = beam_search_opts(om, start, c(), 4, gen_len=GEN)
        assert any(repeats_ngram(h, 3) for b in plain for h in b), plain
        assert any(eos_before(h, 4) for b in plain for h in b), plain
        pen, _ = beam_search_opts(om, start, c(), 4, gen_len=GEN, alpha=FP32_ALPHA_MOVES)
        assert not torch.equal(pen[:, 0], plain[:, 0])
        for K in (4, 2):
            for alpha, n, ml in ((1.0, 3, 4), (1.0, 0, 0), (0.0, 3, 0), (0.0, 0, 4)) + (((FP32_ALPHA_MOVES, 0, 0),) if K == 4 else ()):
                want_ids, want_sc = beam_search_opts(om, start, c(), K, gen_len=GEN, alpha=alpha, ngram=n, min_len=ml)
                m.beam_len_penalty, m.no_repeat_ngram_size, m.min_len = alpha, n, ml
                lp, got, info = m._generate_beam(start.to(DEV), dctx, K, gen_len=GEN, eos=2, n_best=K)
                ids_n, lps_n, sc_n = info.nbest
                print('\nfp32 K=%d (alpha, n, min_len)=%s: scores %s vs definition %s'
                      % (K, (alpha, n, ml), sc_n.cpu().tolist(), want_sc.tolist()))
                same(ids_n, want_ids)
                same(got, want_ids[:, 0])
                assert torch.equal(ids_n[:, 0], got) and torch.equal(lps_n[:, 0], lp)
                assert torch.allclose(sc_n.cpu(), want_sc, rtol=1e-4, atol=5e-4), (sc_n, want_sc)
                assert torch.equal(info.scores, sc_n[:, 0])
                if n:
                    assert not any(repeats_ngram(h, n) for b in ids_n.cpu() for h in b)
                if ml:
                    assert not any(eos_before(h, ml) for b in ids_n.cpu() for h in b)
        for n, ml in ((3, 4), (3, 0), (0, 4)):
            want_ids, want_sc = beam_search_opts(om, start, c(), 1, gen_len=GEN, ngram=n, min_len=ml)
            m.beam_len_penalty, m.no_repeat_ngram_size, m.min_len = 0.0, n, ml
            lp, got, _ = m._generate_cached(start.to(DEV), dctx, gen_len=GEN, eos=2)
            same(got, want_ids[:, 0])
            assert torch.allclose(lp.sum(1).cpu(), want_sc[:, 0], rtol=1e-4, atol=5e-4), (lp.sum(1), want_sc)


# --------------------------------------------------------------------------- 5. / 6. bf16, the fused captured path
BF16_EOS_FACTOR, BF16_OPTS = 12.0, (1.0, 3, 12)          # (factor 12: about one fp32 greedy row in five ends within 12 steps)


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
    opt = build_model('faces_objects', resnet=plain.resnet, roberta=plain.roberta, beam_len_penalty=BF16_OPTS[0],
                      no_repeat_ngram_size=BF16_OPTS[1], min_len=BF16_OPTS[2])
    opt.load_state_dict(sd)
    opt.to(DEV).eval()
    batches = [synthetic_batch(32, 64, 9, True, seed=91, device=DEV)] + \
              [synthetic_batch(4, 64, 9, True, seed=92 + i, device=DEV) for i in range(3)]
    yield plain, opt, batches
    tell_amd.set_compute_dtype(torch.float32)


def _clone(b):
    return {k: (dict(v) if isinstance(v, dict) else v.clone()) for k, v in b.items()}


def _violations(ids, n, m):
    rows = ids.reshape(-1, ids.shape[-1]).cpu()
    return sum(repeats_ngram(h, n) for h in rows), sum(eos_before(h, m) for h in rows)


def test_fused_bf16_path_keeps_the_invariants_at_the_bench_batch(fullsize):
    plain, opt, batches = fullsize
    alpha, n, ml = BF16_OPTS
    b = batches[0]
    with torch.no_grad():
        for K in (4, 1):
            kw = dict(beam_size=K, n_best=K) if K > 1 else {}
            free = plain.generate(**_clone(b), **kw)
            out = opt.generate(**_clone(b), **kw)
            torch.cuda.synchronize()
            free_ids = free['gen_ids_nbest'] if K > 1 else free['gen_ids']
            ids = out['gen_ids_nbest'] if K > 1 else out['gen_ids']
            v_free, v_opt = _violations(free_ids, n, ml), _violations(ids, n, ml)
            print('\nbf16 B=32 K=%d: rows with a repeated %d-gram / an </s> before step %d: %s unconstrained, %s with options; '
                  '%d steps' % (K, n, ml, v_free, v_opt, ids.shape[-1] - 1))
            assert v_free[0] > 0 and v_free[1] > 0, v_free        # the unconstrained run violates both
            assert v_opt == (0, 0), v_opt
            hs = [h for sig, h in opt.__dict__['_decode_graphs'].items() if any(isinstance(s, tuple) and s[:1] == ('search',)
                                                                              for s in sig)]
            assert hs and all(h['graph'] not in (None, False) for h in hs), [h.get('error') for h in hs]
            assert any(h.get(('multi', 8)) for h in hs), [h.get('multi_error') for h in hs]
            if K == 1:
                assert torch.allclose(out['scores'], out['log_probs'].sum(-1))
                continue
            assert torch.equal(out['gen_ids'], ids[:, 0]) and torch.equal(out['log_probs'], out['log_probs_nbest'][:, 0])
            sc = out['scores_nbest']
            assert torch.equal(out['scores'], sc[:, 0])
            assert bool((sc[:, :-1] >= sc[:, 1:]).all()), sc
            # len: generated tokens, </s> included = the non-pad columns behind <s>
            length = (ids[:, :, 1:] != 1).sum(-1)
            table = torch.from_numpy(inv_norm(alpha, 101)).to(DEV)
            want = out['log_probs_nbest'].sum(-1) * table[length]
            assert torch.allclose(sc, want, rtol=2e-5, atol=1e-5), (sc - want).abs().max()


class _Spy:
    """Records the entry points issued through ops.call / decode.call (what a capture records, launch by launch)."""

    def __enter__(self):
        from tell_amd import decode, ops
        self.mods, self.real, self.names = (ops, decode), ops.call, []

        def call(name, *args):
            self.names.append(name)
            return self.real(name, *args)
        for m in self.mods:
            m.call = call
        return self

    def __exit__(self, *exc):
        for m in self.mods:
            m.call = self.real
        return False


def test_defaults_change_nothing_on_the_fused_path(fullsize):
    """A model built with the keys at their defaults against one built without them: bitwise the same tensors, the same
    graph keys, and - warm steps, captures and bookkeeping - the same sequence of entry points, none of them new."""
    from tell_amd.build import build_model
    plain, _, batches = fullsize
    keyed = build_model('faces_objects', resnet=plain.resnet, roberta=plain.roberta, beam_len_penalty=0.0,
                        no_repeat_ngram_size=0, min_len=0)
    keyed.load_state_dict(plain.state_dict())
    keyed.to(DEV).eval()
    b = batches[1]
    with torch.no_grad():
        for K in (4, 1):
            plain.generate(**_clone(b), beam_size=K)                  # (working weights cached on both sides first)
            keyed.generate(**_clone(b), beam_size=K)
            plain.reset_graphs()
            keyed.reset_graphs()
            with _Spy() as sa:
                a = plain.generate(**_clone(b), beam_size=K)
            with _Spy() as sk:
                k_ = keyed.generate(**_clone(b), beam_size=K)
            torch.cuda.synchronize()
            assert torch.equal(a['gen_ids'], k_['gen_ids']) and torch.equal(a['log_probs'], k_['log_probs'])
            assert torch.equal(a['scores'], k_['scores'])
            assert 'gen_ids_nbest' not in k_ and k_['attns'] == []
            pk = [s_[:5] + s_[6:] for s_ in plain.__dict__['_decode_graphs']]     # (all but the position table's address)
            kk = [s_[:5] + s_[6:] for s_ in keyed.__dict__['_decode_graphs']]
            assert pk == kk and not any(isinstance(x, tuple) and x[:1] == ('search',) for s_ in kk for x in s_)
            assert all(h['graph'] not in (None, False) for h in keyed.__dict__['_decode_graphs'].values())
            assert sa.names == sk.names and len(sa.names) > 100
            new = {'tell_decode_ban_list', 'tell_adaptive_logprob_topk_banned', 'tell_beam_update_norm'}
            assert not new & set(sk.names)
            assert ('tell_beam_update' if K > 1 else 'tell_greedy_update') in sk.names


def test_generate_lanes_passes_n_best_through(fullsize):
    _, opt, batches = fullsize
    K = 4
    with torch.no_grad():
        alone = [opt.generate(**_clone(b), beam_size=K, n_best=K) for b in batches[1:]]
        torch.cuda.synchronize()
        seen = 0
        for i, (_, out) in enumerate(opt.generate_lanes((_clone(b) for b in batches[1:]), beam_size=K, lanes=2, n_best=K)):
            torch.cuda.synchronize()
            for key in ('gen_ids', 'log_probs', 'scores', 'gen_ids_nbest', 'log_probs_nbest', 'scores_nbest'):
                assert torch.equal(out[key], alone[i][key]), (i, key)
            seen += 1
        assert seen == len(batches) - 1
        streamed = [o for _, o in opt.generate_stream((_clone(b) for b in batches[1:3]), beam_size=K, n_best=2)]
        for i, o in enumerate(streamed):
            assert torch.equal(o['gen_ids_nbest'], alone[i]['gen_ids_nbest'][:, :2, :o['gen_ids_nbest'].shape[-1]])
