"""Caption completion on the MI355X: tell_adaptive_logprob_forced against a float64 definition, the
fp32 generators against `forced_search` (tests/test_prefix_host.py) at full size, and the fused captured bf16 path at the
bench batch - replay of a run's own output bit for bit in every mode, beam invariants across the prefix boundary, scoring
against the criterion, and the untouched default."""
import math

import numpy as np
import pytest
import torch

from test_beam_options_host import ban_set
from test_gpu_beam_options import C0, TAILS, _Spy, _clone, _rows
from test_prefix_host import caption_len, forced_search, ragged_prefix

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD, EOS = 1, 2
V = C0 + sum(TAILS)


# --------------------------------------------------------------------------- 1. tell_adaptive_logprob_forced
def _f64_logprobs(args, N):
    """[N, V] float64 log-probs of the adaptive softmax from the logits of _rows."""
    head = args[0].cpu().double()[:, :C0 + len(TAILS)]
    hl = torch.log_softmax(head, -1)
    out = [hl[:, :C0]]
    for c, n in enumerate(TAILS):
        t = args[4 + 3 * c].cpu().double()[:, :n]
        out.append(torch.log_softmax(t, -1) + hl[:, C0 + c:C0 + c + 1])
    return torch.cat(out, 1).numpy()


@pytest.mark.parametrize('regs', [1, 0])
@pytest.mark.parametrize('k', [1, 4, 8])
def test_forced_kernel(k, regs):
    """Register (argmax_regs = 1) and streaming forms.  Forced rows: the prefix token with its float64 log-prob within the
    4e-6 of test_banned_topk_kernel, (-inf, pad) behind it; bit-equal to tell_adaptive_logprob_argmax's token_lp where the
    forced token is the arg-max; a banned token is taken.  Free rows: torch.equal to the pick kernel's output.  `step` and
    `step_dev` agree; row_ids and beams > 1 select the sample."""
    from tell_amd import hip
    from tell_amd.hip import call
    N, P, STEP = 12, 6, 2
    args = _rows(N, 7)
    logits = args                                                        # (head, ld, c0, n_tails, three (tail, ld, n))
    full = _f64_logprobs(args, N)
    with hip.options(argmax_regs=regs):
        am_tok = torch.empty(N, dtype=torch.int32, device=DEV)
        am_lp = torch.empty(N, dtype=torch.float32, device=DEV)
        call('tell_adaptive_logprob_argmax', *logits, N, None, 0, am_tok, am_lp)
        am_tok, am_lp = am_tok.cpu().numpy(), am_lp.cpu().numpy()
        best = lambda r, lo, hi: lo + int(np.argmax(full[r, lo:hi]))     # noqa: E731
        plen = [0, 1, 2, 3, 4, 5, 6, 6, 3, 0, 6, 6]
        forced_tok = {3: int(am_tok[3]), 4: C0 + 4321, 5: C0 + TAILS[0] + 12345, 6: int(am_tok[6]), 7: 4999,
                      8: best(8, C0, C0 + TAILS[0]), 10: best(10, C0 + TAILS[0], V), 11: V - 1}
        assert all(0 <= t < V for t in forced_tok.values())              # (the kernel indexes the logits with these)
        assert {r for r in range(N) if plen[r] > STEP} == set(forced_tok)
        prefix = torch.randint(3, V, (N, P + 2), generator=torch.Generator().manual_seed(1))    # (ld_prefix wider than P)
        for r, t in forced_tok.items():
            prefix[r, STEP] = t
        d_prefix, d_plen = prefix.to(DEV), torch.tensor(plen, dtype=torch.int32, device=DEV)
        # the ban list of every row holds its forced token (and the arg-max): the pick respects it, the forcing does not
        ban = torch.zeros(N, 8, dtype=torch.int32)
        for r in range(N):
            ban[r, 0], ban[r, 1] = forced_tok.get(r, int(am_tok[r])), int(am_tok[r])
        ban, n_ban = ban.to(DEV), torch.full((N,), 2, dtype=torch.int32, device=DEV)

        def pick(banned, rows=slice(0, N)):
            n = len(range(N)[rows])
            sub = [a[rows] if torch.is_tensor(a) else a for a in logits]
            tok = torch.full((n, k), -5, dtype=torch.int32, device=DEV)
            lps = torch.zeros(n, k, dtype=torch.float32, device=DEV)
            if banned:
                call('tell_adaptive_logprob_topk_banned', *sub, n, k, ban[rows], ban.stride(0), n_ban[rows], tok, lps)
            else:
                call('tell_adaptive_logprob_topk', *sub, n, k, tok, lps)
            return sub, n, tok, lps

        def force(sub, n, tok, lps, pf, pl, row_ids=None, beams=1, step=STEP, dev_form=False):
            tok, lps = tok.clone(), lps.clone()
            sd = torch.tensor([step - 1], dtype=torch.int32, device=DEV) if dev_form else None
            call('tell_adaptive_logprob_forced', *sub, n, k, pf, pf.stride(0), P, pl, pl.numel(), row_ids, beams,
                 12345 if dev_form else step, sd, PAD, tok, lps)
            return tok, lps

        for banned in (False, True):
            sub, n, p_tok, p_lp = pick(banned)
            got = [force(sub, n, p_tok, p_lp, d_prefix, d_plen, dev_form=f) for f in (False, True)]
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32))
            tok, lps = got[0][0].cpu().numpy(), got[0][1].cpu().numpy()
            for r in range(N):
                if r not in forced_tok:                                  # free: bit for bit the pick
                    assert torch.equal(got[0][0][r], p_tok[r]) and torch.equal(got[0][1][r], p_lp[r]), r
                    continue
                t = forced_tok[r]
                err = abs(float(lps[r, 0]) - full[r, t])
                print('k=%d regs=%d banned=%d row %d token %d: lp %.7f, float64 %.7f, |diff| %.2e'
                      % (k, regs, banned, r, t, lps[r, 0], full[r, t], err))
                assert tok[r, 0] == t, (r, tok[r])
                assert err <= 4e-6, (r, t, lps[r, 0], full[r, t])
                assert (tok[r, 1:] == PAD).all() and np.isneginf(lps[r, 1:]).all(), (r, tok[r], lps[r])
                if t == am_tok[r]:
                    assert lps[r, 0].view(np.int32) == am_lp[r].view(np.int32), (r, lps[r, 0], am_lp[r])
            assert {r for r, t in forced_tok.items() if t == am_tok[r]} >= {3, 6}
            # a launch in which every row is free changes nothing
            t0, l0 = force(sub, n, p_tok, p_lp, d_prefix, torch.zeros_like(d_plen))
            assert torch.equal(t0, p_tok) and torch.equal(l0.view(torch.int32), p_lp.view(torch.int32))
            t0, l0 = force(sub, n, p_tok, p_lp, d_prefix, d_plen, step=P)       # ... and one behind every prefix
            assert torch.equal(t0, p_tok) and torch.equal(l0.view(torch.int32), p_lp.view(torch.int32))
        # compacted rows: logits rows 3..5 belong to the ORIGINAL rows 6, 0, 4
        sub, n, p_tok, p_lp = pick(False, slice(3, 6))
        rid = torch.tensor([6, 0, 4], dtype=torch.int32, device=DEV)
        tok, lps = force(sub, n, p_tok, p_lp, d_prefix, d_plen, row_ids=rid)
        tok, lps = tok.cpu().numpy(), lps.cpu().numpy()
        for i, (lr, orig) in enumerate(zip((3, 4, 5), (6, 0, 4))):
            if orig in forced_tok:
                assert tok[i, 0] == forced_tok[orig] and abs(float(lps[i, 0]) - full[lr, forced_tok[orig]]) <= 4e-6
            else:
                assert (tok[i] == p_tok[i].cpu().numpy()).all() and (lps[i] == p_lp[i].cpu().numpy()).all()
        # beams = 4: rows 4 s .. 4 s + 3 are the hypotheses of sample s (3 samples: free, forced, forced)
        sub, n, p_tok, p_lp = pick(False)
        pf3 = d_prefix[[0, 4, 5]].contiguous()
        pl3 = torch.tensor([0, 6, 6], dtype=torch.int32, device=DEV)
        tok, lps = force(sub, n, p_tok, p_lp, pf3, pl3, beams=4)
        tok, lps = tok.cpu().numpy(), lps.cpu().numpy()
        for r in range(N):
            s = r // 4
            if s == 0:
                assert (tok[r] == p_tok[r].cpu().numpy()).all() and (lps[r] == p_lp[r].cpu().numpy()).all()
            else:
                t = int(pf3[s, STEP])
                assert tok[r, 0] == t and abs(float(lps[r, 0]) - full[r, t]) <= 4e-6 and (tok[r, 1:] == PAD).all()


# --------------------------------------------------------------------------- 2. fp32, full size, against the definition
def test_full_size_generators_with_a_prefix_match_the_definition_fp32():
    """Setup of test_full_size_generators_with_options_match_the_definition_fp32 at four samples: greedy, K = 4 and K = 2 with
    ragged prefixes taken from the plain greedy run (p = 0, 2, 3) and one row forced to end (two tokens, then </s>) - once
    without options, once with (alpha, n, min_len) = (1.0, 3, 4), under which that </s> is banned and taken all the same.
    Ids identical to forced_search (all K hypotheses), scores within rtol 1e-4 / atol 5e-4."""
    import tell_amd
    from oracle.build import build_decoder as obuild
    from tell_amd.build import build_decoder
    from tell_amd.models.transformer import check_prefix
    from test_gpu_beam_options import FP32_EOS_FACTOR, FP32_GEN, FP32_SEED
    from test_gpu_fullsize import _inputs_batch, _oracle, _sharpened_eos, _shell_models, _to_dev
    BB, GEN = 4, FP32_GEN
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
        plain, _, _ = forced_search(om, start, c(), 1, gen_len=GEN)
        best = plain[:, 0]
        plens = [0, min(2, caption_len(best[1]) - 1), min(3, caption_len(best[2]) - 1), 3]
        pfx = ragged_prefix(best, plens)
        pfx[3, :3] = torch.tensor([int(best[3, 1]) if int(best[3, 1]) != EOS else 7, 9, EOS])
        assert plens[0] == 0 and plens[1] >= 1 and plens[2] >= 1, (plens, best)
        checked = check_prefix(pfx, BB, dec.adaptive_softmax.vocab_size, GEN)
        assert checked[1].tolist() == plens
        # the filler of a forced candidate list survives into the next step's embedding lookup: it is pad, a table row
        assert 0 <= PAD < dec.adaptive_softmax.vocab_size and int(pfx.max()) < dec.adaptive_softmax.vocab_size
        for alpha, n, ml in ((0.0, 0, 0), (1.0, 3, 4)):
            m.beam_len_penalty, m.no_repeat_ngram_size, m.min_len = alpha, n, ml
            want_ids, want_sc, want_lps = forced_search(om, start, c(), 1, prefix=pfx, gen_len=GEN, ngram=n, min_len=ml)
            lp, got, _ = m._generate_cached(start.to(DEV), dctx, gen_len=GEN, eos=2, prefix=checked)
            print('\nfp32 greedy (alpha, n, min_len)=%s: scores %s vs definition %s'
                  % ((alpha, n, ml), lp.sum(1).cpu().tolist(), want_sc[:, 0].tolist()))
            same(got, want_ids[:, 0])
            assert torch.allclose(lp.sum(1).cpu(), want_sc[:, 0], rtol=1e-4, atol=5e-4), (lp.sum(1), want_sc)
            for r, p in enumerate(plens):
                assert got[r, 1:1 + p].cpu().tolist() == pfx[r, :p].tolist()
            assert caption_len(got[3].cpu()) == 3                     # forced to </s>: the row ends there
            for K in (4, 2):
                want_ids, want_sc, _ = forced_search(om, start, c(), K, prefix=pfx, gen_len=GEN, alpha=alpha, ngram=n,
                                                     min_len=ml)
                lp, got, info = m._generate_beam(start.to(DEV), dctx, K, gen_len=GEN, eos=2, n_best=K, prefix=checked)
                ids_n, lps_n, sc_n = info.nbest
                print('fp32 K=%d (alpha, n, min_len)=%s: scores %s vs definition %s'
                      % (K, (alpha, n, ml), sc_n.cpu().tolist(), want_sc.tolist()))
                same(ids_n, want_ids)
                same(got, want_ids[:, 0])
                assert torch.allclose(sc_n.cpu(), want_sc, rtol=1e-4, atol=5e-4), (sc_n, want_sc)
                assert torch.equal(info.scores, sc_n[:, 0])
                for r, p in enumerate(plens):
                    for j in range(K):
                        if math.isfinite(float(sc_n[r, j])):
                            assert ids_n[r, j, 1:1 + p].cpu().tolist() == pfx[r, :p].tolist(), (r, j)
                assert bool(torch.isinf(sc_n[3, 1:]).all())           # </s> forced: one finished hypothesis, K - 1 empty ones
    m.beam_len_penalty, m.no_repeat_ngram_size, m.min_len = 0.0, 0, 0


# --------------------------------------------------------------------------- 3. bf16, the fused captured path, B = 32
BF16_EOS_FACTOR, BF16_OPTS = 12.0, (1.0, 3, 12)          # (the model and batches of test_gpu_beam_options' `fullsize`)


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

    def variant(**kw):
        m = build_model('faces_objects', resnet=plain.resnet, roberta=plain.roberta, **kw)
        m.load_state_dict(sd)
        return m.to(DEV).eval()
    batches = [synthetic_batch(32, 64, 9, True, seed=91, device=DEV)] + \
              [synthetic_batch(4, 64, 9, True, seed=92 + i, device=DEV) for i in range(3)]
    yield plain, variant, batches
    tell_amd.set_compute_dtype(torch.float32)


def _ragged_from(ids):
    """Prefix lengths for a replay of `ids` [B, L]: row 0 free, every ended row forced through its </s>, the others 2..6
    tokens (never into the padding)."""
    ids = ids.cpu()
    plens = []
    for r in range(ids.shape[0]):
        n = caption_len(ids[r])
        ended = n >= 1 and int(ids[r, n]) == EOS
        plens.append(0 if r == 0 else (n if ended and r % 3 else max(min(2 + r % 5, n - 1), 0)))
    return ids, plens


def _prefixed_graphs(model):
    return [h for sig, h in model.__dict__['_decode_graphs'].items() if ('prefix',) in sig]


def test_replaying_a_runs_own_output_is_bit_exact_on_the_fused_path(fullsize):
    plain, _, batches = fullsize
    b = batches[0]
    with torch.no_grad():
        a = plain.generate(**_clone(b))
        ids, plens = _ragged_from(a['gen_ids'])
        whole = [r for r, p in enumerate(plens) if p and int(ids[r, p]) == EOS]
        print('\nbf16 B=32 greedy replay: prefix lengths %s (%d rows forced through </s>), %d steps'
              % (plens, len(whole), ids.shape[1] - 1))
        assert sum(p >= 3 for p in plens) >= 8 and plens.count(0) >= 1 and len(whole) >= 1, plens
        pfx = ragged_prefix(ids, plens).to(DEV)
        out = plain.generate(**_clone(b), prefix=pfx)
        torch.cuda.synchronize()
        assert torch.equal(out['gen_ids'], a['gen_ids']) and torch.equal(out['log_probs'], a['log_probs'])
        assert out['prefix_len'].tolist() == plens and torch.equal(out['scores'], a['scores'])
        hs = _prefixed_graphs(plain)
        assert hs and all(h['graph'] not in (None, False) for h in hs), [h.get('error') for h in hs]
        assert any(h.get(('multi', 8)) for h in hs), [h.get('multi_error') for h in hs]
        # attention maps: written for forced steps like any other step
        am = plain.generate(**_clone(b), attention=True)
        ap = plain.generate(**_clone(b), attention=True, prefix=pfx)
        torch.cuda.synchronize()
        assert torch.equal(am['gen_ids'], a['gen_ids']) and torch.equal(ap['gen_ids'], a['gen_ids'])
        assert torch.equal(ap['log_probs'], a['log_probs']) and torch.equal(ap['attn_steps'], am['attn_steps'])
        assert set(ap['attns']) == set(am['attns']) and all(torch.equal(ap['attns'][n], am['attns'][n]) for n in am['attns'])


@pytest.mark.parametrize('mode', ['topk', 'nucleus'])
def test_sampled_runs_replay_under_the_same_seed(fullsize, mode):
    """A free step at index i draws what it draws in the unprefixed run (the uniform is the hash of (seed, row, step)): ids
    torch.equal; log-probs within the atol 1e-4 the sampling tests put on reported log-probs."""
    _, variant, batches = fullsize
    model = variant(sampling_topk=8, sampling_temp=0.8) if mode == 'topk' else \
        variant(sampling_topk=0, sampling_temp=0.8, sampling_topp=0.9)
    b = batches[0]
    with torch.no_grad():
        torch.manual_seed(5)
        a = model.generate(**_clone(b))
        ids, plens = _ragged_from(a['gen_ids'])
        assert sum(p >= 3 for p in plens) >= 8 and plens.count(0) >= 1, plens
        pfx = ragged_prefix(ids, plens).to(DEV)
        torch.manual_seed(5)
        out = model.generate(**_clone(b), prefix=pfx)
        torch.cuda.synchronize()
        diff = (out['log_probs'] - a['log_probs']).abs().max().item()
        print('\nbf16 B=32 %s replay: prefix lengths %s, max |log-prob difference| %.3e' % (mode, plens, diff))
        assert torch.equal(out['gen_ids'], a['gen_ids'])
        assert torch.allclose(out['log_probs'], a['log_probs'], atol=1e-4, rtol=0), diff
        assert _prefixed_graphs(model) and all(h['graph'] not in (None, False) for h in _prefixed_graphs(model))


def test_beam_with_options_keeps_its_invariants_across_the_prefix_boundary(fullsize):
    plain, variant, batches = fullsize
    alpha, n, ml = BF16_OPTS
    opt = variant(beam_len_penalty=alpha, no_repeat_ngram_size=n, min_len=ml)
    b, K = batches[0], 4
    with torch.no_grad():
        a = plain.generate(**_clone(b))
        ids, plens = _ragged_from(a['gen_ids'])
        pfx = ragged_prefix(ids, plens)
        assert 0 <= PAD < opt.decoder.adaptive_softmax.vocab_size     # the filler token is a row of the embedding table
        out = opt.generate(**_clone(b), beam_size=K, n_best=K, prefix=pfx.to(DEV))
        torch.cuda.synchronize()
        hyp, sc = out['gen_ids_nbest'].cpu(), out['scores_nbest'].cpu()
        assert out['prefix_len'].tolist() == plens and bool(torch.isfinite(sc[:, 0]).all())
        assert bool((sc[:, :-1] >= sc[:, 1:]).all()), sc
        free_tokens = 0
        for r, p in enumerate(plens):
            for j in range(K):
                h = hyp[r, j].tolist()
                if not math.isfinite(float(sc[r, j])):
                    continue
                assert h[1:1 + p] == pfx[r, :p].tolist(), (r, j, h)
                for i in range(p, len(h) - 1):                        # every FREE step respects the bans of its history
                    if h[i + 1] == PAD:
                        break
                    assert h[i + 1] not in ban_set(h, i, n, ml, EOS), (r, j, i, h)
                    free_tokens += 1
        assert free_tokens > 100
        assert int(hyp.max()) < opt.decoder.adaptive_softmax.vocab_size and int(hyp.min()) >= 0
        hs = _prefixed_graphs(opt)
        assert hs and all(h['graph'] not in (None, False) for h in hs), [h.get('error') for h in hs]
        # n_best and the prefix come through generate_lanes (batch['prefix']) and generate_stream
        small = []
        for bb in batches[1:]:
            g = plain.generate(**_clone(bb))
            gi, gp = _ragged_from(g['gen_ids'])
            small.append(dict(_clone(bb), prefix=ragged_prefix(gi, gp).to(DEV)))
        alone = [opt.generate(**_clone(bb), beam_size=K, n_best=K) for bb in small]
        torch.cuda.synchronize()
        seen = 0
        for i, (_, o) in enumerate(opt.generate_lanes((_clone(bb) for bb in small), beam_size=K, lanes=2, n_best=K)):
            torch.cuda.synchronize()
            for key in ('gen_ids', 'log_probs', 'scores', 'gen_ids_nbest', 'log_probs_nbest', 'scores_nbest', 'prefix_len'):
                assert torch.equal(o[key], alone[i][key]), (i, key)
            seen += 1
        assert seen == len(small)
        for i, (_, o) in enumerate(opt.generate_stream((_clone(bb) for bb in small[:2]), beam_size=K, n_best=2)):
            assert torch.equal(o['gen_ids_nbest'], alone[i]['gen_ids_nbest'][:, :2, :o['gen_ids_nbest'].shape[-1]])
            assert torch.equal(o['prefix_len'], alone[i]['prefix_len'])


def test_score_captions_matches_the_criterion(fullsize):
    """The summed negative log-probs of score_captions against the criterion's summed NLL of `forward` on the same batch, in
    bf16: rtol 3e-2 (what tests/test_gpu_decoder.py puts on the bf16 loss; it puts 1e-3 on the fp32 one)."""
    from tell_amd.data import synthetic_batch
    plain, _, _ = fullsize
    b = synthetic_batch(32, 64, 9, True, seed=97, variable=True, device=DEV)
    with torch.no_grad():
        fw = plain(**_clone(b))
        nll = float(fw['loss']) * math.log(2.0) * int(fw['sample_size'])
        sc = plain.score_captions(_clone(b))
        torch.cuda.synchronize()
    want_len = (b['caption']['roberta'][:, 1:] != PAD).sum(1)
    assert torch.equal(sc['prefix_len'], want_len) and int(want_len.sum()) == int(fw['sample_size'])
    got = -float(sc['scores'].double().sum())
    print('\nscore_captions bf16: summed NLL %.4f, criterion %.4f, relative %.3e' % (got, nll, abs(got - nll) / nll))
    assert abs(got - nll) <= 3e-2 * abs(nll), (got, nll)
    assert bool((sc['log_probs'] <= 0).all()) and torch.allclose(sc['log_probs'].sum(1), sc['scores'])
    assert bool((sc['log_probs'][torch.arange(8, device=DEV).unsqueeze(0) >= want_len.unsqueeze(1)] == 0).all())


# --------------------------------------------------------------------------- 4. the default is untouched
def test_prefix_none_changes_nothing_on_the_fused_path(fullsize):
    """Modelled on test_defaults_change_nothing_on_the_fused_path: prefix=None against a call without the argument - bitwise
    the same tensors, the same graph keys, the same sequence of entry points, the new one not among them; an all-pad prefix
    gives the same ids and log-probs through the prefixed graph."""
    plain, _, batches = fullsize
    b = batches[1]
    with torch.no_grad():
        for K in (4, 1):
            plain.generate(**_clone(b), beam_size=K)                  # (working weights cached first)
            plain.reset_graphs()
            with _Spy() as sa:
                a = plain.generate(**_clone(b), beam_size=K)
            keys_a = list(plain.__dict__['_decode_graphs'])
            plain.reset_graphs()
            with _Spy() as sk:
                k_ = plain.generate(**_clone(b), beam_size=K, prefix=None)
            torch.cuda.synchronize()
            assert torch.equal(a['gen_ids'], k_['gen_ids']) and torch.equal(a['log_probs'], k_['log_probs'])
            assert torch.equal(a['scores'], k_['scores']) and 'prefix_len' not in k_
            assert list(plain.__dict__['_decode_graphs']) == keys_a
            assert not any(('prefix',) in s_ for s_ in keys_a)
            assert sa.names == sk.names and len(sa.names) > 100
            assert 'tell_adaptive_logprob_forced' not in sk.names
            with _Spy() as sp:
                p_ = plain.generate(**_clone(b), beam_size=K, prefix=torch.full((4, 3), PAD, dtype=torch.long, device=DEV))
            torch.cuda.synchronize()
            assert torch.equal(a['gen_ids'], p_['gen_ids']) and torch.equal(a['log_probs'], p_['log_probs'])
            assert p_['prefix_len'].tolist() == [0] * 4 and 'tell_adaptive_logprob_forced' in sp.names
            assert any(('prefix',) in s_ for s_ in plain.__dict__['_decode_graphs'])
