"""Vocabulary masks on the MI355X: the three entry points against the plain definitions of
tests/test_vocab_mask_host.py (vocab_mask, greedy_masked / beam_search_masked), the fp32 generators against the prefix
re-decoding definition at full size, the fused captured bf16 path at the bench batch, and the defaults, which must change
nothing."""
import numpy as np
import pytest
import torch

from test_gpu_beam_options import C0, TAILS, _clone, _rows, _Spy
from test_gpu_penalties import _bits, _full_rows, _plain_topk, _small_args
from test_gpu_sampling import _expect
from test_vocab_mask_host import beam_search_masked, greedy_masked, mask_bools, outside, vocab_mask
from test_beam_options_host import repeats_ngram

pytestmark = pytest.mark.gpu
DEV = 'cuda'
V = C0 + sum(TAILS)
NEW = {'tell_decode_vocab_mask', 'tell_adaptive_logprob_topk_masked', 'tell_adaptive_logprob_sample_masked'}
EOS = 2


def _dev_bits(words):
    """uint32 words [R, W] (numpy) -> the int32 device tensor the entry points read."""
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(DEV)


def _pack(flags):
    """bool [R, V] -> uint32 [R, words] (the layout of vocab_mask)."""
    return np.stack([vocab_mask([], None, f, -1, f.shape[0]) for f in flags])


# --------------------------------------------------------------------------- 1. tell_decode_vocab_mask
@pytest.mark.parametrize('vocab', [69, 50265])
def test_builder_kernel_matches_vocab_mask(vocab):
    from tell_amd.hip import call
    rows, S, LD, pad = 5, 70, 73, 1
    rng = np.random.default_rng(vocab)
    ctx = rng.integers(0, vocab, (rows, LD))
    ctx[:, 5:9] = pad
    ctx[:, 10] = -4
    ctx[:, 11] = vocab
    ctx[:, 12] = vocab + 1000
    ctx[:, 13] = (1 << 33) + 7                               # (an id that only fits 64 bits)
    ctx[:, 20:24] = ctx[:, 30:34]                            # duplicates
    ctx[0, :S] = pad                                         # a row whose article is all padding
    ctx[:, S:] = np.arange(3)[None, :] + 3                   # behind S (inside the leading dimension): never read
    cls = rng.random(vocab) < 0.5
    cls[[EOS, 3, 4, 5]] = True                               # eos is in the class, and 3..5 (written behind S) stay absent
    ctx[:, :S][np.isin(ctx[:, :S], (3, 4, 5))] = 6
    deny_rows = rng.random((rows, vocab)) < 0.1
    deny_rows[:, EOS] = True                                 # ... and denied
    deny_rows[:, vocab - 1] = [True, False, True, False, True]
    d_ctx = torch.from_numpy(ctx).to(DEV)
    words = (vocab + 31) // 32
    ld_mask = words + 2
    cls_bits = _dev_bits(_pack(cls[None])[0])
    for deny in (None, deny_rows[:1], deny_rows):
        for use_cls in (True, False):
            mask = torch.full((rows, ld_mask), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
            d8 = None if deny is None else torch.from_numpy(deny.astype(np.uint8)).to(DEV)
            call('tell_decode_vocab_mask', d_ctx, d_ctx.stride(0), S, rows, vocab, cls_bits if use_cls else None, d8,
                 0 if deny is None or deny.shape[0] == 1 else d8.stride(0), EOS, pad, mask, mask.stride(0))
            got = mask.cpu().numpy().view(np.uint32)
            assert (got[:, words:] == 0x5A5A5A5A).all()      # nothing changes behind `words`
            for r in range(rows):
                want = vocab_mask(ctx[r, :S], cls if use_cls else None,
                                  None if deny is None else deny[r if deny.shape[0] > 1 else 0], EOS, vocab, pad)
                assert np.array_equal(got[r, :words], want), (vocab, r, use_cls)
                assert not (int(got[r, EOS >> 5]) >> EOS) & 1
    # S = 0: no article at all - the class is masked whole (without eos)
    mask = torch.zeros(rows, words, dtype=torch.int32, device=DEV)
    call('tell_decode_vocab_mask', None, 0, 0, rows, vocab, cls_bits, None, 0, EOS, pad, mask, mask.stride(0))
    assert np.array_equal(mask.cpu().numpy().view(np.uint32)[3], vocab_mask([], cls, None, EOS, vocab))
    # ops.vocab_mask is the same launch
    from tell_amd import ops
    out = ops.vocab_mask(d_ctx[:, :S], vocab, cls_bits, torch.from_numpy(deny_rows.astype(np.uint8)).to(DEV), EOS, pad)
    for r in range(rows):
        assert np.array_equal(out.cpu().numpy().view(np.uint32)[r], vocab_mask(ctx[r, :S], cls, deny_rows[r], EOS, vocab, pad))


# --------------------------------------------------------------------------- 2. tell_adaptive_logprob_topk_masked
N_ROWS, SEED = 12, 7
LAST = V - 1


def _args_with_a_strong_last_token():
    """_rows(12, 7) with the last vocabulary id made the best token of rows 5 and 6 (banned in one, allowed in the other)."""
    args = _rows(N_ROWS, SEED)
    head, last_tail = args[0], args[7]
    for r in (5, 6):
        head[r, C0 + 1] = 30.0                               # the second tail's cluster ...
        last_tail[r, TAILS[1] - 1] = 30.0                    # ... and its last token
    return args


def _exactly_64(rng, must):
    """bool [V], True = masked: everything but 64 tokens - eos, `must` and random others."""
    allowed = {EOS} | {int(t) for t in must}
    while len(allowed) < 64:
        allowed.add(int(rng.integers(0, V)))
    m = np.ones(V, dtype=bool)
    m[sorted(allowed)] = False
    return m


def _planted_masks(full, per, seed=3):
    """bool [N / per, V]: a 50 % random mask per mask row with the planted rows of the issue.  per = 1: one mask row per
    launch row; per = 4: three mask rows, planted from the first launch row of each group."""
    rng = np.random.default_rng(seed)
    N = full.shape[0]
    R = N // per
    m = rng.random((R, V)) < 0.5
    m[:, EOS] = False
    order = [np.lexsort((np.arange(V), -full[r])) for r in range(N)]
    tie = [17 + 97 * q for q in range(8)]

    def clusters(r):
        return [int(np.argmax(full[r, :C0])), C0 + int(np.argmax(full[r, C0:C0 + TAILS[0]])),
                C0 + TAILS[0] + int(np.argmax(full[r, C0 + TAILS[0]:]))]
    # mask row 0 (launch row 0): the eight-way tie straddles k - members 0 and 2 masked, the other six allowed
    m[0, tie] = False
    m[0, [tie[0], tie[2]]] = True
    if per == 1:
        m[1] = False                                         # an all-zero row beside masked rows
        m[2, order[2][:20]] = True                           # the whole top 20
        m[3, clusters(3)] = True                             # the best token of every cluster
        m[4] = _exactly_64(rng, order[4][:3])                # exactly 64 allowed tokens, the row's best three among them
        m[5, LAST], m[6, LAST] = True, False                 # the last vocabulary id: banned in one row, allowed in another
    else:
        m[1, order[4][:20]] = True
        m[1, clusters(5)] = True
        m[1, LAST] = True
        m[2] = _exactly_64(rng, list(order[8][:3]) + list(order[11][:2]))
    return m


def _masked_words(m):
    w = _pack(m)
    w[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(V & 31)   # garbage bits past `vocab` in the last word
    return w


def _mask_topk(args, N, k, bits, per, ban=None, n_ban=None):
    from tell_amd.hip import call
    tok = torch.full((N, k), -5, dtype=torch.int32, device=DEV)
    lps = torch.zeros(N, k, dtype=torch.float32, device=DEV)
    call('tell_adaptive_logprob_topk_masked', *args, N, k, bits, bits.stride(0), per, ban, ban.stride(0) if ban is not None else 0,
         n_ban, tok, lps)
    return tok.cpu().numpy(), lps.cpu().numpy()


@pytest.mark.parametrize('per', [1, 4])
@pytest.mark.parametrize('regs', [1, 0])
@pytest.mark.parametrize('k', [1, 4, 8])
def test_masked_topk_kernel(k, regs, per):
    from tell_amd import hip
    N = N_ROWS
    args = _args_with_a_strong_last_token()
    with hip.options(argmax_regs=regs):
        p_tok, p_lp = _plain_topk(args, N, k)
        zero = torch.zeros(N // per, (V + 31) // 32 + 1, dtype=torch.int32, device=DEV)      # (a leading dimension > words)
        garbage = torch.randint(0, V, (N, 64), dtype=torch.int32).to(DEV)
        # an all-zero mask without a list (NULL n_ban, NULL ban, all-zero n_ban): bitwise the plain kernel
        for ban, n_ban in ((None, None), (garbage, None), (garbage, torch.zeros(N, dtype=torch.int32, device=DEV))):
            t, l = _mask_topk(args, N, k, zero, per, ban, n_ban)
            assert np.array_equal(t, p_tok) and np.array_equal(_bits(l), _bits(p_lp))
        full = _full_rows(args, N, V)
        top8_tok, top8_lp = _plain_topk(args, N, 8)
        m = _planted_masks(full, per)
        assert per != 1 or int((~m[4]).sum()) == 64
        assert per != 4 or int((~m[2]).sum()) == 64
        bits = _dev_bits(_masked_words(m))
        t, l = _mask_topk(args, N, k, bits, per)

        def check(t, l, banned_rows):
            for r in range(N):
                masked = full[r].copy()
                masked[banned_rows[r]] = -np.inf
                want = np.lexsort((np.arange(V), -masked))[:k]
                assert np.array_equal(t[r], want), (r, t[r], want)
                for q in range(k):
                    hit = np.nonzero(top8_tok[r] == t[r, q])[0]
                    if hit.size:
                        assert _bits(l[r, q]) == _bits(top8_lp[r, hit[0]]), (r, q)
                    else:
                        assert abs(l[r, q] - full[r, t[r, q]]) <= 4e-6, (r, q)
        check(t, l, [m[r // per] for r in range(N)])
        # row 0: the unmasked members of the tie come first, in id order
        assert list(t[0][:min(k, 6)]) == [17 + 97 * q for q in (1, 3, 4, 5, 6, 7)][:k]
        if per == 1:
            assert np.array_equal(t[1], p_tok[1]) and np.array_equal(_bits(l[1]), _bits(p_lp[1]))     # the all-zero row
            assert p_tok[5, 0] == LAST and p_tok[6, 0] == LAST and t[6, 0] == LAST and LAST not in t[5]
            assert set(t[4].tolist()) <= set(np.nonzero(~m[4])[0].tolist())
            assert not set(t[2].tolist()) & set(np.lexsort((np.arange(V), -full[2]))[:20].tolist())
        # mask + ban list = the union; a mask-only launch with the same union gives bitwise the same output
        rng = np.random.default_rng(11)
        lists = []
        for r in range(N):
            allowed = np.lexsort((np.arange(V), -np.where(m[r // per], -np.inf, full[r])))
            b = [int(allowed[0]), int(allowed[2]), int(allowed[2])] + rng.integers(0, V, r).tolist() + [-1, V, V + 9]
            lists.append([] if r == 1 else b)
        ban = torch.randint(0, V, (N, 64), dtype=torch.int32)
        for r, b in enumerate(lists):
            ban[r, :len(b)] = torch.tensor(b, dtype=torch.int32)
        n_ban = torch.tensor([len(b) for b in lists], dtype=torch.int32, device=DEV)
        t2, l2 = _mask_topk(args, N, k, bits, per, ban.to(DEV), n_ban)
        union = []
        for r in range(N):
            u = m[r // per].copy()
            u[[x for x in lists[r] if 0 <= x < V]] = True
            union.append(u)
        check(t2, l2, union)
        assert any(t2[r, 0] != t[r, 0] for r in range(N))
        t3, l3 = _mask_topk(args, N, k, _dev_bits(_masked_words(np.stack(union))), 1)
        assert np.array_equal(t3, t2) and np.array_equal(_bits(l3), _bits(l2))
        # rows % per != 0 is an error, and nothing is launched
        with pytest.raises(RuntimeError, match='multiple of per'):
            _mask_topk(args, N, k, bits, 5)


# --------------------------------------------------------------------------- 3. small odd shapes, streaming form
def _mask_sample(args, N, k, inv_temp, seed, step, bits, per, step_dev=False, row_ids=None):
    from tell_amd.hip import call
    tok = torch.empty(N, dtype=torch.int32, device=DEV)
    lp = torch.empty(N, dtype=torch.float32, device=DEV)
    seed_dev = torch.tensor([seed], dtype=torch.int32, device=DEV)
    cnt = torch.tensor([step - 1], dtype=torch.int32, device=DEV) if step_dev else None
    call('tell_adaptive_logprob_sample_masked', *args, N, k, inv_temp, seed_dev, row_ids, 0 if step_dev else step, cnt,
         bits, bits.stride(0), per, tok, lp)
    return tok.cpu().numpy(), lp.cpu().numpy()


@pytest.mark.parametrize('c0,tails', [(37, (29, 3)), (33, ())])
def test_masked_kernels_small_odd_shapes_streaming(c0, tails):
    """The bitmap's last partial word (the last token of the vocabulary is masked in one row and allowed in another) and an
    empty tail set, streaming form.  Five tokens are masked per row: at vocab 69 that leaves exactly 64 allowed tokens; vocab
    33 cannot hold 64, there 28 stay, more than the largest k this test draws from (8) - a pick needs k allowed tokens, 64 is
    the host's limit for the sampler's largest k."""
    from tell_amd import hip
    N, vocab = 3, c0 + sum(tails)
    args = _small_args(c0, tails, N, seed=11)
    inv_temp = float(np.float32(1 / 0.9))
    with hip.options(argmax_regs=0):
        full = _full_rows(args, N, vocab)
        m = np.zeros((N, vocab), dtype=bool)
        rng = np.random.default_rng(2)
        for r in range(N):
            order = np.lexsort((np.arange(vocab), -full[r]))
            pick = [int(order[0]), int(order[3])] + ([vocab - 1] if r != 1 else [vocab - 2])
            for x in rng.permutation(vocab):
                if len(set(pick)) == 5:
                    break
                if int(x) != EOS and int(x) != vocab - 1:
                    pick.append(int(x))
            m[r, list(set(pick))] = True
            assert int(m[r].sum()) == 5
        assert vocab - int(m.sum(1).max()) >= min(64, vocab - 5)
        w = np.stack([vocab_mask([], None, f, -1, vocab) for f in m])
        w[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(vocab & 31)
        bits = _dev_bits(w)
        zero = torch.zeros_like(bits)
        masked = np.where(m, -np.inf, full).astype(np.float32)
        order = np.stack([np.lexsort((np.arange(vocab), -row)) for row in masked])
        for k in (1, 4, 8):
            p_tok, p_lp = _plain_topk(args, N, k)
            t, l = _mask_topk(args, N, k, zero, 1)
            assert np.array_equal(t, p_tok) and np.array_equal(_bits(l), _bits(p_lp))
            t, l = _mask_topk(args, N, k, bits, 1)
            for r in range(N):
                assert np.array_equal(t[r], order[r, :k]), (k, r, t[r], order[r, :k])
                assert np.abs(l[r] - full[r, order[r, :k]]).max() <= 4e-6, (k, r)
            # the sampler: k = 1 is the masked arg-max bit for bit; k > 1 draws tell_sample_pick's token from the masked k best
            a_tok, a_lp = _mask_topk(args, N, 1, bits, 1)
            s_tok, s_lp = _mask_sample(args, N, 1, inv_temp, 5, 3, bits, 1)
            assert np.array_equal(s_tok, a_tok[:, 0]) and np.array_equal(_bits(s_lp), _bits(a_lp[:, 0]))
            if k > 1:
                tok, lp = _mask_sample(args, N, k, inv_temp, 70 + k, 4, bits, 1)
                want_tok, want_lp, near = _expect(masked, order, k, inv_temp, 70 + k, np.arange(N), 4)
                bad = np.nonzero(tok != want_tok)[0]
                assert all(near[r] for r in bad), (k, bad)
                ok = tok == want_tok
                assert np.array_equal(_bits(lp[ok]), _bits(want_lp[ok])), k
                assert not m[np.arange(N), tok].any()


# --------------------------------------------------------------------------- 4. tell_adaptive_logprob_sample_masked
def test_masked_sampler_kernel():
    from tell_amd import hip
    from tell_amd.hip import call
    N = N_ROWS
    args = _args_with_a_strong_last_token()
    inv_temp = float(np.float32(1 / 0.9))
    got = {}
    for regs in (1, 0):
        with hip.options(argmax_regs=regs):
            full = _full_rows(args, N, V)
            for per in (1, 4):
                m = _planted_masks(full, per)
                bits = _dev_bits(_masked_words(m))
                rows_m = np.stack([m[r // per] for r in range(N)])
                # k = 1: the masked arg-max, bit for bit
                a_tok, a_lp = _mask_topk(args, N, 1, bits, per)
                s_tok, s_lp = _mask_sample(args, N, 1, inv_temp, 5, 3, bits, per)
                assert np.array_equal(s_tok, a_tok[:, 0]) and np.array_equal(_bits(s_lp), _bits(a_lp[:, 0])), (regs, per)
                masked = np.where(rows_m, -np.inf, full).astype(np.float32)
                order = np.stack([np.lexsort((np.arange(V), -row))[:64] for row in masked])
                # row_ids (the rows the random numbers are keyed on) with per = 4: the mask row stays launch row // per
                row_ids = torch.tensor([(5 * r + 3) % 97 for r in range(N)], dtype=torch.int32, device=DEV) if per == 4 else None
                keyed = np.arange(N) if row_ids is None else row_ids.cpu().numpy()
                for k in (8, 64):
                    seed, step = 100 + k, 7
                    tok, lp = _mask_sample(args, N, k, inv_temp, seed, step, bits, per, row_ids=row_ids)
                    got[(regs, per, k)] = tok
                    assert not rows_m[np.arange(N), tok].any(), (regs, per, k)       # never a masked token
                    for r in range(N):
                        assert tok[r] in order[r, :k], (regs, per, k, r)
                    want_tok, want_lp, near = _expect(masked, order, k, inv_temp, seed, keyed, step)
                    bad = np.nonzero(tok != want_tok)[0]
                    assert all(near[r] for r in bad), (regs, per, k, bad)            # (only a u on a CDF edge may fall the other way)
                    assert len(bad) <= 1
                    ok = tok == want_tok
                    if regs:
                        np.testing.assert_allclose(lp[ok], want_lp[ok], rtol=0, atol=4e-6)
                    else:                                                            # the streaming form has the full-row kernel's arithmetic
                        assert np.array_equal(_bits(lp[ok]), _bits(want_lp[ok])), k
                    # host step and device step: bitwise the same
                    tok_d, lp_d = _mask_sample(args, N, k, inv_temp, seed, step, bits, per, step_dev=True, row_ids=row_ids)
                    assert np.array_equal(tok_d, tok) and np.array_equal(_bits(lp_d), _bits(lp))
                    # eager and hipGraph replay: bitwise the same
                    o_tok = torch.empty(N, dtype=torch.int32, device=DEV)
                    o_lp = torch.empty(N, dtype=torch.float32, device=DEV)
                    seed_dev = torch.tensor([seed], dtype=torch.int32, device=DEV)
                    cnt = torch.tensor([step - 1], dtype=torch.int32, device=DEV)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        call('tell_adaptive_logprob_sample_masked', *args, N, k, inv_temp, seed_dev, row_ids, 0, cnt, bits,
                             bits.stride(0), per, o_tok, o_lp)
                    g.replay()
                    torch.cuda.synchronize()
                    assert np.array_equal(o_tok.cpu().numpy(), tok) and np.array_equal(_bits(o_lp.cpu().numpy()), _bits(lp))
                # an all-zero mask is the plain sampler, bitwise
                zero = torch.zeros_like(bits)
                tok, lp = _mask_sample(args, N, 8, inv_temp, 9, 2, zero, per)
                p_tok = torch.empty(N, dtype=torch.int32, device=DEV)
                p_lp = torch.empty(N, dtype=torch.float32, device=DEV)
                call('tell_adaptive_logprob_sample', *args, N, 8, inv_temp, torch.tensor([9], dtype=torch.int32, device=DEV), None,
                     2, None, p_tok, p_lp)
                assert np.array_equal(tok, p_tok.cpu().numpy()) and np.array_equal(_bits(lp), _bits(p_lp.cpu().numpy()))
                with pytest.raises(RuntimeError, match='multiple of per'):
                    _mask_sample(args, N, 8, inv_temp, 9, 2, bits, 5)
    for per in (1, 4):                                                               # the register and streaming forms agree
        for k in (8, 64):
            assert np.array_equal(got[(1, per, k)], got[(0, per, k)]), (per, k)


def test_masked_sampler_never_draws_a_masked_token():
    """4 096 draws, k = 64, over the row with exactly 64 allowed tokens (one logit row under 4 096 workgroups: leading
    dimension 0; one mask row for all of them: per = 4 096): every allowed token is a candidate, no masked one is drawn."""
    R, k = 4096, 64
    args = list(_rows(N_ROWS, SEED))
    full = _full_rows(args, N_ROWS, V)
    m = _planted_masks(full, 1)[4]
    assert int((~m).sum()) == 64
    one = [a[4:5].contiguous() if torch.is_tensor(a) else a for a in args]
    for i in (1, 5, 8):                                                              # every row pointer stays on the one row
        one[i] = 0
    bits = _dev_bits(_masked_words(m[None]))
    tok, lp = _mask_sample(one, R, k, float(np.float32(1 / 1.5)), 4242, 3, bits, R)
    assert not m[tok].any()
    assert len(set(tok.tolist())) >= 2                                               # (a draw, not an arg-max: the row's three best
                                                                                     #  tokens are allowed and T = 1.5 keeps them close)
    np.testing.assert_allclose(lp, full[4][tok], rtol=0, atol=4e-6)


# --------------------------------------------------------------------------- 5. fp32, full-size decoder
FP32_GEN, FP32_EOS_FACTOR, FP32_SEED, ART = 12, 14.0, 43, 16


def test_full_size_generators_under_a_grounded_mask_match_the_definition_fp32():
    """Setup of test_full_size_generators_with_penalties_match_the_definition_fp32 at B = 4: the cached fp32 generators (the
    layer-by-layer path, through the same head) with a random half of the vocabulary as the grounded class and articles of 16
    ids, greedy, beam 4 and beam 4 with no_repeat_ngram_size = 2, against greedy_masked / beam_search_masked - identical ids,
    scores within section 16's rtol 1e-4 / atol 5e-4."""
    import tell_amd
    from oracle.build import build_decoder as obuild
    from tell_amd import ops
    from tell_amd.build import build_decoder
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
    rng = np.random.default_rng(5)
    cls = rng.random(V) < 0.5
    art = rng.integers(4, V, (BB, ART))
    art[:, -1] = 1
    masks = np.stack([mask_bools(vocab_mask(art[b], cls, None, EOS, V), V) for b in range(BB)])
    vm = (torch.from_numpy(art).to(DEV), ops.pack_mask_bits(torch.from_numpy(cls)).to(DEV), None)

    def same(got, want):
        got = got.cpu()
        n = min(got.shape[-1], want.shape[-1])
        assert torch.equal(got[..., :n], want[..., :n]), (got, want)
        assert (got[..., n:] == 1).all() and (want[..., n:] == 1).all()
    with torch.no_grad():
        _, plain_ids, _ = m._generate_cached(start.to(DEV), dctx, gen_len=GEN, eos=2)
        assert outside(plain_ids.cpu().numpy(), cls, art) > 0            # non-vacuity: the free decode leaves the articles
        want_ids, want_sc = greedy_masked(om, start, c(), masks, gen_len=GEN)
        with _Spy() as spy:
            lp, got, _ = m._generate_cached(start.to(DEV), dctx, gen_len=GEN, eos=2, vmask=vm)
        assert {'tell_decode_vocab_mask', 'tell_adaptive_logprob_topk_masked'} <= set(spy.names)
        assert spy.names.count('tell_decode_vocab_mask') == 1
        same(got, want_ids)
        assert outside(got.cpu().numpy(), cls, art) == 0
        print('\nfp32 greedy: scores %s vs definition %s' % (lp.sum(1).cpu().tolist(), want_sc.tolist()))
        assert torch.allclose(lp.sum(1).cpu(), want_sc, rtol=1e-4, atol=5e-4)
        for n in (0, 2):
            want_b, want_sc = beam_search_masked(om, start, c(), 4, masks, gen_len=GEN, ngram=n)
            m.no_repeat_ngram_size = n
            with _Spy() as spy:
                lp, got, info = m._generate_beam(start.to(DEV), dctx, 4, gen_len=GEN, eos=2, n_best=4, vmask=vm)
            m.no_repeat_ngram_size = 0
            assert 'tell_adaptive_logprob_topk_masked' in spy.names and ('tell_decode_ban_list' in spy.names) == bool(n)
            assert 'tell_adaptive_logprob_topk_banned' not in spy.names
            ids_n, lps_n, sc_n = info.nbest
            print('fp32 beam 4 (ngram %d): scores %s vs definition %s' % (n, sc_n.cpu().tolist(), want_sc.tolist()))
            same(ids_n, want_b)
            same(got, want_b[:, 0])
            assert torch.allclose(sc_n.cpu(), want_sc, rtol=1e-4, atol=5e-4), (sc_n, want_sc)
            assert outside(ids_n.cpu().numpy(), cls, art) == 0
            if n:
                assert not any(repeats_ngram(h, n) for b in ids_n.cpu() for h in b)


# --------------------------------------------------------------------------- 6. bf16, the fused captured path
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
    cls = torch.from_numpy(np.random.default_rng(9).random(V) < 0.5)
    yield plain, batches, cls
    tell_amd.set_compute_dtype(torch.float32)


def _mask_graphs(model):
    return [h for sig, h in model.__dict__['_decode_graphs'].items() if ('mask',) in sig]


def _articles_of(b):
    return b['context']['roberta'].cpu().numpy()


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
        hs = _mask_graphs(model)
        assert hs and all(h['graph'] is False for h in hs)              # every step of this run was issued eagerly
    finally:
        stepper_mod.graphs = keep
        model.__dict__.pop('_decode_graphs', None)
    return out, spy


@pytest.mark.parametrize('mode', ['greedy', 'beam4', 'topk8_n4'])
def test_fused_bf16_path_under_a_grounded_mask_at_the_bench_batch(fullsize, mode):
    plain, batches, cls = fullsize
    b = batches[0]
    art = _articles_of(b)
    cls_np = cls.numpy()
    kw = {'greedy': {}, 'beam4': dict(beam_size=4, n_best=4), 'topk8_n4': dict(n_samples=4)}[mode]
    keys = ('gen_ids', 'log_probs', 'scores') + {'greedy': (), 'beam4': ('gen_ids_nbest', 'log_probs_nbest', 'scores_nbest'),
                                                 'topk8_n4': ('gen_ids_samples', 'log_probs_samples', 'sample_index')}[mode]
    every = {'greedy': 'gen_ids', 'beam4': 'gen_ids_nbest', 'topk8_n4': 'gen_ids_samples'}[mode]
    keep = (plain.sampling_topk, plain.sampling_temp)
    if mode == 'topk8_n4':
        plain.sampling_topk, plain.sampling_temp = 8, 0.9
    try:
        with torch.no_grad():
            torch.manual_seed(5)
            free = plain.generate(**_clone(b), **kw)
            torch.manual_seed(5)
            out = plain.generate(**_clone(b), **kw, ground=cls)
            torch.cuda.synchronize()
            hs = _mask_graphs(plain)
            assert hs and all(h['graph'] not in (None, False) for h in hs), [h.get('error') for h in hs]
            assert any(h.get(('multi', 8)) for h in hs), [h.get('multi_error') for h in hs]

            def run():
                torch.manual_seed(5)
                return plain.generate(**_clone(b), **kw, ground=cls)
            eager, spy = _eager(plain, run)
    finally:
        plain.sampling_topk, plain.sampling_temp = keep
    pick = 'tell_adaptive_logprob_sample_masked' if mode == 'topk8_n4' else 'tell_adaptive_logprob_topk_masked'
    assert pick in spy.names and spy.names.count('tell_decode_vocab_mask') == 1
    assert not (NEW - {pick, 'tell_decode_vocab_mask'}) & set(spy.names)
    for key in keys:                                                    # captured and launch by launch: bitwise
        assert torch.equal(eager[key], out[key]), (mode, key)
    n_free, n_out = outside(free[every].cpu().numpy(), cls_np, art), outside(out[every].cpu().numpy(), cls_np, art)
    print('\nbf16 B=32 %s: class tokens outside the row\'s article: %d unconstrained, %d grounded; %d steps'
          % (mode, n_free, n_out, out['gen_ids'].shape[1] - 1))
    assert n_free > 0 and n_out == 0
    if mode != 'greedy':
        return
    # nothing is renormalised: the reported log-probs are the model's own teacher-forced log-probs of the generated captions
    with torch.no_grad():
        bb = _clone(b)
        bb['caption'] = dict(bb['caption'])
        bb['caption'][plain.index] = out['gen_ids'].clone()
        sc = plain.score_captions(bb)
        torch.cuda.synchronize()
    lp, got, ids = sc['log_probs'].cpu().numpy(), out['log_probs'].cpu().numpy(), out['gen_ids'].cpu().numpy()
    live = ids[:, 1:] != 1
    n = min(lp.shape[1], got.shape[1])
    n_bits = int((_bits(got[:, :n])[live[:, :n]] != _bits(lp[:, :n])[live[:, :n]]).sum())
    print('bf16 B=32 greedy: %d of %d reported log-probs differ in bits from score_captions' % (n_bits, int(live.sum())))
    assert n_bits == 0 and not live[:, n:].any()


def test_a_forced_prefix_wins_over_the_mask_and_a_second_batch_refills_it(fullsize):
    plain, batches, cls = fullsize
    b, b2 = batches[0], batches[1]
    art, art2 = _articles_of(b), _articles_of(b2)
    cls_np = cls.numpy()
    B = art.shape[0]
    # a prefix of two tokens per row: a class token that is NOT in the row's article (masked), then a free token
    gone = [int(np.nonzero(cls_np & ~np.isin(np.arange(V), art[r]))[0][10 + r]) for r in range(B)]
    prefix = torch.tensor([[g, 4 + r] for r, g in enumerate(gone)], dtype=torch.long)
    prefix[3:6] = 1                                                     # some rows decode freely
    with torch.no_grad():
        base = plain.generate(**_clone(b), prefix=prefix)
        out = plain.generate(**_clone(b), prefix=prefix, ground=cls)
        torch.cuda.synchronize()
        forced = prefix != 1
        assert torch.equal(out['gen_ids'][:, 1:3].cpu()[forced], prefix[forced])       # the prefix is emitted ...
        live = forced[:, 0]                                                            # ... and scored as without the mask
        assert bool(live.any()) and not bool(live.all())
        assert torch.equal(out['log_probs'][:, :2].cpu()[live], base['log_probs'][:, :2].cpu()[live])
        ids = out['gen_ids'].cpu().numpy().copy()
        ids[:, 1:3][forced.numpy()] = 1                                 # (the forced tokens aside) nothing leaves the articles
        assert outside(ids, cls_np, art) == 0
        # a second batch through the same cache entry: its own articles, no recapture
        plain.reset_graphs()
        one = plain.generate(**_clone(b), ground=cls)
        hs = _mask_graphs(plain)
        assert len(hs) == 1
        graph = hs[0]['graph']
        two = plain.generate(**_clone(b2), ground=cls)
        torch.cuda.synchronize()
        hs = _mask_graphs(plain)
        assert len(hs) == 1 and hs[0]['graph'] is graph
        assert outside(one['gen_ids'].cpu().numpy(), cls_np, art) == 0
        assert outside(two['gen_ids'].cpu().numpy(), cls_np, art2) == 0
        held = hs[0]['vmask'].cpu().numpy().view(np.uint32)             # the entry's bitmap now is batch 2's, exactly
        for r in range(B):
            assert np.array_equal(held[r], vocab_mask(art2[r], cls_np, None, EOS, V)), r
        assert not np.array_equal(held[0], vocab_mask(art[0], cls_np, None, EOS, V))
        # banned (per row) and suppress_tokens join: none of them appears
        banned = torch.zeros(B, V, dtype=torch.bool)
        first = one['gen_ids'][:, 1].cpu()
        banned[torch.arange(B), first] = first != EOS
        plain.suppress_tokens = (int(one['gen_ids'][0, 2]),) if int(one['gen_ids'][0, 2]) not in (1, EOS) else (5,)
        try:
            three = plain.generate(**_clone(b), ground=cls, banned=banned)
        finally:
            plain.suppress_tokens = ()
        got = three['gen_ids'].cpu()
        sup = int(one['gen_ids'][0, 2]) if int(one['gen_ids'][0, 2]) not in (1, EOS) else 5
        assert sup not in got[:, 1:].reshape(-1).tolist()
        for r in range(B):
            if int(first[r]) != EOS:
                assert int(first[r]) not in got[r, 1:].tolist(), r
        assert outside(got.numpy(), cls_np, art) == 0


# --------------------------------------------------------------------------- 7. the defaults change nothing
def test_defaults_change_nothing_on_the_fused_path(fullsize):
    """A model built with the keys at their defaults and called with banned=None, ground=None against one built and called
    without them: the same ids, the same graph keys, and - warm steps, captures and bookkeeping - the same sequence of entry
    points, none of them new."""
    from tell_amd.build import build_model
    plain, batches, _ = fullsize
    keyed = build_model('faces_objects', resnet=plain.resnet, roberta=plain.roberta, suppress_tokens=(), ground_names=False)
    keyed.load_state_dict(plain.state_dict())
    keyed.to(DEV).eval()
    b = batches[2]
    with torch.no_grad():
        for K in (4, 1):
            plain.generate(**_clone(b), beam_size=K)                  # (working weights cached on both sides first)
            keyed.generate(**_clone(b), beam_size=K)
            plain.reset_graphs()
            keyed.reset_graphs()
            with _Spy() as sa:
                a = plain.generate(**_clone(b), beam_size=K)
            with _Spy() as sk:
                k_ = keyed.generate(**_clone(b), beam_size=K, banned=None, ground=None)
            torch.cuda.synchronize()
            assert torch.equal(a['gen_ids'], k_['gen_ids']) and torch.equal(a['log_probs'], k_['log_probs'])
            assert torch.equal(a['scores'], k_['scores'])
            pk = [s_[:5] + s_[6:] for s_ in plain.__dict__['_decode_graphs']]     # (all but the position table's address)
            kk = [s_[:5] + s_[6:] for s_ in keyed.__dict__['_decode_graphs']]
            assert pk == kk and not any(('mask',) in s_ for s_ in kk)
            assert all(h['graph'] not in (None, False) for h in keyed.__dict__['_decode_graphs'].values())
            assert all('vmask' not in h for h in keyed.__dict__['_decode_graphs'].values())
            assert sa.names == sk.names and len(sa.names) > 100
            assert not NEW & set(sk.names)
            assert ('tell_beam_update' if K > 1 else 'tell_greedy_update') in sk.names
