"""Repetition, presence and frequency penalties on the MI355X: the three entry points against the plain
definitions of tests/test_penalties_host.py (token_counts, sub_table, penalised, greedy_pen / beam_search_pen), the fp32
generators against the prefix-re-decoding definition at full size, the fused captured bf16 path at the bench batch, and the
defaults, which must change nothing."""
import numpy as np
import pytest
import torch

from test_gpu_beam_options import C0, TAILS, _clone, _rows, _Spy
from test_gpu_sampling import _expect
from test_penalties_host import beam_search_pen, greedy_pen, penalised, repeats, sub_table, token_counts

pytestmark = pytest.mark.gpu
DEV = 'cuda'
THETA, ALPHA, BETA = 1.3, 0.5, 0.25
NEW = {'tell_decode_token_counts', 'tell_adaptive_logprob_topk_penalised', 'tell_adaptive_logprob_sample_penalised'}


# --------------------------------------------------------------------------- 1. tell_decode_token_counts
def _counts(d_hist, L, d_fin, step, dev_form, ld):
    from tell_amd.hip import call
    rows = d_hist.shape[0]
    tok = torch.full((rows, ld), -1, dtype=torch.int32, device=DEV)
    cnt = torch.full((rows, ld), -1, dtype=torch.int32, device=DEV)
    n_pen = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    sd = torch.tensor([step - 1], dtype=torch.int32, device=DEV) if dev_form else None
    call('tell_decode_token_counts', d_hist, d_hist.stride(0), L, d_fin, rows, 12345 if dev_form else step, sd, tok, cnt,
         tok.stride(0), n_pen)
    return tok.cpu().numpy(), cnt.cpu().numpy(), n_pen.cpu().numpy()


def _check_counts(hist, fin, L, steps, ld):
    rows = hist.shape[0]
    d_hist = torch.full((rows, L + 3), -7, dtype=torch.long)          # (a leading dimension wider than L)
    d_hist[:, :L] = hist
    d_hist, d_fin = d_hist.to(DEV), fin.to(DEV)
    for step in steps:
        got = [_counts(d_hist, L, d_fin, step, dev_form, ld) for dev_form in (False, True)]
        for tok, cnt, n_pen in got:
            for r in range(rows):
                want = ([], []) if fin[r] else token_counts(hist[r].tolist(), step)
                n = int(n_pen[r])
                assert n == len(want[0]), (step, r)
                assert tok[r, :n].tolist() == want[0] and cnt[r, :n].tolist() == want[1], (step, r)   # order and counts: exact
                assert (tok[r, n:] == -1).all() and (cnt[r, n:] == -1).all()                          # nothing behind the list
        for a, b in zip(got[0], got[1]):
            assert np.array_equal(a, b)                               # `step` and `step_dev` forms agree


def test_token_counts_kernel_matches_token_counts():
    rows, L = 37, 40
    g = torch.Generator().manual_seed(5)
    hist = torch.randint(3, 8, (rows, L), generator=g)               # a five-token alphabet: every token repeats often
    hist[:, 0] = 0
    hist[3, 1:] = torch.arange(100, 100 + L - 1)                      # a row without any repeat
    hist[4, :] = 9                                                    # one token over and over
    fin = torch.zeros(rows, dtype=torch.uint8)
    fin[[1, 8, 20]] = 1
    _check_counts(hist, fin, L, (0, 1, 2, 7, L - 1), L + 5)


def test_token_counts_kernel_at_the_longest_history():
    L = 256
    hist = torch.stack([torch.arange(1000, 1000 + L), torch.full((L,), 77)])
    _check_counts(hist, torch.zeros(2, dtype=torch.uint8), L, (L - 1, 63, 64), L)


# --------------------------------------------------------------------------- 2. tell_adaptive_logprob_topk_penalised
N_ROWS, SEED = 12, 7
V = C0 + sum(TAILS)


class _Lists:
    """Device form of per-row (tokens, counts) lists, with garbage behind every list."""

    def __init__(self, lists, vocab, ld=256, seed=1):
        N = len(lists)
        g = torch.Generator().manual_seed(seed)
        tok = torch.randint(0, vocab, (N, ld), generator=g, dtype=torch.int32)
        cnt = torch.randint(1, 6, (N, ld), generator=g, dtype=torch.int32)
        for r, (t, c) in enumerate(lists):
            assert len(set(t)) == len(t) and len(t) <= ld
            tok[r, :len(t)] = torch.tensor(t, dtype=torch.int32)
            cnt[r, :len(c)] = torch.tensor(c, dtype=torch.int32)
        self.tok, self.cnt = tok.to(DEV), cnt.to(DEV)
        self.n_pen = torch.tensor([len(t) for t, _ in lists], dtype=torch.int32, device=DEV)
        self.zero = torch.zeros(N, dtype=torch.int32, device=DEV)

    def args(self, theta, sub, empty=False):
        return [self.tok, self.cnt, self.tok.stride(0), self.zero if empty else self.n_pen, float(theta), sub, sub.numel()]


def _cpu_logprobs64(args):
    """The adaptive softmax's log-probs of _rows-style arguments in float64 on the CPU: [N, vocab]."""
    head, _, c0, n_tails = args[:4]
    h = head.cpu().double()[:, :c0 + n_tails]
    hl = torch.log_softmax(h, -1)
    out = [hl[:, :c0]]
    for c in range(n_tails):
        t, _, n = args[4 + 3 * c:7 + 3 * c]
        out.append(torch.log_softmax(t.cpu().double()[:, :n], -1) + hl[:, c0 + c:c0 + c + 1])
    return torch.cat(out, 1).numpy()


def _make_lists(lp64, seed=3):
    """Per row a list that holds, in some combination: the arg-max, the best token of every cluster, counts 1..5, some of row
    0's tied tokens, r random tokens, 255 entries in one row, and nothing in another."""
    rng = np.random.default_rng(seed)
    N, vocab = lp64.shape
    lists = []
    for r in range(N):
        order = np.lexsort((np.arange(vocab), -lp64[r]))
        t = [int(order[0])]
        if vocab == V:
            t += [int(np.argmax(lp64[r, :C0])), C0 + int(np.argmax(lp64[r, C0:C0 + TAILS[0]])),
                  C0 + TAILS[0] + int(np.argmax(lp64[r, C0 + TAILS[0]:]))]
        t += [int(order[2])] + rng.integers(0, vocab, r).tolist()
        if r == 0 and vocab == V:
            t = [17, 17 + 2 * 97, 17 + 5 * 97, int(order[9])]       # members 0, 2 and 5 of the eight-way tie, and a follower
        if r == 1:
            t = []
        if r == 2 and vocab >= 255:
            t = [int(x) for x in order[:20]] + rng.integers(0, vocab, 400).tolist()
        t = list(dict.fromkeys(t))[:255]                             # (a token is listed once)
        if r == 2 and vocab >= 255:
            assert len(t) == 255
        lists.append((t, [1 + (q + r) % 5 for q in range(len(t))]))
    return lists


def _restate64(lp64_row, counts, theta, sub):
    s = lp64_row.copy()
    for t, c in zip(*counts):
        s[t] = min(s[t], 0.0) * np.float64(np.float32(theta)) - np.float64(sub[c])
    return s


def _close_scores(s64, k, theta):
    """Whether two DIFFERENT scores among the row's top k + 1 lie closer than 8e-6 * theta (forms that differ by sub-ulp
    amounts may then order them differently).  Equal scores stay: they come from equal logits with equal list entries, and
    every form breaks that tie by id."""
    top = np.sort(s64)[::-1][:k + 1]
    gaps = top[:-1] - top[1:]
    return bool(((gaps > 0) & (gaps < 8e-6 * theta)).any())


def test_seed_gives_no_close_scores_on_the_cpu():
    """The seed of test 2 is chosen so that the fp64 restatement on the CPU alone skips no row (checked before the GPU runs:
    this test sorts first in the file's penalised top-k section)."""
    args = _rows(N_ROWS, SEED)
    lp64 = _cpu_logprobs64(args)
    lists = _make_lists(lp64)
    sub = sub_table(ALPHA, BETA, 256)
    for r in range(N_ROWS):
        s64 = _restate64(lp64[r], lists[r], THETA, sub)
        assert not _close_scores(s64, 8, THETA), r
        assert not _close_scores(s64, 64, THETA), r              # (the sampler's k)


def _full_rows(args, N, vocab):
    from tell_amd.hip import call
    full = torch.empty(N, vocab, dtype=torch.float32, device=DEV)
    call('tell_adaptive_logprob_argmax', *args, N, full, vocab, torch.empty(N, dtype=torch.int32, device=DEV),
         torch.empty(N, dtype=torch.float32, device=DEV))
    return full.cpu().numpy()


def _plain_topk(args, N, k):
    from tell_amd.hip import call
    tok = torch.empty(N, k, dtype=torch.int32, device=DEV)
    lps = torch.empty(N, k, dtype=torch.float32, device=DEV)
    call('tell_adaptive_logprob_topk', *args, N, k, tok, lps)
    return tok.cpu().numpy(), lps.cpu().numpy()


def _pen_topk(args, N, k, pen_args):
    from tell_amd.hip import call
    tok = torch.full((N, k), -5, dtype=torch.int32, device=DEV)
    lps = torch.zeros(N, k, dtype=torch.float32, device=DEV)
    call('tell_adaptive_logprob_topk_penalised', *args, N, k, *pen_args, tok, lps)
    return tok.cpu().numpy(), lps.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize('regs', [1, 0])
@pytest.mark.parametrize('k', [1, 4, 8])
def test_penalised_topk_kernel(k, regs):
    from tell_amd import hip
    N = N_ROWS
    args = _rows(N, SEED)
    lp64 = _cpu_logprobs64(args)
    lists = _make_lists(lp64)
    sub_np = sub_table(ALPHA, BETA, 256)
    sub = torch.from_numpy(sub_np).to(DEV)
    L = _Lists(lists, V)
    with hip.options(argmax_regs=regs):
        p_tok, p_lp = _plain_topk(args, N, k)
        # n_pen = 0: bitwise the plain kernel (garbage in the list arrays must not matter)
        t, l = _pen_topk(args, N, k, L.args(THETA, sub, empty=True))
        assert np.array_equal(t, p_tok) and np.array_equal(_bits(l), _bits(p_lp))
        # a non-empty list with theta = 1 and sub = 0: bitwise the same
        t, l = _pen_topk(args, N, k, L.args(1.0, torch.zeros_like(sub)))
        assert np.array_equal(t, p_tok) and np.array_equal(_bits(l), _bits(p_lp))
        full = _full_rows(args, N, V)
        assert bool((full <= 0).all())
        top8_tok, top8_lp = _plain_topk(args, N, 8)
        t, l = _pen_topk(args, N, k, L.args(THETA, sub))
    skipped = []
    f = np.float32
    for r in range(N):
        if _close_scores(_restate64(lp64[r], lists[r], THETA, sub_np), k, THETA):
            skipped.append(r)
            continue
        s = penalised(full[r], lists[r], THETA, sub_np)
        want = np.lexsort((np.arange(V), -s))[:k]
        assert np.array_equal(t[r], want), (r, t[r], want)
        cnt_of = dict(zip(*lists[r]))
        for q in range(k):
            tok = int(t[r, q])
            hit = np.nonzero(top8_tok[r] == tok)[0]
            if tok in cnt_of and hit.size:
                lp = top8_lp[r, hit[0]]
                exp = f(f(np.minimum(lp, f(0.0)) * f(THETA)) - sub_np[cnt_of[tok]])
                assert _bits(l[r, q]) == _bits(exp), (r, q, l[r, q], exp)
            elif hit.size:
                assert _bits(l[r, q]) == _bits(top8_lp[r, hit[0]]), (r, q)
            else:
                assert abs(float(l[r, q]) - float(s[tok])) <= 4e-6 * THETA, (r, q, l[r, q], s[tok])
    assert len(skipped) <= 1, skipped
    assert 0 not in skipped and 1 not in skipped
    assert np.array_equal(t[1], p_tok[1]) and np.array_equal(_bits(l[1]), _bits(p_lp[1]))       # the row without a list
    # row 0: the unpenalised members of the eight-way tie come first, in id order
    assert list(t[0][:min(k, 5)]) == [17 + 97 * m for m in (1, 3, 4, 6, 7)][:k]
    # the penalties moved the lists: most rows with a list lose their arg-max to another token
    assert sum(t[r, 0] != p_tok[r, 0] for r in range(2, N)) >= (N - 2) // 2


def _small_args(c0, tails, N, seed):
    g = torch.Generator().manual_seed(seed)

    def buf(n, scale):
        ld = -(-n // 4) * 4
        return (torch.randn(N, ld, generator=g) * scale).to(DEV), ld
    head, ld_h = buf(c0 + len(tails), 3.0)
    args = [head, ld_h, c0, len(tails)]
    for n in tails:
        t, ld = buf(n, 2.0)
        args += [t, ld, n]
    return args + [None, 0, 0] * (3 - len(tails))


@pytest.mark.parametrize('c0,tails', [(37, (29, 3)), (33, ())])
def test_penalised_topk_small_odd_shapes_streaming(c0, tails):
    """The bitmap's last partial word (the last token of the vocabulary is listed) and an empty tail set, streaming form."""
    from tell_amd import hip
    N, vocab = 3, c0 + sum(tails)
    args = _small_args(c0, tails, N, seed=11)
    lp64 = _cpu_logprobs64(args)
    lists = _make_lists(lp64)
    first = list(dict.fromkeys([vocab - 1, int(np.argmax(lp64[0])), 0]))
    lists[0] = (first, [2, 1, 5][:len(first)])
    lists[2] = ([int(x) for x in np.argsort(-lp64[2])[:vocab - 2]], [1 + q % 5 for q in range(vocab - 2)])   # nearly the whole row
    sub_np = sub_table(ALPHA, BETA, 40)
    sub = torch.from_numpy(sub_np).to(DEV)
    L = _Lists(lists, vocab, ld=vocab)
    with hip.options(argmax_regs=0):
        full = _full_rows(args, N, vocab)
        for k in (1, 4, 8):
            p_tok, p_lp = _plain_topk(args, N, k)
            t, l = _pen_topk(args, N, k, L.args(THETA, sub, empty=True))
            assert np.array_equal(t, p_tok) and np.array_equal(_bits(l), _bits(p_lp))
            t, l = _pen_topk(args, N, k, L.args(THETA, sub))
            for r in range(N):
                assert not _close_scores(_restate64(lp64[r], lists[r], THETA, sub_np), k, THETA), (r, k)
                s = penalised(full[r], lists[r], THETA, sub_np)
                want = np.lexsort((np.arange(vocab), -s))[:k]
                assert np.array_equal(t[r], want), (k, r, t[r], want)
                assert np.abs(l[r] - s[want]).max() <= 4e-6 * THETA, (k, r)


# --------------------------------------------------------------------------- 3. tell_adaptive_logprob_sample_penalised
def _pen_sample(args, N, k, inv_temp, seed, step, pen_args, step_dev=False, out=None):
    from tell_amd.hip import call
    tok, lp = out if out is not None else (torch.empty(N, dtype=torch.int32, device=DEV),
                                           torch.empty(N, dtype=torch.float32, device=DEV))
    seed_dev = torch.tensor([seed], dtype=torch.int32, device=DEV)
    cnt = torch.tensor([step - 1], dtype=torch.int32, device=DEV) if step_dev else None
    call('tell_adaptive_logprob_sample_penalised', *args, N, k, inv_temp, seed_dev, None, 0 if step_dev else step, cnt,
         *pen_args, tok, lp)
    return tok.cpu().numpy(), lp.cpu().numpy()


def test_penalised_sampler_kernel():
    from tell_amd import hip
    from tell_amd.hip import call
    N = N_ROWS
    args = _rows(N, SEED)
    lp64 = _cpu_logprobs64(args)
    lists = _make_lists(lp64)
    sub_np = sub_table(ALPHA, BETA, 256)
    sub = torch.from_numpy(sub_np).to(DEV)
    L = _Lists(lists, V)
    pa = L.args(THETA, sub)
    inv_temp = float(np.float32(1 / 0.9))
    got = {}
    for regs in (1, 0):
        with hip.options(argmax_regs=regs):
            # k = 1: the penalised arg-max, bit for bit
            a_tok, a_lp = _pen_topk(args, N, 1, pa)
            s_tok, s_lp = _pen_sample(args, N, 1, inv_temp, 5, 3, pa)
            assert np.array_equal(s_tok, a_tok[:, 0]) and np.array_equal(_bits(s_lp), _bits(a_lp[:, 0])), regs
            full = _full_rows(args, N, V)
            s = np.stack([penalised(full[r], lists[r], THETA, sub_np) for r in range(N)])
            order = np.stack([np.lexsort((np.arange(V), -row))[:64] for row in s])
            for k in (2, 64):
                seed, step = 100 + k, 7
                tok, lp = _pen_sample(args, N, k, inv_temp, seed, step, pa)
                got[(regs, k)] = tok
                for r in range(N):
                    assert tok[r] in order[r, :k], (regs, k, r)        # every drawn token lies in the penalised top k
                want_tok, want_lp, near = _expect(s, order, k, inv_temp, seed, np.arange(N), step)
                bad = np.nonzero(tok != want_tok)[0]
                assert all(near[r] for r in bad), (regs, k, bad)       # (only a u on a CDF edge may fall the other way)
                assert len(bad) <= 1
                ok = tok == want_tok
                if regs:
                    np.testing.assert_allclose(lp[ok], want_lp[ok], rtol=0, atol=4e-6 * THETA)
                else:                                                  # the streaming form has the full-row kernel's arithmetic
                    assert np.array_equal(_bits(lp[ok]), _bits(want_lp[ok])), k
                # host step and device step: bitwise the same
                tok_d, lp_d = _pen_sample(args, N, k, inv_temp, seed, step, pa, step_dev=True)
                assert np.array_equal(tok_d, tok) and np.array_equal(_bits(lp_d), _bits(lp))
                # eager and hipGraph: bitwise the same
                o_tok = torch.empty(N, dtype=torch.int32, device=DEV)
                o_lp = torch.empty(N, dtype=torch.float32, device=DEV)
                seed_dev = torch.tensor([seed], dtype=torch.int32, device=DEV)
                cnt = torch.tensor([step - 1], dtype=torch.int32, device=DEV)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    call('tell_adaptive_logprob_sample_penalised', *args, N, k, inv_temp, seed_dev, None, 0, cnt, *pa, o_tok, o_lp)
                g.replay()
                torch.cuda.synchronize()
                assert np.array_equal(o_tok.cpu().numpy(), tok) and np.array_equal(_bits(o_lp.cpu().numpy()), _bits(lp))
    for k in (2, 64):                                                  # the register and streaming forms agree on tokens
        assert np.array_equal(got[(1, k)], got[(0, k)]), k


def test_penalised_sampler_distribution():
    """One logit row under 8192 workgroups (leading dimension 0) at three steps = 24 576 draws, k = 50, T = 0.8: the counts
    of the drawn tokens against softmax(top-k(s) / T) - the chi2 threshold of tests/test_gpu_sampling.py."""
    R, STEPS, k, T = 8192, (9, 10, 11), 50, 0.8
    one = _rows(1, 5)
    lp64 = _cpu_logprobs64(one)
    top = np.argsort(-lp64[0])
    lists = [([int(top[0]), int(top[1]), int(top[3]), int(top[7]), int(top[60]), 12345], [3, 1, 2, 5, 1, 4])]
    sub_np = sub_table(ALPHA, BETA, 256)
    sub = torch.from_numpy(sub_np).to(DEV)
    L1 = _Lists(lists, V)
    full = _full_rows(one, 1, V)
    s = penalised(full[0], lists[0], THETA, sub_np)
    order = np.lexsort((np.arange(V), -s))[:k]
    assert set(order[:8].tolist()) != set(top[:8].tolist())            # the penalties changed the candidate set's head
    args = list(one)
    for i in (1, 5, 8):                                                # every row pointer stays on the one row
        args[i] = 0
    p_tok, p_cnt = L1.tok.expand(R, -1).contiguous(), L1.cnt.expand(R, -1).contiguous()
    pa = [p_tok, p_cnt, p_tok.stride(0), L1.n_pen.expand(R).contiguous(), THETA, sub, sub.numel()]
    toks, lps = [], []
    for step in STEPS:
        tok, lp = _pen_sample(args, R, k, float(np.float32(1 / T)), 424242, step, pa)
        toks.append(tok)
        lps.append(lp)
    tok, lp = np.concatenate(toks), np.concatenate(lps)
    assert len(tok) == 24576 and np.isin(tok, order).all()
    p = np.exp((s[order].astype(np.float64) - s[order[0]]) / T)
    p /= p.sum()
    cnt = np.array([(tok == t_).sum() for t_ in order], dtype=np.float64)
    exp = p * len(tok)
    big = exp >= 5                                                     # (bins with fewer than 5 expected draws pooled)
    o = np.r_[cnt[big], cnt[~big].sum()]
    e = np.r_[exp[big], exp[~big].sum()]
    chi2 = ((o - e) ** 2 / np.maximum(e, 1e-12)).sum()
    dof = len(o) - 1
    print('\npenalised sampler: chi2 %.1f at %d dof' % (chi2, dof))
    assert chi2 < dof + 3.72 * np.sqrt(2 * dof) + 8, (chi2, dof)
    np.testing.assert_allclose(lp, s[tok], rtol=0, atol=4e-6 * THETA)


# --------------------------------------------------------------------------- 4. generators
FP32_GEN, FP32_EOS_FACTOR, FP32_SEED = 12, 14.0, 43


def test_full_size_generators_with_penalties_match_the_definition_fp32():
    """Setup of test_full_size_generators_with_options_match_the_definition_fp32 at B = 4: the cached fp32 generators
    (the layer-by-layer path, through the same head) under (theta, alpha, beta) = (1.3, 0.5, 0.25), greedy and beam 4,
    against greedy_pen / beam_search_pen - identical ids, scores within section 16's rtol 1e-4 / atol 5e-4."""
    import tell_amd
    from oracle.build import build_decoder as obuild
    from tell_amd.build import build_decoder
    from test_gpu_fullsize import _inputs_batch, _oracle, _sharpened_eos, _shell_models, _to_dev
    BB, GEN, pen = 4, FP32_GEN, (THETA, ALPHA, BETA)
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
        _, plain_ids, _ = m._generate_cached(start.to(DEV), dctx, gen_len=GEN, eos=2)
        want_ids, want_s = greedy_pen(om, start, c(), gen_len=GEN, pen=pen)
        assert repeats(want_ids) < repeats(plain_ids.cpu())           # non-vacuity: the penalties change this decode
        m.repetition_penalty, m.presence_penalty, m.frequency_penalty = pen
        with _Spy() as spy:
            lp, got, _ = m._generate_cached(start.to(DEV), dctx, gen_len=GEN, eos=2)
        assert NEW - {'tell_adaptive_logprob_sample_penalised'} <= set(spy.names)
        same(got, want_ids)
        n = min(lp.shape[1], want_s.shape[1])
        print('\nfp32 greedy: max |s - definition| = %.3g' % float((lp.cpu()[:, :n] - want_s[:, :n]).abs().max()))
        assert torch.allclose(lp.cpu()[:, :n], want_s[:, :n], rtol=1e-4, atol=5e-4)
        want_b, want_sc, _ = beam_search_pen(om, start, c(), 4, gen_len=GEN, pen=pen)
        lp, got, info = m._generate_beam(start.to(DEV), dctx, 4, gen_len=GEN, eos=2, n_best=4)
        ids_n, lps_n, sc_n = info.nbest
        print('fp32 beam 4: scores %s vs definition %s' % (sc_n.cpu().tolist(), want_sc.tolist()))
        same(ids_n, want_b)
        same(got, want_b[:, 0])
        assert torch.allclose(sc_n.cpu(), want_sc, rtol=1e-4, atol=5e-4), (sc_n, want_sc)
        m.repetition_penalty, m.presence_penalty, m.frequency_penalty = 1.0, 0.0, 0.0


BF16_EOS_FACTOR, BF16_PEN = 12.0, (1.2, 0.0, 0.1)


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
    pen = build_model('faces_objects', resnet=plain.resnet, roberta=plain.roberta, repetition_penalty=BF16_PEN[0],
                      presence_penalty=BF16_PEN[1], frequency_penalty=BF16_PEN[2])
    pen.load_state_dict(sd)
    pen.to(DEV).eval()
    batches = [synthetic_batch(32, 64, 9, True, seed=91, device=DEV), synthetic_batch(4, 64, 9, True, seed=92, device=DEV)]
    yield plain, pen, batches
    tell_amd.set_compute_dtype(torch.float32)


def _pen_graphs(model):
    return [h for sig, h in model.__dict__['_decode_graphs'].items()
            if any(isinstance(x, tuple) and x[:1] == ('penalty',) for x in sig)]


def test_fused_bf16_greedy_with_penalties_at_the_bench_batch(fullsize):
    """Captured runs and the same step issued launch by launch over the same static buffers (the capture refused: the
    stepper's eager fallback, step index from the host) give the same ids and scores; the reported log_probs are the penalised scores recomputed from the
    model's own teacher-forced log-probs of the generated captions (score_captions) and the token counts - bit for bit:
    the forced kernel reproduces the arg-max kernels' log-prob and the step is deterministic."""
    import tell_amd
    from tell_amd.models import stepper as stepper_mod
    plain, pen, batches = fullsize
    theta, alpha, beta = BF16_PEN
    b = batches[0]
    keep = stepper_mod.graphs
    with torch.no_grad():
        free = plain.generate(**_clone(b))
        out = pen.generate(**_clone(b))
        torch.cuda.synchronize()
        hs = _pen_graphs(pen)
        assert hs and all(h['graph'] not in (None, False) for h in hs), [h.get('error') for h in hs]
        assert any(h.get(('multi', 8)) for h in hs), [h.get('multi_error') for h in hs]
        class NoCapture:                                      # the stepper's view of tell_amd.graphs, with captures refused
            def __getattr__(self, name):
                return getattr(tell_amd.graphs, name)

            @staticmethod
            def capture(*a, **kw):
                raise RuntimeError('capture refused by the test')
        pen.__dict__.pop('_decode_graphs', None)
        try:
            stepper_mod.graphs = NoCapture()
            with _Spy() as spy:
                eager = pen.generate(**_clone(b))
            torch.cuda.synchronize()
            hs = _pen_graphs(pen)
            assert hs and all(h['graph'] is False for h in hs)              # every step of this run was issued eagerly
        finally:
            stepper_mod.graphs = keep
            pen.__dict__.pop('_decode_graphs', None)
        assert NEW - {'tell_adaptive_logprob_sample_penalised'} <= set(spy.names)
        print('\nbf16 B=32 greedy: eager and captured ids equal: %s, scores bitwise: %s'
              % (torch.equal(eager['gen_ids'], out['gen_ids']), torch.equal(eager['log_probs'], out['log_probs'])))
        assert torch.equal(eager['gen_ids'], out['gen_ids'])
        assert torch.equal(eager['log_probs'], out['log_probs'])
        ids = out['gen_ids']
        print('\nbf16 B=32 greedy: %d repeated positions unpenalised, %d with penalties; %d steps'
              % (repeats(free['gen_ids'].cpu()), repeats(ids.cpu()), ids.shape[1] - 1))
        assert not torch.equal(ids[:, :min(ids.shape[1], free['gen_ids'].shape[1])],
                               free['gen_ids'][:, :min(ids.shape[1], free['gen_ids'].shape[1])]) \
            or ids.shape != free['gen_ids'].shape
        bb = _clone(b)
        bb['caption'] = dict(bb['caption'])
        bb['caption'][plain.index] = ids.clone()
        sc = plain.score_captions(bb)
        torch.cuda.synchronize()
    lp, got = sc['log_probs'].cpu().numpy(), out['log_probs'].cpu().numpy()
    ids = ids.cpu().numpy()
    sub = sub_table(alpha, beta, 101)
    f = np.float32
    want = np.zeros_like(got)
    for r in range(ids.shape[0]):
        for i in range(ids.shape[1] - 1):
            t = int(ids[r, i + 1])
            if t == 1:                                                  # behind the row's </s>
                break
            toks, cnts = token_counts(ids[r].tolist(), i)
            want[r, i] = lp[r, i] if t not in toks else f(f(np.minimum(lp[r, i], f(0.0)) * f(theta)) - sub[cnts[toks.index(t)]])
    diff = np.abs(got - want)
    n_bits = int((_bits(got) != _bits(want)).sum())
    print('bf16 B=32 greedy: %d of %d reported scores differ in bits from the recomputation, max |diff| %.3g'
          % (n_bits, got.size, float(diff.max())))
    assert float(diff.max()) <= 4e-6 * theta, float(diff.max())
    assert n_bits == 0, n_bits


def test_fused_topk_sampling_with_penalties_follows_the_seed(fullsize):
    _, pen, batches = fullsize
    b = batches[0]
    keep = (pen.sampling_topk, pen.sampling_temp)
    pen.sampling_topk, pen.sampling_temp = 8, 0.9
    try:
        with torch.no_grad(), _Spy() as spy:
            torch.manual_seed(5)
            a = pen.generate(**_clone(b))
            torch.manual_seed(5)
            a2 = pen.generate(**_clone(b))
            torch.manual_seed(6)
            c = pen.generate(**_clone(b))
            torch.cuda.synchronize()
    finally:
        pen.sampling_topk, pen.sampling_temp = keep
    assert 'tell_adaptive_logprob_sample_penalised' in spy.names and 'tell_decode_token_counts' in spy.names
    assert torch.equal(a['gen_ids'], a2['gen_ids']) and torch.equal(a['log_probs'], a2['log_probs'])
    assert a['gen_ids'].shape != c['gen_ids'].shape or not torch.equal(a['gen_ids'], c['gen_ids'])
    hs = _pen_graphs(pen)
    assert any(any(isinstance(x, tuple) and x[:1] == ('sample',) for x in sig) and h['graph'] not in (None, False)
               for sig, h in pen.__dict__['_decode_graphs'].items() if h in hs)


# --------------------------------------------------------------------------- 5. the defaults change nothing
def test_defaults_change_nothing_on_the_fused_path(fullsize):
    """A model built with the three keys at their defaults against one built without them: the same ids, the same graph
    keys, and - warm steps, captures and bookkeeping - the same sequence of entry points, none of them new."""
    from tell_amd.build import build_model
    plain, _, batches = fullsize
    keyed = build_model('faces_objects', resnet=plain.resnet, roberta=plain.roberta, repetition_penalty=1.0,
                        presence_penalty=0.0, frequency_penalty=0.0)
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
            pk = [s_[:5] + s_[6:] for s_ in plain.__dict__['_decode_graphs']]     # (all but the position table's address)
            kk = [s_[:5] + s_[6:] for s_ in keyed.__dict__['_decode_graphs']]
            assert pk == kk and not any(isinstance(x, tuple) and x[:1] == ('penalty',) for s_ in kk for x in s_)
            assert all(h['graph'] not in (None, False) for h in keyed.__dict__['_decode_graphs'].values())
            assert all('pen_src' not in h for h in keyed.__dict__['_decode_graphs'].values())
            assert sa.names == sk.names and len(sa.names) > 100
            assert not NEW & set(sk.names)
            assert ('tell_beam_update' if K > 1 else 'tell_greedy_update') in sk.names
