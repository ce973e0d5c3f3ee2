"""Search options of the cached generators: beam_len_penalty, no_repeat_ngram_size, min_len, n_best.
The plain definitions live here as test code - `ban_set`, `beam_update_norm`, `beam_search_opts` (prefix re-decoding over
the oracle decoder, the way oracle/beam.py is written) - and are what tests/test_gpu_beam_options.py holds the kernels and
the generators to.  This file needs no GPU: option validation, the inv_norm table, the definitions' fixed point at the
defaults (== oracle.beam.beam_search) and their effect on the oracle's own output."""
import numpy as np
import pytest
import torch


# --------------------------------------------------------------------------- the definitions
def ban_set(history, i, n, min_len, eos):
    """Banned tokens of a LIVE row at step i with history h[0..i] (h[0] = <s>): with n >= 1 and i + 1 >= n every p in
    0..i+1-n whose n-1 tokens h[p..p+n-2] equal the last n-1 tokens h[i-n+2..i] bans h[p+n-1]; i < min_len bans eos."""
    h = [int(t) for t in history[:i + 1]]
    out = set()
    if n >= 1 and i + 1 >= n:
        last = h[i - n + 2:i + 1]
        for p in range(0, i + 2 - n):
            if h[p:p + n - 1] == last:
                out.add(h[p + n - 1])
    if i < min_len:
        out.add(int(eos))
    return out


def inv_norm(alpha, L):
    t = np.ones(L + 1, dtype=np.float32)
    for l in range(1, L + 1):
        t[l] = np.float32(np.float64(l) ** -np.float64(alpha))
    return t


def beam_update_norm(tk, lp, cum, fin, seqs, lps, length, table, step, pad, eos, inv_temp, back=None):
    """One step's beam bookkeeping with a length penalty, in numpy fp32 (include/tell_hip.h tell_beam_update_norm).
    tk int / lp fp32 [B,K,K], cum fp32 [B,K], fin bool [B,K], seqs int64 [B,K,L], lps fp32 [B,K,L-1], length int [B,K],
    table fp32 [L+1], back int32 [n_back, B*K] or None.  -> dict of the updated arrays (+ cur, rows)."""
    B, K = cum.shape
    f32 = np.float32
    n_cum, n_fin, n_seqs, n_lps, n_len = cum.copy(), fin.copy(), seqs.copy(), lps.copy(), length.copy()
    cur = np.zeros(B * K, dtype=np.int64)
    rows = np.zeros(B * K, dtype=np.int64)
    n_back = None if back is None else back.copy()
    for b in range(B):
        cand = []
        for j in range(K):
            for m in range(K):
                if fin[b, j]:
                    l = f32(0.0) if m == 0 else f32(-np.inf)
                    tok, ln = pad, int(length[b, j])
                else:
                    l = f32(f32(lp[b, j, m]) * f32(inv_temp))
                    tok, ln = int(tk[b, j, m]), step + 1
                with np.errstate(invalid='ignore'):
                    raw = f32(f32(cum[b, j]) + l)
                    score = f32(raw * f32(table[ln]))
                if np.isnan(score):
                    score = f32(-np.inf)
                cand.append((score, j * K + m, j, tok, raw, ln))
        taken = sorted(cand, key=lambda c: (-c[0], c[1]))[:K]         # best score first, lowest candidate index on ties
        for r, (score, _, j, tok, raw, ln) in enumerate(taken):
            n_seqs[b, r] = seqs[b, j]
            n_lps[b, r] = lps[b, j]
            n_seqs[b, r, step + 1] = tok
            with np.errstate(invalid='ignore'):
                n_lps[b, r, step] = f32(0.0) if fin[b, j] else f32(raw - f32(cum[b, j]))
            n_cum[b, r], n_len[b, r] = raw, ln
            n_fin[b, r] = bool(fin[b, j]) or tok == eos
            cur[b * K + r] = tok
            rows[b * K + r] = b * K + j
            if back is not None:
                n_back[0, b * K + r] = b * K + j
                n_back[1:, b * K + r] = back[:-1, b * K + j]
    return dict(cum=n_cum, finished=n_fin, seqs=n_seqs, lps=n_lps, len=n_len, cur=cur, rows=rows, back=n_back)


@torch.no_grad()
def beam_search_opts(model, caption_ids, contexts, beam_size, gen_len=100, eos=2, alpha=0.0, ngram=0, min_len=0):
    """oracle/beam.py's prefix-re-decoding beam search with the search options.  model: oracle CaptionModel.
    -> (ids [B, K, L], scores [B, K]) best first; scores = sum of log-probs * inv_norm[len]."""
    B, K, pad = caption_ids.shape[0], beam_size, model.padding_idx
    ctx = {}
    for name, val in contexts.items():
        ctx[name] = val.repeat_interleave(K, dim=0 if name.endswith('_mask') else 1)
    seqs = caption_ids[:, 0:1].repeat_interleave(K, dim=0).view(B, K, 1)
    cum = torch.full((B, K), float('-inf'))
    cum[:, 0] = 0.0
    finished = seqs[:, :, 0] == eos
    length = torch.zeros(B, K, dtype=torch.long)
    table = torch.from_numpy(inv_norm(alpha, gen_len + 1))
    for i in range(gen_len):
        out = model.decoder({model.index: seqs.view(B * K, -1)}, ctx, incremental_state=None)
        lp = model.decoder.get_normalized_probs((out[0][:, -1:], None), log_probs=True).view(B, K, -1)
        lp = lp / model.sampling_temp
        V = lp.shape[-1]
        for b in range(B):
            for j in range(K):
                if not bool(finished[b, j]):
                    for t in ban_set(seqs[b, j].tolist(), i, ngram, min_len, eos):
                        lp[b, j, t] = float('-inf')
        lp = lp.masked_fill(finished.unsqueeze(-1), float('-inf'))
        lp[..., pad] = torch.where(finished, torch.zeros_like(cum), lp[..., pad])
        raw = (cum.unsqueeze(-1) + lp).view(B, K * V)
        cand_len = torch.where(finished, length, torch.full_like(length, i + 1))
        score = raw * table[cand_len].unsqueeze(-1).expand(B, K, V).reshape(B, K * V)
        score = torch.where(torch.isnan(score), torch.full_like(score, float('-inf')), score)
        idx = torch.sort(score, dim=1, descending=True, stable=True)[1][:, :K]   # lowest candidate index wins a tie
        parent, tok = idx // V, idx % V
        was = finished.gather(1, parent)
        tok = torch.where(was, torch.full_like(tok, pad), tok)
        seqs = torch.cat([seqs.gather(1, parent.unsqueeze(-1).expand(-1, -1, seqs.shape[2])), tok.unsqueeze(-1)], 2)
        finished = was | (tok == eos)
        cum = raw.gather(1, idx)
        length = cand_len.gather(1, parent)
        if bool(finished.all()):
            break
    return seqs, cum * table[length]


def repeats_ngram(ids, n, pad=1):
    """Whether the pad-stripped sequence (its <s> included) holds the same n-gram twice."""
    h = [int(t) for t in ids if int(t) != pad]
    grams = [tuple(h[p:p + n]) for p in range(len(h) - n + 1)]
    return len(set(grams)) < len(grams)


def eos_before(ids, m, eos=2):
    """Whether eos is generated at a step < m (step i writes column i + 1)."""
    return any(int(t) == eos for t in ids[1:m + 1])


# --------------------------------------------------------------------------- a small oracle model on a golden decoder
GEN, NGRAM, MINLEN, ALPHA = 24, 2, 6, 1.0


@pytest.fixture(scope='module')
def small(golden):
    from oracle.build import build_decoder
    from oracle.models import CaptionModel as OModel
    fx = golden('decoder_flattened')
    dec = build_decoder('flattened', article_dim=64, vocab_size=600, dim=64, heads=4, ffn=128, kernels=(3, 7),
                        cutoff=(100, 300)).eval()
    sd = {k: v.clone() for k, v in fx['sd'].items() if k in dec.state_dict()}
    done = set()
    for k, v in sd.items():                                  # (this fixture's </s> logit is negative: flipped and scaled, hypotheses end at different steps)
        if (k.endswith('adaptive_softmax.head.word_proj.weight') or k.endswith('embeddings.0.weight')) and \
                v.data_ptr() not in done:
            v[2] *= -1.3
            v[1] = 0.0
            done.add(v.data_ptr())
    dec.load_state_dict(sd, strict=False)
    om = OModel.__new__(OModel)
    torch.nn.Module.__init__(om)
    om.decoder, om.padding_idx, om.index, om.sampling_topk, om.sampling_temp = dec, 1, 'roberta', 1, 1.0
    ins = fx['in']
    ctx = {k: v for k, v in ins.items() if k not in ('ids', 'target')}
    return om, ins['ids'][:, :1].contiguous(), ctx


def test_ban_set_examples():
    h = [0, 5, 6, 7, 5, 6]
    assert ban_set(h, 5, 3, 0, 2) == {7}                    # "5 6" was followed by 7
    assert ban_set(h, 5, 2, 0, 2) == {7}                    # "6" was followed by 7
    assert ban_set(h, 5, 1, 0, 2) == {0, 5, 6, 7}
    assert ban_set(h, 1, 3, 0, 2) == set()                  # i + 1 < n
    assert ban_set(h, 2, 3, 4, 2) == {2}
    assert ban_set([0, 4, 4, 4], 3, 3, 0, 2) == {4}
    assert ban_set(h, 5, 0, 0, 2) == set()


def test_inv_norm_table_is_the_stated_formula():
    from tell_amd.models.transformer import inv_norm_table
    for alpha in (0.0, 0.6, 1.0, 2.5):
        got = inv_norm_table(alpha, 101)
        assert got.dtype == torch.float32 and got.shape == (102,)
        assert got[0] == 1.0
        assert np.array_equal(got.numpy(), inv_norm(alpha, 101))
    assert bool((inv_norm_table(0.0, 50) == 1.0).all())


def _shell(cls, decoder):
    m = cls.__new__(cls)
    torch.nn.Module.__init__(m)
    m.decoder, m.padding_idx, m.index, m.sampling_topk, m.sampling_temp, m.sampling_topp = decoder, 1, 'roberta', 1, 1.0, None
    return m


class _Dyn(torch.nn.Module):
    def project_contexts(self, contexts):
        raise AssertionError('not reached')


def test_option_validation():
    from tell_amd.models.transformer import CaptionModel, check_beam_options
    assert check_beam_options() == (0.0, 0, 0)
    assert check_beam_options(1, 3, 4) == (1.0, 3, 4)
    for bad, name in (({'beam_len_penalty': -0.1}, 'beam_len_penalty'), ({'beam_len_penalty': float('inf')}, 'beam_len_penalty'),
                      ({'beam_len_penalty': 'x'}, 'beam_len_penalty'), ({'no_repeat_ngram_size': 9}, 'no_repeat_ngram_size'),
                      ({'no_repeat_ngram_size': -1}, 'no_repeat_ngram_size'), ({'no_repeat_ngram_size': 1.5}, 'no_repeat_ngram_size'),
                      ({'min_len': 100}, 'min_len'), ({'min_len': -1}, 'min_len'), ({'min_len': True}, 'min_len')):
        with pytest.raises(ValueError, match=name):
            check_beam_options(**bad)
    assert check_beam_options(min_len=99) == (0.0, 0, 99)
    with pytest.raises(ValueError, match='min_len'):
        check_beam_options(min_len=8, gen_len=8)
    m = _shell(CaptionModel, _Dyn())
    assert m._check_options(4, False, 1) is None            # the defaults: nothing to check, nothing changes
    for bad in (0, 5, 1.0, True):
        with pytest.raises(ValueError, match='n_best'):
            m._check_options(4, False, bad)
    with pytest.raises(ValueError, match='n_best'):
        m._check_options(1, False, 2)
    assert m._check_options(4, False, 4) is None
    m.no_repeat_ngram_size = 3
    assert m._check_options(4, False, 2) == (0.0, 3, 0)
    with pytest.raises(ValueError, match='no_repeat_ngram_size'):
        m._check_options(1, True, 1)                        # attention=True
    m.sampling_topk = 5
    with pytest.raises(ValueError, match='no_repeat_ngram_size'):
        m._check_options(1, False, 1)
    m.sampling_topk, m.sampling_topp = 0, 0.9
    with pytest.raises(ValueError, match='no_repeat_ngram_size'):
        m._check_options(1, False, 1)
    m.sampling_topk, m.sampling_topp, m.no_repeat_ngram_size = 1, None, 0
    for key, val in (('beam_len_penalty', 1.0), ('min_len', 4)):
        setattr(m, key, val)
        with pytest.raises(ValueError, match=key):
            m._check_options(1, True, 1)
        m.sampling_topk = 4
        with pytest.raises(ValueError, match=key):
            m._check_options(1, False, 1)
        m.sampling_topk = 1
        setattr(m, key, 0)
    m.sampling_topp = 0.5
    with pytest.raises(ValueError, match='n_best'):
        m._check_options(4, False, 2)
    m.sampling_topp = None
    with pytest.raises(ValueError, match='n_best'):
        m._check_options(4, True, 2)
    m.min_len = 100
    with pytest.raises(ValueError, match='min_len'):
        m._check_options(1, False, 1)


def test_options_are_refused_on_lstm_decoders_and_copy_models():
    from tell_amd.models.baseline_glove import BaselineGloveModel, _refuse_search_options
    from tell_amd.models.pointer import TransformerPointerModel
    from tell_amd.models.transformer import CaptionModel
    lstm = _shell(CaptionModel, torch.nn.Linear(2, 2))       # a decoder without project_contexts: the LSTM decoders
    ptr = _shell(TransformerPointerModel, _Dyn())
    for m in (lstm, ptr):
        assert m._check_options(1, False, 1) is None
        for key, val in (('beam_len_penalty', 0.5), ('no_repeat_ngram_size', 2), ('min_len', 3)):
            setattr(m, key, val)
            with pytest.raises(ValueError, match=key):
                m._check_options(4, False, 1)
            setattr(m, key, 0)
        with pytest.raises(ValueError, match='n_best'):
            m._check_options(4, False, 2)
    glove = BaselineGloveModel.__new__(BaselineGloveModel)
    _refuse_search_options(glove)
    for kw, key in (({'beam_len_penalty': 0.5}, 'beam_len_penalty'), ({'no_repeat_ngram_size': 2}, 'no_repeat_ngram_size'),
                    ({'min_len': 3}, 'min_len'), ({'n_best': 2}, 'n_best')):
        with pytest.raises(ValueError, match=key):
            _refuse_search_options(glove, **kw)


def test_constructor_keys_and_defaults():
    import inspect
    from tell_amd.build import build_model
    from tell_amd.models.baseline_glove import BaselineGloveModel, TransformerGloveModel
    from tell_amd.models.pointer import PointerModelBase
    from tell_amd.models.transformer import CaptionModel
    for cls in (CaptionModel, TransformerGloveModel, PointerModelBase, BaselineGloveModel):
        p = inspect.signature(cls.__init__).parameters
        assert (p['beam_len_penalty'].default, p['no_repeat_ngram_size'].default, p['min_len'].default) == (0.0, 0, 0), cls
    for fn in (CaptionModel.generate, CaptionModel.generate_lanes, CaptionModel.generate_stream):
        assert inspect.signature(fn).parameters['n_best'].default == 1
    kw = dict(vocab_size=600, dim=64, heads=4, ffn=128, cutoff=(100, 300), kernels=(3, 7))
    stub = torch.nn.Identity()
    m = build_model('flattened', stub, stub, n_bert_layers=3, **kw)
    assert (m.beam_len_penalty, m.no_repeat_ngram_size, m.min_len) == (0.0, 0, 0) and m._search_options() is None
    m = build_model('flattened', stub, stub, n_bert_layers=3, beam_len_penalty=1, no_repeat_ngram_size=3, min_len=4, **kw)
    assert m._search_options() == (1.0, 3, 4)
    with pytest.raises(ValueError, match='no_repeat_ngram_size'):
        build_model('flattened', stub, stub, n_bert_layers=3, no_repeat_ngram_size=3, sampling_topk=5, **kw)
    with pytest.raises(ValueError, match='min_len'):
        build_model('flattened', stub, stub, n_bert_layers=3, min_len=2, sampling_topk=0, sampling_topp=0.9, **kw)
    with pytest.raises(ValueError, match='beam_len_penalty'):
        build_model('pointer', stub, stub, n_bert_layers=3, beam_len_penalty=1.0, **kw)
    with pytest.raises(ValueError, match='min_len'):
        build_model('flattened', stub, stub, n_bert_layers=3, min_len=100, **kw)


def test_definition_at_the_defaults_is_oracle_beam_search(small):
    from oracle.beam import beam_search
    om, start, ctx = small
    for K in (4, 2):
        ref_ids, ref_score = beam_search(om, start, {k: v.clone() for k, v in ctx.items()}, K, gen_len=GEN)
        ids, scores = beam_search_opts(om, start, {k: v.clone() for k, v in ctx.items()}, K, gen_len=GEN)
        assert torch.equal(ids[:, 0], ref_ids) and torch.equal(scores[:, 0], ref_score), K
        assert bool((scores[:, :-1] >= scores[:, 1:]).all())


def test_options_change_the_oracles_own_output(small):
    om, start, ctx = small
    c = lambda: {k: v.clone() for k, v in ctx.items()}       # noqa: E731
    K = 4
    plain, _ = beam_search_opts(om, start, c(), K, gen_len=GEN)
    # non-vacuity: left alone, this decoder repeats an n-gram and ends before MINLEN in at least one row each
    assert any(repeats_ngram(h, NGRAM) for b in plain for h in b)
    assert any(eos_before(h, MINLEN) for b in plain for h in b)
    ids, _ = beam_search_opts(om, start, c(), K, gen_len=GEN, ngram=NGRAM)
    assert not any(repeats_ngram(h, NGRAM) for b in ids for h in b)
    ids, _ = beam_search_opts(om, start, c(), K, gen_len=GEN, min_len=MINLEN)
    assert not any(eos_before(h, MINLEN) for b in ids for h in b)
    ids, scores = beam_search_opts(om, start, c(), K, gen_len=GEN, alpha=ALPHA, ngram=NGRAM, min_len=MINLEN)
    assert not any(repeats_ngram(h, NGRAM) or eos_before(h, MINLEN) for b in ids for h in b)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    # the length penalty moves the best hypothesis of at least one row
    pen, _ = beam_search_opts(om, start, c(), K, gen_len=GEN, alpha=ALPHA)
    assert not torch.equal(pen[:, 0], plain[:, 0])
    # greedy (one hypothesis) under the bans
    g0, _ = beam_search_opts(om, start, c(), 1, gen_len=GEN)
    g1, _ = beam_search_opts(om, start, c(), 1, gen_len=GEN, ngram=NGRAM, min_len=MINLEN)
    assert any(repeats_ngram(h[0], NGRAM) for h in g0) or any(eos_before(h[0], MINLEN) for h in g0)
    assert not any(repeats_ngram(h[0], NGRAM) or eos_before(h[0], MINLEN) for h in g1)


def test_beam_update_norm_definition_with_all_ones_is_the_plain_update():
    """The numpy definition itself: with the all-ones table the survivors are the K best raw sums, best first."""
    rng = np.random.default_rng(0)
    B, K, L = 3, 4, 6
    tk = rng.integers(3, 50, (B, K, K))
    lp = -np.sort(rng.random((B, K, K)).astype(np.float32), -1)
    cum = -rng.random((B, K)).astype(np.float32)
    fin = np.zeros((B, K), bool)
    fin[0, 1] = True
    out = beam_update_norm(tk, lp, cum, fin, np.ones((B, K, L), np.int64), np.zeros((B, K, L - 1), np.float32),
                           np.full((B, K), 2), np.ones(L + 1, np.float32), 2, 1, 2, 1.0)
    for b in range(B):
        allc = sorted([(cum[b, j] + (0.0 if m == 0 else -np.inf) if fin[b, j] else np.float32(cum[b, j] + lp[b, j, m]))
                       for j in range(K) for m in range(K)], reverse=True)[:K]
        assert np.array_equal(out['cum'][b], np.array(allc, np.float32))
    for b in range(B):
        for r in range(K):
            assert out['len'][b, r] == (2 if fin[b, out['rows'][b * K + r] - b * K] else 3)
