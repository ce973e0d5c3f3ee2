"""Repetition, presence and frequency penalties of the cached generators.  The plain definitions live
here as test code - `token_counts`, `sub_table`, `penalised`, `beam_search_pen` / `greedy_pen` (prefix re-decoding over the
oracle decoder, the way oracle/beam.py is written) - and are what tests/test_gpu_penalties.py holds the kernels and the
generators to.  This file needs no GPU: the option ranges, every refused combination, the constructor keys, the definitions'
fixed point at (1, 0, 0) and their effect on the oracle's own output."""
import inspect

import numpy as np
import pytest
import torch

from test_abi_and_host import _write_cfg
from test_beam_options_host import _Dyn, _shell, small  # noqa: F401  (`small`: the module-scoped oracle model fixture)
from test_sampling_host import _builders

KEYS = ('repetition_penalty', 'presence_penalty', 'frequency_penalty')


# --------------------------------------------------------------------------- the definitions
def token_counts(history, i):
    """Step i of a live row with history h[0..i] (h[0] = <s>): -> ([distinct tokens of h[0..i] in order of first occurrence],
    [c_t: the number of positions of h[0..i] that hold t])."""
    toks, cnts = [], []
    for t in (int(t) for t in history[:i + 1]):
        if t in toks:
            cnts[toks.index(t)] += 1
        else:
            toks.append(t)
            cnts.append(1)
    return toks, cnts


def sub_table(alpha, beta, L):
    """fp32 [L + 1]: sub[0] = 0, sub[c] = float32(float64(alpha) + float64(beta) * c)."""
    t = np.zeros(L + 1, dtype=np.float32)
    for c in range(1, L + 1):
        t[c] = np.float32(np.float64(alpha) + np.float64(beta) * np.float64(c))
    return t


def penalised(lp_row, counts, theta, sub):
    """s_t = lp_t for c_t = 0, else min(lp_t, 0) * theta - sub[c_t]: numpy float32, the multiply and the subtract rounded one
    by one.  counts = (tokens, counts) of token_counts."""
    s = np.array(lp_row, dtype=np.float32, copy=True)
    for t, c in zip(*counts):
        m = np.float32(np.minimum(s[t], np.float32(0.0)) * np.float32(theta))
        s[t] = np.float32(m - sub[c])
    return s


@torch.no_grad()
def beam_search_pen(model, caption_ids, contexts, beam_size, gen_len=100, eos=2, pen=(1.0, 0.0, 0.0)):
    """oracle/beam.py's prefix-re-decoding beam search over penalised scores.  model: oracle CaptionModel.
    -> (ids [B, K, L], scores [B, K] = the summed s, per-token s [B, K, L - 1]), best first."""
    theta, alpha, beta = pen
    B, K, pad = caption_ids.shape[0], beam_size, model.padding_idx
    sub = sub_table(alpha, beta, gen_len + 1)
    ctx = {}
    for name, val in contexts.items():
        ctx[name] = val.repeat_interleave(K, dim=0 if name.endswith('_mask') else 1)
    seqs = caption_ids[:, 0:1].repeat_interleave(K, dim=0).view(B, K, 1)
    cum = torch.full((B, K), float('-inf'))
    cum[:, 0] = 0.0
    toks = torch.zeros(B, K, 0)
    finished = seqs[:, :, 0] == eos
    for i in range(gen_len):
        out = model.decoder({model.index: seqs.view(B * K, -1)}, ctx, incremental_state=None)
        lp = model.decoder.get_normalized_probs((out[0][:, -1:], None), log_probs=True).view(B, K, -1)
        lp = (lp / model.sampling_temp).float().clone()
        V = lp.shape[-1]
        if pen != (1.0, 0.0, 0.0):
            for b in range(B):
                for j in range(K):
                    if not bool(finished[b, j]):
                        lp[b, j] = torch.from_numpy(penalised(lp[b, j].numpy(), token_counts(seqs[b, j].tolist(), i), theta, sub))
        lp = lp.masked_fill(finished.unsqueeze(-1), float('-inf'))
        lp[..., pad] = torch.where(finished, torch.zeros_like(cum), lp[..., pad])
        raw = (cum.unsqueeze(-1) + lp).view(B, K * V)
        idx = torch.sort(raw, dim=1, descending=True, stable=True)[1][:, :K]     # lowest candidate index wins a tie
        parent, tok = idx // V, idx % V
        was = finished.gather(1, parent)
        tok = torch.where(was, torch.full_like(tok, pad), tok)
        step_s = torch.where(was, torch.zeros(B, K), lp.view(B, K * V).gather(1, idx))
        seqs = torch.cat([seqs.gather(1, parent.unsqueeze(-1).expand(-1, -1, seqs.shape[2])), tok.unsqueeze(-1)], 2)
        toks = torch.cat([toks.gather(1, parent.unsqueeze(-1).expand(-1, -1, toks.shape[2])), step_s.unsqueeze(-1)], 2)
        finished = was | (tok == eos)
        cum = raw.gather(1, idx)
        if bool(finished.all()):
            break
    return seqs, cum, toks


def greedy_pen(model, caption_ids, contexts, gen_len=100, eos=2, pen=(1.0, 0.0, 0.0)):
    """The greedy decode over penalised scores: one hypothesis.  -> (ids [B, L], per-token s [B, L - 1])."""
    ids, _, s = beam_search_pen(model, caption_ids, contexts, 1, gen_len, eos, pen)
    return ids[:, 0], s[:, 0]


def repeats(ids, pad=1):
    """How many positions of the pad-stripped sequences hold a token that an earlier position already holds."""
    n = 0
    for row in ids:
        h = [int(t) for t in row if int(t) != pad]
        n += len(h) - len(set(h))
    return n


GEN = 24
PEN = (1.3, 0.5, 0.25)              # chosen on the `small` golden model: see test_penalties_change_the_oracles_own_output


# --------------------------------------------------------------------------- hand-made examples
def test_token_counts_examples():
    h = [0, 5, 6, 5, 5, 7, 0]
    assert token_counts(h, 0) == ([0], [1])
    assert token_counts(h, 2) == ([0, 5, 6], [1, 1, 1])
    assert token_counts(h, 4) == ([0, 5, 6], [1, 3, 1])
    assert token_counts(h, 6) == ([0, 5, 6, 7], [2, 3, 1, 1])
    assert token_counts([4] * 9, 8) == ([4], [9])


def test_sub_table_and_the_packages_table_are_the_stated_formula():
    from tell_amd.models.stepper import sub_table as pkg
    for a, b in ((0.0, 0.0), (0.5, 0.25), (0.0, 0.1), (1.7, 0.0), (0.3, 1e-3)):
        want = sub_table(a, b, 101)
        got = pkg(a, b, 101)
        assert got.dtype == torch.float32 and got.shape == (102,) and got[0] == 0.0
        assert np.array_equal(got.numpy(), want)
    t = sub_table(0.5, 0.25, 4)
    assert t.tolist() == [0.0, 0.75, 1.0, 1.25, 1.5]
    assert sub_table(0.0, 0.1, 3)[3] == np.float32(np.float64(0.1) * 3)        # formed in fp64, rounded once


def test_penalised_examples():
    f = np.float32
    lp = np.array([-0.5, -1.0, -2.0, 1e-7, -3.0], dtype=f)
    sub = sub_table(0.5, 0.25, 8)
    s = penalised(lp, ([1, 3, 4], [1, 2, 8]), 1.5, sub)
    assert s[0] == lp[0] and s[2] == lp[2]                           # not listed: untouched
    assert s[1] == f(f(-1.0) * f(1.5)) - f(0.75)
    assert s[3] == f(0.0) - f(1.0)                                   # a log-prob above 0 counts as 0: s <= lp
    assert s[4] == f(f(-3.0) * f(1.5)) - f(2.5)
    assert bool((s <= lp).all())
    # the two roundings are separate: theta and lp chosen so that one fused operation would differ
    lp2 = np.array([-1.0000001], dtype=f)
    th = f(1.0000001)
    two = f(f(lp2[0] * th) - f(0.75))
    assert penalised(lp2, ([0], [1]), th, sub)[0] == two
    # (1, 0, 0) is the identity wherever lp <= 0
    assert np.array_equal(penalised(lp[[0, 1, 2, 4]], ([0, 3], [2, 5]), 1.0, sub_table(0.0, 0.0, 8)), lp[[0, 1, 2, 4]])
    assert lp[0] == f(-0.5)                                          # the input row is left alone


# --------------------------------------------------------------------------- options
def test_check_penalties_ranges():
    from tell_amd.models.transformer import check_penalties
    assert check_penalties() == (1.0, 0.0, 0.0)
    assert check_penalties(1.2, 0, 0.1) == (1.2, 0.0, 0.1)
    assert check_penalties(1, 2, 3) == (1.0, 2.0, 3.0)
    for key, lo in zip(KEYS, (1.0, 0.0, 0.0)):
        for bad in (lo - 0.01, float('inf'), float('nan'), -float('inf'), 'x', None, True, [1.0]):
            with pytest.raises(ValueError, match=key):
                check_penalties(**{key: bad})


def test_penalties_method_and_refused_combinations():
    from tell_amd.models.transformer import CaptionModel
    m = _shell(CaptionModel, _Dyn())
    assert m._penalties() is None and m._check_penalties() is None             # the defaults: nothing set, nothing checked
    m.repetition_penalty = 1.2
    assert m._penalties() == (1.2, 0.0, 0.0) and m._check_penalties() == (1.2, 0.0, 0.0)
    m.sampling_topk = 8                                                         # top-k sampling: in scope
    assert m._check_penalties() == (1.2, 0.0, 0.0)
    m.sampling_topk = 1
    with pytest.raises(ValueError, match='repetition_penalty.*attention'):
        m._check_penalties(True)
    for name, v in (('sampling_topp', 0.9), ('sampling_minp', 0.1), ('sampling_typical', 0.9)):
        setattr(m, name, v)
        with pytest.raises(ValueError, match='repetition_penalty.*' + name):
            m._check_penalties()
        setattr(m, name, None)
    for name, v in (('no_repeat_ngram_size', 3), ('min_len', 4)):
        setattr(m, name, v)
        with pytest.raises(ValueError, match='repetition_penalty.*' + name):
            m._check_penalties()
        setattr(m, name, 0)
    m.repetition_penalty = 1.0
    for key, v in (('presence_penalty', 0.5), ('frequency_penalty', 0.25)):
        setattr(m, key, v)
        assert m._check_penalties() is not None
        with pytest.raises(ValueError, match=key):
            m._check_penalties(True)
        m.no_repeat_ngram_size = 2
        with pytest.raises(ValueError, match=key):
            m._check_penalties()
        m.no_repeat_ngram_size = 0
        setattr(m, key, 0.0)
    m.frequency_penalty = -1.0
    with pytest.raises(ValueError, match='frequency_penalty'):
        m._penalties()


def test_penalties_are_refused_on_lstm_decoders_and_copy_models():
    from tell_amd.build import build_model
    from tell_amd.models.pointer import TransformerPointerModel
    from tell_amd.models.transformer import CaptionModel
    lstm = _shell(CaptionModel, torch.nn.Linear(2, 2))       # a decoder without project_contexts: the LSTM decoders
    ptr = _shell(TransformerPointerModel, _Dyn())
    for m in (lstm, ptr):
        assert m._check_penalties() is None
        for key, v, d in zip(KEYS, (1.5, 0.5, 0.5), (1.0, 0.0, 0.0)):
            setattr(m, key, v)
            with pytest.raises(ValueError, match=key):
                m._check_penalties()
            setattr(m, key, d)
    kw = dict(vocab_size=600, dim=64, heads=4, ffn=128, cutoff=(100, 300))
    for key, v in zip(KEYS, (1.5, 0.5, 0.5)):
        with pytest.raises(ValueError, match=key):
            _builders()['baseline_glove'](**{key: v})
        for kind in ('pointer', 'pointer_2'):
            with pytest.raises(ValueError, match=key):
                build_model(kind, object(), object(), n_bert_layers=3, **{key: v}, **kw)


def test_stepper_refuses_what_the_models_refuse():
    from tell_amd.models.stepper import DecodeStepper
    for kw, name in ((dict(ban=(3, 0, 2)), 'no_repeat_ngram_size'), (dict(attention=True), 'attention'),
                     (dict(sample=(0, 1.0, 0.9)), 'sampling_topp'), (dict(sample=(0, 1.0, 0.1, 'minp')), 'sampling_minp')):
        with pytest.raises(ValueError, match='repetition_penalty.*' + name):
            DecodeStepper(None, 4, None, None, 10, pen=(1.2, 0.0, 0.0), **kw)


@pytest.mark.parametrize('kind', ['faces_objects', 'flattened', 'transformer_glove', 'baseline_glove'])
def test_every_model_takes_the_keys(kind):
    make = _builders()[kind]
    m = make()
    assert (m.repetition_penalty, m.presence_penalty, m.frequency_penalty) == (1.0, 0.0, 0.0)
    if kind == 'baseline_glove':
        return
    assert m._penalties() is None
    m = make(repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=0.1)
    assert m._penalties() == (1.2, 0.5, 0.1)
    assert make(sampling_topk=8, sampling_temp=0.9, frequency_penalty=0.1)._penalties() == (1.0, 0.0, 0.1)
    for bad, name in ((dict(repetition_penalty=0.9), 'repetition_penalty'), (dict(presence_penalty=-0.1), 'presence_penalty'),
                      (dict(frequency_penalty=float('inf')), 'frequency_penalty'),
                      (dict(repetition_penalty=1.2, no_repeat_ngram_size=3), 'no_repeat_ngram_size'),
                      (dict(presence_penalty=0.2, min_len=3), 'min_len'),
                      (dict(frequency_penalty=0.2, sampling_topk=0, sampling_topp=0.9), 'sampling_topp'),
                      (dict(frequency_penalty=0.2, sampling_topk=0, sampling_minp=0.1), 'sampling_minp'),
                      (dict(repetition_penalty=1.1, sampling_topk=0, sampling_typical=0.9), 'sampling_typical')):
        with pytest.raises(ValueError, match=name):
            make(**bad)


def test_constructor_keys_and_defaults():
    from tell_amd.build import build_model
    from tell_amd.models.baseline_glove import BaselineGloveModel, TransformerGloveModel
    from tell_amd.models.pointer import PointerModelBase
    from tell_amd.models.stepper import DecodeStepper
    from tell_amd.models.transformer import CaptionModel
    from tell_amd.modules.softmax import AdaptiveSoftmax
    for cls in (CaptionModel, TransformerGloveModel, PointerModelBase, BaselineGloveModel):
        p = inspect.signature(cls.__init__).parameters
        assert tuple(p[k].default for k in KEYS) == (1.0, 0.0, 0.0), cls
    p = inspect.signature(build_model).parameters
    assert tuple(p[k].default for k in KEYS) == (1.0, 0.0, 0.0)
    assert inspect.signature(DecodeStepper.__init__).parameters['pen'].default is None
    assert hasattr(DecodeStepper, 'pen_source')
    for fn in (AdaptiveSoftmax.topk, AdaptiveSoftmax.sample):
        assert inspect.signature(fn).parameters['pen'].default is None


@pytest.mark.parametrize('kind', ['flattened', 'faces_objects'])
def test_yaml_config_with_the_keys(tmp_path, kind):
    from tell_amd import config
    path = _write_cfg(tmp_path, kind)
    model, _ = config.from_config(path, overrides='{"model": {"repetition_penalty": 1.2, "frequency_penalty": 0.1}}',
                                  resnet=object(), roberta=object())
    assert model._penalties() == (1.2, 0.0, 0.1)
    model, _ = config.from_config(path, overrides='{"model": {"sampling_topk": 8, "presence_penalty": 0.5}}',
                                  resnet=object(), roberta=object())
    assert model._penalties() == (1.0, 0.5, 0.0) and model._sampling() == (8, 1.0)
    model, _ = config.from_config(path, resnet=object(), roberta=object())
    assert model._penalties() is None
    for over in ('{"model": {"repetition_penalty": 0.5}}', '{"model": {"presence_penalty": -1}}',
                 '{"model": {"frequency_penalty": "x"}}', '{"model": {"repetition_penalty": 1.2, "no_repeat_ngram_size": 3}}',
                 '{"model": {"repetition_penalty": 1.2, "sampling_topk": 0, "sampling_topp": 0.9}}'):
        with pytest.raises(ValueError):
            config.from_config(path, overrides=over, resnet=object(), roberta=object())


def test_symbols_declared_and_exported():
    import tell_amd
    protos = tell_amd.hip.parse_header()
    _, _, ban = protos['tell_decode_ban_list']
    _, _, cnt = protos['tell_decode_token_counts']
    assert cnt == ban[:ban.index('ngram')] + ['pen_tok', 'pen_cnt', 'ld_pen', 'n_pen', 'stream']
    lists = ['pen_tok', 'pen_cnt', 'ld_pen', 'n_pen', 'theta', 'sub', 'n_sub']
    _, _, topk = protos['tell_adaptive_logprob_topk']
    _, _, pen = protos['tell_adaptive_logprob_topk_penalised']
    assert pen == topk[:topk.index('tokens')] + lists + ['tokens', 'lps', 'stream']
    _, _, smp = protos['tell_adaptive_logprob_sample']
    _, _, spen = protos['tell_adaptive_logprob_sample_penalised']
    assert spen == smp[:smp.index('tokens')] + lists + ['tokens', 'lps', 'stream']
    lib = tell_amd.hip.lib()
    for name in ('tell_decode_token_counts', 'tell_adaptive_logprob_topk_penalised', 'tell_adaptive_logprob_sample_penalised'):
        assert hasattr(lib, name)


# --------------------------------------------------------------------------- the definitions on the oracle
def test_definition_at_the_defaults_is_the_oracle(small):  # noqa: F811
    from oracle.beam import beam_search
    om, start, ctx = small
    c = lambda: {k: v.clone() for k, v in ctx.items()}       # noqa: E731
    for K in (4, 2):
        ref_ids, ref_score = beam_search(om, start, c(), K, gen_len=GEN)
        ids, scores, _ = beam_search_pen(om, start, c(), K, gen_len=GEN)
        assert torch.equal(ids[:, 0], ref_ids) and torch.equal(scores[:, 0], ref_score), K
        assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    ref_lp, ref_ids, _ = om._generate(start, c(), gen_len=GEN)
    ids, s = greedy_pen(om, start, c(), gen_len=GEN)
    assert torch.equal(ids, ref_ids)
    assert torch.allclose(s, ref_lp, rtol=0, atol=1e-5)      # (the oracle greedy decodes incrementally, this one re-decodes)


def test_penalties_change_the_oracles_own_output(small):  # noqa: F811
    om, start, ctx = small
    c = lambda: {k: v.clone() for k, v in ctx.items()}       # noqa: E731
    plain, _ = greedy_pen(om, start, c(), gen_len=GEN)
    got, s = greedy_pen(om, start, c(), gen_len=GEN, pen=PEN)
    # non-vacuity: left alone, this decoder repeats tokens; under the penalties it decodes something else with fewer repeats
    assert repeats(plain) > 0
    assert not torch.equal(got[:, :min(got.shape[1], plain.shape[1])], plain[:, :min(got.shape[1], plain.shape[1])]) \
        or got.shape != plain.shape
    assert repeats(got) < repeats(plain)
    assert bool((s <= 0).all())
    # each control alone moves the decode as well
    for pen in ((PEN[0], 0.0, 0.0), (1.0, PEN[1], 0.0), (1.0, 0.0, PEN[2])):
        one, _ = greedy_pen(om, start, c(), gen_len=GEN, pen=pen)
        assert repeats(one) <= repeats(plain)
    # beam search under the penalties: sorted, and different from the plain search
    b0, _, _ = beam_search_pen(om, start, c(), 4, gen_len=GEN)
    b1, sc, tok_s = beam_search_pen(om, start, c(), 4, gen_len=GEN, pen=PEN)
    assert bool((sc[:, :-1] >= sc[:, 1:]).all())
    flat = lambda t: t.reshape(-1, t.shape[-1])              # noqa: E731  (all K hypotheses of every sample)
    assert b0.shape != b1.shape or not torch.equal(b0, b1)
    assert repeats(flat(b0)) > 0 and repeats(flat(b1)) < repeats(flat(b0))
    assert torch.allclose(tok_s.sum(-1), sc, rtol=1e-5, atol=1e-5)
