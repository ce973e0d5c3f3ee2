"""Vocabulary masks of the cached generators: a list of suppressed tokens, a banned vocabulary per
request, and grounding - tokens of a class may be generated only if they occur in the row's own article.  The plain
definitions live here as test code - `vocab_mask`, `beam_search_masked` / `greedy_masked` (test_beam_options_host.py's
beam_search_opts with the mask applied beside ban_set) - and are what tests/test_gpu_vocab_mask.py holds the kernels and the
generators to.  This file needs no GPU: the definitions on examples, the class of capitalised BPE pieces, check_vocab_mask,
every refused combination, the constructor / config keys, the exported symbols and the definitions on the oracle."""
import inspect
import types

import numpy as np
import pytest
import torch

from test_abi_and_host import _write_cfg
from test_beam_options_host import _Dyn, _shell, ban_set, inv_norm, repeats_ngram, small  # noqa: F401  (`small`: fixture)
from test_sampling_host import _builders


# --------------------------------------------------------------------------- the definitions
def vocab_mask(ctx_row, cls, deny, eos, vocab, pad=1):
    """The mask of one image as uint32 words, bit (t & 31) of word t >> 5 set = token t may not be picked:
    deny | (cls & ~present) with eos cleared.  present: the ids of ctx_row, without pad, negative ids and ids >= vocab.
    cls / deny: bool [vocab] or None.  Bits past `vocab` in the last word are 0."""
    present = np.zeros(vocab, dtype=bool)
    for t in (int(t) for t in ctx_row):
        if 0 <= t < vocab and t != pad:
            present[t] = True
    m = np.zeros(vocab, dtype=bool)
    if cls is not None:
        m |= np.asarray(cls, dtype=bool) & ~present
    if deny is not None:
        m |= np.asarray(deny, dtype=bool)
    if 0 <= eos < vocab:
        m[eos] = False
    words = np.zeros((vocab + 31) // 32, dtype=np.uint32)
    t = np.nonzero(m)[0]
    np.bitwise_or.at(words, t >> 5, np.uint32(1) << (t & 31).astype(np.uint32))
    return words


def mask_bools(words, vocab):
    """uint32 words -> bool [vocab]."""
    t = np.arange(vocab)
    return ((np.asarray(words, dtype=np.uint32)[t >> 5] >> (t & 31).astype(np.uint32)) & 1).astype(bool)


@torch.no_grad()
def beam_search_masked(model, caption_ids, contexts, beam_size, masks, gen_len=100, eos=2, alpha=0.0, ngram=0, min_len=0):
    """test_beam_options_host.beam_search_opts with a vocabulary mask: a masked token of a live hypothesis has score -inf,
    every other log-prob is untouched; hypothesis j of sample b reads masks[b] (bool [B, V]).
    -> (ids [B, K, L], scores [B, K]) best first."""
    B, K, pad = caption_ids.shape[0], beam_size, model.padding_idx
    masks = torch.as_tensor(np.asarray(masks), dtype=torch.bool)
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
        lp = lp.masked_fill(masks.view(B, 1, V), float('-inf'))
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


def greedy_masked(model, caption_ids, contexts, masks, gen_len=100, eos=2, ngram=0, min_len=0):
    """The greedy decode under a vocabulary mask: one hypothesis.  -> (ids [B, L], scores [B])."""
    ids, sc = beam_search_masked(model, caption_ids, contexts, 1, masks, gen_len, eos, ngram=ngram, min_len=min_len)
    return ids[:, 0], sc[:, 0]


def outside(ids, cls, articles, pad=1, eos=2):
    """How many generated tokens (column 0, <s>, aside) are class tokens that do not occur in their row's article.
    ids [B, L] or [B, n, L]; articles: one id sequence per sample."""
    ids = np.asarray(ids)
    B = len(articles)
    rows = ids.reshape(B, -1, ids.shape[-1])
    n = 0
    for b in range(B):
        have = set(int(t) for t in articles[b])
        for row in rows[b]:
            n += sum(1 for t in row[1:] if int(t) not in (pad, eos) and bool(cls[int(t)]) and int(t) not in have)
    return n


# --------------------------------------------------------------------------- hand-made examples
def test_vocab_mask_examples():
    V, eos = 70, 2
    cls = np.zeros(V, dtype=bool)
    cls[[2, 5, 6, 40, 69]] = True                            # eos is in the class
    deny = np.zeros(V, dtype=bool)
    deny[[2, 7, 6]] = True                                   # ... and denied
    ctx = [0, 5, 1, 1, 40, -3, 70, 700, 40, 2, 1]           # pad, a negative id, ids >= vocab, a duplicate
    got = mask_bools(vocab_mask(ctx, cls, deny, eos, V), V)
    assert sorted(np.nonzero(got)[0].tolist()) == [6, 7, 69]     # 5 and 40 are present; 6 denied; 69 absent; eos never set
    words = vocab_mask(ctx, cls, deny, eos, V)
    assert words.dtype == np.uint32 and words.shape == (3,)
    assert int(words[2]) >> (V & 31) == 0                    # the tail bits of the last word are zero
    assert int(words[2]) == 1 << (69 & 31) and int(words[0]) == (1 << 6) | (1 << 7)
    # pad is ignored as an article token: a class that holds pad keeps it masked however often the article holds it
    cls2 = np.zeros(V, dtype=bool)
    cls2[[1, 9]] = True
    assert np.nonzero(mask_bools(vocab_mask([1, 1, 9], cls2, None, eos, V), V))[0].tolist() == [1]
    # no class: the mask is the denied set without eos; nothing at all: all zero
    assert np.nonzero(mask_bools(vocab_mask(ctx, None, deny, eos, V), V))[0].tolist() == [6, 7]
    assert not vocab_mask(ctx, None, None, eos, V).any()
    full = vocab_mask([], np.ones(64, dtype=bool), None, eos, 64)        # a whole number of words: no tail to clear
    assert full.tolist() == [0xFFFFFFFF & ~(1 << eos), 0xFFFFFFFF]


def test_pack_mask_bits_is_the_definitions_layout():
    from tell_amd.ops import pack_mask_bits
    rng = np.random.default_rng(0)
    for V in (69, 64, 600, 50265):
        flags = rng.random(V) < 0.5
        want = vocab_mask([], None, flags, -1, V)
        got = pack_mask_bits(torch.from_numpy(flags))
        assert got.dtype == torch.int32 and got.shape == ((V + 31) // 32,)
        assert np.array_equal(got.numpy().view(np.uint32), want)
    two = pack_mask_bits(torch.from_numpy(np.stack([rng.random(69) < 0.5, np.zeros(69, dtype=bool)])))
    assert two.shape == (2, 3) and not bool(two[1].any())


def _toy_bpe():
    from tell_amd.data.bpe import ByteBPE, FairseqDictionary
    pieces = ['ĠParis', 'Paris', 'Ġparis', 'aris', 'P', 'Ġ', 'Ġ1', '.', 'ĠÃī', 'ĠÃ©']       # (the last two: ' É' and ' é')
    bpe = ByteBPE({p: i for i, p in enumerate(pieces)}, [])
    d = FairseqDictionary([str(i) for i in range(len(pieces))] + ['madeupword0000', '77'])
    return types.SimpleNamespace(bpe=bpe, source_dictionary=d), pieces


def test_capitalised_tokens_on_a_toy_vocabulary():
    from tell_amd.data.bpe import capitalised_tokens
    both, pieces = _toy_bpe()
    cls = capitalised_tokens(both)
    assert cls.dtype == torch.bool and cls.shape == (len(both.source_dictionary),)
    assert not bool(cls[:4].any())                           # <s> <pad> </s> <unk>
    got = {pieces[i - 4] for i in np.nonzero(cls.numpy())[0]}
    assert got == {'ĠParis', 'Paris', 'P', 'ĠÃī'}
    for out in ('Ġparis', 'aris', 'Ġ', 'Ġ1', '.', 'ĠÃ©'):    # per token: the continuation piece 'aris' is outside the class
        assert not bool(cls[4 + pieces.index(out)])
    assert not bool(cls[-2:].any())                          # entries that are no BPE id of the encoder
    assert torch.equal(capitalised_tokens(both.bpe, both.source_dictionary), cls)
    assert 'per token' in capitalised_tokens.__doc__.lower()


def test_name_tokens_raises_without_the_vocabulary_files(monkeypatch, tmp_path):
    from tell_amd.data import indexers
    from tell_amd.models.transformer import CaptionModel
    m = _shell(CaptionModel, _Dyn())
    monkeypatch.setattr(indexers, 'bpe_directory', lambda *a, **k: str(tmp_path))
    with pytest.raises(FileNotFoundError):
        m.name_tokens()


# --------------------------------------------------------------------------- check_vocab_mask
def test_check_vocab_mask():
    from tell_amd.models.transformer import MIN_ALLOWED_TOKENS, check_vocab_mask
    V, B = 600, 3
    assert MIN_ALLOWED_TOKENS == 64
    assert check_vocab_mask(None, None, V, B) == (None, None)
    banned = torch.zeros(V, dtype=torch.bool)
    banned[[5, 9]] = True
    deny, cls = check_vocab_mask(banned, None, V, B)
    assert cls is None and deny.shape == (1, V) and deny.sum() == 2
    rows = torch.zeros(B, V, dtype=torch.bool)
    rows[1, 7] = True
    ground = torch.zeros(V, dtype=torch.bool)
    ground[[2, 300]] = True
    deny, cls = check_vocab_mask(rows, ground, V, B, suppress=(11,))
    assert deny.shape == (B, V) and bool(deny[:, 11].all()) and bool(deny[1, 7]) and not bool(rows[:, 11].any())
    assert cls.sum() == 1 and not bool(cls[2]) and bool(ground[2])           # eos leaves the class; the argument is left alone
    deny, cls = check_vocab_mask(None, None, V, B, suppress=(4, 8))
    assert deny.shape == (1, V) and deny.sum() == 2 and cls is None
    for bad in (banned.to(torch.uint8), banned[:-1], torch.zeros(B + 1, V, dtype=torch.bool), banned.view(1, 1, V), [0, 1], 1.0):
        with pytest.raises(ValueError, match='banned'):
            check_vocab_mask(bad, None, V, B)
    for bad in (ground.float(), ground[:-1], torch.zeros(B, V, dtype=torch.bool), 'names', 3):
        with pytest.raises(ValueError, match='ground'):
            check_vocab_mask(None, bad, V, B)
    eos_banned = banned.clone()
    eos_banned[2] = True
    with pytest.raises(ValueError, match='banned.*</s>'):
        check_vocab_mask(eos_banned, None, V, B)
    with pytest.raises(ValueError, match='suppress_tokens'):
        check_vocab_mask(None, None, V, B, suppress=(2,))
    with pytest.raises(ValueError, match='suppress_tokens'):
        check_vocab_mask(None, None, V, B, suppress=(V,))
    # fewer than 64 allowed tokens in any row: 63 raises, 64 passes
    tight = torch.ones(B, V, dtype=torch.bool)
    tight[:, 2] = False
    tight[:, 100:163] = False                                # 64 allowed with eos
    assert check_vocab_mask(tight, None, V, B)[0] is not None
    tight[1, 100] = True                                     # row 1: 63
    with pytest.raises(ValueError, match='banned.*63'):
        check_vocab_mask(tight, None, V, B)
    wide = torch.ones(V, dtype=torch.bool)
    wide[:64] = False                                        # complement: 64 tokens (eos among them)
    assert check_vocab_mask(None, wide, V, B)[1] is not None
    wide[63] = True
    with pytest.raises(ValueError, match='ground.*63'):
        check_vocab_mask(None, wide, V, B)


def test_check_vocab_mask_counts_the_union_of_banned_and_ground():
    from tell_amd.models.transformer import check_vocab_mask
    V = 600
    a, b = torch.zeros(V, dtype=torch.bool), torch.zeros(V, dtype=torch.bool)
    a[3:300], b[300:536] = True, True                        # 600 - 297 - 236 = 67 allowed
    check_vocab_mask(a, b, V, 2)
    b[536:540] = True                                        # 63
    with pytest.raises(ValueError, match='banned.*63'):
        check_vocab_mask(a, b, V, 2)


def test_check_mask_keys():
    from tell_amd.models.transformer import check_mask_keys
    assert check_mask_keys() == ((), False)
    assert check_mask_keys([9, 4, 9], True) == ((4, 9), True)
    assert check_mask_keys(None, False) == ((), False)
    for bad in (5, 'x', [1.5], [-1], [True], {3}):
        with pytest.raises(ValueError, match='suppress_tokens'):
            check_mask_keys(bad)
    for bad in (1, 'yes', None):
        with pytest.raises(ValueError, match='ground_names'):
            check_mask_keys((), bad)


# --------------------------------------------------------------------------- refused combinations
def _on(m, key):
    if key == 'suppress_tokens':
        m.suppress_tokens = (7,)
    elif key == 'ground_names':
        m.ground_names = True
    return {'banned': dict(banned=torch.zeros(600, dtype=torch.bool)), 'ground': dict(ground=True)}.get(key, {})


def _off(m):
    m.suppress_tokens, m.ground_names = (), False


MASK_KEYS = ('banned', 'ground', 'suppress_tokens', 'ground_names')


def test_refused_combinations():
    from tell_amd.models.transformer import CaptionModel
    m = _shell(CaptionModel, _Dyn())
    assert m._mask_options() == [] and m._check_mask_options() == []         # the defaults: nothing set, nothing checked
    assert m._vocab_mask({'roberta': None}) is None                           # ... and nothing of the batch is read
    for key in MASK_KEYS:
        kw = _on(m, key)
        assert m._check_mask_options(**kw) == [key]
        m.sampling_topk = 8                                                   # top-k sampling: in scope
        assert m._check_mask_options(**kw) == [key]
        m.sampling_topk = 1
        m.no_repeat_ngram_size, m.min_len, m.beam_len_penalty = 2, 3, 1.0     # the search options: in scope
        assert m._check_mask_options(**kw) == [key]
        m.no_repeat_ngram_size, m.min_len, m.beam_len_penalty = 0, 0, 0.0
        with pytest.raises(ValueError, match=key + '.*attention'):
            m._check_mask_options(attention=True, **kw)
        for name, v in (('sampling_topp', 0.9), ('sampling_minp', 0.1), ('sampling_typical', 0.9)):
            setattr(m, name, v)
            with pytest.raises(ValueError, match=key + '.*' + name):
                m._check_mask_options(**kw)
            setattr(m, name, None)
        for name, v, d in (('repetition_penalty', 1.2, 1.0), ('presence_penalty', 0.5, 0.0), ('frequency_penalty', 0.1, 0.0)):
            setattr(m, name, v)
            with pytest.raises(ValueError, match=key + '.*' + name):
                m._check_mask_options(**kw)
            setattr(m, name, d)
        _off(m)
    assert m._check_mask_options(ground=False) == []                          # ground=False is ground=None


def test_masks_are_refused_on_lstm_decoders_and_copy_models():
    from tell_amd.build import build_model
    from tell_amd.models.baseline_glove import BaselineGloveModel, _refuse_mask_options
    from tell_amd.models.pointer import TransformerPointerModel
    from tell_amd.models.transformer import CaptionModel
    lstm = _shell(CaptionModel, torch.nn.Linear(2, 2))       # a decoder without project_contexts: the LSTM decoders
    ptr = _shell(TransformerPointerModel, _Dyn())
    for m in (lstm, ptr):
        assert m._check_mask_options() == []
        for key in MASK_KEYS:
            kw = _on(m, key)
            with pytest.raises(ValueError, match=key):
                m._check_mask_options(**kw)
            with pytest.raises(ValueError, match=key):
                m._vocab_mask({'roberta': torch.zeros(2, 5, dtype=torch.long)}, **kw)
            _off(m)
    glove = BaselineGloveModel.__new__(BaselineGloveModel)
    assert _refuse_mask_options(glove) == ((), False)
    for kw, key in ((dict(suppress_tokens=[5]), 'suppress_tokens'), (dict(ground_names=True), 'ground_names'),
                    (dict(banned=torch.zeros(9, dtype=torch.bool)), 'banned'), (dict(ground=True), 'ground')):
        with pytest.raises(ValueError, match=key):
            _refuse_mask_options(glove, **kw)
    kw = dict(vocab_size=600, dim=64, heads=4, ffn=128, cutoff=(100, 300))
    for key, v in (('suppress_tokens', [5]), ('ground_names', True)):
        with pytest.raises(ValueError, match=key):
            _builders()['baseline_glove'](**{key: v})
        for kind in ('pointer', 'pointer_2'):
            with pytest.raises(ValueError, match=key):
                build_model(kind, object(), object(), n_bert_layers=3, **{key: v}, **kw)
    # the GloVe transformer has no article ids to ground a class in: banned / suppress_tokens only
    with pytest.raises(ValueError, match='ground_names'):
        _builders()['transformer_glove'](ground_names=True)
    g = _builders()['transformer_glove'](suppress_tokens=[5])
    with pytest.raises(ValueError, match='ground'):
        g._check_grounding(True)


def test_stepper_refuses_what_the_models_refuse():
    from tell_amd.models.stepper import DecodeStepper
    for kw, name in ((dict(pen=(1.2, 0.0, 0.0)), 'repetition_penalty'), (dict(attention=True), 'attention'),
                     (dict(sample=(0, 1.0, 0.9)), 'sampling_topp'), (dict(sample=(0, 1.0, 0.1, 'minp')), 'sampling_minp'),
                     (dict(sample=(0, 1.0, 0.9, 'typical')), 'sampling_typical')):
        with pytest.raises(ValueError, match='banned.*' + name):
            DecodeStepper(None, 4, None, None, 10, mask=True, **kw)


# --------------------------------------------------------------------------- the keys
@pytest.mark.parametrize('kind', ['faces_objects', 'flattened', 'transformer_glove', 'baseline_glove'])
def test_every_model_takes_the_keys(kind):
    make = _builders()[kind]
    m = make()
    assert (m.suppress_tokens, m.ground_names) == ((), False)
    if kind == 'baseline_glove':
        return
    assert m._mask_options() == []
    m = make(suppress_tokens=[9, 5])
    assert m.suppress_tokens == (5, 9) and m._mask_options() == ['suppress_tokens']
    if kind != 'transformer_glove':
        m = make(ground_names=True, sampling_topk=8, no_repeat_ngram_size=0)
        assert m.ground_names is True and m._mask_options() == ['ground_names']
    assert make(suppress_tokens=[5], no_repeat_ngram_size=2, min_len=3)._mask_options() == ['suppress_tokens']
    for bad, name in ((dict(suppress_tokens=5), 'suppress_tokens'), (dict(suppress_tokens=[-1]), 'suppress_tokens'),
                      (dict(ground_names='yes'), 'ground_names'),
                      (dict(suppress_tokens=[5], sampling_topk=0, sampling_topp=0.9), 'sampling_topp'),
                      (dict(suppress_tokens=[5], sampling_topk=0, sampling_minp=0.1), 'sampling_minp'),
                      (dict(suppress_tokens=[5], sampling_topk=0, sampling_typical=0.9), 'sampling_typical'),
                      (dict(suppress_tokens=[5], repetition_penalty=1.2), 'repetition_penalty')):
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
        assert (p['suppress_tokens'].default, p['ground_names'].default) == ((), False), cls
    p = inspect.signature(build_model).parameters
    assert (p['suppress_tokens'].default, p['ground_names'].default) == ((), False)
    for fn in (CaptionModel.generate, CaptionModel.generate_lanes, TransformerGloveModel.generate, PointerModelBase.generate,
               BaselineGloveModel.generate):
        p = inspect.signature(fn).parameters
        assert p['banned'].default is None and p['ground'].default is None, fn
    assert inspect.signature(DecodeStepper.__init__).parameters['mask'].default is False
    assert hasattr(DecodeStepper, 'set_mask')
    for fn in (AdaptiveSoftmax.topk, AdaptiveSoftmax.sample, AdaptiveSoftmax.greedy):
        assert inspect.signature(fn).parameters['mask'].default is None


@pytest.mark.parametrize('kind', ['flattened', 'faces_objects'])
def test_yaml_config_with_the_keys(tmp_path, kind):
    from tell_amd import config
    path = _write_cfg(tmp_path, kind)
    model, _ = config.from_config(path, overrides='{"model": {"suppress_tokens": [7, 3], "ground_names": true}}',
                                  resnet=object(), roberta=object())
    assert model.suppress_tokens == (3, 7) and model.ground_names is True
    assert model._mask_options() == ['suppress_tokens', 'ground_names']
    model, _ = config.from_config(path, overrides='{"model": {"sampling_topk": 8, "suppress_tokens": [7]}}',
                                  resnet=object(), roberta=object())
    assert model._mask_options() == ['suppress_tokens'] and model._sampling() == (8, 1.0)
    model, _ = config.from_config(path, resnet=object(), roberta=object())
    assert model._mask_options() == [] and (model.suppress_tokens, model.ground_names) == ((), False)
    for over in ('{"model": {"suppress_tokens": 7}}', '{"model": {"suppress_tokens": [-2]}}',
                 '{"model": {"ground_names": "yes"}}', '{"model": {"ground_names": true, "repetition_penalty": 1.2}}',
                 '{"model": {"suppress_tokens": [7], "sampling_topk": 0, "sampling_topp": 0.9}}'):
        with pytest.raises(ValueError):
            config.from_config(path, overrides=over, resnet=object(), roberta=object())


def test_symbols_declared_and_exported():
    import tell_amd
    protos = tell_amd.hip.parse_header()
    _, _, build = protos['tell_decode_vocab_mask']
    assert build == ['ctx', 'ld_ctx', 'S', 'rows', 'vocab', 'cls_bits', 'deny8', 'ld_deny', 'eos', 'pad', 'mask', 'ld_mask',
                     'stream']
    _, _, topk = protos['tell_adaptive_logprob_topk']
    _, _, banned = protos['tell_adaptive_logprob_topk_banned']
    _, _, msk = protos['tell_adaptive_logprob_topk_masked']
    lists = banned[banned.index('ban'):banned.index('tokens')]
    assert lists == ['ban', 'ld_ban', 'n_ban']
    assert msk == topk[:topk.index('tokens')] + ['mask', 'ld_mask', 'per'] + lists + ['tokens', 'lps', 'stream']
    _, _, smp = protos['tell_adaptive_logprob_sample']
    _, _, smsk = protos['tell_adaptive_logprob_sample_masked']
    assert smsk == smp[:smp.index('tokens')] + ['mask', 'ld_mask', 'per', 'tokens', 'lps', 'stream']
    lib = tell_amd.hip.lib()
    for name in ('tell_decode_vocab_mask', 'tell_adaptive_logprob_topk_masked', 'tell_adaptive_logprob_sample_masked'):
        assert hasattr(lib, name)
    header = open(tell_amd.hip.HEADER_PATH).read()
    for phrase in ('nothing is\n *     renormalised', 'lower id first', 'r / per', 'deny[b] | (cls & ~present[b])'):
        assert phrase in header, phrase


# --------------------------------------------------------------------------- the definitions on the oracle
GEN, SEED, ART = 24, 0, 12


def _articles(B, V, seed=SEED, n=ART):
    """Short random "articles": n ids per row, with a pad and an id outside the vocabulary among them."""
    rng = np.random.default_rng(seed)
    art = rng.integers(4, V, (B, n))
    art[:, -1] = 1
    art[:, -2] = V + 5
    return art


def _setup(small_fx):
    om, start, ctx = small_fx
    V = 600
    B = start.shape[0]
    cls = np.zeros(V, dtype=bool)
    cls[0::2] = True                                         # every second token id
    art = _articles(B, V)
    masks = np.stack([mask_bools(vocab_mask(art[b], cls, None, 2, V), V) for b in range(B)])
    return om, start, ctx, cls, art, masks


def test_an_all_zero_mask_is_the_oracle(small):  # noqa: F811
    from oracle.beam import beam_search
    om, start, ctx = small
    c = lambda: {k: v.clone() for k, v in ctx.items()}       # noqa: E731
    zero = np.zeros((start.shape[0], 600), dtype=bool)
    for K in (4, 2):
        ref_ids, ref_score = beam_search(om, start, c(), K, gen_len=GEN)
        ids, scores = beam_search_masked(om, start, c(), K, zero, gen_len=GEN)
        assert torch.equal(ids[:, 0], ref_ids) and torch.equal(scores[:, 0], ref_score), K
    _, ref_ids, _ = om._generate(start, c(), gen_len=GEN)
    ids, _ = greedy_masked(om, start, c(), zero, gen_len=GEN)
    assert torch.equal(ids, ref_ids)


def test_grounding_changes_the_oracles_own_output(small):  # noqa: F811
    om, start, ctx, cls, art, masks = _setup(small)
    c = lambda: {k: v.clone() for k, v in ctx.items()}       # noqa: E731
    zero = np.zeros_like(masks)
    assert int((~masks).sum(1).min()) >= 64                  # what check_vocab_mask asks of every row
    # non-vacuity (the seed of _articles is chosen for it): left alone, greedy and beam 4 emit class tokens outside the article
    g0, _ = greedy_masked(om, start, c(), zero, gen_len=GEN)
    b0, _ = beam_search_masked(om, start, c(), 4, zero, gen_len=GEN)
    assert outside(g0, cls, art) > 0 and outside(b0, cls, art) > 0
    g1, _ = greedy_masked(om, start, c(), masks, gen_len=GEN)
    b1, sc = beam_search_masked(om, start, c(), 4, masks, gen_len=GEN)
    assert outside(g1, cls, art) == 0 and outside(b1, cls, art) == 0
    assert bool((sc[:, :-1] >= sc[:, 1:]).all())
    # with the bigram ban as well: no bigram repeats and no masked token appears
    b2, _ = beam_search_masked(om, start, c(), 4, masks, gen_len=GEN, ngram=2)
    assert outside(b2, cls, art) == 0
    assert not any(repeats_ngram(h, 2) for b in b2 for h in b)
    g2, _ = greedy_masked(om, start, c(), masks, gen_len=GEN, ngram=2)
    assert outside(g2, cls, art) == 0 and not any(repeats_ngram(h, 2) for h in g2)
