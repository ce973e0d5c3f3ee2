"""Context guidance of the cached generators: classifier-free guidance over chosen contexts.  A step is
decoded twice - with all contexts (lp_c) and with the contexts in `drop` fully masked (lp_u) - and the pick follows
s = lp_c + (gamma - 1) * (lp_c - lp_u), reported as g = s - logsumexp(s).  The plain definitions live here as test code -
`guided_rows`, `greedy_guided` / `beam_search_guided` on the oracle decoder - and are what tests/test_gpu_guidance.py holds
the kernel and the generators to.  This file needs no GPU: known answers, the key and argument checks, every refused
combination, the constructor / config keys, the exported symbol, and non-vacuity and margins of the GPU test's cases."""
import inspect

import numpy as np
import pytest
import torch

from test_abi_and_host import _write_cfg
from test_beam_options_host import _Dyn, _shell, inv_norm, small  # noqa: F401  (`small`: fixture)
from test_sampling_host import _builders

SCORE_TOL = 5e-4                                             # the fp32 score tolerance of DESIGN.md section 16


def margin(gamma):
    """What the best and the second-best s of a row must differ by for a decode to be comparable token by token: ten times
    the score tolerance, amplified as the formula amplifies an error of the two log-probs (1 + |gamma - 1| on lp_c, |gamma - 1|
    on lp_u)."""
    return 10 * (1 + 2 * abs(gamma - 1)) * SCORE_TOL


# --------------------------------------------------------------------------- the definitions
def guided_rows(lp_c, lp_u, gamma):
    """-> (s fp32, L float64, g fp32) over the last axis: d = lp_c - lp_u, t = (gamma - 1) * d, s = lp_c + t - three fp32
    operations rounded one by one, gamma - 1 formed in fp32 -, L = logsumexp(s) (float64, max-shifted), g = s - L."""
    lp_c, lp_u = np.asarray(lp_c, dtype=np.float32), np.asarray(lp_u, dtype=np.float32)
    gm1 = np.float32(np.float32(gamma) - np.float32(1.0))
    d = (lp_c - lp_u).astype(np.float32)
    t = (gm1 * d).astype(np.float32)
    s = (lp_c + t).astype(np.float32)
    s64 = s.astype(np.float64)
    m = s64.max(-1, keepdims=True)
    L = (m + np.log(np.exp(s64 - m).sum(-1, keepdims=True)))
    g = (s64 - L).astype(np.float32)
    return s, L[..., 0], g


def dropped(contexts, drop):
    """The contexts of the unconditional pass: every key-padding mask in `drop` all-masked (the decoder then attends to the
    bias key and the zero key only)."""
    out = {k: v.clone() for k, v in contexts.items()}
    for n in drop:
        out[n + '_mask'] = torch.ones_like(out[n + '_mask'])
    return out


@torch.no_grad()
def beam_search_guided(model, caption_ids, contexts, drop, gamma, beam_size, gen_len=100, eos=2, alpha=0.0, gaps=None):
    """test_vocab_mask_host.beam_search_masked with the guided log-probs g in place of the model's: every hypothesis is decoded
    on `contexts` and on dropped(contexts, drop), its candidates are scored cum + g.  gaps: a list that receives, per step, the
    smallest difference between the best and the second-best s over the live hypotheses that count (cum > -inf).
    -> (ids [B, K, L], scores [B, K]) best first."""
    B, K, pad = caption_ids.shape[0], beam_size, model.padding_idx
    ctx_c, ctx_u = {}, {}
    for name, val in contexts.items():
        ctx_c[name] = val.repeat_interleave(K, dim=0 if name.endswith('_mask') else 1)
    for name, val in dropped(contexts, drop).items():
        ctx_u[name] = val.repeat_interleave(K, dim=0 if name.endswith('_mask') else 1)
    seqs = caption_ids[:, 0:1].repeat_interleave(K, dim=0).view(B, K, 1)
    cum = torch.full((B, K), float('-inf'))
    cum[:, 0] = 0.0
    finished = seqs[:, :, 0] == eos
    length = torch.zeros(B, K, dtype=torch.long)
    table = torch.from_numpy(inv_norm(alpha, gen_len + 1))

    def rows(ctx):
        out = model.decoder({model.index: seqs.view(B * K, -1)}, {k: v.clone() for k, v in ctx.items()}, incremental_state=None)
        return model.decoder.get_normalized_probs((out[0][:, -1:], None), log_probs=True).view(B, K, -1).float().numpy()
    for i in range(gen_len):
        s, _, g = guided_rows(rows(ctx_c), rows(ctx_u), gamma)
        if gaps is not None:
            top2 = np.sort(s, -1)[..., -2:]
            live = (~finished & (cum > float('-inf'))).numpy()
            gaps.append(float((top2[..., 1] - top2[..., 0])[live].min()) if live.any() else float('inf'))
        lp = torch.from_numpy(g)
        V = lp.shape[-1]
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


def greedy_guided(model, caption_ids, contexts, drop, gamma, gen_len=100, eos=2, gaps=None):
    """The guided greedy decode: one hypothesis.  -> (ids [B, L], scores [B])."""
    ids, sc = beam_search_guided(model, caption_ids, contexts, drop, gamma, 1, gen_len, eos, gaps=gaps)
    return ids[:, 0], sc[:, 0]


# --------------------------------------------------------------------------- known answers by hand
def _two_rows(V=97, seed=0):
    rng = np.random.default_rng(seed)
    lp = []
    for _ in range(2):
        x = rng.normal(size=(3, V)).astype(np.float32) * 3
        x = x - np.log(np.exp(x.astype(np.float64)).sum(-1, keepdims=True))
        lp.append(x.astype(np.float32))
    return lp


def test_gamma_one_is_the_conditional_row_bit_for_bit():
    lp_c, lp_u = _two_rows()
    s, L, g = guided_rows(lp_c, lp_u, 1.0)
    assert np.array_equal(s.view(np.uint32), lp_c.view(np.uint32))
    assert np.abs(L).max() < 1e-6                            # a log-prob row is normalised already
    np.testing.assert_allclose(g, lp_c, rtol=0, atol=2e-6)


def test_equal_rows_give_the_conditional_row_for_every_gamma():
    lp_c, _ = _two_rows()
    for gamma in (0.0, 0.5, 1.5, 3.0, 7.5):
        s, _, _ = guided_rows(lp_c, lp_c.copy(), gamma)
        assert np.array_equal(s.view(np.uint32), lp_c.view(np.uint32)), gamma


def test_gamma_zero_is_the_unconditional_row():
    lp_c, lp_u = _two_rows()
    s, L, g = guided_rows(lp_c, lp_u, 0.0)
    np.testing.assert_allclose(s, lp_u, rtol=0, atol=4e-6)   # lp_c - (lp_c - lp_u): two roundings at |lp| < 32
    np.testing.assert_allclose(g, lp_u, rtol=0, atol=8e-6)


def test_a_small_example_by_hand():
    lp_c = np.log(np.array([[0.5, 0.25, 0.25]]))
    lp_u = np.log(np.array([[0.25, 0.5, 0.25]]))
    s, L, g = guided_rows(lp_c, lp_u, 2.0)                   # p_c ** 2 / p_u = 1, 1/8, 1/4 -> normalised by 11/8
    np.testing.assert_allclose(np.exp(s[0].astype(np.float64)), [1.0, 0.125, 0.25], rtol=1e-6)
    np.testing.assert_allclose(L, [np.log(11 / 8)], rtol=1e-6)
    np.testing.assert_allclose(np.exp(g[0].astype(np.float64)), np.array([8, 1, 2]) / 11, rtol=1e-6)
    assert margin(1.0) == 10 * SCORE_TOL and margin(3.0) == 50 * SCORE_TOL and margin(0.0) == 30 * SCORE_TOL


# --------------------------------------------------------------------------- keys and arguments
def test_check_guidance():
    from tell_amd.models.transformer import GUIDANCE_CONTEXTS, check_guidance
    assert GUIDANCE_CONTEXTS == ('image', 'article', 'faces', 'obj')
    assert check_guidance() == (1.0, ('image',))
    assert check_guidance(3, ['obj', 'image']) == (3.0, ('image', 'obj'))          # the names in context order
    assert check_guidance(0, 'article') == (0.0, ('article',))
    assert check_guidance(0.5, ('faces', 'faces')) == (0.5, ('faces',))
    for bad in ((), [], None, 5, [5], ['image', None]):                            # an empty drop, not a list of names
        with pytest.raises(ValueError, match='guidance_drop'):
            check_guidance(2.0, bad)
    for bad in (['caption'], ['image', 'objects'], ['Image']):                     # an unknown name
        with pytest.raises(ValueError, match='guidance_drop.*unknown'):
            check_guidance(2.0, bad)
    for bad in (-0.1, -1, float('inf'), float('-inf'), float('nan'), 'x', None, True, [2.0]):
        with pytest.raises(ValueError, match='guidance_scale'):
            check_guidance(bad)


class _Layer(torch.nn.Module):
    def __init__(self, names):
        super().__init__()
        self.context_names = list(names)


class _DynNamed(_Dyn):
    """A DynamicConv decoder as far as the checks look: project_contexts and the context names of its layers."""

    def __init__(self, names=('image', 'article')):
        super().__init__()
        self.layers = torch.nn.ModuleList([_Layer(names)])


def test_arguments_of_a_call():
    from tell_amd.models.transformer import CaptionModel
    m = _shell(CaptionModel, _DynNamed())
    assert m._check_guidance() is None                       # the defaults (no keys on the shell): off
    assert m._check_guidance(1.0) is None and m._check_guidance(1) is None
    assert m._check_guidance(3.0) == (('image',), 3.0)
    assert m._check_guidance(0.0, ['article', 'image']) == (('image', 'article'), 0.0)
    m.guidance_scale, m.guidance_drop = 2.0, ('article',)
    assert m._check_guidance() == (('article',), 2.0)        # None reads the model's keys
    assert m._check_guidance(1.0) is None                    # ... and an argument overrides them
    assert m._check_guidance(guidance_drop=['image']) == (('image',), 2.0)
    for drop in (['faces'], ['obj', 'image']):               # a context this decoder lacks, guidance on or off
        with pytest.raises(ValueError, match='guidance_drop.*no context'):
            m._check_guidance(3.0, drop)
        with pytest.raises(ValueError, match='guidance_drop.*no context'):
            m._check_guidance(1.0, drop)
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='guidance_scale'):
            m._check_guidance(bad)
    with pytest.raises(ValueError, match='guidance_drop'):
        m._check_guidance(3.0, [])
    with pytest.raises(ValueError, match='unknown'):
        m._check_guidance(3.0, ['text'])
    four = _shell(CaptionModel, _DynNamed(('image', 'article', 'faces', 'obj')))
    assert four._check_guidance(1.5, ['image', 'faces', 'obj']) == (('image', 'faces', 'obj'), 1.5)


def test_guided_batch_doubles_the_images_and_masks_the_dropped_contexts():
    from tell_amd.models.transformer import guided_batch
    B, S, E = 3, 5, 4
    x = torch.randn(B, S, E)
    ctx = {'image': x.transpose(0, 1), 'image_mask': torch.zeros(B, S, dtype=torch.bool),
           'article': torch.randn(7, B, E), 'article_mask': torch.arange(7)[None, :] >= torch.tensor([[7], [3], [5]])}
    ids = torch.tensor([[0], [0], [0]])
    ids2, out = guided_batch(ids, ctx, ('image',))
    assert ids2.shape == (2 * B, 1) and out['image'].shape == (S, 2 * B, E) and out['article'].shape == (7, 2 * B, E)
    assert torch.equal(out['image'][:, :B], ctx['image']) and torch.equal(out['image'][:, B:], ctx['image'])
    assert out['image'].transpose(0, 1).is_contiguous()      # a [S, B, E] view of [B, S, E] storage, like the encoders' output
    assert torch.equal(out['image_mask'][:B], ctx['image_mask']) and bool(out['image_mask'][B:].all())
    assert out['image_mask'].dtype == torch.bool
    assert torch.equal(out['article_mask'], torch.cat([ctx['article_mask']] * 2, 0))
    u8 = dict(ctx, article_mask=ctx['article_mask'].to(torch.uint8))
    _, out = guided_batch(ids, u8, ('article', 'image'))
    assert out['article_mask'].dtype == torch.uint8 and bool((out['article_mask'][B:] == 1).all())
    with pytest.raises(ValueError, match='no context'):
        guided_batch(ids, ctx, ('faces',))


# --------------------------------------------------------------------------- refused combinations
def test_refused_combinations():
    from tell_amd.models.transformer import CaptionModel
    m = _shell(CaptionModel, _DynNamed())
    ok = (('image',), 3.0)
    assert m._check_guidance(3.0) == ok
    m.beam_len_penalty = 1.0                                 # the length penalty: in scope
    assert m._check_guidance(3.0) == ok
    m.beam_len_penalty = 0.0
    for name, v, d in (('sampling_topk', 8, 1), ('sampling_topp', 0.9, None), ('sampling_minp', 0.1, None),
                       ('sampling_typical', 0.9, None), ('no_repeat_ngram_size', 2, 0), ('min_len', 3, 0),
                       ('repetition_penalty', 1.2, 1.0), ('presence_penalty', 0.5, 0.0), ('frequency_penalty', 0.1, 0.0),
                       ('suppress_tokens', (7,), ()), ('ground_names', True, False)):
        setattr(m, name, v)
        with pytest.raises(ValueError, match='guidance.*' + name):
            m._check_guidance(3.0)
        assert m._check_guidance(1.0) is None                # off: nothing to refuse
        setattr(m, name, d)
    for kw, name in ((dict(banned=torch.zeros(600, dtype=torch.bool)), 'banned'), (dict(ground=True), 'ground'),
                     (dict(prefix=torch.zeros(2, 3, dtype=torch.long)), 'prefix'), (dict(n_samples=4), 'n_samples'),
                     (dict(attention=True), 'attention')):
        with pytest.raises(ValueError, match='guidance.*' + name):
            m._check_guidance(3.0, **kw)
        assert m._check_guidance(1.0, **kw) is None
    assert m._check_guidance(3.0) == ok


def test_guidance_is_refused_on_lstm_decoders_and_copy_models():
    from tell_amd.build import build_model
    from tell_amd.models.baseline_glove import BaselineGloveModel, _refuse_guidance
    from tell_amd.models.pointer import TransformerPointerModel
    from tell_amd.models.transformer import CaptionModel
    lstm = _shell(CaptionModel, torch.nn.Linear(2, 2))       # a decoder without project_contexts: the LSTM decoders
    ptr = _shell(TransformerPointerModel, _DynNamed())
    for m in (lstm, ptr):
        assert m._check_guidance() is None and m._check_guidance(1.0) is None
        with pytest.raises(ValueError, match='guidance=3.0.*' + type(m).__name__):
            m._check_guidance(3.0)
        with pytest.raises(ValueError, match='guidance'):
            m._generate(torch.zeros(2, 1, dtype=torch.long), {}, guide=(('image',), 3.0))
    glove = BaselineGloveModel.__new__(BaselineGloveModel)
    assert _refuse_guidance(glove) == (1.0, ('image',))
    with pytest.raises(ValueError, match='guidance=2.0.*LSTM'):
        _refuse_guidance(glove, 2.0)
    with pytest.raises(ValueError, match='guidance_scale'):
        _refuse_guidance(glove, -1.0)
    kw = dict(vocab_size=600, dim=64, heads=4, ffn=128, cutoff=(100, 300))
    with pytest.raises(ValueError, match='guidance'):
        _builders()['baseline_glove'](guidance_scale=2.0)
    for kind in ('pointer', 'pointer_2'):
        with pytest.raises(ValueError, match='guidance'):
            build_model(kind, object(), object(), n_bert_layers=3, guidance_scale=2.0, **kw)
        assert build_model(kind, object(), object(), n_bert_layers=3, **kw).guidance_scale == 1.0


def test_stepper_refuses_what_the_models_refuse():
    from tell_amd.models.stepper import DecodeStepper
    for kw, name in ((dict(sample=(8, 1.0)), 'sampling'), (dict(sample=(0, 1.0, 0.9)), 'sampling_topp'),
                     (dict(sample=(0, 1.0, 0.1, 'minp')), 'sampling_minp'), (dict(sample=(0, 1.0, 0.9, 'typical')), 'sampling_typical'),
                     (dict(ban=(2, 0, 2)), 'no_repeat_ngram_size'), (dict(ban=(0, 3, 2)), 'min_len'),
                     (dict(pen=(1.2, 0.0, 0.0)), 'repetition_penalty'), (dict(mask=True), 'banned'), (dict(prefix=True), 'prefix'),
                     (dict(sample=(8, 1.0), hyp=4), 'sampling'), (dict(attention=True), 'attention')):
        with pytest.raises(ValueError, match='guidance.*' + name):
            DecodeStepper(None, 4, None, None, 10, guide=('image',), **kw)
    with pytest.raises(ValueError, match='guidance.*even'):
        DecodeStepper(None, 5, None, None, 10, guide=('image',))


def test_the_head_refuses_guidance_beside_another_list():
    from tell_amd import decode, ops
    x = torch.zeros(4, 8)
    for kw in (dict(topk=0), dict(topk=4, ban=(None, None)), dict(topk=4, force=()), dict(topk=4, pen=()), dict(topk=4, mask=()),
               dict(topk=4, sample=())):
        with pytest.raises(ValueError, match='guidance'):
            ops.adaptive_log_probs(x, [4, 8], None, None, [], guide=(2, None), **kw)
        with pytest.raises(ValueError, match='guidance'):
            decode.head_step(x, [4, 8], None, None, [], guide=(2, None), **kw)


# --------------------------------------------------------------------------- the keys
@pytest.mark.parametrize('kind', ['faces_objects', 'flattened', 'transformer_glove', 'baseline_glove'])
def test_every_model_takes_the_keys(kind):
    make = _builders()[kind]
    m = make()
    assert (m.guidance_scale, m.guidance_drop) == (1.0, ('image',))
    if kind == 'baseline_glove':
        with pytest.raises(ValueError, match='guidance'):
            make(guidance_scale=2.0)
        return
    assert m._check_guidance() is None
    m = make(guidance_scale=2.5, guidance_drop=['article', 'image'])
    assert (m.guidance_scale, m.guidance_drop) == (2.5, ('image', 'article'))
    assert m._check_guidance() == (('image', 'article'), 2.5)
    assert make(guidance_scale=2, beam_len_penalty=1.0)._check_guidance() == (('image',), 2.0)
    if kind == 'faces_objects':
        assert make(guidance_scale=0.5, guidance_drop=['image', 'faces', 'obj'])._check_guidance()[0] == ('image', 'faces', 'obj')
    else:
        with pytest.raises(ValueError, match='no context'):
            make(guidance_scale=2.0, guidance_drop=['faces'])
    for bad, name in ((dict(guidance_scale=-1), 'guidance_scale'), (dict(guidance_scale=float('nan')), 'guidance_scale'),
                      (dict(guidance_scale=2.0, guidance_drop=[]), 'guidance_drop'),
                      (dict(guidance_scale=2.0, guidance_drop=['text']), 'unknown'),
                      (dict(guidance_scale=2.0, sampling_topk=8), 'sampling_topk'),
                      (dict(guidance_scale=2.0, sampling_topk=0, sampling_topp=0.9), 'sampling_topp'),
                      (dict(guidance_scale=2.0, no_repeat_ngram_size=2), 'no_repeat_ngram_size'),
                      (dict(guidance_scale=2.0, repetition_penalty=1.2), 'repetition_penalty'),
                      (dict(guidance_scale=2.0, suppress_tokens=[5]), 'suppress_tokens')):
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
        assert (p['guidance_scale'].default, p['guidance_drop'].default) == (1.0, ('image',)), cls
    p = inspect.signature(build_model).parameters
    assert (p['guidance_scale'].default, p['guidance_drop'].default) == (1.0, ('image',))
    for fn in (CaptionModel.generate, CaptionModel.generate_lanes, TransformerGloveModel.generate, PointerModelBase.generate,
               BaselineGloveModel.generate):
        p = inspect.signature(fn).parameters
        assert p['guidance'].default is None and p['guidance_drop'].default is None, fn
    assert inspect.signature(DecodeStepper.__init__).parameters['guide'].default is None
    assert hasattr(DecodeStepper, 'set_guidance')
    assert inspect.signature(AdaptiveSoftmax.topk).parameters['guide'].default is None
    from tell_amd.models.gen_options import DecodePlan
    assert inspect.signature(CaptionModel._generate).parameters['guide'].default is None
    assert DecodePlan().guide is None and DecodePlan._field_defaults['guide'] is None
    for fn in (CaptionModel._generate_cached, CaptionModel._generate_beam):      # (they take the plan's fields as keywords)
        assert inspect.signature(fn).parameters['options'].kind is inspect.Parameter.VAR_KEYWORD
    for fn in (CaptionModel._greedy_steps, CaptionModel._beam_steps):
        assert inspect.signature(fn).parameters['plan'].default == DecodePlan()
    assert 'guidance' not in inspect.signature(CaptionModel.score_captions).parameters


@pytest.mark.parametrize('kind', ['flattened', 'faces_objects'])
def test_yaml_config_with_the_keys(tmp_path, kind):
    from tell_amd import config
    path = _write_cfg(tmp_path, kind)
    model, _ = config.from_config(path, overrides='{"model": {"guidance_scale": 2.5, "guidance_drop": ["article", "image"]}}',
                                  resnet=object(), roberta=object())
    assert (model.guidance_scale, model.guidance_drop) == (2.5, ('image', 'article'))
    assert model._check_guidance() == (('image', 'article'), 2.5)
    model, _ = config.from_config(path, overrides='{"model": {"guidance_scale": 3, "beam_len_penalty": 0.8}}',
                                  resnet=object(), roberta=object())
    assert model._check_guidance() == (('image',), 3.0)
    model, _ = config.from_config(path, resnet=object(), roberta=object())
    assert (model.guidance_scale, model.guidance_drop) == (1.0, ('image',)) and model._check_guidance() is None
    for over in ('{"model": {"guidance_scale": -1}}', '{"model": {"guidance_scale": "high"}}',
                 '{"model": {"guidance_scale": 2.0, "guidance_drop": []}}', '{"model": {"guidance_scale": 2.0, "guidance_drop": ["text"]}}',
                 '{"model": {"guidance_scale": 2.0, "sampling_topk": 8}}', '{"model": {"guidance_scale": 2.0, "min_len": 3}}',
                 '{"model": {"guidance_scale": 2.0, "ground_names": true}}'):
        with pytest.raises(ValueError):
            config.from_config(path, overrides=over, resnet=object(), roberta=object())


def test_symbols_declared_and_exported():
    import tell_amd
    protos = tell_amd.hip.parse_header()
    _, _, topk = protos['tell_adaptive_logprob_topk']
    _, _, guided = protos['tell_adaptive_logprob_topk_guided']
    rows = topk[:topk.index('k')]
    assert guided == rows + ['pair_offset', 'k', 'gamma_dev', 's_rows', 'ld_s', 'tokens', 'lps', 'stream']
    assert hasattr(tell_amd.hip.lib(), 'tell_adaptive_logprob_topk_guided')
    header = open(tell_amd.hip.HEADER_PATH).read()
    for phrase in ('d = lp_c - lp_u;  t = (gamma - 1) * d;  s = lp_c + t', 'never an FMA', 'lower id first on ties',
                   'r + pair_offset', 'gamma_dev'):
        assert phrase in header, phrase


# --------------------------------------------------------------------------- the definitions on the oracle
GEN = 24


def test_gamma_one_is_the_oracle(small):  # noqa: F811
    """gamma = 1: s is lp_c bit for bit, g = lp_c - L with |L| ~ 1e-7 - the ids of the plain searches."""
    from oracle.beam import beam_search
    om, start, ctx = small
    c = lambda: {k: v.clone() for k, v in ctx.items()}       # noqa: E731
    for K in (4, 2):
        ref_ids, ref_score = beam_search(om, start, c(), K, gen_len=GEN)
        ids, scores = beam_search_guided(om, start, c(), ('image',), 1.0, K, gen_len=GEN)
        assert torch.equal(ids[:, 0], ref_ids), K
        assert torch.allclose(scores[:, 0], ref_score, rtol=1e-5, atol=1e-4), K
    _, ref_ids, _ = om._generate(start, c(), gen_len=GEN)
    ids, _ = greedy_guided(om, start, c(), ('image',), 1.0, gen_len=GEN)
    assert torch.equal(ids, ref_ids)


def test_gamma_zero_is_the_decode_without_the_dropped_context(small):  # noqa: F811
    om, start, ctx = small
    c = lambda: {k: v.clone() for k, v in ctx.items()}       # noqa: E731
    _, want, _ = om._generate(start, dropped(c(), ('image',)), gen_len=GEN)
    got, _ = greedy_guided(om, start, c(), ('image',), 0.0, gen_len=GEN)
    assert torch.equal(got, want)
    _, plain, _ = om._generate(start, c(), gen_len=GEN)
    n = min(plain.shape[1], want.shape[1])
    assert plain.shape != want.shape or not torch.equal(plain[:, :n], want[:, :n])     # (the image matters to this decoder)


def test_guidance_changes_the_oracles_own_output(small):  # noqa: F811
    om, start, ctx = small
    c = lambda: {k: v.clone() for k, v in ctx.items()}       # noqa: E731
    g1, _ = greedy_guided(om, start, c(), ('image',), 1.0, gen_len=GEN)
    for drop in (('image',), ('article',), ('image', 'article')):
        g3, sc = greedy_guided(om, start, c(), drop, 3.0, gen_len=GEN)
        n = min(g1.shape[1], g3.shape[1])
        assert g1.shape != g3.shape or not torch.equal(g1[:, :n], g3[:, :n]), drop
        assert bool((sc <= 0).all())                         # sums of normalised log-probs
    b3, sc = beam_search_guided(om, start, c(), ('image',), 3.0, 4, gen_len=GEN, alpha=1.0)
    assert bool((sc[:, :-1] >= sc[:, 1:]).all())


# --------------------------------------------------------------------------- the cases of tests/test_gpu_guidance.py, on the oracle alone
FP32_GEN, FP32_EOS_FACTOR, FP32_SEED, FP32_B, FP32_ALPHA = 12, 14.0, 8, 4, 1.0   # (seed: chosen for the margins below)
FP32_CASES = ((('image',), 3.0), (('image', 'faces', 'obj'), 1.5))


def fullsize_oracle():
    """The full-size oracle decoder with the sharpened </s> row of the fp32 generator tests, its shell model, and the batch."""
    from oracle.build import build_decoder as obuild
    from oracle.models import CaptionModel as OModel
    from tell_amd.build import build_decoder
    from test_gpu_fullsize import _inputs_batch, _sharpened_eos
    torch.manual_seed(0)
    sd = _sharpened_eos({k: v.clone() for k, v in build_decoder('faces_objects').state_dict().items()}, FP32_EOS_FACTOR)
    ref = obuild('faces_objects').eval()
    ref.load_state_dict({k: v for k, v in sd.items() if k in ref.state_dict()}, strict=False)
    om = OModel.__new__(OModel)
    torch.nn.Module.__init__(om)
    om.decoder, om.padding_idx, om.index, om.sampling_topk, om.sampling_temp = ref, 1, 'roberta', 1, 1.0
    ctx, start = _inputs_batch(FP32_B, seed=FP32_SEED)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    return om, sd, ctx, start


@pytest.fixture(scope='module')
def fullsize_cases():
    om, _, ctx, start = fullsize_oracle()
    c = lambda: {k: v.clone() for k, v in ctx.items()}       # noqa: E731
    plain, _ = greedy_guided(om, start, c(), ('image',), 1.0, gen_len=FP32_GEN)
    out = {}
    for drop, gamma in FP32_CASES:
        gg, gb = [], []
        ids, sc = greedy_guided(om, start, c(), drop, gamma, gen_len=FP32_GEN, gaps=gg)
        bids, bsc = beam_search_guided(om, start, c(), drop, gamma, 4, gen_len=FP32_GEN, alpha=FP32_ALPHA, gaps=gb)
        out[(drop, gamma)] = (ids, sc, gg, bids, bsc, gb)
    return plain, out


@pytest.mark.parametrize('case', range(len(FP32_CASES)))
def test_the_gpu_cases_are_not_vacuous_and_have_margin(fullsize_cases, case):
    """For the seed and the gammas of test_gpu_guidance's fp32 generator test: the guided ids differ from the plain ids, and at
    every step of every live row the best and the second-best s differ by at least margin(gamma)."""
    plain, out = fullsize_cases
    drop, gamma = FP32_CASES[case]
    ids, sc, gg, bids, bsc, gb = out[(drop, gamma)]
    n = min(ids.shape[1], plain.shape[1])
    assert ids.shape != plain.shape or not torch.equal(ids[:, :n], plain[:, :n])
    print('\n%s gamma %.1f: smallest top-2 gap of s greedy %.4f, beam 4 %.4f (margin %.4f)'
          % ('+'.join(drop), gamma, min(gg), min(gb), margin(gamma)))
    assert min(gg) >= margin(gamma) and min(gb) >= margin(gamma)
    assert bool((bsc[:, :-1] >= bsc[:, 1:]).all())
