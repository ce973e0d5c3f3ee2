"""CPU checks of several sampled captions per image for the copy models: the ABI of
tell_copy_decide_hyp, the shape checks of ops.copy_decide(per_image=), what generate(n_samples=) accepts and still refuses on
both registered classes, the key sets, and the definition of the grouped copy decision over the hypothesis batches
tests/test_gpu_copy_n_samples.py runs (tests/copy_hyp_cases.py)."""
import os

import numpy as np
import pytest
import torch

import copy_decode_cases as cdc
import copy_hyp_cases as chc
import copy_ref as ref
import tell_amd  # noqa: F401
from test_copy_decode_host import _tiny
from tell_amd.models.transformer import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('transformer_pointer', 'transformer_pointer_2')
KINDS = {'transformer_pointer': 'pointer', 'transformer_pointer_2': 'pointer_2'}
UNCHANGED = 'LSTM decoders, copy models'
SAMPLE_KEYS = {'gen_ids_samples', 'log_probs_samples', 'scores_samples', 'sample_index', 'duplicate', 'scores',
               'should_copy_samples', 'copy_probs_samples', 'generations_samples', 'copied_texts_samples'}
PLAIN_KEYS = {'gen_ids', 'log_probs', 'should_copy', 'copy_probs', 'generations', 'copied_texts'}


class Reached(Exception):
    """the checks of generate() let the call through"""


# ---------------------------------------------------------------- ABI
def test_symbol_is_declared_and_exported():
    from tell_amd import hip
    protos = hip.parse_header()
    assert 'tell_copy_decide_hyp' in protos
    names, base = protos['tell_copy_decide_hyp'][2], protos['tell_copy_decide'][2]
    assert [x for x in names if x != 'per_image'] == list(base), 'tell_copy_decide plus per_image'
    assert names[names.index('per_image') - 1] == 'B' and names[-1] == 'stream'
    if not os.path.exists(hip.LIB_PATH):
        pytest.fail('%s is not built' % hip.LIB_PATH)
    lib = hip.lib()                                    # (resolves every declared symbol; a missing one raises)
    assert getattr(lib, 'tell_copy_decide_hyp').argtypes == protos['tell_copy_decide_hyp'][1]


# ---------------------------------------------------------------- ops.copy_decide(per_image=)
def _operands(images=2, n=3, S=6, H=2, E=128, L=3):
    R = images * n
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)                    # noqa: E731
    return dict(q=z(R, E), k=z(S, images, E), bias_k=z(1, 1, E), mask=z(images, S, dt=torch.uint8),
                proper=z(images, S, dt=torch.int8), ctx_ids=z(images, S, dt=torch.int64), entity_logits=z(R, 2),
                gen_tok=z(R, dt=torch.int32), finished=z(R, dt=torch.uint8), hist=z(R, L + 1, dt=torch.int32),
                copied=z(R, L + 1, dt=torch.uint8), prob=z(R, L), step=0, H=H, scratch=z(R, H, S), tok=z(R, dt=torch.int32),
                per_image=n)


def test_ops_copy_decide_rejects_mismatched_heights_and_per_image(monkeypatch):
    import inspect
    from tell_amd import ops
    assert inspect.signature(ops.copy_decide).parameters['per_image'].default == 1
    issued = []
    monkeypatch.setattr(ops, 'call', lambda name, *a: issued.append((name, a)))
    monkeypatch.setattr(ops.hip, 'dt', lambda t: 0)
    kw = _operands()
    ops.copy_decide(**kw)                                               # the well-formed call reaches the new entry point
    name, a = issued.pop()
    assert name == 'tell_copy_decide_hyp' and not issued
    protos = __import__('tell_amd').hip.parse_header()
    names = protos[name][2][:-1]                                        # (the stream is the caller's)
    assert len(a) == len(names)
    got = dict(zip(names, a))
    assert (got['B'], got['per_image'], got['H'], got['S'], got['D'], got['L']) == (2, 3, 2, 6, 64, 3)
    one = _operands(n=1)
    ops.copy_decide(**{k_: v for k_, v in one.items() if k_ != 'per_image'})
    assert issued.pop()[0] == 'tell_copy_decide'                        # the default: the call of before
    ops.copy_decide(**one)
    assert issued.pop()[0] == 'tell_copy_decide'
    R, images, S, E, L, H = 6, 2, 6, 128, 3, 2
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)                    # noqa: E731
    # the image-height operands at the row height, the row-height operands at the image height
    for key, bad in (('k', z(S, R, E)), ('mask', z(R, S, dt=torch.uint8)), ('proper', z(R, S, dt=torch.int8)),
                     ('ctx_ids', z(R, S, dt=torch.int64)), ('entity_logits', z(images, 2)), ('gen_tok', z(images, dt=torch.int32)),
                     ('finished', z(images, dt=torch.uint8)), ('hist', z(images, L + 1, dt=torch.int32)),
                     ('copied', z(images, L + 1, dt=torch.uint8)), ('tok', z(images, dt=torch.int32)),
                     ('scratch', z(images, H, S))):
        with pytest.raises(ValueError, match=key):
            ops.copy_decide(**dict(kw, **{key: bad}))
    with pytest.raises(ValueError, match='per_image'):
        ops.copy_decide(**dict(kw, q=z(R + 1, E)))                      # rows that are no multiple of n
    for bad in (0, 17, -1, 2.0, True, None, '2'):
        with pytest.raises(ValueError, match='per_image'):
            ops.copy_decide(**dict(kw, per_image=bad))
    assert not issued


# ---------------------------------------------------------------- what generate(n_samples=) accepts and refuses
@pytest.fixture(scope='module')
def models():
    """per registered name: (a model that samples - sampling_topp 0.9, T 0.8 - and a greedy one)"""
    return {name: (_tiny(KINDS[name], sampling_topk=0, sampling_topp=0.9, sampling_temp=0.8), _tiny(KINDS[name])) for name in NAMES}


def _call(model, **kw):
    ids = torch.full((1, 5), 4)
    ctx = {'roberta': ids, 'roberta_proper_masks': torch.ones_like(ids)}
    return model.generate(context=ctx, image=torch.zeros(1, 3, 8, 8), caption={'roberta': ids}, **kw)


@pytest.mark.parametrize('name', NAMES)
def test_n_samples_is_accepted_on_the_cached_path_of_a_sampling_model(name, models, monkeypatch):
    from tell_amd.models.pointer import PointerModelBase
    sampler, greedy = models[name]
    assert type(sampler) is Model.by_name(name) and sampler._sampling() is not None and greedy._sampling() is None

    def reached(self, *a, **kw):
        raise Reached
    monkeypatch.setattr(PointerModelBase, '_require_masks', reached)    # (the first thing behind the checks)
    # ---- accepted: the call decodes through the cached path and the model samples
    with pytest.raises(Reached):
        _call(sampler, n_samples=2, cached=True)
    with pytest.raises(Reached):
        _call(sampler, n_samples=16, rank_by='consensus', rank_len_penalty=0.7, cached=True)
    monkeypatch.setattr(sampler, 'cached_generation', True)
    with pytest.raises(Reached):
        _call(sampler, n_samples=2)                                     # cached_generation: true
    assert sampler._check_n_samples(3, 'draw', 0.0, cached=True) == (3, 'draw', 0.0)
    # ---- refused with the message of before: the eager path (asked for, or by the key's default) ...
    with pytest.raises(ValueError, match=UNCHANGED) as eager:
        _call(sampler, n_samples=2, cached=False)
    assert 'n_samples=2' in str(eager.value)
    monkeypatch.setattr(sampler, 'cached_generation', False)
    with pytest.raises(ValueError, match=UNCHANGED):
        _call(sampler, n_samples=2)
    # ... a greedy model on either path ...
    for cached in (False, True, None):
        with pytest.raises(ValueError, match=UNCHANGED) as err:
            _call(greedy, n_samples=2, cached=cached)
        assert str(err.value) == str(eager.value)
    # ... and the check without the new argument
    for m in (sampler, greedy):
        with pytest.raises(ValueError, match=UNCHANGED):
            m._check_n_samples(2)
        with pytest.raises(ValueError, match=UNCHANGED):
            m._check_n_samples(2, cached=False)
    with pytest.raises(ValueError, match=UNCHANGED):
        greedy._check_n_samples(2, cached=True)
    # n = 1 and the arguments' own checks are untouched
    assert sampler._check_n_samples(1, cached=True) is None
    with pytest.raises(ValueError, match='n_samples'):
        _call(sampler, n_samples=17, cached=True)
    with pytest.raises(ValueError, match='rank_by'):
        _call(sampler, n_samples=2, rank_by='best', cached=True)
    assert sampler.lanes_usable() is False


def test_the_plain_models_and_the_lstm_decoders_are_where_they_were():
    from test_n_samples_host import _sampling_shell
    m = _sampling_shell()
    assert m._check_n_samples(3, cached=True) == m._check_n_samples(3) == (3, 'score', 0.0)
    lstm = _sampling_shell(decoder=torch.nn.Linear(2, 2))
    for cached in (False, True):
        with pytest.raises(ValueError, match=UNCHANGED):
            lstm._check_n_samples(2, cached=cached)
    for cls in (Model.by_name(n) for n in NAMES):                       # a shell that never ran __init__: no key, the eager path
        ptr = _sampling_shell(cls)
        with pytest.raises(ValueError, match=UNCHANGED):
            ptr.generate({'roberta': torch.zeros(1, 4, dtype=torch.long)}, None, {'roberta': torch.zeros(1, 4, dtype=torch.long)},
                         n_samples=2)


@pytest.mark.parametrize('name', NAMES)
def test_every_still_refused_option_is_refused_with_n_samples(name, models):
    """each option's own message, the one it raises without n_samples - never the cached decode"""
    sampler = models[name][0]
    refused = [dict(beam_size=2), dict(n_best=2), dict(attention=True), dict(prefix=torch.full((1, 2), 5)), dict(banned=[5]),
               dict(ground=True), dict(guidance=2.0)]
    for kw in refused:
        with pytest.raises(ValueError) as alone:
            _call(sampler, cached=True, **kw)
        with pytest.raises(ValueError) as both:
            _call(sampler, cached=True, n_samples=2, **kw)
        assert str(both.value) == str(alone.value), kw
    for opt in (dict(repetition_penalty=1.2), dict(presence_penalty=0.5), dict(no_repeat_ngram_size=2), dict(beam_len_penalty=0.5)):
        with pytest.raises(ValueError):                     # (at construction or at the call, as without n_samples)
            m = _tiny(KINDS[name], sampling_topk=0, sampling_topp=0.9, cached_generation=True, **opt)
            _call(m, n_samples=2)


# ---------------------------------------------------------------- the key sets
def _stub_decode(model, monkeypatch, R=2, L=4):
    """everything in front of and behind the decode loop runs; the loop itself (GPU launches) is replaced"""
    from tell_amd.models.pointer import PointerModelBase
    ids = torch.tensor([[0, 7, 8, 2], [0, 9, 2, 1]])
    monkeypatch.setattr(PointerModelBase, 'encode', lambda self, *a, **kw: None)
    monkeypatch.setattr(PointerModelBase, '_forward', lambda self, *a, **kw: (ids[:, :1], None, {}))
    monkeypatch.setattr(PointerModelBase, 'detokenize', lambda self, x: ' '.join(str(int(i)) for i in x))
    plain = (ids, torch.zeros(2, 3), torch.tensor([[1, 0, 1, 0], [1, 1, 0, 0]]).bool(), torch.full((2, 3), 0.5))
    monkeypatch.setattr(PointerModelBase, '_generate_pointer', lambda self, *a, **kw: plain)
    monkeypatch.setattr(PointerModelBase, '_generate_pointer_cached', lambda self, *a, **kw: plain)
    return ids, plain


@pytest.mark.parametrize('name', NAMES)
def test_n_samples_1_returns_the_key_set_of_before(name, models, monkeypatch):
    sampler = models[name][0]
    ids, plain = _stub_decode(sampler, monkeypatch)
    for kw in (dict(), dict(cached=True), dict(cached=True, n_samples=1, rank_by='consensus', rank_len_penalty=0.7),
               dict(cached=False, n_samples=1)):
        out = _call(sampler, **kw)
        assert set(out) == PLAIN_KEYS, kw
        assert out['gen_ids'] is ids and out['copied_texts'] == ['0 8', '0 9'] and out['generations'] == ['7 8 2', '9 2']


@pytest.mark.parametrize('name', NAMES)
def test_n_samples_2_adds_the_sample_keys_in_one_order(name, models, monkeypatch):
    """_pointer_steps replaced by its contract (a generator returning the first rank and the `_samples` dict in rank order):
    what generate() builds from it - the texts, the first-rank keys"""
    from tell_amd.models.pointer import PointerModelBase
    sampler = models[name][0]
    _stub_decode(sampler, monkeypatch)
    B, n = 2, 2
    g = torch.Generator().manual_seed(3)
    gi = torch.randint(3, 50, (B, n, 4), generator=g)
    smp = {'gen_ids_samples': gi, 'log_probs_samples': -torch.rand(B, n, 3, generator=g), 'scores_samples': -torch.rand(B, n, generator=g),
           'sample_index': torch.tensor([[1, 0], [0, 1]]), 'duplicate': torch.zeros(B, n, dtype=torch.bool),
           'should_copy_samples': torch.rand(B, n, 4, generator=g) > 0.5, 'copy_probs_samples': torch.rand(B, n, 3, generator=g)}
    seen = {}

    def steps(self, caption_ids, contexts, enc, context, *a, **kw):
        seen.update(kw)
        return (None, None, None, None, smp)
        yield                                                           # noqa: unreachable - makes this a generator
    monkeypatch.setattr(PointerModelBase, '_pointer_steps', steps)
    out = _call(sampler, cached=True, n_samples=n, rank_by='consensus', rank_len_penalty=0.7)
    assert seen == {'n': 2, 'rank': ('consensus', 0.7)}
    assert set(out) == PLAIN_KEYS | SAMPLE_KEYS
    for k_ in smp:
        assert out[k_] is smp[k_]
    for first, many in (('gen_ids', 'gen_ids_samples'), ('log_probs', 'log_probs_samples'), ('should_copy', 'should_copy_samples'),
                        ('copy_probs', 'copy_probs_samples'), ('scores', 'scores_samples')):
        assert torch.equal(out[first], smp[many][:, 0]), first
    assert [len(x) for x in out['generations_samples']] == [n] * B == [len(x) for x in out['copied_texts_samples']]
    for b in range(B):
        for j in range(n):
            assert out['generations_samples'][b][j] == ' '.join(str(int(i)) for i in gi[b, j])
            assert out['copied_texts_samples'][b][j] == ' '.join(str(int(i)) for i in gi[b, j][smp['should_copy_samples'][b, j]])
    assert out['generations'] == [x[0] for x in out['generations_samples']]
    assert out['copied_texts'] == [x[0] for x in out['copied_texts_samples']]


def test_pointer_steps_signature():
    import inspect
    from tell_amd.models.pointer import PointerModelBase
    p = inspect.signature(PointerModelBase._pointer_steps).parameters
    assert p['n'].default == 1 and p['rank'].default == ('score', 0.0)
    assert inspect.signature(PointerModelBase._check_n_samples).parameters['cached'].default is False


# ---------------------------------------------------------------- the static-row definition over the expanded batch
@pytest.mark.parametrize('n', chc.N_HYP)
def test_hypothesis_rows_are_copy_step_over_the_expanded_batch(n):
    for cid, make in chc.cases():
        h = make('float32', n)
        x = dict(cdc.cases())[cid]('float32')
        B = len(x['fin'])
        R = B * n
        e, base = chc.expected(h), cdc.expected(x)
        assert h['q'].shape[0] == h['ent'].shape[0] == len(h['fin']) == R and h['k'].shape[1] == B and h['ctx'].shape[0] == B
        ex = chc.expand(h)
        assert ex['k'].shape[1] == R and all(np.array_equal(ex['k'][:, r], x['k'][:, r // n]) for r in range(R))
        assert np.array_equal(ex['ctx'], np.repeat(x['ctx'], n, 0))
        dead, between = chc.marked_images(x, n)
        if n >= 2:
            assert h['fin'][dead * n:(dead + 1) * n].all(), cid
        if n >= 3:
            assert h['fin'][between * n:between * n + 3].tolist() == [0, 1, 0], cid
        live = e['rows'].tolist()
        assert live == np.flatnonzero(h['fin'] == 0).tolist()
        for b in range(B):                                                # hypothesis (b, 0) is case row b ...
            r = b * n
            assert np.array_equal(h['q'][r], x['q'][b]) and h['gen'][r] == x['gen'][b]
            if r in live and b in base['rows'].tolist():
                i, j = live.index(r), base['rows'].tolist().index(b)
                assert e['tok'][r] == base['tok'][b] and e['copied'][r] == base['copied'][b], (cid, b)
                assert e['r']['prob'][i] == base['r']['prob'][j] and e['hist'][r].tolist() == base['hist'][b].tolist()
            for j in range(1, n):                                         # ... (b, j) carries row (b + j) mod B
                assert np.array_equal(h['q'][r + j], x['q'][(b + j) % B]) and np.array_equal(h['hist'][r + j], x['hist'][(b + j) % B])
        for r in range(R):                                                # a finished row keeps everything
            if h['fin'][r]:
                assert e['tok'][r] is None and e['hist'][r].tolist() == np.asarray(h['hist'])[r].tolist()


def test_the_hypothesis_batches_hold_rows_that_copy_and_rows_that_do_not():
    for dtype in ref.DTYPES:
        for n in (2, 5):
            kinds = set()
            for cid, make in chc.cases():
                e = chc.expected(make(dtype, n))
                kinds |= {bool(e['copied'][r]) for r in e['rows']}
            assert kinds == {True, False}
