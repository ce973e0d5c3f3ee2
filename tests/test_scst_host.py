"""Self-critical sequence training, the part that needs no GPU: the reward / advantage definition on
hand-worked cases (the package's caption_reward_definition, which is also the CPU path, and the brute-force restatement of
tests/scst_ref.py that the GPU test holds the kernel to), the C prototypes, and what ops.caption_reward, ops.adaptive_loss,
the models' forward and Trainer.train_self_critical refuse."""
import inspect

import numpy as np
import pytest
import torch

import scst_ref
from scst_ref import EOS, PAD
from test_beam_options_host import _Dyn, _shell

A, B_, C_ = 5, 6, 7


def _defs():
    from tell_amd.models.transformer import caption_reward_definition

    def package(ids, ref, n, steps, ref_steps, K, baseline=None):
        d = caption_reward_definition(ids, ref, n, steps, ref_steps, PAD, EOS, K, baseline)
        return d['reward'], d['adv'], d['counts']
    return (('package', package), ('scst_ref', scst_ref.reward))


def _rows(*rows):
    w = max(len(r) for r in rows)
    return np.array([list(r) + [PAD] * (w - len(r)) for r in rows], dtype=np.int64)


# --------------------------------------------------------------------------- the definition, by hand
@pytest.mark.parametrize('name,fn', _defs(), ids=[d[0] for d in _defs()])
def test_reward_known_answers(name, fn):
    # clipping: a a a a against a a.  k = 1: min(4, 2) = 2; k = 2: min(3, 1) = 1; k = 3, 4: the reference has none.
    # th = 4 + 3 + 2 + 1 = 10, tr = 2 + 1 = 3 -> 3 / 10
    ids, ref = _rows([0, A, A, A, A, EOS]), _rows([0, A, A, EOS])
    r, adv, c = fn(ids, ref, 1, 5, 3, 4)
    assert c.tolist() == [[3, 10, 3]] and r.dtype == np.float32 and r.tolist() == [[np.float32(3) / np.float32(10)]]
    assert adv.tolist() == r.tolist()                                    # n = 1, no baseline: the reward itself
    # a hypothesis shorter than k: a b against a b c d, K = 4.  matches a, b, ab = 3; th = 2 + 1 = 3, tr = 4 + 3 + 2 + 1 = 10
    r, _, c = fn(_rows([0, A, B_, EOS]), _rows([0, A, B_, C_, 8, EOS]), 1, 3, 5, 4)
    assert c.tolist() == [[3, 3, 10]] and r.tolist() == [[np.float32(3) / np.float32(10)]]
    # ... and the other way round: the reference longer than the hypothesis swaps th and tr, the reward stays
    r, _, c = fn(_rows([0, A, B_, C_, 8, EOS]), _rows([0, A, B_, EOS]), 1, 5, 3, 4)
    assert c.tolist() == [[3, 10, 3]] and r.tolist() == [[np.float32(3) / np.float32(10)]]
    # an empty hypothesis (eos in column 1): nothing matches, th = 0; both empty: 0 / 0 is 0
    r, _, c = fn(_rows([0, EOS, A, A]), _rows([0, A, A, EOS]), 1, 3, 3, 4)
    assert c.tolist() == [[0, 0, 3]] and r.tolist() == [[0.0]]
    r, _, c = fn(_rows([0, EOS, A]), _rows([0, PAD, A]), 1, 2, 2, 4)
    assert c.tolist() == [[0, 0, 0]] and r.tolist() == [[0.0]]
    # no eos at all: `steps` tokens are read, the column behind them is not.  a b c | against a b c: 3 + 2 + 1 of 6
    r, _, c = fn(_rows([0, A, B_, C_, 8]), _rows([0, A, B_, C_, 9]), 1, 3, 3, 3)
    assert c.tolist() == [[6, 6, 6]] and r.tolist() == [[1.0]]
    r, _, c = fn(_rows([0, A, B_, C_, 8]), _rows([0, A, B_, C_, 9]), 1, 4, 4, 3)
    assert c.tolist() == [[6, 9, 9]]                                     # one column more: a fourth, different, token each
    # a pad id ends a row as eos does; what lies behind is not read
    r, _, c = fn(_rows([0, A, PAD, A, A]), _rows([0, A, EOS, A]), 1, 4, 3, 2)
    assert c.tolist() == [[1, 1, 1]] and r.tolist() == [[1.0]]
    # identical rows give reward 1 at every K
    for K in (1, 2, 3, 4):
        r, _, c = fn(_rows([0, A, B_, A, B_, C_, EOS]), _rows([0, A, B_, A, B_, C_, EOS]), 1, 6, 6, K)
        assert r.tolist() == [[1.0]] and c[0, 0] == c[0, 1] == c[0, 2]
    # K = 1 against K = 2 on b a against a b: unigrams 2 of 2; bigrams none of 1
    assert fn(_rows([0, B_, A, EOS]), _rows([0, A, B_, EOS]), 1, 3, 3, 1)[2].tolist() == [[2, 2, 2]]
    assert fn(_rows([0, B_, A, EOS]), _rows([0, A, B_, EOS]), 1, 3, 3, 2)[2].tolist() == [[2, 3, 3]]


@pytest.mark.parametrize('name,fn', _defs(), ids=[d[0] for d in _defs()])
def test_advantage_known_answers(name, fn):
    f32 = np.float32
    # two images, two hypotheses each: rewards (1, 0) and (1/3, 1); leave-one-out is minus the other one
    ids = _rows([0, A, EOS], [0, B_, EOS], [0, C_, EOS], [0, C_, A, EOS])
    ref = _rows([0, A, EOS], [0, C_, A, EOS])
    r, adv, _ = fn(ids, ref, 2, 3, 3, 2)
    assert r.tolist() == [[1.0, 0.0], [f32(1) / f32(3), 1.0]]
    assert adv.tolist() == [[1.0, -1.0], [f32(f32(1) / f32(3) - f32(1)), f32(f32(1) - f32(1) / f32(3))]]
    # the greedy baseline: one number per image, whatever n
    base = np.array([0.25, 0.5], dtype=np.float32)
    r2, adv2, _ = fn(ids, ref, 2, 3, 3, 2, base)
    assert np.array_equal(r2, r) and adv2.tolist() == [[0.75, -0.25], [f32(f32(1) / f32(3) - f32(0.5)), 0.5]]
    # n = 1 with a baseline
    _, adv3, _ = fn(ids[:2], ref, 1, 3, 3, 2, base)
    assert adv3.tolist() == [[0.75], [-0.5]]


def test_leave_one_out_adds_the_others_in_ascending_order():
    """three rewards whose fp32 sum depends on the order: for hypothesis 0 the others are added as (2^-25 + 1), which is 1 in
    fp32, where 1 + 2^-25 + 2^-25 added the other way round would round differently"""
    from tell_amd.models.transformer import advantage_definition
    f32 = np.float32
    tiny = f32(2.0 ** -24)
    r = np.array([[tiny, 1.0, tiny, tiny]], dtype=np.float32)
    for fn in (advantage_definition, scst_ref.leave_one_out):
        adv = fn(r)
        # j = 1: tiny + tiny + tiny is exact (3 * 2^-24); j = 0: (1 + tiny) rounds to 1 (ties to even), + tiny again 1
        assert adv[0, 1] == f32(f32(1.0) - f32(f32(3) * tiny) / f32(3))
        assert adv[0, 0] == f32(tiny - f32(1.0) / f32(3))
        # j = 3: tiny + 1 -> 1, + tiny -> 1: the same; descending order would give (tiny + tiny) + 1 = 1 + 2^-23
        assert adv[0, 3] == adv[0, 0]
        assert f32(f32(tiny + tiny) + f32(1.0)) != f32(f32(tiny + f32(1.0)) + tiny)
    assert np.array_equal(advantage_definition(r, np.array([0.5], np.float32)), r - f32(0.5))
    assert np.array_equal(advantage_definition(r[:, :1]), r[:, :1])


@pytest.mark.parametrize('n', scst_ref.CASE_N)
@pytest.mark.parametrize('steps', scst_ref.CASE_STEPS[:3])
def test_the_two_definitions_agree_on_the_gpu_cases(n, steps):
    """the package's definition (Counter arithmetic) against the brute-force restatement, on the cases of the GPU test; the
    cases hold what they are meant to: empty rows, rows that never end, identical rows, clipped counts"""
    from tell_amd.models.transformer import caption_reward_definition
    ids, ref, ref_steps = scst_ref.case(n, steps)
    assert ids.shape == (scst_ref.CASE_B * n, steps + 4) and ref.shape[1] == ref_steps + 3
    for K in (1, 4):
        for base in (None, np.linspace(0.1, 0.9, scst_ref.CASE_B).astype(np.float32)):
            d = caption_reward_definition(ids, ref, n, steps, ref_steps, PAD, EOS, K, base)
            r, adv, c = scst_ref.reward(ids, ref, n, steps, ref_steps, K, base)
            assert np.array_equal(d['counts'], c) and np.array_equal(d['reward'].view(np.int32), r.view(np.int32))
            assert np.array_equal(d['adv'].view(np.int32), adv.view(np.int32))
    _, _, c = scst_ref.reward(ids, ref, n, steps, ref_steps, 4)
    assert (c[:, 1] == 0).any() or n == 1                                # an empty hypothesis
    assert (c[:, 1] == scst_ref.positions(range(steps), 4)).any()        # one that never ends
    if steps >= 7:
        assert (c[n] == c[n, 0]).all() and c[n, 0] > 0                   # the hypothesis that is its reference: reward 1


# --------------------------------------------------------------------------- prototypes and argument checks
def test_header_declares_the_new_entry_points():
    from tell_amd import hip
    protos = hip.parse_header()
    assert protos['tell_caption_reward'][2] == ['ids', 'ld_ids', 'ref', 'ld_ref', 'baseline', 'B', 'n', 'steps', 'ref_steps',
                                                'pad', 'eos', 'max_order', 'reward', 'adv', 'counts', 'stream']
    fwd, bwd = protos['tell_ce_fwd'][2], protos['tell_ce_bwd'][2]
    i = fwd.index('ignore_index') + 1
    assert protos['tell_ce_fwd_weighted'][2] == fwd[:i] + ['w', 'w_idx'] + fwd[i:]
    assert protos['tell_ce_bwd_weighted'][2] == bwd[:i] + ['w', 'w_idx'] + bwd[i:]


def test_caption_reward_checks_its_arguments():
    from tell_amd import ops
    ids, ref = torch.zeros(6, 9, dtype=torch.long), torch.zeros(3, 7, dtype=torch.long)
    ok = dict(B=3, n=2, steps=8, ref_steps=6, pad=PAD, eos=EOS)
    for bad, name in ((dict(n=0), 'n'), (dict(n=17), 'n'), (dict(n=True), 'n'), (dict(steps=0), 'steps'),
                      (dict(steps=257), 'steps'), (dict(ref_steps=0), 'ref_steps'), (dict(ref_steps=257), 'ref_steps'),
                      (dict(max_order=0), 'max_order'), (dict(max_order=5), 'max_order'), (dict(max_order=2.0), 'max_order'),
                      (dict(B=0), 'B')):
        with pytest.raises(ValueError, match='caption_reward: %s ' % name):
            ops.caption_reward(ids, ref, **{**ok, **bad})
    with pytest.raises(ValueError, match='ids int64'):
        ops.caption_reward(ids, ref, **{**ok, 'steps': 9})               # ld_ids must exceed steps
    with pytest.raises(ValueError, match='ids int64'):
        ops.caption_reward(ids.int(), ref, **ok)
    with pytest.raises(ValueError, match='ids int64'):
        ops.caption_reward(ids[:5], ref, **ok)
    with pytest.raises(ValueError, match='ref int64'):
        ops.caption_reward(ids, ref, **{**ok, 'ref_steps': 7})
    with pytest.raises(ValueError, match='ref int64'):
        ops.caption_reward(ids, ref[:2], **ok)
    for base in (torch.zeros(2), torch.zeros(3, dtype=torch.float64), [0.0, 0.0, 0.0]):
        with pytest.raises(ValueError, match='baseline fp32'):
            ops.caption_reward(ids, ref, baseline=base, **ok)


def test_adaptive_loss_checks_row_weight_before_any_launch():
    from tell_amd import ops
    x, target = torch.zeros(2, 3, 8), torch.zeros(2, 3, dtype=torch.long)
    for bad in (torch.ones(3, 2), torch.ones(2, 3, dtype=torch.float64), torch.ones(6), [[1.0] * 3] * 2):
        with pytest.raises(ValueError, match='row_weight'):
            ops.adaptive_loss(x, target, (4, 8), 1, None, None, [], row_weight=bad)
    assert inspect.signature(ops.adaptive_loss).parameters['row_weight'].default is None
    from tell_amd.modules import AdaptiveLoss, AdaptiveSoftmax
    assert inspect.signature(AdaptiveLoss.forward).parameters['row_weight'].default is None
    assert inspect.signature(AdaptiveSoftmax.loss).parameters['row_weight'].default is None


def test_forward_defaults_and_checks():
    from tell_amd.models.transformer import CaptionModel, check_caption_weights, check_per_image
    for fn in (CaptionModel.forward, CaptionModel._forward_loss):
        p = inspect.signature(fn).parameters
        assert p['caption_weights'].default is None and p['per_image'].default == 1
    assert inspect.signature(CaptionModel._forward).parameters['per_image'].default == 1
    assert check_per_image(1, 3, 3) == 1 and check_per_image(4, 12, 3) == 4
    for bad in (0, -1, 2.0, True, None, '2'):
        with pytest.raises(ValueError, match='per_image'):
            check_per_image(bad, 6, 3)
    with pytest.raises(ValueError, match='3 images need 6 captions'):
        check_per_image(2, 5, 3)
    tg = torch.zeros(4, 5, dtype=torch.long)
    w = check_caption_weights(torch.arange(4, dtype=torch.float32), tg)
    assert w.shape == (4, 5) and w.is_contiguous() and w[:, 3].tolist() == [0.0, 1.0, 2.0, 3.0]
    full = torch.rand(4, 5, requires_grad=True)
    assert not check_caption_weights(full, tg).requires_grad             # not differentiated
    for bad in (torch.ones(5), torch.ones(4, 4), torch.ones(4, 5, dtype=torch.float64), torch.ones(4, 5, 1), [1.0] * 4):
        with pytest.raises(ValueError, match='caption_weights'):
            check_caption_weights(bad, tg)


def test_forward_hands_the_defaults_through_unchanged(monkeypatch):
    """forward() without the new arguments reaches _forward_loss with (None, 1), and the output dict is the one it returns"""
    from tell_amd.models.transformer import CaptionModel
    seen = {}

    def fake(self, context, image, caption, face_embeds, obj_embeds, encoded, caption_weights=None, per_image=1):
        seen['args'] = (caption_weights, per_image)
        return {'loss': torch.zeros(()), 'sample_size': torch.ones(())}, torch.zeros(2, 3, dtype=torch.long), {}
    monkeypatch.setattr(CaptionModel, '_forward_loss', fake)
    m = _shell(CaptionModel, _Dyn())
    m.evaluate_mode, m.n_samples, m.n_batches = False, 0, 0
    out = m.forward({}, None, {})
    assert seen['args'] == (None, 1) and set(out) == {'loss', 'sample_size'} and m.n_samples == 2
    w = torch.ones(2)
    m.forward({}, None, {}, caption_weights=w, per_image=2)
    assert seen['args'][0] is w and seen['args'][1] == 2


def test_models_outside_the_weighted_pass_refuse_by_name():
    from tell_amd.models import BaselineGloveModel, TransformerGloveModel
    from tell_amd.models.pointer import TransformerPointer2Model, TransformerPointerModel
    from tell_amd.models.transformer import CaptionModel
    w = torch.ones(2)
    for cls in (TransformerPointerModel, TransformerPointer2Model):
        m = _shell(cls, _Dyn())
        for kw in (dict(caption_weights=w), dict(per_image=2)):
            with pytest.raises(ValueError, match=cls.__name__):
                m.forward({}, None, {}, **kw)
    for cls in (BaselineGloveModel, TransformerGloveModel):
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        for kw in (dict(caption_weights=w), dict(per_image=2)):
            with pytest.raises(ValueError, match=cls.__name__):
                m.forward(None, {}, **kw)
    lstm = _shell(CaptionModel, torch.nn.Linear(2, 2))                   # a decoder without project_contexts
    for kw in (dict(caption_weights=w), dict(per_image=2)):
        with pytest.raises(ValueError, match='CaptionModel does not take caption_weights / per_image'):
            lstm.forward({}, None, {}, **kw)


def test_train_self_critical_refusals():
    from tell_amd.models.transformer import CaptionModel
    from tell_amd.training import Trainer
    check = Trainer.check_self_critical
    assert check() == (4, 'leave_one_out', 4) and check(1, 'greedy', 1) == (1, 'greedy', 1)
    assert check(16, 'leave_one_out', 2, reward=lambda ids, batch: None) == (16, 'leave_one_out', 2)
    for bad in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='n_samples'):
            check(bad)
    for bad in ('mean', 'Greedy', None, 0):
        with pytest.raises(ValueError, match='baseline'):
            check(4, bad)
    with pytest.raises(ValueError, match="baseline='leave_one_out' needs n_samples >= 2"):
        check(1)
    for bad in (0, 5, 1.5, True):
        with pytest.raises(ValueError, match='max_order'):
            check(4, 'greedy', bad)
    with pytest.raises(ValueError, match='reward'):
        check(4, 'greedy', 4, reward='gleu')
    t = Trainer.__new__(Trainer)                                         # the checks come before anything of the trainer is used
    t.model = _shell(CaptionModel, _Dyn())                               # sampling_topk = 1: the arg-max decode
    with pytest.raises(ValueError, match='needs a sampling model'):
        t.train_self_critical({}, n_samples=2)
    with pytest.raises(ValueError, match='n_samples'):
        t.train_self_critical({}, n_samples=0)
    t.model = torch.nn.Linear(2, 2)                                      # no generator at all
    with pytest.raises(ValueError, match='needs a sampling model'):
        t.train_self_critical({})


def test_trainer_config_key():
    from tell_amd.training.trainer import CallbackApexTrainer
    p = inspect.signature(CallbackApexTrainer.__init__).parameters
    assert p['self_critical'].default is None
    src = inspect.getsource(CallbackApexTrainer.train)
    assert 'train_self_critical' in src and 'train_one_batch' in src
