"""Several sampled captions per image, the part that needs no GPU: the arguments of
`generate(n_samples=, rank_by=, rank_len_penalty=)` and what they are refused with, the C prototype of tell_sample_rank, and the
host definition of the rank contract (`sample_rank_definition`, what tests/test_gpu_n_samples.py holds the kernel to) on a
hand-written case."""
import inspect

import numpy as np
import pytest
import torch

from test_beam_options_host import _Dyn, _shell

PAD, EOS = 1, 2


def _sampling_shell(cls=None, decoder=None, topk=5):
    from tell_amd.models.transformer import CaptionModel
    m = _shell(cls or CaptionModel, decoder if decoder is not None else _Dyn())
    m.sampling_topk, m.sampling_temp = topk, 0.8
    return m


# --------------------------------------------------------------------------- the arguments
def test_check_n_samples_accepts_and_rejects():
    from tell_amd.models.transformer import MAX_N_SAMPLES, RANK_BY, check_n_samples
    assert MAX_N_SAMPLES == 16 and RANK_BY == ('draw', 'score', 'consensus')
    assert check_n_samples() == (1, 'score', 0.0)
    assert check_n_samples(16, 'consensus', 1) == (16, 'consensus', 1.0)
    assert check_n_samples(2, 'draw', 0.7) == (2, 'draw', 0.7)
    for bad in (0, 17, -1, 2.0, True, '3', None):
        with pytest.raises(ValueError, match='n_samples'):
            check_n_samples(bad)
    for bad in ('best', 'Score', 1, None, ''):
        with pytest.raises(ValueError, match='rank_by'):
            check_n_samples(1, bad)                                     # (checked even when n = 1)
    for bad in (-0.1, float('inf'), float('nan'), 'x', True, None):
        with pytest.raises(ValueError, match='rank_len_penalty'):
            check_n_samples(1, 'score', bad)


def test_the_three_arguments_are_in_every_signature_with_their_defaults():
    from tell_amd.models.pointer import PointerModelBase
    from tell_amd.models.stepper import DecodeStepper
    from tell_amd.models.transformer import CaptionModel
    for fn in (CaptionModel.generate, CaptionModel.generate_lanes, PointerModelBase.generate):
        p = inspect.signature(fn).parameters
        assert p['n_samples'].default == 1 and p['rank_by'].default == 'score' and p['rank_len_penalty'].default == 0.0, fn
    from tell_amd.models.gen_options import DecodePlan
    assert DecodePlan().samples is None                              # (n, rule, alpha) of _check_n_samples; None: one draw
    assert inspect.signature(CaptionModel._greedy_steps).parameters['plan'].default == DecodePlan()
    assert inspect.signature(DecodeStepper.__init__).parameters['hyp'].default == 1
    # (_decode_stepper hands its keywords to the stepper as they are: the stepper's own default is the pin)
    assert inspect.signature(CaptionModel._decode_stepper).parameters['kw'].kind is inspect.Parameter.VAR_KEYWORD


def test_n_samples_refusals():
    from tell_amd.models.pointer import TransformerPointer2Model, TransformerPointerModel
    m = _sampling_shell()
    assert m._check_n_samples() is None                                  # n = 1: nothing to check, nothing changes
    assert m._check_n_samples(1, 'draw', 2.0, beam_size=4, attention=True, forward=True) is None
    assert m._check_n_samples(3) == (3, 'score', 0.0)
    assert m._check_n_samples(16, 'consensus', 0.7) == (16, 'consensus', 0.7)
    with pytest.raises(ValueError, match='n_best'):
        m._check_n_samples(3, beam_size=2)
    with pytest.raises(ValueError, match='attention=True'):
        m._check_n_samples(3, attention=True)
    with pytest.raises(ValueError, match='forward=True'):
        m._check_n_samples(3, forward=True)
    with pytest.raises(ValueError, match='rank_by'):
        m._check_n_samples(1, 'best')
    with pytest.raises(ValueError, match='rank_len_penalty'):
        m._check_n_samples(1, 'score', -1.0)
    greedy = _sampling_shell(topk=1)
    with pytest.raises(ValueError, match='identical captions'):
        greedy._check_n_samples(2)
    for rule in ('sampling_topp', 'sampling_minp', 'sampling_typical'):  # every sampling rule qualifies
        s = _sampling_shell(topk=0)
        setattr(s, rule, 0.9)
        assert s._check_n_samples(2) == (2, 'score', 0.0)
    lstm = _sampling_shell(decoder=torch.nn.Linear(2, 2))                # a decoder without project_contexts
    with pytest.raises(ValueError, match='LSTM decoders, copy models'):
        lstm._check_n_samples(2)
    for cls in (TransformerPointerModel, TransformerPointer2Model):
        ptr = _sampling_shell(cls)
        assert ptr._check_n_samples(1) is None
        with pytest.raises(ValueError, match='LSTM decoders, copy models'):
            ptr._check_n_samples(2)
        with pytest.raises(ValueError, match='n_samples=2'):
            ptr.generate({'roberta': torch.zeros(1, 4, dtype=torch.long)}, None,
                         {'roberta': torch.zeros(1, 4, dtype=torch.long)}, n_samples=2)
    # generate_lanes checks before it touches a batch or a stream
    with pytest.raises(ValueError, match='forward=True'):
        next(m.generate_lanes([], n_samples=2, forward=True))
    with pytest.raises(ValueError, match='n_best'):
        next(m.generate_lanes([], n_samples=2, beam_size=3))
    with pytest.raises(ValueError, match='rank_by'):
        next(m.generate_lanes([], rank_by='best'))


def test_generate_checks_n_samples_before_the_forward(monkeypatch):
    from tell_amd.models.transformer import CaptionModel

    class Reached(Exception):
        pass

    def fake_forward(self, *a, **kw):
        raise Reached
    monkeypatch.setattr(CaptionModel, '_forward', fake_forward)
    m = _sampling_shell()
    with pytest.raises(Reached):
        m.generate({}, 0, {}, n_samples=3, rank_by='consensus', rank_len_penalty=0.5)
    with pytest.raises(ValueError, match='rank_by'):
        m.generate({}, 0, {}, rank_by='best')
    with pytest.raises(ValueError, match='n_samples'):
        m.generate({}, 0, {}, n_samples=17)
    with pytest.raises(ValueError, match='attention=True'):
        m.generate({}, 0, {}, n_samples=2, attention=True)
    with pytest.raises(ValueError, match='identical captions'):
        _sampling_shell(topk=1).generate({}, 0, {}, n_samples=2)


def test_stepper_refuses_hypotheses_per_sample_outside_a_sampling_step():
    from tell_amd.models.stepper import DecodeStepper
    for kw in (dict(topk=2, sample=(5, 0.8)), dict(sample=None), dict(sample=(5, 0.8), attention=True)):
        with pytest.raises(ValueError, match='hyp'):
            DecodeStepper(None, 6, None, None, 10, hyp=3, **kw)
    with pytest.raises(ValueError, match='hyp'):
        DecodeStepper(None, 7, None, None, 10, hyp=3, sample=(5, 0.8))   # 7 rows are no multiple of 3


# --------------------------------------------------------------------------- the C prototype
def test_header_declares_tell_sample_rank():
    from tell_amd import hip
    protos = hip.parse_header()
    assert 'tell_sample_rank' in protos
    _, argtypes, names = protos['tell_sample_rank']
    assert names == ['ids', 'ld_ids', 'lps', 'ld_lps', 'done_step', 'inv_norm', 'B', 'n', 'steps', 'pad', 'eos', 'rule', 'order',
                     'score', 'dup', 'cons', 'len', 'stream']
    assert len(argtypes) == len(names)
    from tell_amd import ops
    assert ops.RANK_RULES == {'draw': 0, 'score': 1, 'consensus': 2} and callable(ops.sample_rank)


# --------------------------------------------------------------------------- the definition on a hand-written case
def _hand_case():
    """One image, four draws, 5 steps.  Draw 1 repeats draw 0 up to </s> and differs behind it (a duplicate); draw 2 never
    ends (done_step beyond `steps`); draw 3 ends with its first token (no bigram)."""
    ids = np.array([[0, 5, 6, 7, EOS, PAD],
                    [0, 5, 6, 7, EOS, 9],
                    [0, 5, 6, 8, 9, 3],
                    [0, EOS, PAD, PAD, PAD, PAD]], dtype=np.int64)
    lps = np.array([[-1, -1, -1, -1, 0],
                    [-.5, -.5, -.5, -.5, -9],
                    [-.25, -.25, -.25, -.25, -.25],
                    [-3, 0, 0, 0, 0]], dtype=np.float32)
    done = np.array([4, 4, 7, 1], dtype=np.int64)
    return ids, lps, done


def test_rank_definition_known_answers():
    from tell_amd.models.transformer import inv_norm_table, sample_rank_definition
    ids, lps, done = _hand_case()
    d = sample_rank_definition(ids, lps, done, 4, 5, EOS, 'score')
    assert d['len'].tolist() == [[4, 4, 5, 1]]
    assert d['score'].tolist() == [[-4.0, -2.0, -1.25, -3.0]] and d['score'].dtype == np.float32
    assert d['dup'].tolist() == [[0, 1, 0, 0]]
    # bigrams: {56, 67}, {56, 67}, {56, 68, 89, 93}, {}: u01 = 1, u02 = u12 = 2 * 1 / 6, everything with draw 3 is 0
    np.testing.assert_allclose(d['cons'][0], [4 / 9, 4 / 9, 2 / 9, 0.0], rtol=0, atol=1e-7)
    assert d['order'].tolist() == [[2, 3, 0, 1]]                         # score descending, the duplicate last
    assert sample_rank_definition(ids, lps, done, 4, 5, EOS, 'draw')['order'].tolist() == [[0, 1, 2, 3]]
    assert sample_rank_definition(ids, lps, done, 4, 5, EOS, 'draw')['dup'].tolist() == [[0, 1, 0, 0]]
    assert sample_rank_definition(ids, lps, done, 4, 5, EOS, 'consensus')['order'].tolist() == [[0, 2, 3, 1]]
    # alpha = 1: score / len = -1, -0.5, -0.25, -3
    d1 = sample_rank_definition(ids, lps, done, 4, 5, EOS, 1, inv_norm_table(1.0, 5).numpy())
    assert d1['score'].tolist() == [[-1.0, -0.5, -0.25, -3.0]] and d1['order'].tolist() == [[2, 0, 3, 1]]
    # the same rows as four images of one draw: nothing to compare with
    s = sample_rank_definition(ids, lps, done, 1, 5, EOS, 'consensus')
    assert s['order'].tolist() == [[0]] * 4 and s['dup'].tolist() == [[0]] * 4 and s['cons'].tolist() == [[0.0]] * 4
    # steps below a row's done_step cuts it: two steps of every row
    c = sample_rank_definition(ids, lps, done, 4, 2, EOS, 'score')
    assert c['len'].tolist() == [[2, 2, 2, 1]] and c['dup'].tolist() == [[0, 1, 1, 0]]
    assert c['order'].tolist() == [[0, 3, 2, 1]]                         # -2 | -3 | duplicates: -0.5 before -1


def test_rank_definition_ties_and_multiset_counts():
    from tell_amd.models.transformer import sample_rank_definition
    # clipped counts: 5 6 5 6 5 has 56 x 2, 65 x 2; 5 6 5 has 56 x 1, 65 x 1 -> |intersection| = 2, u = 2 * 2 / (4 + 2)
    ids = np.array([[0, 5, 6, 5, 6, 5, EOS], [0, 5, 6, 5, EOS, PAD, PAD], [0, 7, 8, 9, EOS, PAD, PAD]], dtype=np.int64)
    lps = np.full((3, 6), -0.5, dtype=np.float32)
    done = np.array([6, 4, 4], dtype=np.int64)
    d = sample_rank_definition(ids, lps, done, 3, 6, EOS, 'consensus')
    np.testing.assert_allclose(d['cons'][0], [(2 / 3 + 0) / 2, (2 / 3 + 0) / 2, 0.0], atol=1e-7)
    assert d['score'].tolist() == [[-3.0, -2.0, -2.0]]
    assert d['order'].tolist() == [[1, 0, 2]]                            # cons ties between 0 and 1: the higher score first
    assert sample_rank_definition(ids, lps, done, 3, 6, EOS, 'score')['order'].tolist() == [[1, 2, 0]]   # score tie: lower draw


def test_rank_on_the_host_for_hypotheses_on_the_cpu():
    """CaptionModel._rank_samples over CPU tensors goes through the definition: rank order, first rank, duplicate flags."""
    ids, lps, done = _hand_case()
    m = _sampling_shell()
    lp, best, info = m._rank_samples(torch.from_numpy(ids), torch.from_numpy(lps), torch.from_numpy(done), 1, 4, 5, 5, EOS,
                                     ('score', 0.0))
    s = info.samples
    assert s['sample_index'].tolist() == [[2, 3, 0, 1]] and s['sample_index'].dtype == torch.long
    assert s['duplicate'].tolist() == [[False, False, False, True]] and s['duplicate'].dtype == torch.bool
    assert s['scores_samples'].tolist() == [[-1.25, -3.0, -4.0, -2.0]]
    assert s['gen_ids_samples'].shape == (1, 4, 6) and s['log_probs_samples'].shape == (1, 4, 5)
    assert torch.equal(s['gen_ids_samples'][0], torch.from_numpy(ids)[[2, 3, 0, 1]])
    assert torch.equal(best, torch.from_numpy(ids)[2:3]) and torch.equal(lp, torch.from_numpy(lps)[2:3])
    assert info.scores.tolist() == [-1.25]
    out = m._attn_output({'gen_ids': best, 'log_probs': lp}, info)
    assert set(out) == {'gen_ids', 'log_probs', 'attns', 'scores', 'gen_ids_samples', 'log_probs_samples', 'scores_samples',
                        'sample_index', 'duplicate'}
    assert out['attns'] == [] and out['scores'].tolist() == [-1.25]
