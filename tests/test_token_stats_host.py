"""Per-token statistics, the part that needs no GPU: the ABI declaration, the float64 reference and the
conditions the GPU cases rest on (tests/token_stats_ref.py), `token_stats_definition` against the reference, the neutral fill,
every refusal and its wording, the untouched defaults, and the word-level view on a hand-made generation."""
import inspect

import numpy as np
import pytest
import torch

import token_stats_ref as R
from test_beam_options_host import _Dyn, _shell


# --------------------------------------------------------------------------- the ABI
def test_the_entry_point_is_declared_with_the_arguments_of_the_issue():
    from tell_amd.hip import parse_header
    res, argtypes, names = parse_header()['tell_adaptive_logprob_stats']
    assert names == ['head', 'ld_head', 'c0', 'n_tails', 'tail0', 'ld0', 'n0', 'tail1', 'ld1', 'n1', 'tail2', 'ld2', 'n2', 'rows',
                     'chosen', 'ld_chosen', 'finished', 'n', 'slots', 'step', 'step_dev', 'pad', 'alt_tok', 'alt_lp', 'rank',
                     'entropy', 'chosen_lp', 'stream']
    forced = parse_header()['tell_adaptive_logprob_forced'][2]
    assert names[:14] == forced[:14]                          # the usual head / tail arguments, rows last


# --------------------------------------------------------------------------- the reference and the conditions of the GPU cases
def test_case_table_covers_what_the_issue_lists():
    by = {c['name']: c for c in R.CASES}
    assert by['tiny']['c0'] == 5 and by['tiny']['tails'] == (3,) and R.vocab(by['tiny']) == 8 and 8 in R.ALTS
    assert by['unaligned']['tails'] == (61, 130, 29) and by['unaligned']['layout'] == 'odd'
    assert by['head8192']['c0'] + len(by['head8192']['tails']) == 8192
    assert by['head8193']['c0'] + len(by['head8193']['tails']) == 8193
    assert R.vocab(by['expt']) == 50265 and by['expt_sliced']['layout'] == 'sliced'
    assert by['no_tails']['tails'] == () and R.ROWS == (1, 5, 33) and R.ALTS == (1, 4, 8)
    for name in ('expt', 'unaligned', 'tie'):
        kinds = set(R.chosen(name, 33)[1])
        assert {'argmax', 'third', 'outside'} <= kinds and {'tail%d' % i for i in range(len(by[name]['tails']))} <= kinds
    assert {'tie_first', 'tie_middle', 'tie_last'} <= set(R.chosen('tie', 33)[1])


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c['name'])
def test_reference_entropy_two_ways_and_the_gap_of_every_row(case):
    """Chain rule against -sum p log p to 1e-12; and for EVERY row (none skipped) the chosen token's float64 log-prob is
    further than twice the fp32 bound of a log-prob from every log-prob that differs from it: the float64 rank - ties to the
    lower id among exactly equal logits of one cluster - is then the only rank fp32 arithmetic within the bound can give."""
    for rows in R.ROWS:
        ref = R.reference(case['name'], rows)
        assert np.abs(ref['entropy'] - ref['entropy_direct']).max() <= 1e-12
        g = R.gap(case['name'], rows)
        assert (g > 2.0 * ref['d_lp']).all(), (case['name'], rows, np.flatnonzero(g <= 2.0 * ref['d_lp']), g.min())
        tok, kinds = R.chosen(case['name'], rows)
        V = R.vocab(case)
        for r, (t, kind) in enumerate(zip(tok, kinds)):
            assert (kind == 'outside') == (not 0 <= t < V)
            if kind == 'argmax':
                assert R.rank_of(ref['lp'][r], int(t)) == 0
            if kind == 'third' and V > 2:
                assert R.rank_of(ref['lp'][r], int(t)) == 2
        assert (ref['d_entropy'] > 0).all() and ref['d_entropy'].max() < 1e-3
    if case['content'] == 'uniform':
        assert np.abs(R.reference(case['name'], 5)['entropy'] - np.log(R.vocab(case))).max() <= 1e-12
    if case['content'] == 'spike':
        assert R.reference(case['name'], 5)['entropy'].max() < 1e-20
    if case['content'] == 'tie':                              # the tied group really is a group, and its members rank by id
        ref, (tok, kinds) = R.reference('tie', 33), R.chosen('tie', 33)
        for r in range(3):
            grp = np.flatnonzero(ref['lp'][r] == ref['lp'][r, tok[r]])
            assert len(grp) >= 3 and kinds[r].startswith('tie_')
            assert R.rank_of(ref['lp'][r], int(tok[r])) == int((ref['lp'][r] > ref['lp'][r, tok[r]]).sum()) + \
                list(grp).index(int(tok[r]))


def test_pin_rounds_eight_times_the_ratio_up_to_a_power_of_two():
    assert R.pin(0.03) == 0.25 and R.pin(0.125) == 1.0 and R.pin(0.2) == 2.0
    assert R.C_ENTROPY >= 1.0 or R.MEASURED_ENTROPY_RATIO is not None
    if R.MEASURED_ENTROPY_RATIO is not None:
        assert R.C_ENTROPY == R.pin(R.MEASURED_ENTROPY_RATIO)


# --------------------------------------------------------------------------- token_stats_definition
@pytest.mark.parametrize('name', ['tiny', 'unaligned', 'tie', 'uniform', 'spike'])
def test_definition_matches_the_reference(name):
    from tell_amd.models.transformer import token_stats_definition
    case = next(c for c in R.CASES if c['name'] == name)
    ref, (tok, _) = R.reference(name, 33), R.chosen(name, 33)
    for r in range(33):
        for n in R.ALTS:
            d = token_stats_definition(torch.from_numpy(ref['lp'][r].copy()), int(tok[r]), n)
            ids, val = R.top_n(ref['lp'][r], n)
            assert d['alt_ids'].tolist() == ids.tolist() and d['alt_ids'].dtype == torch.long
            assert np.array_equal(d['alt_log_probs'].numpy(), val)
            assert d['token_rank'] == R.rank_of(ref['lp'][r], int(tok[r]))
            assert abs(float(d['token_entropy']) - ref['entropy'][r]) <= 1e-12
            inside = 0 <= tok[r] < R.vocab(case)
            assert float(d['token_model_lp']) == (ref['lp'][r, tok[r]] if inside else 0.0)
            if inside and d['token_rank'] < n:                # the two invariants of the issue
                assert d['alt_ids'][d['token_rank']] == tok[r] and d['alt_log_probs'][d['token_rank']] == d['token_model_lp']
            else:
                assert int(tok[r]) not in d['alt_ids'].tolist()


# --------------------------------------------------------------------------- neutral fill, options, refusals, defaults
def test_neutral_fill_and_option_check():
    from tell_amd.models.transformer import TOKEN_STATS_KEYS, check_token_stats, token_stats_neutral
    t = token_stats_neutral(2, 3, 4, pad=1)
    assert list(t) == list(TOKEN_STATS_KEYS) == ['alt_ids', 'alt_log_probs', 'token_rank', 'token_entropy', 'token_model_lp']
    assert t['alt_ids'].shape == (2, 3, 4) and t['alt_ids'].dtype == torch.long and bool((t['alt_ids'] == 1).all())
    assert t['alt_log_probs'].shape == (2, 3, 4) and t['alt_log_probs'].dtype == torch.float32 and not t['alt_log_probs'].any()
    assert t['token_rank'].shape == (2, 3) and t['token_rank'].dtype == torch.long and bool((t['token_rank'] == -1).all())
    for k in ('token_entropy', 'token_model_lp'):
        assert t[k].shape == (2, 3) and t[k].dtype == torch.float32 and not t[k].any()
    assert [check_token_stats(n) for n in range(9)] == list(range(9)) and check_token_stats() == 0
    for bad in (-1, 9, 2.0, True, '4', None):
        with pytest.raises(ValueError, match='token_stats'):
            check_token_stats(bad)


def test_every_refusal_names_its_reason_with_one_wording():
    from tell_amd.models.baseline_glove import BaselineGloveModel
    from tell_amd.models.pointer import TransformerPointerModel
    from tell_amd.models.stepper import TOKEN_STATS_REFUSALS as MSG, DecodeStepper
    from tell_amd.models.transformer import CaptionModel
    import re
    m = _shell(CaptionModel, _Dyn())
    assert m._check_token_stats() == 0 and m._check_token_stats(0, 4, 4, ('image',)) == 0     # off: nothing is checked
    assert m._check_token_stats(4) == 4
    for kw in (dict(beam_size=4), dict(n_best=2)):                                            # beam search and n_best
        with pytest.raises(ValueError, match=re.escape(MSG['beam'])):
            m._check_token_stats(4, **kw)
    with pytest.raises(ValueError, match=re.escape(MSG['guide'])):                            # guidance
        m._check_token_stats(4, guide=(('image',), 2.0))
    lstm = _shell(CaptionModel, torch.nn.Linear(2, 2))                                        # an LSTM decoder behind the class
    with pytest.raises(ValueError, match=re.escape(MSG['lstm'])):
        lstm._check_token_stats(4)
    glove = BaselineGloveModel.__new__(BaselineGloveModel)                                    # the LSTM baseline
    with pytest.raises(ValueError, match=re.escape(MSG['lstm'])):
        glove.generate(None, None, token_stats=4)
    ptr = _shell(TransformerPointerModel, _Dyn())                                             # the copy models
    with pytest.raises(ValueError, match=re.escape(MSG['copy'])):
        ptr.generate(None, None, None, token_stats=4)
    for gen in (m.generate_lanes([], token_stats=4), m.generate_stream([], token_stats=4)):   # lanes / stream
        with pytest.raises(ValueError, match=re.escape(MSG['lanes'])):
            next(gen)
    # the same wording on the second path: the generator behind generate, and the stepper
    with pytest.raises(ValueError, match=re.escape(MSG['beam'])):
        m._generate(None, None, beam_size=4, token_stats=4)
    with pytest.raises(ValueError, match=re.escape(MSG['guide'])):
        m._generate(None, None, guide=(('image',), 2.0), token_stats=4)
    with pytest.raises(ValueError, match='topk: ' + re.escape(MSG['beam'])):
        DecodeStepper(m, 4, [], {}, 10, topk=4, stats=4)
    with pytest.raises(ValueError, match='guide: ' + re.escape(MSG['guide'])):
        DecodeStepper(m, 4, [], {}, 10, guide=('image',), stats=4)
    with pytest.raises(ValueError, match='stats'):
        DecodeStepper(m, 4, [], {}, 10, stats=9)
    for name, msg in MSG.items():
        assert msg.startswith('token_stats '), name


def test_token_stats_is_an_argument_with_default_zero_and_zero_touches_nothing(monkeypatch):
    from tell_amd.models import stepper
    from tell_amd.models.baseline_glove import BaselineGloveModel
    from tell_amd.models.pointer import TransformerPointerModel
    from tell_amd.models.transformer import CaptionModel
    for fn in (CaptionModel.generate, CaptionModel.generate_lanes, CaptionModel.generate_stream, CaptionModel.score_captions,
               TransformerPointerModel.generate, BaselineGloveModel.generate):
        assert inspect.signature(fn).parameters['token_stats'].default == 0, fn
    from tell_amd.models.gen_options import DecodePlan
    assert inspect.signature(stepper.DecodeStepper.__init__).parameters['stats'].default == 0
    assert DecodePlan().stats == 0
    m = _shell(CaptionModel, _Dyn())
    m.fast_generation = True
    seen = {}

    def cached(self, caption_ids, contexts, gen_len=100, eos=2, **kw):
        seen.update(kw)
        return torch.zeros(1, 1), torch.zeros(1, 2, dtype=torch.long), []
    monkeypatch.setattr(CaptionModel, '_generate_cached', cached)
    monkeypatch.setattr(CaptionModel, '_forward', lambda self, *a, **k: (None, None, None))
    out = m.generate(None, None, None)
    assert 'stats' not in seen and not set(out) & {'alt_ids', 'alt_log_probs', 'token_rank', 'token_entropy', 'token_model_lp'}
    out = m.generate(None, None, None, token_stats=0)
    assert 'stats' not in seen                                                # 0: the call of before, no key handed on
    m.generate(None, None, None, token_stats=3)
    assert seen.get('stats') == 3
    # _generate_cached hands _greedy_steps one plan: the plain one without an option, `stats` in its field when set
    monkeypatch.undo()
    got = {}

    def steps(self, caption_ids, contexts, gen_len, eos, check_every, lane, **kw):
        got.update(kw)
        return (None, None, [])
        yield
    monkeypatch.setattr(CaptionModel, '_greedy_steps', steps)
    m._generate_cached(None, None)
    assert set(got) == {'plan'} and got['plan'] == DecodePlan()
    m._generate_cached(None, None, stats=5)
    assert set(got) == {'plan'} and got['plan'] == DecodePlan(stats=5) and got['plan'].stats == 5


def test_stats_sink_layout_and_neutral_reset():
    from tell_amd.decode import StatsSink
    s = StatsSink(4, 7, 3, pad=1, device='cpu')
    assert s.alt_tok.shape == (7, 3, 4) and s.alt_tok.dtype == torch.int32 and s.alt_lp.shape == (7, 3, 4)
    assert s.rank.shape == s.entropy.shape == s.chosen_lp.shape == (7, 3) and s.rank.dtype == torch.int32
    s.alt_tok.fill_(9), s.rank.fill_(5), s.entropy.fill_(2.0), s.alt_lp.fill_(1.0), s.chosen_lp.fill_(3.0)
    s.reset()
    assert bool((s.alt_tok == 1).all()) and bool((s.rank == -1).all()) and not s.alt_lp.any() and not s.entropy.any() and \
        not s.chosen_lp.any()
    assert s.at(3).step == 3 and s.at(torch.zeros(1, dtype=torch.int32)).step.dtype == torch.int32
    for bad in (0, 9):
        with pytest.raises(ValueError, match='token_stats'):
            StatsSink(bad, 7, 3, 1, 'cpu')
    out = __import__('tell_amd').models.transformer.CaptionModel._token_stats_arrays(s, 5)
    assert out['alt_ids'].shape == (3, 5, 4) and out['alt_ids'].dtype == torch.long and out['token_rank'].shape == (3, 5)
    assert out['token_rank'].dtype == torch.long and out['token_entropy'].dtype == torch.float32


# --------------------------------------------------------------------------- the word-level view
class _Bpe:
    """ids 0..3 are <s> <pad> </s> <unk>; every other id i is the GPT-2 piece number i - 4"""
    PIECES = ['A', 'Ġdog', 'gy', 'Ġruns', 'Ġcat', 'Ġsits', 'ish']

    class _D:
        bos_index, pad_index, eos_index = 0, 1, 2

        def __init__(self, n):
            self.symbols = ['<s>', '<pad>', '</s>', '<unk>'] + [str(i) for i in range(n)]

        def __len__(self):
            return len(self.symbols)

    class _B:
        def __init__(self, pieces):
            self.decoder = dict(enumerate(pieces))
            self.byte_decoder = {'Ġ': ord(' ')}

    def __init__(self):
        self.source_dictionary, self.bpe = self._D(len(self.PIECES)), self._B(self.PIECES)


def test_caption_confidence_on_a_hand_made_generation():
    from tell_amd.models.transformer import CaptionModel
    m = _shell(CaptionModel, _Dyn())
    # row 0: "A doggy runs" </s>, then padding; row 1: "A cat" and never ends
    gen = {'gen_ids': torch.tensor([[0, 4, 5, 6, 7, 2, 1], [0, 4, 8, 1, 1, 1, 1]]),
           'alt_ids': torch.tensor([[[4, 8], [5, 8], [6, 10], [7, 9], [2, 7], [1, 1]],
                                    [[8, 4], [8, 5], [1, 1], [1, 1], [1, 1], [1, 1]]]),
           'token_rank': torch.tensor([[0, 0, 0, 0, 0, -1], [1, 0, -1, -1, -1, -1]]),
           'token_entropy': torch.tensor([[0.5, 2.0, 0.25, 1.0, 0.125, 0.0], [3.0, 0.75, 0.0, 0.0, 0.0, 0.0]]),
           'token_model_lp': torch.tensor([[-0.5, -1.0, -0.25, -2.0, -0.125, 0.0], [-3.0, -0.5, 0.0, 0.0, 0.0, 0.0]])}
    view = m.caption_confidence({}, gen, bpe=_Bpe())
    assert [w['tokens'] for w in view[0]] == ['A', ' doggy', ' runs'] and [w['tokens'] for w in view[1]] == ['A', ' cat']
    dog = view[0][1]
    assert dog['log_prob'] == -1.25 and dog['entropy'] == 2.0 and dog['rank'] == 0 and dog['alternatives'] == [' dog', ' cat']
    assert view[0][2] == {'tokens': ' runs', 'log_prob': -2.0, 'entropy': 1.0, 'rank': 0, 'alternatives': [' runs', ' sits']}
    assert view[1][0]['rank'] == 1 and view[1][0]['alternatives'] == [' cat', 'A'] and view[1][0]['log_prob'] == -3.0
    with pytest.raises(ValueError, match='token_stats'):
        m.caption_confidence({}, {'gen_ids': gen['gen_ids']}, bpe=_Bpe())


# --------------------------------------------------------------------------- the rank interval of the score_captions test
def test_the_reference_admits_one_rank_for_most_tokens_of_the_score_batch():
    """The GPU test holds score_captions(token_stats=4) ranks to R.rank_interval at section 27's tolerance.  On the CPU oracle
    alone (the same weights, the same batch, teacher-forced, full log-probs) the interval is a single value for at least 90 % of
    the batch's caption tokens - the check has teeth."""
    from oracle.build import build_model as oracle_model
    from tell_amd.data import synthetic_batch
    gpu = R.score_model()
    cpu = oracle_model('faces_objects', *R.score_encoders(False), n_bert_layers=3, **R.SCORE_KW).eval()
    cpu.load_state_dict({k: v for k, v in gpu.state_dict().items() if k in cpu.state_dict()}, strict=False)
    batch = synthetic_batch(**R.SCORE_BATCH)
    cap = batch['caption']['roberta'].clone()
    with torch.no_grad():
        _, target, contexts = cpu._forward(**{k: (dict(v) if isinstance(v, dict) else v.clone()) for k, v in batch.items()})
        out = cpu.decoder({'roberta': cap[:, :-1]}, contexts)
        lp = cpu.decoder.get_normalized_probs((out[0], None), log_probs=True).double().numpy()
    single = total = 0
    for b in range(cap.shape[0]):
        for t in range(cap.shape[1] - 1):
            c = int(cap[b, t + 1])
            if c == 1:
                continue
            lo, hi = R.rank_interval(lp[b, t], c)
            assert lo <= R.rank_of(lp[b, t], c) <= hi
            single += lo == hi
            total += 1
    print('score batch: %d caption tokens, rank interval single-valued for %d (%.1f %%)' % (total, single, 100.0 * single / total))
    assert total >= 30 and single >= 0.9 * total
