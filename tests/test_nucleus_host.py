"""CPU checks of nucleus (top-p) sampling (include/tell_hip.h tell_adaptive_logprob_nucleus): the fp64
definition on hand-made rows, the models' `sampling_topp`, and the declared / exported entry points."""
import math

import numpy as np
import pytest
import torch

from test_abi_and_host import _write_cfg
from test_sampling_host import _builders


def _lp(probs):
    return np.log(np.asarray(probs, dtype=np.float64))


def test_definition_hand_made():
    from tell_amd.models.transformer import nucleus_definition as nd
    lp = _lp([0.1, 0.4, 0.05, 0.3, 0.15])                     # by value: ids 1, 3, 4, 0, 2 - cumulative .4 .7 .85 .95 1
    assert nd(lp, 1.0, 0.5)['members'].tolist() == [1, 3]
    assert nd(lp, 1.0, 0.7 - 1e-9)['members'].tolist() == [1, 3]
    assert nd(lp, 1.0, 0.71)['members'].tolist() == [1, 3, 4]
    assert nd(lp, 1.0, 0.9)['members'].tolist() == [0, 1, 3, 4]
    assert nd(lp, 1.0, 1.0)['members'].tolist() == [0, 1, 2, 3, 4]      # p = 1: every token
    for p in (1e-9, 1e-3, 0.4 - 1e-9):                        # a tiny p: the best token alone, whatever u
        r = nd(lp, 1.0, p, u=0.999)
        assert r['members'].tolist() == [1] and r['token'] == 1
    r = nd(lp, 1.0, 0.5)
    assert math.isclose(r['boundary'], math.log(0.3)) and math.isclose(r['margin'], 0.1)     # min(.7 - .5, .5 - .4)
    # the draw walks the members in TOKEN-ID order: ids 0 (.1), 1 (.4), 3 (.3), 4 (.15) -> edges .1 .5 .8 .95 of .95
    edges = np.array([0.1, 0.5, 0.8, 0.95]) / 0.95
    for tok, lo, hi in zip((0, 1, 3, 4), np.r_[0.0, edges[:-1]], edges):
        assert nd(lp, 1.0, 0.9, u=(lo + hi) / 2)['token'] == tok
        assert nd(lp, 1.0, 0.9, u=lo + 1e-12)['token'] == tok
    assert nd(lp, 1.0, 0.9, u=0.0)['token'] == 0
    assert nd(lp, 1.0, 0.9, u=1.0 - 2.0 ** -24)['token'] == 4
    # the temperature acts before the cut: T = 0.5 squares the probabilities (.01 .16 .0025 .09 .0225 of .285)
    assert nd(lp, 0.5, 0.5)['members'].tolist() == [1]
    assert nd(lp, 0.5, 0.6)['members'].tolist() == [1, 3]
    assert nd(lp, 1e6, 0.5)['members'].tolist() == [1, 3, 4]            # a huge T: uniform weights, ceil(.5 * 5) tokens


def test_definition_ties_enter_in_id_order():
    from tell_amd.models.transformer import nucleus_definition as nd
    lp = _lp([0.125, 0.25, 0.125, 0.125, 0.25, 0.125])         # by (value, id): 1, 4, then the four ties 0, 2, 3, 5
    assert nd(lp, 1.0, 0.25)['members'].tolist() == [1]
    assert nd(lp, 1.0, 0.3)['members'].tolist() == [1, 4]
    assert nd(lp, 1.0, 0.55)['members'].tolist() == [0, 1, 4]
    assert nd(lp, 1.0, 0.7)['members'].tolist() == [0, 1, 2, 4]
    assert nd(lp, 1.0, 0.8)['members'].tolist() == [0, 1, 2, 3, 4]
    assert nd(lp, 1.0, 0.9)['members'].tolist() == [0, 1, 2, 3, 4, 5]
    flat = np.zeros(7)                                         # all equal: the first ceil(p * 7) ids
    assert nd(flat, 1.0, 0.5)['members'].tolist() == [0, 1, 2, 3]
    assert nd(flat, 0.3, 1e-6)['members'].tolist() == [0]


def test_definition_topk_and_topp_together():
    from tell_amd.models.transformer import nucleus_definition as nd
    lp = _lp([0.1, 0.4, 0.05, 0.3, 0.15])
    assert nd(lp, 1.0, 1.0, topk=3)['members'].tolist() == [1, 3, 4]
    assert nd(lp, 1.0, 0.8, topk=3)['members'].tolist() == [1, 3]       # .7 of .85 = .82 >= .8
    assert nd(lp, 1.0, 0.83, topk=3)['members'].tolist() == [1, 3, 4]
    assert nd(lp, 1.0, 0.9, topk=2)['members'].tolist() == [1, 3]
    r = nd(lp, 1.0, 1.0, topk=3, u=0.5)                        # id order 1 (.4), 3 (.3), 4 (.15) of .85: .5 * .85 = .425 -> 3
    assert r['token'] == 3
    one = np.array([-0.0])                                     # a one-token distribution
    for p in (1e-6, 0.5, 1.0):
        r = nd(one, 0.7, p, u=0.73)
        assert r['members'].tolist() == [0] and r['token'] == 0
    assert nd(_lp([1e-30, 1.0]), 1.0, 0.999999)['members'].tolist() == [1]


def test_check_sampling_third_argument():
    from tell_amd.models.transformer import check_sampling
    assert check_sampling(5, 0.7) == (5, 0.7) and check_sampling(1, 1.0) == (1, 1.0)
    assert check_sampling(5, 0.7, None) == (5, 0.7)
    with pytest.raises(ValueError):
        check_sampling(0, 1.0)
    assert check_sampling(0, 0.7, 0.9) == (0, 0.7, 0.9)
    assert check_sampling(64, 1.0, 1) == (64, 1.0, 1.0) and check_sampling(2, 1.0, 1e-6) == (2, 1.0, 1e-6)
    for bad in (True, False, 'x', 0, 0.0, -0.1, 1.0001, 2, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            check_sampling(0, 1.0, bad)
    for bad_k in (65, -1, 2.5, True, 'x'):
        with pytest.raises(ValueError):
            check_sampling(bad_k, 1.0, 0.9)
    with pytest.raises(ValueError, match='sampling_topk=0'):
        check_sampling(1, 1.0, 0.9)
    for bad_t in (0.0, -1.0, float('nan'), float('inf'), True):
        with pytest.raises(ValueError):
            check_sampling(0, bad_t, 0.9)


@pytest.mark.parametrize('kind', ['faces_objects', 'flattened', 'transformer_glove', 'baseline_glove'])
def test_every_model_takes_sampling_topp(kind):
    make = _builders()[kind]
    m = make(sampling_topk=0, sampling_topp=0.9, sampling_temp=0.7)
    assert (m.sampling_topk, m.sampling_temp, m.sampling_topp) == (0, 0.7, 0.9)
    assert make(sampling_topk=40, sampling_topp=1).sampling_topp == 1.0
    assert make().sampling_topp is None and make(sampling_topk=20).sampling_topp is None
    with pytest.raises(ValueError):                            # without sampling_topp, k = 0 stays an error
        make(sampling_topk=0)
    with pytest.raises(ValueError, match='sampling_topk=0'):   # the default k = 1 is the arg-max: not with a nucleus
        make(sampling_topp=0.9)
    for bad in (dict(sampling_topp=0), dict(sampling_topp=1.5), dict(sampling_topp=True), dict(sampling_topp='0.9'),
                dict(sampling_topp=float('nan')), dict(sampling_topp=-0.5)):
        with pytest.raises(ValueError):
            make(sampling_topk=0, **bad)
    for bad_k in (65, 2.5, -3):
        with pytest.raises(ValueError):
            make(sampling_topk=bad_k, sampling_topp=0.9)
    with pytest.raises(ValueError):
        make(sampling_topk=0, sampling_topp=0.9, sampling_temp=0.0)


def test_sampling_state_and_graph_key():
    make = _builders()['flattened']
    assert make()._sampling() is None                                            # greedy: unchanged
    assert make(sampling_topk=20, sampling_temp=0.7)._sampling() == (20, 0.7)    # top-k: unchanged
    assert make(sampling_topk=0, sampling_topp=0.9)._sampling() == (0, 1.0, 0.9)
    assert make(sampling_topk=8, sampling_topp=0.5, sampling_temp=2)._sampling() == (8, 2.0, 0.5)


def test_pointer_model_takes_sampling_topp():
    from tell_amd.build import build_model
    kw = dict(vocab_size=600, dim=64, heads=4, ffn=128, cutoff=(100, 300))
    m = build_model('pointer', object(), object(), n_bert_layers=3, sampling_topk=0, sampling_topp=0.9, **kw)
    assert m._sampling() == (0, 1.0, 0.9)
    assert build_model('pointer_2', object(), object(), n_bert_layers=3, sampling_topk=16, sampling_topp=0.5,
                       **kw)._sampling() == (16, 1.0, 0.5)
    with pytest.raises(ValueError):                            # top-k alone stays refused by the pointer models
        build_model('pointer', object(), object(), n_bert_layers=3, sampling_topk=5, **kw)
    with pytest.raises(ValueError, match='sampling_topk=0'):
        build_model('pointer', object(), object(), n_bert_layers=3, sampling_topp=0.9, **kw)


@pytest.mark.parametrize('kind', ['flattened', 'faces_objects'])
def test_yaml_config_with_sampling_topp(tmp_path, kind):
    from tell_amd import config
    path = _write_cfg(tmp_path, kind)
    model, _ = config.from_config(path, overrides='{"model": {"sampling_topk": 0, "sampling_topp": 0.9, "sampling_temp": 0.7}}',
                                  resnet=object(), roberta=object())
    assert (model.sampling_topk, model.sampling_temp, model.sampling_topp) == (0, 0.7, 0.9)
    assert model._sampling() == (0, 0.7, 0.9)
    for over in ('{"model": {"sampling_topp": 0.9}}', '{"model": {"sampling_topk": 0, "sampling_topp": 0}}',
                 '{"model": {"sampling_topk": 0, "sampling_topp": 1.5}}', '{"model": {"sampling_topk": 0, "sampling_topp": "p"}}',
                 '{"model": {"sampling_topk": 65, "sampling_topp": 0.9}}', '{"model": {"sampling_topk": 0, "sampling_topp": true}}'):
        with pytest.raises(ValueError):
            config.from_config(path, overrides=over, resnet=object(), roberta=object())


def test_beam_search_and_nucleus_do_not_combine():
    model = _builders()['flattened'](sampling_topk=0, sampling_topp=0.9)
    with pytest.raises(ValueError, match='nucleus'):
        model._generate(torch.zeros(2, 1, dtype=torch.long), {}, beam_size=4)
    with pytest.raises(ValueError, match='nucleus'):
        next(model.generate_lanes(iter([]), beam_size=4))


def test_nucleus_symbols_declared_and_exported():
    import tell_amd
    protos = tell_amd.hip.parse_header()
    _, argtypes, names = protos['tell_adaptive_logprob_nucleus']
    _, _, sample_names = protos['tell_adaptive_logprob_sample']
    i = sample_names.index('inv_temp')                        # the top-k entry's operands plus p and the optional outputs
    assert names == sample_names[:i + 1] + ['p'] + sample_names[i + 1:-1] + ['nuc_size', 'nuc_key', 'stream']
    assert 'tell_nucleus_candidates' in protos
    lib = tell_amd.hip.lib()
    assert hasattr(lib, 'tell_adaptive_logprob_nucleus') and hasattr(lib, 'tell_nucleus_candidates')
