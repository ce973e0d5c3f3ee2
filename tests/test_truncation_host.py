"""CPU checks of min-p and locally typical sampling (include/tell_hip.h tell_adaptive_logprob_minp / _typical, DESIGN.md section
19): the definitions on hand-made rows and at their fixed points, the models' `sampling_minp` / `sampling_typical` and what
they refuse, the unchanged results of check_sampling, and the declared / exported entry points."""
import math

import numpy as np
import pytest
import torch

from test_abi_and_host import _write_cfg
from test_sampling_host import _builders


def _lp(probs):
    return np.log(np.asarray(probs, dtype=np.float64))


def test_minp_definition_hand_made():
    from tell_amd.models.transformer import minp_definition as md
    lp = _lp([0.1, 0.4, 0.05, 0.3, 0.15])                     # ratios to the best: .25 1 .125 .75 .375
    assert md(lp, 1.0, 0.8)['members'].tolist() == [1]
    assert md(lp, 1.0, 0.7)['members'].tolist() == [1, 3]
    assert md(lp, 1.0, 0.3)['members'].tolist() == [1, 3, 4]
    assert md(lp, 1.0, 0.2)['members'].tolist() == [0, 1, 3, 4]
    assert md(lp, 1.0, 0.1)['members'].tolist() == [0, 1, 2, 3, 4]
    # the temperature acts before the cut: T = 0.5 squares the ratios (.0625 1 .0156 .5625 .1406)
    assert md(lp, 0.5, 0.5)['members'].tolist() == [1, 3]
    assert md(lp, 0.5, 0.6)['members'].tolist() == [1]
    assert md(lp, 2.0, 0.6)['members'].tolist() == [1, 3, 4]  # T = 2: square roots (.5 1 .354 .866 .612)
    # the draw walks the members in TOKEN-ID order: ids 0 (.1), 1 (.4), 3 (.3), 4 (.15) -> edges .1 .5 .8 .95 of .95
    edges = np.array([0.1, 0.5, 0.8, 0.95]) / 0.95
    for tok, lo, hi in zip((0, 1, 3, 4), np.r_[0.0, edges[:-1]], edges):
        r = md(lp, 1.0, 0.2, u=(lo + hi) / 2)
        assert r['token'] == tok
        np.testing.assert_allclose(r['cdf'], edges, rtol=1e-6)
    assert md(lp, 1.0, 0.2, u=0.0)['token'] == 0 and md(lp, 1.0, 0.2, u=1.0 - 2.0 ** -24)['token'] == 4
    assert md(lp, 1.0, 0.2)['threshold'] == np.float32(math.log(0.2)) and md(lp, 1.0, 0.2)['token'] is None


def test_minp_definition_fixed_points():
    from tell_amd.models.transformer import minp_definition as md
    g = np.random.default_rng(3)
    lp = g.standard_normal(300) * 3
    lp[[7, 150, 299]] = lp.max() + 0.5                         # three tokens tie at the top
    lp -= np.log(np.exp(lp).sum())
    for T in (0.7, 1.0, 1.3):
        assert md(lp, T, 1e-30)['members'].tolist() == list(range(300))          # a tiny m: the whole row
        assert md(lp, T, 1.0)['members'].tolist() == [7, 150, 299]               # m = 1: the arg-max ties
        for m in (0.02, 0.1, 0.5):
            assert {7, 150, 299} <= set(md(lp, T, m)['members'].tolist())        # the best tokens are always members
    # a constant added to lp changes nothing.  The statement is fp32, so the shift must be exact there: values on a grid
    # of 1 / 256 and a shift of 4
    q = np.round(lp * 256) / 256
    for T in (0.7, 1.0, 1.3):
        for m in (0.02, 0.1, 0.5, 1.0):
            a, b = md(q, T, m, u=0.37), md(q + 4.0, T, m, u=0.37)
            assert a['members'].tolist() == b['members'].tolist() and a['token'] == b['token']
            np.testing.assert_allclose(a['cdf'], b['cdf'], rtol=1e-12)
    sizes = [len(md(lp, 1.0, m)['members']) for m in (1.0, 0.5, 0.1, 0.02, 1e-6)]
    assert sizes == sorted(sizes) and sizes[0] == 3 and sizes[-1] > sizes[0]     # a smaller m never loses a member


def test_typical_definition_hand_made():
    from tell_amd.models.transformer import typical_definition as td
    p = np.array([0.1, 0.4, 0.05, 0.3, 0.15])
    lp = np.log(p)
    H = -(p * lp).sum()                                        # 1.3927 nats; surprises 2.303 .916 2.996 1.204 1.897
    d = np.abs(-lp - H)                                        # .910 .476 1.603 .189 .504 -> order 3, 1, 4, 0, 2
    assert np.argsort(d).tolist() == [3, 1, 4, 0, 2]
    r = td(lp, 1.0, 0.5)
    assert math.isclose(r['c'], H + math.log(0.4))             # the entropy minus the surprise of the best token
    assert td(lp, 1.0, 0.2)['members'].tolist() == [3]         # cumulative .3 .7 .85 .95 1
    assert td(lp, 1.0, 0.3 - 1e-9)['members'].tolist() == [3]
    assert td(lp, 1.0, 0.31)['members'].tolist() == [1, 3]
    assert r['members'].tolist() == [1, 3] and math.isclose(r['boundary'], d[1]) and math.isclose(r['margin'], 0.2)
    assert td(lp, 1.0, 0.8)['members'].tolist() == [1, 3, 4]
    assert td(lp, 1.0, 0.9)['members'].tolist() == [0, 1, 3, 4]
    assert td(lp, 1.0, 1.0)['members'].tolist() == [0, 1, 2, 3, 4]
    # the best token is NOT always a member: the head can be too probable to be typical
    assert 1 not in td(lp, 1.0, 0.25)['members']
    # the draw: members 1 (.4), 3 (.3) in id order -> edge 4/7
    assert td(lp, 1.0, 0.5, u=0.5)['token'] == 1 and td(lp, 1.0, 0.5, u=0.6)['token'] == 3
    np.testing.assert_allclose(td(lp, 1.0, 0.5)['cdf'], [4 / 7, 1.0])
    # the key is the inverted bit pattern of float32(boundary)
    key = td(lp, 1.0, 0.5)['key']
    assert (~np.uint32(key)).view(np.float32) == np.float32(d[1])
    # T = 0.5: p^2 normalised (.0351 .5614 .0088 .3158 .0789), H = 1.049, surprises 3.35 .577 4.74 1.153 2.54 -> order 3, 1, ...
    r = td(lp, 0.5, 0.3)
    assert r['members'].tolist() == [3] and td(lp, 0.5, 0.5)['members'].tolist() == [1, 3]


def test_typical_definition_fixed_points_and_ties():
    from tell_amd.models.transformer import typical_definition as td
    g = np.random.default_rng(5)
    lp = g.standard_normal(400) * 2.5
    lp -= np.log(np.exp(lp).sum())
    for T in (0.7, 1.0, 1.3):
        assert td(lp, T, 1.0)['members'].tolist() == list(range(400))            # tau = 1: the whole row
        for tau in (0.2, 0.9, 0.95):
            a, b = td(lp, T, tau, u=0.41), td(lp + 7.5, T, tau, u=0.41)          # a constant added to lp changes nothing
            assert a['members'].tolist() == b['members'].tolist() and a['token'] == b['token']
            assert math.isclose(a['c'], b['c'], rel_tol=1e-9) and a['c'] >= 0.0
            # the fp32 order under the fp64 c rounded: the same set unless the boundary is within rounding
            c32 = td(lp.astype(np.float32), T, tau, c=np.float32(a['c']))
            if a['margin'] > 1e-3:
                assert abs(len(c32['members']) - len(a['members'])) <= 1
        sizes = [len(td(lp, T, tau)['members']) for tau in (0.05, 0.2, 0.5, 0.9, 0.95, 1.0)]
        assert sizes == sorted(sizes) and sizes[0] >= 1
    flat = np.zeros(7)                                         # all equal: c = 0, d = 0, ties enter in id order
    assert td(flat, 1.0, 0.5)['members'].tolist() == [0, 1, 2, 3] and td(flat, 1.0, 0.5)['c'] == 0.0
    assert td(flat, 0.3, 1e-6)['members'].tolist() == [0]
    one = np.array([-0.0])
    assert td(one, 0.7, 0.5, u=0.9)['token'] == 0
    # tokens at the same distance enter in id order until the mass is reached (a given c = 0: d = |a|, ids 1 and 2 tie)
    p = np.array([0.5, 0.25, 0.25])
    r = td(np.log(p), 1.0, 0.4, c=np.float32(0.0))
    assert r['members'].tolist() == [0]
    r = td(np.log(p), 1.0, 0.6, c=np.float32(0.0))
    assert r['members'].tolist() == [0, 1]


def test_check_sampling_old_results_are_unchanged():
    from tell_amd.models.transformer import check_sampling
    assert check_sampling(5, 0.7) == (5, 0.7) and check_sampling(1, 1.0) == (1, 1.0)
    assert check_sampling(5, 0.7, None) == (5, 0.7) and check_sampling(5, 0.7, None, None, None) == (5, 0.7)
    assert check_sampling(0, 0.7, 0.9) == (0, 0.7, 0.9) and check_sampling(64, 1.0, 1) == (64, 1.0, 1.0)
    assert check_sampling(8, 2, 0.5, sampling_minp=None, sampling_typical=None) == (8, 2.0, 0.5)
    with pytest.raises(ValueError):
        check_sampling(0, 1.0)
    with pytest.raises(ValueError, match='sampling_topk=0'):
        check_sampling(1, 1.0, 0.9)


def test_check_sampling_new_arguments():
    from tell_amd.models.transformer import check_sampling
    assert check_sampling(0, 0.7, sampling_minp=0.1) == (0, 0.7, 0.1, 'minp')
    assert check_sampling(0, 1, sampling_typical=1) == (0, 1.0, 1.0, 'typical')
    assert check_sampling(0, 1.3, None, None, 0.9) == (0, 1.3, 0.9, 'typical')
    for name in ('sampling_minp', 'sampling_typical'):
        for bad in (True, False, 'x', 0, 0.0, -0.1, 1.0001, 2, float('nan'), float('inf')):
            with pytest.raises(ValueError, match=name):
                check_sampling(0, 1.0, **{name: bad})
        for bad_k in (1, 2, 5, 64, -1, True, 'x', 2.5):
            with pytest.raises(ValueError, match=name):
                check_sampling(bad_k, 1.0, **{name: 0.5})
        for bad_t in (0.0, -1.0, float('nan'), float('inf'), True):
            with pytest.raises(ValueError):
                check_sampling(0, bad_t, **{name: 0.5})
    for two in (dict(sampling_topp=0.9, sampling_minp=0.1), dict(sampling_topp=0.9, sampling_typical=0.9),
                dict(sampling_minp=0.1, sampling_typical=0.9), dict(sampling_topp=0.9, sampling_minp=0.1, sampling_typical=0.9)):
        with pytest.raises(ValueError) as e:
            check_sampling(0, 1.0, **two)
        assert all(k in str(e.value) for k in two)


@pytest.mark.parametrize('kind', ['faces_objects', 'flattened', 'transformer_glove'])
def test_cached_generator_models_take_the_options(kind):
    make = _builders()[kind]
    m = make(sampling_topk=0, sampling_minp=0.1, sampling_temp=0.7)
    assert (m.sampling_topk, m.sampling_temp, m.sampling_minp, m.sampling_typical, m.sampling_topp) == (0, 0.7, 0.1, None, None)
    assert m._sampling() == (0, 0.7, 0.1, 'minp')
    m = make(sampling_topk=0, sampling_typical=0.9)
    assert (m.sampling_minp, m.sampling_typical) == (None, 0.9) and m._sampling() == (0, 1.0, 0.9, 'typical')
    d = make()                                                 # the defaults, and what the older options report
    assert d.sampling_minp is None and d.sampling_typical is None and d._sampling() is None
    assert make(sampling_topk=20, sampling_temp=0.7)._sampling() == (20, 0.7)
    assert make(sampling_topk=0, sampling_topp=0.9)._sampling() == (0, 1.0, 0.9)
    for name in ('sampling_minp', 'sampling_typical'):
        with pytest.raises(ValueError, match=name):            # the default k = 1 is the arg-max
            make(**{name: 0.5})
        for bad in (0, 1.5, True, '0.9', float('nan'), -0.5):
            with pytest.raises(ValueError, match=name):
                make(sampling_topk=0, **{name: bad})
        with pytest.raises(ValueError, match=name):
            make(sampling_topk=0, sampling_topp=0.9, **{name: 0.5})
        for opt in (dict(beam_len_penalty=1.0), dict(no_repeat_ngram_size=3), dict(min_len=5)):
            with pytest.raises(ValueError, match=name):
                make(sampling_topk=0, **{name: 0.5}, **opt)
    with pytest.raises(ValueError, match='sampling_minp'):
        make(sampling_topk=0, sampling_minp=0.1, sampling_typical=0.9)


def test_generate_refuses_beams_and_n_best():
    for name in ('sampling_minp', 'sampling_typical'):
        model = _builders()['flattened'](sampling_topk=0, **{name: 0.5})
        with pytest.raises(ValueError, match=name):
            model._generate(torch.zeros(2, 1, dtype=torch.long), {}, beam_size=4)
        with pytest.raises(ValueError, match=name):
            next(model.generate_lanes(iter([]), beam_size=4))
        with pytest.raises(ValueError, match=name):
            model._check_options(beam_size=4, n_best=2)


def test_lstm_and_copy_models_refuse_the_options():
    from tell_amd.build import build_model
    kw = dict(vocab_size=600, dim=64, heads=4, ffn=128, cutoff=(100, 300))
    for name in ('sampling_minp', 'sampling_typical'):
        with pytest.raises(ValueError, match=name):
            _builders()['baseline_glove'](sampling_topk=0, **{name: 0.5})
        for kind in ('pointer', 'pointer_2'):
            with pytest.raises(ValueError, match=name):
                build_model(kind, object(), object(), n_bert_layers=3, sampling_topk=0, **{name: 0.5}, **kw)
            with pytest.raises(ValueError, match=name):
                build_model(kind, object(), object(), n_bert_layers=3, **{name: 0.5}, **kw)
    assert _builders()['baseline_glove'](sampling_topk=0, sampling_topp=0.9).sampling_topp == 0.9      # (as before)
    assert build_model('pointer', object(), object(), n_bert_layers=3, sampling_topk=0, sampling_topp=0.9, **kw)._sampling() \
        == (0, 1.0, 0.9)


@pytest.mark.parametrize('kind', ['flattened', 'faces_objects'])
def test_yaml_config_with_the_options(tmp_path, kind):
    from tell_amd import config
    path = _write_cfg(tmp_path, kind)
    model, _ = config.from_config(path, overrides='{"model": {"sampling_topk": 0, "sampling_minp": 0.05, "sampling_temp": 0.7}}',
                                  resnet=object(), roberta=object())
    assert model._sampling() == (0, 0.7, 0.05, 'minp')
    model, _ = config.from_config(path, overrides='{"model": {"sampling_topk": 0, "sampling_typical": 0.9}}',
                                  resnet=object(), roberta=object())
    assert model._sampling() == (0, 1.0, 0.9, 'typical')
    for over in ('{"model": {"sampling_minp": 0.1}}', '{"model": {"sampling_topk": 0, "sampling_minp": 0}}',
                 '{"model": {"sampling_topk": 0, "sampling_typical": 1.5}}', '{"model": {"sampling_topk": 0, "sampling_typical": "t"}}',
                 '{"model": {"sampling_topk": 5, "sampling_minp": 0.1}}',
                 '{"model": {"sampling_topk": 0, "sampling_minp": 0.1, "sampling_topp": 0.9}}'):
        with pytest.raises(ValueError):
            config.from_config(path, overrides=over, resnet=object(), roberta=object())


def test_symbols_declared_and_exported():
    import tell_amd
    protos = tell_amd.hip.parse_header()
    _, _, nuc = protos['tell_adaptive_logprob_nucleus']
    _, _, minp = protos['tell_adaptive_logprob_minp']
    _, _, typ = protos['tell_adaptive_logprob_typical']
    rows, draw = nuc[:nuc.index('k')], nuc[nuc.index('seed_dev'):nuc.index('nuc_size')]
    assert minp == rows + ['inv_temp', 'log_minp'] + draw + ['nuc_size', 'stream']
    assert typ == rows + ['inv_temp', 'tau'] + draw + ['nuc_size', 'nuc_key', 'typ_c', 'stream']
    lib = tell_amd.hip.lib()
    assert hasattr(lib, 'tell_adaptive_logprob_minp') and hasattr(lib, 'tell_adaptive_logprob_typical')
