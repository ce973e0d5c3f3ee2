"""CPU checks of top-k sampling (include/tell_hip.h tell_adaptive_logprob_sample): the numpy restatement of the sampling
uniform against the library's host twin, its statistics, the fp32 pick, and the models' sampling_topk / sampling_temp."""
import numpy as np
import pytest
import torch

from test_abi_and_host import _write_cfg


def test_sample_uniform_restatement_matches_c():
    import tell_amd
    from tell_amd import rng
    lib = tell_amd.hip.lib()
    rows = [0, 1, 2, 7, 31, 1000, (1 << 20) - 1, 1 << 20, (1 << 20) + 3, 1 << 24, (1 << 31) + 5, (1 << 32) - 1]
    steps = np.arange(101)
    for seed in (0, 1, 0x5EED, 123456789, (1 << 31) - 1, 0xFFFFFFFF):
        for row in rows:
            want = np.array([lib.tell_sample_uniform_host(seed, row, int(t)) for t in steps], dtype=np.float32)
            got = rng.sample_uniform(seed, row, steps)
            assert got.dtype == np.float32 and np.array_equal(got, want), (seed, row)
    assert ((want >= 0) & (want < 1)).all()


def test_sample_uniform_statistics():
    """Mean and 256-bin chi2 of u over (row, step) grids, and no correlation between neighbouring rows, steps or seeds."""
    from tell_amd import rng
    rows, steps = np.meshgrid(np.arange(1 << 12), np.arange(256), indexing='ij')
    n = rows.size
    sd = 1.0 / np.sqrt(n)
    for seed in (1, 12345, 0x7FFFFFFF):
        u = rng.sample_uniform(seed, rows, steps).astype(np.float64)
        assert abs(u.mean() - 0.5) < 5 * np.sqrt(1.0 / 12) * sd
        cnt = np.bincount((u * 256).astype(np.int64).ravel(), minlength=256).astype(float)
        exp = n / 256.0
        assert ((cnt - exp) ** 2 / exp).sum() < 350.0                  # chi2, 255 dof: p ~ 1e-4
        c = u - 0.5
        for a, b in ((c[:-1, :], c[1:, :]), (c[:, :-1], c[:, 1:]), (c[:-2, :], c[2:, :]), (c[:, :-2], c[:, 2:])):
            assert abs(float((a * b).mean()) / (1.0 / 12)) < 6 * sd
        other = rng.sample_uniform(seed + 1, rows, steps).astype(np.float64) - 0.5
        assert abs(float((c * other).mean()) / (1.0 / 12)) < 6 * sd
    # rows far apart in the index space (the original batch rows of large batches)
    big = rng.sample_uniform(9, np.arange(1 << 20, (1 << 20) + (1 << 16)), 3).astype(np.float64)
    assert abs(big.mean() - 0.5) < 5 * np.sqrt(1.0 / 12) / np.sqrt(big.size)


def test_sample_pick_hand_made():
    from tell_amd import rng
    lps = np.array([-0.5, -1.0, -1.5, -4.0, -9.0], dtype=np.float32)
    assert rng.sample_pick(lps, 1.0, 0.0) == 0
    assert rng.sample_pick(lps, 1.0, np.float32(1.0 - 2 ** -24)) == 4          # u -> 1 picks k - 1
    assert rng.sample_pick(lps, 1.0, 0.9999999) == 4
    for u in (0.0, 0.3, 0.999999):
        assert rng.sample_pick(lps[:1], 0.7, u) == 0                          # k = 1
    # the pick follows the CDF of exp(lp / T), normalised
    w = np.exp(lps.astype(np.float64))
    cdf = np.cumsum(w) / w.sum()
    for j in range(len(lps)):
        lo = 0.0 if j == 0 else cdf[j - 1]
        assert rng.sample_pick(lps, 1.0, (lo + cdf[j]) / 2) == j
    # a huge temperature: near-uniform over the k candidates
    us = (np.arange(5000) + 0.5) / 5000
    picks = np.array([rng.sample_pick(lps, 1e-6, u) for u in us])
    cnt = np.bincount(picks, minlength=5)
    assert (abs(cnt - 1000) <= 2).all(), cnt
    # a tiny temperature: the best candidate
    assert all(rng.sample_pick(lps, 1e3, u) == 0 for u in (0.0, 0.5, 0.999))


def _lstm_decoder():
    from tell_amd.build import build_embedder
    from tell_amd.models import LSTMDecoder
    return LSTMDecoder(None, build_embedder(600, 64, (100, 300), 512), num_layers=2, hidden_size=48, dropout=0.1,
                       share_decoder_input_output_embed=True, vocab_size=600, adaptive_softmax_cutoff=[100, 300],
                       tie_adaptive_weights=True, adaptive_softmax_dropout=0, tie_adaptive_proj=False,
                       adaptive_softmax_factor=1, article_embed_size=300, image_embed_size=2048)


def _builders():
    from tell_amd.build import build_decoder, build_model
    from tell_amd.models import BaselineGloveModel, TransformerGloveModel
    from tell_amd.modules import AdaptiveLoss
    kw = dict(vocab_size=600, dim=64, heads=4, ffn=128, cutoff=(100, 300))
    return {
        'faces_objects': lambda **s: build_model('faces_objects', object(), object(), n_bert_layers=3, **kw, **s),
        'flattened': lambda **s: build_model('flattened', object(), object(), n_bert_layers=3, article_dim=64, **kw, **s),
        'transformer_glove': lambda **s: TransformerGloveModel(None, build_decoder('flattened', article_dim=300, **kw),
                                                               AdaptiveLoss(1), vocab_size=600, resnet=object(), **s),
        'baseline_glove': lambda **s: BaselineGloveModel(None, _lstm_decoder(), AdaptiveLoss(1), resnet=object(), **s),
    }


@pytest.mark.parametrize('kind', ['faces_objects', 'flattened', 'transformer_glove', 'baseline_glove'])
def test_every_model_takes_sampling_topk_and_temp(kind):
    make = _builders()[kind]
    m = make(sampling_topk=20, sampling_temp=0.7)
    assert (m.sampling_topk, m.sampling_temp) == (20, 0.7)
    assert make(sampling_topk=64, sampling_temp=2.0).sampling_topk == 64
    assert make().sampling_topk == 1
    for bad in (dict(sampling_topk=0), dict(sampling_topk=65), dict(sampling_topk=2.5), dict(sampling_topk=True),
                dict(sampling_temp=0.0), dict(sampling_temp=-1.0), dict(sampling_temp=float('nan')),
                dict(sampling_topk=5, sampling_temp=0)):
        with pytest.raises(ValueError):
            make(**bad)


@pytest.mark.parametrize('kind', ['flattened', 'faces_objects'])
def test_yaml_config_with_sampling_topk(tmp_path, kind):
    from tell_amd import config
    path = _write_cfg(tmp_path, kind)
    model, _ = config.from_config(path, overrides='{"model": {"sampling_topk": 20, "sampling_temp": 0.7}}',
                                  resnet=object(), roberta=object())
    assert (model.sampling_topk, model.sampling_temp) == (20, 0.7)
    for over in ('{"model": {"sampling_topk": 0}}', '{"model": {"sampling_topk": 65}}',
                 '{"model": {"sampling_topk": 20, "sampling_temp": 0.0}}', '{"model": {"sampling_temp": -0.5}}'):
        with pytest.raises(ValueError):
            config.from_config(path, overrides=over, resnet=object(), roberta=object())


def test_beam_search_and_sampling_do_not_combine():
    model = _builders()['flattened'](sampling_topk=20, sampling_temp=0.7)
    with pytest.raises(ValueError):
        model._generate(torch.zeros(2, 1, dtype=torch.long), {}, beam_size=4)
    with pytest.raises(ValueError):
        next(model.generate_lanes(iter([]), beam_size=4))
