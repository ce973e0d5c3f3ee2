"""GPU: which decode-step signatures every generation mode keys in `_decode_graphs` - the default call and every accepted
option, against tests/golden/decode_signatures.json (recorded once, before the options of a decode call became one
DecodePlan): no mode captures a different or an additional graph, and a second call of the same batch adds no key."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'decode_signatures.json')
V, IMAGES, GEN_LEN = 600, 2, 6

# name -> (the model's keys, generate's arguments); 'prefix' / 'banned' / 'ground' are replaced by tensors (_arguments)
CASES = {
    'default': ({}, {}),
    'sampling_topk': ({'sampling_topk': 5}, {}),
    'sampling_topp': ({'sampling_topk': 0, 'sampling_topp': 0.9}, {}),
    'sampling_minp': ({'sampling_topk': 0, 'sampling_minp': 0.1}, {}),
    'sampling_typical': ({'sampling_topk': 0, 'sampling_typical': 0.9}, {}),
    'beam_len_penalty': ({'beam_len_penalty': 0.8}, {}),
    'no_repeat_ngram_size': ({'no_repeat_ngram_size': 3}, {}),
    'min_len': ({'min_len': 5}, {}),
    'repetition_penalty': ({'repetition_penalty': 1.2}, {}),
    'presence_penalty': ({'presence_penalty': 0.5}, {}),
    'suppress_tokens': ({'suppress_tokens': (5,)}, {}),
    'guidance_scale': ({'guidance_scale': 2.0}, {}),
    'beam_size': ({}, {'beam_size': 4}),
    'attention': ({}, {'attention': True}),
    'prefix': ({}, {'prefix': 3}),
    'banned': ({}, {'banned': True}),
    'ground': ({}, {'ground': True}),
    'guidance': ({}, {'guidance': 2.0}),
    'token_stats': ({}, {'token_stats': 4}),
    'beam_n_best': ({}, {'beam_size': 4, 'n_best': 2}),
    'topk_n_samples': ({'sampling_topk': 5}, {'n_samples': 3}),
    'prefix_banned': ({}, {'prefix': 3, 'banned': True}),
}


def _arguments(kw):
    kw = dict(kw)
    if 'prefix' in kw:
        kw['prefix'] = torch.tensor([[7, 8, 9], [11, 1, 1]][:IMAGES], dtype=torch.long)[:, :kw['prefix']]
    if 'banned' in kw:
        kw['banned'] = torch.zeros(V, dtype=torch.bool, device=DEV)
        kw['banned'][500:520] = True
    if 'ground' in kw:
        kw['ground'] = torch.zeros(V, dtype=torch.bool, device=DEV)
        kw['ground'][300:400] = True
    return kw


def _plain(x):
    """A signature as JSON holds it: tuples as lists, the dtype by name."""
    if isinstance(x, (tuple, list)):
        return [_plain(y) for y in x]
    return str(x) if isinstance(x, torch.dtype) else x


def _keys(model):
    """The cache keys of the model, the address of the position table (element 5) replaced by 0; sorted."""
    return sorted(json.dumps(_plain(sig[:5] + (0,) + sig[6:])) for sig in model.__dict__.get('_decode_graphs', {}))


def signatures(name):
    """-> (keys after one generate, keys after a second generate of the same batch) of the case's model."""
    import tell_amd
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    from tell_amd.models.transformer import CaptionModel
    from test_gpu_train import KW, _Res, _Rob
    tell_amd.hip.require_gpu()
    tell_amd.set_compute_dtype(torch.float32)
    torch.manual_seed(0)
    keys, kw = CASES[name]
    model = build_model('faces_objects', _Res(True), _Rob(1024), n_bert_layers=3, **KW, **keys).to(DEV).eval()
    # (generate has no gen_len of its own: the decode behind it runs GEN_LEN steps instead of 100)
    model._generate = lambda *a, **k: CaptionModel._generate(model, *a, gen_len=GEN_LEN, **k)
    batch = synthetic_batch(B=IMAGES, article_len=24, caption_len=9, faces_objects=True, vocab=V, cutoffs=(100, 300), seed=5,
                            device=DEV)
    out = []
    with torch.no_grad():
        for _ in range(2):
            model.generate(**{k: (dict(v) if isinstance(v, dict) else v.clone()) for k, v in batch.items()}, **_arguments(kw))
            torch.cuda.synchronize()
            out.append(_keys(model))
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_signatures_of_a_mode_are_the_recorded_ones(name):
    want = json.load(open(GOLDEN))[name]
    first, second = signatures(name)
    assert len(first) == len(want), (first, want)
    assert first == want
    assert second == first                                    # the same batch again: no new key
