"""CPU checks of transformer_pointer / transformer_pointer_2: registration, the a1-a3 configs, the parameter layout of
the reference (unused parameters included), the generation options they refuse and checkpoint loading."""
import glob
import logging
import os

import pytest
import torch

import tell_amd  # noqa: F401
from tell_amd.models.transformer import Model

REF_EXPT = '/root/reference/expt'


def _tiny(kind='pointer', **kw):
    from tell_amd.build import build_model
    torch.manual_seed(0)
    return build_model(kind, object(), object(), n_bert_layers=3, vocab_size=600, dim=1024, heads=16, ffn=64,
                       kernels=(3,), cutoff=(100, 300), **kw)


def test_registry_names():
    assert Model.by_name('transformer_pointer').__name__ == 'TransformerPointerModel'
    assert Model.by_name('transformer_pointer_2').__name__ == 'TransformerPointer2Model'
    assert Model.by_name('transformer_pointer').COPY_VARIANT == 1
    assert Model.by_name('transformer_pointer_2').COPY_VARIANT == 2


@pytest.mark.skipif(not os.path.isdir(REF_EXPT), reason='reference tree only exists in the authoring container')
def test_a1_a3_configs_instantiate():
    from tell_amd import config
    paths = sorted(glob.glob(os.path.join(REF_EXPT, '*', 'a[123]_*', 'config.yaml')))
    assert len(paths) == 6
    for p in paths:
        m, params = config.from_config(p, '{"model": {"model_path": null}}', resnet=object(), roberta=object())
        want = 'TransformerPointer2Model' if 'a3_' in p else 'TransformerPointerModel'
        assert type(m).__name__ == want, p
        assert m.decoder.layers[0].context_names == ['image', 'article', 'faces']
        assert m.bert_weight_2.shape == (25,)
        assert '^bert_weight$' in params['trainer']['no_grad']


def test_parameter_layout_of_the_reference():
    m = _tiny()
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes['in_proj_weight'] == (2048, 1024) and shapes['in_proj_bias'] == (2048,)
    assert shapes['bias_k'] == (1, 1, 1024)
    assert shapes['bert_weight_2'] == (3,) and shapes['bert_weight'] == (3,)
    for n in ('entity_fc', 'out_proj', 'entity_attn.in_proj_q', 'entity_attn.in_proj_k', 'entity_attn.in_proj_v',
              'entity_attn.attention.attention_module.out_proj'):
        assert shapes[n + '.weight_g'][1] == 1 and n + '.bias' in shapes and n + '.weight_v' in shapes
    assert shapes['entity_fc.weight_v'] == (2, 1024)
    am = 'entity_attn.attention.attention_module.'
    for proj in ('in_proj_q.', 'in_proj_k.0.', 'in_proj_v.0.'):      # GatedLinear stacks, never applied
        assert shapes[am + proj + '0.weight_v'] == (4096, 1024)
        assert shapes[am + proj + '2.weight_v'] == (2048, 2048)
        assert shapes[am + proj + '4.weight_v'] == (1024, 1024)
    assert shapes['entity_attn.ln.weight'] == (1024,)
    frozen = {n for n, p in m.named_parameters() if not p.requires_grad}
    assert 'out_proj.weight_v' in frozen and am + 'in_proj_q.0.weight_v' in frozen
    assert not any(n.startswith(('entity_fc', 'in_proj', 'bias_k', 'bert_weight_2', 'entity_attn.in_proj',
                                 am + 'out_proj')) for n in frozen)


def test_sampling_and_beam_are_refused():
    with pytest.raises(ValueError):
        _tiny(sampling_topk=4)
    m = _tiny()
    with pytest.raises(ValueError):
        m._check_beam(3)
    m._check_beam(1)
    assert m.STEP_GRAPH is False and m.lanes_usable() is False


def test_faces_checkpoint_loads_with_a_warning(tmp_path, caplog):
    from tell_amd.build import build_model
    from tell_amd.models.pointer import load_state_dict_with_prefix
    torch.manual_seed(1)
    faces = build_model('faces_parallel', object(), object(), n_bert_layers=3, vocab_size=600, dim=1024, heads=16,
                        ffn=64, kernels=(3,), cutoff=(100, 300))
    path = str(tmp_path / 'best.th')
    torch.save(faces.state_dict(), path)
    m = _tiny()
    init = {k: v.clone() for k, v in m.state_dict().items()}
    with caplog.at_level(logging.WARNING):
        load_state_dict_with_prefix(m, torch.load(path))
    assert any('missing keys' in r.getMessage() for r in caplog.records)
    sd = m.state_dict()
    for k, v in faces.state_dict().items():
        assert torch.equal(sd[k], v), k
    for k in ('in_proj_weight', 'bias_k', 'bert_weight_2', 'entity_fc.weight_v'):
        assert torch.equal(sd[k], init[k]), k


def test_batches_without_the_names_matched_masks_are_refused():
    m = _tiny()
    ids = torch.full((1, 5), 4)
    with pytest.raises(ValueError, match='roberta_proper_masks'):
        m(context={'roberta': ids}, image=torch.zeros(1, 3, 8, 8),
          caption={'roberta': ids, 'roberta_copy_masks': torch.zeros_like(ids)})
    with pytest.raises(ValueError, match='roberta_copy_masks'):
        m(context={'roberta': ids, 'roberta_proper_masks': torch.ones_like(ids)}, image=torch.zeros(1, 3, 8, 8),
          caption={'roberta': ids})
    with pytest.raises(ValueError, match='roberta_proper_masks'):
        m.generate(context={'roberta': ids}, image=torch.zeros(1, 3, 8, 8), caption={'roberta': ids})
