"""CPU checks of the copy models' cached generation: the ABI of csrc/copy_decode.hip, the
`cached_generation` key and the options that stay refused, the defaults, the static-row definition of the copy decision and
the conditions on the inputs of every case tests/test_gpu_copy_decode.py runs."""
import os

import numpy as np
import pytest
import torch

import copy_decode_cases as cdc
import copy_ref as ref
import tell_amd  # noqa: F401
from tell_amd.models.transformer import Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('tell_entity_attn_step', 'tell_copy_decide')


def _tiny(kind='pointer', **kw):
    from tell_amd.build import build_model
    torch.manual_seed(0)
    return build_model(kind, object(), object(), n_bert_layers=3, vocab_size=600, dim=1024, heads=16, ffn=64,
                       kernels=(3,), cutoff=(100, 300), **kw)


# ---------------------------------------------------------------- ABI
def test_symbols_are_declared_and_exported():
    from tell_amd import hip
    protos = hip.parse_header()
    for name in SYMBOLS:
        assert name in protos, name
        names = protos[name][2]
        assert names[-1] == 'stream' and 'step' in names and 'step_dev' in names and 'dtype' in names
    if not os.path.exists(hip.LIB_PATH):
        pytest.fail('%s is not built' % hip.LIB_PATH)
    lib = hip.lib()                                    # (resolves every declared symbol; a missing one raises)
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes == protos[name][1]
    assert 'copy_decode' in open(os.path.join(ROOT, 'transform-and-tell_amd', 'csrc', 'build.sh')).read()


# ---------------------------------------------------------------- the key
@pytest.mark.parametrize('name', ['transformer_pointer', 'transformer_pointer_2'])
def test_key_is_accepted_by_both_registered_names_and_defaults_to_false(name):
    import inspect
    cls = Model.by_name(name)
    assert inspect.signature(cls.__init__).parameters['cached_generation'].default is False
    assert inspect.signature(cls.generate).parameters['cached'].default is None


def test_key_through_build_model_and_yaml(tmp_path):
    from tell_amd import config
    assert _tiny().cached_generation is False
    assert _tiny(cached_generation=True).cached_generation is True
    assert _tiny('pointer_2', cached_generation=True).cached_generation is True
    with pytest.raises(ValueError, match='cached_generation'):
        _tiny('faces_parallel', cached_generation=True)
    text = """
model:
  type: %s
  cached_generation: %s
  vocab_size: 600
  decoder:
    type: dynamic_conv_decoder_faces_parallel
"""
    for name in ('transformer_pointer', 'transformer_pointer_2'):
        for value in (True, False):
            p = tmp_path / ('%s_%s.yaml' % (name, value))
            p.write_text(text % (name, 'true' if value else 'false'))
            got = config.yaml_to_params(str(p), '')['model']
            assert got['type'] == name and got['cached_generation'] is value
            # what model_from_params does with the parsed keys: they go to the registered class's constructor as they are
            kw = {k: v for k, v in got.items() if k not in ('type', 'decoder')}
            m = _construct(Model.by_name(name), **kw)
            assert m.cached_generation is value


def _construct(cls, **kw):
    from tell_amd.build import build_decoder
    from tell_amd.modules import AdaptiveLoss
    torch.manual_seed(0)
    dec = build_decoder('faces_parallel', vocab_size=600, dim=1024, heads=16, ffn=64, kernels=(3,), cutoff=(100, 300))
    return cls(None, dec, AdaptiveLoss(padding_idx=1), n_bert_layers=3, resnet=object(), roberta=object(), **kw)


def test_defaults_report_no_lanes_and_no_step_graph():
    for m in (_tiny(), _tiny(cached_generation=True)):
        assert m.lanes_usable() is False and m.STEP_GRAPH is False and m.SEARCH_OPTIONS is False


def test_cached_generation_refuses_what_the_eager_path_refuses():
    ids = torch.full((1, 5), 4)
    ctx = {'roberta': ids, 'roberta_proper_masks': torch.ones_like(ids)}
    img = torch.zeros(1, 3, 8, 8)
    refused = [dict(beam_size=2), dict(prefix=torch.full((1, 2), 5)), dict(guidance=2.0), dict(attention=True),
               dict(n_samples=2), dict(banned=[5]), dict(ground=True), dict(n_best=2)]
    for kw in refused:
        msgs = []
        for cached in (False, True):
            m = _tiny()
            with pytest.raises(ValueError) as err:
                m.generate(context=dict(ctx), image=img, caption={'roberta': ids}, cached=cached, **kw)
            msgs.append(str(err.value))
        assert msgs[0] == msgs[1], kw
    for opt in (dict(beam_len_penalty=0.5), dict(no_repeat_ngram_size=2), dict(repetition_penalty=1.2)):
        with pytest.raises(ValueError):                      # (at construction or at the call, as without the key)
            m = _tiny(cached_generation=True, **opt)
            m.generate(context=dict(ctx), image=img, caption={'roberta': ids})
    with pytest.raises(ValueError, match='roberta_proper_masks'):
        _tiny().generate(context={'roberta': ids}, image=img, caption={'roberta': ids}, cached=True)


def test_stepper_signature_gains_hidden_only_when_set():
    import inspect
    from tell_amd.models.stepper import DecodeStepper
    assert inspect.signature(DecodeStepper.__init__).parameters['hidden'].default is False
    src = inspect.getsource(DecodeStepper._entry)
    assert "if self.hidden:" in src and "('hidden',)" in src


# ---------------------------------------------------------------- the static-row definition
def test_static_rows_are_copy_step_over_the_unfinished_rows():
    case = next(c for c in ref.STEP if c['id'] == 'S20')
    x = cdc.from_step(case, 'float32')
    assert x['fin'].tolist() == [0, 1, 0, 0] and x['p'] == 0 and x['L'] == ref.HIST_LEN - 1
    e = cdc.expected(x)
    assert e['rows'].tolist() == sorted(ref.STEP_ROWS)
    base = ref.copy_step(**ref.step_inputs(case, 'float32'))                 # rows in copy_ref's own order (2, 0, 3)
    for i, b in enumerate(ref.STEP_ROWS):
        j = e['rows'].tolist().index(b)
        assert e['tok'][b] == base['tok'][i] and e['copied'][b] == bool(base['copied'][i])
        assert e['r']['prob'][j] == base['prob'][i]
    assert e['tok'][cdc.FINISHED_ROW] is None and e['copied'][cdc.FINISHED_ROW] is None
    # the finished row keeps its column of the history although its entity logits and its keys would copy
    assert e['hist'][cdc.FINISHED_ROW].tolist() == x['hist'][cdc.FINISHED_ROW].tolist()
    assert (e['hist'][:, :x['p'] + 1] == x['hist'][:, :x['p'] + 1]).all()


# ---------------------------------------------------------------- conditions on the inputs of the GPU cases
def _walk(dtype):
    for cid, make in cdc.cases():
        x = make(dtype)
        yield cid, x, cdc.expected(x)


@pytest.mark.parametrize('dtype', ref.DTYPES)
def test_every_non_tie_row_is_decided_beyond_the_bound(dtype):
    for cid, x, e in _walk(dtype):
        r = e['r']
        if x['tie']:
            assert (r['gap'] == 0).all(), cid                              # two byte-identical keys: the tie is exact
            continue
        b = ref.step_bound(r, c=max(ref.C.get('prob', 1.0), 1.0))
        assert (r['gap'] > 2 * b).all(), (cid, dtype, r['gap'], b)


@pytest.mark.parametrize('dtype', ref.DTYPES)
def test_each_table_holds_every_kind_of_row(dtype):
    tables = {'step': [], 'extra': []}
    for cid, x, e in _walk(dtype):
        tables['step' if cid.startswith('step_') else 'extra'].append((cid, x, e))
    for name, rows in tables.items():
        kinds = set()
        for cid, x, e in rows:
            r = e['r']
            for i, b in enumerate(e['rows']):
                wants = bool(x['ent'][b][1] > x['ent'][b][0])
                empty = float(r['prob'][i]) == float(np.float32(1e-6)) and not r['copied'][i]
                seen = int(r['best_id'][i]) in x['hist'][b, :x['p'] + 1].tolist()
                if r['copied'][i]:
                    kinds.add('copies')
                elif empty and wants:
                    kinds.add('below 1e-6')
                elif seen and wants and not empty:
                    kinds.add('refused by hist')
                elif not wants and not empty and not seen:
                    kinds.add('refused by the entity logits')
        assert kinds == {'copies', 'below 1e-6', 'refused by hist', 'refused by the entity logits'}, (name, kinds)


def test_entity_attention_reference_covers_the_empty_history():
    """copy_ref.causal at pos0 = S = 0 (step 0 of the static history): the zero slot alone, out = 0"""
    B, H = 2, 2
    z = np.zeros((0, B, H * 64))
    f = ref.causal(np.ones((1, B, H * 64)), z, z, ref.C_SCALE, 0, 0, H)
    assert f['out'].shape == (1, B, H * 64) and not f['out'].any() and f['n'] == 0
