"""Records what every single generation option and every pair of them does at the front doors - refused (exception class and
message) or accepted (the generator reached and the non-default options that arrived there) - into option_grid.json.  No GPU:
the models are shells without weights, `_forward` is stubbed and the generators are replaced by recorders.

    python tests/golden/make_option_grid.py          # rewrites tests/golden/option_grid.json

tests/test_option_grid_host.py replays the grid and requires equality.  The file was generated on the commit before the
options of a decode call became one DecodePlan; the script holds the adapters of both sides (keywords before, plan fields
after), so the replay runs on either.

`first_of`: where two refusals apply, TransformerGloveModel.generate and generate_lanes used to test them in another order than
CaptionModel.generate; for such a case both messages are stored (the front door's own and CaptionModel.generate's) and the
replay accepts either - the exception class must still match."""
import contextlib
import itertools
import json
import os
import sys
from unittest import mock

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(HERE, 'option_grid.json')
V, B = 600, 2


def _prefix():
    return torch.tensor([[7, 8, 9], [11, 1, 1]], dtype=torch.long)


def _flags(lo, hi):
    t = torch.zeros(V, dtype=torch.bool)
    t[lo:hi] = True
    return t


# name -> (attributes of the model, arguments of the call)
OPTIONS = {
    'sampling_topk': ({'sampling_topk': 5}, {}),
    'sampling_topp': ({'sampling_topp': 0.9}, {}),
    'sampling_minp': ({'sampling_minp': 0.1}, {}),
    'sampling_typical': ({'sampling_typical': 0.9}, {}),
    'beam_len_penalty': ({'beam_len_penalty': 0.8}, {}),
    'no_repeat_ngram_size': ({'no_repeat_ngram_size': 3}, {}),
    'min_len': ({'min_len': 5}, {}),
    'repetition_penalty': ({'repetition_penalty': 1.2}, {}),
    'presence_penalty': ({'presence_penalty': 0.5}, {}),
    'suppress_tokens': ({'suppress_tokens': (5,)}, {}),
    'guidance_scale': ({'guidance_scale': 2.0}, {}),
    'beam_size': ({}, {'beam_size': 4}),
    'n_best': ({}, {'beam_size': 4, 'n_best': 2}),
    'attention': ({}, {'attention': True}),
    'prefix': ({}, {'prefix': _prefix}),
    'n_samples': ({}, {'n_samples': 3}),
    'banned': ({}, {'banned': lambda: _flags(500, 520)}),
    'ground': ({}, {'ground': lambda: _flags(300, 400)}),
    'guidance': ({}, {'guidance': 2.0}),
    'token_stats': ({}, {'token_stats': 4}),
}
CASES = [()] + [(n,) for n in OPTIONS] + list(itertools.combinations(OPTIONS, 2))


class _Softmax:
    vocab_size = V


class _Dyn(torch.nn.Module):
    """A DynamicConv decoder as far as the checks look."""
    adaptive_softmax = _Softmax()

    def project_contexts(self, contexts):
        raise AssertionError('not reached')


class _Lstm(torch.nn.Module):
    adaptive_softmax = _Softmax()


def _shell(cls, decoder, **attrs):
    m = cls.__new__(cls)
    torch.nn.Module.__init__(m)
    m.decoder, m.padding_idx, m.index, m.sampling_topk, m.sampling_temp, m.sampling_topp = decoder, 1, 'roberta', 1, 1.0, None
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _kinds():
    from tell_amd.models.baseline_glove import BaselineGloveModel, TransformerGloveModel
    from tell_amd.models.pointer import TransformerPointerModel
    from tell_amd.models.transformer import CaptionModel
    return {
        'dynconv': lambda: _shell(CaptionModel, _Dyn()),
        'dynconv_reference_flow': lambda: _shell(CaptionModel, _Dyn(), fast_generation=False),
        'lstm_decoder': lambda: _shell(CaptionModel, _Lstm()),
        'transformer_glove': lambda: _shell(TransformerGloveModel, _Dyn()),
        'baseline_glove': lambda: _shell(BaselineGloveModel, _Lstm()),
        'transformer_pointer': lambda: _shell(TransformerPointerModel, _Dyn()),
    }


LANES = ('dynconv', 'lstm_decoder')          # the kinds whose grid also runs through generate_lanes (one batch)


def _plain(x):
    """What JSON holds of an option's value: tuples as lists, a tensor as its shape and dtype."""
    if torch.is_tensor(x):
        return {'shape': list(x.shape), 'dtype': str(x.dtype)}
    if isinstance(x, (tuple, list)):
        return [_plain(y) for y in x]
    return x


_RESULT = (torch.zeros(B, 1), torch.zeros(B, 2, dtype=torch.long), [])


@contextlib.contextmanager
def _recorders(log):
    """The generators behind the front doors replaced by recorders of (name, non-default options), `_forward` and everything
    that touches a device stubbed."""
    from tell_amd import ops, streams
    from tell_amd.models import transformer as T
    from tell_amd.models.baseline_glove import BaselineGloveModel, TransformerGloveModel
    from tell_amd.models.pointer import PointerModelBase
    C = T.CaptionModel
    planned = hasattr(sys.modules.get('tell_amd.models.gen_options'), 'DecodePlan')

    def reached(name, **opts):
        off = dict(beam_size=1, n_best=1, attention=False, prefix=None, samples=None, vmask=None, guide=None, stats=0)
        log.append((name, {k: _plain(v) for k, v in opts.items() if not (v is off[k] or (off[k] is not None and v == off[k]))}))

    if planned:
        def greedy(self, caption_ids, contexts, gen_len=100, eos=2, check_every=8, lane=0, seed=None, plan=None):
            reached('greedy', **({} if plan is None else plan._asdict()))
            return _RESULT
            yield

        def beam(self, caption_ids, contexts, gen_len=100, eos=2, check_every=8, lane=0, seed=None, plan=None):
            reached('beam', **({} if plan is None else plan._asdict()))
            return _RESULT
            yield
    else:
        def greedy(self, caption_ids, contexts, gen_len=100, eos=2, check_every=8, lane=0, seed=None, attention=False,
                   prefix=None, n=1, rank=('score', 0.0), vmask=None, guide=None, stats=0):
            reached('greedy', attention=attention, prefix=prefix, samples=(n,) + tuple(rank) if n > 1 else None, vmask=vmask,
                    guide=guide, stats=stats)
            return _RESULT
            yield

        def beam(self, caption_ids, contexts, beam_size, gen_len=100, eos=2, check_every=8, lane=0, n_best=1, prefix=None,
                 vmask=None, guide=None):
            reached('beam', beam_size=beam_size, n_best=n_best, prefix=prefix, vmask=vmask, guide=guide)
            return _RESULT
            yield

    def reference(self, caption_ids, contexts, attn_idx=None, gen_len=100, eos=2):
        reached('reference')
        return _RESULT

    def lstm(self, caption_ids, contexts, gen_len=100, eos=2):
        reached('lstm')
        return _RESULT[:2]

    def pointer(name):
        def run(self, caption_ids, contexts, enc, context, *a, **kw):
            reached(name)
            return _RESULT[1], _RESULT[0], torch.zeros(B, 2, dtype=torch.bool), torch.zeros(B, 1)
        return run

    def pointer_steps(self, caption_ids, contexts, enc, context, gen_len=100, eos=2, check_every=8, n=1, rank=('score', 0.0)):
        reached('pointer_steps', samples=(n,) + tuple(rank) if n > 1 else None)
        raise _Done
        yield

    ids = torch.zeros(B, 4, dtype=torch.long)

    class Stream:
        def wait_event(self, ev):
            pass

    class Event:
        def record(self, stream=None):
            pass
    null = lambda *a, **k: contextlib.nullcontext()       # noqa: E731
    with contextlib.ExitStack() as es:
        for owner, name, new in (
                (C, '_greedy_steps', greedy), (C, '_beam_steps', beam), (C, '_generate_reference_flow', reference),
                (C, '_forward', lambda self, *a, **k: (ids, None, {})),
                (C, '_forward_loss', lambda self, *a, **k: ({}, ids, {})),
                (BaselineGloveModel, '_generate', lstm),
                (BaselineGloveModel, '_forward', lambda self, *a, **k: (ids, None, {})),
                (BaselineGloveModel, '_vectors', staticmethod(lambda *a, **k: None)),
                (TransformerGloveModel, '_glove_forward', lambda self, *a, **k: (ids, None, {})),
                (TransformerGloveModel, '_vectors', staticmethod(lambda *a, **k: None)),
                (PointerModelBase, '_require_masks', lambda self, *a, **k: None),
                (PointerModelBase, 'encode', lambda self, *a, **k: None),
                (PointerModelBase, 'detokenize', lambda self, x: ''),
                (PointerModelBase, '_generate_pointer', pointer('pointer')),
                (PointerModelBase, '_generate_pointer_cached', pointer('pointer_cached')),
                (PointerModelBase, '_pointer_steps', pointer_steps),
                (streams, 'get', lambda *a, **k: Stream()), (torch.cuda, 'current_stream', lambda *a, **k: Stream()),
                (torch.cuda, 'Event', Event), (torch.cuda, 'stream', null), (ops.hip, 'bound_stream', null)):
            es.enter_context(mock.patch.object(owner, name, new))
        yield


class _Done(Exception):
    """Ends a recorded generator whose result nothing behind it could use."""


def _batch():
    return {'context': {'roberta': torch.full((B, 7), 9, dtype=torch.long)}, 'image': None,
            'caption': {'roberta': torch.full((B, 5), 9, dtype=torch.long)}}


def run_case(make, kind, case, door):
    """One case at one front door ('generate' / 'lanes') -> {'error', 'message'} or {'reached', 'options'}."""
    attrs, kw = {}, {}
    for name in case:
        a, k = OPTIONS[name]
        attrs.update(a)
        kw.update({n: (v() if callable(v) else v) for n, v in k.items()})
    log = []
    try:
        with _recorders(log):
            m = make()
            for k, v in attrs.items():
                setattr(m, k, v)
            b = _batch()
            if door == 'lanes':
                if 'prefix' in kw:
                    b['prefix'] = kw.pop('prefix')
                list(m.generate_lanes([b], **kw))
            elif kind in ('transformer_glove', 'baseline_glove'):
                m.generate(b['image'], b['caption'], **kw)
            else:
                m.generate(b['context'], b['image'], b['caption'], **kw)
    except _Done:
        pass
    except Exception as e:                                    # noqa: BLE001 - the refusal is what is recorded
        return {'error': type(e).__name__, 'message': str(e)}
    assert len(log) == 1, (kind, case, door, log)
    return {'reached': log[0][0], 'options': log[0][1]}


def record():
    """-> {kind or kind + '/lanes': {'a+b': result}} over CASES."""
    out = {}
    for kind, make in _kinds().items():
        for door in ('generate',) + (('lanes',) if kind in LANES else ()):
            out[kind if door == 'generate' else kind + '/lanes'] = {
                '+'.join(case): run_case(make, kind, case, door) for case in CASES}
    return out


def mark_first_of(grid):
    """Where a front door with an order of its own (TransformerGloveModel.generate, generate_lanes) and CaptionModel.generate
    both refuse a case with the same exception class and different messages, the case gets first_of = both messages (the class
    name in CaptionModel.generate's replaced by the front door's own).  -> (first_of cases, refused pairs) over those doors."""
    marked = refused = 0
    for key, norm, old, new in (('transformer_glove', 'dynconv', 'CaptionModel', 'TransformerGloveModel'),
                                ('dynconv/lanes', 'dynconv', '', ''), ('lstm_decoder/lanes', 'lstm_decoder', '', '')):
        for case, got in grid[key].items():
            want = grid[norm][case]
            if 'error' not in got:
                continue
            refused += case.count('+') == 1
            if want.get('error') == got['error']:
                other = want['message'].replace(old, new) if old else want['message']
                if other != got['message']:
                    got['first_of'] = [got['message'], other]
                    marked += 1
    return marked, refused


def dump(grid, path=PATH):
    """The grid in the file's compact form: every distinct result once ('results', one per line), and for every front door
    the index of each case's result, in the order of CASES."""
    results = sorted({json.dumps(r, sort_keys=True) for v in grid.values() for r in v.values()})
    at = {r: i for i, r in enumerate(results)}
    rows = ['"%s": %s' % (k, json.dumps([at[json.dumps(v['+'.join(c)], sort_keys=True)] for c in CASES]))
            for k, v in sorted(grid.items())]
    with open(path, 'w') as f:
        f.write('{"cases": %s,\n"results": [\n%s\n],\n"grid": {\n%s\n}}\n'
                % (json.dumps(['+'.join(c) for c in CASES]), ',\n'.join(results), ',\n'.join(rows)))


def load(path=PATH):
    """-> {front door: {'a+b': result}} of the file `dump` wrote."""
    d = json.load(open(path))
    return {k: {c: d['results'][i] for c, i in zip(d['cases'], idx)} for k, idx in d['grid'].items()}


def main():
    grid = record()
    marked, refused = mark_first_of(grid)
    dump(grid)
    total = sum(len(v) for v in grid.values())
    print('%d cases, %d refused; first_of: %d cases (of %d refused pairs at the doors with an order of their own); %d bytes'
          % (total, sum('error' in r for v in grid.values() for r in v.values()), marked, refused, os.path.getsize(PATH)))


if __name__ == '__main__':
    main()
