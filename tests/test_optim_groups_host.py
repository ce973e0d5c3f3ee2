"""CPU half of BertAdam's parameter groups: the group resolution of training/optimizers.py against
its restatement in tests/optim_groups_ref.py, every refusal, the declared ABI of tell_bertadam_step_groups, the host wrapper
with hip.call recorded instead of run, and tests/optim_groups_ref.py itself - its exact lane against the closed form and its
MUTANTS against the case table."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest
import torch

import optim_groups_ref as grp
import optim_ref as ref
from test_optim_ema_host import CFG, STEP2_ARGS, bits, calls  # noqa: F401 - (calls is a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ['decoder.embedder.weight', 'decoder.layers.0.conv.weight', 'decoder.layers.0.conv.bias',
         'decoder.layers.0.norm.weight', 'decoder.layers.1.fc.weight', 'decoder.layers.1.fc.bias',
         'decoder.adaptive_softmax.head.weight']
SHAPES = [(30, 70), (40, 30), (5,), (1025,), (33, 3), (3,), (2049,)]


def _flat(names=NAMES, shapes=SHAPES):
    from tell_amd.training.optimizers import FlatParams
    torch.manual_seed(0)
    return FlatParams([(n, torch.nn.Parameter(torch.randn(*s))) for n, s in zip(names, shapes)], 'cpu')


def _opt(groups, names=NAMES, shapes=SHAPES, **kw):
    from tell_amd.training.optimizers import BertAdam
    return BertAdam(_flat(names, shapes), parameter_groups=groups, **dict(CFG, **kw))


def _values(g):
    return {k: g[k] for k in grp.HOST_KEYS}


# ---------------------------------------------------------------- group resolution
def test_first_match_wins_rest_goes_to_the_default_group():
    groups = [[['bias', r'norm\.weight$'], {'weight_decay': 0.0}],
              [['^decoder.embedder', '^decoder.adaptive_softmax', 'conv.bias'], {'lr': 1e-3, 'warmup': 0.4}]]
    opt = _opt(groups)
    assert len(opt.groups) == 3
    assert opt.groups[0]['names'] == [NAMES[2], NAMES[3], NAMES[5]]                  # conv.bias: the FIRST group that matches
    assert opt.groups[1]['names'] == [NAMES[0], NAMES[6]]
    assert opt.groups[2]['names'] == [NAMES[1], NAMES[4]]                            # no regex matches: the default group
    assert _values(opt.groups[0]) == dict(CFG, weight_decay=0.0)                     # a group inherits what it does not override
    assert _values(opt.groups[1]) == dict(CFG, lr=1e-3, warmup=0.4)
    assert _values(opt.groups[2]) == CFG
    assert [opt.group_of(n) for n in NAMES] == [1, 2, 0, 0, 2, 0, 1]
    with pytest.raises(KeyError):
        opt.group_of('nobody')
    want, tg = grp.resolve(NAMES, CFG, groups)
    assert opt.groups == want and opt.flat.tensor_group.tolist() == tg == [1, 2, 0, 0, 2, 0, 1]
    assert opt.flat.tensor_group.dtype == torch.int32 and opt.lr_dev.shape == (3,)
    # re.search, not re.match: an unanchored pattern matches inside the name
    assert _opt([[['layers'], {'b1': 0.5}]]).groups[0]['names'] == NAMES[1:6]


def test_empty_groups_are_dropped_and_equal_groups_merged():
    with pytest.warns(UserWarning, match='zzz'):
        opt = _opt([[['zzz'], {'lr': 1.0}], [['bias'], {'weight_decay': 0.0}]])
    assert len(opt.groups) == 2 and opt.groups[0]['weight_decay'] == 0.0 and opt.flat.tensor_group.tolist() == [1, 1, 0, 1, 1, 0, 1]
    # a listed group that holds every tensor: the default group is empty and dropped - ONE group, with the override
    one = _opt([[['^decoder'], {'lr': 0.5}]])
    assert len(one.groups) == 1 and one.groups[0]['lr'] == 0.5 and one.flat.tensor_group is None and one.group_hp is None
    # equal values: merged, whichever way they are spelled (an override equal to the global; int against float)
    merged = _opt([[['embedder'], {'weight_decay': 0.0}], [['conv'], {'lr': CFG['lr']}], [['norm'], {'weight_decay': 0}],
                   [['fc'], {'t_total': 10.0, 'b1': 0.9}]])
    assert len(merged.groups) == 2
    assert merged.groups[0]['names'] == [NAMES[0], NAMES[3]] and merged.flat.tensor_group.tolist() == [0, 1, 1, 0, 1, 1, 1]
    assert grp.resolve(NAMES, CFG, [[['embedder'], {'weight_decay': 0.0}], [['norm'], {'weight_decay': 0}]])[1] == \
        [0, 1, 1, 0, 1, 1, 1]


@pytest.mark.parametrize('groups', [None, [], [[['^decoder.layers.0'], {}], [['bias'], {}]],
                                    [[['embedder'], {'lr': CFG['lr'], 'e': CFG['e'], 'schedule': 'warmup_linear'}]]])
def test_one_group_allocates_nothing_and_launches_what_it_launched(groups, calls):   # noqa: F811
    opt = _opt(groups)
    flat = opt.flat
    assert len(opt.groups) == 1 and _values(opt.groups[0]) == CFG and opt.groups[0]['names'] == NAMES
    assert flat.tensor_group is None and opt.group_hp is None and opt.lr_dev.shape == (1,)
    # (optim_ref.schedule rounds its three arguments to fp32 first, as the kernel's are: 3 x 2^-24 apart at the most)
    assert opt.current_lr(3) == opt.current_lr(3, group=0) == pytest.approx(ref.schedule(3, 1e-2, 0.2, 10), rel=1e-6, abs=0.0)
    skip = torch.zeros(2, dtype=torch.int32)
    opt.launch(grad_scale=0.5, zero_grad=True, skip=skip)
    assert len(calls) == 1
    name, args = calls[0]
    f = flat
    want = (f.flat, f.grad, f.m, f.v, f.chunk_tensor, f.chunk_begin, f.n_chunks, 7, f.partial, f.norms, opt.lr_dev, 0.9,
            0.98, 1e-6, 1e-2, 0.5, 0.5, None, 1, skip, None, opt.step_dev, 1e-2, 0.2, 10.0, None)
    assert name == 'tell_bertadam_step2' and len(args) == len(want) == len(STEP2_ARGS)
    assert all((a is b) if (torch.is_tensor(a) or torch.is_tensor(b)) else (a == b and type(a) is type(b))
               for a, b in zip(args, want)), args


def test_unused_regex_warns_once_and_names_it():
    with pytest.warns(UserWarning) as rec:
        _opt([[['^encoder', 'bias'], {'lr': 1.0}], [['^resnet'], {}]])
    texts = [str(w.message) for w in rec]
    assert len(texts) == 2 and sum("'^encoder'" in t for t in texts) == 1 and sum("'^resnet'" in t for t in texts) == 1
    with warnings.catch_warnings():
        warnings.simplefilter('error')                      # a regex whose tensors an earlier group took IS used
        opt = _opt([[['bias'], {'lr': 1.0}], [['conv.bias'], {'lr': 2.0}]])
    assert len(opt.groups) == 2


BAD = [({'requires_grad': False}, 'requires_grad'), ({'momentum': 0.9}, 'momentum'), ({'lr': '1e-3'}, 'lr'),
       ({'lr': None}, 'lr'), ({'lr': True}, 'lr'), ({'warmup': float('nan')}, 'warmup'), ({'t_total': float('inf')}, 't_total'),
       ({'weight_decay': float('-inf')}, 'weight_decay'), ({'max_grad_norm': [1.0]}, 'max_grad_norm'), ({'e': 0.0}, 'e'),
       ({'e': -1e-6}, 'e'), ({'e': 1e-50}, 'e'), ({'b1': 1.5}, 'b1'), ({'b1': -0.1}, 'b1'), ({'b2': 1.0001}, 'b2'), ({'b2': -1}, 'b2'),
       ({'schedule': 'warmup_cosine'}, 'schedule'), ({'schedule': None}, 'schedule')]


@pytest.mark.parametrize('over,key', BAD)
def test_refusals_name_the_group_index_and_the_key(over, key):
    flat = _flat()
    from tell_amd.training.optimizers import BertAdam
    with pytest.raises(ValueError) as err:
        BertAdam(flat, parameter_groups=[[['embedder'], {}], [['bias'], {'lr': 1e-3}], [['conv'], over]], **CFG)
    assert 'parameter_groups[2]' in str(err.value) and repr(key) in str(err.value), str(err.value)
    assert flat.tensor_group is None
    # the ends of the ranges are inside
    opt = _opt([[['bias'], {'b1': 0.0, 'b2': 1.0, 'e': 1e-30, 'max_grad_norm': 0, 'weight_decay': -0.5, 'lr': 0}]])
    assert len(opt.groups) == 2


def test_a_malformed_entry_names_its_index():
    with pytest.raises(ValueError, match=r'parameter_groups\[1\]'):
        _opt([[['bias'], {}], ['conv']])


def test_sixteen_groups_fit_and_seventeen_do_not():
    names = ['t%02d.weight' % i for i in range(17)]
    shapes = [(3,)] * 17
    groups = [[['^t%02d' % i], {'lr': 0.5 + i}] for i in range(17)]
    opt = _opt(groups[:15], names, shapes)                  # 15 listed + the default group
    assert len(opt.groups) == 16 and opt.lr_dev.shape == (16,) and len(opt.group_hp) == 128
    assert opt.flat.tensor_group.tolist() == list(range(15)) + [15, 15]
    opt = _opt(groups[:16] + [[['^t16'], {'lr': 0.5}]], names, shapes)              # 17 listed, 16 distinct after the merge
    assert len(opt.groups) == 16 and opt.flat.tensor_group.tolist() == list(range(16)) + [0]
    flat = _flat(names, shapes)
    from tell_amd.training.optimizers import BertAdam
    with pytest.raises(ValueError, match='17 distinct groups'):
        BertAdam(flat, parameter_groups=groups[:16], **CFG)                            # 16 listed + the default group
    with pytest.raises(ValueError, match='17 distinct groups'):
        BertAdam(flat, parameter_groups=groups, **CFG)
    assert flat.tensor_group is None


def test_the_shipped_configs_resolve_to_one_group(calls):   # noqa: F811
    """tests/golden/optimizer_parameter_groups.json: the optimizer's parameter_groups of every expt/*/config.yaml of the
    reference (settings only).  All carry `{}` overrides: one group, and the launch the parent commit issued."""
    cfgs = json.load(open(os.path.join(HERE, 'golden', 'optimizer_parameter_groups.json')))
    assert len(cfgs) == 23 and all(c['type'] == 'bert_adam' for c in cfgs.values())
    for path, c in cfgs.items():
        assert len(c['parameter_groups']) == 6
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                 # (NAMES has no layers 2 and 3)
            opt = _opt(c['parameter_groups'])
        assert len(opt.groups) == 1 and opt.flat.tensor_group is None and _values(opt.groups[0]) == CFG, path
        del calls[:]
        opt.launch(zero_grad=True)
        assert [n for n, _ in calls] == ['tell_bertadam_step2'], path
        assert calls[0][1][11:16] == (0.9, 0.98, 1e-6, 1e-2, 0.5) and calls[0][1][22:25] == (1e-2, 0.2, 10.0)


# ---------------------------------------------------------------- the grouped launch
OVERRIDE = [[['bias', 'norm'], {'weight_decay': 0.0}], [['^decoder.embedder'], {'lr': 1e-3, 'max_grad_norm': 0}]]


@pytest.mark.parametrize('ema', [False, True])
def test_an_override_reaches_the_kernel_in_one_grouped_launch(ema, calls):   # noqa: F811
    """on the parent commit the override is dropped and tell_bertadam_step2 is recorded with the global values"""
    import tell_amd
    opt = _opt(OVERRIDE, **(dict(ema_decay=0.9, ema_warmup=4.0) if ema else {}))
    f = opt.flat
    skip = torch.zeros(2, dtype=torch.int32)
    wire = torch.zeros(f.total, dtype=torch.bfloat16)
    opt.launch(grad_scale=0.25, zero_grad=True, skip=skip, grad_wire=wire)
    assert [n for n, _ in calls] == ['tell_bertadam_step_groups']                 # one launch sequence, not one per group
    names = tell_amd.hip.parse_header()['tell_bertadam_step_groups'][2]
    args = calls[0][1]
    assert len(args) == len(names) - 1
    got = dict(zip(names, args))
    for key, t in (('param', f.flat), ('grad', f.grad), ('m', f.m), ('v', f.v), ('chunk_tensor', f.chunk_tensor),
                   ('chunk_begin', f.chunk_begin), ('partial', f.partial), ('norms', f.norms), ('lr_dev', opt.lr_dev),
                   ('tensor_group', f.tensor_group), ('step_dev', opt.step_dev), ('skip', skip), ('grad_wire_bf16', wire)):
        assert got[key] is t, key
    assert got['group_hp'] is opt.group_hp and isinstance(got['group_hp'], ctypes.Array)
    assert got['n_groups'] == 3 and got['n_tensors'] == 7 and got['n_chunks'] == f.n_chunks
    assert got['grad_scale'] == 0.25 and got['zero_grad'] == 1 and got['keep_grad'] is None and got['shadow_bf16'] is None
    rows = np.array(list(got['group_hp']), dtype=np.float32).reshape(3, 8)
    want = grp.table([dict(lr=1e-2, warmup=0.2, t_total=10, b1=0.9, b2=0.98, eps=1e-6, wd=0.0, max_norm=0.5),
                      dict(lr=1e-3, warmup=0.2, t_total=10, b1=0.9, b2=0.98, eps=1e-6, wd=1e-2, max_norm=0.0),
                      dict(lr=1e-2, warmup=0.2, t_total=10, b1=0.9, b2=0.98, eps=1e-6, wd=1e-2, max_norm=0.5)])
    assert np.array_equal(bits(rows), bits(want))
    assert np.array_equal(bits(rows), bits(grp.table([grp.row_of(g) for g in opt.groups])))
    assert f.tensor_group.tolist() == [1, 2, 0, 0, 2, 0, 2] == grp.resolve(NAMES, CFG, OVERRIDE)[1]
    assert int(f.tensor_group.max()) < got['n_groups'] and int(f.tensor_group.min()) >= 0
    if ema:
        assert got['ema'] is f.ema and got['ema_omd_dev'] is f.ema_omd and (got['ema_decay'], got['ema_warm']) == (0.9, 4.0)
    else:
        assert got['ema'] is None and got['ema_omd_dev'] is None and f.ema is None
    # groups are configuration, not state
    assert set(opt.state_dict()) == ({'step', 'm', 'v', 'ema'} if ema else {'step', 'm', 'v'})


def test_header_declares_the_grouped_entry_point():
    import tell_amd
    protos = tell_amd.hip.parse_header()
    res, types, names = protos['tell_bertadam_step_groups']
    assert res is ctypes.c_int
    ema_names = protos['tell_bertadam_step_ema'][2]
    gone = ['b1', 'b2', 'eps', 'wd', 'max_norm', 'lr_base', 'warmup', 't_total']
    want = [n for n in ema_names if n not in gone]
    i = want.index('lr_dev') + 1
    want[i:i] = ['tensor_group', 'group_hp', 'n_groups']
    assert names == want
    by = dict(zip(names, types))
    assert by['group_hp'] is ctypes.c_void_p and by['tensor_group'] is ctypes.c_void_p and by['n_groups'] is ctypes.c_int
    assert by['ema'] is ctypes.c_void_p and by['ema_decay'] is ctypes.c_float and by['stream'] is ctypes.c_void_p
    assert hasattr(tell_amd.hip.lib(), 'tell_bertadam_step_groups')


def test_current_lr_per_group():
    opt = _opt([[['bias', 'norm'], {'weight_decay': 0.0}],
                [['^decoder.embedder'], {'lr': 1e-3, 'warmup': 0.5, 't_total': 20}],
                [['adaptive'], {'lr': 3e-3, 't_total': -1}]])
    assert len(opt.groups) == 4
    with pytest.raises(ValueError, match='group='):
        opt.current_lr()
    with pytest.raises(ValueError, match='group='):
        opt.current_lr(3)
    for step in (0, 1, 2, 5, 9, 10, 15, 25):
        for gi, g in enumerate(opt.groups):
            want = ref.schedule(step, g['lr'], g['warmup'], g['t_total'])
            assert opt.current_lr(step, group=gi) == pytest.approx(want, rel=1e-6, abs=0.0), (step, gi)
        assert opt.current_lr(step, group='embedder') == opt.current_lr(step, group=1)
        assert opt.current_lr(step, group=r'conv\.weight') == opt.current_lr(step, group=3)
    assert opt.current_lr(7, group='adaptive') == 3e-3                              # t_total -1: constant
    opt.step_count = 5
    assert opt.current_lr(group=1) == opt.current_lr(5, group=1) == pytest.approx(1e-3 * 0.5)
    with pytest.raises(ValueError, match='2 groups'):
        opt.current_lr(1, group='conv')                     # conv.weight (default group) and conv.bias (group 0)
    with pytest.raises(ValueError, match='0 groups'):
        opt.current_lr(1, group='nobody')
    with pytest.raises(IndexError):
        opt.current_lr(1, group=4)


# ---------------------------------------------------------------- the reference itself
def _emulated(cid, aname, mutant=None, fused=True):
    c, d, kw, g = grp.case_kw(cid)
    tg, rows = grp.ASSIGNMENTS[aname]
    return d, grp.grouped(ref.emulate, d['p'], g, d['m'], d['v'], d['lay'], rows, tg, mutant=mutant, fused=fused, **kw)


def _differs(a, b):
    if a['lr'] != b['lr'] or a['applied'] != b['applied']:
        return True
    return any(not np.array_equal(bits(a[k]), bits(b[k])) for k in ('p', 'm', 'v'))


def test_rows_differ_in_every_value():
    for rows in (grp.ROWS, grp.ROWS_THREE):
        for key in grp.ROW_KEYS:
            vals = [float(np.float32(r[key])) for r in rows]
            assert len(set(vals)) == len(vals), key
        assert all(0 <= r['b1'] <= 1 and 0 <= r['b2'] <= 1 and r['eps'] > 0 for r in rows)
    assert grp.ROWS_THREE[0]['max_norm'] == 0 and grp.ROWS_THREE[1]['wd'] == 0 and grp.ROWS_THREE[2]['lr'] == 0
    assert len(grp.ROWS) == 16 and grp.table(grp.ROWS).shape == (16, 8)
    lay = ref.Layout(ref.SIZES)
    assert lay.n_tensors == 7 and lay.n_chunks == 30
    tg = np.asarray(grp.ASSIGNMENTS['alternating'][0])[lay.chunk_tensor]
    assert (tg[1:] != tg[:-1]).sum() == 6                   # every tensor boundary is a group boundary


def test_the_grouped_step_is_the_plain_step_tensor_by_tensor():
    """every tensor of group g comes out as optim_ref.emulate with g's row writes it; with one group the loop is the call"""
    for cid in grp.CASE_IDS:
        c, d, kw, g = grp.case_kw(cid)
        lay = d['lay']
        for aname, (tg, rows) in grp.ASSIGNMENTS.items():
            got = grp.grouped(ref.emulate, d['p'], g, d['m'], d['v'], lay, rows, tg, fused=True, **kw)
            eg = np.asarray(tg)[lay.tensor_of_elem()]
            assert got['applied'] and len(got['lr']) == len(rows)
            for gi, r in enumerate(rows):
                one = ref.emulate(d['p'], g, d['m'], d['v'], lay, dict(b1=r['b1'], b2=r['b2'], eps=r['eps'], wd=r['wd']),
                                  max_norm=r['max_norm'], lr_base=r['lr'], warmup=r['warmup'], t_total=r['t_total'],
                                  fused=True, **kw)
                for key in ('p', 'm', 'v', 'shadow'):
                    assert np.array_equal(bits(got[key])[eg == gi], bits(one[key])[eg == gi]), (cid, aname, gi, key)
                assert got['lr'][gi] == one['lr']
                if r['max_norm'] > 0:
                    assert np.array_equal(bits(got['norms']), bits(one['norms']))
            for key in ('p', 'm', 'v'):
                assert not bits(got[key])[~lay.real].any()               # the padding stays +0
            # and the float64 loop agrees with the fp32 one within the pinned constants
            want = grp.grouped(ref.step, d['p'], g, d['m'], d['v'], lay, rows, tg, **kw)
            r64 = ref.ratios(got, want)
            assert ref.inside(r64), (cid, aname, r64)


CAUGHT_BY = {'group_off_by_one': ('normal-clip0.5', 'alternating'), 'default_for_all': ('normal-clip0.5', 'alternating'),
             'clip_by_group0': ('normal-clip0.5', 'alternating'), 'shared_lr': ('normal-clip0.5', 'alternating')}


@pytest.mark.parametrize('mutant', grp.MUTANTS)
def test_mutant_is_rejected(mutant):
    """bit for bit on the case table; with one group every mutant is the reference itself"""
    first = None
    for cid in grp.CASE_IDS:
        for aname in grp.ASSIGNMENTS:
            d, want = _emulated(cid, aname)
            d, got = _emulated(cid, aname, mutant)
            if aname == 'one':
                assert not _differs(got, want), (cid, mutant)
            elif _differs(got, want) and first is None:
                first = (cid, aname)
    assert first == CAUGHT_BY[mutant]
    # each mutant is caught by what it gets wrong and by nothing else: rows that agree in that respect hide it
    c, d, kw, g = grp.case_kw('normal-clip0.5')
    tg = grp.ASSIGNMENTS['alternating'][0]
    same_rows = {'clip_by_group0': [grp.ROWS[0], dict(grp.ROWS[1], max_norm=grp.ROWS[0]['max_norm'])],
                 'shared_lr': [grp.ROWS[0], dict(grp.ROWS[1], **{k: grp.ROWS[0][k] for k in ('lr', 'warmup', 't_total')})],
                 'default_for_all': [grp.ROWS[1], grp.ROWS[1]], 'group_off_by_one': [grp.ROWS[1], grp.ROWS[1]]}[mutant]
    a = grp.grouped(ref.emulate, d['p'], g, d['m'], d['v'], d['lay'], same_rows, tg, fused=True, **kw)
    b = grp.grouped(ref.emulate, d['p'], g, d['m'], d['v'], d['lay'], same_rows, tg, fused=True, mutant=mutant, **kw)
    assert not _differs(a, b)


def test_skip_is_global_in_the_reference():
    """a NaN in a tensor of the group that does not clip: found by the norm pass another group asks for - nobody moves;
    with no clipping group it is not looked for"""
    c, d, kw, g = grp.case_kw('normal-clip0.5')
    lay = d['lay']
    tg, rows = grp.ASSIGNMENTS['three']
    g = g.copy()
    g[int(lay.offsets[3]) + 2] = np.nan                     # tensor 3 is of group 0, max_norm 0
    for fn in (ref.step, ref.emulate):
        got = grp.grouped(fn, d['p'], g, d['m'], d['v'], lay, rows, tg, skip=(0, 0), **kw)
        assert not got['applied'] and got['skip'] == (2, 1) and got['step'] == kw['step']
        assert np.array_equal(bits(np.asarray(got['p'], dtype=np.float32)), bits(d['p']))
        none_clips = [dict(r, max_norm=0.0) for r in rows]
        got = grp.grouped(fn, d['p'], g, d['m'], d['v'], lay, none_clips, tg, skip=(0, 0), **kw)
        assert got['applied'] and got['skip'] == (0, 0) and got['step'] == kw['step'] + 1 and got['norms'] is None
        assert np.isnan(got['p'][int(lay.offsets[3]) + 2]) and np.isfinite(np.asarray(got['p'])[lay.real]).sum() == lay.real.sum() - 1
    # an index outside the table counts as row 0
    a = grp.grouped(ref.emulate, d['p'], d['grads'][0], d['m'], d['v'], lay, rows, [0, 1, 2, 99, 1, 2, -1], **kw)
    b = grp.grouped(ref.emulate, d['p'], d['grads'][0], d['m'], d['v'], lay, rows, tg, **kw)
    assert not _differs(a, b)


def test_exact_lane_rows_are_exact_and_differ():
    """float64 rounded to fp32 = the kernels' fp32 arithmetic, fused or not = the closed form, for every layout; and two
    rows never give one element with a gradient the same (p', m, v), so a tensor updated with another group's row shows"""
    for k in range(len(ref.EXACT_LAYOUTS)):
        d = ref.exact_case(k)
        lay, tg = d['lay'], grp.exact_groups(k)
        kw = dict(zero_grad=1, lrs=[r['lr'] for r in grp.EXACT_ROWS])
        want = grp.grouped(ref.step, d['p'], d['g'], d['m'], d['v'], lay, grp.EXACT_ROWS, tg, **kw)
        w32 = ref.to_f32(want)
        closed = grp.exact_closed_form(k)
        for key in ('p', 'm', 'v'):
            assert np.array_equal(closed[key] * 512, np.round(closed[key] * 512)) and np.abs(closed[key]).max() < 2.0 ** 11
            assert np.array_equal(bits(w32[key]), bits(closed[key].astype(np.float32))), (k, key)
            assert not bits(w32[key])[~lay.real].any()
        for fused in (False, True):
            got = grp.grouped(ref.emulate, d['p'], d['g'], d['m'], d['v'], lay, grp.EXACT_ROWS, tg, fused=fused, **kw)
            for key in ('p', 'm', 'v', 'norms'):
                assert np.array_equal(bits(got[key]), bits(w32[key])), (k, fused, key)
            assert np.array_equal(got['shadow'], want['shadow'])
        assert np.array_equal(bits(w32['norms']), bits(d['norms'].astype(np.float32)))
        ps = []
        for r in grp.EXACT_ROWS:
            one = ref.step(d['p'], d['g'], d['m'], d['v'], lay, dict(b1=r['b1'], b2=r['b2'], eps=r['eps'], wd=r['wd']),
                           max_norm=r['max_norm'], zero_grad=1, lr=r['lr'])
            ps.append(ref.to_f32(one))
        hot = lay.real & (d['g'] != 0)
        for i in range(len(ps)):
            for j in range(i):              # (p' alone can coincide - rows 0 and 1 agree where p = 0; m or v then tells)
                other = np.zeros(lay.total, dtype=bool)
                for key in ('p', 'm', 'v'):
                    other |= bits(ps[i][key]) != bits(ps[j][key])
                assert other[hot].all(), (k, i, j)
                assert (bits(ps[i]['p']) != bits(ps[j]['p']))[hot].mean() > 0.9, (k, i, j)
