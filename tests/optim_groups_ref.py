"""Reference for BertAdam's parameter groups (tell_bertadam_step_groups, csrc/optim.hip), numpy only,
on top of tests/optim_ref.py:
  * resolve():  the group resolution of training/optimizers.py restated (first matching listed group wins, the rest go to
                the default group, empty groups dropped, equal groups merged);
  * grouped():  the grouped step as a thin loop over optim_ref.step (float64) or optim_ref.emulate (the kernels' fp32
                arithmetic): one call per group with that group's row, every tensor taken from the call of its group; what
                is global - the norm pass, the non-finite flag, the skip, the step counter - is taken once;
  * MUTANTS:    deliberately wrong variants of grouped() that a bit-for-bit comparison has to reject;
  * the case tables shared by tests/test_optim_groups_host.py and tests/test_gpu_optim_groups.py."""
import re

import numpy as np

import optim_ref as ref

ROW_KEYS = ('lr', 'warmup', 't_total', 'b1', 'b2', 'eps', 'wd', 'max_norm')          # a row of group_hp, in its order
HOST_KEYS = ('lr', 'warmup', 't_total', 'b1', 'b2', 'e', 'weight_decay', 'max_grad_norm')        # BertAdam's names for them
MAX_GROUPS = 16
MUTANTS = ('group_off_by_one', 'default_for_all', 'clip_by_group0', 'shared_lr')


# ---------------------------------------------------------------- group resolution
def resolve(names, defaults, parameter_groups):
    """-> ([dict(HOST_KEYS..., names=[...])], [group index per name]); no validation, no warnings - semantics only"""
    listed = [(list(rxs), dict(defaults, **{k: v for k, v in over.items() if k != 'schedule'}))
              for rxs, over in (parameter_groups or [])]
    homes = []
    for name in names:
        hit = [i for i, (rxs, _) in enumerate(listed) if any(re.search(rx, name) for rx in rxs)]
        homes.append(hit[0] if hit else len(listed))
    values = [v for _, v in listed] + [dict(defaults)]
    groups, seen, where = [], {}, {}
    for i, vals in enumerate(values):
        if i not in homes:                                   # empty: dropped
            continue
        key = tuple(float(vals[k]) for k in HOST_KEYS)
        if key not in seen:
            seen[key] = len(groups)
            groups.append(dict(vals, names=[]))
        where[i] = seen[key]                                 # equal values: merged into the first of them
    tensor_group = [where[h] for h in homes]
    for n, gi in zip(names, tensor_group):
        groups[gi]['names'].append(n)
    return groups, tensor_group


def row_of(group):
    """a resolved group of BertAdam (HOST_KEYS) -> a row dict (ROW_KEYS)"""
    return dict(zip(ROW_KEYS, (group[k] for k in HOST_KEYS)))


def table(rows):
    """rows -> the fp32 array [n_groups, 8] that tell_bertadam_step_groups takes"""
    return np.array([[r[k] for k in ROW_KEYS] for r in rows], dtype=np.float32)


# ---------------------------------------------------------------- the grouped step
def grouped(fn, p, g, m, v, lay, rows, tensor_group, step=None, lrs=None, mutant=None, **kw):
    """fn: optim_ref.step or optim_ref.emulate (or anything with their signature and result - the GPU tests pass a function
    that runs tell_bertadam_step2 on the device).  step None: lrs[g] is what the caller left in lr_dev[g].  kw: grad_scale,
    zero_grad, keep_grad, skip, wire (and p_dev for optim_ref.step).  -> the dict of fn with `lr` a list per group and
    every per-element entry (aux included) taken from the call of the element's group."""
    rows = [dict(r) for r in rows]
    tg = np.asarray(tensor_group, dtype=np.int64)
    tg = np.where((tg >= 0) & (tg < len(rows)), tg, 0)                # an index outside the table counts as row 0
    if mutant == 'group_off_by_one':
        tg = (tg + 1) % len(rows)
    if mutant == 'default_for_all':
        rows = [dict(rows[-1]) for _ in rows]
    if mutant == 'clip_by_group0':
        rows = [dict(r, max_norm=rows[0]['max_norm']) for r in rows]
    outs = []
    for gi, r in enumerate(rows):
        s = rows[0] if mutant == 'shared_lr' else r
        if step is not None:
            lr_kw = dict(step=step, lr_base=s['lr'], warmup=s['warmup'], t_total=s['t_total'])
        else:
            lr_kw = dict(lr=lrs[0 if mutant == 'shared_lr' else gi])
        outs.append(fn(p, g, m, v, lay, dict(b1=r['b1'], b2=r['b2'], eps=r['eps'], wd=r['wd']), max_norm=r['max_norm'],
                       **lr_kw, **kw))
    # the norm pass runs iff any row clips, and then looks at every tensor: its verdict is the verdict of the step
    clipping = [o for o, r in zip(outs, rows) if np.float32(r['max_norm']) > 0]
    probe = clipping[0] if clipping else outs[0]
    out = dict(probe, lr=[o['lr'] for o in outs], norms=probe['norms'] if clipping else None)
    if not probe['applied']:
        return out
    eg = tg[lay.tensor_of_elem()]
    for key in ('p', 'm', 'v', 'shadow', 'e'):              # ('e': a moving average, where fn keeps one)
        if probe.get(key) is None:
            continue
        merged = np.array(probe[key])
        for gi, o in enumerate(outs):
            merged[eg == gi] = o[key][eg == gi]
        out[key] = merged
    if probe['aux'] is not None:
        aux = {}
        for key in probe['aux']:
            merged = np.array(np.broadcast_to(np.asarray(probe['aux'][key]), (lay.total,)))
            for gi, o in enumerate(outs):
                merged[eg == gi] = np.broadcast_to(np.asarray(o['aux'][key]), (lay.total,))[eg == gi]
            aux[key] = merged
        out['aux'] = aux
    return out


# ---------------------------------------------------------------- the random lane's table
def _row(k):
    """rows that differ from one another in every one of the eight values (b1, b2 and the rest well inside their ranges)"""
    return dict(lr=1e-2 * (1 + 0.5 * k), warmup=0.2 + 0.05 * k, t_total=10.0 + 2 * k, b1=0.9 - 0.05 * k, b2=0.98 - 0.01 * k,
                eps=1e-6 * (1 + k), wd=1e-2 * (1 + k), max_norm=0.5 / (1 + k))


ROWS = [_row(k) for k in range(MAX_GROUPS)]
# one group without a clip, one without weight decay, one with the learning rate 0
ROWS_THREE = [dict(_row(7), max_norm=0.0), dict(_row(8), wd=0.0), dict(_row(9), lr=0.0)]
N_TENSORS = len(ref.SIZES)
ASSIGNMENTS = {
    'one': ([0] * N_TENSORS, ROWS[:1]),
    'alternating': ([t % 2 for t in range(N_TENSORS)], ROWS[:2]),                    # neighbouring chunks differ
    'seven': (list(range(N_TENSORS)), ROWS[:N_TENSORS]),                             # one group per tensor
    'three': ([t % 3 for t in range(N_TENSORS)], ROWS_THREE),
}
# the cases of optim_ref.CASES the grouped launch is run on: fp32 gradient with shadow and mixed keep_grad; the bf16 wire
# gradient without shadow and without zeroing; a gradient scale that moves a norm across a threshold; plain
CASE_IDS = ('normal-clip0.5', 'heavy-clip0.5-keepmixed', 'wire-gs8-heavy-clip0.1', 'gs8-clip0.5')


def case_kw(cid):
    """-> (c, d, kw of grouped() for step 0, the fp32 gradient buffer)"""
    c = ref.BY_ID[cid]
    d = ref.make_case(c)
    args, g = ref.step_args(c, d, 0)
    kw = dict(grad_scale=args['grad_scale'], zero_grad=args['zero_grad'], keep_grad=args['keep_grad'], step=args['step'])
    if 'wire' in args:
        kw['wire'] = args['wire']
    return c, d, kw, g


# ---------------------------------------------------------------- the exact lane
# optim_ref's exact lane (m = v = 0, every non-zero g' = +-2^5 after the clip, max_norm 2^8 for all) with four rows of
# powers of two: r0 is EXACT_HP; r1: m = g'/4, sqrt(v) + eps = 2^5, u = +-1/4; r2: v = g'^2/16, sqrt(v) + eps = 2^4, u = +-1;
# r3: b1 = b2 = 0, m = g', v = g'^2, sqrt(v) + eps = 2^6, u = +-1/2.  lr and wd are powers of two, p small integers: every
# product and sum is a multiple of 2^-9 below 2^11 - exact in fp32 in any association, fused or not - and every row gives
# another p', m and v for the same inputs.
EXACT_ROWS = [
    dict(lr=2.0 ** -3, warmup=-1.0, t_total=-1.0, b1=0.5, b2=0.75, eps=16.0, wd=2.0 ** -4, max_norm=256.0),
    dict(lr=2.0 ** -2, warmup=-1.0, t_total=-1.0, b1=0.75, b2=0.75, eps=16.0, wd=2.0 ** -3, max_norm=256.0),
    dict(lr=2.0 ** -4, warmup=-1.0, t_total=-1.0, b1=0.5, b2=0.9375, eps=8.0, wd=2.0 ** -5, max_norm=256.0),
    dict(lr=2.0 ** -1, warmup=-1.0, t_total=-1.0, b1=0.0, b2=0.0, eps=32.0, wd=2.0 ** -2, max_norm=256.0),
]


def exact_groups(k):
    """tensor t of exact layout k -> row (t + k) % 4"""
    return [(t + k) % len(EXACT_ROWS) for t in range(len(ref.EXACT_LAYOUTS[k][0]))]


def exact_closed_form(k):
    """p', m', v' of exact layout k by the closed form, per element, in float64: g' = g x 2^-j of the tensor"""
    d = ref.exact_case(k)
    lay = d['lay']
    tg = np.asarray(exact_groups(k))[lay.tensor_of_elem()]
    j = np.array([s[1] for s in ref.EXACT_LAYOUTS[k][1]], dtype=np.float64)[lay.tensor_of_elem()]
    col = lambda key: np.array([r[key] for r in EXACT_ROWS])[tg]                     # noqa: E731
    gp = d['g'].astype(np.float64) * 2.0 ** -j
    m = (1 - col('b1')) * gp
    v = (1 - col('b2')) * gp * gp
    p0 = d['p'].astype(np.float64)
    p = p0 - col('lr') * (m / (np.sqrt(v) + col('eps')) + col('wd') * p0)
    return dict(p=p, m=m, v=v)
