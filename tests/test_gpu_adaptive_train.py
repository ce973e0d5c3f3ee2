"""The adaptive embedding and loss kernels of the training step (the first 320 lines of csrc/adaptive.hip) and the adaptive
input embedding of the decode step (csrc/decode.hip) through the C ABI, element by element against the float64 reference
and the bounds of tests/adaptive_ref.py: tell_adaptive_partition, tell_embed_finalize,
tell_embed_finalize_bwd, tell_embed_table_grad, tell_ce_fwd, tell_ce_bwd, tell_sum_f32, tell_embed_gather_step,
tell_embed_lookup_step.  Every operand and every output is a view inside a buffer of sentinels (tests/guarded.py): after
each launch every guard band and every row gap is intact, and every read-only operand is bit for bit what was put in.  The
backward launches read what the forward launch stored.
Run on the MI355X box:  python -m pytest tests/test_gpu_adaptive_train.py -m gpu -s   (-s prints the ratios c is pinned from
and the time of the whole file)"""
import time

import numpy as np
import pytest
import torch

import adaptive_ref as ref
from guarded import Guard
from test_gpu_small_reduce import I32, TD, In, _gpu, host, intact, out_guard      # noqa: F401  (_gpu: the autouse fixture)

pytestmark = pytest.mark.gpu

OUTS = ('bfloat16', 'float32')
_RATIOS, _UNPINNED = {}, {}


@pytest.fixture(autouse=True)
def _fresh():
    _UNPINNED.clear()
    yield


@pytest.fixture(scope='module', autouse=True)
def _report():
    t0 = time.time()
    yield
    for k in sorted(_RATIOS):
        print('\nlargest (|got - ref| - u_out |ref|) / (gamma 2^-24 S)  %-12s %.6f   c = %s' % (k, _RATIOS[k], ref.C.get(k)))
    print('\n%s: %.1f s' % (__name__, time.time() - t0))


def int_guard(*shape):
    """an int32 output (host() reads it as fp32: every integer of these kernels is below 2^24)"""
    return Guard(shape, I32)


def check(got, o, tag):
    """`got` (Guard, tensor or numpy) against the Out `o`: exact and derived-bound outputs at once, a measured group against
    its pinned constant - or, not pinned yet, recorded for settle()"""
    got = got if isinstance(got, np.ndarray) else host(got)
    assert got.shape == np.shape(o.value), tag
    if o.group in ('exact', None):
        bad = ref.failures(got, o)
        assert bad == 0, '%s: %d of %d elements %s' % (tag, bad, got.size, 'differ' if o.group else 'outside the derived bound')
        return
    rt = ref.ratio(got, o)
    _RATIOS[o.group] = max(_RATIOS.get(o.group, 0.0), rt)
    print('ratio %-12s %-52s %.6f' % (o.group, tag, rt))
    if o.group not in ref.C:
        _UNPINNED[o.group] = max(_UNPINNED.get(o.group, 0.0), rt)
        assert np.isfinite(got[np.isfinite(np.asarray(o.value, np.float64))]).all(), tag
        assert o.exact_at is None or ref.same_bits(got[o.exact_at], np.asarray(o.value, np.float32)[o.exact_at]), tag
        return
    bad = ref.failures(got, o)
    assert bad == 0, '%s %s: %d of %d outside the bound (ratio %.4f, c = %g)' % (o.group, tag, bad, got.size, rt, ref.C[o.group])


def settle():
    """until c is pinned the test fails with the measured ratio in its message"""
    assert not _UNPINNED, 'constant not pinned yet, largest ratios of this case: %s' % \
        ', '.join('%s %.6f' % kv for kv in sorted(_UNPINNED.items()))


def ids(table):
    return [c['id'] for c in table]


def no_position_counter():
    from tell_amd import hip
    hip.call('tell_set_pos_step_ptr', None)


# ---------------------------------------------------------------- tell_adaptive_partition (exact)
def part_operands(case, N=None, nb=None):
    N, nb = max(case['N'] if N is None else N, 1), max(case['nb'] if nb is None else nb, 1)
    g = dict(rows=int_guard(nb, N), local=int_guard(nb, N), count=int_guard(nb), slot=int_guard(N), head_target=int_guard(N),
             n_valid=int_guard(1))
    return In(ref.part_inputs(case)['ids'], 'int64'), g


def part_call(case, src, g, N, nb, cut):
    from tell_amd import hip
    from tell_amd.decode import _ints
    opt = lambda k: None if k in case['null'] else g[k].t                                  # noqa: E731
    hip.call('tell_adaptive_partition', src.t, N, _ints(list(cut)), nb, case['pad'], g['rows'].t, g['local'].t, g['count'].t,
             opt('slot'), opt('head_target'), opt('n_valid'))


PART_LAUNCHED = [c for c in ref.PART if 1 <= c['nb'] <= 4 and c['N'] > 0]


@pytest.mark.parametrize('case', PART_LAUNCHED, ids=ids(PART_LAUNCHED))
def test_partition(case):
    """every list entry, count, slot, head target and n_valid; list entries past a band's count, the slots of ids outside
    every band and the outputs given as null pointers keep the sentinel"""
    src, g = part_operands(case)
    part_call(case, src, g, case['N'], case['nb'], ref.part_cut(case))
    intact(src, *g.values())
    want = ref.part_case(case)
    for k in g:
        if k in case['null']:
            assert g[k].untouched(), k
        else:
            check(g[k], want[k], '%s %s' % (case['id'], k))


# ---------------------------------------------------------------- tell_embed_finalize / _bwd (derived bounds)
@pytest.mark.parametrize('dty', OUTS)
@pytest.mark.parametrize('case', ref.FIN, ids=ids(ref.FIN))
def test_embed_finalize_and_backward(case, dty):
    from tell_amd import hip
    no_position_counter()
    x, B, T, E = ref.fin_inputs(case, dty), case['B'], case['T'], case['E']
    N, scale, code = B * T, ref.fin_scale(case), hip.dt(TD[dty])
    band, slot, tok = In(x['band_out'], dty), In(x['slot'], 'int32'), In(x['ids'], 'int64')
    pos, dout = In(x['pos_table'], 'float32'), In(x['dout'], dty)
    out, dband = out_guard((N, E), dty), out_guard((3 * N, E), dty, x['dband0'])
    hip.call('tell_embed_finalize', band.t, slot.t, tok.t, pos.t, case['pos_rows'] or ref.FIN_TABLE_ROWS, out.t, B, T, E, scale,
             ref.FIN_PAD, case['start'], case['tbc'], code)
    intact(band, slot, tok, pos, out)
    want = ref.fin_case(case, dty)
    check(out, want['out'], '%s %s out' % (case['id'], dty))
    hip.call('tell_embed_finalize_bwd', dout.t, slot.t, dband.t, B, T, E, scale, case['tbc'], code)
    intact(dout, slot, dband)
    check(dband, want['dband'], '%s %s dband' % (case['id'], dty))


# ---------------------------------------------------------------- tell_embed_table_grad (derived bound and bit for bit)
@pytest.mark.parametrize('dty', OUTS)
@pytest.mark.parametrize('case', ref.TG, ids=ids(ref.TG))
def test_embed_table_grad(case, dty):
    """against float64 with k = the band rows that name the table row, and bit for bit against the fp32 sum in increasing j
    added to the prefilled gradient once; a second launch on the same operands gives the same bits"""
    from tell_amd import hip
    x, dim, ld = ref.tg_inputs(case, dty), case['dim'], case['ld']
    drows, local = In(x['drows'], dty, (ld, 1)), In(x['local'], 'int32')
    count = In(np.array([case['count']]), 'int32')
    want, seen = ref.tg_case(case, dty), []
    for _ in range(2):
        demb = out_guard(x['demb0'].shape, 'float32', x['demb0'])
        hip.call('tell_embed_table_grad', drows.t, ld, local.t, count.t, case['cap'], demb.t, dim, case['pad'], hip.dt(TD[dty]))
        intact(drows, local, count, demb)
        seen.append(host(demb))
    check(seen[0], want['demb'], '%s %s demb' % (case['id'], dty))
    check(seen[0], want['demb_bits'], '%s %s demb, fp32 in increasing j' % (case['id'], dty))
    assert ref.same_bits(seen[0], seen[1]), 'two launches on the same operands differ'


# ---------------------------------------------------------------- tell_ce_fwd / tell_ce_bwd (measured)
@pytest.mark.parametrize('dty', OUTS)
@pytest.mark.parametrize('case', ref.CE, ids=ids(ref.CE))
def test_cross_entropy(case, dty):
    """the forward, then the backward on the lse the forward itself stored; rows at or past the count: loss = lse = 0, and
    their rows of dlogits, like the columns V .. ld_d - 1, keep the sentinel; ignored rows are zero up to sign"""
    from tell_amd import hip
    x, M, V, ld = ref.ce_inputs(case), case['M'], case['V'], case['ld']
    ld_d = (V + 7) // 8 * 8
    logits, tg = In(x['logits'], 'float32', (ld, 1)), In(x['targets'], 'int32')
    perm = None if x['row_idx'] is None else In(x['row_idx'], 'int32')
    m = None if case['m'] is None else In(np.array([case['m']]), 'int32')
    g = In(np.array([ref.CE_G[case['g']]]), 'float32')
    lse, loss = out_guard((M,), 'float32'), out_guard((M,), 'float32')
    dl = out_guard((M, V), dty, strides=(ld_d, 1))
    opt = lambda a: None if a is None else a.t                                             # noqa: E731
    hip.call('tell_ce_fwd', logits.t, ld, M, V, tg.t, opt(perm), opt(m), ref.CE_IGNORE, lse.t, loss.t)
    intact(logits, tg, perm, m, lse, loss)
    assert dl.untouched()
    want = ref.ce_case(case, dty)
    check(lse, want['lse'], '%s lse' % case['id'])
    check(loss, want['loss'], '%s loss' % case['id'])
    kept = host(lse)
    hip.call('tell_ce_bwd', logits.t, ld, M, V, tg.t, opt(perm), opt(m), ref.CE_IGNORE, lse.t, g.t, dl.t, ld_d, hip.dt(TD[dty]))
    intact(logits, tg, perm, m, g, lse, dl)
    assert ref.same_bits(host(lse), kept)
    want = ref.ce_case(case, dty, lse=kept)
    check(dl, want['dlogits'], '%s %s dlogits' % (case['id'], dty))
    zero = ref.ce_zero_rows(case) & ~want['dlogits'].exact_at[:, 0]
    assert (host(dl)[zero] == 0).all(), 'an ignored row is zero (up to sign)'
    settle()


# ---------------------------------------------------------------- tell_sum_f32 (derived bound and bit for bit)
@pytest.mark.parametrize('case', ref.SUM, ids=ids(ref.SUM))
def test_sum_f32(case):
    from tell_amd import hip
    x = ref.sum_inputs(case)
    src = In(x['x'], 'float32')
    m = None if case['m'] is None else In(np.array([case['m']]), 'int32')
    out = out_guard((1,), 'float32', np.array([x['out0']]))
    hip.call('tell_sum_f32', src.t, case['n'], None if m is None else m.t, out.t, case['acc'])
    intact(src, m, out)
    want = ref.sum_case(case)
    check(out, want['out'], '%s out' % case['id'])
    check(out, want['out_bits'], '%s out, fp32 in the kernel\'s order' % case['id'])


# ---------------------------------------------------------------- tell_embed_gather_step / tell_embed_lookup_step
def step_operands(case):
    x, (lo, hi, dim, off, ktot) = ref.step_inputs(case), ref.step_bands(case)
    return dict(ids=In(x['ids'], 'int64'), tables=[In(t, 'bfloat16') for t in x['tables']], pos=In(x['pos_table'], 'float32'),
                table=In(x['table'], 'float32'), cat=out_guard((case['M'], ktot), 'bfloat16'),
                pos_out=out_guard((case['M'], case['E']), 'float32'), out=out_guard((case['M'], case['E']), 'bfloat16'))


def step_launch(case, o, ktot=None, E=None, off=None):
    from tell_amd import hip
    from tell_amd.decode import _ints, _ptrs
    lo, hi, dim, off0, ktot0 = ref.step_bands(case)
    M, E, ktot = case['M'], case['E'] if E is None else E, ktot0 if ktot is None else ktot
    hip.call('tell_embed_gather_step', o['ids'].t, M, case['nb'], _ptrs([t.t for t in o['tables']]), _ints(list(lo)),
             _ints(list(hi)), _ints(list(dim)), _ints(list(off0 if off is None else off)), o['cat'].t, ktot, o['pos'].t,
             ref.STEP_POS_ROWS, ref.STEP_PAD, case['start'], o['pos_out'].t, E)
    hip.call('tell_embed_lookup_step', o['ids'].t, M, o['table'].t, hi[-1], o['pos'].t, ref.STEP_POS_ROWS, ref.STEP_PAD,
             case['start'], o['out'].t, E)


@pytest.mark.parametrize('case', ref.STEP, ids=ids(ref.STEP))
def test_step_embedding(case):
    """cat and pos_out bit for bit, the looked-up embedding inside one fp32 sum and a bf16 store; one case with a device
    counter of 3 registered through tell_set_pos_step_ptr (the next-offset word stays unset)"""
    from tell_amd import hip
    no_position_counter()
    o = step_operands(case)
    counter = None if case['step'] is None else torch.full((1,), case['step'], dtype=I32, device='cuda')
    try:
        if counter is not None:
            hip.call('tell_set_pos_step_ptr', counter)
        step_launch(case, o)
        torch.cuda.synchronize()
    finally:
        no_position_counter()
    intact(o['ids'], o['pos'], o['table'], o['cat'], o['pos_out'], o['out'], *o['tables'])
    assert counter is None or int(counter.item()) == case['step']
    want = ref.step_case(case)
    for k in ('cat', 'pos_out', 'out'):
        check(o[k], want[k], '%s %s' % (case['id'], k))


# ---------------------------------------------------------------- refusals and launches that write nothing
def test_refused_calls_and_empty_launches_write_nothing():
    """partition with 0 or 5 bands (the binding's error) and with N = 0 (returns at once: band_count and n_valid included);
    the step embedding with ktot % 8, E % 4 and a band past ktot"""
    from tell_amd import hip
    for case in [c for c in ref.PART if c not in PART_LAUNCHED]:
        src, g = part_operands(case, N=8, nb=5)
        if 1 <= case['nb'] <= 4:
            part_call(case, src, g, case['N'], case['nb'], ref.part_cut(case))
        else:
            with pytest.raises(RuntimeError, match='tell_adaptive_partition'):
                part_call(case, src, g, case['N'], case['nb'], ref.part_cut(case) or (100,))
        intact(src, *g.values())
        assert all(v.untouched() for v in g.values()), case['id']
        for k, o in ref.part_case(case).items():
            assert (o.value == ref.SENTINEL).all(), k
    no_position_counter()
    case = next(c for c in ref.STEP if c['nb'] == 3 and c['step'] is None)
    o = step_operands(case)
    lo, hi, dim, off, ktot = ref.step_bands(case)
    for kw in (dict(ktot=ktot - 4), dict(E=case['E'] - 2), dict(off=(off[0], off[1], off[2] + 8))):
        with pytest.raises(RuntimeError, match='tell_embed_gather_step'):
            step_launch(case, o, **kw)
    with pytest.raises(RuntimeError, match='tell_embed_lookup_step'):
        hip.call('tell_embed_lookup_step', o['ids'].t, case['M'], o['table'].t, hi[-1], o['pos'].t, ref.STEP_POS_ROWS,
                 ref.STEP_PAD, case['start'], o['out'].t, case['E'] - 2)
    torch.cuda.synchronize()
    assert o['cat'].untouched() and o['pos_out'].untouched() and o['out'].untouched()
