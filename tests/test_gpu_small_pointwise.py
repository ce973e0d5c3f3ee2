"""The movers and pointwise small kernels of the training step (csrc/elementwise.hip, csrc/multi.hip, csrc/encoders.hip)
through the C ABI against tests/small_ref.py.  Bit for bit: tell_cast, tell_gather_rows, tell_nan_rows,
tell_relu_bwd, tell_mask_rows, the positions of tell_roberta_embed and the masks of tell_dropout / tell_dropout_add (against
tell_amd.rng.keep_mask).  Held to the derived bound of one element (no measured constant): tell_scale_cast, tell_axpy,
tell_sum_n, tell_scatter_add_rows, tell_gelu (against float64 erf), tell_loss_bits, the sum of tell_roberta_embed and the kept
elements of the dropouts.  Against a measured constant: tell_glu_fwd / tell_glu_bwd.
Every operand and every output is a view inside a buffer of sentinels (tests/guarded.py): after each launch every guard band
and every row gap is intact, read-only operands are bit for bit what was put in, and rows past a device-side count keep the
sentinel.  A refused call launches nothing.
Run on the MI355X box:  python -m pytest tests/test_gpu_small_pointwise.py -m gpu"""
import numpy as np
import pytest
import torch

import small_ref as ref
from guarded import Guard
from test_gpu_small_reduce import (F32, TD, In, _gpu, check, host, intact, out_guard,      # noqa: F401  (_gpu: the autouse
                                   settle)                                                  # fixture)

pytestmark = pytest.mark.gpu


def cases(op):
    return [c for c in ref.PW if c['op'] == op]


def ids(op):
    return [c['id'] for c in cases(op)]


@pytest.mark.parametrize('case', cases('cast'), ids=ids('cast'))
def test_cast(case):
    from tell_amd import hip
    x = In(ref.pw_inputs(case)['x'], case['src'])
    dst = out_guard((case['n'],), case['dst'])
    hip.call('tell_cast', x.t, hip.dt(TD[case['src']]), dst.t, hip.dt(TD[case['dst']]), case['n'])
    intact(x, dst)
    check(dst, ref.pw_case(case)['dst'], case['id'])


@pytest.mark.parametrize('case', cases('scale_cast'), ids=ids('scale_cast'))
def test_scale_cast(case):
    """fp32: in place (dst is src); bf16: a buffer of its own.  scale: a null pointer or one float on the device"""
    from tell_amd import hip
    x0, n = ref.pw_inputs(case)['x'], case['n']
    sc = None if case['scale'] is None else In(np.array([case['scale']], np.float32), 'float32')
    if case['dst'] == 'float32':
        dst = src = out_guard((n,), 'float32', x0)
    else:
        src, dst = In(x0, 'float32'), out_guard((n,), 'bfloat16')
    hip.call('tell_scale_cast', src.t, dst.t, hip.dt(TD[case['dst']]), n, None if sc is None else sc.t)
    intact(src, dst, sc)
    check(dst, ref.pw_case(case)['dst'], case['id'])


@pytest.mark.parametrize('case', cases('axpy'), ids=ids('axpy'))
def test_axpy(case):
    from tell_amd import hip
    v = ref.pw_inputs(case)
    x, y = In(v['x'], case['dtype']), out_guard((case['n'],), case['dtype'], v['y'])
    hip.call('tell_axpy', x.t, y.t, case['n'], v['alpha'], hip.dt(TD[case['dtype']]))
    intact(x, y)
    check(y, ref.pw_case(case)['y'], case['id'])


@pytest.mark.parametrize('case', cases('sum_n'), ids=ids('sum_n'))
def test_sum_n(case):
    from tell_amd import hip
    xs = [In(a, case['dtype']) for a in ref.pw_inputs(case)['xs']]
    out = out_guard((case['n'],), case['dtype'])
    hip.call('tell_sum_n', *([x.t for x in xs] + [None] * (8 - len(xs))), len(xs), out.t, case['n'], hip.dt(TD[case['dtype']]))
    intact(out, *xs)
    check(out, ref.pw_case(case)['out'], case['id'])


@pytest.mark.parametrize('case', cases('relu_bwd'), ids=ids('relu_bwd'))
def test_relu_bwd(case):
    """y = +0, -0 and negative pass nothing, and what is passed is dy bit for bit"""
    from tell_amd import hip
    v = ref.pw_inputs(case)
    dy, y, dx = In(v['dy'], case['dtype']), In(v['y'], case['dtype']), out_guard((case['n'],), case['dtype'])
    hip.call('tell_relu_bwd', dy.t, y.t, dx.t, case['n'], hip.dt(TD[case['dtype']]))
    intact(dy, y, dx)
    check(dx, ref.pw_case(case)['dx'], case['id'])


def _count(case):
    return None if case['count'] is None else In(np.array([case['count']]), 'int32')


@pytest.mark.parametrize('case', cases('gather'), ids=ids('gather'))
def test_gather_rows(case):
    """cap 2100 of 2550 rows: past the 2048-block grid; rows past min(count, cap) keep the sentinel"""
    from tell_amd import hip
    v, Cc = ref.pw_inputs(case), case['C']
    src, idx, cnt = In(v['src'], case['dtype'], (Cc + 3, 1)), In(v['idx'], 'int32'), _count(case)
    dst = out_guard((ref.PW_ROWS, Cc), case['dtype'], strides=(Cc + 2, 1))
    hip.call('tell_gather_rows', src.t, Cc + 3, idx.t, None if cnt is None else cnt.t, case['cap'], dst.t, Cc + 2, Cc,
             hip.dt(TD[case['dtype']]))
    intact(src, idx, cnt, dst)
    check(dst, ref.pw_case(case)['dst'], case['id'])


@pytest.mark.parametrize('case', cases('scatter'), ids=ids('scatter'))
def test_scatter_add_rows(case):
    """unique indices; the rows of dst that no index names stay bit for bit"""
    from tell_amd import hip
    v, Cc = ref.pw_inputs(case), case['C']
    src, idx, cnt = In(v['src'], case['dtype'], (Cc + 3, 1)), In(v['idx'], 'int32'), _count(case)
    dst = out_guard(v['dst0'].shape, case['dtype'], v['dst0'], strides=(Cc + 2, 1))
    hip.call('tell_scatter_add_rows', src.t, Cc + 3, idx.t, None if cnt is None else cnt.t, case['cap'], dst.t, Cc + 2, Cc,
             hip.dt(TD[case['dtype']]))
    intact(src, idx, cnt, dst)
    check(dst, ref.pw_case(case)['dst'], case['id'])


@pytest.mark.parametrize('case', cases('nan_rows'), ids=ids('nan_rows'))
def test_nan_rows(case):
    """a NaN in the first, the last or the 64th-plus column masks and zeroes the row; a row holding only inf stays"""
    from tell_amd import hip
    x = In(ref.pw_inputs(case)['x'], 'float32')
    y = out_guard((ref.NAN_ROWS, case['C']), case['dtype'])
    mask = Guard((ref.NAN_ROWS,), torch.uint8)
    hip.call('tell_nan_rows', x.t, ref.NAN_ROWS, case['C'], y.t, hip.dt(TD[case['dtype']]), mask.t)
    intact(x, y, mask)
    want = ref.pw_case(case)
    check(y, want['y'], case['id'] + ' y')
    check(mask, want['mask'], case['id'] + ' mask')


@pytest.mark.parametrize('case', cases('glu'), ids=ids('glu'))
def test_glu(case):
    """gate values in +-20; the forward and the backward of the same h"""
    from tell_amd import hip
    v, rows, Cc, dty = ref.pw_inputs(case), case['rows'], case['C'], case['dtype']
    h, dy = In(v['h'], dty), In(v['dy'], dty)
    y, dh = out_guard((rows, Cc), dty), out_guard((rows, 2 * Cc), dty)
    hip.call('tell_glu_fwd', h.t, y.t, rows, Cc, hip.dt(TD[dty]))
    hip.call('tell_glu_bwd', h.t, dy.t, dh.t, rows, Cc, hip.dt(TD[dty]))
    intact(h, dy, y, dh)
    want = ref.pw_case(case)
    check(y, want['y'], case['id'] + ' y')
    check(dh, want['dh'], case['id'] + ' dh')
    settle()


@pytest.mark.parametrize('case', cases('gelu'), ids=ids('gelu'))
def test_gelu(case):
    """against float64 erf, x in +-6; in place too"""
    from tell_amd import hip
    x0, n = ref.pw_inputs(case)['x'], case['n']
    x, y, both = In(x0, 'bfloat16'), out_guard((n,), 'bfloat16'), out_guard((n,), 'bfloat16', x0)
    hip.call('tell_gelu', x.t, y.t, n, hip.dt(torch.bfloat16))
    hip.call('tell_gelu', both.t, both.t, n, hip.dt(torch.bfloat16))
    intact(x, y, both)
    check(y, ref.pw_case(case)['y'], case['id'])
    assert ref.same_bits(host(y), host(both))


@pytest.mark.parametrize('case', cases('dropout') + cases('dropout_add'), ids=ids('dropout') + ids('dropout_add'))
def test_dropout(case):
    """the mask is tell_amd.rng.keep_mask over the element indices, bit for bit (a dropped element is x * 0 [+ add]); both
    entry points see the same mask for the same seed, salt and index"""
    from tell_amd import hip
    v, n, dty = ref.pw_inputs(case), case['n'], case['dtype']
    x, add, y = In(v['x'], dty), In(v['add'], dty), out_guard((n,), dty)
    if case['op'] == 'dropout':
        hip.call('tell_dropout', x.t, y.t, n, case['p'], ref.SEED, ref.SALT, hip.dt(TD[dty]))
    else:
        hip.call('tell_dropout_add', x.t, add.t, y.t, n, case['p'], ref.SEED, ref.SALT, hip.dt(TD[dty]))
    intact(x, add, y)
    check(y, ref.pw_case(case)['y'], case['id'])


def test_loss_bits():
    from tell_amd import hip
    case = cases('loss_bits')[0]
    v = ref.pw_inputs(case)
    x, n, out = In(np.array([v['x']]), 'float32'), In(np.array([v['n']]), 'int32'), out_guard((1,), 'float32')
    hip.call('tell_loss_bits', x.t, n.t, out.t)
    intact(x, n, out)
    check(out, ref.pw_case(case)['out'], 'loss_bits')


@pytest.mark.parametrize('case', cases('embed'), ids=ids('embed'))
def test_roberta_embed(case):
    """B = 3: pads at the front, in the middle, an all-pad row; the positions workspace exactly"""
    from tell_amd import hip
    v, S, E, dty = ref.pw_inputs(case), case['S'], case['E'], case['dtype']
    ids_, word, posemb = In(v['ids'], 'int64'), In(v['word'], dty), In(v['posemb'], dty)
    pos, out = Guard((3, S), torch.int32), out_guard((3, S, E), dty)
    hip.call('tell_roberta_embed', ids_.t, 3, S, v['pad'], word.t, posemb.t, pos.t, out.t, E, hip.dt(TD[dty]))
    intact(ids_, word, posemb, pos, out)
    want = ref.pw_case(case)
    check(pos, want['pos'], case['id'] + ' positions')
    check(out, want['out'], case['id'] + ' out')


@pytest.mark.parametrize('case', cases('mask_rows'), ids=ids('mask_rows'))
def test_mask_rows(case):
    """4096 + 50 rows: the grid's second trip; in place, unmasked rows bit for bit"""
    from tell_amd import hip
    v = ref.pw_inputs(case)
    x, mask = out_guard(v['x'].shape, case['dtype'], v['x']), In(v['mask'], 'uint8')
    hip.call('tell_mask_rows', x.t, mask.t, case['rows'], case['C'], hip.dt(TD[case['dtype']]))
    intact(x, mask)
    check(x, ref.pw_case(case)['x'], case['id'])


def test_refused_calls_launch_nothing():
    """sum_n, dropout_add, gelu: a partial 16-byte chunk, a misaligned buffer (sum_n: no or nine inputs, a null input) - the
    binding's error, the output untouched"""
    from tell_amd import hip
    a = In(np.zeros(1032, np.float32), 'float32')
    off = In(np.zeros(1032, np.float32), 'float32', off=1)
    out = out_guard((1032,), 'float32')
    code = hip.dt(F32)
    for args in ((a.t, a.t, None, None, None, None, None, None, 2, out.t, 1030, code),
                 (a.t, off.t, None, None, None, None, None, None, 2, out.t, 1024, code),
                 (a.t, None, None, None, None, None, None, None, 2, out.t, 1024, code),
                 (a.t, a.t, None, None, None, None, None, None, 0, out.t, 1024, code),
                 (a.t,) * 8 + (9, out.t, 1024, code)):
        with pytest.raises(RuntimeError, match='tell_sum_n'):
            hip.call('tell_sum_n', *args)
    with pytest.raises(RuntimeError, match='tell_scale_cast'):
        hip.call('tell_scale_cast', off.t, out.t, code, 1024, None)
    with pytest.raises(RuntimeError, match='tell_cast'):
        hip.call('tell_cast', a.t, 7, out.t, code, 1024)
    for args in ((a.t, a.t, out.t, 1030, 0.1, 1, 2, code), (a.t, off.t, out.t, 1024, 0.1, 1, 2, code),
                 (off.t, a.t, out.t, 1024, 0.1, 1, 2, code), (a.t, a.t, out.t, 1024, 1.0, 1, 2, code)):
        with pytest.raises(RuntimeError, match='tell_dropout_add'):
            hip.call('tell_dropout_add', *args)
    h, h_off, hy = In(np.zeros(1032, np.float32), 'bfloat16'), In(np.zeros(1032, np.float32), 'bfloat16', off=1), \
        out_guard((1032,), 'bfloat16')
    bf = hip.dt(torch.bfloat16)
    for args in ((h.t, hy.t, 1028, bf), (h_off.t, hy.t, 1024, bf), (a.t, out.t, 1024, code)):
        with pytest.raises(RuntimeError, match='tell_gelu'):
            hip.call('tell_gelu', *args)
    torch.cuda.synchronize()
    assert out.untouched() and hy.untouched() and a.intact() and off.intact()
