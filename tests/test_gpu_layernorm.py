"""The LayerNorm kernels (csrc/layernorm.hip: tell_layernorm_fwd / _bwd, tell_layernorm_cat_fwd / _bwd; csrc/decode.hip:
tell_layernorm_rows) through the C ABI, element by element against the float64 reference and the bounds of tests/ln_ref.py
(DESIGN.md section 36).  Every operand and every output is a view inside a buffer of sentinels (tests/guarded.py): after each
launch every guard band and every row gap is intact, every read-only operand is bit for bit what was put in, and a refused
call leaves its outputs untouched.  A backward launch is fed the mean / rstd the forward launch itself stored, and its
reference is computed from those; the forward holds mean and rstd to float64.
Run on the MI355X box:  python -m pytest tests/test_gpu_layernorm.py -m gpu -s   (-s prints the ratios c is pinned from and the
time of the whole file)"""
import contextlib
import ctypes
import time

import numpy as np
import pytest
import torch

import ln_ref as ref
from test_gpu_small_reduce import F32, TD, In, _gpu, host, intact, out_guard      # noqa: F401  (_gpu: the autouse fixture)

pytestmark = pytest.mark.gpu

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


def check(got, o, tag):
    """`got` (Guard, tensor or numpy) against the Out `o`: a measured group against its pinned constant - or, not pinned yet,
    recorded for settle(); the elements of exact_at bit for bit either way"""
    got = got if isinstance(got, np.ndarray) else host(got)
    assert got.shape == np.shape(o.value), tag
    rt = ref.ratio(got, o)
    _RATIOS[o.group] = max(_RATIOS.get(o.group, 0.0), rt)
    print('ratio %-12s %-52s %.6f' % (o.group, tag, rt))
    if o.group not in ref.C:
        _UNPINNED[o.group] = max(_UNPINNED.get(o.group, 0.0), rt)
        assert np.isfinite(got[np.isfinite(np.asarray(o.value, np.float64))]).all(), tag
        if o.exact_at is not None:
            assert not got[o.exact_at].any(), '%s: a dropped element is not zero' % tag
        return
    bad = ref.failures(got, o)
    assert bad == 0, '%s %s: %d of %d outside the bound (ratio %.4f, c = %g)' % (o.group, tag, bad, got.size, rt, ref.C[o.group])


def settle():
    """until c is pinned the test fails with the measured ratio in its message"""
    assert not _UNPINNED, 'constant not pinned yet, largest ratios of this case: %s' % \
        ', '.join('%s %.6f' % kv for kv in sorted(_UNPINNED.items()))


def ids(table):
    return [c['id'] for c in table]


def t_(g):
    return None if g is None else g.t


def option(value):
    """ln_var through tell_set_option, the previous value put back on the way out (hip.options restores in __exit__)"""
    from tell_amd import hip
    return contextlib.nullcontext() if value is None else hip.options(ln_var=value)


def u32s(vals):
    return (ctypes.c_uint32 * len(vals))(*vals)


# ---------------------------------------------------------------- tell_layernorm_fwd / tell_layernorm_bwd
@pytest.mark.parametrize('case', ref.LN, ids=ids(ref.LN))
def test_layernorm_forward_and_backward(case):
    """the forward (y, mean, rstd against float64; a null mean changes no bit of y; two rows per wave against ln_var 0 bit for
    bit), then the backward on the stored statistics: dx, dres (stored or accumulated onto a prefill), partial, dgamma and dbeta
    (stored or accumulated), or dgamma null"""
    from tell_amd import hip
    v, rows, Cc, dty = ref.ln_inputs(case), case['rows'], case['C'], case['dtype']
    ld, code, salt, has_res = Cc + case['pad'], hip.dt(TD[dty]), ref.ln_salt(case), case['res']
    off = lambda who: int(case['off'] == who)                                                    # noqa: E731
    x = In(v['x'], dty, (ld, 1), off('x'))
    res = In(v['res'], dty, (ld, 1), off('res')) if has_res else None
    gamma, beta = In(v['gamma'], 'float32'), In(v['beta'], 'float32')
    ins = [x, res, gamma, beta]

    def forward(with_stats=True):
        y = out_guard((rows, Cc), dty, None, (ld, 1), off('y'))
        mean, rstd = (out_guard((rows,), 'float32'), out_guard((rows,), 'float32')) if with_stats else (None, None)
        hip.call('tell_layernorm_fwd', x.t, ld, t_(res), ld if has_res else 0, gamma.t, beta.t, y.t, ld, t_(mean), t_(rstd),
                 rows, Cc, case['eps'], case['p'], ref.SEED, salt, code)
        intact(*(ins + [y, mean, rstd]))
        return y, mean, rstd

    with option(case['ln_var']):
        y, mean, rstd = forward()
        y_only = forward(False)[0]
    mk, rk = host(mean), host(rstd)
    want = ref.ln_case(case, stats=(mk, rk))
    for k, g in (('y', y), ('mean', mean), ('rstd', rstd)):
        check(g, want[k], '%s %s' % (case['id'], k))
    assert ref.same_bits(host(y_only), host(y)), 'a null mean changes y'
    if ref.ln_fwd_path(case) == 'fwd:rows2':
        with option(0):
            one = forward()
        for a, b, k in zip(one, (y, mean, rstd), ('y', 'mean', 'rstd')):
            assert ref.same_bits(host(a), host(b)), 'two rows per wave: %s differs from one row per wave' % k
    if not case['bwd']:
        settle()
        return
    nb = hip.lib().tell_layernorm_bwd_blocks(rows)
    assert nb == -(-rows // 4)
    dy = In(v['dy'], dty, (ld, 1), off('dy'))
    dx = out_guard((rows, Cc), dty, None, (ld, 1), off('dx')) if case['outs'] in ('both', 'dx') else None
    dres = out_guard((rows, Cc), dty, v['dres0'], (ld, 1), off('dres')) if case['outs'] in ('both', 'dres') else None
    null = case['dgamma_null']
    dgamma = out_guard((Cc,), 'float32', None if null else v['dg0'])
    dbeta = out_guard((Cc,), 'float32', None if null else v['db0'])
    partial = out_guard((nb, 2 * Cc), 'float32')
    hip.call('tell_layernorm_bwd', dy.t, ld, x.t, ld, t_(res), ld if has_res else 0, gamma.t, mean.t, rstd.t, t_(dx),
             ld if dx is not None else 0, t_(dres), ld if dres is not None else 0, case['dres_acc'], None if null else dgamma.t,
             None if null else dbeta.t, case['dparam_acc'], partial.t, rows, Cc, case['p'], ref.SEED, salt, code)
    intact(*(ins + [dy, mean, rstd, dx, dres, dgamma, dbeta, partial]))
    assert ref.same_bits(host(mean), mk) and ref.same_bits(host(rstd), rk)
    for k, g in (('dx', dx), ('dres', dres), ('partial', partial)):
        if g is not None:
            check(g, want[k], '%s %s' % (case['id'], k))
    if null:
        assert dgamma.untouched() and dbeta.untouched(), 'dgamma null: the parameter gradients are the caller\'s to fold'
    else:
        check(dgamma, want['dgamma'], '%s dgamma' % case['id'])
        check(dbeta, want['dbeta'], '%s dbeta' % case['id'])
    if case['outs'] == 'both' and not case['p'] and not case['dres_acc']:
        assert ref.same_bits(host(dx), host(dres)), 'p = 0: dx and dres are the same value'
    settle()


# ---------------------------------------------------------------- tell_layernorm_cat_fwd / tell_layernorm_cat_bwd
class Cat:
    """the guarded operands of one cat case; fresh outputs per launch"""

    def __init__(self, case):
        v = ref.cat_inputs(case)
        self.case, self.v, self.n, self.rows, self.Cc = case, v, case['n'], case['rows'], case['C']
        self.ld = self.n * self.Cc + case['pad_y']
        self.salts = ref.cat_salts(case)
        self.xs = [In(a, 'bfloat16') for a in v['xs']]
        self.res = In(v['res'], 'bfloat16')
        self.gammas, self.betas = [In(a, 'float32') for a in v['gammas']], [In(a, 'float32') for a in v['betas']]
        self.dcat = In(v['dcat'], 'bfloat16', (self.ld, 1))
        self.ins = self.xs + [self.res] + self.gammas + self.betas + [self.dcat]

    def forward(self, single=False):
        from tell_amd import hip
        from tell_amd.decode import _ptrs
        n, rows, Cc, case = self.n, self.rows, self.Cc, self.case
        y = out_guard((rows, n * Cc), 'bfloat16', None, (self.ld, 1))
        mean, rstd = out_guard((n, rows), 'float32'), out_guard((n, rows), 'float32')
        if single:
            for i in range(n):
                hip.call('tell_layernorm_fwd', self.xs[i].t, Cc, self.res.t, Cc, self.gammas[i].t, self.betas[i].t,
                         y.t[:, i * Cc:(i + 1) * Cc], self.ld, mean.t[i], rstd.t[i], rows, Cc, case['eps'], case['p'], ref.SEED,
                         self.salts[i], hip.dt(torch.bfloat16))
        else:
            hip.call('tell_layernorm_cat_fwd', n, _ptrs([a.t for a in self.xs]), Cc, self.res.t, Cc,
                     _ptrs([a.t for a in self.gammas]), _ptrs([a.t for a in self.betas]), y.t, self.ld, mean.t, rstd.t, rows, Cc,
                     case['eps'], case['p'], ref.SEED, u32s(self.salts), hip.dt(torch.bfloat16))
        intact(*(self.ins + [y, mean, rstd]))
        return y, mean, rstd

    def backward(self, mean, rstd, dx_null):
        """-> dxs (the guard of a null entry is made, and not passed), dres, dgammas, dbetas, partial"""
        from tell_amd import hip
        from tell_amd.decode import _ptrs
        n, rows, Cc, case, v = self.n, self.rows, self.Cc, self.case, self.v
        nb = -(-rows // 4)
        r = ref._rng('cat_prefill', case['id'])
        dxs = [out_guard((rows, Cc), 'bfloat16') for _ in range(n)]
        dres = out_guard((rows, Cc), 'bfloat16', ref.store(r.standard_normal((rows, Cc)), 'bfloat16'))
        null = case['dgamma_null']
        dgs = [out_guard((Cc,), 'float32', None if null else a) for a in v['dg0']]
        dbs = [out_guard((Cc,), 'float32', None if null else a) for a in v['db0']]
        partial = out_guard((n, nb, 2 * Cc), 'float32')
        hip.call('tell_layernorm_cat_bwd', n, self.dcat.t, self.ld, _ptrs([a.t for a in self.xs]), Cc, self.res.t, Cc,
                 _ptrs([a.t for a in self.gammas]), mean.t, rstd.t, _ptrs([None if i in dx_null else d.t for i, d in enumerate(dxs)]),
                 Cc, None if case['dres_null'] else dres.t, Cc, None if null else _ptrs([a.t for a in dgs]),
                 None if null else _ptrs([a.t for a in dbs]), partial.t, rows, Cc, case['p'], ref.SEED, u32s(self.salts),
                 hip.dt(torch.bfloat16))
        intact(*(self.ins + [mean, rstd, dres, partial] + dxs + dgs + dbs))
        return dxs, dres, dgs, dbs, partial


@pytest.mark.parametrize('case', ref.CAT, ids=ids(ref.CAT))
def test_layernorm_cat(case):
    """the forward against float64 and, bit for bit, against n single launches into the slices of an equally padded y; the
    backward on the stored statistics: dx_i (a null entry leaves its buffer untouched and changes nothing else), dres = sum_i
    dz_i over a prefill that must be gone, dgamma_i / dbeta_i accumulated onto a prefill, partial [n, blocks, 2C]"""
    t = Cat(case)
    n = t.n
    y, mean, rstd = t.forward()
    mk, rk = host(mean), host(rstd)
    want = ref.cat_case(case, stats=(mk, rk))
    for k, g in (('y', y), ('mean', mean), ('rstd', rstd)):
        check(g, want[k], '%s %s' % (case['id'], k))
    for a, b, k in zip(t.forward(single=True), (y, mean, rstd), ('y', 'mean', 'rstd')):
        assert ref.same_bits(host(a), host(b)), 'the cat forward is n single forwards: %s differs' % k
    dxs, dres, dgs, dbs, partial = t.backward(mean, rstd, case['dx_null'])
    assert ref.same_bits(host(mean), mk) and ref.same_bits(host(rstd), rk)
    for i in range(n):
        if i in case['dx_null']:
            assert dxs[i].untouched()
        else:
            check(dxs[i], want['dx%d' % i], '%s dx%d' % (case['id'], i))
        if case['dgamma_null']:
            assert dgs[i].untouched() and dbs[i].untouched()
        else:
            check(dgs[i], want['dgamma%d' % i], '%s dgamma%d' % (case['id'], i))
            check(dbs[i], want['dbeta%d' % i], '%s dbeta%d' % (case['id'], i))
    if case['dres_null']:
        assert ref.same_bits(host(dres), ref.store(ref._rng('cat_prefill', case['id']).standard_normal(dres.t.shape), 'bfloat16'))
    else:
        check(dres, want['dres'], '%s dres' % case['id'])
    check(partial, want['partial'], '%s partial' % case['id'])
    salts = t.salts
    for i in range(n):
        for j in range(i + 1, n):
            if salts[i] == salts[j] and case['p'] and not {i, j} & set(case['dx_null']):
                assert np.array_equal(host(dxs[i]) == 0, host(dxs[j]) == 0), 'equal salts, different masks'
    if case['dx_null']:
        full = t.backward(mean, rstd, ())
        for i in range(n):
            if i not in case['dx_null']:
                assert ref.same_bits(host(full[0][i]), host(dxs[i])), 'a null dx entry changed dx%d' % i
            assert ref.same_bits(host(full[2][i]), host(dgs[i])) and ref.same_bits(host(full[3][i]), host(dbs[i]))
        assert ref.same_bits(host(full[1]), host(dres)) and ref.same_bits(host(full[4]), host(partial))
    settle()


# ---------------------------------------------------------------- tell_layernorm_rows
@pytest.mark.parametrize('case', ref.ROWS, ids=ids(ref.ROWS))
def test_layernorm_rows(case):
    """fp32 rows to bf16 with padded leading dimensions; stats_out null changes no bit of y"""
    from tell_amd import hip
    v, M, Cc = ref.rows_inputs(case), case['M'], case['C']
    ld_x, ld_y = Cc + case['pad_x'], Cc + case['pad_y']
    x, gamma, beta = In(v['x'], 'float32', (ld_x, 1)), In(v['gamma'], 'float32'), In(v['beta'], 'float32')
    ys = {}
    for null in (case['stats_null'], not case['stats_null']):
        y = out_guard((M, Cc), 'bfloat16', None, (ld_y, 1))
        stats = None if null else out_guard((M, 2), 'float32')
        hip.call('tell_layernorm_rows', x.t, ld_x, gamma.t, beta.t, case['eps'], y.t, ld_y, t_(stats), M, Cc)
        intact(x, gamma, beta, y, stats)
        want = ref.rows_case(case, stats_null=null)
        check(y, want['y'], '%s y stats %s' % (case['id'], 'null' if null else 'given'))
        if stats is not None:
            check(stats, want['stats'], '%s stats' % case['id'])
        ys[null] = host(y)
    assert ref.same_bits(ys[True], ys[False]), 'stats_out null changes y'
    settle()


# ---------------------------------------------------------------- refusals and no-ops
def test_refused_calls_and_empty_launches_write_nothing():
    """rows = 0 is a no-op; p = 1, p < 0 and a backward with C = 2049 are refused; the cat entry points are refused with n = 0 /
    9, C = 256, fp32, ld_x % 8 != 0, an x[i] two bytes off, or a null res / y / dcat / mean / rstd (which ends on the host, before
    any launch); tell_layernorm_rows with C = 512 / 5120, ld_x % 4 != 0 or M = 0.  Every output stays untouched"""
    from tell_amd import hip
    from tell_amd.decode import _ptrs
    bf, f32 = hip.dt(torch.bfloat16), hip.dt(F32)
    rows, Cc = 3, 2049
    z = In(np.zeros((rows, Cc), np.float32), 'float32')
    g = In(np.ones(Cc, np.float32), 'float32')
    st = In(np.ones(rows, np.float32), 'float32')
    y, dx, dres = (out_guard((rows, Cc), 'float32') for _ in range(3))
    mean, rstd, dg, db = (out_guard((Cc,), 'float32') for _ in range(4))
    partial = out_guard((1, 2 * Cc), 'float32')

    def fwd(r_, C_, p):
        hip.call('tell_layernorm_fwd', z.t, Cc, z.t, Cc, g.t, g.t, y.t, Cc, mean.t, rstd.t, r_, C_, 1e-5, p, 1, 2, f32)

    def bwd(r_, C_, p):
        hip.call('tell_layernorm_bwd', z.t, Cc, z.t, Cc, z.t, Cc, g.t, st.t, st.t, dx.t, Cc, dres.t, Cc, 0, dg.t, db.t, 0, partial.t,
                 r_, C_, p, 1, 2, f32)
    fwd(0, 64, 0.0)
    bwd(0, 64, 0.0)
    for call, name in ((fwd, 'tell_layernorm_fwd'), (bwd, 'tell_layernorm_bwd')):
        for p in (1.0, -0.1):
            with pytest.raises(RuntimeError, match=name):
                call(rows, 64, p)
    with pytest.raises(RuntimeError, match='tell_layernorm_bwd'):
        bwd(rows, Cc, 0.0)

    n9, rc, Cq = 9, 2, 512
    xb = In(np.zeros((rc, Cq + 8), np.float32), 'bfloat16')
    xb_off = In(np.zeros((rc, Cq), np.float32), 'bfloat16', off=1)
    gq = In(np.ones(Cq, np.float32), 'float32')
    sq = In(np.ones((n9, rc), np.float32), 'float32')
    yc, dxc, drc = out_guard((rc, n9 * Cq), 'bfloat16'), out_guard((rc, Cq), 'bfloat16'), out_guard((rc, Cq), 'bfloat16')
    mc, rsc = out_guard((n9, rc), 'float32'), out_guard((n9, rc), 'float32')
    dgc, dbc, pc = out_guard((Cq,), 'float32'), out_guard((Cq,), 'float32'), out_guard((n9, 1, 2 * Cq), 'float32')
    salts = u32s(list(range(n9)))

    def cat_fwd(n=2, C_=Cq, dtype=bf, ld_x=Cq, x1=xb, r_=rc, res=xb, y_=yc, m_=mc, s_=rsc):
        hip.call('tell_layernorm_cat_fwd', n, _ptrs([xb.t, x1.t] + [xb.t] * 7), ld_x, t_(res), Cq, _ptrs([gq.t] * 9), _ptrs([gq.t] * 9),
                 t_(y_), n9 * Cq, t_(m_), t_(s_), r_, C_, 1e-5, 0.0, 1, salts, dtype)

    def cat_bwd(n=2, C_=Cq, dtype=bf, ld_x=Cq, x1=xb, r_=rc, res=xb, d_=xb, m_=sq, s_=sq):
        hip.call('tell_layernorm_cat_bwd', n, t_(d_), Cq + 8, _ptrs([xb.t, x1.t] + [xb.t] * 7), ld_x, t_(res), Cq, _ptrs([gq.t] * 9),
                 t_(m_), t_(s_), _ptrs([dxc.t] * 9), Cq, drc.t, Cq, _ptrs([dgc.t] * 9), _ptrs([dbc.t] * 9), pc.t, r_, C_, 0.0, 1,
                 salts, dtype)
    cat_fwd(r_=0)
    cat_bwd(r_=0)
    refused = [dict(n=0), dict(n=9), dict(C_=256), dict(dtype=f32), dict(ld_x=Cq + 4), dict(x1=xb_off), dict(res=None),
               dict(m_=None), dict(s_=None)]
    for kw in refused + [dict(y_=None)]:
        with pytest.raises(RuntimeError, match='tell_layernorm_cat_fwd'):
            cat_fwd(**kw)
    for kw in refused + [dict(d_=None)]:
        with pytest.raises(RuntimeError, match='tell_layernorm_cat_bwd'):
            cat_bwd(**kw)

    xr = In(np.zeros((2, 5120 + 2), np.float32), 'float32')
    gr = In(np.ones(5120, np.float32), 'float32')
    yr, sr_ = out_guard((2, 5120), 'bfloat16'), out_guard((2, 2), 'float32')
    for M, C_, ld_x in ((2, 512, 5120), (2, 5120, 5120), (2, 1024, 5122), (0, 1024, 5120)):
        with pytest.raises(RuntimeError, match='tell_layernorm_rows'):
            hip.call('tell_layernorm_rows', xr.t, ld_x, gr.t, gr.t, 1e-5, yr.t, 5120, sr_.t, M, C_)
    torch.cuda.synchronize()
    outs = (y, dx, dres, mean, rstd, dg, db, partial, yc, dxc, drc, mc, rsc, dgc, dbc, pc, yr, sr_)
    for i, o in enumerate(outs):
        assert o.untouched(), 'output %d was written by a refused or empty call' % i
    intact(z, g, st, xb, xb_off, gq, sq, xr, gr)
