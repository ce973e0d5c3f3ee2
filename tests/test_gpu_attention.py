"""The attention kernels (csrc/attention.hip: tell_attn_fwd, tell_attn_bwd, tell_attn_avg_weights) through the C ABI, element by
element against the float64 reference and the bounds of tests/attn_ref.py.  Every operand and every output
is a view inside a buffer of sentinels (tests/guarded.py): after each launch every guard band, row gap and foreign column is
intact, every read-only operand is bit for bit what was put in, and a refused call leaves its outputs untouched.  A backward
launch is fed the out / lse the forward launch itself stored, and its reference is computed from those; the forward holds out and
lse to float64.  Options go through hip.options(...), which restores them; no environment variable is read.
Run on the MI355X box:  python -m pytest tests/test_gpu_attention.py -m gpu -s   (-s prints the ratios c is pinned from, the paths
that were launched and the time of the whole file)"""
import time

import numpy as np
import pytest
import torch

import attn_ref as ref
from test_gpu_small_reduce import F32, TD, In, _gpu, host, intact, out_guard      # noqa: F401  (_gpu: the autouse fixture)

pytestmark = pytest.mark.gpu

_RATIOS, _UNPINNED, _TAKEN, _RAN = {}, {}, set(), set()
DEFAULTS = dict(attn_self=1, attn_dma=0, attn_occ=2, attn_tile64=0)      # set, not assumed: TELL_ATTN_* may have been loaded


@pytest.fixture(autouse=True)
def _fresh():
    _UNPINNED.clear()
    yield


@pytest.fixture(scope='module', autouse=True)
def _report():
    t0 = time.time()
    yield
    for k in sorted(_RATIOS):
        print('\nlargest (|got - ref| - u_out |ref| - derived) / (gamma 2^-24 S)  %-18s %.6f   c = %s' % (k, _RATIOS[k], ref.C.get(k)))
    print('\npaths taken (%d): %s' % (len(_TAKEN), ' '.join(sorted(_TAKEN))))
    print('\n%s: %.1f s' % (__name__, time.time() - t0))


def check(got, o, tag):
    """`got` (Guard, tensor or numpy) against the Out `o`: a measured group against its pinned constant - or, not pinned yet,
    recorded for settle(); the elements of exact_at for equality either way"""
    got = got if isinstance(got, np.ndarray) else host(got)
    assert got.shape == np.shape(o.value), tag
    rt = ref.ratio(got, o)
    _RATIOS[o.group] = max(_RATIOS.get(o.group, 0.0), rt)
    print('ratio %-18s %-40s %.6f' % (o.group, tag, rt))
    bad = ref.exact_failures(got, o)
    assert bad == 0, '%s %s: %d elements that must be exact are not' % (o.group, tag, bad)
    if o.group not in ref.C:
        _UNPINNED[o.group] = max(_UNPINNED.get(o.group, 0.0), rt)
        ex = np.zeros(got.shape, bool) if o.exact_at is None else np.broadcast_to(o.exact_at, got.shape)
        assert np.isfinite(got[~ex]).all(), tag
        return
    bad = ref.failures(got, o)
    assert bad == 0, '%s %s: %d of %d outside the bound (ratio %.4f, c = %g)' % (o.group, tag, bad, got.size, rt, ref.C[o.group])


def settle():
    """until c is pinned the test fails with the measured ratio in its message"""
    assert not _UNPINNED, 'constant not pinned yet, largest ratios of this case: %s' % \
        ', '.join('%s %.6f' % kv for kv in sorted(_UNPINNED.items()))


def ids(table):
    return [c['id'] for c in table]


def switches(case):
    """every attention option at a stated value for the block: the defaults, then what the case asks for"""
    from tell_amd import hip
    return hip.options(**dict(DEFAULTS, **(case['opts'] or {})))


def t_(g):
    return None if g is None else g.t


def h_(t):
    """a tensor (a view into a Guard) as fp32 numpy"""
    return t.float().cpu().numpy()


# ---------------------------------------------------------------- layouts
def strides(layout, B, H, n, D, who):
    """(row stride, batch stride) of an operand [n, B, E] in elements: dense [n, B, E]; batch-major storage [B, n, E] seen as
    [n, B, E]; K | V interleaved in one [S, B, 2E] buffer; q a column slice of [T, B, 3E]; out with 8 spare columns per row
    beside a sliced q"""
    E = H * D
    if layout == 'batch_major':
        return E, n * E
    if layout == 'q_slice' and who == 'q':
        return B * 3 * E, 3 * E
    if layout == 'q_slice' and who == 'o':
        return B * (E + 8), E + 8
    if layout == 'kv_packed' and who == 'kv':
        return B * 2 * E, 2 * E
    return B * E, E


def view4(st, sb, D):
    """Guard strides of the [B, H, n, D] view: element (b, h, t, d) at t st + b sb + h D + d"""
    return (sb, D, st, 1)


class Launch:
    """the guarded operands of one case in one layout; fresh outputs per launch"""

    def __init__(self, case, x=None, layout=None, salt=None):
        from tell_amd import hip
        self.case, self.x = case, x or ref.inputs(case)
        x, dty = self.x, case['dtype']
        B, H, Tq, S, D = case['B'], case['H'], case['Tq'], case['S'], case['D']
        self.B, self.H, self.Tq, self.S, self.D, self.dty, self.code = B, H, Tq, S, D, dty, hip.dt(TD[dty])
        self.layout = layout = layout or case['layout']
        self.salt = ref.salt_of('attn', case['id']) if salt is None else salt
        n = max(S, 1)                                 # S = 0: one row nobody reads, as the caller passes
        self.n = n
        self.q_st, self.q_sb = strides(layout, B, H, Tq, D, 'q')
        self.o_st, self.o_sb = strides(layout, B, H, Tq, D, 'o')
        self.k_ss, self.k_sb = strides(layout, B, H, n, D, 'kv')
        k = x['k'] if S else np.zeros((B, H, 1, D), np.float32)
        v = x['v'] if S else np.zeros((B, H, 1, D), np.float32)
        self.q = In(x['q'], dty, view4(self.q_st, self.q_sb, D))
        self.dout = In(x['dout'], dty, view4(self.o_st, self.o_sb, D))
        if layout == 'kv_packed':
            self.kv = In(np.stack([k, v]), dty, (H * D,) + view4(self.k_ss, self.k_sb, D))
            self.k_t, self.v_t, kv_ins = self.kv.t[0], self.kv.t[1], [self.kv]
        else:
            self.k, self.v = In(k, dty, view4(self.k_ss, self.k_sb, D)), In(v, dty, view4(self.k_ss, self.k_sb, D))
            self.k_t, self.v_t, kv_ins = self.k.t, self.v.t, [self.k, self.v]
        self.mask = None if x['mask'] is None else In(x['mask'], 'uint8')
        self.bk = None if x['bk'] is None else In(x['bk'], dty)
        self.bv = None if x['bv'] is None else In(x['bv'], dty)
        self.ins = [self.q, self.dout, self.mask, self.bk, self.bv] + kv_ins

    def forward(self, with_lse=True, p=None, salt=None):
        from tell_amd import hip
        c = self.case
        out = out_guard((self.B, self.H, self.Tq, self.D), self.dty, None, view4(self.o_st, self.o_sb, self.D))
        lse = out_guard((self.B * self.H, self.Tq), 'float32') if with_lse else None
        hip.call('tell_attn_fwd', self.q.t, self.k_t, self.v_t, out.t, t_(lse), t_(self.mask), t_(self.bk), t_(self.bv), self.B,
                 self.H, self.Tq, self.S, self.D, self.q_st, self.q_sb, self.k_ss, self.k_sb, self.k_ss, self.k_sb, self.o_st,
                 self.o_sb, int(c['zero']), c['p'] if p is None else p, ref.SEED, self.salt if salt is None else salt, self.code)
        intact(*(self.ins + [out, lse]))
        return out, lse

    def backward(self, out, lse):
        """-> dq, dk, dv (views), dbias_k, dbias_v (numpy or None), and every guard that was passed"""
        from tell_amd import hip
        c, B, H, D, n = self.case, self.B, self.H, self.D, self.n
        dq = out_guard((B, H, self.Tq, D), self.dty, None, view4(self.q_st, self.q_sb, D))
        if self.layout == 'kv_packed':
            dkv = out_guard((2, B, H, n, D), self.dty, None, (H * D,) + view4(self.k_ss, self.k_sb, D))
            dk_t, dv_t, g = dkv.t[0], dkv.t[1], [dkv]
        else:
            dk = out_guard((B, H, n, D), self.dty, None, view4(self.k_ss, self.k_sb, D))
            dv = out_guard((B, H, n, D), self.dty, None, view4(self.k_ss, self.k_sb, D))
            dk_t, dv_t, g = dk.t, dv.t, [dk, dv]
        gk = gv = None
        if c['bias'] and c['dbias'] == 'one':                   # the halves of one [B, 2 H D] buffer: dbias_v == dbias_k + H D
            both = out_guard((B, 2 * H * D), 'float32')
            gk, gv, g = both.t[:, :H * D], both.t[:, H * D:], g + [both]
            assert gv.data_ptr() == gk.data_ptr() + 4 * H * D
        elif c['bias']:
            one, two = out_guard((B, H * D), 'float32'), out_guard((B, H * D), 'float32')
            gk, gv, g = one.t, two.t, g + [one, two]
            assert gv.data_ptr() != gk.data_ptr() + 4 * H * D
        hip.call('tell_attn_bwd', self.q.t, self.k_t, self.v_t, out.t, self.dout.t, lse.t, t_(self.mask), t_(self.bk), t_(self.bv),
                 dq.t, dk_t, dv_t, gk, gv, B, H, self.Tq, self.S, D, self.q_st, self.q_sb, self.k_ss, self.k_sb, self.k_ss,
                 self.k_sb, self.o_st, self.o_sb, int(c['zero']), c['p'], ref.SEED, self.salt, self.code)
        intact(*(self.ins + [out, lse, dq] + g))
        if not self.S:
            assert all(x.untouched() for x in g[:2 if self.layout != 'kv_packed' else 1]), 'S = 0: dk / dv were written'
        res = dict(dq=host(dq), dk=h_(dk_t)[:, :, :self.S], dv=h_(dv_t)[:, :, :self.S])
        if c['bias']:
            res.update(dbias_k=h_(gk), dbias_v=h_(gv))
        return res


def lse3(lse, case):
    return host(lse).reshape(case['B'], case['H'], case['Tq'])


def forward_checks(case, run):
    """out and lse against float64; a second launch repeats the first bit for bit; a null lse changes no bit of out; a layout
    changes no bit either (the kernels' arithmetic depends on no address)"""
    out, lse = run.forward()
    want = ref.fwd_case(case)
    check(out, want['out'], '%s out' % case['id'])
    check(lse3(lse, case), want['lse'], '%s lse' % case['id'])
    again = run.forward()
    assert ref.same_bits(host(again[0]), host(out)) and ref.same_bits(host(again[1]), host(lse)), 'a second launch differs'
    assert ref.same_bits(host(run.forward(with_lse=False)[0]), host(out)), 'a null lse changes out'
    if case['layout'] != 'dense':
        dense = Launch(case, layout='dense').forward()
        assert ref.same_bits(host(dense[0]), host(out)) and ref.same_bits(host(dense[1]), host(lse)), \
            'layout %s: not the bits of the dense layout' % case['layout']
    return out, lse


DEFAULT = [c for c in ref.CASES if not c['opts']]
SWITCHED = [c for c in ref.CASES if c['opts']]


# ---------------------------------------------------------------- the default launch paths
@pytest.mark.parametrize('case', DEFAULT, ids=ids(DEFAULT))
def test_attention_forward_and_backward(case):
    """tell_attn_fwd as dispatched by default, then tell_attn_bwd on the stored out / lse: dq, dk, dv, dbias element-wise; rows
    without a live key are +0.0 / +inf and give exact zeros, masked keys have gradient +-0 (exact_at of the reference)"""
    run = Launch(case)
    _RAN.add(case['id'])
    _TAKEN.add(ref.fwd_path(case))
    with switches(case):
        out, lse = forward_checks(case, run)
    if case['bwd']:
        _TAKEN.add(ref.bwd_path(case))
        ok, lk = host(out), lse3(lse, case)
        want = ref.attn_bwd(case, ok, lk)
        got = run.backward(out, lse)
        assert ref.same_bits(host(out), ok) and ref.same_bits(lse3(lse, case), lk)
        for k in sorted(got):
            check(got[k], want[k], '%s %s' % (case['id'], k))
        again = run.backward(out, lse)
        for k in sorted(got):
            assert ref.same_bits(again[k], got[k]), 'a second backward launch differs in %s' % k
        if case['layout'] != 'dense':
            d = Launch(case, layout='dense')
            with switches(case):
                od, ld = d.forward()
            dense = d.backward(od, ld)
            for k in sorted(got):
                assert ref.same_bits(dense[k], got[k]), 'layout %s: %s is not the dense layout\'s' % (case['layout'], k)
    settle()


# ---------------------------------------------------------------- dropout decisions, element by element
def _onehot(kern_case):
    """inputs with V the identity on the (at most 64) keys: out IS the dropped probability row"""
    c = kern_case
    r = ref._rng('onehot', c['id'])
    B, H, Tq, S, D = c['B'], c['H'], c['Tq'], c['S'], c['D']
    St = ref.sizes(c)[0]
    assert St <= 64 and D == 64
    eye = np.eye(64, dtype=np.float32)
    x = dict(q=ref.store(r.standard_normal((B, H, Tq, D)) * 0.2, c['dtype']), k=ref.store(r.standard_normal((B, H, S, D)), c['dtype']),
             v=np.broadcast_to(eye[:S], (B, H, S, D)).copy(), dout=np.zeros((B, H, Tq, D), np.float32), mask=None,
             bk=ref.store(r.standard_normal((H, D)), c['dtype']) if c['bias'] else None,
             bv=np.broadcast_to(eye[S], (H, D)).copy() if c['bias'] else None)
    return x


ONEHOT = [ref._c('oh_%s' % name, dt, Tq, S, p=0.5, opts=opts, **kw) for name, dt, Tq, S, opts, kw in (
    ('fwd_ksplit_pair', 'bf16', 20, 64, None, {}), ('fwd_qblocks_pair', 'bf16', 40, 62, None, {}),
    ('fwd_single', 'bf16', 40, 62, None, dict(bias=True)), ('fwd_f32_pair', 'f32', 40, 61, None, dict(bias=True)),
    ('reg_quad', 'bf16', 100, 64, dict(attn_self=0), {}), ('reg_pair', 'bf16', 100, 61, None, dict(bias=True)),
    ('reg_single', 'bf16', 100, 62, None, dict(zero=True)), ('self_quad', 'bf16', 100, 64, None, {}),
    ('tile64_f32_pair', 'f32', 100, 64, None, {}), ('tile64_f32_single', 'f32', 130, 63, None, {}),
    ('tile64_bf16_pair', 'bf16', 100, 62, dict(attn_tile64=1), {}))]


@pytest.mark.parametrize('case', ONEHOT, ids=ids(ONEHOT))
def test_dropout_keeps_exactly_the_reference_elements(case):
    """p = 0.5 and V = I: the zeros of out are the dropped probabilities, element by element those of rng.keep_mask at index
    ((b H + h) Tq + t) S_total + s - on every forward kernel and all three walks; equal salts give one mask, different salts
    different ones.  (The zero key's value is 0: its column shows nothing and is left out.)"""
    from tell_amd import hip
    want_walk = {'quad': 'quad', 'pair': 'pair', 'single': 'single'}[case['id'].rsplit('_', 1)[1]]
    assert ref.fwd_path(case).endswith(want_walk), ref.fwd_path(case)
    x = _onehot(case)
    run = Launch(case, x)
    salts = (ref.salt_of('oh', case['id'], 0), ref.salt_of('oh', case['id'], 1))
    zeros = []
    with switches(case):
        for salt in salts + salts[:1]:
            out, _ = run.forward(salt=salt)
            n = case['S'] + int(case['bias'])            # the keys with a one-hot value
            got = host(out)[..., :n]
            keep = ref.keep_of(case, salt)[..., :n]
            assert (keep == 0).any() and (keep == 1).any()
            wrong = (got == 0) != (keep == 0)
            assert not wrong.any(), '%d of %d keep decisions differ from rng.keep_mask (first at %s)' % (
                wrong.sum(), wrong.size, np.argwhere(wrong)[0])
            assert not host(out)[..., n:].any()
            zeros.append(got == 0)
    assert np.array_equal(zeros[0], zeros[2]), 'equal salts, different masks'
    assert not np.array_equal(zeros[0], zeros[1]), 'different salts, one mask'


# ---------------------------------------------------------------- tell_attn_avg_weights
@pytest.mark.parametrize('case', ref.AVG, ids=ids(ref.AVG))
def test_average_weights(case):
    """w [B, Tq, S_total] fp32 from the lse the forward launch stored; a masked key's column is +0"""
    from tell_amd import hip
    run = Launch(case)
    with switches(case):
        out, lse = run.forward()
    St = ref.sizes(case)[0]
    ws = []
    for _ in range(2):
        w = out_guard((case['B'], case['Tq'], St), 'float32')
        hip.call('tell_attn_avg_weights', run.q.t, run.k_t, lse.t, t_(run.mask), t_(run.bk), w.t, run.B, run.H, run.Tq, run.S, run.D,
                 run.q_st, run.q_sb, run.k_ss, run.k_sb, int(case['zero']), run.code)
        intact(*(run.ins + [lse, w]))
        ws.append(host(w))
    check(ws[0], ref.avg_weights(case, lse3(lse, case)), '%s w' % case['id'])
    assert ref.same_bits(ws[0], ws[1]), 'a second launch differs'
    settle()


# ---------------------------------------------------------------- the switches attn_dma, attn_occ, attn_tile64
@pytest.mark.parametrize('case', SWITCHED, ids=ids(SWITCHED))
def test_attention_switches(case):
    """attn_self = 0 names the reg kernel on a self-kernel shape; attn_dma = 1 equals the default self kernel bit for bit, attn_occ
    = 3 equals attn_occ = 2 bit for bit (out and lse, with and without dropout); attn_tile64 = 1 (bf16) is held to its own bounds"""
    from tell_amd import hip
    run = Launch(case)
    opts = case['opts']
    _RAN.add(case['id'])
    with switches(case):
        _TAKEN.add(ref.fwd_path(case))
        out, lse = forward_checks(case, run)
        other_p = 0.0 if case['p'] else 0.1
        flipped = run.forward(p=other_p)
    base = {k: v for k, v in opts.items() if k == 'attn_self'}
    if opts.get('attn_dma') == 1 or opts.get('attn_occ') == 3:
        with hip.options(**dict(DEFAULTS, **base)):
            plain = run.forward()
            plain_flipped = run.forward(p=other_p)
        for a, b, what in ((plain, (out, lse), 'p = %g' % case['p']), (plain_flipped, flipped, 'p = %g' % other_p)):
            assert ref.same_bits(host(a[0]), host(b[0])), '%s changes out (%s)' % (opts, what)
            assert ref.same_bits(host(a[1]), host(b[1])), '%s changes lse (%s)' % (opts, what)
    settle()


# ---------------------------------------------------------------- refusals
def test_refused_calls_write_nothing():
    """D = 32, p = 1, p < 0, no keys at all, bias_k without bias_v, q_st % 8 != 0 (bf16), q / out / dout two bytes off, a null out,
    an out stride that is no multiple of the 16-byte chunk, a backward with bias rows but no dbias buffers or with a null dq / dk / dv /
    out / dout / lse: TELL_ERR_ARG on the host, before any launch, every output untouched"""
    from tell_amd import hip
    bf = hip.dt(torch.bfloat16)
    B, H, Tq, S, D = 1, 1, 4, 4, 64
    E = H * D
    z = lambda rows, off=0, ld=E: In(np.zeros((rows, E), np.float32), 'bfloat16', (ld, 1), off)     # noqa: E731
    q, k, v, do, o_in = z(Tq), z(S), z(S), z(Tq), z(Tq)
    q_off, do_off, q_ld = z(Tq, 1), z(Tq, 1), z(Tq, 0, E + 4)
    bias = In(np.zeros(E, np.float32), 'bfloat16')
    lse_in = In(np.zeros((B * H, Tq), np.float32), 'float32')
    out, out_off, out_ld = out_guard((Tq, E), 'bfloat16'), out_guard((Tq, E), 'bfloat16', None, None, 1), \
        out_guard((Tq, E), 'bfloat16', None, (E + 4, 1))
    lse = out_guard((B * H, Tq), 'float32')
    dq, dk, dv = out_guard((Tq, E), 'bfloat16'), out_guard((S, E), 'bfloat16'), out_guard((S, E), 'bfloat16')
    gk, gv = out_guard((B, E), 'float32'), out_guard((B, E), 'float32')

    def fwd(q_=q, o_=out, D_=D, S_=S, p=0.0, bk=None, bv=None, zero=0, q_st=E, o_st=E):
        hip.call('tell_attn_fwd', q_.t, k.t, v.t, t_(o_), lse.t, None, t_(bk), t_(bv), B, H, Tq, S_, D_, q_st, q_st, E, E, E, E, o_st,
                 o_st, zero, p, 1, 2, bf)

    def bwd(bk=None, gk_=None, gv_=None, o_=o_in, do_=do, l_=lse_in, dq_=dq, dk_=dk, dv_=dv):
        hip.call('tell_attn_bwd', q.t, k.t, v.t, t_(o_), t_(do_), t_(l_), None, t_(bk), t_(bk), t_(dq_), t_(dk_), t_(dv_), t_(gk_),
                 t_(gv_), B, H, Tq, S, D, E, E, E, E, E, E, E, E, 0, 0.0, 1, 2, bf)

    refused_fwd = [dict(D_=32), dict(p=1.0), dict(p=-0.1), dict(S_=0), dict(bk=bias), dict(q_=q_ld, q_st=E + 4), dict(q_=q_off),
                   dict(o_=out_off), dict(o_=out_ld, o_st=E + 4), dict(o_=None)]
    for kw in refused_fwd:
        with pytest.raises(RuntimeError, match='tell_attn_fwd'):
            fwd(**kw)
    refused_bwd = [dict(bk=bias), dict(bk=bias, gk_=gk), dict(do_=do_off), dict(o_=None), dict(do_=None), dict(l_=None), dict(dq_=None),
                   dict(dk_=None), dict(dv_=None)]
    for kw in refused_bwd:
        with pytest.raises(RuntimeError, match='tell_attn_bwd'):
            bwd(**kw)
    torch.cuda.synchronize()
    for i, g in enumerate((out, out_off, out_ld, lse, dq, dk, dv, gk, gv)):
        assert g.untouched(), 'output %d was written by a refused call' % i
    intact(q, k, v, do, o_in, q_off, do_off, q_ld, bias, lse_in)


def test_every_path_of_the_tables_is_launched():
    """every case of the table is a parameter of a launching test above (whatever was selected in this run), and what was launched
    in this process carries the names fwd_path / bwd_path give for it; with the whole file run that is every name of the tables.
    (The names are the launchers' conditions restated with every option SET for the launch; the library has no query for the
    kernel it launched.)"""
    assert sorted(ids(DEFAULT) + ids(SWITCHED)) == sorted(ids(ref.CASES))
    ran = [c for c in ref.CASES if c['id'] in _RAN]
    named = {ref.fwd_path(c) for c in ran} | {ref.bwd_path(c) for c in ran if c['bwd']}
    assert named == _TAKEN, sorted(named ^ _TAKEN)
    if len(ran) == len(ref.CASES):
        every = {ref.fwd_path(c) for c in ref.CASES} | {ref.bwd_path(c) for c in ref.CASES if c['bwd']}
        assert every == _TAKEN, sorted(every ^ _TAKEN)
