"""The GEMM family (csrc/gemm.hip, gemm_pp2.hip, gemm_q4.hip, gemm_q4e.hip, gemm_s64.hip, gemm_epi.h) through the C ABI,
every launch path of tell_gemm_nt / tell_gemm_bf16 / tell_gemm_grouped / tell_splitk_reduce2 and
tell_gemm_nt_dropout_residual with integer-valued operands: every output must equal the float64 product of
tests/gemm_ref.py BIT FOR BIT; GELU is the one epilogue with a bound.  Every output is a view with
ldc > N inside a buffer of sentinels, the operands too, so a store or a row stride that is off shows without anything
running out of range.  Before every tell_gemm_nt launch the plan label is asserted, so a case cannot drift off its path.
Run on the MI355X box:  python -m pytest tests/test_gpu_gemm.py -m gpu   (-s prints the GELU ratios c is pinned from)"""
import pytest
import torch

import gemm_ref as ref
from guarded import DEV, SENTINEL, Vec, View          # the guarded views, shared with tests/test_gpu_copy.py

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
assert SENTINEL == ref.SENTINEL

_GELU = {}


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                  # a device fault: every later launch of this process would fail the same way
        pytest.exit('GPU error, nothing more is launched: %s' % err, 3)


@pytest.fixture(scope='module', autouse=True)
def _report_gelu():
    yield
    for k in sorted(_GELU):
        print('\nlargest (|got - ref| - u_out |ref|) / (2^-24 max(1, |x|))  %-40s %.4f' % (k, _GELU[k]))
    if _GELU:
        print('\nGELU: largest ratio over all cases %.4f, c = %s' % (max(_GELU.values()), ref.GELU_C))


def n_cu():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    if n % 16:
        pytest.skip('the whole-round shapes are built for a CU count that is a multiple of 16, this device has %d' % n)
    return n


def r8(n):
    return (n + 7) // 8 * 8


def exact(got, want, tag):
    msg = ref.mismatch(got, want.to(DEV))
    assert msg is None, '%s: %s' % (tag, msg)


def gelu_check(got, want, x, out_dtype, tag):
    got = got.cpu()
    assert bool(torch.isfinite(got).all()), tag
    r = ref.gelu_ratio(got, want, x, out_dtype)
    _GELU[tag] = max(_GELU.get(tag, 0.0), r)
    print('gelu ratio %-50s %.4f' % (tag, r))
    assert ref.GELU_C is not None, 'GELU constant not pinned yet (largest ratio of this case: %.4f)' % r
    assert r <= ref.GELU_C, '%s: ratio %.4f above c = %g' % (tag, r, ref.GELU_C)


_DEV = {}


def cached(key, make):
    if key not in _DEV:
        _DEV[key] = make()
    return _DEV[key]


def side_dev(M, N, out_dtype, seed=0):
    side = cached(('side', M, N, out_dtype, seed), lambda: ref.side_inputs(M, N, out_dtype, seed))
    bn = cached(('bn', M, N, out_dtype, seed), lambda: Vec(side['bias_n']))
    bm = cached(('bm', M, N, out_dtype, seed), lambda: Vec(side['bias_m']))
    return side, bn, bm


def mdev_tensor(v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------- tell_gemm_nt: the case table
@pytest.mark.parametrize('case', ref.CASES, ids=[c['id'] for c in ref.CASES])
def test_gemm_nt_paths(case):
    from tell_amd import hip
    M, N, K = ref.case_shape(case, n_cu())
    din, dout = case['in_dtype'], case['out_dtype']
    A, B, amp = ref.operands(M, N, K, din, case['seed'], wide=case['wide'])
    key = (M, N, K, din, case['seed'], case['wide'])
    acc = ref.product(A, B, key)
    side, bn, bm = side_dev(M, N, dout)
    lda, ldb, ldc, off = K + case['lda_pad'], K + case['ldb_pad'], N + case['ldc_pad'], case['c_off']
    Ad = cached(('A',) + key + (lda,), lambda: View(M, K, lda, din, 0, A))
    Bd = cached(('B',) + key + (ldb,), lambda: View(N, K, ldb, din, 0, B))
    At, Bt = Ad.t, Bd.t
    aux = cached(('aux', M, N, dout, ldc, off), lambda: View(M, N, ldc, dout, off, side['aux']))
    for name, e in case['epis']:
        e = ref.resolve(e, M)
        if e['act'] == 2:
            e['alpha'] = ref.case_gelu_alpha(case, n_cu())
        tag = '%s %dx%dx%d %s' % (case['id'], M, N, K, name)
        if not case['wide']:
            assert ref.intermediate_bound(K, amp, e) < ref.LIMIT
        C = View(M, N, ldc, dout, off, side['prev'])
        md = mdev_tensor(e['m_dev'])
        bias = {0: None, 1: bn.t, 2: bm.t}[e['bias_mode']]
        args = (At, lda, Bt, ldb, C.t, ldc, M, N, K, hip.dt(din), hip.dt(dout), bias, e['bias_mode'], e['act'],
                aux.t if e['act'] in (3, 4) else None, float(e['alpha']), int(e['accumulate']), md)
        with hip.options(**case['opts']):
            assert hip.query('tell_gemm_nt_plan', *args) == case['plan'], tag
            hip.call('tell_gemm_nt', *args)
        torch.cuda.synchronize()
        assert C.intact() and aux.intact() and bn.intact() and bm.intact(), tag + ': store outside the view'
        assert Ad.intact() and Bd.intact(), tag
        want = ref.expected(acc, dout, e, side, side['prev'], ref.LIMIT_WIDE if case['wide'] else ref.LIMIT)
        if e['act'] == 2:
            gelu_check(C.t, want[0], want[1], dout, tag)
        else:
            exact(C.t, want, tag)


def test_options_are_read_per_launch():
    """one process, one shape, three kernels: the plan label follows hip.options from launch to launch"""
    from tell_amd import hip
    n = n_cu()
    M, N, K = 4096, 16 * n, 128
    A, B, _ = ref.operands(M, N, K)
    Ad, Bd = View(M, K, K + 8, BF16, 0, A), View(N, K, K, BF16, 0, B)
    C = View(M, N, N + 8, BF16)
    args = (Ad.t, K + 8, Bd.t, K, C.t, N + 8, M, N, K, hip.BF16, hip.BF16, None, 0, 0, None, 1.0, 0, None)
    want = ref.expected(ref.product(A, B, (M, N, K, BF16, 0, False)), BF16, ref.epi(), None)
    for opts, label in (({}, ref.Q4[0]), (ref.NO_Q4, ref.PP2[0]), (ref.NO_PP2, ref.PP[0]), ({}, ref.Q4[0])):
        with hip.options(**opts):
            assert hip.query('tell_gemm_nt_plan', *args) == label
            hip.call('tell_gemm_nt', *args)
        torch.cuda.synchronize()
        assert Ad.intact() and Bd.intact() and C.intact()
        exact(C.t, want, label)
        C.t.fill_(SENTINEL)


# ---------------------------------------------------------------- tell_gemm_nt_dropout_residual
@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('shape', [(4096, 4096, 64), (8192, 4096, 192), (4096, 4096, 128)], ids=str)
def test_dropout_residual(shape, p):
    """res + bf16((lin + bias) * keep * 2) at p = 0.5 (the fp32 factor 1 / (1 - p) is exactly 2) and p = 0, strided res and
    out, on the ping-pong kernel (K = 64, 192) and on the four-wave kernel (K = 128: one rounding); the decline codes"""
    from tell_amd import hip, rng
    M, N, K = shape
    N = N * n_cu() // 256
    A, B, _ = ref.operands(M, N, K)
    acc = ref.product(A, B, (M, N, K, BF16, 0, False))
    side, bn, _ = side_dev(M, N, BF16)
    Ad = cached(('A', M, N, K, BF16, 0, False, K + 8), lambda: View(M, K, K + 8, BF16, 0, A))
    Bd = cached(('B', M, N, K, BF16, 0, False, K), lambda: View(N, K, K, BF16, 0, B))
    res = View(M, N, N + 16, BF16, 0, side['res'])
    C = View(M, N, N + 8, BF16)
    assert hip.call_rc('tell_gemm_nt_dropout_residual', Ad.t, K + 8, Bd.t, K, bn.t, res.t, N + 16, C.t, N + 8, M, N, K, p, 17,
                       23) == 0
    torch.cuda.synchronize()
    assert C.intact() and res.intact() and bn.intact() and Ad.intact() and Bd.intact()
    keep = torch.from_numpy(rng.keep_mask(17, 23, M * N, p)).view(M, N) if p > 0 else None
    roundings = 1 if K % 128 == 0 else 2          # K % 128 == 0 runs on the four-wave kernel, which rounds once
    exact(C.t, ref.expected_dropout_residual(acc, side['bias_n'], side['res'], keep, p, roundings),
          'dropout residual %s p=%g' % (shape, p))
    if p > 0:
        assert 0.49 < float((keep == 0).float().mean()) < 0.51
    # shapes it declines: ragged rows, fewer tiles than CUs, a row stride that is no multiple of 8
    before = C.buf.clone()
    for m, ldc in ((M - 8, N + 8), (256, N + 8), (M, N + 4)):
        assert hip.call_rc('tell_gemm_nt_dropout_residual', Ad.t, K + 8, Bd.t, K, bn.t, res.t, N + 16, C.t, ldc, m, N, K, p, 17,
                           23) == 1
    torch.cuda.synchronize()
    assert torch.equal(C.buf, before)


# ---------------------------------------------------------------- tell_gemm_bf16: the K-major forms
class Problem:
    """one product of tell_gemm_bf16 / tell_gemm_grouped (form 'nt', 'nn': B stored [K, N], 'tn': A stored [K, M] as well,
    'ta': A stored [K, M] and B row-major - tell_gemm_bf16 only): operands laid out for the form inside guarded views, the output
    a guarded view preset to the previous C, and the exact expectation"""

    def __init__(self, M, N, K, form, dout=BF16, accumulate=False, alpha=1.0, bias=False, act=0, asum=None, lim=None,
                 seed=0, how='float64'):
        self.M, self.N, self.K, self.form, self.dout = M, N, K, form, dout
        self.tag = '%s %dx%dx%d %s%s%s' % (form, M, N, K, str(dout).split('.')[-1], ' acc' if accumulate else '',
                                          '' if lim is None else ' lim=%d' % lim)
        A, B, amp = ref.operands(M, N, K, BF16, seed)
        self.e = ref.epi(bias_mode=int(bias), act=act, alpha=alpha, accumulate=accumulate,
                         m_dev=None if form == 'tn' else lim)
        assert ref.intermediate_bound(K, amp, self.e) < ref.LIMIT
        k_lim = min(lim, K) if (form == 'tn' and lim is not None) else K
        self.side, self.bn, _ = side_dev(M, N, dout, seed)
        acc = ref.product(A[:, :k_lim], B[:, :k_lim], how=how) if k_lim else torch.zeros(M, N, dtype=torch.float64)
        self.want = ref.expected(acc, dout, self.e, self.side, self.side['prev'])
        k8 = r8(K)
        if form in ('tn', 'ta'):                               # A stored [K, M]
            self.A = View(K, M, r8(M) + 8, BF16, 0, A.t())
        else:                                                  # row-major, zero padded to a whole 8-element chunk
            a = torch.zeros(M, k8, dtype=BF16)
            a[:, :K] = A
            self.A = View(M, k8, k8 + 8, BF16, 0, a)
        if form in ('nt', 'ta'):
            b = torch.zeros(N, k8, dtype=BF16)
            b[:, :K] = B
            self.B = View(N, k8, k8 + 8, BF16, 0, b)
        else:                                                  # B stored [K, N]
            self.B = View(K, N, r8(N) + 8, BF16, 0, B.t())
        self.C = View(M, N, N + 8, dout, 0, self.side['prev'])
        self.lim = mdev_tensor(lim)
        self.asum = self.asum_scale = self.asum_want = None
        if asum is not None:
            preset = torch.arange(M, dtype=F32) - 3.0
            self.asum, self.asum_scale = Vec(preset), asum
            self.asum_want = ref.expected_asum(A, asum, preset, k_lim)

    def struct(self, q):
        q.A, q.lda, q.B, q.ldb, q.C, q.ldc = self.A.t.data_ptr(), self.A.ld, self.B.t.data_ptr(), self.B.ld, \
            self.C.t.data_ptr(), self.C.ld
        q.M, q.N, q.K = self.M, self.N, self.K
        q.trans_a, q.trans_b = int(self.form == 'tn'), int(self.form in ('tn', 'nn'))
        q.out_dtype, q.accumulate, q.alpha = int(self.dout == BF16), int(self.e['accumulate']), float(self.e['alpha'])
        q.bias, q.bias_mode, q.act = (self.bn.t.data_ptr() if self.e['bias_mode'] else None), self.e['bias_mode'], self.e['act']
        q.asum = self.asum.t.data_ptr() if self.asum is not None else None
        q.asum_scale = float(self.asum_scale or 0.0)
        q.lim_dev = self.lim.data_ptr() if self.lim is not None else None

    def single(self):
        """through tell_gemm_bf16"""
        from tell_amd import hip
        assert self.form != 'tn' or self.lim is None
        hip.call('tell_gemm_bf16', self.A.t, self.A.ld, int(self.form in ('tn', 'ta')), self.B.t, self.B.ld,
                 int(self.form in ('tn', 'nn')), self.C.t, self.C.ld, self.M, self.N, self.K, hip.dt(self.dout),
                 self.bn.t if self.e['bias_mode'] else None, self.e['bias_mode'], self.e['act'], None, float(self.e['alpha']),
                 int(self.e['accumulate']), self.lim, self.asum.t if self.asum is not None else None,
                 float(self.asum_scale or 0.0))

    def check(self):
        assert self.A.intact() and self.B.intact() and self.C.intact() and self.bn.intact(), self.tag + ': store outside'
        exact(self.C.t, self.want, self.tag)
        if self.asum is not None:
            assert self.asum.intact(), self.tag
            exact(self.asum.t, self.asum_want, self.tag + ' asum')


def grouped(problems, **opts):
    from tell_amd import hip, ops
    arr = (ops._GemmProblem * len(problems))()
    for q, p in zip(arr, problems):
        p.struct(q)
    with hip.options(**opts):
        hip.call('tell_gemm_grouped', len(problems), arr)
    torch.cuda.synchronize()
    for p in problems:
        p.check()


KMAJOR = [(64, 64, 64), (96, 200, 72), (2, 1024, 300), (200, 70, 130), (2048, 2048, 64)]


@pytest.mark.parametrize('shape', KMAJOR, ids=str)
def test_gemm_bf16_kmajor_forms(shape):
    """TN, NN and K-major A with row-major B in place on K-major operands (64 x 64 tiles, 128 x 128 from 256 of them): both output types, the fused
    column sums with a scale and a preset value, accumulate with alpha, m_dev; K % 8 != 0 with the documented padding"""
    M, N, K = shape
    ps = [Problem(M, N, K, 'tn', F32, accumulate=True, alpha=0.5, asum=0.5),
          Problem(M, N, K, 'tn', BF16),
          Problem(M, N, K, 'tn', BF16, accumulate=True, alpha=2.0, asum=1.0),
          Problem(M, N, K, 'ta', BF16),                            # A K-major, B row-major: tell_gemm_bf16 only
          Problem(M, N, K, 'ta', F32, accumulate=True, alpha=0.5, asum=0.5),
          Problem(M, N, K, 'nn', BF16),
          Problem(M, N, K, 'nn', F32, accumulate=True, alpha=0.5),
          Problem(M, N, K, 'nn', BF16, lim=M // 2),
          Problem(M, N, K, 'nn', F32, lim=1),
          Problem(M, N, K, 'nn', BF16, lim=0)]
    for p in ps:
        p.single()
    torch.cuda.synchronize()
    for p in ps:
        p.check()


@pytest.mark.parametrize('splits', [2, 3])
@pytest.mark.parametrize('shape', [(256, 256, 4096), (250, 130, 4096)], ids=str)
def test_gemm_bf16_atomic_split_k(shape, splits):
    """gemm_splitk > 0: an accumulating fp32 TN product split over gridDim.y, partial tiles added with float atomics -
    exact here whatever the order"""
    from tell_amd import hip
    M, N, K = shape
    ps = [Problem(M, N, K, 'tn', F32, accumulate=True, alpha=0.5), Problem(M, N, K, 'tn', F32, accumulate=True, seed=1)]
    with hip.options(gemm_splitk=splits):
        for p in ps:
            p.single()
    torch.cuda.synchronize()
    for p in ps:
        p.check()


# ---------------------------------------------------------------- tell_gemm_grouped
FORMS = ('nt', 'nn', 'tn')


def _all_forms(M, N, K, seed=0):
    return [Problem(M, N, K, f, d, seed=seed + i) for i, (f, d) in enumerate((f, d) for f in FORMS for d in (BF16, F32))]


@pytest.mark.parametrize('tile', [64, 128, 0])
def test_grouped_every_form_and_tile(tile):
    """one call: three forms x both output types x small and big problems.  group_tile 64 / 128 force a tile, 0 is the
    rule (128 x 128 from 512 big tiles per form and type)"""
    big = (2040, 4090, 64) if tile == 0 else (250, 136, 64)
    ps = _all_forms(96, 200, 64) + _all_forms(*big, seed=10)
    ps += [Problem(130, 70, 64, 'nt', BF16, bias=True, act=1, seed=20), Problem(130, 70, 64, 'tn', F32, accumulate=True,
                                                                                alpha=0.5, asum=0.5, seed=21),
           Problem(96, 200, 72, 'nt', BF16, seed=22)]                    # K % 64 != 0: falls through to the dispatcher
    grouped(ps, group_tile=tile)


@pytest.mark.parametrize('wide', [1, 0])
@pytest.mark.parametrize('lim', [None, 0, 1, 37, 4096])
def test_grouped_wide_bucket(wide, lim):
    """fp32 TN with K >= 4096, M >= 256: the 256 x 128 tile kernel and its group_wide = 0 twin, with and without a
    device-side reduction length"""
    ps = [Problem(256, 128, 4096, 'tn', F32, accumulate=True, alpha=0.5, lim=lim),
          Problem(300, 130, 4096, 'tn', F32, accumulate=True, lim=lim, seed=1)]
    if lim is None:
        ps.append(Problem(256, 136, 4096, 'tn', F32, asum=0.5, seed=2))
    grouped(ps, group_wide=wide)


@pytest.mark.parametrize('lim', [0, 1, 37, 96])
def test_grouped_lim_dev(lim):
    """lim_dev in both senses: the row limit of nt / nn (rows past it untouched), the reduction limit of an accumulating tn
    (rows past it of both operands not read: they hold data that must not arrive)"""
    ps = [Problem(96, 200, 64, 'nt', BF16, lim=lim), Problem(96, 200, 64, 'nt', F32, bias=True, act=1, lim=lim, seed=1),
          Problem(96, 200, 72, 'nn', BF16, lim=lim, seed=2), Problem(96, 72, 130, 'nn', F32, lim=lim, seed=3),
          Problem(70, 200, 96, 'tn', F32, accumulate=True, lim=lim, seed=4),
          Problem(70, 200, 96, 'tn', BF16, accumulate=True, alpha=0.5, lim=lim, seed=5)]
    grouped(ps)


@pytest.mark.parametrize('sort', [1, 0])
def test_grouped_fifty_problems(sort):
    """more than 2 x GROUP_MAX problems in one call, reductions of different lengths (group_sort orders them)"""
    ps = []
    for i in range(50):
        f = FORMS[i % 3]
        ps.append(Problem(70 + 8 * (i % 4), 72, 64 * (1 + i % 3), f, F32 if i % 2 else BF16, accumulate=(f == 'tn'), seed=100 + i))
    grouped(ps, group_sort=sort)


def test_grouped_ring_4_kernels():
    """nt buckets of at most 512 tiles of 64 x 64 with K >= 512: the four-stage group kernels"""
    grouped([Problem(128, 128, 512, 'nt', BF16), Problem(96, 200, 576, 'nt', BF16, bias=True, act=1, seed=1),
             Problem(128, 128, 512, 'nt', F32, seed=2), Problem(70, 72, 512, 'nt', F32, accumulate=True, seed=3)])


# ---------------------------------------------------------------- tell_splitk_reduce2
def _partials(splits, M, N, amp, seed=0):
    g = torch.Generator().manual_seed(seed * 1000 + splits + M + N)
    return torch.randint(-amp, amp + 1, (splits, M, N), generator=g).float()


@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('dout', [BF16, F32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('splits,M,N', [(1, 7, 64), (3, 37, 72), (8, 130, 1024), (3, 1030, 2052)], ids=str)
def test_splitk_reduce_direct(splits, M, N, act, dout):
    """out = act((sum_s partial_s + bias) * alpha) with a strided out and m_dev; the last shape has more quads than the
    2048 x 256 threads of the largest grid (grid-stride loop)"""
    from tell_amd import hip
    # GELU: |sum| <= 24 and |bias| <= 4 times alpha 0.25 keep the pre-activations inside [-7, 7], where erf is at work
    amp = 24 // splits if act == 2 else 100000
    part = _partials(splits, M, N, amp)
    side, bn, _ = side_dev(M, N, dout)
    if act == 2:
        side = dict(side, bias_n=(side['bias_n'] / 64).round())
        bn = Vec(side['bias_n'])
    alpha = 0.25 if act == 2 else 0.5
    acc = part.double().sum(0)
    for md in (None, 0, 1, M // 2):
        e = ref.epi(bias_mode=1, act=act, alpha=alpha, m_dev=md)
        tag = 'splitk_reduce %dx%dx%d act %d %s m_dev %s' % (splits, M, N, act, dout, md)
        P = Vec(part.view(-1))
        C = View(M, N, N + 4, dout, 0, side['prev'])
        hip.call('tell_splitk_reduce2', P.t, splits, M * N, M, N, bn.t, act, alpha, C.t, N + 4, hip.dt(dout), mdev_tensor(md))
        torch.cuda.synchronize()
        assert C.intact() and P.intact() and bn.intact(), tag
        want = ref.expected(acc, dout, e, side, side['prev'])
        if act == 2:
            lim = M if md is None else md
            if lim:
                gelu_check(C.t[:lim], want[0][:lim], want[1][:lim], dout, tag)
            exact(C.t[lim:], side['prev'][lim:], tag + ' rows past m_dev')
        else:
            exact(C.t, want, tag)


@pytest.mark.parametrize('M,N,K,act', [(32, 1024, 4096, 0), (128, 1024, 4096, 1), (7, 4096, 2048, 0), (64, 192, 4096, 1)])
def test_splitk_through_ops_gemm(M, N, K, act):
    """the decode step's skinny linears: K slices as one grouped launch + the fold"""
    from tell_amd import ops
    assert ops._SPLITK
    A, B, _ = ref.operands(M, N, K)
    side, bn, _ = side_dev(M, N, BF16)
    C, Ad, Bd = View(M, N, N + 8, BF16), View(M, K, K + 8, BF16, 0, A), View(N, K, K, BF16, 0, B)
    ops.gemm(Ad.t, Bd.t, out=C.t, bias=bn.t, bias_mode=1, act=act, alpha=0.5)
    torch.cuda.synchronize()
    assert C.intact() and Ad.intact() and Bd.intact() and bn.intact()
    exact(C.t, ref.expected(ref.product(A, B), BF16, ref.epi(bias_mode=1, act=act, alpha=0.5), side), 'ops.gemm split-K')


@pytest.mark.parametrize('M,N,K', [(256, 64, 8257), (1024, 1024, 17385)], ids=str)
def test_splitk_through_ops_gemm_nn(M, N, K):
    """few output columns from a very long reduction: ragged last slice, zero padding beyond K; m_dev with zero_rows"""
    from tell_amd import ops
    assert ops._SPLITK and ops._COUNT_LIMIT
    A, B, _ = ref.operands(M, N, K)
    rows = 200
    a = torch.zeros(M, r8(K), dtype=BF16)
    a[:rows, :K] = A[:rows]
    acc = torch.zeros(M, N, dtype=torch.float64)
    acc[:rows] = ref.product(A[:rows], B, how='float32')
    Bd, Ag = View(K, N, N + 8, BF16, 0, B.t()), View(M, r8(K), r8(K) + 8, BF16, 0, a)
    ad = Ag.t
    C = View(M, N, N + 8, BF16)
    ops.gemm_nn(ad, Bd.t, out=C.t, alpha=0.5)
    torch.cuda.synchronize()
    assert C.intact() and Bd.intact() and Ag.intact()
    exact(C.t, ref.expected(acc, BF16, ref.epi(alpha=0.5), None), 'ops.gemm_nn split-K')
    prev = torch.full((M, N), 3.0, dtype=BF16)
    C = View(M, N, N + 8, BF16, 0, prev)
    ops.gemm_nn(ad, Bd.t, out=C.t, alpha=0.5, m_dev=mdev_tensor(rows), zero_rows=True)
    torch.cuda.synchronize()
    assert C.intact()
    exact(C.t, ref.expected(acc, BF16, ref.epi(alpha=0.5, m_dev=rows), None, prev), 'ops.gemm_nn split-K m_dev')


def test_ops_gemm_lays_an_aux_with_another_row_stride_out_like_the_output():
    """the epilogue reads aux[m, n] at m * ldc + n: ops.gemm copies an aux whose rows are laid out differently"""
    from tell_amd import ops
    A, B, _ = ref.operands(37, 70, 72)
    side, _, _ = side_dev(37, 70, BF16)
    C = View(37, 70, 78, BF16)
    aux = side['aux'].to(DEV)                                      # row stride 70, the output's is 78
    Ad, Bd = View(37, 72, 80, BF16, 0, A), View(70, 72, 72, BF16, 0, B)
    ops.gemm(Ad.t, Bd.t, out=C.t, act=4, aux=aux)
    torch.cuda.synchronize()
    assert C.intact() and Ad.intact() and Bd.intact()
    exact(C.t, ref.expected(ref.product(A, B), BF16, ref.epi(act=4), side), 'ops.gemm aux stride')
