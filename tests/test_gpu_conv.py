"""The ResNet trunk kernels through the C ABI (csrc/conv.hip, the convolution launches of csrc/gemm.hip, the statistics
epilogue staged_store_stats of csrc/gemm_epi.h) against the references of tests/conv_ref.py:
  * convolutions on integer operands: the stored bf16 output BIT FOR BIT, on every tile / ring / s64 path and epilogue;
  * BatchNorm statistics (conv epilogue + combine, tell_gemm_bn_stats, tell_bn_stats) against the float64 statistics of
    the stored activation, to the bounds c_m / c_v / c_r of conv_ref.py;
  * tell_bn_apply / tell_im2col_bn on integer / power-of-two parameters bit for bit, on random ones to c_a;
  * tell_conv_bn_act (fused finish + apply, super-chunk combine, the two-launch fallback) to c_a;
  * tell_im2col / tell_maxpool3x3s2 / tell_nchw_to_nhwc bit for bit.
Every output, workspace and statistics vector sits between guard bands (tests/guarded.py), workspaces are sized exactly
as include/tell_hip.h documents, and for one case per path the launched kernel names are asserted from a trace.
Run on the MI355X box:  python -m pytest tests/test_gpu_conv.py -m gpu   (-s prints every ratio the constants are pinned from)"""
import numpy as np
import pytest
import torch

import conv_ref as ref
import gemm_ref
from guarded import DEV, SENTINEL, Guard, Vec

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
TD = {'bf16': BF16, 'f32': F32}
EPS = float(np.float32(1e-5))
WS_FILL = 7777.0                   # what a workspace holds before a launch: a slot read without being written shows
_R = {}                            # kind -> {tag: largest ratio}
_CACHE = {}


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
def _report():
    yield
    for kind in sorted(_R):
        tag = max(_R[kind], key=_R[kind].get)
        print('\nlargest %-8s ratio over %4d checks: %.4f  (%s)' % (kind, len(_R[kind]), _R[kind][tag], tag))


def hold(kind, tag, ratio, limit):
    """record, print, assert: every inexact quantity goes through here"""
    _R.setdefault(kind, {})[tag] = max(_R.get(kind, {}).get(tag, 0.0), ratio)
    print('%-8s %-70s %.4f' % (kind, tag, ratio))
    assert ratio <= limit, '%s %s: ratio %.4f above %g' % (kind, tag, ratio, limit)


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def dev(a, dtype=BF16):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV)


def vec(a):
    return Vec(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))


def ws(n):
    return Vec(torch.full((int(n),), WS_FILL))


def npy(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def exact(got, want, tag):
    msg = gemm_ref.mismatch(got.cpu(), want)
    assert msg is None, '%s: %s' % (tag, msg)


def kernel_names(fn):
    """names of the device kernels fn() launches (as tests/test_gpu_encoders.py _device_kernel_names)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events()}


def assert_kernels(names, *want, absent=()):
    for w in want:
        assert any(w in n for n in names), 'no kernel %r among %s' % (w, sorted(names))
    for w in absent:
        assert not any(w in n for n in names), 'kernel %r ran: %s' % (w, sorted(names))


def zero_page():
    return cached('zero', lambda: torch.zeros(64, dtype=BF16, device=DEV))


def geometry(c):
    OH, OW = ref.out_size(c['H'], c['k'], c['s'], c['p']), ref.out_size(c['W'], c['k'], c['s'], c['p'])
    return OH, OW, c['B'] * OH * OW, (c['B'], c['H'], c['W'], c['cin'], c['k'], c['k'], c['s'], c['p'], OH, OW, c['cout'])


def conv_data(c):
    """operands on the device, the exact product and the stored raw output with its float64 statistics"""
    def make():
        OH, OW, M, _ = geometry(c)
        if c['k'] == 7:
            img, w, bias, a, _ = ref.stem_operands(c)
            x = ref.nhwc4(img).astype(np.int64)
            res = np.random.default_rng(M).integers(-255, 256, (M, c['cout']))
            wd = dev(ref.stem_layout(w))
        else:
            x, w, bias, res, a = ref.conv_operands(c)
            wd = dev(w.reshape(c['cout'], -1))
        assert ref.intermediate_bound(c) < ref.LIMIT
        acc = ref.conv_nhwc(x, w, c['s'], c['p'], how='float64' if M > 100000 else 'int64').reshape(M, c['cout'])
        raw = ref.conv_expected(acc)
        return dict(x=dev(x), w=wd, bias=bias, res=res, acc=acc, raw=raw, rawd=npy(raw), M=M)
    return cached(('conv', c['id']), make)


def check_stats(tag, st, mean, invstd, rm, rv, momentum, rm0, rv0):
    hold('mean', tag, ref.mean_ratio(npy(mean), st), ref.C_M)
    hold('invstd', tag, ref.invstd_ratio(npy(invstd), st, EPS), ref.C_R)
    if rm is None:
        return
    if momentum == 1.0:
        hold('mean', tag + ' running', ref.mean_ratio(npy(rm), st), ref.C_M)
        hold('var', tag, ref.var_ratio(npy(rv), st), ref.C_V)
    else:
        hold('running', tag, ref.running_ok(npy(rm), npy(rv), st, momentum, rm0, rv0), 1.0)


def running_start(C, seed=0):
    rng = np.random.default_rng([seed, C])
    return rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32)


# ---------------------------------------------------------------- a + b: convolutions and their statistics
def run_conv_case(c, epilogues=ref.EPILOGUES, rounds=((1.0, True), (0.1, True), (0.1, False))):
    from tell_amd import hip
    d = conv_data(c)
    OH, OW, M, geo = geometry(c)
    C, tag, zp = c['cout'], c['id'], zero_page()
    with hip.options(**c['opts']):
        # the convolution alone
        Y = Guard((M, C), BF16)
        launch = lambda: hip.call('tell_conv_bn_stats', d['x'], d['w'], Y.t, *geo, EPS, 1.0, None, None, None, None, None, zp)
        if c['kernel']:
            names = kernel_names(launch)
            assert_kernels(names, c['kernel'], absent=('bn_finish', 'im2col'))
        else:
            launch()
        torch.cuda.synchronize()
        assert Y.intact(), tag
        exact(Y.t, d['raw'], tag + ' plain')
        # the folded (eval-mode) epilogues
        bias, res = vec(d['bias']), dev(d['res'])
        for name, has_bias, has_res, relu in epilogues:
            Y = Guard((M, C), BF16)
            hip.call('tell_conv_bias_act', d['x'], d['w'], Y.t, *geo, bias.t if has_bias else None, res if has_res else None,
                     int(relu), zp)
            torch.cuda.synchronize()
            assert Y.intact() and bias.intact(), tag + ' ' + name
            exact(Y.t, ref.conv_expected(d['acc'], d['bias'] if has_bias else None, d['res'] if has_res else None, relu),
                  tag + ' ' + name)
        # the statistics of the stored output: momentum 1.0 from zeros, 0.1 from non-trivial values, no running vectors
        rm0, rv0 = running_start(C)
        for momentum, running in rounds:
            r0 = (np.zeros(C), np.zeros(C)) if momentum == 1.0 else (rm0, rv0)
            st = ref.bn_stats64(d['rawd'], EPS, momentum, *r0)
            Y, mean, invstd = Guard((M, C), BF16), vec(np.full(C, SENTINEL)), vec(np.full(C, SENTINEL))
            rm, rv, w = vec(r0[0]), vec(r0[1]), ws(2 * ((M + 63) // 64) * C)
            hip.call('tell_conv_bn_stats', d['x'], d['w'], Y.t, *geo, EPS, momentum, mean.t, invstd.t,
                     rm.t if running else None, rv.t if running else None, w.t, zp)
            torch.cuda.synchronize()
            assert all(g.intact() for g in (Y, mean, invstd, rm, rv, w)), tag
            exact(Y.t, d['raw'], tag + ' with statistics')
            if running:
                check_stats('%s m=%g' % (tag, momentum), st, mean.t, invstd.t, rm.t, rv.t, momentum, *r0)
            else:
                check_stats('%s no running' % tag, st, mean.t, invstd.t, None, None, momentum, *r0)
                assert torch.equal(rm.t.cpu(), torch.from_numpy(r0[0])) and torch.equal(rv.t.cpu(), torch.from_numpy(r0[1]))


@pytest.mark.parametrize('c', ref.CONV_CASES, ids=[c['id'] for c in ref.CONV_CASES])
def test_conv_paths_exact_with_statistics(c):
    run_conv_case(c)


def test_conv_default_rule_128x64_tiles():
    """>= 6000 tiles of 64x64 and Cout % 64 == 0: the launcher itself picks 128x64 (3004 row chunks of 128)"""
    run_conv_case(ref.BIG_CASE, epilogues=ref.EPILOGUES[3:], rounds=((1.0, True),))


def test_conv_bias_act_residual_without_relu_is_refused():
    from tell_amd import hip
    c = ref.CONV_CASES[0]
    d = conv_data(c)
    OH, OW, M, geo = geometry(c)
    Y, bias = Guard((M, c['cout']), BF16), vec(d['bias'])
    with pytest.raises(RuntimeError):
        hip.call('tell_conv_bias_act', d['x'], d['w'], Y.t, *geo, bias.t, dev(d['res']), 0, zero_page())
    torch.cuda.synchronize()
    assert Y.untouched()


@pytest.mark.parametrize('what', ['Cin=96', 'Cout=12', '5x5', 'no zero page'])
def test_conv_refusals_leave_the_output_untouched(what):
    from tell_amd import hip
    B, H, W = 2, 5, 7
    cin, cout, k, zp = 64, 64, 3, zero_page()
    if what == 'Cin=96':
        cin = 96
    elif what == 'Cout=12':
        cout = 12
    elif what == '5x5':
        k = 5
    else:
        zp = None
    p = (k - 1) // 2
    x, w = torch.ones(B, H, W, cin, dtype=BF16, device=DEV), torch.ones(cout, k * k * cin, dtype=BF16, device=DEV)
    M = B * H * W
    for entry in ('stats', 'bias_act', 'bn_act'):
        Y, wk = Guard((M, cout), BF16), ws(2 * ((M + 63) // 64) * cout + 258 * cout)
        g = vec(np.ones(cout))
        geo = (B, H, W, cin, k, k, 1, p, H, W, cout)
        with pytest.raises(RuntimeError):
            if entry == 'stats':
                hip.call('tell_conv_bn_stats', x, w, Y.t, *geo, EPS, 0.1, None, None, None, None, None, zp)
            elif entry == 'bias_act':
                hip.call('tell_conv_bias_act', x, w, Y.t, *geo, None, None, 1, zp)
            else:
                hip.call('tell_conv_bn_act', x, w, Y.t, *geo, EPS, 0.1, g.t, g.t, None, None, None, 1, wk.t, zp)
        torch.cuda.synchronize()
        assert Y.untouched() and wk.intact() and bool((wk.t == WS_FILL).all()), (what, entry)


@pytest.mark.parametrize('B,H,W', ref.STEM_SHAPES, ids=str)
def test_stem_gather_from_nhwc4_pixels(B, H, W):
    """tell_nchw_to_nhwc4 for 1..4 channels (the missing ones +0), then the 7x7 / stride 2 / padding 3 gather over those
    pixels with weights that are non-zero in all four channel slots, through both entry points"""
    from tell_amd import hip
    first = True
    for C in (1, 2, 3, 4):
        for cout in (64, 72):
            c = ref.stem_case(B, H, W, C, cout)
            img, w, bias, a, M = ref.stem_operands(c)
            X4 = Guard((B, H, W, 4), BF16)
            imgd = torch.from_numpy(img.astype(np.float32)).to(DEV)
            conv = lambda: hip.call('tell_nchw_to_nhwc4', imgd, X4.t, B, C, H, W)
            if first:
                assert_kernels(kernel_names(conv), 'nchw_to_nhwc4_kernel')
            else:
                conv()
            torch.cuda.synchronize()
            assert X4.intact()
            want4 = torch.from_numpy(ref.nhwc4(img)).to(BF16)
            exact(X4.t, want4, c['id'] + ' nhwc4')
            assert bool((X4.t.view(torch.int16)[..., C:] == 0).all()), 'missing channels must be +0'
            d = conv_data(c)
            OH, OW, M, geo = geometry(c)
            st = ref.bn_stats64(d['rawd'], EPS, 1.0)
            Y, mean, invstd = Guard((M, cout), BF16), vec(np.zeros(cout)), vec(np.zeros(cout))
            rm, rv, wk = vec(np.zeros(cout)), vec(np.zeros(cout)), ws(2 * ((M + 63) // 64) * cout)
            launch = lambda: hip.call('tell_conv_bn_stats', X4.t, d['w'], Y.t, *geo, EPS, 1.0, mean.t, invstd.t, rm.t, rv.t,
                                      wk.t, zero_page())
            if first:
                assert_kernels(kernel_names(launch), ref.STEM_KERNEL, 'bn_finish_kernel', absent=('im2col',))
                first = False
            else:
                launch()
            torch.cuda.synchronize()
            assert all(g.intact() for g in (Y, mean, invstd, rm, rv, wk))
            exact(Y.t, d['raw'], c['id'])
            check_stats(c['id'], st, mean.t, invstd.t, rm.t, rv.t, 1.0, None, None)
            Y, bd = Guard((M, cout), BF16), vec(bias)
            hip.call('tell_conv_bias_act', X4.t, d['w'], Y.t, *geo, bd.t, None, 1, zero_page())
            torch.cuda.synchronize()
            assert Y.intact() and bd.intact()
            exact(Y.t, ref.conv_expected(d['acc'], bias, None, True), c['id'] + ' bias+relu')


def test_stem_odd_width_is_refused():
    from tell_amd import hip
    B, H, W, cout = 2, 18, 21, 64
    x, w = torch.ones(B, H, W, 4, dtype=BF16, device=DEV), torch.ones(cout, 256, dtype=BF16, device=DEV)
    OH, OW = ref.out_size(H, 7, 2, 3), ref.out_size(W, 7, 2, 3)
    Y = Guard((B * OH * OW, cout), BF16)
    with pytest.raises(RuntimeError):
        hip.call('tell_conv_bn_stats', x, w, Y.t, B, H, W, 4, 7, 7, 2, 3, OH, OW, cout, EPS, 0.1, None, None, None, None, None,
                 zero_page())
    with pytest.raises(RuntimeError):
        hip.call('tell_conv_bias_act', x, w, Y.t, B, H, W, 4, 7, 7, 2, 3, OH, OW, cout, None, None, 1, zero_page())
    torch.cuda.synchronize()
    assert Y.untouched()


# ---------------------------------------------------------------- b: tell_gemm_bn_stats
REG = 'gemm_nt_kernel<unsigned short, unsigned short, %d, %d'
GLDS = 'gemm_nt_glds_kernel<unsigned short, %d, %d, %d, %d, false, 2>'
GEMM_STATS = [
    ('64x64 register-staged', (70, 72, 152), {}, 0, REG % (64, 64)),
    ('128x128 direct-to-LDS', (8192, 512, 64), {}, 0, GLDS % (128, 128, 2, 2)),
    ('128x128 direct-to-LDS lda>K', (8192, 512, 64), {}, 16, GLDS % (128, 128, 2, 2)),
    ('128x128 register-staged', (8200, 512, 72), {}, 0, REG % (128, 128)),
    ('256x128 register-staged', (16400, 512, 152), {}, 8, REG % (256, 128)),
    # a forced tile (tuning aid, read per launch) must not change the statistics: 2 runs 256-row chunks, 5 (256x256, whose
    # tile cannot carry the statistics epilogue) is ignored by a statistics launch, 7 / 8 / 9 do not apply to one
    ('gemm_tile=2', (8192, 512, 64), dict(gemm_tile=2), 0, GLDS % (256, 128, 4, 2)),
    ('gemm_tile=5', (8192, 512, 64), dict(gemm_tile=5), 0, GLDS % (128, 128, 2, 2)),
    ('gemm_tile=7', (8192, 512, 64), dict(gemm_tile=7), 0, None),
    ('gemm_tile=8', (8192, 512, 64), dict(gemm_tile=8), 0, None),
    ('gemm_tile=9', (8192, 512, 64), dict(gemm_tile=9), 0, None),
    ('gemm_tile=2 ragged M', (8200, 512, 64), dict(gemm_tile=2), 0, None),
    ('gemm_tile=5 ragged M', (8200, 512, 64), dict(gemm_tile=5), 0, None),
]


@pytest.mark.parametrize('name,shape,opts,lda_pad,kernel', GEMM_STATS, ids=[g[0] for g in GEMM_STATS])
def test_gemm_bn_stats(name, shape, opts, lda_pad, kernel):
    from tell_amd import hip
    M, N, K = shape
    A, B, amp = gemm_ref.operands(M, N, K, BF16, 0, headroom=ref.HEADROOM)
    assert K * amp * amp < ref.LIMIT
    acc = gemm_ref.product(A, B, (M, N, K, 'stats'), how='float32')
    raw = gemm_ref.expected(acc, BF16, gemm_ref.epi(), None)
    rawd = cached(('gstat', shape), lambda: npy(raw))
    lda, ldc = K + lda_pad, N + 8
    Ad = Guard((M, K), BF16, strides=(lda, 1), fill=A)
    Bd = B.to(DEV)
    rm0, rv0 = running_start(N, 1)
    for momentum in (1.0, 0.1):
        r0 = (np.zeros(N), np.zeros(N)) if momentum == 1.0 else (rm0, rv0)
        st = ref.bn_stats64(rawd, EPS, momentum, *r0)
        C, mean, invstd = Guard((M, N), BF16, strides=(ldc, 1)), vec(np.full(N, SENTINEL)), vec(np.full(N, SENTINEL))
        rm, rv, w = vec(r0[0]), vec(r0[1]), ws(2 * ((M + 63) // 64) * N)
        launch = lambda: hip.call('tell_gemm_bn_stats', Ad.t, lda, Bd, K, C.t, ldc, M, N, K, EPS, momentum, mean.t, invstd.t,
                                  rm.t, rv.t, w.t)
        with hip.options(**opts):
            if kernel and momentum == 1.0:
                assert_kernels(kernel_names(launch), kernel, 'bn_finish_kernel')
            else:
                launch()
        torch.cuda.synchronize()
        assert all(g.intact() for g in (Ad, C, mean, invstd, rm, rv, w)), name
        exact(C.t, raw, name)
        check_stats('gemm_bn_stats %s m=%g' % (name, momentum), st, mean.t, invstd.t, rm.t, rv.t, momentum, *r0)


# ---------------------------------------------------------------- c: tell_bn_stats
M_ALL = (1, 7, 8, 9, 521, 4097, 70001)      # one chunk, a ragged one, > 64 chunks (4097: 171 of 24 rows; 70001: 250 of 280 and one row)
M_WIDE = (1, 9, 521)
VEC_K, SCALAR_K = 'bn_partial_vec_kernel<%s>', 'bn_partial_kernel<%s>'
BN_STATS = [
    # dtype, C, rows, element offset of the pointer, kernel
    ('bf16', 8, M_ALL, 0, VEC_K),           # one 16-byte chunk per row
    ('bf16', 64, M_ALL, 0, VEC_K),
    ('bf16', 2048, M_WIDE, 0, VEC_K),       # 256 chunks per row: one row lane
    ('bf16', 4096, M_WIDE, 0, VEC_K),       # 512: two workgroups across
    ('f32', 4, M_ALL, 0, VEC_K),
    ('f32', 1024, M_WIDE, 0, VEC_K),
    ('f32', 2048, M_WIDE, 0, VEC_K),
    ('bf16', 24, M_ALL, 0, SCALAR_K),       # three chunks per row: not a power of two
    ('bf16', 20, M_ALL, 0, SCALAR_K),
    ('f32', 3, M_ALL, 0, SCALAR_K),
    ('f32', 20, M_ALL, 0, SCALAR_K),
    ('bf16', 64, (9, 521, 4097), 2, SCALAR_K),    # vector-eligible C, the pointer 4 bytes off 16-byte alignment
    ('f32', 1024, (9, 521), 1, SCALAR_K),
]


@pytest.mark.parametrize('dtype,C,rows,off,kernel', BN_STATS, ids=['%s C=%d off=%d' % (b[0], b[1], b[3]) for b in BN_STATS])
def test_bn_stats(dtype, C, rows, off, kernel):
    from tell_amd import hip
    kernel = kernel % ('unsigned short' if dtype == 'bf16' else 'float')
    code = hip.dt(TD[dtype])
    first = True
    for M in rows:
        for kind in ('normal', 'relu', 'large_mean'):
            x = ref.bn_input(kind, M, C, dtype)
            st = ref.bn_stats64(x, EPS, 1.0)
            buf = torch.zeros(M * C + 16, dtype=TD[dtype], device=DEV)
            xd = buf[off:off + M * C].view(M, C)
            xd.copy_(torch.from_numpy(x))
            assert xd.data_ptr() % 16 == (off * xd.element_size()) % 16
            chunks = hip.lib().tell_bn_chunks(M)
            mean, invstd, rm, rv, w = vec(np.full(C, SENTINEL)), vec(np.full(C, SENTINEL)), vec(np.zeros(C)), vec(np.zeros(C)), \
                ws(2 * chunks * C)
            launch = lambda: hip.call('tell_bn_stats', xd, M, C, EPS, 1.0, mean.t, invstd.t, rm.t, rv.t, w.t, code)
            if first:
                assert_kernels(kernel_names(launch), kernel, 'bn_finish_kernel')
                first = False
            else:
                launch()
            torch.cuda.synchronize()
            assert all(g.intact() for g in (mean, invstd, rm, rv, w))
            tag = 'bn_stats %s C=%d off=%d M=%d %s' % (dtype, C, off, M, kind)
            check_stats(tag, st, mean.t, invstd.t, rm.t, rv.t, 1.0, None, None)
            # the constant column: exact
            assert float(mean.t[C - 1]) == 1024.0 and float(rv.t[C - 1]) == 0.0 and bool(torch.isfinite(invstd.t).all()), tag
    # momentum 0.1 from non-trivial running values, and no running vectors at all (last M, last kind)
    rm0, rv0 = running_start(C, 2)
    st = ref.bn_stats64(x, EPS, 0.1, rm0, rv0)
    for running in (True, False):
        mean, invstd, rm, rv = vec(np.zeros(C)), vec(np.zeros(C)), vec(rm0), vec(rv0)
        hip.call('tell_bn_stats', xd, M, C, EPS, 0.1, mean.t, invstd.t, rm.t if running else None, rv.t if running else None,
                 w.t, code)
        torch.cuda.synchronize()
        assert all(g.intact() for g in (mean, invstd, rm, rv, w))
        check_stats(tag + ' m=0.1', st, mean.t, invstd.t, rm.t if running else None, rv.t, 0.1, rm0, rv0)
        if not running:
            assert torch.equal(rm.t.cpu(), torch.from_numpy(rm0)) and torch.equal(rv.t.cpu(), torch.from_numpy(rv0))


# ---------------------------------------------------------------- d: tell_bn_apply, tell_im2col_bn
def exact_bn_params(C, seed, positive_zero_tap=False):
    """integers for mean and beta, powers of two for invstd and gamma (negative gammas included): every product and sum
    of the normalisation is exact in fp32 in any association order"""
    rng = np.random.default_rng([seed, C])
    invstd = 2.0 ** -rng.integers(0, 4, C)
    gamma = 2.0 ** rng.integers(-1, 2, C) * rng.choice([-1.0, 1.0], C)
    mean = rng.integers(1, 9, C).astype(np.float64) * rng.choice([-1.0, 1.0], C)
    beta = rng.integers(-8, 9, C).astype(np.float64)
    if positive_zero_tap:                      # beta - mean scale > 0: a normalised padding tap would be non-zero after relu
        mean = -np.abs(mean) * np.sign(gamma)
        beta = np.abs(beta) + 1.0
        assert ((beta - mean * invstd * gamma) > 0).all()
    return mean, invstd, gamma, beta


APPLY = [('bf16', 64, 0, 'bn_apply_vec_kernel<unsigned short>'), ('f32', 64, 0, 'bn_apply_vec_kernel<float>'),
         ('bf16', 20, 0, 'bn_apply_kernel<unsigned short>'), ('f32', 20, 0, 'bn_apply_vec_kernel<float>'),
         ('f32', 22, 0, 'bn_apply_kernel<float>'),             # (20 floats are five 16-byte chunks: still the vector kernel)
         ('bf16', 64, 2, 'bn_apply_kernel<unsigned short>'), ('f32', 64, 1, 'bn_apply_kernel<float>')]


@pytest.mark.parametrize('dtype,C,res_off,kernel', APPLY, ids=['%s C=%d residual off=%d' % a[:3] for a in APPLY])
def test_bn_apply_exact(dtype, C, res_off, kernel):
    from tell_amd import hip
    M, code = 521, hip.dt(TD[dtype])
    rng = np.random.default_rng([C, res_off])
    x = rng.integers(-40, 41, (M, C)).astype(np.float64)
    res = rng.integers(-30, 31, (M, C)).astype(np.float64)
    mean, invstd, gamma, beta = exact_bn_params(C, 1)
    md, sd, gd, bd = vec(mean), vec(invstd), vec(gamma), vec(beta)
    rbuf = torch.zeros(M * C + 16, dtype=TD[dtype], device=DEV)
    rd = rbuf[res_off:res_off + M * C].view(M, C)
    rd.copy_(torch.from_numpy(res))
    first = True
    for relu in (0, 1):
        for has_res in (False, True):
            if res_off and not has_res:
                continue
            v, mag = ref.bn_apply64(x, mean, invstd, gamma, beta, res if has_res else None, bool(relu))
            assert np.array_equal(v, v.astype(np.float32)), 'the case must be exact in fp32'
            want = torch.from_numpy(ref.rnd(v, dtype)).to(TD[dtype])
            for in_place in (False, True):
                Y = Guard((M, C), TD[dtype], fill=x if in_place else None)
                xd = Y.t if in_place else dev(x, TD[dtype])
                launch = lambda: hip.call('tell_bn_apply', xd, md.t, sd.t, gd.t, bd.t, rd if has_res else None, Y.t, M, C, relu, code)
                if first and (has_res or not res_off):
                    assert_kernels(kernel_names(launch), kernel)
                    first = False
                else:
                    launch()
                torch.cuda.synchronize()
                assert Y.intact() and all(g.intact() for g in (md, sd, gd, bd))
                exact(Y.t, want, 'bn_apply %s C=%d relu=%d residual=%s in place=%s' % (dtype, C, relu, has_res, in_place))


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('C', [64, 22])
def test_bn_apply_random_parameters(dtype, C):
    from tell_amd import hip
    M = 521
    rng = np.random.default_rng([C, 7])
    x = ref.rnd(2.0 + 3.0 * rng.standard_normal((M, C)), dtype)
    res = ref.rnd(rng.standard_normal((M, C)), dtype)
    st = ref.bn_stats64(x, EPS)
    mean, invstd = st['mean'].astype(np.float32), st['invstd'].astype(np.float32)       # what the caller supplies: fp32
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32) * rng.choice([-1, 1], C), rng.standard_normal(C).astype(np.float32)
    for relu in (0, 1):
        for has_res in (False, True):
            v, mag = ref.bn_apply64(x, mean, invstd, gamma, beta, res if has_res else None, bool(relu))
            Y = Guard((M, C), TD[dtype])
            hip.call('tell_bn_apply', dev(x, TD[dtype]), vec(mean).t, vec(invstd).t, vec(gamma).t, vec(beta).t,
                     dev(res, TD[dtype]) if has_res else None, Y.t, M, C, relu, hip.dt(TD[dtype]))
            torch.cuda.synchronize()
            assert Y.intact()
            hold('out', 'bn_apply %s C=%d relu=%d residual=%s' % (dtype, C, relu, has_res), ref.out_ratio(npy(Y.t), v, mag, dtype),
                 ref.C_A)


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('stride', [1, 2])
def test_im2col_bn(dtype, stride):
    """integer / power-of-two parameters: bit for bit, the padding taps bitwise +0 although a normalised zero would be
    positive; then random parameters to c_a"""
    from tell_amd import hip
    B, H, W, C = 3, 9, 13, 16
    OH, OW = ref.out_size(H, 3, stride, 1), ref.out_size(W, 3, stride, 1)
    M, K, code = B * OH * OW, 9 * C, hip.dt(TD[dtype])
    rng = np.random.default_rng([stride, 11])
    x = rng.integers(-40, 41, (B, H, W, C)).astype(np.float64)
    pad = torch.from_numpy(ref.im2col(np.ones((B, H, W, C)), 3, 3, stride, 1) == 0)
    mean, invstd, gamma, beta = exact_bn_params(C, 2, positive_zero_tap=True)
    first = True
    for relu in (1, 0):
        want, v, mag = ref.im2col_bn(x, mean, invstd, gamma, beta, bool(relu), dtype, 3, 3, stride, 1)
        assert np.array_equal(v, v.astype(np.float32))
        col = Guard((M, K), TD[dtype])
        launch = lambda: hip.call('tell_im2col_bn', dev(x, TD[dtype]), col.t, B, H, W, C, 3, 3, stride, 1, OH, OW, vec(mean).t,
                                  vec(invstd).t, vec(gamma).t, vec(beta).t, relu, code)
        if first:
            assert_kernels(kernel_names(launch), 'im2col_bn_vec_kernel<%s>' % ('unsigned short' if dtype == 'bf16' else 'float'))
            first = False
        else:
            launch()
        torch.cuda.synchronize()
        assert col.intact()
        exact(col.t, torch.from_numpy(want).to(TD[dtype]), 'im2col_bn %s s=%d relu=%d' % (dtype, stride, relu))
        bits = col.t.cpu().view(torch.int16 if dtype == 'bf16' else torch.int32)
        assert bool(pad.any()) and bool((bits[pad] == 0).all()), 'padding taps must be +0 bit for bit'
    xr = ref.rnd(2.0 + 3.0 * rng.standard_normal((B, H, W, C)), dtype)
    st = ref.bn_stats64(xr.reshape(-1, C), EPS)
    mean, invstd = st['mean'].astype(np.float32), st['invstd'].astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32) * rng.choice([-1, 1], C), rng.standard_normal(C).astype(np.float32)
    for relu in (1, 0):
        want, v, mag = ref.im2col_bn(xr, mean, invstd, gamma, beta, bool(relu), dtype, 3, 3, stride, 1)
        col = Guard((M, K), TD[dtype])
        hip.call('tell_im2col_bn', dev(xr, TD[dtype]), col.t, B, H, W, C, 3, 3, stride, 1, OH, OW, vec(mean).t, vec(invstd).t,
                 vec(gamma).t, vec(beta).t, relu, code)
        torch.cuda.synchronize()
        assert col.intact()
        got = col.t.cpu()
        assert bool((got.view(torch.int16 if dtype == 'bf16' else torch.int32)[pad] == 0).all())
        live = ~pad.numpy()
        hold('out', 'im2col_bn %s s=%d relu=%d' % (dtype, stride, relu), ref.out_ratio(npy(got)[live], v[live], mag[live], dtype),
             ref.C_A)


# ---------------------------------------------------------------- e: tell_conv_bn_act
FA, COMB, FIN, APPLY_V = 'bn_finish_apply_kernel', 'bn_combine_kernel', 'bn_finish_kernel', 'bn_apply_vec_kernel<unsigned short>'


def chunk_case(chunks, cout, opts):
    M = 64 * (chunks - 1) + 1
    return ref.conv_case('fused %d chunks c64->%d' % (chunks, cout), 1, 1, M, 64, cout, 1, 1, opts)


def run_fused(c, relu, has_res, want_kernels=None, absent=(), momenta=(1.0,)):
    from tell_amd import hip
    d = conv_data(c)
    OH, OW, M, geo = geometry(c)
    C = c['cout']
    rng = np.random.default_rng([C, M])
    gamma = (rng.uniform(0.5, 1.5, C) * rng.choice([-1, 1], C)).astype(np.float32)
    beta = (rng.uniform(0.25, 1.0, C) * rng.choice([-1, 1], C)).astype(np.float32)
    res = ref.rnd(rng.standard_normal((M, C)), 'bf16') if has_res else None
    rm0, rv0 = running_start(C, 3)
    for momentum in momenta:
        r0 = (np.zeros(C), np.zeros(C)) if momentum == 1.0 else (rm0, rv0)
        st = ref.bn_stats64(d['rawd'], EPS, momentum, *r0)
        v, mag = ref.bn_apply64(d['rawd'], st['mean'], st['invstd'], gamma, beta, res, bool(relu))
        Y, gd, bd, rm, rv = Guard((M, C), BF16), vec(gamma), vec(beta), vec(r0[0]), vec(r0[1])
        wk = ws(2 * ((M + 63) // 64) * C + 258 * C)
        resd = dev(res) if has_res else None
        launch = lambda: hip.call('tell_conv_bn_act', d['x'], d['w'], Y.t, *geo, EPS, momentum, gd.t, bd.t, rm.t, rv.t, resd,
                                  int(relu), wk.t, zero_page())
        tag = '%s %s relu=%d residual=%s m=%g' % (c['id'], sorted(c['opts'].items()), relu, has_res, momentum)
        with hip.options(**c['opts']):
            if want_kernels and momentum == momenta[0]:
                assert_kernels(kernel_names(launch), *want_kernels, absent=absent)
            else:
                launch()
        torch.cuda.synchronize()
        assert all(g.intact() for g in (Y, gd, bd, rm, rv, wk)), tag
        hold('out', tag, ref.out_ratio(npy(Y.t), v, mag, 'bf16'), ref.C_A)
        if momentum == 1.0:
            hold('mean', tag, ref.mean_ratio(npy(rm.t), st), ref.C_M)
            hold('var', tag, ref.var_ratio(npy(rv.t), st), ref.C_V)
        else:
            hold('running', tag, ref.running_ok(npy(rm.t), npy(rv.t), st, momentum, *r0), 1.0)


@pytest.mark.parametrize('chunks', [1, 2, 4, 5, 127, 128, 129])
def test_fused_conv_bn_chunk_counts(chunks):
    """1x1 / stride 1 with M = 64 (chunks - 1) + 1 rows: the last chunk holds ONE row.  Up to 128 chunks the fused finish +
    apply launch; 129: the two-launch fallback, or with bn_combine = 1 the super-chunk merge in front of the fused launch"""
    few = chunks <= 128
    run_fused(chunk_case(chunks, 64, {}), 1, False, (FA,) if few else (FIN, APPLY_V), () if few else (FA,), momenta=(1.0, 0.1))
    run_fused(chunk_case(chunks, 64, dict(bn_combine=1)), 1, True, (FA,) if few else (COMB, FA), (FIN,) + ((COMB,) if few else ()))
    run_fused(chunk_case(chunks, 64, dict(bn_fuse=0)), 0, True, (FIN, APPLY_V), (FA, COMB))
    if chunks in (5, 129):
        run_fused(chunk_case(chunks, 128, dict(bn_combine=1)), 1, True, (FA,))
        run_fused(chunk_case(chunks, 72, dict(bn_combine=1)), 1, True, (FIN, APPLY_V), (FA, COMB))     # Cout % 64 != 0
        run_fused(chunk_case(chunks, 72, dict(bn_fuse=0)), 0, False, (FIN, APPLY_V), (FA, COMB))


@pytest.mark.parametrize('relu,has_res', [(0, False), (0, True), (1, False), (1, True)])
@pytest.mark.parametrize('bn_wgs', [768, 5, 1], ids=['32 rows', '64 rows', '128 rows'])
def test_fused_conv_bn_rows_per_workgroup(bn_wgs, relu, has_res):
    """M = 257: a workgroup of the fused launch takes 32 / 64 / 128 rows (1 / 2 / 4 passes), the last one a single row"""
    run_fused(chunk_case(5, 64, dict(bn_wgs=bn_wgs)), relu, has_res, (FA,))
    run_fused(chunk_case(5, 128, dict(bn_wgs=bn_wgs)), relu, has_res)


FUSED_PATHS = [
    ref.conv_case('fused 3x3s2 c128->64 s64', 3, 9, 13, 128, 64, 3, 2),
    ref.conv_case('fused 3x3s1 c256->128', 3, 9, 13, 256, 128, 3, 1),
    ref.conv_case('fused 1x1s2 c64->64', 3, 9, 13, 64, 64, 1, 2),
    ref.conv_case('fused tile1 3x3s1 c64->64', 3, 9, 13, 64, 64, 3, 1, dict(conv_tile=1)),       # 3 chunks of 128 rows, 95 last
    ref.conv_case('fused tile2 3x3s2 c64->128', 3, 9, 13, 64, 128, 3, 2, dict(conv_tile=2)),
    ref.conv_case('fused tile2 1x1s1 c64->72', 3, 9, 13, 64, 72, 1, 1, dict(conv_tile=2)),       # the fallback on 128-row chunks
]


@pytest.mark.parametrize('c', FUSED_PATHS, ids=[c['id'] for c in FUSED_PATHS])
def test_fused_conv_bn_on_convolution_paths(c):
    """3x3 / strided forms and the forced 128-row tiles (chunks of 128 rows) behind the fused launch"""
    run_fused(c, 1, True, (FIN, APPLY_V) if c['cout'] % 64 else (FA,), momenta=(1.0, 0.1))
    run_fused(c, 0, False)


@pytest.mark.parametrize('comb', [1, 0])
def test_fused_conv_bn_3004_chunks(comb):
    """M = 384 400 on 128x64 tiles: 3004 chunks of 128 rows -> with bn_combine = 1 126 super-chunks of S = 24"""
    c = dict(ref.BIG_CASE, opts=dict(bn_combine=comb))
    run_fused(c, 1, True, (COMB, FA) if comb else (FIN, APPLY_V), (FIN,) if comb else (FA, COMB))


def test_fused_conv_bn_stem():
    c = ref.stem_case(2, 18, 22, 3, 64)
    run_fused(c, 1, False, (ref.STEM_KERNEL, FA), momenta=(1.0, 0.1))
    run_fused(ref.stem_case(2, 18, 22, 3, 72), 1, False, (ref.STEM_KERNEL, FIN, APPLY_V), (FA,))


# ---------------------------------------------------------------- f: data movement
IM2COL = [
    # dtype, Cin, k, stride, Kp (None: unpadded), element offset of col, kernel
    ('bf16', 16, 3, 1, None, 0, 'im2col_vec_kernel<unsigned short>'),
    ('bf16', 16, 3, 2, None, 0, 'im2col_vec_kernel<unsigned short>'),
    ('f32', 8, 3, 2, None, 0, 'im2col_vec_kernel<float>'),
    ('f32', 8, 1, 2, None, 0, 'im2col_vec_kernel<float>'),
    ('f32', 3, 7, 2, 148, 0, 'im2col_kernel<float>'),
    ('bf16', 3, 7, 2, 150, 1, 'im2col_kernel<unsigned short>'),
    ('bf16', 16, 3, 1, None, 1, 'im2col_kernel<unsigned short>'),
]


@pytest.mark.parametrize('dtype,C,k,s,Kp,off,kernel', IM2COL, ids=['%s C=%d %dx%d/s%d Kp=%s off=%d' % (i[0], i[1], i[2], i[2], i[3], i[4], i[5])
                                                                    for i in IM2COL])
def test_im2col_exact(dtype, C, k, s, Kp, off, kernel):
    from tell_amd import hip
    B, H, W, p = 3, 9, 13, (k - 1) // 2
    OH, OW = ref.out_size(H, k, s, p), ref.out_size(W, k, s, p)
    x = ref.rnd(np.random.default_rng([C, k, s]).standard_normal((B, H, W, C)) + 0.5, dtype)
    want = ref.im2col(x, k, k, s, p, Kp)
    M, Kc = want.shape
    col = Guard((M, Kc), TD[dtype], off=off)
    launch = lambda: hip.call('tell_im2col', dev(x, TD[dtype]), col.t, B, H, W, C, k, k, s, p, OH, OW, Kc, hip.dt(TD[dtype]))
    assert_kernels(kernel_names(launch), kernel)
    torch.cuda.synchronize()
    assert col.intact()
    exact(col.t, torch.from_numpy(want).to(TD[dtype]), 'im2col')
    assert not bool((col.t.cpu().view(torch.int16 if dtype == 'bf16' else torch.int32)[torch.from_numpy(want == 0)] != 0).any())


POOL = [('bf16', 20, 'maxpool_kernel<unsigned short>'), ('f32', 5, 'maxpool_kernel<float>'), ('f32', 8, 'maxpool_kernel<float>'),
        ('bf16', 24, 'maxpool_vec_kernel')]


@pytest.mark.parametrize('dtype,C,kernel', POOL, ids=['%s C=%d' % p[:2] for p in POOL])
def test_maxpool_exact(dtype, C, kernel):
    from tell_amd import hip
    first = True
    for B, H, W in ((3, 9, 13), (2, 1, 13), (2, 8, 12), (1, 1, 1)):
        for negative in (False, True):
            x = ref.rnd(np.random.default_rng([C, H, W]).standard_normal((B, H, W, C)), dtype)
            if negative:
                x = -1.0 - np.abs(x)                          # a pool that starts from 0 instead of -inf returns 0 everywhere
                x = ref.rnd(x, dtype)
            want = ref.maxpool3x3s2(x)
            OH, OW = want.shape[1:3]
            Y = Guard((B, OH, OW, C), TD[dtype])
            launch = lambda: hip.call('tell_maxpool3x3s2', dev(x, TD[dtype]), Y.t, B, H, W, C, OH, OW, hip.dt(TD[dtype]))
            if first:
                assert_kernels(kernel_names(launch), kernel)
                first = False
            else:
                launch()
            torch.cuda.synchronize()
            assert Y.intact()
            exact(Y.t, torch.from_numpy(want.astype(np.float32)).to(TD[dtype]), 'maxpool %s C=%d %dx%d negative=%s' % (dtype, C, H, W, negative))


@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_nchw_to_nhwc_exact(dtype):
    from tell_amd import hip
    B, C, H, W = 3, 5, 9, 13
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((B, C, H, W)) * 10.0 ** rng.integers(-3, 4, (B, C, H, W))).astype(np.float32)
    x[0, 0, 0, :4] = [1.00390625, 1.01171875, -1.00390625, 1.0039063692092896]      # ties to even, and just above a tie
    Y = Guard((B, H, W, C), TD[dtype])
    launch = lambda: hip.call('tell_nchw_to_nhwc', torch.from_numpy(x).to(DEV), Y.t, B, C, H, W, hip.dt(TD[dtype]))
    assert_kernels(kernel_names(launch), 'nchw_to_nhwc_kernel<float, %s>' % ('unsigned short' if dtype == 'bf16' else 'float'))
    torch.cuda.synchronize()
    assert Y.intact()
    exact(Y.t, torch.from_numpy(ref.nchw_to_nhwc(x, dtype)).to(TD[dtype]), 'nchw_to_nhwc ' + dtype)
