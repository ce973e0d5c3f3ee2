"""References of the ResNet trunk kernels (csrc/conv.hip, the convolution launches of csrc/gemm.hip and the statistics
epilogue of csrc/gemm_epi.h).  numpy in float64 / int64 on the CPU, no GPU; amplitudes and the
once-rounded epilogue come from tests/gemm_ref.py.

Convolutions run on integer-valued operands whose every partial sum stays below 2^23, so the fp32 accumulation of the
kernels is exact in any order and the stored bf16 output is ONE number (bit equality).  BatchNorm statistics are then the
float64 statistics of known bf16 numbers; they and the normalised outputs are held to bounds whose constants were measured
on the MI355X against these references and pinned at 4 x the largest ratio, rounded up to a power of two.  With integer
x / mean / beta and power-of-two invstd / gamma the normalisation is exact as well.

Every reference takes `mutant=`: a deliberately wrong variant that tests/test_conv_ref_host.py shows the comparisons
reject (a reference that cannot tell a wrong kernel from a right one checks nothing)."""
import math

import numpy as np

import gemm_ref

LIMIT, SIDE_AMP, BIAS_AMP = gemm_ref.LIMIT, gemm_ref.SIDE_AMP, gemm_ref.BIAS_AMP
HEADROOM = 4
U24 = 2.0 ** -24
U_OUT = {'bf16': 2.0 ** -8, 'f32': 2.0 ** -24}

# ---------------------------------------------------------------- pinned constants (measured on the MI355X, all cases of
# tests/test_gpu_conv.py against the float64 references below; pinned = 4 x measured, rounded up to a power of two)
C_M = 16.0        # mean:   largest ratio measured 3.8462 (tell_bn_stats fp32 C = 2048, M = 9, normal)
C_V = 128.0       # var:    largest ratio measured 25.4559 (tell_bn_stats fp32 C = 2048, M = 9, post-relu).  Above 16, so a
#                   finding: bn_partial_vec_kernel accumulates sum(x - s), sum((x - s)^2) SHIFTED by the chunk's first row s
#                   and takes M2 = q - t^2 / n, so its error scales with var + (s - mean)^2, not with var: where the first
#                   row of a chunk is an outlier (6 var at the worst column of that case) the ratio is 20 - 25.  A plain
#                   fp32 emulation of the kernel's arithmetic on the same inputs gives 21.8 / 22.8 / 22.2 where the device
#                   gives 21.6 / 22.3 / 24.7.  The two-pass paths stay below 14.
C_R = 4.0         # invstd: largest ratio measured 0.9192 (beyond the share of the variance bound at c_v = 128)
C_A = 8.0         # normalised outputs: largest ratio measured 1.6553 (tell_bn_apply fp32 C = 64, residual, no relu)
BLEND = 4.0       # running statistics with momentum != 1: (1 - m) r + m s in fp32 is four roundings (1 - m, two products,
#                   one sum), each at most 2^-24 of |r| + |s|: analytic, not measured


# ---------------------------------------------------------------- rounding
def round_bf16(x):
    """float64 -> the nearest bf16 number (ties to even) as float64: ONE rounding, not float64 -> fp32 -> bf16.  Normal
    range only (nothing here comes near the subnormals or the overflow threshold)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.int64)
    sh = 52 - 7
    r = (b + ((1 << (sh - 1)) - 1) + ((b >> sh) & 1)) >> sh << sh
    out = r.view(np.float64).copy()
    out[~np.isfinite(x)] = x[~np.isfinite(x)]
    return out


def rnd(x, dtype):
    """float64 -> float32 array holding the value rounded ONCE to dtype ('bf16' / 'f32')"""
    if dtype == 'bf16':
        return round_bf16(x).astype(np.float32)
    return np.asarray(x, dtype=np.float64).astype(np.float32)


# ---------------------------------------------------------------- gathers
def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def gather(x, KH, KW, stride, pad, fill=0, mutant=None):
    """x [B, H, W, C] -> [B, OH, OW, KH, KW, C]: tap (kh, kw) of output pixel (oh, ow) is x[b, oh s - pad + kh,
    ow s - pad + kw, :], `fill` outside the image.  An explicit index gather, no library convolution."""
    B, H, W, C = x.shape
    OH, OW = out_size(H, KH, stride, pad), out_size(W, KW, stride, pad)
    if mutant == 'pad_one':
        fill = 1
    first = 1 if (mutant == 'stride_off' and stride == 2) else 0
    ih = np.arange(OH)[:, None] * stride - pad + first + np.arange(KH)[None, :]          # [OH, KH]
    iw = np.arange(OW)[:, None] * stride - pad + np.arange(KW)[None, :]                  # [OW, KW]
    if mutant == 'col_shift':
        iw = iw + 1
    vh, vw = (ih >= 0) & (ih < H), (iw >= 0) & (iw < W)
    g = x[:, np.clip(ih, 0, H - 1)[:, None, :, None], np.clip(iw, 0, W - 1)[None, :, None, :], :]
    valid = (vh[:, None, :, None] & vw[None, :, None, :])[None, ..., None]
    g = np.where(valid, g, np.asarray(fill, dtype=x.dtype))
    if mutant == 'swap_khkw':
        assert KH == KW
        g = g.transpose(0, 1, 2, 4, 3, 5)
    return g


def conv_nhwc(x, w, stride, pad, how='int64', mutant=None):
    """x [B, H, W, Cin], w [Cout, KH, KW, Cin], both integer-valued -> int64 [B, OH, OW, Cout].  how = 'float64': the same
    integers through a float64 product (exact below 2^53; the 384 400-row case, where numpy's int64 product takes long)"""
    x, w = np.asarray(x), np.asarray(w)
    assert np.array_equal(x, np.rint(x)) and np.array_equal(w, np.rint(w))
    Cout, KH, KW, Cin = w.shape
    g = gather(x.astype(np.int64), KH, KW, stride, pad, 0, mutant)
    B, OH, OW = g.shape[:3]
    a, b = g.reshape(B * OH * OW, KH * KW * Cin), w.astype(np.int64).reshape(Cout, KH * KW * Cin)
    if how == 'float64':
        y = np.rint(a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)
    else:
        y = a @ b.T
    return y.reshape(B, OH, OW, Cout)


def stem_layout(w):
    """[Cout, 7, 7, C <= 4] -> [Cout, 256] = 8 kernel rows (the 8th zero) x 8 window columns (the FIRST zero: the window
    of output column ow starts at input column 2 ow - 4) x 4 channels (models/resnet.py stem_weight)"""
    w = np.asarray(w)
    Cout, KH, KW, C = w.shape
    assert KH == 7 and KW == 7 and C <= 4
    wk = np.zeros((Cout, 8, 8, 4), dtype=w.dtype)
    wk[:, :7, 1:, :C] = w
    return wk.reshape(Cout, 256)


def nhwc4(x, C=None):
    """fp32 NCHW [B, C <= 4, H, W] -> the bf16 NHWC4 pixels of tell_nchw_to_nhwc4 (missing channels +0) as float32"""
    x = np.asarray(x, dtype=np.float64)
    B, Cx, H, W = x.shape
    C = Cx if C is None else C
    out = np.zeros((B, H, W, 4), dtype=np.float32)
    out[..., :C] = rnd(x[:, :C].transpose(0, 2, 3, 1), 'bf16')
    return out


def nchw_to_nhwc(x, dtype):
    return rnd(np.asarray(x, dtype=np.float64).transpose(0, 2, 3, 1), dtype)


def im2col(x, KH, KW, stride, pad, Kp=None, mutant=None):
    """-> [B OH OW, Kp]: column (kh KW + kw) Cin + c; padding taps and the columns KH KW Cin .. Kp - 1 are zeros"""
    g = gather(x, KH, KW, stride, pad, 0, mutant)
    B, OH, OW = g.shape[:3]
    K = KH * KW * x.shape[3]
    col = np.zeros((B * OH * OW, K if Kp is None else Kp), dtype=x.dtype)
    col[:, :K] = g.reshape(B * OH * OW, K)
    return col


def maxpool3x3s2(x, mutant=None):
    """3x3 / stride 2 / padding 1 with -inf outside the image -> [B, OH, OW, C]"""
    g = gather(np.asarray(x, dtype=np.float64), 3, 3, 2, 1, 0.0 if mutant == 'pad_zero' else -np.inf)
    return g.max(axis=(3, 4))


# ---------------------------------------------------------------- operands of the exact convolutions
def conv_K(c):
    return c['k'] * c['k'] * c['cin']


def conv_operands(c):
    """-> x [B, H, W, Cin], w [Cout, k, k, Cin] int64, uniform in [-a, a] with a = amplitude(K, 4); bias [Cout] and
    residual [M, Cout] integers in [-255, 255] (exact in bf16)"""
    K = conv_K(c)
    a = gemm_ref.amplitude(K, HEADROOM)
    rng = np.random.default_rng([c.get('seed', 0), c['B'], c['H'], c['W'], c['cin'], c['cout'], c['k'], c['s']])
    x = rng.integers(-a, a + 1, (c['B'], c['H'], c['W'], c['cin']))
    w = rng.integers(-a, a + 1, (c['cout'], c['k'], c['k'], c['cin']))
    OH, OW = out_size(c['H'], c['k'], c['s'], c['p']), out_size(c['W'], c['k'], c['s'], c['p'])
    M = c['B'] * OH * OW
    bias = rng.integers(-BIAS_AMP, BIAS_AMP + 1, c['cout'])
    res = rng.integers(-SIDE_AMP, SIDE_AMP + 1, (M, c['cout']))
    return x, w, bias, res, a


def intermediate_bound(c, epilogue=True):
    """largest magnitude any partial sum or epilogue intermediate can take: K a^2 (+ bias + residual)"""
    a = gemm_ref.amplitude(conv_K(c), HEADROOM)
    return conv_K(c) * a * a + (BIAS_AMP + SIDE_AMP if epilogue else 0)


def conv_case(id, B, H, W, cin, cout, k, s, opts=None, kernel=None, **kw):
    d = dict(id=id, B=B, H=H, W=W, cin=cin, cout=cout, k=k, s=s, p=(k - 1) // 2, opts=opts or {}, kernel=kernel)
    d.update(kw)
    return d


def _glds(bm, bn, conv, ns):
    return 'gemm_nt_glds_kernel<unsigned short, %d, %d, 2, 2, %s, %d>' % (bm, bn, 'true' if conv else 'false', ns)


S64_CONV, S64_PLAIN = 'gemm_nt_s64_kernel<unsigned short, true, 4>', 'gemm_nt_s64_kernel<unsigned short, false, 4>'
T3 = dict(conv_tile=3)

# B = 3, H = 9, W = 13: M = 351 (s1) / 105 (s2), ragged against 64 and 128, OH != OW.  kernel: a substring of the one
# device kernel of the convolution launch (asserted from a trace for the cases that name one).
CONV_CASES = [
    conv_case('1x1s1 c64->64', 3, 9, 13, 64, 64, 1, 1, kernel=_glds(64, 64, False, 2)),
    conv_case('1x1s2 c64->72', 3, 9, 13, 64, 72, 1, 2, kernel=_glds(64, 64, True, 2)),
    conv_case('3x3s1 c64->136', 3, 9, 13, 64, 136, 3, 1, kernel=_glds(64, 64, True, 4)),
    conv_case('3x3s2 c64->72', 3, 9, 13, 64, 72, 3, 2, kernel=_glds(64, 64, True, 4)),
    conv_case('3x3s2 c128->64 s64', 3, 9, 13, 128, 64, 3, 2, kernel=S64_CONV),
    conv_case('3x3s1 c128->72 s64', 3, 9, 13, 128, 72, 3, 1, kernel=S64_CONV),
    conv_case('3x3s1 c128->72 s64=0', 3, 9, 13, 128, 72, 3, 1, dict(gemm_s64=0), kernel=_glds(64, 64, True, 4)),
    conv_case('3x3s2 c64->72 s64=2', 3, 9, 13, 64, 72, 3, 2, dict(gemm_s64=2), kernel=S64_CONV),
    conv_case('1x1s1 c1024->72 s64 plain', 3, 9, 13, 1024, 72, 1, 1, kernel=S64_PLAIN),
    conv_case('1x1s1 c256->136 s64=2 plain', 3, 9, 13, 256, 136, 1, 1, dict(gemm_s64=2), kernel=S64_PLAIN),
    conv_case('3x3s1 c256->64', 3, 9, 13, 256, 64, 3, 1),
    conv_case('1x1s2 c256->136', 3, 9, 13, 256, 136, 1, 2),
    conv_case('3x3s1 H=1', 3, 1, 13, 64, 72, 3, 1),
    conv_case('3x3s2 H=1', 3, 1, 13, 128, 64, 3, 2),
    conv_case('tile1 3x3s2 c64->136', 3, 9, 13, 64, 136, 3, 2, dict(conv_tile=1), kernel=_glds(128, 128, True, 2)),
    conv_case('tile1 1x1s1 c128->72', 3, 9, 13, 128, 72, 1, 1, dict(conv_tile=1), kernel=_glds(128, 128, False, 2)),
    conv_case('tile2 3x3s1 c64->72', 3, 9, 13, 64, 72, 3, 1, dict(conv_tile=2), kernel=_glds(128, 64, True, 2)),
    conv_case('tile2 1x1s1 c64->136', 3, 9, 13, 64, 136, 1, 1, dict(conv_tile=2), kernel=_glds(128, 64, False, 2)),
    conv_case('tile3 ring2 3x3s1 c64->72', 3, 9, 13, 64, 72, 3, 1, dict(conv_tile=3, gemm_ring=2),
              kernel=_glds(64, 64, True, 2)),
    conv_case('tile3 ring3 3x3s2 c64->136', 3, 9, 13, 64, 136, 3, 2, dict(conv_tile=3, gemm_ring=3),
              kernel=_glds(64, 64, True, 4)),
    conv_case('tile3 ring4 1x1s1 c64->72', 3, 9, 13, 64, 72, 1, 1, dict(conv_tile=3, gemm_ring=4),
              kernel=_glds(64, 64, False, 4)),
    conv_case('tile3 s64=0 3x3s1 c128->136', 3, 9, 13, 128, 136, 3, 1, dict(conv_tile=3, gemm_s64=0)),
]
# the launcher's own 128x64 rule: >= 6000 tiles of 64x64 (B H W = 384 400 rows -> 6007 x 1)
BIG_CASE = conv_case('default 128x64, M=384400', 4, 310, 310, 64, 64, 1, 1, kernel=_glds(128, 64, False, 2))
EPILOGUES = [('none', False, False, False), ('bias', True, False, False), ('bias+relu', True, False, True),
             ('bias+residual+relu', True, True, True)]

STEM_SHAPES = [(2, 18, 22), (3, 37, 40)]
STEM_KERNEL = 'gemm_nt_glds_kernel<unsigned short, 64, 64, 2, 2, true, '


def stem_case(B, H, W, C, cout):
    return dict(id='stem B%d %dx%d C%d->%d' % (B, H, W, C, cout), B=B, H=H, W=W, cin=4, cout=cout, k=7, s=2, p=3, C=C,
                opts={}, kernel=STEM_KERNEL)


def stem_operands(c):
    """image [B, C, H, W] (integers, fp32 NCHW) and w [Cout, 7, 7, 4]: the weights of ALL four channels are non-zero, so
    a channel that tell_nchw_to_nhwc4 did not zero would show in the sums"""
    K = 7 * 7 * 4
    a = gemm_ref.amplitude(K, HEADROOM)
    rng = np.random.default_rng([5, c['B'], c['H'], c['W'], c['C'], c['cout']])
    img = rng.integers(-a, a + 1, (c['B'], c['C'], c['H'], c['W']))
    w = rng.integers(-a, a + 1, (c['cout'], 7, 7, 4))
    OH, OW = out_size(c['H'], 7, 2, 3), out_size(c['W'], 7, 2, 3)
    bias = rng.integers(-BIAS_AMP, BIAS_AMP + 1, c['cout'])
    return img, w, bias, a, c['B'] * OH * OW


def conv_expected(acc, bias=None, residual=None, relu=False):
    """the stored bf16 output of tell_conv_bias_act / tell_conv_bn_stats: act(acc + bias [+ residual]) rounded ONCE
    (gemm_ref.expected: act 4 = relu(v + aux)).  acc int64 [M, Cout] -> torch bf16 [M, Cout]"""
    import torch
    e = gemm_ref.epi(bias_mode=1 if bias is not None else 0, act=4 if residual is not None else (1 if relu else 0))
    side = dict(bias_n=None if bias is None else torch.from_numpy(np.asarray(bias, dtype=np.float64)),
                aux=None if residual is None else torch.from_numpy(np.asarray(residual, dtype=np.float64)))
    return gemm_ref.expected(torch.from_numpy(np.asarray(acc, dtype=np.float64)), gemm_ref.BF16, e, side)


# ---------------------------------------------------------------- BatchNorm in float64
def bn_stats64(y, eps, momentum=1.0, rm=None, rv=None, mutant=None):
    """y [M, C]: the STORED (type-rounded) activation.  -> dict(mean, var (biased), invstd, rm, rv): rm / rv the running
    statistics after the momentum update from rm / rv (zeros when not given), with the unbiased variance - for M = 1 the
    biased one, as the kernels do"""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    unb = var * n / (n - 1) if (n > 1 and mutant != 'biased') else var
    rm = np.zeros_like(mean) if rm is None else np.asarray(rm, dtype=np.float64)
    rv = np.zeros_like(mean) if rv is None else np.asarray(rv, dtype=np.float64)
    return dict(mean=mean, var=var, unb=unb, invstd=1.0 / np.sqrt(var + eps), n=n,
                rm=(1.0 - momentum) * rm + momentum * mean, rv=(1.0 - momentum) * rv + momentum * unb)


def chunk_stats64(y, rows):
    """per chunk of `rows` rows (the last one ragged): mean and M2 = sum (y - mean)^2, [chunks, C] each"""
    y = np.asarray(y, dtype=np.float64)
    ch = [y[r:r + rows] for r in range(0, y.shape[0], rows)]
    return np.stack([c.mean(0) for c in ch]), np.stack([((c - c.mean(0)) ** 2).sum(0) for c in ch])


def combine64(pmean, pm2, M, rows, mutant=None):
    """Chan's combine of chunk statistics -> (mean, biased variance).  mutant 'last_full': the ragged last chunk counted
    as a full one (what bn_finish_apply_kernel / bn_combine_kernel would do with n_last = n_full)"""
    k = pmean.shape[0]
    cnt = np.full(k, float(rows))
    if mutant != 'last_full':
        cnt[-1] = M - (k - 1) * rows
    n = cnt.sum()
    mean = (cnt[:, None] * pmean).sum(0) / n
    m2 = (pm2 + cnt[:, None] * (pmean - mean) ** 2).sum(0)
    return mean, m2 / n


def var_single_pass_f32(y):
    """the variance a kernel gets from fp32 running sums as E[x^2] - E[x]^2 (the cancellation the kernels avoid)"""
    y = np.asarray(y, dtype=np.float32)
    n = np.float32(y.shape[0])
    s, q = np.zeros(y.shape[1], np.float32), np.zeros(y.shape[1], np.float32)
    for r in range(y.shape[0]):
        s = s + y[r]
        q = q + y[r] * y[r]
    m = s / n
    return (q / n - m * m).astype(np.float64)


def bn_apply64(x, mean, invstd, gamma, beta, residual=None, relu=False, mutant=None):
    """normalise, THEN add the residual, THEN relu, all in float64 -> (value before the one rounding to the output type,
    mag = |x - mean| invstd |gamma| + |beta| + |residual|: the scale of the fp32 intermediates, for out_ratio)"""
    x = np.asarray(x, dtype=np.float64)
    v = (x - mean) * invstd * gamma + beta
    mag = np.abs(x - mean) * invstd * np.abs(gamma) + np.abs(beta)
    if mutant == 'relu_first' and relu:
        v = np.maximum(v, 0.0)
    if residual is not None:
        v = v + np.asarray(residual, dtype=np.float64)
        mag = mag + np.abs(residual)
    if relu and mutant != 'relu_first':
        v = np.maximum(v, 0.0)
    return v, mag


def im2col_bn(x, mean, invstd, gamma, beta, relu, dtype, KH, KW, stride, pad, mutant=None):
    """im2col of rnd(relu(BatchNorm(x))): padding taps are exact +0 AFTER the normalisation.  -> (col float32 [M, K],
    unrounded float64 col, mag col).  mutant 'norm_pad': the gather first, the normalisation over every tap"""
    if mutant == 'norm_pad':
        g = gather(np.asarray(x, dtype=np.float64), KH, KW, stride, pad, 0.0)
        v, mag = bn_apply64(g, mean, invstd, gamma, beta, None, relu)
    else:
        v, mag = bn_apply64(x, mean, invstd, gamma, beta, None, relu)
        v, mag = gather(v, KH, KW, stride, pad, 0.0), gather(mag, KH, KW, stride, pad, 0.0)
    B, OH, OW = v.shape[:3]
    v, mag = v.reshape(B * OH * OW, -1), mag.reshape(B * OH * OW, -1)
    return rnd(v, dtype), v, mag


# ---------------------------------------------------------------- comparisons: each returns the largest ratio
def _ratio(err, scale):
    """max err / scale; where the scale is 0 the error must be 0 too"""
    err, scale = np.asarray(err, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    if not np.isfinite(err).all():
        return math.inf
    r = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def _spread(st):
    return st['var'] + np.abs(st['mean']) * np.sqrt(st['var'])


def mean_ratio(got, st):
    """|got - mean| / (2^-24 (|mean| + std)); holds when <= C_M"""
    return _ratio(np.abs(np.asarray(got, np.float64) - st['mean']), U24 * (np.abs(st['mean']) + np.sqrt(st['var'])))


def var_ratio(got, st):
    """got: running_var after a momentum = 1.0 update (the blend is exact: 0 r + 1 v).  |got - ref| / (2^-24 (var +
    |mean| std)); holds when <= C_V"""
    return _ratio(np.abs(np.asarray(got, np.float64) - st['unb']), U24 * _spread(st))


def invstd_ratio(got, st, eps):
    """(relative error - 0.5 (variance bound) / (var + eps)) / 2^-24; holds when <= C_R"""
    rel = np.abs(np.asarray(got, np.float64) - st['invstd']) / st['invstd']
    if not np.isfinite(rel).all():
        return math.inf
    return float(((rel - 0.5 * C_V * U24 * _spread(st) / (st['var'] + eps)) / U24).max())


def running_ok(got_rm, got_rv, st, momentum, rm0, rv0):
    """the momentum blend of the running statistics: the statistic's own bound scaled by the momentum, plus BLEND
    roundings of the blend itself -> the largest (error / allowance), holds when <= 1"""
    rm0, rv0 = np.asarray(rm0, np.float64), np.asarray(rv0, np.float64)
    am = momentum * C_M * U24 * (np.abs(st['mean']) + np.sqrt(st['var'])) + BLEND * U24 * (np.abs(rm0) + np.abs(st['mean']))
    av = momentum * C_V * U24 * _spread(st) + BLEND * U24 * (np.abs(rv0) + np.abs(st['unb']))
    return max(_ratio(np.abs(np.asarray(got_rm, np.float64) - st['rm']), am),
               _ratio(np.abs(np.asarray(got_rv, np.float64) - st['rv']), av))


def out_ratio(got, ref, mag, dtype):
    """(|got - ref| - u_out |ref|) / (2^-24 mag) with u_out = 2^-8 (bf16) / 2^-24 (fp32); holds when <= C_A"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return _ratio(np.maximum(np.abs(got - ref) - U_OUT[dtype] * np.abs(ref), 0.0), U24 * np.asarray(mag, np.float64))


# ---------------------------------------------------------------- inputs of tell_bn_stats
def bn_input(kind, M, C, dtype, seed=0):
    """-> float32 [M, C] holding dtype-representable values"""
    rng = np.random.default_rng([seed, M, C, {'normal': 1, 'relu': 2, 'large_mean': 3, 'steps': 4}[kind]])
    if kind == 'normal':
        x = rng.standard_normal((M, C))
    elif kind == 'relu':
        x = np.maximum(rng.standard_normal((M, C)), 0.0)
    elif kind == 'large_mean':
        x = 1000.0 + 0.5 * rng.standard_normal((M, C)) if dtype == 'f32' else 96.0 + 0.5 * rng.integers(-8, 9, (M, C))
    else:
        raise KeyError(kind)
    x = rnd(x, dtype)
    x[:, C - 1] = 1024.0                       # a constant column: mean exactly 1024, variance exactly 0
    return x
