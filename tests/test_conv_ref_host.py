"""The references of tests/conv_ref.py proved on the CPU: cross-checks against torch in float64,
the exactness bounds of every convolution case, and the reference MUTANTS - deliberately wrong variants that the
comparisons of tests/test_gpu_conv.py must reject, and that differ from the reference only where they should."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as ref
import gemm_ref

T = torch.from_numpy
ALL_CONV = ref.CONV_CASES + [ref.stem_case(B, H, W, 3, 72) for B, H, W in ref.STEM_SHAPES]


def torch_conv(x, w, s, p):
    y = F.conv2d(T(x.astype(np.float64)).permute(0, 3, 1, 2), T(w.astype(np.float64)).permute(0, 3, 1, 2), None, s, p)
    return y.permute(0, 2, 3, 1).numpy()


def operands(c):
    if c['k'] == 7:
        img, w, bias, a, M = ref.stem_operands(c)
        return ref.nhwc4(img).astype(np.int64), w
    x, w, bias, res, a = ref.conv_operands(c)
    return x, w


@pytest.mark.parametrize('c', ALL_CONV, ids=[c['id'] for c in ALL_CONV])
def test_conv_nhwc_equals_torch_bit_for_bit(c):
    x, w = operands(c)
    y = ref.conv_nhwc(x, w, c['s'], c['p'])
    assert y.dtype == np.int64
    assert np.array_equal(y.astype(np.float64), torch_conv(x, w, c['s'], c['p']))
    assert np.array_equal(y, ref.conv_nhwc(x, w, c['s'], c['p'], how='float64'))
    assert np.abs(y).max() < ref.LIMIT


def test_big_case_float64_product_equals_torch():
    c = ref.BIG_CASE
    x, w, bias, res, a = ref.conv_operands(c)
    y = ref.conv_nhwc(x, w, 1, 0, how='float64')
    assert y.shape == (4, 310, 310, 64) and 4 * 310 * 310 == 384400 and (384400 + 63) // 64 >= 6000
    assert np.array_equal(y.astype(np.float64), torch_conv(x, w, 1, 0))
    rows = slice(1000, 1300)                                     # the int64 product on a slab of rows
    assert np.array_equal(y.reshape(-1, 64)[rows], x.reshape(-1, 64)[rows] @ w.reshape(64, 64).T)


def test_stem_layout_is_the_models_layout():
    """stem_layout against the words of models/resnet.py stem_weight, and the gather it stands for: the [Cout, 256]
    weight applied to an 8 x 8 x 4 window that starts at input column 2 ow - 4 is the 7x7 / stride 2 / padding 3 conv"""
    c = ref.stem_case(2, 18, 22, 3, 72)
    img, w, bias, a, M = ref.stem_operands(c)
    x4 = ref.nhwc4(img).astype(np.int64)
    assert (x4[..., 3] == 0).all()
    wl = ref.stem_layout(w).reshape(72, 8, 8, 4)
    assert (wl[:, 7] == 0).all() and (wl[:, :, 0] == 0).all() and np.array_equal(wl[:, :7, 1:], w)
    xp = np.zeros((2, 18 + 8, 22 + 8, 4), dtype=np.int64)
    xp[:, 3:21, 4:26] = x4                                       # row oh 2 - 3 + kh, column ow 2 - 4 + j
    OH, OW = ref.out_size(18, 7, 2, 3), ref.out_size(22, 7, 2, 3)
    y = np.zeros((2, OH, OW, 72), dtype=np.int64)
    for oh in range(OH):
        for ow in range(OW):
            y[:, oh, ow] = xp[:, 2 * oh:2 * oh + 8, 2 * ow:2 * ow + 8].reshape(2, 256) @ wl.reshape(72, 256).T
    assert np.array_equal(y, ref.conv_nhwc(x4, w, 2, 3))


def test_nhwc4_and_nchw_to_nhwc():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 5, 7)).astype(np.float32)
    for C in (1, 2, 3):
        got = ref.nhwc4(x[:, :C])
        want = torch.zeros(2, 5, 7, 4)
        want[..., :C] = T(x[:, :C]).permute(0, 2, 3, 1).bfloat16().float()
        assert np.array_equal(got, want.numpy()) and not np.signbit(got[..., C:]).any()
    assert np.array_equal(ref.nchw_to_nhwc(x, 'bf16'), T(x).permute(0, 2, 3, 1).bfloat16().float().numpy())
    assert np.array_equal(ref.nchw_to_nhwc(x, 'f32'), T(x).permute(0, 2, 3, 1).numpy())


def test_round_bf16_is_one_rounding_to_nearest_even():
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 7, 20000), [0.0, -0.0, 1.0, 257.0, 255.0]])
    x32 = x.astype(np.float32)
    assert np.array_equal(ref.round_bf16(x32.astype(np.float64)), T(x32).bfloat16().double().numpy())
    # ties go to even; a value just above a tie that fp32 would first round ONTO the tie goes up (double rounding down)
    assert ref.round_bf16(np.array([1.00390625]))[0] == 1.0 and ref.round_bf16(np.array([1.01171875]))[0] == 1.015625
    x = 1.00390625 + 2.0 ** -40
    assert ref.round_bf16(np.array([x]))[0] == 1.0078125 and float(torch.tensor(x, dtype=torch.float64).float().bfloat16()) == 1.0


@pytest.mark.parametrize('M,C', [(1, 4), (2, 3), (37, 8), (521, 5)])
def test_bn_stats64_and_apply64_equal_torch_float64(M, C):
    rng = np.random.default_rng(M)
    x = 3.0 + 2.0 * rng.standard_normal((M, C))
    g, b = rng.uniform(0.5, 1.5, C), rng.standard_normal(C)
    rm0, rv0 = rng.standard_normal(C), rng.uniform(0.5, 2, C)
    for mom in (1.0, 0.1):
        st = ref.bn_stats64(x, 1e-5, mom, rm0, rv0)
        v, mag = ref.bn_apply64(x, st['mean'], st['invstd'], g, b)
        if M > 1:
            rm, rv = T(rm0.copy()), T(rv0.copy())
            y = F.batch_norm(T(x), rm, rv, T(g), T(b), True, mom, 1e-5)
            assert np.abs(v - y.numpy()).max() <= 1e-12 * max(1.0, np.abs(v).max())
            assert np.abs(st['rm'] - rm.numpy()).max() <= 1e-12 and np.abs(st['rv'] - rv.numpy()).max() <= 1e-12
        else:
            assert np.array_equal(st['unb'], st['var']) and (st['var'] == 0).all()
        assert np.abs(st['mean'] - x.mean(0)).max() <= 1e-12 and np.abs(st['var'] - x.var(0)).max() <= 1e-12
    res = rng.standard_normal((M, C))
    v, mag = ref.bn_apply64(x, st['mean'], st['invstd'], g, b, res, True)
    assert np.array_equal(v, np.maximum((x - st['mean']) * st['invstd'] * g + b + res, 0)) and (mag >= np.abs(res)).all()


@pytest.mark.parametrize('M,rows', [(65, 64), (521, 64), (1000, 128), (64, 64), (7, 8)])
def test_chan_combine_of_chunks_equals_the_direct_statistics(M, rows):
    rng = np.random.default_rng(M)
    y = 5.0 + rng.standard_normal((M, 6))
    pm, pq = ref.chunk_stats64(y, rows)
    mean, var = ref.combine64(pm, pq, M, rows)
    st = ref.bn_stats64(y, 1e-5)
    assert np.abs(mean - st['mean']).max() <= 1e-12 and np.abs(var - st['var']).max() <= 1e-12


@pytest.mark.parametrize('k,s,p,Kp', [(3, 1, 1, None), (3, 2, 1, None), (1, 2, 0, None), (7, 2, 3, 152), (3, 1, 1, 80)])
def test_im2col_equals_unfold(k, s, p, Kp):
    rng = np.random.default_rng(k + s)
    x = rng.standard_normal((2, 9, 13, 3 if Kp == 152 else 8))
    col = ref.im2col(x, k, k, s, p, Kp)
    C = x.shape[3]
    u = F.unfold(T(x).permute(0, 3, 1, 2), k, 1, p, s)                       # [B, C k k, L], rows ordered (c, kh, kw)
    u = u.reshape(2, C, k, k, -1).permute(0, 4, 2, 3, 1).reshape(-1, k * k * C).numpy()
    assert np.array_equal(col[:, :k * k * C], u) and (col[:, k * k * C:] == 0).all()
    assert col.shape[1] == (Kp or k * k * C)


@pytest.mark.parametrize('H,W', [(9, 13), (8, 12), (1, 13), (1, 1), (2, 2)])
def test_maxpool_equals_torch(H, W):
    rng = np.random.default_rng(H * W)
    x = rng.standard_normal((2, H, W, 5)) - 3.0
    want = F.max_pool2d(T(x).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(ref.maxpool3x3s2(x), want)


def test_intermediate_bounds_of_every_exact_case():
    for c in ref.CONV_CASES + [ref.BIG_CASE]:
        assert ref.intermediate_bound(c) < ref.LIMIT, c['id']
        assert gemm_ref.amplitude(ref.conv_K(c), ref.HEADROOM) >= 1, c['id']
        x, w, bias, res, a = (None,) * 5 if c is ref.BIG_CASE else ref.conv_operands(c)
        if x is not None:
            assert np.abs(x).max() <= a and np.abs(w).max() <= a and np.abs(bias).max() <= 255 and np.abs(res).max() <= 255
    for B, H, W in ref.STEM_SHAPES:
        for C in (1, 2, 3, 4):
            c = ref.stem_case(B, H, W, C, 64)
            assert ref.intermediate_bound(c) < ref.LIMIT


# ---------------------------------------------------------------- mutants of the reference
def _equal(a, b):
    return gemm_ref.mismatch(a, b) is None


def test_mutant_kh_kw_swapped():
    c = ref.CONV_CASES[2]                                            # 3x3 / stride 1
    x, w, bias, res, a = ref.conv_operands(c)
    good, bad = ref.conv_nhwc(x, w, 1, 1), ref.conv_nhwc(x, w, 1, 1, mutant='swap_khkw')
    assert not _equal(ref.conv_expected(bad.reshape(-1, c['cout'])), ref.conv_expected(good.reshape(-1, c['cout'])))
    ws = w + w.transpose(0, 2, 1, 3)                                 # a kernel symmetric in (kh, kw) cannot tell
    assert np.array_equal(ref.conv_nhwc(x, ws, 1, 1), ref.conv_nhwc(x, ws, 1, 1, mutant='swap_khkw'))


@pytest.mark.parametrize('idx', [2, 3])
def test_mutant_padding_ring_of_ones(idx):
    c = ref.CONV_CASES[idx]
    x, w, bias, res, a = ref.conv_operands(c)
    good, bad = ref.conv_nhwc(x, w, c['s'], 1), ref.conv_nhwc(x, w, c['s'], 1, mutant='pad_one')
    assert not _equal(ref.conv_expected(bad.reshape(-1, c['cout'])), ref.conv_expected(good.reshape(-1, c['cout'])))
    d = (good != bad).any(3)                                         # only windows that reach outside the image differ
    OH, OW = d.shape[1:]
    lo_h = (c['H'] - 1 + 1 - 2) // c['s']                            # last oh whose window ends inside: oh s - 1 + 2 <= H - 1
    lo_w = (c['W'] - 1 + 1 - 2) // c['s']
    assert not d[:, 1:lo_h + 1, 1:lo_w + 1].any() and d[:, 0].any() and d[:, :, 0].any()


def test_mutant_stride_2_window_one_row_late():
    c = ref.CONV_CASES[3]                                            # 3x3 / stride 2
    x, w, bias, res, a = ref.conv_operands(c)
    good, bad = ref.conv_nhwc(x, w, 2, 1), ref.conv_nhwc(x, w, 2, 1, mutant='stride_off')
    assert not _equal(ref.conv_expected(bad.reshape(-1, 72)), ref.conv_expected(good.reshape(-1, 72)))
    c1 = ref.CONV_CASES[2]                                           # stride 1 is not touched by it
    x, w, bias, res, a = ref.conv_operands(c1)
    assert np.array_equal(ref.conv_nhwc(x, w, 1, 1), ref.conv_nhwc(x, w, 1, 1, mutant='stride_off'))


def test_mutant_stem_window_column_shifted():
    c = ref.stem_case(2, 18, 22, 3, 64)
    img, w, bias, a, M = ref.stem_operands(c)
    x4 = ref.nhwc4(img).astype(np.int64)
    good, bad = ref.conv_nhwc(x4, w, 2, 3), ref.conv_nhwc(x4, w, 2, 3, mutant='col_shift')
    assert not _equal(ref.conv_expected(bad.reshape(M, 64)), ref.conv_expected(good.reshape(M, 64)))
    x5 = np.concatenate([x4[:, :, :1] * 0, x4], axis=2)              # the same image one column to the right undoes it
    assert np.array_equal(ref.conv_nhwc(x5, w, 2, 3, mutant='col_shift')[:, :, :good.shape[2]], good)


@pytest.mark.parametrize('M,rows', [(65, 64), (129, 64), (8129, 64), (257, 128)])
def test_mutant_last_chunk_counted_as_full(M, rows):
    """the ragged last chunk (one row here) weighted as a whole chunk: far outside the bounds of mean and variance"""
    y = ref.bn_input('normal', M, 8, 'bf16')
    pm, pq = ref.chunk_stats64(y, rows)
    st = ref.bn_stats64(y, 1e-5)
    mean, var = ref.combine64(pm, pq, M, rows)
    ok = dict(st, unb=var * M / (M - 1))
    assert ref.mean_ratio(mean, st) < 1e-3 and ref.var_ratio(ok['unb'], st) < 1e-3
    mean, var = ref.combine64(pm, pq, M, rows, mutant='last_full')
    live = slice(0, 7)                                               # (column 7 is the constant one: any weights agree)
    sub = {k: (v[live] if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    assert ref.mean_ratio(mean[live], sub) > 100 * ref.C_M
    assert ref.var_ratio((var * M / (M - 1))[live], sub) > 100 * ref.C_V
    M2 = (M // rows) * rows                                          # no ragged chunk: the mutant is the reference
    y2 = y[:M2]
    pm, pq = ref.chunk_stats64(y2, rows)
    assert np.array_equal(ref.combine64(pm, pq, M2, rows)[1], ref.combine64(pm, pq, M2, rows, mutant='last_full')[1])


def test_mutant_biased_running_variance():
    for M in (9, 521, 70001):
        y = ref.bn_input('normal', M, 8, 'bf16')
        st, bad = ref.bn_stats64(y, 1e-5), ref.bn_stats64(y, 1e-5, mutant='biased')
        assert np.array_equal(st['mean'], bad['mean']) and np.array_equal(st['invstd'], bad['invstd'])
        # the two differ by var / M, i.e. by 2^24 / M of the bound's unit: 1.9e6 (M = 9), 3.2e4, 240 (M = 70001) against
        # c_v = 128 - beyond about 130 000 rows the bound cannot tell them apart, the smaller cases of the file do
        r = ref.var_ratio(bad['rv'][:7], {k: (v[:7] if isinstance(v, np.ndarray) else v) for k, v in st.items()})
        assert r > 1.5 * ref.C_V and r > 0.9 * 2 ** 24 / M
        assert ref.running_ok(bad['rm'], bad['rv'], st, 1.0, np.zeros(8), np.zeros(8)) > 1.5
    st, bad = ref.bn_stats64(y[:1], 1e-5), ref.bn_stats64(y[:1], 1e-5, mutant='biased')
    assert np.array_equal(st['rv'], bad['rv'])                       # one row: the kernels use the biased one too


def test_mutant_relu_before_the_residual():
    rng = np.random.default_rng(8)
    x = rng.integers(-40, 41, (50, 8)).astype(np.float64)
    mean, invstd, gamma, beta = np.full(8, 3.0), np.full(8, 0.25), np.full(8, -2.0), np.full(8, 1.0)
    res = rng.integers(-30, 31, (50, 8)).astype(np.float64)
    good, mag = ref.bn_apply64(x, mean, invstd, gamma, beta, res, True)
    bad, _ = ref.bn_apply64(x, mean, invstd, gamma, beta, res, True, mutant='relu_first')
    for dt in ('bf16', 'f32'):
        assert ref.out_ratio(ref.rnd(bad, dt), good, mag, dt) > 100 * ref.C_A
        assert ref.out_ratio(ref.rnd(good, dt), good, mag, dt) == 0.0
    pre = (x - mean) * invstd * gamma + beta
    keep = (pre >= 0) & (pre + res >= 0)                            # neither relu clips: the order cannot matter
    assert np.array_equal(good[keep], bad[keep]) and keep.any() and (good != bad)[~keep].any()
    same, _ = ref.bn_apply64(x, mean, invstd, gamma, beta, None, True, mutant='relu_first')
    assert np.array_equal(same, ref.bn_apply64(x, mean, invstd, gamma, beta, None, True)[0])


@pytest.mark.parametrize('s', [1, 2])
def test_mutant_im2col_bn_normalises_the_padding(s):
    rng = np.random.default_rng(9)
    x = rng.integers(-20, 21, (2, 5, 7, 8)).astype(np.float64)
    mean, invstd, gamma, beta = np.full(8, -4.0), np.full(8, 0.5), np.full(8, 2.0), np.full(8, 3.0)
    assert ((beta - mean * invstd * gamma) > 0).all()                # a normalised zero tap would be 7, not 0
    good, v, mag = ref.im2col_bn(x, mean, invstd, gamma, beta, True, 'bf16', 3, 3, s, 1)
    bad, _, _ = ref.im2col_bn(x, mean, invstd, gamma, beta, True, 'bf16', 3, 3, s, 1, mutant='norm_pad')
    pad = ref.im2col(np.ones_like(x), 3, 3, s, 1) == 0
    assert pad.any() and (good[pad] == 0).all() and not np.signbit(good[pad]).any()
    assert (bad[pad] == 7.0).all() and np.array_equal(good[~pad], bad[~pad])
    assert not np.array_equal(good, bad)


def test_mutant_maxpool_padding_zero():
    rng = np.random.default_rng(10)
    x = -1.0 - np.abs(rng.standard_normal((2, 9, 13, 4)))            # all negative: a zero padding tap wins every border max
    good, bad = ref.maxpool3x3s2(x), ref.maxpool3x3s2(x, mutant='pad_zero')
    assert (good < 0).all() and (bad[:, 0] == 0).all() and (bad[:, :, 0] == 0).all()
    assert np.array_equal(good[:, 1:4, 1:6], bad[:, 1:4, 1:6])       # windows inside the image
    assert np.array_equal(ref.maxpool3x3s2(-x), ref.maxpool3x3s2(-x, mutant='pad_zero'))   # a positive input cannot tell


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('M', [9, 521, 4097, 70001])
def test_mutant_single_pass_variance_on_large_mean(dtype, M):
    """fp32 E[x^2] - E[x]^2 on the large-mean inputs.  Its ratio is about |mean| / std (2000 for 1000 + 0.5 N(0, 1), 40
    for 96 + 0.5 k) times the growth of the rounding error with the number of accumulated rows.  Figures (ratio; c_v = 128):
        fp32   M = 9: 5.5e3   521: 6.9e3   4097: 1.1e5   70001: 5.5e6
        bf16   M = 9: 1.3e2   521: 1.2e3   4097: 8.4e3   70001: 2.7e4
    Held: >= 100 c_v on the fp32 large-mean input once thousands of rows are accumulated (M = 4097, 70001: the row counts
    of the trunk are 6 272 .. 401 408); on the others the mutant is rejected (> c_v) except bf16 M = 9, whose nine
    two-digit values the single pass sums without a rounding that matters.  With c_v = 16, which the variance bound was
    expected to reach before the measurement, every fp32 size would clear 100 c_v."""
    y = ref.bn_input('large_mean', M, 4, dtype)
    st = ref.bn_stats64(y, 1e-5)
    bad = ref.var_single_pass_f32(y) * M / (M - 1)
    live = {k: (v[:3] if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    r = ref.var_ratio(bad[:3], live)
    print('single-pass variance %s M=%d: ratio %.1f = %.1f c_v' % (dtype, M, r, r / ref.C_V))
    if dtype == 'f32' and M >= 4097:
        assert r >= 100 * ref.C_V
    elif (dtype, M) != ('bf16', 9):
        assert r > 4 * ref.C_V
    assert ref.var_ratio(st['unb'].astype(np.float32), st) <= 1.0     # the reference itself, rounded to fp32
