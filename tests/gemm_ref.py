"""Exact integer-operand reference of the GEMM family (csrc/gemm*.hip).  numpy / torch on the CPU,
no GPU.

With integer-valued operands every product and every partial sum is an integer; while every intermediate stays below
2^23 in magnitude (half-integers from alpha = 0.5 included), fp32 accumulation is exact in ANY order, so MFMA order,
split-K and float atomics cannot change a bit.  The expected output is one well-defined number, for a bf16 output that
number rounded to nearest even.  Everything but GELU is therefore held to bit equality."""
import math

import numpy as np
import torch

F32, BF16 = torch.float32, torch.bfloat16
LIMIT = 1 << 23              # every intermediate of an exact case stays below this
LIMIT_WIDE = 1 << 24         # the 11-bit K = 4 flavour: sums of four 22-bit products, plain epilogue only
BIAS_AMP = 255               # integer biases
SIDE_AMP = 255               # integer residual / aux / previous C (exact in bf16)
SENTINEL = -65536.0          # exact in both types; nothing a case produces

EPI_DEFAULT = dict(bias_mode=0, act=0, alpha=1.0, accumulate=False, m_dev=None)


def epi(**kw):
    e = dict(EPI_DEFAULT)
    e.update(kw)
    return e


# ---------------------------------------------------------------- amplitudes and bounds (analytic, never by trial)
def amplitude(K, headroom=1, cap=255):
    """largest a with K a^2 headroom <= 2^23 (capped: 255 uses all 8 mantissa bits of bf16)"""
    return min(cap, math.isqrt(LIMIT // (K * headroom)))


HEADROOM = 4                 # alpha <= 2 doubles (acc + bias); bias, aux and previous C fit in the second factor of 2


def intermediate_bound(K, a, e=None, wide=False):
    """largest magnitude any intermediate of the product + epilogue can take, from the amplitudes alone"""
    e = e or EPI_DEFAULT
    v = K * a * a
    if wide:
        return v
    if e.get('bias_mode'):
        v += BIAS_AMP
    v = max(v, v * abs(e.get('alpha', 1.0)))
    if e.get('act') == 4:
        v += SIDE_AMP
    if e.get('accumulate'):
        v += SIDE_AMP
    return v


# ---------------------------------------------------------------- operands and products, cached per key
_OPS, _ACC = {}, {}


def operands(M, N, K, dtype=BF16, seed=0, headroom=HEADROOM, wide=False):
    """A [M, K], B [N, K]: uniform integers in [-a, a], exact in dtype.  wide: the fp32 flavour with 11-bit integers at
    K = 4 (catches an operand narrowed to bf16 / tf32 width, which small integers cannot)."""
    key = (M, N, K, dtype, seed, headroom, wide)
    if key not in _OPS:
        a = 2047 if wide else amplitude(K, headroom)
        assert not wide or (dtype == F32 and K == 4)
        rng = np.random.default_rng([seed, M, N, K, int(wide)])
        A = torch.from_numpy(rng.integers(-a, a + 1, (M, K)).astype(np.float32)).to(dtype)
        B = torch.from_numpy(rng.integers(-a, a + 1, (N, K)).astype(np.float32)).to(dtype)
        _OPS[key] = (A, B, a)
    return _OPS[key]


def product(A, B, key=None, how='float64'):
    """A B^T, exact.  float64 by default; 'int64' and 'float32' give the same numbers (test_gemm_ref_host checks it) and
    the long reductions use float32, which is 40 times faster there."""
    if key is not None and (key, how) in _ACC:
        return _ACC[(key, how)]
    if how == 'int64':
        r = (A.to(torch.int64) @ B.to(torch.int64).t()).double()
    elif how == 'float32':
        r = (A.float() @ B.float().t()).double()
    else:
        r = A.double() @ B.double().t()
    if key is not None:
        _ACC[(key, how)] = r
    return r


def side_inputs(M, N, out_dtype, seed=0):
    """integer bias[n], bias[m], aux for act 3 (zeros, negatives, positives) / act 4, previous C: aux and previous C
    already rounded to the output dtype (exact: |.| <= 255)"""
    rng = np.random.default_rng([seed, M, N, 77])
    f = lambda *s: torch.from_numpy(rng.integers(-BIAS_AMP, BIAS_AMP + 1, s).astype(np.float32))
    aux = torch.from_numpy(rng.integers(-2, 3, (M, N)).astype(np.float32) * 100).to(out_dtype)
    return dict(bias_n=f(N), bias_m=f(M), aux=aux, res=f(M, N).to(out_dtype), prev=f(M, N).to(out_dtype))


def gelu64(x):
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def gelu_alpha(K, a):
    """power of two that brings the pre-activations into about [-8, 8]: a sum of K products of uniform integers in
    [-a, a] has a standard deviation of about sqrt(K) a^2 / 3, and 4 sigma go to 8"""
    sigma = math.sqrt(K) * a * a / 3.0
    return 2.0 ** -max(0, round(math.log2(sigma / 2.0)))


def expected(acc, out_dtype, e, side, prev=None, limit=LIMIT):
    """the epilogue in the order of gemm_epilogue_act: ((acc + bias) * alpha) -> act -> + previous C -> round; rows >=
    m_dev keep prev.  acc: float64 [M, N]; limit: what every value must stay below for the exactness argument (LIMIT_WIDE
    for the 11-bit flavour).  -> tensor of out_dtype; for act 2 (GELU) the float64 (reference, x)."""
    M, N = acc.shape
    v = acc
    if e['bias_mode'] == 1:
        v = v + side['bias_n'].double()[None, :]
    elif e['bias_mode'] == 2:
        v = v + side['bias_m'].double()[:, None]
    v = v * e['alpha']
    if e['act'] == 2:
        return gelu64(v), v
    if e['act'] == 1:
        v = torch.relu(v)
    elif e['act'] == 3:
        v = torch.where(side['aux'].double() > 0, v, torch.zeros_like(v))
    elif e['act'] == 4:
        v = torch.relu(v + side['aux'].double())
    if e['accumulate']:
        v = v + prev.double()
    assert float(acc.abs().max()) < limit and float(v.abs().max()) < limit
    out = v.to(out_dtype)                      # every v is an fp32 number, so this is ONE rounding, nearest even
    if e['m_dev'] is not None and e['m_dev'] < M:
        out[e['m_dev']:] = prev[e['m_dev']:]
    return out


def expected_dropout_residual(acc, bias_n, res, keep, p, roundings=2):
    """res + bf16((lin + bias) * keep / (1 - p)) at p = 0.5 (the factor is exactly 2) or p = 0, then rounded: the two
    roundings of the ping-pong kernel's staged epilogue.  roundings = 1: bf16(res + (lin + bias) * keep / (1 - p)) from
    fp32, what the four-wave kernel (K % 128 == 0) computes (see the comment at the entry point in csrc/gemm_pp2.hip)."""
    assert p in (0.0, 0.5)
    v = acc + bias_n.double()[None, :]
    if p > 0:
        v = v * keep.double() * 2.0
    if roundings == 2:
        v = v.to(BF16).double()
    return (res.double() + v).to(BF16)


def expected_asum(A, scale, preset, k_lim=None):
    """asum[m] = preset + scale * sum_k A[m, k] (A as [M, K]), exact"""
    k = A.shape[1] if k_lim is None else k_lim
    return (preset.double() + scale * A[:, :k].double().sum(1)).float()


def mismatch(got, want):
    """the comparison every exact test uses: torch.equal on the raw tensors; on a difference the count, the first
    (m, n) and got / want there.  -> None or the message"""
    if got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want):
        return None
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = (got != want) | (got.isnan() != want.isnan())
    idx = bad.nonzero()
    first = tuple(int(i) for i in idx[0])
    return '%d of %d differ, first at %s: got %r want %r' % (idx.shape[0], bad.numel(), first, float(got[first]),
                                                              float(want[first]))


def gelu_ratio(got, ref, x, out_dtype):
    """largest (|got - ref| - u_out |ref|) / (2^-24 max(1, |x|)): the constant c of the GELU bound is pinned from it"""
    u = 2.0 ** -8 if out_dtype == BF16 else 2.0 ** -24
    err = (got.double() - ref).abs() - u * ref.abs()
    return float((err / (2.0 ** -24 * x.abs().clamp(min=1.0))).max())


GELU_C = 16.0             # largest ratio on the MI355X 2.3618 (all GELU cases); 4 x that, rounded up to a power of two


# ---------------------------------------------------------------- epilogue lists
NONE = ('none', epi())
BN_RELU_A = ('bias_n+relu+alpha0.5', epi(bias_mode=1, act=1, alpha=0.5))
BN = ('bias_n', epi(bias_mode=1))
BN_RELU = ('bias_n+relu', epi(bias_mode=1, act=1))
BM = ('bias_m', epi(bias_mode=2))
BM_RELU = ('bias_m+relu', epi(bias_mode=2, act=1))
A2 = ('alpha2', epi(alpha=2.0))
GELU = ('gelu', epi(act=2))
BN_GELU = ('bias_n+gelu', epi(bias_mode=1, act=2))
ACT3 = ('act3', epi(act=3))
ACT4 = ('act4', epi(bias_mode=1, act=4))
ACC = ('accumulate', epi(accumulate=True, alpha=0.5))


def MDEV(v):
    return ('m_dev=%s' % v, epi(m_dev=v))            # v: 0, 1, 'half', 'M'


FULL = [NONE, BN_RELU_A, BM, ACT3, ACT4, ACC, MDEV(0), MDEV(1), MDEV('half'), MDEV('M')]   # the list of issue table 2
WHOLE = [NONE, BN_RELU_A, BM, GELU]                   # what the whole-tile kernels (q4, pp2, pp) take


# ---------------------------------------------------------------- the case table
# One entry per launch path of tell_gemm_nt.  shape: (M, N, K) at 256 CUs; with scale_n the N of the entry is multiplied
# by n_cu / 256 (whole rounds of 256 x 256 tiles on any CU count that is a multiple of 16).  plan: the label
# tell_gemm_nt_plan must give under `opts` for every epilogue of the entry; kernel: the instantiation a kernel trace shows.
# lda_pad / ldb_pad / ldc_pad: row stride minus width (A is a column slice of a wider matrix by default, B contiguous;
# both sit between guard bands).  The small and register-staged paths run FULL; the 11-bit flavour runs the plain
# product only, because its sums leave no headroom for an epilogue.
def nt(id, shape, plan, kernel, epis, opts=None, in_dtype=BF16, out_dtype=BF16, scale_n=False, **kw):
    d = dict(id=id, entry='tell_gemm_nt', shape=shape, plan=plan, kernel=kernel, epis=epis, opts=opts or {},
             in_dtype=in_dtype, out_dtype=out_dtype, scale_n=scale_n, lda_pad=8, ldb_pad=0, ldc_pad=8, c_off=0, wide=False,
             seed=0)
    d.update(kw)
    return d


Q4 = ('gemm_nt_q4_kernel<bf16,256,256>', 'gemm_nt_q4_kernel')
Q4E = ('gemm_nt_q4e_kernel<bf16,256,256>', 'gemm_nt_q4e_kernel')
PP2 = ('gemm_nt_pp2_kernel<bf16,256,256>', 'gemm_nt_pp2_kernel<0, false>')
PP = ('gemm_nt_pp_kernel<bf16,256,256>', 'gemm_nt_pp_kernel<unsigned short>')


def GLDS(out, bm, bn, extra=', false, 2'):
    o = 'bf16' if out == BF16 else 'f32'
    t = 'unsigned short' if out == BF16 else 'float'
    wm, wn = {(256, 192): (4, 2), (256, 256): (2, 4), (256, 128): (4, 2), (128, 128): (2, 2), (64, 64): (2, 2)}[(bm, bn)]
    return ('gemm_nt_glds_kernel<%s,%d,%d>' % (o, bm, bn), 'gemm_nt_glds_kernel<%s, %d, %d, %d, %d%s>' % (t, bm, bn, wm, wn, extra))


def REG(inp, out, bm, bn):
    n = {BF16: 'bf16', F32: 'f32'}
    t = {BF16: 'unsigned short', F32: 'float'}
    return ('gemm_nt_kernel<%s,%s,%d,%d>' % (n[inp], n[out], bm, bn), 'gemm_nt_kernel<%s, %s, %d, %d' % (t[inp], t[out], bm, bn))


def S64(out):
    return ('gemm_nt_s64_kernel<%s,64,64>' % ('bf16' if out == BF16 else 'f32'),
            'gemm_nt_s64_kernel<%s, false, 4>' % ('unsigned short' if out == BF16 else 'float'))


NO_Q4 = dict(gemm_q4=0)
NO_PP2 = dict(gemm_q4=0, gemm_pp2=0)
G64 = dict(gemm_s64=0)

CASES = [
    # ---- whole rounds of 256 x 256 bf16 tiles, K % 128 == 0: gemm_nt_q4_kernel
    nt('q4 K=128', (4096, 4096, 128), *Q4, WHOLE, scale_n=True),
    nt('q4 K=256', (4096, 4096, 256), *Q4, [NONE, BN_RELU_A], scale_n=True),
    nt('q4 K=384', (4096, 4096, 384), *Q4, [NONE, BN_GELU], scale_n=True),
    nt('q4 two tiles static', (8192, 4096, 256), *Q4, [NONE, BM], dict(q4_dynamic=0), scale_n=True),
    nt('q4 two tiles queue', (8192, 4096, 256), *Q4, [NONE, BM], dict(q4_dynamic=1), scale_n=True),
    nt('q4 partial round', (3072, 4096, 128), *Q4, [NONE, BN_RELU_A], scale_n=True),
    nt('q4 var 1', (4096, 4096, 256), *Q4, [BN_RELU_A], dict(q4_var=1), scale_n=True),
    nt('q4 var 2', (4096, 4096, 256), *Q4, [BN_RELU_A], dict(q4_var=2), scale_n=True),
    nt('q4 strided', (4096, 4096, 128), *Q4, [NONE, BN_RELU_A], scale_n=True, lda_pad=64, ldb_pad=128, ldc_pad=24),
    # ---- the same with the epilogue inside the next K loop: gemm_nt_q4e_kernel (bias[n], K >= 832)
    nt('q4e', (8192, 4096, 896), *Q4E, [BN, BN_RELU], scale_n=True),
    nt('q4e everywhere', (4096, 4096, 896), *Q4E, [BN, BN_RELU, BN_GELU], dict(gemm_q4e=2), scale_n=True),
    nt('q4e queue', (8192, 4096, 896), *Q4E, [BN_RELU], dict(q4_dynamic=1), scale_n=True),
    # ---- K % 128 != 0 (or gemm_q4 = 0): gemm_nt_pp2_kernel
    nt('pp2 K=64', (4096, 4096, 64), *PP2, [NONE, BN_GELU, BM_RELU], scale_n=True),
    nt('pp2 K=192', (4096, 4096, 192), *PP2, [NONE, BM_RELU], scale_n=True),
    nt('pp2 K=320', (4096, 4096, 320), *PP2, [NONE, BN_GELU], scale_n=True),
    nt('pp2 for q4', (4096, 4096, 128), *PP2, [NONE, BM_RELU], NO_Q4, scale_n=True),
    nt('pp2 static', (8192, 4096, 64), *PP2, [NONE, BM_RELU], dict(pp2_dynamic=0), scale_n=True),
    nt('pp2 queue', (8192, 4096, 64), *PP2, [NONE, BM_RELU], dict(pp2_dynamic=1), scale_n=True),
    nt('pp2=1 two rounds', (8192, 4096, 64), *PP2, [NONE], dict(gemm_pp2=1), scale_n=True),
    nt('pp2 grid 64', (4096, 4096, 64), *PP2, [NONE, BM_RELU], dict(pp2_grid=64), scale_n=True),
    # ---- one workgroup per tile: gemm_nt_pp_kernel
    nt('pp2=1 one round', (4096, 4096, 64), *PP, [NONE], dict(gemm_pp2=1), scale_n=True),
    nt('pp K=64', (4096, 4096, 64), *PP, [NONE, BN_RELU], NO_PP2, scale_n=True),
    nt('pp K=192', (4096, 4096, 192), *PP, [NONE, BN_RELU], NO_PP2, scale_n=True),
    nt('pp persistent', (8192, 4096, 64), *PP, [NONE, BN_RELU], dict(gemm_q4=0, gemm_pp2=0, gemm_persist=1), scale_n=True),
    # ---- 256 x 192
    nt('glds 256x192', (8192, 1536, 64), *GLDS(BF16, 256, 192), [NONE, BN, ACT4], scale_n=True),
    nt('glds 256x192 f32', (8192, 1536, 64), *GLDS(F32, 256, 192), [NONE, BN, ACT4], out_dtype=F32, scale_n=True),
    nt('glds 256x192 ragged', (8190, 1536, 64), *GLDS(BF16, 256, 192), [NONE, BN, ACT4], scale_n=True),
    nt('glds 256x192 forced', (8192, 1536, 64), *GLDS(BF16, 256, 192), [NONE], dict(gemm_tile=9), scale_n=True),
    # ---- lockstep 256 x 256
    nt('glds 256x256 f32', (4096, 4096, 64), *GLDS(F32, 256, 256), [NONE, BN_RELU_A, ACT3], out_dtype=F32, scale_n=True),
    nt('glds 256x256 ragged', (4090, 4090, 64), *GLDS(BF16, 256, 256), [NONE, BN_RELU_A, BM, ACT3, ACT4]),
    nt('glds 256x256 m_dev', (4096, 4096, 64), *GLDS(BF16, 256, 256), [MDEV(0), MDEV(1), MDEV('half'), MDEV('M'), ACT3, ACT4],
       scale_n=True),
    nt('glds 256x256 forced', (4096, 4096, 64), *GLDS(BF16, 256, 256), [NONE, BN_RELU_A], dict(gemm_tile=5), scale_n=True),
    # (gemm_tile = 7 is "the default choice without the ping-pong kernels": whole rounds go to the lockstep kernel, an
    #  accumulating launch of the same shape to 128 x 128)
    nt('glds 256x256 no pp', (4096, 4096, 64), *GLDS(BF16, 256, 256), [NONE, BN_RELU_A], dict(gemm_tile=7), scale_n=True),
    nt('glds 128 no pp', (4096, 4096, 64), *GLDS(BF16, 128, 128), [ACC], dict(gemm_tile=7), scale_n=True),
    # ---- 128 x 128 (and the opt-in 256 x 128)
    nt('glds 128', (2048, 2048, 64), *GLDS(BF16, 128, 128), FULL),
    nt('glds 128 f32', (2048, 2048, 64), *GLDS(F32, 128, 128), FULL, out_dtype=F32),
    nt('glds 128 ragged', (2050, 2046, 64), *GLDS(BF16, 128, 128), FULL),
    nt('glds 256x128', (4096, 4096, 64), *GLDS(BF16, 256, 128), [NONE, BN_RELU_A, ACT3], dict(gemm_tile=2), scale_n=True),
    nt('glds 256x128 f32', (4096, 4096, 64), *GLDS(F32, 256, 128), [NONE, ACT4], dict(gemm_tile=2), out_dtype=F32, scale_n=True),
    # ---- small: gemm_nt_s64_kernel
    nt('s64', (512, 64, 1024), *S64(BF16), FULL),
    nt('s64 f32', (512, 64, 1024), *S64(F32), FULL, out_dtype=F32),
    nt('s64 ragged', (520, 72, 1088), *S64(BF16), FULL),
    nt('s64 ragged f32', (520, 72, 1088), *S64(F32), FULL, out_dtype=F32),
    nt('s64 K=64', (512, 64, 64), *S64(BF16), FULL, dict(gemm_s64=2)),
    # ---- small direct-to-LDS 64 x 64, rings 2 / 3 / 4
    nt('glds 64 ring 2', (512, 64, 64), *GLDS(BF16, 64, 64, ', false, 2'), FULL, G64),
    nt('glds 64 ring 4', (512, 128, 512), *GLDS(BF16, 64, 64, ', false, 4'), FULL, G64),
    nt('glds 64 ring 3', (512, 128, 512), *GLDS(BF16, 64, 64, ', false, 3'), FULL, dict(gemm_s64=0, gemm_ring=3)),
    nt('glds 64 ragged', (520, 72, 64), *GLDS(BF16, 64, 64, ', false, 2'), FULL, G64),
    nt('glds 64 ragged f32', (520, 72, 512), *GLDS(F32, 64, 64, ', false, 4'), FULL, G64, out_dtype=F32),
    nt('glds 64 ring 2 f32', (512, 64, 64), *GLDS(F32, 64, 64, ', false, 2'), FULL, G64, out_dtype=F32),
    nt('glds 64 ring 3 f32', (512, 128, 512), *GLDS(F32, 64, 64, ', false, 3'), FULL,
       dict(gemm_s64=0, gemm_ring=3), out_dtype=F32),
    # ---- register-staged kernels
    nt('reg 64 tiny', (5, 8, 8), *REG(BF16, BF16, 64, 64), FULL),
    nt('reg 64 odd', (37, 70, 72), *REG(BF16, BF16, 64, 64), FULL),
    nt('reg 64 two tiles', (130, 70, 96), *REG(BF16, BF16, 64, 64), FULL),
    nt('reg 64 f32 out', (130, 70, 96), *REG(BF16, F32, 64, 64), FULL, out_dtype=F32),
    nt('reg 64 not small', (512, 64, 64), *REG(BF16, BF16, 64, 64), FULL, dict(gemm_small=0, gemm_s64=0)),
    nt('reg 64 scalar stores', (37, 70, 72), *REG(BF16, BF16, 64, 64), FULL, ldc_pad=3),
    nt('reg 64 scalar stores N', (37, 67, 72), *REG(BF16, BF16, 64, 64), FULL, ldc_pad=9),
    # N % 4 == 0 and ldc % 4 == 0: the base address alone (2 bytes off 8-byte alignment) sends the stores down the scalar path
    nt('reg 64 C off alignment', (37, 72, 72), *REG(BF16, BF16, 64, 64), FULL, c_off=1),
    nt('reg 128', (2048, 2048, 72), *REG(BF16, BF16, 128, 128), FULL),
    nt('reg 128 f32 out', (2048, 2048, 72), *REG(BF16, F32, 128, 128), FULL, out_dtype=F32),
    nt('reg 128 ragged', (2050, 2046, 72), *REG(BF16, BF16, 128, 128), FULL),
    nt('reg 256x128', (4096, 2048, 72), *REG(BF16, BF16, 256, 128), FULL),
    nt('reg 256x128 f32 out', (4096, 2048, 72), *REG(BF16, F32, 256, 128), FULL, out_dtype=F32),
    # ---- fp32 operands
    nt('f32 64', (37, 70, 36), *REG(F32, F32, 64, 64), FULL, in_dtype=F32, out_dtype=F32),
    nt('f32 64 bf16 out', (37, 70, 36), *REG(F32, BF16, 64, 64), FULL, in_dtype=F32),
    nt('f32 K=4', (37, 70, 4), *REG(F32, F32, 64, 64), FULL, in_dtype=F32, out_dtype=F32),
    nt('f32 11-bit', (130, 70, 4), *REG(F32, F32, 64, 64), [NONE], in_dtype=F32, out_dtype=F32, wide=True),
    nt('f32 128', (2048, 2048, 32), *REG(F32, F32, 128, 128), FULL, in_dtype=F32, out_dtype=F32),
    nt('f32 128 bf16 out', (2048, 2048, 32), *REG(F32, BF16, 128, 128), FULL, in_dtype=F32),
    nt('f32 128 11-bit', (2048, 2048, 4), *REG(F32, F32, 128, 128), [NONE], in_dtype=F32, out_dtype=F32, wide=True),
]


def case_shape(c, n_cu=256):
    M, N, K = c['shape']
    if c['scale_n']:
        assert (N * n_cu) % 256 == 0
        N = N * n_cu // 256
    return M, N, K


def resolve(e, M):
    """m_dev 'half' / 'M' -> a number"""
    e = dict(e)
    if e['m_dev'] == 'half':
        e['m_dev'] = M // 2
    elif e['m_dev'] == 'M':
        e['m_dev'] = M
    return e


def case_amplitude(c, n_cu=256):
    M, N, K = case_shape(c, n_cu)
    return 2047 if c['wide'] else amplitude(K, HEADROOM)


def case_gelu_alpha(c, n_cu=256):
    return gelu_alpha(case_shape(c, n_cu)[2], case_amplitude(c, n_cu))
