"""float64 reference of DynamicConv forward / backward and the element-wise error bounds the kernels are held to
(DESIGN.md section 23).  numpy only; nothing here comes from oracle/.

    taps = softmax_K(logits[t,b,h,:])                               (float64)
    y[t,b,h,c]  = sum_k taps[k] keep[k] x[t-(K-1)+k, b, h, c]         x[< 0] = 0
    dw[t,b,h,k] = keep[k] <dy[t,b,h,:], x[t-(K-1)+k,b,h,:]>
    dlogits     = w (dw - sum_j w_j dw_j)
    dx[t',b,h,c] = sum_k taps[t'+(K-1)-k][k] keep[t'+(K-1)-k][k] dy[t'+(K-1)-k, b, h, c]

keep is 0 or 1/(1-p), element ((t*B+b)*H+h)*K+k of tell_amd.rng.keep_mask - the index the kernels hash.  Every function
also returns the sum of the ABSOLUTE values of the terms the kernel adds up (S below): an fp32 sum of n terms is off by
at most about n 2^-24 S whatever the order of the additions, so a bound built on S holds for the tree-shaped wave
reductions and the sequential loops alike, and stays tight where terms cancel.

Bound of one output element:   u_out |ref|  +  c gamma 2^-24 S  +  2^-126 (1 + S)
  u_out   half an ulp of the stored type: 2^-8 bf16 (f2bf rounds to nearest even), 2^-24 fp32
  gamma   operation count of the element: y and taps K + 8 + D (D = largest max - min of a logit row: the argument
          scaling inside __expf costs about D ulps), dx K + 8, dlogits R + K + 8
  c       the one constant that is measured, not derived (the accuracy of __expf is stated nowhere): four times the
          largest observed (|got - ref| - u_out |ref|) / (gamma 2^-24 S) over the whole GPU grid of
          tests/test_gpu_dynconv.py, rounded up to a power of two.  Measured on the MI355X and pinned in C below.
  2^-126  the smallest normal fp32: below it the format has no relative precision (and __expf flushes), which only
          matters for taps that underflow (logit spread > 87)
Inputs are rounded to the compute dtype BEFORE they reach the reference, so it sees the values the kernel sees; the
backward takes the taps as given (the GPU tests pass the kernel's own fp32 taps), so it is not charged the softmax
error.

Measured on the MI355X, largest ratio over the grid (fp32 and bf16, p = 0 and 0.1, the dispatchers' choice and the
forced wave-per-row path) -> pinned c = 4 x that, rounded up to a power of two:
    y 0.2482 -> 1     taps 0.3321 -> 2     dx 0.1601 -> 1     dlogits 0.0414 -> 0.25
(logits x 30, D ~ 200, outside the grid: y 0.3256, taps 0.5322, dx 0.0658, dlogits 0.0253 - inside the same c.)
"""
import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -126
U_OUT = {'float32': 2.0 ** -24, 'bfloat16': 2.0 ** -8}

# largest observed ratio (fp32 and bf16, every grid shape, p = 0 and 0.1, both launch paths) and the pinned constant
MEASURED = {'y': 0.2482, 'taps': 0.3321, 'dx': 0.1601, 'dlogits': 0.0414}
C = {'y': 1.0, 'taps': 2.0, 'dx': 1.0, 'dlogits': 0.25}

MUTANTS = ('k_lo', 'n_src', 'dx_no_keep', 'keep_late')


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def softmax_taps(logits, H, K):
    lg = _f64(logits)
    T, B = lg.shape[:2]
    lg = lg.reshape(T, B, H, K)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def logit_spread(logits, H, K):
    """D: the largest (max - min) of one row of K tap logits."""
    lg = _f64(logits)
    lg = lg.reshape(lg.shape[0], lg.shape[1], H, K)
    return float((lg.max(-1) - lg.min(-1)).max()) if lg.size else 0.0


def _padded(x, H, K):
    """[T,B,C] -> [T+K-1,B,H,R] with K-1 rows of zeros in front: tap k of row t reads row t + k."""
    x = _f64(x)
    T, B, Cn = x.shape
    xp = np.zeros((T + K - 1, B, H, Cn // H))
    xp[K - 1:] = x.reshape(T, B, H, Cn // H)
    return xp


def forward(x, logits, H, K, keep=None, taps=None, mutant=None):
    """-> y [T,B,C], A [T,B,C] (sum of |terms|), taps [T,B,H,K].  `taps` given: used instead of softmax(logits).
    mutant 'k_lo': the first live tap of every row is skipped (k_lo one too large)."""
    x = _f64(x)
    T, B, Cn = x.shape
    w = softmax_taps(logits, H, K) if taps is None else _f64(taps).reshape(T, B, H, K)
    wk = w if keep is None else w * _f64(keep).reshape(T, B, H, K)
    xp = _padded(x, H, K)
    y = np.zeros((T, B, H, Cn // H))
    A = np.zeros_like(y)
    k_lo = np.maximum(K - 1 - np.arange(T), 0)
    for k in range(K):
        term = wk[..., k, None] * xp[k:k + T]
        if mutant == 'k_lo':
            term[k_lo == k] = 0.0
        y += term
        A += np.abs(term)
    return y.reshape(T, B, Cn), A.reshape(T, B, Cn), w


def backward(x, dy, taps, keep=None, dx0=None, mutant=None):
    """-> dlogits [T,B,H*K], dx [T,B,C], S_dlogits, S_dx.  dx0: what dx held before (dx_accumulate = 1).
    mutants: 'n_src' (the last source row of every dx row is skipped), 'dx_no_keep' (no DropConnect factor in dx),
    'keep_late' (DropConnect applied after the softmax backward instead of before it)."""
    x, dy, w = _f64(x), _f64(dy), _f64(taps)
    T, B, Cn = x.shape
    H, K = w.shape[2], w.shape[3]
    R = Cn // H
    kp = np.ones_like(w) if keep is None else _f64(keep).reshape(T, B, H, K)
    xp = _padded(x, H, K)
    dyr = dy.reshape(T, B, H, R)
    dwr = np.zeros_like(w)
    Sr = np.zeros_like(w)
    for k in range(K):
        prod = dyr * xp[k:k + T]
        dwr[..., k] = prod.sum(-1)
        Sr[..., k] = np.abs(prod).sum(-1)
    dw, S = kp * dwr, kp * Sr
    if mutant == 'keep_late':
        dl = kp * w * (dwr - (w * dwr).sum(-1, keepdims=True))
    else:
        dl = w * (dw - (w * dw).sum(-1, keepdims=True))
    S_dl = w * (S + (w * S).sum(-1, keepdims=True))
    wk = w if mutant == 'dx_no_keep' else w * kp
    dx = np.zeros((T, B, H, R))
    S_dx = np.zeros_like(dx)
    n_src = np.minimum(T - np.arange(T), K)
    for j in range(min(K, T)):                    # source row t' + j reaches row t' through tap K - 1 - j
        term = wk[j:, :, :, K - 1 - j, None] * dyr[j:]
        if mutant == 'n_src':
            term[n_src[:T - j] - 1 == j] = 0.0
        dx[:T - j] += term
        S_dx[:T - j] += np.abs(term)
    dx, S_dx = dx.reshape(T, B, Cn), S_dx.reshape(T, B, Cn)
    if dx0 is not None:
        dx = dx + _f64(dx0)
        S_dx = S_dx + np.abs(_f64(dx0))
    return dl.reshape(T, B, H * K), dx, S_dl.reshape(T, B, H * K), S_dx


def gamma(out, K, R=0, D=0.0):
    """operation count of one element of output `out`"""
    return {'y': K + 8 + D, 'taps': K + 8 + D, 'dx': K + 8, 'dlogits': R + K + 8}[out]


def bound(out, ref, S, dtype, gam, c=None):
    """element-wise bound of output `out` ('y', 'taps', 'dx', 'dlogits'); dtype 'float32' / 'bfloat16' is the STORED
    type (taps are always float32); for taps S is the reference itself."""
    c = C[out] if c is None else c
    ref, S = _f64(ref), _f64(S)
    return U_OUT[dtype] * np.abs(ref) + c * gam * EPS * S + TINY * (1.0 + S)


def ratio(got, ref, S, dtype, gam):
    """largest (|got - ref| - u_out |ref|) / (gamma 2^-24 S): the figure c is pinned from (0 where S = 0)."""
    got, ref, S = _f64(got), _f64(ref), _f64(S)
    num = np.abs(got - ref) - U_OUT[dtype] * np.abs(ref) - TINY * (1.0 + S)
    den = gam * EPS * S
    ok = den > 0
    return float((num[ok] / den[ok]).max()) if ok.any() else 0.0


def keep_factors(seed, salt, T, B, H, K, p):
    """[T,B,H,K] float64 of 0 or 1/(1-p) (the kernels' fp32 value of it), or None for p = 0."""
    if not p > 0:
        return None
    from tell_amd import rng
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return rng.keep_mask(seed, salt, T * B * H * K, p).astype(np.float64).reshape(T, B, H, K) * float(inv)


# ---------------------------------------------------------------- the shapes both test files walk
# (T, B, H, K, R): the smallest that reach each launch path of tell_dynconv_fwd / tell_dynconv_bwd
GRID_LDS = [(1, 2, 3, 1, 64), (1, 3, 2, 31, 64), (5, 2, 3, 31, 64), (32, 3, 2, 3, 64), (33, 2, 3, 31, 64),
            (63, 3, 2, 32, 64), (64, 2, 3, 32, 64), (64, 3, 2, 1, 64)]          # LDS forward + LDS backward
GRID_LDS_FWD = [(65, 2, 3, 31, 64), (128, 3, 2, 32, 64)]                        # LDS forward + wave-per-row backward
# wave-per-row both ways: T > 128, K > 32, head widths other than 64 (R > 64: the c0 loop).  B = H = 3 and an odd T:
# the wave count is no multiple of the 4 waves of a workgroup (at T = 12 every B, H gives a multiple of 4)
GRID_ROW = [(129, 3, 3, 15, 64), (41, 3, 3, 33, 64), (67, 3, 3, 64, 64), (9, 3, 3, 64, 64)] + \
           [(T, 3, 3, K, R) for R in (16, 96, 128) for T, K in ((9, 7), (12, 31))]
GRID = GRID_LDS + GRID_LDS_FWD + GRID_ROW
SEED, SALT = 9, 101


def case_inputs(T, B, H, K, R, dtype, logit_scale=1.0, seed=0):
    """x, logits, dy, dx0 as torch CPU tensors ALREADY rounded to `dtype` (torch.float32 / torch.bfloat16)."""
    import torch
    g = torch.Generator().manual_seed(1000 * T + 10 * K + R + seed)
    x = torch.randn(T, B, H * R, generator=g).to(dtype)
    lg = (torch.randn(T, B, H * K, generator=g) * logit_scale).to(dtype)
    dy = torch.randn(T, B, H * R, generator=g).to(dtype)
    dx0 = torch.randn(T, B, H * R, generator=g).to(dtype)
    return x, lg, dy, dx0


def np64(t):
    return t.detach().double().cpu().numpy()
