"""float64 reference of the three kernels every generation step runs on (csrc/decode.hip: attn_decode_kernel<NQ, LSE>,
attn_decode_packed_kernel, dynconv_step_kernel<R, NK, HAS_BACK, KB>), the element-wise bounds they are held to and the case
tables that tests/test_decode_ref_host.py, tests/test_gpu_attn_decode.py and tests/test_gpu_dynconv_step.py walk (DESIGN.md
section 33).  numpy only; nothing here comes from oracle/.  Inputs are rounded to bf16 BEFORE they reach a function.

Every function returns, beside each value, the sum of the ABSOLUTE values of the terms the kernel adds up for it (S_*).
Bound of one output element, as in sections 23 and 26:

    u_out |ref|  +  c gamma 2^-24 S  +  2^-126 (1 + S)        (+ 2^-8 S_out on the packed path, see below)

u_out = 2^-8 for the bf16 stores (out, y), 2^-24 for lse2; gamma = the element's operation count, read off the kernel (the
table below); c = the one measured number per output (MEASURED, C).  Every function takes dt (np.float64: the reference;
np.float32: the same formulas with every product, exp2 / exp and sequential sum rounded to fp32 - the emulation the host
test holds to the bounds at c = 1) and a mutant name (MUTANTS: wrong-answer variants that must break a bound).

gamma.  A probability exp2(s - lse2) has the relative error of its argument: the score is an fp32 dot product of 64 terms,
off by at most 64 2^-24 L with L = sum_d |q_d k_d|, times log2 e (one rounding, <= |s| 2^-24 <= L 2^-23), and the
subtraction in front of v_exp_f32 costs |s - lse2| ulps.  So   gP = 8 + spread + 64 Lmax   (spread = largest |s - lse2| over
the live keys of the case, in base 2; Lmax = largest L) is the relative error count of one probability on a GIVEN lse2; on
the kernel's own sum it carries 2 gP.  n = live keys of the row (the two virtual keys included).

    attention (VALU)   out: 2 n + 8 + 2 gP        lse2: n + 8 + gP   (S = 1 + |lse2|)
    attention (packed) out: 2 n + 8 + 2 gP, and a DERIVED additive term 2^-8 S_out: every probability is rounded to bf16
                       (unit roundoff 2^-8) in front of the second MFMA while the row sum l keeps the unrounded ones, so
                       |sum_s (bf16(p_s) - p_s) v_s| / l <= 2^-8 sum_s p_s |v_s| / l = 2^-8 S_out.  Not folded into c.
    DynamicConv step   a tap logit comes off the matrix cores: C products, C / 4 per wave, and the 4-way fold of the waves'
                       partial tiles through LDS: C + 4 additions at most, so   gT = 8 + spread + (C + 4) Lmax   (natural
                       log here: __expf; L = sum_c |x_c w_c|) and   y: 2 K + 8 + 2 gT   (K fused multiply-adds, K
                       additions of the tap sum).

Definitions the kernels leave open are stated here: a (row, head) without any live key gives out = +0.0 and lse2 = -inf
(what the kernel writes), not NaN.

Measured on the MI355X: MEASURED and C below, and DESIGN.md section 33.
"""
import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -126
U_OUT = {'float32': 2.0 ** -24, 'bfloat16': 2.0 ** -8}
PK_PROB = 2.0 ** -8                      # the derived packed-probability term (times S_out)
AD_MAXS = 2048
LOG2E = 1.4426950408889634

# largest observed (|got - ref| - u_out |ref| [- 2^-8 S_out, packed]) / (gamma 2^-24 S) over the GPU grids of
# tests/test_gpu_attn_decode.py and tests/test_gpu_dynconv_step.py on the MI355X, and the pinned constant: four times that,
# rounded up to a power of two; 2^-10 where the ratio never left u_out |ref| (ratio <= 0).  An output missing from MEASURED
# is not pinned: the GPU test then fails with the measured ratio in its message.
MEASURED = {'ad_out_nq1': 0.0, 'ad_out_nq2': 0.0, 'ad_out_nq4': 0.000376, 'ad_lse2': 0.002574, 'pk_out': 0.0,
            'dcs_y': 0.000119}


def _pin(r):
    return 2.0 ** -10 if r <= 0 else 2.0 ** int(np.ceil(np.log2(4.0 * r)))


C = {k: _pin(v) for k, v in MEASURED.items()}

OUTPUTS = ('ad_out_nq1', 'ad_out_nq2', 'ad_out_nq4', 'ad_lse2', 'pk_out', 'dcs_y')

ATTN_MUTANTS = ('drop_last_key', 'tail_key_live', 'mask_by_row', 'cache_by_row', 'first_q_for_all', 'no_zero_key',
                'bias_v_as_bias_k', 'drop_wave3', 'drop_second_trip', 'no_rescale', 'ctx_swap', 'lse_natural')
PK_MUTANTS = ('pk_block_round_robin', 'pk_v_perm')
DCS_MUTANTS = ('dcs_tap_reversed', 'dcs_plane_off_by_one', 'dcs_back_ignored', 'dcs_softmax_over_32', 'dcs_second_tile_lost')
MUTANTS = ATTN_MUTANTS + PK_MUTANTS + DCS_MUTANTS


def _sum(a, axis, dt):
    """sum along axis; fp32: sequential (np.sum adds pairwise; the kernels' loops do not)"""
    a = np.asarray(a, dtype=dt)
    if dt is np.float64:
        return a.sum(axis)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), dtype=dt)
    return np.take(np.add.accumulate(a, axis=axis, dtype=dt), -1, axis=axis)


def bf16_round(a):
    """fp32 -> the nearest bf16 (ties to even), as fp32"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7fff)
    return ((u + r) & np.uint32(0xffff0000)).view(np.float32)


def bound(out, ref, S, dtype, gam, c=None, extra=0.0):
    c = C[out] if c is None else c
    ref, S = np.asarray(ref, np.float64), np.asarray(S, np.float64)
    return U_OUT[dtype] * np.abs(ref) + c * gam * EPS * S + TINY * (1.0 + S) + extra


def ratio(got, ref, S, dtype, gam, extra=0.0):
    """largest (|got - ref| - u_out |ref| - extra) / (gamma 2^-24 S) over the finite reference elements with S > 0"""
    got, ref, S = (np.asarray(a, np.float64) for a in (got, ref, S))
    ref, S = np.broadcast_to(ref, got.shape), np.broadcast_to(S, got.shape)
    extra = np.broadcast_to(np.asarray(extra, np.float64), got.shape)
    ok = np.isfinite(ref) & (gam * EPS * S > 0)
    if not ok.any():
        return 0.0
    num = np.abs(got - ref)[ok] - U_OUT[dtype] * np.abs(ref[ok]) - TINY * (1.0 + S[ok]) - extra[ok]
    return float((num / (gam * EPS * S[ok])).max())


def np64(t):
    return t.detach().double().cpu().numpy()


# ---------------------------------------------------------------- one-query attention over a cached context
def nq_of(beams):
    """hypotheses per workgroup of tell_attn_decode's choice of instantiation"""
    return 1 if beams == 1 else (2 if beams == 2 else 4)


def attn_decode(q, k, v, mask, bias_k, bias_v, has_zero, beams, dt=np.float64, mutant=None, packed=False):
    """q [B, H 64] (scaled), k, v [S, B / beams, H 64], mask [B / beams, S] (non-zero = padding) or None, bias_k / bias_v
    [H 64] or None -> dict out, S_out [B, H 64], lse2, S_lse [B, H], spread, Lmax, n, w (the unnormalised probabilities
    [B, H, S + 2]: what the coverage facts of the host test look at) and s2 (the base-2 scores, -inf where dead).
    Hypothesis row b reads the cache and the mask row of sample b // beams.  Two more keys, never masked: bias_k (value
    bias_v, or zeros) and, with has_zero, a key of score 0 and value 0.  packed: the matrix-core path - with dt fp32 the
    probabilities are rounded to bf16 in front of P V, the row sum is not."""
    q = np.asarray(q, dt)
    B, E = q.shape
    H, S, Bs = E // 64, np.shape(k)[0], B // beams
    rows = np.arange(B)
    smp = rows // beams
    csmp = rows % Bs if mutant == 'cache_by_row' else smp
    msmp = rows % Bs if mutant == 'mask_by_row' else smp
    qrow = rows
    if mutant == 'first_q_for_all':
        grp = 16 if packed else nq_of(beams)
        qrow = smp * beams + (rows % beams) // grp * grp
    qh = q[qrow].reshape(B, H, 64)
    kx, vx = np.zeros((B, H, S + 2, 64), dt), np.zeros((B, H, S + 2, 64), dt)
    live = np.zeros((B, S + 2), bool)
    if S:
        kx[:, :, :S] = np.asarray(k, dt).reshape(S, Bs, H, 64).transpose(1, 2, 0, 3)[csmp]
        vx[:, :, :S] = np.asarray(v, dt).reshape(S, Bs, H, 64).transpose(1, 2, 0, 3)[csmp]
        live[:, :S] = True if mask is None else (np.asarray(mask).reshape(Bs, S)[msmp] == 0)
    if bias_k is not None:
        kx[:, :, S] = np.asarray(bias_k, dt).reshape(H, 64)
        live[:, S] = True
        bv = bias_k if mutant == 'bias_v_as_bias_k' else bias_v
        if bv is not None:
            vx[:, :, S] = np.asarray(bv, dt).reshape(H, 64)
    live[:, S + 1] = bool(has_zero) and mutant != 'no_zero_key'
    S8 = (S + 7) & ~7
    mult = np.ones(S + 2, dt)
    if mutant == 'drop_last_key' and S:
        live[:, S - 1] = False
    if mutant == 'tail_key_live' and S and not packed:
        mult[S - 1] = 1 + S8 - S
    if mutant == 'drop_wave3' and S8 == 32 and not packed:
        live[:, 24:S] = False
    if mutant == 'drop_second_trip' and not packed:
        live[:, 128:S] = False
    if mutant == 'pk_block_round_robin' and packed:
        live[:, 128:] = False
    if mutant == 'pk_v_perm' and packed:
        Sp = -(-(S + 2) // 32) * 32
        vp = np.zeros((B, H, Sp, 64), dt)
        vp[:, :, :S + 2] = vx
        vx = vp[:, :, np.arange(Sp) ^ 16][:, :, :S + 2]
    if dt is np.float64:
        sc, L = np.einsum('bhd,bhsd->bhs', qh, kx), np.einsum('bhd,bhsd->bhs', np.abs(qh), np.abs(kx))
    else:
        prod = qh[:, :, None, :] * kx
        sc, L = _sum(prod, -1, dt), _sum(np.abs(prod), -1, dt)
    s2 = (sc * dt(LOG2E)).astype(dt)
    s2 = np.where(live[:, None, :], s2, -np.inf).astype(dt)
    m = s2.max(-1)
    has = np.isfinite(m)
    ms = np.where(has, m, 0.0).astype(dt)
    with np.errstate(all='ignore'):
        if mutant == 'no_rescale':
            # keys are absorbed in blocks (a trip of 128 keys, the virtual keys last; packed: 32 keys) against the running
            # maximum of the blocks so far, and what was absorbed before the maximum moved is never scaled down
            blk = np.arange(S + 2) // (32 if packed else 128)
            if not packed:
                blk[S:] = blk[:S].max() + 1 if S else 0
            mrun = np.full(s2.shape[:2] + (blk.max() + 1,), -np.inf, dt)
            for i in range(blk.max() + 1):
                bm = s2[:, :, blk == i].max(-1)
                mrun[:, :, i] = np.maximum(bm, mrun[:, :, i - 1]) if i else bm
            at = mrun[:, :, blk]
            w = np.exp2(s2 - np.where(np.isfinite(at), at, 0.0)).astype(dt)
        else:
            w = np.exp2(s2 - ms[..., None]).astype(dt)
        wm = (w * mult).astype(dt)
        l = _sum(wm, -1, dt)
        wv = wm
        if packed and dt is np.float32:
            wv = bf16_round(wm)
        if dt is np.float64:
            o, so = np.einsum('bhs,bhsd->bhd', wv, vx), np.einsum('bhs,bhsd->bhd', wv, np.abs(vx))
        else:
            t = wv[..., None] * vx
            o, so = _sum(t, 2, dt), np.abs(np.asarray(t, np.float64)).sum(2)
        ls = np.where(has, l, 1.0).astype(dt)
        out = np.where(has[..., None], o / ls[..., None], 0.0).astype(dt)
        S_out = np.where(has[..., None], so / np.asarray(ls, np.float64)[..., None], 0.0)
        lse2 = np.where(has, ms + np.log2(ls), -np.inf).astype(dt)
        if mutant == 'lse_natural':
            lse2 = (lse2 * dt(np.log(2.0))).astype(dt)
        fin = live[:, None, :] & has[..., None]
        spread = float(np.abs(np.where(fin, s2 - np.where(has, lse2, 0.0)[..., None], 0.0)).max())
    Lmax = float(np.where(fin, L, 0.0).max())
    n = int((live * mult).sum(-1).max())
    return dict(out=out.reshape(B, E), S_out=S_out.reshape(B, E), lse2=lse2, S_lse=1.0 + np.abs(np.where(has, lse2, 0.0)),
                spread=spread, Lmax=Lmax, n=n, w=np.where(live[:, None, :], w, np.nan), s2=s2, has=has)


def attn_gamma(out, r):
    g = 8.0 + r['spread'] + 64.0 * r['Lmax']
    return {'out': 2 * r['n'] + 8 + 2 * g, 'lse': r['n'] + 8 + g}[out]


# ---------------------------------------------------------------- DynamicConv step
def dynconv_rule(M, H):
    """rows per workgroup the launcher picks"""
    if H * ((M + 3) // 4) <= 256:
        return 4
    return 8 if H * ((M + 7) // 8) <= 512 else 16


def dynconv_bucket(K):
    return 4 if K <= 4 else (8 if K <= 8 else (16 if K <= 16 else 32))


def tap_logits(x, wt, H, K, dt=np.float64):
    """x [M, C], wt [H K, C] -> logits, L [M, H, K]: x[m] . wt[h K + k] over all C channels (fp32: one term after the other)"""
    x, wt = np.asarray(x, dt), np.asarray(wt, dt)
    M, Cc = x.shape
    if dt is np.float64:
        lg, L = x @ wt.T, np.abs(x) @ np.abs(wt).T
    else:
        lg, L = np.zeros((M, H * K), dt), np.zeros((M, H * K), dt)
        for c in range(Cc):
            p = x[:, c, None] * wt[None, :, c]
            lg += p
            L += np.abs(p)
    return lg.reshape(M, H, K), L.reshape(M, H, K)


def dynconv_step(x, ring, wt, t, back, H, K, dt=np.float64, mutant=None, logits=None, inplace=False):
    """x [M, C] (this step's input), ring [K, M, C] (plane s mod K holds the input of step s; never written planes are
    zero), wt [H K, C], back [K - 1, M] (back[j - 1][m]: the slot, j steps ago, of the hypothesis now in slot m) or None
    (m itself) -> dict y, S_y [M, C], ring (the expected ring: plane t mod K is x, every other plane as before), spread,
    Lmax.  Taps: softmax_k of x[m] . wt[h K + k]; window: the K - 1 past rows, oldest first, then x.  logits: (logits, L) of
    tap_logits when the caller has them already; inplace: `ring` itself takes x (a step sequence does not copy K planes per
    step)."""
    x = np.asarray(x, dt)
    M, Cc = x.shape
    lg, L = tap_logits(x, wt, H, K, dt) if logits is None else logits
    lg = np.asarray(lg, dt)
    if mutant == 'dcs_softmax_over_32':
        lg = np.concatenate([lg, np.zeros((M, H, 32 - K), dt)], -1)
    mx = lg.max(-1, keepdims=True)
    e = np.exp(lg - mx).astype(dt)
    den = _sum(e, -1, dt)
    p = (e / den[..., None]).astype(dt)[..., :K]
    lse = mx[..., 0] + np.log(den)
    spread = float(np.abs(lg[..., :K] - lse[..., None]).max())
    if mutant == 'dcs_second_tile_lost':
        p = p.copy()
        p[..., 16:] = 0
    if mutant == 'dcs_tap_reversed':
        p = p[..., ::-1]
    rows = np.arange(M)
    win = []
    for j in list(range(1, K)) + [0]:                          # the kernel's order: 1 .. K - 1 steps ago, then x
        if j:
            slot = rows if back is None or mutant == 'dcs_back_ignored' else np.asarray(back)[j - 1]
            plane = ring[(t - j + (1 if mutant == 'dcs_plane_off_by_one' else 0)) % K]
            win.append(plane if slot is rows else plane[slot])
        else:
            win.append(x)
    pw = np.concatenate([p[..., K - 2::-1], p[..., K - 1:]], -1) if K > 1 else p      # tap of window row i: K - 1 - j
    if dt is np.float64:
        wn = np.stack(win).reshape(K, M, H, 64)
        y = np.einsum('kmhd,mhk->mhd', wn, pw).reshape(M, Cc)
        S_y = None if mutant else np.einsum('kmhd,mhk->mhd', np.abs(wn), pw).reshape(M, Cc)   # (a mutant is judged on the reference's S)
    else:
        y, S_y = np.zeros((M, Cc), dt), np.zeros((M, Cc))
        for i, w in enumerate(win):
            term = (np.repeat(pw[..., i], 64, axis=-1) * np.asarray(w, dt)).astype(dt)      # [M, H] -> [M, C]
            y = (y + term).astype(dt)
            S_y += np.abs(term)
    new = ring if inplace else np.array(ring, copy=True)
    new[t % K] = np.asarray(x, new.dtype)
    return dict(y=y, S_y=S_y, ring=new, spread=spread, Lmax=float(L.max()))


def dcs_gamma(r, Cc, K):
    g = 8.0 + r['spread'] + (Cc + 4.0) * r['Lmax']
    return 2 * K + 8 + 2 * g


# ================================================================ the case tables
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _gen(seed):
    import torch
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    import torch
    return torch.randn(*shape, generator=g)


def _bf(t):
    """a torch tensor rounded to bf16, as float64 numpy"""
    import torch
    return t.to(torch.bfloat16).double().numpy()


# One LAUNCH of the attention entry points: 1 to 4 contexts that share samples, H and the virtual keys.
#   S       cached keys per context (different per context; n_ctx < 4: the launcher fills the argument block from context 0)
#   wide    the beam width of the launch beside 1 (NQ = 1, and the LSE form) and 2 (NQ = 2): NQ = 4, packed: 17 two groups
#   masks   per context: none (null pointer) | ragged (sample b of n keeps S - (n - 1 - b) S // 4 keys) | s0 (sample 0 fully masked, the
#           others ragged) | last (only key S - 1 live) | first (only key 0 live)
#   virt    VALU entry points: kvz (bias_k + bias_v + zero key) | k (bias_k without bias_v, no zero key) | z (zero key only) |
#           none (with a fully masked sample: the exact-zero row).  The packed path always has kvz.
#   klay    what the case is BOUND-checked in: row ([S, B, E], null k_sh) | head ([B, H, S, 64] through strides) | inter (K and V
#           in one [S, B, 2E] buffer); the GPU test runs all three and requires bit-equal outputs
#   qwide / owide   q a column slice of a [B, 2E] buffer / out a column slice of [B, 4E]
#   scale   default (|score| a few units) | ascending (key norms grow with s: the running maximum moves in the last trip) |
#           peaked (one key outscores the rest by more than 150 in base 2: the other probabilities are 0 in fp32)
ATTN = [
    dict(id='S0_129', S=(0, 129), H=3, wide=3, masks=('none', 'ragged'), virt='kvz', klay='row'),
    dict(id='S1', S=(1,), H=16, wide=8, masks=('none',), virt='k', klay='head', qwide=True),
    dict(id='S7_8_9', S=(7, 8, 9), H=1, wide=3, masks=('ragged', 'none', 'last'), virt='z', klay='inter', owide=True),
    dict(id='S16_25', S=(16, 17, 24, 25), H=3, wide=4, masks=('none', 's0', 'ragged', 'last'), virt='kvz', klay='row',
         qwide=True, owide=True),
    dict(id='S30_33', S=(30, 31, 32, 33), H=16, wide=5, masks=('ragged', 'none', 'first', 's0'), virt='none', klay='head'),
    dict(id='S62_63', S=(62, 63), H=1, wide=8, masks=('s0', 'none'), virt='k', klay='inter'),
    dict(id='S126_128', S=(126, 127, 128), H=3, wide=16, masks=('last', 'ragged', 'none'), virt='z', klay='row'),
    dict(id='S257', S=(257,), H=1, wide=17, masks=('ragged',), virt='kvz', klay='head', owide=True),
    dict(id='S2048', S=(2048,), H=2, wide=4, masks=('ragged',), virt='kvz', klay='row', samples=2),
    dict(id='ascending', S=(257, 129), H=3, wide=5, masks=('none', 'none'), virt='kvz', klay='inter', scale='ascending'),
    dict(id='peaked', S=(129, 33, 9), H=16, wide=4, masks=('none', 'ragged', 'none'), virt='z', klay='head', scale='peaked'),
    dict(id='unmasked', S=(32, 24, 127, 8), H=3, wide=4, masks=('none', 's0', 'none', 'none'), virt='none', klay='row'),
    dict(id='S17_63', S=(17, 63), H=16, wide=3, masks=('first', 'none'), virt='k', klay='row', qwide=True),
]
BEAMS = (1, 2, 3, 4, 5, 8, 16, 17)


def launch_beams(L):
    return (1, 2, L['wide'])


def _mask(kind, Bs, S):
    if kind == 'none' or S == 0:
        return None
    m = np.ones((Bs, S), np.uint8)
    for b in range(Bs):
        m[b, :max(S - (Bs - 1 - b) * S // 4, 1)] = 0                   # ragged: the last sample keeps every key
    if kind == 's0':
        m[0] = 1
    if kind == 'last':
        m[:] = 1
        m[:, S - 1] = 0
    if kind == 'first':
        m[:] = 1
        m[:, 0] = 0
    return m


def attn_inputs(L):
    """per context: q [samples, wide', E] (wide' = the widest beam of the launch), k, v [S, samples, E], mask, bias_k,
    bias_v [E] - float64 arrays holding bf16 values"""
    def make():
        import torch
        Bs, H = L.get('samples', 3), L['H']
        E, bmax = H * 64, max(launch_beams(L))
        out = []
        for c, S in enumerate(L['S']):
            g = _gen(4000 + 17 * S + c)
            q, k, v = _randn(g, Bs, bmax, E) * 0.5, _randn(g, S, Bs, E) * 0.5, _randn(g, S, Bs, E)
            bk, bv = _randn(g, E) * 0.5, _randn(g, E)
            u = _randn(g, Bs, E)
            if L.get('scale') == 'ascending':
                ramp = torch.linspace(-1, 1, max(S, 2))[:S].view(S, 1, 1)
                q = u.view(Bs, 1, E) * 0.6 + q * 0.05
                k = u.view(1, Bs, E) * ramp + k * 0.02
            if L.get('scale') == 'peaked' and S:
                q = u.view(Bs, 1, E) + q * 0.05
                k[S - 1 if S >= 129 else S // 2] = torch.from_numpy(_bf(u)).float() * 3.0
            if L.get('scale') is None and S >= 129:
                # a second trip that matters: the last key of the last sample is aligned with its first hypothesis
                k[S - 1, Bs - 1] = torch.from_numpy(_bf(q[Bs - 1, 0])).float()
            out.append(dict(q=_bf(q), k=_bf(k), v=_bf(v), bias_k=_bf(bk), bias_v=_bf(bv), mask=_mask(L['masks'][c], Bs, S)))
        return out
    return cached(('attn_in', L['id']), make)


def virt_of(L, path):
    return 'kvz' if path == 'packed' else L['virt']


def launch_ref(L, beams, path='valu', dt=np.float64, mutant=None):
    """every context of a launch -> [attn_decode dict]; path valu | packed.  mutant ctx_swap: contexts 1 and 2 exchange S
    (the longer of the two loses its tail; the shorter would read past its cache)"""
    def make():
        Bs, E = L.get('samples', 3), L['H'] * 64
        virt = virt_of(L, path)
        res = []
        for c, (S, x) in enumerate(zip(L['S'], attn_inputs(L))):
            if mutant == 'ctx_swap' and len(L['S']) >= 3 and c in (1, 2):
                S = min(S, L['S'][3 - c])
            mask = None if x['mask'] is None else x['mask'][:, :S]
            q = x['q'][:, :beams].reshape(Bs * beams, E)
            res.append(attn_decode(q, x['k'][:S], x['v'][:S], mask, x['bias_k'] if 'k' in virt else None,
                                   x['bias_v'] if 'v' in virt else None, 'z' in virt, beams, dt, mutant, path == 'packed'))
        return res
    if mutant is None:
        return cached(('attn_ref', L['id'], beams, path, dt), make)
    return make()


# DynamicConv step: (C, H), M picked so that the launcher's rule selects R (recorded; the host test recomputes it), K, and
# the tap variant: plain | peaked (one tap logit of every head far above the rest) | equal (wt rows identical within a
# head: the taps are exactly 1 / K)
DCS = [
    dict(id='C2048_M5_K32', C=2048, H=32, M=5, R=4, K=32),
    dict(id='C2048_M33_K9', C=2048, H=32, M=33, R=8, K=9),
    dict(id='C2048_M129_K4', C=2048, H=32, M=129, R=16, K=4),
    dict(id='C1024_M5_K17', C=1024, H=16, M=5, R=4, K=17),
    dict(id='C1024_M70_K2', C=1024, H=16, M=70, R=8, K=2),
    dict(id='C1024_M70_K31', C=1024, H=16, M=70, R=8, K=31),
    dict(id='C1024_M257_K8', C=1024, H=16, M=257, R=16, K=8),
    dict(id='C512_M7_K5', C=512, H=8, M=7, R=4, K=5),
    dict(id='C512_M7_K3', C=512, H=8, M=7, R=4, K=3),
    dict(id='C512_M129_K16', C=512, H=8, M=129, R=8, K=16),
    dict(id='C512_M513_K17', C=512, H=8, M=513, R=16, K=17),
    dict(id='peaked_K9', C=1024, H=16, M=5, R=4, K=9, taps='peaked'),
    dict(id='equal_K3', C=1024, H=16, M=70, R=8, K=3, taps='equal'),
    dict(id='equal_K32', C=512, H=8, M=7, R=4, K=32, taps='equal'),
]


def dcs_steps(case):
    """[(t, has_back)]: t = 0 .. K + 2 from a zeroed ring without back, one step with a random ancestor table, one with a
    large t"""
    K = case['K']
    return [(t, False) for t in range(K + 3)] + [(K + 3, True), (1000 + K, False)]


def dcs_inputs(case):
    """base [M, C] and wt [H K, C] (bf16 values), and per step the row permutation that makes its input x = base[perm]
    (the tap logits of a step are then rows of ONE product) and the ancestor table"""
    def make():
        import torch
        Cc, H, M, K = case['C'], case['H'], case['M'], case['K']
        g = _gen(7000 + Cc + 3 * M + K)
        base, wt = _randn(g, M, Cc), _randn(g, H * K, Cc) * (2.0 / np.sqrt(Cc))
        if case.get('taps') == 'peaked':
            base[:, :64] += 1.0
            for h in range(H):
                wt[h * K + h % K, :64] += 1.0
        if case.get('taps') == 'equal':
            wt = wt.view(H, K, Cc)[:, :1].expand(H, K, Cc).reshape(H * K, Cc)
        steps = dcs_steps(case)
        perms = [torch.randperm(M, generator=g).numpy() for _ in steps]
        back = torch.randint(0, M, (K - 1, M), generator=g).numpy().astype(np.int32)
        return dict(base=_bf(base), wt=_bf(wt), perms=perms, back=back)
    return cached(('dcs_in', case['id']), make)


def dcs_run(case, dt=np.float64, mutant=None):
    """the whole step sequence of a case -> [dynconv_step dict per step]; the ring is carried from step to step in place, so
    a step's dict holds no ring of its own (the expected ring after step i: planes t mod K of the steps so far = their x)"""
    def make():
        x = dcs_inputs(case)
        H, K = case['H'], case['K']
        lg, L = tap_logits(x['base'], x['wt'], H, K, dt)
        ring = np.zeros((K,) + x['base'].shape)
        res = []
        for (t, hb), perm in zip(dcs_steps(case), x['perms']):
            r = dynconv_step(x['base'][perm], ring, x['wt'], t, x['back'] if hb else None, H, K, dt, mutant,
                             logits=(lg[perm], L[perm]), inplace=True)
            del r['ring']
            res.append(r)
        return res
    if mutant is None:
        return cached(('dcs_ref', case['id'], dt), make)
    return make()
