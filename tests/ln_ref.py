"""float64 reference of the LayerNorm kernels (csrc/layernorm.hip: tell_layernorm_fwd / _bwd, tell_layernorm_cat_fwd / _bwd;
csrc/decode.hip: tell_layernorm_rows), their fp32 emulation in the kernels' own summation order, the element-wise bounds, the
case tables, the mutants and the path-naming functions that tests/test_ln_ref_host.py and tests/test_gpu_layernorm.py walk
(DESIGN.md section 36).  numpy only; nothing here comes from oracle/.  Inputs are rounded to their storage type BEFORE they
reach a function.  The conventions are those of tests/small_ref.py (Out, store, ratio, the bound of one element):

    u_out |ref|  +  c gamma 2^-24 S  +  2^-126 (1 + S)

z = x keep / (1 - p) + res is the normalised row; Sz_c = |x keep / (1 - p)| + |res| its absolute terms, mSz their row mean,
nz the roundings of z itself (one for the product when p > 0, one for the residual sum), d = z - mean, T = ceil(C / 64) the
additions of one lane (lane-strided trips, or NCH x VEC register elements), 6 the butterfly.  First-order propagation:

    group       gamma                         S
    ln_mean     T + 6 + nz + 8                mSz
    ln_rstd     T + 6 + nz + 8                rstd R,  R = 1 + V + V2:  V = mean_j |d_j| (|d_j| + nz Sz_j) / (var + eps) (the
                                              roundings of d and of z in the sum of squares; the error of the mean cancels in
                                              it to first order), V2 = gamma 2^-24 mSz^2 / (var + eps) (its second-order rest,
                                              which is all there is on a constant row)
    ln_y        T + 6 + nz + 8                |gamma_c| rstd (Sz_c + mSz)  +  |xhat_c gamma_c| R  +  |beta_c|
                                              (the subtraction z - mean, the relative error of the variance, the shift)
    ln_dx       T + 6 + nz + 8                dx, dres (and the dx_i of the cat form): rstd (|g| + S1 + |xhat| S2 + |s2| Exh +
                                              |xhat| mean_j |g_j| Exh_j) [/ (1 - p) for dx] [+ |dres0|], g = dy gamma,
                                              S1 = mean |g|, S2 = mean |g xhat|, Exh = |xhat| + nz rstd Sz (xhat from the
                                              STORED mean and rstd, so only its own roundings count)
    cat_dres    the same + n                  sum_i of the above (n additions in registers, one rounding to bf16)
    ln_partial  4 + 4                         sum over the block's 4 rows of |dy| Exh (gamma half), |dy| (beta half)
    ln_dparam   4 + ceil(ceil(nb / 16) / 4) + 3 + 16
                                              [|prefill| +] sum over all rows of the same
    rows_y, rows_stats  (C / 1024 + 2) + 6 + 2 + 8   as ln_y, ln_mean, ln_rstd with nz = 0 (fp32 rows, no dropout, no residual)

Exact: dx of a dropped element is +-0; the option ln_var 0 against the default, a null mean, a null stats_out and the cat
forward against n single launches are compared bit for bit by the GPU test itself.

Definitions the kernels leave open.  `mean` given with `rstd` null is not a case (the kernels store both or neither).  A
constant row has variance 0: its rstd is 1 / sqrt(eps) only as far as eps dominates the square of the mean's own rounding
error, which V2 states - at eps = 1e-12 and |z| near 1 that bound is vacuous, and only y = beta within the first term of S
is held.  C = 1 is a constant row.  rows = 0 writes nothing.

Measured on the MI355X: MEASURED and C below, and DESIGN.md section 36.
"""
import zlib

import numpy as np

import small_ref as sr
from decode_ref import EPS, _pin, _sum
from small_ref import SENTINEL, Out, _rng, cached, ratio, same_bits, store, wave_fold      # noqa: F401  (re-exported)

F32, F64 = np.float32, np.float64
SEED = 20251

# largest observed (|got - ref| - u_out |ref|) / (gamma 2^-24 S) over the grid of tests/test_gpu_layernorm.py on the MI355X,
# and the pinned constant: four times that, rounded up to a power of two; 2^-10 where the ratio never left u_out |ref|.  A
# group missing from MEASURED is not pinned: its GPU test then fails with the measured ratio in its message.
MEASURED = {'ln_y': 0.085051, 'ln_mean': 0.118224, 'ln_rstd': 0.033145, 'ln_dx': 0.085410, 'ln_partial': 0.233782,
            'ln_dparam': 0.080004, 'cat_dres': 0.0, 'rows_y': 0.016176, 'rows_stats': 0.021739}
C = {k: _pin(v) for k, v in MEASURED.items()}
GROUPS = ('ln_y', 'ln_mean', 'ln_rstd', 'ln_dx', 'ln_partial', 'ln_dparam', 'cat_dres', 'rows_y', 'rows_stats')

FWD_MUTANTS = ('fwd_one_pass_variance', 'fwd_eps_outside_root', 'fwd_dropout_on_sum', 'fwd_keep_index_row_ld',
               'fwd_last_trip_dropped', 'fwd_mean_by_padded_width')
ROWS2_MUTANTS = ('rows2_second_row_first_stats', 'rows2_last_odd_row_unwritten')
BWD_MUTANTS = ('bwd_s2_without_xhat', 'bwd_dx_without_keep', 'bwd_dres_overwritten_under_accumulate', 'bwd_dgamma_from_g',
               'bwd_dead_wave_lds_not_zeroed', 'finish_fourth_accumulator_dropped', 'finish_remainder_dropped',
               'bwd_dparam_accumulate_ignored')
CAT_MUTANTS = ('cat_stats_rows_major', 'cat_slice_offset_by_ld', 'cat_one_salt_for_all', 'cat_dres_last_problem_only',
               'cat_dgamma_stored')
LNROWS_MUTANTS = ('rows_fourth_wave_left_out_of_mean', 'rows_stats_index_without_2')
MUTANTS = FWD_MUTANTS + ROWS2_MUTANTS + BWD_MUTANTS + CAT_MUTANTS + LNROWS_MUTANTS
# wrong only through fp32 rounding: run in the fp32 emulation (float64 forgives a one-pass variance)
FP32_MUTANTS = ('fwd_one_pass_variance',)


def failures(got, o, c=None):
    """small_ref.failures with this file's constants; a dropped element may be +0 or -0"""
    got = np.asarray(got, np.float32)
    if o.exact_at is not None:
        got = np.where(o.exact_at, np.abs(got), got)
    if o.group in ('exact', None):
        return sr.failures(got, o)
    return sr.failures(got, o, C[o.group] if c is None else c)


# ---------------------------------------------------------------- pieces of the kernels
def inv_keep(p, dt):
    """1 / (1 - p) as the launcher computes it (fp32 on the host)"""
    p32 = np.float32(p)
    if float(p32) == 0.0:
        return dt(1)
    return dt(np.float32(1) / (np.float32(1) - p32)) if dt is F32 else 1.0 / (1.0 - float(p32))


def keep_of(salt, rows, Cc, p, stride=None):
    """the 0 / 1 keep flags of a [rows, C] problem: element index row * C + c (stride: a mutant's row * ld + c)"""
    if not p:
        return None

    def make():
        from tell_amd import rng
        idx = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(Cc if stride is None else stride) + \
            np.arange(Cc, dtype=np.uint64)[None, :]
        return rng.keep_mask(SEED, salt, idx, p)
    return cached(('ln_keep', salt, rows, Cc, float(p), stride), make)


def lane_acc(t, dt, vec=1):
    """one wave's sum of a row t [..., C]: lane l adds, one by one, the `vec` consecutive terms of its chunk (l + 64 i) vec,
    chunk after chunk (vec = 1: the lane-strided trips of the generic kernels), then the butterfly"""
    t = np.asarray(t, dt)
    if dt is F64:
        return t.sum(-1)
    n, per = t.shape[-1], 64 * vec
    trips = max(-(-n // per), 1)
    p = np.zeros(t.shape[:-1] + (trips * per,), dt)
    p[..., :n] = t
    p = p.reshape(t.shape[:-1] + (trips, 64, vec))
    acc = np.zeros(t.shape[:-1] + (64,), dt)
    for i in range(trips):
        for k in range(vec):
            acc = (acc + p[..., i, :, k]).astype(dt)
    return wave_fold(acc, dt)


def _z(x, res, keep, p, dt, mutant=None):
    """-> z, Sz, the keep factor (0 or 1 / (1 - p); None without dropout)"""
    x = np.asarray(x, dt)
    kf = None if keep is None else (np.asarray(keep, dt) * inv_keep(p, dt)).astype(dt)
    if mutant == 'fwd_dropout_on_sum' and kf is not None and res is not None:
        z = ((x + np.asarray(res, dt)).astype(dt) * kf).astype(dt)
        return z, np.abs(np.asarray(z, F64)), kf
    t = x if kf is None else (x * kf).astype(dt)
    Sz = np.abs(np.asarray(t, F64))
    if res is None:
        return t, Sz, kf
    return (t + np.asarray(res, dt)).astype(dt), Sz + np.abs(np.asarray(res, F64)), kf


def _rsqrt(a, dt):
    with np.errstate(all='ignore'):
        return (1.0 / np.sqrt(np.asarray(a, F64))).astype(dt)


def fwd_gamma(Cc, nz):
    return -(-Cc // 64) + 6 + nz + 8


def _fwd_S(z, Sz, mu, var, rs, gamma, beta, eps, nz, gam):
    """the S of mean, rstd and y from (float64 views of) the row's quantities"""
    z, mu, var, rs = (np.asarray(a, F64) for a in (z, mu, var, rs))
    d = z - mu[:, None]
    mSz = Sz.mean(-1)
    den = np.maximum(var, 0.0) + float(np.float32(eps))
    R = 1.0 + (np.abs(d) * (np.abs(d) + nz * Sz)).mean(-1) / den + gam * EPS * mSz ** 2 / den
    g64, b64 = np.abs(np.asarray(gamma, F64)), np.abs(np.asarray(beta, F64))
    S_y = g64 * rs[:, None] * (Sz + mSz[:, None]) + np.abs(d * rs[:, None]) * g64 * R[:, None] + b64
    return mSz, rs * R, S_y


def ln_fwd(x, res, gamma, beta, eps, p, keep, vec, dtype, dt=F64, mutant=None, ld=None, rows2=False, groups=None):
    """x, res [rows, C] -> y, mean, rstd.  vec: 1 (ln_fwd_kernel) or the elements of a 16-byte chunk (the register kernels);
    rows2: ln_fwd_vec_rows_kernel took the launch; ld: the padded width (a mutant divides by it)"""
    gy, gm, gr = groups or ('ln_y', 'ln_mean', 'ln_rstd')
    rows, Cc = np.shape(x)
    z, Sz, _ = _z(x, res, keep, p, dt, mutant)
    gamma, beta = np.asarray(gamma, dt), np.asarray(beta, dt)
    nz = int(keep is not None) + int(res is not None)
    per = 64 * vec
    live = np.ones(Cc, bool)
    if mutant == 'fwd_last_trip_dropped':
        live[(-(-Cc // per) - 1) * per:] = False
    width = dt(ld if mutant == 'fwd_mean_by_padded_width' else Cc)
    e = dt(np.float32(eps))
    with np.errstate(all='ignore'):
        mu = (lane_acc(np.where(live, z, dt(0)), dt, vec) / width).astype(dt)
        d = (z - mu[:, None]).astype(dt)
        if mutant == 'fwd_one_pass_variance':
            var = ((lane_acc(np.where(live, (z * z).astype(dt), dt(0)), dt, vec) / width).astype(dt) - (mu * mu).astype(dt)).astype(dt)
        else:
            var = (lane_acc(np.where(live, (d * d).astype(dt), dt(0)), dt, vec) / width).astype(dt)
        if mutant == 'fwd_eps_outside_root':
            rs = (dt(1) / (np.sqrt(var).astype(dt) + e).astype(dt)).astype(dt)
        else:
            rs = _rsqrt((var + e).astype(dt), dt)
        if rows2 and mutant == 'rows2_second_row_first_stats':
            src = np.arange(rows) - (np.arange(rows) & 1)
            mu, rs = mu[src], rs[src]
            d = (z - mu[:, None]).astype(dt)
        y = (((d * rs[:, None]).astype(dt) * gamma).astype(dt) + beta).astype(dt)
    if rows2 and mutant == 'rows2_last_odd_row_unwritten' and rows % 2:
        y, mu, rs = y.copy(), mu.copy(), rs.copy()
        y[-1], mu[-1], rs[-1] = SENTINEL, SENTINEL, SENTINEL
    gam = fwd_gamma(Cc, nz)
    S_m, S_r, S_y = _fwd_S(z, Sz, mu, var, rs, gamma, beta, eps, nz, gam)
    return dict(y=Out(y, S_y, gam, dtype, gy), mean=Out(mu, S_m, gam, 'float32', gm), rstd=Out(rs, S_r, gam, 'float32', gr))


def block_partials(t, dt, dead=0.0):
    """[rows, W] -> [blocks, W]: the four waves' LDS slices of a block, ((w0 + w1) + w2) + w3; a dead wave's slice holds `dead`"""
    t = np.asarray(t, dt)
    rows, W = t.shape
    nb = -(-rows // 4)
    p = np.full((nb * 4, W), dead, dt)
    p[:rows] = t
    p = p.reshape(nb, 4, W)
    return (((p[:, 0] + p[:, 1]).astype(dt) + p[:, 2]).astype(dt) + p[:, 3]).astype(dt)


def finish_fold(part, dt, mutant=None):
    """ln_bwd_finish_kernel: [blocks, W] -> [W].  Group by of 16 walks the blocks by, by + 16, ...: rounds of four blocks
    into four accumulators while b + 48 < blocks, the rest into the first; (s0 + s1) + (s2 + s3); the 16 groups in order"""
    part = np.asarray(part, dt)
    nb, W = part.shape
    groups = []
    for by in range(16):
        a, b = [np.zeros(W, dt) for _ in range(4)], by
        while b + 48 < nb:
            for q in range(4):
                if not (q == 3 and mutant == 'finish_fourth_accumulator_dropped'):
                    a[q] = (a[q] + part[b + 16 * q]).astype(dt)
            b += 64
        while b < nb and mutant != 'finish_remainder_dropped':
            a[0] = (a[0] + part[b]).astype(dt)
            b += 16
        groups.append(((a[0] + a[1]).astype(dt) + (a[2] + a[3]).astype(dt)).astype(dt))
    return _sum(np.stack(groups), 0, dt)


def dparam_gamma(nb):
    return 4 + -(-(-(-nb // 16)) // 4) + 3 + 16


def _bwd_core(dy, x, res, gamma, mean, rstd, p, keep, vec, dt, mutant=None):
    """one problem's row work: dz [rows, C] (unrounded to storage), its S, the keep factor, the dgamma / dbeta terms"""
    Cc = np.shape(x)[1]
    z, Sz, kf = _z(x, res, keep, p, dt)
    nz = int(keep is not None) + int(res is not None)
    dy, gamma = np.asarray(dy, dt), np.asarray(gamma, dt)
    mu, rs = np.asarray(mean, dt)[:, None], np.asarray(rstd, dt)[:, None]
    with np.errstate(all='ignore'):
        xh = ((z - mu).astype(dt) * rs).astype(dt)
        g = (dy * gamma).astype(dt)
        s1 = (lane_acc(g, dt, vec) / dt(Cc)).astype(dt)[:, None]
        s2 = (lane_acc(g if mutant == 'bwd_s2_without_xhat' else (g * xh).astype(dt), dt, vec) / dt(Cc)).astype(dt)[:, None]
        dz = (rs * ((g - s1).astype(dt) - (xh * s2).astype(dt)).astype(dt)).astype(dt)
        tg = ((g if mutant == 'bwd_dgamma_from_g' else dy) * xh).astype(dt)
    rs64, xh64, g64 = np.abs(np.asarray(rs, F64)), np.abs(np.asarray(xh, F64)), np.abs(np.asarray(g, F64))
    Exh = xh64 + nz * rs64 * Sz
    S_dz = rs64 * (g64 + g64.mean(-1, keepdims=True) + xh64 * (g64 * xh64).mean(-1, keepdims=True) +
                   np.abs(np.asarray(s2, F64)) * Exh + xh64 * (g64 * Exh).mean(-1, keepdims=True))
    d64 = np.abs(np.asarray(dy, F64))
    return dict(dz=dz, S_dz=S_dz, kf=kf, tg=tg, tb=dy, S_tg=d64 * Exh, S_tb=d64, nz=nz)


def _dx_out(k, keep, p, gam, dtype, dt, mutant=None):
    kf = None if (k['kf'] is None or mutant == 'bwd_dx_without_keep') else k['kf']
    dx = k['dz'] if kf is None else (k['dz'] * kf).astype(dt)
    S = k['S_dz'] * float(inv_keep(p, F64))
    if keep is None:
        return Out(dx, S, gam, dtype, 'ln_dx')
    drop = np.asarray(keep) == 0
    return Out(np.where(drop & (np.asarray(dx) == 0), dt(0), dx), S, gam, dtype, 'ln_dx', exact_at=drop)


def _partials(k, dt, mutant=None):
    dead = SENTINEL if mutant == 'bwd_dead_wave_lds_not_zeroed' else 0.0
    part = np.concatenate([block_partials(k['tg'], dt, dead), block_partials(k['tb'], dt, dead)], 1)
    S = np.concatenate([block_partials(k['S_tg'], F64), block_partials(k['S_tb'], F64)], 1)
    return part, S


def ln_bwd(dy, x, res, gamma, mean, rstd, p, keep, vec, dtype, dres0, dg0, db0, outs='both', dres_acc=0, dparam_acc=0,
           dgamma_null=False, dt=F64, mutant=None):
    """tell_layernorm_bwd on the STORED mean / rstd -> dx, dres (outs: both | dx | dres), partial [blocks, 2C], and dgamma,
    dbeta unless dgamma is null"""
    Cc = np.shape(x)[1]
    k = _bwd_core(dy, x, res, gamma, mean, rstd, p, keep, vec, dt, mutant)
    gam = fwd_gamma(Cc, k['nz'])
    out = {}
    if outs in ('both', 'dx'):
        out['dx'] = _dx_out(k, keep, p, gam, dtype, dt, mutant)
    if outs in ('both', 'dres'):
        d0 = np.asarray(dres0, dt)
        acc = dres_acc and mutant != 'bwd_dres_overwritten_under_accumulate'
        out['dres'] = Out((d0 + k['dz']).astype(dt) if acc else k['dz'], k['S_dz'] + (np.abs(np.asarray(dres0, F64)) if dres_acc else 0.0),
                          gam, dtype, 'ln_dx')
    part, S_part = _partials(k, dt, mutant)
    out['partial'] = Out(part, S_part, 8, 'float32', 'ln_partial')
    if not dgamma_null:
        nb = part.shape[0]
        s = finish_fold(part, dt, mutant)
        d0 = np.concatenate([np.asarray(dg0, dt), np.asarray(db0, dt)])
        acc = dparam_acc and mutant != 'bwd_dparam_accumulate_ignored'
        v = (d0 + s).astype(dt) if acc else s
        S = S_part.sum(0) + (np.abs(np.asarray(d0, F64)) if dparam_acc else 0.0)
        out['dgamma'] = Out(v[:Cc], S[:Cc], dparam_gamma(nb), 'float32', 'ln_dparam')
        out['dbeta'] = Out(v[Cc:], S[Cc:], dparam_gamma(nb), 'float32', 'ln_dparam')
    return out


# ================================================================ dispatch, restated from the launchers
def _vec(dtype):
    return 8 if dtype == 'bfloat16' else 4


def fwd_path(dtype, Cc, rows, ld, off=None, has_res=True, ln_var=None):
    """the branch tell_layernorm_fwd takes (every operand has the row stride ld; off: the operand one element off 16 bytes)"""
    vec = _vec(dtype)
    al_ptr = off not in ('x', 'y') and not (off == 'res' and has_res)
    aligned = ld % vec == 0 and al_ptr
    var = 1 if ln_var is None or ln_var < 0 else ln_var
    if var and aligned and dtype == 'bfloat16' and Cc == 1024 and rows >= 4096:
        return 'fwd:rows2'
    nch = Cc // (64 * vec) if Cc % (64 * vec) == 0 else 0
    if aligned and nch in (1, 2, 4):
        return 'fwd:vec:nch%d' % nch
    why = 'ld' if ld % vec else ('ptr_' + off if not al_ptr else ('nch3' if nch == 3 else ('nch>4' if nch > 4 else 'ragged')))
    return 'fwd:generic:' + why


def bwd_path(dtype, Cc, ld, off=None, has_res=True, outs='both'):
    """the branch tell_layernorm_bwd takes; a null operand passes the alignment test"""
    vec = _vec(dtype)
    there = {'dy', 'x'} | ({'res'} if has_res else set()) | ({'dx'} if outs in ('both', 'dx') else set()) | \
        ({'dres'} if outs in ('both', 'dres') else set())
    al_ptr = off not in there
    aligned = ld % vec == 0 and al_ptr
    nch = Cc // (64 * vec) if Cc % (64 * vec) == 0 else 0
    if aligned and (nch in (1, 2) or (nch == 4 and dtype == 'float32')):
        return 'bwd:vec:nch%d' % nch
    why = 'ld' if ld % vec else ('ptr_' + off if not al_ptr else (
        'nch3' if nch == 3 else ('bf16_nch4' if nch == 4 else ('nch>4' if nch > 4 else 'ragged'))))
    return 'bwd:generic:' + why + (':lds64k' if Cc * 32 == 65536 else '')


def finish_walk(nb):
    """what the 16 groups of the finish kernel do with nb partial blocks"""
    if nb < 16:
        return 'groups_empty'
    if nb <= 48:
        return 'remainder_only'
    return 'unrolled' if nb % 64 == 0 else ('unrolled_for_some' if nb < 64 else 'unrolled+remainder')


# ================================================================ inputs
KINDS = ('plain', 'mean100', 'tiny_var', 'constant', 'outlier')


def rows_of_kinds(r, rows, Cc, kind0, with_res):
    """x, res [rows, C] float64 cycling the row kinds: mean = 100 x the deviation; variance far below eps; a constant row; one
    outlier of 2^10 in the last column a lane visits"""
    x, res = r.standard_normal((rows, Cc)), r.standard_normal((rows, Cc))
    kind = (np.arange(rows) + kind0) % len(KINDS)
    m = kind == 1
    x[m] += 100.0
    res[m] *= 0.25
    m = kind == 2
    x[m] *= 3e-4
    res[m] *= 3e-4
    m = kind == 3
    x[m], res[m] = 0.75, 0.5
    x[kind == 4, Cc - 1] = 1024.0
    return x, (res if with_res else None)


def affine(r, Cc):
    """gamma with zeros and negative entries, beta large against y - beta on every fifth column"""
    gamma, beta = r.standard_normal(Cc), r.standard_normal(Cc)
    gamma[np.arange(Cc) % 7 == 3] = 0.0
    beta[np.arange(Cc) % 5 == 0] *= 64.0
    return np.asarray(gamma, F32), np.asarray(beta, F32)


def salt_of(*key):
    return zlib.crc32(repr(key).encode()) & 0xFFFFFFFF


# ================================================================ tell_layernorm_fwd / tell_layernorm_bwd
def _ln(id, dtype, Cc, rows, mutants=(), **kw):
    c = dict(id=id, dtype={'bf16': 'bfloat16', 'f32': 'float32'}[dtype], C=Cc, rows=rows, mutants=tuple(mutants), pad=0, off=None,
             res=True, p=0.0, eps=1e-5, outs='both', dres_acc=0, dparam_acc=0, dgamma_null=False, ln_var=None, bwd=True, kind0=0)
    c.update(kw)
    return c


LN = [
    # the generic kernels: ragged lane trips, NCH = 3, NCH = 8, 64 KB of dynamic LDS in the backward
    _ln('g_c1', 'f32', 1, 1, ['bwd_dparam_accumulate_ignored'], dparam_acc=1, kind0=0),
    _ln('g_c63', 'bf16', 63, 3, ['fwd_eps_outside_root', 'bwd_dead_wave_lds_not_zeroed'], p=0.1),
    _ln('g_c64', 'f32', 64, 4, ['fwd_one_pass_variance'], res=False, outs='dx', eps=1e-12),
    _ln('g_c65', 'bf16', 65, 5, ['fwd_last_trip_dropped', 'bwd_dres_overwritten_under_accumulate'], dres_acc=1, p=0.5),
    _ln('g_c200', 'f32', 200, 9, ['fwd_keep_index_row_ld', 'fwd_mean_by_padded_width', 'bwd_dx_without_keep'], pad=4, p=0.1),
    _ln('g_bf16_1536', 'bf16', 1536, 5, ['fwd_last_trip_dropped'], eps=1e-12, outs='dres'),
    _ln('g_f32_768', 'f32', 768, 3, ['bwd_s2_without_xhat'], dgamma_null=True),
    _ln('g_f32_2048', 'f32', 2048, 4, ['bwd_dgamma_from_g'], res=False, kind0=1),
    _ln('v_bf16_2048', 'bf16', 2048, 5, ['fwd_last_trip_dropped', 'bwd_dead_wave_lds_not_zeroed'], p=0.1, kind0=4),
    # the register kernels
    _ln('v_bf16_512', 'bf16', 512, 9, ['fwd_dropout_on_sum', 'bwd_dx_without_keep'], p=0.5),
    _ln('v_bf16_1024', 'bf16', 1024, 4, ['fwd_eps_outside_root', 'bwd_s2_without_xhat'], dres_acc=1, dparam_acc=1),
    _ln('v_f32_256', 'f32', 256, 5, ['fwd_one_pass_variance', 'fwd_last_trip_dropped'], res=False, outs='dx'),
    _ln('v_f32_512', 'f32', 512, 1, ['bwd_dgamma_from_g'], kind0=4, p=0.1, outs='dres'),
    _ln('v_f32_1024', 'f32', 1024, 3, ['bwd_dead_wave_lds_not_zeroed', 'bwd_dparam_accumulate_ignored'], dparam_acc=1, eps=1e-12),
    # demotions: each alone turns a register case into a generic one
    _ln('d_ld1028', 'bf16', 1024, 5, ['fwd_mean_by_padded_width'], pad=4),
    _ln('d_x_off', 'bf16', 512, 5, off='x'),
    _ln('d_res_off', 'f32', 256, 6, off='res'),
    _ln('d_y_off', 'bf16', 512, 3, off='y', p=0.1),
    _ln('d_dy_off', 'f32', 256, 5, off='dy', dres_acc=1),
    _ln('d_dx_off', 'bf16', 512, 5, off='dx', p=0.1),
    _ln('d_dres_off', 'bf16', 1024, 3, off='dres', dres_acc=1),
    _ln('v_ld1032', 'bf16', 1024, 5, ['fwd_keep_index_row_ld'], pad=8, p=0.1),
    # partial blocks: rows = 4 nb - 1 around the 16 groups and the 4-way unrolled fold of the finish kernel
    _ln('nb1', 'f32', 64, 3, ['finish_remainder_dropped']),
    _ln('nb15', 'bf16', 64, 59, ['finish_remainder_dropped'], dparam_acc=1),
    _ln('nb16', 'f32', 64, 63, ['bwd_dparam_accumulate_ignored'], dparam_acc=1, p=0.1),
    _ln('nb17', 'bf16', 64, 67, ['finish_remainder_dropped']),
    _ln('nb48', 'f32', 64, 191, ['finish_remainder_dropped'], res=False),
    _ln('nb49', 'bf16', 64, 195, ['finish_fourth_accumulator_dropped', 'finish_remainder_dropped'], dparam_acc=1),
    _ln('nb64', 'f32', 64, 255, ['finish_fourth_accumulator_dropped']),
    _ln('nb65', 'bf16', 64, 259, ['finish_fourth_accumulator_dropped', 'finish_remainder_dropped'], p=0.1),
    _ln('nb113', 'f32', 64, 451, ['finish_fourth_accumulator_dropped', 'finish_remainder_dropped'], dparam_acc=1),
    _ln('nb49_c1024', 'bf16', 1024, 195, ['finish_fourth_accumulator_dropped', 'bwd_dgamma_from_g']),
    # two rows per wave: bf16, C = 1024, rows >= 4096
    _ln('r2_4096', 'bf16', 1024, 4096, ['rows2_second_row_first_stats'], bwd=False),
    _ln('r2_4097_p', 'bf16', 1024, 4097, ['rows2_last_odd_row_unwritten', 'fwd_keep_index_row_ld'], pad=8, p=0.1),
    _ln('r2_4097_nores', 'bf16', 1024, 4097, ['rows2_last_odd_row_unwritten'], res=False, ln_var=-1, bwd=False, eps=1e-12),
    _ln('r2_4095', 'bf16', 1024, 4095, ['fwd_last_trip_dropped'], bwd=False),
    _ln('r2_4096_var0', 'bf16', 1024, 4096, ln_var=0, bwd=False, res=False),
]


def ln_fwd_path(case):
    return fwd_path(case['dtype'], case['C'], case['rows'], case['C'] + case['pad'], case['off'], case['res'], case['ln_var'])


def ln_bwd_path(case):
    return bwd_path(case['dtype'], case['C'], case['C'] + case['pad'], case['off'], case['res'], case['outs'])


def _path_vec(path, dtype):
    return 1 if ':generic' in path else _vec(dtype)


def ln_paths(case):
    rows, nb = case['rows'], -(-case['rows'] // 4)
    p = {ln_fwd_path(case), 'ln:' + case['dtype'], 'ln:res' if case['res'] else 'ln:no_res',
         'ln:p0' if not case['p'] else 'ln:dropout', 'ln:eps_small' if case['eps'] < 1e-8 else 'ln:eps',
         'ln:ld>C' if case['pad'] else 'ln:ld=C', 'ln:last_block:%d_rows' % ((rows - 1) % 4 + 1),
         'ln:one_block' if nb == 1 else 'ln:several_blocks', 'ln:option:%s' % case['ln_var']}
    if case['bwd']:
        p |= {ln_bwd_path(case), 'bwd:outs:' + case['outs'], 'bwd:dres_acc%d' % case['dres_acc'],
              'bwd:dgamma_null' if case['dgamma_null'] else 'bwd:dparam_acc%d' % case['dparam_acc'],
              'finish:' + finish_walk(nb)}
    return p


def ln_inputs(case):
    def make():
        r, rows, Cc, dty = _rng('ln', case['id']), case['rows'], case['C'], case['dtype']
        x, res = rows_of_kinds(r, rows, Cc, case['kind0'], case['res'])
        gamma, beta = affine(r, Cc)
        f = lambda a: np.asarray(a, F32)                                                          # noqa: E731
        return dict(x=store(x, dty), res=None if res is None else store(res, dty), gamma=gamma, beta=beta,
                    dy=store(r.standard_normal((rows, Cc)), dty), dres0=store(r.standard_normal((rows, Cc)), dty),
                    dg0=f(r.standard_normal(Cc)), db0=f(r.standard_normal(Cc)))
    return cached(('ln_in', case['id']), make)


def ln_salt(case):
    return salt_of('ln', case['id'])


def ln_case(case, dt=F64, mutant=None, stats=None):
    """forward and (unless the case is forward only) backward of one case -> dict of Out.  stats: the stored (mean, rstd) the
    backward reads (default: this forward's own, unmutated, rounded to fp32)"""
    v, rows, Cc, dty, ld = ln_inputs(case), case['rows'], case['C'], case['dtype'], case['C'] + case['pad']
    keep = keep_of(ln_salt(case), rows, Cc, case['p'])
    fkeep = keep_of(ln_salt(case), rows, Cc, case['p'], ld) if mutant == 'fwd_keep_index_row_ld' else keep
    fp = ln_fwd_path(case)
    args = (v['x'], v['res'], v['gamma'], v['beta'], case['eps'], case['p'])
    out = ln_fwd(*args, fkeep, _path_vec(fp, dty), dty, dt, mutant, ld, fp == 'fwd:rows2')
    if not case['bwd']:
        return out
    if stats is None:
        own = ln_fwd(*args, keep, _path_vec(fp, dty), dty, dt)
        stats = (own['mean'].value.astype(F32), own['rstd'].value.astype(F32))
    out.update(ln_bwd(v['dy'], v['x'], v['res'], v['gamma'], stats[0], stats[1], case['p'], keep, _path_vec(ln_bwd_path(case), dty),
                      dty, v['dres0'], v['dg0'], v['db0'], case['outs'], case['dres_acc'], case['dparam_acc'], case['dgamma_null'],
                      dt, mutant))
    return out


# ================================================================ tell_layernorm_cat_fwd / tell_layernorm_cat_bwd
def _cat(id, n, Cc, rows, mutants=(), **kw):
    c = dict(id=id, n=n, C=Cc, rows=rows, mutants=tuple(mutants), pad_y=0, p=0.0, eps=1e-5, salts=None, dx_null=(), dres_null=False,
             dgamma_null=False)
    c.update(kw)
    return c


CAT = [
    _cat('n1_c512_r1', 1, 512, 1, ['cat_dgamma_stored']),
    _cat('n2_c1024_r4', 2, 1024, 4, ['cat_slice_offset_by_ld', 'cat_one_salt_for_all', 'cat_stats_rows_major'], pad_y=8, p=0.1),
    _cat('n4_c512_r5_equal_salts', 4, 512, 5, ['cat_dres_last_problem_only', 'cat_one_salt_for_all', 'bwd_dead_wave_lds_not_zeroed'],
         p=0.1, salts=(7, 9, 7, 11), dx_null=(1,), eps=1e-12),
    _cat('n8_c512_r33', 8, 512, 33, ['cat_stats_rows_major', 'cat_slice_offset_by_ld', 'cat_dgamma_stored'], pad_y=8, dres_null=True,
         dx_null=(0, 7)),
    _cat('n4_c1024_r197', 4, 1024, 197, ['cat_dres_last_problem_only', 'finish_fourth_accumulator_dropped'], p=0.1),
    _cat('n2_c512_r33', 2, 512, 33, ['cat_dres_last_problem_only'], p=0.1, dgamma_null=True),
]


def cat_salts(case):
    return tuple(case['salts'] or [salt_of('cat', case['id'], i) for i in range(case['n'])])


def cat_paths(case):
    n, rows, nb = case['n'], case['rows'], -(-case['rows'] // 4)
    s = cat_salts(case)
    return {'cat:nch%d' % (case['C'] // 512), 'cat:n=1' if n == 1 else ('cat:n=max' if n == 8 else 'cat:n'),
            'cat:ld_y>nC' if case['pad_y'] else 'cat:ld_y=nC', 'cat:p0' if not case['p'] else 'cat:dropout',
            'cat:salts:' + ('equal' if len(set(s)) < n else 'distinct'), 'cat:dx_null' if case['dx_null'] else 'cat:dx_all',
            'cat:dres_null' if case['dres_null'] else 'cat:dres', 'cat:dgamma_null' if case['dgamma_null'] else 'cat:finish',
            'cat:last_block:%d_rows' % ((rows - 1) % 4 + 1), 'cat:one_block' if nb == 1 else 'cat:several_blocks'} | \
        (set() if case['dgamma_null'] else {'cat:finish:' + finish_walk(nb)})


def cat_inputs(case):
    def make():
        r, n, rows, Cc = _rng('cat', case['id']), case['n'], case['rows'], case['C']
        xs, res = [], None
        for i in range(n):
            x, rr = rows_of_kinds(r, rows, Cc, i, True)
            xs.append(store(x, 'bfloat16'))
            res = rr if res is None else res
        ab = [affine(r, Cc) for _ in range(n)]
        f = lambda a: np.asarray(a, F32)                                                          # noqa: E731
        return dict(xs=xs, res=store(res, 'bfloat16'), gammas=[a for a, _ in ab], betas=[b for _, b in ab],
                    dcat=store(r.standard_normal((rows, n * Cc)), 'bfloat16'),
                    dg0=[f(r.standard_normal(Cc)) for _ in range(n)], db0=[f(r.standard_normal(Cc)) for _ in range(n)])
    return cached(('cat_in', case['id']), make)


def cat_case(case, dt=F64, mutant=None, stats=None):
    """-> dict of Out: y [rows, n C], mean / rstd [n, rows], dx<i>, dres, partial [n, blocks, 2C], dgamma<i> / dbeta<i>"""
    v, n, rows, Cc = cat_inputs(case), case['n'], case['rows'], case['C']
    salts = cat_salts(case)
    keeps = [keep_of(s, rows, Cc, case['p']) for s in salts]
    if mutant == 'cat_one_salt_for_all':
        keeps = [keeps[0]] * n
    f = [ln_fwd(v['xs'][i], v['res'], v['gammas'][i], v['betas'][i], case['eps'], case['p'], keeps[i], 8, 'bfloat16', dt)
         for i in range(n)]
    y, S_y = np.concatenate([o['y'].value for o in f], 1), np.concatenate([o['y'].S for o in f], 1)
    if mutant == 'cat_slice_offset_by_ld':
        ld = n * Cc + case['pad_y']                  # problem i lands ld i elements on: row r of it in row r + i, columns 0 .. C - 1
        flat = np.full((rows + n) * ld, SENTINEL, y.dtype)
        for i in range(n):
            for r_ in range(rows):
                flat[(r_ + i) * ld:(r_ + i) * ld + Cc] = f[i]['y'].value[r_]
        y = flat[:rows * ld].reshape(rows, ld)[:, :n * Cc]
    out = dict(y=Out(y, S_y, f[0]['y'].gam, 'bfloat16', 'ln_y'))
    for kk, grp in (('mean', 'ln_mean'), ('rstd', 'ln_rstd')):
        val = np.stack([o[kk].value for o in f])
        if mutant == 'cat_stats_rows_major':
            val = np.ascontiguousarray(val.T).reshape(n, rows)
        out[kk] = Out(val, np.stack([o[kk].S for o in f]), f[0][kk].gam, 'float32', grp)
    if stats is None:
        stats = (np.stack([o['mean'].value for o in f]).astype(F32), np.stack([o['rstd'].value for o in f]).astype(F32))
    mean, rstd = stats
    if mutant == 'cat_stats_rows_major':             # the backward reads mean[row * n + i]
        pick = lambda a, i: np.asarray(a).reshape(-1)[np.arange(rows) * n + i]                   # noqa: E731
    else:
        pick = lambda a, i: np.asarray(a)[i]                                                      # noqa: E731
    dr, S_dr, parts, S_parts = np.zeros((rows, Cc), dt), np.zeros((rows, Cc)), [], []
    gam = fwd_gamma(Cc, 1 + int(bool(case['p'])))
    for i in range(n):
        k = _bwd_core(v['dcat'][:, i * Cc:(i + 1) * Cc], v['xs'][i], v['res'], v['gammas'][i], pick(mean, i), pick(rstd, i),
                      case['p'], keeps[i], 8, dt, mutant)
        if i not in case['dx_null']:
            out['dx%d' % i] = _dx_out(k, keeps[i], case['p'], gam, 'bfloat16', dt)
        dr = k['dz'] if mutant == 'cat_dres_last_problem_only' else (dr + k['dz']).astype(dt)
        S_dr = S_dr + k['S_dz']
        part, S_part = _partials(k, dt, mutant)
        parts.append(part)
        S_parts.append(S_part)
        if not case['dgamma_null']:
            s = finish_fold(part, dt, mutant)
            d0 = np.concatenate([v['dg0'][i], v['db0'][i]]).astype(dt)
            val = s if mutant == 'cat_dgamma_stored' else (d0 + s).astype(dt)
            S = S_part.sum(0) + np.abs(np.asarray(d0, F64))
            g_ = dparam_gamma(part.shape[0])
            out['dgamma%d' % i] = Out(val[:Cc], S[:Cc], g_, 'float32', 'ln_dparam')
            out['dbeta%d' % i] = Out(val[Cc:], S[Cc:], g_, 'float32', 'ln_dparam')
    if not case['dres_null']:
        out['dres'] = Out(dr, S_dr, gam + n, 'bfloat16', 'cat_dres')
    out['partial'] = Out(np.stack(parts), np.stack(S_parts), 8, 'float32', 'ln_partial')
    return out


# ================================================================ tell_layernorm_rows
def sk_wave_fold(v, dt):
    """sk_wave_sum of csrc/decode.hip over [..., 64]: xor 1, 2 inside a quad, the two mirrors (xor 4, xor 8 once a quad agrees),
    then the four rows of 16 lanes, (r0 + r1) + (r2 + r3)"""
    idx = np.arange(64)
    for o in (1, 2, 4, 8):
        v = (v + v[..., idx ^ o]).astype(dt)
    return ((v[..., 0] + v[..., 16]).astype(dt) + (v[..., 32] + v[..., 48]).astype(dt)).astype(dt)


def _rows_sum(t, dt, mutant=None):
    """the block's sum of t [M, C]: thread tid holds t[tid * 4 + j * 1024 ..+ 4], (a + b) + (c + d) per float4, float4 after
    float4, the wave fold, (w0 + w1) + (w2 + w3)"""
    t = np.asarray(t, dt)
    if dt is F64 and mutant is None:
        return t.sum(-1)
    M, Cc = t.shape
    q = t.reshape(M, Cc // 1024, 256, 4)
    acc = np.zeros((M, 256), dt)
    for j in range(Cc // 1024):
        acc = (acc + ((q[:, j, :, 0] + q[:, j, :, 1]).astype(dt) + (q[:, j, :, 2] + q[:, j, :, 3]).astype(dt)).astype(dt)).astype(dt)
    w = sk_wave_fold(acc.reshape(M, 4, 64), dt)
    w3 = dt(0) if mutant == 'rows_fourth_wave_left_out_of_mean' else w[:, 3]
    return ((w[:, 0] + w[:, 1]).astype(dt) + (w[:, 2] + w3).astype(dt)).astype(dt)


def ln_rows(x, gamma, beta, eps, stats_null=False, dt=F64, mutant=None):
    """fp32 x [M, C] -> y bf16, stats [M, 2] = (mean, rstd) unless stats_out is null"""
    x, gamma, beta = np.asarray(x, dt), np.asarray(gamma, dt), np.asarray(beta, dt)
    M, Cc = x.shape
    with np.errstate(all='ignore'):
        mu = (_rows_sum(x, dt, mutant) / dt(Cc)).astype(dt)
        d = (x - mu[:, None]).astype(dt)
        var = (_rows_sum((d * d).astype(dt), dt) / dt(Cc)).astype(dt)
        rs = _rsqrt((var + dt(np.float32(eps))).astype(dt), dt)
        y = (((d * rs[:, None]).astype(dt) * gamma).astype(dt) + beta).astype(dt)
    gam = Cc // 1024 + 2 + 6 + 2 + 8
    S_m, S_r, S_y = _fwd_S(x, np.abs(np.asarray(x, F64)), mu, var, rs, gamma, beta, eps, 0, gam)
    out = dict(y=Out(y, S_y, gam, 'bfloat16', 'rows_y'))
    if not stats_null:
        st, S = np.stack([mu, rs], 1), np.stack([S_m, S_r], 1)
        if mutant == 'rows_stats_index_without_2':                  # stats_out[m] = mean, stats_out[m + 1] = rstd, row after row
            flat = np.full(2 * M, SENTINEL, st.dtype)
            for m in range(M):
                flat[m], flat[m + 1] = mu[m], rs[m]
            st = flat.reshape(M, 2)
        out['stats'] = Out(st, S, gam, 'float32', 'rows_stats')
    return out


ROWS = [
    dict(id='m1_c1024', M=1, C=1024, pad_x=0, pad_y=0, stats_null=False, eps=1e-5, mutants=('rows_fourth_wave_left_out_of_mean',)),
    dict(id='m5_c2048', M=5, C=2048, pad_x=4, pad_y=0, stats_null=True, eps=1e-12, mutants=('rows_fourth_wave_left_out_of_mean',)),
    dict(id='m33_c3072', M=33, C=3072, pad_x=0, pad_y=4, stats_null=False, eps=1e-5, mutants=('rows_stats_index_without_2',)),
    dict(id='m5_c4096', M=5, C=4096, pad_x=4, pad_y=4, stats_null=False, eps=1e-5,
         mutants=('rows_stats_index_without_2', 'rows_fourth_wave_left_out_of_mean')),
]


def rows_paths(case):
    M = case['M']
    return {'rows:float4_per_thread:%d' % (case['C'] // 1024), 'rows:ld_x>C' if case['pad_x'] else 'rows:ld_x=C',
            'rows:ld_y>C' if case['pad_y'] else 'rows:ld_y=C', 'rows:stats_null' if case['stats_null'] else 'rows:stats',
            'rows:one_row' if M == 1 else 'rows:several_rows'}


def rows_inputs(case):
    def make():
        r, M, Cc = _rng('lnrows', case['id']), case['M'], case['C']
        x, _ = rows_of_kinds(r, M, Cc, 1 if M == 1 else 0, False)
        gamma, beta = affine(r, Cc)
        return dict(x=np.asarray(x, F32), gamma=gamma, beta=beta)
    return cached(('lnrows_in', case['id']), make)


def rows_case(case, dt=F64, mutant=None, stats_null=None):
    v = rows_inputs(case)
    return ln_rows(v['x'], v['gamma'], v['beta'], case['eps'], case['stats_null'] if stats_null is None else stats_null, dt, mutant)
