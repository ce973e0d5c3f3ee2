"""float64 reference of the copy-mechanism kernels (csrc/copy.hip), the element-wise bounds they are held to and the
case table that tests/test_copy_ref_host.py and tests/test_gpu_copy.py both walk.  numpy only;
nothing here comes from oracle/.  Inputs are rounded to the compute dtype BEFORE they reach a function.

Every function returns, beside each value, the sum of the ABSOLUTE values of the terms the kernel adds up for it (S_*).
Bound of one output element, as in section 23:

    u_out |ref|  +  c gamma 2^-24 S  +  2^-126 (1 + S)

u_out = 2^-8 for a bf16 store, 2^-24 for fp32; gamma = the element's operation count, read off the kernel (the table below);
c = the one measured number per output (MEASURED, C).  Every function takes dt (np.float64: the reference; np.float32:
the same formulas with every product, exp and sequential sum rounded to fp32 - the emulation the host test holds to the
bounds at c = 1) and a mutant name (MUTANTS: wrong-answer variants that must break a bound).

gamma.  A probability exp(lg - lse) has the relative error of its argument: the logit is an fp32 dot product of D terms,
off by at most D 2^-24 L with L = sum_d |q_d k_d|, and __expf scales its argument, which costs about |lg - lse| ulps.
So   gP = 8 + spread + D Lmax   (spread = largest |lg - lse| of the case, Lmax = largest L) is the relative error count
of one probability on a GIVEN lse; a probability on the kernel's own lse carries 2 gP.

    copy attention   w: H + 8 + 2 gP          lse: 16 + gP (S = 1 + |lse|)
                     delta: 16 + gP           dq: S/4 + 24 + 2 gP     dk: T + 16 + 2 gP     dbias_k_rows: 16 + 2 gP
    copy loss        n = longest chain of equal ids;  p_target: n + 2     z: n + S/256 + 12     term: n + S/256 + 16
                     (S_term = |log p| + |log z| + 2: the relative errors of p and z arrive as absolute ones)
                     scale: 2     loss: term's + B T/256 + 12 + max index     dw: n + S/256 + 20
    entity head      logits: E/64 + 10     loss: logits' + B T/256 + 24     dlogits: 16     dx: 40
                     dw, dbias: B T/4 + 40   (their S built on S_dlogits = |g| (softmax + onehot): the difference cancels)
    causal           n = keys seen;  out: 2 n + 8 + 2 gP     lse: n + 8 + gP (S = 1 + |lse|)     delta: 8
                     dq, dk: T + 24 + 2 gP     dv: T + 8 + gP
    copy step        prob: H + n + 8 + 2 gP

Measured on the MI355X: MEASURED and C below, and DESIGN.md section 26.
"""
import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -126
U_OUT = {'float32': 2.0 ** -24, 'bfloat16': 2.0 ** -8}
NT, NW, MAX_S = 256, 4, 512
SEED, SALT = 9, 101

# largest observed (|got - ref| - u_out |ref|) / (gamma 2^-24 S) over the GPU grid of tests/test_gpu_copy.py on the MI355X
# (both dtypes, every case of the tables below, p = 0, 0.1 and 0.5, the two cases through ops) and the pinned constant:
# four times that, rounded up to a power of two.  scale and ent_db never left u_out |ref| (ratio <= 0): they get the
# smallest constant, 2^-10.  An output missing from MEASURED is not pinned: the GPU test then fails with the measured ratio
# in its message.
MEASURED = {'w': 0.125590, 'lse': 0.021451, 'delta': 0.044071, 'dq': 0.019601, 'dk': 0.039610, 'dbk': 0.045157,
            'p_target': 0.045410, 'z': 0.024003, 'term': 0.052428, 'scale': 0.0, 'loss': 0.003193, 'loss_dw': 0.050851,
            'ent_logits': 0.048579, 'ent_loss': 0.000419, 'ent_dlogits': 0.498477, 'ent_dx': 0.047136, 'ent_dw': 0.029067,
            'ent_db': 0.0, 'c_out': 0.010326, 'c_lse': 0.007899, 'c_delta': 0.064876, 'c_dq': 0.003061, 'c_dk': 0.003654,
            'c_dv': 0.025421, 'prob': 0.022217}


def _pin(r):
    return 2.0 ** -10 if r <= 0 else 2.0 ** int(np.ceil(np.log2(4.0 * r)))


C = {k: _pin(v) for k, v in MEASURED.items()}

OUTPUTS = ('w', 'lse', 'delta', 'dq', 'dk', 'dbk',
           'p_target', 'z', 'term', 'scale', 'loss', 'loss_dw',
           'ent_logits', 'ent_loss', 'ent_dlogits', 'ent_dx', 'ent_dw', 'ent_db',
           'c_out', 'c_lse', 'c_delta', 'c_dq', 'c_dk', 'c_dv', 'prob')

MUTANTS = ('keep_row', 'proper_gt1', 'dq_no_bias', 'causal_sees_self', 'chain_drop_last', 'tie_high', 'drop_col_256',
           'causal_scale_once')


def _sum(a, axis, dt):
    """sequential sum along axis (np.sum adds pairwise; the kernels' loops do not)"""
    a = np.asarray(a, dtype=dt)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), dtype=dt)
    return np.take(np.add.accumulate(a, axis=axis, dtype=dt), -1, axis=axis)


def bound(out, ref, S, dtype, gam, c=None):
    c = C[out] if c is None else c
    ref, S = np.asarray(ref, np.float64), np.asarray(S, np.float64)
    return U_OUT[dtype] * np.abs(ref) + c * gam * EPS * S + TINY * (1.0 + S)


def ratio(got, ref, S, dtype, gam):
    """largest (|got - ref| - u_out |ref|) / (gamma 2^-24 S) over the finite reference elements with S > 0"""
    got, ref, S = (np.asarray(a, np.float64) for a in (got, ref, S))
    ref, S = np.broadcast_to(ref, got.shape), np.broadcast_to(S, got.shape)
    ok = np.isfinite(ref) & (gam * EPS * S > 0)
    if not ok.any():
        return 0.0
    num = np.abs(got - ref)[ok] - U_OUT[dtype] * np.abs(ref[ok]) - TINY * (1.0 + S[ok])
    return float((num / (gam * EPS * S[ok])).max())


def np64(t):
    return t.detach().double().cpu().numpy()


# ---------------------------------------------------------------- dropout
def keep_factors(seed, salt, B, H, T, S, p, mutant=None):
    """[B,H,T,S+2] float64 of 0 or the fp32 value of 1/(1-p): element ((b H + h) T + t)(S + 2) + s of
    tell_amd.rng.keep_mask.  None for p = 0.  mutant 'keep_row': the row length S instead of S + 2."""
    if not p > 0:
        return None
    from tell_amd import rng
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    row = S if mutant == 'keep_row' else S + 2
    idx = (np.arange(B * H * T, dtype=np.uint64)[:, None] * np.uint64(row) + np.arange(S + 2, dtype=np.uint64)[None])
    return rng.keep_mask(seed, salt, idx.reshape(-1), p).astype(np.float64).reshape(B, H, T, S + 2) * float(inv)


# ---------------------------------------------------------------- copy attention
def _heads(x, H):
    """[N,B,E] -> [B,H,N,D]"""
    N, B, E = x.shape
    return x.reshape(N, B, H, E // H).transpose(1, 2, 0, 3)


def _copy_logits(q, k, bias_k, mask, H, dt, mutant=None):
    """-> qh [B,H,T,D], kx [B,H,S+2,D] (bias_k and the zero key appended), lg, L [B,H,T,S+2] (masked: -inf)"""
    q, k, bias_k = (np.asarray(a, dtype=dt) for a in (q, k, bias_k))
    T, B, E = q.shape
    S, D = k.shape[0], E // H
    qh = _heads(q, H)
    kx = np.concatenate([_heads(k.reshape(S, B, E), H), np.broadcast_to(bias_k.reshape(1, H, 1, D), (B, H, 1, D)),
                         np.zeros((B, H, 1, D), dt)], 2)
    prod = qh[:, :, :, None, :] * kx[:, :, None, :, :]
    lg, L = _sum(prod, -1, dt), _sum(np.abs(prod), -1, dt)
    dead = np.zeros((B, S + 2), bool)
    if mask is not None:
        dead[:, :S] = np.asarray(mask).reshape(B, S) != 0
    if mutant == 'drop_col_256' and S > 256:
        dead[:, 256] = True
    lg = np.where(dead[:, None, None, :], -np.inf, lg).astype(dt)
    return qh, kx, lg, L


def _proper_ok(proper, B, S, mutant=None):
    if proper is None:
        return np.ones((B, S), bool)
    proper = np.asarray(proper).reshape(B, S)
    return proper > 1 if mutant == 'proper_gt1' else proper >= 1


def _stats(lg, lse, L):
    fin = np.isfinite(lg)
    spread = float(np.abs(np.where(fin, lg - lse[..., None], 0.0)).max()) if lg.size else 0.0
    return dict(spread=spread, Lmax=float(L.max()) if L.size else 0.0)


def g_p(st, D):
    return 8.0 + st['spread'] + D * st['Lmax']


def copy_attn_fwd(q, k, bias_k, mask, proper, H, keep=None, dt=np.float64, mutant=None):
    """q [T,B,E] (scaled), k [S,B,E], bias_k [E], mask [B,S] (non-zero = padding) or None, proper [B,S] or None,
    keep from keep_factors -> dict w [B,T,S], S_w, lse [B,H,T], S_lse, P [B,H,T,S+2] (the per-head probabilities, no
    dropout), spread, Lmax"""
    T, B, E = np.shape(q)
    S = np.shape(k)[0]
    qh, kx, lg, L = _copy_logits(q, k, bias_k, mask, H, dt, mutant)
    m = lg.max(-1)
    lse = (m + np.log(_sum(np.exp(lg - m[..., None]), -1, dt))).astype(dt)
    P = np.exp(lg - lse[..., None]).astype(dt)
    pk = P[..., :S] if keep is None else P[..., :S] * np.asarray(keep, dt)[..., :S]
    w = _sum(pk, 1, dt) * dt(1.0 / H) if dt is np.float32 else _sum(pk, 1, dt) / H
    w = np.where(_proper_ok(proper, B, S, mutant)[:, None, :], w, 0.0)
    out = dict(w=w, S_w=np.abs(w), lse=lse, S_lse=1.0 + np.abs(lse), P=P)
    out.update(_stats(lg, lse, L))
    return out


def copy_attn_bwd(q, k, bias_k, mask, proper, H, keep, lse, dw, dt=np.float64, mutant=None):
    """the backward on a GIVEN lse [B,H,T] (the GPU test passes the kernel's own, so the forward's error is not charged
    here) and dw [B,T,S] -> dict dq [T,B,E], dk [S,B,E], dbk [B T, E], delta [B,H,T] and their S_*"""
    T, B, E = np.shape(q)
    S, D = np.shape(k)[0], E // H
    qh, kx, lg, L = _copy_logits(q, k, bias_k, mask, H, dt, mutant)
    lse = np.asarray(lse, dt).reshape(B, H, T)
    P = np.exp(lg - lse[..., None]).astype(dt)
    dp = np.zeros_like(P)
    d = np.broadcast_to((np.asarray(dw, dt).reshape(B, 1, T, S) * dt(1.0 / H)), (B, H, T, S)).astype(dt)
    if keep is not None:
        d = d * np.asarray(keep, dt)[..., :S]
    dp[..., :S] = np.where(_proper_ok(proper, B, S, mutant)[:, None, None, :], d, 0.0)
    delta, S_delta = _sum(P * dp, -1, dt), _sum(P * np.abs(dp), -1, dt)
    dl = P * (dp - delta[..., None])
    S_dl = P * (np.abs(dp) + S_delta[..., None])
    n = S if mutant == 'dq_no_bias' else S + 1
    dq = _sum(dl[..., :n, None] * kx[:, :, None, :n, :], 3, dt)
    S_dq = _sum(S_dl[..., :n, None] * np.abs(kx[:, :, None, :n, :]), 3, dt)
    dk = _sum(dl[..., :S, None] * qh[:, :, :, None, :], 2, dt)
    S_dk = _sum(S_dl[..., :S, None] * np.abs(qh[:, :, :, None, :]), 2, dt)
    dbk, S_dbk = dl[..., S, None] * qh, S_dl[..., S, None] * np.abs(qh)

    def tbe(x):                              # [B,H,N,D] -> [N,B,E]
        return x.transpose(2, 0, 1, 3).reshape(x.shape[2], B, E)

    def rows(x):                             # [B,H,T,D] -> [B T, E]
        return x.transpose(0, 2, 1, 3).reshape(B * T, E)
    out = dict(dq=tbe(dq), S_dq=tbe(S_dq), dk=tbe(dk), S_dk=tbe(S_dk), dbk=rows(dbk), S_dbk=rows(S_dbk), delta=delta,
               S_delta=S_delta)
    out.update(_stats(lg, lse, L))
    return out


def attn_gamma(out, st, H, T, S, D):
    g = g_p(st, D)
    return {'w': H + 8 + 2 * g, 'lse': 16 + g, 'delta': 16 + g, 'dq': S / 4.0 + 24 + 2 * g, 'dk': T + 16 + 2 * g,
            'dbk': 16 + 2 * g}[out]


# ---------------------------------------------------------------- copy loss
def _chains(ids):
    """{id: [positions, increasing]} in order of first occurrence"""
    ch = {}
    for s, v in enumerate(ids):
        ch.setdefault(int(np.int32(v)), []).append(s)           # the kernel keeps (int)id
    return ch


def vocab_count(ctx, tgt, vocab):
    """the number of distinct ids of cat(ctx, tgt), an exact integer; -1 when an id lies outside [0, vocab)"""
    ids = np.concatenate([np.asarray(ctx).reshape(-1), np.asarray(tgt).reshape(-1)]).astype(np.int64)
    if ((ids < 0) | (ids >= vocab)).any():
        return -1
    return int(len(set(ids.tolist())))


def copy_loss(w, ctx, tgt, cm, variant, V, dloss=0.37, dt=np.float64, mutant=None):
    """w [B,T,S] is taken AS GIVEN (fp32 values, non-negative, with exact zeros), so every p > 0 decision is exact in both
    precisions: a chain of non-negative terms is zero only if every term is.  ctx [B,S], tgt, cm [B,T] integers; V: the
    vocabulary count (variant 2; V < 0 gives NaN terms).  Duplicates are summed in increasing position order.  An entity
    index in 1 .. max without rows gives a NaN loss.  -> dict term, p_target, z, scale [B,T], loss, dw [B,T,S], their S_*
    and n (the longest chain)"""
    w = np.asarray(w, dt)
    B, T, S = w.shape
    ctx, tgt, cm = np.asarray(ctx).reshape(B, S), np.asarray(tgt).reshape(B, T), np.asarray(cm).reshape(B, T)
    o = {k: np.zeros((B, T), dt) for k in ('term', 'p_target', 'z', 'scale', 'S_term', 'S_z')}
    dw, S_dw = np.zeros((B, T, S), dt), np.zeros((B, T, S), dt)
    Vf = dt(V if variant == 2 else 0.0)
    nmax, pos_of = 1, {}
    for b in range(B):
        ch = _chains(ctx[b])
        nmax = max([nmax] + [len(v) for v in ch.values()])
        for t in range(T):
            if cm[b, t] < 1:
                continue
            pt, zsum, npos, live = dt(0.0), dt(0.0), 0, np.zeros(S, bool)
            for v, ps in ch.items():
                use = ps[:-1] if mutant == 'chain_drop_last' else ps
                p = _sum(w[b, t, use], 0, dt)
                if v == int(np.int32(tgt[b, t])):
                    pt = p
                if p > 0:
                    npos, zsum = npos + 1, dt(zsum + p)
                    live[ps] = True
            z = dt(zsum + (Vf - dt(npos)))
            with np.errstate(all='ignore'):
                lp = np.log(pt) if pt > 0 else dt(0.0)
                lz = np.log(z) if variant == 2 else dt(0.0)
                o['term'][b, t] = (np.nan if Vf < 0 else -lp + lz) if variant == 2 else -lp
            o['S_term'][b, t] = abs(lp) + (abs(lz) if np.isfinite(lz) else 0.0) + 2.0
            o['p_target'][b, t], o['z'][b, t], o['S_z'][b, t] = pt, z, zsum + abs(Vf - npos)
            pos_of[(b, t)] = live
    top = int(max(cm.max(), 0))
    loss, S_loss = dt(0.0), 0.0
    with np.errstate(all='ignore'):
        for i in range(1, top + 1):
            sel = cm == i
            c = dt(sel.sum())
            loss = dt(loss + _sum(o['term'][sel], 0, dt) / c)
            S_loss += float(o['S_term'][sel].sum() / c) if sel.any() else 0.0
            o['scale'][sel] = dt(1.0) / c
        for (b, t), live in pos_of.items():
            g = dt(dloss) * o['scale'][b, t]
            pt = o['p_target'][b, t]
            gt = -g / pt if pt > 0 else dt(0.0)
            tpos = ctx[b].astype(np.int32) == np.int32(tgt[b, t])
            if variant == 2:
                gz = g / o['z'][b, t]
                dw[b, t] = np.where(live, gz, 0.0) + np.where(tpos, gt, 0.0)
                S_dw[b, t] = np.where(live, abs(gz), 0.0) + np.where(tpos, abs(gt), 0.0)
            else:
                dw[b, t] = np.where(tpos, gt, 0.0)
                S_dw[b, t] = np.abs(dw[b, t])
    o.update(loss=loss, S_loss=S_loss, dw=dw, S_dw=S_dw, n=nmax, S_p_target=np.abs(o['p_target']),
             S_scale=np.abs(o['scale']), top=top)
    return o


def loss_gamma(out, n, B, T, S, top):
    a = n + S / 256.0
    return {'p_target': n + 2, 'z': a + 12, 'term': a + 16, 'scale': 2, 'loss': a + 16 + B * T / 256.0 + 12 + top,
            'loss_dw': a + 20}[out]


# ---------------------------------------------------------------- entity head
def entity_head(x, w, bias, cm, dloss=0.37, logits=None, dbias0=None, dt=np.float64, mutant=None):
    """x [T,B,E], w [2,E], bias [2], cm [B,T] (-1: ignored, >= 1: class 1) -> dict logits [B,T,2], loss, nvalid, and the
    backward on `logits` if given (the GPU test passes the kernel's own), else on its own: dlogits [B,T,2], dx [T,B,E],
    dw [2,E], dbias [2] (added to dbias0), with their S_*"""
    x, w, bias = np.asarray(x, dt), np.asarray(w, dt), np.asarray(bias, dt)
    T, B, E = x.shape
    cm = np.asarray(cm).reshape(B, T)
    prod = x.transpose(1, 0, 2)[:, :, None, :] * w[None, None]                    # B T 2 E
    lg = _sum(prod, -1, dt) + bias
    S_lg = _sum(np.abs(prod), -1, dt) + np.abs(bias)
    own = lg if logits is None else np.asarray(logits, dt).reshape(B, T, 2)
    valid = cm != -1
    cls = (cm >= 1).astype(int)

    def ce(l):
        m = l.max(-1)
        return m + np.log(np.exp(l[..., 0] - m) + np.exp(l[..., 1] - m))
    with np.errstate(all='ignore'):
        lz = ce(lg)
        lt = np.take_along_axis(lg, cls[..., None], -1)[..., 0]
        n = dt(valid.sum())
        loss = _sum((lz - lt)[valid], 0, dt) / n
        S_loss = float((S_lg.sum(-1) + np.abs(lz) + np.abs(lt))[valid].sum() / n) if valid.any() else 0.0
        sm = np.exp(own - ce(own)[..., None])
        hot = np.eye(2, dtype=dt)[cls]
        g = dt(dloss) / n
        dl = np.where(valid[..., None], g * (sm - hot), 0.0).astype(dt)
        S_dl = np.where(valid[..., None], np.abs(g) * (sm + hot), 0.0)
    dxp = dl[..., None] * w[None, None]                                            # B T 2 E
    # S of everything downstream is built on S_dlogits, not |dlogits|: softmax - onehot cancels
    dx, S_dx = _sum(dxp, 2, dt).transpose(1, 0, 2), _sum(S_dl[..., None] * np.abs(w[None, None]), 2, dt).transpose(1, 0, 2)
    # rows in the kernel's order r = t B + b
    dlr = dl.transpose(1, 0, 2).reshape(T * B, 2)
    xr = x.reshape(T * B, E)
    dwp = dlr[:, :, None] * xr[:, None, :]
    S_dlr = S_dl.transpose(1, 0, 2).reshape(T * B, 2)
    db0 = np.zeros(2, dt) if dbias0 is None else np.asarray(dbias0, dt)
    return dict(logits=lg, S_logits=S_lg, loss=loss, S_loss=S_loss, nvalid=float(n), dlogits=dl, S_dlogits=S_dl, dx=dx,
                S_dx=S_dx, dw=_sum(dwp, 0, dt), S_dw=_sum(S_dlr[:, :, None] * np.abs(xr[:, None, :]), 0, dt),
                dbias=db0 + _sum(dlr, 0, dt), S_dbias=np.abs(db0) + _sum(S_dlr, 0, dt))


def ent_gamma(out, B, T, E):
    lg = E / 64.0 + 10
    return {'ent_logits': lg, 'ent_loss': lg + B * T / 256.0 + 24, 'ent_dlogits': 16, 'ent_dx': 40,
            'ent_dw': B * T / 4.0 + 40, 'ent_db': B * T / 4.0 + 40}[out]


# ---------------------------------------------------------------- causal entity attention
def _causal_logits(q, k, scale, pos0, S, H, dt, mutant=None):
    q, k = np.asarray(q, dt), np.asarray(k, dt)[:S]
    Tq = q.shape[0]
    qh, kh = _heads(q * dt(scale), H), _heads(k, H)
    prod = qh[:, :, :, None, :] * kh[:, :, None, :, :]                            # B H Tq S D
    lg, L = _sum(prod, -1, dt), _sum(np.abs(prod), -1, dt)
    n = np.minimum(pos0 + np.arange(Tq) + (1 if mutant == 'causal_sees_self' else 0), S)
    vis = np.arange(S)[None, :] < n[:, None]
    lg = np.where(vis[None, None], lg, -np.inf).astype(dt)
    L = np.where(vis[None, None], L, 0.0)
    return qh, kh, lg, L, vis


def causal(q, k, v, scale, pos0, S, H, dt=np.float64, mutant=None):
    """query i at position pos0 + i sees keys s < min(pos0 + i, S) and a slot of logit 0 and value 0.  q [Tq,B,E]
    (unscaled), k, v [>= S, B, E] -> dict out [Tq,B,E], S_out, lse [B,H,Tq], S_lse, spread, Lmax, n"""
    Tq, B, E = np.shape(q)
    qh, kh, lg, L, vis = _causal_logits(q, k, scale, pos0, S, H, dt, mutant)
    vh = _heads(np.asarray(v, dt)[:S], H)
    m = np.maximum(lg.max(-1), 0.0) if S else np.zeros(lg.shape[:3], dt)
    l = np.exp(-m) + _sum(np.exp(lg - m[..., None]), -1, dt)
    lse = (m + np.log(l)).astype(dt)
    P = np.exp(lg - lse[..., None]).astype(dt)
    t = P[..., None] * vh[:, :, None, :, :]
    out, S_out = _sum(t, 3, dt), _sum(np.abs(t), 3, dt)

    def tbe(x):
        return x.transpose(2, 0, 1, 3).reshape(Tq, B, E)
    o = dict(out=tbe(out), S_out=tbe(S_out), lse=lse, S_lse=1.0 + np.abs(lse), n=int(vis.sum(1).max()) if S else 0)
    o.update(_stats(lg, lse, L))
    return o


def causal_bwd(q, k, v, out, dout, lse, scale, H, dt=np.float64, mutant=None):
    """training backward (Tq = S = T, pos0 = 0) on the GIVEN out [T,B,E] and lse [B,H,T] (the kernel's own in the GPU
    test) -> dict dq, dk, dv [T,B,E], delta [B,H,T] and their S_*"""
    T, B, E = np.shape(q)
    qh, kh, lg, L, vis = _causal_logits(q, k, scale, 0, T, H, dt, mutant)
    vh, oh, gh = (_heads(np.asarray(a, dt), H) for a in (v, out, dout))
    lse = np.asarray(lse, dt).reshape(B, H, T)
    P = np.exp(lg - lse[..., None]).astype(dt)                                     # B H T S
    delta, S_delta = _sum(gh * oh, -1, dt), _sum(np.abs(gh * oh), -1, dt)
    gv = gh[:, :, :, None, :] * vh[:, :, None, :, :]
    dp, S_dp = _sum(gv, -1, dt), _sum(np.abs(gv), -1, dt)
    dl = P * (dp - delta[..., None])
    S_dl = P * (S_dp + S_delta[..., None])
    sc = dt(1.0) if mutant == 'causal_scale_once' else dt(scale)
    dq = _sum(dl[..., None] * kh[:, :, None, :, :], 3, dt) * sc
    S_dq = _sum(S_dl[..., None] * np.abs(kh[:, :, None, :, :]), 3, dt) * abs(scale)
    dk = _sum(dl[..., None] * qh[:, :, :, None, :], 2, dt)                         # (qh carries the scale)
    S_dk = _sum(S_dl[..., None] * np.abs(qh[:, :, :, None, :]), 2, dt)
    dv = _sum(P[..., None] * gh[:, :, :, None, :], 2, dt)
    S_dv = _sum(P[..., None] * np.abs(gh[:, :, :, None, :]), 2, dt)

    def tbe(x):
        return x.transpose(2, 0, 1, 3).reshape(T, B, E)
    o = dict(dq=tbe(dq), S_dq=tbe(S_dq), dk=tbe(dk), S_dk=tbe(S_dk), dv=tbe(dv), S_dv=tbe(S_dv), delta=delta,
             S_delta=S_delta)
    o.update(_stats(lg, lse, L))
    return o


def causal_gamma(out, st, n, T, D=64):
    g = g_p(st, D)
    return {'c_out': 2 * n + 8 + 2 * g, 'c_lse': n + 8 + g, 'c_delta': 8, 'c_dq': T + 24 + 2 * g, 'c_dk': T + 24 + 2 * g,
            'c_dv': T + 8 + g}[out]


# ---------------------------------------------------------------- the copy decision of one generation step
def copy_step(q, k, bias_k, mask, proper, ctx, rows, ent, gen, hist, n_hist, H, dt=np.float64, mutant=None):
    """q [Ba,E] (scaled), k [S,B,E], mask / proper / ctx [B,S], rows [Ba], ent [Ba,2], gen [Ba], hist [B,hist_len] ->
    dict tok, copied, prob [Ba], S_prob, hist_col [B] (what hist[:, n_hist] holds afterwards; untouched rows keep theirs),
    gap [Ba] (best minus second-best per-id sum, inf with fewer than two ids), best_id, gam [Ba]"""
    q, k = np.asarray(q, dt), np.asarray(k, dt)
    Ba, E = q.shape
    S, B, D = k.shape[0], k.shape[1], E // H
    ctx, hist = np.asarray(ctx).reshape(B, S), np.asarray(hist)
    col = hist[:, n_hist].copy()
    o = dict(tok=np.zeros(Ba, np.int64), copied=np.zeros(Ba, bool), prob=np.zeros(Ba, dt), gap=np.full(Ba, np.inf),
             best_id=np.zeros(Ba, np.int64), gam=np.zeros(Ba))
    for i in range(Ba):
        b = int(rows[i])
        f = copy_attn_fwd(q[i].reshape(1, 1, E), k[:, b:b + 1], bias_k, None if mask is None else np.asarray(mask)[b:b + 1],
                          None if proper is None else np.asarray(proper)[b:b + 1], H, None, dt,
                          mutant if mutant in ('proper_gt1', 'drop_col_256') else None)
        w = f['w'][0, 0]
        ch = _chains(ctx[b])
        sums = []
        for v, ps in ch.items():
            use = ps[:-1] if mutant == 'chain_drop_last' else ps
            sums.append((_sum(w[use], 0, dt), v))
        n = max([1] + [len(ps) for ps in ch.values()])
        if sums:
            top = max(p for p, _ in sums)
            tied = [v for p, v in sums if p == top]
            bid = max(tied) if mutant == 'tie_high' else min(tied)
            rest = [p for p, v in sums if v != bid]
            o['gap'][i] = float(top - max(rest)) if rest else np.inf
        else:
            top, bid = dt(-1.0), 0
        empty = top < dt(np.float32(1e-6))
        p = dt(np.float32(1e-6)) if empty else top
        should = bool(ent[i][1] > ent[i][0]) and not empty and bid not in hist[b, :n_hist].tolist()
        col[b] = bid if should else -1
        o['tok'][i], o['copied'][i], o['prob'][i], o['best_id'][i] = (bid if should else int(gen[i])), should, p, bid
        o['gam'][i] = H + n + 8 + 2 * g_p(f, D)
    o.update(S_prob=np.abs(o['prob']), hist_col=col)
    return o


# ================================================================ the case table
def _round(t, dtype):
    import torch
    return t.to(getattr(torch, dtype)).double().numpy()


def _gen(seed):
    import torch
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    import torch
    return torch.randn(*shape, generator=g)


P_DROP = (0.0, 0.1, 0.5)
DTYPES = ('float32', 'bfloat16')

# copy attention: id, (B,H,T,S,D), mask pattern, proper pattern, layout, logit scale
#   mask:   none | padrow (batch row 1 fully padded) | tail (the last third of batch row 1 padded)
#   proper: none | mixed (-1, 0, 1, 2 in turn) | zero_row (batch row 0 all zero, the others mixed)
#   layout: dense | q_third (q = the first third of a [T,B,3E] buffer) | k_half (k = the second half of [S,B,2E]) |
#           k_bse (k stored [B,S,E], viewed [S,B,E]: k_sb > k_ss)
ATTN = [dict(id='S0', shape=(2, 3, 1, 0, 64), mask='none', proper='none', layout='dense'),
        dict(id='S1', shape=(2, 3, 5, 1, 64), mask='none', proper='none', layout='q_third'),
        dict(id='S24', shape=(2, 2, 9, 24, 64), mask='padrow', proper='mixed', layout='k_half'),
        dict(id='S63', shape=(2, 2, 4, 63, 64), mask='tail', proper='zero_row', layout='k_bse'),
        dict(id='S64', shape=(2, 2, 4, 64, 64), mask='none', proper='mixed', layout='dense'),
        dict(id='S65', shape=(2, 2, 4, 65, 64), mask='padrow', proper='none', layout='q_third'),
        dict(id='S255', shape=(2, 2, 4, 255, 64), mask='tail', proper='mixed', layout='k_half'),
        dict(id='S256', shape=(2, 2, 4, 256, 64), mask='none', proper='zero_row', layout='k_bse'),
        dict(id='S257', shape=(2, 2, 4, 257, 64), mask='tail', proper='mixed', layout='dense'),
        dict(id='S300', shape=(2, 2, 4, 300, 64), mask='padrow', proper='mixed', layout='q_third'),
        dict(id='S511', shape=(2, 2, 4, 511, 64), mask='tail', proper='none', layout='k_half'),
        dict(id='S512', shape=(2, 2, 4, 512, 64), mask='tail', proper='mixed', layout='k_bse'),
        dict(id='D16', shape=(2, 3, 5, 40, 16), mask='tail', proper='mixed', layout='k_bse'),
        dict(id='D48', shape=(2, 3, 5, 257, 48), mask='tail', proper='mixed', layout='q_third'),
        dict(id='spread60', shape=(2, 2, 4, 65, 64), mask='tail', proper='mixed', layout='dense', scale=4.5)]

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _masks(B, S, mask, proper):
    m = None
    if mask != 'none':
        m = np.zeros((B, S), np.uint8)
        m[1 % B, (0 if mask == 'padrow' else S - S // 3):] = 1
    pr = None
    if proper != 'none':
        pr = (np.arange(B * S).reshape(B, S) % 4 - 1).astype(np.int8)            # -1, 0, 1, 2
        if proper == 'zero_row':
            pr[0] = 0
    return m, pr


def attn_inputs(case, dtype):
    """q [T,B,E], k [S,B,E], bias_k [E], dw [B,T,S] (float64 arrays holding values of `dtype`; dw fp32), mask, proper"""
    def make():
        B, H, T, S, D = case['shape']
        E = H * D
        g = _gen(1000 * S + 10 * T + D)
        a = 0.3 * case.get('scale', 1.0)
        q, k, bk = _round(_randn(g, T, B, E) * a, dtype), _round(_randn(g, S, B, E) * a, dtype), \
            _round(_randn(g, E) * a, dtype)
        dw = _round(_randn(g, B, T, S), 'float32')
        m, pr = _masks(B, S, case['mask'], case['proper'])
        return dict(q=q, k=k, bias_k=bk, dw=dw, mask=m, proper=pr)
    return cached(('attn', case['id'], dtype), make)


def attn_ref(case, dtype, p):
    """the float64 forward of a case, computed once and shared"""
    def make():
        B, H, T, S, D = case['shape']
        x = attn_inputs(case, dtype)
        keep = keep_factors(SEED, SALT, B, H, T, S, p)
        return keep, copy_attn_fwd(x['q'], x['k'], x['bias_k'], x['mask'], x['proper'], H, keep)
    return cached(('attn_ref', case['id'], dtype, p), make)


# copy loss: id, (B,T,S), what the ids hold, vocab
LOSS = [dict(id='S0', shape=(1, 3, 0), kind='plain', vocab=600),
        dict(id='S1', shape=(2, 3, 1), kind='plain', vocab=600),
        dict(id='rich', shape=(4, 10, 24), kind='rich', vocab=33),          # every content item of the issue's list
        dict(id='gap', shape=(4, 10, 24), kind='gap', vocab=33),            # entity index 2 missing: NaN
        dict(id='oov', shape=(4, 10, 24), kind='oov', vocab=33),            # an id >= vocab: count -1, NaN in variant 2
        dict(id='negative', shape=(4, 10, 24), kind='negative', vocab=33),  # a negative id
        dict(id='S257', shape=(2, 5, 257), kind='stride', vocab=600),       # one id at positions 0, 255, 256
        dict(id='S512_equal', shape=(2, 4, 512), kind='equal', vocab=600),  # one chain of 512
        dict(id='S512_distinct', shape=(2, 4, 512), kind='distinct', vocab=600),
        dict(id='rows300', shape=(3, 100, 40), kind='plain', vocab=600)]    # B T > 256: the reduce kernel loops


def loss_inputs(case):
    """w [B,T,S] fp32 values (non-negative, exact zeros), ctx [B,S], tgt, cm [B,T] int64, pads: tgt_sb - T, cm_sb - T"""
    def make():
        import torch
        B, T, S = case['shape']
        kind = case['kind']
        g = _gen(77 + S + T)
        w = torch.rand(B, T, S, generator=g)
        hi = 30 if case['vocab'] == 33 else 40
        ctx = torch.randint(3, hi, (B, S), generator=g)
        tgt = torch.randint(3, hi, (B, T), generator=g)
        cm = torch.zeros(B, T, dtype=torch.long)
        cm[:, 0] = 1
        cm[0, 1:3] = 2 if T > 2 else 1
        cm[:, -1] = -1 if T > 2 else 1
        if S:
            tgt[:, 0] = ctx[:, 0]
        if T >= 100:
            cm = torch.randint(-1, 4, (B, T), generator=g)
            tgt[:, ::3] = ctx[:, :tgt[:, ::3].shape[1]]
        if kind in ('rich', 'gap', 'oov', 'negative'):
            w[:, :, 5] = 0.0
            ctx[:, 7] = ctx[:, 3]
            ctx[:, 5] = 32                                          # id 32 of vocab 33: only ever weight 0
            tgt[0, 2] = 32                                          # a target whose p_t is 0
            tgt[1, 4] = 31                                          # a target absent from the context
            cm = torch.zeros(B, T, dtype=torch.long)
            cm[0, 1:4], cm[0, 6], cm[1, 4], cm[2, 0:2], cm[2, 5], cm[1, 7], cm[2, 8] = 1, 2, 1, 2, 3, 4, 5
            cm[:, -1] = -1                                          # (row 3 has no entity)
            if kind == 'gap':
                cm[cm == 2] = 0
            if kind == 'oov':
                ctx[3, 9] = 33
            if kind == 'negative':
                ctx[3, 9] = -4
        if kind == 'stride':
            ctx[:, [0, 255, 256]] = 50
            tgt[:, 1] = 50
            cm[:, 1] = 1
        if kind == 'equal':
            ctx[:] = 7
            tgt[:, 0] = 7
        if kind == 'distinct':
            ctx = torch.stack([torch.randperm(S, generator=g) + 3 for _ in range(B)])
            tgt[:, 0] = ctx[:, 300]
        if S:
            w = w / w.sum(-1, keepdim=True)
        return dict(w=_round(w, 'float32'), ctx=ctx.numpy(), tgt=tgt.numpy(), cm=cm.numpy(), tgt_pad=3, cm_pad=5)
    return cached(('loss', case['id']), make)


# entity head: id, (B,T,E), copy-mask pattern
ENT = [dict(id='E%d' % E, shape=(3, 7, E), cm='mixed') for E in (1, 63, 64, 65, 100, 1024)] + \
      [dict(id='all_ignored', shape=(3, 7, 64), cm='ignored')]
ENT_LOGITS = dict(id='logits_T1', shape=(5, 1, 100), cm='mixed')


def ent_inputs(case, dtype):
    def make():
        B, T, E = case['shape']
        g = _gen(300 + E)
        x = _round(_randn(g, T, B, E), dtype)
        w = _round(_randn(g, 2, E) * 0.3, 'float32')
        bias = _round(_randn(g, 2), 'float32')
        cm = (np.arange(B * T).reshape(B, T) % 5 - 1).astype(np.int64)          # -1, 0, 1, 2, 3
        if case['cm'] == 'ignored':
            cm[:] = -1
        return dict(x=x, w=w, bias=bias, cm=cm, dbias0=np.array([0.75, -1.5]))
    return cached(('ent', case['id'], dtype), make)


# causal attention, D = 64: training shapes (B,H,T) and step forms (Tq, pos0, S)
CAUSAL = [dict(id='T1', shape=(1, 1, 1)), dict(id='T2', shape=(2, 3, 2)), dict(id='T12', shape=(2, 3, 12)),
          dict(id='T65', shape=(1, 2, 65)), dict(id='ascending', shape=(1, 2, 12), order=1),
          dict(id='descending', shape=(1, 2, 12), order=-1)]
CAUSAL_STEP = [dict(id='step_%d_%d_%d' % f, form=f) for f in ((1, 0, 1), (1, 1, 2), (1, 39, 40), (3, 5, 8), (3, 5, 6))]
C_SCALE = 0.125


def causal_inputs(case, dtype):
    """q, k, v, dout [T,B,E]; order +-1: dots ascending / descending in s with |scale q.k| up to about 60"""
    def make():
        if 'form' in case:
            Tq, pos0, S = case['form']
            B, H, Tk = 2, 2, S
        else:
            B, H, Tq = case['shape']
            Tk = Tq
        E = H * 64
        g = _gen(500 + Tq + Tk)
        q, k, v, do = (_randn(g, n, B, E) * 0.5 for n in (Tq, Tk, Tk, Tq))
        if case.get('order'):
            import torch
            u = _randn(g, 1, B, E)
            ramp = torch.linspace(-1, 1, Tk).view(Tk, 1, 1) * case['order']
            q = u * 7.5 + q * 0.05
            k = u * ramp + k * 0.02
        return dict(q=_round(q, dtype), k=_round(k, dtype), v=_round(v, dtype), dout=_round(do, dtype))
    return cached(('causal', case['id'], dtype), make)


# copy step: id, (Ba,B,H,S,D), what is special
STEP = [dict(id='S0', shape=(3, 4, 2, 0, 64)), dict(id='S1', shape=(3, 4, 2, 1, 64)), dict(id='S20', shape=(3, 4, 3, 20, 64)),
        dict(id='S257', shape=(3, 4, 2, 257, 64)), dict(id='S512', shape=(3, 4, 2, 512, 64)),
        dict(id='D16', shape=(3, 4, 3, 40, 16)), dict(id='tie', shape=(3, 4, 2, 20, 64), tie=True),
        dict(id='entity_tie', shape=(3, 4, 2, 20, 64), ent_tie=True), dict(id='in_hist', shape=(3, 4, 2, 20, 64), in_hist=True),
        dict(id='last_hist', shape=(3, 4, 2, 20, 64), last_hist=True)]
HIST_LEN = 4
STEP_ROWS = (2, 0, 3)


def step_inputs(case, dtype):
    def make():
        import torch
        Ba, B, H, S, D = case['shape']
        E = H * D
        g = _gen(900 + S + D + case.get('seed', 0))
        q, k, bk = _randn(g, Ba, E) * 0.6, _randn(g, S, B, E) * 0.6, _randn(g, E) * 0.3
        m, pr = _masks(B, S, 'tail' if S > 2 else 'none', 'none' if S < 2 else 'mixed')
        if pr is not None:
            pr[:, ::2] = 1
        ctx = torch.randint(3, 40, (B, S), generator=g).numpy()
        rows = np.array(STEP_ROWS, np.int32)
        if case.get('tie'):
            # ids all distinct; positions 2 and 9 of every row: byte-identical key rows aligned with the row's query, same
            # mask and proper -> two equal largest sums; the LOWER id sits at the LATER position
            ctx = np.stack([np.arange(S) * 3 + 5 for _ in range(B)])
            ctx[:, 2], ctx[:, 9] = 90, 80
            for i, b in enumerate(STEP_ROWS):
                k[2, b] = q[i] * 0.5
            k = torch.from_numpy(_round(k, dtype)).float()
            k[9] = k[2]
            if m is not None:
                m[:, [2, 9]] = 0
            pr[:, [2, 9]] = 1
        ent = np.array([[0.0, 1.0], [-1.0, 2.0], [0.5, 1.5]], np.float32)
        if case.get('ent_tie'):
            ent[1] = [1.0, 1.0]
        hist = np.full((B, HIST_LEN), -1, np.int64)
        hist[:, 0] = 1000 + np.arange(B)
        n_hist = HIST_LEN - 1 if case.get('last_hist') else 1
        x = dict(q=_round(q, dtype), k=_round(k, dtype), bias_k=_round(bk, dtype), mask=m, proper=pr, ctx=ctx, rows=rows,
                 ent=ent, gen=np.array([11, 12, 13], np.int64), hist=hist, n_hist=n_hist, H=H)
        if case.get('in_hist'):
            first = copy_step(**x)
            hist[rows[0], 0] = first['best_id'][0]
        return x
    return cached(('step', case['id'], dtype), make)


def step_bound(r, dtype_unused=None, c=None):
    """bound of prob per alive row (prob is stored fp32)"""
    return np.array([bound('prob', r['prob'][i], r['S_prob'][i], 'float32', r['gam'][i], c) for i in range(len(r['prob']))])
