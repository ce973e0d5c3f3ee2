"""References for the BertAdam step kernels of csrc/optim.hip, numpy only:
  * step():     ONE step of the header comment of optim.hip in float64 from given fp32 state, with everything the entry
                point tell_bertadam_step2 takes (grad_scale, per-tensor clip, skip, wire gradient, keep_grad, schedule);
  * emulate():  the kernels' own fp32 arithmetic - same association, the wave / block sum order of sqsum_chunks_kernel<4>
                and tensor_norms_kernel, multiply-adds fused or not;
  * *_ratio():  the bounds, each returning its largest ratio so that the constants C can be read off;
  * the case tables shared by tests/test_optim_ref_host.py and tests/test_gpu_optim.py.
All comparisons are one step deep: a multi-step case restarts step() from the state the device (or the emulation) left."""
import numpy as np

CHUNK = 1024
U24 = 2.0 ** -24
TINY = 2.0 ** -125            # absolute slack: an fp32 intermediate (g'^2, a product with it) in the subnormal range
F32_LIMIT = float(np.float32(3.4e38))       # tensor_norms_kernel: a sum of squares above this (or NaN) flags the step
NORM_EPS = float(np.float32(1e-6))
DECOY = 77.0                  # what the fp32 gradient buffer holds when the step reads the bf16 wire gradient
# pinned = 4 x the largest ratio measured on the MI355X over tests/test_gpu_optim.py, rounded up to a power of two
# (DESIGN.md section 30 has the measured values and the cases)
C = dict(n=8.0, m=8.0, v=16.0, p=4.0, lr=2.0)

MUTANTS = ('global_norm', 'norm_unscaled', 'neighbour_norm', 'v_unclipped', 'sqrt_inside', 'bias_correction', 'wd_after',
           'schedule_next', 'wire_swapped', 'shadow_trunc', 'tail_chunk_dropped', 'skip_advances', 'skip_ignores_keep')


# ---------------------------------------------------------------- layout, bf16
class Layout:
    """tensors of the given sizes, each starting on a chunk boundary (training/optimizers.py FlatParams)"""

    def __init__(self, sizes):
        self.sizes = [int(n) for n in sizes]
        chunks = [(n + CHUNK - 1) // CHUNK for n in self.sizes]
        self.chunk_begin = np.concatenate([[0], np.cumsum(chunks)]).astype(np.int64)
        self.n_tensors, self.n_chunks = len(self.sizes), int(self.chunk_begin[-1])
        self.total = self.n_chunks * CHUNK
        self.chunk_tensor = np.repeat(np.arange(self.n_tensors), chunks).astype(np.int32)
        self.offsets = (self.chunk_begin[:-1] * CHUNK).astype(np.int64)
        self.real = np.zeros(self.total, dtype=bool)
        for o, n in zip(self.offsets, self.sizes):
            self.real[o:o + n] = True

    def tensor_of_elem(self):
        return np.repeat(self.chunk_tensor, CHUNK)

    def scatter(self, parts, dtype=np.float32):
        out = np.zeros(self.total, dtype=dtype)
        for o, n, a in zip(self.offsets, self.sizes, parts):
            out[o:o + n] = a
        return out


def bf16_rne(x):
    """fp32 -> bf16 bits, round to nearest even (NaN-free input)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_trunc(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_widen(h):
    return (np.ascontiguousarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def schedule(step, lr_base, warmup, t_total):
    """lr_schedule_kernel in float64 from the fp32 arguments: lr_base * warmup_linear(step / t_total, warmup)"""
    lr_base, warmup, t_total = float(np.float32(lr_base)), float(np.float32(warmup)), float(np.float32(t_total))
    f = 1.0
    if t_total > 0:
        x = step / t_total
        f = x / warmup if x < warmup else max((x - 1.0) / (warmup - 1.0), 0.0)
    return lr_base * f


def _hp64(hp):
    return tuple(np.float64(np.float32(hp[k])) for k in ('b1', 'b2', 'eps', 'wd'))


def _grad_after(g, lay, zero_grad, keep_grad, ignore_keep=False):
    out = np.array(g, dtype=np.float32)
    if zero_grad:
        zero = np.ones(lay.n_tensors, dtype=bool)
        if keep_grad is not None and not ignore_keep:
            zero = np.asarray(keep_grad) == 0
        out[zero[lay.tensor_of_elem()]] = 0.0
    return out


# ---------------------------------------------------------------- the float64 reference
def step(p, g, m, v, lay, hp, grad_scale=1.0, max_norm=0.0, zero_grad=0, keep_grad=None, skip=None, wire=None,
         step=None, lr=None, lr_base=0.0, warmup=-1.0, t_total=-1.0, p_dev=None, mutant=None, c=None):
    """-> dict(p, m, v float64; shadow uint16 (None: not written); grad fp32; norms float64 (None: not computed); lr;
    step; skip (s0, s1) or None; applied; aux for the bounds).  step None: the caller's `lr` is used.  p_dev: the
    device's fp32 master after the step - the shadow is its bf16 rounding, so the shadow check is bit-exact."""
    c = C if c is None else c
    f64 = np.float64
    b1, b2, eps, wd = _hp64(hp)
    gs, mn = f64(np.float32(grad_scale)), f64(np.float32(max_norm))
    p, m, v = (np.asarray(a, dtype=f64) for a in (p, m, v))
    src = (bf16_widen(wire) if wire is not None else np.asarray(g, dtype=np.float32)).astype(f64)
    if mutant == 'wire_swapped' and wire is not None:
        src = src.reshape(-1, 2)[:, ::-1].reshape(-1)
    s0, s1 = (0, 0) if skip is None else (int(skip[0]), int(skip[1]))
    if step is not None:
        lr = schedule(step + 1 if mutant == 'schedule_next' else step, lr_base, warmup, t_total)
    else:
        lr = float(np.float32(lr))
    tel = lay.tensor_of_elem()
    norms = None
    if mn > 0:
        gn = src if mutant == 'norm_unscaled' else src * gs
        with np.errstate(over='ignore', invalid='ignore'):
            sq = np.add.reduceat(gn * gn, lay.offsets)
        if mutant == 'global_norm':
            sq = np.full_like(sq, sq.sum())
        norms = np.sqrt(sq)
        if skip is not None and not bool((sq <= F32_LIMIT).all()):
            s0 |= 2
    out = dict(norms=norms, lr=lr, aux=None)
    if skip is not None and s0 != 0:          # skipped: p, m, v, shadow untouched; the gradient is still cleared
        out.update(p=p, m=m, v=v, shadow=None, applied=False, skip=(s0, s1 + 1),
                   grad=_grad_after(g, lay, zero_grad, keep_grad, mutant == 'skip_ignores_keep'),
                   step=None if step is None else step + (1 if mutant == 'skip_advances' else 0))
        return out
    coef = np.full(lay.n_tensors, gs)
    near = np.zeros(lay.n_tensors, dtype=bool)
    if mn > 0:
        with np.errstate(invalid='ignore'):
            cc = mn / (norms + NORM_EPS)
            coef = np.where(cc < 1, gs * cc, gs)
            near = cc < 1 + 4 * c['n'] * U24            # clipped, or so close that the device may decide the other way
    ce = coef[tel]
    if mutant == 'neighbour_norm' and lay.n_tensors > 1:
        for t in range(lay.n_tensors):
            o = int(lay.offsets[t])
            ce[o:o + CHUNK] = coef[t - 1 if t > 0 else 1]
    gp = src * ce
    m2 = b1 * m + (1 - b1) * gp
    gv = src * gs if mutant == 'v_unclipped' else gp
    v2 = b2 * v + (1 - b2) * gv * gv
    sv = np.sqrt(v2)
    den = np.sqrt(v2 + eps) if mutant == 'sqrt_inside' else sv + eps
    with np.errstate(invalid='ignore'):         # (a NaN / Inf gradient that nothing inspected: max_norm <= 0)
        u = m2 / den
    if mutant == 'bias_correction':
        t = (step or 0) + 1
        u = (m2 / (1 - b1 ** t)) / (np.sqrt(v2 / (1 - b2 ** t)) + eps)
    if mutant == 'wd_after':
        p2 = p - lr * u
        p2 = p2 - lr * wd * p2
    else:
        p2 = p - lr * (u + wd * p)
    master = np.asarray(p_dev, dtype=np.float32) if p_dev is not None else p2.astype(np.float32)
    out.update(p=p2, m=m2, v=v2, shadow=bf16_trunc(master) if mutant == 'shadow_trunc' else bf16_rne(master),
               grad=_grad_after(g, lay, zero_grad, keep_grad), applied=True,
               step=None if step is None else step + 1, skip=None if skip is None else (s0, s1),
               aux=dict(b1m=np.abs(b1 * m), gterm=np.abs((1 - b1) * gp), b2v=b2 * v, gv2=(1 - b2) * gp * gp,
                        near=near[tel], sv=sv, eps=eps, u=u, p0=np.abs(p), wd=wd, lr=abs(lr)))
    return out


# ---------------------------------------------------------------- bounds
def _ratio(err, scale, slack):
    """largest (err - slack)+ / scale; where the scale is 0 the error has to be inside the slack"""
    ex = np.maximum(np.asarray(err, dtype=np.float64) - slack, 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(ex > 0, ex / scale, 0.0)
    r = np.where(np.isnan(np.asarray(err, dtype=np.float64)), np.inf, r)
    return float(r.max()) if r.size else 0.0


def norms_ratio(got, ref):
    """|got - ref| <= c_n 2^-24 ref; an exactly zero gradient gives exactly 0"""
    return _ratio(np.abs(np.asarray(got, dtype=np.float64) - ref['norms']), U24 * ref['norms'], 0.0)


def _m_parts(ref, c):
    a = ref['aux']
    return U24 * (a['b1m'] + a['gterm']), a['near'] * a['gterm'] * (c['n'] * U24) + TINY


def _v_parts(ref, c):
    a = ref['aux']
    return U24 * (a['b2v'] + a['gv2']), a['near'] * a['gv2'] * (2.001 * c['n'] * U24) + TINY


def m_ratio(got, ref, c=None):
    scale, slack = _m_parts(ref, C if c is None else c)
    return _ratio(np.abs(np.asarray(got, dtype=np.float64) - ref['m']), scale, slack)


def v_ratio(got, ref, c=None):
    scale, slack = _v_parts(ref, C if c is None else c)
    return _ratio(np.abs(np.asarray(got, dtype=np.float64) - ref['v']), scale, slack)


def u_bound(ref, c=None):
    """bound on u = m / (sqrt(v) + eps) from the bounds on m and v: |m'/d' - m/d| <= dm / d' + |m| |d - d'| / (d d'),
    d' >= sqrt(max(v - dv, 0)) + eps, |sqrt(v +- dv) - sqrt(v)| <= sqrt(v) - sqrt(max(v - dv, 0)) (concavity)"""
    c = C if c is None else c
    a = ref['aux']
    ms, ml = _m_parts(ref, c)
    vs, vl = _v_parts(ref, c)
    dm, dv = c['m'] * ms + ml, c['v'] * vs + vl
    lo = np.sqrt(np.maximum(ref['v'] - dv, 0.0))
    d, dlo = a['sv'] + a['eps'], lo + a['eps']
    return dm / dlo + np.abs(ref['m']) * (a['sv'] - lo) / (d * dlo)


def p_ratio(got, ref, c=None):
    """|got - ref| <= c_p 2^-24 (|p| + lr (|u| + wd |p|)) + lr (bound on u)"""
    a = ref['aux']
    scale = U24 * (a['p0'] + a['lr'] * (np.abs(a['u']) + a['wd'] * a['p0']))
    return _ratio(np.abs(np.asarray(got, dtype=np.float64) - ref['p']), scale, a['lr'] * u_bound(ref, c) + TINY)


def lr_ratio(got, ref_lr, lr_base):
    """|got - ref| <= c_lr 2^-24 lr_base, and exactly 0 where the float64 schedule is 0"""
    err = abs(float(got) - ref_lr)
    if ref_lr == 0.0:
        return 0.0 if err == 0.0 else float('inf')
    return err / (U24 * abs(float(np.float32(lr_base))))


def ratios(got, ref, c=None):
    """{kind: largest ratio} of one applied step (got: dict of p, m, v and, where computed, norms)"""
    out = dict(m=m_ratio(got['m'], ref, c), v=v_ratio(got['v'], ref, c), p=p_ratio(got['p'], ref, c))
    if ref['norms'] is not None:
        out['n'] = norms_ratio(got['norms'], ref)
    return out


def inside(r, c=None):
    c = C if c is None else c
    return all(r[k] <= c[k] for k in r)


# ---------------------------------------------------------------- the kernels' arithmetic in fp32
def _fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)) \
        .astype(np.float32)


_LANE = np.arange(64)


def _wave_sum(s):
    """common.h wave_sum: xor butterfly over the last axis (64 lanes)"""
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., _LANE ^ o]
    return s[..., 0]


def emu_partials(src, gs, fused=False):
    """sqsum_chunks_kernel<4>: per chunk, thread t squares the float4 at 4 t, wave sums, four waves folded left to right"""
    x = np.asarray(src, dtype=np.float32).reshape(-1, 256, 4)
    gs = np.float32(gs)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        if fused:
            s = _fma(x[..., 3], x[..., 3], _fma(x[..., 2], x[..., 2], _fma(x[..., 1], x[..., 1], x[..., 0] * x[..., 0])))
        else:
            s = ((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2]) + x[..., 3] * x[..., 3]
        s = (s * gs) * gs
        r = _wave_sum(s.reshape(-1, 4, 64))
        return ((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]


def emu_norms(partial, chunk_begin):
    """tensor_norms_kernel: 256 threads, the four-way unrolled trips while c + 768 < c1, then the single-stride tail"""
    partial = np.asarray(partial, dtype=np.float32)
    sums = np.zeros(len(chunk_begin) - 1, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for t in range(len(sums)):
            c0, c1 = int(chunk_begin[t]), int(chunk_begin[t + 1])
            s = np.zeros((4, 256), dtype=np.float32)
            cur = c0 + np.arange(256)
            while True:
                act = cur + 768 < c1
                if not act.any():
                    break
                for j in range(4):
                    s[j, act] += partial[cur[act] + 256 * j]
                cur = np.where(act, cur + 1024, cur)
            while True:
                act = cur < c1
                if not act.any():
                    break
                s[0, act] += partial[cur[act]]
                cur = np.where(act, cur + 256, cur)
            r = _wave_sum(((s[0] + s[1]) + (s[2] + s[3])).reshape(4, 64))
            sums[t] = (r[0] + r[1]) + (r[2] + r[3])
        return np.sqrt(sums), sums


def emulate(p, g, m, v, lay, hp, grad_scale=1.0, max_norm=0.0, zero_grad=0, keep_grad=None, skip=None, wire=None,
            step=None, lr=None, lr_base=0.0, warmup=-1.0, t_total=-1.0, fused=False, U=4, mutant=None):
    """what the three kernels compute, in numpy float32 -> the dict of step() with fp32 p, m, v, norms, lr"""
    f32 = np.float32
    b1, b2, eps, wd = (f32(hp[k]) for k in ('b1', 'b2', 'eps', 'wd'))
    gs, mn, one = f32(grad_scale), f32(max_norm), f32(1)
    p, m, v = (np.asarray(a, dtype=f32) for a in (p, m, v))
    src = bf16_widen(wire) if wire is not None else np.asarray(g, dtype=f32)
    s0, s1 = (0, 0) if skip is None else (int(skip[0]), int(skip[1]))
    lr = f32(schedule(step, lr_base, warmup, t_total)) if step is not None else f32(lr)
    norms = None
    if mn > 0:
        norms, sums = emu_norms(emu_partials(src, gs, fused), lay.chunk_begin)
        if skip is not None and not bool((np.abs(sums) <= f32(3.4e38)).all()):
            s0 |= 2
    out = dict(norms=norms, lr=lr, aux=None)
    if skip is not None and s0 != 0:
        out.update(p=p, m=m, v=v, shadow=None, applied=False, skip=(s0, s1 + 1), step=step,
                   grad=_grad_after(g, lay, zero_grad, keep_grad))
        return out
    coef = np.full(lay.n_tensors, gs, dtype=f32)
    if mn > 0:
        with np.errstate(invalid='ignore', over='ignore'):
            cc = mn / (norms + f32(1e-6))
            coef = np.where(cc < one, gs * cc, gs).astype(f32)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        gg = src * coef[lay.tensor_of_elem()]
        if fused:         # the update kernel's multiply-adds as it spells them out (section 30: one arithmetic for all U)
            m2 = _fma(one - b1, gg, b1 * m)
            v2 = b2 * v + ((one - b2) * gg) * gg
            p2 = _fma(-lr, _fma(wd, p, m2 / (np.sqrt(v2) + eps)), p)
        else:
            m2 = b1 * m + (one - b1) * gg
            v2 = b2 * v + ((one - b2) * gg) * gg
            p2 = p - lr * (m2 / (np.sqrt(v2) + eps) + wd * p)
    if mutant == 'tail_chunk_dropped' and U > 1:          # the last chunk of every group of U never stored
        keep = np.repeat(np.arange(lay.n_chunks) % U == U - 1, CHUNK)
        p2, m2, v2 = np.where(keep, p, p2), np.where(keep, m, m2), np.where(keep, v, v2)
    assert p2.dtype == f32 and m2.dtype == f32 and v2.dtype == f32
    out.update(p=p2, m=m2, v=v2, shadow=bf16_rne(p2), grad=_grad_after(g, lay, zero_grad, keep_grad), applied=True,
               step=None if step is None else step + 1, skip=None if skip is None else (s0, s1))
    return out


# ---------------------------------------------------------------- the random lane's case table
HP = dict(b1=0.9, b2=0.98, eps=1e-6, wd=1e-2)
SIZES = (300 * 70, 5, 1024, 33, 2049, 1025, 1)            # 21 + 1 + 1 + 1 + 3 + 2 + 1 = 30 chunks
# per-tensor gradient amplitudes: neighbours orders of magnitude apart, norms on both sides of max_norm 0.1 / 0.5, and
# tensor 5 (norm about 1.6) crosses 0.5 under grad_scale 1/8
AMP = (1.0, 1e-3, 30.0, 1e-2, 1.0, 0.05, 0.03)


def _case(id, **kw):
    c = dict(id=id, sizes=SIZES, seed=len(id), grad='normal', wd=1e-2, max_norm=0.5, grad_scale=1.0, wire=False,
             widened=False, zero_grad=1, keep=None, shadow=True, steps=1, step0=3, lr=1e-2, warmup=0.2, t_total=10.0,
             p='normal')
    c.update(kw)
    return c


CASES = [
    _case('normal-clip0.5'),
    _case('normal-clip0.1-wd0', max_norm=0.1, wd=0.0, keep='zero'),
    _case('heavy-clip0.5-keepmixed', grad='heavy', keep='mixed'),
    _case('heavy-noclip-nozero-noshadow', grad='heavy', max_norm=0.0, zero_grad=0, shadow=False),
    _case('gs8-clip0.5', grad_scale=0.125, keep='mixed'),
    _case('gs3-clip0.1-heavy', grad_scale=1.0 / 3.0, max_norm=0.1, grad='heavy', wd=0.0),
    _case('gs3-noclip', grad_scale=1.0 / 3.0, max_norm=0.0, zero_grad=0),
    _case('wire-clip0.5', wire=True, keep='mixed'),
    _case('wire-clip0.5-widened', wire=True, widened=True, keep='mixed', seed=len('wire-clip0.5')),
    _case('wire-gs8-heavy-clip0.1', wire=True, grad='heavy', grad_scale=0.125, max_norm=0.1, zero_grad=0, shadow=False),
    _case('lr0.1-wd0.1', lr=0.1, wd=0.1, step0=2),
    _case('ties-lr0', p='ties', step0=0),
    _case('three-steps', steps=3, step0=1, keep='mixed'),
    _case('three-steps-wire-gs3', steps=3, step0=0, wire=True, grad_scale=1.0 / 3.0, max_norm=0.1),
]
BY_ID = {c['id']: c for c in CASES}


def _grad(rng, lay, kind):
    parts = []
    for n, a in zip(lay.sizes, AMP):
        x = rng.standard_normal(n) if kind == 'normal' else rng.standard_t(1.5, n)
        parts.append(np.clip(a * x, -1e15, 1e15))
    return lay.scatter(parts)


def make_case(c):
    """-> dict(lay, hp, p, m, v fp32, grads (one per step; fp32, or bf16 bits when the case reads the wire), keep)"""
    rng = np.random.default_rng(1000 + c['seed'])
    lay = Layout(c['sizes'])
    hp = dict(HP, wd=c['wd'])
    if c['p'] == 'ties':            # bf16 rounding ties (both neighbours' parities), just off a tie, and the +-max range
        base = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23,
                         3.38e38, -3.38e38, 3.4e38, -3.4e38, 2.0 ** -126, 2.0 ** -130, 0.0, -1.0 - 2.0 ** -8])
        sign = np.where(np.arange(lay.total) % 3 == 0, -1.0, 1.0)
        p = np.where(lay.real, np.resize(base, lay.total) * sign, 0.0).astype(np.float32)
    else:
        p = lay.scatter([rng.standard_normal(n) for n in lay.sizes])
    m = lay.scatter([0.1 * a * rng.standard_normal(n) for n, a in zip(lay.sizes, AMP)])
    v = lay.scatter([(0.1 * a * rng.standard_normal(n)) ** 2 for n, a in zip(lay.sizes, AMP)])
    grads = []
    for _ in range(c['steps']):
        g = _grad(rng, lay, c['grad'])
        if c['wire']:
            g = bf16_rne(g)
        grads.append(g)
    keep = None
    if c['keep'] == 'zero':
        keep = np.zeros(lay.n_tensors, dtype=np.int32)
    elif c['keep'] == 'mixed':
        keep = (np.arange(lay.n_tensors) % 2).astype(np.int32) * 7          # any non-zero value counts
    return dict(lay=lay, hp=hp, p=p, m=m, v=v, grads=grads, keep=keep)


def step_args(c, d, i):
    """keyword arguments of step() / emulate() for step i of case c (state p, m, v is passed by the caller)"""
    kw = dict(grad_scale=c['grad_scale'], max_norm=c['max_norm'], zero_grad=c['zero_grad'], keep_grad=d['keep'],
              step=c['step0'] + i, lr_base=c['lr'], warmup=c['warmup'], t_total=c['t_total'])
    g = d['grads'][i]
    if c['wire'] and not c['widened']:          # the fp32 buffer holds a decoy: it must not be read, and its zeroing shows
        return dict(kw, wire=g), np.where(d['lay'].real, DECOY, 0.0).astype(np.float32)
    return kw, (bf16_widen(g) if c['wire'] else g)


# ---------------------------------------------------------------- the exact lane
# m = v = 0, b1 = 1/2, b2 = 3/4, every non-zero g' = +-2^5 after the clip, eps = 2^4: m = g'/2, v = g'^2/4,
# sqrt(v) + eps = 2^5, u = +-1/2; lr = 2^-3, wd = 2^-4, p small integers: every product and sum is a multiple of 2^-7 below
# 2^6 - exact in fp32 in any association, fused or not.  max_norm = 2^8; a tensor with 4^c non-zero gradients of 2^5 has
# the norm 2^(5+c): unclipped for c <= 3 (c = 3 sits ON the threshold: norm + 1e-6f rounds back to 256, the coefficient is
# exactly 1); a clipped tensor has 64 gradients of 2^(5+j), norm 2^(8+j) >= 512, coefficient 2^-j.  The float64 reference
# keeps the 1e-6: its g' is 2^5 (1 - d) with d <= 1e-6 / 256 = 3.9e-9, which is under a seventh of the 2^-25 that would
# move an fp32 rounding (twice that for v), so ROUNDED to fp32 it is the same number (test_optim_ref_host.py checks it).
EXACT_HP = dict(b1=0.5, b2=0.75, eps=16.0, wd=2.0 ** -4)
EXACT_LR, EXACT_MAX_NORM = 2.0 ** -3, 256.0
# (sizes, per tensor (log4 of the count of non-zero gradients or None for an all-zero gradient, clip exponent j))
EXACT_LAYOUTS = [
    ((1,), [(0, 0)]),                                             # 1 chunk
    ((1025,), [(3, 2)]),                                          # 2 chunks, clipped
    ((5, 1023, 1), [(1, 0), (3, 0), (None, 0)]),                  # 3 chunks; tensor 1 on the threshold
    ((2049, 1024), [(3, 1), (2, 0)]),                             # 4
    ((1, 1025, 5, 1024), [(0, 0), (3, 3), (0, 0), (3, 0)]),       # 5
    ((2049, 1, 1025, 1023), [(2, 0), (None, 0), (3, 1), (3, 2)]),             # 7
    ((1025, 1025, 1025, 1025), [(3, 1), (1, 0), (3, 3), (0, 0)]),             # 8
    ((2049, 2049, 1024, 1023, 5), [(3, 2), (3, 0), (2, 0), (3, 1), (1, 0)]),  # 9
    ((2049, 2049, 2049, 1025), [(3, 0), (3, 1), (None, 0), (3, 3)]),          # 11
    ((2049, 2049, 2049, 2049, 5), [(3, 1), (0, 0), (3, 2), (3, 0), (1, 0)]),  # 13
]


def exact_case(k, zero_mv=True):
    sizes, spec = EXACT_LAYOUTS[k]
    lay = Layout(sizes)
    parts_p, parts_g = [], []
    for t, (n, (c4, j)) in enumerate(zip(sizes, spec)):
        i = np.arange(n)
        parts_p.append(((i * 7 + 3 * t) % 33 - 16).astype(np.float32))
        g = np.zeros(n, dtype=np.float32)
        if c4 is not None:
            count = 4 ** c4
            assert count <= n and (j == 0 or c4 == 3)
            pos = np.floor(np.linspace(0, n - 1, count)).astype(np.int64)        # spread over all chunks, both ends included
            assert len(np.unique(pos)) == count
            g[pos] = np.where((pos * 5 + t) % 3 == 0, -1.0, 1.0) * 2.0 ** (5 + j)
        parts_g.append(g)
    z = np.zeros(lay.total, dtype=np.float32)
    return dict(lay=lay, hp=EXACT_HP, p=lay.scatter(parts_p), g=lay.scatter(parts_g), m=z, v=z.copy(),
                norms=np.array([0.0 if c4 is None else 2.0 ** (5 + c4 + j) for c4, j in spec]))


def to_f32(ref):
    """the float64 reference rounded to fp32 - what the exact lane compares bit for bit"""
    return {k: ref[k].astype(np.float32) for k in ('p', 'm', 'v', 'norms') if ref[k] is not None}
