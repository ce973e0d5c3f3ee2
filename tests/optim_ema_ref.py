"""Reference for the exponential moving average that tell_bertadam_step_ema keeps (csrc/optim.hip),
numpy only, on top of tests/optim_ref.py:
  * decay_at():  d_t of the step that follows n applied updates, in float64 from the fp32 arguments;
  * omd_at():    what ema_schedule_kernel leaves in *ema_omd_dev, (float32)(1 - d_t);
  * fma32():     a * b + c rounded ONCE to fp32 (optim_ref._fma rounds the float64 sum a second time: TRAPS below);
  * ema_step():  e' = fma32(omd, fl32(p' - e), e) - the kernel's two roundings, so that the comparison is bit for bit;
  * run():       consecutive steps with skips and MUTANTS - deliberately wrong variants that a bit-for-bit comparison
                 against run() has to reject (tests/test_optim_ema_host.py shows it does, on SCHEDULE x DATA);
  * the small tables shared by tests/test_optim_ema_host.py and tests/test_gpu_optim_ema.py."""
import numpy as np

MUTANTS = ('ema_of_old_p', 'decay_swapped', 'n_off_by_one', 'skip_ticks', 'warmup_ignored', 'unfused')

# (decay, warm, n): n = None stands for step_dev = NULL.  n = 9 is the last step of the warm-up for decay 0.9 and warm 10
# ((1 + 9) / (10 + 9) = 0.53 < 0.9 still, the crossing (1 + n) / (10 + n) = 0.9 is at n = 80), 10^5 is far behind it
STEPS_N = (0, 1, 2, 9, 10, 11, 10 ** 5)
SCHEDULE = [(0.9, 10.0, n) for n in STEPS_N] + [(0.9999, 10.0, n) for n in STEPS_N] + \
    [(0.9, 0.0, n) for n in STEPS_N] + [(0.9, 10.0, None), (0.9999, 0.0, None), (0.0, 10.0, 3), (0.5, 1.0, 0), (0.75, 0.5, 2)]


def decay_at(n, decay, warm):
    """d_t after n applied updates (n None: no device counter).  float64 from the fp32 arguments."""
    decay, warm = float(np.float32(decay)), float(np.float32(warm))
    if n is None or warm <= 0.0:
        return decay
    return min(decay, (1.0 + n) / (warm + n))


def omd_at(n, decay, warm):
    return np.float32(1.0 - decay_at(n, decay, warm))


def fma32(a, b, c):
    """a * b + c with ONE rounding to fp32, for fp32 operands.  The float64 product of two fp32 numbers is exact (48
    bits); the float64 sum is not, and rounding it to fp32 afterwards can round twice.  TwoSum gives the sum's error
    exactly; where there is one the sum is moved to its ODD float64 neighbour on the error's side (round to odd), after
    which the rounding to fp32 - 29 bits shorter - is the rounding of the exact value."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(over='ignore', invalid='ignore'):
        prod = a * b
        s = prod + c
        t = s - prod
        err = (prod - (s - t)) + (c - t)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0.0) & ((np.atleast_1d(s).view(np.int64).reshape(s.shape) & 1) == 0)
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def ema_step(e, p_new, omd):
    """the kernel's arithmetic: the fp32 difference, then one fused multiply-add"""
    e, p_new = np.asarray(e, dtype=np.float32), np.asarray(p_new, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        d = p_new - e
    assert d.dtype == np.float32
    return fma32(np.float32(omd), d, e)


def run(e, steps, n, decay, warm, mutant=None):
    """steps: [(p_old, p_new, skipped)] - the masters before and after each launch.  -> ([e after each step], n after
    the last).  A skipped step leaves e and n alone."""
    out = []
    e = np.asarray(e, dtype=np.float32)
    for p_old, p_new, skipped in steps:
        if skipped:
            if mutant == 'skip_ticks' and n is not None:
                n += 1
            out.append(e)
            continue
        k = n
        if mutant == 'n_off_by_one' and n is not None:
            k = n + 1
        d = decay_at(k, decay, 0.0 if mutant == 'warmup_ignored' else warm)
        omd = np.float32(d) if mutant == 'decay_swapped' else np.float32(1.0 - d)
        src = np.asarray(p_old if mutant == 'ema_of_old_p' else p_new, dtype=np.float32)
        if mutant == 'unfused':                                     # d e + (1 - d) p', every operation rounded
            e = np.float32(1.0 - float(omd)) * e + omd * src
            assert e.dtype == np.float32
        else:
            e = ema_step(e, src, omd)
        out.append(e)
        if n is not None:
            n += 1
    return out, n


# Inputs that sit on the double-rounding trap: (e, p', omd, e' as it must be, e' as float64-then-fp32 rounding gives it).
# 2^32 + 1 = 641 x 6700417 and 2^32 - 1 = 65535 x 65537 are products of two numbers an fp32 holds, 2^-32 away (relatively)
# from a power of two: omd (p' - e) = 2^-24 (1 +- 2^-32) is a hair off HALF an ulp of e, and that hair is under half a
# float64 ulp of the sum - the float64 sum lands exactly on the fp32 tie and the second rounding goes to even.
_U = 2.0 ** -23
TRAPS = [
    # just above the tie, even neighbour below: must go up; the double rounding stays at 1
    (1.0, 6700418.0, 641.0 * 2.0 ** -56, 1.0 + _U, 1.0),
    # just below the tie, even neighbour above: must stay; the double rounding goes up to 1 + 2 ulp
    (1.0 + _U, 65538.0, 65535.0 * 2.0 ** -56, 1.0 + _U, 1.0 + 2 * _U),
    # the mirror images with negative e
    (-1.0, -6700418.0, 641.0 * 2.0 ** -56, -1.0 - _U, -1.0),
    (-1.0 - _U, -65538.0, 65535.0 * 2.0 ** -56, -1.0 - _U, -1.0 - 2 * _U),
]


def make_e(p, real, seed):
    """an average near the masters (it differs from them by a few updates' worth), +0 in the padding"""
    rng = np.random.default_rng(5000 + seed)
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        e = (p.astype(np.float64) * (1.0 + 0.01 * rng.standard_normal(p.shape)) + 1e-3 * rng.standard_normal(p.shape))
        e = np.clip(e, -3.0e38, 3.0e38).astype(np.float32)
    return np.where(real, e, np.float32(0.0)).astype(np.float32)


def exact_e(lay):
    """the exact lane's average (optim_ref.exact_case): small integers, +0 in the padding"""
    i = np.arange(lay.total)
    return np.where(lay.real, (i * 5) % 23 - 11, 0).astype(np.float32)
