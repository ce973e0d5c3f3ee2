"""numpy restatement of the device dropout RNG (csrc/common.h: tell_quad_* / tell_keep_field: one hash per aligned
index quad, four 16-bit fields) so that tests can rebuild the exact keep-masks a kernel used."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_U = np.uint64


def keep_field(seed, salt, idx):
    """The 16-bit field element idx is judged by (tell_keep_field)."""
    idx = np.asarray(idx, dtype=np.uint64)
    quad = idx >> _U(2)
    lo = quad & M32
    hi = quad >> _U(32)
    x = (lo * _U(0x9E3779B1) + _U(seed) * _U(0x85EBCA6B)) & M32
    y = (hi * _U(0x85EBCA77) + _U(salt) * _U(0xC2B2AE3D) + _U(0x27D4EB2F)) & M32
    h = x ^ y                                                # tell_quad_mix
    h = h ^ (h >> _U(16))
    h = (h * _U(0x7FEB352D)) & M32
    h = h ^ (h >> _U(15))
    a = ((h & _U(0xFFFFFF)) * _U(0xD1B54B)) & M32            # tell_quad_a: elements 0, 1
    a = a ^ (a >> _U(15))
    b = ((h >> _U(8)) * _U(0xA54FF5)) & M32                  # tell_quad_b: elements 2, 3
    b = b ^ (b >> _U(15))
    w = np.where((idx & _U(2)) == 0, a, b)
    return np.where((idx & _U(1)) == 1, w >> _U(16), w & _U(0xFFFF))


def threshold(p):
    """16-bit drop threshold (0 = no dropout)."""
    return np.uint64(min(max(int(float(np.float32(p)) * 65536.0), 0), 65535))


def keep_mask(seed, salt, n_or_idx, p):
    """float32 array of 0/1 keep flags for element indices 0..n-1 (or the given indices)."""
    idx = np.arange(n_or_idx, dtype=np.uint64) if np.isscalar(n_or_idx) else np.asarray(n_or_idx, dtype=np.uint64)
    return (keep_field(seed, salt, idx) >= threshold(p)).astype(np.float32)


def _mix(x, y):
    """tell_quad_mix on uint64 arrays holding 32-bit words."""
    h = x ^ y
    h = h ^ (h >> _U(16))
    h = (h * _U(0x7FEB352D)) & M32
    return h ^ (h >> _U(15))


def sample_uniform(seed, row, step):
    """u in [0, 1) of one top-k draw (csrc/common.h tell_sample_u): two rounds of the quad mix over (seed, row) and the
    step, 24 bits as a float32.  Broadcasts over array arguments."""
    seed, row, step = (np.asarray(v, dtype=np.uint64) & M32 for v in (seed, row, step))
    x = (((row * _U(0x9E3779B1)) & M32) + ((seed * _U(0x85EBCA6B)) & M32)) & M32     # tell_quad_x(seed, row)
    y = (((step * _U(0xC2B2AE3D)) & M32) + _U(0x27D4EB2F)) & M32               # tell_quad_y(step, row): row < 2^32
    h = _mix(_mix(x, y), _U(0x27D4EB2F))
    return ((h >> _U(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def sample_pick(sorted_lps, inv_temp, u):
    """The pick of tell_sample_pick over candidates sorted best first, in fp32 with the kernel's order of additions:
    w_j = exp((lp_j - lp_0) * inv_temp), c_j = w_0 + ... + w_j, the smallest j with u * c_{k-1} < c_j (k - 1 if none)."""
    lp = np.asarray(sorted_lps, dtype=np.float32)
    it = np.float32(inv_temp)
    w = np.exp((lp - lp[0]) * it).astype(np.float32)
    c = np.add.accumulate(w, dtype=np.float32)                        # sequential, like the kernel's loop
    t = np.float32(u) * c[-1]
    hit = np.nonzero(t < c)[0]
    return int(hit[0]) if hit.size else len(lp) - 1
