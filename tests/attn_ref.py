"""float64 reference of the attention kernels (csrc/attention.hip: tell_attn_fwd, tell_attn_bwd, tell_attn_avg_weights), their
fp32 emulation in the kernels' own tile order, the element-wise bounds, the case tables, the mutants and the path-naming
functions that tests/test_attn_ref_host.py and tests/test_gpu_attention.py walk.  numpy only; nothing
here comes from oracle/.  Inputs are rounded to their storage type BEFORE they reach a function.  Conventions and helpers are
those of tests/small_ref.py and tests/ln_ref.py; the bound of one element is

    u_out |ref|  +  derived bf16 terms  +  c gamma 2^-24 S  +  2^-126 (1 + S) [+ 2^-126 e^8 sum_s |v_s| for out]

Definitions, taken from the kernels.  The S real keys are followed by the virtual ones, which no mask reaches: key S is bias_k
with value bias_v when given, the next key has score 0 and value 0 when has_zero is set; S_total counts all of them.  The keep
flag of probability (b, h, t, s) is tell_amd.rng.keep_mask(seed, salt, ((b H + h) Tq + t) S_total + s, p); kept probabilities
are scaled by 1 / (1 - p).  lse is the natural logarithm of the sum of the UNDROPPED exponentials.  A (b, h, t) without a live
key has out = +0.0 and lse = +inf and adds exact zeros to every gradient; the gradient of a masked real key is exactly +-0.
Those elements are compared for equality (exact_at) and the reference produces no NaN for them.

The backward reference is computed from what the forward launch stored (out, lse), as section 36 does with mean / rstd:
P = exp(s - lse), delta = <dout, out>, dS = P (keep dP / (1 - p) - delta), dV = Pd^T dO, dK = dS^T Q, dQ = dS K.

Per element, with w'_s = the undropped softmax weight, w_s = w'_s keep_s / (1 - p), a_s = sum_d |q_d k_sd| (the score's own
terms), x_s = |s_s - max| + |max| (what the exponential's argument is made of) and R_s = 1 + a_s + x_s + 8 (8: the lazy maximum of
the self kernel), first-order propagation gives

    group      gamma                         S
    *_out      D + S_total + 5 nkt + 48      sum_s |w_s v_s| (R_s + sum_j w'_j R_j)
               (D: the score's accumulation; S_total: the P V accumulation; per tile the rescale, its exponential and the row
                sum; 48: exp2 / log2e products, the lane fold, 1 / l, the KSPLIT combine of four waves)
    *_lse      the same                      1 + |lse| + |max| + 8 + sum_j w'_j R_j
    bwd_dv     D + 40 + QB + nkt             sum_t Pd_ts |do_td| Rp_ts [+ sum_qb |running partial|],  Rp = 1 + a + |s - lse|
    bwd_dk     the same                      sum_t M_ts |q_td| [+ sum_qb |running partial|]
    bwd_dq     the same                      sum_s M_ts |k_sd|
    bwd_dbias  the same                      the dK / dV sums of key S
               M_ts = |dS_ts| Rp_ts + P_ts (kf_ts b_ts + dabs_t + |kf dP| + |delta|), b_ts = sum_d |v_sd do_td|,
               dabs_t = sum_d |do_td o_td|
    avg_w      D + H + 8                     (1 / H) sum_h P_hts (1 + a_hts + |s_hts - lse_ht|)

The bf16 kernels round every probability to bf16 in front of the second product; those terms are derived, never part of c:
2^-8 sum_s w_s |v_s| for out (p~_s / l is w_s), 2^-8 sum_t Pd |do| for dV, 2^-8 sum_t |dS q| for dK and the bias-key row,
2^-8 sum_s |dS k| for dQ, and for bf16 dK / dV at QB > 1 2^-8 times the sum, over the query blocks before the last, of the
absolute running partial that is stored and read back (the last store is u_out |ref|).

Measured on the MI355X: MEASURED and C below, and DESIGN.md section 38.
"""
import zlib

import numpy as np

from decode_ref import EPS, TINY, U_OUT, _pin
from small_ref import SENTINEL, _rng, cached, same_bits, store     # noqa: F401  (re-exported)
from decode_ref import bf16_round

F32, F64 = np.float32, np.float64
SEED = 20261
THR = 8.0                      # ATTN_SELF_THR
NW = 4                         # waves of a forward workgroup

# largest observed (|got - ref| - u_out |ref| - derived terms) / (gamma 2^-24 S) over the grid of tests/test_gpu_attention.py on
# the MI355X, and the pinned constant: four times that, rounded up to a power of two; 2^-10 where the error never left the
# first terms.  A group missing from MEASURED is not pinned: its GPU test then fails with the measured ratio in its message.
MEASURED = {'fwd_bf16_out': 0.000000, 'fwd_bf16_lse': 0.002015, 'fwd_f32_out': 0.003135, 'fwd_f32_lse': 0.007217,
            'fwd_bf16_d16_out': 0.000000, 'fwd_bf16_d16_lse': 0.000682, 'fwd_f32_d16_out': 0.001819,
            'fwd_f32_d16_lse': 0.001598, 'tile64_bf16_out': 0.000000, 'tile64_bf16_lse': 0.002002,
            'tile64_f32_out': 0.003794, 'tile64_f32_lse': 0.004878, 'reg_out': 0.000000, 'reg_lse': 0.001654,
            'self_out': 0.000000, 'self_lse': 0.002159, 'bwd_bf16_nw1_dq': 0.002508, 'bwd_bf16_nw1_dk': 0.000000,
            'bwd_bf16_nw1_dv': 0.000000, 'bwd_bf16_nw1_dbias': 0.002508, 'bwd_bf16_nw2_dq': 0.001853,
            'bwd_bf16_nw2_dk': 0.000322, 'bwd_bf16_nw2_dv': 0.000000, 'bwd_bf16_nw2_dbias': 0.000000,
            'bwd_bf16_nw4_dq': 0.000000, 'bwd_bf16_nw4_dk': 0.000000, 'bwd_bf16_nw4_dv': 0.000000,
            'bwd_bf16_nw4_dbias': 0.000000, 'bwd_bf16_d16_dq': 0.000000, 'bwd_bf16_d16_dk': 0.000000,
            'bwd_bf16_d16_dv': 0.000000, 'bwd_bf16_d16_dbias': 0.000000, 'bwd_f32_dq': 0.011807, 'bwd_f32_dk': 0.011058,
            'bwd_f32_dv': 0.024826, 'bwd_f32_dbias': 0.011433, 'bwd_f32_d16_dq': 0.017300, 'bwd_f32_d16_dk': 0.014715,
            'bwd_f32_d16_dv': 0.019855, 'bwd_f32_d16_dbias': 0.010897, 'avg_w_bf16': 0.016957, 'avg_w_f32': 0.054668}
C = {k: _pin(v) for k, v in MEASURED.items()}
FWD_KERNELS = ('fwd_bf16', 'fwd_f32', 'fwd_bf16_d16', 'fwd_f32_d16', 'tile64_bf16', 'tile64_f32', 'reg', 'self')
BWD_SHAPES = ('bwd_bf16_nw1', 'bwd_bf16_nw2', 'bwd_bf16_nw4', 'bwd_bf16_d16', 'bwd_f32', 'bwd_f32_d16')
GROUPS = tuple('%s_%s' % (k, o) for k in FWD_KERNELS for o in ('out', 'lse')) + \
    tuple('%s_%s' % (k, o) for k in BWD_SHAPES for o in ('dq', 'dk', 'dv', 'dbias')) + ('avg_w_bf16', 'avg_w_f32')

KEY_MUTANTS = ('drop_last_key', 'tail_key_live', 'no_zero_key', 'bias_v_as_bias_k', 'bias_masked', 'mask_of_other_sample',
               'head_swap', 'drop_second_tile64', 'drop_odd_tile', 'ksplit_wave3_lost')
MAX_MUTANTS = ('no_rescale', 'lazy_max_never_moves')
DROP_MUTANTS = ('keep_pair_swapped', 'keep_quad_rotated', 'keep_index_without_head', 'dropout_scales_lse')
LSE_MUTANTS = ('lse_base2',)
BWD_MUTANTS = ('bwd_delta_without_keep', 'bwd_dk_last_qblock_only', 'bwd_second_wave_lost', 'dbias_not_summed_over_t',
               'dv_from_undropped_p')
W_MUTANTS = ('avg_w_not_divided_by_H',)
MUTANTS = KEY_MUTANTS + MAX_MUTANTS + DROP_MUTANTS + LSE_MUTANTS + BWD_MUTANTS + W_MUTANTS
# wrong only through the kernel's tile order: they run in the tiled emulation (no_rescale in float64, the lazy maximum in
# fp32, where e^120 is not a number any more)
TILED_MUTANTS = {'no_rescale': F64, 'lazy_max_never_moves': F32}
# about the forward kernels' tiles: the backward of such a library is right
FWD_TILE_MUTANTS = ('tail_key_live', 'drop_second_tile64', 'drop_odd_tile', 'ksplit_wave3_lost')


class Out:
    """one output of a launch: value, S, gamma, storage dtype, group, the derived additive term `extra`, and exact_at: the
    elements that are compared for equality (zero_sign: either zero passes there)"""

    def __init__(self, value, S, gam, dtype, group, extra=0.0, exact_at=None, zero_sign=False):
        self.value, self.S, self.gam, self.dtype, self.group = value, S, gam, dtype, group
        self.extra, self.exact_at, self.zero_sign = extra, exact_at, zero_sign


def _parts(got, o):
    g, ref = np.asarray(got, F64), np.asarray(o.value, F64)
    S = np.broadcast_to(np.asarray(o.S, F64), ref.shape)
    extra = np.broadcast_to(np.asarray(o.extra, F64), ref.shape)
    ex = np.zeros(ref.shape, bool) if o.exact_at is None else np.broadcast_to(o.exact_at, ref.shape)
    return g, ref, S, extra, ex


def ratio(got, o):
    """largest (|got - ref| - u_out |ref| - derived terms) / (gamma 2^-24 S) over the bounded elements with S > 0"""
    g, ref, S, extra, ex = _parts(got, o)
    ok = np.isfinite(ref) & (o.gam * EPS * S > 0) & ~ex
    if not ok.any():
        return 0.0
    num = np.abs(g[ok] - ref[ok]) - U_OUT[o.dtype] * np.abs(ref[ok]) - extra[ok] - TINY * (1.0 + S[ok])
    num = np.where(np.isfinite(num), num, np.inf)
    return float((num / (o.gam * EPS * S[ok])).max())


def exact_failures(got, o):
    """elements of exact_at that are not the reference's value (bit for bit; either zero where zero_sign)"""
    if o.exact_at is None:
        return 0
    g32 = np.ascontiguousarray(got, F32)
    r32 = np.ascontiguousarray(np.broadcast_to(np.asarray(o.value, F32), g32.shape))
    ex = np.broadcast_to(o.exact_at, g32.shape)
    same = g32.view(np.uint32) == r32.view(np.uint32)
    if o.zero_sign:
        same |= (g32 == 0) & (r32 == 0)
    return int((ex & ~same).sum())


def failures(got, o, c=None):
    """number of elements of `got` (what a kernel, the emulation or a mutant stored) outside what `o` allows; every element is
    either bounded or compared for equality"""
    g, ref, S, extra, ex = _parts(got, o)
    assert g.shape == ref.shape
    c = C[o.group] if c is None else c
    with np.errstate(invalid='ignore'):
        b = U_OUT[o.dtype] * np.abs(ref) + extra + c * o.gam * EPS * S + TINY * (1.0 + S)
        bad = ~(np.abs(g - ref) <= b) & ~ex
    return int(bad.sum()) + exact_failures(got, o)


# ================================================================ dispatch, restated from the launchers
def sizes(case):
    St = case['S'] + int(case['bias']) + int(case['zero'])
    return St, -(-case['Tq'] // 32)


def walk(St, p, quads):
    """the dropout walk of a forward kernel: quads (reg / self) when S_total % 4 == 0, pairs when even, single elements"""
    if not p:
        return 'nodrop'
    return 'quad' if quads and St % 4 == 0 else ('pair' if St % 2 == 0 else 'single')


def fwd_kernel(case, options=None):
    """the kernel tell_attn_fwd launches: conditions on D, QB >= 4, dtype, the three options, has_bias, has_zero, S % 64"""
    o = dict(attn_tile64=0, attn_self=1, attn_dma=0, attn_occ=2)
    o.update(options or case.get('opts') or {})
    St, QB = sizes(case)
    bf = case['dtype'] == 'bfloat16'
    if case['D'] == 64 and QB >= 4:
        if bf and not o['attn_tile64'] and o['attn_self'] and not case['bias'] and not case['zero'] and case['S'] % 64 == 0:
            return 'self', o
        if bf and not o['attn_tile64']:
            return 'reg', o
        return ('tile64_bf16' if bf else 'tile64_f32'), o
    return ('fwd_bf16' if bf else 'fwd_f32') + ('' if case['D'] == 64 else '_d16'), o


def fwd_path(case, options=None):
    """names the branch taken: kernel, DROP, OCC, DMA, KSPLIT (and whether every wave has a key tile), the dropout walk"""
    kern, o = fwd_kernel(case, options)
    St, QB = sizes(case)
    if kern == 'self':
        return 'self:%s:%s' % ('dma' if o['attn_dma'] == 1 else 'regs', walk(St, case['p'], True))
    if kern == 'reg':
        return 'reg:occ%d:%s' % (3 if o['attn_occ'] == 3 else 2, walk(St, case['p'], True))
    if kern.startswith('tile64'):
        return '%s:%s' % (kern, walk(St, case['p'], False))
    nkt = -(-St // 32)
    split = 'ksplit:%s' % ('nkt<nw' if nkt < NW else 'nkt>=nw') if QB == 1 else 'qblocks'
    return '%s:%s:%s' % (kern, split, walk(St, case['p'], False))


def bwd_shape(case):
    St, _ = sizes(case)
    nkt = -(-St // 32)
    if case['dtype'] == 'bfloat16':
        if case['D'] != 64:
            return 'bwd_bf16_d16', 4
        return ('bwd_bf16_nw1', 1) if nkt <= 1 else (('bwd_bf16_nw2', 2) if nkt <= 4 else ('bwd_bf16_nw4', 4))
    return ('bwd_f32' if case['D'] == 64 else 'bwd_f32_d16'), 2


def bwd_path(case):
    St, QB = sizes(case)
    return '%s:%s:%s:dbias_%s' % (bwd_shape(case)[0], 'qb1' if QB == 1 else 'qb>1', walk(St, case['p'], False),
                                 case['dbias'] if case['bias'] else 'none')


# the sizes at which a path can still go wrong (tile and workgroup edges); other sizes are no path of their own
EDGE_TQ = (1, 31, 32, 33, 64, 95, 96, 97, 127, 128, 129, 160)
EDGE_ST = (1, 2, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 193, 256, 257)
FAMILY = {'fwd_bf16_d16': 'fwd_d16', 'fwd_f32_d16': 'fwd_d16', 'bwd_bf16_d16': 'bwd_d16', 'bwd_f32_d16': 'bwd_d16'}


def family(name):
    """the two D = 16 instantiations of a kernel count as one family in the layout coverage"""
    return FAMILY.get(name, name)


def tq_class(Tq):
    return 'tq:ksplit' if Tq <= 32 else ('tq:own_blocks' if Tq <= 96 else ('tq:one_wg' if Tq <= 128 else 'tq:two_wgs'))


def paths(case):
    St, QB = sizes(case)
    virt = {(1, 1): 'bias+zero', (1, 0): 'bias', (0, 1): 'zero', (0, 0): 'none'}[(int(case['bias']), int(case['zero']))]
    kern = fwd_kernel(case)[0]
    p = {fwd_path(case), kern + ':virtual:' + virt, kern + ':mask:' + case['mask'], kern + ':layout:' + case['layout'],
         kern + ':profile:' + case['profile'], kern + ':' + tq_class(case['Tq']), kern + ':p%g' % case['p']}
    if St in EDGE_ST:
        p.add('st:%d' % St)
    if case['Tq'] in EDGE_TQ:
        p.add('tq:%d' % case['Tq'])
    if case['S'] == 0:
        p.add(kern + ':no_real_keys')
    if case['bwd']:
        p |= {bwd_path(case), bwd_shape(case)[0] + ':layout:' + case['layout'], bwd_shape(case)[0] + ':qb%d' % QB,
              bwd_shape(case)[0] + ':st%d' % St, bwd_shape(case)[0] + ':virtual:' + virt}
    return p


# ================================================================ inputs
MASKS = ('none', 'ragged', 'sample0', 'last_only', 'first_only', 'tile32', 'tile64', 'first64')
PROFILES = ('plain', 'staircase', 'step7.9', 'jump', 'descending', 'one_row', 'cliff')
LAYOUTS = ('dense', 'kv_packed', 'batch_major', 'q_slice')


def key_mask(case):
    """[B, S] uint8, 1 = masked; None for 'none'"""
    B, S, kind = case['B'], case['S'], case['mask']
    if kind == 'none' or S == 0:
        return None
    m = np.zeros((B, S), np.uint8)
    if kind == 'ragged':
        for b in range(B):
            m[b, S - min(S - 1, 3 + 5 * b):] = 1
    elif kind == 'sample0':                        # every key of sample 0, a ragged tail on the others
        m[0] = 1
        m[1:, S - min(S - 1, 2):] = 1
    elif kind == 'last_only':
        m[:, :S - 1] = 1
    elif kind == 'first_only':
        m[:, 1:] = 1
    elif kind == 'tile32':
        m[:, 32:64] = 1
    elif kind == 'tile64':
        m[:, 64:128] = 1
    elif kind == 'first64':
        m[:, :64] = 1
    return m


def inputs(case):
    """q, dout [B, H, Tq, D]; k, v [B, H, S, D]; bk, bv [H, D] or None; mask: fp32 arrays holding storage-rounded values.
    Column 0 carries the score profile (q[..., 0] = 1 on the rows that see it, k[..., 0] = the profile), the other columns are
    random: sd 0.35 x 1 for 'plain' (scores of a few units), small otherwise so that the profile decides each tile's maximum.
    'cliff': every key from 64 on is ahead by 86 - 64 e^86 is past fp32, so a running maximum that stays behind shows as inf"""
    def make():
        r = _rng('attn', case['id'])
        B, H, Tq, S, D, dty, prof = case['B'], case['H'], case['Tq'], case['S'], case['D'], case['dtype'], case['profile']
        q = r.standard_normal((B, H, Tq, D)) * (0.35 if D == 64 else 0.7)
        k, v = r.standard_normal((B, H, S, D)), r.standard_normal((B, H, S, D))
        bk, bv = r.standard_normal((H, D)), r.standard_normal((H, D))
        s = np.arange(S)
        if prof != 'plain':
            q *= 0.5 if prof != 'step7.9' else 0.003
            q[..., 0] = 1.0
            k[..., 0] = {'staircase': 6.0 * (s // 64), 'step7.9': 7.9 * (s >= 64), 'jump': 120.0 * (s == min(S - 1, 70)),
                         'descending': -6.0 * (s // 64), 'one_row': 6.0 * (s // 64), 'cliff': 86.0 * (s >= 64)}[prof]
            if prof == 'one_row':
                q[..., 0] = 0.0
                q[..., min(Tq - 1, 5), 0] = 1.0
        out = dict(q=store(q, dty), k=store(k, dty), v=store(v, dty), dout=store(r.standard_normal((B, H, Tq, D)), dty),
                   bk=store(bk, dty) if case['bias'] else None, bv=store(bv, dty) if case['bias'] else None, mask=key_mask(case))
        return out
    return cached(('attn_in', case['id']), make)


def salt_of(*key):
    return zlib.crc32(repr(key).encode()) & 0xFFFFFFFF


def keep_of(case, salt=None, mutant=None):
    """[B, H, Tq, S_total] 0 / 1 keep flags (None at p = 0)"""
    if not case['p']:
        return None
    salt = salt_of('attn', case['id']) if salt is None else salt

    def make():
        from tell_amd import rng
        B, H, Tq = case['B'], case['H'], case['Tq']
        St = sizes(case)[0]
        b, h, t, s = np.meshgrid(*(np.arange(n, dtype=np.uint64) for n in (B, H, Tq, St)), indexing='ij')
        quads = St % 4 == 0 and fwd_kernel(case)[0] in ('reg', 'self')
        if mutant == 'keep_pair_swapped' and St % 2 == 0:            # the pair walk's two outputs
            s = s ^ np.uint64(1)
        if mutant == 'keep_quad_rotated' and quads:                 # the quad walk's four
            s = (s & ~np.uint64(3)) | ((s + np.uint64(1)) & np.uint64(3))
        bh = b if mutant == 'keep_index_without_head' else b * np.uint64(H) + h
        return rng.keep_mask(SEED, salt, (bh * np.uint64(Tq) + t) * np.uint64(St) + s, case['p'])
    return cached(('attn_keep', case['id'], salt, mutant), make)


def inv_keep(p, dt):
    """1 / (1 - p): as the launcher computes it (fp32 on the host), or exactly for the reference"""
    p32 = np.float32(p)
    return dt(np.float32(1) / (np.float32(1) - p32)) if dt is F32 else 1.0 / (1.0 - float(p32))


class Problem:
    """one case as the kernels see it: K, V [B, H, S_total, D] with the virtual keys appended, live [B, 1, 1, S_total], the
    keep flags; a key mutant changes which keys count, a dropout mutant which flags"""

    def __init__(self, case, mutant=None, salt=None):
        x = inputs(case)
        B, H, Tq, S, D = case['B'], case['H'], case['Tq'], case['S'], case['D']
        self.case, self.x = case, x
        k, v, bk, bv, mask = x['k'], x['v'], x['bk'], x['bv'], x['mask']
        if mutant == 'head_swap':
            k = k[:, ::-1]
        if mutant == 'mask_of_other_sample' and mask is not None:
            mask = np.roll(mask, -1, 0)
        live = np.ones((B, S), bool) if mask is None else mask == 0
        ks, vs, lv = [k], [v], [live]
        if case['bias']:
            ks.append(np.broadcast_to(bk, (B, H, D))[:, :, None])
            vs.append(np.broadcast_to(bk if mutant == 'bias_v_as_bias_k' else bv, (B, H, D))[:, :, None])
            lb = np.ones((B, 1), bool)
            if mutant == 'bias_masked' and S and mask is not None:   # the mask read at key index S: the NEXT sample's first key
                lb[:-1, 0] = mask[1:, 0] == 0
            lv.append(lb)
        if case['zero']:
            ks.append(np.zeros((B, H, 1, D), F32))
            vs.append(np.zeros((B, H, 1, D), F32))
            lv.append(np.full((B, 1), mutant != 'no_zero_key'))
        self.K, self.V, live = np.concatenate(ks, 2), np.concatenate(vs, 2), np.concatenate(lv, 1)
        St = self.St = live.shape[1]
        s = np.arange(St)
        if mutant == 'drop_last_key':
            live[:, St - 1] = False
        kern, QB = fwd_kernel(case)[0], sizes(case)[1]
        if mutant == 'drop_second_tile64':                    # any kernel: the keys 64 .. 127
            live[:, (s >= 64) & (s < 128)] = False
        if mutant == 'drop_odd_tile' and kern == 'self':      # the second tile of every unrolled pair: the self kernel only
            live[:, (s // 64) % 2 == 1] = False
        if mutant == 'ksplit_wave3_lost' and QB == 1 and kern.startswith('fwd'):      # KSPLIT only: the 32-key tiles of wave 3
            live[:, (s // 32) % NW == 3] = False
        self.tail = mutant == 'tail_key_live'         # key S_total of a ragged last tile counts: score 0, value 0
        self.live = live[:, None, None, :]
        self.q, self.dout = x['q'], x['dout']
        self.keep = keep_of(case, salt, mutant if mutant in DROP_MUTANTS else None)
        self.p = case['p']


# ================================================================ forward
def _scores(pr, dt):
    q, K = np.asarray(pr.q, dt), np.asarray(pr.K, dt)
    with np.errstate(all='ignore'):
        s = np.matmul(q, np.swapaxes(K, -1, -2))
    return np.where(pr.live, s, dt(-np.inf))


def fwd_gamma(case):
    St, _ = sizes(case)
    return case['D'] + St + 5 * -(-St // 32) + 48


def attn_fwd(case, mutant=None, salt=None):
    """float64: softmax over the live keys, dropout, P V -> out [B, H, Tq, D], lse [B, H, Tq] as Out, and what the bounds and
    the coverage facts are made of"""
    pr = Problem(case, mutant, salt)
    kern = fwd_kernel(case)[0]
    dty, p = case['dtype'], case['p']
    s = _scores(pr, F64)
    V = np.asarray(pr.V, F64)
    if pr.tail and pr.St % 32:
        s = np.concatenate([s, np.zeros(s.shape[:-1] + (1,))], -1)
        V = np.concatenate([V, np.zeros(V.shape[:2] + (1, V.shape[3]))], 2)
    n = s.shape[-1]
    mx = s.max(-1)
    dead = ~np.isfinite(mx)                                          # no live key
    m0 = np.where(dead, 0.0, mx)
    e = np.exp(s - m0[..., None])
    l = e.sum(-1)
    w1 = e / np.where(dead, 1.0, l)[..., None]                       # undropped softmax
    kf = np.ones(s.shape) if pr.keep is None else np.asarray(pr.keep, F64) * float(inv_keep(p, F64))
    if kf.shape[-1] < n:
        kf = np.concatenate([kf, np.ones(kf.shape[:-1] + (1,))], -1)
    w = w1 * kf
    out = np.matmul(w, V)
    with np.errstate(divide='ignore'):
        lse = np.where(dead, np.inf, m0 + np.log(np.where(dead, 1.0, (e * kf).sum(-1) if mutant == 'dropout_scales_lse' else l)))
    if mutant == 'lse_base2':
        lse = lse / np.log(2.0)
    a = np.matmul(np.abs(np.asarray(pr.q, F64)), np.swapaxes(np.abs(np.asarray(pr.K, F64)), -1, -2))
    if a.shape[-1] < n:
        a = np.concatenate([a, np.zeros(a.shape[:-1] + (1,))], -1)
    sf = np.where(np.isfinite(s), s, 0.0)
    R = 1.0 + a + np.abs(sf - m0[..., None]) + np.abs(m0)[..., None] + THR
    Rbar = (w1 * R).sum(-1)
    aV = np.abs(V)
    S_out = np.matmul(w * R, aV) + np.matmul(w, aV) * Rbar[..., None]
    extra = TINY * np.exp(THR) * aV.sum(2)[:, :, None, :] * np.ones(out.shape)
    if dty == 'bfloat16':
        extra = extra + 2.0 ** -8 * np.matmul(w, aV)
    S_lse = 1.0 + np.abs(np.where(dead, 0.0, lse)) + np.abs(m0) + THR + Rbar
    gam = fwd_gamma(case)
    dead4 = np.broadcast_to(dead[..., None], out.shape)
    return dict(out=Out(np.where(dead4, 0.0, out), S_out, gam, dty, kern + '_out', extra, dead4),
                lse=Out(lse, S_lse, gam, 'float32', kern + '_lse', 0.0, dead),
                w1=w1, w=w, scores=s, dead=dead, problem=pr)


def _kernel_shape(kern):
    """key tile, lazy maximum, probabilities rounded to bf16, 1 / (1 - p) applied to the output row instead of each probability"""
    bf = kern in ('fwd_bf16', 'fwd_bf16_d16', 'tile64_bf16', 'reg', 'self')
    return dict(KT=32 if kern.startswith('fwd') else 64, lazy=kern == 'self', bf=bf, late=kern in ('reg', 'self'))


def attn_fwd_tiled(case, dt=F32, mutant=None, salt=None):
    """the launched kernel's own order in `dt`: key tiles of 32 or 64, the online rescale (the self kernel's lazy maximum is a
    test over the 32 query rows of a wave, rows past Tq included - their q is zero), probabilities rounded to bf16 in front of
    P V, the four key streams of KSPLIT combined through their maxima -> stored out, lse (fp32 arrays)"""
    pr = Problem(case, mutant if mutant not in TILED_MUTANTS else None, salt)
    kern = fwd_kernel(case)[0]
    ks = _kernel_shape(kern)
    B, H, Tq, D, St, p = case['B'], case['H'], case['Tq'], case['D'], pr.St, case['p']
    QB = -(-Tq // 32)
    Tp = QB * 32
    q = np.zeros((B, H, Tp, D), dt)
    q[:, :, :Tq] = pr.q
    K, V = np.asarray(pr.K, dt), np.asarray(pr.V, dt)
    with np.errstate(all='ignore'):
        s = np.where(pr.live, np.matmul(q, np.swapaxes(K, -1, -2)), dt(-np.inf)).astype(dt)
    ik = inv_keep(p, dt)
    keep = np.ones((B, H, Tp, St), dt)
    if pr.keep is not None:
        keep[:, :, :Tq] = pr.keep
    KT = ks['KT']
    nkt = -(-St // KT)
    streams = [range(w, nkt, NW) for w in range(NW)] if (QB == 1 and KT == 32) else [range(nkt)]
    rnd = (lambda a: bf16_round(a).astype(dt)) if (ks['bf'] and dt is F32) else (lambda a: a)
    res = []
    for tiles in streams:
        m = np.full((B, H, Tp), -np.inf, dt)
        l = np.zeros((B, H, Tp), dt)
        o = np.zeros((B, H, Tp, D), dt)
        for kt in tiles:
            sl = slice(kt * KT, min((kt + 1) * KT, St))
            st = s[..., sl]
            with np.errstate(all='ignore'):
                mc = np.maximum(m, st.max(-1))
                if ks['lazy']:
                    move = ~(mc - m <= dt(THR))
                    move = np.broadcast_to(move.reshape(B, H, QB, 32).any(-1, keepdims=True), (B, H, QB, 32)).reshape(B, H, Tp)
                    if mutant == 'lazy_max_never_moves':
                        move = np.isinf(m)
                else:
                    move = np.ones((B, H, Tp), bool)
                m_new = np.where(move, mc, m)
                alpha = np.where(move, np.where(np.isinf(m), dt(0), np.exp(m - m_new)), dt(1)).astype(dt)
                m_safe = np.where(np.isinf(m_new), dt(0), m_new)
                pv = np.exp(st - m_safe[..., None]).astype(dt)
                l = (l * alpha + pv.sum(-1, dtype=dt)).astype(dt)
                kk = keep[..., sl] if ks['late'] else (keep[..., sl] * ik).astype(dt)
                pd = rnd((pv * kk).astype(dt))
                if mutant != 'no_rescale':
                    o = (o * alpha[..., None]).astype(dt)
                o = (o + np.matmul(pd, V[:, :, sl])).astype(dt)
            m = m_new
        res.append((m, l, o))
    with np.errstate(all='ignore'):
        if len(res) > 1:
            mm = np.maximum.reduce([r[0] for r in res])
            l, o = np.zeros_like(res[0][1]), np.zeros_like(res[0][2])
            for m_w, l_w, o_w in res:
                sc = np.where(np.isinf(m_w), dt(0), np.exp(m_w - mm)).astype(dt)
                l = (l + l_w * sc).astype(dt)
                o = (o + o_w * sc[..., None]).astype(dt)
            m = mm
        else:
            m, l, o = res[0]
        inv_l = np.where(l > 0, dt(1) / np.where(l > 0, l, dt(1)), dt(0)).astype(dt)
        if ks['late']:
            inv_l = (inv_l * ik).astype(dt)
        out = (o * inv_l[..., None]).astype(dt)
        lse = np.where(l > 0, m + np.log(np.where(l > 0, l, dt(1))), dt(np.inf)).astype(dt)
    return dict(out=store(out[:, :, :Tq], case['dtype']), lse=store(lse[:, :, :Tq], 'float32'))


def lazy_moves(case):
    """coverage facts of a self-kernel case in float64: how often a wave moved its running maximum after the first tile, and the
    largest probability exp(s - m_run) any live key was given"""
    pr = Problem(case)
    s = _scores(pr, F64)
    B, H, Tq, St = s.shape
    m = np.full((B, H, Tq), -np.inf)
    moves, top = 0, 0.0
    for kt in range(St // 64):
        st = s[..., kt * 64:(kt + 1) * 64]
        with np.errstate(all='ignore'):
            mc = np.maximum(m, st.max(-1))
            move = ~(mc - m <= THR)
        any_ = np.zeros_like(move)
        for w0 in range(0, Tq, 32):
            any_[..., w0:w0 + 32] = move[..., w0:w0 + 32].any(-1, keepdims=True)
        if kt:
            moves += int(any_.any())
        m = np.where(any_, mc, m)
        with np.errstate(all='ignore'):
            top = max(top, float(np.exp(st - np.where(np.isinf(m), 0.0, m)[..., None]).max()))
    return moves, top


# ================================================================ backward
def bwd_gamma(case):
    St, QB = sizes(case)
    return case['D'] + 40 + QB + -(-St // 32)


def attn_bwd(case, out_st, lse_st, mutant=None, salt=None):
    """float64, from the STORED out [B, H, Tq, D] and lse [B, H, Tq] -> dq, dk, dv [and dbias_k, dbias_v [B, H D]] as Out"""
    pr = Problem(case, mutant if mutant in KEY_MUTANTS + DROP_MUTANTS and mutant not in FWD_TILE_MUTANTS else None, salt)
    grp, nw = bwd_shape(case)
    B, H, Tq, S, D, dty, p = case['B'], case['H'], case['Tq'], case['S'], case['D'], case['dtype'], case['p']
    St, QB = pr.St, -(-Tq // 32)
    bf = dty == 'bfloat16'
    q, K, V, do = (np.asarray(a, F64) for a in (pr.q, pr.K, pr.V, pr.dout))
    o, lse = np.asarray(out_st, F64), np.asarray(lse_st, F64)
    s = _scores(pr, F64)
    with np.errstate(all='ignore'):
        P = np.where(np.isfinite(s) & np.isfinite(lse)[..., None], np.exp(np.where(np.isfinite(s), s, 0.0) -
                                                                           np.where(np.isfinite(lse), lse, 0.0)[..., None]), 0.0)
    kf = np.ones(s.shape) if pr.keep is None else np.asarray(pr.keep, F64) * float(inv_keep(p, F64))
    dP = np.matmul(do, np.swapaxes(V, -1, -2))
    delta = (do * o).sum(-1)
    if mutant == 'bwd_delta_without_keep':            # delta as the undropped sum_s P dP: off by sum_s P dP (1 - keep / (1 - p))
        delta = delta + (P * dP * (1.0 - kf)).sum(-1)
    dS = P * (kf * dP - delta[..., None])
    Pd = P * (1.0 if mutant == 'dv_from_undropped_p' else kf)
    if mutant == 'bwd_second_wave_lost':
        dSq = np.where(((np.arange(St) // 32) % nw == 1) & (nw > 1), 0.0, dS)
    else:
        dSq = dS
    aq, aK, aV, ado = (np.abs(x) for x in (q, K, V, do))
    a = np.matmul(aq, np.swapaxes(aK, -1, -2))
    sl = np.abs(np.where(np.isfinite(s), s, 0.0) - np.where(np.isfinite(lse), lse, 0.0)[..., None])
    Rp = 1.0 + a + sl
    bts = np.matmul(ado, np.swapaxes(aV, -1, -2))
    dabs = (ado * np.abs(o)).sum(-1)[..., None]
    M = np.abs(dS) * Rp + P * (kf * bts + dabs + np.abs(kf * dP) + np.abs(delta)[..., None])

    def blocks(left, right):
        """sum_t left[t, s] right[t, d] per query block -> [QB, B, H, St, D]"""
        Tp = QB * 32
        L = np.zeros(left.shape[:2] + (Tp, St))
        L[:, :, :Tq] = left
        Rr = np.zeros(right.shape[:2] + (Tp, D))
        Rr[:, :, :Tq] = right
        L, Rr = L.reshape(B, H, QB, 32, St), Rr.reshape(B, H, QB, 32, D)
        return np.moveaxis(np.matmul(np.swapaxes(L, -1, -2), Rr), 2, 0)

    dVb, dKb = blocks(Pd, do), blocks(dS, q)
    if mutant == 'bwd_dk_last_qblock_only':
        dV_all, dK_all = dVb[-1], dKb[-1]
    else:
        dV_all, dK_all = dVb.sum(0), dKb.sum(0)
    run_v = np.abs(np.cumsum(dVb, 0)[:-1]).sum(0)                    # the partials stored and read back (all but the last)
    run_k = np.abs(np.cumsum(dKb, 0)[:-1]).sum(0)
    S_dv = np.matmul(np.swapaxes(P * kf * Rp, -1, -2), ado) + run_v
    S_dk = np.matmul(np.swapaxes(M, -1, -2), aq) + run_k
    S_dq = np.matmul(M, aK)
    dQ = np.matmul(dSq, K)
    u8 = 2.0 ** -8 if bf else 0.0
    x_dv = u8 * np.matmul(np.swapaxes(np.abs(P * kf), -1, -2), ado)
    x_dk = u8 * np.matmul(np.swapaxes(np.abs(dS), -1, -2), aq)
    x_dq = u8 * np.matmul(np.abs(dS), aK)
    gam = bwd_gamma(case)
    masked = np.broadcast_to(~pr.live[:, :, 0, :S, None], (B, H, S, D))                 # masked real keys: exactly +-0
    deadq = np.broadcast_to(~np.isfinite(lse)[..., None], dQ.shape)
    out = dict(dq=Out(dQ, S_dq, gam, dty, grp + '_dq', x_dq, deadq, True),
               dk=Out(dK_all[:, :, :S], S_dk[:, :, :S], gam, dty, grp + '_dk', x_dk[:, :, :S] + u8 * run_k[:, :, :S], masked, True),
               dv=Out(dV_all[:, :, :S], S_dv[:, :, :S], gam, dty, grp + '_dv', x_dv[:, :, :S] + u8 * run_v[:, :, :S], masked, True))
    if case['bias']:
        gk, gv = dK_all[:, :, S], dV_all[:, :, S]
        if mutant == 'dbias_not_summed_over_t':
            gk, gv = dS[:, :, -1, S, None] * q[:, :, -1], Pd[:, :, -1, S, None] * do[:, :, -1]
        flat = lambda x: x.reshape(B, H * D)                                                    # noqa: E731
        for name, g, Sx, ex in (('dbias_k', gk, S_dk, x_dk), ('dbias_v', gv, S_dv, x_dv)):
            out[name] = Out(flat(g), flat(Sx[:, :, S]), gam, 'float32', grp + '_dbias', flat(ex[:, :, S]))
    return out


def attn_bwd_tiled(case, out_st, lse_st, dt=F32, salt=None):
    """the backward kernel's own order in `dt`: one workgroup per (b, h), query blocks of 32 outside, every 32-key tile owned by
    wave kt % NW; Pd, dS^T and dS rounded to bf16 in the bf16 kernels; dQ of a block folded over the waves in order; dK / dV
    stored in the storage type and read back once per later query block; the bias-key row accumulates in fp32"""
    pr = Problem(case, None, salt)
    grp, nw = bwd_shape(case)
    B, H, Tq, S, D, dty, p = case['B'], case['H'], case['Tq'], case['S'], case['D'], case['dtype'], case['p']
    St, QB = pr.St, -(-Tq // 32)
    bf = dty == 'bfloat16'
    rnd = (lambda x: bf16_round(x).astype(dt)) if (bf and dt is F32) else (lambda x: x)
    st_ = (lambda x: store(x, dty).astype(dt)) if dt is F32 else (lambda x: x)
    Tp = QB * 32
    pad = lambda x: np.concatenate([np.asarray(x, dt), np.zeros(x.shape[:2] + (Tp - Tq,) + x.shape[3:], dt)], 2)   # noqa: E731
    q, do, o = pad(pr.q), pad(pr.dout), pad(np.asarray(out_st, dt))
    lse = np.concatenate([np.asarray(lse_st, dt), np.full((B, H, Tp - Tq), np.inf, dt)], 2)
    K, V = np.asarray(pr.K, dt), np.asarray(pr.V, dt)
    ik = inv_keep(p, dt)
    keep = np.ones((B, H, Tp, St), dt)
    if pr.keep is not None:
        keep[:, :, :Tq] = (pr.keep * ik).astype(dt)
    live = np.broadcast_to(pr.live, (B, H, Tp, St)) & (np.arange(Tp) < Tq)[None, None, :, None]
    nkt = -(-St // 32)
    dK, dV = np.zeros((B, H, St, D), dt), np.zeros((B, H, St, D), dt)
    dQ = np.zeros((B, H, Tp, D), dt)
    with np.errstate(all='ignore'):
        for qb in range(QB):
            t = slice(qb * 32, qb * 32 + 32)
            delta = (do[:, :, t] * o[:, :, t]).sum(-1, dtype=dt)
            dq_w = [np.zeros((B, H, 32, D), dt) for _ in range(nw)]
            for kt in range(nkt):
                sl = slice(kt * 32, min(kt * 32 + 32, St))
                s = np.matmul(q[:, :, t], np.swapaxes(K[:, :, sl], -1, -2)).astype(dt)
                dp = np.matmul(do[:, :, t], np.swapaxes(V[:, :, sl], -1, -2)).astype(dt)
                pv = np.where(live[:, :, t, sl], np.exp(s - lse[:, :, t, None]), dt(0)).astype(dt)
                kp = keep[:, :, t, sl]
                ds = (pv * ((dp * kp).astype(dt) - delta[..., None]).astype(dt)).astype(dt)
                pd, dsr = rnd((pv * kp).astype(dt)), rnd(ds)
                dv = np.matmul(np.swapaxes(pd, -1, -2), do[:, :, t]).astype(dt)
                dk = np.matmul(np.swapaxes(dsr, -1, -2), q[:, :, t]).astype(dt)
                dq_w[kt % nw] = (dq_w[kt % nw] + np.matmul(dsr, K[:, :, sl])).astype(dt)
                real = slice(sl.start, min(sl.stop, S))
                n = max(real.stop - real.start, 0)
                if qb:
                    dv, dk = (dv + dV[:, :, sl]).astype(dt), (dk + dK[:, :, sl]).astype(dt)
                dV[:, :, sl], dK[:, :, sl] = dv, dk
                if n:
                    dV[:, :, real], dK[:, :, real] = st_(dv[:, :, :n]), st_(dk[:, :, :n])
            acc = dq_w[0]
            for w in range(1, nw):
                acc = (acc + dq_w[w]).astype(dt)
            dQ[:, :, t] = acc
    out = dict(dq=store(dQ[:, :, :Tq], dty), dk=store(dK[:, :, :S], dty), dv=store(dV[:, :, :S], dty))
    if case['bias']:
        out['dbias_k'] = store(dK[:, :, S].reshape(B, H * D), 'float32')
        out['dbias_v'] = store(dV[:, :, S].reshape(B, H * D), 'float32')
    return out


# ================================================================ head-averaged weights
def avg_weights(case, lse_st, dt=F64, mutant=None):
    """w[b, t, s] = (1 / H) sum_h exp(q_h . k_h[s] - lse[b, h, t]), 0 on a masked key -> [B, Tq, S_total] fp32"""
    pr = Problem(case)
    q, K = np.asarray(pr.q, dt), np.asarray(pr.K, dt)
    H = case['H']
    lse = np.asarray(lse_st, dt)
    with np.errstate(all='ignore'):
        dot = np.matmul(q, np.swapaxes(K, -1, -2)).astype(dt)
        e = np.where(pr.live, np.exp(dot - lse[..., None]), dt(0)).astype(dt)
        acc = np.zeros(e.shape[:1] + e.shape[2:], dt)
        for h in range(H):
            acc = (acc + e[:, h]).astype(dt)
        w = acc if mutant == 'avg_w_not_divided_by_H' else (acc / dt(H)).astype(dt)
    a = np.matmul(np.abs(np.asarray(pr.q, F64)), np.swapaxes(np.abs(np.asarray(pr.K, F64)), -1, -2))
    e64 = np.asarray(e, F64)
    with np.errstate(all='ignore'):
        sl = np.where(e64 > 0, np.abs(np.asarray(dot, F64) - np.asarray(lse, F64)[..., None]), 0.0)
    S = (e64 * (1.0 + a + sl)).sum(1) / H
    masked = np.broadcast_to(~pr.live[:, 0], w.shape)
    return Out(w, S, case['D'] + H + 8, 'float32', 'avg_w_bf16' if case['dtype'] == 'bfloat16' else 'avg_w_f32', 0.0, masked)


# ================================================================ cases
def _c(id, dtype, Tq, S, mutants=(), **kw):
    c = dict(id=id, dtype={'bf16': 'bfloat16', 'f32': 'float32'}[dtype], B=2, H=2, D=64, Tq=Tq, S=S, bias=False, zero=False, p=0.0,
             mask='none', profile='plain', layout='dense', opts=None, bwd=False, dbias='two', mutants=tuple(mutants), not_caught=())
    c.update(kw)
    return c


BZ, B_, Z_ = dict(bias=True, zero=True), dict(bias=True), dict(zero=True)
CASES = [
    # ---- attn_fwd_kernel<bf16, 64>: KSPLIT (Tq <= 32), S_total 1 / 2 of virtual keys alone, the backward edges 32 | 33
    _c('k1_s0_b', 'bf16', 1, 0, ['bias_v_as_bias_k'], bwd=True, **B_),
    _c('k31_s0_bz', 'bf16', 31, 0, ['no_zero_key', 'keep_pair_swapped', 'dbias_not_summed_over_t'], p=0.1, bwd=True, dbias='one', **BZ, layout='batch_major'),
    _c('k32_s31', 'bf16', 32, 31, ['mask_of_other_sample', 'keep_index_without_head'], p=0.1, mask='sample0',
       bwd=True, not_caught=('keep_pair_swapped', 'keep_quad_rotated', 'no_zero_key', 'bias_v_as_bias_k', 'bwd_second_wave_lost', 'dbias_not_summed_over_t',), layout='q_slice'),
    _c('k32_s31_z', 'bf16', 32, 31, ['no_zero_key', 'dv_from_undropped_p'], p=0.1, mask='ragged', bwd=True, layout='kv_packed', **Z_),
    _c('k32_s31_bz', 'bf16', 32, 31, ['bias_v_as_bias_k', 'bwd_delta_without_keep'], p=0.1, mask='ragged',
       bwd=True, dbias='one', **BZ, not_caught=('bias_masked', 'bwd_dk_last_qblock_only',)),
    _c('k1_s128', 'bf16', 1, 128, ['ksplit_wave3_lost', 'head_swap'], p=0.5, mask='tile32', bwd=True, H=3, not_caught=('tail_key_live',)),
    _c('k31_s127_bz', 'bf16', 31, 127, ['tail_key_live', 'bwd_second_wave_lost', 'ksplit_wave3_lost'], p=0.1, bwd=True,
       layout='batch_major', **BZ),
    _c('k32_s63_last', 'bf16', 32, 63, ['drop_last_key'], mask='last_only', layout='q_slice', bwd=True, not_caught=('drop_second_tile64',)),
    _c('k31_s64_first', 'bf16', 31, 64, ['lse_base2'], mask='first_only', profile='jump', not_caught=('drop_last_key',)),
    _c('k32_s257_jump', 'bf16', 32, 257, ['head_swap', 'lse_base2'], profile='jump'),
    # ---- the waves own query blocks (Tq 33 .. 96), QB 2 / 3, more S_total classes
    _c('q33_s63_b', 'bf16', 33, 63, ['bwd_dk_last_qblock_only', 'lse_base2'], bwd=True, layout='kv_packed', **B_, not_caught=('bwd_delta_without_keep', 'dv_from_undropped_p',)),
    _c('q64_s127', 'bf16', 64, 127, ['tail_key_live', 'keep_index_without_head'], p=0.1, mask='ragged', bwd=True, layout='batch_major'),
    _c('q95_s64_bz', 'bf16', 95, 64, ['keep_pair_swapped', 'dropout_scales_lse'], p=0.5, mask='tile32', bwd=True, dbias='one', **BZ),
    _c('q64_s96_b_first64', 'bf16', 64, 96, ['bias_masked'], mask='first64', bwd=True, not_caught=('no_zero_key', 'mask_of_other_sample',), **B_),
    _c('q96_s193', 'bf16', 96, 193, ['no_rescale'], profile='staircase', mask='tile64', not_caught=('ksplit_wave3_lost',)),
    _c('q96_s130', 'bf16', 96, 130, ['drop_second_tile64'], layout='batch_major', not_caught=('keep_index_without_head', 'dropout_scales_lse',)),
    # ---- reg kernel (Tq >= 97): three walks, four virtual-key forms, the options, S % 64 alone
    _c('r97_s62_bz', 'bf16', 97, 62, ['keep_quad_rotated', 'no_zero_key'], p=0.1, mask='ragged', **BZ),
    _c('r128_s64_b', 'bf16', 128, 64, ['bias_v_as_bias_k', 'keep_index_without_head'], p=0.1, layout='kv_packed', **B_),
    _c('r129_s65_z', 'bf16', 129, 65, ['keep_pair_swapped', 'no_zero_key'], p=0.5, mask='tile32', layout='q_slice', **Z_,
       not_caught=('keep_quad_rotated',)),
    _c('r160_s130', 'bf16', 160, 130, ['drop_second_tile64', 'tail_key_live'], p=0.1, mask='sample0', bwd=True, H=3, layout='q_slice'),
    _c('r97_s128_noself', 'bf16', 97, 128, ['keep_quad_rotated'], p=0.1, opts=dict(attn_self=0), mask='first64'),
    _c('r128_s256_occ3', 'bf16', 128, 256, ['no_rescale'], p=0.1, opts=dict(attn_self=0, attn_occ=3), profile='staircase', not_caught=('drop_odd_tile',)),
    _c('r128_s128_occ3', 'bf16', 128, 128, ['drop_last_key'], opts=dict(attn_self=0, attn_occ=3), mask='last_only'),
    _c('r160_s66', 'bf16', 160, 66, ['drop_last_key', 'tail_key_live']),
    _c('r127_s257', 'bf16', 127, 257, ['lse_base2'], mask='ragged', profile='descending', layout='batch_major'),
    # ---- tile64 kernel: fp32 (the default for fp32) and bf16 behind attn_tile64 = 1
    _c('t97_s63_bz_f32', 'f32', 97, 63, ['no_zero_key', 'bias_masked'], p=0.1, mask='last_only', bwd=True, dbias='one', **BZ),
    _c('t128_s129_z_f32', 'f32', 128, 129, ['drop_second_tile64', 'keep_pair_swapped'], p=0.5, mask='sample0', layout='kv_packed',
       zero=True, not_caught=('keep_quad_rotated',)),
    _c('t160_s255_b_f32', 'f32', 160, 255, ['no_rescale', 'lse_base2'], profile='staircase', layout='q_slice', bias=True),
    _c('t97_s64_f32', 'f32', 97, 64, ['mask_of_other_sample'], mask='sample0', layout='batch_major'),
    _c('t129_s66_bf16', 'bf16', 129, 66, ['keep_pair_swapped'], p=0.1, opts=dict(attn_tile64=1), mask='tile32', layout='kv_packed'),
    _c('t128_s128_bf16', 'bf16', 128, 128, ['drop_second_tile64'], opts=dict(attn_tile64=1), profile='jump', layout='batch_major'),
    _c('t97_s192_b_bf16', 'bf16', 97, 192, ['bias_v_as_bias_k'], p=0.5, opts=dict(attn_tile64=1), mask='tile64', **B_, layout='q_slice'),
    # ---- self kernel: Tq 97 / 128 / 160 x S 64 / 128 / 192 / 256, p 0 / 0.1 / 0.5, the four masks, the score profiles, DMA
    _c('s97_s64', 'bf16', 97, 64, ['keep_quad_rotated', 'dropout_scales_lse'], p=0.1, mask='ragged'),
    _c('s128_s128', 'bf16', 128, 128, ['drop_odd_tile', 'head_swap'], p=0.5, mask='first64', bwd=True),
    _c('s160_s192', 'bf16', 160, 192, ['drop_odd_tile', 'mask_of_other_sample'], mask='sample0', layout='kv_packed', H=3),
    _c('s128_s256_stair', 'bf16', 128, 256, ['no_rescale', 'drop_odd_tile'], p=0.1, profile='staircase'),
    _c('s97_s128_79', 'bf16', 97, 128, ['lse_base2'], profile='step7.9', not_caught=('lazy_max_never_moves',)),
    _c('s128_s192_jump', 'bf16', 128, 192, ['lazy_max_never_moves', 'no_rescale'], profile='jump', layout='q_slice'),
    _c('s160_s256_desc', 'bf16', 160, 256, ['keep_index_without_head'], p=0.1, profile='descending', mask='tile64', layout='batch_major',
       not_caught=('no_rescale', 'lazy_max_never_moves')),
    _c('s128_s128_cliff', 'bf16', 128, 128, ['lazy_max_never_moves'], p=0.1, profile='cliff'),
    _c('s128_s256_onerow', 'bf16', 128, 256, ['no_rescale'], profile='one_row'),
    _c('s97_s192_dma', 'bf16', 97, 192, ['keep_quad_rotated'], p=0.1, opts=dict(attn_dma=1), mask='ragged', profile='staircase'),
    _c('s128_s64_dma', 'bf16', 128, 64, ['head_swap'], opts=dict(attn_dma=1), mask='sample0'),
    # ---- D = 16 (H = 4, E = 64), both dtypes, forward and backward; Tq = 130: more than one workgroup in x
    _c('d16_k32_s33_bz', 'bf16', 32, 33, ['no_zero_key', 'bwd_delta_without_keep'], p=0.1, bwd=True,
       H=4, D=16, dbias='one', mask='ragged', **BZ, layout='batch_major'),
    _c('d16_q130_s65', 'bf16', 130, 65, ['bwd_dk_last_qblock_only', 'drop_last_key'], bwd=True, H=4, D=16, mask='tile32', layout='q_slice'),
    _c('d16_q130_s66_f32', 'f32', 130, 66, ['bwd_dk_last_qblock_only', 'keep_index_without_head'], p=0.1, bwd=True, H=4, D=16, **B_, layout='batch_major'),
    _c('d16_k1_s2_f32', 'f32', 1, 2, ['dv_from_undropped_p'], p=0.5, bwd=True, H=4, D=16, layout='kv_packed'),
    # ---- fp32 attn_fwd_kernel and the fp32 backward (NW = 2)
    _c('f32_k1_s0_z', 'f32', 1, 0, ['no_zero_key'], bwd=True, **Z_),
    _c('f32_k32_s129', 'f32', 32, 129, ['ksplit_wave3_lost', 'bwd_second_wave_lost'], p=0.1, mask='sample0', bwd=True, layout='q_slice'),
    _c('f32_q95_s33_bz', 'f32', 95, 33, ['bwd_dk_last_qblock_only', 'dbias_not_summed_over_t', 'tail_key_live'], p=0.1, bwd=True,
       layout='kv_packed', mask='ragged', **BZ),
    _c('f32_q64_s64_jump', 'f32', 64, 64, ['no_rescale'], profile='jump', bwd=True, layout='batch_major'),
    # ---- the backward's launch shapes at workgroup-sized query counts: QB = 5, bf16 NW = 4 at 129, NW = 2 at 128
    _c('b160_s128_self', 'bf16', 160, 128, ['bwd_dk_last_qblock_only', 'bwd_second_wave_lost'], p=0.1, mask='ragged', bwd=True),
    _c('b160_s127_bz', 'bf16', 160, 127, ['bwd_second_wave_lost', 'dv_from_undropped_p'], p=0.1, mask='ragged', bwd=True, dbias='two',
       layout='kv_packed', **BZ),
]

# tell_attn_avg_weights: S_total 1 / 255 / 256 / 257 (the 256-thread stride), H 1 / 3, both dtypes, mask, bias with / without zero
AVG = [
    _c('w_s0_b', 'bf16', 5, 0, ['avg_w_not_divided_by_H'], H=3, **B_),
    _c('w_s255', 'f32', 33, 255, ['drop_last_key'], H=1, mask='tile64', not_caught=('avg_w_not_divided_by_H', 'head_swap',)),
    _c('w_s255_b', 'bf16', 33, 255, ['avg_w_not_divided_by_H'], H=3, mask='ragged', **B_),
    _c('w_s255_bz', 'f32', 2, 255, ['no_zero_key'], H=3, mask='sample0', **BZ),
]
BY_ID = {c['id']: c for c in CASES + AVG}
assert len(BY_ID) == len(CASES) + len(AVG)


def fwd_case(case, mutant=None, salt=None):
    """the float64 forward of a case, cached (references are computed once and left unchanged)"""
    if mutant is None and salt is None:
        return cached(('attn_fwd', case['id']), lambda: attn_fwd(case))
    return attn_fwd(case, mutant, salt)


def stored(outs):
    return {k: store(o.value, o.dtype) for k, o in outs.items() if isinstance(o, Out)}
