"""float64 reference of the small kernels of the training step (csrc/elementwise.hip, csrc/multi.hip, csrc/lstm.hip,
csrc/encoders.hip): weight norm (single and multi-tensor, forward and backward), the RoBERTa layer mix (forward, backward
partials, logit gradient), column sums (single and multi-job), the two transposes, the LSTM cell, the dot attention and tanh of
the LSTM decoder, and the movers / pointwise kernels cast, scale_cast, axpy, sum_n, relu_bwd, gather_rows, scatter_add_rows,
nan_rows, GLU, GELU, dropout, dropout_add, loss_bits, roberta_embed and mask_rows - with the element-wise bounds they are
held to, the case tables and the mutants that tests/test_small_ref_host.py, tests/test_gpu_small_reduce.py and
tests/test_gpu_small_pointwise.py walk.  numpy only; nothing here comes from oracle/.  Inputs are
rounded to their storage type BEFORE they reach a function.

Every function takes dt (np.float64: the reference; np.float32: the same formulas with every product, transcendental and
sequential or tree sum rounded to fp32, in the kernel's order where the order is fixed - the emulation the host test holds to
the bounds at c = 1) and a mutant name (MUTANTS: wrong-answer variants that must break a bound or an exact comparison on the
case that names them).  A function returns a dict of Out: the value, S (the sum of the ABSOLUTE values of the terms the
kernel adds up for the element), gamma, the storage type and the output group.  Bound of one element:

    u_out |ref|  +  c gamma 2^-24 S  +  2^-126 (1 + S)

u_out = 2^-8 for a bf16 store, 2^-24 for fp32; c = the one measured number per output group (MEASURED, C).

gamma, read off the kernels (T = trips of one lane or thread over its share, 6 = the butterfly of a 64-lane wave):

    wn_norms, wn_scale   ceil(cols / 64) + 6 + 4       sum of squares: one lane adds cols / 64 terms, the fold, sqrt, divide
    wn_w                 ceil(cols / 64) + 6 + 4       the same norm, g / norm, one product
    wn_dg                ceil(cols / 64) + 6 + 4       S = |dg0| + S_dot / norm,  S_dot = sum |dW v|
    wn_dv                ceil(cols / 64) + 6 + 8       S = |dv0| + |g / norm| (|dW| + |v| S_dot / norm^2)
    mix_out              L + 16 + spread               L fused multiply-adds; a softmax weight e^(w - max) / sum carries the
                                                       relative error of its argument: spread = max_l |w_l - lse| for __expf,
                                                       8 for the exponential, 6 for the fold of the sum, one divide
    mix_partial          T + 6 + 3                     T = ceil(n / (256 n_blocks)) terms per thread (n / 8 chunks of 8 terms on
                                                       the vector path: 8 T), the fold, the sum of the four waves
    mix_gw               ceil(n_blocks / 16) + 16 + L + 16 + spread
                                                       the 16-way split of the partial rows and its fold, the dot product over
                                                       L, the softmax as above; S = |gw0| + sm_l (S_d[l] + sum_j sm_j S_d[j])
    colsum               ceil(rpc / 4) + 3 + nch + 2   rpc rows of a chunk over 4 row lanes, their sum, nch chunk partials,
                                                       scale and accumulate; S = |out0| + |scale| sum |x|
    colsum_multi         ceil(rows / 64) + 3 + 16 + 1  the 4-way unrolled walk of one of 16 row groups, the sum of the four
                                                       accumulators, the 16 groups, the accumulate; S = |dst0| + sum |x|
    lstm_gates, _c, _h   16 + max |pre-activation|     a sigmoid 1 / (1 + __expf(-x)) carries the rounding of x log2 e, which
                                                       grows with |x|; S_c = |f c_prev| + |i g|, S_h = o S_c (tanh of a sum
                                                       that may cancel)
    lstm_dgates, _dc_prev  16                          products of stored gates; S_dcn = |dc| + |dh o| (1 - tanh^2 is rounded on
                                                       the scale of 1), 1 - g^2 likewise: S carries 1 + g^2
    tanh_y               8                             tanhf
    da_probs             2 gP + ceil(L / 256) + 8      gP = 8 + spread + (ceil(D / 64) + 6) Lmax as in section 33 (natural log:
                                                       spread = max |s - lse| over the live keys, Lmax = max sum_d |src x|), twice
                                                       because the kernel divides by its own sum; the 256-strided sum and fold
    da_ctx               L + gamma(da_probs)           L sequential multiply-adds; S = sum_l p_l |src|
    da_dx                L + ceil(D / 64) + 6 + ceil(L / 256) + 6 + 8
                                                       S = sum_l S_ds[l] |src|, S_ds = p (S_dp + sum_l p S_dp),
                                                       S_dp = sum |dctx src|
    da_dsrc              the same without L            S = p |dctx| + S_ds |x|
    glu_y, glu_dh        8 + max |gate|                a sigmoid as above through __builtin_amdgcn_rcpf; the gate half of dh has
                                                       S = |dy a| s (1 - s is rounded on the scale of 1)

Kernels that move, select or round once have no c.  Exact (bit for bit): cast, transpose (one fp32 product with row_scale,
one rounding: computed in fp32 here whatever dt is), transpose_multi, gather_rows, nan_rows, relu_bwd, mask_rows, the
positions of roberta_embed, and the dropout masks (tell_amd.rng.keep_mask; a dropped element is x * 0 [+ add]).  Derived bound
(group None: the bound is  u_out |ref| + k 2^-24 S + 2^-126 (1 + S)  with k written below, no measured constant):

    scale_cast           k = 0: the product is rounded once when the store is fp32 ... and twice when it is bf16 (fp32 product,
                         then the bf16 store): k = 1, S = |x scale|
    axpy                 y + alpha x: without contraction the product is rounded (2^-24 |alpha x|) and then the sum (2^-24
                         |ref|, which is u_out |ref| for an fp32 store); with an FMA the product is exact.  The compiler may
                         choose either, so the bound holds the uncontracted form: fp32 k = 1 + 2^-23 on S = |alpha x| (the
                         2^-23: the sum rounds the ROUNDED product); FMA contraction needs nothing more, it only removes the
                         term.  A bf16 store takes u_out |ref| for itself, so the fp32 sum's rounding moves into k: k = 2 on
                         S = |y| + |alpha x|.
    sum_n                n_in - 1 sequential fp32 additions: k = n_in, S = sum_j |x_j|
    scatter_add_rows     one addition of stored values: one rounding in fp32 (k = 0); the bf16 store rounds the fp32 sum a
                         second time: k = 1, S = |dst0| + |src|
    tanh_bwd             dy (1 - y^2): k = 3, S = |dy| (1 + y^2)
    dropout, dropout_add kept elements: 1 / (1 - p) is a difference and a quotient in fp32, then the product [and the sum]:
                         k = 3 [4], S = |x / (1 - p)| [+ |add|]
    gelu                 against float64 erf: k = 3e-7 / 2^-24 + 112 on S = |x| / 2 (the kernel's erfc is Abramowitz-Stegun
                         7.1.28, absolute error 3e-7; see gelu())
    loss_bits            two quotients and the rounded ln 2: k = 3
    roberta_embed        word + position: one rounding in fp32 (k = 0), a second one for a bf16 store (k = 1)

Definitions the kernels leave open are stated here.  A weight-norm row of norm zero divides by zero: it is NOT a case (row
norms are kept in [0.5, 8] by construction).  rows = 0 in tell_colsum writes out = accumulate ? out : 0.  A dot-attention row
whose keys are all masked is softmax of all -inf: its probs, ctx, dx and dsrc are NaN, and every other row stays in bound.

Measured on the MI355X: MEASURED and C below, and DESIGN.md section 35.
"""
import zlib

import numpy as np

from decode_ref import EPS, TINY, U_OUT, _pin, _sum, bf16_round

SENTINEL = -65536.0

# largest observed (|got - ref| - u_out |ref|) / (gamma 2^-24 S) over the GPU grids of tests/test_gpu_small_reduce.py and (GLU)
# tests/test_gpu_small_pointwise.py on the MI355X, and the pinned constant: four times that, rounded up to a power of two;
# 2^-10 where the ratio never left u_out |ref| (ratio <= 0).  An output group missing from MEASURED is not pinned: its GPU
# test then fails with the measured ratio in its message.
MEASURED = {'wn_norms': 0.047750, 'wn_scale': 0.025289, 'wn_w': 0.136797, 'wn_dg': 0.059213, 'wn_dv': 0.056931,
            'mix_out': 0.034358, 'mix_partial': 0.026410, 'mix_gw': 0.004517, 'colsum': 0.022603, 'colsum_multi': 0.097729,
            'lstm_gates': 0.465517, 'lstm_c': 0.199346, 'lstm_h': 0.280033, 'lstm_dgates': 0.170002, 'lstm_dc_prev': 0.092065,
            'tanh_y': 0.131533, 'da_probs': 0.073797, 'da_ctx': 0.013677, 'da_dx': 0.007981, 'da_dsrc': 0.026437,
            'glu_y': 0.542520, 'glu_dh': 0.545201}
C = {k: _pin(v) for k, v in MEASURED.items()}
GROUPS = ('wn_norms', 'wn_scale', 'wn_w', 'wn_dg', 'wn_dv', 'mix_out', 'mix_partial', 'mix_gw', 'colsum', 'colsum_multi',
          'lstm_gates', 'lstm_c', 'lstm_h', 'lstm_dgates', 'lstm_dc_prev', 'tanh_y', 'da_probs', 'da_ctx', 'da_dx', 'da_dsrc',
          'glu_y', 'glu_dh')

WN_MUTANTS = ('wn_norm_tail_lanes_dropped', 'wn_reg_path_last_trip_dropped', 'wn_scale_times_norm', 'wn_bwd_k_without_square',
              'wn_bwd_store_accumulates', 'wn_bwd_accumulate_stores', 'wn_multi_store_bit_by_global_index',
              'wn_multi_row_start_off_by_one')
MIX_MUTANTS = ('mix_last_layer_dropped', 'mix_layers_past_32_dropped', 'mix_vec_tail_block_dropped', 'mix_bwd_block_stride_256',
               'mix_wgrad_without_dot', 'mix_wgrad_rows_past_16_dropped', 'mix_wgrad_overwrites')
COLSUM_MUTANTS = ('colsum_last_row_of_chunk_dropped', 'colsum_m_dev_ignored', 'colsum_scale_twice', 'colsum_accumulate_ignored',
                  'colsum_multi_remainder_rows_dropped', 'colsum_multi_w0_off_by_one', 'colsum_multi_job_48_lost')
TR_MUTANTS = ('tr_row_scale_by_column', 'tr_plain_unscaled', 'trm_tail_columns_zero', 'trm_tail_rows_dropped')
LSTM_MUTANTS = ('lstm_gate_order_ifog_as_igfo', 'lstm_dc_ignored', 'lstm_tanh_of_c_prev', 'lstm_dgate_o_uses_dcn')
DA_MUTANTS = ('da_mask_l_major', 'da_probs_b_major', 'da_wave3_keys_dropped', 'da_keys_past_256_dropped',
              'da_dx_without_softmax_centering', 'da_dsrc_without_score_term', 'da_stride_swapped')
PW2_MUTANTS = ('dropout_add_index_by_chunk', 'pos_wave_offset_dropped', 'pos_pad_counts', 'mask_rows_second_trip_dropped',
               'glu_gate_first')
PW_MUTANTS = ('sc_tail_dropped', 'gather_count_ignored', 'gather_cap_ignored', 'scatter_overwrites', 'nan_inf_counts',
              'nan_only_first_64_columns', 'sum_n_last_input_dropped', 'relu_bwd_by_dy_sign', 'cast_trips_past_cap_dropped')
MUTANTS = WN_MUTANTS + MIX_MUTANTS + COLSUM_MUTANTS + TR_MUTANTS + LSTM_MUTANTS + DA_MUTANTS + PW_MUTANTS + PW2_MUTANTS


class Out:
    """one output of a launch.  group: a key of C (measured constant), None with k (derived bound, see the docstring) or
    'exact' (bit for bit in the storage type).  exact_at: elements that must equal `value` bit for bit whatever the group
    (rows a kernel must leave alone)."""

    def __init__(self, value, S=None, gam=0.0, dtype='float32', group='exact', k=0.0, exact_at=None):
        self.value, self.S, self.gam, self.dtype, self.group, self.k, self.exact_at = value, S, gam, dtype, group, k, exact_at


def store(a, dtype):
    """a value as the storage type holds it (fp32 array): one rounding, ties to even"""
    a32 = np.asarray(a, np.float64).astype(np.float32)
    return bf16_round(a32) if dtype == 'bfloat16' else a32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def ratio(got, o):
    """largest (|got - ref| - u_out |ref|) / (gamma 2^-24 S) over the elements with S > 0"""
    got, ref, S = np.asarray(got, np.float64), np.asarray(o.value, np.float64), np.asarray(o.S, np.float64)
    S = np.broadcast_to(S, ref.shape)
    ok = np.isfinite(ref) & (o.gam * EPS * S > 0)
    if o.exact_at is not None:
        ok &= ~o.exact_at
    if not ok.any():
        return 0.0
    num = np.abs(got - ref)[ok] - U_OUT[o.dtype] * np.abs(ref[ok]) - TINY * (1.0 + S[ok])
    num = np.where(np.isfinite(num), num, np.inf)
    return float((num / (o.gam * EPS * S[ok])).max())


def failures(got, o, c=None):
    """number of elements of `got` (what a kernel, the emulation or a mutant stored) outside what `o` allows"""
    got = np.asarray(got)
    if o.group == 'exact':
        g, r = np.asarray(got, np.float32), np.asarray(o.value, np.float32)
        return int((~((g.view(np.uint32) == r.view(np.uint32)) | (np.isnan(g) & np.isnan(r)))).sum())
    g, ref = np.asarray(got, np.float64), np.asarray(o.value, np.float64)
    S = np.broadcast_to(np.asarray(o.S, np.float64), ref.shape)
    if o.group is None:
        b = U_OUT[o.dtype] * np.abs(ref) + o.k * EPS * S + TINY * (1.0 + S)
    else:
        b = U_OUT[o.dtype] * np.abs(ref) + (C[o.group] if c is None else c) * o.gam * EPS * S + TINY * (1.0 + S)
    bad = ~(np.abs(g - ref) <= b)                       # (a NaN where the reference is finite is a failure)
    bad &= ~(np.isnan(g) & np.isnan(ref))
    if o.exact_at is not None:
        g32, r32 = np.asarray(got, np.float32), np.asarray(o.value, np.float32)
        bad = np.where(o.exact_at, g32.view(np.uint32) != r32.view(np.uint32), bad)
    return int(bad.sum())


# ---------------------------------------------------------------- fp32 emulation of the kernels' summation orders
def wave_fold(v, dt):
    """wave_sum of common.h: six xor-butterfly steps over [..., 64]"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., idx ^ o]).astype(dt)
    return v[..., 0]


def lane_sum(t, dt, group=1):
    """one wave's sum of the terms t [..., n]: lane l takes `group` consecutive terms per trip (added left to right), trip
    after trip, then the butterfly"""
    t = np.asarray(t, dt)
    if dt is np.float64:
        return t.sum(-1)
    n, per = t.shape[-1], 64 * group
    trips = max(-(-n // per), 1)
    p = np.zeros(t.shape[:-1] + (trips * per,), dt)
    p[..., :n] = t
    p = p.reshape(t.shape[:-1] + (trips, 64, group))
    acc = np.zeros(t.shape[:-1] + (64,), dt)
    for k in range(trips):
        g = p[..., k, :, 0]
        for q in range(1, group):
            g = (g + p[..., k, :, q]).astype(dt)
        acc = (acc + g).astype(dt)
    return wave_fold(acc, dt)


def block_sum(t, dt, group=1):
    """a 256-thread block's sum of t [..., n] (n: the block's own terms in trip-major order, `group` per thread and trip,
    added one by one into the thread's accumulator): four waves folded, then ((w0 + w1) + w2) + w3"""
    t = np.asarray(t, dt)
    if dt is np.float64:
        return t.sum(-1)
    n, per = t.shape[-1], 256 * group
    trips = max(-(-n // per), 1)
    p = np.zeros(t.shape[:-1] + (trips * per,), dt)
    p[..., :n] = t
    p = p.reshape(t.shape[:-1] + (trips, 4, 64, group))
    acc = np.zeros(t.shape[:-1] + (4, 64), dt)
    for k in range(trips):
        for q in range(group):
            acc = (acc + p[..., k, :, :, q]).astype(dt)
    w = wave_fold(acc, dt)
    return (((w[..., 0] + w[..., 1]).astype(dt) + w[..., 2]).astype(dt) + w[..., 3]).astype(dt)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ================================================================ weight norm
def wn_path(cols, aligned=True):
    """the branch wn_weight_row / wn_backward_row take (forward: the entry point refuses unaligned buffers)"""
    if cols % 4 == 0 and aligned:
        return 'reg' if cols % 256 == 0 and cols <= 4096 else 'vec4'
    return 'scalar'


def wn_gamma(cols, extra):
    return -(-cols // 64) + 6 + extra


def wn_forward(g, v, out, dt=np.float64, mutant=None):
    """g [rows], v [rows, cols] (fp32 values) -> norms, scale (tell_wn_rowscale), w (tell_wn_weight, stored as `out`)"""
    g, v = np.asarray(g, dt), np.asarray(v, dt)
    rows, cols = v.shape
    path = wn_path(cols)
    sq = (v * v).astype(dt)
    if mutant == 'wn_norm_tail_lanes_dropped':
        sq = sq[:, :cols // 64 * 64]
    if mutant == 'wn_reg_path_last_trip_dropped' and path == 'reg':
        sq = sq[:, :cols - 256]
    with np.errstate(all='ignore'):
        ss = lane_sum(sq, dt, 1 if path == 'scalar' else 4) if sq.shape[1] else np.zeros(rows, dt)
        nrm = np.sqrt(ss).astype(dt)
        sc = (g * nrm).astype(dt) if mutant == 'wn_scale_times_norm' else (g / nrm).astype(dt)
        w = (v * sc[:, None]).astype(dt)
    gam = wn_gamma(cols, 4)
    return dict(norms=Out(nrm, np.abs(nrm), gam, 'float32', 'wn_norms'), scale=Out(sc, np.abs(sc), gam, 'float32', 'wn_scale'),
                w=Out(w, np.abs(w), gam, out, 'wn_w'))


def wn_backward(dW, g, v, norms, dg0, dv0, store_flag, aligned=True, dt=np.float64, mutant=None):
    """dg = (store ? 0 : dg0) + <dW, v> / norm;  dv = (store ? 0 : dv0) + g / norm (dW - v <dW, v> / norm^2); norms: what the
    forward launch stored"""
    dW, g, v, norms, dg0, dv0 = (np.asarray(a, dt) for a in (dW, g, v, norms, dg0, dv0))
    cols = v.shape[1]
    path = wn_path(cols, aligned)
    if mutant == 'wn_bwd_store_accumulates':
        store_flag = 0
    if mutant == 'wn_bwd_accumulate_stores':
        store_flag = 1
    pr = (dW * v).astype(dt)
    dot, S_dot = lane_sum(pr, dt, 1 if path == 'scalar' else 4), np.abs(np.asarray(pr, np.float64)).sum(-1)
    gs = (g / norms).astype(dt)
    k = (dot / norms).astype(dt) if mutant == 'wn_bwd_k_without_square' else (dot / (norms * norms).astype(dt)).astype(dt)
    a_g, a_v = (np.zeros_like(dg0), np.zeros_like(dv0)) if store_flag else (dg0, dv0)
    dg = (a_g + (dot / norms).astype(dt)).astype(dt)
    dv = (a_v + (gs[:, None] * (dW - (v * k[:, None]).astype(dt)).astype(dt)).astype(dt)).astype(dt)
    n64, gs64 = np.asarray(norms, np.float64), np.abs(np.asarray(gs, np.float64))
    S_dg = np.abs(a_g) + S_dot / n64
    S_dv = np.abs(a_v) + gs64[:, None] * (np.abs(dW) + np.abs(v) * (S_dot / n64 ** 2)[:, None])
    return dict(dg=Out(dg, S_dg, wn_gamma(cols, 4), 'float32', 'wn_dg'), dv=Out(dv, S_dv, wn_gamma(cols, 8), 'float32', 'wn_dv'))


# rows, cols, store, off: which of dW / dv sits one element off 16 bytes in the backward (cols % 4 == 0: forces the scalar
# path).  Every case runs with a bf16 and an fp32 working weight.
WN = [
    dict(id='r1_c256', rows=1, cols=256, store=0, off=None, mutants=('wn_reg_path_last_trip_dropped',
         'wn_bwd_accumulate_stores')),
    dict(id='r5_c768', rows=5, cols=768, store=1, off=None, mutants=('wn_reg_path_last_trip_dropped',
         'wn_bwd_store_accumulates')),
    dict(id='r4_c4096', rows=4, cols=4096, store=1, off=None, mutants=('wn_reg_path_last_trip_dropped',
         'wn_bwd_k_without_square')),
    dict(id='r7_c4096_dW_off', rows=7, cols=4096, store=0, off='dW', mutants=('wn_scale_times_norm',)),
    dict(id='r4_c4', rows=4, cols=4, store=0, off=None, mutants=('wn_bwd_k_without_square',)),
    dict(id='r5_c8_dv_off', rows=5, cols=8, store=1, off='dv', mutants=('wn_bwd_store_accumulates',)),
    dict(id='r7_c260', rows=7, cols=260, store=0, off=None, mutants=('wn_norm_tail_lanes_dropped',)),
    dict(id='r1_c4352', rows=1, cols=4352, store=1, off=None, mutants=('wn_scale_times_norm',)),
    dict(id='r7_c1', rows=7, cols=1, store=0, off=None, mutants=('wn_norm_tail_lanes_dropped',)),
    dict(id='r5_c63', rows=5, cols=63, store=1, off=None, mutants=('wn_norm_tail_lanes_dropped',)),
    dict(id='r4_c65', rows=4, cols=65, store=0, off=None, mutants=('wn_norm_tail_lanes_dropped', 'wn_bwd_accumulate_stores')),
    dict(id='r1_c130', rows=1, cols=130, store=1, off=None, mutants=('wn_norm_tail_lanes_dropped',)),
    dict(id='r5_c1023', rows=5, cols=1023, store=0, off=None, mutants=('wn_norm_tail_lanes_dropped', 'wn_bwd_k_without_square')),
]


def wn_paths(case):
    al = case['off'] is None
    return {'wn_fwd:' + wn_path(case['cols']), 'wn_bwd:' + wn_path(case['cols'], al) + ('' if al else ':misaligned'),
            'wn_rows%%4=%d' % (case['rows'] % 4), 'wn_bwd:store' if case['store'] else 'wn_bwd:accumulate'}


def wn_inputs(case):
    """fp32 g, v (row norms in [0.5, 8]), dW, dg0, dv0"""
    def make():
        r, rows, cols = _rng('wn', case['id']), case['rows'], case['cols']
        v = r.standard_normal((rows, cols))
        v *= (r.uniform(0.5, 8.0, rows) / np.sqrt((v * v).sum(1)))[:, None]
        f = lambda a: np.asarray(a, np.float32)                                                # noqa: E731
        return dict(g=f(r.standard_normal(rows)), v=f(v), dW=f(r.standard_normal((rows, cols))), dg0=f(r.standard_normal(rows)),
                    dv0=f(r.standard_normal((rows, cols))))
    return cached(('wn_in', case['id']), make)


def wn_case(case, out, dt=np.float64, mutant=None, norms=None):
    """forward and backward of one case -> dict of Out; norms: the stored norms the backward reads (default: this forward's,
    rounded to fp32)"""
    x = wn_inputs(case)
    res = wn_forward(x['g'], x['v'], out, dt, mutant)
    if norms is None:
        norms = wn_forward(x['g'], x['v'], out, dt)['norms'].value.astype(np.float32)
    res.update(wn_backward(x['dW'], x['g'], x['v'], norms, x['dg0'], x['dv0'], case['store'], case['off'] is None, dt, mutant))
    return res


# multi-tensor launches: 36 tensors cycling the shapes of WN (all aligned), so a second launch of 4 is made; `store` sets differ
# between a tensor's global index and its index in the second launch
WN_MULTI_N = 36
WN_MULTI_STORE = {'late': (0, 5, 33, 35), 'early': (0, 5, 1, 3)}


def wn_multi_case(j):
    c = dict(WN[j % len(WN)])
    c.update(id='multi%d_%s' % (j, c['id']), off=None)
    return c


def wn_multi(pattern, out, dt=np.float64, mutant=None, norms=None):
    """-> [dict of Out per tensor] of tell_wn_weight_multi + tell_wn_backward_multi2 with store pattern `pattern`"""
    res = []
    for j in range(WN_MULTI_N):
        c = wn_multi_case(j)
        flag = j in WN_MULTI_STORE[pattern]
        if mutant == 'wn_multi_store_bit_by_global_index' and j >= 32:
            # the second launch's mask and the host's `store` array indexed one by j, the other by j - 32 (a 32-bit shift by
            # j wraps to j - 32 on the device, so either way round tensor j takes the flag of tensor j - 32)
            flag = (j - 32) in WN_MULTI_STORE[pattern]
        c['store'] = int(flag)
        r = wn_case(c, out, dt, None, None if norms is None else norms[j])
        if mutant == 'wn_multi_row_start_off_by_one' and j % 32:
            # the first row of every tensor but a launch's first is taken for one more row of its neighbour, so nothing writes
            # it: the fresh outputs keep the buffer's sentinel, the accumulated ones what they held
            x = wn_inputs(c)
            for k, keep in (('norms', SENTINEL), ('w', SENTINEL), ('dg', x['dg0'][0]), ('dv', x['dv0'][0])):
                r[k].value = np.array(r[k].value, copy=True)
                r[k].value[0] = keep
        res.append(r)
    return res


# ================================================================ RoBERTa layer mix
def mix_path(L, n, dtype, aligned=True):
    return 'vec' if L <= 32 and n % 8 == 0 and aligned and dtype == 'bfloat16' else 'scalar'


def softmax_w(w, dt):
    """-> sm, spread (max |w - lse|)"""
    w = np.asarray(w, dt)
    m = w.max()
    e = np.exp((w - m).astype(dt)).astype(dt)
    s = lane_sum(e, dt)
    lse = float(m) + np.log(float(np.asarray(e, np.float64).sum()))
    return (e / s).astype(dt), float(np.abs(np.asarray(w, np.float64) - lse).max())


def mix_fwd(H, w, dtype, aligned=True, dt=np.float64, mutant=None):
    """H [L, n], w [L] -> out [n] = sum_l softmax(w)[l] H[l]"""
    H = np.asarray(H, dt)
    L, n = H.shape
    sm, spread = softmax_w(w, dt)
    lim = L
    if mutant == 'mix_last_layer_dropped':
        lim = L - 1
    if mutant == 'mix_layers_past_32_dropped':
        lim = min(L, 32)
    acc = np.zeros(n, dt)
    for l in range(lim):
        acc = (acc + (sm[l] * H[l]).astype(dt)).astype(dt)
    if mutant == 'mix_vec_tail_block_dropped' and mix_path(L, n, dtype, aligned) == 'vec':
        acc[(n // 8) // 256 * 256 * 8:] = SENTINEL                 # (never written: the buffer's sentinel stays)
    S = (np.asarray(sm, np.float64)[:, None] * np.abs(np.asarray(H, np.float64))).sum(0)
    return dict(out=Out(acc, S, L + 16 + spread, dtype, 'mix_out'))


def mix_bwd(H, dout, nb, dtype, aligned=True, dt=np.float64, mutant=None):
    """partial [nb, L]: block b sums dout[i] H[l][i] over its elements - blocks of 256 elements (scalar) or of 256 chunks of 8
    (vector) taken round robin"""
    H, dout = np.asarray(H, dt), np.asarray(dout, dt)
    L, n = H.shape
    grp = 8 if mix_path(L, n, dtype, aligned) == 'vec' else 1
    unit = 256 * grp
    nblk = -(-n // unit)
    part, S = np.zeros((nb, L), dt), np.zeros((nb, L))
    T = 1
    for b in range(nb):
        mine = range(b, nblk, 1 if mutant == 'mix_bwd_block_stride_256' else nb)
        T = max(T, len(mine))
        idx = np.concatenate([np.arange(k * unit, min((k + 1) * unit, n)) for k in mine] + [np.zeros(0, np.int64)])
        idx = idx.astype(np.int64)
        # (every block of a thread's walk but the last is whole, so trip-major order is the concatenation)
        t = (dout[idx][None, :] * H[:, idx]).astype(dt)
        part[b] = block_sum(t, dt, grp) if idx.size else 0
        S[b] = np.abs(np.asarray(t, np.float64)).sum(-1)
    return dict(partial=Out(part, S, T * grp + 6 + 3, 'float32', 'mix_partial'))


def mix_wgrad(partial, w, gw0, dt=np.float64, mutant=None):
    """gw = gw0 + sm (d - <sm, d>), d = the column sums of partial [n_blocks, L]"""
    partial, gw0 = np.asarray(partial, dt), np.asarray(gw0, dt)
    nb, L = partial.shape
    p = partial[:16] if mutant == 'mix_wgrad_rows_past_16_dropped' else partial
    if dt is np.float64:
        d = p.sum(0)
    else:
        grp = np.stack([_sum(p[g::16], 0, dt) for g in range(16)])
        d = _sum(grp, 0, dt)
    sm, spread = softmax_w(w, dt)
    dot = _sum((sm * d).astype(dt), 0, dt)
    if mutant == 'mix_wgrad_without_dot':
        dot = dt(0)
    upd = (sm * (d - dot).astype(dt)).astype(dt)
    gw = upd if mutant == 'mix_wgrad_overwrites' else (gw0 + upd).astype(dt)
    S_d, sm64 = np.abs(np.asarray(partial, np.float64)).sum(0), np.asarray(sm, np.float64)
    S = np.abs(gw0) + sm64 * (S_d + (sm64 * S_d).sum())
    return dict(gw=Out(gw, S, -(-nb // 16) + 16 + L + 16 + spread, 'float32', 'mix_gw'))


MIX_BIG = 5 * 2048 + 8 * 37
# L, n, kind (bf16 | bf16_off: H one element off 16 bytes | f32), logits (equal | spread | random); every case runs forward,
# backward with n_blocks 1, 3 and 7, and bw_wgs 0 and 13
MIX = [
    dict(id='L1_n1', L=1, n=1, kind='bf16', logits='equal', mutants=('mix_last_layer_dropped',)),
    dict(id='L3_n7_f32', L=3, n=7, kind='f32', logits='random', mutants=('mix_last_layer_dropped',)),
    dict(id='L25_n8', L=25, n=8, kind='bf16', logits='random', mutants=('mix_last_layer_dropped',)),
    dict(id='L32_n2047', L=32, n=2047, kind='bf16', logits='spread', mutants=('mix_bwd_block_stride_256',)),
    dict(id='L32_n2048', L=32, n=2048, kind='bf16', logits='equal', mutants=('mix_last_layer_dropped',)),
    dict(id='L25_big', L=25, n=MIX_BIG, kind='bf16', logits='random', mutants=('mix_vec_tail_block_dropped',
         'mix_bwd_block_stride_256')),
    dict(id='L25_big_off', L=25, n=MIX_BIG, kind='bf16_off', logits='spread', mutants=('mix_bwd_block_stride_256',)),
    dict(id='L33_n2048', L=33, n=2048, kind='bf16', logits='random', mutants=('mix_layers_past_32_dropped',)),
    dict(id='L64_big_f32', L=64, n=MIX_BIG, kind='f32', logits='random', mutants=('mix_layers_past_32_dropped',
         'mix_bwd_block_stride_256')),
    dict(id='L64_n8', L=64, n=8, kind='bf16', logits='spread', mutants=('mix_layers_past_32_dropped',)),
]
MIX_BLOCKS = (1, 3, 7)
# tell_mix_wgrad on the partials of tell_mix_bwd of case L25_big_off (the scalar path: 42 blocks of 256 elements, so each of
# the 40 partial rows holds a sum), gw prefilled
MIX_WGRAD_BLOCKS = (1, 16, 17, 40)
MIX_WGRAD = [dict(id='wgrad_nb%d' % nb, nb=nb, mutants=m) for nb, m in zip(MIX_WGRAD_BLOCKS, (
    ('mix_wgrad_without_dot',), ('mix_wgrad_overwrites',), ('mix_wgrad_rows_past_16_dropped',),
    ('mix_wgrad_rows_past_16_dropped',)))]


def mix_wgrad_source():
    return next(c for c in MIX if c['id'] == 'L25_big_off')


def mix_dtype(case):
    return 'float32' if case['kind'] == 'f32' else 'bfloat16'


def mix_paths(case):
    L, n, dty, al = case['L'], case['n'], mix_dtype(case), case['kind'] != 'bf16_off'
    p = mix_path(L, n, dty, al)
    why = 'L>32' if L > 32 else ('float32' if dty == 'float32' else ('n%8' if n % 8 else ('misaligned' if not al else dty)))
    unit = 2048 if p == 'vec' else 256
    return {'mix:%s:%s' % (p, why), 'mix:logits:' + case['logits'], 'mix:blocks>work' if -(-n // unit) < 7 else 'mix:several_trips',
            'mix:ragged_tail' if n % unit else 'mix:whole_blocks'}


def mix_inputs(case):
    def make():
        r, L, n, dty = _rng('mix', case['id']), case['L'], case['n'], mix_dtype(case)
        w = {'equal': np.full(L, 0.25), 'spread': np.linspace(-30.0, 30.0, L) if L > 1 else np.zeros(1),
             'random': r.standard_normal(L)}[case['logits']]
        return dict(H=store(r.standard_normal((L, n)), dty), dout=store(r.standard_normal(n), dty), w=np.asarray(w, np.float32),
                    gw0=np.asarray(r.standard_normal(L), np.float32))
    return cached(('mix_in', case['id']), make)


def mix_case(case, nb, dt=np.float64, mutant=None):
    x, dty, al = mix_inputs(case), mix_dtype(case), case['kind'] != 'bf16_off'
    res = mix_fwd(x['H'], x['w'], dty, al, dt, mutant)
    res.update(mix_bwd(x['H'], x['dout'], nb, dty, al, dt, mutant))
    return res


# ================================================================ column sums
def colsum_chunks(rows):
    return min(max((rows + 127) // 128, 1), 128)


def colsum(x, rows, out0, accumulate, scale, m_dev, dtype, dt=np.float64, mutant=None):
    """x [rows, C] -> out [C] = (accumulate ? out0 : 0) + scale sum_{r < min(rows, m_dev)} x[r]"""
    x, out0 = np.asarray(x, dt), np.asarray(out0, dt)
    C = x.shape[1]
    nch = colsum_chunks(rows)
    rpc = (rows + nch - 1) // nch
    live = rows if m_dev is None or mutant == 'colsum_m_dev_ignored' else min(rows, m_dev)
    tot = np.zeros(C, dt)
    for k in range(nch):
        r0, r1 = k * rpc, min(k * rpc + rpc, live)
        if mutant == 'colsum_last_row_of_chunk_dropped':
            r1 -= 1
        if dt is np.float64:
            t = x[r0:max(r1, r0)].sum(0)
        else:
            p = [_sum(x[r0 + ry:max(r1, r0 + ry):4], 0, dt) for ry in range(4)]
            t = (((p[0] + p[1]).astype(dt) + p[2]).astype(dt) + p[3]).astype(dt)
        tot = (tot + t).astype(dt)
    sc = dt(np.float32(scale))
    t = (tot * sc).astype(dt)
    if mutant == 'colsum_scale_twice':
        t = (t * sc).astype(dt)
    acc = accumulate and mutant != 'colsum_accumulate_ignored'
    out = (out0 + t).astype(dt) if acc else t
    S = abs(float(np.float32(scale))) * np.abs(np.asarray(x[:min(rows, live)], np.float64)).sum(0)
    if accumulate:
        S = S + np.abs(out0)
    return dict(out=Out(out, S, -(-rpc // 4) + 3 + nch + 2, 'float32', 'colsum'))


# rows, C, pad (ld = C + pad), acc, scale, m (None: null m_dev | int: the device row count), dtype of x
COLSUM = [
    dict(id='rows0', rows=0, C=63, pad=0, acc=1, scale=1.0, m=None, dtype='float32', mutants=('colsum_accumulate_ignored',)),
    dict(id='rows0_store', rows=0, C=1, pad=5, acc=0, scale=0.37, m=None, dtype='bfloat16', mutants=()),
    dict(id='rows1', rows=1, C=1, pad=0, acc=0, scale=0.37, m=None, dtype='bfloat16', mutants=('colsum_scale_twice',)),
    dict(id='rows3_m0', rows=3, C=64, pad=5, acc=1, scale=1.0, m=0, dtype='float32', mutants=('colsum_m_dev_ignored',)),
    dict(id='rows127', rows=127, C=65, pad=0, acc=0, scale=1.0, m=None, dtype='bfloat16',
         mutants=('colsum_last_row_of_chunk_dropped',)),
    dict(id='rows128_m_above', rows=128, C=200, pad=5, acc=1, scale=0.37, m=500, dtype='float32',
         mutants=('colsum_accumulate_ignored', 'colsum_scale_twice')),
    dict(id='rows129_m_inside', rows=129, C=63, pad=5, acc=0, scale=1.0, m=70, dtype='float32',
         mutants=('colsum_m_dev_ignored',)),
    dict(id='rows1000_m_edge', rows=1000, C=65, pad=0, acc=1, scale=0.37, m=375, dtype='bfloat16',
         mutants=('colsum_m_dev_ignored', 'colsum_scale_twice')),
    dict(id='rows1000', rows=1000, C=64, pad=5, acc=0, scale=1.0, m=None, dtype='float32',
         mutants=('colsum_last_row_of_chunk_dropped',)),
    dict(id='rows16462', rows=16385 + 77, C=200, pad=0, acc=1, scale=1.0, m=None, dtype='float32',
         mutants=('colsum_last_row_of_chunk_dropped', 'colsum_accumulate_ignored')),
    dict(id='rows16462_bf16_m', rows=16385 + 77, C=1, pad=5, acc=0, scale=0.37, m=16000, dtype='bfloat16',
         mutants=('colsum_m_dev_ignored',)),
]


def colsum_paths(case):
    rows, m = case['rows'], case['m']
    nch = colsum_chunks(rows)
    rpc = (rows + nch - 1) // nch
    mk = 'null' if m is None else ('zero' if m == 0 else ('above' if m >= rows else ('edge' if m % rpc == 0 else 'inside')))
    return {'colsum:direct' if nch == 1 else ('colsum:finish:128x%d' % rpc if nch == 128 else 'colsum:finish'),
            'colsum:m_dev:' + mk, 'colsum:' + case['dtype'], 'colsum:acc%d' % case['acc'],
            'colsum:rows0' if rows == 0 else 'colsum:C%%64=%d' % (case['C'] % 64), 'colsum:ld>C' if case['pad'] else 'colsum:ld=C'}


def colsum_inputs(case):
    def make():
        r = _rng('colsum', case['id'])
        return dict(x=store(r.standard_normal((case['rows'], case['C'])), case['dtype']),
                    out0=np.asarray(r.standard_normal(case['C']), np.float32))
    return cached(('colsum_in', case['id']), make)


def colsum_case(case, dt=np.float64, mutant=None):
    x = colsum_inputs(case)
    return colsum(x['x'], case['rows'], x['out0'], case['acc'], case['scale'], case['m'], case['dtype'], dt, mutant)


# tell_colsum_multi: 50 jobs (a second launch of 2); job j has rows, width and the w0 kind of the cycles below
CSM_N = 50
CSM_ROWS = (1, 15, 16, 17, 48, 49, 64, 65, 113, 200)
CSM_WIDTH = (1, 64, 65, 130)
CSM_W0 = ('zero', 'width', 'mid')
CSM_MUTANTS = ('colsum_multi_remainder_rows_dropped', 'colsum_multi_w0_off_by_one', 'colsum_multi_job_48_lost')


def csm_job(j):
    rows, width = CSM_ROWS[j % 10], CSM_WIDTH[(j // 2) % 4]
    kind = CSM_W0[(j // 3) % 3]
    w0 = {'zero': 0, 'width': width, 'mid': (width * 37) // 64 if width > 1 else 0}[kind]
    return dict(rows=rows, width=width, w0=w0, ld=width + 3 + j % 5)


def csm_paths():
    p = set()
    for j in range(CSM_N):
        job = csm_job(j)
        w0 = 'zero' if job['w0'] == 0 else ('width' if job['w0'] == job['width'] else 'mid%%64=%d' % min(job['w0'] % 64, 1))
        rows, width = job['rows'], job['width']
        # the walk of row group `by` (rows by, by + 16, ...): 4-way unrolled rounds while r + 48 < rows, then the remainder
        walk = 'unrolled' if rows % 64 == 0 else ('unrolled_for_some' if rows < 64 else 'unrolled+remainder')
        walk = 'groups_empty' if rows < 16 else ('remainder_only' if rows <= 48 else walk)
        p |= {'csm:walk:' + walk, 'csm:cols:' + ('partial' if width < 64 else ('whole' if width % 64 == 0 else 'ragged')),
              'csm:launch%d' % (j // 48), 'csm:w0:' + w0}
    return p


def csm_inputs():
    def make():
        r = _rng('csm')
        return [dict(x=np.asarray(r.standard_normal((csm_job(j)['rows'], csm_job(j)['width'])), np.float32),
                     d0=np.asarray(r.standard_normal(csm_job(j)['width']), np.float32)) for j in range(CSM_N)]
    return cached('csm_in', make)


def colsum_multi(dt=np.float64, mutant=None):
    """-> [Out per job]: dst [width] = d0 + column sums (the test splits it into dst0 = [:w0] and dst1 = [w0:])"""
    res = []
    for j, x in enumerate(csm_inputs()):
        job, xs, d0 = csm_job(j), np.asarray(x['x'], dt), np.asarray(x['d0'], dt)
        rows = job['rows']
        use = np.ones(rows, bool)
        if mutant == 'colsum_multi_remainder_rows_dropped':
            use[:] = False
            for by in range(16):
                r = by
                while r + 48 < rows:
                    use[[r, r + 16, r + 32, r + 48]] = True
                    r += 64
        if dt is np.float64:
            s = xs[use].sum(0)
        else:
            grp = []
            for by in range(16):
                a, r = [np.zeros(job['width'], dt) for _ in range(4)], by
                while r + 48 < rows:
                    for q in range(4):
                        a[q] = (a[q] + xs[r + 16 * q]).astype(dt)
                    r += 64
                while r < rows:
                    a[0] = (a[0] + xs[r]).astype(dt)
                    r += 16
                grp.append(((a[0] + a[1]).astype(dt) + (a[2] + a[3]).astype(dt)).astype(dt))
            s = _sum(np.stack(grp), 0, dt)
        out = (d0 + s).astype(dt)
        if mutant == 'colsum_multi_job_48_lost' and j == 48:
            out = d0.copy()
        if mutant == 'colsum_multi_w0_off_by_one' and 0 < job['w0'] < job['width']:
            out[job['w0']] = d0[job['w0']]                  # (the sum went to dst0[w0], past dst0's end)
        S = np.abs(d0) + np.abs(np.asarray(xs, np.float64)).sum(0)
        res.append(Out(out, S, -(-rows // 64) + 3 + 16 + 1, 'float32', 'colsum_multi'))
    return res


# ================================================================ transposes (exact)
def transpose(src, row_scale, dst_dtype, mutant=None):
    """-> t [cols, rows], plain [rows, cols]: src * row_scale[r] (one fp32 product), stored as dst_dtype"""
    src = np.asarray(src, np.float32)
    rows, cols = src.shape
    v = src
    if row_scale is not None:
        sc = np.asarray(row_scale, np.float32)
        v = src * (sc[np.arange(cols) % rows][None, :] if mutant == 'tr_row_scale_by_column' else sc[:, None])
    v = store(v, dst_dtype)
    plain = store(src, dst_dtype) if mutant == 'tr_plain_unscaled' else v
    return dict(t=Out(np.ascontiguousarray(v.T), dtype=dst_dtype), plain=Out(plain, dtype=dst_dtype))


# rows, cols, (src, dst) types, scaled, outputs; every leading dimension is padded
TR = [
    dict(id='1x1', rows=1, cols=1, types=('float32', 'bfloat16'), scaled=True, outs='both', mutants=('tr_plain_unscaled',)),
    dict(id='63x65', rows=63, cols=65, types=('float32', 'float32'), scaled=True, outs='t', mutants=('tr_row_scale_by_column',)),
    dict(id='64x64', rows=64, cols=64, types=('bfloat16', 'bfloat16'), scaled=False, outs='plain', mutants=()),
    dict(id='70x130', rows=70, cols=130, types=('bfloat16', 'float32'), scaled=True, outs='both',
         mutants=('tr_row_scale_by_column', 'tr_plain_unscaled')),
    dict(id='129x3', rows=129, cols=3, types=('float32', 'bfloat16'), scaled=True, outs='t', mutants=('tr_row_scale_by_column',)),
    dict(id='129x3_scaled', rows=129, cols=3, types=('bfloat16', 'bfloat16'), scaled=True, outs='plain',
         mutants=('tr_plain_unscaled',)),
]


def tr_paths(case):
    edge = lambda v: 'one_ragged' if v < 64 else ('whole' if v % 64 == 0 else 'several_ragged')       # noqa: E731
    return {'tr:%s->%s' % case['types'], 'tr:scaled' if case['scaled'] else 'tr:unscaled', 'tr:outs:' + case['outs'],
            'tr:row_tiles:' + edge(case['rows']), 'tr:col_tiles:' + edge(case['cols'])}


def tr_inputs(case):
    def make():
        r = _rng('tr', case['id'])
        return dict(src=store(r.standard_normal((case['rows'], case['cols'])), case['types'][0]),
                    scale=np.asarray(r.uniform(0.5, 2.0, case['rows']), np.float32) if case['scaled'] else None)
    return cached(('tr_in', case['id']), make)


def tr_case(case, mutant=None):
    x = tr_inputs(case)
    r = transpose(x['src'], x['scale'], case['types'][1], mutant)
    return {k: o for k, o in r.items() if case['outs'] in ('both', k)}


TRM_N = 50
TRM_SHAPES = ((1, 1), (8, 8), (64, 64), (70, 130), (3, 200), (65, 7), (129, 66))


def trm_inputs():
    def make():
        r = _rng('trm')
        return [store(r.standard_normal(TRM_SHAPES[j % 7]), 'bfloat16') for j in range(TRM_N)]
    return cached('trm_in', make)


def transpose_multi(mutant=None):
    """-> [Out per job]: dst [cols, rows] bf16; an unwritten element keeps SENTINEL"""
    res = []
    for x in trm_inputs():
        rows, cols = x.shape
        d = np.ascontiguousarray(x.T)
        if mutant == 'trm_tail_columns_zero' and cols % 8:
            d[cols // 8 * 8:] = 0
        if mutant == 'trm_tail_rows_dropped' and rows % 8:
            d[:, rows // 8 * 8:] = SENTINEL
        res.append(Out(d, dtype='bfloat16'))
    return res


def trm_paths():
    p = set()
    for j in range(TRM_N):
        rows, cols = TRM_SHAPES[j % 7]
        p |= {'trm:launch%d' % (j // 48), 'trm:load:' + ('vec' if cols >= 8 else 'none') + ('+tail' if cols % 8 else ''),
              'trm:store:' + ('vec' if rows >= 8 else 'none') + ('+tail' if rows % 8 else ''),
                   'trm:tiles%d' % (-(-rows // 64) * -(-cols // 64))}
    return p


# ================================================================ movers and pointwise kernels
def stream_launch(op, dtype):
    """(share, cap) of a streaming launcher: the grid is min(ceil(n / share), cap) blocks of 256 threads, so the clamp is taken -
    and a thread makes more trips than share / 256 - only when n > share cap.  cast, axpy, relu_bwd, dropout: grid_for(n,
    256 * 4); GLU: grid_for(rows C, 256 * 2); sum_n: grid_for(n / vec, 256) over 16-byte chunks; dropout_add: its own cap of
    2048 blocks of 256 chunks"""
    vec = 8 if dtype == 'bfloat16' else 4
    return {'cast': (1024, 4096), 'axpy': (1024, 4096), 'relu_bwd': (1024, 4096), 'dropout': (1024, 4096), 'glu': (512, 4096),
            'sum_n': (256 * vec, 4096), 'dropout_add': (256 * vec, 2048)}[op]


def past_cap(op, dtype, extra):
    """the smallest interesting n that takes the launcher's grid clamp: share cap + extra"""
    share, cap = stream_launch(op, dtype)
    return share * cap + extra


def stream_size(op, dtype, n):
    share, cap = stream_launch(op, dtype)
    return 'grid_capped' if n > share * cap else ('below' if n < share else ('at' if n == share else 'above'))


def cast(x, dst, mutant=None):
    v = store(x, dst)
    if mutant == 'cast_trips_past_cap_dropped':          # every thread stops after its share / 256 trips: right up to the cap
        v[past_cap('cast', dst, 0):] = SENTINEL          # (what was never written keeps the buffer's sentinel)
    return dict(dst=Out(v, dtype=dst))


def scale_cast(x, scale, dst, dt=np.float64, mutant=None):
    x = np.asarray(x, dt)
    v = (x * dt(np.float32(1.0 if scale is None else scale))).astype(dt)
    if mutant == 'sc_tail_dropped':
        v[x.size // 4 * 4:] = SENTINEL
    return dict(dst=Out(v, np.abs(v), dtype=dst, group=None, k=1.0 if dst == 'bfloat16' else 0.0))


def axpy(x, y, alpha, dtype, dt=np.float64, mutant=None):
    """fp32: k = 1 + 2^-23 on S = |alpha x| (the product's rounding; u_out |ref| is the sum's, and the sum is taken of the
    ROUNDED product: a second-order 2^-48 |alpha x|); bf16: k = 2 on S = |y| + |alpha x| (the fp32 sum's own rounding is no
    longer inside u_out |ref|, which the store takes)"""
    x, y = np.asarray(x, dt), np.asarray(y, dt)
    t = (x * dt(np.float32(alpha))).astype(dt)
    S, k = (np.abs(t), 1.0 + 2.0 ** -23) if dtype == 'float32' else (np.abs(y) + np.abs(t), 2.0)
    return dict(y=Out((y + t).astype(dt), S, dtype=dtype, group=None, k=k))


def sum_n(xs, dtype, dt=np.float64, mutant=None):
    xs = [np.asarray(x, dt) for x in xs]
    acc = np.zeros_like(xs[0])
    for x in (xs[:-1] if mutant == 'sum_n_last_input_dropped' else xs):
        acc = (acc + x).astype(dt)
    return dict(out=Out(acc, sum(np.abs(np.asarray(x, np.float64)) for x in xs), dtype=dtype, group=None, k=float(len(xs))))


def relu_bwd(dy, y, dtype, mutant=None):
    dy, y = np.asarray(dy, np.float32), np.asarray(y, np.float32)
    return dict(dx=Out(np.where((dy if mutant == 'relu_bwd_by_dy_sign' else y) > 0, dy, np.float32(0)), dtype=dtype))


def gather_rows(src, idx, count, cap, dtype, mutant=None):
    """dst [PW_ROWS, C]: rows past min(count, cap) keep SENTINEL"""
    n = cap if count is None or mutant == 'gather_count_ignored' else count
    if mutant != 'gather_cap_ignored':
        n = min(n, cap)
    dst = np.full((PW_ROWS, src.shape[1]), SENTINEL, np.float32)
    dst[:n] = np.asarray(src, np.float32)[np.asarray(idx)[:n]]
    return dict(dst=Out(dst, dtype=dtype))


def scatter_add_rows(src, idx, count, cap, dst0, dtype, dt=np.float64, mutant=None):
    """dst[idx[r]] += src[r] for r < min(count, cap); the other rows of dst stay as they were"""
    n = min(cap if count is None else count, cap)
    src, d = np.asarray(src, dt), np.array(dst0, dt)
    touched = np.zeros(d.shape, bool)
    rows = np.asarray(idx)[:n]
    d[rows] = src[:n] if mutant == 'scatter_overwrites' else (d[rows] + src[:n]).astype(dt)
    touched[rows] = True
    S = np.abs(np.asarray(dst0, np.float64))
    S[rows] += np.abs(np.asarray(src[:n], np.float64))
    return dict(dst=Out(d, S, dtype=dtype, group=None, k=1.0 if dtype == 'bfloat16' else 0.0, exact_at=~touched))


def nan_rows(x, dtype, mutant=None):
    x = np.asarray(x, np.float32)
    look = x[:, :64] if mutant == 'nan_only_first_64_columns' else x
    bad = (~np.isfinite(look)).any(1) if mutant == 'nan_inf_counts' else np.isnan(look).any(1)
    with np.errstate(all='ignore'):
        y = store(np.where(bad[:, None], np.float32(0), x), dtype)
    return dict(y=Out(y, dtype=dtype), mask=Out(bad.astype(np.float32)))


# Streaming kernels: n one below, at and above a block's share and just past share x cap of stream_launch(), where the grid is
# clamped and the grid-stride loop makes a trip more than the share holds.  scale_cast: n % 4 = 0 .. 3, null and device scale,
# fp32 (run in place) and bf16 out.  gather / scatter: cap 2100 (past the 2048-block grid), C = 5, padded rows; the buffers
# hold PW_ROWS rows, so a count above the cap has somewhere to go wrong.
PW_ROWS = 2550


def _pw(op, mutants=(), **kw):
    tag = '_'.join('%s' % (v[0] if isinstance(v, str) else v) for v in kw.values())
    return dict(id='%s_%s' % (op, tag), op=op, mutants=tuple(mutants), **kw)


PW = [_pw('cast', ['cast_trips_past_cap_dropped'] if n > 10 ** 6 else [], src=s, dst=d, n=n) for s, d, ns in (
    ('float32', 'bfloat16', (1023, 1024, 1025, past_cap('cast', 'bfloat16', 1000))), ('bfloat16', 'float32', (1023,)),
    ('float32', 'float32', (1024,)),
    ('bfloat16', 'bfloat16', (1025,))) for n in ns]
PW += [_pw('scale_cast', ['sc_tail_dropped'] if n % 4 else [], n=n, dst=d, scale=sc) for n, d, sc in (
    (1024, 'float32', None), (1025, 'bfloat16', 0.37), (2050, 'float32', 0.37), (515, 'bfloat16', None), (3, 'float32', 0.37))]
PW += [_pw('axpy', n=n, dtype=d) for d, ns in (
    ('float32', (1023, 1024, 1025, past_cap('axpy', 'float32', 1000))), ('bfloat16', (1023,))) for n in ns]
PW += [_pw('sum_n', ['sum_n_last_input_dropped'] if k > 1 else [], dtype=d, k=k, n=n) for d, k, n in (
    ('float32', 1, 1020), ('float32', 3, 1024), ('float32', 8, 1028), ('bfloat16', 8, 2040), ('bfloat16', 2, 2048),
    ('float32', 3, past_cap('sum_n', 'float32', 1028)))]
PW += [_pw('relu_bwd', ['relu_bwd_by_dy_sign'], n=n, dtype=d) for d, ns in (
    ('bfloat16', (1023, 1024, 1025, past_cap('relu_bwd', 'bfloat16', 1000))), ('float32', (1023, 1025))) for n in ns]
PW += [_pw('gather', m, dtype=d, count=cnt, cap=2100, C=5) for d, cnt, m in (
    ('float32', None, ()), ('bfloat16', 0, ('gather_count_ignored',)), ('float32', 1500, ('gather_count_ignored',)),
    ('bfloat16', 2500, ('gather_cap_ignored',)))]
PW += [_pw('scatter', ['scatter_overwrites'] if cnt != 0 else [], dtype=d, count=cnt, cap=2100, C=5) for d, cnt in (
    ('float32', None), ('bfloat16', 0), ('float32', 1500), ('bfloat16', 2500))]
PW += [_pw('nan_rows', m, C=Cc, dtype=d) for Cc, d, m in (
    (1, 'float32', ('nan_inf_counts',)), (63, 'bfloat16', ('nan_inf_counts',)), (65, 'float32', ('nan_only_first_64_columns',)),
    (200, 'bfloat16', ('nan_only_first_64_columns', 'nan_inf_counts')))]
NAN_ROWS = 11            # rows of a nan_rows case: three blocks of four waves, the last one ragged


def _mover_paths(case):
    """what the launcher and the kernel of a case decide on: the trip structure, the type, the optional pointers"""
    op = case['op']
    if op in ('cast', 'axpy', 'relu_bwd', 'sum_n'):
        dty = case.get('dtype') or case['dst']
        p = {'%s:%s' % (op, stream_size(op, dty, case['n'])), '%s:%s' % (op, dty)}
        if op == 'cast':
            p.add('cast:%s->%s' % (case['src'], case['dst']))
        if op == 'sum_n':
            p.add('sum_n:inputs%d' % case['k'])
        return p
    if op == 'scale_cast':
        return {'scale_cast:n%%4=%d' % (case['n'] % 4), 'scale_cast:' + case['dst'],
                'scale_cast:scale:' + ('null' if case['scale'] is None else 'device')}
    if op in ('gather', 'scatter'):
        cnt = case['count']
        kind = 'null' if cnt is None else ('zero' if cnt == 0 else ('below' if cnt < case['cap'] else 'above'))
        return {'%s:count:%s' % (op, kind), '%s:%s' % (op, case['dtype'])}
    Cc = case['C']                  # one lane trip over part of a wave, a ragged second trip, several trips
    lanes = 'partial' if Cc < 64 else ('two_trips' if Cc <= 128 else 'several_trips')
    return {'nan_rows:lanes:' + lanes, 'nan_rows:' + case['dtype']}


def _mover_inputs(case):
    def make():
        r, op = _rng('pw', case['id']), case['op']
        f = lambda shape, d: store(r.standard_normal(shape), d)                                # noqa: E731
        if op == 'cast':
            return dict(x=f(case['n'], case['src']))
        if op == 'scale_cast':
            return dict(x=f(case['n'], 'float32'))
        if op == 'axpy':
            return dict(x=f(case['n'], case['dtype']), y=f(case['n'], case['dtype']), alpha=0.37)
        if op == 'sum_n':
            return dict(xs=[f(case['n'], case['dtype']) for _ in range(case['k'])])
        if op == 'relu_bwd':
            y = f(case['n'], case['dtype'])
            y[::7], y[3::7] = 0.0, -0.0                      # +0 and -0 pass no gradient; dy is non-zero there
            return dict(dy=store(f(case['n'], case['dtype']) + np.float32(4.0), case['dtype']), y=y)
        if op in ('gather', 'scatter'):
            Cc, big = case['C'], PW_ROWS + 37
            idx = r.permutation(big)[:PW_ROWS].astype(np.int32)                 # unique
            if op == 'gather':
                return dict(src=f((big, Cc), case['dtype']), idx=idx)
            return dict(src=f((PW_ROWS, Cc), case['dtype']), idx=idx, dst0=f((big, Cc), case['dtype']))
        x = np.asarray(r.standard_normal((NAN_ROWS, case['C'])), np.float32)
        Cc = case['C']
        x[1, 0], x[2, Cc - 1], x[5, Cc // 2] = np.nan, np.nan, np.nan
        x[3, min(64, Cc - 1)] = np.nan                        # seen only by a lane's second trip when C > 64
        x[4, 0], x[8, Cc - 1] = np.inf, -np.inf               # a row holding only inf is not masked
        x[10, Cc - 1] = np.nan
        return dict(x=x)
    return cached(('pw_in', case['id']), make)


def _mover_case(case, dt=np.float64, mutant=None):
    x, op = _mover_inputs(case), case['op']
    if op == 'cast':
        return cast(x['x'], case['dst'], mutant)
    if op == 'scale_cast':
        return scale_cast(x['x'], case['scale'], case['dst'], dt, mutant)
    if op == 'axpy':
        return axpy(x['x'], x['y'], x['alpha'], case['dtype'], dt, mutant)
    if op == 'sum_n':
        return sum_n(x['xs'], case['dtype'], dt, mutant)
    if op == 'relu_bwd':
        return relu_bwd(x['dy'], x['y'], case['dtype'], mutant)
    if op == 'gather':
        return gather_rows(x['src'], x['idx'], case['count'], case['cap'], case['dtype'], mutant)
    if op == 'scatter':
        return scatter_add_rows(x['src'], x['idx'], case['count'], case['cap'], x['dst0'], case['dtype'], dt, mutant)
    return nan_rows(x['x'], case['dtype'], mutant)


# ================================================================ LSTM pieces (csrc/lstm.hip)
def _sig(x, dt):
    return (dt(1) / (dt(1) + np.exp(-x).astype(dt)).astype(dt)).astype(dt)


def lstm_fwd(g1, g2, c_prev, dtype, dt=np.float64, mutant=None):
    """g1, g2 [B, 4H] (chunks i, f, g, o), c_prev [B, H] -> h, c (stored as dtype), gates [B, 4H] fp32 (activated)"""
    g1, g2, c_prev = (np.asarray(a, dt) for a in (g1, g2, c_prev))
    B, H = c_prev.shape
    pre = (g1 + g2).astype(dt).reshape(B, 4, H)
    ki, kf, kg, ko = (0, 2, 1, 3) if mutant == 'lstm_gate_order_ifog_as_igfo' else (0, 1, 2, 3)
    i, f, g, o = _sig(pre[:, ki], dt), _sig(pre[:, kf], dt), np.tanh(pre[:, kg]).astype(dt), _sig(pre[:, ko], dt)
    t1, t2 = (f * c_prev).astype(dt), (i * g).astype(dt)
    cn = (t1 + t2).astype(dt)
    h = (o * np.tanh(cn).astype(dt)).astype(dt)
    gates = np.stack([i, f, g, o], 1).reshape(B, 4 * H)
    gam = 16.0 + float(np.abs(pre).max())
    S_c = np.abs(t1) + np.abs(t2)
    return dict(h=Out(h, np.maximum(np.abs(h), o * S_c), gam, dtype, 'lstm_h'), c=Out(cn, S_c, gam, dtype, 'lstm_c'),
                gates=Out(gates, np.abs(gates), gam, 'float32', 'lstm_gates'))


def lstm_bwd(dh, dc, gates, c, c_prev, dtype, dt=np.float64, mutant=None):
    """dh, dc [B, H] or None; gates: what the forward stored; c: the NEW cell state as stored -> dgates [B, 4H], dc_prev"""
    gates, c, c_prev = (np.asarray(a, dt) for a in (gates, c, c_prev))
    B, H = c.shape
    i, f, g, o = (gates.reshape(B, 4, H)[:, k] for k in range(4))
    tc = np.tanh(c_prev if mutant == 'lstm_tanh_of_c_prev' else c).astype(dt)
    gh = np.zeros((B, H), dt) if dh is None else np.asarray(dh, dt)
    gc = np.zeros((B, H), dt) if dc is None or mutant == 'lstm_dc_ignored' else np.asarray(dc, dt)
    t = ((gh * o).astype(dt) * (1 - (tc * tc).astype(dt)).astype(dt)).astype(dt)
    dcn = (gc + t).astype(dt)
    S_dcn = np.abs(gc) + np.abs(gh * o)
    one = dt(1)
    top = dcn if mutant == 'lstm_dgate_o_uses_dcn' else gh
    dg = [dcn * g * i * (one - i), dcn * c_prev * f * (one - f), dcn * i * (one - (g * g).astype(dt)), top * tc * o * (one - o)]
    S = [S_dcn * np.abs(g) * i * (1 - i), S_dcn * np.abs(c_prev) * f * (1 - f), S_dcn * i * (1 + g * g), np.abs(gh) * o * (1 - o)]
    dgates = np.stack([np.asarray(a, dt) for a in dg], 1).reshape(B, 4 * H)
    return dict(dgates=Out(dgates, np.stack(S, 1).reshape(B, 4 * H), 16.0, dtype, 'lstm_dgates'),
                dc_prev=Out((dcn * f).astype(dt), S_dcn * f, 16.0, dtype, 'lstm_dc_prev'))


# B, H, which of the incoming gradients is a null pointer; every case runs in bf16 and fp32
LSTM = [
    dict(id='B1_H1', B=1, H=1, null=None, mutants=('lstm_gate_order_ifog_as_igfo', 'lstm_tanh_of_c_prev')),
    dict(id='B5_H48_no_dh', B=5, H=48, null='dh', mutants=('lstm_dc_ignored',)),
    dict(id='B3_H257_no_dc', B=3, H=257, null='dc', mutants=('lstm_gate_order_ifog_as_igfo', 'lstm_dgate_o_uses_dcn')),
    dict(id='B3_H257', B=3, H=257, null=None, mutants=('lstm_dc_ignored', 'lstm_dgate_o_uses_dcn', 'lstm_tanh_of_c_prev')),
]


def lstm_paths(case):
    n = case['B'] * case['H']
    return {'lstm:null:%s' % case['null'], 'lstm:' + ('one_block' if n <= 256 else 'ragged_last_block')}


def lstm_inputs(case, dtype):
    def make():
        r, B, H = _rng('lstm', case['id']), case['B'], case['H']
        f = lambda *shape: store(r.standard_normal(shape) * 1.5, dtype)                                  # noqa: E731
        return dict(g1=f(B, 4 * H), g2=f(B, 4 * H), c_prev=f(B, H), dh=f(B, H), dc=f(B, H))
    return cached(('lstm_in', case['id'], dtype), make)


def lstm_case(case, dtype, dt=np.float64, mutant=None, gates=None, c=None):
    """forward and backward; gates, c: what the forward launch stored (default: this forward's, rounded)"""
    x = lstm_inputs(case, dtype)
    res = lstm_fwd(x['g1'], x['g2'], x['c_prev'], dtype, dt, mutant)
    if gates is None:
        base = lstm_fwd(x['g1'], x['g2'], x['c_prev'], dtype, dt)
        gates, c = store(base['gates'].value, 'float32'), store(base['c'].value, dtype)
    res.update(lstm_bwd(None if case['null'] == 'dh' else x['dh'], None if case['null'] == 'dc' else x['dc'], gates, c,
                        x['c_prev'], dtype, dt, mutant))
    return res


def tanh_fwd(x, dtype, dt=np.float64):
    y = np.tanh(np.asarray(x, dt)).astype(dt)
    return dict(y=Out(y, np.abs(y), 8.0, dtype, 'tanh_y'))


def tanh_bwd(dy, y, dtype, dt=np.float64):
    """dx = dy (1 - y^2): the square, the difference, the product - k = 3 on S = |dy| (1 + y^2), no measured constant"""
    dy, y = np.asarray(dy, dt), np.asarray(y, dt)
    dx = (dy * (dt(1) - (y * y).astype(dt)).astype(dt)).astype(dt)
    return dict(dx=Out(dx, np.abs(dy) * (1 + y * y), dtype=dtype, group=None, k=3.0))


TANH_N = (1, 255, 256, 257)


# ---------------------------------------------------------------- dot attention
def da_fwd(src, x, mask, dtype, dt=np.float64, mutant=None):
    """src [L, B, D], x [B, D], mask [B, L] (non-zero = padding) or None -> probs [L, B] fp32, ctx [B, D].  A fully masked
    row is softmax of all -inf: its probs and ctx are NaN."""
    src, x = np.asarray(src, dt), np.asarray(x, dt)
    L, B, D = src.shape
    rd = src
    if mutant == 'da_stride_swapped':
        lb = (np.arange(B)[None, :] * B + np.arange(L)[:, None]) % (L * B)
        rd = src.reshape(L * B, D)[lb]
    pr = (rd * x[None]).astype(dt)
    sc, Labs = lane_sum(pr, dt), np.abs(np.asarray(pr, np.float64)).sum(-1)                       # [L, B]
    if mask is not None:
        mk = np.asarray(mask).reshape(-1)[(np.arange(L)[:, None] * B + np.arange(B)[None, :])] if mutant == 'da_mask_l_major' \
            else np.asarray(mask).T
        sc = np.where(mk != 0, -np.inf, sc).astype(dt)
    if mutant == 'da_wave3_keys_dropped':
        sc[3::4] = -np.inf
    if mutant == 'da_keys_past_256_dropped':
        sc[256:] = -np.inf
    with np.errstate(all='ignore'):
        m = sc.max(0)
        e = np.exp((sc - m[None]).astype(dt)).astype(dt)
        den = block_sum(e.T, dt)
        p = (e * (dt(1) / den).astype(dt)[None]).astype(dt)
        if dt is np.float64:
            ctx = np.einsum('lb,lbd->bd', p, rd)
        else:
            ctx = np.zeros((B, D), dt)
            for l in range(L):
                ctx = (ctx + (p[l][:, None] * rd[l]).astype(dt)).astype(dt)
        S_ctx = np.einsum('lb,lbd->bd', np.nan_to_num(np.asarray(p, np.float64)), np.abs(np.asarray(rd, np.float64)))
        live = np.isfinite(sc)
        lse = np.where(np.isfinite(m), m + np.log(np.asarray(den, np.float64)), 0.0)
        spread = float(np.abs(np.where(live, sc - lse[None], 0.0)).max())
    Lmax = float(np.where(live, Labs, 0.0).max())
    gP = 8.0 + spread + (-(-D // 64) + 6) * Lmax
    gp = 2 * gP + -(-L // 256) + 8
    probs = np.ascontiguousarray(p.T).reshape(L, B) if mutant == 'da_probs_b_major' else p
    return dict(probs=Out(probs, np.abs(p), gp, 'float32', 'da_probs'), ctx=Out(ctx, S_ctx, L + gp, dtype, 'da_ctx'))


def da_bwd(src, probs, dctx, x, dtype, want_dsrc, dt=np.float64, mutant=None):
    """probs: what the forward stored -> dx [B, D] and, if asked for, dsrc [L, B, D] (contiguous)"""
    src, probs, dctx, x = (np.asarray(a, dt) for a in (src, probs, dctx, x))
    L, B, D = src.shape
    pr = (src * dctx[None]).astype(dt)
    dp, S_dp = lane_sum(pr, dt), np.abs(np.asarray(pr, np.float64)).sum(-1)
    t = (probs * dp).astype(dt)
    s = block_sum(t.T, dt)
    p64 = np.abs(np.asarray(probs, np.float64))
    S_s = (p64 * S_dp).sum(0)
    ds = (probs * dp).astype(dt) if mutant == 'da_dx_without_softmax_centering' else (probs * (dp - s[None]).astype(dt)).astype(dt)
    S_ds = p64 * (S_dp + S_s[None])
    if dt is np.float64:
        dx = np.einsum('lb,lbd->bd', ds, src)
    else:
        dx = np.zeros((B, D), dt)
        for l in range(L):
            dx = (dx + (ds[l][:, None] * src[l]).astype(dt)).astype(dt)
    base = -(-D // 64) + 6 + -(-L // 256) + 6 + 8
    res = dict(dx=Out(dx, np.einsum('lb,lbd->bd', S_ds, np.abs(np.asarray(src, np.float64))), L + base, dtype, 'da_dx'))
    if want_dsrc:
        a = (probs[..., None] * dctx[None]).astype(dt)
        b = np.zeros_like(a) if mutant == 'da_dsrc_without_score_term' else (ds[..., None] * x[None]).astype(dt)
        S = p64[..., None] * np.abs(dctx)[None] + S_ds[..., None] * np.abs(x)[None]
        res['dsrc'] = Out((a + b).astype(dt), S, base, dtype, 'da_dsrc')
    return res


# L, D, B, source layout (lbd: [L, B, D] contiguous | bld: batch first, s_sl = D, s_sb = L D | padded: rows of D + 3), mask
# (none: a null pointer | ragged | one: one live key per row | row0: row 0 fully masked, the others ragged), dsrc asked for;
# every case runs in bf16 and fp32
DA = [
    dict(id='L1_D1_B1', L=1, D=1, B=1, lay='lbd', mask='none', dsrc=True, mutants=()),
    dict(id='L3_D63_B5', L=3, D=63, B=5, lay='bld', mask='ragged', dsrc=False, mutants=('da_mask_l_major', 'da_stride_swapped')),
    dict(id='L4_D64_B5', L=4, D=64, B=5, lay='padded', mask='one', dsrc=True, mutants=('da_probs_b_major', 'da_mask_l_major')),
    dict(id='L5_D72_B1', L=5, D=72, B=1, lay='lbd', mask='none', dsrc=True, mutants=('da_wave3_keys_dropped',
         'da_dx_without_softmax_centering')),
    dict(id='L23_D300_B5', L=23, D=300, B=5, lay='bld', mask='row0', dsrc=True, mutants=('da_wave3_keys_dropped',
         'da_stride_swapped', 'da_dsrc_without_score_term')),
    dict(id='L257_D64_B5', L=257, D=64, B=5, lay='padded', mask='ragged', dsrc=False, mutants=('da_keys_past_256_dropped',
         'da_probs_b_major')),
    dict(id='L1024_D63_B1', L=1024, D=63, B=1, lay='lbd', mask='none', dsrc=True, mutants=('da_keys_past_256_dropped',
         'da_dx_without_softmax_centering')),
]


def da_paths(case):
    L, D = case['L'], case['D']
    # keys: waves without a key (L < 4), a wave's ragged last round (L % 4), one or several 256-strided trips of the softmax;
    # D: one lane trip (partial or whole), a ragged second one, and more than one 256-strided trip of the ctx / dx loops
    return {'da:lay:' + case['lay'], 'da:mask:' + case['mask'], 'da:dsrc:%d' % case['dsrc'],
            'da:keys:' + ('<4' if L < 4 else ('one_trip' if L <= 256 else 'several_trips')) + (':ragged' if L % 4 else ':whole'),
            'da:lanes:' + ('partial' if D < 64 else ('whole' if D % 64 == 0 else 'ragged')), 'da:D>256' if D > 256 else 'da:D<=256',
            'da:one_block' if case['B'] == 1 else 'da:several_blocks'}


def da_mask(case):
    L, B = case['L'], case['B']
    if case['mask'] == 'none':
        return None
    m = np.ones((B, L), np.uint8)
    for b in range(B):
        m[b, :max(L - (B - 1 - b) * L // 6, 1)] = 0                     # ragged: the last row keeps every key
    if case['mask'] == 'one':
        m[:] = 1
        m[np.arange(B), (np.arange(B) * 3) % L] = 0
    if case['mask'] == 'row0':
        m[0] = 1
    return m


def da_inputs(case, dtype):
    def make():
        r, L, B, D = _rng('da', case['id']), case['L'], case['B'], case['D']
        f = lambda sc, *shape: store(r.standard_normal(shape) * sc, dtype)                               # noqa: E731
        return dict(src=f(1.0, L, B, D), x=f(2.0 / np.sqrt(D), B, D), dctx=f(1.0, B, D), mask=da_mask(case))
    return cached(('da_in', case['id'], dtype), make)


def da_case(case, dtype, dt=np.float64, mutant=None, probs=None):
    x = da_inputs(case, dtype)
    res = da_fwd(x['src'], x['x'], x['mask'], dtype, dt, mutant)
    if probs is None:
        probs = store(da_fwd(x['src'], x['x'], x['mask'], dtype, dt)['probs'].value, 'float32')
    with np.errstate(all='ignore'):
        res.update(da_bwd(x['src'], probs, x['dctx'], x['x'], dtype, case['dsrc'], dt, mutant))
    return res


# ================================================================ more pointwise kernels: GLU, GELU, dropout, loss, embedding
def glu_fwd(h, dtype, dt=np.float64, mutant=None):
    """h [rows, 2C] = [a | gate] -> y = a sigmoid(gate); gamma = 8 + max |gate| (the exponent's own rounding)"""
    h = np.asarray(h, dt)
    Cc = h.shape[1] // 2
    a, g = (h[:, Cc:], h[:, :Cc]) if mutant == 'glu_gate_first' else (h[:, :Cc], h[:, Cc:])
    y = (a * _sig(g, dt)).astype(dt)
    return dict(y=Out(y, np.abs(y), 8.0 + float(np.abs(g).max()), dtype, 'glu_y'))


def glu_bwd(h, dy, dtype, dt=np.float64, mutant=None):
    """dh = [dy s | dy a s (1 - s)]; 1 - s is rounded on the scale of 1, so S of the gate half is |dy a| s"""
    h, dy = np.asarray(h, dt), np.asarray(dy, dt)
    Cc = h.shape[1] // 2
    a, g = h[:, :Cc], h[:, Cc:]
    s = _sig(g, dt)
    da, dg = (dy * s).astype(dt), (((dy * a).astype(dt) * s).astype(dt) * (dt(1) - s).astype(dt)).astype(dt)
    return dict(dh=Out(np.concatenate([da, dg], 1), np.concatenate([np.abs(da), np.abs(dy * a) * s], 1),
                       8.0 + float(np.abs(g).max()), dtype, 'glu_dh'))


GELU_K = 3e-7 / EPS + 112.0


def gelu(x, dt=np.float64):
    """x Phi(x) against float64 erf.  The kernel (gemm_common.h gelu_erf2) evaluates erfc by Abramowitz-Stegun 7.1.28,
    1 / (1 + a1 x + ... + a6 x^6)^16, whose error is at most 3e-7 ABSOLUTE; in fp32 the polynomial carries about 6 roundings
    that the sixteenth power multiplies by 16, plus the four squarings, the reciprocal and the two products: 112.  So the
    derived bound is u_out |ref| + (3e-7 / 2^-24 + 112) 2^-24 |x| / 2 - no measured constant."""
    x = np.asarray(x, dt)
    if dt is np.float64:
        from math import erf
        y = x * 0.5 * (1.0 + np.vectorize(erf)(x / np.sqrt(2.0)))
    else:
        av = np.abs(x)
        z = (av * dt(0.70710678118654752)).astype(dt)
        q = (z * dt(0.0000430638) + dt(0.0002765672)).astype(dt)
        for cf in (0.0001520143, 0.0092705272, 0.0422820123, 0.0705230784, 1.0):
            q = (q * z + dt(cf)).astype(dt)
        for _ in range(4):
            q = (q * q).astype(dt)
        y = ((av * dt(-0.5)).astype(dt) * (dt(1) / q).astype(dt) + np.maximum(x, dt(0))).astype(dt)
    return dict(y=Out(y, np.abs(x) / 2, dtype='bfloat16', group=None, k=GELU_K))


def dropout(x, keep, p, dtype, add=None, dt=np.float64, mutant=None):
    """y = [add +] x keep / (1 - p), keep: the 0 / 1 flags of tell_amd.rng.keep_mask over the element indices.  The mask is
    exact (a dropped element is x * 0 [+ add] bit for bit); a kept one carries the rounding of 1 / (1 - p) (a difference and a
    quotient in fp32 on the host: 1.5), the product and, with add, the sum: k = 3 (4 with add) on S = |x / (1 - p)| [+ |add|]."""
    x, p32 = np.asarray(x, dt), np.float32(p)
    ik = dt(np.float32(1) / (np.float32(1) - p32)) if dt is np.float32 else 1.0 / (1.0 - float(p32))
    if float(p32) == 0.0:
        ik = dt(1)
    t = (x * (np.asarray(keep, dt) * ik).astype(dt)).astype(dt)
    S = np.abs(t)
    if add is not None:
        add = np.asarray(add, dt)
        t, S = (add + t).astype(dt), S + np.abs(add)
    return dict(y=Out(t, S, dtype=dtype, group=None, k=3.0 + (add is not None), exact_at=np.asarray(keep) == 0))


def loss_bits(x, n, dt=np.float64):
    """x / ln 2 / n: two quotients and the rounded constant, k = 3"""
    v = (dt(x) / dt(np.float32(0.69314718055994531))) / dt(np.float32(n)) if dt is np.float32 else float(x) / np.log(2.0) / n
    return dict(out=Out(np.array([v], dt), np.array([abs(float(v))]), group=None, k=3.0))


def roberta_embed(ids, pad, word, posemb, dtype, dt=np.float64, mutant=None):
    """ids [B, S] -> pos [B, S] (cumsum of the non-pad flags, + pad; pad where the token is pad), out = word[ids] + posemb[pos]
    (one sum: exact to one rounding in fp32, k = 1 for the second rounding of a bf16 store)"""
    ids = np.asarray(ids)
    ok = ids != pad
    cnt = np.ones_like(ok) if mutant == 'pos_pad_counts' else ok
    cum = np.cumsum(cnt, 1)
    if mutant == 'pos_wave_offset_dropped':
        Bn, S = ids.shape
        c64 = np.zeros((Bn, -(-S // 64) * 64), np.int64)
        c64[:, :S] = cnt
        cum = np.cumsum(c64.reshape(Bn, -1, 64), 2).reshape(Bn, -1)[:, :S]
    pos = np.where(ok, cum + pad, pad).astype(np.int32)
    w, q = np.asarray(word, dt)[ids], np.asarray(posemb, dt)[pos]
    return dict(pos=Out(pos.astype(np.float32)), out=Out((w + q).astype(dt), np.abs(w) + np.abs(q), dtype=dtype, group=None,
                                                         k=1.0 if dtype == 'bfloat16' else 0.0))


def mask_rows(x, mask, dtype, mutant=None):
    x = np.array(x, np.float32)
    m = np.asarray(mask) != 0
    if mutant == 'mask_rows_second_trip_dropped':
        m = m & (np.arange(len(m)) < 4096)
    x[m] = 0
    return dict(x=Out(x, dtype=dtype))


PW2 = [_pw('glu', ['glu_gate_first'] if d == 'bfloat16' else [], dtype=d, rows=r, C=Cc) for d, r, Cc in (
    ('bfloat16', 511, 1), ('float32', 512, 1), ('bfloat16', 103, 5), ('float32', 8, 64),
    ('bfloat16', past_cap('glu', 'bfloat16', 640) // 64, 64))]
PW2 += [_pw('gelu', n=n) for n in (8, 2048, 2056)]
PW2 += [_pw('dropout', dtype=d, p=p, n=n) for d, p, n in (
    ('bfloat16', 0.0, 1023), ('float32', 0.1, 1024), ('bfloat16', 0.999, 1025),
    ('float32', 0.1, past_cap('dropout', 'float32', 1000)))]
PW2 += [_pw('dropout_add', ['dropout_add_index_by_chunk'] if p == 0.1 else [], dtype=d, p=p, n=n) for d, p, n in (
    ('bfloat16', 0.0, 2040), ('float32', 0.1, 1024), ('bfloat16', 0.999, 2056), ('bfloat16', 0.1, 2048),
    ('float32', 0.1, past_cap('dropout_add', 'float32', 1000)))]
PW2 += [_pw('loss_bits', n=37)]
PW2 += [_pw('embed', m, dtype=d, S=S, E=E) for d, S, E, m in (
    ('float32', 1, 5, ()), ('bfloat16', 63, 260, ('pos_pad_counts',)), ('float32', 64, 8, ('pos_pad_counts',)),
    ('bfloat16', 65, 8, ('pos_wave_offset_dropped',)), ('float32', 1024, 8, ('pos_wave_offset_dropped', 'pos_pad_counts')))]
PW2 += [_pw('mask_rows', ['mask_rows_second_trip_dropped'], dtype=d, rows=4096 + 50, C=3) for d in ('bfloat16', 'float32')]
PW += PW2
PW2_OPS = ('glu', 'gelu', 'dropout', 'dropout_add', 'loss_bits', 'embed', 'mask_rows')
SEED, SALT = 1234, 77


def pw_paths(case):
    op = case['op']
    if op == 'glu':
        return {'glu:C%d' % case['C'], 'glu:' + case['dtype'], 'glu:' + stream_size(op, case['dtype'], case['rows'] * case['C'])}
    if op == 'gelu':
        n = case['n'] // 8
        return {'gelu:' + ('below' if n < 256 else ('at' if n == 256 else 'above'))}
    if op in ('dropout', 'dropout_add'):
        dty = case['dtype']
        return {'%s:%s' % (op, stream_size(op, dty, case['n'])), '%s:p%g' % (op, case['p']), '%s:%s' % (op, dty)}
    if op == 'loss_bits':
        return {'loss_bits'}
    if op == 'embed':
        S = case['S']               # the prefix over one partial wave, one whole wave, into a second wave, over all sixteen
        waves = 'one_wave' if S == 64 else ('all_waves' if S == 1024 else 'two_waves')
        waves = 'one_token' if S == 1 else ('partial_wave' if S < 64 else waves)
        return {'embed:' + waves, 'embed:' + case['dtype'], 'embed:E' + ('>256' if case['E'] > 256 else '<=256')}
    if op == 'mask_rows':
        return {'mask_rows:second_trip', 'mask_rows:' + case['dtype']}
    return _mover_paths(case)


def pw_inputs(case):
    def make():
        r, op = _rng('pw2', case['id']), case['op']
        f = lambda shape, d: store(r.standard_normal(shape), d)                                # noqa: E731
        if op == 'glu':
            h = r.standard_normal((case['rows'], 2 * case['C']))
            h[:, case['C']:] = r.uniform(-20.0, 20.0, (case['rows'], case['C']))
            return dict(h=store(h, case['dtype']), dy=f((case['rows'], case['C']), case['dtype']))
        if op == 'gelu':
            return dict(x=store(r.uniform(-6.0, 6.0, case['n']), 'bfloat16'))
        if op in ('dropout', 'dropout_add'):
            return dict(x=f(case['n'], case['dtype']), add=f(case['n'], case['dtype']))
        if op == 'loss_bits':
            return dict(x=np.float32(123.456), n=case['n'])
        if op == 'embed':
            S, pad = case['S'], 1
            ids = r.integers(2, 50, (3, S))
            ids[0, :S // 3] = pad                                # pads at the front
            ids[1, S // 2:S // 2 + max(S // 5, 1)] = pad         # in the middle
            ids[2] = pad                                         # an all-pad row
            return dict(ids=ids.astype(np.int64), pad=pad, word=f((50, case['E']), case['dtype']),
                        posemb=f((S + pad + 1, case['E']), case['dtype']))
        mask = (r.uniform(size=case['rows']) < 0.4).astype(np.uint8)
        mask[[0, 4095, 4096, case['rows'] - 1]] = (1, 1, 1, 1)
        return dict(x=f((case['rows'], case['C']), case['dtype']), mask=mask)
    return cached(('pw2_in', case['id']), make) if case['op'] in PW2_OPS else _mover_inputs(case)


def keep_of(case, mutant=None):
    """the keep flags of a dropout case from the project's own restatement of the hash (tell_amd.rng)"""
    from tell_amd import rng
    idx = np.arange(case['n'], dtype=np.uint64)
    if mutant == 'dropout_add_index_by_chunk':
        idx = idx // np.uint64(8 if case['dtype'] == 'bfloat16' else 4)
    return cached(('keep', case['id'], mutant), lambda: rng.keep_mask(SEED, SALT, idx, case['p']))


def pw_case(case, dt=np.float64, mutant=None):
    op = case['op']
    if op not in PW2_OPS:
        return _mover_case(case, dt, mutant)
    x = pw_inputs(case)
    if op == 'glu':
        res = glu_fwd(x['h'], case['dtype'], dt, mutant)
        res.update(glu_bwd(x['h'], x['dy'], case['dtype'], dt, mutant))
        return res
    if op == 'gelu':
        return gelu(x['x'], dt)
    if op in ('dropout', 'dropout_add'):
        return dropout(x['x'], keep_of(case, mutant), case['p'], case['dtype'], x['add'] if op == 'dropout_add' else None, dt)
    if op == 'loss_bits':
        return loss_bits(x['x'], x['n'], dt)
    if op == 'embed':
        return roberta_embed(x['ids'], x['pad'], x['word'], x['posemb'], case['dtype'], dt, mutant)
    return mask_rows(x['x'], x['mask'], case['dtype'], mutant)
