"""float64 reference of the adaptive embedding and loss kernels of the training step (the first 320 lines of csrc/adaptive.hip:
tell_adaptive_partition, tell_embed_finalize, tell_embed_finalize_bwd, tell_embed_table_grad, tell_ce_fwd, tell_ce_bwd,
tell_sum_f32) and of the two kernels that are the adaptive input embedding of the decode step (csrc/decode.hip:
tell_embed_gather_step, tell_embed_lookup_step) - with the element-wise bounds they are held to, the case tables and the
mutants that tests/test_adaptive_ref_host.py and tests/test_gpu_adaptive_train.py walk.  numpy only;
nothing here comes from oracle/.  The shared pieces (Out, store, same_bits, ratio, failures, wave_fold, the bound itself) are
those of tests/small_ref.py; failures() is given this module's constant as its parameter.  Inputs are
rounded to their storage type BEFORE they reach a function.

Every function takes dt (np.float64: the reference; np.float32: the same formulas rounded to fp32 in the kernel's order)
and a mutant name, and returns a dict of Out (value, S, gamma, storage type, group).  Integer outputs are carried as fp32
arrays (every value is below 2^24) in group 'exact'; a buffer's prefill is SENTINEL.  Bound of one element of a measured group:

    u_out |ref|  +  c gamma 2^-24 S  +  2^-126 (1 + S)

gamma, read off the kernels (a 256-thread workgroup: ceil(V / 256) terms per thread, 6 = the butterfly of a wave, 4 = the sum
of the four waves):

    ce_lse      ceil(V / 256) + 6 + 4 + 8 + spread + 4     the sum of __expf(row - mx); __expf is exp2(x log2 e): 8 for the
                                                           exponential, and the rounding of its argument grows with it:
                                                           spread = max_j |row_j - lse| over the finite entries; 4 for the
                                                           maximum's subtraction, __logf and the final sum.
                                                           S = 1 + |mx| + |log s|: the two terms the kernel adds, and 1 because
                                                           the ABSOLUTE error of log s is the RELATIVE error of s
    ce_loss     the same                                   S = |lse| + |row[tg]| (the difference cancels when the target
                                                           dominates its row)
    ce_dlogits  8 + spread + 2                             one __expf of row - lse (lse: what the forward launch STORED),
                                                           the one-hot's subtraction, the product; S = |g| (p + onehot)

Derived bounds (group None:  u_out |ref| + k 2^-24 S + 2^-126 (1 + S), no measured constant):

    embed_finalize       scale x + pos, as axpy in section 35: fp32 k = 1 + 2^-23 on S = |scale x|; bf16 k = 2 on
                         S = |scale x| + |pos|.  The position (pad -> pos_pad, else pos_pad + 1 + t + start_pos, clamped to
                         pos_rows - 1) is exact: a wrong one adds another row of the table
    embed_finalize_bwd   one product: k = 0 (fp32), 1 (bf16) on S = |scale dout|; rows of dband no slot names keep their prefill
    embed_table_grad     a table row named by m band rows is m - 1 sequential additions and one accumulate: k = m on
                         S = |demb0| + sum |drows|.  AND bit for bit (output demb_bits) the fp32 sum of the band rows in
                         increasing j, added to the prefilled demb once: the arithmetic is additions only, the build has no
                         fast-math, and the order is what round 6 promised
    sum_f32              k = ceil(n / 1024) + 6 + 16 + 1 on S = |out0| + sum |x|.  AND bit for bit (out_bits): thread t adds
                         x[t], x[t + 1024], ..., the butterfly, the 16 wave sums left to right, out0 + t when accumulating
    embed_lookup_step    one fp32 sum and a bf16 store: k = 1 on S = |table| + |pos|; an id outside [0, V) gives bf16(pos)

Exact: everything tell_adaptive_partition writes, and cat / pos_out of tell_embed_gather_step.

Definitions the kernels leave open are stated here.  tell_adaptive_partition with N <= 0 writes NOTHING, band_count and
n_valid included.  An id outside every band gets no entry in any band list, and its slot / head_target keep the buffer's
prefill; it still counts in n_valid unless it equals pad_idx.  n_bands 0 and 5 are refused.  tell_ce_fwd zeroes loss and
lse of the rows at or past min(M, *m_dev); tell_ce_bwd leaves those rows of dlogits alone.  A row whose target is the
ignored index has loss 0 exactly, a held lse, and a gradient of zeros up to sign ((p - onehot) * 0 is -0 where p < onehot).
tell_embed_gather_step with an id outside every band writes a row of zeros.

Measured on the MI355X: MEASURED and C below, and DESIGN.md section 40.
"""
import numpy as np

from decode_ref import EPS, TINY, U_OUT, _pin, _sum, bf16_round                # noqa: F401  (re-exported)
from small_ref import SENTINEL, Out, _rng, block_sum, cached, ratio, same_bits, store, wave_fold   # noqa: F401  (re-exported)
from small_ref import failures as _failures

F32, F64 = np.float32, np.float64

# largest observed (|got - ref| - u_out |ref|) / (gamma 2^-24 S) over the grid of tests/test_gpu_adaptive_train.py on the
# MI355X, and the pinned constant: four times that, rounded up to a power of two; 2^-10 where the ratio never left u_out |ref|.
# A group missing from MEASURED is not pinned: its GPU test then fails with the measured ratio in its message.
MEASURED = {'ce_lse': 0.032098, 'ce_loss': 0.048938, 'ce_dlogits': 1.063200}
C = {k: _pin(v) for k, v in MEASURED.items()}
GROUPS = ('ce_lse', 'ce_loss', 'ce_dlogits')

PART_MUTANTS = ('part_base_not_carried', 'part_wave_offset_dropped', 'part_tail_head_target_plus_one', 'part_n_valid_per_band',
                'part_pad_counted', 'part_local_without_lo')
FIN_MUTANTS = ('fin_tbc_row_b_major', 'fin_pos_without_plus_one', 'fin_pad_pos_advanced', 'fin_clamp_missing',
               'fin_scale_on_pos', 'finb_rows_by_n')
TG_MUTANTS = ('tg_second_chunk_dropped', 'tg_fourth_candidate_dropped', 'tg_owner_twice', 'tg_cols_past_1024_dropped',
              'tg_count_not_clipped', 'tg_padding_accumulated', 'tg_store_not_accumulate', 'tg_decreasing_order')
CE_MUTANTS = ('ce_second_trip_dropped', 'ce_max_not_subtracted', 'ce_row_idx_ignored', 'ce_m_dev_ignored',
              'ce_ignored_still_charged', 'ce_onehot_plus_one', 'ce_gscale_squared')
SUM_MUTANTS = ('sum_threads_past_512_dropped', 'sum_accumulate_ignored', 'sum_m_dev_ignored')
STEP_MUTANTS = ('step_band_offset_dropped', 'step_unknown_id_reads_row0', 'step_second_trip_dropped')
MUTANTS = PART_MUTANTS + FIN_MUTANTS + TG_MUTANTS + CE_MUTANTS + SUM_MUTANTS + STEP_MUTANTS


def failures(got, o, c=None):
    """small_ref.failures with this module's pinned constant"""
    if c is None and o.group in GROUPS:
        c = C[o.group]
    return _failures(got, o, c)


def skipped(o):
    """the elements ratio() does not judge: a non-finite reference, or S = 0"""
    ref, S = np.asarray(o.value, F64), np.broadcast_to(np.asarray(o.S, F64), np.shape(o.value))
    bad = ~(np.isfinite(ref) & (o.gam * EPS * S > 0))
    return bad if o.exact_at is None else bad & ~o.exact_at


def _prefill(*shape):
    return np.full(shape, SENTINEL, F32)


# ================================================================ tell_adaptive_partition (exact)
PART_CUT = (100, 300, 600, 1000)


def partition(ids, N, cut, pad_idx, null=(), mutant=None):
    """ids [>= N] int64, cut: the bands' upper bounds -> rows, local [n_bands, N], count [n_bands], slot, head_target [N],
    n_valid [1]; what the kernel does not write keeps SENTINEL.  One 1024-thread workgroup walks N in chunks of 1024: a row's
    place in its band list is the band's rows before this chunk (base_s), plus those in earlier waves of the chunk, plus
    those in earlier lanes of its wave.  null: the optional outputs given as null pointers (left out of the result)"""
    nb, W = len(cut), max(N, 1)
    o = dict(rows=_prefill(max(nb, 1), W), local=_prefill(max(nb, 1), W), count=_prefill(max(nb, 1)), slot=_prefill(W),
             head_target=_prefill(W), n_valid=_prefill(1))
    if 1 <= nb <= 4 and N > 0:
        ids = np.asarray(ids, np.int64)[:N]
        for b in range(nb):
            lo, hi, base = (0 if b == 0 else cut[b - 1]), cut[b], 0
            for start in range(0, N, 1024):
                chunk = ids[start:start + 1024]
                i = np.nonzero((chunk >= lo) & (chunk < hi))[0]
                rank = np.arange(i.size)
                if mutant == 'part_wave_offset_dropped':
                    rank = rank - np.searchsorted(i, i // 64 * 64)
                j = rank + (0 if mutant == 'part_base_not_carried' else base)
                o['rows'][b, j] = start + i
                o['local'][b, j] = chunk[i] - (0 if mutant == 'part_local_without_lo' else lo)
                o['slot'][start + i] = b * N + j
                o['head_target'][start + i] = chunk[i] if b == 0 else \
                    cut[0] + b - (0 if mutant == 'part_tail_head_target_plus_one' else 1)
                base += i.size
            o['count'][b] = base
        valid = N if mutant == 'part_pad_counted' else int((ids != pad_idx).sum())
        o['n_valid'][0] = valid * (nb if mutant == 'part_n_valid_per_band' else 1)
    return {k: Out(v, dtype='int32') for k, v in o.items() if k not in null}


def _part(N, nb, pat, pad=1, pads='none', null=(), mutants=()):
    tag = 'N%d_b%d_%s' % (N, nb, pat) + ('' if pads == 'none' else '_pad_' + pads) + ('_padm1' if pad == -1 else '') + \
        ''.join('_no_' + k for k in null)
    return dict(id=tag, N=N, nb=nb, pat=pat, pad=pad, pads=pads, null=tuple(null), mutants=tuple(mutants))


PART = [
    _part(1, 1, 'random'),
    _part(63, 2, 'alternate', pads='scattered', mutants=('part_pad_counted', 'part_n_valid_per_band', 'part_local_without_lo',
                                                         'part_tail_head_target_plus_one')),
    _part(64, 3, 'empty_middle', null=('slot',), mutants=('part_local_without_lo',)),
    _part(65, 4, 'alternate', mutants=('part_wave_offset_dropped', 'part_tail_head_target_plus_one')),
    _part(65, 2, 'random', pads='all', mutants=('part_pad_counted',)),
    _part(1023, 3, 'edges', null=('head_target',), mutants=('part_wave_offset_dropped',)),
    _part(1024, 2, 'one_band', null=('n_valid',), mutants=('part_wave_offset_dropped',)),
    _part(1025, 3, 'alternate', mutants=('part_base_not_carried',)),
    _part(2049, 2, 'late_band', mutants=('part_base_not_carried',)),
    _part(2049, 4, 'alternate', pads='front', mutants=('part_base_not_carried', 'part_wave_offset_dropped',
                                                       'part_n_valid_per_band')),
    _part(3000, 3, 'outside', pad=-1, mutants=('part_base_not_carried', 'part_pad_counted')),
    _part(0, 3, 'random'),
    _part(5, 0, 'random'),
    _part(5, 5, 'random'),
]


def part_cut(case):
    return (PART_CUT + (1500,))[:case['nb']]


def part_inputs(case):
    def make():
        N, nb, pat, r = case['N'], case['nb'], case['pat'], _rng('part', case['id'])
        cut = part_cut(case) or (100,)
        lo = (0,) + tuple(cut[:-1])
        n = max(N, 1)
        inband = lambda b: r.integers(lo[b], cut[b], n)                                      # noqa: E731
        pick = lambda bands: np.choose(bands, [inband(b) for b in range(len(cut))])           # noqa: E731
        i = np.arange(n)
        if pat == 'random':
            ids = r.integers(0, cut[-1], n)
        elif pat == 'one_band':
            ids = inband(len(cut) - 1)
        elif pat == 'empty_middle':
            ids = pick(np.where(r.integers(0, 2, n) == 1, len(cut) - 1, 0))
        elif pat == 'late_band':                    # band 0 owns the whole first chunk, band 1 has no row before the second
            ids = pick(np.where(i < 1024, 0, 1))
        elif pat == 'alternate':
            ids = pick(i % len(cut))
        elif pat == 'edges':                        # every cut-off (the last one: outside) and one below it, and 0
            edge = np.array([0] + [c - d for c in cut for d in (1, 0)])
            ids = edge[i % edge.size]
        else:                                       # 'outside': below 0 and at or above the last cut-off too
            ids = r.integers(-5, cut[-1] + 50, n)
        ids = ids.astype(np.int64)
        pad = case['pad']
        if case['pads'] == 'front':
            ids[:n // 3] = pad
        elif case['pads'] == 'scattered':
            ids[::5] = pad
        elif case['pads'] == 'all':
            ids[:] = pad
        return dict(ids=ids)
    return cached(('part_in', case['id']), make)


def part_case(case, mutant=None):
    return partition(part_inputs(case)['ids'], case['N'], part_cut(case), case['pad'], case['null'], mutant)


def part_paths(case):
    """the branches of the launcher and of partition_kernel: refused, nothing to do, one chunk or a carried base_s, a ragged
    or whole last chunk, and per band what its ballots look like"""
    N, nb = case['N'], case['nb']
    if not 1 <= nb <= 4:
        return {'part:refused:bands%d' % nb}
    if N <= 0:
        return {'part:N<=0'}
    ids, cut = part_inputs(case)['ids'][:N], part_cut(case)
    p = {'part:bands%d' % nb, 'part:chunks:one' if N <= 1024 else 'part:chunks:carried',
         'part:last_chunk:whole' if N % 1024 == 0 else ('part:last_chunk:partial_wave' if N % 1024 < 64 else
                                                        'part:last_chunk:ragged'),
         'part:pad_idx:-1' if case['pad'] < 0 else 'part:pad_idx:token'}
    p |= {'part:null:' + k for k in case['null']} or {'part:null:none'}
    n_pad = int((ids == case['pad']).sum())
    p.add('part:pads:' + ('none' if n_pad == 0 else ('all' if n_pad == N else 'some')))
    if ((ids < 0) | (ids >= cut[-1])).any():
        p.add('part:ids:outside_every_band')
    for b in range(nb):
        f = (ids >= (0 if b == 0 else cut[b - 1])) & (ids < cut[b])
        per = [f[s:s + 1024] for s in range(0, N, 1024)]
        if not f.any():
            p.add('part:band:empty')
        if any(c.all() and c.size == 1024 for c in per):
            p.add('part:band:owns_a_chunk')
        if len(per) > 1 and not per[0].any() and f.any():
            p.add('part:band:second_chunk_only')
        w = [f[s:s + 64] for s in range(0, N, 64)]
        if any(x.any() and not x.all() for x in w):
            p.add('part:ballot:mixed')
        if any(x.all() for x in w):
            p.add('part:ballot:full')
    return p


# ================================================================ tell_embed_finalize / _bwd
FIN_CUT = (20, 50, 90)
FIN_PAD = 1


def fin_rows(B, T, tbc):
    n = np.arange(B * T)
    b, t = n // T, n % T
    return n, b, t, (t * B + b if tbc else n)


def embed_finalize(band_out, slot, ids, pos_table, pos_rows, B, T, scale, pos_pad, start_pos, tbc, dtype, dt=F64, mutant=None):
    """out [B T, E]: out[row(n)] = scale band_out[slot[n]] + pos_table[pos(n)]; pos_table may be TALLER than pos_rows (the
    clamp case: a kernel without the clamp then reads a higher row, inside the buffer)"""
    band_out, pos_table = np.asarray(band_out, dt), np.asarray(pos_table, dt)
    n, b, t, row = fin_rows(B, T, tbc and mutant != 'fin_tbc_row_b_major')
    pos = pos_pad + t + start_pos + (0 if mutant == 'fin_pos_without_plus_one' else 1)
    if mutant != 'fin_pad_pos_advanced':
        pos = np.where(np.asarray(ids) == pos_pad, pos_pad, pos)
    if mutant != 'fin_clamp_missing':
        pos = np.minimum(pos, pos_rows - 1)
    sc = dt(np.float32(scale))
    x, p = band_out[np.asarray(slot, np.int64)], pos_table[pos]
    prod = (sc * x).astype(dt)
    v = (sc * (x + p).astype(dt)).astype(dt) if mutant == 'fin_scale_on_pos' else (prod + p).astype(dt)
    out, S = np.zeros_like(v), np.zeros(v.shape)
    out[row] = v
    S[row] = np.abs(prod) if dtype == 'float32' else np.abs(prod) + np.abs(p)
    return dict(out=Out(out, S, dtype=dtype, group=None, k=1.0 + 2.0 ** -23 if dtype == 'float32' else 2.0))


def embed_finalize_bwd(dout, slot, dband0, B, T, scale, tbc, dtype, dt=F64, mutant=None):
    """dband[slot[n]] = scale dout[row(n)]; every other row of dband [n_bands B T, E] keeps its prefill"""
    dout = np.asarray(dout, dt)
    n, b, t, row = fin_rows(B, T, tbc)
    d, S = np.array(dband0, dt), np.zeros(np.shape(dband0))
    where = n if mutant == 'finb_rows_by_n' else np.asarray(slot, np.int64)
    d[where] = (dt(np.float32(scale)) * dout[row]).astype(dt)
    S[where] = np.abs(d[where])
    named = np.zeros(d.shape, bool)
    named[where] = True
    return dict(dband=Out(d, S, dtype=dtype, group=None, k=1.0 if dtype == 'bfloat16' else 0.0, exact_at=~named))


# B, T, E, tbc, scale ('one' | 'sqrt'), start_pos, pos_rows (None: a table tall enough); every case runs in bf16 and fp32
FIN = [
    dict(id='b1_t1_e1', B=1, T=1, E=1, tbc=0, scale='one', start=0, pos_rows=None, mutants=('fin_pos_without_plus_one',)),
    dict(id='b1_t7_e255_tbc', B=1, T=7, E=255, tbc=1, scale='sqrt', start=5, pos_rows=None,
         mutants=('fin_pad_pos_advanced', 'fin_scale_on_pos')),
    dict(id='b5_t1_e256_tbc', B=5, T=1, E=256, tbc=1, scale='one', start=0, pos_rows=None, mutants=('finb_rows_by_n',)),
    dict(id='b3_t4_e257_tbc', B=3, T=4, E=257, tbc=1, scale='sqrt', start=0, pos_rows=None,
         mutants=('fin_tbc_row_b_major', 'fin_pos_without_plus_one', 'finb_rows_by_n')),
    dict(id='b3_t4_e1024', B=3, T=4, E=1024, tbc=0, scale='sqrt', start=5, pos_rows=None,
         mutants=('fin_scale_on_pos', 'fin_pad_pos_advanced')),
    dict(id='b3_t4_e257_clamp', B=3, T=4, E=257, tbc=1, scale='one', start=5, pos_rows=9, mutants=('fin_clamp_missing',)),
]
FIN_TABLE_ROWS = 16             # rows of the position table a case allocates (>= pos_pad + 1 + T + start_pos)


def fin_scale(case):
    return 1.0 if case['scale'] == 'one' else float(np.float32(np.sqrt(case['E'])))


def fin_paths(case):
    B, T, E = case['B'], case['T'], case['E']
    trips = 'E<256' if E < 256 else ('E=256' if E == 256 else ('E%256=0' if E % 256 == 0 else 'E>256:ragged'))
    clamp = case['pos_rows'] is not None and FIN_PAD + T + case['start'] >= case['pos_rows']
    return {'fin:' + trips, 'fin:tbc%d' % case['tbc'], 'fin:B1' if B == 1 else 'fin:B>1', 'fin:T1' if T == 1 else 'fin:T>1',
            'fin:scale:' + case['scale'], 'fin:start_pos:%s' % ('0' if case['start'] == 0 else '>0'),
            'fin:clamped' if clamp else 'fin:in_table'}


def fin_inputs(case, dtype):
    """ids [B T] (right padding, (b + 1) % T pads in row b; one pad token when T = 1 < B), slot from the partition reference of
    three bands:
    a permutation of the rows with gaps, since each band's list starts at b N"""
    def make():
        B, T, E, r = case['B'], case['T'], case['E'], _rng('fin', case['id'])
        N = B * T
        ids = r.integers(2, FIN_CUT[-1], (B, T))
        for b in range(B if T > 1 else 0):
            ids[b, T - (b + 1) % T:] = FIN_PAD
        if T == 1 and B > 1:
            ids[B - 1, 0] = FIN_PAD
        ids = ids.reshape(N).astype(np.int64)
        slot = partition(ids, N, FIN_CUT, -1)['slot'].value.astype(np.int32)
        assert (slot >= 0).all()
        return dict(ids=ids, slot=slot, band_out=store(r.standard_normal((3 * N, E)), dtype),
                    pos_table=np.asarray(r.standard_normal((FIN_TABLE_ROWS, E)), F32),
                    dout=store(r.standard_normal((N, E)), dtype),
                    dband0=store(r.standard_normal((3 * N, E)), dtype))
    return cached(('fin_in', case['id'], dtype), make)


def fin_case(case, dtype, dt=F64, mutant=None):
    x, B, T = fin_inputs(case, dtype), case['B'], case['T']
    res = embed_finalize(x['band_out'], x['slot'], x['ids'], x['pos_table'], case['pos_rows'] or FIN_TABLE_ROWS, B, T,
                         fin_scale(case), FIN_PAD, case['start'], case['tbc'], dtype, dt, mutant)
    res.update(embed_finalize_bwd(x['dout'], x['slot'], x['dband0'], B, T, fin_scale(case), case['tbc'], dtype, dt, mutant))
    return res


# ================================================================ tell_embed_table_grad
def table_grad_sum(drows, local, count, cap, demb0, padding_idx, dt, mutant=None):
    """demb [rows, dim]: for every table row named by local[:min(count, cap)] (padding_idx excepted) the band rows that name
    it, added in increasing j, and that sum added to demb0 once -> demb, S, m (band rows per table row), touched rows"""
    n = count if mutant == 'tg_count_not_clipped' else min(count, cap)
    drows, local = np.asarray(drows, dt), np.asarray(local)[:n]
    d, S = np.array(demb0, dt), np.abs(np.asarray(demb0, F64))
    m, dim = np.ones(d.shape[0]), d.shape[1]
    touched = np.zeros(d.shape, bool)
    for row in np.unique(local):
        if row == padding_idx and mutant != 'tg_padding_accumulated':
            continue
        js = np.nonzero(local == row)[0]
        S[row] += np.abs(np.asarray(drows[js], F64)).sum(0)
        m[row] = js.size
        touched[row] = True
        if mutant == 'tg_second_chunk_dropped':
            js = js[js < js[0] + 1024]
        if mutant == 'tg_fourth_candidate_dropped':
            js = js[(js - js[0]) % 4 != 3]
        if mutant == 'tg_owner_twice':
            js = np.concatenate([js[:1], js])
        if mutant == 'tg_decreasing_order':
            js = js[::-1]
        acc = _sum(drows[js], 0, dt)
        new = acc if mutant == 'tg_store_not_accumulate' else (d[row] + acc).astype(dt)
        lim = min(dim, 1024) if mutant == 'tg_cols_past_1024_dropped' else dim
        d[row, :lim] = new[:lim]
    return d, S, m, touched


def embed_table_grad(drows, local, count, cap, demb0, padding_idx, dt=F64, mutant=None):
    d, S, m, touched = table_grad_sum(drows, local, count, cap, demb0, padding_idx, dt, mutant)
    bits = table_grad_sum(drows, local, count, cap, demb0, padding_idx, F32, mutant)[0]
    return dict(demb=Out(d, S, dtype='float32', group=None, k=m[:, None], exact_at=~touched), demb_bits=Out(bits))


TG_ROWS = 40          # rows of the band table; the id patterns name rows 0 .. 39 (distinct: the case's own, larger table)


def _tg(dim, cap, count, pat, ld=0, pad=-1, mutants=()):
    tag = 'dim%d_cap%d_n%d_%s' % (dim, cap, count, pat) + ('_ld+%d' % ld if ld else '') + ('' if pad < 0 else '_pad%d' % pad)
    return dict(id=tag, dim=dim, cap=cap, count=count, pat=pat, ld=dim + ld, pad=pad, mutants=tuple(mutants))


# dim, cap, *count_dev, id pattern, ld - dim, padding_idx; every case runs with bf16 and fp32 drows, demb prefilled
TG = [
    _tg(1, 1, 1, 'distinct', mutants=('tg_store_not_accumulate',)),
    _tg(255, 5, 0, 'runs', ld=3),
    _tg(256, 5, 3, 'runs', ld=3, mutants=('tg_owner_twice',)),
    _tg(1023, 5, 9, 'runs', mutants=('tg_count_not_clipped',)),
    _tg(1024, 5, 5, 'pad_in_run', pad=7, mutants=('tg_padding_accumulated', 'tg_owner_twice')),
    _tg(1025, 5, 5, 'runs', ld=3, mutants=('tg_cols_past_1024_dropped',)),
    _tg(1300, 5, 5, 'runs', mutants=('tg_cols_past_1024_dropped', 'tg_store_not_accumulate')),
    _tg(64, 1024, 1024, 'distinct', ld=3, mutants=('tg_store_not_accumulate',)),
    _tg(64, 1100, 1100, 'equal', mutants=('tg_second_chunk_dropped', 'tg_fourth_candidate_dropped', 'tg_decreasing_order')),
    _tg(64, 2100, 2100, 'equal', ld=3, mutants=('tg_second_chunk_dropped', 'tg_decreasing_order')),
    _tg(8, 2100, 2000, 'pairs', mutants=('tg_second_chunk_dropped', 'tg_fourth_candidate_dropped')),
]
TG_PAIRS = ((10, 1023), (20, 1024), (30, 1025))         # (first row, distance to the second row that names the same id)


def tg_table_rows(case):
    return case['cap'] + 1 if case['pat'] in ('distinct', 'pairs') else TG_ROWS


def tg_inputs(case, dtype):
    def make():
        r, dim, cap, pat = _rng('tg', case['id']), case['dim'], case['cap'], case['pat']
        rows = max(cap, case['count'])                       # (a count above cap has rows to go wrong in)
        if pat == 'distinct':
            local = r.permutation(tg_table_rows(case))[:rows]
        elif pat == 'equal':
            local = np.full(rows, 13)
        elif pat == 'pairs':
            local = r.permutation(tg_table_rows(case))[:rows]
            for first, dist in TG_PAIRS:
                local[first + dist] = local[first]
        elif pat == 'pad_in_run':
            local = np.array([3, case['pad'], 3, 3, case['pad']] * (rows // 5 + 1))[:rows]
        else:                                                # 'runs': the owner of row 2 is band row 1, not band row 0
            local = np.array([4, 2, 2, 4, 2, 9, 2, 4, 11] * (rows // 9 + 1))[:rows]
        return dict(local=local.astype(np.int32), drows=store(r.standard_normal((rows, dim)), dtype),
                    demb0=np.asarray(r.standard_normal((tg_table_rows(case), dim)), F32))
    return cached(('tg_in', case['id'], dtype), make)


def tg_case(case, dtype, dt=F64, mutant=None):
    x = tg_inputs(case, dtype)
    return embed_table_grad(x['drows'], x['local'], case['count'], case['cap'], x['demb0'], case['pad'], dt, mutant)


def tg_paths(case):
    dim, cap, cnt = case['dim'], case['cap'], case['count']
    local = tg_inputs(case, 'float32')['local'][:min(cnt, cap)]
    p = {'tg:grid:' + ('clamped' if cap > 1024 else 'cap'), 'tg:c0:' + ('one_trip' if dim <= 1024 else 'second_trip'),
         'tg:dim%256=0' if dim % 256 == 0 else ('tg:dim<256' if dim < 256 else 'tg:dim%256:ragged'),
         'tg:ld>dim' if case['ld'] > dim else 'tg:ld=dim',
         'tg:count:' + ('zero' if cnt == 0 else ('one' if cnt == 1 else ('inside' if cnt < cap else
                                                                          ('equal' if cnt == cap else 'above')))),
         'tg:padding_idx:-1' if case['pad'] < 0 else 'tg:padding_idx:row'}
    for row in np.unique(local):
        js = np.nonzero(local == row)[0]
        if js.size > 1:
            p.add('tg:duplicates')
            if js[0] > 0:
                p.add('tg:owner_not_row0')
            if js[-1] - js[0] >= 1024:
                p.add('tg:list_crosses_chunk')
            if js.size > 1024:
                p.add('tg:list_longer_than_chunk')
            if case['pad'] >= 0 and (local[js[0]:js[-1]] == case['pad']).any():
                p.add('tg:padding_row_inside_run')
    return p


# ================================================================ tell_ce_fwd / tell_ce_bwd
def ce_gamma(V, spread):
    return -(-V // 256) + 6 + 4 + 8 + spread + 4


def ce_targets(targets, row_idx, M, mutant=None):
    """the target of compacted row i: targets[row_idx ? row_idx[i] : i]"""
    if row_idx is None or mutant == 'ce_row_idx_ignored':
        return np.asarray(targets)[:M]
    return np.asarray(targets)[np.asarray(row_idx)]


def ce_fwd(logits, targets, row_idx, m, ignore, dt=F64, mutant=None):
    """logits [M, V] fp32, targets [>= M] int32, row_idx [M] or None, m: *m_dev or None -> lse, loss [M]"""
    x = np.asarray(logits, dt)
    M, V = x.shape
    Me = M if m is None or mutant == 'ce_m_dev_ignored' else min(m, M)
    tg = ce_targets(targets, row_idx, M, mutant)
    with np.errstate(all='ignore'):
        mx = x.max(1)
        e = np.exp(x if mutant == 'ce_max_not_subtracted' else (x - mx[:, None]).astype(dt)).astype(dt)
        s = block_sum(e[:, :256] if mutant == 'ce_second_trip_dropped' else e, dt)
        logs = np.log(s).astype(dt)
        lse = (mx + logs).astype(dt)
        loss = (lse - x[np.arange(M), tg]).astype(dt)
        lse64 = np.asarray(mx, F64) + np.log(np.exp(np.asarray(x, F64) - np.asarray(mx, F64)[:, None]).sum(1))
    if mutant != 'ce_ignored_still_charged':
        loss = np.where(tg == ignore, dt(0), loss)
    live = np.arange(M) < Me
    lse, loss = np.where(live, lse, dt(0)), np.where(live, loss, dt(0))
    d = np.abs(np.asarray(x, F64) - lse64[:, None])
    spread = float(d[np.isfinite(d) & live[:, None]].max()) if Me > 0 else 0.0
    gam = ce_gamma(V, spread)
    S_lse = 1.0 + np.abs(np.asarray(mx, F64)) + np.abs(lse64 - np.asarray(mx, F64))
    S_loss = np.abs(lse64) + np.abs(np.asarray(x, F64)[np.arange(M), tg])
    return dict(lse=Out(lse, S_lse, gam, 'float32', 'ce_lse', exact_at=~live),
                loss=Out(loss, S_loss, gam, 'float32', 'ce_loss', exact_at=~live | (tg == ignore)))


def ce_bwd(logits, targets, row_idx, m, ignore, lse, gscale, dtype, dt=F64, mutant=None):
    """dlogits [M, V] = (exp(logits - lse) - onehot) g, g = 0 for an ignored row; lse: what the forward launch stored; rows at
    or past the count keep SENTINEL"""
    x, lse = np.asarray(logits, dt), np.asarray(lse, dt)
    M, V = x.shape
    Me = M if m is None or mutant == 'ce_m_dev_ignored' else min(m, M)
    tg = ce_targets(targets, row_idx, M, mutant)
    gs = dt(np.float32(gscale))
    if mutant == 'ce_gscale_squared':
        gs = dt(gs * gs)
    g = np.where(tg == ignore, dt(0), gs)
    hot = np.zeros((M, V), dt)
    hot[np.arange(M), (tg + 1) % V if mutant == 'ce_onehot_plus_one' else tg] = 1
    with np.errstate(all='ignore'):
        p = np.exp((x - lse[:, None]).astype(dt)).astype(dt)
        d = ((p - hot).astype(dt) * g[:, None]).astype(dt)
        arg = np.abs(np.asarray(x, F64) - np.asarray(lse, F64)[:, None])
    live = np.arange(M) < Me
    d = np.where(live[:, None], d, dt(SENTINEL))
    S = np.abs(np.asarray(g, F64))[:, None] * (np.asarray(p, F64) + (np.arange(V)[None, :] == tg[:, None]))
    spread = float(arg[np.isfinite(arg) & live[:, None]].max()) if Me > 0 else 0.0
    return dict(dlogits=Out(d, S, 8 + spread + 2, dtype, 'ce_dlogits', exact_at=np.broadcast_to(~live[:, None], d.shape).copy()))


def _ce(V, M, logits, m=None, perm=False, call='head', g='one', ld=0, mutants=()):
    tag = 'v%d_m%d_%s_%s' % (V, M, logits, call) + ('' if m is None else '_cnt%d' % m) + ('_perm' if perm else '') + \
        ('' if g == 'one' else '_g' + g) + ('_ld+%d' % ld if ld else '')
    return dict(id=tag, V=V, M=M, logits=logits, m=m, perm=perm, call=call, g=g, ld=(V + 3) // 4 * 4 + ld, mutants=tuple(mutants))


CE_IGNORE = 1
CE_G = {'one': 1.0, '1/37': float(np.float32(1.0 / 37.0)), 'zero': 0.0}
# V, M, logits, *m_dev, row_idx a permutation, head call (targets may be the ignored index, as head targets are) or tail call
# (band-local ids: the ignored index is a quirk there), gscale, extra leading dimension; dlogits in bf16 and fp32
CE = [
    _ce(1, 1, 'random'),
    _ce(2, 3, 'spread', g='1/37', mutants=('ce_gscale_squared', 'ce_onehot_plus_one')),
    _ce(255, 3, 'random', m=0, call='tail', mutants=('ce_m_dev_ignored',)),
    _ce(256, 70, 'random', m=33, perm=True, call='tail', mutants=('ce_m_dev_ignored', 'ce_row_idx_ignored')),
    _ce(257, 3, 'equal', m=3, call='tail', mutants=('ce_second_trip_dropped', 'ce_ignored_still_charged')),
    _ce(600, 70, 'offset', m=100, perm=True, g='1/37', mutants=('ce_max_not_subtracted', 'ce_ignored_still_charged',
                                                                 'ce_row_idx_ignored', 'ce_gscale_squared')),
    _ce(600, 3, 'random', g='zero'),
    _ce(5002, 3, 'dominated', call='tail', m=2, mutants=('ce_second_trip_dropped', 'ce_onehot_plus_one')),
    _ce(8195, 1, 'neginf', ld=4, mutants=('ce_second_trip_dropped', 'ce_max_not_subtracted')),
]


def ce_inputs(case):
    def make():
        V, M, kind, r = case['V'], case['M'], case['logits'], _rng('ce', case['id'])
        x = r.uniform(-1.0, 1.0, (M, V))
        tg = r.integers(0, V, M)
        tg[0] = V - 1
        if M > 1:
            tg[1] = 0
        if V > CE_IGNORE and M > 2:                 # the ignored index: a head target, or - the quirk - a band-local id
            tg[2::4] = CE_IGNORE
        if kind == 'spread':
            x = r.uniform(-30.0, 30.0, (M, V))
            x[:, 0], x[:, V - 1] = -30.0, 30.0
        elif kind == 'equal':
            x[:] = 0.25
        elif kind == 'offset':
            x += 1000.0
        elif kind == 'dominated':                   # row 0: the target's logit dominates, so loss = lse - row[tg] cancels
            x[0, tg[0]] = 30.0
        elif kind == 'neginf':
            x[0, (tg[0] + V // 2) % V] = -np.inf
            x[0, 5] = -np.inf
        perm = r.permutation(M).astype(np.int32) if case['perm'] else None
        return dict(logits=np.asarray(x, F32), targets=tg.astype(np.int32), row_idx=perm)
    return cached(('ce_in', case['id']), make)


def ce_case(case, dtype, dt=F64, mutant=None, lse=None):
    """forward and backward of one case; lse: what the backward reads (default: this forward's, rounded to fp32)"""
    x = ce_inputs(case)
    res = ce_fwd(x['logits'], x['targets'], x['row_idx'], case['m'], CE_IGNORE, dt, mutant)
    if lse is None:
        lse = store(ce_fwd(x['logits'], x['targets'], x['row_idx'], case['m'], CE_IGNORE, dt)['lse'].value, 'float32')
    res.update(ce_bwd(x['logits'], x['targets'], x['row_idx'], case['m'], CE_IGNORE, lse, CE_G[case['g']], dtype, dt, mutant))
    return res


def ce_zero_rows(case):
    """[M] rows of dlogits whose gradient is zero by definition (an ignored target; every row when gscale = 0)"""
    x = ce_inputs(case)
    tg = ce_targets(x['targets'], x['row_idx'], case['M'])
    return (tg == CE_IGNORE) | (CE_G[case['g']] == 0.0)


def ce_paths(case):
    V, M, m = case['V'], case['M'], case['m']
    x = ce_inputs(case)
    tg = ce_targets(x['targets'], x['row_idx'], M)
    live = tg[:M if m is None else min(m, M)]
    p = {'ce:trips:' + ('partial' if V < 256 else ('one' if V == 256 else ('two_ragged' if V < 512 else 'many_ragged'))),
         'ce:m_dev:' + ('null' if m is None else ('zero' if m == 0 else ('inside' if m < M else
                                                                           ('equal' if m == M else 'above')))),
         'ce:row_idx:' + ('perm' if case['perm'] else 'null'), 'ce:logits:' + case['logits'], 'ce:gscale:' + case['g'],
         'ce:ld>V' if case['ld'] > V else 'ce:ld=V', 'ce:rows:one' if M == 1 else 'ce:rows:several'}
    if (live == CE_IGNORE).any():
        p.add('ce:ignored_target:' + case['call'])
    if (live == 0).any():
        p.add('ce:target:first')
    if (live == V - 1).any():
        p.add('ce:target:last')
    return p


# ================================================================ tell_sum_f32
def sum_f32(x, n, m, out0, accumulate, dt=F64, mutant=None):
    """out[0] = (accumulate ? out0 : 0) + sum of x[:min(n, *m_dev)].  fp32: thread t of 1024 adds x[t], x[t + 1024], ...; each
    of the 16 waves folds; the 16 sums are added left to right"""
    ne = n if m is None or mutant == 'sum_m_dev_ignored' else min(m, n)
    ne = max(ne, 0)

    def run(dt):
        xs = np.asarray(x, dt)[:ne]
        trips = max(-(-ne // 1024), 1)
        p = np.zeros(trips * 1024, dt)
        p[:ne] = xs
        acc = _sum(p.reshape(trips, 1024), 0, dt) if dt is F32 else p.reshape(trips, 1024).sum(0)
        if mutant == 'sum_threads_past_512_dropped':
            acc[512:] = 0
        t = _sum(wave_fold(acc.reshape(16, 64), dt), 0, dt) if dt is F32 else acc.sum()
        acc_flag = accumulate and mutant != 'sum_accumulate_ignored'
        return np.array([(dt(out0) + t) if acc_flag else t], dt).astype(dt)
    S = (abs(float(out0)) if accumulate else 0.0) + np.abs(np.asarray(x, F64)[:max(min(n, n if m is None else m), 0)]).sum()
    k = float(-(-ne // 1024) + 6 + 16 + 1)
    return dict(out=Out(run(dt), np.array([S]), dtype='float32', group=None, k=k), out_bits=Out(run(F32)))


SUM = [dict(id='n%d_%s_acc%d' % (n, 'null' if m is None else 'cnt%d' % m, a) + ('_cancel' if c else ''), n=n, m=m, acc=a,
            cancel=c, mutants=mu) for n, m, a, c, mu in (
    (0, None, 1, False, ()), (1, None, 0, False, ()), (63, 0, 0, False, ('sum_m_dev_ignored',)),
    (1023, None, 1, False, ('sum_threads_past_512_dropped', 'sum_accumulate_ignored')),
    (1024, 700, 0, True, ('sum_m_dev_ignored', 'sum_threads_past_512_dropped')),
    (1025, 4000, 1, True, ('sum_threads_past_512_dropped',)), (5000, None, 0, True, ('sum_threads_past_512_dropped',)))]


def sum_inputs(case):
    def make():
        r, n = _rng('sum', case['id']), max(case['n'], 1)
        x = r.standard_normal(n)
        if case['cancel']:                          # large values that cancel in pairs, small ones that must survive
            big = r.standard_normal(n // 2) * 1000.0
            x[:n // 2 * 2:2] += big
            x[1:n // 2 * 2:2] -= big
        return dict(x=np.asarray(x, F32), out0=float(np.float32(r.standard_normal())))
    return cached(('sum_in', case['id']), make)


def sum_case(case, dt=F64, mutant=None):
    x = sum_inputs(case)
    return sum_f32(x['x'], case['n'], case['m'], x['out0'], case['acc'], dt, mutant)


def sum_paths(case):
    n, m = case['n'], case['m']
    return {'sum:n:' + ('zero' if n == 0 else ('one' if n == 1 else ('partial_wave' if n < 64 else (
        'ragged' if n < 1024 else ('one_trip' if n == 1024 else ('second_trip:one_thread' if n == 1025 else 'many_trips')))))),
        'sum:m_dev:' + ('null' if m is None else ('zero' if m == 0 else ('below' if m < n else 'above'))),
        'sum:acc%d' % case['acc'], 'sum:cancel' if case['cancel'] else 'sum:plain'}


# ================================================================ tell_embed_gather_step / tell_embed_lookup_step
STEP_CUT = (20, 50, 90, 140)
STEP_DIMS = (8, 16, 64, 1968)
STEP_PAD = 1
STEP_POS_ROWS = 12


def step_bands(case):
    """-> lo, hi, dim, off per band, ktot.  One band: 16 columns at offset 8 of 88; 3 bands: 8 + 16 + 64 = 88; 4: 2056"""
    nb = case['nb']
    if nb == 1:
        return (0,), (STEP_CUT[0],), (16,), (8,), 88
    dim = STEP_DIMS[:nb]
    off = tuple(int(v) for v in np.cumsum((0,) + dim[:-1]))
    return (0,) + STEP_CUT[:nb - 1], STEP_CUT[:nb], dim, off, int(sum(dim))


def embed_gather_step(ids, tables, bands, pos_table, pos_rows, pos_pad, start_pos, step, mutant=None):
    """cat [M, ktot] bf16: the token's table row in its band's columns, zeros elsewhere; pos_out [M, E] fp32: the sinusoid
    row pad -> pos_pad, else pos_pad + 1 + start_pos + step, clamped to pos_rows - 1.  Both exact"""
    lo, hi, dim, off, ktot = bands
    ids, pos_table = np.asarray(ids), np.asarray(pos_table, F32)
    M, E = ids.size, pos_table.shape[1]
    cat = np.zeros((M, ktot), F32)
    for m_, id_ in enumerate(ids):
        band = [b for b in range(len(lo)) if lo[b] <= id_ < hi[b]]
        if band:
            b = band[-1]
            c0 = 0 if mutant == 'step_band_offset_dropped' else off[b]
            cat[m_, c0:c0 + dim[b]] = tables[b][id_ - lo[b]]
        elif mutant == 'step_unknown_id_reads_row0':
            cat[m_, off[0]:off[0] + dim[0]] = tables[0][0]
    pos = np.minimum(np.where(ids == pos_pad, pos_pad, pos_pad + 1 + start_pos + step), pos_rows - 1)
    pos_out = pos_table[pos].copy()
    if mutant == 'step_second_trip_dropped':
        cat[:, 2048:], pos_out[:, 1024:] = SENTINEL, SENTINEL
    return dict(cat=Out(cat, dtype='bfloat16'), pos_out=Out(pos_out))


def embed_lookup_step(ids, table, pos_table, pos_rows, pos_pad, start_pos, step, dt=F64, mutant=None):
    """out [M, E] bf16 = table[id] + pos_table[pos]; an id outside [0, V) adds nothing"""
    ids, table, pos_table = np.asarray(ids), np.asarray(table, dt), np.asarray(pos_table, dt)
    known = (ids >= 0) & (ids < table.shape[0])
    a = np.where(known[:, None], table[np.where(known, ids, 0)], dt(0))
    if mutant == 'step_unknown_id_reads_row0':
        a = table[np.where(known, ids, 0)]
    pos = np.minimum(np.where(ids == pos_pad, pos_pad, pos_pad + 1 + start_pos + step), pos_rows - 1)
    out = (a + pos_table[pos]).astype(dt)
    if mutant == 'step_second_trip_dropped':
        out[:, 1024:] = SENTINEL
    S = np.abs(np.asarray(a, F64)) + np.abs(np.asarray(pos_table[pos], F64))
    return dict(out=Out(out, S, dtype='bfloat16', group=None, k=1.0))


# M, bands, E, ids (see step_inputs), start_pos, step: the device counter registered with tell_set_pos_step_ptr (None: none)
STEP = [
    dict(id='m1_b1_e4', M=1, nb=1, E=4, ids='edge', start=0, step=None, mutants=('step_band_offset_dropped',)),
    dict(id='m5_b3_e1020', M=5, nb=3, E=1020, ids='low_edges', start=2, step=None,
         mutants=('step_band_offset_dropped', 'step_unknown_id_reads_row0')),
    dict(id='m5_b4_e1024', M=5, nb=4, E=1024, ids='high_edges', start=0, step=None, mutants=('step_second_trip_dropped',)),
    dict(id='m5_b3_e1028_clamp', M=5, nb=3, E=1028, ids='low_edges', start=40, step=None, mutants=('step_second_trip_dropped',)),
    dict(id='m5_b3_e4_counter', M=5, nb=3, E=4, ids='high_edges', start=2, step=3, mutants=()),
]


def step_inputs(case):
    def make():
        r, nb, E = _rng('step', case['id']), case['nb'], case['E']
        lo, hi, dim, off, ktot = step_bands(case)
        c = STEP_CUT
        ids = {'edge': [c[0] - 1], 'low_edges': [0, c[0] - 1, c[0], STEP_PAD, hi[-1] + 5],
               'high_edges': [c[1] - 1, c[1], hi[-1] - 1, hi[-1], c[0]]}[case['ids']]
        return dict(ids=np.array(ids, np.int64), tables=[store(r.standard_normal((hi[b] - lo[b], dim[b])), 'bfloat16')
                                                         for b in range(nb)],
                    pos_table=np.asarray(r.standard_normal((STEP_POS_ROWS, E)), F32),
                    table=np.asarray(r.standard_normal((hi[-1], E)), F32))
    return cached(('step_in', case['id']), make)


def step_case(case, dt=F64, mutant=None):
    x = step_inputs(case)
    res = embed_gather_step(x['ids'], x['tables'], step_bands(case), x['pos_table'], STEP_POS_ROWS, STEP_PAD, case['start'],
                            case['step'] or 0, mutant)
    res.update(embed_lookup_step(x['ids'], x['table'], x['pos_table'], STEP_POS_ROWS, STEP_PAD, case['start'],
                                 case['step'] or 0, dt, mutant))
    return res


def step_paths(case):
    x, (lo, hi, dim, off, ktot) = step_inputs(case), step_bands(case)
    E, ids = case['E'], x['ids']
    p = {'step:bands%d' % case['nb'], 'step:ktot:' + ('second_trip' if ktot > 2048 else 'one_trip'),
         'step:E:' + ('second_trip' if E > 1024 else ('whole_trip' if E == 1024 else 'ragged')),
         'step:counter:' + ('none' if case['step'] is None else 'registered')}
    if (ids == STEP_PAD).any():
        p.add('step:id:pad')
    if ((ids < 0) | (ids >= hi[-1])).any():
        p.add('step:id:outside_every_band')
    if STEP_PAD + 1 + case['start'] + (case['step'] or 0) >= STEP_POS_ROWS:
        p.add('step:pos:clamped')
    if off[0] > 0:
        p.add('step:band_not_at_column0')
    return p
