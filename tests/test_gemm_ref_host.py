"""tests/gemm_ref.py on the CPU: the exactness invariants of every entry of its case table, and mutants of the reference
that the comparison of tests/test_gpu_gemm.py must reject."""
import pytest
import torch

import gemm_ref as ref

F32, BF16 = torch.float32, torch.bfloat16
IDS = [c['id'] for c in ref.CASES]


# ---------------------------------------------------------------- (a) exactness invariants
@pytest.mark.parametrize('case', ref.CASES, ids=IDS)
def test_every_intermediate_stays_exact_and_the_shape_meets_the_abi(case):
    M, N, K = ref.case_shape(case, 256)
    a = ref.case_amplitude(case, 256)
    vec = 8 if case['in_dtype'] == BF16 else 4
    assert K > 0 and K % vec == 0 and (K + case['lda_pad']) % vec == 0 and (K + case['ldb_pad']) % vec == 0
    assert case['ldc_pad'] > 0                                       # every output is a view with ldc > N
    assert case['plan'].split('<')[0] == case['kernel'].split('<')[0]
    for name, e in case['epis']:
        e = ref.resolve(e, M)
        if case['wide']:
            assert (e['bias_mode'], e['act'], e['alpha'], e['accumulate']) == (0, 0, 1.0, False)
            assert ref.intermediate_bound(K, a, e, wide=True) < ref.LIMIT_WIDE
            assert 2 * a * a >= 1 << 22 and a >= 1 << 10             # products of 22 bits from operands of 11
        elif e['act'] == 2:
            al = ref.case_gelu_alpha(case, 256)
            assert al == 2.0 ** round(__import__('math').log2(al)) and al <= 1.0
            assert ref.intermediate_bound(K, a, dict(e, alpha=1.0)) < ref.LIMIT
        else:
            assert ref.intermediate_bound(K, a, e) < ref.LIMIT, name
        assert e['m_dev'] is None or 0 <= e['m_dev'] <= M
    assert ref.amplitude(128, 1) == 255 and 128 * 255 * 255 < ref.LIMIT      # K <= 128, headroom 1: all 8 mantissa bits


SMALL = [c for c in ref.CASES if ref.case_shape(c)[0] * ref.case_shape(c)[1] <= 2050 * 2048]


@pytest.mark.parametrize('case', SMALL, ids=[c['id'] for c in SMALL])
def test_fp32_float64_and_int64_products_agree_bit_for_bit(case):
    M, N, K = ref.case_shape(case)
    A, B, a = ref.operands(M, N, K, case['in_dtype'], case['seed'], wide=case['wide'])
    assert float(A.float().abs().max()) <= a and torch.equal(A.float(), A.float().round())
    r64 = ref.product(A, B, how='float64')
    assert torch.equal(r64, ref.product(A, B, how='int64')) and torch.equal(r64, ref.product(A, B, how='float32'))
    assert float(r64.abs().max()) < (ref.LIMIT_WIDE if case['wide'] else ref.LIMIT // ref.HEADROOM + 1)


def test_most_outputs_need_a_real_bf16_rounding():
    A, B, _ = ref.operands(512, 512, 128)
    r = ref.product(A, B)
    assert float((r.to(BF16).double() != r).double().mean()) > 0.9


# ---------------------------------------------------------------- (b) mutants of the reference
M_, N_, K_ = 200, 136, 72
E_ = ref.epi(bias_mode=1, alpha=0.5, accumulate=True, m_dev=150)


def _base():
    A, B, _ = ref.operands(M_, N_, K_)
    side = ref.side_inputs(M_, N_, BF16)
    return A, B, side, ref.product(A, B)


def _rejected(got, want, rows=None, cols=None):
    """the comparison rejects the mutant, and the mutant differs only inside rows x cols -> share of elements that differ"""
    msg = ref.mismatch(got, want)
    assert msg is not None and 'differ, first at' in msg
    bad = got != want
    inside = torch.zeros_like(bad)
    inside[rows if rows is not None else slice(None), cols if cols is not None else slice(None)] = True
    assert not bool((bad & ~inside).any())
    return float(bad[inside].float().mean())


def test_reference_equals_itself():
    A, B, side, acc = _base()
    want = ref.expected(acc, BF16, E_, side, side['prev'])
    assert ref.mismatch(want.clone(), want) is None
    assert torch.equal(want[150:], side['prev'][150:])


def test_mutant_last_k_chunk_dropped_in_the_last_row_tile():
    A, B, side, acc = _base()
    m0 = 192                                                         # last 64-row tile of 200 rows
    mut = acc.clone()
    mut[m0:] -= A[m0:, K_ - 8:].double() @ B[:, K_ - 8:].double().t()
    e = ref.epi(bias_mode=1, alpha=0.5)
    share = _rejected(ref.expected(mut, BF16, e, side), ref.expected(acc, BF16, e, side), rows=slice(m0, None))
    assert share > 0.9


def test_mutant_bias_shifted_by_four_columns():
    A, B, side, acc = _base()
    e = ref.epi(bias_mode=1)
    mut = dict(side, bias_n=torch.roll(side['bias_n'], 4))
    assert _rejected(ref.expected(acc, BF16, e, mut), ref.expected(acc, BF16, e, side)) > 0.5


def test_mutant_m_dev_one_too_large():
    A, B, side, acc = _base()
    got = ref.expected(acc, BF16, dict(E_, m_dev=151), side, side['prev'])
    assert _rejected(got, ref.expected(acc, BF16, E_, side, side['prev']), rows=slice(150, 151)) > 0.9


def test_mutant_accumulate_reads_the_neighbouring_row():
    A, B, side, acc = _base()
    e = ref.epi(accumulate=True)
    got = ref.expected(acc, F32, e, side, torch.roll(side['prev'].float(), 1, 0))
    assert _rejected(got, ref.expected(acc, F32, e, side, side['prev'].float())) > 0.9


TRUNCATION_SHARE = (0.40, 0.55)      # half of the outputs that need a rounding round up under nearest-even, truncation
                                     # never does; the share found here is 0.4937


def test_mutant_truncation_instead_of_nearest_even():
    A, B, side, acc = _base()
    want = ref.expected(acc, BF16, ref.epi(), side)
    bits = acc.float().view(torch.int32) & ~0xFFFF
    got = bits.view(F32).to(BF16)                                    # exact: the low 16 bits are gone
    share = _rejected(got, want)
    print('truncation differs from nearest-even in %.4f of the elements' % share)
    assert TRUNCATION_SHARE[0] < share < TRUNCATION_SHARE[1]


def test_mutant_output_transposed_within_one_block():
    A, B, side, acc = _base()
    want = ref.expected(acc, BF16, ref.epi(), side)
    got = want.clone()
    got[64:96, 32:64] = want[64:96, 32:64].t()
    assert _rejected(got, want, rows=slice(64, 96), cols=slice(32, 64)) > 0.9


def test_dropout_residual_reference_rounds_twice():
    """bf16(res + bf16(2 (lin + bias) keep)): dropped elements are the residual, bit for bit"""
    A, B, side, acc = _base()
    keep = (torch.arange(M_ * N_).view(M_, N_) % 2).float()
    out = ref.expected_dropout_residual(acc, side['bias_n'], side['res'], keep, 0.5)
    assert torch.equal(out[keep == 0], side['res'][keep == 0])
    lin = ((acc + side['bias_n'].double()) * 2).to(BF16).double()
    assert torch.equal(out[keep == 1], (side['res'].double() + lin)[keep == 1].to(BF16))
