"""GPU parity tests of the HIP ops (through the C ABI) against the CPU oracle.
Run on the MI355X box:  python -m pytest tests -m gpu
fp32 mode: tight tolerances (f32 MFMA == fmaf chain).  bf16 mode: bf16-level tolerances."""
import math

import numpy as np
import os
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    yield
    torch.cuda.synchronize()


def tol(dtype):
    return dict(rtol=2e-4, atol=2e-5) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)


def close(a, b, dtype=torch.float32, scale=1.0, **kw):
    a, b = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    if dtype == torch.float32:
        t = tol(dtype)
        t['atol'] *= scale
        t.update(kw)
        torch.testing.assert_close(a, b, **t)
    else:
        # bf16 compute: compare in norm (relative Frobenius error) + a loose element-wise bound
        assert a.shape == b.shape, (a.shape, b.shape)
        denom = b.norm().item() + 1e-6
        rel = (a - b).norm().item() / denom
        assert rel < kw.get('rtol', 3e-2), 'relative error %.4g' % rel
        bound = 0.08 * (b.abs().max().item() + 1e-6) * max(scale, 1.0) ** 0.5 + 1e-3
        assert (a - b).abs().max().item() < bound, ((a - b).abs().max().item(), bound)


def check_fx(fx, key, got, dtype, scale=1.0, **kw):
    """compare with a fixture entry, stored either in full ('out') or subsampled ('sub')"""
    import seeded
    if key in fx.get('out', {}):
        close(got, fx['out'][key], dtype, scale, **kw)
    else:
        close(torch.from_numpy(seeded.subsample(got.detach().float().cpu().numpy())), fx['sub'][key], dtype,
              scale, **kw)


DTYPES = [torch.float32, torch.bfloat16]


# ------------------------------------------------------------------ GEMM
@pytest.mark.parametrize('M,N,K', [(64, 64, 64), (96, 200, 72), (1024, 1024, 512), (496, 1024, 512),
                                   (2, 1024, 300), (5000, 128, 40), (2048, 2304, 130), (1000, 1000, 8192)])
def test_gemm_kmajor_forms(M, N, K):
    """tell_gemm_bf16: TN (wgrad) and NN (dgrad) read K-major operands in place (ds_read_b64_tr_b16)."""
    from tell_amd import ops
    g = torch.Generator().manual_seed(M * 13 + N + K)
    Mp, Np = (M + 7) // 8 * 8, (N + 7) // 8 * 8
    a_km = torch.zeros(K, Mp).bfloat16()
    a_km[:, :M] = torch.randn(K, M, generator=g).bfloat16()
    b_kn = torch.zeros(K, Np).bfloat16()
    b_kn[:, :N] = torch.randn(K, N, generator=g).bfloat16()
    ad, bd = a_km.to(DEV), b_kn.to(DEV)
    ref = a_km[:, :M].float().t() @ b_kn[:, :N].float()
    # TN, fp32 output accumulated onto ones (the fused wgrad form)
    out = torch.ones(M, N, device=DEV)
    asum = torch.full((M,), 2.0, device=DEV)
    ops.gemm_tn(ad[:, :M], bd[:, :N], out=out, accumulate=True, alpha=0.5, asum=asum, asum_scale=0.25)
    close(out, 0.5 * ref + 1, torch.bfloat16, scale=math.sqrt(K))
    close(asum, 2.0 + 0.25 * a_km[:, :M].float().sum(0), torch.float32, scale=math.sqrt(K))   # fused bias gradient
    # TN, bf16 output
    out2 = ops.gemm_tn(ad[:, :M], bd[:, :N])
    assert out2.dtype == torch.bfloat16
    close(out2, ref, torch.bfloat16, scale=math.sqrt(K))
    # NN: x[M2,K] @ b_kn[K,N]; K not a multiple of 8 -> zero padded columns in x
    M2 = 200
    Kp = (K + 7) // 8 * 8
    x = torch.zeros(M2, Kp).bfloat16()
    x[:, :K] = torch.randn(M2, K, generator=g).bfloat16()
    ref2 = x[:, :K].float() @ b_kn[:, :N].float()
    out3 = ops.gemm_nn(x.to(DEV), bd[:, :N])
    close(out3, ref2, torch.bfloat16, scale=math.sqrt(K))
    mdev = torch.tensor([M2 // 2], dtype=torch.int32, device=DEV)
    out4 = torch.full((M2, N), 3.0, device=DEV, dtype=torch.bfloat16)
    ops.gemm_nn(x.to(DEV), bd[:, :N], out=out4, m_dev=mdev)
    close(out4[:M2 // 2], ref2[:M2 // 2], torch.bfloat16, scale=math.sqrt(K))
    assert (out4[M2 // 2:] == 3).all()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('M,N,K', [(64, 64, 64), (130, 70, 96), (512, 1024, 1024), (37, 5002, 128),
                                   (1000, 48, 1024), (300, 300, 2048), (2048, 2048, 512),
                                   (4096, 4096, 256), (5000, 6200, 128), (8192, 4096, 320),
                                   (8192, 3072, 128)])   # 128x128 / 256x256 / 256x192 direct-to-LDS tiles, ragged
def test_gemm_nt(dtype, M, N, K):
    from tell_amd import ops
    g = torch.Generator().manual_seed(M * 7 + N)
    a = torch.randn(M, K, generator=g)
    b = torch.randn(N, K, generator=g)       # asymmetric operands -> detects transposed outputs
    bias = torch.randn(N, generator=g)
    ad, bd = a.to(DEV, dtype), b.to(DEV, dtype)
    ref = (ad.float().cpu() @ bd.float().cpu().t())
    out = ops.gemm(ad, bd, out_dtype=torch.float32)
    close(out, ref, dtype, scale=math.sqrt(K))
    out2 = ops.gemm(ad, bd, bias=bias.to(DEV), bias_mode=1, act=1, alpha=0.5)
    close(out2, torch.relu((ref + bias) * 0.5), dtype, scale=math.sqrt(K))
    out3 = ops.gemm(ad, bd, out_dtype=torch.float32, bias=torch.arange(M, dtype=torch.float32, device=DEV),
                    bias_mode=2, act=2)
    close(out3, torch.nn.functional.gelu(ref + torch.arange(M, dtype=torch.float32)[:, None]), dtype,
          scale=math.sqrt(K))
    acc = torch.ones(M, N, device=DEV)
    ops.gemm(ad, bd, out=acc, accumulate=True)
    close(acc, ref + 1, dtype, scale=math.sqrt(K))
    # act 4: relu(result + residual) - the tail of a residual block with its BatchNorm folded into the weights
    res = torch.randn(M, N, generator=g)
    resd = res.to(DEV, dtype)
    out5 = ops.gemm(ad, bd, bias=bias.to(DEV), bias_mode=1, act=4, aux=resd)
    close(out5, torch.relu(ref + bias + resd.float().cpu()), dtype, scale=math.sqrt(K))
    mdev = torch.tensor([M // 2], dtype=torch.int32, device=DEV)
    part = torch.full((M, N), 7.0, device=DEV)
    ops.gemm(ad, bd, out=part, m_dev=mdev)
    close(part[:M // 2], ref[:M // 2], dtype, scale=math.sqrt(K))
    assert (part[M // 2:] == 7).all()


@pytest.mark.parametrize('M,N,K', [(4096, 4096, 64), (4096, 4096, 128), (4096, 4096, 192), (8192, 2048, 320),
                                   (2048, 8192, 1024)])
def test_gemm_pingpong_kernel(M, N, K):
    """gemm_nt_pp2_kernel / gemm_nt_pp_kernel (whole rounds of full 256x256 bf16 tiles; the resident form is the default): K-tile counts 1, 2, 3, 5, 16 walk the prologue /
    steady state / tail of the counted-vmcnt pipeline; every epilogue form; repeated launches must be bit-identical
    (a staging race shows up as run-to-run differences long before it shows up as a tolerance failure)."""
    from tell_amd import ops
    g = torch.Generator().manual_seed(M + 3 * N + K)
    a = torch.randn(M, K, generator=g).bfloat16()
    b = torch.randn(N, K, generator=g).bfloat16()
    bias_n = torch.randn(N, generator=g)
    bias_m = torch.randn(M, generator=g)
    ad, bd = a.to(DEV), b.to(DEV)
    ref = a.float() @ b.float().t()
    out = ops.gemm(ad, bd)
    assert out.dtype == torch.bfloat16
    close(out, ref, torch.bfloat16, scale=math.sqrt(K))
    assert (out.float().cpu() - ref).norm() / ref.norm() < 4e-3          # bf16 output rounding only (2^-9 per element)
    # the same product through a lockstep kernel (ragged M keeps it off the ping-pong path): identical k order per
    # output element is not guaranteed, so compare with the tolerance, not bitwise
    out_small = ops.gemm(ad[:M - 8], bd)
    close(out[:M - 8], out_small.float().cpu(), torch.bfloat16, scale=math.sqrt(K))
    out2 = ops.gemm(ad, bd, bias=bias_n.to(DEV), bias_mode=1, act=2, alpha=0.5)
    close(out2, torch.nn.functional.gelu((ref + bias_n) * 0.5), torch.bfloat16, scale=math.sqrt(K))
    out3 = ops.gemm(ad, bd, bias=bias_m.to(DEV), bias_mode=2, act=1)
    close(out3, torch.relu(ref + bias_m[:, None]), torch.bfloat16, scale=math.sqrt(K))
    for _ in range(4):
        assert torch.equal(ops.gemm(ad, bd), out)
        assert torch.equal(ops.gemm(ad, bd, bias=bias_n.to(DEV), bias_mode=1, act=2, alpha=0.5), out2)
    # the library itself says which kernel these calls ran on (and that the ragged one did not)
    from tell_amd import hip

    def plan(x, y, o):
        return hip.query('tell_gemm_nt_plan', x, x.stride(0), y, y.stride(0), o, o.stride(0), x.shape[0], y.shape[0],
                         x.shape[1], hip.BF16, hip.BF16, None, 0, 0, None, 1.0, 0, None)
    # (K a multiple of 128: the four-wave kernel of round 4, csrc/gemm_q4.hip; TELL_GEMM_Q4=0 / TELL_GEMM_PP2=0 select the others)
    assert plan(ad, bd, out) in ('gemm_nt_q4_kernel<bf16,256,256>', 'gemm_nt_pp2_kernel<bf16,256,256>', 'gemm_nt_pp_kernel<bf16,256,256>')
    if K % 128 == 0 and hip.get_option('gemm_q4') == 1:
        assert plan(ad, bd, out) == 'gemm_nt_q4_kernel<bf16,256,256>'
    assert plan(ad[:M - 8], bd, out_small).startswith('gemm_nt_glds_kernel<bf16,')


def test_gelu_launch_matches_torch_and_the_gemm_epilogue():
    """tell_gelu (exact-erf GELU as its own bf16 launch, in place) against torch's erf GELU, and against act 2 of the GEMM
    epilogue on the same pre-activation (identical up to the one extra bf16 rounding of the pre-activation)."""
    from tell_amd import hip, ops
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(4096, 1024, generator=g) * 2.5).bfloat16()
    x[0, :8] = torch.tensor([0.0, -0.0, 9.0, -9.0, 40.0, -40.0, 1e-3, -1e-3]).bfloat16()
    xd = x.to(DEV)
    y = torch.empty_like(xd)
    hip.call('tell_gelu', xd, y, xd.numel(), hip.BF16)
    ref = torch.nn.functional.gelu(x.float())
    got = y.float().cpu()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max() <= 2.0 ** -8 * ref.abs().max() and (got - ref.bfloat16().float()).norm() / ref.norm() < 2e-3
    hip.call('tell_gelu', xd, xd, xd.numel(), hip.BF16)                      # in place
    assert torch.equal(xd, y)
    a = torch.randn(4096, 256, generator=g).bfloat16().to(DEV)
    w = torch.randn(1024, 256, generator=g).bfloat16().to(DEV)
    fused = ops.gemm(a, w, act=2)
    pre = ops.gemm(a, w)
    hip.call('tell_gelu', pre, pre, pre.numel(), hip.BF16)
    assert (fused.float() - pre.float()).norm() / fused.float().norm() < 4e-3


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('M,N,K', [(16384, 1024, 1024), (8192, 2048, 192), (4096, 4096, 64)])
def test_gemm_dropout_residual_epilogue(M, N, K, p):
    """tell_gemm_nt_dropout_residual (fairseq's  x = residual + dropout(out_proj(.)) / dropout(fc2(.))  inside the GEMM
    epilogue, transformer_faces_objects.py:352-353) against the tensor formulation with the mask rebuilt by the RNG
    restatement - i.e. the mask tell_layernorm_fwd draws for the same (seed, salt) - and the decline code for shapes the
    resident kernel does not take."""
    from tell_amd import hip, rng
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).bfloat16()
    b = torch.randn(N, K, generator=g).bfloat16()
    res = torch.randn(M, N, generator=g).bfloat16()
    bias = torch.randn(N, generator=g)
    ad, bd, rd, biasd = a.to(DEV), b.to(DEV), res.to(DEV), bias.to(DEV)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    rc = hip.call_rc('tell_gemm_nt_dropout_residual', ad, K, bd, K, biasd, rd, N, out, N, M, N, K, p, 17, 23)
    assert rc == 0
    lin = (ad.float() @ bd.float().t() + biasd).cpu()
    keep = torch.from_numpy(rng.keep_mask(17, 23, M * N, p)).view(M, N) / (1 - p) if p > 0 else 1.0
    ref = res.float() + (lin * keep).bfloat16().float()          # the kernel rounds the dropped-out product, then adds
    got = out.float().cpu()
    assert (got - ref).abs().max() <= 2.0 ** -7 * ref.abs().max() and (got - ref).norm() / ref.norm() < 3e-3
    if p > 0:                                                    # dropped elements are exactly the residual
        dropped = torch.from_numpy(rng.keep_mask(17, 23, M * N, p)).view(M, N) == 0
        assert 0.08 < dropped.float().mean() < 0.12
        assert torch.equal(got[dropped], res.float()[dropped])
    for _ in range(2):
        out2 = torch.empty_like(out)
        assert hip.call_rc('tell_gemm_nt_dropout_residual', ad, K, bd, K, biasd, rd, N, out2, N, M, N, K, p, 17, 23) == 0
        assert torch.equal(out2, out)
    # shapes it declines: ragged rows, fewer tiles than CUs
    assert hip.call_rc('tell_gemm_nt_dropout_residual', ad, K, bd, K, biasd, rd, N, out, N, M - 8, N, K, p, 17, 23) == 1
    assert hip.call_rc('tell_gemm_nt_dropout_residual', ad, K, bd, K, biasd, rd, N, out, N, 256, N, K, p, 17, 23) == 1


@pytest.mark.parametrize('env', [{'TELL_GEMM_PP2': '0'}, {'TELL_GEMM_PP2': '1'}, {'TELL_GEMM_PP2': '2', 'TELL_PP2_DYNAMIC': '1'},
                                 {'TELL_GEMM_PP2': '2', 'TELL_PP2_DYNAMIC': '0'}],
                         ids=['pp', 'pp2-multi-round', 'pp2-tile-queue', 'pp2-static'])
def test_gemm_kernel_variants_behind_switches(env):
    """The GEMM kernels that are not the default choice (the ping-pong family: fallback for K % 128 != 0)
    stay correct: each runs tools/probes/gemm_variant_check.py in a process of its own, which takes the switches from
    TELL_<KEY> when the library is loaded.  (The library reads its options per launch: tests/test_gpu_gemm.py switches
    kernels inside one process and asserts the plan label each time.)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ); e.update(env)
    e['TELL_GEMM_Q4'] = '0'                                   # (the default since round 4 takes the K % 128 == 0 shapes otherwise)
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'probes', 'gemm_variant_check.py')], env=e,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    want = 'gemm_nt_pp_kernel' if env['TELL_GEMM_PP2'] == '0' else 'gemm_nt_pp2_kernel'
    assert want in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize('env', [{}, {'TELL_GEMM_TILE': '8'}, {'TELL_Q4_DYNAMIC': '1'}, {'TELL_GEMM_Q4E': '2'},
                                 {'TELL_GEMM_Q4E': '2', 'TELL_Q4_DYNAMIC': '1'}, {'TELL_GEMM_Q4E': '0', 'TELL_Q4_VAR': '1'},
                                 {'TELL_GEMM_Q4E': '0', 'TELL_Q4_VAR': '2'},
                                 # the wrong-result timing ablations are not in the shipped library: their names change nothing
                                 {'TELL_Q4_ABL': '1', 'TELL_PP2_ABL': '1', 'TELL_DCB_ABL': '2', 'TELL_Q4E_VAR': '0'}],
                         ids=['default', 'partial-rounds', 'tile-queue', 'q4e-everywhere', 'q4e-tile-queue', 'schedule-1', 'schedule-2',
                              'ablation-names-inert'])
def test_gemm_q4_kernel(env):
    """gemm_nt_q4_kernel (csrc/gemm_q4.hip: four waves of 128x128, hand-placed K loop - the default for whole rounds of
    256x256 bf16 tiles with K % 128 == 0) through tools/probes/q4_check.py: 2 to 64 K tiles (first / steady-state / last
    body of the generated stream), 1 to 4 output tiles per resident workgroup incl. a last round with fewer tiles than
    workgroups (forced), every epilogue form, strided operands and output, repeated launches bit-identical; the
    alternative instruction schedules kept behind TELL_Q4_VAR; gemm_nt_q4e_kernel (csrc/gemm_q4e.hip: the previous tile's
    epilogue inside the K loop; default for act 0 / 1 with per-column bias and >= 2 tiles per workgroup, everywhere it
    applies - also with GELU and one tile per workgroup - under TELL_GEMM_Q4E=2); per-XCD tile counters (TELL_Q4_DYNAMIC=1)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ); e.update(env)
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'probes', 'q4_check.py')], env=e,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'ALL OK' in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert r.stdout.count('gemm_nt_q4_kernel') >= 9, r.stdout[-3000:]
    if not env:                                # variable-length shapes: 192 / 384 tiles (75 % of 1 / 2 rounds) are taken by q4
        # (qkv, N = 3072, has whole rounds of 256x192 tiles at those row counts and keeps that kernel)
        for shape in ('M=12288 N=1024 K=1024', 'M=12288 N=1024 K=4096', 'M=12288 N=2048 K=1024'):
            line = [ln for ln in r.stdout.splitlines() if shape in ln]
            assert line and line[0].startswith('gemm_nt_q4_kernel'), (shape, line)


def test_gemm_s64_kernel_is_bit_identical_to_the_general_body(monkeypatch):
    """gemm_nt_s64_kernel (csrc/gemm_s64.hip: the 64x64 direct-to-LDS tile with a K loop written for one wave per SIMD;
    taken from K = 1024 by the small-GEMM branch of tell_gemm_nt and by the implicit convolutions) against the general body
    it replaces (option gemm_s64 = 0, read per launch): same tiles, same MFMA order -> the same bits.  Plain products with bias /
    ReLU / ragged M and N / fp32 output / an accumulating epilogue, and the implicit 3x3 convolutions of ResNet layer3 /
    layer4 (stride 1 and 2, padding ring = out-of-range buffer offsets) with their BatchNorm-statistics epilogue."""
    from tell_amd import hip, ops
    g = torch.Generator().manual_seed(11)

    def both(fn):
        with hip.options(gemm_s64=0):
            a = fn()
        with hip.options(gemm_s64=1):
            b = fn()
        torch.cuda.synchronize()
        return a, b
    for M, N, K, kw in ((1024, 1024, 1024, {}), (1024, 496, 1024, {}), (1000, 1000, 4096, dict(act=1)),
                        (1536, 1024, 2048, dict(out_dtype=torch.float32)), (520, 72, 1088, {})):
        x = (torch.randn(M, K, generator=g) * 0.5).bfloat16().to(DEV)
        w = (torch.randn(N, K, generator=g) * 0.05).bfloat16().to(DEV)
        bias = torch.randn(N, generator=g).to(DEV)
        out = torch.empty(M, N, dtype=kw.get('out_dtype', torch.bfloat16), device=DEV)
        name = hip.query('tell_gemm_nt_plan', x, x.stride(0), w, w.stride(0), out, out.stride(0), M, N, K, hip.BF16,
                         hip.dt(out), bias, 1, 0, None, 1.0, 0, None)
        assert name.startswith('gemm_nt_s64_kernel'), (M, N, K, name)
        a, b = both(lambda: ops.gemm(x, w, bias=bias, bias_mode=1, act=kw.get('act', 0),
                                     **({'out_dtype': kw['out_dtype']} if 'out_dtype' in kw else {})).clone())
        assert torch.equal(a, b), (M, N, K)
        ref = torch.nn.functional.linear(x.float(), w.float(), bias)
        if kw.get('act'):
            ref = torch.relu(ref)
        assert ((b.float() - ref).norm() / ref.norm()).item() < 6e-3
    zero = torch.zeros(256, dtype=torch.uint8, device=DEV)
    B = 4
    for H, Cin, k, s, Cout in ((14, 256, 3, 1, 256), (28, 256, 3, 2, 256), (7, 512, 3, 1, 512), (14, 1024, 1, 1, 256)):
        p = k // 2
        OH = (H + 2 * p - k) // s + 1
        M = B * OH * OH
        x = torch.randn(B, H, H, Cin, generator=g).bfloat16().to(DEV)
        w = (torch.randn(Cout, k * k * Cin, generator=g) * 0.05).bfloat16().to(DEV)
        ws = torch.zeros(1 << 22, dtype=torch.float32, device=DEV)
        gamma, beta = torch.rand(Cout, generator=g).to(DEV) + 0.5, torch.randn(Cout, generator=g).to(DEV)

        def conv():
            y = torch.empty(M, Cout, dtype=torch.bfloat16, device=DEV)
            hip.call('tell_conv_bn_stats', x, w, y, B, H, H, Cin, k, k, s, p, OH, OH, Cout, 1e-5, 0.1, None, None, None, None,
                     None, zero)                                                   # the convolution alone
            z = torch.empty(M, Cout, dtype=torch.bfloat16, device=DEV)
            rm, rv = torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV)
            hip.call('tell_conv_bn_act', x, w, z, B, H, H, Cin, k, k, s, p, OH, OH, Cout, 1e-5, 0.1, gamma, beta, rm, rv, None,
                     1, ws, zero)                                                  # + statistics epilogue, BatchNorm, ReLU
            return y, torch.cat([z.float().reshape(-1), rm, rv])
        (ya, wa), (yb, wb) = both(conv)
        assert torch.equal(ya, yb) and torch.equal(wa, wb), (H, Cin, k, s)
        xr = x.float().permute(0, 3, 1, 2)
        wr = w.float().view(Cout, k, k, Cin).permute(0, 3, 1, 2)
        ref = torch.nn.functional.conv2d(xr, wr, stride=s, padding=p).permute(0, 2, 3, 1).reshape(M, Cout)
        assert ((yb.float() - ref).norm() / ref.norm()).item() < 6e-3


@pytest.mark.parametrize('dtype', DTYPES)
def test_lstm_cell_and_dot_attention_vs_torch(dtype):
    """csrc/lstm.hip against torch on CPU: nn.LSTMCell semantics from the two gate pre-activations, and the
    AttentionLayer core (masked softmax over the source, weighted sum) incl. the gradient w.r.t. the source states."""
    from tell_amd import ops
    g = torch.Generator().manual_seed(5)
    B, H, L, D = 5, 48, 23, 72
    g1, g2, c0 = torch.randn(B, 4 * H, generator=g), torch.randn(B, 4 * H, generator=g), torch.randn(B, H, generator=g)
    gh, gc = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g)
    a, b, c = [t.clone().to(dtype).float().requires_grad_(True) for t in (g1, g2, c0)]
    i, f, gg, o = (a + b).chunk(4, dim=1)
    cn = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    hn = torch.sigmoid(o) * torch.tanh(cn)
    (hn * gh + cn * gc).sum().backward()
    ad, bd, cd = [t.clone().to(DEV, dtype).requires_grad_(True) for t in (g1, g2, c0)]
    h2, c2 = ops.lstm_cell(ad, bd, cd)
    (h2.float() * gh.to(DEV) + c2.float() * gc.to(DEV)).sum().backward()
    close(h2, hn, dtype)
    close(c2, cn, dtype)
    close(ad.grad, a.grad, dtype, scale=2)
    close(bd.grad, a.grad, dtype, scale=2)
    close(cd.grad, c.grad, dtype, scale=2)
    src, x = torch.randn(L, B, D, generator=g), torch.randn(B, D, generator=g) * 0.3
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[1, 17:] = True
    mask[3, 5:] = True
    gctx = torch.randn(B, D, generator=g)
    sr, xr = src.clone().to(dtype).float().requires_grad_(True), x.clone().to(dtype).float().requires_grad_(True)
    sc = (sr * xr.unsqueeze(0)).sum(2).masked_fill(mask.t(), float('-inf'))
    pr = torch.softmax(sc, dim=0)
    ctx = (pr.unsqueeze(2) * sr).sum(0)
    (ctx * gctx).sum().backward()
    sd, xd = src.clone().to(DEV, dtype).requires_grad_(True), x.clone().to(DEV, dtype).requires_grad_(True)
    ctx2, pr2 = ops.dot_attention(xd, sd, mask.to(DEV).to(torch.uint8))
    (ctx2.float() * gctx.to(DEV)).sum().backward()
    close(ctx2, ctx, dtype)
    close(pr2, pr, torch.float32 if dtype == torch.float32 else dtype)
    close(xd.grad, xr.grad, dtype, scale=4)
    close(sd.grad, sr.grad, dtype, scale=4)
    y = ops.tanh(xd.detach().requires_grad_(True))
    close(y, torch.tanh(x.to(dtype).float()), dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_transpose_and_weight_norm(dtype):
    from tell_amd import ops
    x = torch.randn(70, 130)
    xt, plain = ops.transpose(x.to(DEV), out_dtype=dtype, want_plain=True)
    close(xt[:, :70], x.t(), dtype)
    close(plain, x, dtype)
    assert (xt[:, 70:] == 0).all()
    from oracle import functional as OF
    g = torch.rand(40, 1) + 0.5
    v = torch.randn(40, 24)
    gp = torch.nn.Parameter(g.to(DEV))
    vp = torch.nn.Parameter(v.to(DEV))
    import tell_amd
    tell_amd.set_compute_dtype(dtype)
    w, norms = ops.wn_weight(gp, vp)
    wt = ops.wn_weight_t(gp, vp)
    close(w, OF.weight_norm_weight(g, v), dtype)
    close(wt[:, :40], OF.weight_norm_weight(g, v).t(), dtype)
    close(norms, v.norm(dim=1))


@pytest.mark.parametrize('dtype', DTYPES)
def test_gehring_linear_golden(golden, dtype):
    import tell_amd
    from tell_amd import ops
    tell_amd.set_compute_dtype(dtype)
    fx = golden('gehring_linear')
    g = torch.nn.Parameter(fx['sd']['weight_g'].to(DEV))
    v = torch.nn.Parameter(fx['sd']['weight_v'].to(DEV))
    b = torch.nn.Parameter(fx['sd']['bias'].to(DEV))
    x = fx['in']['x'].to(DEV, dtype).requires_grad_(True)
    y = ops.wn_linear(x, g, v, b)
    y.backward(fx['in']['gy'].to(DEV, dtype))
    close(y, fx['out']['y'], dtype)
    close(x.grad, fx['out']['gx'], dtype)
    close(g.grad, fx['out']['g_weight_g'], dtype, scale=4)
    close(v.grad, fx['out']['g_weight_v'], dtype, scale=4)
    close(b.grad, fx['out']['g_bias'], dtype, scale=4)


@pytest.mark.parametrize('dtype', DTYPES)
def test_weight_norm_many_tensors_one_launch(dtype):
    """wn_prepare + deferred chain rule (one launch each over all GehringLinears) == the per-layer kernels, bit for bit,
    across more tensors than one launch carries (32) and ragged shapes."""
    import tell_amd
    from tell_amd import ops
    tell_amd.set_compute_dtype(dtype)
    torch.manual_seed(3)
    shapes = [(40, 24), (7, 130), (64, 64), (128, 1024)] * 9                     # 36 tensors
    gs = [torch.nn.Parameter((torch.rand(r, 1) + 0.5).to(DEV)) for r, _ in shapes]
    vs = [torch.nn.Parameter(torch.randn(r, c).to(DEV)) for r, c in shapes]
    xs = [torch.randn(16, c, device=DEV, dtype=dtype) for _, c in shapes]

    def run(batched):
        ops.clear_weight_cache()
        for p in gs + vs:
            p.grad = None
        if batched:
            ops.wn_prepare(list(zip(gs, vs)))
            ops.wn_defer(True)
        ws, outs = [], []
        for g, v, x in zip(gs, vs, xs):
            ws.append(ops.wn_weight(g, v))
            xr = x.clone().requires_grad_(True)
            y = ops.wn_linear(xr, g, v)
            y.backward(torch.ones_like(y))
            outs.append(xr.grad)
        ops.wn_defer(False)
        ops.wn_flush()
        return ws, outs, [p.grad.clone() for p in gs + vs]

    w0, dx0, g0 = run(False)
    w1, dx1, g1 = run(True)
    for (wa, na), (wb, nb) in zip(w0, w1):
        assert torch.equal(wa, wb) and torch.equal(na, nb)
    for a, b in zip(dx0 + g0, dx1 + g1):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dtype', DTYPES)
def test_glu_dropout_layernorm(dtype):
    import tell_amd
    from tell_amd import ops, rng
    tell_amd.manual_seed(123)
    h = torch.randn(6, 5, 64)
    hd = h.to(DEV, dtype).requires_grad_(True)
    y = ops.glu(hd)
    hc = hd.detach().float().cpu().requires_grad_(True)
    yr = torch.nn.functional.glu(hc, dim=-1)
    gy = torch.randn_like(yr)
    y.backward(gy.to(DEV, dtype))
    yr.backward(gy)
    close(y, yr, dtype)
    close(hd.grad, hc.grad, dtype)
    # dropout mask == numpy restatement of the device hash
    x = torch.ones(1000, device=DEV, dtype=dtype)
    yd = ops.dropout(x, 0.3, True, salt=77)
    mask = rng.keep_mask(123, 77, 1000, 0.3)
    close(yd, torch.from_numpy(mask) / 0.7, dtype)
    assert 0.6 < mask.mean() < 0.8
    # y = LN(res + dropout(x))
    C = 64
    xx, rr = torch.randn(10, 3, C), torch.randn(10, 3, C)
    gam = torch.nn.Parameter((torch.rand(C) + 0.5).to(DEV))
    bet = torch.nn.Parameter(torch.randn(C).to(DEV))
    for p in (0.0, 0.25):
        gam.grad = bet.grad = None
        xd = xx.to(DEV, dtype).requires_grad_(True)
        rd = rr.to(DEV, dtype).requires_grad_(True)
        tell_amd.manual_seed(5, salt=10)
        out = ops.layer_norm(xd, rd, gam, bet, 1e-5, p, training=True)
        keep = torch.from_numpy(rng.keep_mask(5, 11, 30 * C, p)).view(10, 3, C) / (1 - p) if p > 0 else 1.0
        xc = xd.detach().float().cpu().requires_grad_(True)
        rc = rd.detach().float().cpu().requires_grad_(True)
        gc = gam.detach().cpu().requires_grad_(True)
        bc = bet.detach().cpu().requires_grad_(True)
        ref = torch.nn.functional.layer_norm(rc + xc * keep, (C,), gc, bc, 1e-5)
        go = torch.randn_like(ref)
        out.backward(go.to(DEV, dtype))
        ref.backward(go)
        close(out, ref, dtype)
        close(xd.grad, xc.grad, dtype)
        close(rd.grad, rc.grad, dtype)
        close(gam.grad, gc.grad, dtype, scale=8)
        close(bet.grad, bc.grad, dtype, scale=8)


# ------------------------------------------------------------------ DynamicConv
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('K,T', [(3, 6), (7, 4), (31, 12), (15, 40)])
def test_dynamic_conv_golden(golden, dtype, K, T):
    """kernel vs what the REFERENCE produced (fixtures), incl. K > T."""
    import tell_amd
    from tell_amd import ops
    tell_amd.set_compute_dtype(dtype)
    fx = golden('dynconv_K%d_T%d' % (K, T))
    w = torch.nn.Parameter(fx['sd']['weight_linear.weight'].to(DEV))
    x = fx['in']['x'].to(DEV, dtype).requires_grad_(True)
    logits = ops.linear(x, w)
    y = ops.dynamic_conv(x, logits, 4, K)
    y.backward(fx['in']['gy'].to(DEV, dtype))
    check_fx(fx, 'y', y, dtype)
    check_fx(fx, 'gx', x.grad, dtype, scale=4)
    check_fx(fx, 'g_weight', w.grad, dtype, scale=8)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('K,T', [(3, 6), (31, 12)])
def test_lightweight_conv_golden(golden, dtype, K, T):
    """`decoder_conv_type: lightweight` (static taps per head) on the DynamicConv kernels vs what the REFERENCE's
    LightweightConv1dTBC produced, incl. K > T and the incremental (generation) path."""
    import tell_amd
    from tell_amd.modules import LightweightConv1dTBC
    tell_amd.set_compute_dtype(dtype)
    fx = golden('lightconv_K%d_T%d' % (K, T))
    m = LightweightConv1dTBC(64, K, padding_l=K - 1, num_heads=4, weight_softmax=True, weight_dropout=0.1).eval()
    m.load_state_dict(fx['sd'])
    m.to(DEV)
    x = fx['in']['x'].to(DEV, dtype).requires_grad_(True)
    m.weight.grad = torch.zeros_like(m.weight)             # gradient buffer the kernels accumulate into
    y = m(x)
    y.backward(fx['in']['gy'].to(DEV, dtype))
    check_fx(fx, 'y', y, dtype)
    check_fx(fx, 'gx', x.grad, dtype, scale=4)
    check_fx(fx, 'g_weight', m.weight.grad, dtype, scale=8)
    with torch.no_grad():
        st = {}
        inc = torch.cat([m(x[t:t + 1].detach(), incremental_state=st) for t in range(T)], dim=0)
    check_fx(fx, 'y_incremental', inc, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('T,K', [(32, 31), (32, 3), (32, 7), (32, 15), (5, 31), (100, 15)])
def test_dynamic_conv_full_size_dropconnect(dtype, T, K):
    """decoder shapes (B=16, C=1024, H=16, head width 64: the LDS-tiled kernels; T=100 takes the tiled forward and the
    wave-per-row backward, T < K the tap narrowing) with DropConnect, vs the oracle with the same mask."""
    import tell_amd
    from tell_amd import ops, rng
    from oracle import functional as OF
    B, C, H, p = 16, 1024, 16, 0.1
    g = torch.Generator().manual_seed(3)
    x = torch.randn(T, B, C, generator=g)
    lg = torch.randn(T, B, H * K, generator=g)
    xd = x.to(DEV, dtype).requires_grad_(True)
    ld = lg.to(DEV, dtype).requires_grad_(True)
    tell_amd.manual_seed(9, salt=100)
    y = ops.dynamic_conv(xd, ld, H, K, p, training=True)
    mask = torch.from_numpy(rng.keep_mask(9, 101, T * B * H * K, p)).view(T, B, H, K)
    xc = xd.detach().float().cpu().requires_grad_(True)
    lc = ld.detach().float().cpu().requires_grad_(True)
    ref = OF.dynamic_conv_apply(xc, OF.dynamic_conv_taps(lc, H, K, mask, p))
    gy = torch.randn(T, B, C, generator=g)
    y.backward(gy.to(DEV, dtype))
    ref.backward(gy)
    close(y, ref, dtype)
    close(xd.grad, xc.grad, dtype, scale=2)
    close(ld.grad, lc.grad, dtype, scale=2)


@pytest.mark.parametrize('T,B,K,p', [(32, 32, 31, 0.1), (32, 16, 3, 0.0), (17, 8, 15, 0.1), (5, 4, 31, 0.1), (32, 3, 7, 0.1)])
def test_dynconv_block_fused_forward(T, B, K, p):
    """tell_dynconv_block_fwd: GLU + tap logits + tap softmax + DropConnect + K-tap sum of the decoder's conv block
    (decoder_faces_objects.py:259-261, dynamic.py:300-336) in one launch.  gl must be what tell_glu_fwd writes, bit for
    bit; taps and y are checked against the oracle fed with that gl, fp32 logits (the kernel never rounds them) and the
    DropConnect mask of the RNG restatement; shapes it does not take are declined, not approximated."""
    from tell_amd import hip, rng
    from oracle import functional as OF
    E, H = 1024, 16
    g = torch.Generator().manual_seed(T * 100 + K)
    h1 = torch.randn(T * B, 2 * E, generator=g).bfloat16().to(DEV)
    wt = (torch.randn(H * K, E, generator=g) * 0.05).bfloat16().to(DEV)
    gl = torch.full((T * B, E), 7.0, dtype=torch.bfloat16, device=DEV)
    y = torch.empty_like(gl)
    taps = torch.empty(T * B * H, K, device=DEV)
    assert hip.call_rc('tell_dynconv_block_fwd', h1, wt, gl, y, taps, T, B, H, K, p, 9, 101) == 0
    gl_ref = torch.empty_like(gl)
    hip.call('tell_glu_fwd', h1, gl_ref, T * B, E, hip.BF16)
    assert torch.equal(gl, gl_ref)
    x = gl.float().cpu().view(T, B, E)
    logits = (gl.float() @ wt.float().t()).cpu().view(T, B, H * K)
    mask = torch.from_numpy(rng.keep_mask(9, 101, T * B * H * K, p)).view(T, B, H, K) if p > 0 else None
    w_ref = torch.softmax(logits.view(T, B, H, K), dim=-1)
    assert (taps.cpu().view(T, B, H, K) - w_ref).abs().max() < 2e-5
    ref = OF.dynamic_conv_apply(x, OF.dynamic_conv_taps(logits, H, K, mask, p))
    close(y.view(T, B, E), ref, torch.bfloat16)
    # the three-launch path on the same inputs (its logits pass through bf16): same mask, same numbers to that rounding
    lg16 = (gl @ wt.t())
    y3, taps3 = torch.empty_like(gl), torch.empty_like(taps)
    hip.call('tell_dynconv_fwd', gl, lg16, y3, taps3, T, B, H, K, 64, p, 9, 101, hip.BF16)
    assert (taps3 - taps).abs().max() < 2e-2 and (y3.float() - y.float()).norm() <= 1e-2 * y.float().norm()
    if p > 0:                                              # dropped taps are the same taps: zeros in y line up
        assert ((y3 == 0) == (y == 0)).float().mean() > 0.999
    # declined: longer captions, wider kernels, other widths
    assert hip.call_rc('tell_dynconv_block_fwd', h1, wt, gl, y, taps, 33, 1, H, K, p, 9, 101) == 1
    assert hip.call_rc('tell_dynconv_block_fwd', h1, wt, gl, y, taps, T, B, 8, K, p, 9, 101) == 1
    assert hip.call_rc('tell_dynconv_block_fwd', h1, wt, gl, y, taps, T, B, H, 33, p, 9, 101) == 1


# ------------------------------------------------------------------ attention
def _attn_case(dtype, T, B, E, H, S, kdim, use_mask, p, seed, has_bias=True):
    import tell_amd
    from tell_amd import ops, rng
    from oracle import functional as OF
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(T, B, E, generator=g) * 0.5
    k = torch.randn(S, B, E, generator=g)
    v = torch.randn(S, B, E, generator=g)
    bias_k = torch.randn(1, 1, E, generator=g)
    bias_v = torch.randn(1, 1, E, generator=g)
    mask = None
    if use_mask:
        mask = torch.rand(B, S, generator=g) < 0.3
    qd = q.to(DEV, dtype).requires_grad_(True)
    kd = k.to(DEV, dtype).requires_grad_(True)
    vd = v.to(DEV, dtype).requires_grad_(True)
    bk = torch.nn.Parameter(bias_k.to(DEV))
    bv = torch.nn.Parameter(bias_v.to(DEV))
    tell_amd.manual_seed(21, salt=40)
    md = mask.to(DEV).to(torch.uint8).contiguous() if mask is not None else None
    out = ops.attention(qd, kd, vd, md, bk if has_bias else None, bv if has_bias else None, H, True, p, training=True)
    # ---- reference: same math in fp32 on CPU, using the kernel's dropout mask
    qc = qd.detach().float().cpu().requires_grad_(True)
    kc = kd.detach().float().cpu().requires_grad_(True)
    vc = vd.detach().float().cpu().requires_grad_(True)
    bkc = bias_k.to(dtype).float().requires_grad_(True)
    bvc = bias_v.to(dtype).float().requires_grad_(True)
    hd = E // H
    S1 = S + (1 if has_bias else 0) + 1
    kk = torch.cat([kc] + ([bkc.expand(1, B, E)] if has_bias else []) + [torch.zeros(1, B, E)], 0)
    vv = torch.cat([vc] + ([bvc.expand(1, B, E)] if has_bias else []) + [torch.zeros(1, B, E)], 0)
    qh = qc.reshape(T, B * H, hd).transpose(0, 1)
    kh = kk.reshape(S1, B * H, hd).transpose(0, 1)
    vh = vv.reshape(S1, B * H, hd).transpose(0, 1)
    sc = torch.bmm(qh, kh.transpose(1, 2))
    if mask is not None:
        full = torch.cat([mask, torch.zeros(B, S1 - S, dtype=torch.bool)], 1)
        sc = sc.view(B, H, T, S1).masked_fill(full[:, None, None, :], float('-inf')).view(B * H, T, S1)
    pr = torch.softmax(sc, -1)
    if p > 0:
        keep = torch.from_numpy(rng.keep_mask(21, 41, B * H * T * S1, p)).view(B * H, T, S1) / (1 - p)
        pr = pr * keep
    ref = torch.bmm(pr, vh).transpose(0, 1).reshape(T, B, E)
    go = torch.randn(T, B, E, generator=g)
    out.backward(go.to(DEV, dtype))
    ref.backward(go)
    close(out, ref, dtype)
    close(qd.grad, qc.grad, dtype, scale=2)
    close(kd.grad, kc.grad, dtype, scale=2)
    close(vd.grad, vc.grad, dtype, scale=2)
    if has_bias:
        close(bk.grad, bkc.grad, dtype, scale=4)
        close(bv.grad, bvc.grad, dtype, scale=4)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('T,B,E,H,S,mask,p', [
    (3, 2, 64, 4, 6, True, 0.0),        # reduced dims (head_dim 16), like the fixtures
    (9, 2, 64, 4, 40, True, 0.2),
    (32, 4, 1024, 16, 49, False, 0.0),  # image context
    (32, 3, 1024, 16, 512, True, 0.1),  # article context, padding + dropout
    (32, 2, 1024, 16, 4, True, 0.0),    # faces
    (33, 2, 1024, 16, 64, True, 0.0),   # T not a multiple of 32 -> 2 query blocks
    (1, 5, 1024, 16, 100, True, 0.0),   # generation step
    (70, 2, 1024, 16, 130, True, 0.1),
    (160, 2, 1024, 16, 200, True, 0.1),  # >= 4 query blocks: shared 64-key-tile forward kernel
    (128, 1, 1024, 16, 64, False, 0.0),
    (130, 2, 1024, 16, 77, True, 0.1),   # odd key count (per-element dropout decisions), ragged query tail
])
def test_attention_core(dtype, T, B, E, H, S, mask, p):
    _attn_case(dtype, T, B, E, H, S, E, mask, p, seed=T * 131 + S)


@pytest.mark.parametrize('dtype', DTYPES)
def test_attention_self_no_extra_rows(dtype):
    """RoBERTa-style self attention: no bias row, no zero row, T = S = 128, padded keys."""
    import tell_amd
    from tell_amd import ops
    T = S = 128
    B, E, H = 2, 1024, 16
    g = torch.Generator().manual_seed(8)
    qkv = torch.randn(T, B, 3 * E, generator=g).to(DEV, dtype)
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[1, 100:] = True
    q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    out = ops.attention(q, k, v, mask.to(DEV).to(torch.uint8), None, None, H, has_zero=False)
    hd = E // H
    qc, kc, vc = [t.float().cpu().reshape(T, B * H, hd).transpose(0, 1) for t in (q, k, v)]
    sc = torch.bmm(qc, kc.transpose(1, 2)).view(B, H, T, S).masked_fill(mask[:, None, None, :], float('-inf'))
    ref = torch.bmm(torch.softmax(sc, -1).view(B * H, T, S), vc).transpose(0, 1).reshape(T, B, E)
    close(out, ref, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('tag', ['sep', 'same', 'nomask', 'empty'])
def test_mha_module_golden(golden, dtype, tag):
    import tell_amd
    from tell_amd.modules import MultiHeadAttention
    tell_amd.set_compute_dtype(dtype)
    fx = golden('mha_' + tag)
    kdim = int(fx['in']['kdim'])
    m = MultiHeadAttention(64, 4, kdim=kdim if kdim else 16, vdim=kdim if kdim else 16, dropout=0.1).eval()
    m.load_state_dict(fx['sd'])
    m.to(DEV)
    q = fx['in']['q'].to(DEV, dtype).requires_grad_(True)
    key = fx['in']['key'].to(DEV, dtype)
    mask = fx['in'].get('mask')
    y, w = m(q, key, key, key_padding_mask=mask.to(DEV) if mask is not None else None, need_weights=True)
    y.backward(fx['in']['gy'].to(DEV, dtype))
    close(y, fx['out']['y'], dtype)
    close(w, fx['out']['w'], dtype)
    close(q.grad, fx['out']['gq'], dtype, scale=2)
    import seeded
    for name, p in m.named_parameters():
        key_ = 'g_' + name
        if key_ in fx['out']:
            close(p.grad, fx['out'][key_], dtype, scale=8)
        elif key_ in fx.get('sub', {}):
            close(torch.from_numpy(seeded.subsample(p.grad.float().cpu().numpy())), fx['sub'][key_], dtype, scale=8)


# ------------------------------------------------------------------ embedder / adaptive softmax
@pytest.mark.parametrize('dtype', DTYPES)
def test_embedder_golden(golden, dtype):
    import tell_amd
    from tell_amd.build import build_embedder
    tell_amd.set_compute_dtype(dtype)
    fx = golden('embedder')
    emb = build_embedder(600, 32, (100, 300), init_size=8)
    emb.load_state_dict(fx['sd'], strict=False)
    emb.to(DEV)
    ids = fx['in']['ids'].to(DEV)
    y = emb({'roberta': ids})
    y.backward(fx['in']['gy'].to(DEV, dtype))
    close(y, fx['out']['y'], dtype, scale=4)
    for name, p in emb.named_parameters():
        check_fx(fx, 'g_' + name, p.grad, dtype, scale=16)
    st = {}
    inc = torch.cat([emb({'roberta': ids[:, t:t + 1]}, incremental_state=st) for t in range(ids.shape[1])], 1)
    close(inc, fx['out']['y_incremental'], dtype, scale=4)


@pytest.mark.parametrize('dtype', DTYPES)
def test_adaptive_softmax_golden(golden, dtype):
    import tell_amd
    from tell_amd.build import build_embedder
    from tell_amd.modules import AdaptiveLoss, AdaptiveSoftmax
    tell_amd.set_compute_dtype(dtype)
    fx = golden('adaptive_softmax')
    emb = build_embedder(600, 32, (100, 300))
    asm = AdaptiveSoftmax(600, 32, [100, 300], adaptive_inputs=emb.token_embedder_adaptive)
    asm.load_state_dict(fx['sd'], strict=False)
    asm.to(DEV)
    crit = AdaptiveLoss(1)
    x = fx['in']['x'].to(DEV, dtype).requires_grad_(True)
    loss, n = crit(asm, (x, None), fx['in']['target'].to(DEV))
    loss.backward()
    assert int(n) == fx['out']['sample_size']
    close(loss.reshape(1), fx['out']['loss'], dtype, rtol=1e-3 if dtype == torch.float32 else 2e-2)
    close(x.grad, fx['out']['gx'], dtype)
    import seeded
    for name, p in asm.named_parameters():
        if p.grad is None:
            continue
        k = 'g_' + name
        if k in fx['out']:
            close(p.grad, fx['out'][k], dtype, scale=8)
        elif k in fx.get('sub', {}):
            close(torch.from_numpy(seeded.subsample(p.grad.float().cpu().numpy())), fx['sub'][k], dtype, scale=8)
    loss2, n2 = crit(asm, (x.detach(), None), fx['in']['target2'].to(DEV))     # a band with no rows
    assert int(n2) == fx['out']['sample_size2']
    close(loss2.reshape(1), fx['out']['loss2'], dtype, rtol=1e-3 if dtype == torch.float32 else 2e-2)
    lp = asm.get_log_prob(x.detach())
    check_fx(fx, 'log_probs', lp, dtype, scale=4)
    tok, tlp = asm.greedy(x.detach())
    # full reference log-probs from the (golden-pinned) oracle on the same weights
    from oracle.build import build_embedder as o_emb
    from oracle.modules import AdaptiveSoftmax as OASM
    oasm = OASM(600, 32, [100, 300], o_emb(600, 32, (100, 300)).token_embedder_adaptive)
    oasm.load_state_dict({k: v for k, v in fx['sd'].items() if k in oasm.state_dict()}, strict=False)
    ref = oasm.get_log_prob(x.detach().float().cpu()).view(-1, 600)
    if dtype == torch.float32:
        assert torch.equal(tok.cpu().long().view(-1), ref.argmax(dim=1))
    close(tlp.view(-1), ref.max(dim=1).values, dtype, scale=4)


def test_grouped_wgrad_gemms_match_single_launches():
    """gemm_tn queued + flushed as grouped launches == the same products launched one by one, bit for bit (the K
    reduction order does not depend on the tile shape), over both output types, both tile shapes, ragged sizes, fused bias column sums and
    two products accumulating into ONE buffer (tied weights: must not share a launch)."""
    import tell_amd
    from tell_amd import ops
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(5)
    shapes = [(1024, 1024, 1024), (1024, 2048, 1024), (128, 2048, 512), (1568, 2048, 2048), (96, 200, 72),
              (1024, 496, 1024), (64, 64, 64), (2048, 1024, 4096), (4160, 520, 264)] * 4  # (K rows, M, N) x 36
    # (the last one is a long reduction: fp32 outputs of K >= 4096 take the 256x128-tile kernel, ragged edges included)
    probs = []
    for i, (K, M, N) in enumerate(shapes):
        a = torch.randn(K, M, device=DEV).bfloat16()
        b = torch.randn(K, N, device=DEV).bfloat16()
        probs.append((a, b, torch.float32 if i % 3 else torch.bfloat16, i % 2 == 0, i % 4 == 1))
    tied = torch.zeros(1024, 1024, device=DEV)

    def run(grouped):
        outs = []
        ops.wgrad_group_defer(grouped)
        try:
            for a, b, dt, acc, with_sum in probs:
                out = torch.full((a.shape[1], b.shape[1]), 0.5, device=DEV, dtype=dt) if acc else None
                asum = torch.full((a.shape[1],), 0.25, device=DEV) if with_sum else None
                o = ops.gemm_tn(a, b, out=out, out_dtype=dt, accumulate=acc, alpha=0.5, asum=asum, asum_scale=0.5)
                outs.append((o, asum))
            t = tied.clone()
            for a, b, *_ in probs[:9:8]:                       # two 1024 x 1024 products into the same buffer
                ops.gemm_tn(a, b, out=t, accumulate=True)
            outs.append((t, None))
        finally:
            ops.wgrad_group_defer(False)
        ops.wgrad_group_flush()
        return outs

    ref = run(False)
    got = run(True)
    for (o0, s0), (o1, s1) in zip(ref, got):
        assert torch.equal(o0, o1)
        if s0 is not None:            # the fused column sums fold in tile order: 64- and 128-row tiles differ in the last bits
            assert torch.allclose(s0, s1, rtol=1e-5, atol=1e-3)


def test_grouped_linear_matches_single_linears():
    """ops.grouped_linear (one launch forward, one for the input gradients) == one ops.linear per item: outputs and
    input gradients bit for bit, parameter gradients to fp32 rounding; row slices of a packed in_proj weight, scaling,
    missing bias, ragged row counts."""
    import tell_amd
    from tell_amd import ops
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(11)
    E = 1024
    packed_w = torch.nn.Parameter(torch.randn(3 * E, E, device=DEV) * 0.03)
    packed_b = torch.nn.Parameter(torch.randn(3 * E, device=DEV) * 0.1)
    ws = [torch.nn.Parameter(torch.randn(n, k, device=DEV) * 0.03) for n, k in ((E, E), (512, E), (E, 2048), (200, 72 * 8))]
    bs = [torch.nn.Parameter(torch.randn(w.shape[0], device=DEV) * 0.1) for w in ws]
    specs = [(packed_w, (0, E), packed_b, (0, E), 0.125), (ws[0], None, bs[0], None, 1.0), (ws[1], None, None, None, 1.0),
             (ws[2], None, bs[2], None, 0.5), (ws[3], None, bs[3], None, 1.0)]
    xs0 = [torch.randn(32, 32, E, device=DEV).bfloat16(), torch.randn(32, 32, E, device=DEV).bfloat16(),
           torch.randn(1024, E, device=DEV).bfloat16(), torch.randn(160, 2048, device=DEV).bfloat16(),   # (> 128 rows: not the split-K path)
           torch.randn(7, 3, 576, device=DEV).bfloat16()]
    gys = None

    def run(grouped):
        nonlocal gys
        for p in [packed_w, packed_b] + ws + bs:
            p.grad = None
        xs = [x.clone().requires_grad_(True) for x in xs0]
        if grouped:
            ys = ops.grouped_linear(xs, specs)
        else:
            ys = [ops.linear(x, w, b, rows=r, alpha=a, b_rows=br) for x, (w, r, b, br, a) in zip(xs, specs)]
        if gys is None:
            gys = [torch.randn_like(y) for y in ys]
        torch.autograd.backward(ys, gys)
        grads = [p.grad.clone() for p in [packed_w, packed_b] + ws + [b for b in bs if b.grad is not None]]
        return [y.detach() for y in ys], [x.grad for x in xs], grads

    y0, dx0, g0 = run(False)
    y1, dx1, g1 = run(True)
    for a, b in zip(y0 + dx0, y1 + dx1):
        assert torch.equal(a, b)
    for a, b in zip(g0, g1):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize('C,rows,n', [(1024, 1024, 4), (512, 70, 2), (1024, 33, 3)])
def test_layer_norm_cat_one_launch(C, rows, n):
    """layer_norm_cat (n LayerNorms over one residual, one launch each way) == n ops.layer_norm calls + cat: same dropout
    masks (same salt sequence), outputs bit for bit; gradients to bf16 rounding (the fused backward sums the residual
    gradient in fp32 registers, the separate calls re-round it after every LayerNorm; < 1 % of the dx elements differ
    in their last bit)."""
    import tell_amd
    from tell_amd import ops
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(17)
    lns = [torch.nn.LayerNorm(C).to(DEV) for _ in range(n)]
    for ln in lns:
        ln.weight.data.uniform_(0.5, 1.5)
        ln.bias.data.uniform_(-0.5, 0.5)
    x0 = [torch.randn(rows, C, device=DEV).bfloat16() for _ in range(n)]
    r0 = torch.randn(rows, C, device=DEV).bfloat16()
    gy = torch.randn(rows, n * C, device=DEV).bfloat16()

    def run(fused):
        tell_amd.manual_seed(99)
        for ln in lns:
            ln.weight.grad = ln.bias.grad = None
        xs = [x.clone().requires_grad_(True) for x in x0]
        res = r0.clone().requires_grad_(True)
        if fused:
            y = ops.layer_norm_cat(xs, res, lns, 0.1, True)
        else:
            y = torch.cat([ops.layer_norm(x, res, ln.weight, ln.bias, ln.eps, 0.1, True) for x, ln in zip(xs, lns)], dim=-1)
        y.backward(gy)
        return y.detach(), [x.grad for x in xs], res.grad, [ln.weight.grad.clone() for ln in lns] + [ln.bias.grad.clone() for ln in lns]

    y0, dx0, dr0, gp0 = run(False)
    y1, dx1, dr1, gp1 = run(True)
    assert torch.equal(y0, y1)
    for a, b in zip(dx0, dx1):                      # (an fma here and there: last-bit differences before the bf16 rounding)
        close(b, a.float().cpu(), torch.bfloat16)
        assert (a != b).float().mean() < 0.01
    close(dr1, dr0.float().cpu(), torch.bfloat16, scale=n)
    for a, b in zip(gp0, gp1):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize('M,N,K,act', [(32, 1024, 4096, 0), (128, 1024, 4096, 1), (7, 4096, 2048, 2), (64, 192, 4096, 0)])
def test_skinny_gemm_split_k(monkeypatch, M, N, K, act):
    """Decode-step GEMMs (few rows, K >= 2048) run as K slices of one grouped launch + a fold-and-epilogue launch: same
    result as the single fused kernel up to fp32 summation order, bias / relu / gelu / alpha applied after the fold."""
    from tell_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.03).bfloat16().to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    y1 = ops.gemm(a, w, bias=bias, bias_mode=1, act=act, alpha=0.5)
    monkeypatch.setattr(ops, '_SPLITK', False)
    y0 = ops.gemm(a, w, bias=bias, bias_mode=1, act=act, alpha=0.5)
    ref = (a.float() @ w.float().t() + bias) * 0.5
    ref = torch.relu(ref) if act == 1 else torch.nn.functional.gelu(ref) if act == 2 else ref
    close(y1, ref.cpu(), torch.bfloat16, scale=2)
    assert (y1.float() - y0.float()).abs().max() <= 2e-2 * max(1.0, y0.float().abs().max().item())
    assert (y1 != y0).float().mean() < 0.02           # the two differ only where the fp32 sum rounds the other way


@pytest.mark.parametrize('M,N,K', [(256, 64, 8200 + 57), (1024, 1024, 2 * 8192 + 1001)])
def test_long_reduction_few_columns_split_k(monkeypatch, M, N, K):
    """gemm_nn with few output columns and a very long reduction (adaptive-softmax tails: dh[rows, 64] =
    dlogits[rows, 30265] . W with a reduced dimension, [rows, 1024] with adaptive_softmax_factor 1) runs as K slices of
    one grouped launch + the fold; zero padding columns of the left operand beyond K and a ragged last slice included."""
    from tell_amd import ops
    torch.manual_seed(23)
    a = torch.zeros(M, ops._round_up(K, 8), device=DEV).bfloat16()
    a[:200, :K] = torch.randn(200, K, device=DEV).bfloat16()
    w = (torch.randn(K, N, device=DEV) * 0.05).bfloat16()
    out = torch.zeros(M, N, device=DEV).bfloat16()
    y1 = ops.gemm_nn(a, w, out=out, alpha=0.5).clone()
    monkeypatch.setattr(ops, '_SPLITK', False)
    y0 = ops.gemm_nn(a, w, alpha=0.5)
    ref = (a[:, :K].float() @ w.float()) * 0.5
    close(y1, ref.cpu(), torch.bfloat16, scale=math.sqrt(K) * 0.05)
    close(y0, ref.cpu(), torch.bfloat16, scale=math.sqrt(K) * 0.05)
    assert (y1[200:] == 0).all()


@pytest.mark.parametrize('cnt', [0, 37, 300, 1024])
def test_count_limited_products_of_the_softmax_tails(cnt):
    """The adaptive softmax's tails work on fixed-capacity buffers with a DEVICE-side row count (adaptive.py:61-76 without
    the mask.any() / nonzero() syncs).  tell_gemm_grouped's lim_dev: the K-major weight-gradient form stops READING at
    the count (rows past it hold garbage here and must not matter), the K-sliced input-gradient form skips the row tiles
    past it and tell_splitk_reduce2 leaves those output rows untouched."""
    from tell_amd import ops
    torch.manual_seed(cnt)
    cap, V, E = 1024, 2 * 8192 + 1000, 1024
    n = torch.tensor([cnt], dtype=torch.int32, device=DEV)
    # ---- weight gradient: dW[V', E] = dl[:cnt]^T h[:cnt]
    Vs = 1536
    dl = torch.randn(cap, Vs, device=DEV).bfloat16(); h = torch.randn(cap, E, device=DEV).bfloat16()
    out = torch.ones(Vs, E, device=DEV)
    ops.gemm_tn(dl, h, out=out, accumulate=True, k_dev=n)
    ref = 1.0 + dl[:cnt].float().t() @ h[:cnt].float()
    close(out, ref.cpu(), torch.bfloat16, scale=math.sqrt(max(cnt, 1)))
    # ---- input gradient of a tail with the model width: dh[:cnt] = dl[:cnt] . W   (K = V, sliced)
    a = torch.zeros(cap, ops._round_up(V, 8), device=DEV).bfloat16()
    a[:cnt, :V] = torch.randn(cnt, V, device=DEV).bfloat16()
    w = (torch.randn(V, E, device=DEV) * 0.05).bfloat16()
    dh = torch.full((cap, E), 3.0, device=DEV).bfloat16()
    ops.gemm_nn(a, w, out=dh, m_dev=n, zero_rows=True)
    ref2 = a[:cnt, :V].float() @ w.float()
    if cnt:
        close(dh[:cnt], ref2.cpu(), torch.bfloat16, scale=math.sqrt(V) * 0.05)
    assert (dh[cnt:] == 3).all()                           # row tiles past the count: skipped by the slices AND by the fold


@pytest.mark.parametrize('L', [3, 25])
def test_weigh_bert_mix_forward_and_logit_gradient(L):
    """sum_l softmax(w)[l] * H[l] (transformer_faces_objects.py:355-364): output and the gradient of the L mixing logits
    (tell_mix_bwd partial sums + tell_mix_wgrad: column sums and the softmax chain rule in one launch) vs autograd."""
    import tell_amd
    from tell_amd import ops
    tell_amd.set_compute_dtype(torch.bfloat16)
    g = torch.Generator().manual_seed(L)
    stack = (torch.randn(L, 4, 64, 1024, generator=g) * 0.5).to(DEV, torch.bfloat16)
    w = torch.nn.Parameter((torch.randn(L, generator=g) * 0.7).to(DEV))
    dout = (torch.randn(4, 64, 1024, generator=g) * 0.1).to(DEV, torch.bfloat16)
    out = ops.mix_layers(stack, w)
    out.backward(dout)
    got = ops.grad_buffer(w).clone()
    w2 = w.detach().clone().requires_grad_(True)
    ref = (torch.softmax(w2, 0).view(L, 1, 1, 1) * stack.float()).sum(0)
    ref.backward(dout.float())
    rel = ((out.float() - ref).norm() / ref.norm()).item()
    assert rel < 5e-3, rel
    torch.testing.assert_close(got, w2.grad, rtol=2e-2, atol=2e-3 * float(w2.grad.abs().max()))


def test_beam_bookkeeping_kernels_match_the_tensor_formulation():
    """tell_beam_update (candidate scores, top-K per sample, histories gathered by parent, next inputs, parent rows) and
    tell_reorder_rows (every layer's DynamicConv buffer rows follow their hypotheses, in place) against the elementwise /
    gather / topk formulation they replace in CaptionModel._generate_beam, over several steps with random head outputs,
    finished hypotheses and an EOS token in play.  Round 6: the ANCESTOR TABLE of the DynamicConv rings, composed by the same
    launch - rows pushed into a ring of planes that is never re-ordered, read back through the table, against a history
    that is physically re-ordered by parent every step (the reference's reorder_incremental_state); and the decode position
    counter the launch leaves for the next replay of a captured step."""
    from tell_amd import ops
    B, K, L, pad, eos, temp = 5, 4, 12, 1, 2, 0.7
    g = torch.Generator().manual_seed(3)
    cum = torch.full((B, K), float('-inf'), device=DEV)
    cum[:, 0] = 0.0
    finished = torch.zeros(B, K, dtype=torch.bool, device=DEV)
    seqs = torch.full((B, K, L), pad, dtype=torch.long, device=DEV)
    seqs[:, :, 0] = 0
    lps = torch.zeros(B, K, L - 1, device=DEV)
    k_cum, k_fin, k_seqs, k_lps = cum.clone(), finished.to(torch.uint8), seqs.clone(), lps.clone()
    k_cur = torch.zeros(B * K, dtype=torch.long, device=DEV)
    k_rows = torch.zeros(B * K, dtype=torch.long, device=DEV)
    bufs = [torch.randn(p, B * K, 1024, generator=g).to(DEV, torch.bfloat16) for p in (2, 6, 0, 14)]
    ref_bufs = [b.clone() for b in bufs]
    base = (torch.arange(B, device=DEV) * K).view(B, 1)
    NB = 6                                                      # ancestor table: 6 steps back = a ring of 7 planes
    k_back = torch.arange(B * K, dtype=torch.int32, device=DEV).repeat(NB, 1).contiguous()
    m_back = k_back.clone()                                    # the tensor formulation (decoders.reorder_incremental_state)
    ring = torch.zeros(NB + 1, B * K, 8, device=DEV)
    moved = torch.zeros(NB, B * K, 8, device=DEV)               # most recent first, re-ordered physically
    counter = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    for i in range(L - 1):
        lp_raw = torch.log_softmax(torch.randn(B, K, 50, generator=g), -1).topk(K, dim=-1)
        tk = lp_raw.indices.to(DEV, torch.int32).contiguous()
        tk[tk == 7] = eos                                              # some hypotheses end
        lp_t = lp_raw.values.to(DEV).contiguous()
        # ---- tensor formulation (transformer.py, the non-fused branch)
        tkl, lp = tk.long(), lp_t / temp
        fin = finished.unsqueeze(-1)
        first = torch.zeros(K, dtype=torch.bool, device=DEV)
        first[0] = True
        lp = torch.where(fin, torch.where(first, torch.zeros_like(lp), torch.full_like(lp, float('-inf'))), lp)
        tkl = torch.where(fin, torch.full_like(tkl, pad), tkl)
        top, idx = (cum.unsqueeze(-1) + lp).view(B, K * K).topk(K, dim=1)
        parent = idx // K
        tok = tkl.view(B, K * K).gather(1, idx)
        rows = (base + parent).view(-1)
        was = finished.gather(1, parent)
        tok = torch.where(was, torch.full_like(tok, pad), tok)
        seqs = seqs.view(B * K, -1).index_select(0, rows).view(B, K, -1)
        lps = lps.view(B * K, -1).index_select(0, rows).view(B, K, -1)
        seqs[:, :, i + 1] = tok
        lps[:, :, i] = torch.where(was, torch.zeros_like(top), top - cum.gather(1, parent))
        finished = was | (tok == eos)
        cum = top
        ref_bufs = [b.index_select(1, rows) for b in ref_bufs]
        # ---- kernels
        xrow = torch.randn(B * K, 8, generator=g).to(DEV)           # what step i pushes: slot r of plane i mod (NB + 1)
        ring[i % (NB + 1)] = xrow
        moved = torch.cat([xrow[None], moved[:-1]], 0).index_select(1, rows)
        ops.call('tell_beam_update', tk, lp_t, k_cum, k_fin, k_seqs, k_lps, k_cur, k_rows, B, K, L, i, pad, eos, 1.0 / temp,
                 k_back, NB, counter, None)
        assert int(counter) == i
        nb = torch.empty_like(m_back)
        nb[0] = rows.to(torch.int32)
        nb[1:] = m_back[:-1].index_select(1, rows)
        m_back = nb
        assert torch.equal(k_back, m_back), i
        for j in range(1, min(i + 1, NB) + 1):                      # step i + 1 reads the row of j steps before it
            got = ring[(i + 1 - j) % (NB + 1)].gather(0, k_back[j - 1].long()[:, None].expand(-1, 8))
            assert torch.equal(got, moved[j - 1]), (i, j)
        live = [b for b in bufs if b.shape[0] > 0]
        ops.call('tell_reorder_rows', len(live), ops._ptr_array(live), ops._int_array([b.shape[0] for b in live]), k_rows,
                 B * K, 1024, K)
        assert torch.equal(k_rows, rows) and torch.equal(k_cur, tok.reshape(-1)), i
        assert torch.equal(k_seqs, seqs) and torch.equal(k_fin.bool(), finished), i
        torch.testing.assert_close(k_cum, cum, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(k_lps, lps, rtol=1e-6, atol=1e-6)
        for a_, b_ in zip(bufs, ref_bufs):
            assert torch.equal(a_, b_), i
    assert bool(finished.any()) and not bool(finished.all())


@pytest.mark.parametrize('beams', [1, 2, 4, 6])
def test_one_query_attention_over_cached_contexts(beams):
    """tell_attn_decode (generation step: up to 4 contexts in one launch, the hypotheses of a beam share their sample's
    K/V, bias_k / bias_v and the zero row as extra keys) against tell_attn_fwd with the hypotheses presented as query
    positions - including an EMPTY context (S = 0: only the two virtual keys), a fully masked sample and ragged masks."""
    import ctypes
    import tell_amd
    from tell_amd import ops
    tell_amd.set_compute_dtype(torch.bfloat16)
    n, H, E = 3, 16, 1024                      # samples
    M = n * beams
    g = torch.Generator().manual_seed(beams)
    S_list = [0, 5, 70, 512]
    bf = dict(dtype=torch.bfloat16, device=DEV)
    q = [(torch.randn(M, E, generator=g) * 0.3).to(**bf) for _ in S_list]
    ks = [(torch.randn(S, n, E, generator=g) * 0.5).to(**bf) for S in S_list]
    vs = [(torch.randn(S, n, E, generator=g) * 0.5).to(**bf) for S in S_list]
    masks = []
    for S in S_list:
        lens = torch.randint(0, S + 1, (n,), generator=g)
        lens[0] = 0                                             # sample 0: every real key masked
        masks.append((torch.arange(S)[None, :] >= lens[:, None]).to(torch.uint8).to(DEV).contiguous())
    bk = [torch.nn.Parameter((torch.randn(1, 1, E, generator=g) * 0.3).to(DEV)) for _ in S_list]
    bv = [torch.nn.Parameter((torch.randn(1, 1, E, generator=g) * 0.3).to(DEV)) for _ in S_list]
    want = []
    for c, S in enumerate(S_list):
        qq = q[c].view(n, beams, E).transpose(0, 1)             # [beams, n, E]: hypotheses as query positions
        out, _ = ops.attention(qq, ks[c], vs[c], masks[c] if S else None, bk[c], bv[c], H, True, 0.0, False,
                               return_lse=True)
        want.append(out.transpose(0, 1).reshape(M, E))
    outs = [torch.empty(M, E, **bf) for _ in S_list]
    P = lambda ts: (ctypes.c_void_p * len(ts))(*[(t.data_ptr() if t is not None else 0) for t in ts])   # noqa: E731
    Lg = lambda v: (ctypes.c_long * len(v))(*v)                                                        # noqa: E731
    kk = [k if k.shape[0] else q[c] for c, k in enumerate(ks)]
    vv = [v if v.shape[0] else q[c] for c, v in enumerate(vs)]
    ops.call('tell_attn_decode', 4, P(q), Lg([E] * 4), P(kk), Lg([k.stride(0) if k.dim() == 3 else 0 for k in kk]),
             Lg([k.stride(1) if k.dim() == 3 else 0 for k in kk]), None, P(vv),
             Lg([v.stride(0) if v.dim() == 3 else 0 for v in vv]), Lg([v.stride(1) if v.dim() == 3 else 0 for v in vv]), None,
             P([m if S else None for m, S in zip(masks, S_list)]),
             P([ops._bias_row(b, torch.bfloat16) for b in bk]), P([ops._bias_row(b, torch.bfloat16) for b in bv]), 1,
             (ctypes.c_int * 4)(*S_list), P(outs), Lg([E] * 4), M, H, beams)
    for c in range(4):
        rel = ((outs[c].float() - want[c].float()).norm() / want[c].float().norm()).item()
        assert rel < 1e-2, (S_list[c], rel)          # bf16 outputs; the MFMA kernel rounds probabilities to bf16, this one does not
    # the generation loop's HEAD-MAJOR cache ([B, H, S, 64] seen as [S, B, H, 64]: explicit head strides): the same bits
    from tell_amd import decode
    hm = lambda t: (torch.empty(n, H, t.shape[0], 64, **bf).permute(2, 0, 1, 3).copy_(t.view(t.shape[0], n, H, 64))   # noqa: E731
                    if t.shape[0] else t)

    class _Mod:
        def __init__(self, c):
            self.head_dim, self.num_heads, self.bias_k, self.bias_v, self.add_zero_attn = 64, H, bk[c], bv[c], True
    mods = [_Mod(c) for c in range(4)]
    names = ['c%d' % c for c in range(4)]
    kvl = {nm: (hm(ks[c]), hm(vs[c])) for c, nm in enumerate(names)}
    ctx = {nm + '_mask': masks[c] for c, nm in enumerate(names) if S_list[c]}
    assert decode.attn_decode_usable(mods, kvl, names, q[0])
    got = decode.attn_decode_all(mods, names, q, kvl, ctx, M, E)
    for c in range(4):
        assert torch.equal(got[c], outs[c]), S_list[c]
    # ... and PACKED for the matrix cores (decode.PackedKV / tell_attn_decode_packed: keys head-major with the two virtual keys
    # appended, values transposed and permuted inside blocks of 32 keys, probabilities rounded to bf16 for the second MFMA)
    for m_, c in zip(mods, range(4)):
        m_.bias_k, m_.bias_v = bk[c], bv[c]
    pk = {}
    for c, nm in enumerate(names):
        pk[nm] = decode.PackedKV(mods[c], S_list[c], n, DEV)
        pk[nm].fill(ks[c], vs[c], masks[c] if S_list[c] else None)
        pk[nm].fill(ks[c], vs[c], masks[c] if S_list[c] else None)            # (refilling a cache is idempotent)
    assert decode.attn_decode_usable(mods, pk, names, q[0])
    got = decode.attn_decode_all(mods, names, q, pk, ctx, M, E)
    for c in range(4):
        rel = ((got[c].float() - want[c].float()).norm() / want[c].float().norm()).item()
        assert rel < 1e-2, ('packed', S_list[c], rel)
        assert bool(torch.isfinite(got[c].float()).all())


@pytest.mark.parametrize('M', [5, 32, 70, 128])
def test_generation_step_linears_layernorm_and_dynconv_step(M):
    """csrc/decode.hip entry points against torch at the shapes of one decoder layer: tell_skinny_linear with every
    prologue / epilogue the step uses (GLU, ReLU, scale, bf16 / fp32 / LayerNorm-rebuilt residuals, 4 problems per launch,
    the four-segment LayerNorm in front of context_fc, the bf16 side copy of trailing columns), tell_layernorm_rows,
    tell_dynconv_step (K = 3 and 31: tap softmax, window sum, in-place buffer shift)."""
    import torch.nn.functional as Fn
    import tell_amd
    from tell_amd import decode, ops
    tell_amd.set_compute_dtype(torch.bfloat16)
    E, F = 1024, 4096
    g = torch.Generator().manual_seed(M)
    bf, f32 = dict(dtype=torch.bfloat16, device=DEV), dict(dtype=torch.float32, device=DEV)
    R = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k)                         # noqa: E731

    class LN:
        def __init__(self):
            self.weight, self.bias, self.eps = (torch.rand(E, generator=g) + 0.5).to(**f32), R(E, k=0.1).to(**f32), 1e-5
    rel = lambda a, b: ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()   # noqa: E731
    lnf = lambda t, l: Fn.layer_norm(t, (E,), l.weight, l.bias, l.eps)                        # noqa: E731
    W = lambda n_, k_: R(n_, k_, k=0.03).to(**bf)                                             # noqa: E731
    Bv = lambda n_: R(n_, k=0.1).to(**f32)                                                    # noqa: E731
    x, x4 = R(M, E).to(**bf), R(M, F).to(**bf)
    raw, raw4 = (R(M, E, k=2.0) + 0.3).to(**f32), (R(M, 4 * E, k=2.0) - 0.2).to(**f32)
    ln, lns = LN(), [LN() for _ in range(4)]
    xn = lnf(raw, ln)
    # linear1 + GLU, from bf16 rows and from LayerNorm(fp32 rows) (+ row statistics)
    w, b = W(2 * E, E), Bv(2 * E)
    out = torch.empty(M, E, **bf)
    decode._skinny([x], E, [w], [b], [out], E, M, E, E, act=2)
    assert rel(out, Fn.glu(x.float() @ w.float().t() + b, dim=-1)) < 4e-3
    st = torch.zeros(M, 2, **f32)
    decode._skinny([raw], E, [w], [b], [out], E, M, E, E, pro=1, gammas=[ln.weight], betas=[ln.bias], stats_out=st, act=2)
    assert rel(out, Fn.glu(xn.bfloat16().float() @ w.float().t() + b, dim=-1)) < 4e-3
    torch.testing.assert_close(st[:, 0], raw.mean(1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(st[:, 1], (raw.var(1, unbiased=False) + 1e-5).rsqrt(), rtol=1e-5, atol=1e-6)
    # linear2 + bf16 residual / + LayerNorm(fp32 rows) rebuilt from the statistics / + fp32 residual, fp32 out
    w, b = W(E, E), Bv(E)
    o32 = torch.empty(M, E, **f32)
    decode._skinny([x], E, [w], [b], [o32], E, M, E, E, res=x, ld_res=E, out_f32=True)
    assert rel(o32, x.float() @ w.float().t() + b + x.float()) < 1e-5
    decode._skinny([x], E, [w], [b], [o32], E, M, E, E, res_raw=raw, res_stats=st, res_ln=ln, out_f32=True)
    assert rel(o32, x.float() @ w.float().t() + b + xn) < 1e-5
    decode._skinny([x], E, [w], None, [o32], E, M, E, E, scale=0.5, res_f32=raw, out_f32=True)
    assert rel(o32, (x.float() @ w.float().t()) * 0.5 + raw) < 1e-5
    # 4 problems per launch: query projections (LayerNorm first, scaled), output projections into column slices
    wq, bq = [W(E, E) for _ in range(4)], [Bv(E) for _ in range(4)]
    q4 = torch.empty(4, M, E, **bf)
    decode._skinny([raw] * 4, E, wq, bq, [q4[i] for i in range(4)], E, M, E, E, pro=1, gammas=[ln.weight], betas=[ln.bias],
                   stats_out=st, scale=0.125)
    r6 = torch.empty(M, 4 * E, **f32)
    decode._skinny([q4[i] for i in range(4)], E, wq, bq, [r6[:, i * E:(i + 1) * E] for i in range(4)], 4 * E, M, E, E,
                   res_raw=raw, res_stats=st, res_ln=ln, out_f32=True)
    for i in range(4):
        assert rel(q4[i], (xn.bfloat16().float() @ wq[i].float().t() + bq[i]) * 0.125) < 4e-3
        assert rel(r6[:, i * E:(i + 1) * E], q4[i].float() @ wq[i].float().t() + bq[i] + xn) < 1e-5
    # context_fc behind the four LayerNorms; fc1 + ReLU; fc2 (K = 4096) + residual; the side copy of trailing columns
    wc, bc = W(E, 4 * E), Bv(E)
    decode._skinny([raw4], 4 * E, [wc], [bc], [out], E, M, E, 4 * E, pro=2, gammas=[l.weight for l in lns],
                   betas=[l.bias for l in lns], seg=E)
    cat = torch.cat([lnf(raw4[:, i * E:(i + 1) * E], lns[i]) for i in range(4)], 1)
    assert rel(out, cat.bfloat16().float() @ wc.float().t() + bc) < 4e-3
    w1, b1, w2, b2 = W(F, E), Bv(F), W(E, F), Bv(E)
    h = torch.empty(M, F, **bf)
    decode._skinny([x], E, [w1], [b1], [h], F, M, F, E, act=1)
    assert rel(h, torch.relu(x.float() @ w1.float().t() + b1)) < 4e-3
    decode._skinny([x4], F, [w2], [b2], [o32], E, M, E, F, res=x, ld_res=E, out_f32=True)
    assert rel(o32, x4.float() @ w2.float().t() + b2 + x.float()) < 1e-5
    wo = W(1000 + 24, E)                                     # 1000 fp32 logits + 24 projected columns also as bf16
    lo = torch.empty(M, 1024, **f32)
    side = torch.empty(M, 24, **bf)
    decode._skinny([x], E, [wo], None, [lo], 1024, M, 1024, E, out2=side, out2_from=1000, out_f32=True)
    assert rel(lo, x.float() @ wo.float().t()) < 1e-5 and torch.equal(side, lo[:, 1000:].bfloat16())
    # ---- the LayerNorms FOLDED into their consumers (round 5): bf16 pre-norm rows in, weights scaled by gamma, the row
    # statistics gathered from the kernel's own operands, corrected in the epilogue; against LayerNorm in fp32 of the
    # rows the kernel saw (their bf16 rounding is the producer's side copy)
    raw_bf, raw4_bf = raw.bfloat16(), raw4.bfloat16()
    xnb = lnf(raw_bf.float(), ln)
    w, b = W(2 * E, E), Bv(2 * E)
    wf, sv, cv = decode._folded(torch.nn.Parameter(torch.zeros(1, device=DEV)), w, [ln], E)
    st2 = torch.zeros(M, 2, **f32)
    decode._skinny([raw_bf], E, [wf], [b], [out], E, M, E, E, pro=3, gammas=[sv], betas=[cv], eps=ln.eps, stats_out=st2, act=2)
    assert rel(out, Fn.glu(xnb @ w.float().t() + b, dim=-1)) < 6e-3
    torch.testing.assert_close(st2[:, 0], raw_bf.float().mean(1), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(st2[:, 1], (raw_bf.float().var(1, unbiased=False) + 1e-5).rsqrt(), rtol=1e-4, atol=1e-6)
    fq = [decode._folded(torch.nn.Parameter(torch.zeros(1, device=DEV)), wq[i], [ln], E) for i in range(4)]
    decode._skinny([raw_bf] * 4, E, [f[0] for f in fq], bq, [q4[i] for i in range(4)], E, M, E, E, pro=3,
                   gammas=[f[1] for f in fq], betas=[f[2] for f in fq], eps=ln.eps, stats_out=st2, scale=0.125)
    for i in range(4):
        assert rel(q4[i], (xnb @ wq[i].float().t() + bq[i]) * 0.125) < 6e-3, i
    # four problems' fp32 outputs side by side with their bf16 copies side by side (out2 per problem)
    side4 = torch.empty(M, 4 * E, **bf)
    decode._skinny([q4[i] for i in range(4)], E, wq, bq, [r6[:, i * E:(i + 1) * E] for i in range(4)], 4 * E, M, E, E,
                   res_raw=raw, res_stats=st, res_ln=ln, out2=side4, out_f32=True)
    assert torch.equal(side4, r6.bfloat16())
    for nseg in (4, 2, 1):                                   # context_fc behind n = 4 / 2 / 1 LayerNorms of 1024 columns
        wcn, rn = wc[:, :nseg * E].contiguous(), raw4_bf[:, :nseg * E].contiguous()
        wcf, sc, cc = decode._folded(torch.nn.Parameter(torch.zeros(1, device=DEV)), wcn, lns[:nseg], E)
        decode._skinny([rn], nseg * E, [wcf], [bc], [out], E, M, E, nseg * E, pro=4, gammas=[sc], betas=[cc], seg=E, eps=1e-5)
        catb = torch.cat([lnf(rn[:, i * E:(i + 1) * E].float(), lns[i]) for i in range(nseg)], 1)
        assert rel(out, catb @ wcn.float().t() + bc) < 6e-3, nseg
    # LayerNorm of fp32 rows to bf16
    y = torch.empty(M, E, **bf)
    ops.call('tell_layernorm_rows', raw, E, ln.weight, ln.bias, ln.eps, y, E, None, M, E)
    assert rel(y, xn) < 4e-3
    # DynamicConv step on the ring of past inputs (K planes indexed by time; zero planes = before the caption starts):
    # K + 3 consecutive steps from an empty ring (the ring wraps), greedy (no ancestor table); then one step whose rows find
    # their past through a random ancestor table (beam search)
    for K in (3, 7, 31):
        H = 16
        wt = W(H * K, E)
        ring = torch.zeros(K, M, E, **bf)
        past = []                                            # inputs of the previous steps, most recent last
        for t in range(K + 3):
            xt = R(M, E).to(**bf)
            ops.call('tell_dynconv_step', xt, ring, wt, out, M, E, H, K, t, None)
            taps = torch.softmax((xt.float() @ wt.float().t()).view(M, H, K), -1)
            hist = ([torch.zeros(M, E, **bf)] * (K - 1) + past)[-(K - 1):]
            win = torch.stack(hist + [xt], 0).float().view(K, M, H, 64)
            assert rel(out, torch.einsum('mhk,kmhd->mhd', taps, win).reshape(M, E)) < 4e-3, (K, t)
            past.append(xt)
            assert torch.equal(ring[t % K], xt), (K, t)
        t = K + 3
        before = ring.clone()
        back = torch.randint(0, M, (K - 1, M), generator=g).to(DEV, torch.int32)
        xt = R(M, E).to(**bf)
        ops.call('tell_dynconv_step', xt, ring, wt, out, M, E, H, K, t, back)
        taps = torch.softmax((xt.float() @ wt.float().t()).view(M, H, K), -1)
        hist = [before[(t - j) % K].index_select(0, back[j - 1].long()) for j in range(K - 1, 0, -1)]
        win = torch.stack(hist + [xt], 0).float().view(K, M, H, 64)
        assert rel(out, torch.einsum('mhk,kmhd->mhd', taps, win).reshape(M, E)) < 4e-3, K
        want_ring = before.clone()
        want_ring[t % K] = xt
        assert torch.equal(ring, want_ring), K               # exactly one plane written: the one the step does not read


@pytest.mark.parametrize('M', [5, 32, 70, 128])
def test_skinny_linear_operands_staged_through_lds_bit_identical_to_direct_loads(M):
    """The skinny linears' operands reach the matrix cores through LDS (whole cache lines per wave load, a wave-private XOR-
    swizzled transposition; option sk_staged, csrc/decode.hip) - the k -> fragment-slot assignment and the order of the
    accumulation are those of the direct form, so every form of the step (GLU, ReLU, four problems per launch, folded
    LayerNorms over 1 / 4 segments, K = 1024 / 2048 / 4096, few-column tiles, the in-launch split reduction, ragged row
    counts) must give the SAME BITS either way."""
    import tell_amd
    from tell_amd import decode, hip
    tell_amd.set_compute_dtype(torch.bfloat16)
    E, F = 1024, 4096
    g = torch.Generator().manual_seed(100 + M)
    bf, f32 = dict(dtype=torch.bfloat16, device=DEV), dict(dtype=torch.float32, device=DEV)
    R = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k)                         # noqa: E731

    class LN:
        def __init__(self):
            self.weight, self.bias, self.eps = (torch.rand(E, generator=g) + 0.5).to(**f32), R(E, k=0.1).to(**f32), 1e-5
    W = lambda n_, k_: R(n_, k_, k=0.03).to(**bf)                                             # noqa: E731
    Bv = lambda n_: R(n_, k=0.1).to(**f32)                                                    # noqa: E731
    x, x2, x4 = R(M, E).to(**bf), R(M, 2 * E).to(**bf), R(M, F).to(**bf)
    raw_bf, raw4_bf = (R(M, E, k=2.0) + 0.3).to(**bf), (R(M, 4 * E, k=2.0) - 0.2).to(**bf)
    ln, lns = LN(), [LN() for _ in range(4)]
    w_l1, b_l1, w_l2, b_l2 = W(2 * E, E), Bv(2 * E), W(E, E), Bv(E)
    wq, bq = [W(E, E) for _ in range(4)], [Bv(E) for _ in range(4)]
    wc, bc, w1, b1, w2, b2, w22 = W(E, 4 * E), Bv(E), W(F, E), Bv(F), W(E, F), Bv(E), W(E, 2 * E)
    P = lambda: torch.nn.Parameter(torch.zeros(1, device=DEV))                                # noqa: E731
    wf1, s1, c1 = decode._folded(P(), w_l1, [ln], E)
    fq = [decode._folded(P(), wq[i], [ln], E) for i in range(4)]
    wcf, scf, ccf = decode._folded(P(), wc, lns, E)
    ws = decode.split_workspace(torch.device(DEV))

    def run():
        outs = []
        o = torch.zeros(M, E, **bf)
        decode._skinny([x], E, [w_l1], [b_l1], [o], E, M, E, E, act=2)
        outs.append(o)
        o = torch.zeros(M, E, **bf)
        st = torch.zeros(M, 2, **f32)
        decode._skinny([raw_bf], E, [wf1], [b_l1], [o], E, M, E, E, pro=3, gammas=[s1], betas=[c1], eps=ln.eps, stats_out=st, act=2)
        outs += [o, st]
        o32 = torch.zeros(M, E, **f32)
        decode._skinny([x], E, [w_l2], [b_l2], [o32], E, M, E, E, res=x, ld_res=E, out_f32=True)
        outs.append(o32)
        q4 = torch.zeros(4, M, E, **bf)
        decode._skinny([raw_bf] * 4, E, [f[0] for f in fq], bq, [q4[i] for i in range(4)], E, M, E, E, pro=3,
                       gammas=[f[1] for f in fq], betas=[f[2] for f in fq], eps=ln.eps, scale=0.125)
        outs.append(q4)
        r6 = torch.zeros(M, 4 * E, **f32)
        decode._skinny([q4[i] for i in range(4)], E, wq, bq, [r6[:, i * E:(i + 1) * E] for i in range(4)], 4 * E, M, E, E,
                       res_f32=o32, out_f32=True)
        outs.append(r6)
        for split in (0, 1):
            with hip.options(sk_split=split):
                o = torch.zeros(M, E, **bf)
                decode._skinny([raw4_bf], 4 * E, [wcf], [bc], [o], E, M, E, 4 * E, pro=4, gammas=[scf], betas=[ccf], seg=E, eps=1e-5)
                o32 = torch.zeros(M, E, **f32)
                decode._skinny([x4], F, [w2], [b2], [o32], E, M, E, F, res=x, ld_res=E, out_f32=True)
                o2 = torch.zeros(M, E, **f32)
                decode._skinny([x2], 2 * E, [w22], [b2], [o2], E, M, E, 2 * E, out_f32=True)
                outs += [o, o32, o2]
        h = torch.zeros(M, F, **bf)
        decode._skinny([x], E, [w1], [b1], [h], F, M, F, E, act=1)
        outs.append(h)
        torch.cuda.synchronize()
        return outs
    with hip.options(sk_staged=0):
        direct = run()
    with hip.options(sk_staged=1):
        staged = run()
    assert ws is not None
    for i, (a, b) in enumerate(zip(direct, staged)):
        assert torch.equal(a, b), i
        assert bool(torch.isfinite(a.float()).all()) and float(a.float().abs().sum()) > 0, i


@pytest.mark.parametrize('M', [7, 19, 32, 64])
def test_skinny_linear_reduction_shared_between_workgroups(M):
    """tell_skinny_linear with split_ws (round 6): context_fc / fc2 of the generation step (N = 1024, K = 4096 / 2048) with
    the reduction of an output tile shared by 4 / 2 workgroups that combine INSIDE the launch (write-through partial tiles,
    an agent-scope arrival counter, the last arrival sums in slice order).  Against fp32 and against the unsplit kernel;
    and what an in-launch hand-off can get wrong: 300 launches that ALTERNATE between two inputs while another stream keeps
    the memory system busy - every output must be bit-identical to the first one of its input (a stale partial tile, a
    counter that lost an arrival or a sum that depends on the arrival order would show)."""
    import torch.nn.functional as Fn
    import tell_amd
    from tell_amd import decode, hip
    tell_amd.set_compute_dtype(torch.bfloat16)
    hip.set_option('sk_split', 1)                 # (off by default since the operands are staged through LDS: no gain left)
    E = 1024
    g = torch.Generator().manual_seed(100 + M)
    bf, f32 = dict(dtype=torch.bfloat16, device=DEV), dict(dtype=torch.float32, device=DEV)
    R = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k)                         # noqa: E731
    rel = lambda a, b: ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()   # noqa: E731

    class LN:
        def __init__(self):
            self.weight, self.bias, self.eps = (torch.rand(E, generator=g) + 0.5).to(**f32), R(E, k=0.1).to(**f32), 1e-5
    for nseg in (4, 2):
        K = nseg * E
        xs = [R(M, K).to(**bf) for _ in range(2)]
        res = R(M, E).to(**bf)
        w2, b2 = R(E, K, k=0.03).to(**bf), R(E, k=0.1).to(**f32)
        raws = [(R(M, K, k=2.0) + 0.3).to(**bf) for _ in range(2)]
        lns = [LN() for _ in range(nseg)]
        wc, bc = R(E, K, k=0.03).to(**bf), R(E, k=0.1).to(**f32)
        wcf, sc, cc = decode._folded(torch.nn.Parameter(torch.zeros(1, device=DEV)), wc, lns, E)
        o32, side, x2 = torch.empty(M, E, **f32), torch.empty(M, E, **bf), torch.empty(M, E, **bf)

        def fc2(x):                                   # fc2: K = 4096 (2048), + bias + bf16 residual, fp32 out + bf16 copy
            decode._skinny([x], K, [w2], [b2], [o32], E, M, E, K, res=res, ld_res=E, out2=side, out_f32=True)
            return o32.clone(), side.clone()

        def cfc(raw):                                 # context_fc behind nseg folded LayerNorms
            decode._skinny([raw], K, [wcf], [bc], [x2], E, M, E, K, pro=4, gammas=[sc], betas=[cc], seg=E, eps=1e-5)
            return x2.clone()
        with hip.options(sk_split=0):
            plain = [fc2(xs[i]) for i in range(2)], [cfc(raws[i]) for i in range(2)]
        first = [fc2(xs[i]) for i in range(2)], [cfc(raws[i]) for i in range(2)]
        for i in range(2):
            assert rel(first[0][i][0], xs[i].float() @ w2.float().t() + b2 + res.float()) < 1e-5
            assert torch.equal(first[0][i][1], first[0][i][0].bfloat16())
            assert rel(first[0][i][0], plain[0][i][0]) < 1e-6                  # (another summation order, the same sum)
            cat = torch.cat([Fn.layer_norm(raws[i][:, j * E:(j + 1) * E].float(), (E,), lns[j].weight, lns[j].bias, 1e-5)
                             for j in range(nseg)], 1)
            assert rel(first[1][i], cat @ wc.float().t() + bc) < 6e-3
            assert rel(first[1][i], plain[1][i]) < 4e-3
        # the split path really ran: its launches do not write what sk_split = 0 writes bit for bit at K = 4096 ... (not a
        # reliable probe) - ask the profiler instead
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as pf:
            fc2(xs[0]); cfc(raws[0])
            torch.cuda.synchronize()
        names = ' '.join(e.name for e in pf.events())
        import re
        split_ran = re.search(r'skinny_mfma_kernel<\d+, ?\d+, ?\d+, ?(true|false), ?\d+, ?true', names) is not None   # <RT, ACT, U, FOLD, NW, SPLIT = true, ..>
        assert split_ran == (M <= 32), names          # (measured: a loss above 32 rows - csrc/decode.hip; those keep the unsplit form)
        # ---- alternate inputs under memory traffic on another stream
        side_stream = torch.cuda.Stream()
        big = torch.empty(64 << 20, dtype=torch.float32, device=DEV)
        stop = torch.cuda.Event()
        with torch.cuda.stream(side_stream):
            for _ in range(40):
                big.add_(1.0)
        bad = 0
        for it in range(300):
            i = it & 1
            a, b = fc2(xs[i]), cfc(raws[i])
            bad += int(not torch.equal(a[0], first[0][i][0])) + int(not torch.equal(a[1], first[0][i][1]))
            bad += int(not torch.equal(b, first[1][i]))
        side_stream.synchronize()
        assert bad == 0, (M, nseg, bad)


def test_packed_attention_cache_layout_is_the_documented_fragment_order():
    """include/tell_hip.h (tell_attn_decode_packed) documents the cache the kernel reads: kc [Bs, H, Sp/16, 2, 64 lanes, 8] with lane
    l = key l & 15 of the tile, elements c * 32 + (l >> 4) * 8 ..; vt [Bs, H, Sp/32, 4, 64 lanes, 8] with lane l = dimension rt * 16 +
    (l & 15), keys 4 g + j (j < 4) | 16 + 4 g + j - 4 of k-group g = l >> 4; bias row and zero row as keys S, S + 1; the rest zero;
    mask 1 past S + 1.  decode.PackedKV.fill is the host mirror of that layout: element by element against the formula."""
    import tell_amd
    from tell_amd import decode
    tell_amd.set_compute_dtype(torch.bfloat16)
    try:
        g = torch.Generator().manual_seed(5)

        class Mod:
            num_heads = 3
            bias_k = torch.randn(1, 1, 192, generator=g).to(DEV)
            bias_v = torch.randn(1, 1, 192, generator=g).to(DEV)
        S, Bc, H = 45, 2, 3
        pk = decode.PackedKV(Mod, S, Bc, DEV)
        assert pk.Sp == 64
        k = torch.randn(S, Bc, H * 64, generator=g).to(DEV, torch.bfloat16)
        v = torch.randn(S, Bc, H * 64, generator=g).to(DEV, torch.bfloat16)
        mask = (torch.rand(Bc, S, generator=g) < 0.2).to(DEV)
        pk.fill(k, v, mask)
        knat = torch.zeros(Bc, H, pk.Sp, 64, dtype=torch.bfloat16, device=DEV)
        vnat = torch.zeros_like(knat)
        knat[:, :, :S] = k.view(S, Bc, H, 64).permute(1, 2, 0, 3)
        vnat[:, :, :S] = v.view(S, Bc, H, 64).permute(1, 2, 0, 3)
        knat[:, :, S] = Mod.bias_k.view(H, 64).bfloat16()
        vnat[:, :, S] = Mod.bias_v.view(H, 64).bfloat16()
        kc = pk.kc.view(Bc, H, pk.Sp // 16, 2, 64, 8).cpu()
        vt = pk.vt.view(Bc, H, pk.Sp // 32, 4, 64, 8).cpu()
        kn, vn = knat.cpu(), vnat.cpu()
        for lane in (0, 5, 17, 31, 48, 63):
            lr, lg = lane & 15, lane >> 4
            for tile in range(pk.Sp // 16):
                for c in range(2):
                    assert torch.equal(kc[:, :, tile, c, lane], kn[:, :, tile * 16 + lr, c * 32 + lg * 8:c * 32 + lg * 8 + 8]), (lane, tile, c)
            for blk in range(pk.Sp // 32):
                for rt in range(4):
                    keys = [blk * 32 + 4 * lg + j for j in range(4)] + [blk * 32 + 16 + 4 * lg + j for j in range(4)]
                    assert torch.equal(vt[:, :, blk, rt, lane], vn[:, :, keys, rt * 16 + lr]), (lane, blk, rt)
        want_mask = torch.ones(Bc, pk.Sp, dtype=torch.uint8)
        want_mask[:, :S] = mask.cpu().to(torch.uint8)
        want_mask[:, S:S + 2] = 0
        assert torch.equal(pk.mask.cpu(), want_mask)
    finally:
        tell_amd.set_compute_dtype(torch.float32)
