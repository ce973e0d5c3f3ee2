#!/usr/bin/env python
"""Cost of min-p and locally typical sampling (tell_adaptive_logprob_minp / tell_adaptive_logprob_typical, DESIGN.md section
19) beside nucleus sampling (tell_adaptive_logprob_nucleus, k = 0) in the same run.
  1. the generation head's LAST launch over full-size adaptive-softmax logits (head 5000 + 2 clusters, tails 15000 / 30265,
     fp32, rows on 16 bytes), timed inside a hipGraph at N = 32 / 128 rows, on flat rows (the rows of tools/bench_sampling.py)
     and on rows scaled x4 (peaked); each leg three times over, interleaved: the spread is printed;
  2. the full-size faces_objects decode loop (bf16, captured steps) at 32 and 128 captions: sampling_minp = M and
     sampling_typical = TAU against sampling_topp = P, legs alternating loop by loop, medians.
usage (GPU box): python tools/bench_truncation.py [--skip-model] [--minp M] [--typical TAU] [--topp P]"""
import math
import sys

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402
from tell_amd.hip import call  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'


def arg(name, default):
    return float(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timeit(fn, n=400):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with tell_amd.hip.bound_stream():
            for _ in range(20):
                fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n // 20):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (n // 20 * 20)


def head_launches(minp, tau, topp, repeats=3):
    c0, tails = 5000, (15000, 30265)
    inv_temp = 1.0 / 0.8
    for N in (32, 128):
        g = torch.Generator().manual_seed(N)
        ld = lambda n: -(-n // 4) * 4                                          # noqa: E731
        head = (torch.randn(N, ld(c0 + 2), generator=g) * 3).to(dev)
        tl = [(torch.randn(N, ld(n), generator=g) * 2).to(dev) for n in tails]
        tok = torch.empty(N, dtype=torch.int32, device=dev)
        lp = torch.empty(N, dtype=torch.float32, device=dev)
        size = torch.empty(N, dtype=torch.int32, device=dev)
        seed = torch.tensor([12345], dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        for name, mul in (('flat rows', 1.0), ('rows x4  ', 4.0)):
            h, t0, t1 = head * mul, tl[0] * mul, tl[1] * mul
            rows = [h, h.stride(0), c0, 2, t0, t0.stride(0), tails[0], t1, t1.stride(0), tails[1], None, 0, 0, N]
            draw = [seed, None, 0, cnt, tok, lp]
            legs = (('nucleus p=%.2f' % topp, lambda s: call('tell_adaptive_logprob_nucleus', *rows, 0, inv_temp, topp, *draw, s,
                                                             None)),
                    ('min-p m=%.2f' % minp, lambda s: call('tell_adaptive_logprob_minp', *rows, inv_temp, math.log(minp), *draw,
                                                           s)),
                    ('typical tau=%.2f' % tau, lambda s: call('tell_adaptive_logprob_typical', *rows, inv_temp, tau, *draw, s,
                                                              None, None)))
            times = {n_: [] for n_, _ in legs}
            for _ in range(repeats):
                for n_, fn in legs:
                    times[n_].append(timeit(lambda: fn(None)))
            base = sorted(times[legs[0][0]])[repeats // 2]
            for n_, fn in legs:
                fn(size)
                med = sorted(times[n_])[repeats // 2]
                print('head last launch  N=%3d  %-17s %s %7.2f us   (min %.2f max %.2f of %d; %.2fx nucleus; median set %d tokens)'
                      % (N, n_, name, med, min(times[n_]), max(times[n_]), repeats, med / base, int(size.median())))
            sys.stdout.flush()


def decode_steps(minp, tau, topp, sizes=(32, 128), loops=7):
    """Decode step with sampling_minp / sampling_typical against sampling_topp (all with sampling_topk = 0): the legs alternate
    loop by loop on the same model and batch, warm (captures recorded first), medians."""
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects', sampling_topk=0, sampling_topp=topp).to(dev).eval()
    legs = (('topp=%.2f' % topp, (topp, None, None)), ('minp=%.2f' % minp, (None, minp, None)),
            ('typical=%.2f' % tau, (None, None, tau)))
    for B in sizes:
        batch = synthetic_batch(B, 512, 33, True, seed=3, device=dev)
        with torch.no_grad():
            caption_ids, _, contexts = model._forward(batch['context'], batch['image'], batch['caption'],
                                                      batch['face_embeds'], batch['obj_embeds'])
        per = {name: [] for name, _ in legs}
        for it in range(2 + loops):
            for name, (p, m, t) in legs:
                model.sampling_topp, model.sampling_minp, model.sampling_typical = p, m, t
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _, ids, _ = model._generate(caption_ids, contexts)
                e1.record()
                torch.cuda.synchronize()
                if it >= 2:                                                    # (the first two loops record the graphs)
                    per[name].append(1e3 * e0.elapsed_time(e1) / (ids.shape[1] - 1))
        med = {name: sorted(v)[len(v) // 2] for name, v in per.items()}
        for name, _ in legs:
            print('decode step  B=%3d  %-14s %7.1f us per step (median of %d loops; min %.1f max %.1f; %.3fx nucleus)'
                  % (B, name, med[name], loops, min(per[name]), max(per[name]), med[name] / med[legs[0][0]]))
        sys.stdout.flush()


if __name__ == '__main__':
    minp, tau, topp = arg('--minp', 0.1), arg('--typical', 0.9), arg('--topp', 0.9)
    head_launches(minp, tau, topp)
    if '--skip-model' not in sys.argv:
        decode_steps(minp, tau, topp)
