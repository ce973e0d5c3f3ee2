#!/usr/bin/env python
"""Cost of top-k sampling (tell_adaptive_logprob_sample) against the arg-max it replaces.
  1. the generation head's LAST launch over full-size adaptive-softmax logits (head 5000 + 2 clusters, tails 15000 / 30265,
     fp32, rows on 16 bytes), timed inside a hipGraph: register arg-max vs the sampling kernel at k = 1 / 8 / 50 / 64,
     N = 32 / 128 rows;
  2. the full-size faces_objects decode loop (bf16, captured steps), greedy vs sampling_topk = 50, B = 32: microseconds per
     decode step (HIP events around `_generate`, divided by the steps taken; random weights decode all 100 steps).
  3. --topp P: nucleus sampling (tell_adaptive_logprob_nucleus, k = 0) - its launch beside the legs of 1., on the rows of 1.
     (flat: nuclei of thousands of tokens) and on rows scaled x4 (peaked); and the decode step at 32 and 128 captions with
     sampling_topk = 0, sampling_topp = P against sampling_topk = 64, legs interleaved, medians.
usage (GPU box): python tools/bench_sampling.py [--skip-model] [--topp P]"""
import sys

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402
from tell_amd.hip import call  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'


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


def head_launches(topp=None):
    c0, tails = 5000, (15000, 30265)
    for N in (32, 128):
        g = torch.Generator().manual_seed(N)
        ld = lambda n: -(-n // 4) * 4                                          # noqa: E731
        head = (torch.randn(N, ld(c0 + 2), generator=g) * 3).to(dev)
        tl = [(torch.randn(N, ld(n), generator=g) * 2).to(dev) for n in tails]
        args = [head, head.stride(0), c0, 2, tl[0], tl[0].stride(0), tails[0], tl[1], tl[1].stride(0), tails[1], None, 0, 0]
        tok = torch.empty(N, dtype=torch.int32, device=dev)
        lp = torch.empty(N, dtype=torch.float32, device=dev)
        seed = torch.tensor([12345], dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        t_arg = timeit(lambda: call('tell_adaptive_logprob_argmax', *args, N, None, 0, tok, lp))
        print('head last launch  N=%3d  argmax (registers)   %7.2f us' % (N, t_arg))
        for k in (1, 8, 50, 64):
            t = timeit(lambda: call('tell_adaptive_logprob_sample', *args, N, k, 1.0 / 0.8, seed, None, 0, cnt, tok, lp))
            print('head last launch  N=%3d  sample k=%-2d          %7.2f us   (%.2fx the arg-max)' % (N, k, t, t / t_arg))
        if topp is not None:
            t64 = t
            for name, mul in (('flat rows', 1.0), ('rows x4  ', 4.0)):
                sc = [a.mul(mul) if torch.is_tensor(a) else a for a in args]
                sc = [sc[0], sc[0].stride(0)] + sc[2:]
                nuc = lambda: call('tell_adaptive_logprob_nucleus', *sc, N, 0, 1.0 / 0.8, topp, seed, None, 0, cnt,  # noqa: E731
                                   tok, lp, None, None)
                t = timeit(nuc)
                size = torch.empty(N, dtype=torch.int32, device=dev)
                call('tell_adaptive_logprob_nucleus', *sc, N, 0, 1.0 / 0.8, topp, seed, None, 0, cnt, tok, lp, size, None)
                print('head last launch  N=%3d  nucleus p=%.2f %s %7.2f us   (%.2fx sample k=64; median nucleus %d tokens)'
                      % (N, topp, name, t, t / t64, int(size.median())))
        sys.stdout.flush()


def decode_steps(B=32):
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects').to(dev).eval()
    batch = synthetic_batch(B, 512, 33, True, seed=3, device=dev)
    with torch.no_grad():
        caption_ids, _, contexts = model._forward(batch['context'], batch['image'], batch['caption'], batch['face_embeds'],
                                                  batch['obj_embeds'])
    res = {}
    for name, k in (('greedy', 1), ('sampling_topk=50', 50)):
        model.sampling_topk, model.sampling_temp = k, 1.0
        for _ in range(2):                                                     # capture + multi-step graphs
            model._generate(caption_ids, contexts)
        torch.cuda.synchronize()
        per = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, ids, _ = model._generate(caption_ids, contexts)
            e1.record()
            torch.cuda.synchronize()
            per.append(1e3 * e0.elapsed_time(e1) / (ids.shape[1] - 1))
        res[name] = sorted(per)[len(per) // 2]
        print('decode step  B=%d  %-17s %7.1f us per step (median of 5 loops of %d steps)' % (B, name, res[name],
                                                                                          ids.shape[1] - 1))
    print('decode step  sampling / greedy: %.3f' % (res['sampling_topk=50'] / res['greedy']))


def decode_steps_topp(topp, sizes=(32, 128), loops=7):
    """Decode step with sampling_topk = 0, sampling_topp = topp against sampling_topk = 64: the legs alternate loop by loop
    on the same model and batch, warm (captures recorded first), medians."""
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects').to(dev).eval()
    legs = (('sampling_topk=64', 64, None), ('topk=0 topp=%.2f' % topp, 0, topp))
    for B in sizes:
        batch = synthetic_batch(B, 512, 33, True, seed=3, device=dev)
        with torch.no_grad():
            caption_ids, _, contexts = model._forward(batch['context'], batch['image'], batch['caption'],
                                                      batch['face_embeds'], batch['obj_embeds'])
        per = {name: [] for name, _, _ in legs}
        for it in range(2 + loops):
            for name, k, p in legs:
                model.sampling_topk, model.sampling_temp, model.sampling_topp = k, 1.0, p
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _, ids, _ = model._generate(caption_ids, contexts)
                e1.record()
                torch.cuda.synchronize()
                if it >= 2:                                                    # (the first two loops record the graphs)
                    per[name].append(1e3 * e0.elapsed_time(e1) / (ids.shape[1] - 1))
        med = {name: sorted(v)[len(v) // 2] for name, v in per.items()}
        for name, _, _ in legs:
            print('decode step  B=%3d  %-18s %7.1f us per step (median of %d loops; min %.1f max %.1f)'
                  % (B, name, med[name], loops, min(per[name]), max(per[name])))
        print('decode step  B=%3d  nucleus / top-k 64: %.3f' % (B, med[legs[1][0]] / med[legs[0][0]]))
        sys.stdout.flush()


if __name__ == '__main__':
    topp = float(sys.argv[sys.argv.index('--topp') + 1]) if '--topp' in sys.argv else None
    head_launches(topp)
    if '--skip-model' not in sys.argv:
        if topp is None:
            decode_steps()
        else:
            decode_steps_topp(topp)
