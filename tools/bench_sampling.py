#!/usr/bin/env python
"""Cost of top-k sampling (tell_adaptive_logprob_sample) against the arg-max it replaces.
  1. the generation head's LAST launch over full-size adaptive-softmax logits (head 5000 + 2 clusters, tails 15000 / 30265,
     fp32, rows on 16 bytes), timed inside a hipGraph: register arg-max vs the sampling kernel at k = 1 / 8 / 50 / 64,
     N = 32 / 128 rows;
  2. the full-size faces_objects decode loop (bf16, captured steps), greedy vs sampling_topk = 50, B = 32: microseconds per
     decode step (HIP events around `_generate`, divided by the steps taken; random weights decode all 100 steps).
usage (GPU box): python tools/bench_sampling.py [--skip-model]"""
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


def head_launches():
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


if __name__ == '__main__':
    head_launches()
    if '--skip-model' not in sys.argv:
        decode_steps()
