#!/usr/bin/env python
"""Cost of the per-token statistics (generate(token_stats=n)).
  1. the new launch alone (tell_adaptive_logprob_stats, n = 4 and n = 8) over the fp32 logits of the expt vocabulary (head 5000
     + 2 clusters, tails 15000 / 30265) at 32 and 128 rows, next to tell_adaptive_logprob_topk(k = 8) on the same buffers - the
     yardstick: it reads the same bytes - legs interleaved, each timed inside a hipGraph, medians of repeated windows;
  2. the full-size faces_objects decode loop (bf16, captured greedy step) at 32 captions with token_stats = 0 and 4:
     microseconds per decode step, legs interleaved loop by loop, medians.
usage (GPU box): python tools/bench_token_stats.py [--skip-model] [--skip-head]"""
import sys

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402
from tell_amd.decode import StatsSink  # noqa: E402
from tell_amd.hip import call  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'


def graph_of(fn, reps=20):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with tell_amd.hip.bound_stream():
            for _ in range(reps):
                fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def window(g, n=400, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n // reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (n // reps * reps)


def head_launches(windows=7):
    c0, tails = 5000, (15000, 30265)
    for N in (32, 128):
        g = torch.Generator().manual_seed(N)
        ld = lambda n: -(-n // 4) * 4                                          # noqa: E731
        head = (torch.randn(N, ld(c0 + 2), generator=g) * 3).to(dev)
        tl = [(torch.randn(N, ld(n), generator=g) * 2).to(dev) for n in tails]
        args = [head, head.stride(0), c0, 2, tl[0], tl[0].stride(0), tails[0], tl[1], tl[1].stride(0), tails[1], None, 0, 0]
        tok = torch.empty(N, 8, dtype=torch.int32, device=dev)
        lp = torch.empty(N, 8, dtype=torch.float32, device=dev)
        chosen = torch.randint(3, c0 + sum(tails), (N, 1), generator=g).to(torch.int32).to(dev)
        cnt = torch.full((1,), 49, dtype=torch.int32, device=dev)
        legs = {'top-k 8 (yardstick)': graph_of(lambda: call('tell_adaptive_logprob_topk', *args, N, 8, tok, lp))}
        keep = []
        for n in (4, 8):
            sink = StatsSink(n, 100, N, 1, dev)
            keep.append(sink)
            legs['stats n = %d' % n] = graph_of(lambda s=sink, n=n: call(
                'tell_adaptive_logprob_stats', *args, N, chosen, 1, None, n, 100, 0, cnt, 1, s.alt_tok, s.alt_lp, s.rank,
                s.entropy, s.chosen_lp))
        per = {k: [] for k in legs}
        for _ in range(windows):                                               # interleaved: a window of every leg in turn
            for k, gr in legs.items():
                per[k].append(window(gr))
        for k, v in per.items():
            print('head launch  N=%3d  %-20s %7.2f us (median of %d windows; min %.2f max %.2f)'
                  % (N, k, sorted(v)[len(v) // 2], windows, min(v), max(v)))
        sys.stdout.flush()


def decode_steps(B=32, loops=9):
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects').to(dev).eval()
    batch = synthetic_batch(B, 512, 33, True, seed=3, device=dev)
    with torch.no_grad():
        caption_ids, _, contexts = model._forward(batch['context'], batch['image'], batch['caption'],
                                                  batch['face_embeds'], batch['obj_embeds'])
    legs = [('token_stats = 0', {}), ('token_stats = 4', {'token_stats': 4})]
    per = {name: [] for name, _ in legs}
    for it in range(2 + loops):
        for name, kw in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            with torch.no_grad():
                _, ids, _ = model._generate(caption_ids, contexts, **kw)
            e1.record()
            torch.cuda.synchronize()
            if it >= 2:                                                        # (the first two loops record the graphs)
                per[name].append(1e3 * e0.elapsed_time(e1) / (ids.shape[1] - 1))
    med = {name: sorted(v)[len(v) // 2] for name, v in per.items()}
    for name, _ in legs:
        print('decode step  B=%3d  greedy  %-16s %7.1f us per step (median of %d loops of %d steps; min %.1f max %.1f)'
              % (B, name, med[name], loops, ids.shape[1] - 1, min(per[name]), max(per[name])))
    print('decode step  B=%3d  greedy  token_stats = 4 - 0: %+.1f us per step' % (B, med[legs[1][0]] - med[legs[0][0]]))


if __name__ == '__main__':
    if '--skip-head' not in sys.argv:
        head_launches()
    if '--skip-model' not in sys.argv:
        decode_steps()
