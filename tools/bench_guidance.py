#!/usr/bin/env python
"""Cost of context guidance in the cached generators.
  1. the head's last launch over full-size adaptive-softmax logits (head 5000 + 2 clusters, tails 15000 / 30265, fp32), timed
     inside a hipGraph, legs interleaved: tell_adaptive_logprob_topk over 32 and over 64 rows against
     tell_adaptive_logprob_topk_guided over 32 pairs (the same 64 logit rows), k = 1 and k = 4, register and streaming forms;
  2. the full-size faces_objects decode loop (bf16, captured steps), greedy and beam 4: the guided step at 32 captions
     (gamma = 3, the image dropped: 64 images in the static batch) against the plain step at 32 and at 64 captions -
     microseconds per decode step, legs interleaved, medians.
Nothing here is a gate: the numbers go to profiles/guidance_bench.txt.
usage (GPU box): python tools/bench_guidance.py [--skip-model] [--skip-head]"""
import sys

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402
from tell_amd.hip import call  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'


def graph_of(fn, reps=20):
    for _ in range(3):
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


def time_legs(legs, reps=20, rounds=15, replays=4):
    """legs: [(name, fn)] -> {name: median microseconds per call}; the legs' graphs are replayed in turn, round by round."""
    graphs = [(name, graph_of(fn, reps)) for name, fn in legs]
    per = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, g in graphs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            per[name].append(1e3 * e0.elapsed_time(e1) / (replays * reps))
    return {name: sorted(v)[len(v) // 2] for name, v in per.items()}


def head_launches(R=32):
    c0, tails = 5000, (15000, 30265)
    N = 2 * R
    g = torch.Generator().manual_seed(N)
    ld = lambda n: -(-n // 4) * 4                                              # noqa: E731
    head = (torch.randn(N, ld(c0 + 2), generator=g) * 3).to(dev)
    tl = [(torch.randn(N, ld(n), generator=g) * 2).to(dev) for n in tails]
    args = [head, head.stride(0), c0, 2, tl[0], tl[0].stride(0), tails[0], tl[1], tl[1].stride(0), tails[1], None, 0, 0]
    gamma = torch.full((1,), 3.0, dtype=torch.float32, device=dev)
    for regs in (1, 0):
        form = 'registers' if regs else 'streaming'
        with tell_amd.hip.options(argmax_regs=regs):
            legs = []
            for k in (1, 4):
                tok = torch.empty(N, k, dtype=torch.int32, device=dev)
                lp = torch.empty(N, k, dtype=torch.float32, device=dev)
                legs += [('top-k %d, %d rows' % (k, R), lambda k=k, tok=tok, lp=lp: call('tell_adaptive_logprob_topk', *args, R, k, tok, lp)),
                         ('top-k %d, %d rows' % (k, N), lambda k=k, tok=tok, lp=lp: call('tell_adaptive_logprob_topk', *args, N, k, tok, lp)),
                         ('guided k=%d, %d pairs' % (k, R), lambda k=k, tok=tok, lp=lp: call(
                             'tell_adaptive_logprob_topk_guided', *args, R, R, k, gamma, None, 0, tok, lp))]
            med = time_legs(legs)                                              # (the form is recorded with the captured launch)
        for name, _ in legs:
            print('head last launch  %-9s  %-22s %7.2f us' % (form, name, med[name]))
        for k in (1, 4):
            print('head last launch  %-9s  guided k=%d / top-k %d: %.2f x at %d rows, %.2f x at %d rows'
                  % (form, k, k, med['guided k=%d, %d pairs' % (k, R)] / med['top-k %d, %d rows' % (k, R)], R,
                     med['guided k=%d, %d pairs' % (k, R)] / med['top-k %d, %d rows' % (k, N)], N))
        sys.stdout.flush()


def decode_steps(B=32, loops=7):
    """The legs alternate loop by loop on the same model, warm (captures recorded first), medians."""
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects').to(dev).eval()
    inputs = {}
    for n in (B, 2 * B):
        batch = synthetic_batch(n, 512, 33, True, seed=3, device=dev)
        with torch.no_grad():
            caption_ids, _, contexts = model._forward(batch['context'], batch['image'], batch['caption'],
                                                      batch['face_embeds'], batch['obj_embeds'])
        inputs[n] = (caption_ids, contexts)
    legs = [('plain %d' % B, B, None), ('plain %d' % (2 * B), 2 * B, None), ('guided %d' % B, B, (('image',), 3.0))]
    for mode, K in (('greedy', 1), ('beam 4', 4)):
        per = {name: [] for name, _, _ in legs}
        for it in range(2 + loops):
            for name, n, guide in legs:
                caption_ids, contexts = inputs[n]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                with torch.no_grad():
                    _, ids, _ = model._generate(caption_ids, contexts, beam_size=K, **({'guide': guide} if guide else {}))
                e1.record()
                torch.cuda.synchronize()
                if it >= 2:                                                    # (the first two loops record the graphs)
                    per[name].append(1e3 * e0.elapsed_time(e1) / (ids.shape[1] - 1))
        med = {name: sorted(v)[len(v) // 2] for name, v in per.items()}
        for name, _, _ in legs:
            print('decode step  %-7s %-10s %7.1f us per step (median of %d loops; min %.1f max %.1f)'
                  % (mode, name, med[name], loops, min(per[name]), max(per[name])))
        print('decode step  %-7s guided %d / plain %d: %.2f x; / plain %d: %.2f x'
              % (mode, B, B, med['guided %d' % B] / med['plain %d' % B], 2 * B, med['guided %d' % B] / med['plain %d' % (2 * B)]))
        sys.stdout.flush()


if __name__ == '__main__':
    if '--skip-head' not in sys.argv:
        head_launches()
    if '--skip-model' not in sys.argv:
        decode_steps()
