#!/usr/bin/env python
"""Cost of the repetition / presence / frequency penalties of the cached generators.
  1. the head's last launches over full-size adaptive-softmax logits (head 5000 + 2 clusters, tails 15000 / 30265, fp32), timed
     inside a hipGraph at N = 32 / 128 rows, legs interleaved: the arg-max against tell_decode_token_counts +
     tell_adaptive_logprob_topk_penalised (k = 1), top-k 4 against its penalised form, the top-k 64 sampler against its
     penalised form - on histories of 50 tokens over 400 ids;
  2. the full-size faces_objects decode loop (bf16, captured steps) at 32 and 128 captions for greedy, beam 4 and top-k
     sampling (k = 8, T = 0.9): microseconds per decode step with the penalties at their defaults and with
     (theta, alpha, beta) = (1.2, 0, 0.1), legs interleaved, medians.
--default-only runs the default legs alone (it then needs nothing this tool's commit added: the same file times the parent
commit).  usage (GPU box): python tools/bench_penalties.py [--default-only] [--skip-model] [--skip-head]"""
import sys

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402
from tell_amd.hip import call  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'
DEFAULT_ONLY = '--default-only' in sys.argv
PEN = (1.2, 0.0, 0.1)


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


def head_launches():
    c0, tails, L = 5000, (15000, 30265), 101
    for N in (32, 128):
        g = torch.Generator().manual_seed(N)
        ld = lambda n: -(-n // 4) * 4                                          # noqa: E731
        head = (torch.randn(N, ld(c0 + 2), generator=g) * 3).to(dev)
        tl = [(torch.randn(N, ld(n), generator=g) * 2).to(dev) for n in tails]
        args = [head, head.stride(0), c0, 2, tl[0], tl[0].stride(0), tails[0], tl[1], tl[1].stride(0), tails[1], None, 0, 0]
        tok1 = torch.empty(N, dtype=torch.int32, device=dev)
        lp1 = torch.empty(N, dtype=torch.float32, device=dev)
        tok4 = torch.empty(N, 4, dtype=torch.int32, device=dev)
        lp4 = torch.empty(N, 4, dtype=torch.float32, device=dev)
        seed = torch.tensor([7], dtype=torch.int32, device=dev)
        cnt = torch.full((1,), 49, dtype=torch.int32, device=dev)                # step 50 from the device counter
        legs = [('arg-max', lambda: call('tell_adaptive_logprob_argmax', *args, N, None, 0, tok1, lp1)),
                ('top-k 4', lambda: call('tell_adaptive_logprob_topk', *args, N, 4, tok4, lp4)),
                ('sample 64', lambda: call('tell_adaptive_logprob_sample', *args, N, 64, 1.0, seed, None, 0, cnt, tok1, lp1))]
        if not DEFAULT_ONLY:
            hist = torch.randint(3, 400, (N, L), generator=g).to(dev)          # 50 tokens of history over 400 ids
            fin = torch.zeros(N, dtype=torch.uint8, device=dev)
            p_tok = torch.zeros(N, L, dtype=torch.int32, device=dev)
            p_cnt = torch.zeros(N, L, dtype=torch.int32, device=dev)
            n_pen = torch.zeros(N, dtype=torch.int32, device=dev)
            from tell_amd.models.stepper import sub_table
            sub = sub_table(PEN[1], PEN[2], L).to(dev)
            pa = [p_tok, p_cnt, L, n_pen, PEN[0], sub, sub.numel()]
            counts = lambda: call('tell_decode_token_counts', hist, L, L, fin, N, 0, cnt, p_tok, p_cnt, L, n_pen)  # noqa: E731
            counts()
            legs += [('counts', counts),
                     ('penalised k=1', lambda: call('tell_adaptive_logprob_topk_penalised', *args, N, 1, *pa, tok1, lp1)),
                     ('counts + penalised k=1', lambda: (counts(), call('tell_adaptive_logprob_topk_penalised', *args, N, 1, *pa,
                                                                         tok1, lp1))),
                     ('penalised top-k 4', lambda: call('tell_adaptive_logprob_topk_penalised', *args, N, 4, *pa, tok4, lp4)),
                     ('penalised sample 64', lambda: call('tell_adaptive_logprob_sample_penalised', *args, N, 64, 1.0, seed, None,
                                                          0, cnt, *pa, tok1, lp1))]
        med = time_legs(legs)
        for name, _ in legs:
            print('head last launch  N=%3d  %-24s %7.2f us' % (N, name, med[name]))
        if not DEFAULT_ONLY:
            print('head last launch  N=%3d  mean list length %.1f; counts + penalised k=1 - arg-max: %+.2f us; penalised top-k 4 - '
                  'top-k 4: %+.2f us; penalised sample 64 - sample 64: %+.2f us'
                  % (N, float(n_pen.float().mean()), med['counts + penalised k=1'] - med['arg-max'],
                     med['penalised top-k 4'] - med['top-k 4'], med['penalised sample 64'] - med['sample 64']))
        sys.stdout.flush()


def decode_steps(sizes=(32, 128), loops=7):
    """The legs alternate loop by loop on the same model and batch, warm (captures recorded first), medians."""
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects').to(dev).eval()
    legs = [('default', (1.0, 0.0, 0.0))] + ([] if DEFAULT_ONLY else [('theta=%g alpha=%g beta=%g' % PEN, PEN)])
    for B in sizes:
        batch = synthetic_batch(B, 512, 33, True, seed=3, device=dev)
        with torch.no_grad():
            caption_ids, _, contexts = model._forward(batch['context'], batch['image'], batch['caption'],
                                                      batch['face_embeds'], batch['obj_embeds'])
        for mode, K, topk in (('greedy', 1, 1), ('beam 4', 4, 1), ('top-k 8', 1, 8)):
            model.sampling_topk, model.sampling_temp = topk, (0.9 if topk > 1 else 1.0)
            per = {name: [] for name, _ in legs}
            for it in range(2 + loops):
                for name, o in legs:
                    if not DEFAULT_ONLY:
                        model.repetition_penalty, model.presence_penalty, model.frequency_penalty = o
                    torch.manual_seed(11)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    with torch.no_grad():
                        _, ids, _ = model._generate(caption_ids, contexts, beam_size=K)
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= 2:                                                # (the first two loops record the graphs)
                        per[name].append(1e3 * e0.elapsed_time(e1) / (ids.shape[1] - 1))
            med = {name: sorted(v)[len(v) // 2] for name, v in per.items()}
            for name, _ in legs:
                print('decode step  B=%3d  %-7s %-28s %7.1f us per step (median of %d loops of %d steps; min %.1f max %.1f)'
                      % (B, mode, name, med[name], loops, ids.shape[1] - 1, min(per[name]), max(per[name])))
            if len(legs) > 1:
                print('decode step  B=%3d  %-7s penalties / default: %.3f' % (B, mode, med[legs[1][0]] / med[legs[0][0]]))
            sys.stdout.flush()
        model.sampling_topk, model.sampling_temp = 1, 1.0


if __name__ == '__main__':
    if '--skip-head' not in sys.argv:
        head_launches()
    if '--skip-model' not in sys.argv:
        decode_steps()
