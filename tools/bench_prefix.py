#!/usr/bin/env python
"""Cost of a forced decode step (caption completion, generate(prefix=...)).
  1. the new launch alone over full-size adaptive-softmax logits (head 5000 + 2 clusters, tails 15000 / 30265, fp32), timed
     inside a hipGraph at N = 32 / 128 rows (greedy, k = 1) and 128 / 512 rows (beam 4, k = 4): the pick kernel as it is, the
     pick followed by tell_adaptive_logprob_forced with every row free and with every row forced (tokens spread over the
     head and both tails), and the forced launch on its own in both cases;
  2. the full-size faces_objects decode loop (bf16, captured steps) at 32 and 128 captions, greedy and beam 4: microseconds
     per decode step without a prefix (the plain graph), with an all-pad prefix (every step a free step of the prefixed
     graph) and with a prefix of gen_len tokens (every step forced), legs interleaved, medians of repeated loops.
--default-only runs the plain legs alone (it then needs nothing this tool's commit added: the same file times the parent
commit).  usage (GPU box): python tools/bench_prefix.py [--default-only] [--skip-model] [--skip-head]"""
import sys

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402
from tell_amd.hip import call  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'
DEFAULT_ONLY = '--default-only' in sys.argv
GEN = 100


def timeit(fn, n=400, windows=5):
    """Median over `windows` timed windows of n launches replayed from a hipGraph of 20."""
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
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n // 20):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / (n // 20 * 20))
    return sorted(out)[len(out) // 2]


def head_launches():
    c0, tails = 5000, (15000, 30265)
    V = c0 + sum(tails)
    for N, k in ((32, 1), (128, 1), (128, 4), (512, 4)):
        g = torch.Generator().manual_seed(N)
        ld = lambda n: -(-n // 4) * 4                                          # noqa: E731
        head = (torch.randn(N, ld(c0 + 2), generator=g) * 3).to(dev)
        tl = [(torch.randn(N, ld(n), generator=g) * 2).to(dev) for n in tails]
        args = [head, head.stride(0), c0, 2, tl[0], tl[0].stride(0), tails[0], tl[1], tl[1].stride(0), tails[1], None, 0, 0]
        tok = torch.empty(N, k, dtype=torch.int32, device=dev)
        lp = torch.empty(N, k, dtype=torch.float32, device=dev)
        if k == 1:
            pick = lambda: call('tell_adaptive_logprob_argmax', *args, N, None, 0, tok, lp)     # noqa: E731
        else:
            pick = lambda: call('tell_adaptive_logprob_topk', *args, N, k, tok, lp)             # noqa: E731
        t0 = timeit(pick)
        name = 'argmax (registers)' if k == 1 else 'top-k %d           ' % k
        print('head last launch  N=%3d  %s                      %7.2f us' % (N, name, t0))
        if DEFAULT_ONLY:
            continue
        S = N // k
        prefix = torch.randint(3, V, (S, GEN), generator=g).to(dev)            # 60 % of 50 k ids lie in the last tail
        cnt = torch.full((1,), 49, dtype=torch.int32, device=dev)
        for label, plen in (('every row free  ', torch.zeros(S, dtype=torch.int32, device=dev)),
                            ('every row forced', torch.full((S,), GEN, dtype=torch.int32, device=dev))):
            forced = lambda: call('tell_adaptive_logprob_forced', *args, N, k, prefix, GEN, GEN, plen, S, None, k, 0, cnt,  # noqa: E731
                                  1, tok, lp)
            t_f = timeit(forced)
            t_both = timeit(lambda: (pick(), forced()))
            print('head last launch  N=%3d  forced launch alone, %s %7.2f us; behind the pick %7.2f us (+%.2f us)'
                  % (N, label, t_f, t_both, t_both - t0))
        sys.stdout.flush()


def decode_steps(sizes=(32, 128), loops=7):
    """The legs alternate loop by loop on the same model and batch, warm (captures recorded first), medians."""
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects').to(dev).eval()
    V = model.decoder.adaptive_softmax.vocab_size
    for B in sizes:
        batch = synthetic_batch(B, 512, 33, True, seed=3, device=dev)
        with torch.no_grad():
            caption_ids, _, contexts = model._forward(batch['context'], batch['image'], batch['caption'],
                                                      batch['face_embeds'], batch['obj_embeds'])
        legs = [('no prefix (plain graph)', None)]
        if not DEFAULT_ONLY:
            from tell_amd.models.transformer import check_prefix
            g = torch.Generator().manual_seed(B)
            legs += [('all-pad prefix (free steps)', check_prefix(torch.ones(B, 1, dtype=torch.long), B, V)),
                     ('prefix of %d (forced steps)' % GEN, check_prefix(torch.randint(3, V, (B, GEN), generator=g), B, V))]
        for K in (1, 4):
            per = {name: [] for name, _ in legs}
            for it in range(2 + loops):
                for name, pfx in legs:
                    kw = {'prefix': pfx} if pfx is not None else {}
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    with torch.no_grad():
                        _, ids, _ = model._generate(caption_ids, contexts, beam_size=K, **kw)
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= 2:                                                # (the first two loops record the graphs)
                        per[name].append(1e3 * e0.elapsed_time(e1) / (ids.shape[1] - 1))
            med = {name: sorted(v)[len(v) // 2] for name, v in per.items()}
            what = 'greedy' if K == 1 else 'beam %d' % K
            for name, _ in legs:
                print('decode step  B=%3d  %-7s %-28s %7.1f us per step (median of %d loops of %d steps; min %.1f max %.1f)'
                      % (B, what, name, med[name], loops, ids.shape[1] - 1, min(per[name]), max(per[name])))
            for name, _ in legs[1:]:
                print('decode step  B=%3d  %-7s %-28s - plain: %+.1f us' % (B, what, name, med[name] - med[legs[0][0]]))
            sys.stdout.flush()


if __name__ == '__main__':
    if '--skip-head' not in sys.argv:
        head_launches()
    if '--skip-model' not in sys.argv:
        decode_steps()
