#!/usr/bin/env python
"""Cost of the search options of the cached generators (beam_len_penalty, no_repeat_ngram_size, min_len).
  1. the head's last launches over full-size adaptive-softmax logits (head 5000 + 2 clusters, tails 15000 / 30265, fp32), timed
     inside a hipGraph at N = 32 / 128 rows (greedy) and 128 / 512 rows (beam 4): arg-max / top-k 4 as they are, against
     tell_decode_ban_list + tell_adaptive_logprob_topk_banned on histories of 50 tokens (n = 3, min_len = 4), and
     tell_beam_update against tell_beam_update_norm;
  2. the full-size faces_objects decode loop (bf16, captured steps) at 32 and 128 captions, greedy and beam 4: microseconds
     per decode step with the options at their defaults and with (alpha = 1, n = 3, min_len = 4), legs interleaved, medians.
--default-only runs the default legs alone (it then needs nothing this tool's commit added: the same file times the parent
commit).  usage (GPU box): python tools/bench_beam_options.py [--default-only] [--skip-model] [--skip-head]"""
import sys

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402
from tell_amd.hip import call  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'
DEFAULT_ONLY = '--default-only' in sys.argv
OPTS = (1.0, 3, 4)


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
    c0, tails, L, eos = 5000, (15000, 30265), 101, 2
    for N, k in ((32, 1), (128, 1), (128, 4), (512, 4)):
        g = torch.Generator().manual_seed(N)
        ld = lambda n: -(-n // 4) * 4                                          # noqa: E731
        head = (torch.randn(N, ld(c0 + 2), generator=g) * 3).to(dev)
        tl = [(torch.randn(N, ld(n), generator=g) * 2).to(dev) for n in tails]
        args = [head, head.stride(0), c0, 2, tl[0], tl[0].stride(0), tails[0], tl[1], tl[1].stride(0), tails[1], None, 0, 0]
        tok = torch.empty(N, k, dtype=torch.int32, device=dev)
        lp = torch.empty(N, k, dtype=torch.float32, device=dev)
        if k == 1:
            t0 = timeit(lambda: call('tell_adaptive_logprob_argmax', *args, N, None, 0, tok, lp))
        else:
            t0 = timeit(lambda: call('tell_adaptive_logprob_topk', *args, N, k, tok, lp))
        name = 'argmax (registers)' if k == 1 else 'top-k %d           ' % k
        print('head last launch  N=%3d  %s            %7.2f us' % (N, name, t0))
        if DEFAULT_ONLY:
            continue
        hist = torch.randint(3, 400, (N, L), generator=g).to(dev)              # 50 tokens of history, a few repeated bigrams
        fin = torch.zeros(N, dtype=torch.uint8, device=dev)
        ban = torch.zeros(N, L + 1, dtype=torch.int32, device=dev)
        n_ban = torch.zeros(N, dtype=torch.int32, device=dev)
        cnt = torch.full((1,), 49, dtype=torch.int32, device=dev)
        bl = lambda: call('tell_decode_ban_list', hist, L, L, fin, N, 0, cnt, OPTS[1], OPTS[2], eos, ban, L + 1, n_ban)  # noqa: E731
        tb = lambda: call('tell_adaptive_logprob_topk_banned', *args, N, k, ban, L + 1, n_ban, tok, lp)                 # noqa: E731
        t_list, t_top = timeit(bl), timeit(tb)
        t_both = timeit(lambda: (bl(), tb()))
        print('head last launch  N=%3d  ban list %5.2f us, banned top-k %d %7.2f us, both %7.2f us   (+%.2f us; mean n_ban %.2f)'
              % (N, t_list, k, t_top, t_both, t_both - t0, float(n_ban.float().mean())))
        n_ban.fill_(0)
        print('head last launch  N=%3d  banned top-k %d with empty lists        %7.2f us' % (N, k, timeit(tb)))
        cnt1 = torch.full((1,), 49, dtype=torch.int32, device=dev)
        call('tell_decode_ban_list', hist, L, L, fin, N, 0, cnt1, 1, 99, eos, ban, L + 1, n_ban)    # n = 1: the whole history
        print('head last launch  N=%3d  banned top-k %d with %d bans per row     %7.2f us' % (N, k, int(n_ban[0]), timeit(tb)))
        if k > 1:
            B = N // k
            cum = torch.zeros(B, k, device=dev)
            seqs = torch.ones(B, k, L, dtype=torch.long, device=dev)
            lps = torch.zeros(B, k, L - 1, device=dev)
            cur = torch.zeros(N, dtype=torch.long, device=dev)
            rows = torch.zeros(N, dtype=torch.long, device=dev)
            length = torch.zeros(B, k, dtype=torch.int32, device=dev)
            table = torch.ones(L + 1, device=dev)
            tk = torch.randint(3, 400, (B, k, k), generator=g).to(dev, torch.int32)
            lpk = -torch.rand(B, k, k, generator=g).to(dev)
            t_u = timeit(lambda: call('tell_beam_update', tk, lpk, cum, fin, seqs, lps, cur, rows, B, k, L, 50, 1, eos, 1.0, None, 0,
                                      None, None))
            cum.zero_()
            t_n = timeit(lambda: call('tell_beam_update_norm', tk, lpk, cum, fin, seqs, lps, cur, rows, length, table, B, k, L, 50, 1,
                                      eos, 1.0, None, 0, None, None))
            print('bookkeeping       B=%3d  beam_update %6.2f us, beam_update_norm %6.2f us' % (B, t_u, t_n))
        sys.stdout.flush()


def decode_steps(sizes=(32, 128), loops=7):
    """The legs alternate loop by loop on the same model and batch, warm (captures recorded first), medians."""
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects').to(dev).eval()
    legs = [('default', (0.0, 0, 0))] + ([] if DEFAULT_ONLY else [('a=%g n=%d min_len=%d' % OPTS, OPTS)])
    for B in sizes:
        batch = synthetic_batch(B, 512, 33, True, seed=3, device=dev)
        with torch.no_grad():
            caption_ids, _, contexts = model._forward(batch['context'], batch['image'], batch['caption'],
                                                      batch['face_embeds'], batch['obj_embeds'])
        for K in (1, 4):
            per = {name: [] for name, _ in legs}
            for it in range(2 + loops):
                for name, o in legs:
                    if not DEFAULT_ONLY:
                        model.beam_len_penalty, model.no_repeat_ngram_size, model.min_len = o
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
                print('decode step  B=%3d  %-7s %-22s %7.1f us per step (median of %d loops of %d steps; min %.1f max %.1f)'
                      % (B, 'greedy' if K == 1 else 'beam %d' % K, name, med[name], loops, ids.shape[1] - 1, min(per[name]),
                         max(per[name])))
            if len(legs) > 1:
                print('decode step  B=%3d  %-7s options / default: %.3f' % (B, 'greedy' if K == 1 else 'beam %d' % K,
                                                                           med[legs[1][0]] / med[legs[0][0]]))
            sys.stdout.flush()


if __name__ == '__main__':
    if '--skip-head' not in sys.argv:
        head_launches()
    if '--skip-model' not in sys.argv:
        decode_steps()
