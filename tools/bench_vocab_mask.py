#!/usr/bin/env python
"""Cost of the vocabulary masks of the cached generators.
  1. the head's last launch over full-size adaptive-softmax logits (head 5000 + 2 clusters, tails 15000 / 30265, fp32), timed
     inside a hipGraph at N = 32 / 128 rows, legs interleaved, for arg-max / top-k 4 / the top-k 64 sampler: plain; a ban list
     (tell_adaptive_logprob_topk_banned, 3 entries per row: the same code path as the masked pick with another staging);
     masked at a 50 % random mask and at a grounded mask (a class of about 8 000 tokens, articles of 512 ids);
  2. the builder launch alone (tell_decode_vocab_mask, 512 article ids per image, class and a shared deny row);
  3. the full-size faces_objects decode loop (bf16, captured steps) at 32 and 128 captions for greedy, beam 4 and top-k
     sampling (k = 8, T = 0.9): microseconds per decode step by default and grounded, legs interleaved, medians.
--default-only runs the default legs alone (it then needs nothing this tool's commit added: the same file times the parent
commit).  usage (GPU box): python tools/bench_vocab_mask.py [--default-only] [--skip-model] [--skip-head]"""
import sys

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402
from tell_amd.hip import call  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'
DEFAULT_ONLY = '--default-only' in sys.argv
VOCAB, N_CLASS = 50265, 8000


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


def name_class(g):
    """A stand-in for the class of capitalised BPE pieces: about 8 000 token ids spread over the three clusters."""
    cls = torch.zeros(VOCAB, dtype=torch.bool)
    cls[torch.randperm(VOCAB - 4, generator=g)[:N_CLASS] + 4] = True
    return cls


def head_launches():
    from tell_amd import ops
    c0, tails = 5000, (15000, 30265)
    for N in (32, 128):
        g = torch.Generator().manual_seed(N)
        ld = lambda n: -(-n // 4) * 4                                          # noqa: E731
        head = (torch.randn(N, ld(c0 + 2), generator=g) * 3).to(dev)
        tl = [(torch.randn(N, ld(n), generator=g) * 2).to(dev) for n in tails]
        args = [head, head.stride(0), c0, 2, tl[0], tl[0].stride(0), tails[0], tl[1], tl[1].stride(0), tails[1], None, 0, 0]
        tok1 = torch.empty(N, dtype=torch.int32, device=dev)
        lp1 = torch.empty(N, dtype=torch.float32, device=dev)
        tok1k = torch.empty(N, 1, dtype=torch.int32, device=dev)
        lp1k = torch.empty(N, 1, dtype=torch.float32, device=dev)
        tok4 = torch.empty(N, 4, dtype=torch.int32, device=dev)
        lp4 = torch.empty(N, 4, dtype=torch.float32, device=dev)
        seed = torch.tensor([7], dtype=torch.int32, device=dev)
        cnt = torch.full((1,), 49, dtype=torch.int32, device=dev)                # step 50 from the device counter
        legs = [('arg-max', lambda: call('tell_adaptive_logprob_argmax', *args, N, None, 0, tok1, lp1)),
                ('top-k 4', lambda: call('tell_adaptive_logprob_topk', *args, N, 4, tok4, lp4)),
                ('sample 64', lambda: call('tell_adaptive_logprob_sample', *args, N, 64, 1.0, seed, None, 0, cnt, tok1, lp1))]
        if not DEFAULT_ONLY:
            ban = torch.randint(4, VOCAB, (N, 8), generator=g).to(dev, torch.int32)
            n_ban = torch.full((N,), 3, dtype=torch.int32, device=dev)
            half = ops.pack_mask_bits(torch.rand(N, VOCAB, generator=g) < 0.5).to(dev)
            ctx = torch.randint(4, VOCAB, (N, 512), generator=g).to(dev)
            cls_bits = ops.pack_mask_bits(name_class(g)).to(dev)
            deny8 = torch.zeros(1, VOCAB, dtype=torch.uint8, device=dev)
            deny8[0, 3] = 1
            grounded = ops.vocab_mask(ctx, VOCAB, cls_bits, deny8)
            scratch = torch.empty_like(grounded)
            for label, bits in (('50 %', half), ('grounded', grounded)):
                ma = [bits, bits.stride(0), 1]
                legs += [('masked k=1 ' + label, lambda ma=ma: call('tell_adaptive_logprob_topk_masked', *args, N, 1, *ma, None, 0,
                                                                    None, tok1k, lp1k)),
                         ('masked top-k 4 ' + label, lambda ma=ma: call('tell_adaptive_logprob_topk_masked', *args, N, 4, *ma, None,
                                                                        0, None, tok4, lp4)),
                         ('masked sample 64 ' + label, lambda ma=ma: call('tell_adaptive_logprob_sample_masked', *args, N, 64, 1.0,
                                                                          seed, None, 0, cnt, *ma, tok1, lp1))]
            legs += [('banned k=1', lambda: call('tell_adaptive_logprob_topk_banned', *args, N, 1, ban, ban.stride(0), n_ban, tok1k,
                                                 lp1k)),
                     ('banned top-k 4', lambda: call('tell_adaptive_logprob_topk_banned', *args, N, 4, ban, ban.stride(0), n_ban,
                                                     tok4, lp4)),
                     ('masked + banned top-k 4', lambda: call('tell_adaptive_logprob_topk_masked', *args, N, 4, grounded,
                                                              grounded.stride(0), 1, ban, ban.stride(0), n_ban, tok4, lp4)),
                     ('builder', lambda: ops.vocab_mask(ctx, VOCAB, cls_bits, deny8, out=scratch))]
        med = time_legs(legs)
        for name, _ in legs:
            print('head last launch  N=%3d  %-28s %7.2f us' % (N, name, med[name]))
        if not DEFAULT_ONLY:
            print('head last launch  N=%3d  masked against banned (grounded): k=1 %+.2f us, top-k 4 %+.2f us; masked sample 64 - '
                  'sample 64: %+.2f us; masked k=1 - arg-max: %+.2f us'
                  % (N, med['masked k=1 grounded'] - med['banned k=1'], med['masked top-k 4 grounded'] - med['banned top-k 4'],
                     med['masked sample 64 grounded'] - med['sample 64'], med['masked k=1 grounded'] - med['arg-max']))
        sys.stdout.flush()


def decode_steps(sizes=(32, 128), loops=7):
    """The legs alternate loop by loop on the same model and batch, warm (captures recorded first), medians."""
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects').to(dev).eval()
    legs = [('default', False)] + ([] if DEFAULT_ONLY else [('grounded', True)])
    cls = name_class(torch.Generator().manual_seed(1))
    for B in sizes:
        batch = synthetic_batch(B, 512, 33, True, seed=3, device=dev)
        with torch.no_grad():
            caption_ids, _, contexts = model._forward(batch['context'], batch['image'], batch['caption'],
                                                      batch['face_embeds'], batch['obj_embeds'])
            vm = None if DEFAULT_ONLY else model._vocab_mask(batch['context'], None, cls)
        for mode, K, topk in (('greedy', 1, 1), ('beam 4', 4, 1), ('top-k 8', 1, 8)):
            model.sampling_topk, model.sampling_temp = topk, (0.9 if topk > 1 else 1.0)
            per = {name: [] for name, _ in legs}
            for it in range(2 + loops):
                for name, on in legs:
                    torch.manual_seed(11)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    with torch.no_grad():
                        _, ids, _ = model._generate(caption_ids, contexts, beam_size=K, **({'vmask': vm} if on else {}))
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= 2:                                                # (the first two loops record the graphs)
                        per[name].append(1e3 * e0.elapsed_time(e1) / (ids.shape[1] - 1))
            med = {name: sorted(v)[len(v) // 2] for name, v in per.items()}
            for name, _ in legs:
                print('decode step  B=%3d  %-7s %-10s %7.1f us per step (median of %d loops of %d steps; min %.1f max %.1f)'
                      % (B, mode, name, med[name], loops, ids.shape[1] - 1, min(per[name]), max(per[name])))
            if len(legs) > 1:
                print('decode step  B=%3d  %-7s grounded / default: %+.1f %%' % (B, mode, 100.0 * (med['grounded'] / med['default'] - 1)))
            sys.stdout.flush()
        model.sampling_topk, model.sampling_temp = 1, 1.0


if __name__ == '__main__':
    if '--skip-head' not in sys.argv:
        head_launches()
    if '--skip-model' not in sys.argv:
        decode_steps()
