"""What several sampled captions per image cost on the copy models' cached step, at B = 32 images, S = 512,
H = 16, D = 64, bf16, step 49 of L = 100, n = 2, 4, 8 hypotheses per image:
  1. the kernels, as hipGraph replays of 20 launches, legs interleaved, medians of 15 rounds: tell_copy_decide over 32 n rows
     with the article keys expanded to [S, 32 n, E] - what the kernel of before would have to be given, the yardstick - against
     tell_copy_decide_hyp on the same rows over the keys [S, 32, E];
  2. the whole decode loop of a full-size random-weight transformer_pointer drawing from the nucleus, encoders excluded, legs
     interleaved, medians: generate(cached=True, n_samples=n) (_pointer_steps with n rows per image, ranking included) against
     n calls of generate(cached=True) (_generate_pointer_cached).  The encoder pass a further caption of an image no longer
     needs - n - 1 passes per batch - is NOT in these numbers: it is saved on top of them.
Nothing here is a gate: the numbers go to profiles/copy_n_samples_bench.txt.
usage (GPU box): python tools/bench_copy_n_samples.py [--skip-model] [--skip-kernels]"""
import sys

import torch

sys.path.insert(0, '.')
sys.path.insert(0, 'tools')
import tell_amd  # noqa: E402
from bench_copy_decode import time_legs  # noqa: E402  (the method of section 27's tool; its legs sit behind __main__)
from tell_amd.hip import call  # noqa: E402

dev = 'cuda'
B, S, H, D, L, P = 32, 512, 16, 64, 100, 49
E = H * D
NS = (2, 4, 8)


def kernels():
    bf = torch.bfloat16
    dt = tell_amd.hip.dt(bf)
    g = torch.Generator().manual_seed(0)
    k_bse = (torch.randn(B, S, E, generator=g) * 0.1).to(dev).to(bf)             # the article keys as _copy_k stores them
    bk = (torch.randn(E, generator=g) * 0.1).to(dev).to(bf)
    mask = torch.zeros(B, S, dtype=torch.uint8, device=dev)
    proper = (torch.rand(B, S, generator=g) > 0.5).to(torch.int8).to(dev)
    ctx = torch.randint(3, 5000, (B, S), generator=g).to(dev)
    for n in NS:
        R = B * n
        q = (torch.randn(R, E, generator=g) * 0.1).to(dev).to(bf)
        ent = torch.tensor([[0., 1.]], device=dev).expand(R, 2).contiguous()
        gen, fin = torch.full((R,), 7, dtype=torch.int32, device=dev), torch.zeros(R, dtype=torch.uint8, device=dev)
        hist = torch.full((R, L + 1), -1, dtype=torch.int32, device=dev)
        mk = lambda: (torch.zeros(R, L + 1, dtype=torch.uint8, device=dev), torch.zeros(R, L, dtype=torch.float32, device=dev),      # noqa: E731
                      torch.empty(R, H, S, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.int32, device=dev))
        k_rep = k_bse.repeat_interleave(n, dim=0).contiguous().transpose(0, 1)   # [S, R, E]
        k = k_bse.transpose(0, 1)                                                # [S, B, E]
        mask_r, proper_r, ctx_r = (t.repeat_interleave(n, dim=0).contiguous() for t in (mask, proper, ctx))
        (cp1, pr1, sc1, tok1), (cp2, pr2, sc2, tok2) = mk(), mk()

        def expanded():
            call('tell_copy_decide', q, E, k_rep, k_rep.stride(0), k_rep.stride(1), bk, mask_r, proper_r, ctx_r, ent, gen, fin, hist,
                 L + 1, cp1, L + 1, pr1, L, L, P, None, R, H, S, D, sc1, tok1, dt)

        def grouped():
            call('tell_copy_decide_hyp', q, E, k, k.stride(0), k.stride(1), bk, mask, proper, ctx, ent, gen, fin, hist, L + 1, cp2,
                 L + 1, pr2, L, L, P, None, B, n, H, S, D, sc2, tok2, dt)
        med = time_legs([('tell_copy_decide, keys expanded', expanded), ('tell_copy_decide_hyp', grouped)])
        torch.cuda.synchronize()
        same = all(torch.equal(a, b_) for a, b_ in ((cp1, cp2), (pr1, pr2), (tok1, tok2)))
        a, b_ = med['tell_copy_decide, keys expanded'], med['tell_copy_decide_hyp']
        kb, sb = B * S * E * 2, 2 * R * H * S * 4                                # keys read once; scratch written and read
        print('copy decision  B=%d n=%d (%d rows) S=%d bf16  expanded %8.2f us  grouped %8.2f us  expanded / grouped %.2f x  '
              '(outputs bit-equal: %s)' % (B, n, R, S, a, b_, a / b_, same))
        print('copy decision  n=%d traffic: expanded %.1f MB of keys + %.1f MB of scratch, moved at %.0f GB/s; grouped %.1f MB of '
              'keys + %.1f MB of scratch, moved at %.0f GB/s' % (n, n * kb / 1e6, sb / 1e6, (n * kb + sb) / a / 1e3, kb / 1e6, sb / 1e6,
                                                                 (kb + sb) / b_ / 1e3))
        sys.stdout.flush()
        del k_rep


def decode_loop(loops=5):
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('pointer', sampling_topk=0, sampling_topp=0.9, sampling_temp=0.8).to(dev).eval()
    batch = synthetic_batch(B, S, 33, True, seed=3, device=dev)
    g = torch.Generator().manual_seed(5)
    context = batch['context']
    context['roberta_proper_masks'] = (torch.rand(context['roberta'].shape, generator=g) > 0.5).long().to(dev)
    with torch.no_grad():
        enc = model.encode(context, batch['image'])
        caption_ids, _, contexts = model._forward(context, batch['image'], batch['caption'], batch['face_embeds'], None, enc)
    for n in NS:
        def grouped():
            out = model._drive(model._pointer_steps(caption_ids, contexts, enc, context, n=n, rank=('score', 0.0)))
            return out[4]['gen_ids_samples'].shape[2] - 1

        def repeated():
            return max(model._generate_pointer_cached(caption_ids, contexts, enc, context)[0].shape[1] - 1 for _ in range(n))
        legs = [('n_samples=%d' % n, grouped), ('%d calls' % n, repeated)]
        per, steps = {name: [] for name, _ in legs}, {}
        for it in range(2 + loops):
            for name, fn in legs:
                torch.manual_seed(100 + it)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                with torch.no_grad():
                    st = fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= 2:                                                   # (the first two loops record the graphs)
                    per[name].append(e0.elapsed_time(e1))
                    steps[name] = st
        med = {name: sorted(v)[len(v) // 2] for name, v in per.items()}
        for name, _ in legs:
            print('decode loop  B=%d n=%d S=%d bf16  %-13s %8.1f ms for %d captions (longest %3d steps), %7.1f captions/s  (median of '
                  '%d loops; min %.1f max %.1f ms)' % (B, n, S, name, med[name], B * n, steps[name], B * n / (med[name] / 1e3), loops,
                                                       min(per[name]), max(per[name])))
        a, b_ = legs[0][0], legs[1][0]
        print('decode loop  n=%d: %d calls / n_samples=%d: %.2f x;  per step of the grouped loop %.1f us' %
              (n, n, n, med[b_] / med[a], 1e3 * med[a] / steps[a]))
        sys.stdout.flush()
    h = [x for sig, x in model.__dict__['_decode_graphs'].items() if ('hidden',) in sig]
    print('decode loop  entries %d, captured: %s' % (len(h), [x['graph'] not in (None, False) for x in h]))
    print('decode loop  the encoder pass saved per further caption of an image is not in these numbers')
    sys.stdout.flush()


if __name__ == '__main__':
    tell_amd.hip.require_gpu()
    if '--skip-kernels' not in sys.argv:
        kernels()
    if '--skip-model' not in sys.argv:
        decode_loop()
