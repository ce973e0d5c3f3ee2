#!/usr/bin/env python
"""Cost of the attention-map export.
  1. the attention launch(es) of one decoder layer inside a hipGraph at 32 and 128 rows with the configs[4] context shapes
     (article 512, image 49, faces 4, objects 64; head-major bf16 cache): plain tell_attn_decode against
     tell_attn_decode_weights (the one-pass kernel in its exporting form + the weights kernel);
  2. the full-size faces_objects decode step (bf16, captured steps), greedy, 32 and 128 captions: attention=False against
     attention=True, legs interleaved loop by loop on the same model and batch, warm, medians (tools/bench_sampling.py's way);
  3. captions/s WITH maps: generate(attention=True) against the only way there was - fast_generation = False with
     need_attn = True on every layer (the reference's control flow, eager, a host copy per layer and context and step).
usage (GPU box): python tools/bench_attn_maps.py [--skip-model] [--gen-len N]"""
import sys
import time

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402
from tell_amd.decode import _ints, _longs, _ptrs  # noqa: E402
from tell_amd.hip import call  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'
H, E = 16, 1024
SHAPES = (('image', 49), ('article', 512), ('faces', 4), ('obj', 64))


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


def attention_launches():
    for B in (32, 128):
        g = torch.Generator(device=dev).manual_seed(B)
        bf = torch.bfloat16
        q = [(torch.randn(B, E, generator=g, device=dev) * 0.35).to(bf) for _ in SHAPES]
        k = [torch.randn(B, H, S, 64, generator=g, device=dev).to(bf).permute(2, 0, 1, 3) for _, S in SHAPES]
        v = [torch.randn(B, H, S, 64, generator=g, device=dev).to(bf).permute(2, 0, 1, 3) for _, S in SHAPES]
        mask = [(torch.arange(S, device=dev)[None, :] >= torch.randint(S // 2, S + 1, (B, 1), generator=g, device=dev))
                .to(torch.uint8).contiguous() for _, S in SHAPES]
        bk = [torch.randn(E, generator=g, device=dev).to(bf) for _ in SHAPES]
        bv = [torch.randn(E, generator=g, device=dev).to(bf) for _ in SHAPES]
        out = torch.empty(4, B, E, dtype=bf, device=dev)
        S = [s for _, s in SHAPES]
        common = (4, _ptrs(q), _longs([E] * 4), _ptrs(k), _longs([t.stride(0) for t in k]), _longs([t.stride(1) for t in k]),
                  _longs([t.stride(2) for t in k]), _ptrs(v), _longs([t.stride(0) for t in v]), _longs([t.stride(1) for t in v]),
                  _longs([t.stride(2) for t in v]), _ptrs(mask), _ptrs(bk), _ptrs(bv), 1, _ints(S),
                  _ptrs([out[i] for i in range(4)]), _longs([E] * 4), B, H, 1)
        w = [torch.empty(100, B, s + 2, dtype=torch.float32, device=dev) for s in S]
        lse = torch.empty(4, B, H, dtype=torch.float32, device=dev)
        word = torch.zeros(1, dtype=torch.int32, device=dev)
        t_plain = timeit(lambda: call('tell_attn_decode', *common))
        t_exp = timeit(lambda: call('tell_attn_decode_weights', *common, lse, _ptrs(w), _longs([x.stride(0) for x in w]),
                                    _longs([x.stride(1) for x in w]), 1, 100, word))
        kb = sum(B * H * s * 64 * 2 for s in S) / 1e6
        print('attention of one layer  rows=%3d  tell_attn_decode %7.2f us   tell_attn_decode_weights %7.2f us   (+%.2f us, %.2fx; '
              'K cache %.1f MB, %d floats of weights)' % (B, t_plain, t_exp, t_exp - t_plain, t_exp / t_plain, kb,
                                                           B * sum(s + 2 for s in S)))
        sys.stdout.flush()


def model_and_contexts(B):
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects').to(dev).eval()
    batch = synthetic_batch(B, 512, 33, True, seed=3, device=dev)
    with torch.no_grad():
        caption_ids, _, contexts = model._forward(batch['context'], batch['image'], batch['caption'], batch['face_embeds'],
                                                  batch['obj_embeds'])
    return model, caption_ids, contexts


def decode_steps(sizes=(32, 128), loops=7, gen_len=100):
    for B in sizes:
        model, caption_ids, contexts = model_and_contexts(B)
        legs = (('attention=False', False), ('attention=True', True))
        per = {name: [] for name, _ in legs}
        for it in range(2 + loops):
            for name, att in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                with torch.no_grad():
                    _, ids, _ = model._generate(caption_ids, contexts, gen_len=gen_len, attention=att)
                e1.record()
                torch.cuda.synchronize()
                if it >= 2:                                                    # (the first two loops record the graphs)
                    per[name].append(1e3 * e0.elapsed_time(e1) / (ids.shape[1] - 1))
        med = {name: sorted(v)[len(v) // 2] for name, v in per.items()}
        for name, _ in legs:
            print('decode step  B=%3d  %-16s %7.1f us per step (median of %d loops of %d steps; min %.1f max %.1f)'
                  % (B, name, med[name], loops, ids.shape[1] - 1, min(per[name]), max(per[name])))
        print('decode step  B=%3d  on / off: %.3f' % (B, med['attention=True'] / med['attention=False']))
        sys.stdout.flush()
        del model


def captions_per_second(B=32, gen_len=100, loops=3):
    model, caption_ids, contexts = model_and_contexts(B)

    def timed(fn, n):
        fn()                                                                   # warm (captures, caches)
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2]

    def new_way():
        with torch.no_grad():
            model._generate(caption_ids, contexts, gen_len=gen_len, attention=True)

    def old_way():
        model.fast_generation = False
        for layer in model.decoder.layers:
            layer.need_attn = True
        try:
            with torch.no_grad():
                model._generate(caption_ids, contexts, gen_len=gen_len)
        finally:
            model.fast_generation = True
            for layer in model.decoder.layers:
                layer.need_attn = False

    def plain():
        with torch.no_grad():
            model._generate(caption_ids, contexts, gen_len=gen_len)
    t_plain, t_new, t_old = timed(plain, loops), timed(new_way, loops), timed(old_way, 1)
    print('captions/s  B=%d x %d steps (decode loop only)  no maps %7.1f   generate(attention=True) %7.1f   '
          'fast_generation=False + need_attn %7.1f   (new / old: %.1fx)' % (B, gen_len, B / t_plain, B / t_new, B / t_old, t_old / t_new))


if __name__ == '__main__':
    gen_len = int(sys.argv[sys.argv.index('--gen-len') + 1]) if '--gen-len' in sys.argv else 100
    attention_launches()
    if '--skip-model' not in sys.argv:
        decode_steps(gen_len=gen_len)
        captions_per_second(gen_len=gen_len)
