"""What the copy models' cached generation costs and saves, at B = 32, S = 512, bf16:
  1. the kernels, as hipGraph replays of 20 launches, legs interleaved, medians: tell_copy_step against tell_copy_decide (both
     of its launches; and both launches with every row finished, i.e. what two launches cost when they do nothing), and
     tell_causal_attn_fwd in its step form against tell_entity_attn_step, at step 50 of a history of 100;
  2. the whole decode loop of a full-size transformer_pointer: the eager loop (_generate_pointer, what generate() runs by default
     and what the parent commit ran) against the cached, captured step (_generate_pointer_cached), encoders excluded, legs
     interleaved, medians - microseconds per decode step and captions per second for the 32-caption batch.
Nothing here is a gate: the numbers go to profiles/copy_decode_bench.txt.
usage (GPU box): python tools/bench_copy_decode.py [--skip-model] [--skip-kernels]"""
import sys

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402
from tell_amd.hip import call  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'
B, S, H, D, L = 32, 512, 16, 64, 100
E = H * D


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


def kernels():
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(0)
    q = (torch.randn(B, E, generator=g) * 0.1).to(dev).to(bf)
    k_bse = (torch.randn(B, S, E, generator=g) * 0.1).to(dev).to(bf)             # the article keys as _copy_k stores them
    k = k_bse.transpose(0, 1)
    bk = (torch.randn(E, generator=g) * 0.1).to(dev).to(bf)
    mask = torch.zeros(B, S, dtype=torch.uint8, device=dev)
    proper = (torch.rand(B, S, generator=g) > 0.5).to(torch.int8).to(dev)
    ctx = torch.randint(3, 5000, (B, S), generator=g).to(dev)
    ent = torch.tensor([[0., 1.]], device=dev).expand(B, 2).contiguous()
    rows = torch.arange(B, dtype=torch.int32, device=dev)
    gen64, gen32 = torch.full((B,), 7, dtype=torch.long, device=dev), torch.full((B,), 7, dtype=torch.int32, device=dev)
    hist64 = torch.full((B, L + 1), -1, dtype=torch.long, device=dev)
    hist32 = torch.full((B, L + 1), -1, dtype=torch.int32, device=dev)
    tok64, tok32 = torch.empty(B, dtype=torch.long, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    cp1, pr1 = torch.empty(B, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
    cp, pr = torch.zeros(B, L + 1, dtype=torch.uint8, device=dev), torch.zeros(B, L, dtype=torch.float32, device=dev)
    scratch = torch.empty(B, H, S, dtype=torch.float32, device=dev)
    none, every = torch.zeros(B, dtype=torch.uint8, device=dev), torch.ones(B, dtype=torch.uint8, device=dev)
    dt = tell_amd.hip.dt(bf)

    def step():
        call('tell_copy_step', q, E, k, k.stride(0), k.stride(1), bk, mask, proper, ctx, rows, ent, gen64, hist64, L + 1, 50, B, H,
             S, D, tok64, cp1, pr1, dt)

    def decide(fin):
        call('tell_copy_decide', q, E, k, k.stride(0), k.stride(1), bk, mask, proper, ctx, ent, gen32, fin, hist32, L + 1, cp, L + 1,
             pr, L, L, 49, None, B, H, S, D, scratch, tok32, dt)
    med = time_legs([('tell_copy_step', step), ('tell_copy_decide', lambda: decide(none)),
                     ('tell_copy_decide, every row finished', lambda: decide(every))])
    kbytes, sbytes = B * S * E * 2, 2 * B * H * S * 4                             # keys read once; scratch written and read
    for name, us in med.items():
        print('copy decision  B=%d S=%d bf16  %-40s %8.2f us' % (B, S, name, us))
    print('copy decision  tell_copy_step / tell_copy_decide: %.2f x' % (med['tell_copy_step'] / med['tell_copy_decide']))
    print('copy decision  traffic floor: %.1f MB of keys + %.1f MB of scratch = %.1f MB; tell_copy_decide moves them at %.0f GB/s'
          % (kbytes / 1e6, sbytes / 1e6, (kbytes + sbytes) / 1e6, (kbytes + sbytes) / med['tell_copy_decide'] / 1e3))
    # the entity attention of step p = 50: the step form of the training kernel over a history of 51 rows against the
    # static-history kernel (which also appends row 50)
    p = 50
    x, kn, vn = ((torch.randn(B, E, generator=g) * 0.5).to(dev).to(bf) for _ in range(3))
    kh, vh = ((torch.randn(L, B, E, generator=g) * 0.5).to(dev).to(bf) for _ in range(2))
    out1, lse = torch.empty(1, B, E, dtype=bf, device=dev), torch.empty(B, H, 1, dtype=torch.float32, device=dev)
    out2 = torch.empty(B, E, dtype=bf, device=dev)
    med = time_legs([
        ('tell_causal_attn_fwd, step form', lambda: call('tell_causal_attn_fwd', x, kh, vh, out1, lse, B, H, 1, p + 1, 64, p, B * E, E,
                                                         B * E, E, B * E, E, B * E, E, 0.125, dt)),
        ('tell_entity_attn_step', lambda: call('tell_entity_attn_step', x, E, kn, E, vn, E, kh, vh, B * E, E, out2, E, B, H, 64, L,
                                               0.125, p, None, dt))])
    for name, us in med.items():
        print('entity attention  B=%d step %d bf16  %-34s %8.2f us' % (B, p, name, us))
    sys.stdout.flush()


def decode_loop(loops=5):
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('pointer').to(dev).eval()
    batch = synthetic_batch(B, S, 33, True, seed=3, device=dev)
    g = torch.Generator().manual_seed(5)
    context = batch['context']
    context['roberta_proper_masks'] = (torch.rand(context['roberta'].shape, generator=g) > 0.5).long().to(dev)
    with torch.no_grad():
        enc = model.encode(context, batch['image'])
        caption_ids, _, contexts = model._forward(context, batch['image'], batch['caption'], batch['face_embeds'], None, enc)
    legs = [('eager loop', model._generate_pointer), ('cached, captured', model._generate_pointer_cached)]
    per, steps, copies = {n: [] for n, _ in legs}, {}, {}
    for it in range(2 + loops):
        for name, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            with torch.no_grad():
                ids, _, sc, _ = fn(caption_ids, contexts, enc, context)
            e1.record()
            torch.cuda.synchronize()
            if it >= 2:                                                       # (the first two loops record the graphs)
                per[name].append(e0.elapsed_time(e1))
                steps[name], copies[name] = ids.shape[1] - 1, int(sc[:, 1:].sum())
    med = {n: sorted(v)[len(v) // 2] for n, v in per.items()}
    for name, _ in legs:
        print('decode loop  B=%d S=%d bf16  %-17s %8.1f ms for %3d steps = %7.1f us per step, %6.1f captions/s  (median of %d '
              'loops; min %.1f max %.1f ms; %d copies)' % (B, S, name, med[name], steps[name], 1e3 * med[name] / steps[name],
                                                           B / (med[name] / 1e3), loops, min(per[name]), max(per[name]), copies[name]))
    a, b = legs[0][0], legs[1][0]
    print('decode loop  eager / cached per step: %.2f x' % ((med[a] / steps[a]) / (med[b] / steps[b])))
    h = [h for sig, h in model.__dict__['_decode_graphs'].items() if ('hidden',) in sig]
    print('decode loop  captured: %s; tail inside the captured step: %s; multi-step graphs: %s'
          % ([x['graph'] not in (None, False) for x in h], [bool(x.get('graph_has_post')) for x in h],
             [[k for k in x if isinstance(k, tuple) and k[:1] == ('multi',) and len(k) == 2 and x[k]] for x in h]))
    sys.stdout.flush()


if __name__ == '__main__':
    if '--skip-kernels' not in sys.argv:
        kernels()
    if '--skip-model' not in sys.argv:
        decode_loop()
