#!/usr/bin/env python
"""n sampled captions per image: generate(n_samples=n) against the repeated batch.
Full-size faces_objects model, bf16, captured steps, B = 32 images with 512-token articles, n in {2, 4, 8}, top-k 64 and
nucleus 0.9 (T = 1).  Two legs per setting, whole `generate` calls - encoders, K/V projection, decode loop, ranking:
  shared    generate(**batch, n_samples=n): the encoders and the context K/V once, B * n decode rows over a cache of width B;
  repeated  generate(**batch with every image n times): what the parent commit can run - B * n images through the encoders,
            B * n decode rows over a cache of width B * n.
The legs alternate call by call on the same model, warm (captures recorded first); every leg is measured in TWO runs of
`--loops` calls each, so that the run-to-run spread stands beside the difference.  Captions per second = B * n / median call.
--repeated-only runs the repeated leg alone (it needs nothing this tool's commit added: the same file times the parent commit).
Before the legs (not with --repeated-only): tell_sample_rank alone at B = 32, 100 steps, n in {2, 4, 8, 16}.
usage (GPU box): python tools/bench_n_samples.py [--repeated-only] [--loops 5] [--n 2,4,8]"""
import sys

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'
REPEATED_ONLY = '--repeated-only' in sys.argv


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


LOOPS = int(_arg('--loops', 5))
NS = [int(v) for v in str(_arg('--n', '2,4,8')).split(',')]
B = int(_arg('--batch', 32))
SETTINGS = (('top-k 64', dict(sampling_topk=64, sampling_topp=None)), ('nucleus 0.9', dict(sampling_topk=0, sampling_topp=0.9)))


def repeat(batch, n):
    return {k: ({kk: vv.repeat_interleave(n, dim=0) for kk, vv in v.items()} if isinstance(v, dict)
                else v.repeat_interleave(n, dim=0)) for k, v in batch.items()}


def clone(batch):
    return {k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()}


def main():
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects').to(dev).eval()
    batch = synthetic_batch(B, 512, 33, True, seed=3, device=dev)
    for name, setting in SETTINGS:
        for k_, v_ in setting.items():
            setattr(model, k_, v_)
        for n in NS:
            wide = repeat(batch, n)
            legs = [('repeated', lambda: model.generate(**clone(wide)))]
            if not REPEATED_ONLY:
                legs.insert(0, ('shared', lambda: model.generate(**clone(batch), n_samples=n)))
            runs = {leg: [[], []] for leg, _ in legs}
            steps = {}
            for run in range(2):
                for it in range((3 if run == 0 else 1) + LOOPS):       # (the first calls record the graphs)
                    for leg, fn in legs:
                        torch.manual_seed(11 + it)
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        with torch.no_grad():
                            out = fn()
                        e1.record()
                        torch.cuda.synchronize()
                        steps[leg] = out['gen_ids'].shape[1] - 1
                        if it >= (3 if run == 0 else 1):
                            runs[leg][run].append(e0.elapsed_time(e1))
            rate = {}
            for leg, _ in legs:
                med = [sorted(v)[len(v) // 2] for v in runs[leg]]
                rate[leg] = [1e3 * B * n / m for m in med]
                print('%-11s B=%d n=%d  %-8s  run 1 %7.1f ms  run 2 %7.1f ms  (median of %d calls, %d steps; min %.1f max %.1f)  '
                      '%7.1f / %7.1f captions/s' % (name, B, n, leg, med[0], med[1], LOOPS, steps[leg], min(sum(runs[leg], [])),
                                                    max(sum(runs[leg], [])), rate[leg][0], rate[leg][1]))
            if len(legs) > 1:
                s, r = rate['shared'], rate['repeated']
                spread = max(abs(s[0] - s[1]) / max(s), abs(r[0] - r[1]) / max(r))
                print('%-11s B=%d n=%d  shared / repeated: %.3f (run 1) %.3f (run 2); run-to-run spread of a leg: %.1f %%'
                      % (name, B, n, s[0] / r[0], s[1] / r[1], 100 * spread))
            sys.stdout.flush()


def rank_cost(steps=100, reps=50):
    """tell_sample_rank alone: B images, n hypotheses of `steps` tokens over a 200-token alphabet that never end (the most
    work a caption of that length gives), microseconds per launch, median of 5 rounds of `reps` launches."""
    from tell_amd import ops
    g = torch.Generator().manual_seed(5)
    for n in (2, 4, 8, 16):
        ids = torch.randint(3, 200, (B * n, steps + 1), generator=g).to(dev)
        lps = (-torch.rand(B * n, steps, generator=g)).to(dev)
        done = torch.full((B * n,), steps, dtype=torch.long, device=dev)
        for rule in ('score', 'consensus'):
            per = []
            for _ in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    ops.sample_rank(ids, lps, done, B, n, steps, 1, 2, rule)
                e1.record()
                torch.cuda.synchronize()
                per.append(1e3 * e0.elapsed_time(e1) / reps)
            per = sorted(per[1:])
            print('tell_sample_rank  B=%d n=%2d steps=%d  %-9s %8.1f us per launch (median of 5 x %d; min %.1f max %.1f)'
                  % (B, n, steps, rule, per[2], reps, per[0], per[-1]))
    sys.stdout.flush()


if __name__ == '__main__':
    if not REPEATED_ONLY:
        rank_cost()
    main()
