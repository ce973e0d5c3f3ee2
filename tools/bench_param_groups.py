#!/usr/bin/env python
"""BertAdam's parameter groups: what the per-chunk lookup costs.
Flat buffers of the full decoder's size (the layout of tools/bench_ema.py: about 176 M parameters in 330 tensors), the update
launches as the trainer issues them (gradient zeroing, bf16 shadow, skip flag, default adam_var), each leg captured into a
hipGraph and timed with events around single replays, the legs interleaved replay by replay, medians:
  step2, step2_again    tell_bertadam_step2 - the parent commit's launch sequence (its kernels are unchanged instruction for
                        instruction), captured twice: the difference of the two is the spread the yardstick has by itself;
  groups_2 / _6 / _16   tell_bertadam_step_groups, tensor i in group i mod n - neighbouring tensors always differ - and
                        rows that differ in every value;
  ema, ema_groups_*     the same with the moving average (tell_bertadam_step_ema; 42 instead of 34 B / parameter).
By bytes the grouped pass moves what the plain pass moves: the prediction is 1.00 x, the lookups are what is measured.
usage (GPU box): python tools/bench_param_groups.py [--loops 40] [--out profiles/param_groups_bench.txt]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def alternating(n_tensors, n):
    """AllenNLP-style groups that put tensor p<i> into group i mod n (the last one is the default group)"""
    return [[['^p%d$' % i for i in range(k, n_tensors, n)],
             {'lr': 1e-4 * (1 + 0.1 * (k + 1)), 'warmup': 0.05 + 1e-3 * (k + 1), 't_total': 437600 + k + 1,
              'b1': 0.9 - 0.01 * (k + 1), 'b2': 0.98 - 1e-3 * (k + 1), 'e': 1e-6 * (k + 2), 'weight_decay': 1e-5 * (k + 2),
              'max_grad_norm': 0.1 * (k + 2)}] for k in range(n - 1)]


def main():
    import torch
    from tell_amd import hip
    from tell_amd.training.optimizers import BertAdam, FlatParams
    out_path = _arg('--out', os.path.join(ROOT, 'profiles', 'param_groups_bench.txt'))
    loops = max(int(_arg('--loops', 40)), 15)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say('tools/bench_param_groups.py --loops %d' % loops)
    hip.require_gpu()
    dev = 'cuda'
    torch.manual_seed(0)
    shapes = [(50265, 1024)] + [(4096, 1024)] * 29 + [(1024,)] * 300
    params = [torch.nn.Parameter(torch.randn(*s, device=dev) * 0.05) for s in shapes]
    flat = FlatParams([('p%d' % i, p) for i, p in enumerate(params)], dev)
    del params
    cfg = dict(lr=1e-4, warmup=0.05, t_total=437600, b1=0.9, b2=0.98, e=1e-6, weight_decay=1e-5, max_grad_norm=0.1)
    skip = torch.zeros(2, dtype=torch.int32, device=dev)
    say('flat buffers: %d tensors, %.1f M parameters, %.1f M elements with the padding, adam_var %d (-1: the default)' % (
        len(shapes), flat.numel() / 1e6, flat.total / 1e6, hip.get_option('adam_var')))

    legs = [('step2', None, None), ('groups_2', 2, None), ('groups_6', 6, None), ('groups_16', 16, None),
            ('step2_again', None, None), ('ema', None, 0.9999), ('ema_groups_2', 2, 0.9999), ('ema_groups_6', 6, 0.9999),
            ('ema_groups_16', 16, 0.9999)]
    graphs, alive = {}, []
    for name, n, decay in legs:
        opt = BertAdam(flat, parameter_groups=alternating(len(shapes), n) if n else None, ema_decay=decay, **cfg)
        assert len(opt.groups) == (n or 1)
        alive.append((opt, flat.tensor_group))                # (a captured launch holds the pointer of ITS tensor_group)
        flat.grad.normal_(0.0, 1e-3)
        opt.launch(zero_grad=True, skip=skip)                 # warm, eager
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            opt.launch(zero_grad=True, skip=skip)
        graphs[name] = g
    times = {name: [] for name, _, _ in legs}
    for i in range(loops + 5):
        flat.grad.normal_(0.0, 1e-3)
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            if i >= 5:
                times[name].append(a.elapsed_time(b) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    for name, n, decay in legs:
        v = sorted(times[name])
        per = 42 if decay else 34
        say('%-14s median %8.1f us  (min %8.1f, max %8.1f, %d replays)  %2d B/parameter -> %.2f TB/s' % (
            name, med[name], v[0], v[-1], len(v), per, per * flat.total / med[name] / 1e6))
    say('spread of the yardstick: step2_again / step2 = %.4f x' % (med['step2_again'] / med['step2']))
    for n in (2, 6, 16):
        say('%2d groups: %.4f x of step2 (%+.1f us), with the average %.4f x of ema (%+.1f us); predicted by the byte count 1.00 x'
            % (n, med['groups_%d' % n] / med['step2'], med['groups_%d' % n] - med['step2'],
               med['ema_groups_%d' % n] / med['ema'], med['ema_groups_%d' % n] - med['ema']))
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
