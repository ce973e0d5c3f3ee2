#!/usr/bin/env python
"""The moving average of the weights in the BertAdam step: what it costs.
Kernel legs: flat buffers of the full decoder's size (about 176 M parameters in 330 tensors), the update launches as the
trainer issues them (clip 0.1, gradient zeroing, bf16 shadow, default adam_var), each leg captured into a hipGraph and timed
with events around single replays, the legs interleaved replay by replay, medians:
  step2     tell_bertadam_step2 - the parent commit's launch, and this commit's with the feature off: 34 B / parameter;
  step_ema  tell_bertadam_step_ema: 42 B / parameter, predicted 42 / 34 = 1.24 x;
  swap      tell_ema_swap alone: 18 B / parameter.
(The two norm launches in front of the update read 4 B / parameter more in both step legs; they are inside the timing, as
they are inside the step, and not in the 34 / 42.)
--bench: also `bench.py --gpus 1 --steps 20 --warmup 5` in child processes - this tree with the feature off, --parent DIR
(a built checkout of the parent commit) when given, and this tree with ema_decay set through the trainer's optimizer
option (bench.py itself is not edited: the child wraps Trainer.__init__ and then runs bench.py as __main__).
usage (GPU box): python tools/bench_ema.py [--loops 40] [--bench] [--parent DIR] [--out profiles/ema_bench.txt]"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


BENCH_ARGS = ['--gpus', '1', '--steps', '20', '--warmup', '5']


def bench_child(decay):
    """this process becomes `bench.py` with every Trainer it builds given ema_decay"""
    import runpy
    import tell_amd.training.trainer as tr
    init = tr.Trainer.__init__

    def with_ema(self, model, optimizer_cfg=None, *a, **kw):
        init(self, model, dict(optimizer_cfg or {}, ema_decay=decay), *a, **kw)
    tr.Trainer.__init__ = with_ema
    sys.argv = [os.path.join(ROOT, 'bench.py')] + BENCH_ARGS
    runpy.run_path(sys.argv[0], run_name='__main__')


def run_bench(cwd, cmd):
    out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900)
    line = None
    for ln in out.stdout.splitlines():
        if ln.startswith('{') and '"value"' in ln:
            line = json.loads(ln)
    if out.returncode != 0 or line is None:
        raise RuntimeError('bench failed (%d): %s' % (out.returncode, (out.stdout + out.stderr)[-2000:]))
    return line


def kernel_legs(loops, say):
    import torch
    from tell_amd import hip
    from tell_amd.training.optimizers import BertAdam, FlatParams
    hip.require_gpu()
    dev = 'cuda'
    torch.manual_seed(0)
    # the decoder's shape in round numbers: the tied 50265 x 1024 table, 29 matrices of 4096 x 1024 and 300 vectors of 1024
    shapes = [(50265, 1024)] + [(4096, 1024)] * 29 + [(1024,)] * 300
    params = [torch.nn.Parameter(torch.randn(*s, device=dev) * 0.05) for s in shapes]
    flat = FlatParams([('p%d' % i, p) for i, p in enumerate(params)], dev)
    del params
    cfg = dict(lr=1e-4, warmup=0.05, t_total=437600, b1=0.9, b2=0.98, e=1e-6, weight_decay=1e-5, max_grad_norm=0.1)
    plain = BertAdam(flat, **cfg)
    avg = BertAdam(flat, ema_decay=0.9999, **cfg)               # (the same flat buffers; this one adds flat.ema)
    skip = torch.zeros(2, dtype=torch.int32, device=dev)
    n = flat.total
    say('flat buffers: %d tensors, %.1f M parameters, %.1f M elements with the padding, adam_var %d (-1: the default)' % (
        len(shapes), flat.numel() / 1e6, n / 1e6, hip.get_option('adam_var')))

    def refill():
        flat.grad.normal_(0.0, 1e-3)

    legs = {
        'step2': lambda: plain.launch(zero_grad=True, skip=skip),
        'step_ema': lambda: avg.launch(zero_grad=True, skip=skip),
        'swap': lambda: hip.call('tell_ema_swap', flat.flat, flat.ema, flat.shadow, n),
    }
    graphs = {}
    for name, fn in legs.items():
        refill()
        fn()                                                  # warm, eager
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        graphs[name] = g
    times = {name: [] for name in legs}
    for i in range(loops + 5):
        refill()
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            if i >= 5:
                times[name].append(a.elapsed_time(b) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    bytes_per = {'step2': 34, 'step_ema': 42, 'swap': 18}
    for k in legs:
        v = sorted(times[k])
        say('%-9s median %8.1f us  (min %8.1f, max %8.1f, %d replays)  %2d B/parameter -> %.2f TB/s' % (
            k, med[k], v[0], v[-1], len(v), bytes_per[k], bytes_per[k] * n / med[k] / 1e6))
    say('step_ema / step2: measured %.3f x, predicted by the byte count 42 / 34 = %.3f x' % (med['step_ema'] / med['step2'], 42 / 34))
    say('swap / step2:     measured %.3f x, predicted by the byte count 18 / 34 = %.3f x' % (med['swap'] / med['step2'], 18 / 34))


def main():
    if '--bench-child' in sys.argv:
        return bench_child(float(_arg('--bench-child')))
    out_path = _arg('--out', os.path.join(ROOT, 'profiles', 'ema_bench.txt'))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    loops = int(_arg('--loops', 40))
    say('tools/bench_ema.py --loops %d%s' % (loops, ' --bench' if '--bench' in sys.argv else ''))
    kernel_legs(loops, say)
    if '--bench' in sys.argv:
        runs = [('this tree, feature off', ROOT, [sys.executable, 'bench.py'] + BENCH_ARGS)]
        if _arg('--parent'):
            runs.append(('parent commit', os.path.abspath(_arg('--parent')), [sys.executable, 'bench.py'] + BENCH_ARGS))
        runs.append(('this tree, ema_decay 0.9999', ROOT, [sys.executable, os.path.join('tools', 'bench_ema.py'),
                                                             '--bench-child', '0.9999']))
        say('bench.py ' + ' '.join(BENCH_ARGS) + ' (one child process each, in this order):')
        for name, cwd, cmd in runs:
            r = run_bench(cwd, cmd)
            say('  %-28s %8.1f %s, %.3f ms/step, spread of the windows %s' % (
                name, r['value'], r['unit'], r['ms_per_step'], r.get('spread')))
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
