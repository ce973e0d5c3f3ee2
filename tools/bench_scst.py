#!/usr/bin/env python
"""The self-critical training step against its parts.  Full-size faces_objects model, bf16, top-k 64
sampling, B = 32 images with 512-token articles, n = 4 samples per image.  Each leg inside its own pair of events, after warm-up
(the decode graphs, the encoder graphs and the plain step's graph are recorded first), median of --loops calls:
  scst      Trainer.train_self_critical(batch, n_samples=4): encode, generate, reward, the weighted pass at 128 rows, update;
  generate  model.generate(n_samples=4, rank_by='draw') alone, its encoders included;
  plain     Trainer.train_one_batch on the same batch repeated to 128 rows alone (captured), its encoders included;
  reward    tell_caption_reward alone on the captions the scst leg drew.
No speed is promised: the file records how far the SCST step is from the sum of its parts (the step encodes once where
generate + plain encode twice, 32 and 128 images; its training pass is issued kernel by kernel where the plain step replays a graph).
usage (GPU box): python tools/bench_scst.py [--loops 5] [--batch 32] [--n 4] [--out profiles/scst_bench.txt]"""
import sys

import torch

sys.path.insert(0, '.')
import tell_amd  # noqa: E402

tell_amd.hip.require_gpu()
dev = 'cuda'


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


LOOPS, B, N = int(_arg('--loops', 5)), int(_arg('--batch', 32)), int(_arg('--n', 4))
OUT = _arg('--out', 'profiles/scst_bench.txt')


def repeat(batch, n):
    return {k: ({kk: vv.repeat_interleave(n, dim=0) for kk, vv in v.items()} if isinstance(v, dict)
                else v.repeat_interleave(n, dim=0)) for k, v in batch.items()}


def clone(batch):
    return {k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()}


def timed(fn, warm, loops):
    ms = []
    for it in range(warm + loops):
        torch.manual_seed(11 + it)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warm:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1], out


def main():
    from tell_amd import ops
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    from tell_amd.training import Trainer
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = build_model('faces_objects', sampling_topk=64).to(dev)
    trainer = Trainer(model, device=dev, capture_after=1)
    batch = synthetic_batch(B, 512, 33, True, seed=3, device=dev)
    wide = repeat(batch, N)
    lines = ['self-critical step against its parts: faces_objects, bf16, top-k 64, B = %d images, n = %d, 512-token articles; '
             'ms per call, median of %d (min .. max)' % (B, N, LOOPS)]

    def generate():
        model.eval()
        with torch.no_grad():
            return model.generate(**clone(batch), n_samples=N, rank_by='draw')
    legs = {}
    legs['scst'] = timed(lambda: trainer.train_self_critical(clone(batch), n_samples=N), 3, LOOPS)
    legs['generate'] = timed(generate, 3, LOOPS)
    legs['plain'] = timed(lambda: trainer.train_one_batch(clone(wide)), 4, LOOPS)
    ids = legs['scst'][3]['gen_ids_samples']
    flat = ids.reshape(B * N, -1).contiguous()
    ref = batch['caption']['roberta']
    legs['reward'] = timed(lambda: ops.caption_reward(flat, ref, B, N, flat.shape[1] - 1, ref.shape[1] - 1, 1, 2, 4), 3,
                           max(LOOPS, 20))
    for leg in ('scst', 'generate', 'plain', 'reward'):
        med, lo, hi, _ = legs[leg]
        lines.append('%-9s %9.3f  (%.3f .. %.3f)' % (leg, med, lo, hi))
    parts = sum(legs[k][0] for k in ('generate', 'plain', 'reward'))
    lines.append('sum of the parts %.3f ms; scst / sum of the parts = %.3f  (%d decode steps in the last scst call)'
                 % (parts, legs['scst'][0] / parts, ids.shape[2] - 1))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(OUT, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
