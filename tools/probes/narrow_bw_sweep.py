"""Each of the step's six long bandwidth-bound launches ALONE on an idle GPU, wide (bw_wgs = 0) and in the narrow form at
G = 32 / 48 / 64 / 96 / 128 workgroups, at the sizes of the configs[2] step: BertAdam and its norm
pass over 176 M parameters (fp32 gradient, bf16 shadow, zeroing, one clip threshold), the 25-layer mix over 32 x 512 x 1024
bf16 elements forward and backward (1024 blocks, as ops.MixFn launches it), and the two multi weight-norm launches over 20
matrices of the decoder's two shapes (336 MB of fp32; the decoder's own 20 add up to 372 MB).  HIP events around every
launch, median of 10 after 3 warm launches; r = narrow / wide.
  python tools/probes/narrow_bw_sweep.py [G ...]"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import tell_amd                                             # noqa: E402
from tell_amd import hip                                    # noqa: E402

hip.require_gpu()
GS = [int(a) for a in sys.argv[1:]] or [32, 48, 64, 96, 128]
dev = 'cuda'
CH = hip.lib().tell_opt_chunk()


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1))
    return statistics.median(out)


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def ints(vs):
    return (ctypes.c_int * len(vs))(*vs)


cases = {}

# ---- BertAdam: 40 tensors of 4.4 M parameters
n_t, per = 40, 4300 * CH
n = n_t * per
p = torch.randn(n, device=dev) * 0.1
g = torch.randn(n, device=dev) * 0.01
m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
shadow = torch.empty(n, dtype=torch.bfloat16, device=dev)
n_chunks = n // CH
chunk_tensor = (torch.arange(n_chunks, device=dev) // (per // CH)).int()
chunk_begin = (torch.arange(n_t + 1, device=dev) * (per // CH)).long()
partial, norms = torch.empty(n_chunks, device=dev), torch.empty(n_t, device=dev)
lr = torch.full((1,), 1e-4, device=dev)


def adam(max_norm):
    return lambda: hip.call('tell_bertadam_step2', p, g, m, v, chunk_tensor, chunk_begin, n_chunks, n_t, partial, norms, lr,
                            0.9, 0.98, 1e-6, 1e-2, max_norm, 1.0, shadow, 1, None, None, None, 0.0, -1.0, -1.0, None)


cases['bertadam_update (no norm pass)'] = adam(0.0)
cases['bertadam_update + sqsum_chunks + tensor_norms'] = adam(0.1)

# ---- layer mix
L, nm = 25, 32 * 512 * 1024
H = torch.randn(L, nm, device=dev).bfloat16()
w = torch.randn(L, device=dev)
out, dout = torch.empty(nm, dtype=torch.bfloat16, device=dev), torch.randn(nm, device=dev).bfloat16()
mpart = torch.empty(1024, L, device=dev)
cases['mix_fwd_vec'] = lambda: hip.call('tell_mix_fwd', H, w, L, nm, out, hip.BF16)
cases['mix_bwd_vec'] = lambda: hip.call('tell_mix_bwd', H, dout, L, nm, mpart, 1024, hip.BF16)

# ---- weight norm over 20 matrices
shapes = [(4096, 1024)] * 10 + [(1024, 4096)] * 10
wg = [torch.randn(r, device=dev) for r, c in shapes]
wv = [torch.randn(r, c, device=dev) for r, c in shapes]
ww = [torch.empty(r, c, dtype=torch.bfloat16, device=dev) for r, c in shapes]
wn = [torch.empty(r, device=dev) for r, c in shapes]
dW = [torch.randn(r, c, device=dev) for r, c in shapes]
dg = [torch.zeros(r, device=dev) for r, c in shapes]
dv = [torch.zeros(r, c, device=dev) for r, c in shapes]
rows, cols, store = ints([r for r, c in shapes]), ints([c for r, c in shapes]), ints([1] * len(shapes))
cases['wn_multi forward'] = lambda: hip.call('tell_wn_weight_multi', len(shapes), ptrs(wg), ptrs(wv), ptrs(ww), ptrs(wn), rows,
                                             cols, hip.BF16)
cases['wn_multi backward'] = lambda: hip.call('tell_wn_backward_multi2', len(shapes), ptrs(dW), ptrs(wg), ptrs(wv), ptrs(wn),
                                              rows, cols, ptrs(dg), ptrs(dv), store)

print('%-48s %9s' % ('launch (us, median of 10)', 'wide') + ''.join(' %7s     r' % ('G=%d' % G) for G in GS))
total = {G: 0.0 for G in [0] + GS}
for name, fn in cases.items():
    row = {}
    for G in [0] + GS:
        with hip.options(bw_wgs=G):
            row[G] = timed(fn)
        if 'no norm pass' not in name:
            total[G] += row[G]
    print('%-48s %9.1f' % (name, row[0]) + ''.join(' %7.1f %5.2f' % (row[G], row[G] / row[0]) for G in GS), flush=True)
print('%-48s %9.1f' % ('sum (update counted once)', total[0]) + ''.join(' %7.1f %5.2f' % (total[G], total[G] / total[0]) for G in GS))
