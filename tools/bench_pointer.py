"""Time the copy head of transformer_pointer(_2) (csrc/copy.hip) at B = 32, S = 512, T = 48 in bf16, forward + backward,
against the same arithmetic written the reference's way in ATen (pointer_loss :180-313: per-head bmm scores, softmax,
head mean, unique + scatter_add_ over the reduced vocabulary, a host loop over entity indices), alternating in one
process.  Also the per-step cost of the copy decision of generation (tell_copy_step) for 32 rows.

Eager launches timed with CUDA events (no hipGraph): the number includes the launch overhead of the Python wrappers.
The projections (in_proj rows, the entity attention's q/k/v/out GehringLinears) are the library's GEMMs in both legs and
are left out of both; what is timed is the part this head adds.  Prints one JSON line."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tell_amd  # noqa: E402
from tell_amd import ops  # noqa: E402

B, S, T, H, D = 32, 512, 48, 16, 64
E = H * D


def inputs(dtype):
    g = torch.Generator().manual_seed(0)
    q = (torch.randn(T, B, E, generator=g) * 0.1).cuda().to(dtype)
    k = (torch.randn(S, B, E, generator=g) * 0.1).cuda().to(dtype)
    bk = torch.nn.Parameter((torch.randn(1, 1, E, generator=g) * 0.1).cuda())
    mask = torch.zeros(B, S, dtype=torch.uint8, device='cuda')
    proper = (torch.rand(B, S, generator=g) > 0.5).to(torch.int8).cuda()
    ctx = torch.randint(3, 5000, (B, S), generator=g).cuda()
    tgt = ctx[:, :T].clone()
    cm = torch.zeros(B, T, dtype=torch.long)
    cm[:, 1:4] = 1
    cm[:, 7:9] = 2
    cm[:, 12] = 3
    return q, k, bk, mask, proper, ctx, tgt, cm.cuda()


def hip_head(q, k, bk, mask, proper, ctx, tgt, cm, x, g, v, b):
    q = q.detach().requires_grad_()
    k = k.detach().requires_grad_()
    w = ops.copy_attention(q, k, bk, mask, proper, H, p=0.1, training=True)
    loss = ops.copy_loss(w, ctx, tgt, cm, 2, 50265)
    xe = x.detach().requires_grad_()
    att = ops.causal_attention(xe, xe, xe, H, D ** -0.5)
    el, _ = ops.entity_head(att, g, v, b, cm)
    (loss + el).backward()


def aten_head(q, k, bk, mask, proper, ctx, tgt, cm, x, g, v, b):
    q = q.detach().float().requires_grad_()
    k = k.detach().float().requires_grad_()
    qh = q.reshape(T, B * H, D).transpose(0, 1)
    kk = torch.cat([k, bk.expand(1, B, E).float(), k.new_zeros(1, B, E)])
    kh = kk.reshape(S + 2, B * H, D).transpose(0, 1)
    lg = torch.bmm(qh, kh.transpose(1, 2)).view(B, H, T, S + 2)
    lg = lg.masked_fill(torch.cat([mask.bool(), mask.new_zeros(B, 2).bool()], 1)[:, None, None], -math.inf)
    p = torch.nn.functional.dropout(torch.softmax(lg, -1), 0.1, True)
    w = p.mean(1)[:, :, :-2].clone()
    w[(proper < 1)[:, None, :].expand_as(w)] = 0
    uniq = torch.cat([ctx, tgt], 1).unique()
    V = len(uniq)
    inv = uniq.new_full([50265], -1)
    inv.index_copy_(0, uniq, torch.arange(V, device='cuda'))
    probs = w.new_zeros(B, T, V).scatter_add_(2, inv.index_select(0, ctx.reshape(-1)).view(B, 1, S).expand(B, T, S), w)
    lp = probs.new_zeros(probs.shape)
    lp[probs > 0] = torch.log(probs[probs > 0])
    lp = lp.view(B * T, V)
    nt = inv.index_select(0, tgt.reshape(-1)).reshape(-1, 1)
    loss = w.new_zeros(())
    for i in range(1, int(cm.max().item()) + 1):
        sel = (cm == i).view(-1)
        loss = loss + torch.nn.functional.cross_entropy(lp[sel], nt[sel].squeeze(1))
    xe = x.detach().float().requires_grad_()
    xh = xe.reshape(T, B * H, D).transpose(0, 1)
    a = torch.bmm(xh * D ** -0.5, xh.transpose(1, 2))
    a = a.masked_fill(torch.ones(T, T, dtype=torch.bool, device='cuda').triu(), -math.inf)
    a = torch.cat([a.new_zeros(B * H, T, 1), a], -1)
    att = torch.bmm(torch.softmax(a, -1)[..., 1:], xh).transpose(0, 1).reshape(T, B, E)
    wt = g * v / v.norm(dim=1, keepdim=True)
    tr = cm.clone()
    tr[tr > 1] = 1
    el = torch.nn.functional.cross_entropy((att.transpose(0, 1) @ wt.t() + b).reshape(-1, 2), tr.reshape(-1),
                                           ignore_index=-1)
    (loss + el).backward()


def timed(fn, args, n):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn(*args)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / n


def main():
    tell_amd.hip.require_gpu()
    tell_amd.set_compute_dtype(torch.bfloat16)
    q, k, bk, mask, proper, ctx, tgt, cm = inputs(torch.bfloat16)
    x = (torch.randn(T, B, E, device='cuda') * 0.5).to(torch.bfloat16)
    from tell_amd.modules.linear import GehringLinear
    fc = GehringLinear(E, 2).cuda()
    args = (q, k, bk, mask, proper, ctx, tgt, cm, x, fc.weight_g, fc.weight_v, fc.bias)
    for fn in (hip_head, aten_head):
        timed(fn, args, 3)
    hip_ms, aten_ms = [], []
    for _ in range(5):                                        # alternating windows
        hip_ms.append(timed(hip_head, args, 20))
        aten_ms.append(timed(aten_head, args, 20))
    rows = torch.arange(B, dtype=torch.int32, device='cuda')
    ent = torch.tensor([[0., 1.]], device='cuda').expand(B, 2).contiguous()
    gen = torch.full((B,), 7, dtype=torch.long, device='cuda')
    hist = torch.full((B, 101), -1, dtype=torch.long, device='cuda')
    q1 = q[0].contiguous()
    step = timed(lambda: ops.copy_step(q1, k, bk, mask, proper, ctx, rows, ent, gen, hist, 50, H), (), 200)
    hip_med, aten_med = sorted(hip_ms)[2], sorted(aten_ms)[2]
    # bytes the head must move at least: K (bf16) read by the copy attention forward and twice in backward, dK written,
    # W [B,T,S] fp32 written / read / dW written / read
    kbytes = S * B * E * 2
    wbytes = B * T * S * 4
    min_bytes = 4 * kbytes + 4 * wbytes
    flops = 2 * B * H * T * (S + 2) * D * 3                  # scores fwd, dq, dk (no PV)
    print(json.dumps({'metric': 'copy head fwd+bwd (B=32, S=512, T=48, bf16, eager)', 'hip_ms': round(hip_med, 4),
                      'aten_ms': round(aten_med, 4), 'speedup': round(aten_med / hip_med, 2),
                      'hip_windows_ms': [round(t, 4) for t in hip_ms], 'aten_windows_ms': [round(t, 4) for t in aten_ms],
                      'copy_step_us_32_rows': round(step * 1000, 2), 'min_bytes': min_bytes,
                      'score_flops': flops}))


if __name__ == '__main__':
    main()
