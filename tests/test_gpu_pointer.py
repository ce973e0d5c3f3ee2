"""The copy-mechanism kernels of transformer_pointer(_2) (csrc/copy.hip) against fp32 torch restatements of the
reference's arithmetic (transformer_pointer.py pointer_loss / _generate, multi_head.py score forward,
downsampled_single_head.py with _mask_future_full + scalar_bias), and the models end to end."""
import math

import pytest
import torch

import tell_amd
from tell_amd import ops

pytestmark = pytest.mark.gpu

H, D = 16, 64
E = H * D


@pytest.fixture(autouse=True)
def _fp32():
    tell_amd.hip.require_gpu()
    prev = tell_amd.compute_dtype()
    tell_amd.set_compute_dtype(torch.float32)
    yield
    tell_amd.set_compute_dtype(prev)


def ref_copy_attn(q, k, bias_k, mask, proper):
    """q [T,B,E] scaled, k [S,B,E] -> [B,T,S] head mean, virtual columns dropped, proper < 1 zeroed."""
    T, B, _ = q.shape
    S = k.shape[0]
    qh = q.reshape(T, B, H, D).permute(1, 2, 0, 3)                       # B H T D
    kh = torch.cat([k, bias_k.reshape(1, 1, E).expand(1, B, E), torch.zeros(1, B, E, dtype=k.dtype, device=k.device)])
    kh = kh.reshape(S + 2, B, H, D).permute(1, 2, 0, 3)                  # B H S+2 D
    lg = qh @ kh.transpose(-1, -2)
    if mask is not None:
        m = torch.cat([mask.bool(), torch.zeros(B, 2, dtype=torch.bool, device=q.device)], 1)
        lg = lg.masked_fill(m[:, None, None, :], -math.inf)
    w = torch.softmax(lg, -1).mean(1)[:, :, :S]
    if proper is not None:
        w = w.masked_fill((proper < 1)[:, None, :], 0.)
    return w


def ref_copy_loss(w, ctx, tgt, cm, variant):
    """pointer_loss :253-313 as the reference writes it (unique, scatter_add_, a loop over entity indices)."""
    B, T, S = w.shape
    uniq = torch.cat([ctx, tgt], 1).unique()
    V = len(uniq)
    inv = torch.full((int(uniq.max()) + 1,), -1, dtype=torch.long, device=w.device)
    inv[uniq] = torch.arange(V, device=w.device)
    probs = w.new_zeros(B, T, V).scatter_add(2, inv[ctx].unsqueeze(1).expand(B, T, S), w)
    lprobs = torch.where(probs > 0, torch.log(probs.clamp_min(1e-30)), torch.zeros_like(probs)).view(B * T, V)
    nt = inv[tgt].reshape(-1, 1)
    loss = w.new_zeros(())
    for i in range(1, int(cm.max()) + 1):
        sel = (cm == i).view(-1)
        if variant == 1:
            loss = loss + (-lprobs[sel].gather(-1, nt[sel])).mean()
        else:
            loss = loss + torch.nn.functional.cross_entropy(lprobs[sel], nt[sel].squeeze(1))
    return loss


def ref_causal(q, k, v, scale):
    T, B, _ = q.shape
    qh, kh, vh = (t.reshape(T, B, H, D).permute(1, 2, 0, 3) for t in (q, k, v))
    lg = (qh * scale) @ kh.transpose(-1, -2)
    lg = lg.masked_fill(torch.ones(T, T, dtype=torch.bool, device=q.device).triu(), -math.inf)
    lg = torch.cat([torch.zeros(B, H, T, 1, device=q.device), lg], -1)
    p = torch.softmax(lg, -1)[..., 1:]
    return (p @ vh).permute(2, 0, 1, 3).reshape(T, B, E)


def _inputs(B, T, S, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(T, B, E, generator=g) * 0.3).cuda().to(dtype)
    k = (torch.randn(S, B, E, generator=g) * 0.3).cuda().to(dtype)
    bk = (torch.randn(1, 1, E, generator=g) * 0.3).cuda()
    mask = torch.zeros(B, S, dtype=torch.uint8)
    for b in range(B):
        mask[b, S - b % max(S, 1):] = 1 if b % 2 else 0
    proper = (torch.rand(B, S, generator=g) > 0.3).to(torch.int8)
    proper[mask.bool()] = -1
    ctx = torch.randint(3, 40, (B, S), generator=g)
    if S > 3:
        ctx[:, 1] = ctx[:, 0]                                      # duplicated ids
    ctx[mask.bool()] = 1
    return q, k, bk, mask.cuda(), proper.cuda(), ctx.cuda()


@pytest.mark.parametrize('B,T,S', [(3, 5, 24), (2, 1, 7), (2, 9, 512), (1, 3, 0)])
def test_copy_attention_forward_backward(B, T, S):
    q, k, bk, mask, proper, _ = _inputs(B, T, S)
    if B > 1:
        proper[1] = 0                                              # an all-zero proper row
    qa, ka = q.clone().requires_grad_(), k.clone().requires_grad_()
    bkp = torch.nn.Parameter(bk.clone())
    w = ops.copy_attention(qa, ka, bkp, mask, proper, H)
    qr, kr, bkr = q.clone().requires_grad_(), k.clone().requires_grad_(), bk.clone().requires_grad_()
    wr = ref_copy_attn(qr, kr, bkr, mask, proper)
    torch.testing.assert_close(w, wr, rtol=1e-4, atol=1e-6)
    dw = torch.randn_like(w)
    w.backward(dw)
    wr.backward(dw)
    torch.testing.assert_close(qa.grad, qr.grad, rtol=1e-3, atol=1e-5)
    if S > 0:
        torch.testing.assert_close(ka.grad, kr.grad, rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(bkp.grad, bkr.grad, rtol=1e-3, atol=1e-5)


def test_copy_attention_dropout_is_replayable_and_unbiased():
    q, k, bk, mask, _, _ = _inputs(2, 6, 64, seed=1)
    w1 = ops.CopyAttnFn.apply(q, k, bk, mask, None, H, 0.1, 77)
    w2 = ops.CopyAttnFn.apply(q, k, bk, mask, None, H, 0.1, 77)
    w0 = ops.CopyAttnFn.apply(q, k, bk, mask, None, H, 0.0, 0)
    assert torch.equal(w1, w2)
    assert not torch.equal(w1, w0)
    means = torch.stack([ops.CopyAttnFn.apply(q, k, bk, mask, None, H, 0.1, s) for s in range(1, 65)]).mean(0)
    assert (means - w0).abs().mean() < 0.05 * w0.abs().mean()


@pytest.mark.parametrize('variant', [1, 2])
def test_copy_loss_forward_backward(variant):
    B, T, S = 4, 10, 24
    g = torch.Generator().manual_seed(3)
    w = torch.rand(B, T, S, generator=g)
    w[:, :, 5] = 0.                                                  # zero weights: p = 0 ids
    w = (w / w.sum(-1, keepdim=True)).cuda()
    ctx = torch.randint(3, 30, (B, S), generator=g)
    ctx[:, 7] = ctx[:, 3]                                            # duplicates
    ctx[:, 5] = 29                                                   # an id that only ever has weight 0
    tgt = torch.randint(3, 30, (B, T), generator=g)
    tgt[0, 2] = 29                                                   # a target with p = 0
    tgt[1, 4] = 55                                                   # a target absent from the context
    cm = torch.zeros(B, T, dtype=torch.long)
    cm[0, 1:4] = 1
    cm[0, 6] = 2
    cm[1, 4] = 1
    cm[2, 0:2] = 2
    cm[2, 5] = 3
    cm[:, -1] = -1                                                   # padding
    ctx, tgt, cm = ctx.cuda(), tgt.cuda(), cm.cuda()                 # (row 3 has no entity)
    wa = w.clone().requires_grad_()
    loss = ops.copy_loss(wa, ctx, tgt, cm, variant, 600)
    wr = w.clone().requires_grad_()
    ref = ref_copy_loss(wr, ctx, tgt, cm, variant)
    torch.testing.assert_close(loss, ref, rtol=1e-4, atol=1e-5)
    loss.backward()
    ref.backward()
    torch.testing.assert_close(wa.grad, wr.grad, rtol=1e-3, atol=1e-5)


def test_copy_loss_missing_index_is_nan_and_no_entity_is_zero():
    w = torch.full((1, 3, 4), 0.25, device='cuda')
    ctx = torch.tensor([[3, 4, 5, 6]], device='cuda')
    tgt = torch.tensor([[3, 4, 5]], device='cuda')
    assert math.isnan(float(ops.copy_loss(w, ctx, tgt, torch.tensor([[1, 3, 0]], device='cuda'), 1, 10)))
    assert float(ops.copy_loss(w, ctx, tgt, torch.tensor([[0, 0, -1]], device='cuda'), 1, 10)) == 0.0


def test_entity_head_matches_linear_and_cross_entropy():
    from tell_amd.modules.linear import GehringLinear
    T, B = 7, 3
    fc = GehringLinear(E, 2).cuda()
    x = torch.randn(T, B, E, device='cuda').requires_grad_()
    cm = torch.tensor([[0, 1, 2, 0, -1, 0, 3], [0, 0, 0, 0, 0, 0, -1], [1, 1, 0, 0, 0, 0, 0]], device='cuda')
    loss, logits = ops.entity_head(x, fc.weight_g, fc.weight_v, fc.bias, cm)
    xr = x.detach().clone().requires_grad_()
    g, v, b = (t.detach().clone().requires_grad_() for t in (fc.weight_g, fc.weight_v, fc.bias))
    lr = xr.transpose(0, 1) @ (g * v / v.norm(dim=1, keepdim=True)).t() + b
    tr = cm.clone()
    tr[tr > 1] = 1
    ref = torch.nn.functional.cross_entropy(lr.reshape(-1, 2), tr.reshape(-1), ignore_index=-1)
    torch.testing.assert_close(logits, lr.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-6)
    loss.backward()
    ref.backward()
    torch.testing.assert_close(x.grad, xr.grad, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(fc.bias.grad, b.grad, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(fc.weight_v.grad, v.grad, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(fc.weight_g.grad, g.grad, rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize('T,B', [(1, 2), (12, 3), (512, 1)])
def test_causal_attention_and_step(T, B):
    g = torch.Generator().manual_seed(T)
    q, k, v = ((torch.randn(T, B, E, generator=g) * 0.5).cuda() for _ in range(3))
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
    out = ops.causal_attention(qa, ka, va, H, D ** -0.5)
    qr, kr, vr = (t.clone().requires_grad_() for t in (q, k, v))
    ref = ref_causal(qr, kr, vr, D ** -0.5)
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-5)
    assert out[0].abs().max() == 0                                 # row 0 sees only the zero slot
    dout = torch.randn_like(out)
    out.backward(dout)
    ref.backward(dout)
    for a, r in ((qa, qr), (ka, kr), (va, vr)):
        torch.testing.assert_close(a.grad, r.grad, rtol=1e-3, atol=1e-5)
    step = ops.causal_attention_step(q[-1:], k, v, H, D ** -0.5)
    torch.testing.assert_close(step[0], out[-1].detach(), rtol=1e-5, atol=1e-6)


def test_copy_step_decision():
    B, S = 4, 20
    q, k, bk, mask, proper, ctx = _inputs(B, 1, S, seed=9)
    proper[2] = 0                                                   # nothing to copy: p < 1e-6
    rows = torch.tensor([0, 2, 3], dtype=torch.int32, device='cuda')
    qa = q[0, rows.long()].contiguous()
    ent = torch.tensor([[0., 1.], [0., 1.], [1., 1.]], device='cuda')   # row 3: a tie -> no copy
    gen = torch.tensor([11, 12, 13], device='cuda')
    hist = torch.full((B, 4), -1, dtype=torch.long, device='cuda')
    w = ref_copy_attn(q[:, rows.long()], k[:, rows.long()], bk, mask[rows.long()], proper[rows.long()])[:, 0]
    best = []
    for i, b in enumerate(rows.tolist()):
        sums = {}
        for s in range(S):
            sums[int(ctx[b, s])] = sums.get(int(ctx[b, s]), 0.) + float(w[i, s])
        top = max(sums.values())
        best.append((min(t for t, p in sums.items() if p == top), top))
    hist[0, 0] = -1
    tok, copied, prob = ops.copy_step(qa, k, bk, mask, proper, ctx, rows, ent, gen, hist, 1, H)
    assert tok.tolist() == [best[0][0], 12, 13]
    assert copied.tolist() == [True, False, False]
    assert abs(float(prob[0]) - best[0][1]) < 1e-5 and float(prob[1]) == pytest.approx(1e-6)
    assert hist[:, 1].tolist() == [best[0][0], -1, -1, -1]
    tok, copied, _ = ops.copy_step(qa, k, bk, mask, proper, ctx, rows, ent, gen, hist, 2, H)   # already copied
    assert tok.tolist() == [11, 12, 13] and not copied.any()


class _Roberta(torch.nn.Module):
    def __init__(self, L=3):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.register_buffer('tab', torch.randn(L, 64, 1024, generator=g) * 0.5)

    def extract_features(self, ids, return_all_hiddens=False):
        out = self.tab[:, ids % 64].to(tell_amd.compute_dtype())
        return out if return_all_hiddens else out[-1]


class _Resnet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(4)
        self.register_buffer('proj', torch.randn(2048, 3, generator=g) * 0.3)

    def forward(self, image):
        f = torch.relu(torch.einsum('oc,bchw->bohw', self.proj, torch.nn.functional.avg_pool2d(image, 32)))
        return f.permute(0, 2, 3, 1).reshape(f.shape[0], 49, 2048).to(tell_amd.compute_dtype()).contiguous()


def _pointer_batch(B=3, S=24, T=9, entities=True):
    from tell_amd.data import synthetic_batch
    batch = synthetic_batch(B=B, article_len=S, caption_len=T, faces_objects=True, vocab=600, cutoffs=(100, 300))
    g = torch.Generator().manual_seed(11)
    cap = batch['caption']['roberta']
    ctx = batch['context']['roberta']
    cm = torch.zeros_like(cap)
    if entities:
        cm[0, 2:4] = 1
        cm[0, 5] = 2
        cm[1, 3] = 1
        cap[1, 3] = 599                                               # a target absent from the context
        cap[0, 2:4] = ctx[0, 4:6]
    batch['caption']['roberta_copy_masks'] = cm
    batch['context']['roberta_proper_masks'] = (torch.rand(ctx.shape, generator=g) > 0.3).long()
    batch['face_embeds'] = torch.randn(B, 2, 512, generator=g)
    batch.pop('obj_embeds', None)
    return {k: ({kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else
                (v.cuda() if torch.is_tensor(v) else v)) for k, v in batch.items()}


def _model(kind='pointer'):
    from tell_amd.build import build_model
    torch.manual_seed(0)
    return build_model(kind, _Resnet(), _Roberta(), n_bert_layers=3, vocab_size=600, dim=1024, heads=16, ffn=256,
                       kernels=(3,), cutoff=(100, 300)).cuda()


def _ref_head(P, X, ctx_ids, targets, cm, proper, x_article2, mask, variant):
    """pointer_loss in fp32 torch from the parameter dict P (no dropout)."""
    a = 'entity_attn.'

    def wn(name, x):
        g, v, b = P[name + '.weight_g'], P[name + '.weight_v'], P[name + '.bias']
        return x @ (g * v / v.norm(dim=1, keepdim=True)).t() + b
    Xt = X.transpose(0, 1)
    att = ref_causal(wn(a + 'in_proj_q', Xt), wn(a + 'in_proj_k', Xt), wn(a + 'in_proj_v', Xt), D ** -0.5)
    xe = torch.nn.functional.layer_norm(wn(a + 'attention.attention_module.out_proj', att) + Xt, (E,),
                                        P[a + 'ln.weight'], P[a + 'ln.bias'])
    lg = wn('entity_fc', xe.transpose(0, 1)).reshape(-1, 2)
    tr = cm.clone()
    tr[tr > 1] = 1
    ent = torch.nn.functional.cross_entropy(lg, tr.reshape(-1), ignore_index=-1)
    W, bb = P['in_proj_weight'], P['in_proj_bias']
    q = (Xt @ W[:E].t() + bb[:E]) * D ** -0.5
    k = (x_article2 @ W[E:].t() + bb[E:]).transpose(0, 1)
    w = ref_copy_attn(q, k, P['bias_k'], mask, proper)
    return ent / math.log(2), ref_copy_loss(w, ctx_ids, targets, cm, variant) / math.log(2)


@pytest.mark.parametrize('kind,variant', [('pointer', 1), ('pointer_2', 2)])
def test_pointer_model_loss_and_gradients_match_restatement(kind, variant):
    model = _model(kind).eval()
    batch = _pointer_batch()
    cap = batch['caption']['roberta']
    cm = batch['caption']['roberta_copy_masks'][:, 1:]
    targets = cap[:, 1:]
    enc = model.encode(batch['context'], batch['image'])
    X = {}
    orig = model.pointer_loss

    def spy(Xd, context, copy_masks, tg, enc_):
        X['x'] = Xd.detach().float().clone()
        return orig(Xd, context, copy_masks, tg, enc_)
    model.pointer_loss = spy
    out = model(**{k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()}, encoded=enc)
    out['loss'].backward()
    got = {n: p.grad.clone() for n, p in model.named_parameters()
           if p.grad is not None and (n.startswith(('entity', 'in_proj', 'bias_k', 'bert_weight_2')))}
    for p in model.parameters():
        p.grad = None
    params = {n: p.detach().float().clone().requires_grad_() for n, p in model.named_parameters()}
    stack = enc.stack.float()
    sm = torch.softmax(params['bert_weight_2'], 0)
    x_article2 = (stack * sm[:, None, None, None]).sum(0)
    ent, cp = _ref_head(params, X['x'], batch['context']['roberta'], targets, cm,
                        batch['context']['roberta_proper_masks'], x_article2, enc.article_mask, variant)
    torch.testing.assert_close(out['loss'].detach(), (ent + cp).detach(), rtol=1e-4, atol=1e-5)
    metrics = model.get_metrics()                                  # batch_history over the one batch
    assert metrics['entity_loss'] == pytest.approx(float(ent.detach()), rel=1e-4)
    assert metrics['copy_loss'] == pytest.approx(float(cp.detach()), rel=1e-4)
    (ent + cp).backward()
    for n, g in got.items():
        torch.testing.assert_close(g, params[n].grad, rtol=1e-3, atol=1e-5, msg=n)
    for n in ('entity_attn.attention.attention_module.in_proj_q.0.weight_v', 'out_proj.weight_v',
              'entity_attn.attention.attention_module.in_proj_k.0.4.bias'):
        assert n not in got and dict(model.named_parameters())[n].grad is None


def test_pointer_trainer_step_freezes_and_skips():
    from tell_amd.training import Trainer
    model = _model('pointer')
    no_grad = (r'^resnet', r'^roberta', r'^decoder.embedder', r'^decoder.layers.(0|1|2|3)', r'^decoder.adaptive_softmax',
               r'^bert_weight$')
    trainer = Trainer(model, optimizer_cfg={'warmup': 0.0}, no_grad=no_grad, device='cuda:0')   # lr > 0 at step 1
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    assert trainer.train_one_batch(_pointer_batch(entities=False)) is None
    torch.cuda.synchronize()
    assert all(torch.equal(before[n], p.detach()) for n, p in model.named_parameters())
    loss = trainer.train_one_batch(_pointer_batch())
    torch.cuda.synchronize()
    assert loss is not None and math.isfinite(float(loss))
    after = dict(model.named_parameters())
    for n, p in after.items():
        frozen = (n.startswith(('decoder.', 'bert_weight')) and not n.startswith('bert_weight_2')) \
            or '.attention.attention_module.in_proj_' in n or n.startswith('out_proj.')
        if frozen:
            assert torch.equal(before[n], p.detach()), n
    for n in ('entity_fc.weight_v', 'in_proj_weight', 'bias_k', 'bert_weight_2', 'entity_attn.ln.weight'):
        assert not torch.equal(before[n], after[n].detach()), n


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_pointer_generation_runs_and_records_copies(dtype):
    tell_amd.set_compute_dtype(dtype)
    model = _model('pointer').eval()
    with torch.no_grad():
        model.entity_fc.bias.data = torch.tensor([-5., 5.], device='cuda')      # copy whenever something is copyable
    batch = _pointer_batch(B=4)
    out = model.generate(batch['context'], batch['image'], batch['caption'], batch['face_embeds'])
    ids, sc = out['gen_ids'], out['should_copy']
    assert ids.shape == sc.shape and bool(sc[:, 0].all())
    assert ids.shape[1] >= 2
    copied = ids[:, 1:][sc[:, 1:]]
    assert copied.numel() > 0
    ctx = batch['context']['roberta']
    for b in range(ids.shape[0]):
        row = ids[b, 1:][sc[b, 1:]].tolist()
        assert len(row) == len(set(row))                            # an id is copied at most once per row
        assert set(row) <= set(ctx[b].tolist())
    assert len(out['copied_texts']) == 4
    model.sampling_temp = 2.0                                       # the recorded log-prob is topk_lprob / T (:636-637)
    out2 = model.generate(batch['context'], batch['image'], batch['caption'], batch['face_embeds'])
    assert torch.equal(out2['gen_ids'], ids)
    torch.testing.assert_close(out2['log_probs'], out['log_probs'] / 2.0)
    with pytest.raises(ValueError):
        model.generate(batch['context'], batch['image'], batch['caption'], batch['face_embeds'], beam_size=2)


def _no_dropout(model):
    for m in model.modules():
        for a in ('dropout', 'input_dropout', 'relu_dropout', 'weight_dropout'):
            if isinstance(getattr(m, a, None), float):
                setattr(m, a, 0.0)
    model.copy_dropout = 0.0


@pytest.mark.parametrize('kind', ['pointer', 'pointer_2'])
def test_trainer_step_loss_equals_the_eager_loss(kind):
    """The trainer's default path (graphs on, shape buckets (128, 16)) computes the model's own loss on the batch: the
    article of 24 tokens is NOT padded to 128 for these models, whose variant-2 loss counts every context id."""
    from tell_amd.training import Trainer
    model = _model(kind)
    _no_dropout(model)
    batch = _pointer_batch()
    model.eval()
    want = model(**{k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()})['loss']
    trainer = Trainer(model, no_grad=(r'^resnet', r'^roberta'), device='cuda:0')
    assert trainer._bucketed(batch) is batch
    got = trainer.train_one_batch(batch)
    torch.cuda.synchronize()
    torch.testing.assert_close(got, want.detach(), rtol=1e-5, atol=1e-6)


def test_shape_buckets_pad_the_proper_masks_with_minus_one():
    from types import SimpleNamespace
    from tell_amd.training.trainer import Trainer
    batch = _pointer_batch()
    fake = SimpleNamespace(shape_buckets=(128, 16), nan_check=False, model=SimpleNamespace(index='roberta', padding_idx=1))
    out = Trainer._bucketed(fake, batch)
    ctx = out['context']
    assert ctx['roberta'].shape[1] == 128 and ctx['roberta_proper_masks'].shape == ctx['roberta'].shape
    assert torch.equal(ctx['roberta_proper_masks'][:, :24], batch['context']['roberta_proper_masks'])
    assert bool((ctx['roberta_proper_masks'][:, 24:] == -1).all())


def test_copy_ops_refuse_masks_of_another_width():
    q, k, bk, mask, proper, ctx = _inputs(2, 3, 24)
    with pytest.raises(ValueError, match='proper'):
        ops.copy_attention(q, k, bk, mask, proper[:, :20], H)
    with pytest.raises(ValueError, match='mask'):
        ops.copy_attention(q, k, bk, mask[:, :20], proper, H)
    w = torch.full((2, 3, 24), 1.0 / 24, device='cuda')
    cm = torch.ones(2, 3, dtype=torch.long, device='cuda')
    with pytest.raises(ValueError, match='ctx_ids'):
        ops.copy_loss(w, ctx[:, :20], ctx[:, :3], cm, 1, 600)
    with pytest.raises(ValueError, match='copy_mask'):
        ops.copy_loss(w, ctx, ctx[:, :3], cm[:, :2], 1, 600)


def test_copy_loss_variant_2_with_an_id_beyond_the_vocabulary_is_nan():
    w = torch.full((1, 3, 4), 0.25, device='cuda')
    ctx = torch.tensor([[3, 4, 5, 6]], device='cuda')
    cm = torch.tensor([[1, 0, 0]], device='cuda')
    assert math.isfinite(float(ops.copy_loss(w, ctx, torch.tensor([[3, 4, 5]], device='cuda'), cm, 2, 10)))
    assert math.isnan(float(ops.copy_loss(w, ctx, torch.tensor([[3, 4, 10]], device='cuda'), cm, 2, 10)))
    assert math.isfinite(float(ops.copy_loss(w, ctx, torch.tensor([[3, 4, 10]], device='cuda'), cm, 1, 10)))
