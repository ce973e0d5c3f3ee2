"""Self-critical sequence training on the MI355X: tell_caption_reward bit for bit against the
definition of tests/scst_ref.py; tell_ce_fwd_weighted / tell_ce_bwd_weighted bit for bit against tell_ce_fwd / tell_ce_bwd run
with the product as gscale; ops.adaptive_loss(row_weight=); forward(caption_weights=, per_image=) against the plain step, the
repeated batch and the CPU oracle; Trainer.train_self_critical end to end, and the plain captured step around it.
Run on the MI355X box:  python -m pytest tests/test_gpu_scst.py -m gpu -s"""
import math

import numpy as np
import pytest
import torch

import adaptive_ref as ref
import scst_ref
from guarded import Guard
from scst_ref import EOS, PAD
from test_gpu_small_reduce import I32, TD, In, host, intact, out_guard
from test_gpu_train import DEV, KW, _no_dropout, _Res, _Rob

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu(monkeypatch):
    import tell_amd
    tell_amd.hip.require_gpu()
    monkeypatch.setenv('TELL_STEP_GRAPH_STRICT', '1')       # a failed capture fails the test instead of going eager
    yield
    tell_amd.set_compute_dtype(torch.float32)
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                  # a device fault: every later launch of this process would fail the same way
        pytest.exit('GPU error, nothing more is launched: %s' % err, 3)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# =========================================================================== 1. tell_caption_reward
def _reward_call(ids, refs, base, B, n, steps, ref_steps, K, out, ld_ids=None, ld_ref=None):
    from tell_amd import hip
    hip.call('tell_caption_reward', ids.t, ids.t.stride(0) if ld_ids is None else ld_ids, refs.t,
             refs.t.stride(0) if ld_ref is None else ld_ref, None if base is None else base.t, B, n, steps, ref_steps, PAD, EOS, K,
             out['reward'].t, out['adv'].t, None if out.get('counts') is None else out['counts'].t)


def _reward_outs(B, n, counts=True):
    o = dict(reward=out_guard((B, n), 'float32'), adv=out_guard((B, n), 'float32'))
    if counts:
        o['counts'] = Guard((B * n, 3), I32)
    return o


@pytest.mark.parametrize('steps', scst_ref.CASE_STEPS)
@pytest.mark.parametrize('n', scst_ref.CASE_N)
def test_reward_kernel_is_the_definition_bit_for_bit(n, steps):
    """reward, adv and counts of B = 3 images, both baseline modes, K in {1, 4}; ids and ref are strided views inside
    guarded buffers (ld_ids > steps + 1), the outputs guarded too; counts may be NULL"""
    B = scst_ref.CASE_B
    ids_np, ref_np, ref_steps = scst_ref.case(n, steps)
    ids = In(ids_np, 'int64', (ids_np.shape[1] + 5, 1))                  # rows further apart than they are long
    refs = In(ref_np, 'int64')
    base_np = np.array([0.3, 1.0, 0.0], dtype=np.float32)
    base = In(base_np, 'float32')
    for K in (1, 4):
        for b_np, b_dev in ((None, None), (base_np, base)):
            want_r, want_a, want_c = scst_ref.reward(ids_np, ref_np, n, steps, ref_steps, K, b_np)
            out = _reward_outs(B, n)
            _reward_call(ids, refs, b_dev, B, n, steps, ref_steps, K, out)
            intact(ids, refs, base, *out.values())
            tag = (n, steps, K, b_np is not None)
            assert np.array_equal(out['counts'].t.cpu().numpy(), want_c), tag
            assert np.array_equal(_bits(host(out['reward'])), _bits(want_r)), tag
            assert np.array_equal(_bits(host(out['adv'])), _bits(want_a)), tag
    out = _reward_outs(B, n, counts=False)                               # counts == NULL
    _reward_call(ids, refs, None, B, n, steps, ref_steps, 4, out)
    intact(ids, refs, *out.values())
    want_r, want_a, _ = scst_ref.reward(ids_np, ref_np, n, steps, ref_steps, 4)
    assert np.array_equal(_bits(host(out['reward'])), _bits(want_r)) and np.array_equal(_bits(host(out['adv'])), _bits(want_a))


def test_reward_wrapper_and_declined_calls():
    """ops.caption_reward is the launch; what lies outside the limits is declined by the library and nothing is written"""
    from tell_amd import ops
    n, steps, B = 5, 7, scst_ref.CASE_B
    ids_np, ref_np, ref_steps = scst_ref.case(n, steps)
    ids_t, ref_t = torch.from_numpy(ids_np).to(DEV), torch.from_numpy(ref_np).to(DEV)
    r, a, c = ops.caption_reward(ids_t, ref_t, B, n, steps, ref_steps, PAD, EOS, 4, want_counts=True)
    want_r, want_a, want_c = scst_ref.reward(ids_np, ref_np, n, steps, ref_steps, 4)
    assert np.array_equal(_bits(r.cpu().numpy()), _bits(want_r)) and np.array_equal(_bits(a.cpu().numpy()), _bits(want_a))
    assert np.array_equal(c.cpu().numpy(), want_c) and ops.caption_reward(ids_t, ref_t, B, n, steps, ref_steps, PAD, EOS)[2] is None
    g = ops.caption_reward(ids_t[::n].contiguous(), ref_t, B, 1, steps, ref_steps, PAD, EOS, 2)      # the greedy call: n = 1
    r2, a2, _ = ops.caption_reward(ids_t, ref_t, B, n, steps, ref_steps, PAD, EOS, 2, baseline=g[0].reshape(B))
    w2 = scst_ref.reward(ids_np, ref_np, n, steps, ref_steps, 2, scst_ref.reward(ids_np[::n], ref_np, 1, steps, ref_steps, 2)[0])
    assert np.array_equal(_bits(r2.cpu().numpy()), _bits(w2[0])) and np.array_equal(_bits(a2.cpu().numpy()), _bits(w2[1]))
    assert (a2[:, 0] == 0).all()                                         # a hypothesis against itself as the baseline
    ids, refs = In(ids_np, 'int64'), In(ref_np, 'int64')
    out = _reward_outs(B, 16)
    ld = ids_np.shape[1]
    for kw in (dict(n=0), dict(n=17), dict(steps=0), dict(steps=257), dict(ref_steps=0), dict(ref_steps=257), dict(K=0),
               dict(K=5), dict(ld_ids=steps), dict(ld_ref=ref_steps), dict(B=0)):
        a_ = dict(B=B, n=n, steps=steps, ref_steps=ref_steps, K=4)
        a_.update(kw)
        with pytest.raises(RuntimeError, match='tell_caption_reward'):
            _reward_call(ids, refs, None, a_['B'], a_['n'], a_['steps'], a_['ref_steps'], a_['K'], out,
                         ld_ids=a_.get('ld_ids', ld), ld_ref=a_.get('ld_ref'))
    intact(ids, refs, *out.values())
    assert all(o.untouched() for o in out.values())


# =========================================================================== 2. weighted cross entropy
# the smallest cases of adaptive_ref.CE that cover, between them: a second trip over V, row_idx, m_dev < M, an ignored row
CE_CASES = [c for c in ref.CE if (c['V'], c['M']) in ((256, 70), (257, 3))]
WEIGHTS = (0.0, 1.0, 0.3)                                                # zero, one, a value that is no power of two


def test_the_weighted_ce_cases_cover_their_paths():
    paths = set().union(*[ref.ce_paths(c) for c in CE_CASES])
    assert {'ce:trips:two_ragged', 'ce:row_idx:perm', 'ce:m_dev:inside'} <= paths, paths
    assert any(p.startswith('ce:ignored_target:') for p in paths), paths


@pytest.mark.parametrize('dty', ('bfloat16', 'float32'))
@pytest.mark.parametrize('w_perm', (False, True), ids=('w_idx_null', 'w_idx_perm'))
@pytest.mark.parametrize('case', CE_CASES, ids=[c['id'] for c in CE_CASES])
def test_weighted_cross_entropy_is_the_plain_one_with_the_product(case, w_perm, dty):
    """forward: lse bit for bit, loss = one fp32 multiply; backward: every row bit for bit the row tell_ce_bwd writes with
    gscale = fp32(gscale * weight); rows at or past *m_dev keep the sentinel; weight 0 rows are zero; weight 1 everywhere is
    the unweighted call"""
    from tell_amd import hip
    x, M, V, ld = ref.ce_inputs(case), case['M'], case['V'], case['ld']
    ld_d = (V + 7) // 8 * 8
    Me = M if case['m'] is None else min(case['m'], M)
    logits, tg = In(x['logits'], 'float32', (ld, 1)), In(x['targets'], 'int32')
    perm = None if x['row_idx'] is None else In(x['row_idx'], 'int32')
    m = None if case['m'] is None else In(np.array([case['m']]), 'int32')
    rng = np.random.RandomState(V + M)
    w_np = np.array([WEIGHTS[j % 3] for j in range(M)], dtype=np.float32)
    widx_np = rng.permutation(M).astype(np.int32) if w_perm else None
    w, widx = In(w_np, 'float32'), (None if widx_np is None else In(widx_np, 'int32'))
    w_row = w_np if widx_np is None else w_np[widx_np]                   # the weight of compacted row i
    assert set(w_row[:Me].tolist()) == set(np.float32(WEIGHTS).tolist()) or Me < 3
    opt = lambda a: None if a is None else a.t                           # noqa: E731
    code = hip.dt(TD[dty])

    def fwd(weights):
        lse, loss = out_guard((M,), 'float32'), out_guard((M,), 'float32')
        if weights is None:
            hip.call('tell_ce_fwd', logits.t, ld, M, V, tg.t, opt(perm), opt(m), ref.CE_IGNORE, lse.t, loss.t)
        else:
            hip.call('tell_ce_fwd_weighted', logits.t, ld, M, V, tg.t, opt(perm), opt(m), ref.CE_IGNORE, weights.t, opt(widx),
                     lse.t, loss.t)
        intact(logits, tg, perm, m, w, widx, lse, loss)
        return lse, loss

    def bwd(lse, g, weights):
        dl = out_guard((M, V), dty, strides=(ld_d, 1))
        gs = In(np.array([g], np.float32), 'float32')
        if weights is None:
            hip.call('tell_ce_bwd', logits.t, ld, M, V, tg.t, opt(perm), opt(m), ref.CE_IGNORE, lse.t, gs.t, dl.t, ld_d, code)
        else:
            hip.call('tell_ce_bwd_weighted', logits.t, ld, M, V, tg.t, opt(perm), opt(m), ref.CE_IGNORE, weights.t, opt(widx),
                     lse.t, gs.t, dl.t, ld_d, code)
        intact(logits, tg, perm, m, w, widx, gs, lse, dl)
        return host(dl)
    lse0, loss0 = fwd(None)
    lse1, loss1 = fwd(w)
    assert ref.same_bits(host(lse1), host(lse0))
    assert ref.same_bits(host(loss1), (w_row * host(loss0)).astype(np.float32))
    assert (host(loss1)[w_row == 0] == 0).all() and (host(loss1)[Me:] == 0).all() and (host(lse1)[Me:] == 0).all()
    ones = In(np.ones(M, np.float32), 'float32')
    lse_1, loss_1 = fwd(ones)
    assert ref.same_bits(host(lse_1), host(lse0)) and ref.same_bits(host(loss_1), host(loss0))
    tgt = ref.ce_targets(x['targets'], x['row_idx'], M)
    for g in (1.0, ref.CE_G['1/37']):
        got = bwd(lse0, g, w)
        assert (got[Me:] == ref.SENTINEL).all()                          # rows past the count are left alone
        for v in WEIGHTS:
            prod = float(np.float32(g) * np.float32(v))                  # the fp32 product, formed once
            plain = bwd(lse0, prod, None)
            rows = np.nonzero(w_row[:Me] == np.float32(v))[0]
            assert ref.same_bits(got[rows], plain[rows]), (g, v)
        assert (got[:Me][w_row[:Me] == 0] == 0).all() and (got[:Me][tgt[:Me] == ref.CE_IGNORE] == 0).all()
        assert ref.same_bits(bwd(lse0, g, ones), bwd(lse0, g, None))     # weight 1 everywhere: the unweighted call


def test_weighted_ce_needs_its_weights():
    from tell_amd import hip
    z = torch.zeros(4, 8, device=DEV)
    zi = torch.zeros(4, dtype=torch.int32, device=DEV)
    out = torch.zeros(4, device=DEV)
    with pytest.raises(RuntimeError, match='tell_ce_fwd_weighted'):
        hip.call('tell_ce_fwd_weighted', z, 8, 4, 8, zi, None, None, 1, None, None, out, out)
    with pytest.raises(RuntimeError, match='tell_ce_bwd_weighted'):
        hip.call('tell_ce_bwd_weighted', z, 8, 4, 8, zi, None, None, 1, None, None, out, out, z, 8, 0)


# =========================================================================== 3. ops.adaptive_loss(row_weight=)
def _asm(golden):
    import tell_amd
    from tell_amd.build import build_embedder
    from tell_amd.modules import AdaptiveLoss, AdaptiveSoftmax
    tell_amd.set_compute_dtype(torch.float32)
    fx = golden('adaptive_softmax')
    emb = build_embedder(600, 32, (100, 300))
    asm = AdaptiveSoftmax(600, 32, [100, 300], adaptive_inputs=emb.token_embedder_adaptive)
    asm.load_state_dict(fx['sd'], strict=False)
    asm.to(DEV)
    return asm, AdaptiveLoss(1), fx['in']['x'].to(DEV), fx['in']['target'].to(DEV)


def _loss_and_grads(asm, crit, x, target, row_weight=None, upstream=None):
    for p in asm.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    loss, n = crit(asm, (xg, None), target) if row_weight is None else crit(asm, (xg, None), target, row_weight=row_weight)
    saved = loss.grad_fn.saved
    loss.backward(upstream)
    torch.cuda.synchronize()
    grads = {'x': xg.grad.clone()}
    grads.update({k: p.grad.clone() for k, p in asm.named_parameters() if p.grad is not None})
    return loss.detach().clone(), int(n), grads, saved


def test_adaptive_loss_with_unit_weights_is_the_unweighted_call(golden):
    """weights all 1: the loss and every gradient bit for bit; a constant weight c that is no power of two: bit for bit the
    unweighted call differentiated with the upstream gradient c (the same fp32 product gscale * weight in every row)"""
    asm, crit, x, target = _asm(golden)
    l0, n0, g0, _ = _loss_and_grads(asm, crit, x, target)
    l1, n1, g1, _ = _loss_and_grads(asm, crit, x, target, torch.ones(target.shape, device=DEV))
    assert n1 == n0 and torch.equal(l1, l0) and set(g1) == set(g0) and len(g0) >= 6
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    c = 0.3
    _, _, gc, _ = _loss_and_grads(asm, crit, x, target, torch.full(target.shape, c, device=DEV))
    _, _, gu, _ = _loss_and_grads(asm, crit, x, target, upstream=torch.full((1,), c, device=DEV))
    for k in g0:
        assert torch.equal(gc[k], gu[k]), k


def _float64_loss(asm, x, target, w, pad=1):
    """sum_r w_r * -log p(y_r) of the adaptive softmax in float64 torch, with the quirk of the kernels: a tail target whose
    band-local id equals the ignored index is charged in the head only"""
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in asm.named_parameters()}
    xd = x.detach().double().cpu().requires_grad_(True)
    emb0, cls = p['head.word_proj.weight'], p['head.class_proj.weight']
    cut = asm.cutoff
    X, tg, wf = xd.reshape(-1, xd.shape[-1]), target.reshape(-1).cpu(), w.double().cpu().reshape(-1)
    head = torch.log_softmax(X @ torch.cat([emb0, cls]).t(), dim=-1)
    total = torch.zeros((), dtype=torch.float64)
    for r in range(X.shape[0]):
        t = int(tg[r])
        if t == pad:
            continue
        band = next(i for i, c in enumerate(cut) if t < c)
        if band == 0:
            total = total - wf[r] * head[r, t]
            continue
        total = total - wf[r] * head[r, cut[0] + band - 1]
        local = t - cut[band - 1]
        if local != pad:
            proj, emb = p['tail.%d.0.weight' % (band - 1)], p['tail.%d.2.weight' % (band - 1)]
            total = total - wf[r] * torch.log_softmax(emb @ (proj @ X[r]), dim=-1)[local]
    total.backward()
    grads = {'x': xd.grad.float()}
    grads.update({k: v.grad.float() for k, v in p.items() if v.grad is not None})
    return float(total.detach()), grads


def _loss_bound(saved, w, pad=1):
    """the float64 value of the weighted sum FROM THE LOGITS THE OP ITSELF COMPUTED, and how far the op's total may be from
    it by the bounds tests/adaptive_ref.py derives for the unweighted kernels: per row |w| times the ce_loss bound (u |ref| +
    c gamma 2^-24 S) plus one rounding of the product, per tell_sum_f32 launch its k 2^-24 S"""
    x2, w_head, head_logits, lse_h, part, tails = saved
    N = head_logits.shape[0]
    wf = w.double().cpu().numpy().reshape(-1)
    calls = [(head_logits, part['head_target'], None, None)]
    for i, (xg, h, logits, lse_t) in enumerate(tails):
        calls.append((logits, part['local'][i + 1], int(part['count'][i + 1]), part['rows'][i + 1]))
    total, bound, u = 0.0, 0.0, ref.U_OUT['float32']
    for logits, tg, m, rows in calls:
        Me = N if m is None else m
        lg = logits.float().cpu().numpy().copy()
        tgn = tg.cpu().numpy()[:N].copy()
        lg[Me:], tgn[Me:] = 0.0, 0                                       # (never written, never read)
        o = ref.ce_fwd(lg, tgn, None, m, pad)['loss']
        wr = np.zeros(N)
        wr[:Me] = wf[:Me] if rows is None else wf[rows.cpu().numpy()[:Me]]
        v, S = np.asarray(o.value, np.float64), np.broadcast_to(np.asarray(o.S, np.float64), (N,))
        prod = wr * v
        row_b = np.abs(wr) * (u * np.abs(v) + ref.C['ce_loss'] * o.gam * ref.EPS * S + ref.TINY * (1.0 + S)) + u * np.abs(prod)
        s = ref.sum_f32(prod.astype(np.float32), N, m, np.float32(total), 1)['out']
        bound += float(row_b[:Me].sum()) + s.k * ref.EPS * float(np.asarray(s.S).sum()) + u * abs(total)
        total += float(prod[:Me].sum())
    return total, bound


def test_adaptive_loss_with_general_weights_against_float64(golden):
    """signed weights between -2 and 2, some zero.  The loss: against the float64 restatement from the op's own logits, inside
    the bound adaptive_ref derives for tell_ce_fwd and tell_sum_f32, every row's share times |w| (_loss_bound; max |w| = 2
    enters through the rows).  The gradients: against float64 autograd of the same sum from the inputs, inside the tolerances
    tests/test_gpu_ops.py::test_adaptive_softmax_golden holds the unweighted gradients to, times max |w|.  n_valid stays
    the count of non-pad targets."""
    from test_gpu_ops import close
    asm, crit, x, target = _asm(golden)
    g = torch.Generator().manual_seed(11)
    w = (torch.rand(target.shape, generator=g) * 4 - 2)
    w[torch.rand(target.shape, generator=g) < 0.2] = 0.0
    w.view(-1)[0] = 2.0
    w = w.to(DEV)
    wmax = float(w.abs().max())
    _, n0, _, _ = _loss_and_grads(asm, crit, x, target)
    loss, n, grads, saved = _loss_and_grads(asm, crit, x, target, w)
    assert n == n0 == int((target != 1).sum())
    want, bound = _loss_bound(saved, w)
    print('\nweighted loss %.9g, float64 from the same logits %.9g, |difference| %.3g, bound %.3g'
          % (float(loss), want, abs(float(loss) - want), bound))
    assert abs(float(loss) - want) <= bound
    want64, g64 = _float64_loss(asm, x, target, w)
    print('float64 from the inputs (its own logits): %.9g' % want64)
    assert set(g64) <= set(grads) and len(g64) >= 6
    close(grads['x'], g64['x'].reshape(grads['x'].shape), torch.float32, scale=wmax)
    for k in g64:
        if k != 'x':
            close(grads[k], g64[k], torch.float32, scale=8 * wmax)


# =========================================================================== 4. model and trainer
def _dev(b):
    return {k: ({kk: vv.to(DEV) for kk, vv in v.items()} if isinstance(v, dict) else v.to(DEV)) for k, v in b.items()}


def _clone(x):
    return {k: (dict(v) if isinstance(v, dict) else v.clone()) for k, v in x.items()}


def _repeat(batch, n):
    return {k: ({kk: vv.repeat_interleave(n, dim=0) for kk, vv in v.items()} if isinstance(v, dict)
                else v.repeat_interleave(n, dim=0)) for k, v in batch.items()}


def _batch(kind, B=3, seed=50, caption_len=9):
    from tell_amd.data import synthetic_batch
    return synthetic_batch(B=B, article_len=20, caption_len=caption_len, faces_objects=(kind == 'faces_objects'), vocab=600,
                           cutoffs=(100, 300), seed=seed, variable=True)


OCFG = dict(lr=5e-3, warmup=0.5, t_total=4, b1=0.9, b2=0.98, e=1e-6, weight_decay=1e-5, max_grad_norm=0.1)


def _fp32_trainer(kind, oracle=False, ocfg=None, **model_kw):
    import tell_amd
    from tell_amd.build import build_model
    from tell_amd.training import Trainer
    tell_amd.set_compute_dtype(torch.float32)
    torch.manual_seed(0)
    adim = 64 if kind == 'flattened' else 1024
    gpu = build_model(kind, _Res(True), _Rob(adim), n_bert_layers=3, article_dim=adim, **KW, **model_kw)
    _no_dropout(gpu)
    cpu = None
    if oracle:
        from oracle.build import build_model as obuild
        cpu = obuild(kind, _Res(False), _Rob(adim), n_bert_layers=3, article_dim=adim, **KW).train()
        cpu.load_state_dict({k: v for k, v in gpu.state_dict().items() if k in cpu.state_dict()}, strict=False)
        _no_dropout(cpu)
    trainer = Trainer(gpu, dict(ocfg or OCFG), device=DEV)
    trainer.defer_update = True                              # a step stops behind backward: flat.grad can be read
    return trainer, cpu


def _grads_of(trainer):
    torch.cuda.synchronize()
    g = trainer.flat.grad.clone()
    trainer.flat.zero_grad()
    return g


def _weighted_step(trainer, batch, **kw):
    """the eager step with the model's forward given the new arguments: _grad_store_begin, forward, the plain step's tail"""
    from tell_amd import hip, ops
    trainer.model.train()
    with hip.bound_stream():
        try:
            trainer._grad_store_begin(batch)
            loss = trainer._finish_step(trainer.model(**_clone(batch), **kw))
        finally:
            ops.grad_store_mode(False)
    return loss.clone(), _grads_of(trainer)


def _plain_step(trainer, batch):
    loss = trainer.train_one_batch(_clone(batch)).clone()
    return loss, _grads_of(trainer)


@pytest.mark.parametrize('kind', ['flattened', 'faces_objects'])
def test_unit_caption_weights_are_the_plain_step(kind):
    """(a) forward(caption_weights=ones, per_image=1): the loss and the gradients of _eager_step, bit for bit - per row and
    per token weights alike"""
    trainer, _ = _fp32_trainer(kind)
    trainer.step_graph = None
    batch = trainer._bucketed(_dev(_batch(kind)))            # (what train_one_batch does to a batch first)
    _plain_step(trainer, batch)                              # (the first pass builds the caches)
    l0, g0 = _plain_step(trainer, batch)
    rows, T = batch['caption']['roberta'].shape[0], batch['caption']['roberta'].shape[1] - 1
    for ones in (torch.ones(rows, device=DEV), torch.ones(rows, T, device=DEV)):
        l1, g1 = _weighted_step(trainer, batch, caption_weights=ones, per_image=1)
        assert torch.equal(l1, l0) and torch.equal(g1, g0) and float(g0.abs().max()) > 0


def _mix_slice(trainer):
    fl = trainer.flat
    idx = [i for i, name in enumerate(fl.names) if name == 'bert_weight']
    assert len(idx) == 1, fl.names[:5]
    return fl.offsets[idx[0]], fl.offsets[idx[0]] + fl.params[idx[0]].numel()


@pytest.mark.parametrize('kind', ['flattened', 'faces_objects'])
def test_per_image_is_the_repeated_batch(kind):
    """(b) per_image = n on B images against the batch repeated n times with the same B * n captions and weights: the loss
    bit for bit, every gradient bit for bit but the layer-mix weights, whose sum over the rows runs in another order (held to
    the tolerance of test_gpu_train.py::test_two_training_steps_match_oracle_fp32: 2e-3 of the largest magnitude)"""
    n, B = 3, 2
    trainer, _ = _fp32_trainer(kind)
    trainer.step_graph = None
    images = _dev(_batch(kind, B=B, seed=51))
    caps = _dev(_batch(kind, B=B * n, seed=52))['caption']
    g = torch.Generator().manual_seed(3)
    w = (torch.rand(B * n, caps['roberta'].shape[1] - 1, generator=g) * 2 - 0.5).to(DEV)
    shared = dict(images, caption=caps)
    repeated = dict(_repeat(images, n), caption=caps)
    l_rep, g_rep = _weighted_step(trainer, repeated, caption_weights=w)
    l_pi, g_pi = _weighted_step(trainer, shared, caption_weights=w, per_image=n)
    assert torch.equal(l_pi, l_rep)
    lo, hi = _mix_slice(trainer)
    keep = torch.ones_like(g_rep, dtype=torch.bool)
    keep[lo:hi] = False
    assert torch.equal(g_pi[keep], g_rep[keep]) and float(g_rep[keep].abs().max()) > 0
    mix_pi, mix_rep = g_pi[lo:hi], g_rep[lo:hi]
    assert float(mix_rep.abs().max()) > 0
    assert float((mix_pi - mix_rep).abs().max()) <= 2e-3 * (float(mix_rep.abs().max()) + 1e-6), (mix_pi, mix_rep)
    with pytest.raises(ValueError, match='per_image'):
        trainer.model(**_clone(shared), per_image=2)
    with pytest.raises(ValueError, match='caption_weights'):
        trainer.model(**_clone(shared), per_image=n, caption_weights=w[:B])


@pytest.mark.parametrize('per_image', [1, 2])
@pytest.mark.parametrize('kind', ['flattened', 'faces_objects'])
def test_weighted_step_matches_the_cpu_oracle(kind, per_image):
    """(c) sum_r w_r NLL_r / n_valid in bits and its gradients by torch autograd on the CPU oracle, within the tolerances of
    test_gpu_train.py::test_two_training_steps_match_oracle_fp32 for the unweighted step: the loss to 1e-3 relative, every
    tensor to 2e-3 of its largest magnitude.  Positive weights per token, so that the loss is no cancelling sum."""
    B = 2
    trainer, cpu = _fp32_trainer(kind, oracle=True)
    trainer.step_graph = None
    images = _batch(kind, B=B, seed=53)
    caps = _batch(kind, B=B * per_image, seed=54)['caption']
    cap = caps['roberta']
    g = torch.Generator().manual_seed(4)
    w = torch.rand(cap.shape[0], cap.shape[1] - 1, generator=g) * 1.3 + 0.2
    loss, grad = _weighted_step(trainer, _dev(dict(images, caption=caps)), caption_weights=w.to(DEV), per_image=per_image)
    rep = _clone(_repeat(images, per_image))
    _, _, ctx = cpu._forward(rep['context'], rep['image'], {'roberta': cap.clone()}, rep.get('face_embeds'), rep.get('obj_embeds'))
    out = cpu.decoder({'roberta': cap[:, :-1]}, ctx)
    lp = cpu.decoder.get_normalized_probs((out[0], None), log_probs=True).float()
    tgt = cap[:, 1:]
    live = tgt != PAD
    nll = -lp.gather(2, tgt.unsqueeze(-1)).squeeze(-1)
    want = (w * nll)[live].sum() / live.sum() / math.log(2)
    want.backward()
    w64, _ = scst_ref.weighted_bits(lp.detach().numpy(), tgt.numpy(), w.numpy())
    assert abs(float(want) - w64) <= 1e-5 * abs(w64)
    print('\n%s per_image=%d: weighted loss %.6f (HIP) vs %.6f (CPU oracle)' % (kind, per_image, float(loss), float(want)))
    assert abs(float(loss) - float(want)) <= 1e-3 * abs(float(want)), (float(loss), float(want))
    fl = trainer.flat
    cp = dict(cpu.named_parameters())
    worst, seen = 0.0, 0
    for name, lo, p in zip(fl.names, fl.offsets, fl.params):
        got = grad[lo:lo + p.numel()].cpu()                  # (tensors start on aligned offsets of the flat buffer)
        if cp[name].grad is None:
            assert float(got.abs().max()) == 0.0, name
            continue
        r = cp[name].grad.reshape(-1)
        d = float((got - r).abs().max()) / (float(r.abs().max()) + 1e-6)
        worst, seen = max(worst, d), seen + 1
    print('largest |gradient - oracle| / max |oracle| over %d tensors: %.3g' % (seen, worst))
    assert seen > 20 and worst < 2e-3, worst


def _small_bf16(**kw):
    import tell_amd
    from tell_amd.build import build_model
    from test_gpu_pointer import _Resnet, _Roberta
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    return build_model('faces_objects', _Resnet(), _Roberta(), n_bert_layers=3, vocab_size=600, dim=1024, heads=16, ffn=256,
                       kernels=(3,), cutoff=(100, 300), **kw).to(DEV).eval()


def _small_batch(B=3, seed=31):
    from tell_amd.data import synthetic_batch
    return synthetic_batch(B, 24, 9, True, vocab=600, cutoffs=(100, 300), seed=seed, device=DEV)


def _check_against_host(out, ref_ids, n, baseline):
    ids = out['gen_ids_samples'].cpu().numpy()
    B, _, L = ids.shape
    base = out['baseline'].cpu().numpy().reshape(B) if baseline == 'greedy' else None
    r, a, _ = scst_ref.reward(ids.reshape(B * n, L), ref_ids.cpu().numpy(), n, L - 1, ref_ids.shape[1] - 1, 4, base)
    assert np.array_equal(_bits(out['reward'].cpu().numpy()), _bits(r))
    assert np.array_equal(_bits(out['adv'].cpu().numpy()), _bits(a))
    return r


def test_train_self_critical_end_to_end():
    """(d) the small bf16 top-k model; the references are the model's own greedy captions, so that samples overlap them.  A
    seed out of five under which at least half the images have two samples with different rewards (a step that only ever sees
    zero advantages shows nothing); reward / adv are the host definition on the returned ids; the loss is finite; the
    parameters move; both baselines; the refusals."""
    from tell_amd.training import Trainer
    n = 4
    # (top-2 at T = 0.5: near enough to the arg-max decode for samples to share n-grams with it; batch seed 33: the random
    #  weights give every image a greedy caption that does not start with the pad id, i.e. a reference that is not empty)
    model = _small_bf16(sampling_topk=2, sampling_temp=0.5)
    trainer = Trainer(model, dict(lr=1e-3, warmup=0.0, t_total=100, max_grad_norm=1.0, weight_decay=0.0), device=DEV)
    b = _small_batch(seed=33)
    B = b['image'].shape[0]
    with torch.no_grad(), trainer._arg_max_decode():
        greedy = model.eval().generate(**_clone(b))['gen_ids']
    assert greedy.shape[1] >= 2 and greedy.shape[1] <= 257
    b['caption'] = {'roberta': greedy.clone()}
    # ---- the greedy baseline first, without an update: the greedy caption inside the step is then the reference itself
    trainer.defer_update = True
    torch.manual_seed(20)
    out = trainer.train_self_critical(_clone(b), n_samples=n, baseline='greedy')
    torch.cuda.synchronize()
    assert set(out) >= {'loss', 'reward_mean', 'baseline_mean', 'reward', 'adv'} and all(v.is_cuda for v in out.values())
    assert out['reward'].shape == out['adv'].shape == (B, n) and bool(torch.isfinite(out['loss']))
    _check_against_host(out, greedy, n, 'greedy')
    base = out['baseline'].reshape(B).cpu()
    print('\ngreedy baseline per image: %s, rewards %s' % (base.tolist(), out['reward'].cpu().tolist()))
    assert ((base >= 0.0) & (base <= 1.0)).all()             # (1 where the step's greedy caption is the reference again)
    # a row contributes when its advantage is not zero and it has a target (a sample that starts with the pad id has none)
    counted = (out['adv'] != 0) & (out['gen_ids_samples'][:, :, 1] != PAD)
    assert bool(counted.any()) == (float(trainer.flat.grad.abs().max()) > 0)
    trainer.flat.zero_grad()
    trainer.defer_update = False
    # ---- leave-one-out, with the update
    before = trainer.flat.flat.clone()
    found = None
    for seed in (21, 22, 23, 24, 25):
        torch.manual_seed(seed)
        out = trainer.train_self_critical(_clone(b), n_samples=n, baseline='leave_one_out', max_order=4)
        torch.cuda.synchronize()
        r = _check_against_host(out, greedy, n, 'leave_one_out')
        assert bool(torch.isfinite(out['loss'])), seed
        differ = sum(len(set(_bits(r[i]).tolist())) > 1 for i in range(B))
        print('seed %d: images with two different rewards %d of %d, reward mean %.4f, loss %.6f'
              % (seed, differ, B, float(out['reward_mean']), float(out['loss'])))
        if 2 * differ >= B:
            found = seed
            break
    assert found is not None, 'no seed in 21..25 under which half the images have two samples with different rewards'
    assert float(out['adv'].abs().max()) > 0
    assert torch.allclose(out['reward_mean'], out['reward'].mean()) and torch.allclose(out['baseline_mean'], out['baseline'].mean())
    assert not torch.equal(trainer.flat.flat, before)        # the parameters moved
    assert trainer.skipped_steps() == 0 and model.training
    # ---- a caller's reward in place of the kernel's: the same definition of the advantage
    torch.manual_seed(found)
    seen = {}

    def length_reward(ids, batch):
        seen['shape'] = tuple(ids.shape)
        return ((ids[:, :, 1:] != PAD) & (ids[:, :, 1:] != EOS)).sum(-1).float() / 100.0
    out = trainer.train_self_critical(_clone(b), n_samples=n, reward=length_reward)
    rw = out['reward'].cpu().numpy()
    assert seen['shape'][:2] == (B, n) and np.array_equal(_bits(out['adv'].cpu().numpy()), _bits(scst_ref.leave_one_out(rw)))
    # ---- refusals
    for kw, what in ((dict(n_samples=0), 'n_samples'), (dict(n_samples=17), 'n_samples'), (dict(baseline='mean'), 'baseline'),
                     (dict(n_samples=1), 'leave_one_out'), (dict(max_order=5), 'max_order')):
        with pytest.raises(ValueError, match=what):
            trainer.train_self_critical(_clone(b), **kw)
    model.sampling_topk = 1
    with pytest.raises(ValueError, match='sampling model'):
        trainer.train_self_critical(_clone(b))


@pytest.mark.parametrize('defer', [True, False], ids=['defer_update', 'with_update'])
def test_the_plain_step_is_undisturbed(defer):
    """(e) lr = 0, weight_decay = 0, dropout off: a captured plain step, an SCST step, a plain step again - the two plain
    steps' losses and gradients are bit-equal and the second one is a graph replay; with the update in the step (gradient
    stores in force) the weights stay where they were as well"""
    kind = 'faces_objects'
    trainer, _ = _fp32_trainer(kind, ocfg=dict(OCFG, lr=0.0, weight_decay=0.0), sampling_topk=4, sampling_temp=0.8)
    trainer.defer_update = defer
    batch = _dev(_batch(kind, seed=55))
    sg = trainer.step_graph
    assert sg is not None

    def plain():
        before = sg.replays
        loss = trainer.train_one_batch(_clone(batch)).clone()
        torch.cuda.synchronize()
        g = trainer.flat.grad.clone()
        if defer:
            trainer.flat.zero_grad()
        return loss, g, sg.replays - before
    for _ in range(3):
        plain()                                              # eager, capture + first replay, replay
    weights = trainer.flat.flat.clone()
    l_a, g_a, replayed_a = plain()
    assert replayed_a == 1 and float(g_a.abs().max()) > 0
    state = (trainer._store, trainer._stored_last, trainer.flat.accum_pending)
    torch.manual_seed(7)
    replays = sg.replays
    out = trainer.train_self_critical(_clone(batch), n_samples=2)
    torch.cuda.synchronize()
    assert sg.replays == replays and bool(torch.isfinite(out['loss']))   # the SCST step never enters StepGraph.run
    assert trainer._store == state[0]
    if defer:
        assert trainer.flat.accum_pending
        trainer.flat.zero_grad()
    else:
        assert float(trainer.flat.grad.abs().max()) == 0.0   # zero + accumulate: its update cleared the whole buffer
    l_b, g_b, replayed_b = plain()
    assert replayed_b == 1
    assert torch.equal(l_b, l_a) and torch.equal(g_b, g_a)
    assert torch.equal(trainer.flat.flat, weights)
    if not defer:
        assert trainer._stored_last and trainer.flat.stored_numel > 0
