"""Several sampled captions per image on the MI355X: tell_sample_rank against its host definition
(`sample_rank_definition`), `generate(n_samples=n)` on the fp32 golden models against the repeated batch and the CPU oracle,
the packed-K/V bf16 step, and generate_lanes."""
import numpy as np
import pytest
import torch

from test_gpu_sampling import _alive, _clone, _golden_model
from test_prefix_host import ragged_prefix

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD, EOS = 1, 2


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    yield
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- 1. tell_sample_rank against the definition
RANK_B, RANK_L = 3, 12
RANK_SEEDS = {1: 0, 2: 1, 5: 1, 16: 8}        # per n: a seed whose consensus gaps pass _gaps_ok (checked in the test)


def _rank_case(n, seed, B=RANK_B, L=RANK_L):
    """ids int64 [B * n, L], lps fp32 [B * n, L - 1], done_step int64 [B * n] over a six-token alphabet (bigrams overlap), with
    something behind every row's end that must not be read, and the deliberate cases: image 0 draws 0 / 1 identical (n >= 2);
    image 1 draws 0 / 1 different tokens with the same log-probs - an exact score tie (n >= 2); image 2 draw 1 equal to draw 0
    up to </s> and different behind it (n >= 2); rows that never end (done_step = 100 > steps) and a row whose first token is
    </s> (n = 1 and n >= 5)."""
    rng = np.random.RandomState(1000 * n + seed)
    steps, R = L - 1, B * n
    ids = np.full((R, L), PAD, dtype=np.int64)
    ids[:, 0] = 0
    lps = np.zeros((R, steps), dtype=np.float32)
    done = np.zeros(R, dtype=np.int64)

    def put(r, ln, ended):
        ids[r, 1:] = rng.randint(3, 9, size=steps)
        lps[r] = -(rng.rand(steps).astype(np.float32) * 3 + np.float32(0.01))
        if ended:
            ids[r, ln] = EOS
        done[r] = ln if ended else 100
    for r in range(R):
        put(r, int(rng.randint(2, steps + 1)), True)
    never, first = ([(0, 0)], [(1, 0)]) if n == 1 else ([(0, 2), (2, 4)], [(1, 3)]) if n >= 5 else ([], [])
    for b, j in never:
        put(b * n + j, steps, False)
    for b, j in first:
        put(b * n + j, 1, True)
    if n >= 2:
        ids[1], lps[1], done[1] = ids[0], lps[0], done[0]                   # image 0: identical
        a = n                                                               # image 1: an exact score tie, other tokens
        ln = int(done[a])
        put(a + 1, ln, True)
        lps[a + 1] = lps[a]
        if (ids[a + 1, 1:ln] == ids[a, 1:ln]).all():
            ids[a + 1, 1] = 3 + (ids[a, 1] - 3 + 1) % 6
        c = 2 * n                                                           # image 2: the same up to </s>
        ln = int(done[c])
        ids[c + 1, :ln + 1], done[c + 1] = ids[c, :ln + 1], ln
    return ids, lps, done, steps


def _bigrams(ids, ln, eos=EOS):
    from collections import Counter
    g = [int(t) for t in ids[1:1 + ln]]
    if g and g[-1] == eos:
        g = g[:-1]
    return Counter(zip(g, g[1:]))


def _gaps_ok(ids, d, n):
    """Every pair of hypotheses of an image: consensus more than 1e-3 apart, or a deliberate tie (the same bigram multiset -
    identical rows, rows without bigrams - whose consensus is then exactly equal)."""
    for b in range(d['cons'].shape[0]):
        for i in range(n):
            for j in range(i + 1, n):
                gap = abs(float(d['cons'][b, i]) - float(d['cons'][b, j]))
                same = _bigrams(ids[b * n + i], int(d['len'][b, i])) == _bigrams(ids[b * n + j], int(d['len'][b, j]))
                if not (gap > 1e-3 or (same and gap == 0.0)):
                    return False
    return True


def test_rank_case_seeds_keep_the_consensus_gaps_open():
    """(no device work) the cases of the committed seeds pass _gaps_ok and hold what they promise."""
    from tell_amd.models.transformer import sample_rank_definition
    for n, seed in RANK_SEEDS.items():
        ids, lps, done, steps = _rank_case(n, seed)
        d = sample_rank_definition(ids, lps, done, n, steps, EOS, 'consensus')
        assert _gaps_ok(ids, d, n), (n, seed)
        assert ids.shape == (RANK_B * n, 12)
        if n >= 2:
            assert d['dup'][0, 1] == 1 and d['dup'][2, 1] == 1 and d['dup'][1, 1] == 0
            assert d['score'][1, 0] == d['score'][1, 1] and (ids[n] != ids[n + 1]).any()
            assert (ids[2 * n] != ids[2 * n + 1]).any()                     # (they differ, behind </s>)
        if n == 1 or n >= 5:
            assert (d['len'] == steps).any() and (done == 100).any() and (d['len'] == 1).any()


@pytest.mark.parametrize('n', [1, 2, 5, 16])
def test_rank_kernel_matches_the_definition(n):
    """len, dup and order exactly, score bit for bit, cons within 1e-6 - for the three rules, without a length penalty and
    with alpha = 0.7."""
    from tell_amd import ops
    from tell_amd.models.transformer import inv_norm_table, sample_rank_definition
    ids, lps, done, steps = _rank_case(n, RANK_SEEDS[n])
    t_ids, t_lps, t_done = torch.from_numpy(ids).to(DEV), torch.from_numpy(lps).to(DEV), torch.from_numpy(done).to(DEV)
    for alpha in (None, 0.7):
        table = None if alpha is None else inv_norm_table(alpha, steps)
        for rule in ('draw', 'score', 'consensus'):
            want = sample_rank_definition(ids, lps, done, n, steps, EOS, rule, None if table is None else table.numpy())
            order, score, dup, cons, ln = ops.sample_rank(t_ids, t_lps, t_done, RANK_B, n, steps, PAD, EOS, rule,
                                                          inv_norm=None if table is None else table.to(DEV),
                                                          want_cons=True, want_len=True)
            torch.cuda.synchronize()
            assert np.array_equal(ln.cpu().numpy(), want['len']), (rule, alpha)
            assert np.array_equal(dup.cpu().numpy(), want['dup']), (rule, alpha)
            assert np.array_equal(score.cpu().numpy().view(np.int32), want['score'].view(np.int32)), (rule, alpha)
            diff = np.abs(cons.cpu().numpy() - want['cons']).max()
            print('\nn=%d %s alpha=%s: max |cons - definition| = %.3g' % (n, rule, alpha, diff))
            assert diff <= 1e-6, (rule, alpha, diff)
            assert np.array_equal(order.cpu().numpy(), want['order']), (rule, alpha, order.cpu().numpy(), want['order'])
            if rule != 'consensus':                                         # cons may be NULL unless the rule needs it
                o2, s2, d2, c2, l2 = ops.sample_rank(t_ids, t_lps, t_done, RANK_B, n, steps, PAD, EOS, rule,
                                                     inv_norm=None if table is None else table.to(DEV))
                assert c2 is None and l2 is None and torch.equal(o2, order) and torch.equal(s2, score) and torch.equal(d2, dup)


def test_rank_kernel_reads_strided_rows_of_the_longest_caption():
    """The generator's own buffers: ids [R, 257] / lps [R, 256] at steps = 256, 16 hypotheses - the LDS capacity."""
    from tell_amd import ops
    from tell_amd.models.transformer import sample_rank_definition
    rng = np.random.RandomState(7)
    B, n, steps = 2, 16, 256
    ids = rng.randint(3, 40, size=(B * n, steps + 1)).astype(np.int64)
    lps = -rng.rand(B * n, steps).astype(np.float32)
    done = rng.randint(200, 300, size=B * n).astype(np.int64)
    for r in range(B * n):
        if done[r] <= steps:
            ids[r, done[r]] = EOS
    ids[5], lps[5], done[5] = ids[3], lps[3], done[3]
    want = sample_rank_definition(ids, lps, done, n, steps, EOS, 'consensus')
    got = ops.sample_rank(torch.from_numpy(ids).to(DEV), torch.from_numpy(lps).to(DEV), torch.from_numpy(done).to(DEV), B, n,
                          steps, PAD, EOS, 'consensus', want_len=True)
    torch.cuda.synchronize()
    assert np.array_equal(got[4].cpu().numpy(), want['len']) and np.array_equal(got[2].cpu().numpy(), want['dup'])
    assert want['dup'][0, 5] == 1 and want['dup'].sum() == 1
    assert np.array_equal(got[1].cpu().numpy().view(np.int32), want['score'].view(np.int32))
    assert np.abs(got[3].cpu().numpy() - want['cons']).max() <= 1e-6
    with pytest.raises(RuntimeError, match='sample_rank'):
        ops.sample_rank(torch.from_numpy(ids).to(DEV), torch.from_numpy(lps).to(DEV), torch.from_numpy(done).to(DEV), 1, 32,
                        steps, PAD, EOS, 'score')


# --------------------------------------------------------------------------- 2. the fp32 golden models
N_FP32, T_FP32 = 3, 0.8
KEYS = ('gen_ids', 'log_probs', 'scores', 'gen_ids_samples', 'log_probs_samples', 'scores_samples', 'sample_index', 'duplicate')


def _repeat(batch, n):
    return {k: ({kk: vv.repeat_interleave(n, dim=0) for kk, vv in v.items()} if isinstance(v, dict)
                else v.repeat_interleave(n, dim=0)) for k, v in batch.items()}


def _seed_of(torch_seed):
    from tell_amd.models.transformer import draw_seed
    torch.manual_seed(torch_seed)
    return draw_seed()


def _same(a, b, keys=KEYS):
    return all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in keys)


def _oracle_lp(kind, fx, batch_cpu, ids):
    """Teacher-forced log-probs [R, steps, V] of the fp32 CPU oracle on ids [R, steps + 1]."""
    from oracle.build import build_model as obuild
    from test_gpu_decoder import DEC_KW
    from test_oracle_golden import _PoolResnet as OResnet, _TableRoberta as ORoberta
    art_dim = 64 if kind == 'flattened' else 1024
    cpu = obuild(kind, OResnet(), ORoberta(art_dim), article_dim=art_dim, **DEC_KW).eval()
    own = cpu.state_dict()
    cpu.load_state_dict({k: v for k, v in fx['sd'].items() if k in own}, strict=False)
    with torch.no_grad():
        b = batch_cpu
        _, _, ctx = cpu._forward(b['context'], b['image'], b['caption'], b.get('face_embeds'), b.get('obj_embeds'))
        out = cpu.decoder({'roberta': ids[:, :-1]}, ctx)
        return cpu.decoder.get_normalized_probs((out[0], None), log_probs=True).float()


@pytest.mark.parametrize('kind', ['flattened', 'faces_objects'])
def test_golden_models_draw_n_samples_fp32(golden, kind):
    import tell_amd
    model, fx, batch = _golden_model(golden, kind, 5, T_FP32)
    n, T = N_FP32, T_FP32
    B = batch()['image'].shape[0]
    R = B * n
    keep = tell_amd.graphs.ENABLED

    def run(seed, graphed=True, **kw):
        tell_amd.graphs.ENABLED = graphed
        try:
            torch.manual_seed(seed)
            out = model.generate(**kw.pop('b', None) or batch(), **kw)
            torch.cuda.synchronize()
            return out
        finally:
            tell_amd.graphs.ENABLED = keep
    # ---- n_samples = 1 is the plain call: the same outputs, the same keys, the same graph signatures
    plain = run(123)
    sigs = set(model.__dict__['_decode_graphs'])
    one = run(123, n_samples=1, rank_by='consensus', rank_len_penalty=0.7)
    assert set(one) == set(plain) and all(torch.equal(one[k], plain[k]) for k in ('gen_ids', 'log_probs', 'scores'))
    assert set(model.__dict__['_decode_graphs']) == sigs
    # ---- a seed under which the repeated batch agrees with itself, eager against captured
    rep = None
    for seed in (123, 124, 125, 126, 127):
        a, b_ = run(seed, b=_repeat(batch(), n)), run(seed, graphed=False, b=_repeat(batch(), n))
        if a['gen_ids'].shape == b_['gen_ids'].shape and torch.equal(a['gen_ids'], b_['gen_ids']) and \
                torch.equal(a['log_probs'], b_['log_probs']):
            rep = a
            break
    assert rep is not None, 'no seed in 123..127 under which the repeated batch agrees eager / captured'
    # ---- draw order: hypothesis (b, j) is row b * n + j of the repeated batch
    draw = run(seed, n_samples=n, rank_by='draw')
    assert set(draw) == set(plain) | set(KEYS)
    L = draw['gen_ids_samples'].shape[2]
    assert draw['gen_ids_samples'].shape == (B, n, L) and draw['log_probs_samples'].shape == (B, n, L - 1)
    assert draw['scores_samples'].shape == (B, n) and draw['duplicate'].shape == (B, n) and draw['duplicate'].dtype == torch.bool
    assert draw['sample_index'].dtype == torch.long and draw['sample_index'].tolist() == [list(range(n))] * B
    ids = draw['gen_ids_samples'].reshape(R, L).cpu()
    lps = draw['log_probs_samples'].reshape(R, L - 1).cpu()
    W = max(L, rep['gen_ids'].shape[1])
    pad_to = lambda t, w, v: torch.cat([t, t.new_full((t.shape[0], w - t.shape[1]), v)], 1)   # noqa: E731
    r_ids, r_lps = pad_to(rep['gen_ids'].cpu(), W, PAD), pad_to(rep['log_probs'].cpu(), W - 1, 0.0)
    w_ids, w_lps = pad_to(ids, W, PAD), pad_to(lps, W - 1, 0.0)
    lp_all = _oracle_lp(kind, fx, _repeat(batch('cpu'), n), ids)                       # [R, L - 1, V]
    differ = [r for r in range(R) if not (torch.equal(w_ids[r], r_ids[r]) and torch.equal(w_lps[r], r_lps[r]))]
    print('\n%s: rows that differ from the repeated batch: %s of %d (seed %d)' % (kind, differ, R, seed))
    assert len(differ) <= 1, differ
    for r in differ:                                     # only from a boundary draw
        t = int((w_ids[r] != r_ids[r]).nonzero()[0]) - 1                               # the first differing step
        top = lp_all[r, t].topk(5)
        assert lp_all[r, t, w_ids[r, t + 1]] >= top.values[-1] - 1e-4 and lp_all[r, t, r_ids[r, t + 1]] >= top.values[-1] - 1e-4
        u = tell_amd.hip.lib().tell_sample_uniform_host(_seed_of(seed), r, t)
        c = np.cumsum(np.exp((top.values.double().numpy() - float(top.values[0])) / T))
        assert np.abs(u - c / c[-1]).min() <= 1e-4, (r, t, u, c / c[-1])
    # ---- every hypothesis against the CPU oracle: inside the top 5, log-prob = lp / T
    alive = _alive(ids)
    tok = ids[:, 1:]
    fifth = lp_all.topk(5, dim=-1).values[..., -1]
    lp_tok = lp_all.gather(2, tok.unsqueeze(-1)).squeeze(-1)
    assert (lp_tok >= fifth - 1e-4)[alive].all()
    assert torch.allclose(lps[alive], (lp_tok / T)[alive], atol=2e-4, rtol=0), (lps - lp_tok / T)[alive].abs().max()
    assert (lps[~alive] == 0).all() and (tok[~alive] == PAD).all()
    # (the kernel adds in ascending order, torch pairwise: a few ulps of a sum of a dozen terms)
    assert torch.allclose(draw['scores_samples'].cpu(), lps.view(B, n, -1).sum(-1), atol=1e-5, rtol=1e-5)
    assert any(len({tuple(ids[b * n + j].tolist()) for j in range(n)}) > 1 for b in range(B))   # not n copies of one caption
    # ---- the flows agree; a seed is a seed
    assert _same(run(seed, n_samples=n, rank_by='draw'), draw) and _same(run(seed, graphed=False, n_samples=n, rank_by='draw'), draw)
    other = run(seed + 100, n_samples=n, rank_by='draw')
    assert other['gen_ids_samples'].shape != draw['gen_ids_samples'].shape or \
        not torch.equal(other['gen_ids_samples'], draw['gen_ids_samples'])
    hs = [h for sig, h in model.__dict__['_decode_graphs'].items() if ('hyp', n) in sig]
    assert len(hs) == 1 and hs[0]['graph'] not in (None, False), [h.get('error') for h in hs]
    assert not any(('hyp', n) in sig for sig in sigs)
    # ---- rank order: a permutation of the draws, duplicates last, scores non-increasing among the others
    for rule, alpha in (('score', 0.0), ('score', 0.7), ('consensus', 0.0)):
        out = run(seed, n_samples=n, rank_by=rule, rank_len_penalty=alpha)
        idx = out['sample_index']
        assert idx.sort(1).values.tolist() == [list(range(n))] * B
        pick = lambda t: t.gather(1, idx.view(B, n, *[1] * (t.dim() - 2)).expand(-1, -1, *t.shape[2:]))   # noqa: E731
        assert torch.equal(out['gen_ids_samples'], pick(draw['gen_ids_samples']))
        assert torch.equal(out['log_probs_samples'], pick(draw['log_probs_samples']))
        assert torch.equal(out['duplicate'], pick(draw['duplicate']))
        assert torch.equal(out['gen_ids'], out['gen_ids_samples'][:, 0]) and torch.equal(out['log_probs'], out['log_probs_samples'][:, 0])
        assert torch.equal(out['scores'], out['scores_samples'][:, 0])
        dup, sc = out['duplicate'].cpu(), out['scores_samples'].cpu()
        for b in range(B):
            k = int((~dup[b]).sum())
            assert not dup[b, :k].any() and dup[b, k:].all()                           # duplicates behind the others
            if rule == 'score':
                assert (sc[b, 1:k] <= sc[b, :k - 1]).all(), sc[b]
        if alpha == 0.0:
            assert torch.equal(out['scores_samples'], pick(draw['scores_samples']))
    # ---- a ragged prefix, one row per image, shared by its n hypotheses
    plens = [0, 1, 3, 1][:B]
    pfx = ragged_prefix(plain['gen_ids'].cpu(), plens).to(DEV)
    out = run(seed, n_samples=n, rank_by='draw', prefix=pfx)
    assert out['prefix_len'].tolist() == plens
    for b, p in enumerate(plens):
        for j in range(n):
            assert torch.equal(out['gen_ids_samples'][b, j, 1:1 + p], pfx[b, :p]), (b, j)
            assert torch.equal(out['log_probs_samples'][b, j, :p], out['log_probs_samples'][b, 0, :p]), (b, j)
    assert len([1 for sig in model.__dict__['_decode_graphs'] if ('hyp', n) in sig and ('prefix',) in sig]) == 1


# --------------------------------------------------------------------------- 3. bf16: the packed-K/V step
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


def _max_count(ids):
    """The largest number of positions of one row that hold the same (non-pad) token."""
    best = 0
    for row in ids.reshape(-1, ids.shape[-1]).cpu():
        h = [int(t) for t in row[1:] if int(t) != PAD]
        best = max([best] + [h.count(t) for t in set(h)])
    return best


BF16_RULES = {'nucleus': dict(sampling_topk=0, sampling_topp=0.9), 'minp': dict(sampling_topk=0, sampling_minp=0.1),
              'penalised': dict(sampling_topk=8, repetition_penalty=1.3)}


@pytest.mark.parametrize('n', [2, 5])
@pytest.mark.parametrize('mode', sorted(BF16_RULES))
def test_small_bf16_model_draws_n_samples_on_the_captured_step(mode, n):
    import tell_amd
    from tell_amd import decode
    try:
        model = _small_bf16(**BF16_RULES[mode])
        b = _small_batch()
        B = 3

        def run(seed, **kw):
            torch.manual_seed(seed)
            with torch.no_grad():
                out = model.generate(**kw.pop('b', None) or _clone(b), **kw)
            torch.cuda.synchronize()
            return out
        a, a2 = run(9, n_samples=n), run(9, n_samples=n)
        assert _same(a, a2)
        L = a['gen_ids_samples'].shape[2]
        assert a['gen_ids_samples'].shape == (B, n, L) and a['log_probs_samples'].shape == (B, n, L - 1)
        assert a['scores_samples'].shape == a['duplicate'].shape == a['sample_index'].shape == (B, n)
        hs = [h for sig, h in model.__dict__['_decode_graphs'].items() if ('hyp', n) in sig]
        assert len(hs) == 1 and hs[0]['graph'] not in (None, False), [h.get('error') for h in hs]
        assert all(isinstance(c, decode.PackedKV) for lk in hs[0]['kv'] for c in lk.values())     # the packed step, n = 2 and odd n
        # the score the rank kernel reports is the sum of the recorded log-probs (alpha = 0): sequential against pairwise
        # fp32 adds of at most 100 terms of magnitude <= 400 in sum - a few ulps of the sum
        sums = a['log_probs_samples'].sum(-1)
        assert torch.allclose(a['scores_samples'], sums, rtol=1e-5, atol=1e-5), (a['scores_samples'] - sums).abs().max()
        if mode == 'penalised':
            d = run(9, n_samples=n, rank_by='draw')
            single = run(9, b=_repeat(_clone(b), n))                     # one draw per row, the same row keys
            got, allowed = _max_count(d['gen_ids_samples']), _max_count(single['gen_ids'])
            # row by row, for the record: the shared call attends with the packed MFMA kernel, the repeated batch with one
            # hypothesis per sample (another kernel, other bf16 rounding), so a row may part from its twin at a boundary draw
            # and the two counts of such a row are unrelated - the assertion is on what the setting allows over all rows
            W = max(d['gen_ids_samples'].shape[2], single['gen_ids'].shape[1])
            widen = lambda t: torch.cat([t, t.new_full((t.shape[0], W - t.shape[1]), PAD)], 1)   # noqa: E731
            rows_s, rows_r = widen(d['gen_ids_samples'].reshape(B * n, -1)), widen(single['gen_ids'])
            same = [bool(torch.equal(rows_s[r], rows_r[r])) for r in range(B * n)]
            per_row = [(_max_count(rows_s[r:r + 1]), _max_count(rows_r[r:r + 1])) for r in range(B * n)]
            print('\nbf16 %s n=%d: a token at most %d times in a hypothesis, %d times in the single-draw rows; %d of %d rows equal '
                  'their single-draw twin; per row (shared, single): %s' % (mode, n, got, allowed, sum(same), B * n, per_row))
            assert got <= allowed
            return
        # score_captions on a hypothesis' own tokens gives its summed log-prob (rtol 3e-2: the bf16 score tolerance of
        # tests/test_gpu_prefix.py; the scoring pass attends with one hypothesis per sample, another kernel)
        # A random-weight model also draws the pad id as a token, which a right-padded caption cannot hold: such a hypothesis
        # is scored up to that token - its summed log-prob over the same steps is what score_captions must give.
        for j in range(n):
            cap = a['gen_ids_samples'][:, j].clone()
            lead = (cap[:, 1:] != PAD).long().cumprod(1).bool()          # the leading non-pad tokens behind <s>
            cap[:, 1:] = torch.where(lead, cap[:, 1:], torch.full_like(cap[:, 1:], PAD))
            sb = _clone(b)
            sb['caption'] = {'roberta': cap}
            with torch.no_grad():
                got = model.score_captions(sb)
            sc = got['scores']
            assert got['prefix_len'].tolist() == lead.sum(1).tolist()
            want = (a['log_probs_samples'][:, j] * lead).sum(-1)
            print('\nbf16 %s n=%d draw %d: %s of %s steps compared; scores %s, score_captions %s'
                  % (mode, n, j, lead.sum(1).tolist(), (a['gen_ids_samples'][:, j, 1:] != PAD).sum(1).tolist(), want.tolist(),
                     sc.tolist()))
            assert torch.allclose(sc, want, rtol=3e-2, atol=0), (sc, want)
    finally:
        tell_amd.set_compute_dtype(torch.float32)


def test_lanes_with_two_samples_equal_batch_by_batch():
    import tell_amd
    try:
        model = _small_bf16(sampling_topk=8, sampling_temp=0.9)
        batches = [_small_batch(3, seed=41 + i) for i in range(4)]
        torch.manual_seed(21)
        with torch.no_grad():
            alone = [model.generate(**_clone(b), n_samples=2, rank_by='consensus') for b in batches]
        torch.cuda.synchronize()
        torch.manual_seed(21)
        seen = 0
        for i, (_, out) in enumerate(model.generate_lanes((_clone(b) for b in batches), lanes=2, n_samples=2, rank_by='consensus')):
            torch.cuda.synchronize()
            assert set(out) == set(alone[i]) and _same(out, alone[i]), i
            seen += 1
        assert seen == len(batches)
    finally:
        tell_amd.set_compute_dtype(torch.float32)
