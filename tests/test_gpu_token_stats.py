"""Per-token statistics on the MI355X: tell_adaptive_logprob_stats over the case table of
tests/token_stats_ref.py - alternatives bit-equal to tell_adaptive_logprob_topk, the rank invariants, ranks against float64,
entropy within the derived bound - and generate(token_stats=) / score_captions(token_stats=) through the captured step."""
import numpy as np
import pytest
import torch

import token_stats_ref as R
from guarded import Guard

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD, EOS = 1, 2
SLOTS, STEP = 3, 1


# --------------------------------------------------------------------------- 1. the kernel
def _device_logits(case, rows):
    """-> the head / tail arguments of the entry points for a case in its layout (tests/token_stats_ref.py CASES)."""
    head, tl = R.logits(case['name'], rows)
    c0, tails = case['c0'], case['tails']

    def ld_of(n):
        ld = -(-n // 4) * 4
        return ld + 1 if case['layout'] == 'odd' else ld      # (odd: rows 1.. start off 16 bytes)
    if case['layout'] == 'sliced':                            # head_step's composed layout: segments padded to 4, one buffer
        offs, off = [], 0
        for n in (c0 + len(tails),) + tuple(tails):
            offs.append(off)
            off += -(-n // 4) * 4
        big = torch.zeros(rows, off, dtype=torch.float32, device=DEV)
        big[:, :c0 + len(tails)] = torch.from_numpy(head.copy())
        for o, t in zip(offs[1:], tl):
            big[:, o:o + t.shape[1]] = torch.from_numpy(t.copy())
        args = [big, off, c0, len(tails)]
        for i in range(3):
            args += [big[:, offs[1 + i]:], off, tails[i]] if i < len(tails) else [None, 0, 0]
        return args
    bufs = []
    for a in [head] + list(tl):
        ld = ld_of(a.shape[1])
        b = torch.zeros(rows, ld, dtype=torch.float32, device=DEV)
        b[:, :a.shape[1]] = torch.from_numpy(a.copy())
        bufs.append((b, ld))
    args = [bufs[0][0], bufs[0][1], c0, len(tails)]
    for i in range(3):
        args += [bufs[1 + i][0], bufs[1 + i][1], tails[i]] if i < len(tails) else [None, 0, 0]
    return args


def _outputs(rows, n):
    return (Guard((SLOTS, rows, n), torch.int32), Guard((SLOTS, rows, n), torch.float32), Guard((SLOTS, rows), torch.int32),
            Guard((SLOTS, rows), torch.float32), Guard((SLOTS, rows), torch.float32))


def _stats(args, rows, chosen, ld_chosen, fin, n, outs, step=STEP, step_dev=None, slots=SLOTS):
    from tell_amd.hip import call
    call('tell_adaptive_logprob_stats', *args, rows, chosen, ld_chosen, fin, n, slots, step, step_dev, PAD,
         *[g.t for g in outs])


ENTROPY_RATIOS = {}


@pytest.mark.parametrize('regs', [1, 0])
@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c['name'])
def test_stats_kernel(case, regs):
    """Rows 1 / 5 / 33 x n 1 / 4 / 8, every output a guarded view, the chosen column the first of a wider [rows, 3] buffer.
    alt_tok / alt_lp: bit-equal to tell_adaptive_logprob_topk(k = n); chosen_lp bit-equal to the alternatives' entry where
    rank < n, c absent from them where rank >= n; rank == the float64 rank on every row (the host test shows it is the only
    admissible one; the tie table included, ties to the lower id); with argmax_regs = 0 also the count over the full row of
    tell_adaptive_logprob_argmax(log_probs=); entropy within bound_entropy of float64 (printed as a ratio to the derived
    bound); a token outside the vocabulary: rank -1, chosen_lp 0; finished rows neutral; step_dev gives the bytes of step;
    slots other than the step's are untouched."""
    from tell_amd import hip
    from tell_amd.hip import call
    V = R.vocab(case)
    with hip.options(argmax_regs=regs):
        for rows in R.ROWS:
            args = _device_logits(case, rows)
            ref = R.reference(case['name'], rows)
            tok, kinds = R.chosen(case['name'], rows)
            chosen = torch.full((rows, 3), -77, dtype=torch.int32, device=DEV)
            chosen[:, 0] = torch.from_numpy(tok)
            full = None
            if not regs:
                full = torch.empty(rows, V, dtype=torch.float32, device=DEV)
                call('tell_adaptive_logprob_argmax', *args, rows, full, V, torch.empty(rows, dtype=torch.int32, device=DEV),
                     torch.empty(rows, dtype=torch.float32, device=DEV))
                full = full.cpu().numpy()
            for n in R.ALTS:
                t_tok = torch.empty(rows, n, dtype=torch.int32, device=DEV)
                t_lp = torch.empty(rows, n, dtype=torch.float32, device=DEV)
                call('tell_adaptive_logprob_topk', *args, rows, n, t_tok, t_lp)
                outs = _outputs(rows, n)
                _stats(args, rows, chosen, 3, None, n, outs)
                torch.cuda.synchronize()
                assert all(g.intact() for g in outs), (rows, n)
                a_tok, a_lp, rank, ent, c_lp = (g.t[STEP] for g in outs)
                for g in outs:                                # the other slots: nothing written
                    assert bool((g.t[0] == g.sentinel).all()) and bool((g.t[2] == g.sentinel).all())
                assert torch.equal(a_tok, t_tok) and torch.equal(a_lp.view(torch.int32), t_lp.view(torch.int32)), (rows, n)
                a_tok, a_lp, rank, ent, c_lp = (x.cpu().numpy() for x in (a_tok, a_lp, rank, ent, c_lp))
                for r in range(rows):
                    c = int(tok[r])
                    if kinds[r] == 'outside':
                        assert rank[r] == -1 and c_lp[r] == 0.0, (rows, n, r)
                        continue
                    want = R.rank_of(ref['lp'][r], c)
                    assert rank[r] == want, (case['name'], rows, n, r, kinds[r], rank[r], want)
                    assert abs(float(c_lp[r]) - ref['lp'][r, c]) <= ref['d_lp'][r], (rows, n, r)
                    if rank[r] < n:
                        assert a_tok[r, rank[r]] == c and a_lp[r, rank[r]].view(np.int32) == c_lp[r].view(np.int32), (rows, n, r)
                    else:
                        assert c not in a_tok[r].tolist(), (rows, n, r)
                    if full is not None:
                        cnt = int(((full[r] > full[r, c]) | ((full[r] == full[r, c]) & (np.arange(V) < c))).sum())
                        assert rank[r] == cnt, (rows, n, r, rank[r], cnt)
                err = np.abs(ent.astype(np.float64) - ref['entropy'])
                ratio = float((err / ref['d_entropy']).max())
                ENTROPY_RATIOS[(case['name'], regs, rows, n)] = ratio
                print('%s regs=%d rows=%d n=%d: entropy max |err| %.3e, largest ratio to the derived bound %.4f'
                      % (case['name'], regs, rows, n, err.max(), ratio))
                assert (err <= R.bound_entropy(case['name'], rows, c=1.0)).all(), (rows, n, ratio)       # the derived bound
                assert (err <= R.bound_entropy(case['name'], rows)).all(), (rows, n, ratio, R.C_ENTROPY)  # the pinned one
                # finished rows are neutral and leave the others as they were; step_dev = step - 1 gives the same bytes
                fin = torch.zeros(rows, dtype=torch.uint8, device=DEV)
                fin[::2] = 1
                outs_f, outs_d = _outputs(rows, n), _outputs(rows, n)
                _stats(args, rows, chosen, 3, fin, n, outs_f)
                _stats(args, rows, chosen, 3, None, n, outs_d, step=12345,
                       step_dev=torch.tensor([STEP - 1], dtype=torch.int32, device=DEV))
                torch.cuda.synchronize()
                assert all(g.intact() for g in outs_f + outs_d)
                for g, gf, gd, neutral in zip(outs, outs_f, outs_d, (PAD, 0.0, -1, 0.0, 0.0)):
                    assert torch.equal(gd.buf.view(torch.int32), g.buf.view(torch.int32))
                    assert bool((gf.t[STEP][::2] == neutral).all())
                    assert torch.equal(gf.t[STEP][1::2].view(torch.int32), g.t[STEP][1::2].view(torch.int32))
    if case['content'] == 'uniform':
        assert abs(float(ent[0]) - np.log(V)) <= 4e-6
    mine = {k: v for k, v in ENTROPY_RATIOS.items() if k[0] == case['name'] and k[1] == regs}
    worst = max(mine, key=mine.get)
    print('%s regs=%d: largest entropy ratio %.5f at rows=%d n=%d (so far overall %.5f; pinned c = %g)'
          % (case['name'], regs, mine[worst], worst[2], worst[3], max(ENTROPY_RATIOS.values()), R.C_ENTROPY))


def test_slot_out_of_range_writes_nothing_and_declined_calls_launch_nothing():
    from tell_amd import hip
    case = R.CASES[0]
    rows, n = 5, 4
    args = _device_logits(case, rows)
    chosen = torch.zeros(rows, 1, dtype=torch.int32, device=DEV)
    for dev_step in (SLOTS - 1, SLOTS + 5, -2):               # device path: slot = *step_dev + 1 outside [0, slots)
        outs = _outputs(rows, n)
        _stats(args, rows, chosen, 1, None, n, outs, step=0, step_dev=torch.tensor([dev_step], dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        assert all(g.untouched() for g in outs), dev_step
    lib = hip.lib()
    for kw, what in ((dict(step=SLOTS), 'step'), (dict(step=-1), 'step'), (dict(n=0), 'n'), (dict(n=9), 'n'), (dict(rows=0), 'rows')):
        outs = _outputs(rows, max(kw.get('n', n), 1))
        a = dict(step=STEP, n=n, rows=rows)
        a.update(kw)
        ptr = [x.data_ptr() if torch.is_tensor(x) else x for x in args]
        rc = lib.tell_adaptive_logprob_stats(*ptr, a['rows'], chosen.data_ptr(), 1, None, a['n'], SLOTS, a['step'], None, PAD,
                                             *[g.t.data_ptr() for g in outs], None)
        torch.cuda.synchronize()
        assert rc < 0 and what in lib.tell_last_error().decode(), (kw, rc)
        assert all(g.untouched() for g in outs), kw
        with pytest.raises(RuntimeError, match='tell_adaptive_logprob_stats'):
            hip.call('tell_adaptive_logprob_stats', *args, a['rows'], chosen, 1, None, a['n'], SLOTS, a['step'], None, PAD,
                     *[g.t for g in outs])


# --------------------------------------------------------------------------- 2. the generators
KEYS = ('alt_ids', 'alt_log_probs', 'token_rank', 'token_entropy', 'token_model_lp')
NEUTRAL = (PAD, 0.0, -1, 0.0, 0.0)


class _Spy:
    """Records the entry points issued through ops.call / decode.call (what a capture records, launch by launch)."""

    def __enter__(self):
        from tell_amd import decode, ops
        self.mods, self.real, self.names = (ops, decode), ops.call, []

        def call(name, *args):
            self.names.append(name)
            return self.real(name, *args)
        for m in self.mods:
            m.call = call
        return self

    def __exit__(self, *exc):
        for m in self.mods:
            m.call = self.real
        return False


def _clone(b):
    return {k: (dict(v) if isinstance(v, dict) else v.clone()) for k, v in b.items()}


@pytest.fixture(scope='module')
def models():
    """The full-width bf16 decoder (vocabulary 50265, width 1024: the composed one-product head, captured steps and multi-step
    replays) behind stand-in encoders, its </s> row sharpened so that rows end at different steps; 8 captions."""
    import tell_amd
    from tell_amd.build import build_model
    from tell_amd.data import synthetic_batch
    from test_gpu_fullsize import _sharpened_eos
    tell_amd.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    enc = R.score_encoders(True)
    plain = build_model('faces_objects', *enc, n_bert_layers=3)
    sd = _sharpened_eos(plain.state_dict(), 12.0)
    plain.load_state_dict(sd)
    plain.to(DEV).eval()

    def variant(**kw):
        m = build_model('faces_objects', *enc, n_bert_layers=3, **kw)
        m.load_state_dict(sd)
        return m.to(DEV).eval()
    batch = synthetic_batch(8, 24, 9, True, seed=91, device=DEV)
    yield plain, variant, batch
    tell_amd.set_compute_dtype(torch.float32)


def _check_neutral_behind_eos(out):
    ids = out['gen_ids'].cpu()
    steps = ids.shape[1] - 1
    live = torch.ones(ids.shape[0], steps, dtype=torch.bool)
    for b in range(ids.shape[0]):
        hit = (ids[b, 1:] == EOS).nonzero()
        if hit.numel():
            live[b, int(hit[0]) + 1:] = False
    for k, v in zip(KEYS, NEUTRAL):
        t = out[k].cpu()
        assert t.shape[:2] == (ids.shape[0], steps), (k, t.shape)
        assert bool((t[~live] == v).all()), k
    return live


def test_greedy_with_token_stats(models):
    plain, _, batch = models
    with torch.no_grad():
        base = plain.generate(**_clone(batch))
        out = plain.generate(**_clone(batch), token_stats=4)
        torch.cuda.synchronize()
    assert torch.equal(out['gen_ids'], base['gen_ids']) and torch.equal(out['log_probs'], base['log_probs'])
    assert not set(base) & set(KEYS)
    assert out['alt_ids'].dtype == torch.long and out['token_rank'].dtype == torch.long and out['alt_ids'].shape[2] == 4
    live = _check_neutral_behind_eos(out)
    print('greedy: %d steps, live tokens %d of %d' % (live.shape[1], int(live.sum()), live.numel()))
    assert 0 < int((~live).sum()) and int(live.sum()) > 20    # rows end at different steps, and most steps are live
    live = live.to(DEV)
    assert bool((out['token_rank'][live] == 0).all())
    assert torch.equal(out['alt_ids'][..., 0][live], out['gen_ids'][:, 1:][live])
    assert torch.equal(out['alt_log_probs'][..., 0][live].view(torch.int32), out['log_probs'][live].view(torch.int32))
    assert torch.equal(out['token_model_lp'][live].view(torch.int32), out['log_probs'][live].view(torch.int32))
    assert bool((out['token_entropy'][live] > 0).all()) and bool((out['alt_log_probs'][live][:, :-1] >=
                                                                  out['alt_log_probs'][live][:, 1:]).all())
    hs = [h for sig, h in plain.__dict__['_decode_graphs'].items() if ('stats', 4) in sig]
    assert hs and all(h['graph'] not in (None, False) for h in hs), [h.get('error') for h in hs]
    assert any(h.get(('multi', 8)) for h in hs), [h.get('multi_error') for h in hs]


def test_captured_run_equals_the_launch_by_launch_run_and_replays_issue_nothing(models, monkeypatch):
    """The same path - static buffers, device counter, in-step bookkeeping - once replayed from the captured graphs and once
    issued launch by launch (the stepper's own fall-back when a capture is refused: h['graph'] = False)."""
    from tell_amd import graphs
    from tell_amd.models import stepper
    plain, _, batch = models
    with torch.no_grad():
        plain.generate(**_clone(batch), token_stats=4)        # captured by now
        with _Spy() as spy:
            cap = plain.generate(**_clone(batch), token_stats=4)
        torch.cuda.synchronize()
        step_calls = {'tell_adaptive_logprob_stats', 'tell_adaptive_logprob_argmax', 'tell_greedy_update', 'tell_embed_gather_step'}
        assert not step_calls & set(spy.names), sorted(step_calls & set(spy.names))

        class NoCapture:
            def __getattr__(self, k):
                return getattr(graphs, k)

            def capture(self, *a, **k):
                raise RuntimeError('captures are off in this test')
        monkeypatch.setattr(stepper, 'graphs', NoCapture())
        plain.reset_graphs()
        with _Spy() as eager_spy:
            eag = plain.generate(**_clone(batch), token_stats=4)
        torch.cuda.synchronize()
        hs = [h for sig, h in plain.__dict__['_decode_graphs'].items() if ('stats', 4) in sig]
        assert hs and all(h['graph'] is False for h in hs)
        monkeypatch.undo()
        plain.reset_graphs()
    steps = cap['gen_ids'].shape[1] - 1
    assert eager_spy.names.count('tell_adaptive_logprob_stats') >= steps
    assert torch.equal(cap['gen_ids'], eag['gen_ids']) and torch.equal(cap['log_probs'], eag['log_probs'])
    for k in KEYS:
        assert torch.equal(cap[k].view(torch.int32) if cap[k].dtype == torch.float32 else cap[k],
                           eag[k].view(torch.int32) if eag[k].dtype == torch.float32 else eag[k]), k


def test_token_stats_zero_issues_the_launch_list_of_before(models):
    plain, _, batch = models
    with torch.no_grad():
        plain.generate(**_clone(batch))                       # (working weights cached first)
        plain.reset_graphs()
        with _Spy() as sa:
            a = plain.generate(**_clone(batch))
        keys_a = list(plain.__dict__['_decode_graphs'])
        plain.reset_graphs()
        with _Spy() as sz:
            z = plain.generate(**_clone(batch), token_stats=0)
        torch.cuda.synchronize()
        assert list(plain.__dict__['_decode_graphs']) == keys_a and not any(isinstance(x, tuple) and x[:1] == ('stats',)
                                                                              for s_ in keys_a for x in s_)
        assert sa.names == sz.names and len(sa.names) > 50 and 'tell_adaptive_logprob_stats' not in sz.names
        assert torch.equal(a['gen_ids'], z['gen_ids']) and torch.equal(a['log_probs'], z['log_probs']) and set(a) == set(z)
        with _Spy() as s4:
            plain.generate(**_clone(batch), token_stats=4)
        assert 'tell_adaptive_logprob_stats' in s4.names      # (the warm step and the capture issue it)


@pytest.mark.parametrize('mode', ['topk', 'nucleus'])
def test_sampling_reports_the_models_own_distribution(models, mode):
    _, variant, batch = models
    T = 0.7
    model = variant(sampling_topk=8, sampling_temp=T) if mode == 'topk' else \
        variant(sampling_topk=0, sampling_temp=T, sampling_topp=0.9)
    with torch.no_grad():
        torch.manual_seed(5)
        base = model.generate(**_clone(batch))
        torch.manual_seed(5)
        out = model.generate(**_clone(batch), token_stats=8)
        torch.cuda.synchronize()
    assert torch.equal(out['gen_ids'], base['gen_ids']) and torch.equal(out['log_probs'], base['log_probs'])
    live = _check_neutral_behind_eos(out).to(DEV)
    rank, mlp, alt, alp = out['token_rank'], out['token_model_lp'], out['alt_ids'], out['alt_log_probs']
    assert bool((rank[live] >= 0).all()) and int((rank[live] > 0).sum()) > 0       # sampled: not always the arg-max
    # 'log_probs' carries the temperature (lp / T), token_model_lp does not
    assert torch.allclose(mlp[live] / T, out['log_probs'][live], rtol=1e-6, atol=1e-6)
    tok = out['gen_ids'][:, 1:]
    inside = live & (rank < 8)
    idx = rank.clamp(min=0, max=7).unsqueeze(-1)
    assert torch.equal(alt.gather(2, idx).squeeze(-1)[inside], tok[inside])
    assert torch.equal(alp.gather(2, idx).squeeze(-1)[inside].view(torch.int32), mlp[inside].view(torch.int32))
    outside = live & (rank >= 8)
    assert not bool(((alt == tok.unsqueeze(-1)).any(-1) & outside).any())
    if mode == 'topk':
        assert bool((rank[live] < 8).all())                   # a top-8 draw is one of the 8 alternatives


def _invariants(out, n):
    """the two rank invariants on the live steps of a generation; -> the live mask"""
    live = _check_neutral_behind_eos(out).to(DEV)
    rank, tok = out['token_rank'], out['gen_ids'][:, 1:]
    assert bool((rank[live] >= 0).all())
    inside = live & (rank < n)
    idx = rank.clamp(min=0, max=n - 1).unsqueeze(-1)
    assert torch.equal(out['alt_ids'].gather(2, idx).squeeze(-1)[inside], tok[inside])
    assert torch.equal(out['alt_log_probs'].gather(2, idx).squeeze(-1)[inside].view(torch.int32),
                       out['token_model_lp'][inside].view(torch.int32))
    assert not bool(((out['alt_ids'] == tok.unsqueeze(-1)).any(-1) & live & (rank >= n)).any())
    return live


@pytest.mark.parametrize('combo', ['ban', 'pen', 'mask', 'attention', 'prefix'])
def test_token_stats_combines_with_the_other_options(models, combo):
    """Bans, penalties, a vocabulary mask, attention maps and a forced prefix: tokens and log-probs are those of the run without
    statistics, the statistics are the model's own distribution (the invariants hold; a banned / penalised / masked / forced
    step may take a token that is not the arg-max)."""
    plain, variant, batch = models
    kw = {}
    if combo == 'ban':
        model = variant(no_repeat_ngram_size=2, min_len=6)
    elif combo == 'pen':
        model = variant(repetition_penalty=1.5, presence_penalty=0.5)
    elif combo == 'mask':
        model = variant(suppress_tokens=list(range(900, 1400)) + list(range(2500, 5000)))
    else:
        model = plain
    with torch.no_grad():
        if combo == 'attention':
            kw = {'attention': True}
        if combo == 'prefix':
            kw = {'prefix': torch.randint(3, 50265, (8, 5), generator=torch.Generator().manual_seed(3)).to(DEV)}
        base = model.generate(**_clone(batch), **kw)
        out = model.generate(**_clone(batch), **kw, token_stats=4)
        torch.cuda.synchronize()
    assert torch.equal(out['gen_ids'], base['gen_ids']) and torch.equal(out['log_probs'], base['log_probs'])
    live = _invariants(out, 4)
    moved = int((out['token_rank'][live] > 0).sum())
    print('%s: %d live steps, %d of them took a token that is not the model\'s arg-max' % (combo, int(live.sum()), moved))
    if combo in ('ban', 'pen', 'mask', 'prefix'):
        assert moved > 0
    if combo == 'attention':
        assert moved == 0 and set(out['attns']) == set(base['attns']) and torch.equal(out['attn_steps'], base['attn_steps'])
        assert all(torch.equal(out['attns'][k], base['attns'][k]) for k in base['attns'])
    if combo == 'prefix':                                     # forced steps report the model's log-prob of the forced token
        assert torch.equal(out['token_model_lp'][:, :5].view(torch.int32), out['log_probs'][:, :5].view(torch.int32))
    if combo != 'pen':                                        # (under penalties 'log_probs' holds scores, not log-probs)
        assert torch.equal(out['token_model_lp'][live].view(torch.int32), out['log_probs'][live].view(torch.int32))


def test_n_samples_forms_are_the_gather_by_sample_index(models):
    _, variant, batch = models
    model = variant(sampling_topk=8, sampling_temp=0.9)
    with torch.no_grad():
        torch.manual_seed(7)
        out = model.generate(**_clone(batch), n_samples=2, rank_by='draw', token_stats=4)
        torch.manual_seed(7)
        ranked = model.generate(**_clone(batch), n_samples=2, rank_by='score', token_stats=4)
        torch.cuda.synchronize()
    order = ranked['sample_index']
    assert out['sample_index'].tolist() == [[0, 1]] * order.shape[0]
    for k in KEYS:
        d, r = out[k + '_samples'], ranked[k + '_samples']
        assert d.shape[:3] == (order.shape[0], 2, ranked['gen_ids'].shape[1] - 1), (k, d.shape)
        want = d.gather(1, order.view(-1, 2, *([1] * (d.dim() - 2))).expand_as(d))
        assert torch.equal(r, want), k
        assert torch.equal(ranked[k], r[:, 0]), k
    tok = ranked['gen_ids_samples'][:, :, 1:]
    live = ranked['token_rank_samples'] >= 0
    assert torch.equal(ranked['alt_ids_samples'].gather(3, ranked['token_rank_samples'].clamp(0, 3).unsqueeze(-1)).squeeze(-1)[
        live & (ranked['token_rank_samples'] < 4)], tok[live & (ranked['token_rank_samples'] < 4)])


def test_score_captions_token_stats_against_the_teacher_forced_forward_fp32():
    """The small fp32 model of tests/token_stats_ref.py: score_captions(token_stats=4) - the cached step, forced - against the
    layer-by-layer teacher-forced forward with full log-probs: token_model_lp and entropy within rtol 1e-4 / atol 5e-4, every
    rank inside the interval the reference admits at that tolerance (single-valued for >= 90 % of the tokens: host test)."""
    import tell_amd
    from tell_amd.data import synthetic_batch
    tell_amd.set_compute_dtype(torch.float32)
    model = R.score_model().to(DEV)
    batch = synthetic_batch(**R.SCORE_BATCH, device=DEV)
    cap = batch['caption']['roberta'].clone()
    with torch.no_grad():
        sc = model.score_captions(_clone(batch), token_stats=4)
        base = model.score_captions(_clone(batch))
        b2 = _clone(batch)
        _, _, contexts = model._forward(b2['context'], b2['image'], b2['caption'], b2.get('face_embeds'), b2.get('obj_embeds'))
        dec = model.decoder(b2['caption'], contexts)
        full = model.decoder.adaptive_softmax.get_log_prob(dec[0]).double().cpu().numpy()       # [B, T - 1, V]
        torch.cuda.synchronize()
    assert torch.equal(sc['log_probs'], base['log_probs']) and torch.equal(sc['prefix_len'], base['prefix_len'])
    T1 = cap.shape[1] - 1
    plen = sc['prefix_len'].cpu().tolist()
    rank, mlp, ent, alt = (sc[k].cpu().numpy() for k in ('token_rank', 'token_model_lp', 'token_entropy', 'alt_ids'))
    assert rank.shape == (cap.shape[0], T1) and alt.shape == (cap.shape[0], T1, 4)
    checked = single = 0
    for b in range(cap.shape[0]):
        for t in range(T1):
            if t >= plen[b]:
                assert rank[b, t] == -1 and mlp[b, t] == 0 and ent[b, t] == 0 and (alt[b, t] == PAD).all()
                continue
            c = int(cap[b, t + 1])
            lp = full[b, t]
            assert abs(mlp[b, t] - lp[c]) <= R.SCORE_ATOL + R.SCORE_RTOL * abs(lp[c]), (b, t, mlp[b, t], lp[c])
            assert mlp[b, t] == sc['log_probs'][b, t].item()
            H = float(-(np.exp(lp) * lp).sum())
            assert abs(ent[b, t] - H) <= R.SCORE_ATOL + R.SCORE_RTOL * abs(H), (b, t, ent[b, t], H)
            lo, hi = R.rank_interval(lp, c)
            assert lo <= rank[b, t] <= hi, (b, t, rank[b, t], lo, hi)
            single += lo == hi
            checked += 1
    print('score_captions fp32: %d tokens, rank interval single-valued for %d' % (checked, single))
    assert checked == sum(plen) and checked >= 30
