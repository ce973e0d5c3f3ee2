"""Attention maps from cached generation: tell_attn_decode_weights through the C ABI - output
untouched, the definition against an fp64 restatement with tell_attn_avg_weights as the yardstick, order-freedom, slots -
and model.generate(attention=True) against the oracle's `attns`, the layer-by-layer need_attn path and attention=False."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H, E = 16, 1024
SHAPES = {'image': (49, 2048), 'article': (512, 1024), 'faces': (4, 512), 'obj': (64, 2048)}


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    yield
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ C ABI
def _case(B, S_list, head_major, masks, seed):
    """One launch's worth of inputs.  masks[i]: None | 'ragged' | 'full' (every cached key of every row masked)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    bf = dict(dtype=torch.bfloat16, device=DEV)
    c = dict(B=B, S=list(S_list), q=[], k=[], v=[], mask=[], bk=[], bv=[])
    for S, mk in zip(S_list, masks):
        c['q'].append((torch.randn(B, E, generator=g, device=DEV) * 0.35).to(torch.bfloat16))
        if head_major and S > 0:
            k = torch.randn(B, H, S, 64, generator=g, device=DEV).to(torch.bfloat16).permute(2, 0, 1, 3)    # [S, B, H, 64] view
            v = torch.randn(B, H, S, 64, generator=g, device=DEV).to(torch.bfloat16).permute(2, 0, 1, 3)
        else:
            k = torch.randn(S, B, E, generator=g, device=DEV).to(torch.bfloat16)
            v = torch.randn(S, B, E, generator=g, device=DEV).to(torch.bfloat16)
        c['k'].append(k)
        c['v'].append(v)
        if mk is None or S == 0:
            c['mask'].append(None)
        elif mk == 'full':
            c['mask'].append(torch.ones(B, S, dtype=torch.uint8, device=DEV))
        else:
            lens = torch.randint(0, S + 1, (B,), generator=g, device=DEV)
            c['mask'].append((torch.arange(S, device=DEV)[None, :] >= lens[:, None]).to(torch.uint8).contiguous())
        c['bk'].append((torch.randn(E, generator=g, device=DEV) * 0.5).to(torch.bfloat16))
        c['bv'].append((torch.randn(E, generator=g, device=DEV) * 0.5).to(torch.bfloat16))
    return c


def _common(c, out):
    from tell_amd.decode import _ints, _longs, _ptrs
    n = len(c['S'])
    ks, vs, k_ss, k_sb, k_sh, v_ss, v_sb, v_sh = [], [], [], [], [], [], [], []
    for i in range(n):
        k, v = c['k'][i], c['v'][i]
        if c['S'][i] == 0:
            ks.append(c['q'][i]); vs.append(c['q'][i])
            for lst, val in ((k_ss, 0), (k_sb, 0), (v_ss, 0), (v_sb, 0), (k_sh, 64), (v_sh, 64)):
                lst.append(val)
            continue
        ks.append(k); vs.append(v)
        k_ss.append(k.stride(0)); k_sb.append(k.stride(1)); v_ss.append(v.stride(0)); v_sb.append(v.stride(1))
        k_sh.append(k.stride(2) if k.dim() == 4 else 64); v_sh.append(v.stride(2) if v.dim() == 4 else 64)
    return (n, _ptrs(c['q']), _longs([E] * n), _ptrs(ks), _longs(k_ss), _longs(k_sb), _longs(k_sh), _ptrs(vs), _longs(v_ss),
            _longs(v_sb), _longs(v_sh), _ptrs(c['mask']), _ptrs(c['bk']), _ptrs(c['bv']), 1, _ints(c['S']),
            _ptrs([out[i] for i in range(n)]), _longs([E] * n), c['B'], H, 1)


def _plain(c):
    from tell_amd.hip import call
    out = torch.zeros(len(c['S']), c['B'], E, dtype=torch.bfloat16, device=DEV)
    call('tell_attn_decode', *_common(c, out))
    return out


def _export(c, slot=0, n_slots=1, step_dev=None, w=None, fill=float('nan')):
    from tell_amd.decode import _longs, _ptrs
    from tell_amd.hip import call
    n, B = len(c['S']), c['B']
    out = torch.zeros(n, B, E, dtype=torch.bfloat16, device=DEV)
    if w is None:
        w = [torch.full((n_slots, B, S + 2), fill, dtype=torch.float32, device=DEV) for S in c['S']]
    lse = torch.empty(n, B, H, dtype=torch.float32, device=DEV)
    call('tell_attn_decode_weights', *_common(c, out), lse, _ptrs(w), _longs([x.stride(0) for x in w]),
         _longs([x.stride(1) for x in w]), int(slot), int(n_slots), step_dev)
    return out, w


def _fp64(c, i):
    """softmax per head over the S + 2 keys (cached | bias_k | zero), mean over the heads -> ([B, S + 2], natural lse [B, H])."""
    S, B = c['S'][i], c['B']
    q = c['q'][i].double().view(B, H, 64)
    cols = []
    if S:
        k = c['k'][i].double().reshape(S, B, H, 64)
        sc = torch.einsum('bhd,sbhd->bhs', q, k)
        if c['mask'][i] is not None:
            sc = sc.masked_fill(c['mask'][i].bool()[:, None, :], float('-inf'))
        cols.append(sc)
    cols.append(torch.einsum('bhd,hd->bh', q, c['bk'][i].double().view(H, 64))[..., None])
    cols.append(torch.zeros(B, H, 1, dtype=torch.float64, device=DEV))
    sc = torch.cat(cols, -1)
    return torch.softmax(sc, -1).mean(1), torch.logsumexp(sc, -1)


CASES = [((0, 4, 49, 77), (None, 'ragged', 'full', None)), ((512, 2048, 4, 49), ('ragged', None, 'full', 'ragged')),
         ((2048,), ('ragged',)), ((77, 512), ('full', None))]


@pytest.mark.parametrize('head_major', [False, True])
@pytest.mark.parametrize('B', [1, 32, 128])
def test_export_leaves_the_attention_output_untouched(B, head_major):
    for n_case, (S_list, masks) in enumerate(CASES):
        c = _case(B, S_list, head_major, masks, seed=100 + n_case)
        want = _plain(c)
        got, _ = _export(c)
        assert torch.equal(got, want), (B, head_major, S_list)


@pytest.mark.parametrize('head_major', [False, True])
@pytest.mark.parametrize('B', [1, 32, 128])
def test_weights_match_the_fp64_definition_within_twice_the_avg_weights_kernel(B, head_major):
    """Bound: 2 x the maximum absolute error of tell_attn_avg_weights (given the fp32 natural-log lse of the fp64
    restatement, row-major K) against the fp64 values, + 1e-7.  Measured on MI355X: over these cases the
    yardstick errs by 1.2e-8 .. 1.2e-7 and the exporting kernel by 4.2e-9 .. 1.6e-7 (66 (case, context) pairs; worst: 1.55e-7
    against the yardstick's 1.17e-7; never more than 1.64 x the yardstick)."""
    from tell_amd.hip import BF16, call
    for n_case, (S_list, masks) in enumerate(CASES):
        c = _case(B, S_list, head_major, masks, seed=200 + n_case)
        _, w = _export(c)
        for i, S in enumerate(S_list):
            ref, lse = _fp64(c, i)
            got = w[i][0]
            krow = c['k'][i].reshape(S, B, E).contiguous() if S else c['q'][i]
            yard = torch.empty(B, 1, S + 2, dtype=torch.float32, device=DEV)
            call('tell_attn_avg_weights', c['q'][i], krow, lse.float().contiguous(), c['mask'][i], c['bk'][i], yard, B, H, 1, S,
                 64, 0, E, B * E if S else 0, E if S else 0, 1, BF16)
            e_yard = (yard[:, 0].double() - ref).abs().max().item()
            e_new = (got.double() - ref).abs().max().item()
            print('\nB %d head-major %d S %d mask %s: avg_weights err %.3e, exporting kernel err %.3e'
                  % (B, head_major, S, masks[i], e_yard, e_new))
            assert e_new <= 2 * e_yard + 1e-7, (B, head_major, S, e_new, e_yard)
            assert not torch.isnan(got).any()
            assert (got.sum(-1) - 1).abs().max().item() <= 1e-4
            if c['mask'][i] is not None:
                assert (got[:, :S][c['mask'][i].bool()] == 0.0).all()
            if masks[i] == 'full' and S:
                assert (got[:, :S] == 0.0).all() and (got[:, S:].sum(-1) - 1).abs().max().item() <= 1e-4


@pytest.mark.parametrize('head_major', [False, True])
def test_weights_do_not_depend_on_batch_launch_mode_or_run(head_major):
    S_list, masks = (512, 49, 4, 64), ('ragged', None, 'ragged', 'ragged')
    big = _case(128, S_list, head_major, masks, seed=7)
    rows = slice(40, 72)
    small = dict(B=32, S=list(S_list), q=[q[rows].contiguous() for q in big['q']], bk=big['bk'], bv=big['bv'],
                 mask=[None if m is None else m[rows].contiguous() for m in big['mask']],
                 k=[(k[:, rows].permute(1, 2, 0, 3).contiguous().permute(2, 0, 1, 3) if k.dim() == 4 else k[:, rows].contiguous())
                    for k in big['k']],
                 v=[(v[:, rows].permute(1, 2, 0, 3).contiguous().permute(2, 0, 1, 3) if v.dim() == 4 else v[:, rows].contiguous())
                    for v in big['v']])
    o_big, w_big = _export(big)
    o_small, w_small = _export(small)
    o_again, w_again = _export(small)
    # captured
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    w_cap = [torch.full((1, 32, S + 2), float('nan'), dtype=torch.float32, device=DEV) for S in S_list]
    _export(small, w=[torch.empty_like(x) for x in w_cap])             # (warm: nothing lazy inside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o_cap, _ = _export(small, slot=0, n_slots=1, step_dev=word, w=w_cap)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(o_small, o_big[:, rows]) and torch.equal(o_cap, o_small)
    for i in range(len(S_list)):
        assert torch.equal(w_small[i], w_big[i][:, rows])
        assert torch.equal(w_small[i], w_again[i])
        assert torch.equal(w_small[i], w_cap[i])


def test_captured_launch_fills_one_fresh_slot_per_replay_and_a_block_of_eight():
    S_list, masks = (77, 4), ('ragged', None)
    c = _case(8, S_list, True, masks, seed=11)
    _, want = _export(c)
    N = 20
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    w = [torch.full((N, 8, S + 2), float('nan'), dtype=torch.float32, device=DEV) for S in S_list]
    torch.cuda.synchronize()
    single, multi = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(single):                       # slot = 1 + word: the captured decode step (counter holds i - 1)
        _export(c, slot=1, n_slots=N, step_dev=word, w=w)
    with torch.cuda.graph(multi):                        # eight steps in one graph; the word moves between them on the device
        for _ in range(8):
            _export(c, slot=1, n_slots=N, step_dev=word, w=w)
            word.add_(1)
    for i in range(1, 10):                               # steps 1 .. 9
        word.fill_(i - 1)
        single.replay()
    torch.cuda.synchronize()
    for i, x in enumerate(w):
        assert torch.isnan(x[0]).all() and torch.isnan(x[10:]).all()
        for s in range(1, 10):
            assert torch.equal(x[s], want[i][0]), s
    word.fill_(9)                                        # steps 10 .. 17 as one replay
    multi.replay()
    torch.cuda.synchronize()
    for i, x in enumerate(w):
        assert torch.isnan(x[0]).all() and torch.isnan(x[18:]).all()
        for s in range(1, 18):
            assert torch.equal(x[s], want[i][0]), s
    # a slot outside the buffer is skipped on the device, refused on the host
    word.fill_(N + 5)
    single.replay()
    torch.cuda.synchronize()
    assert torch.isnan(w[0][18:]).all()
    with pytest.raises(RuntimeError):
        _export(c, slot=N, n_slots=N, w=w)


def test_beams_above_one_are_refused():
    from tell_amd.decode import _longs, _ptrs
    from tell_amd.hip import call
    c = _case(4, (4,), False, (None,), seed=3)
    c['B'] = 8
    c['q'] = [c['q'][0].repeat_interleave(2, 0).contiguous()]
    out = torch.zeros(1, 8, E, dtype=torch.bfloat16, device=DEV)
    args = list(_common(c, out))
    args[-1] = 2
    w = [torch.zeros(1, 8, 6, dtype=torch.float32, device=DEV)]
    with pytest.raises(RuntimeError):
        call('tell_attn_decode_weights', *args, torch.empty(1, 8, H, dtype=torch.float32, device=DEV), _ptrs(w), _longs([48]),
             _longs([6]), 0, 1, None)


# ------------------------------------------------------------------------------------------------ model level
def _no_dropout(m):
    for mod in m.modules():
        for a in ('dropout', 'input_dropout', 'relu_dropout', 'weight_dropout', 'attention_dropout'):
            if isinstance(getattr(mod, a, None), float):
                setattr(mod, a, 0.0)


def _inputs_batch(batch, seed):
    g = torch.Generator().manual_seed(seed)
    ctx = {}
    for n in ('image', 'article', 'faces', 'obj'):
        S, C = SHAPES[n]
        x = torch.randn(S, batch, C, generator=g) * 0.5
        if n in ('image', 'obj'):
            x = x.abs()
        lens = torch.randint(max(S // 2, 1), S + 1, (batch,), generator=g)
        if n == 'image':
            lens = torch.full((batch,), S)
        if n == 'faces':
            lens = torch.randint(0, S + 1, (batch,), generator=g)
            lens[0] = 0
        mask = torch.arange(S)[None, :] >= lens[:, None]
        ctx[n], ctx[n + '_mask'] = x * (~mask).t()[:, :, None], mask
    return ctx, torch.zeros(batch, 1, dtype=torch.long)


def _to_dev(ctx, dtype):
    return {k: (v.to(DEV) if v.dtype == torch.bool else v.to(DEV, dtype)) for k, v in ctx.items()}


def _sharpened_eos(sd, factor):
    sd = {k: v.clone() for k, v in sd.items()}
    done = set()
    for k, v in sd.items():
        if (k.endswith('adaptive_softmax.head.word_proj.weight') or k.endswith('embed_tokens.embeddings.0.weight') or
                k.endswith('embedders.adaptive.embeddings.0.weight')) and v.data_ptr() not in done:
            v[2] *= factor
            v[1] = 0.0
            done.add(v.data_ptr())
    return sd


_SD = {}


def _weights():
    if 'sd' not in _SD:
        from tell_amd.build import build_decoder
        torch.manual_seed(0)
        _SD['sd'] = {k: v.clone() for k, v in build_decoder('faces_objects').state_dict().items()}
    return _SD['sd']


def _shell(dec, topk=1, topp=None):
    from tell_amd.models.transformer import CaptionModel
    m = CaptionModel.__new__(CaptionModel)
    torch.nn.Module.__init__(m)
    m.decoder, m.padding_idx, m.index, m.sampling_topk, m.sampling_temp, m.sampling_topp = dec, 1, 'roberta', topk, 1.0, topp
    m.training = False
    return m


def _hip_decoder(sd, dtype):
    import tell_amd
    from tell_amd.build import build_decoder
    tell_amd.set_compute_dtype(dtype)
    dec = build_decoder('faces_objects')
    dec.load_state_dict(sd)
    return dec.to(DEV).eval()


def test_fp32_cached_generator_maps_match_the_oracle_generate():
    """oracle/models.py::_generate drops finished rows from its batch: step i's `attns` rows are the rows alive at step i."""
    from oracle.build import build_decoder as obuild
    from oracle.models import CaptionModel as OModel
    BB, GEN = 8, 10
    sd = _sharpened_eos(_weights(), 12.0)
    ref = obuild('faces_objects').eval()
    ref.load_state_dict({k: v for k, v in sd.items() if k in ref.state_dict()}, strict=False)
    om = OModel.__new__(OModel)
    torch.nn.Module.__init__(om)
    om.decoder, om.padding_idx, om.index, om.sampling_topk, om.sampling_temp = ref, 1, 'roberta', 1, 1.0
    ctx, start = _inputs_batch(BB, seed=41)
    m = _shell(_hip_decoder(sd, torch.float32))
    torch.set_num_threads(min(32, torch.get_num_threads()))
    with torch.no_grad():
        _, want_ids, want_attns = om._generate(start, {k: v.clone() for k, v in ctx.items()}, gen_len=GEN, eos=2)
        _, got_ids, (maps, steps) = m._generate(start.to(DEV), _to_dev(ctx, torch.float32), gen_len=GEN, eos=2, attention=True)
    n = min(got_ids.shape[1], want_ids.shape[1])
    assert torch.equal(got_ids.cpu()[:, :n], want_ids[:, :n])
    assert set(maps) == {'image', 'article', 'faces', 'obj'}
    for name, t in maps.items():
        assert t.shape == (BB, got_ids.shape[1] - 1, len(ref.layers), SHAPES[name][0] + 2) and t.dtype == torch.float32
    alive = torch.ones(BB, dtype=torch.bool)
    checked = 0
    for i in range(min(len(want_attns), maps['image'].shape[1])):
        rows = alive.nonzero().squeeze(1)
        for li, layer_attn in enumerate(want_attns[i]):
            for name, w in layer_attn.items():
                w = torch.as_tensor(w).float()                                 # [alive, 1, S + 2]
                assert w.shape[0] == rows.numel()
                torch.testing.assert_close(maps[name][rows, i, li].cpu(), w[:, 0], rtol=1e-3, atol=2e-5)
                checked += 1
        alive = alive & (want_ids[:, i + 1] != 2)
        assert (steps.cpu()[~alive] <= i + 1).all()
    assert checked >= 4 * 4 * 3


def test_bf16_fused_step_maps_match_fp32_and_the_layer_by_layer_need_attn_path():
    """Teacher-forced for 8 steps: the fused captured-step kernels' maps against the fp32 maps (bf16 rule 5e-2 in norm) and
    at most 1.25 x the error of the bf16 layer-by-layer need_attn path + 1e-3 (the rule of the fused-step test)."""
    from tell_amd import decode
    from tell_amd.data.synthetic import _ids
    BB, STEPS = 4, 8
    sd = _weights()
    ctx, _ = _inputs_batch(BB, seed=5)
    g = torch.Generator().manual_seed(9)
    seq = _ids(g, BB, STEPS, torch.full((BB,), STEPS), 50265, (5000, 20000)).to(DEV)
    names = ('image', 'article', 'faces', 'obj')

    def legacy(dec, dctx, dtype):
        """The need_attn path (per-context attention + tell_attn_avg_weights, numpy per step) -> {name: [B, STEPS, L, S + 2]}."""
        for layer in dec.layers:
            layer.need_attn = True
        st, per = {}, []
        kv = dec.project_contexts(dctx)
        for i in range(STEPS):
            a = dec({'roberta': seq[:, i:i + 1]}, dctx, incremental_state=st, kv_cache=kv)[1]['attn']
            per.append(a)
        for layer in dec.layers:
            layer.need_attn = False
        return {n: torch.stack([torch.stack([torch.from_numpy(per[i][li][n])[:, 0] for li in range(len(dec.layers))], 1)
                                for i in range(STEPS)], 1) for n in names}

    with torch.no_grad():
        dec32 = _hip_decoder(sd, torch.float32)
        want = legacy(dec32, _to_dev(ctx, torch.float32), torch.float32)
        del dec32
        dec = _hip_decoder(sd, torch.bfloat16)
        dctx = _to_dev(ctx, torch.bfloat16)
        plain = legacy(dec, dctx, torch.bfloat16)
        kv = dec.project_contexts(dctx)
        state = dec.static_incremental_state(BB, DEV, torch.bfloat16)
        assert decode.usable(dec, torch.empty(1, BB, 1024, dtype=torch.bfloat16, device=DEV), state, kv)
        sink = decode.AttnSink([{n: torch.full((STEPS, BB, SHAPES[n][0] + 2), float('nan'), dtype=torch.float32, device=DEV)
                                 for n in names} for _ in dec.layers], STEPS)
        for i in range(STEPS):
            dec({'roberta': seq[:, i:i + 1]}, dctx, incremental_state=state, kv_cache=kv, attn_sink=sink.at(i))
        fused = {n: torch.stack([lb[n] for lb in sink.bufs], 0).permute(2, 1, 0, 3).cpu() for n in names}

    def rel(a, b):
        return (a.float() - b.float()).norm().item() / (b.float().norm().item() + 1e-30)
    for n in names:
        e_fused, e_plain = rel(fused[n], want[n]), rel(plain[n], want[n])
        print('\nmaps %s: fused bf16 vs fp32 %.3e, layer-by-layer bf16 vs fp32 %.3e' % (n, e_fused, e_plain))
        assert not torch.isnan(fused[n]).any()
        assert e_fused < 5e-2 and e_fused <= 1.25 * e_plain + 1e-3, (n, e_fused, e_plain)


@pytest.mark.parametrize('mode', ['greedy', 'topk', 'topp'])
def test_tokens_are_bit_identical_with_and_without_maps_and_every_graph_lands_in_its_slot(mode):
    """gen_len = 24 with rows that stay alive to the cap: step 0 is the eager warm step, steps 1..7 replay the single-step
    capture, steps 8..15 and 16..23 are one replay each of the stepper's `step.multi` graph of 8.  The stepper's own static
    buffers are poisoned with NaN before the run that is compared, slot by slot, with eager teacher-forced steps."""
    BB, GEN = 8, 24
    sd = _sharpened_eos(_weights(), 12.0)         # (some rows end early, most run to the cap)
    dec = _hip_decoder(sd, torch.bfloat16)
    m = _shell(dec, topk=20 if mode == 'topk' else (0 if mode == 'topp' else 1), topp=0.9 if mode == 'topp' else None)
    ctx, start = _inputs_batch(BB, seed=21)
    dctx, dstart = _to_dev(ctx, torch.bfloat16), start.to(DEV)
    torch.manual_seed(5)
    lp0, ids0, at0 = m._generate(dstart, dctx, gen_len=GEN, eos=2)
    keys_off = set(m.__dict__['_decode_graphs'])
    torch.manual_seed(5)
    lp1, ids1, (maps1, steps1) = m._generate(dstart, dctx, gen_len=GEN, eos=2, attention=True)   # (outside no_grad on purpose)
    entries = [h for k, h in m.__dict__['_decode_graphs'].items() if ('attn',) in k]
    assert len(entries) == 1
    h = entries[0]
    for lb in h['attn'].bufs:                     # poison the stepper's static sinks: every slot below must be re-written
        for t in lb.values():
            assert not t.requires_grad and t.grad_fn is None
            t.fill_(float('nan'))
    torch.manual_seed(5)
    lp, ids, (maps, steps) = m._generate(dstart, dctx, gen_len=GEN, eos=2, attention=True)
    assert at0 == []
    assert not any(('attn',) in k for k in keys_off)                       # the plain captures are keyed as before
    assert keys_off <= set(m.__dict__['_decode_graphs'])
    assert torch.equal(ids0, ids) and torch.equal(lp0, lp) and torch.equal(ids1, ids)
    assert all(torch.equal(maps[n], maps1[n]) for n in maps) and torch.equal(steps, steps1)
    n_steps = ids.shape[1] - 1
    assert n_steps == GEN, n_steps                                        # rows alive past step 16: both blocks of 8 ran
    # the run went through the real graphs of the stepper: the single-step capture and step.multi's graph of 8
    assert isinstance(h.get('graph'), torch.cuda.CUDAGraph) and h.get('graph_has_post'), h.get('error')
    assert isinstance(h.get(('multi', 8)), torch.cuda.CUDAGraph), h.get('multi_error')
    for n, t in maps.items():
        assert t.shape == (BB, n_steps, 4, SHAPES[n][0] + 2) and t.is_cuda and not t.requires_grad
        assert not torch.isnan(t).any(), n
        assert (t.sum(-1) - 1).abs().max().item() <= 1e-4
        mk = dctx[n + '_mask'].bool()
        assert (t.permute(0, 3, 1, 2)[:, :SHAPES[n][0]][mk] == 0).all()
    ended = (ids == 2).any(1).cpu()
    first = (ids == 2).float().argmax(1).cpu()
    assert (~ended).any()
    assert (steps.cpu()[ended] == first[ended]).all() and (steps.cpu()[~ended] == n_steps).all()
    # the maps of the warm step, the captured step and the multi-step graph are those of eager teacher-forced steps on the
    # same tokens, slot by slot
    from tell_amd import decode
    with torch.no_grad():
        kv = dec.project_contexts(dctx)
        state = dec.static_incremental_state(BB, DEV, torch.bfloat16)
        sink = decode.AttnSink([{n: torch.zeros(n_steps, BB, SHAPES[n][0] + 2, dtype=torch.float32, device=DEV) for n in maps}
                                for _ in dec.layers], n_steps)
        for i in range(n_steps):
            dec({'roberta': ids[:, i:i + 1].contiguous()}, dctx, incremental_state=state, kv_cache=kv, attn_sink=sink.at(i))
    alive = torch.ones(BB, dtype=torch.bool, device=DEV)
    for i in range(n_steps):
        assert alive.any()
        for li in range(4):
            for n in maps:                                # (a finished row is fed pad by the generator: compared while alive)
                assert torch.equal(maps[n][alive, i, li], sink.bufs[li][n][i][alive]), (n, i, li)
        alive = alive & (ids[:, i + 1] != 2)


def test_generate_lanes_with_maps_equals_generate_batch_by_batch(monkeypatch):
    from tell_amd.models.transformer import CaptionModel
    BB = 4
    dec = _hip_decoder(_sharpened_eos(_weights(), 12.0), torch.bfloat16)
    m = _shell(dec)
    m.fast_generation = True
    cases = [_inputs_batch(BB, seed=60 + i) for i in range(3)]

    def fake_forward(self, context, image, caption, face_embeds=None, obj_embeds=None, encoded=None):
        ctx, start = cases[int(image)]
        return start.to(DEV), None, _to_dev(ctx, torch.bfloat16)
    monkeypatch.setattr(CaptionModel, '_forward', fake_forward)
    batches = [dict(context={}, image=i, caption={}) for i in range(3)]
    with torch.no_grad():
        single = [m.generate(**b, attention=True) for b in batches]
        laned = [o for _, o in m.generate_lanes(batches, lanes=2, attention=True)]
        off = [o for _, o in m.generate_lanes(batches, lanes=2)]
    for a, b, c in zip(single, laned, off):
        assert torch.equal(a['gen_ids'], b['gen_ids']) and torch.equal(a['log_probs'], b['log_probs'])
        assert torch.equal(a['attn_steps'], b['attn_steps'])
        assert set(a['attns']) == set(b['attns']) and all(torch.equal(a['attns'][n], b['attns'][n]) for n in a['attns'])
        assert torch.equal(a['gen_ids'], c['gen_ids']) and c['attns'] == [] and 'attn_steps' not in c
