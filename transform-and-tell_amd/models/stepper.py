"""One decode step of the cached caption generators (CaptionModel._greedy_steps / _beam_steps): eager, or captured once per
signature into a hipGraph and replayed.  The captured state lives in the model's cache (`_decode_graphs`: signature -> entry
dict); a DecodeStepper is a view over one entry plus the arguments of one caption batch."""
import os

import torch

from .. import decode, graphs, ops


def sub_table(alpha, beta, L):
    """The subtrahend table of the penalised pick kernels: fp32 [L + 1], sub[0] = 0, sub[c] = float32(float64(alpha) +
    float64(beta) * c) - built on the host like the length-penalty table (inv_norm_table)."""
    import numpy as np
    t = np.zeros(int(L) + 1, dtype=np.float32)
    t[1:] = (np.float64(alpha) + np.float64(beta) * np.arange(1, int(L) + 1, dtype=np.float64)).astype(np.float32)
    return torch.from_numpy(t)

# why generate(token_stats=n) / DecodeStepper(stats=n) is refused - one wording wherever two paths refuse the same thing
TOKEN_STATS_REFUSALS = {
    'beam': 'token_stats does not combine with beam search (beam_size > 1, n_best): the rows of a beam move between steps, '
            'per-hypothesis statistics would have to follow the ancestor table',
    'guide': 'token_stats does not combine with guidance: a guided step decodes paired rows and picks from a combined score, '
             'not from one row\'s distribution',
    'lanes': 'token_stats is not supported by generate_lanes / generate_stream (out of scope): use generate()',
    'copy': 'token_stats is not supported by the copy models (pointer, pointer_2): their step mixes a copy distribution into '
            'the pick',
    'lstm': 'token_stats is not supported by the LSTM baseline: it has no cached decode step',
}

# decode steps per graph replay once a generation loop is past its first all-finished test (DecodeStepper.multi)
MULTI_STEP_GRAPHS = os.environ.get('TELL_MULTI_STEP_GRAPHS', '1') != '0'


class DecodeStepper:
    """step(i, cur [B,1]) -> (token [B,1], log-prob [B,1]) - or, with topk=k, the k best (tokens [B,1,k],
    log-probs [B,1,k]) of every row - for the cached greedy / beam generators; step.reorder(rows) permutes the
    rows of the incremental state (beam search).

    With graphs enabled the decode step (about 150 launches of a few microseconds each, host-bound when issued
    one by one) is captured ONCE per (batch, context shapes) signature and replayed: every tensor it touches is
    static - the DynamicConv input buffers have their final K-1 rows from the start (zero history), the
    projected K/V and masks are copied into fixed buffers per caption batch, and the position offset comes from
    the graph's device step counter (embed_finalize reads it, like the dropout kernels).  `step.static` says which kind
    this is: True - a cache entry `step.h` with static buffers (step.cur, step.book, step.counter_out, step.back) that the
    captured graphs pin; False (graphs disabled, training, or K/V not on the device) - the same step issued launch by
    launch over the caller's tensors, no cache entry.

    sample = (k, T): every step draws from the top k at temperature T (AdaptiveSoftmax.sample) with the seed in the
    device word step.seed and the step index from the host (eager) or from the device counter (captured: every replay of
    the single-step and the multi-step graphs draws fresh numbers); (k, T) is part of the capture's signature.

    attention=True: the step also exports the head-averaged attention weights of every (layer, context) into static
    fp32 buffers [gen_len, B, S + 2] (decode.AttnSink, handed out as step.attn), slot = step index: from the host in an
    eager step, from the device counter in a captured one (single-step and multi-step graphs alike).  ('attn',) joins
    the signature only then: the captures without maps are keyed and recorded exactly as before.

    ban = (n, min_len, eos): the head's last launch becomes two - tell_decode_ban_list over the caller's histories
    (step.ban_source(hist [B, L] int64, finished [B] uint8): static buffers of the caller's book when the step is
    captured) with the step index from the host or from the device counter, then tell_adaptive_logprob_topk_banned (k = 1
    for the greedy decode).  opts: the caller's whole option tuple; it joins the signature when given (a captured
    bookkeeping launch differs with it), the default captures are keyed and recorded exactly as before.

    pen = (theta, alpha, beta) (repetition / presence / frequency penalties): the head's last launch
    becomes two - tell_decode_token_counts over the caller's histories (step.pen_source(hist, finished), like ban_source) with
    the step index from the host or from the device counter, then the pick over penalised scores:
    tell_adaptive_logprob_topk_penalised (k = 1 for the greedy decode) or, with sample = (k, T),
    tell_adaptive_logprob_sample_penalised.  The list buffers and the `sub` table live in the cache entry, next to the graphs
    that pin them.  ('penalty', theta, alpha, beta) joins the signature only when set; it does not combine with `ban`, with
    attention maps or with a truncation rule.

    prefix=True (caption completion): the stepper owns a forcing table - int64 [samples, gen_len] + int32 [samples], static,
    filled per caption batch by step.set_prefix(tokens, plen) - and every head ends in tell_adaptive_logprob_forced with the
    step index from the host or from the device counter.  ('prefix',) joins the signature: its own captured graph, one for
    every prefix width; without it nothing is allocated, launched or keyed differently.

    hyp = n > 1 (generate(n_samples=n); without topk): the B rows are n sampled hypotheses of each of
    B / n samples, row = sample * n + j, over contexts and K/V of width B / n - what beam search hands in with topk = K, but no
    row ever moves: the DynamicConv rings get no ancestor table, the forcing table has B / n rows (beams = n in the forced
    launch).  ('hyp', n) joins the signature only then.

    mask=True (vocabulary masks): the stepper owns one bitmap per sample - int32 [B / per_sample, words],
    static in the cache entry (h['vmask']), filled per caption batch by step.set_mask(ctx_ids, cls_bits, deny8, eos)
    (tell_decode_vocab_mask, outside the captured step) - and the head's pick becomes the masked one:
    tell_adaptive_logprob_topk_masked (k = 1 for the greedy decode; with `ban`, behind tell_decode_ban_list and with its list) or,
    with sample = (k, T), tell_adaptive_logprob_sample_masked.  ('mask',) joins the signature only when set; it does not combine
    with `pen`, with attention maps or with a truncation rule.

    guide = drop (context guidance; a tuple of context names): the B rows are B / 2 conditional rows and,
    B / 2 rows further down, their unconditional twins - contexts, K/V and masks of twice the images, the twins' dropped
    contexts fully masked (transformer.guided_batch) - and the head's pick is the guided one:
    tell_adaptive_logprob_topk_guided (k = 1 for the greedy decode) with pair_offset = B / 2, which writes the same candidates
    to both rows of a pair.  gamma lives in a device float of the cache entry (h['gamma'], step.set_guidance(gamma) per caption
    batch): the captured step reads it, so one graph serves every gamma.  ('guide', drop) joins the signature only when set;
    it combines with nothing but beam search and its length penalty.

    hidden=True (the copy models): the step hands out the decoder's last hidden row next to the pick -
    (token, log-prob, x [B, 1, E]) - so that the caller's `post` can run its own tail on it (entity attention, copy decision, then
    the bookkeeping launch); `post` is recorded into the captured single-step and multi-step graphs as ever, however many
    launches it issues.  ('hidden',) joins the signature only when set.

    stats = n in 1..8 (per-token statistics): the stepper owns a decode.StatsSink - static buffers
    [gen_len, B(, n)] in the cache entry, handed out as step.stats, slot = step index (from the host in an eager step, from
    the device counter in a captured one, as the attention sink) - and every head ends in tell_adaptive_logprob_stats, behind
    the pick and the forced pick.  step.stats_source(finished uint8 [B]) hands in the caller's finished flags (static ones of
    the caller's book when the step is captured), as ban_source does.  ('stats', n) joins the signature only when set; it
    combines with greedy, every sampling rule, ban, pen, mask, prefix, hyp and attention, and is refused for topk and guide."""

    def __init__(self, model, B, kv, contexts, gen_len, topk=0, lane=0, sample=None, attention=False, ban=None, opts=None,
                 prefix=False, pen=None, hyp=1, mask=False, guide=None, hidden=False, stats=0):
        self.hidden = bool(hidden)
        self.n_stats = int(stats)
        if self.n_stats:
            if not 1 <= self.n_stats <= 8:
                raise ValueError('stats: 1..8 alternatives per token, got %r' % (stats,))
            if topk:
                raise ValueError('topk: ' + TOKEN_STATS_REFUSALS['beam'])
            if guide is not None:
                raise ValueError('guide: ' + TOKEN_STATS_REFUSALS['guide'])
        if guide is not None:
            for on, what in ((sample is not None, 'sampling (sampling_topk / sampling_topp / sampling_minp / sampling_typical)'),
                             (ban is not None, 'no_repeat_ngram_size / min_len'),
                             (pen is not None, 'repetition_penalty / presence_penalty / frequency_penalty'),
                             (bool(mask), 'banned / ground / suppress_tokens / ground_names (a vocabulary mask)'),
                             (bool(prefix), 'prefix'), (int(hyp) > 1, 'n_samples'), (bool(attention), 'attention maps')):
                if on:
                    raise ValueError('guidance does not combine with %s: the guided pick covers the arg-max and beam decodes' % what)
            if B % 2:
                raise ValueError('guidance: an even number of rows (every conditional row and its twin), got %d' % B)
        self.guide, self.gamma = (None if guide is None else tuple(guide)), None
        if int(hyp) > 1 and (topk or attention or sample is None or B % int(hyp)):
            raise ValueError('hyp = %d hypotheses per sample: a sampling step without beam search or attention maps, over a '
                             'multiple of %d rows' % (int(hyp), int(hyp)))
        if ban is not None and (sample is not None or attention):
            raise ValueError('no_repeat_ngram_size / min_len do not combine with sampling or attention maps')
        if pen is not None and (ban is not None or attention or (sample is not None and len(sample) != 2)):
            raise ValueError('repetition_penalty / presence_penalty / frequency_penalty do not combine with no_repeat_ngram_size '
                             '/ min_len, attention maps or sampling_topp / sampling_minp / sampling_typical')
        if mask and (pen is not None or attention or (sample is not None and len(sample) != 2)):
            raise ValueError('banned / ground / suppress_tokens / ground_names (a vocabulary mask) do not combine with '
                             'repetition_penalty / presence_penalty / frequency_penalty, attention maps or sampling_topp / '
                             'sampling_minp / sampling_typical')
        self.mask, self.vmask = bool(mask), None
        self.pen = None if pen is None else (float(pen[0]), float(pen[1]), float(pen[2]))
        dec = self.dec = model.decoder
        self.index, self.pad = model.index, int(model.padding_idx)
        self.B, self.gen_len, self.topk, self.n_hyp, self.lane = B, int(gen_len), topk, max(int(topk), 1), int(lane)
        self.per_sample = max(self.n_hyp, int(hyp))               # rows that share one sample's contexts and prefix
        self.sample, self.ban = sample, ban
        names = [n for layer_kv in kv[:1] for n in layer_kv]
        self.static = bool(graphs.ENABLED and not model.training and torch.is_tensor(kv[0][names[0]][0]) and
                           kv[0][names[0]][0].is_cuda)
        if not self.static:
            dev = next(dec.parameters()).device
            self.h, self.state, self.ctx, self.kv = None, {}, contexts, kv
            self.seed = torch.zeros(1, dtype=torch.int32, device=dev)
            if self.guide is not None:
                self.gamma = torch.ones(1, dtype=torch.float32, device=dev)
            self.pfx = self._make_prefix(dev) if prefix else {}
            self.ban_src, self.pen_src = {}, {}
            self.attn = self._make_sink(kv, dev) if attention else None
            self.stats = self._make_stats(dev) if self.n_stats else None
            self.cur = self.counter_out = self.back = None
            return
        h = self.h = self._entry(model, names, kv, contexts, sample, attention, opts, prefix)
        self._fill(kv, contexts)
        self.state, self.ctx, self.kv = h['state'], h['ctx'], h['kv']
        # (the captured launches hold these buffers' addresses: from the entry, never freshly allocated)
        self.pfx, self.ban_src, self.attn = h.get('pfx', {}), h['ban_src'], h.get('attn')
        self.pen_src = h.setdefault('pen_src', {}) if self.pen is not None else {}
        self.vmask = h.get('vmask')
        self.stats = h.get('stats')
        if self.stats is not None:                                # (slots of steps this caption batch never reaches stay neutral)
            self.stats.reset()
        self.gamma = h.get('gamma')
        self.seed, self.cur = h['seed'], h['cur']
        self.c_cur, self.c_next = h['counter'][0:1], h['counter'][1:2]
        # where a bookkeeping launch leaves the next step's offset: the word the embedder's kernel reads (in-graph
        # bookkeeping), or the counter itself  (base 1: the offset of step i is i - 1)
        self.counter_out = self.c_next if h['ig'] else self.c_cur
        self.back = h['state'].get('_back')                       # ancestor table of the DynamicConv rings, or None

    # ---- the cache entry ------------------------------------------------------------
    def _make_prefix(self, device):
        return {'tab': torch.full((self.B // self.per_sample, self.gen_len), self.pad, dtype=torch.long, device=device),
                'plen': torch.zeros(self.B // self.per_sample, dtype=torch.int32, device=device)}

    def _make_mask(self, device):
        words = (int(self.dec.adaptive_softmax.vocab_size) + 31) // 32
        return torch.zeros(self.B // self.per_sample, words, dtype=torch.int32, device=device)

    def _make_stats(self, device):
        return decode.StatsSink(self.n_stats, self.gen_len, self.B, self.pad, device)

    def _make_sink(self, kv, device):
        return decode.AttnSink([{n: torch.zeros(self.gen_len, self.B, int(pair[0].shape[0]) + 2, dtype=torch.float32,
                                                device=device) for n, pair in lk.items()} for lk in kv], self.gen_len)

    def _entry(self, model, names, kv, contexts, sample, attention, opts, prefix):
        """The cache entry of this step's signature: found, or made with every static buffer a capture will pin."""
        dec, B, topk, gen_len, ban = self.dec, self.B, self.topk, self.gen_len, self.ban
        dev, dtype = kv[0][names[0]][0].device, kv[0][names[0]][0].dtype
        # lane: decode loops that are in flight TOGETHER (generate_lanes: two caption batches decoded on two streams) own
        # their graphs, static buffers, counters and split-reduction workspace
        sig = (B, dtype, topk, gen_len, tuple((n, tuple(kv[0][n][0].shape), tuple(kv[0][n][1].shape)) for n in names),
               dec.embedder.token_embedder_position.weights.data_ptr(), self.lane)
        if sample is not None:                                    # (greedy and beam signatures are unchanged)
            sig = sig + ((('sample', int(sample[0]), float(sample[1])) if len(sample) == 2 else
                          ('nucleus', int(sample[0]), float(sample[1]), float(sample[2])) if len(sample) == 3 else
                          (str(sample[3]), int(sample[0]), float(sample[1]), float(sample[2]))),)
        if attention:                                             # (... and so are the sampling ones)
            sig = sig + (('attn',),)
        if ban is not None or opts is not None:                   # (... and the ones without search options)
            sig = sig + (('search', tuple(ban or ()), tuple(opts or ())),)
        if prefix:                                                # (... and every one without a forced prefix)
            sig = sig + (('prefix',),)
        if self.pen is not None:                                  # (... and every one without penalties)
            sig = sig + (('penalty',) + self.pen,)
        if self.per_sample > self.n_hyp:                          # (... and every one with one draw per sample)
            sig = sig + (('hyp', self.per_sample),)
        if self.mask:                                             # (... and every one without a vocabulary mask)
            sig = sig + (('mask',),)
        if self.guide is not None:                                # (... and every one without guidance)
            sig = sig + (('guide', self.guide),)
        if self.hidden:                                           # (... and every one that keeps its hidden row to itself)
            sig = sig + (('hidden',),)
        if self.n_stats:                                          # (... and every one without per-token statistics)
            sig = sig + (('stats', self.n_stats),)
        cache = model.__dict__.setdefault('_decode_graphs', {})
        # A captured step bakes in the addresses of the working weights (weight-normalised copies, the concatenated
        # softmax head) that ops._cached rebuilds - at NEW addresses - whenever the weights change (optimizer step,
        # load_state_dict): every capture belongs to one state of the weights and is dropped with it
        stamp = (ops.rt.weights_epoch(), sum(p._version for p in dec.parameters()))
        if model.__dict__.get('_decode_graphs_stamp') != stamp:
            cache.clear()
            model.__dict__['_decode_graphs_stamp'] = stamp
        h = cache.get(sig)
        if h is not None:
            return h
        if len(cache) >= graphs.MAX_SIGNATURES:
            cache.pop(next(iter(cache)))
        h = cache[sig] = {
            # counter[0]: the position offset the kernels of a replay read; counter[1]: the NEXT step's offset when
            # the bookkeeping launch is part of the captured step (`ig`, below)
            'graph': None, 'counter': torch.zeros(2, dtype=torch.int32, device=dev), 'book': {}, 'ban_src': {},
            'seed': torch.zeros(1, dtype=torch.int32, device=dev),      # the sampling seed (written per caption batch)
            'cur': torch.zeros(B, 1, dtype=torch.long, device=dev),
            'kv': None,
            # (key-padding masks as the uint8 the attention kernels read: converted once per caption batch)
            'ctx': {k: torch.empty_like(v, dtype=torch.uint8 if v.dtype == torch.bool else v.dtype)
                    for k, v in contexts.items() if torch.is_tensor(v)},
            'state': dec.static_incremental_state(B, dev, dtype, beam=bool(topk)),
        }
        po = dec.embedder.token_embedder_position            # the table must already cover the longest caption
        po.next_start(gen_len + 2, None)
        # The static copy of the projected K / V.  Where the weight-streaming step takes this batch (decode.usable: all
        # four attentions of a layer are one tell_attn_decode launch) the copy is HEAD-MAJOR - [B, H, S, 64], handed on
        # as [S, B, H, 64] views: the keys a (sample, head) workgroup walks are one contiguous block instead of 128-byte
        # pieces a whole [B, 2E] projection row (128 KB at B = 32) apart.  The re-layout rides on the copy into the
        # static buffers that the captured step needs anyway, once per caption batch.
        probe = torch.empty(1, B, dec.embedder.get_output_dim(), dtype=dtype, device=dev)
        hm = decode.KV_HEAD_MAJOR and dtype == torch.bfloat16 and decode.usable(dec, probe, h['state'], kv)

        def static_like(t, mod):
            if hm and t.shape[0] > 0 and t.dim() == 3 and t.shape[2] == mod.num_heads * 64:
                S_, Bc, H_ = t.shape[0], t.shape[1], mod.num_heads
                return torch.empty(Bc, H_, S_, 64, dtype=t.dtype, device=t.device).permute(2, 0, 1, 3)
            return torch.empty_like(t)
        # (measured, B = 32: packed 28.6 -> 22.6-24.9 us per launch at beam 4; with ONE hypothesis per sample the VALU kernel on
        #  the head-major cache is the faster one, 18.7 against 20.4 us - packed from two hypotheses per sample on)
        n_cached = kv[0][names[0]][0].shape[1] if kv[0][names[0]][0].dim() == 3 else B
        several = B >= decode.PACKED_MIN_HYP * max(int(n_cached), 1)
        layer_pk = (B > decode.MAX_ROWS and dtype == torch.bfloat16 and bool(h['state'].get('_ring')) and
                    decode.layer_path_takes_packed(dec))     # (the layer-by-layer step above MAX_ROWS rows)
        if decode.KV_PACKED and several and (hm or layer_pk):
            # ... or PACKED for the matrix cores: keys head-major with the two virtual keys appended, values transposed
            # and permuted (decode.PackedKV); one launch per layer reads all four contexts (tell_attn_decode_packed)
            h['kv'] = [{n: decode.PackedKV(layer.context_attns[n], pair[0].shape[0], pair[0].shape[1], dev)
                        for n, pair in lk.items()} for lk, layer in zip(kv, dec.layers)]
        else:
            h['kv'] = [{n: tuple(static_like(t, layer.context_attns[n]) for t in pair) for n, pair in lk.items()}
                       for lk, layer in zip(kv, dec.layers)]
        if attention:
            if topk:
                raise ValueError('attention maps: one hypothesis per sample only (no beam search)')
            h['attn'] = self._make_sink(kv, dev)
        # in-graph bookkeeping needs the step's first kernel to be tell_embed_gather_step (it publishes the counter)
        h['ig'] = bool(decode.IN_GRAPH_BOOK and dtype == torch.bfloat16 and decode.usable(dec, probe, h['state'], kv) and
                       decode.embed_usable(dec.embedder, h['cur'], h['state']))
        if prefix:
            h['pfx'] = self._make_prefix(dev)
        if self.mask:
            h['vmask'] = self._make_mask(dev)
        if self.guide is not None:
            h['gamma'] = torch.ones(1, dtype=torch.float32, device=dev)
        if self.n_stats:
            h['stats'] = self._make_stats(dev)
        return h

    def _fill(self, kv, contexts):
        """This caption batch into the entry's static buffers; the incremental state back to step 0."""
        h = self.h
        for lk, ls in zip(kv, h['kv']):
            for n, pair in lk.items():
                if not isinstance(ls[n], tuple):                  # decode.PackedKV
                    mk = contexts.get(n + '_mask')
                    ls[n].fill(pair[0], pair[1], mk)
                    continue
                for t, s in zip(pair, ls[n]):
                    s.copy_(t.view(s.shape) if s.dim() == 4 else t)
        for k, s in h['ctx'].items():
            s.copy_(contexts[k])
        self.dec.reset_static_state(h['state'])
        h['state'].pop(self.dec.embedder.token_embedder_position._state_key, None)

    # ---- per caption batch ----------------------------------------------------------
    def set_prefix(self, tokens, plen):
        pfx = self.pfx
        if not pfx:
            raise ValueError('set_prefix: the stepper was built without prefix=True')
        if tokens.shape[0] != pfx['tab'].shape[0] or tokens.shape[1] > pfx['tab'].shape[1] or plen.numel() != tokens.shape[0]:
            raise ValueError('set_prefix: tokens [%d, P <= %d] and plen [%d] expected' % (
                pfx['tab'].shape[0], pfx['tab'].shape[1], pfx['tab'].shape[0]))
        pfx['tab'].fill_(self.pad)
        pfx['tab'][:, :tokens.shape[1]].copy_(tokens)
        pfx['plen'].copy_(plen.to(torch.int32))

    def set_guidance(self, gamma):
        """This caption batch's guidance scale into the device float the guided pick reads (a captured step included)."""
        if self.guide is None:
            raise ValueError('set_guidance: the stepper was built without guide=drop')
        self.gamma.fill_(float(gamma))

    def set_mask(self, ctx_ids, cls_bits=None, deny8=None, eos=2):
        """This caption batch's vocabulary masks (one launch, tell_decode_vocab_mask: deny | (cls & ~present) without eos) into
        the stepper's bitmap - the static one of the cache entry, which the captured picks read, or a fresh tensor when the
        step is issued launch by launch.  ctx_ids int64 [samples, S]: every sample's article ids; cls_bits int32 [words]
        (ops.pack_mask_bits) or None; deny8 uint8 [1 or samples, vocab] or None."""
        if not self.mask:
            raise ValueError('set_mask: the stepper was built without mask=True')
        n = self.B // self.per_sample
        if ctx_ids.dim() != 2 or ctx_ids.shape[0] != n:
            raise ValueError('set_mask: ctx_ids int64 [%d, S] expected' % n)
        dev = next(self.dec.parameters()).device
        if not self.static:
            self.vmask = self._make_mask(dev)
        ctx_ids = ctx_ids.to(dev)
        ops.vocab_mask(ctx_ids if ctx_ids.stride(1) == 1 else ctx_ids.contiguous(), self.dec.adaptive_softmax.vocab_size,
                       cls_bits, deny8, eos, self.pad, out=self.vmask)

    def ban_source(self, hist, fin):
        """The histories the ban lists are built from (before every eager step; once when the buffers are static)."""
        B, ban_src = self.B, self.ban_src
        if hist.dtype != torch.long or hist.dim() != 2 or hist.shape[0] != B or hist.stride(1) != 1 or \
                hist.shape[1] > 256 or fin.dtype != torch.uint8 or fin.numel() != B or not fin.is_contiguous():
            raise ValueError('ban_source: hist int64 [%d, L <= 256] and finished uint8 [%d] expected' % (B, B))
        ban_src['hist'], ban_src['fin'] = hist, fin
        if 'ban' not in ban_src or ban_src['ban'].shape[1] < hist.shape[1] + 1 or ban_src['ban'].device != hist.device:
            ban_src['ban'] = torch.zeros(B, hist.shape[1] + 1, dtype=torch.int32, device=hist.device)
            ban_src['n_ban'] = torch.zeros(B, dtype=torch.int32, device=hist.device)

    def stats_source(self, fin):
        """The finished flags the statistics launch reads (before every eager step; once when the buffer is static): a finished
        row writes the neutral values and requests no logit."""
        if self.stats is None:
            raise ValueError('stats_source: the stepper was built without stats=n')
        if fin.dtype != torch.uint8 or fin.numel() != self.B or not fin.is_contiguous():
            raise ValueError('stats_source: finished uint8 [%d] expected' % self.B)
        self.stats.fin = fin

    def pen_source(self, hist, fin):
        """The histories the penalty lists are counted from (before every eager step; once when the buffers are static).  The
        list buffers and the `sub` table (fp32 [L + 1]: sub[0] = 0, sub[c] = float32(alpha + beta * c) formed in fp64) are kept
        while they fit: captured launches hold their addresses."""
        B, src = self.B, self.pen_src
        if self.pen is None:
            raise ValueError('pen_source: the stepper was built without pen=(theta, alpha, beta)')
        if hist.dtype != torch.long or hist.dim() != 2 or hist.shape[0] != B or hist.stride(1) != 1 or \
                hist.shape[1] > 256 or fin.dtype != torch.uint8 or fin.numel() != B or not fin.is_contiguous():
            raise ValueError('pen_source: hist int64 [%d, L <= 256] and finished uint8 [%d] expected' % (B, B))
        src['hist'], src['fin'] = hist, fin
        L = hist.shape[1]
        if 'tok' not in src or src['tok'].shape[1] < L or src['tok'].device != hist.device or src['sub'].numel() != L + 1:
            src['tok'] = torch.zeros(B, L, dtype=torch.int32, device=hist.device)
            src['cnt'] = torch.zeros(B, L, dtype=torch.int32, device=hist.device)
            src['n_pen'] = torch.zeros(B, dtype=torch.int32, device=hist.device)
            src['sub'] = sub_table(self.pen[1], self.pen[2], L).to(hist.device)

    def book(self, kind, make):
        """The caller's static bookkeeping buffers of this signature (made once: a captured bookkeeping launch pins them)."""
        if kind not in self.h['book']:
            self.h['book'][kind] = make()
        return self.h['book'][kind]

    def reorder(self, rows, group=0):                             # in place: the buffers are part of the graph
        state = self.state
        if not self.static or state.get('_ring'):                 # rings: only the ancestor table changes
            self.dec.reorder_incremental_state(state, rows)
            return
        bufs = [s for k_, s in state.items() if 'Conv1dTBC' in k_ and torch.is_tensor(s) and s.shape[0] > 0]
        if (group and 1 <= group <= 8 and bufs and all(s.dtype == torch.bfloat16 and s.is_contiguous() and
                                                       s.shape[2] == 1024 for s in bufs) and len(bufs) <= 8):
            # rows[r] lies inside r's group of `group` hypotheses: every layer's buffer in ONE launch
            ops.call('tell_reorder_rows', len(bufs), ops._ptr_array(bufs), ops._int_array([s.shape[0] for s in bufs]),
                     rows, bufs[0].shape[1], 1024, int(group))
            return
        for s in bufs:
            s.copy_(s.index_select(1, rows))

    # ---- one step -------------------------------------------------------------------
    def _head(self, x, sidx):
        """The head over the decoder's output x at step index sidx (the host's int, or the device counter of a captured
        step): arg-max, top-k, a draw, the banned top-k, or - after the counts launch - the penalised top-k / draw; with a
        forcing table every one of them ends in the forced pick."""
        soft, pfx = self.dec.adaptive_softmax, self.pfx
        force = (pfx['tab'], pfx['plen'], None, self.per_sample, sidx, self.pad) if pfx else None
        skw = {'stats': self.stats.at(sidx)} if self.stats is not None else {}     # (without it every call is the call it was)
        if self.guide is not None:                                    # row r and its twin r + B / 2: one pick for both
            tok, lp = soft.topk(x, self.n_hyp, guide=(self.B // 2, self.gamma))
            return (tok, lp) if self.topk else (tok.view(tok.shape[0], tok.shape[1]), lp.view(lp.shape[0], lp.shape[1]))
        if self.mask:
            if self.vmask is None:
                raise ValueError('a stepper with mask=True needs set_mask(...) before its first step')
            mask, ban = (self.vmask, self.per_sample), None
            if self.ban is not None:                                  # the ban list first; the masked pick ORs it in
                src = self.ban_src
                hist = src['hist']
                step_dev = sidx if torch.is_tensor(sidx) else None
                ops.call('tell_decode_ban_list', hist, hist.stride(0), hist.shape[1], src['fin'], self.B,
                         0 if step_dev is not None else int(sidx), step_dev, int(self.ban[0]), int(self.ban[1]),
                         int(self.ban[2]), src['ban'], src['ban'].stride(0), src['n_ban'])
                ban = (src['ban'], src['n_ban'])
            if self.sample is not None:
                return soft.sample(x, self.sample[0], self.sample[1], self.seed, sidx, force=force, mask=mask, **skw)
            tok, lp = soft.topk(x, self.n_hyp, ban=ban, force=force, mask=mask, **skw)
            return (tok, lp) if self.topk else (tok.view(tok.shape[0], tok.shape[1]), lp.view(lp.shape[0], lp.shape[1]))
        if self.ban is not None:
            ban, src = self.ban, self.ban_src
            hist = src['hist']
            step_dev = sidx if torch.is_tensor(sidx) else None
            ops.call('tell_decode_ban_list', hist, hist.stride(0), hist.shape[1], src['fin'], self.B,
                     0 if step_dev is not None else int(sidx), step_dev, int(ban[0]), int(ban[1]), int(ban[2]),
                     src['ban'], src['ban'].stride(0), src['n_ban'])
            tok, lp = soft.topk(x, self.n_hyp, ban=(src['ban'], src['n_ban']), force=force, **skw)
            return (tok, lp) if self.topk else (tok.view(tok.shape[0], tok.shape[1]), lp.view(lp.shape[0], lp.shape[1]))
        pen = None
        if self.pen is not None:
            src = self.pen_src
            hist = src['hist']
            step_dev = sidx if torch.is_tensor(sidx) else None
            ops.call('tell_decode_token_counts', hist, hist.stride(0), hist.shape[1], src['fin'], self.B,
                     0 if step_dev is not None else int(sidx), step_dev, src['tok'], src['cnt'], src['tok'].stride(0),
                     src['n_pen'])
            pen = (self.pen[0], src['sub'], src['tok'], src['cnt'], src['n_pen'])
            if self.sample is None:
                tok, lp = soft.topk(x, self.n_hyp, force=force, pen=pen, **skw)
                return (tok, lp) if self.topk else (tok.view(tok.shape[0], tok.shape[1]), lp.view(lp.shape[0], lp.shape[1]))
            return soft.sample(x, self.sample[0], self.sample[1], self.seed, sidx, force=force, pen=pen, **skw)
        if self.sample is not None:
            topp = self.sample[2] if len(self.sample) > 2 else None      # nucleus: p is a launch argument, like the temperature
            rule = self.sample[3] if len(self.sample) > 3 else None      # 'minp' / 'typical': topp is m / tau
            return soft.sample(x, self.sample[0], self.sample[1], self.seed, sidx, topp=topp, force=force, rule=rule, **skw)
        if self.topk:
            return soft.topk(x, self.topk, force=force)
        return soft.greedy(x, force=force, **skw)

    def _run(self, sidx, cur):
        """sidx: the step index for a sampling head - the host's int, or c_cur inside a captured step (i - 1 there)."""
        prev_lane = decode.CUR_LANE[0]
        decode.CUR_LANE[0] = self.lane
        try:
            kw = {}
            if self.attn is not None:
                # slot = step index: the host's in an eager step; captured, the counter holds i - 1 (base 1)
                kw['attn_sink'] = self.attn.at(1, sidx) if torch.is_tensor(sidx) else self.attn.at(int(sidx))
            out = self.dec({self.index: cur}, self.ctx, incremental_state=self.state, kv_cache=self.kv, **kw)
            x = out[0][:, -1:]
            return self._head(x, sidx) + ((x,) if self.hidden else ())
        finally:
            decode.CUR_LANE[0] = prev_lane

    def _eager(self, i, cur, post):
        res = self._run(int(i), cur)
        if post is not None:
            post(res, i, None)
        return res

    def __call__(self, i, cur, counter_set=False, post=None):
        """post(out, i, step_dev): the caller's per-token bookkeeping launch (over static buffers: step.book).  With
        in-graph bookkeeping it is recorded as the LAST launch of the captured step."""
        h = self.h
        if h is None:
            return self._eager(i, cur, post)
        if cur is not None:                                   # (None: the caller already wrote step.cur)
            self.cur.copy_(cur)
        if h['graph'] is None and i != 1:
            return self._eager(i, self.cur, post)             # warm step(s) before the capture, or fallback
        if h['graph'] is None:                                # i == 1: the host position state is 1 now
            inside = post is not None and h['ig']
            # the host's part of the step's position state as THIS capture sees it (step.multi records further steps
            # with the same constants: the device counter is what moves a recorded step along)
            h['host_ints'] = {k_: v_ for k_, v_ in h['state'].items() if isinstance(v_, int) and not isinstance(v_, bool)}
            try:
                g = torch.cuda.CUDAGraph()
                # (the captured step's resident GEMM launches keep their tile-counter slots until this entry is
                #  dropped - `held` gives them back, like StepGraph / GraphedCall do)
                with graphs.capture(g, rng=self.c_cur, pos=self.c_cur, pos_next=self.c_next if inside else None) as held:
                    h['out'] = self._run(self.c_cur, self.cur)
                    if inside:
                        post(h['out'], i, self.c_cur)
                h['tile_slots'] = held
                h['graph'], h['base'], h['graph_has_post'] = g, 1, inside
            except Exception as exc:                          # noqa: BLE001 - stay eager for this signature
                h['graph'], h['error'] = False, repr(exc)
                return self._eager(i, self.cur, post)
        if h['graph'] is False:
            return self._eager(i, self.cur, post)
        if not counter_set:
            # position offset of this step (may be -1): into the word the step's first kernel reads
            (self.c_next if h.get('graph_has_post') else self.c_cur).fill_(i - h['base'])
        h['graph'].replay()
        if post is not None and not h.get('graph_has_post'):
            post(h['out'], i, None)
        return h['out']

    def multi(self, i, n, post):
        """Steps i .. i + n - 1 as ONE graph replay (n consecutive steps recorded into one graph: the bookkeeping launch
        that ends a recorded step leaves the position offset of the next one in the device counter, so the steps chain
        on the device exactly as n single replays would - what goes is the per-replay cost between them, ~25 us of a
        360-490 us step).  Needs the single-step graph with in-graph bookkeeping (captured at step 1) and the counter
        already set by step i - 1's bookkeeping launch.  -> False: not available, issue the steps one by one."""
        h = self.h
        if not self.static or not h.get('graph') or not h.get('graph_has_post') or post is None or i < 2 or \
                not MULTI_STEP_GRAPHS:
            return False
        key = ('multi', int(n))
        g = h.get(key)
        if g is None:
            saved = {k_: h['state'].get(k_) for k_ in h['host_ints']}
            try:
                g = torch.cuda.CUDAGraph()
                try:
                    with graphs.capture(g, rng=self.c_cur, pos=self.c_cur, pos_next=self.c_next) as held:
                        for j in range(int(n)):
                            h['state'].update(h['host_ints'])   # the constants of the single-step capture
                            post(self._run(self.c_cur, self.cur), i + j, self.c_cur)
                    h[key + ('slots',)] = held
                finally:
                    h['state'].update(saved)
                h[key] = g
            except Exception as exc:                          # noqa: BLE001 - keep the single-step replays
                h[key], h['multi_error'] = False, repr(exc)
                return False
        if g is False:
            return False
        g.replay()
        return True

    def steps(self, gen_len, check_every, post, fin8, multi=True, after=None):
        """The issue loop of a search over static buffers - a generator: yields i after every issued step i or multi-step
        replay ending in step i (generate_lanes alternates its lanes on these), BEFORE the all-finished test; returns the
        number of steps issued when it stopped.  post: the bookkeeping launch that ends a step (see __call__), or None with
        after(out, i): host-side work behind a single step.  fin8: the search's finished flags, read (one sync) every
        `check_every` steps.  multi: whether `check_every` steps may go as one replay (self.multi) from the first test on."""
        i = 0
        while i < gen_len:
            # (the bookkeeping launch of step i - 1 left the position offset of step i in the device counter: no fill launch;
            #  the host's part of a step is ONE graph replay - and from the first all-finished test on, of `check_every` steps)
            n = check_every if (multi and i >= check_every and i % check_every == 0 and i + check_every <= gen_len) else 1
            if n == 1 or not self.multi(i, n, post):
                n = 1
                out = self(i, None, counter_set=i > 0, post=post)
                if after is not None:
                    after(out, i)
            i += n
            yield i - 1
            if i % check_every == 0 and bool(fin8.all()):
                break
        return i
