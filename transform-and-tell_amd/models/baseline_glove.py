"""tell/models/baseline_glove.py:22-320 (`baseline_glove`, expt/*/1_lstm_glove) on the MI355X path.

The reference turns the raw article strings into GloVe vectors with spaCy INSIDE the model (:207-220).  That lookup is
data plane (no spaCy / vectors offline); this class starts from what it produces - `context_vectors`, a [B, L, 300]
fp32 tensor of the vectors of the tokens that have one, NaN-padded to the longest article of the batch (:216-220) -
passed either directly or as `metadata[i]['context_vectors']`."""
import math

import torch

from .. import ops
from .transformer import (PENALTY_KEYS, CaptionModel, Model, check_beam_options, check_guidance, check_mask_keys,
                          check_penalties, check_sampling, draw_seed, refuse_weighted_forward, set_sampling)


def _refuse_mask_options(model, suppress_tokens=(), ground_names=False, banned=None, ground=None):
    """BaselineGloveModel decodes with an LSTM decoder: the vocabulary masks are out of scope there."""
    st, gn = check_mask_keys(suppress_tokens, ground_names)
    used = [n for n, on in (('banned', banned is not None), ('ground', ground is not None and ground is not False),
                            ('suppress_tokens', bool(st)), ('ground_names', gn)) if on]
    if used:
        raise ValueError('%s: %s decodes with an LSTM decoder, whose step has its own decision launch; vocabulary masks cover '
                         'the cached DynamicConv generator only' % (' / '.join(used), type(model).__name__))
    return st, gn


def _refuse_guidance(model, guidance_scale=1.0, guidance_drop=('image',)):
    """BaselineGloveModel decodes with an LSTM decoder: context guidance is out of scope there."""
    gamma, drop = check_guidance(guidance_scale, guidance_drop)
    if gamma != 1.0:
        raise ValueError('guidance=%r: %s decodes with an LSTM decoder, whose step has its own decision launch; context guidance '
                         'covers the cached DynamicConv generator only' % (gamma, type(model).__name__))
    return gamma, drop


def _refuse_search_options(model, beam_len_penalty=0.0, no_repeat_ngram_size=0, min_len=0, n_best=1):
    """The LSTM decoders' step has its own decision launch: the search options of the cached DynamicConv generator
     are refused here unless they are at their defaults."""
    opts = check_beam_options(beam_len_penalty, no_repeat_ngram_size, min_len)
    used = ['%s=%r' % (k, v) for k, v in zip(('beam_len_penalty', 'no_repeat_ngram_size', 'min_len'), opts) if v]
    if isinstance(n_best, bool) or not isinstance(n_best, int) or n_best < 1:
        raise ValueError('n_best must be an integer >= 1 (got %r)' % (n_best,))
    if n_best != 1:
        used.append('n_best=%r' % (n_best,))
    if used:
        raise ValueError('%s: %s decodes with an LSTM decoder; the search options cover the cached DynamicConv generator '
                         'only' % (' / '.join(used), type(model).__name__))


@Model.register('baseline_glove')
class BaselineGloveModel(Model):
    def __init__(self, vocab, decoder, criterion, evaluate_mode=False, namespace='bpe', index='roberta',
                 padding_value=1, use_context=True, sampling_topk=1, sampling_temp=1.0, max_caption_len=50,
                 weigh_bert=False, initializer=None, resnet=None, sampling_topp=None, beam_len_penalty=0.0,
                 no_repeat_ngram_size=0, min_len=0, sampling_minp=None, sampling_typical=None, repetition_penalty=1.0,
                 presence_penalty=0.0, frequency_penalty=0.0, suppress_tokens=(), ground_names=False, guidance_scale=1.0,
                 guidance_drop=('image',)):
        super().__init__(vocab)
        _refuse_search_options(self, beam_len_penalty, no_repeat_ngram_size, min_len)
        self.suppress_tokens, self.ground_names = _refuse_mask_options(self, suppress_tokens, ground_names)
        self.guidance_scale, self.guidance_drop = _refuse_guidance(self, guidance_scale, guidance_drop)
        pen = check_penalties(repetition_penalty, presence_penalty, frequency_penalty)
        if pen != (1.0, 0.0, 0.0):
            raise ValueError('%s: %s decodes with an LSTM decoder; the penalties cover the cached DynamicConv generator only'
                             % (' / '.join('%s=%r' % (k_, v) for k_, v, d in zip(PENALTY_KEYS, pen, (1.0, 0.0, 0.0)) if v != d),
                                type(self).__name__))
        self.repetition_penalty, self.presence_penalty, self.frequency_penalty = pen
        for name, v in (('sampling_minp', sampling_minp), ('sampling_typical', sampling_typical)):
            if v is not None:
                raise ValueError('%s=%r: %s has a decode step with its own decision launch (LSTM decoder); min-p and typical '
                                 'sampling cover the cached DynamicConv generator only' % (name, v, type(self).__name__))
        self.decoder, self.criterion = decoder, criterion
        self.index, self.namespace = index, namespace
        if resnet is None:
            from .resnet import resnet152
            resnet = resnet152()
        self.resnet = resnet
        self.use_context, self.padding_idx, self.evaluate_mode = use_context, padding_value, evaluate_mode
        self.sampling_topk, self.sampling_temp = check_sampling(sampling_topk, sampling_temp, sampling_topp)[:2]
        self.sampling_topp = None if sampling_topp is None else float(sampling_topp)
        self.max_caption_len = max_caption_len
        self.n_batches = self.n_samples = 0

    @staticmethod
    def _vectors(context_vectors, metadata):
        if context_vectors is not None:
            return context_vectors
        vs = [torch.as_tensor(m['context_vectors'], dtype=torch.float32) for m in metadata]
        L = max(v.shape[0] for v in vs)
        out = torch.full((len(vs), L, 300), float('nan'))
        for i, v in enumerate(vs):
            out[i, :v.shape[0]] = v
        return out

    def _forward(self, context_vectors, image, caption):                       # :164-245
        dtype = ops.rt.compute_dtype()
        cap = caption[self.index]
        target_ids = torch.zeros_like(cap)
        target_ids[:, :-1] = cap[:, 1:]
        caption_ids = cap[:, :-1][:, :self.max_caption_len].contiguous()       # :176-181
        target_ids = target_ids[:, :-1][:, :self.max_caption_len].contiguous()
        caption[self.index] = caption_ids
        with torch.no_grad():
            x_image = CaptionModel._run_resnet(self, image)                    # [B, 49, 2048]  (:186-198)
        B, P, _ = x_image.shape
        cv = context_vectors.to(image.device)
        Bc, L, dim = cv.shape
        clean = torch.empty(Bc, L, dim, dtype=dtype, device=cv.device)         # :222-226 NaN rows -> mask, zeros
        mask = torch.empty(Bc, L, dtype=torch.uint8, device=cv.device)
        ops.call('tell_nan_rows', cv.float().contiguous(), Bc * L, dim, clean, ops.hip.dt(dtype), mask)
        contexts = {'image': x_image.transpose(0, 1),
                    'image_mask': torch.zeros(B, P, dtype=torch.bool, device=image.device),
                    'article': clean.transpose(0, 1), 'article_mask': mask.bool(),
                    'sections': None, 'sections_mask': None}
        return caption_ids, target_ids, contexts

    def forward(self, image, caption, metadata=None, context_vectors=None, caption_weights=None, per_image=1):    # :71-162
        refuse_weighted_forward(self, caption_weights, per_image)
        ops.hip.require_gpu()
        caption_ids, target_ids, contexts = self._forward(self._vectors(context_vectors, metadata), image, caption)
        ops.rt.wait_weight_update()
        decoder_out = self.decoder(caption, contexts)
        loss_sum, sample_size = self.criterion(self.decoder.adaptive_softmax, decoder_out, target_ids)
        loss = (loss_sum / math.log(2) / sample_size.to(torch.float32)).reshape(())
        out = {'loss': loss, 'sample_size': sample_size.reshape(())}
        if not self.training and self.evaluate_mode:
            _, gen_ids = self._generate(caption_ids, contexts)
            out['gen_ids'] = gen_ids.cpu().numpy()
        self.n_samples += caption_ids.shape[0]
        self.n_batches += 1
        return out

    def generate(self, image, caption, metadata=None, context_vectors=None, attention=False, n_best=1, prefix=None,
                 n_samples=1, rank_by='score', rank_len_penalty=0.0, banned=None, ground=None, guidance=None,
                 guidance_drop=None, token_stats=0):
        if token_stats:
            from .stepper import TOKEN_STATS_REFUSALS
            raise ValueError('token_stats=%r: %s' % (token_stats, TOKEN_STATS_REFUSALS['lstm']))
        _refuse_search_options(self, n_best=n_best)
        _refuse_mask_options(self, banned=banned, ground=ground)
        _refuse_guidance(self, getattr(self, 'guidance_scale', 1.0) if guidance is None else guidance,
                         getattr(self, 'guidance_drop', ('image',)) if guidance_drop is None else guidance_drop)
        from .transformer import check_n_samples
        if check_n_samples(n_samples, rank_by, rank_len_penalty)[0] > 1:
            raise ValueError('n_samples=%d: %s decodes with an LSTM decoder, whose step has its own decision launch; several '
                             'samples per image cover the cached DynamicConv generator only (DESIGN.md section 21)'
                             % (n_samples, type(self).__name__))
        if prefix is not None:
            raise ValueError('prefix: %s decodes with an LSTM decoder, whose step has its own decision launch; a forced '
                             'prefix is out of scope there (DESIGN.md section 17)' % type(self).__name__)
        if attention:
            raise ValueError('attention=True: %s decodes with an LSTM decoder; attention maps are exported for the DynamicConv '
                             'decoders only (its dot attention is not covered)' % type(self).__name__)
        caption_ids, _, contexts = self._forward(self._vectors(context_vectors, metadata), image, caption)
        log_probs, gen_ids = self._generate(caption_ids, contexts)
        return {'gen_ids': gen_ids, 'log_probs': log_probs}

    @torch.no_grad()
    def _generate(self, caption_ids, contexts, gen_len=100, eos=2):
        """Greedy decode of :247-320.  The reference re-decodes the whole prefix for the still-active rows at every
        step; rows are independent and the decoder is recurrent, so carrying the LSTM state forward and keeping the
        batch at its full size (finished rows masked) gives the same token ids: pad after <eos>, length = 1 + steps
        until the last row has finished.  sampling_topk = k > 1 (:247-320 with topk + multinomial): the k best of the full
        log-prob row, sorted, and the draw of tell_sample_candidates keyed on (seed, row, step) - one seed per call from
        torch's default CPU generator.  sampling_topp = p: the nucleus draw - of those k candidates
        (tell_nucleus_candidates), or with k = 0 of the whole row (tell_adaptive_logprob_nucleus over the log-prob row as a
        head without tails: a log-softmax of log-probs leaves them as they are)."""
        B, dev = caption_ids.shape[0], caption_ids.device
        k = int(self.sampling_topk)
        topp = self.sampling_topp
        if k > 1 or topp is not None:
            seed_word = torch.full((1,), draw_seed(), dtype=torch.int32, device=dev)
            inv_temp = 1.0 / float(self.sampling_temp)
        cur = caption_ids[:, 0:1].contiguous()
        finished = cur[:, 0] == eos
        ids = torch.full((B, gen_len + 1), self.padding_idx, dtype=torch.long, device=dev)
        ids[:, 0] = cur[:, 0]
        lps = torch.zeros(B, gen_len, dtype=torch.float32, device=dev)
        state, steps = {}, gen_len
        for i in range(gen_len):
            out = self.decoder({self.index: cur}, contexts, incremental_state=state)
            lp_all = self.decoder.get_normalized_probs((out[0][:, -1:], None), log_probs=True).squeeze(1).float()
            if topp is not None:
                tok32 = torch.empty(B, dtype=torch.int32, device=dev)
                lp = torch.empty(B, dtype=torch.float32, device=dev)
                if k == 0:
                    lp_all = lp_all.contiguous()
                    ops.call('tell_adaptive_logprob_nucleus', lp_all, lp_all.stride(0), lp_all.shape[1], 0, None, 0, 0, None, 0,
                             0, None, 0, 0, B, 0, inv_temp, topp, seed_word, None, i, None, tok32, lp, None, None)
                else:
                    top_lp, top_ix = lp_all.topk(k, dim=-1)                        # sorted, best first
                    ops.call('tell_nucleus_candidates', top_ix.to(torch.int32).contiguous(), top_lp.contiguous(), B, k,
                             inv_temp, topp, seed_word, None, i, None, tok32, lp)
                tok = tok32.long()
            elif k == 1:
                lp, tok = lp_all.max(dim=-1)
            else:
                top_lp, top_ix = lp_all.topk(k, dim=-1)                            # sorted, best first
                tok32 = torch.empty(B, dtype=torch.int32, device=dev)
                lp = torch.empty(B, dtype=torch.float32, device=dev)
                ops.call('tell_sample_candidates', top_ix.to(torch.int32).contiguous(), top_lp.contiguous(), B, k, inv_temp,
                         seed_word, None, i, None, tok32, lp)
                tok = tok32.long()
            ids[:, i + 1] = torch.where(finished, ids[:, i + 1], tok)
            lps[:, i] = torch.where(finished, lps[:, i], lp / self.sampling_temp)
            finished = finished | (tok == eos)
            cur = tok.view(B, 1)
            if bool(finished.all()):
                steps = i + 1
                break
        return lps[:, :steps], ids[:, :steps + 1]


@Model.register('transformer_glove')
class TransformerGloveModel(CaptionModel):
    """tell/models/transformer_glove.py (`transformer_glove`, expt/*/2_transformer_glove): the 2-context DynamicConv decoder
    over ResNet regions and GloVe article vectors.  `_forward` is the baseline's (:161-230, no caption truncation);
    generation is the transformer models' (projected-K/V cache, static batch, captured decode step)."""

    def __init__(self, vocab, decoder, criterion, evaluate_mode=False, attention_dim=1024, hidden_size=1024, dropout=0.1,
                 vocab_size=50264, model_name='roberta-base', namespace='bpe', index='roberta', padding_value=1,
                 use_context=True, sampling_topk=1, sampling_temp=1.0, initializer=None, resnet=None, sampling_topp=None,
                 beam_len_penalty=0.0, no_repeat_ngram_size=0, min_len=0, sampling_minp=None, sampling_typical=None,
                 repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, suppress_tokens=(), ground_names=False,
                 guidance_scale=1.0, guidance_drop=('image',)):
        Model.__init__(self, vocab)
        self.decoder, self.criterion = decoder, criterion
        self.index, self.namespace = index, namespace
        if resnet is None:
            from .resnet import resnet152
            resnet = resnet152()
        self.resnet = resnet
        self.use_context, self.padding_idx, self.evaluate_mode = use_context, padding_value, evaluate_mode
        set_sampling(self, sampling_topk, sampling_temp, sampling_topp, sampling_minp, sampling_typical)
        self.beam_len_penalty, self.no_repeat_ngram_size, self.min_len = check_beam_options(
            beam_len_penalty, no_repeat_ngram_size, min_len)
        self._check_options()
        self._check_truncation()
        self.repetition_penalty, self.presence_penalty, self.frequency_penalty = check_penalties(
            repetition_penalty, presence_penalty, frequency_penalty)
        self._check_penalties()
        self.suppress_tokens, self.ground_names = check_mask_keys(suppress_tokens, ground_names)
        self._check_mask_options()
        self._check_grounding()
        self.guidance_scale, self.guidance_drop = check_guidance(guidance_scale, guidance_drop)
        self._check_guidance()
        self.weigh_bert = False
        self.max_caption_len = 1 << 30
        self.n_batches = self.n_samples = 0

    EVAL_ATTENTION = False       # its own forward(): evaluate mode generates without maps (no article pieces to merge either)

    def _check_grounding(self, ground=None):
        """The article of this model is a matrix of GloVe vectors: its batches carry no article token ids, so there is nothing
        to ground a class in - `banned` and `suppress_tokens` apply, `ground` / `ground_names` are refused."""
        if (ground is not None and ground is not False) or getattr(self, 'ground_names', False):
            raise ValueError('%s: %s reads GloVe article vectors; its batches hold no article token ids to ground a class in'
                             % ('ground' if ground is not None and ground is not False else 'ground_names', type(self).__name__))

    def _no_article(self, caption):
        """The `context` of a batch without article ids, for _vocab_mask: an empty article - the mask is the banned set alone."""
        ids = caption[self.index]
        return {self.index: ids.new_zeros(ids.shape[0], 0)}
    _vectors = staticmethod(BaselineGloveModel._vectors)
    _glove_forward = BaselineGloveModel._forward

    def forward(self, image, caption, metadata=None, context_vectors=None, caption_weights=None, per_image=1):
        refuse_weighted_forward(self, caption_weights, per_image)
        ops.hip.require_gpu()
        caption_ids, target_ids, contexts = self._glove_forward(self._vectors(context_vectors, metadata), image, caption)
        contexts = {k: v for k, v in contexts.items() if v is not None}
        ops.rt.wait_weight_update()
        decoder_out = self.decoder(caption, contexts)
        loss_sum, sample_size = self.criterion(self.decoder.adaptive_softmax, decoder_out, target_ids)
        loss = (loss_sum / math.log(2) / sample_size.to(torch.float32)).reshape(())
        out = {'loss': loss, 'sample_size': sample_size.reshape(())}
        if not self.training and self.evaluate_mode:
            vm = self._vocab_mask(self._no_article(caption))
            guide = self._check_guidance()
            _, gen_ids, _ = self._generate(caption_ids, contexts, vmask=vm, guide=guide)
            out['gen_ids'] = gen_ids.cpu().numpy()
        self.n_samples += caption_ids.shape[0]
        self.n_batches += 1
        return out

    def generate(self, image, caption, metadata=None, context_vectors=None, beam_size=1, attention=False, n_best=1,
                 prefix=None, n_samples=1, rank_by='score', rank_len_penalty=0.0, banned=None, ground=None, guidance=None,
                 guidance_drop=None, token_stats=0):
        if attention:
            self._check_attention(beam_size)
        self._check_grounding(ground)
        plan = self._plan(beam_size, attention, n_best, prefix, n_samples, rank_by, rank_len_penalty, banned, ground, guidance,
                          guidance_drop, token_stats, self._no_article(caption), caption[self.index].shape[0])
        caption_ids, _, contexts = self._glove_forward(self._vectors(context_vectors, metadata), image, caption)
        contexts = {k: v for k, v in contexts.items() if v is not None}
        return self._generated(plan, *self._generate(caption_ids, contexts, **plan.keywords()))
