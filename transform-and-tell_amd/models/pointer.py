"""tell/models/transformer_pointer.py and transformer_pointer_2.py on the MI355X path: transformer_faces plus the
copy mechanism (an entity head that decides, per caption token, whether to copy a name from the article, and a copy
attention over the article that picks which).

Training restates `pointer_loss` (:180-313) with the kernels of csrc/copy.hip: entity self-attention over strictly
earlier positions, entity_fc + cross entropy, 16-head copy attention with head-mean weights, and the fused copy loss
(no [B, T, V] tensor, no host loop over entity indices).  Variant 1 (transformer_pointer) takes the mean -log p of
each entity index, variant 2 (transformer_pointer_2) a cross entropy over the batch's reduced vocabulary.  The loss
is entity_loss + copy_loss in bits; gen_loss is computed and logged only.

Generation (_generate :427-696) is greedy: per step the decoder's token, the entity decision over the step's output
and its history, and one copy-decision launch (csrc/copy.hip tell_copy_step) with the article keys projected once
per batch.  With `cached_generation` / `generate(cached=True)` the same decode runs through the cached, captured step of the
plain models (_pointer_steps; csrc/copy_decode.hip tell_entity_attn_step and tell_copy_decide), and a
model that samples (`sampling_topp`) draws `n_samples` captions per image there, from one pass of the encoders, one cached
context and one read of the article keys per step (tell_copy_decide_hyp)."""
import logging
import math
from collections import defaultdict

import torch
import torch.nn as nn
from torch.nn.init import constant_, xavier_normal_, xavier_uniform_

from .. import ops
from ..modules.linear import GehringLinear
from ..modules.self_attention import SelfAttention
from .transformer import CaptionModel, Model, draw_seed, refuse_weighted_forward

logger = logging.getLogger(__name__)


def load_state_dict_with_prefix(module, state_dict, prefix=''):
    """tell/modules/mixins.py LoadStateDictWithPrefix: keys missing from / unexpected by the checkpoint are reported
    as a warning, not an error."""
    sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
    result = nn.Module.load_state_dict(module, sd, strict=False)
    if result.missing_keys:
        logger.warning('missing keys in the checkpoint: %s', result.missing_keys)
    if result.unexpected_keys:
        logger.warning('unexpected keys in the checkpoint: %s', result.unexpected_keys)
    return result


class PointerModelBase(CaptionModel):
    USE_FACES_OBJECTS = True
    EXTRA_CONTEXTS = ('faces',)
    COPY_VARIANT = 1
    SEARCH_OPTIONS = False         # the decode step ends in the copy decision: the search options are out of scope
    CACHED_N_SAMPLES = True        # ... but n sampled hypotheses per image decode through the cached step (_pointer_steps)
    STEP_GRAPH = False             # the loss may be None (no copy target in the batch): the trainer stays eager
    # the trainer's shape buckets would pad the article with pad ids: transformer_pointer_2's reduced vocabulary counts
    # every id of the context, so padding the graphs need (and these models do not capture) would change its loss
    SHAPE_BUCKETS = False

    def __init__(self, vocab, decoder, criterion, evaluate_mode=False, attention_dim=1024, hidden_size=1024,
                 dropout=0.1, vocab_size=50264, model_name='roberta-base', namespace='bpe', index='roberta',
                 padding_value=1, use_context=True, sampling_topk=1, sampling_temp=1.0, weigh_bert=False,
                 model_path=None, initializer=None, resnet=None, roberta=None, n_bert_layers=25, sampling_topp=None,
                 beam_len_penalty=0.0, no_repeat_ngram_size=0, min_len=0, sampling_minp=None, sampling_typical=None,
                 repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, suppress_tokens=(), ground_names=False,
                 guidance_scale=1.0, guidance_drop=('image',), cached_generation=False):
        if sampling_topk != 1 and sampling_topp is None and sampling_minp is None and sampling_typical is None:       # (with sampling_topp: the generated token is a nucleus draw)
            raise ValueError('transformer_pointer generates greedily: sampling_topk must be 1 (got %r)' % (sampling_topk,))
        super().__init__(vocab, decoder, criterion, evaluate_mode, attention_dim, hidden_size, dropout, vocab_size,
                         model_name, namespace, index, padding_value, use_context, sampling_topk, sampling_temp,
                         weigh_bert, initializer, resnet, roberta, n_bert_layers, sampling_topp,
                         beam_len_penalty, no_repeat_ngram_size, min_len,   # (refused unless at their defaults: SEARCH_OPTIONS)
                         sampling_minp, sampling_typical,                   # (... and so are these: _check_truncation)
                         repetition_penalty, presence_penalty, frequency_penalty,       # (... and these: _check_penalties)
                         suppress_tokens, ground_names,                                 # (... and these: _check_mask_options)
                         guidance_scale, guidance_drop)                                 # (... and these: _check_guidance)
        if weigh_bert:
            self.bert_weight_2 = nn.Parameter(torch.rand(n_bert_layers))      # :61-62
        self.batch_history = defaultdict(float)        # summed on the device (0-d tensors); floats once get_metrics reads
        self.copy_dropout = 0.1                      # p of the per-head copy weights (:234, a constant in the reference)
        self.entity_fc = GehringLinear(1024, 2)
        self.in_proj_weight = nn.Parameter(torch.empty(2 * 1024, 1024))     # :78-84
        self.in_proj_bias = nn.Parameter(torch.empty(2 * 1024))
        self.out_proj = GehringLinear(1024, 1024, bias=True)                 # never used (as in the reference)
        self.bias_k = nn.Parameter(torch.empty(1, 1, 1024))
        xavier_uniform_(self.in_proj_weight)
        constant_(self.in_proj_bias, 0.)
        xavier_normal_(self.bias_k)
        self.entity_attn = SelfAttention(out_channels=1024, embed_dim=1024, num_heads=16, gated=True)
        # never applied (project_input=False; out_proj of the copy attention): in the reference their grad stays None
        # and BertAdam skips them, here the trainer's flat optimizer leaves out what does not require a gradient
        am = self.entity_attn.attention.attention_module
        for m in (self.out_proj, am.in_proj_q, am.in_proj_k, am.in_proj_v):
            for p in m.parameters():
                p.requires_grad_(False)
        self.vocab_size = vocab_size
        self.copy_heads = 16
        # generate() / forward() in evaluate mode decode through the cached, captured step (_pointer_steps)
        self.cached_generation = bool(cached_generation)
        if model_path is not None:
            logger.info('Recovering weights from %s.', model_path)
            load_state_dict_with_prefix(self, torch.load(model_path, map_location='cpu'))

    def lanes_usable(self):
        return False

    EVAL_ATTENTION = False       # forward() generates through _generate_pointer: no attention maps

    def _check_attention(self, beam_size=1):
        raise ValueError('attention=True: %s is a pointer model; attention maps are exported for the plain caption models only '
                         '(the copy attention is not covered)' % type(self).__name__)

    def _check_beam(self, beam_size):
        if int(beam_size) > 1:
            raise ValueError('transformer_pointer has no beam search (beam_size %d)' % int(beam_size))

    # ------------------------------------------------------------------ pieces shared by loss and generation
    def _require_masks(self, context, caption=None):
        """The masks of the names-matched indexer (`<index>_copy_masks`: entity index of each caption token, padded
        with -1; `<index>_proper_masks`: 1 for the article tokens a name may be copied from, padded with -1)."""
        need = [(context, '_proper_masks')] + ([(caption, '_copy_masks')] if caption is not None else [])
        for field, key in need:
            if self.index + key not in field:
                raise ValueError('%s needs %s%s in the batch (a names-matched batch: see DESIGN.md section 13)'
                                 % (type(self).__name__, self.index, key))

    def _article_2(self, enc):
        return ops.mix_layers(enc.stack, self.bert_weight_2) if self.weigh_bert else enc.stack[-1]   # :199-213

    def _copy_q(self, X):
        E = self.in_proj_weight.shape[1]
        return ops.linear(X, self.in_proj_weight, self.in_proj_bias, rows=(0, E), alpha=(E // self.copy_heads) ** -0.5)

    def _copy_k(self, x_article):
        E = self.in_proj_weight.shape[1]
        return ops.linear(x_article, self.in_proj_weight, self.in_proj_bias, rows=(E, 2 * E)).transpose(0, 1)

    # ------------------------------------------------------------------ :103-178
    def forward(self, context, image, caption, face_embeds=None, obj_embeds=None, metadata=None, names=None,
                attn_idx=None, encoded=None, caption_weights=None, per_image=1):
        refuse_weighted_forward(self, caption_weights, per_image)
        self._require_masks(context, caption)
        copy_masks = caption[self.index + '_copy_masks'][:, 1:]
        enc = encoded if encoded is not None else self.encode(context, image)
        caption_ids, target_ids, contexts = self._forward(context, image, caption, face_embeds, None, enc)
        decoder_out = self.decoder(caption, contexts)
        loss_sum, sample_size = self.criterion(self.decoder.adaptive_softmax, decoder_out, target_ids)
        gen_loss = loss_sum.detach().float() / sample_size / math.log(2)
        entity_loss, copy_loss = self.pointer_loss(decoder_out[0], context, copy_masks, target_ids, enc)
        entity_loss = entity_loss / math.log(2)
        copy_loss = copy_loss / math.log(2)
        loss = entity_loss + copy_loss
        # :118-128.  A NaN loss in training is left to the trainer, which skips the update on a device flag (no host
        # synchronisation here); outside training it is None, as in the reference
        if (self.training and not loss.requires_grad) or (not self.training and bool(torch.isnan(loss))):
            loss = None
        for key, value in (('gen_loss', gen_loss), ('entity_loss', entity_loss), ('copy_loss', copy_loss)):
            v = value.detach().float()
            self.batch_history[key] = self.batch_history[key] + torch.where(torch.isnan(v), torch.zeros_like(v), v)
        output_dict = {'loss': loss, 'sample_size': sample_size.reshape(())}
        if not self.training and self.evaluate_mode:
            decode = self._generate_pointer_cached if self.cached_generation else self._generate_pointer
            gen_ids, _, should_copy, _ = decode(caption_ids, contexts, enc, context)
            self._forward_generated(output_dict, gen_ids, [], metadata)
            ids = gen_ids.cpu()
            output_dict['copied_texts'] = [self.detokenize(x[should_copy[i].cpu()]) for i, x in enumerate(ids)]
        self.n_samples += caption_ids.shape[0]
        self.n_batches += 1
        return output_dict

    def pointer_loss(self, X, context, copy_masks, targets, enc):
        """:180-313 -> (entity_loss, copy_loss), each a scalar (constant zeros when no token is an entity)."""
        if not bool((copy_masks >= 1).any()):
            z = torch.zeros((), device=X.device)
            return z, z.clone()
        X = X.transpose(0, 1)                                                       # [T, B, E]
        X_entity = self.entity_attn(X)
        fc = self.entity_fc
        entity_loss, _ = ops.entity_head(X_entity, fc.weight_g, fc.weight_v, fc.bias, copy_masks)
        proper = context[self.index + '_proper_masks'].to(torch.int8)
        w = ops.copy_attention(self._copy_q(X), self._copy_k(self._article_2(enc)), self.bias_k, enc.article_mask,
                               proper, self.copy_heads, p=self.copy_dropout, training=self.training)
        copy_loss = ops.copy_loss(w, context[self.index], targets, copy_masks, self.COPY_VARIANT, self.vocab_size)
        return entity_loss, copy_loss

    # ------------------------------------------------------------------ :397-426, :427-696
    def generate(self, context, image, caption, face_embeds=None, obj_embeds=None, metadata=None, names=None,
                 attn_idx=None, beam_size=1, encoded=None, attention=False, n_best=1, prefix=None, n_samples=1,
                 rank_by='score', rank_len_penalty=0.0, banned=None, ground=None, guidance=None, guidance_drop=None, cached=None,
                 token_stats=0):
        """cached (None: the model's `cached_generation` key): the same greedy / nucleus decode through the cached generator -
        projected context K/V, a batch that keeps its shape, one captured step per token (_pointer_steps).  Everything refused
        below is refused on both paths.
        n_samples = n (2..16): only on the cached path and only for a model that samples
        (`sampling_topp`) - n draws per image, row b * n + j of the decode step draw j of image b, keyed (seed, b * n + j,
        step), ranked by rank_by / rank_len_penalty as for the plain models (section 21).  The keys of n = 1 then hold the
        first rank; added are 'gen_ids_samples' [B, n, L], 'log_probs_samples' [B, n, L - 1], 'scores_samples' [B, n],
        'sample_index' [B, n], 'duplicate' [B, n], 'scores' [B], 'should_copy_samples' [B, n, L] bool, 'copy_probs_samples'
        [B, n, L - 1] and 'generations_samples' / 'copied_texts_samples' (n strings per image), all in rank order.  On the eager
        path, or for a greedy model, n > 1 is refused as before.  n_samples = 1: exactly the call of before."""
        if token_stats:                                               # (refused on both paths: the copy decision is out of scope)
            from .stepper import TOKEN_STATS_REFUSALS
            raise ValueError('token_stats=%r: %s' % (token_stats, TOKEN_STATS_REFUSALS['copy']))
        if attention:
            self._check_attention(beam_size)
        self._check_mask_options(banned, ground, attention)           # (refused: the copy decision is out of scope)
        self._check_guidance(guidance, guidance_drop)                 # (gamma != 1 refused: the copy decision is out of scope)
        if prefix is not None:
            self._check_prefix(prefix, 0)                             # (refused: the copy decision is out of scope)
        self._check_beam(beam_size)
        self._check_options(beam_size, attention, n_best)
        # (the shells of the host tests never ran __init__: no key means the eager path)
        use_cached = getattr(self, 'cached_generation', False) if cached is None else bool(cached)
        # n > 1: the cached path of a sampling model only, refused like the prefix otherwise
        ns = self._check_n_samples(n_samples, rank_by, rank_len_penalty, beam_size, attention, cached=use_cached)
        self._require_masks(context)
        enc = encoded if encoded is not None else self.encode(context, image)
        caption_ids, _, contexts = self._forward(context, image, caption, face_embeds, None, enc)
        if ns is not None:
            return self._generate_samples(caption_ids, contexts, enc, context, ns)
        decode = self._generate_pointer_cached if use_cached else self._generate_pointer
        gen_ids, log_probs, should_copy, copy_probs = decode(caption_ids, contexts, enc, context)
        ids = gen_ids.cpu()
        return {'gen_ids': gen_ids, 'log_probs': log_probs, 'should_copy': should_copy, 'copy_probs': copy_probs,
                'generations': [self.detokenize(x[x > 1]) for x in ids],
                'copied_texts': [self.detokenize(x[should_copy[i].cpu()]) for i, x in enumerate(ids)]}

    @torch.no_grad()
    def _generate_samples(self, caption_ids, contexts, enc, context, ns):
        """generate(n_samples=n > 1, cached=True): ns = (n, rule, alpha) of _check_n_samples -> the result dict, every
        `_samples` key in rank order and the keys of n = 1 the first rank."""
        n = ns[0]
        _, _, _, _, smp = self._drive(self._pointer_steps(caption_ids, contexts, enc, context, n=n, rank=ns[1:]))
        ids, sc = smp['gen_ids_samples'].cpu(), smp['should_copy_samples'].cpu()
        out = dict(smp)
        out['generations_samples'] = [[self.detokenize(x[x > 1]) for x in img] for img in ids]
        out['copied_texts_samples'] = [[self.detokenize(x[sc[b, j]]) for j, x in enumerate(img)] for b, img in enumerate(ids)]
        out.update(gen_ids=smp['gen_ids_samples'][:, 0].contiguous(), log_probs=smp['log_probs_samples'][:, 0].contiguous(),
                   should_copy=smp['should_copy_samples'][:, 0].contiguous(),
                   copy_probs=smp['copy_probs_samples'][:, 0].contiguous(), scores=smp['scores_samples'][:, 0].contiguous(),
                   generations=[g[0] for g in out['generations_samples']],
                   copied_texts=[g[0] for g in out['copied_texts_samples']])
        return out

    @torch.no_grad()
    def _generate_pointer(self, caption_ids, contexts, enc, context, gen_len=100, eos=2):
        """-> (gen_ids [B, n+1], log_probs [B, n], should_copy [B, n+1] bool, copy_probs [B, n])."""
        B = caption_ids.shape[0]
        dev = caption_ids.device
        E = self.in_proj_weight.shape[1]
        k_article = self._copy_k(self._article_2(enc))                # [S, B, E], once per batch
        proper = context[self.index + '_proper_masks'].to(torch.int8).contiguous()
        ctx_ids = context[self.index].contiguous()
        art_mask = enc.article_mask
        hist = torch.full((B, gen_len + 1), -1, dtype=torch.int64, device=dev)    # copied ids, column 0 = the seed
        state = {}
        seed = caption_ids[:, 0:1]
        alive = seed[:, -1] != eos
        keep = alive
        cur = seed
        k_hist = v_hist = None
        log_probs, paths, copies, probs = [], [seed], [torch.ones(B, 1, dtype=torch.bool, device=dev)], []
        names = [k for k in contexts if not k.endswith('_mask') and not k.startswith('_')]
        ea = self.entity_attn
        sampling = self._sampling()                                   # (k, T, p) with sampling_topp, else None
        if sampling is not None:
            seed_word = torch.full((1,), draw_seed(), dtype=torch.int32, device=dev)
        for i in range(gen_len):
            self.decoder.filter_incremental_state(state, keep)
            ctx_i = {}
            for n in names:
                ctx_i[n] = contexts[n][:, alive]
                ctx_i[n + '_mask'] = contexts[n + '_mask'][alive]
            dec_out = self.decoder({self.index: cur[:, -1:]}, ctx_i, incremental_state=state)
            h = dec_out[0][:, -1:]                                                   # [Ba, 1, E]
            rows = alive.nonzero().squeeze(1).to(torch.int32)
            if sampling is None:
                gen_tok, lp = self.decoder.adaptive_softmax.greedy(h)
            else:                                                                    # keyed on the ORIGINAL batch rows
                gen_tok, lp = self.decoder.adaptive_softmax.sample(h, sampling[0], sampling[1], seed_word, i, row_ids=rows,
                                                                   topp=sampling[2])
            x = h.transpose(0, 1).contiguous()                                       # [1, Ba, E]
            k, v = ea.project_kv(x)
            if k_hist is not None:
                k_hist, v_hist = k_hist[:, keep], v_hist[:, keep]
                k_hist, v_hist = torch.cat([k_hist, k], 0), torch.cat([v_hist, v], 0)
            else:
                k_hist, v_hist = k, v
            x_entity = ea.step(x, k_hist, v_hist)
            fc = self.entity_fc
            ent = ops.entity_logits(x_entity, fc.weight_g, fc.weight_v, fc.bias)
            tok, copied, prob = ops.copy_step(self._copy_q(x[0]).contiguous(), k_article, self.bias_k, art_mask, proper,
                                              ctx_ids, rows, ent, gen_tok.reshape(-1).long(), hist, i + 1,
                                              self.copy_heads)
            full_lp = lp.new_zeros(B, 1)
            full_lp[alive] = lp.reshape(-1, 1).float() / self.sampling_temp        # :636-637 topk_lprobs / T
            full_ix = tok.new_full((B, 1), self.padding_idx)
            full_ix[alive] = tok.unsqueeze(1)
            full_cp = copied.new_zeros(B, 1)
            full_cp[alive] = copied.unsqueeze(1)
            full_pr = prob.new_zeros(B, 1)
            full_pr[alive] = prob.unsqueeze(1)
            log_probs.append(full_lp)
            paths.append(full_ix)
            copies.append(full_cp)
            probs.append(full_pr)
            keep = tok != eos
            alive = alive.clone()
            alive[alive.nonzero().squeeze(1)[~keep]] = False
            cur = torch.cat([cur, tok.unsqueeze(1)], dim=1)[keep]
            if int(keep.sum()) == 0:
                break
        return torch.cat(paths, -1), torch.cat(log_probs, -1), torch.cat(copies, -1), torch.cat(probs, -1)

    @torch.no_grad()
    def _generate_pointer_cached(self, caption_ids, contexts, enc, context, gen_len=100, eos=2, check_every=8):
        return self._drive(self._pointer_steps(caption_ids, contexts, enc, context, gen_len, eos, check_every))

    def _pointer_steps(self, caption_ids, contexts, enc, context, gen_len=100, eos=2, check_every=8, n=1, rank=('score', 0.0)):
        """_generate_pointer on the cached generator - a generator in the style of _greedy_steps (one `yield` per issued step or
        multi-step replay), same results.  The context K/V are projected once, the batch keeps its shape (finished rows are
        masked, never compacted), the entity K/V history and the copy bookkeeping are static buffers, and the step's tail -
        entity projections, tell_entity_attn_step, out_proj + LayerNorm, entity_fc, the copy query, tell_copy_decide and the
        unchanged tell_greedy_update - is the stepper's `post`: part of the captured single-step and multi-step graphs, with the
        step index from the device counter.  One host synchronisation per `check_every` steps and one at the end.  When the
        stepper is not static (graphs disabled) the same launches run one by one over buffers of this call.
        n > 1 (a sampling model; generate(n_samples=n)): R = images * n rows are resident, hypothesis j of
        image b in row b * n + j, as in _greedy_steps - cur, ids, lps, done_step, fin8, hist, copied, probs, tok, the entity K/V
        histories and the scratch are R rows tall; the contexts, the projected K/V and the copy buffers k_article, proper,
        ctx_ids and mask stay one row per image (the stepper's hyp = n; the copy decision's per_image = n,
        tell_copy_decide_hyp).  One seed, row r draws with (seed, r, step).  Behind the loop _rank_samples scores,
        de-duplicates and ranks; the result gains a fifth entry, the dict of the `_samples` keys in rank order.  n = 1
        allocates, keys, captures and launches exactly what it did before."""
        dec = self.decoder
        n = int(n)
        images = caption_ids.shape[0]
        B = images * n                                                       # decode rows
        dev = caption_ids.device
        E = self.in_proj_weight.shape[1]
        H = self.copy_heads
        kv = dec.project_contexts(contexts)
        sampling = self._sampling()
        step = self._decode_stepper(B, kv, contexts, gen_len, sample=sampling, hidden=True, hyp=n)
        k_src = self._copy_k(self._article_2(enc)).transpose(0, 1)           # [B, S, E], once per batch
        S, dtype = k_src.shape[1], k_src.dtype
        ea = self.entity_attn
        He, scaling = ea.attention.num_heads, ea.attention.attention_module.scaling

        def make_book():
            return dict(ids=torch.empty(B, gen_len + 1, dtype=torch.long, device=dev),
                        lps=torch.empty(B, gen_len, dtype=torch.float32, device=dev),
                        done_step=torch.empty(B, dtype=torch.long, device=dev), fin8=torch.empty(B, dtype=torch.uint8, device=dev))

        def make_copy():
            return dict(k_article=torch.empty(images, S, E, dtype=dtype, device=dev),
                        proper=torch.empty(images, S, dtype=torch.int8, device=dev),
                        ctx_ids=torch.empty(images, S, dtype=torch.long, device=dev),
                        mask=torch.empty(images, S, dtype=torch.uint8, device=dev),
                        hist=torch.empty(B, gen_len + 1, dtype=torch.int32, device=dev),
                        copied=torch.empty(B, gen_len + 1, dtype=torch.uint8, device=dev),
                        probs=torch.empty(B, gen_len, dtype=torch.float32, device=dev),
                        k_hist=torch.empty(gen_len, B, E, dtype=dtype, device=dev),
                        v_hist=torch.empty(gen_len, B, E, dtype=dtype, device=dev),
                        scratch=torch.empty(B, H, S, dtype=torch.float32, device=dev),
                        tok=torch.empty(B, dtype=torch.int32, device=dev))
        bk = step.book('greedy', make_book) if step.static else make_book()
        cp = step.book('pointer', make_copy) if step.static else make_copy()
        ids, lps, done_step, fin8 = bk['ids'], bk['lps'], bk['done_step'], bk['fin8']
        ops._check_rows('cached generation', (images, S), proper_masks=context[self.index + '_proper_masks'],
                        context_ids=context[self.index], article_mask=enc.article_mask)
        cp['k_article'].copy_(k_src)
        cp['proper'].copy_(context[self.index + '_proper_masks'])
        cp['ctx_ids'].copy_(context[self.index])
        if enc.article_mask is None:
            cp['mask'].zero_()
        else:
            cp['mask'].copy_(enc.article_mask)
        cp['hist'].fill_(-1)
        cp['copied'].zero_()
        cp['copied'][:, 0] = 1
        cp['probs'].zero_()
        cp['k_hist'].zero_()
        cp['v_hist'].zero_()
        k_article = cp['k_article'].transpose(0, 1)                          # the [S, images, E] view the kernel takes by strides
        ids.fill_(self.padding_idx)
        lps.zero_()
        done_step.fill_(gen_len)
        cur = caption_ids[:, 0:1].contiguous() if n == 1 else caption_ids[:, 0:1].repeat_interleave(n, dim=0).contiguous()
        finished = cur[:, 0] == eos
        ids[:, 0] = cur[:, 0]
        done_step[finished] = 0
        fin8.copy_(finished)
        if sampling is not None:
            step.seed.fill_(draw_seed())
        next_cur = step.cur if step.static else torch.empty(B, 1, dtype=torch.long, device=dev)
        next_cur.copy_(cur)
        inv_temp = 1.0 / float(self.sampling_temp)
        fc = self.entity_fc

        def post(out, i, step_dev):
            gen_tok, lp, x = out
            xt = x.transpose(0, 1)                                           # [1, B, E]
            k_new, v_new = ea.project_kv(xt)
            attn = ops.entity_attn_step(ea.in_proj_q(xt)[0], k_new[0], v_new[0], cp['k_hist'], cp['v_hist'], He, scaling, i,
                                        step_dev)
            x_entity = ea._finish(attn.unsqueeze(0), xt)
            ent = ops.entity_logits(x_entity, fc.weight_g, fc.weight_v, fc.bias)
            ops.copy_decide(self._copy_q(xt[0]), k_article, self.bias_k, cp['mask'], cp['proper'], cp['ctx_ids'], ent,
                            gen_tok.reshape(B), fin8, cp['hist'], cp['copied'], cp['probs'], i, H, cp['scratch'], cp['tok'],
                            step_dev, per_image=n)
            # the bookkeeping of the plain greedy decode, on the copy decision's token; the log-prob stays the generator's
            ops.call('tell_greedy_update', cp['tok'], lp.reshape(B), fin8, ids, ids.stride(0), lps, lps.stride(0), done_step,
                     next_cur, B, int(i), int(eos), inv_temp, step.counter_out, step_dev)
        if step.static:
            yield from step.steps(gen_len, check_every, post, fin8)
        else:
            for i in range(gen_len):
                step(i, next_cur, post=post)
                yield i
                if (i + 1) % check_every == 0 and bool(fin8.all()):
                    break
        steps = max(int(done_step.max()), 1)                                  # one sync at the end
        if n > 1:
            lp0, ids0, info = self._rank_samples(ids, lps, done_step, images, n, steps, gen_len, eos, rank)
            smp = dict(info.samples)
            order = smp['sample_index']

            def ranked(t):                                                    # [R, W] -> [images, n, W] by the same order
                t = t.reshape(images, n, -1)
                return t.gather(1, order.unsqueeze(-1).expand(-1, -1, t.shape[-1]))
            smp['should_copy_samples'] = ranked(cp['copied'][:, :steps + 1]).bool()
            smp['copy_probs_samples'] = ranked(cp['probs'][:, :steps])
            return (ids0, lp0, smp['should_copy_samples'][:, 0].contiguous(), smp['copy_probs_samples'][:, 0].contiguous(), smp)
        return (ids[:, :steps + 1].clone(), lps[:, :steps].clone(), cp['copied'][:, :steps + 1].bool(),
                cp['probs'][:, :steps].clone())

    def get_metrics(self, reset=False):
        metrics = super().get_metrics(reset=False)
        for key, value in self.batch_history.items():
            metrics[key] = float(value) / max(self.n_batches, 1)
        if reset:
            super().get_metrics(reset=True)
            self.batch_history = defaultdict(float)
        return metrics


@Model.register('transformer_pointer')
class TransformerPointerModel(PointerModelBase):
    """tell/models/transformer_pointer.py: copy_loss = sum_i mean over rows of entity index i of -log p_target."""
    COPY_VARIANT = 1


@Model.register('transformer_pointer_2')
class TransformerPointer2Model(PointerModelBase):
    """tell/models/transformer_pointer_2.py: each term is CrossEntropy over the batch's reduced vocabulary."""
    COPY_VARIANT = 2
