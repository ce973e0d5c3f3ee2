"""tell/models/transformer_faces_objects.py:23-517 and tell/models/transformer_flattened.py:24-443
on the MI355X path (training forward + loss, greedy generation)."""
import os
from collections import defaultdict

import torch
import torch.nn as nn

from .. import graphs, ops, streams
from ..common.registrable import Registrable
# (the option code and the host definitions live in gen_options.py / definitions.py; their names stay importable from here)
from .definitions import (_id_order_draw, advantage_definition, caption_reward_definition, minp_definition,  # noqa: F401
                          nucleus_definition, sample_rank_definition, token_stats_definition, typical_definition)
from .gen_options import (DEFAULT_GEN_LEN, GUIDANCE_CONTEXTS, MAX_N_SAMPLES, MAX_NO_REPEAT_NGRAM,  # noqa: F401
                          MAX_SAMPLING_TOPK, MIN_ALLOWED_TOKENS, PENALTY_KEYS, RANK_BY, TOKEN_STATS_KEYS, AttnMaps, AttnMapsStats,
                          DecodeInfo, DecodePlan, OptionChecks, check_beam_options, check_caption_weights, check_guidance,
                          check_mask_keys, check_n_samples, check_penalties, check_per_image, check_prefix, check_sampling,
                          check_token_stats, check_vocab_mask, draw_seed, encode_prefix, guided_batch, inv_norm_table,
                          token_stats_neutral)
from .stepper import TOKEN_STATS_REFUSALS, DecodeStepper

_OVERLAP = os.environ.get('TELL_ENCODER_OVERLAP', '1') != '0'
# where the PREFETCHED ResNet pass of the next batch is enqueued: 'own' = its side stream (three streams share the chip),
# 'main' = the training stream, in front of the decoder step of the current batch (two streams: RoBERTa against ResNet +
# decoder back to back - 4.3 + 6.7 ms against 11.2 ms alone).  MEASURED in round 6: tools/step_timeline.py, DESIGN.md.
_RESNET_STREAM = os.environ.get('TELL_RESNET_STREAM', 'own')
def _side_stream(device, name='resnet'):
    return streams.get(name, device)


class EncodedBatch:
    """Outputs of the frozen encoders for one batch (CaptionModel.encode), possibly still in flight on the
    encoder streams."""

    def __init__(self):
        self.stack = self.x_image = self.article_mask = None
        self.events = []
        self.static = False      # stack / x_image are graph-owned static buffers (stable addresses across steps)
        self.slots = []          # (graph slot, generation at production): a later replay of the slot overwrites the data

    def stale(self):
        """True when a graph replay issued after this batch was encoded has reused one of its output buffers."""
        return any(s.get('generation') != g for s, g in self.slots)

    def wait(self):
        """Join the producing streams into the current stream (idempotent)."""
        if self.events:
            cur = torch.cuda.current_stream()
            for ev in self.events:
                cur.wait_event(ev)
            self.events = []
            for t in (self.x_image, self.article_mask, self.stack):
                for u in (t if isinstance(t, (list, tuple)) else (t,)):
                    if torch.is_tensor(u) and u.is_cuda:
                        u.record_stream(cur)


class Model(nn.Module, Registrable):
    """Stand-in for allennlp.models.Model (forward(**batch) -> dict with 'loss')."""

    def __init__(self, vocab=None):
        super().__init__()
        self.vocab = vocab

    def get_metrics(self, reset=False):
        return {}

    def decode(self, output_dict):
        return output_dict


def refuse_weighted_forward(model, caption_weights=None, per_image=1):
    """The models outside the weighted / per-image training pass (copy, GloVe, LSTM) say so by name."""
    if caption_weights is not None or per_image != 1:
        raise ValueError('%s does not take caption_weights / per_image: the weighted training pass (self-critical '
                         'training) covers the transformer_faces_objects family only' % type(model).__name__)


def set_sampling(model, sampling_topk, sampling_temp, sampling_topp=None, sampling_minp=None, sampling_typical=None):
    """check_sampling, kept on the model: sampling_topk / _temp / _topp / _minp / _typical."""
    model.sampling_topk, model.sampling_temp = check_sampling(sampling_topk, sampling_temp, sampling_topp, sampling_minp,
                                                              sampling_typical)[:2]
    model.sampling_topp = None if sampling_topp is None else float(sampling_topp)
    model.sampling_minp = None if sampling_minp is None else float(sampling_minp)
    model.sampling_typical = None if sampling_typical is None else float(sampling_typical)


class CaptionModel(OptionChecks, Model):
    USE_FACES_OBJECTS = False
    EVAL_ATTENTION = True        # forward() in evaluate mode honours `eval_attention` (commands/evaluate.py attention_maps=True)
    EXTRA_CONTEXTS = ()          # which of ('faces', 'obj') the model feeds to its decoder

    def __init__(self, vocab, decoder, criterion, evaluate_mode=False, attention_dim=1024, hidden_size=1024,
                 dropout=0.1, vocab_size=50264, model_name='roberta-base', namespace='bpe', index='roberta',
                 padding_value=1, use_context=True, sampling_topk=1, sampling_temp=1.0, weigh_bert=False,
                 initializer=None, resnet=None, roberta=None, n_bert_layers=25, sampling_topp=None,
                 beam_len_penalty=0.0, no_repeat_ngram_size=0, min_len=0, sampling_minp=None, sampling_typical=None,
                 repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, suppress_tokens=(),
                 ground_names=False, guidance_scale=1.0, guidance_drop=('image',)):
        super().__init__(vocab)
        self.decoder, self.criterion = decoder, criterion
        self.index, self.namespace = index, namespace
        if resnet is None:
            from .resnet import resnet152
            resnet = resnet152()
        if roberta is None:
            from .roberta import roberta_large
            roberta = roberta_large()
        self.resnet, self.roberta = resnet, roberta
        self.use_context = use_context
        self.padding_idx = padding_value
        self.evaluate_mode = evaluate_mode
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
        self.guidance_scale, self.guidance_drop = check_guidance(guidance_scale, guidance_drop)
        self._check_guidance()
        self.weigh_bert = weigh_bert
        if weigh_bert:
            self.bert_weight = nn.Parameter(torch.rand(n_bert_layers))      # nn.init.uniform_, :57-59
        self.n_batches = 0
        self.n_samples = 0
        self.sample_history = defaultdict(float)
        # captured encoder / decode graphs bake in the addresses of working copies of the weights: anything that can
        # re-home those copies (a checkpoint load, a trainer re-flagging requires_grad) drops the captures
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.reset_graphs())

    def name_tokens(self):
        """The grounded class of generate(ground=True): data.bpe.capitalised_tokens over the installed roberta-base vocabulary -
        bool [vocab], the BPE pieces that start a capitalised word (per token, not per word: continuation pieces are
        unconstrained).  Cached; FileNotFoundError when the vocabulary files are absent."""
        cls = self.__dict__.get('_name_tokens')
        if cls is None:
            from ..data.bpe import RobertaBPE, capitalised_tokens
            from ..data.indexers import bpe_directory
            cls = capitalised_tokens(RobertaBPE(bpe_directory()))
            V = int(self.decoder.adaptive_softmax.vocab_size)
            full = torch.zeros(V, dtype=torch.bool)
            full[:min(V, cls.numel())] = cls[:V]
            cls = self.__dict__['_name_tokens'] = full
        return cls

    def _vocab_mask(self, context, banned=None, ground=None, attention=False, eos=2):
        """The vocabulary mask of one caption batch, from generate's arguments and the model's `suppress_tokens` /
        `ground_names`: -> None when nothing is set (the default path reads nothing of the batch), else (ctx_ids int64 [B, S] -
        the article ids context[self.index] -, cls_bits int32 [words] or None, deny8 uint8 [1 or B, V] or None), what
        DecodeStepper.set_mask takes.  check_vocab_mask and _check_mask_options apply."""
        used = self._check_mask_options(banned, ground, attention)
        if not used:
            return None
        ctx_ids = context[self.index]
        if ground is True or (ground is None and 'ground_names' in used):
            ground = self.name_tokens()
        if ground is False:
            ground = None
        V = int(self.decoder.adaptive_softmax.vocab_size)
        deny, cls = check_vocab_mask(banned, ground, V, ctx_ids.shape[0], eos,
                                     suppress=getattr(self, 'suppress_tokens', ()) or ())
        dev = ctx_ids.device
        cls_bits = None if cls is None else ops.pack_mask_bits(cls).to(dev)
        deny8 = None if deny is None else deny.to(device=dev, dtype=torch.uint8).contiguous()
        return ctx_ids, cls_bits, deny8

    @staticmethod
    def _attn_output(out, attns):
        """'attns' (+ 'attn_steps') of an output dict from a generator's third result: an AttnMaps, or the plain list."""
        if isinstance(attns, AttnMaps):
            out['attns'], out['attn_steps'] = attns.maps, attns.steps
        else:
            out['attns'] = [] if isinstance(attns, DecodeInfo) else attns
        if torch.is_tensor(out.get('log_probs')):
            # 'scores': the hypothesis' score - the (tempered) log-prob sum; beam search: normalised by beam_len_penalty
            info = attns if isinstance(attns, DecodeInfo) else None
            out['scores'] = info.scores if info is not None and info.scores is not None else out['log_probs'].sum(-1)
            if info is not None and info.nbest is not None:
                out['gen_ids_nbest'], out['log_probs_nbest'], out['scores_nbest'] = info.nbest
            if info is not None and info.samples is not None:
                out.update(info.samples)
        if getattr(attns, 'token_stats', None) is not None:
            out.update(attns.token_stats)
        return out

    def reset_graphs(self):
        """Forget every captured hipGraph of this model (encoders, decode steps); they are re-recorded on next use."""
        for k in ('_resnet_graph', '_roberta_graph'):
            g = self.__dict__.get(k)
            if g is not None:
                g.reset()
        self.__dict__.pop('_decode_graphs', None)
        self.__dict__.pop('_decode_graphs_stamp', None)

    def set_capture_after(self, n):
        """Sightings of an input shape before the encoder graphs capture it (graphs.CAPTURE_AFTER by default)."""
        self.__dict__['_capture_after'] = n
        self.reset_graphs()
        for k in ('_resnet_graph', '_roberta_graph'):
            self.__dict__.pop(k, None)

    def _run_resnet(self, image, slot=None):
        """The frozen trunk as one hipGraph replay per step (graphs.GraphedCall); eager for the first call."""
        from .resnet import ResNetFeatureExtractor
        if not isinstance(self.resnet, ResNetFeatureExtractor):      # a user-supplied trunk: no assumptions
            return self.resnet(image)
        g = self.__dict__.get('_resnet_graph')
        if g is None:
            g = self.__dict__['_resnet_graph'] = graphs.GraphedCall(self.resnet, 'resnet152',
                                                                    capture_after=self.__dict__.get('_capture_after'))
        w = self.resnet.conv1.weight                 # a reloaded / moved / re-typed trunk must not replay stale pointers
        from .resnet import stats_epoch
        # (eval captures bake in weights folded with the running statistics: a train-mode pass in between retires them)
        return g(image, key=(self.resnet.training, ops.rt.compute_dtype(), w._version, w.data_ptr(),
                             0 if self.resnet.training else stats_epoch()), slot=slot)

    def _run_roberta(self, article_ids, slot=None):
        """RoBERTa-large (~170 launches, dropout active in train mode) as one hipGraph replay per step."""
        from .roberta import RobertaEncoder
        if not isinstance(self.roberta, RobertaEncoder):
            return self.roberta.extract_features(article_ids, return_all_hiddens=True)
        g = self.__dict__.get('_roberta_graph')
        if g is None:
            g = self.__dict__['_roberta_graph'] = graphs.GraphedCall(
                lambda ids: self.roberta.extract_features(ids, return_all_hiddens=True), 'roberta-large', rng=True,
                capture_after=self.__dict__.get('_capture_after'))
        w = self.roberta.model.decoder.sentence_encoder.layers[0].fc1.weight
        return g(article_ids, key=(self.roberta.training, ops.rt.compute_dtype(), w._version, w.data_ptr()), slot=slot)

    # ---- frozen encoders -------------------------------------------------------------
    def encode(self, context, image, ahead=False):
        """ResNet-152 + RoBERTa-large on one batch (transformer_faces_objects.py:335-353) -> EncodedBatch.

        The two encoders are independent and read no trainable weight.  ahead=False: RoBERTa runs on the current
        stream, ResNet's many small launches on a side stream underneath RoBERTa's chip-filling GEMMs
        (TELL_ENCODER_OVERLAP=0 serialises them).  ahead=True: both run on their own streams and the call returns
        at once - the trainer uses it to encode batch N+1 underneath the latency-bound decoder forward /
        backward / optimizer of batch N; `EncodedBatch.wait()` joins them into the consumer's stream."""
        with torch.no_grad():
            main = torch.cuda.current_stream()
            article_ids = context[self.index]
            enc = EncodedBatch()
            # both encoder graphs replay into the buffer set of this call's parity: consecutive batches never share a
            # buffer, and the addresses the decoder step graph is keyed on depend on the parity alone (graphs.py)
            par = self.__dict__['_enc_parity'] = self.__dict__.get('_enc_parity', -1) + 1
            if ahead:
                rs = _side_stream(image.device, 'roberta')
                is_ = main if _RESNET_STREAM == 'main' else _side_stream(image.device, 'resnet')
                start = torch.cuda.Event()
                start.record(main)
                rs.wait_event(start)
                if is_ is not main:
                    is_.wait_event(start)
                with torch.cuda.stream(rs), ops.hip.bound_stream():
                    enc.article_mask = self._pad_mask(article_ids)                      # :347
                    enc.stack = self._run_roberta(article_ids, par)
                    article_ids.record_stream(rs)
                    enc.events.append(torch.cuda.Event())
                    enc.events[-1].record(rs)
                with torch.cuda.stream(is_), ops.hip.bound_stream():
                    enc.x_image = self._run_resnet(image, par)
                    image.record_stream(is_)
                    enc.events.append(torch.cuda.Event())
                    enc.events[-1].record(is_)
                enc.static = self._encoders_replayed()
                self._note_slots(enc)
                return enc
            side = _side_stream(image.device, 'resnet') if _OVERLAP else None
            enc.article_mask = self._pad_mask(article_ids)                              # :347
            if side is not None:
                start = torch.cuda.Event()
                start.record(main)
            # RoBERTa is issued FIRST: its ~300 launches keep the main stream busy for ~10 ms of GPU time
            # while the host is still issuing ResNet's small launches onto the side stream.
            enc.stack = self._run_roberta(article_ids, par)                                   # [L,B,S,E]
            if side is not None:
                side.wait_event(start)
                with torch.cuda.stream(side), ops.hip.bound_stream():
                    enc.x_image = self._run_resnet(image, par)             # [B,49,2048] (NHWC == :335-341)
                    enc.events.append(torch.cuda.Event())
                    enc.events[-1].record(side)
            else:
                enc.x_image = self._run_resnet(image, par)
            enc.static = self._encoders_replayed()
            self._note_slots(enc)
            return enc

    def _encoders_replayed(self):
        return all(getattr(self.__dict__.get(k), 'last_replayed', False) for k in ('_resnet_graph', '_roberta_graph'))

    def _note_slots(self, enc):
        for k in ('_resnet_graph', '_roberta_graph'):
            g = self.__dict__.get(k)
            if g is not None and getattr(g, 'last_replayed', False):
                enc.slots.append((g.last_slot, g.last_slot['generation']))

    def _pad_mask(self, ids):
        """Key-padding mask of the article (:347).  On the GPU as the uint8 the attention kernels read - produced once,
        inside the encoder graph - instead of a bool that every decoder call converts."""
        m = ids == self.padding_idx
        return m.to(torch.uint8) if ids.is_cuda else m

    def _no_mask(self, B, P, device):
        """The all-visible mask of the image regions (:371): a constant, built once per shape."""
        cache = self.__dict__.setdefault('_no_mask_cache', {})
        key = (B, P, str(device))
        if key not in cache:
            cache[key] = torch.zeros(B, P, dtype=torch.uint8 if torch.device(device).type == 'cuda' else torch.bool,
                                     device=device)
        return cache[key]

    # ---- :311-397 -----------------------------------------------------------------
    def _forward(self, context, image, caption, face_embeds=None, obj_embeds=None, encoded=None, per_image=1):
        """per_image = n: `caption` holds n captions for each of the B images (caption b * n + j belongs to image b); every
        context and its mask is repeated n times along the batch axis AFTER the encoders and the layer mix - one encode for
        the n captions, and autograd sums the mix's gradient over them."""
        dtype = ops.rt.compute_dtype()
        cap = caption[self.index]
        plain = type(per_image) is int and per_image == 1                  # (the default reads nothing more of the batch)
        n_per = 1 if plain else check_per_image(per_image, cap.shape[0], image.shape[0])
        target_ids = cap[:, 1:].contiguous()                               # :321-328
        caption_ids = cap[:, :-1].contiguous()
        caption[self.index] = caption_ids                                  # :329

        enc = encoded if encoded is not None else self.encode(context, image)   # frozen encoders (config :150-152)
        enc.wait()
        stack, x_image, article_mask = enc.stack, enc.x_image, enc.article_mask
        B, P, _ = x_image.shape
        ops.rt.wait_weight_update()      # everything below reads trainable weights (the encoders above do not)
        if self.weigh_bert:
            x_article = ops.mix_layers(stack, self.bert_weight)            # :355-364
        else:
            x_article = stack[-1]
        if n_per > 1:
            B = B * n_per
            x_image, x_article, article_mask = (t.repeat_interleave(n_per, dim=0) for t in (x_image, x_article, article_mask))
            face_embeds, obj_embeds = (None if t is None else t.repeat_interleave(n_per, dim=0)
                                       for t in (face_embeds, obj_embeds))
        contexts = {
            'image': x_image.transpose(0, 1),
            'image_mask': self._no_mask(B, P, image.device),                  # :371
            'article': x_article.transpose(0, 1),
            'article_mask': article_mask,
        }
        if self.EXTRA_CONTEXTS:                                            # :373-379
            for key, emb in (('faces', face_embeds), ('obj', obj_embeds)):
                if key not in self.EXTRA_CONTEXTS:
                    continue
                Bf, n, dim = emb.shape
                if n == 0 or dim == 0:
                    contexts[key] = emb.new_zeros(n, Bf, dim).to(dtype)
                    contexts[key + '_mask'] = torch.zeros(Bf, n, dtype=torch.bool, device=emb.device)
                    continue
                clean = torch.empty(Bf, n, dim, dtype=dtype, device=emb.device)
                mask = torch.empty(Bf, n, dtype=torch.uint8, device=emb.device)
                ops.call('tell_nan_rows', emb.float().contiguous(), Bf * n, dim, clean, ops.hip.dt(dtype), mask)
                contexts[key] = clean.transpose(0, 1)
                contexts[key + '_mask'] = mask if mask.is_cuda else mask.bool()    # (uint8 is what the kernels read)
        return caption_ids, target_ids, contexts

    # ---- :67-140 ------------------------------------------------------------------
    def forward(self, context, image, caption, face_embeds=None, obj_embeds=None, metadata=None, names=None,
                attn_idx=None, encoded=None, caption_weights=None, per_image=1):
        """encoded: optional EncodedBatch of THIS batch produced earlier by `encode(..., ahead=True)`.
        caption_weights: fp32 [rows] or [rows, T] on the captions' device, T = caption length - 1 - the
        loss becomes sum_r sum_t w_rt * -log p(y_rt) over the number of non-pad targets (still bits per token) and every
        token's gradient carries its weight; not differentiated.  A per-row advantage (Trainer.train_self_critical), a mask
        that keeps a forced prefix out of the loss, a weight on entity tokens.  None: exactly the call of before.
        per_image = n: the batch holds B images and B * n captions, caption b * n + j for image b: one pass of the encoders
        and of the layer mix, their outputs repeated n times for the decoder.  1: exactly the call of before."""
        if not hasattr(getattr(self, 'decoder', None), 'project_contexts'):          # an LSTM decoder behind this class
            refuse_weighted_forward(self, caption_weights, per_image)
        output_dict, caption_ids, contexts = self._forward_loss(context, image, caption, face_embeds, obj_embeds, encoded,
                                                                caption_weights, per_image)
        if not self.training and self.evaluate_mode:                       # :92-116
            # (eval_attention: commands/evaluate.py's opt-in - the captions come with their attention maps)
            attention = bool(getattr(self, 'eval_attention', False))
            vm = self._vocab_mask(context, attention=attention)
            guide = self._check_guidance(attention=attention)
            _, gen_ids, attns = self._generate(caption_ids, contexts, beam_size=getattr(self, 'eval_beam_size', 1),
                                               attention=attention, vmask=vm, guide=guide)
            self._forward_generated(output_dict, gen_ids, attns, metadata)
        self.n_samples += caption_ids.shape[0]
        self.n_batches += 1
        return output_dict

    def _forward_loss(self, context, image, caption, face_embeds=None, obj_embeds=None, encoded=None, caption_weights=None,
                      per_image=1):
        """:67-88 - encoders, teacher-forced decoder pass, loss in bits per token -> (output_dict, caption_ids, contexts)."""
        caption_ids, target_ids, contexts = self._forward(context, image, caption, face_embeds, obj_embeds, encoded,
                                                          per_image)
        decoder_out = self.decoder(caption, contexts)
        if caption_weights is None:
            loss_sum, sample_size = self.criterion(self.decoder.adaptive_softmax, decoder_out, target_ids)
        else:
            loss_sum, sample_size = self.criterion(self.decoder.adaptive_softmax, decoder_out, target_ids,
                                                   row_weight=check_caption_weights(caption_weights, target_ids))
        loss = ops.loss_bits(loss_sum, sample_size)                        # :85-88, bits per token
        return {'loss': loss, 'sample_size': sample_size.reshape(())}, caption_ids, contexts

    def _forward_generated(self, output_dict, gen_ids, attns, metadata):
        """:92-116 - what evaluate mode adds to the output once the captions are decoded: ids, text, per-sample BLEU."""
        ids_cpu = gen_ids.cpu()
        output_dict['gen_ids'] = ids_cpu.numpy()
        self._attn_output(output_dict, attns)
        gen_texts = [self.detokenize(x[x > 1]) for x in ids_cpu]        # :96 "we ignore <s> and <pad>"
        output_dict['generations'] = gen_texts
        if metadata is not None:
            captions = [m.get('caption') or '' for m in metadata]
            output_dict['captions'] = captions
            output_dict['metadata'] = metadata
            import re
            from ..metrics import BleuScorer
            gens = [re.sub(r'[^\w\s]', '', t) for t in gen_texts]       # :105-106 remove punctuation
            refs = [re.sub(r'[^\w\s]', '', t) for t in captions]
            for gen, ref in zip(gens, refs):                            # :108-116
                scorer = BleuScorer(n=4)
                scorer += (gen, [ref])
                score, _ = scorer.compute_score(option='closest')
                for k in range(4):
                    self.sample_history['bleu-%d' % (k + 1)] += score[k] * 100

    def detokenize(self, ids):
        """`self.roberta.decode(ids)` of the reference (:96): BPE ids -> text.  Uses the encoder's own `decode` when it
        has one (a fairseq hub model), else the byte-level BPE of the data plane when its files are installed
        (data/indexers.bpe_directory), else the ids themselves as space-separated words (synthetic data has no text)."""
        dec = getattr(self.roberta, 'decode', None)
        if callable(dec):
            try:
                return dec(ids)
            except Exception:                                   # noqa: BLE001 - fall through to the local tokenizer
                pass
        bpe = self.__dict__.get('_bpe')
        if bpe is None:
            from ..data.bpe import RobertaBPE
            from ..data.indexers import bpe_directory
            try:
                bpe = RobertaBPE(bpe_directory())
            except FileNotFoundError:
                bpe = False
            self.__dict__['_bpe'] = bpe
        if bpe:
            return bpe.decode(ids)
        return ' '.join(str(int(i)) for i in ids if int(i) != 2)

    def generate(self, context, image, caption, face_embeds=None, obj_embeds=None, metadata=None, names=None,
                 attn_idx=None, beam_size=1, encoded=None, attention=False, n_best=1, prefix=None, n_samples=1,
                 rank_by='score', rank_len_penalty=0.0, banned=None, ground=None, guidance=None, guidance_drop=None,
                 token_stats=0):
        """encoded: optional EncodedBatch of THIS batch produced earlier by `encode(..., ahead=True)`.
        token_stats = n (0..8; per-token statistics): every step of the cached generator also leaves, for
        the token it took, the n best tokens of the MODEL'S OWN distribution (no temperature, penalty, mask), the token's rank in
        it (0 = the arg-max), its log-prob and the distribution's entropy in nats - one more launch behind the pick, inside the
        captured step.  Adds, with steps = gen_ids.shape[1] - 1: 'alt_ids' int64 [B, steps, n], 'alt_log_probs' fp32 [B, steps,
        n], 'token_rank' int64 [B, steps], 'token_entropy' fp32 [B, steps], 'token_model_lp' fp32 [B, steps]; positions behind a
        row's </s> hold pad, 0, -1, 0, 0.  With n_samples > 1 also their '_samples' forms [B, n_samples, steps, ...] in rank
        order (the plain keys are the first rank).  Greedy and every sampling rule, with the search options, penalties, masks,
        a prefix and attention maps; refused for beam search / n_best and guidance.  0: exactly the call of before.
        guidance = gamma / guidance_drop = names (context guidance; None: the model's `guidance_scale` /
        `guidance_drop`): every step is decoded twice in one static batch - with all contexts, and with the contexts in
        `guidance_drop` (out of image / article / faces / obj) fully masked - and the pick follows
        s = lp_c + (gamma - 1) * (lp_c - lp_u), reported as the normalised log-prob s - logsumexp(s): gamma > 1 rewards the
        tokens the dropped contexts made more likely, 0 <= gamma < 1 interpolates towards the decode without them.  Greedy and
        beam search (with beam_len_penalty and n_best); 'log_probs' / 'scores' then hold the guided log-probs.  gamma = 1.0:
        exactly the call of before.
        banned / ground (vocabulary masks): banned - bool [V] or [B, V] - lists tokens no caption (of
        that row) may contain; ground - bool [V], or True for `name_tokens()`, the BPE pieces that start a capitalised word -
        is a class of tokens that may be generated only if they occur in the row's own article context[index] (the class is per
        token, not per word: continuation pieces are unconstrained).  The model's `suppress_tokens` joins `banned`,
        `ground_names` means ground=True.  A masked token is never picked - greedy, beam search (with its search options and
        n_best) and top-k sampling (with n_samples), with or without a prefix; every reported log-prob is the model's own
        (nothing is renormalised), </s> is always allowed, a forced prefix token still wins.  None / None with the model's keys
        at their defaults: exactly the call of before.
        n_samples = n (2..16; a sampling model): n draws per image from ONE pass of the encoders and ONE
        cached context - row b * n + j of the decode step is draw j of image b, keyed (seed, b * n + j, step): under the same
        torch.manual_seed the draws of the batch with every image repeated n times.  Adds 'gen_ids_samples' [B, n, L],
        'log_probs_samples' [B, n, L - 1], 'scores_samples' [B, n] in rank order, 'sample_index' [B, n] (the draw in every rank
        slot) and 'duplicate' [B, n] bool (an earlier draw of the image has the same tokens); 'gen_ids' / 'log_probs' /
        'scores' are the first rank.  rank_by: 'draw' (draw order, duplicates flagged only), 'score' (sum of the recorded
        log-probs * len ** -rank_len_penalty, best first) or 'consensus' (mean bigram overlap with the other draws); with the
        last two every duplicate ranks behind every non-duplicate (tell_sample_rank).  A prefix row is shared by the n
        hypotheses of its image.  n_samples = 1: exactly the call of before.
        prefix (caption completion): int64 [B, P], the tokens every caption starts with after <s>,
        right-padded with padding_idx (`check_prefix`; `encode_prefix` builds it from strings).  Row r's first plen[r] steps take
        the prefix token instead of the model's pick - inside the decode step, every mode of the cached generators - and
        report the model's log-prob of it; 'gen_ids' is <s>, the prefix, the generated rest, 'log_probs' has one entry per
        step (forced steps: the teacher-forced log-probs), 'prefix_len' [B] is plen.  None: exactly the launches of before.
        'scores' [B]: the score of every caption (sum of its log-probs; beam search with `beam_len_penalty` alpha: * len ** -alpha).
        With `repetition_penalty` / `presence_penalty` / `frequency_penalty` set every pick is taken over
        penalised scores s = min(lp, 0) * theta - (alpha + beta * count) for the tokens the caption already holds, and
        'log_probs' / 'scores' (and their n-best forms) then hold THOSE SCORES, not log-probs - the convention of the
        generators that introduced these penalties; forced prefix steps still report the model's own log-prob.
        n_best = n (2..beam_size): also 'gen_ids_nbest' [B, n, L], 'log_probs_nbest' [B, n, L - 1], 'scores_nbest' [B, n] - the
        n best hypotheses of the beam, best first ('gen_ids' / 'log_probs' stay hypothesis 0).
        attention=True (greedy / top-k / nucleus, DynamicConv decoders): 'attns' is a dict name -> fp32 device tensor
        [B, steps, n_layers, S_name + 2] of head-averaged attention weights, one row per generated token and decoder layer
        (steps = gen_ids.shape[1] - 1; columns: the S context positions, the learned bias_k key, the zero key), and
        'attn_steps' [B] is the number of steps a row took part in, THE STEP THAT PRODUCED ITS </s> INCLUDED (= the column of
        </s> in gen_ids; `steps` for a row that never ended): maps[b, :attn_steps[b] - 1] are the steps of the words of an ended
        row, maps[b, attn_steps[b]:] what the static batch computed after it.  The tokens and log-probs are bit for bit those of attention=False.  `caption_attention` turns the maps into the
        reference's per-word view.  Default: 'attns' is [] on the cached generators."""
        # (prefix=None reads nothing of the batch here: the default path is the path of before)
        plan = self._plan(beam_size, attention, n_best, prefix, n_samples, rank_by, rank_len_penalty, banned, ground, guidance,
                          guidance_drop, token_stats, context, None if prefix is None else caption[self.index].shape[0])
        caption_ids, _, contexts = self._forward(context, image, caption, face_embeds, obj_embeds, encoded)
        return self._generated(plan, *self._generate(caption_ids, contexts, attn_idx, **plan.keywords()))

    def _generated(self, plan, log_probs, gen_ids, attns):
        """generate's output dict from a generator's three results."""
        out = self._attn_output({'gen_ids': gen_ids, 'log_probs': log_probs}, attns)
        if plan.prefix is not None:
            out['prefix_len'] = plan.prefix[1].to(gen_ids.device, torch.long)
        return out

    @torch.no_grad()
    def score_captions(self, batch, token_stats=0):
        """token_stats = n (1..8): also the five per-token arrays of generate(token_stats=n) for the batch's own captions -
        'alt_ids' / 'alt_log_probs' [B, T - 1, n], 'token_rank' / 'token_entropy' / 'token_model_lp' [B, T - 1]: where the model
        ranks every reference token, what it would have preferred and how flat its distribution was; neutral values (pad, 0,
        -1, 0, 0) behind a row's </s>.  They come from the same launch as generate's (the forced-prefix path).
        How likely the model finds the batch's OWN captions: the caption after <s>, its </s> included, is forced token by
        token through the greedy cached generator (generate(prefix=...)).  -> {'log_probs' [B, T - 1]: the teacher-forced
        log-prob of every caption token (0 behind a row's </s>), 'scores' [B]: their sum, 'prefix_len' [B]: tokens scored}.
        The captions may be at most gen_len (100) tokens long."""
        cap = batch['caption'][self.index]
        prefix = cap[:, 1:].contiguous()
        f = {k: (dict(v) if isinstance(v, dict) else v) for k, v in batch.items()
             if k in ('context', 'image', 'caption', 'face_embeds', 'obj_embeds', 'encoded')}
        n_ts = check_token_stats(token_stats)
        out = self.generate(**f, prefix=prefix, token_stats=n_ts)
        plen = out['prefix_len']
        lp = out['log_probs']
        T = prefix.shape[1]
        full = lp.new_zeros(lp.shape[0], T)
        n = min(T, lp.shape[1])
        full[:, :n] = lp[:, :n]
        live = torch.arange(T, device=lp.device).unsqueeze(0) < plen.unsqueeze(1)
        full = full * live
        res = {'log_probs': full, 'scores': full.sum(1), 'prefix_len': plen}
        if n_ts:
            neutral = token_stats_neutral(lp.shape[0], T, n_ts, self.padding_idx, lp.device)
            for k_ in TOKEN_STATS_KEYS:
                t = neutral[k_]
                t[:, :n] = out[k_][:, :n]
                keep = live if t.dim() == 2 else live.unsqueeze(-1)
                res[k_] = torch.where(keep, t, token_stats_neutral(1, 1, n_ts, self.padding_idx, lp.device)[k_])
        return res

    def caption_confidence(self, batch, gen, bpe=None):
        """The word-level view of `gen = generate(**batch, token_stats=n)` (attention_maps.caption_confidence)."""
        from .attention_maps import caption_confidence
        return caption_confidence(self, batch, gen, bpe=bpe)

    def caption_attention(self, batch, gen, bpe=None):
        """The reference's per-word attention view of `gen = generate(**batch, attention=True)` (attention_maps.py)."""
        from .attention_maps import caption_attention
        return caption_attention(self, batch, gen, bpe=bpe)

    def lanes_usable(self):
        """Whether `generate_lanes` has a decode loop to interleave: the K/V-cached static-batch generator on a GPU."""
        return (self.fast_generation and hasattr(self.decoder, 'project_contexts')
                and next(self.parameters()).is_cuda)

    @torch.no_grad()
    def generate_lanes(self, batches, beam_size=1, lanes=2, forward=False, attention=False, n_best=1, n_samples=1,
                       rank_by='score', rank_len_penalty=0.0, banned=None, ground=None, guidance=None, guidance_drop=None,
                       token_stats=0):
        """Captions for a sequence of batches with `lanes` decode loops IN FLIGHT TOGETHER, each on its own stream with its
        own DecodeStepper - captured step, static buffers and counters (_decode_stepper(lane=)): a decode step is a chain of ~40 dependent
        launches that each fill the chip for a few microseconds and then wait on memory - at 12-27 % of the HBM roofline a second
        chain fits beside the first.  The host alternates the lanes' graph replays (one replay per lane and token).  The
        encoders of a group of batches run first (eval mode: no randomness, results identical to `generate`).
        Yields (batch, output) in order.  forward=True: the outputs of `forward` in evaluate mode (loss + captions + per-sample
        BLEU bookkeeping: what commands/evaluate.py consumes) instead of `generate`'s; beam_size then is `eval_beam_size`.
        n_samples / rank_by / rank_len_penalty: as `generate` - every lane decodes the n hypotheses of its batch's images.
        banned (bool [V]) / ground (bool [V] or True): the shared forms of `generate`'s vocabulary masks, applied to every batch
        (each row grounded in its own article).
        guidance / guidance_drop: as `generate` - every lane decodes its batch and the batch's unconditional twin.
        token_stats: refused here (0 only); `generate` keeps the per-token statistics."""
        if check_token_stats(token_stats):
            raise ValueError('token_stats=%d: %s' % (token_stats, TOKEN_STATS_REFUSALS['lanes']))
        if banned is not None and (not torch.is_tensor(banned) or banned.dim() != 1):
            raise ValueError('generate_lanes takes the shared form of banned: a bool tensor [V]')
        if forward:                                    # (forward=True decodes under the model's keys and eval_* attributes)
            self._check_n_samples(n_samples, rank_by, rank_len_penalty, beam_size, attention, forward)
            if guidance is not None or guidance_drop is not None:
                raise ValueError('guidance / guidance_drop as arguments go with generate, not with forward=True')
            if attention:
                raise ValueError('attention=True goes with generate, not with forward=True')
            beam_size = getattr(self, 'eval_beam_size', 1)
            attention = bool(getattr(self, 'eval_attention', False) and not self.training and self.evaluate_mode)
            if self.training or not self.evaluate_mode or not self.lanes_usable():
                yield from self.generate_stream(batches, forward=True)  # nothing to decode / no static-batch decode loop
                return
        # (the prefix and the article ids a mask is grounded in come with every batch: the plan of a batch adds them)
        plan = self._plan(beam_size, attention, n_best, None, n_samples, rank_by, rank_len_penalty, banned, ground, guidance,
                          guidance_drop)
        self._check_beam(beam_size)
        self._check_penalties(attention)
        it = iter(batches)
        main = torch.cuda.current_stream()
        lane_streams = [streams.get('decode_lane_%d' % i) for i in range(lanes)]
        while True:
            group = []
            for _ in range(lanes):
                b = next(it, None)
                if b is not None:
                    group.append(b)
            if not group:
                return
            gens, outs, heads, thirds, plans = [], [None] * len(group), [], [None] * len(group), []
            for ln, b in enumerate(group):
                f = {k: v for k, v in b.items() if k in ('context', 'image', 'caption', 'face_embeds', 'obj_embeds')}
                if forward:
                    od, caption_ids, contexts = self._forward_loss(**f)
                    heads.append((od, b.get('metadata'), caption_ids.shape[0]))
                else:
                    caption_ids, _, contexts = self._forward(**f)
                # (sampling: the batch's seed is drawn here, in batch order - the draws of `generate` batch by batch)
                seed = draw_seed() if self._sampling() is not None else None
                if b.get('prefix') is not None and forward:
                    raise ValueError('prefix goes with generate, not with forward=True')
                pfx = self._check_prefix(b.get('prefix'), caption_ids.shape[0])
                if plan.guide is not None and pfx is not None:
                    self._check_guidance(guidance, guidance_drop, prefix=pfx)
                steps = self._beam_steps if beam_size > 1 else self._greedy_steps
                plans.append(plan._replace(prefix=pfx, vmask=self._vocab_mask(b['context'], banned, ground, attention)))
                ev = torch.cuda.Event()
                ev.record(main)
                lane_streams[ln].wait_event(ev)
                with torch.cuda.stream(lane_streams[ln]), ops.hip.bound_stream():
                    g = steps(caption_ids, contexts, lane=ln, seed=seed, plan=plans[ln])
                gens.append(g)
            live = list(range(len(group)))
            while live:
                for ln in list(live):
                    with torch.cuda.stream(lane_streams[ln]), ops.hip.bound_stream():
                        try:
                            next(gens[ln])
                        except StopIteration as done:
                            outs[ln], thirds[ln] = self._generated(plans[ln], *done.value), done.value[2]
                            live.remove(ln)
            for ln in range(len(group)):
                ev = torch.cuda.Event()
                ev.record(lane_streams[ln])
                main.wait_event(ev)
            for ln, (b, o) in enumerate(zip(group, outs)):
                if forward:
                    od, metadata, n = heads[ln]
                    self._forward_generated(od, o['gen_ids'], thirds[ln], metadata)
                    self.n_samples += n
                    self.n_batches += 1
                    o = od
                yield b, o

    def generate_stream(self, batches, beam_size=1, forward=False, attention=False, n_best=1, token_stats=0):
        """Captions for a sequence of batches (the test-set loop of tell/commands/evaluate.py:118-160) with the frozen
        encoders of batch N+1 launched on their own streams BEFORE the decode loop of batch N is issued - the trainer's
        schedule applied to generation.  Numerics are those of `generate` / `forward` batch by batch: the encoders read
        nothing the decode loop writes, and consecutive batches' encoder outputs live in different buffer sets.

        MEASURED (MI355X, full model, 32 captions x 100 steps): 534 -> 544 captions/s greedy, 375 -> 381 beam 4 - not the
        25 % the two legs' sum promises.  A decode step is ~44 dependent launches of 5-20 us whose workgroups fill the
        chip for one round each; every one of them queues behind a wave of 100-us GEMM workgroups of the encoders, so
        the two mostly take turns.  Giving the decode chain compute units of its own (hipExtStreamCreateWithCUMask
        streams - hipGraph replays launched on them DO keep the mask, tools/probes/cumask_probe.hip) was built and
        measured: 64 / 128 CUs for the chain -> 260 / 416 captions/s - the chain's kernels are one round of
        latency-bound workgroups on 256 CUs and become two / four rounds on fewer (profiles/r05_cu_partition.txt); not
        kept.  What moves generation throughput is the batch (the iterator's knob): 544 / 747 / 939 captions/s greedy at
        32 / 64 / 128 captions per batch.

        batches: any iterable of batch dicts (keys of `forward`); forward=True yields `self(**batch)` (evaluate mode:
        loss + generation + metrics) instead of `generate(**batch)`.  Yields (batch, output_dict) in order.
        token_stats: refused here (0 only); `generate` keeps the per-token statistics."""
        if check_token_stats(token_stats):
            raise ValueError('token_stats=%d: %s' % (token_stats, TOKEN_STATS_REFUSALS['lanes']))
        if forward and (attention or n_best != 1):
            raise ValueError('%s goes with generate, not with forward=True' % ('attention=True' if attention else 'n_best'))
        if attention:
            self._check_attention(beam_size)
        it = iter(batches)
        cur = next(it, None)
        enc = None
        while cur is not None:
            nxt = next(it, None)
            ahead = None
            can = hasattr(self, 'encode') and torch.is_tensor(cur.get('image')) and cur['image'].is_cuda
            if can and enc is None:
                enc = self.encode(cur['context'], cur['image'])
            if can and nxt is not None and torch.is_tensor(nxt.get('image')) and nxt['image'].is_cuda:
                ahead = self.encode(nxt['context'], nxt['image'], ahead=True)
            if enc is not None and enc.stale():
                enc = self.encode(cur['context'], cur['image'])
            extra = {'encoded': enc} if enc is not None else {}
            if forward and cur.get('prefix') is not None:
                raise ValueError('prefix goes with generate, not with forward=True')
            out = self(**{k_: v_ for k_, v_ in cur.items() if k_ != 'prefix'}, **extra) if forward else self.generate(**cur, beam_size=beam_size, attention=attention, n_best=n_best, **extra)
            yield cur, out
            cur, enc = nxt, ahead

    # ---- :399-494 -----------------------------------------------------------------
    fast_generation = True      # projected-K/V cache + static batch; False = the reference's control flow

    def _generate(self, caption_ids, contexts, attn_idx=None, gen_len=100, eos=2, beam_size=1, attention=False, n_best=1,
                  prefix=None, samples=None, vmask=None, guide=None, token_stats=0):
        """The generator of one decode call, chosen by its DecodePlan: the LSTM decoder's own loop; beam search; the cached
        generator - with fast_generation, or whenever an option of the plan or of the model (search options, penalties) is
        set, all of which live there; else the reference's control flow."""
        plan = DecodePlan(beam_size, n_best, attention, prefix, samples, vmask, guide, token_stats)
        _, opts, _, pen = plan.resolve(self, gen_len, eos, rows=None if prefix is None else caption_ids.shape[0])
        if not hasattr(self.decoder, 'project_contexts'):
            # a recurrent decoder behind this model class (expt/*/3_lstm_roberta: `lstm_decoder_flattened`): greedy
            # decode that carries the LSTM state.  (The reference's loop feeds such a decoder only the last token with
            # an incremental_state its LSTMDecoder ignores, i.e. every step restarts from the initial state -
            # transformer_flattened.py:_generate with decoder_flattened_lstm.py:131-152; not reproduced.)
            from .baseline_glove import BaselineGloveModel
            lps, ids = BaselineGloveModel._generate(self, caption_ids, contexts, gen_len, eos)
            return lps, ids, []
        self._check_beam(beam_size)
        options = plan.options()
        if beam_size > 1:
            return self._generate_beam(caption_ids, contexts, options.pop('beam_size'), gen_len, eos, **options)
        # (attention maps too: fast_generation = False is the reference's control flow with the legacy need_attn export)
        if self.fast_generation or opts is not None or pen is not None or options:
            return self._generate_cached(caption_ids, contexts, gen_len, eos, **options)
        return self._generate_reference_flow(caption_ids, contexts, attn_idx, gen_len, eos)

    @staticmethod
    def _drive(gen):
        """Run a decode generator (one `yield` per issued step) to its result."""
        try:
            while True:
                next(gen)
        except StopIteration as done:
            return done.value

    @torch.no_grad()
    def _generate_cached(self, caption_ids, contexts, gen_len=100, eos=2, check_every=8, lane=0, **options):
        """options: the fields of a DecodePlan (attention=, prefix=, samples=, vmask=, guide=, stats=)."""
        return self._drive(self._greedy_steps(caption_ids, contexts, gen_len, eos, check_every, lane, plan=DecodePlan(**options)))

    def _greedy_steps(self, caption_ids, contexts, gen_len=100, eos=2, check_every=8, lane=0, seed=None, plan=DecodePlan()):
        """A generator: yields after every issued decode step (generate_lanes interleaves two of these on two streams), returns
        (log_probs, ids, []).  plan: the DecodePlan of the call, resolved here once (its checks, the model's sampling rule, ban
        list and penalties); attention, prefix, samples = (n,) + rank, vmask, guide and stats below are its fields.
        Same greedy decode, restructured for the GPU: (1) context K/V projected once per caption,
        (2) the batch keeps its shape - finished rows are masked instead of compacted, so there is no
        per-step gather of the contexts and no per-step host synchronisation (the all-finished test
        runs every `check_every` steps), (3) fused arg-max over the adaptive softmax.  Rows are
        independent, so every row sees exactly the arithmetic of the reference flow: token ids are
        identical, pad=1 after EOS, output length = 1 + steps until the last row finished.
        sampling_topk > 1: the head's last launch draws from the top k instead (tell_adaptive_logprob_sample), keyed on
        (seed, row, step) - `seed` (default: drawn now, draw_seed) goes into the stepper's device word before the first step.
        attention=True: every step also leaves its head-averaged attention weights in the stepper's sink (step.attn, one slot
        per step); the third result is then an AttnMaps (maps {name: [B, steps, n_layers, S + 2] fp32}, steps [B]) instead of [].
        prefix = (tokens int64 [B, P], plen int32 [B]) of check_prefix: the stepper's forcing table is filled before the first step
        and the head of every step ends in one more launch (tell_adaptive_logprob_forced); the bookkeeping is untouched - it
        books a forced token exactly as a picked one.
        With penalties set (_penalties()): the head counts every row's tokens (step.pen_source over `ids`) and picks - arg-max or
        top-k draw - over the penalised scores, which is what `log_probs` then holds.
        n > 1 (a sampling model; generate(n_samples=n)): R = B * n rows are resident, hypothesis j of image b in row b * n + j -
        cur, ids, lps, done_step and fin8 are R rows tall, the contexts, masks, projected K/V and the prefix stay at width B (as
        _beam_steps hands them to the stepper), one seed, row r draws with (seed, r, step).  Behind the loop one launch
        (tell_sample_rank, rank = (rule, alpha)) scores, de-duplicates and ranks the n hypotheses of every image: the results
        are the first rank's, the third a DecodeInfo with .scores and .samples.
        vmask = (ctx_ids, cls_bits, deny8) of _vocab_mask: the stepper's bitmap - one row per image - is built before the first
        step (step.set_mask) and every pick is the masked one; the bookkeeping is untouched.
        guide = (drop, gamma) of _check_guidance: the batch is decoded with its unconditional twin behind
        it (guided_batch: 2 * images rows), every pick is the guided arg-max - one token and one normalised log-prob for both
        rows of a pair - the bookkeeping runs over all rows unchanged and the results are the first half.
        stats = n_alt in 1..8 (generate(token_stats=)): every head ends in tell_adaptive_logprob_stats,
        which reads the finished flags as they stand BEFORE the step's bookkeeping (step.stats_source) and writes slot = step of
        the stepper's sink; behind the loop the slots become the five [rows, steps(, n_alt)] arrays, carried as .token_stats of
        the third result (a DecodeInfo, or an AttnMapsStats with attention=True)."""
        dec = self.decoder
        # greedy: the bans apply (no_repeat_ngram_size, min_len); the length penalty ranks hypotheses and there is one
        sampling, _, ban, pen = plan.resolve(self, gen_len, eos)
        _, _, attention, prefix, samples, vmask, guide, stats = plan
        n, rank = (int(samples[0]), samples[1:]) if samples is not None else (1, None)
        if guide is not None:
            cond = caption_ids.shape[0]
            caption_ids, contexts = guided_batch(caption_ids, contexts, guide[0])
        images = caption_ids.shape[0]
        B = images * n                                           # decode rows
        dev = caption_ids.device
        kv = dec.project_contexts(contexts)
        step = self._decode_stepper(B, kv, contexts, gen_len, lane=lane, sample=sampling, attention=attention, ban=ban,
                                    prefix=prefix is not None, pen=pen, hyp=n, mask=vmask is not None,
                                    guide=None if guide is None else guide[0], stats=stats)
        if guide is not None:
            step.set_guidance(guide[1])
        if prefix is not None:
            step.set_prefix(*prefix)
        if vmask is not None:
            step.set_mask(*vmask, eos=int(eos))
        if sampling is not None:
            step.seed.fill_(draw_seed() if seed is None else int(seed))
        cur = caption_ids[:, 0:1].contiguous() if n == 1 else caption_ids[:, 0:1].repeat_interleave(n, dim=0).contiguous()
        finished = cur[:, 0] == eos
        fused = caption_ids.is_cuda and step.static              # one bookkeeping launch per token (tell_greedy_update)
        if fused:
            # the histories live in STATIC buffers of the stepper (the bookkeeping launch is part of the captured step)
            bk = step.book('greedy', lambda: dict(
                ids=torch.empty(B, gen_len + 1, dtype=torch.long, device=dev),
                lps=torch.empty(B, gen_len, dtype=torch.float32, device=dev),
                done_step=torch.empty(B, dtype=torch.long, device=dev), fin8=torch.empty(B, dtype=torch.uint8, device=dev)))
            ids, lps, done_step, fin8 = bk['ids'], bk['lps'], bk['done_step'], bk['fin8']
            ids.fill_(self.padding_idx)
            lps.zero_()
            done_step.fill_(gen_len)
            if ban is not None:
                step.ban_source(ids, fin8)
            if pen is not None:
                step.pen_source(ids, fin8)
            if stats:
                step.stats_source(fin8)
        else:
            ids = torch.full((B, gen_len + 1), self.padding_idx, dtype=torch.long, device=dev)
            lps = torch.zeros(B, gen_len, dtype=torch.float32, device=dev)
            done_step = torch.full((B,), gen_len, dtype=torch.long, device=dev)   # steps this row took part in
        ids[:, 0] = cur[:, 0]
        done_step[finished] = 0
        steps = gen_len
        if fused:
            fin8.copy_(finished)
            step.cur.copy_(cur)
            inv_temp = 1.0 / float(self.sampling_temp)

            def book(out, i, step_dev):
                # the step's LAST launch: inside the captured step it takes the step index from the device counter
                # (step_dev), eagerly from the host; either way it leaves the next step's position offset behind
                tok, lp = out
                ops.call('tell_greedy_update', tok.reshape(B), lp.reshape(B), fin8, ids, ids.stride(0), lps, lps.stride(0),
                         done_step, step.cur, B, int(i), int(eos), inv_temp, step.counter_out, step_dev)
            yield from step.steps(gen_len, check_every, book, fin8)
        for i in range(0 if fused else gen_len):
            if ban is not None:
                step.ban_source(ids, finished.to(torch.uint8))
            if pen is not None:
                step.pen_source(ids, finished.to(torch.uint8))
            if stats:
                step.stats_source(finished.to(torch.uint8))
            tok, lp = step(i, cur)
            yield i
            tok = tok.long().view(B)
            lp = lp.view(B) / self.sampling_temp
            ids[:, i + 1] = torch.where(finished, ids[:, i + 1], tok)
            lps[:, i] = torch.where(finished, lps[:, i], lp)
            newly = (~finished) & (tok == eos)
            done_step = torch.where(newly, torch.full_like(done_step, i + 1), done_step)
            finished = finished | newly
            cur = tok.view(B, 1)
            if (i + 1) % check_every == 0 and bool(finished.all()):
                break
        steps = int(done_step.max())                                          # one sync at the end
        steps = max(steps, 1)
        ts = self._token_stats_arrays(step.stats, steps) if stats else None
        if n > 1:
            return self._rank_samples(ids, lps, done_step, images, n, steps, gen_len, eos, rank, stats=ts)
        attns = []
        if ts is not None:
            attns = DecodeInfo()
            attns.token_stats = ts
        if attention:
            # slot i of a layer's buffer = step i (the token at ids[:, i + 1]); copied out: the buffers belong to the stepper
            bufs = step.attn.bufs
            attns = (AttnMapsStats if ts is not None else AttnMaps)(
                {n: torch.stack([lb[n][:steps] for lb in bufs], 0).permute(2, 1, 0, 3).contiguous() for n in bufs[0]},
                done_step.clamp(max=steps).clone())
            if ts is not None:
                attns.token_stats = ts
        if guide is not None:                                                 # (the unconditional twins took the same decisions)
            return lps[:cond, :steps].clone(), ids[:cond, :steps + 1].clone(), attns
        if fused:                                                             # (the static buffers belong to the stepper)
            return lps[:, :steps].clone(), ids[:, :steps + 1].clone(), attns
        return lps[:, :steps], ids[:, :steps + 1], attns

    @staticmethod
    def _token_stats_arrays(sink, steps):
        """The first `steps` slots of a decode.StatsSink [slots, rows(, n)] -> the five arrays of generate(token_stats=n),
        [rows, steps(, n)] (copies: the buffers belong to the stepper)."""
        return {'alt_ids': sink.alt_tok[:steps].permute(1, 0, 2).long().contiguous(),
                'alt_log_probs': sink.alt_lp[:steps].permute(1, 0, 2).contiguous(),
                'token_rank': sink.rank[:steps].t().long().contiguous(),
                'token_entropy': sink.entropy[:steps].t().contiguous(),
                'token_model_lp': sink.chosen_lp[:steps].t().contiguous()}

    def _rank_samples(self, ids, lps, done_step, B, n, steps, gen_len, eos, rank, stats=None):
        """The end of _greedy_steps with n > 1 hypotheses per image: ids [B * n, gen_len + 1], lps [B * n, gen_len], done_step
        [B * n] of the decode loop -> (log_probs [B, steps], ids [B, steps + 1] of the first rank, DecodeInfo).  One launch
        (tell_sample_rank; hypotheses on the CPU: its host definition), then the gathers by its order."""
        rule, alpha = rank
        inv_norm = inv_norm_table(alpha, gen_len).to(ids.device) if alpha else None
        if ids.is_cuda:
            order, score, dup = ops.sample_rank(ids, lps, done_step, B, n, steps, self.padding_idx, eos, rule, inv_norm=inv_norm)[:3]
        else:
            d = sample_rank_definition(ids.numpy(), lps.numpy(), done_step.numpy(), n, steps, eos, rule,
                                       None if inv_norm is None else inv_norm.numpy())
            order, score, dup = (torch.from_numpy(d[k_]) for k_ in ('order', 'score', 'dup'))
        order = order.long()

        def ranked(t):                                            # [B * n, W] -> [B, n, W] in rank order (a new tensor)
            t = t.reshape(B, n, -1)
            return t.gather(1, order.unsqueeze(-1).expand(-1, -1, t.shape[-1]))
        info = DecodeInfo()
        info.samples = {'gen_ids_samples': ranked(ids[:, :steps + 1]), 'log_probs_samples': ranked(lps[:, :steps]),
                        'scores_samples': score.gather(1, order), 'sample_index': order,
                        'duplicate': dup.gather(1, order).bool()}
        info.scores = info.samples['scores_samples'][:, 0].contiguous()
        if stats is not None:                                     # the per-token statistics of every draw, in rank order too
            for k_, t in stats.items():
                t = t.reshape(B, n, *t.shape[1:])
                info.samples[k_ + '_samples'] = t.gather(1, order.view(B, n, *([1] * (t.dim() - 2))).expand_as(t))
            info.token_stats = {k_: info.samples[k_ + '_samples'][:, 0].contiguous() for k_ in stats}
        return (info.samples['log_probs_samples'][:, 0].contiguous(), info.samples['gen_ids_samples'][:, 0].contiguous(), info)

    def _decode_stepper(self, B, kv, contexts, gen_len, **kw):
        """-> the DecodeStepper (models/stepper.py) of the cached greedy / beam generators for this caption batch: a view over
        the cache entry of its signature in `_decode_graphs` (static buffers, captured graphs), or the eager step."""
        return DecodeStepper(self, B, kv, contexts, gen_len, **kw)

    @torch.no_grad()
    def _generate_beam(self, caption_ids, contexts, beam_size, gen_len=100, eos=2, check_every=8, lane=0, **options):
        """options: the fields of a DecodePlan (n_best=, prefix=, vmask=, guide=)."""
        return self._drive(self._beam_steps(caption_ids, contexts, gen_len, eos, check_every, lane,
                                            plan=DecodePlan(beam_size, **options)))

    def _beam_steps(self, caption_ids, contexts, gen_len=100, eos=2, check_every=8, lane=0, seed=None, plan=DecodePlan()):
        """A generator like _greedy_steps; plan.beam_size = K, and n_best, prefix, vmask and guide below are the plan's fields.
        Beam search on the cached static-shape generator (SURVEY 8-f1 / BASELINE config 5; the reference itself
        only samples top-1, transformer_faces_objects.py:443-464).  B*K rows (row = b*K + j) stay resident; the
        projected K/V of the static contexts are computed once per caption and replicated per beam; the DynamicConv
        input buffers are reordered by parent with the reference's `reorder_incremental_state` contract
        (dynamic.py:338-342).  Score = sum of token log-probs (no length penalty); a finished hypothesis keeps its
        score and is extended with pad only.  -> (log_probs [B,steps], ids [B,steps+1] of the best hypothesis, []).
        With search options: `beam_len_penalty` alpha ranks the candidates by sum * len ** -alpha (len:
        generated tokens, </s> included; frozen when a hypothesis ends), `no_repeat_ngram_size` / `min_len` ban tokens per
        hypothesis before its K best are taken.  The third result is a DecodeInfo (an empty list) with .scores [B] and, for
        n_best = n > 1, .nbest = (ids [B,n,steps+1], log_probs [B,n,steps], scores [B,n]).
        prefix = (tokens, plen) of check_prefix: during a sample's forced steps every hypothesis' candidate list is the forced
        token and K - 1 fillers (-inf, pad), so only slot 0 stays live - as at step 0 - and the beam opens at the first free
        step; the bookkeeping is untouched.
        With penalties set (_penalties()): every hypothesis' K best are taken over its penalised scores (step.pen_source over
        `seqs`), and `cum`, the log_probs and the scores accumulate those scores.
        vmask = (ctx_ids, cls_bits, deny8) of _vocab_mask: the K hypotheses of a sample share its row of the stepper's bitmap
        (step.set_mask) and every hypothesis' K best are taken under it - with a ban list, in the same launch.
        guide = (drop, gamma) of _check_guidance: samples B .. 2B - 1 are the unconditional twins
        (guided_batch), hypothesis row r's partner is row r + B * K; every pair's K candidates come from the guided pick and are
        the same for both rows, so tell_beam_update takes the same decisions in both halves; the results are the first half."""
        dec = self.decoder
        _, opts, ban, pen = plan.resolve(self, gen_len, eos)
        K, n_best, _, prefix, _, vmask, guide, _ = plan
        if guide is not None:
            cond = caption_ids.shape[0]
            caption_ids, contexts = guided_batch(caption_ids, contexts, guide[0])
        B = caption_ids.shape[0]
        dev = caption_ids.device
        pad = self.padding_idx
        alpha = opts[0] if opts is not None else 0.0
        rep = lambda t, dim: t.repeat_interleave(K, dim=dim).contiguous()           # noqa: E731
        # contexts, masks and projected K/V stay at batch B: the attention modules present the K hypotheses of a
        # sample as K query positions of that sample (modules/attention.py), nothing is replicated per beam
        ctx = {k_: v_ for k_, v_ in contexts.items() if torch.is_tensor(v_)}
        kv = dec.project_contexts(contexts)
        step = self._decode_stepper(B * K, kv, ctx, gen_len, topk=K, lane=lane, ban=ban,
                                    opts=(opts + (int(eos),)) if opts is not None else None, prefix=prefix is not None,
                                    pen=pen, mask=vmask is not None, guide=None if guide is None else guide[0])
        if guide is not None:
            step.set_guidance(guide[1])
        if prefix is not None:
            step.set_prefix(*prefix)
        if vmask is not None:
            step.set_mask(*vmask, eos=int(eos))
        cur = rep(caption_ids[:, 0:1], 0)
        finished = (cur[:, 0] == eos).view(B, K)
        fused = caption_ids.is_cuda and step.static and K <= 8 and gen_len + 1 <= 256
        if fused:
            bk = step.book('beam', lambda: dict(
                cum=torch.empty(B, K, dtype=torch.float32, device=dev), fin8=torch.empty(B, K, dtype=torch.uint8, device=dev),
                seqs=torch.empty(B, K, gen_len + 1, dtype=torch.long, device=dev),
                lps=torch.empty(B, K, gen_len, dtype=torch.float32, device=dev),
                rows=torch.empty(B * K, dtype=torch.long, device=dev)))
            cum, fin8, seqs, lps, rows = bk['cum'], bk['fin8'], bk['seqs'], bk['lps'], bk['rows']
            cum.fill_(float('-inf'))
            seqs.fill_(pad)
            lps.zero_()
            if alpha:
                nb = step.book('beam_norm', lambda: dict(len=torch.empty(B, K, dtype=torch.int32, device=dev),
                                                         inv_norm=torch.empty(gen_len + 2, dtype=torch.float32, device=dev)))
                hyp_len, inv_norm = nb['len'], nb['inv_norm']
                hyp_len.zero_()
                inv_norm.copy_(inv_norm_table(alpha, gen_len + 1))
        else:
            cum = torch.full((B, K), float('-inf'), dtype=torch.float32, device=dev)
            seqs = torch.full((B, K, gen_len + 1), pad, dtype=torch.long, device=dev)
            lps = torch.zeros(B, K, gen_len, dtype=torch.float32, device=dev)
            if alpha:
                hyp_len = torch.zeros(B, K, dtype=torch.long, device=dev)
                inv_norm = inv_norm_table(alpha, gen_len + 1).to(dev)
        cum[:, 0] = 0.0                                     # all K rows start identical: only hypothesis 0 counts
        seqs[:, :, 0] = cur.view(B, K)
        base = (torch.arange(B, device=dev) * K).view(B, 1)
        n_steps = gen_len
        if fused:
            # one bookkeeping launch per token (tell_beam_update: candidate scores, top-K per sample, histories gathered
            # by parent, next inputs; ring buffers: it also composes the ancestor table with this step's parents - no row
            # of any layer's DynamicConv buffer is moved) - the LAST launch of the captured step where the stepper allows
            fin8.copy_(finished)
            step.cur.copy_(cur)
            ring = step.back is not None
            inv_temp = 1.0 / float(self.sampling_temp)

            if ban is not None:
                step.ban_source(seqs.view(B * K, gen_len + 1), fin8.view(B * K))
            if pen is not None:
                step.pen_source(seqs.view(B * K, gen_len + 1), fin8.view(B * K))

            def book(out, i, step_dev):
                tk, lp = out
                if alpha:
                    ops.call('tell_beam_update_norm', tk, lp, cum, fin8, seqs, lps, step.cur, rows, hyp_len, inv_norm, B, K,
                             gen_len + 1, int(i), int(pad), int(eos), inv_temp, step.back, step.back.shape[0] if ring else 0,
                             step.counter_out, step_dev)
                    return
                ops.call('tell_beam_update', tk, lp, cum, fin8, seqs, lps, step.cur, rows, B, K, gen_len + 1, int(i), int(pad),
                         int(eos), inv_temp, step.back, step.back.shape[0] if ring else 0, step.counter_out, step_dev)

            def host_book(out, i):
                # (time-ordered buffers - fp32 parity mode: the bookkeeping stays a host-side launch and one more launch
                #  re-orders every layer's rows by parent)
                book(out, i, None)
                step.reorder(rows, K)
            # (multi-step replays need the bookkeeping inside the captured step: ring buffers only)
            n_steps = yield from step.steps(gen_len, check_every, book if ring else None, fin8, multi=ring,
                                            after=None if ring else host_book)
        for i in range(0 if fused else gen_len):
            # each hypothesis contributes its own K best tokens (the best K of K x V always lie among them)
            if ban is not None:
                step.ban_source(seqs.view(B * K, -1).contiguous(), finished.to(torch.uint8).view(B * K).contiguous())
            if pen is not None:
                step.pen_source(seqs.view(B * K, -1).contiguous(), finished.to(torch.uint8).view(B * K).contiguous())
            tk, lp = step(i, cur)
            tk, lp = tk.view(B, K, K).long(), lp.view(B, K, K) / self.sampling_temp
            # a finished hypothesis has ONE continuation: pad, at no cost
            fin = finished.unsqueeze(-1)
            first = torch.zeros(K, dtype=torch.bool, device=dev)
            first[0] = True
            lp = torch.where(fin, torch.where(first, torch.zeros_like(lp), torch.full_like(lp, float('-inf'))), lp)
            tk = torch.where(fin, torch.full_like(tk, pad), tk)
            raw = (cum.unsqueeze(-1) + lp).view(B, K * K)
            if alpha:
                # candidates of a live hypothesis have i + 1 tokens, a finished one keeps its length; one fp32 multiply
                cand_len = torch.where(finished, hyp_len, torch.full_like(hyp_len, i + 1)).unsqueeze(-1).expand(B, K, K)
                score = raw * inv_norm[cand_len.reshape(B, K * K)]
                score = torch.where(torch.isnan(score), torch.full_like(score, float('-inf')), score)
                # (the lowest candidate index wins a tie: a stable descending sort)
                idx = torch.sort(score, dim=1, descending=True, stable=True)[1][:, :K]
                top = raw.gather(1, idx)
                hyp_len = cand_len.reshape(B, K * K).gather(1, idx)
            else:
                top, idx = raw.topk(K, dim=1)                                       # sorted, best first
            parent = idx // K
            tok = tk.view(B, K * K).gather(1, idx)
            rows = (base + parent).view(-1)
            was_finished = finished.gather(1, parent)
            tok = torch.where(was_finished, torch.full_like(tok, pad), tok)
            seqs = seqs.view(B * K, -1).index_select(0, rows).view(B, K, -1)
            lps = lps.view(B * K, -1).index_select(0, rows).view(B, K, -1)
            seqs[:, :, i + 1] = tok
            lps[:, :, i] = torch.where(was_finished, torch.zeros_like(top), top - cum.gather(1, parent))
            finished = was_finished | (tok == eos)
            cum = top
            step.reorder(rows)
            cur = tok.view(B * K, 1)
            yield i
            if (i + 1) % check_every == 0 and bool(finished.all()):
                n_steps = i + 1
                break
        best = seqs[:, 0]                                    # topk keeps hypotheses sorted by score
        n_best = int(n_best)
        # one sync: length of the longest best caption (n_best > 1: of the longest of the n best)
        steps = int((best[:, 1:] != pad).sum(1).max()) if n_best == 1 else int((seqs[:, :n_best, 1:] != pad).sum(2).max())
        steps = max(min(steps, n_steps), 1)
        info = DecodeInfo()
        scores = cum * inv_norm[hyp_len.long()] if alpha else cum      # (the multiply the ranking used)
        if guide is not None:                                # (the unconditional twins took the same decisions)
            seqs, lps, scores, best = seqs[:cond], lps[:cond], scores[:cond], best[:cond]
        info.scores = scores[:, 0].clone()
        if n_best > 1:
            info.nbest = (seqs[:, :n_best, :steps + 1].clone(), lps[:, :n_best, :steps].clone(), scores[:, :n_best].clone())
        if fused:                                            # (the static buffers belong to the stepper)
            return lps[:, 0, :steps].clone(), best[:, :steps + 1].clone(), info
        return lps[:, 0, :steps], best[:, :steps + 1], info

    @torch.no_grad()
    def _generate_reference_flow(self, caption_ids, contexts, attn_idx=None, gen_len=100, eos=2):
        """Greedy decoding with the reference's semantics (finished rows leave the batch, pad=1 after
        EOS, loop ends when no row is active).  The arg-max over the 50 265-way adaptive softmax is
        fused (no [B, vocab] log-prob tensor).  sampling_topk > 1: the fused top-k draw keyed on the alive rows' ORIGINAL
        batch rows, so the captions equal the cached flow's under the same seed."""
        state = {}
        B = caption_ids.shape[0]
        dev = caption_ids.device
        sampling = self._sampling()
        if sampling is not None:
            seed_word = torch.full((1,), draw_seed(), dtype=torch.int32, device=dev)
        seed = caption_ids[:, 0:1]
        alive = seed[:, -1] != eos
        keep = alive
        cur = seed
        log_probs, paths, attns = [], [seed], []
        names = [k for k in contexts if not k.endswith('_mask') and not k.startswith('_')]
        for i in range(gen_len):
            self.decoder.filter_incremental_state(state, keep)                      # :417
            ctx_i = {}
            for n in names:                                                         # :420-431
                ctx_i[n] = contexts[n][:, alive]
                ctx_i[n + '_mask'] = contexts[n + '_mask'][alive]
            dec_out = self.decoder({self.index: cur[:, -1:]}, ctx_i, incremental_state=state)
            attns.append(dec_out[1]['attn'])
            if sampling is None:
                tok, lp = self.decoder.adaptive_softmax.greedy(dec_out[0][:, -1:])  # :443-464
            else:                                                                   # :443-470, topk + multinomial
                rows = alive.nonzero().squeeze(1).to(torch.int32)
                tok, lp = self.decoder.adaptive_softmax.sample(dec_out[0][:, -1:], sampling[0], sampling[1], seed_word, i,
                                                               row_ids=rows, topp=sampling[2] if len(sampling) > 2 else None,
                                                               rule=sampling[3] if len(sampling) > 3 else None)
            sel_ix = tok.long()
            sel_lp = lp / self.sampling_temp
            full_lp = sel_lp.new_zeros(B, 1)
            full_lp[alive] = sel_lp
            full_ix = sel_ix.new_full((B, 1), self.padding_idx)
            full_ix[alive] = sel_ix
            log_probs.append(full_lp)
            paths.append(full_ix)
            keep = sel_ix.squeeze(-1) != eos                                        # :476-483
            alive = alive.clone()
            alive[alive.nonzero().squeeze(1)[~keep]] = False
            cur = torch.cat([cur, sel_ix], dim=1)[keep]
            if int(keep.sum()) == 0:                                                # :485
                break
        return torch.cat(log_probs, dim=-1), torch.cat(paths, dim=-1), attns

    def get_metrics(self, reset=False):                                             # :504-517
        metrics = {'_n_batches': self.n_batches, '_n_samples': self.n_samples}
        for key, value in self.sample_history.items():
            metrics[key] = value / max(self.n_samples, 1)
        if reset:
            self.n_batches = 0
            self.n_samples = 0
            self.sample_history = defaultdict(float)
        return metrics


@Model.register('transformer_faces_objects')
class TransformerFacesObjectModel(CaptionModel):
    """tell/models/transformer_faces_objects.py:22-23"""
    USE_FACES_OBJECTS = True
    EXTRA_CONTEXTS = ('faces', 'obj')


@Model.register('transformer_faces')
class TransformerFacesModel(CaptionModel):
    """tell/models/transformer_faces.py:21-22 (expt/*/8_transformer_faces): image + article + faces, driven by
    `dynamic_conv_decoder_faces_parallel`; the faces+objects forward without `obj_embeds`."""
    USE_FACES_OBJECTS = True
    EXTRA_CONTEXTS = ('faces',)


@Model.register('transformer_flattened')
class TransformerFlattenedModel(CaptionModel):
    """tell/models/transformer_flattened.py:23-24 (also drives `dynamic_conv_decoder_flattened_no_image`)"""
    USE_FACES_OBJECTS = False
    EXTRA_CONTEXTS = ()
