"""tell/modules/softmax.py:43-222 on the MI355X path."""
import torch
import torch.nn as nn

from .. import ops
from .linear import Linear


class TiedLinear(nn.Module):
    """tell/modules/linear.py:37-50 - holds the shared Parameter as `.weight`."""

    def __init__(self, weight, transpose=False):
        super().__init__()
        self.weight = weight
        self.transpose = transpose


class TiedHeadModule(nn.Module):
    """tell/modules/softmax.py:11-40."""

    def __init__(self, weights, input_dim, n_classes):
        super().__init__()
        tied_emb, _ = weights
        self.num_words, emb_dim = tied_emb.shape
        assert emb_dim == input_dim
        self.word_proj = TiedLinear(tied_emb)
        self.n_classes = n_classes
        self.class_proj = Linear(input_dim, n_classes, bias=False)
        self.out_dim = self.num_words + n_classes
        self.register_buffer('_float_tensor', torch.zeros(1))


class AdaptiveSoftmax(nn.Module):
    """Adaptive softmax tied to the adaptive input embedding (tie_adaptive_weights=True,
    tie_adaptive_proj=False, factor 1, dropout 0 - config.yaml:66-72)."""

    def __init__(self, vocab_size, input_dim, cutoff, dropout=0, factor=1., adaptive_inputs=None, tie_proj=False):
        super().__init__()
        if adaptive_inputs is None or tie_proj or dropout:
            raise NotImplementedError('only the tied-embedding configuration of the expt/ configs is implemented')
        cutoff = list(cutoff)
        if not cutoff or vocab_size > cutoff[-1]:
            cutoff.append(vocab_size)
        assert vocab_size == cutoff[-1]
        self.vocab_size, self.cutoff, self.input_dim = vocab_size, cutoff, input_dim
        n_tails = len(cutoff) - 1
        self.head = TiedHeadModule(adaptive_inputs.weights_for_band(0), input_dim, n_tails)
        self.tail = nn.ModuleList()
        for i in range(n_tails):
            emb, proj = adaptive_inputs.weights_for_band(i + 1)
            self.tail.append(nn.Sequential(Linear(input_dim, proj.shape[1], bias=False), nn.Dropout(0.0),
                                           TiedLinear(emb)))
        self.register_buffer('version', torch.LongTensor([1]))

    def _tails(self):
        out = []
        for t in self.tail:
            out += [t[0].weight, t[2].weight]
        return out

    def loss(self, x, target, padding_idx, row_weight=None):
        """-> (loss_sum in nats [1], sample_size [1] int32), both on the device.
        row_weight: fp32 in the layout of `target` or None (ops.adaptive_loss)."""
        if row_weight is not None and (not torch.is_tensor(row_weight) or row_weight.shape != target.shape):
            raise ValueError('AdaptiveSoftmax.loss: row_weight must have the shape %s of target' % (tuple(target.shape),))
        if x.dim() == 3 and not x.is_contiguous() and x.transpose(0, 1).is_contiguous():
            # the decoder hands its T x B x C buffer over as a [B,T,C] view: the summed loss does not care about the row
            # order, so the (tiny) target is transposed instead of the activations (and of their gradient)
            x, target = x.transpose(0, 1), target.t().contiguous()
            if row_weight is not None:
                row_weight = row_weight.t().contiguous()
        return ops.adaptive_loss(x, target, self.cutoff, padding_idx, self.head.word_proj.weight,
                                 self.head.class_proj.weight, self._tails(), row_weight=row_weight)

    def get_log_prob(self, X, target=None):
        assert target is None
        B, T, E = X.shape
        _, _, full = ops.adaptive_log_probs(ops.as2dc(X), self.cutoff, self.head.word_proj.weight,
                                            self.head.class_proj.weight, self._tails(), want_full=True)
        return full.view(B, T, self.vocab_size)

    def topk(self, X, k, ban=None, force=None, pen=None, mask=None, guide=None, stats=None):
        """The k best (token, log-prob) of every position, best first, fused like `greedy` (beam search).
        ban = (ban int32 [B * T, ld], n_ban int32 [B * T]): the row's banned tokens never enter its list
        (tell_adaptive_logprob_topk_banned; k = 1 is the greedy decode under bans).
        pen = (theta, sub fp32 [n_sub], pen_tok int32 [B * T, ld], pen_cnt alike, n_pen int32 [B * T]): the k best PENALISED
        scores s = min(lp, 0) * theta - sub[count] of the listed tokens, lp of every other (DESIGN.md section 20,
        tell_adaptive_logprob_topk_penalised); the second result then holds scores, not log-probs.
        mask = (bits int32 [B * T / per, words], per): position r never lists a token whose bit is set in bits[r // per]; every
        log-prob is the unmasked one (tell_adaptive_logprob_topk_masked; a ban list may join it).
        guide = (pair_offset, gamma fp32 [1] on the device): position r < pair_offset and its partner r + pair_offset get the
        same k candidates, ranked by s = lp_c + (gamma - 1) * (lp_c - lp_u) and reported as s - logsumexp(s) (DESIGN.md section 24,
        tell_adaptive_logprob_topk_guided); on its own - no ban list, penalties, mask or forcing table.
        stats (here, in `sample` and in `greedy`): a decode.StatsSink - the head ends in tell_adaptive_logprob_stats, which
        leaves the step's alternatives, rank, entropy and model log-prob in the sink's slot."""
        B, T, E = X.shape
        kw = {'pen': pen} if pen is not None else {}
        if mask is not None:
            kw['mask'] = mask
        if guide is not None:
            kw['guide'] = guide
        if stats is not None:
            kw['stats'] = stats
        tok, lp, _ = ops.adaptive_log_probs(ops.as2dc(X), self.cutoff, self.head.word_proj.weight,
                                            self.head.class_proj.weight, self._tails(), topk=k, ban=ban, force=force, **kw)
        return tok.view(B, T, k), lp.view(B, T, k)

    def sample(self, X, k, temp, seed_dev, step, row_ids=None, topp=None, force=None, rule=None, pen=None, mask=None,
               stats=None):
        """One top-k draw with temperature per position (transformer_faces_objects.py:443-470: lprobs.topk(k), / temp,
        multinomial), fused like `greedy`: -> (token [B, T], log-prob [B, T] WITHOUT the temperature).  seed_dev: int32 [1]
        device word holding the seed; step: host step index or the int32 [1] device counter of a captured step (step - 1);
        row_ids: int32 [B * T] original batch rows (compacted batches), default the row index
        (include/tell_hip.h tell_adaptive_logprob_sample).  topp = p: the nucleus draw instead (k = 0: no top-k cut;
        tell_adaptive_logprob_nucleus) - the same launches up to the last one.  rule = 'minp' / 'typical': topp is that
        rule's parameter (m / tau; k = 0; tell_adaptive_logprob_minp / tell_adaptive_logprob_typical).
        pen (as in `topk`; the top-k draw only): the draw runs over the penalised scores and the second result is the drawn
        token's score (tell_adaptive_logprob_sample_penalised).
        mask (as in `topk`; the top-k draw only): the candidates are the k best tokens that are not masked
        (tell_adaptive_logprob_sample_masked)."""
        if pen is not None and (topp is not None or rule is not None):
            raise ValueError('sample: penalties go with the top-k draw, not with sampling_topp / sampling_minp / sampling_typical')
        if mask is not None and (topp is not None or rule is not None or pen is not None):
            raise ValueError('sample: a vocabulary mask goes with the top-k draw, not with sampling_topp / sampling_minp / '
                             'sampling_typical or the penalties')
        B, T, E = X.shape
        kw = {'pen': pen} if pen is not None else {}
        if mask is not None:
            kw['mask'] = mask
        if stats is not None:
            kw['stats'] = stats
        sample = (int(k), 1.0 / float(temp), seed_dev, row_ids, step)
        if topp is not None:
            sample = sample + (float(topp),)
        if rule is not None:
            sample = sample + (rule,)
        tok, lp, _ = ops.adaptive_log_probs(ops.as2dc(X), self.cutoff, self.head.word_proj.weight,
                                            self.head.class_proj.weight, self._tails(), sample=sample, force=force, **kw)
        return tok.view(B, T), lp.view(B, T)

    def greedy(self, X, force=None, mask=None, stats=None):
        """Fused arg-max over the full vocabulary (get_log_prob + topk(1),
        transformer_faces_objects.py:443-464) without materialising [N, vocab].
        force (here, in `topk` and in `sample`): the forcing table of a caption completion (ops.logprob_forced) - rows with
        prefix left take the prefix token and its log-prob instead of the pick.
        mask (as in `topk`): the arg-max over the tokens that are not masked - `topk` with k = 1."""
        B, T, E = X.shape
        skw = {'stats': stats} if stats is not None else {}
        if mask is not None:
            tok, lp = self.topk(X, 1, force=force, mask=mask, **skw)
            return tok.view(B, T), lp.view(B, T)
        tok, lp, _ = ops.adaptive_log_probs(ops.as2dc(X), self.cutoff, self.head.word_proj.weight,
                                            self.head.class_proj.weight, self._tails(), force=force, **skw)
        return tok.view(B, T), lp.view(B, T)
