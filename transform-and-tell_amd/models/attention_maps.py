"""The per-word attention view of a generated caption: what the reference's `generate()` returns
(tell/models/transformer_faces_objects.py:142-309), computed on the host from the device maps of
`model.generate(..., attention=True)`.

For every generated WORD (BPE pieces merged) the view says how much each decoder layer looked at every article word,
image region, face and object while the word was produced:

    [{'tokens': 'Milan',
      'attns': {'article': [{'text': 'The', 'attns': [l0, l1, ..]}, ...],     # one entry per article word
                'image':   [[49 floats] per layer], 'faces': [[..] per layer], 'obj': [[..] per layer]}}, ...]

Rules restated from the reference:
  * article pieces: padding removed, then a leading <s> and a trailing </s>; a piece opens a new article word when it is
    the first one, starts with 'Ġ' (space) or 'Ċ' (newline), or follows a piece that starts with 'Ċ' (:189-213);
  * an article word's weight is the MEAN over its pieces' columns (:236-247);
  * generated pieces: <s> and </s> dropped; a piece opens a new generated word when it is the first one or starts with 'Ġ'
    (:250); every weight of a generated word is the MEAN over the word's pieces (the reference sums, then divides, :252-262).
  * piece j of a step is the decoder step that produced it: step j of the maps.

Departures, both deliberate:
  * COLUMN OFFSET.  The reference strips <s> from the article ids but slices the weights from column 0 (:244-252), so
    every article word reads one column early (the first word gets <s>'s weight).  Here piece j of the article without
    <s> reads column j + 1, the column of its own key.
  * VIRTUAL KEYS.  The last two columns of every map (the learned bias_k key and the zero key) are not positions of any
    context; they are dropped from the image / faces / obj lists as they are from the article words (the reference keeps
    them at the end of those three vectors).
A static batch keeps computing rows after their </s>: 'attn_steps' counts a row's steps including the one that produced
</s>; that step and everything after it are ignored.
Contexts the model does not feed its decoder are absent keys."""
import torch


def _piece_strings(ids, rb):
    """fairseq ids -> byte-level BPE piece strings (the dictionary symbol is the GPT-2 id as text; anything else - <unk>,
    madeupword - stays its own symbol)."""
    d, dec = rb.source_dictionary, rb.bpe.decoder
    out = []
    for i in ids:
        sym = d.symbols[int(i)] if 0 <= int(i) < len(d) else '<unk>'
        out.append(dec.get(int(sym), sym) if sym.isdigit() else sym)
    return out


def _text(pieces, rb):
    bd = rb.bpe.byte_decoder
    raw = bytearray()
    for c in ''.join(pieces):
        if c in bd:
            raw.append(bd[c])
        else:
            raw.extend(c.encode('utf-8'))
    return raw.decode('utf-8', errors='replace')


def merge_article(pieces):
    """-> list of (first piece index, one past the last) per article word."""
    words, newline = [], False
    for j, b in enumerate(pieces):
        if j == 0 or b[:1] in ('Ġ', 'Ċ') or newline:
            words.append([j, j + 1])
            newline = b[:1] == 'Ċ'
        else:
            words[-1][1] = j + 1
    return [tuple(w) for w in words]


def merge_generated(pieces):
    words = []
    for j, b in enumerate(pieces):
        if j == 0 or b[:1] == 'Ġ':
            words.append([j, j + 1])
        else:
            words[-1][1] = j + 1
    return [tuple(w) for w in words]


def caption_attention(model, batch, gen, bpe=None):
    """batch: the batch `generate` was given (its `context[index]` holds the article ids); gen: generate's output with
    attention=True ('gen_ids', 'attns', 'attn_steps').  bpe: an object with `.bpe` (data.bpe.ByteBPE: decoder,
    byte_decoder) and `.source_dictionary` (data.bpe.FairseqDictionary) - default: the installed RoBERTa files
    (data.indexers.bpe_directory; FileNotFoundError when they are absent).
    -> one list per caption of {'tokens': word, 'attns': {...}} (module docstring)."""
    attns = gen.get('attns')
    if not isinstance(attns, dict) or 'attn_steps' not in gen:
        raise ValueError('caption_attention needs the output of generate(..., attention=True)')
    if bpe is None:
        from ..data.bpe import RobertaBPE
        from ..data.indexers import bpe_directory
        bpe = RobertaBPE(bpe_directory())
    d = bpe.source_dictionary
    pad = int(getattr(model, 'padding_idx', d.pad_index))
    index = getattr(model, 'index', 'roberta')
    gen_ids = torch.as_tensor(gen['gen_ids']).cpu().tolist()
    n_steps = torch.as_tensor(gen['attn_steps']).cpu().tolist()
    maps = {k: v.detach().to(torch.float64).cpu() for k, v in attns.items()}         # [B, steps, L, S + 2]
    if not isinstance(batch.get('context'), dict) or index not in batch['context']:
        raise ValueError('caption_attention needs the article ids of the batch (context[%r])' % index)
    article_ids = batch['context'][index].cpu()
    out = []
    for i, row in enumerate(gen_ids):
        art = [int(t) for t in article_ids[i].tolist() if int(t) != pad]
        col0 = 0                                                  # column of the first kept article piece
        if art and art[0] == d.bos_index:
            art, col0 = art[1:], 1
        if art and art[-1] == d.eos_index:
            art = art[:-1]
        art_pieces = _piece_strings(art, bpe)
        art_words = merge_article(art_pieces)
        art_texts = [_text(art_pieces[a:b], bpe) for a, b in art_words]
        toks = row[1:]                                            # (column 0 is the seed the generator was given)
        toks = toks[:int(n_steps[i])]                             # (everything from the row's EOS on is gone)
        if toks and toks[-1] == d.eos_index:
            toks = toks[:-1]
        pieces = _piece_strings(toks, bpe)
        words = []
        for a, b in merge_generated(pieces):
            entry = {'tokens': _text(pieces[a:b], bpe), 'attns': {}}
            for name, m in maps.items():
                S = m.shape[-1] - 2
                w = m[i, a:b].mean(0)                             # mean over the word's pieces -> [L, S + 2]
                if name == 'article':
                    entry['attns'][name] = [
                        {'text': t, 'attns': w[:, col0 + wa:col0 + wb].mean(1).tolist()}
                        for t, (wa, wb) in zip(art_texts, art_words) if col0 + wb <= S]
                else:
                    entry['attns'][name] = w[:, :S].tolist()
            words.append(entry)
        out.append(words)
    return out


def caption_confidence(model, batch, gen, bpe=None):
    """The word-level view of the per-token statistics: gen is generate's output with token_stats=n ('gen_ids', 'alt_ids',
    'token_rank', 'token_entropy', 'token_model_lp').  Generated pieces are merged into words as in `caption_attention`
    (<s> dropped, everything from the row's </s> on ignored; a piece opens a word when it is the first or starts with 'Ġ').
    -> one list per caption of
        {'tokens': word, 'log_prob': the sum of its pieces' token_model_lp, 'entropy': the maximum of its pieces' entropies,
         'rank': the rank of its first piece, 'alternatives': the decoded first-piece alternatives, best first}.
    bpe: as in `caption_attention`.  `batch` is unused (kept for the signature of the attention view).  Host code only."""
    need = ('gen_ids', 'alt_ids', 'token_rank', 'token_entropy', 'token_model_lp')
    if any(k not in gen for k in need):
        raise ValueError('caption_confidence needs the output of generate(..., token_stats=n)')
    if bpe is None:
        from ..data.bpe import RobertaBPE
        from ..data.indexers import bpe_directory
        bpe = RobertaBPE(bpe_directory())
    d = bpe.source_dictionary
    pad = int(getattr(model, 'padding_idx', d.pad_index))
    gen_ids = torch.as_tensor(gen['gen_ids']).cpu().tolist()
    alt =torch.as_tensor(gen['alt_ids']).cpu().tolist()
    rank = torch.as_tensor(gen['token_rank']).cpu().tolist()
    ent = torch.as_tensor(gen['token_entropy']).to(torch.float64).cpu().tolist()
    mlp = torch.as_tensor(gen['token_model_lp']).to(torch.float64).cpu().tolist()
    out = []
    for i, row in enumerate(gen_ids):
        toks = row[1:]                                            # (column 0 is the seed the generator was given)
        for stop in (d.eos_index, pad):                           # (the row's </s> and everything behind it are gone)
            if stop in toks:
                toks = toks[:toks.index(stop)]
        pieces = _piece_strings(toks, bpe)
        words = []
        for a, b in merge_generated(pieces):
            words.append({'tokens': _text(pieces[a:b], bpe), 'log_prob': float(sum(mlp[i][a:b])),
                          'entropy': float(max(ent[i][a:b])), 'rank': int(rank[i][a]),
                          'alternatives': [_text(_piece_strings([t], bpe), bpe) for t in alt[i][a] if 0 <= int(t) < len(d)]})
        out.append(words)
    return out
