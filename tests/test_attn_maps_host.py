"""Host side of the attention maps: the reference's per-word view restated in
models/attention_maps.py, on a hand-made BPE and hand-made maps with expected values worked out by hand; the
configurations generate(attention=True) refuses; the header parse binds the new entry point."""
import json
import os

import pytest
import torch

TOKENS = ['The', 'Ġcat', 'Ġs', 'at', 'Ċ', 'on', 'Ġmat', '.', 'ĠMi', 'lan', 'ĠA', 'Ġin']


def _bpe(d):
    """data/bpe.py's RobertaBPE over a dozen symbols: GPT-2 id i = position in TOKENS, fairseq id = 4 + i."""
    from tell_amd.data.bpe import RobertaBPE
    with open(os.path.join(d, 'encoder.json'), 'w') as f:
        json.dump({t: i for i, t in enumerate(TOKENS)}, f)
    with open(os.path.join(d, 'vocab.bpe'), 'w', encoding='utf-8') as f:
        f.write('#version: 0.2\n')
    with open(os.path.join(d, 'dict.txt'), 'w') as f:
        f.write(''.join('%d 1\n' % i for i in range(len(TOKENS))))
    return RobertaBPE(d)


def _id(tok):
    return 4 + TOKENS.index(tok)


class _Model:
    padding_idx, index = 1, 'roberta'


def _maps(B, steps, L, S):
    """value(b, step, layer, column) = b + 0.1 step + 0.01 layer + 0.001 (column + 1): every mean is easy by hand."""
    b = torch.arange(B, dtype=torch.float64)[:, None, None, None]
    t = torch.arange(steps, dtype=torch.float64)[None, :, None, None]
    l = torch.arange(L, dtype=torch.float64)[None, None, :, None]
    c = torch.arange(S + 2, dtype=torch.float64)[None, None, None, :]
    return (b + 0.1 * t + 0.01 * l + 0.001 * (c + 1)).float()


def test_caption_attention_merges_pieces_into_words_by_hand(tmp_path):
    from tell_amd.models.attention_maps import caption_attention, merge_article, merge_generated
    rb = _bpe(str(tmp_path))
    # boundaries: at 'Ġ', at 'Ċ', and after a 'Ċ' piece
    assert merge_article(['The', 'Ġcat', 'Ġs', 'at', 'Ċ', 'on', 'Ġmat', '.']) == [(0, 1), (1, 2), (2, 4), (4, 5), (5, 6), (6, 8)]
    assert merge_article(['Ċ', 'Ċ', 'on', 'at']) == [(0, 1), (1, 2), (2, 4)]
    assert merge_generated(['ĠMi', 'lan', 'Ċ', 'Ġin']) == [(0, 3), (3, 4)]          # only 'Ġ' opens a generated word
    art = torch.tensor([
        [0] + [_id(t) for t in ('The', 'Ġcat', 'Ġs', 'at', 'Ċ', 'on', 'Ġmat', '.')] + [2, 1, 1],       # <s> 8 pieces </s> pad pad
        [0, _id('ĠA'), _id('Ġcat'), 2] + [1] * 8])
    S = art.shape[1]
    gen_ids = torch.tensor([
        [0, _id('ĠMi'), _id('lan'), _id('Ġin'), _id('ĠA'), 2, 1],      # row 0: </s> at column 5 -> 5 meaningful steps
        [0, _id('The'), _id('Ġcat'), _id('Ġs'), _id('at'), _id('on'), _id('Ġmat')]])      # row 1 never ends
    gen = {'gen_ids': gen_ids, 'attn_steps': torch.tensor([5, 6]),
           'attns': {'article': _maps(2, 6, 2, S), 'image': _maps(2, 6, 2, 3)}}
    out = caption_attention(_Model(), {'context': {'roberta': art}}, gen, bpe=rb)
    assert len(out) == 2
    r0 = out[0]
    # <s>, </s> and everything from the EOS on are gone; pieces merged into words
    assert [w['tokens'] for w in r0] == [' Milan', ' in', ' A']
    assert set(r0[0]['attns']) == {'article', 'image'}                               # no faces / objects: no such keys
    assert [a['text'] for a in r0[0]['attns']['article']] == ['The', ' cat', ' sat', '\n', 'on', ' mat.']
    # ' Milan' = steps 0 and 1 (mean step term 0.05); article word ' sat' = pieces 2, 3 of the article without <s> = columns
    # 3 and 4 (mean column term 0.001 * (4 + 5) / 2 = 0.0045)
    sat = r0[0]['attns']['article'][2]['attns']
    assert sat == pytest.approx([0.05 + 0.0045, 0.05 + 0.01 + 0.0045], abs=1e-6)
    # 'The' reads column 1, not column 0 (<s>): 0.001 * 2
    assert r0[0]['attns']['article'][0]['attns'] == pytest.approx([0.05 + 0.002, 0.05 + 0.01 + 0.002], abs=1e-6)
    # ' mat.' = columns 7, 8 -> 0.001 * (8 + 9) / 2; generated word ' in' = step 2 alone
    assert r0[1]['attns']['article'][5]['attns'] == pytest.approx([0.2 + 0.0085, 0.2 + 0.01 + 0.0085], abs=1e-6)
    # image: the 3 regions, the two virtual columns dropped; ' A' = step 3
    img = r0[2]['attns']['image']
    assert len(img) == 2 and len(img[0]) == 3
    assert img[1] == pytest.approx([0.3 + 0.01 + 0.001, 0.3 + 0.01 + 0.002, 0.3 + 0.01 + 0.003], abs=1e-6)
    # row 1: no </s> - all six steps; article '<s> ĠA Ġcat </s> pad..' -> two words at columns 1, 2
    r1 = out[1]
    assert [w['tokens'] for w in r1] == ['The', ' cat', ' saton', ' mat']            # only 'Ġ' opens a generated word
    # ' saton' = steps 2, 3, 4 (mean step term 0.3), batch row 1, layer 0, image region 0: 1 + 0.3 + 0.001
    assert r1[2]['attns']['image'][0][0] == pytest.approx(1.301, abs=1e-6)
    assert [a['text'] for a in r1[0]['attns']['article']] == [' A', ' cat']
    assert r1[0]['attns']['article'][1]['attns'] == pytest.approx([1 + 0.003, 1 + 0.01 + 0.003], abs=1e-6)
    json.dumps(out)                                                                  # plain lists / floats / strings


def test_caption_attention_needs_maps():
    from tell_amd.models.attention_maps import caption_attention
    with pytest.raises(ValueError):
        caption_attention(_Model(), {'context': {'roberta': torch.zeros(1, 3, dtype=torch.long)}},
                          {'gen_ids': torch.zeros(1, 2, dtype=torch.long), 'attns': []}, bpe=object())


def test_attention_is_refused_for_beam_search_lstm_decoders_and_pointer_models():
    from tell_amd.models.baseline_glove import BaselineGloveModel
    from tell_amd.models.pointer import TransformerPointerModel
    from tell_amd.models.transformer import CaptionModel

    class Conv(torch.nn.Module):
        def project_contexts(self, contexts):
            raise AssertionError('not reached')

    class LSTMDecoder(torch.nn.Module):
        pass

    def shell(cls, dec):
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.decoder, m.sampling_topk, m.sampling_temp, m.sampling_topp, m.index = dec, 1, 1.0, None, 'roberta'
        return m
    kw = dict(context={}, image=None, caption={})
    with pytest.raises(ValueError, match='beam'):
        shell(CaptionModel, Conv()).generate(**kw, beam_size=4, attention=True)
    with pytest.raises(ValueError, match='beam'):
        next(iter(shell(CaptionModel, Conv()).generate_lanes([kw], beam_size=4, attention=True)))
    with pytest.raises(ValueError, match='beam'):
        next(iter(shell(CaptionModel, Conv()).generate_stream([kw], beam_size=2, attention=True)))
    with pytest.raises(ValueError, match='LSTM'):
        shell(CaptionModel, LSTMDecoder()).generate(**kw, attention=True)
    with pytest.raises(ValueError, match='LSTM'):
        shell(BaselineGloveModel, LSTMDecoder()).generate(image=None, caption={}, attention=True)
    with pytest.raises(ValueError, match='pointer'):
        shell(TransformerPointerModel, Conv()).generate(**kw, attention=True)


def test_header_declares_the_exporting_entry_point_and_the_plain_ones_keep_their_signatures():
    """(That the built library resolves every declared symbol is test_abi_and_host.py's job: hip.lib binds them all.)"""
    from tell_amd.hip import parse_header
    protos = parse_header()
    plain, exp = protos['tell_attn_decode'], protos['tell_attn_decode_weights']
    assert len(plain[2]) == 22 and plain[2][-1] == 'stream' and plain[2][-2] == 'beams'
    assert exp[2][:21] == plain[2][:21]                              # everything tell_attn_decode takes, in its order
    assert exp[2][21:] == ['lse_ws', 'w', 'w_st', 'w_sb', 'slot', 'n_slots', 'step_dev', 'stream']
    assert len(protos['tell_attn_decode_packed'][2]) == 13


# ------------------------------------------------------------------------------------------------ commands/evaluate.py
class _StubModel(torch.nn.Module):
    """What evaluate() drives, on the CPU: forward() in evaluate mode returns the fields of CaptionModel.forward; with
    `eval_attention` set it adds the maps, as CaptionModel does."""
    EVAL_ATTENTION = True
    padding_idx, index = 1, 'roberta'

    def __init__(self, fail_at=None):
        super().__init__()
        self.evaluate_mode, self.calls, self.fail_at, self.seen = False, 0, fail_at, []

    def _check_attention(self, beam_size=1):
        if int(beam_size) > 1:
            raise ValueError('beam')

    def caption_attention(self, batch, gen, bpe=None):
        from tell_amd.models.attention_maps import caption_attention
        return caption_attention(self, batch, gen, bpe=bpe)

    def forward(self, context, metadata):
        self.calls += 1
        self.seen.append(bool(getattr(self, 'eval_attention', False)))
        if self.fail_at == self.calls:
            raise RuntimeError('boom')
        B, S = context['roberta'].shape
        gen_ids = torch.tensor([[0, _id('ĠMi'), _id('lan'), 2]] * B)
        out = {'loss': torch.tensor(2.0), 'gen_ids': gen_ids.numpy(), 'generations': [' Milan'] * B,
               'captions': [m['caption'] for m in metadata], 'metadata': metadata, 'attns': []}
        if getattr(self, 'eval_attention', False):
            out['attns'] = {'article': _maps(B, 3, 2, S), 'image': _maps(B, 3, 2, 3)}
            out['attn_steps'] = torch.full((B,), 3)
        return out

    def get_metrics(self, reset=False):
        return {}


def _eval_batches():
    art = torch.tensor([[0, _id('The'), _id('Ġcat'), 2], [0, _id('ĠA'), 2, 1]])
    meta = [{'caption': 'a cat', 'web_url': 'u0', 'image_path': 'p0', 'context': 'c0'},
            {'caption': 'A', 'web_url': 'u1', 'image_path': 'p1', 'context': 'c1'}]
    return [dict(context={'roberta': art}, metadata=meta)]


def _iterator(instances, num_epochs=1, shuffle=False, device=None):
    return list(instances)


def test_evaluate_adds_the_word_view_only_when_asked(tmp_path):
    from tell_amd.commands.evaluate import _ttr, evaluate
    rb = _bpe(str(tmp_path))
    off_dir, on_dir = str(tmp_path / 'off'), str(tmp_path / 'on')
    m = _StubModel()
    evaluate(m, _eval_batches(), _iterator, -1, off_dir)
    assert m.seen == [False] and m.eval_attention is False
    # off: the file is, byte for byte, the record the command always wrote (keys and order of write_to_json before the option)
    want = ''
    for meta in _eval_batches()[0]['metadata']:
        want += json.dumps({'caption': meta['caption'], 'raw_caption': meta['caption'], 'generation': ' Milan',
                            'copied_texts': '', 'web_url': meta['web_url'], 'image_path': meta['image_path'],
                            'context': meta['context'], 'caption_np': _ttr(meta['caption']), 'gen_np': _ttr(' Milan')}) + '\n'
    assert open(os.path.join(off_dir, 'generations.jsonl')).read() == want
    m = _StubModel()
    evaluate(m, _eval_batches(), _iterator, -1, on_dir, attention_maps=True, bpe=rb)
    assert m.seen == [True] and m.eval_attention is False
    recs = [json.loads(ln) for ln in open(os.path.join(on_dir, 'generations.jsonl'))]
    assert len(recs) == 2
    for b, (rec, off_line) in enumerate(zip(recs, want.splitlines())):
        words = rec.pop('attns')
        assert rec == json.loads(off_line)                                  # nothing else changes
        assert [w['tokens'] for w in words] == [' Milan'] and set(words[0]['attns']) == {'article', 'image'}
    # record 0: ' Milan' = steps 0, 1 (the </s> step dropped); article word 'The' = column 1 -> 0.05 + 0.002 in layer 0
    art = json.loads(open(os.path.join(on_dir, 'generations.jsonl')).readline())['attns'][0]['attns']['article']
    assert [a['text'] for a in art] == ['The', ' cat']
    assert art[0]['attns'] == pytest.approx([0.052, 0.062], abs=1e-6)


def test_evaluate_refuses_models_without_maps_and_never_leaves_the_switch_on(tmp_path):
    from tell_amd.commands.evaluate import evaluate
    from tell_amd.models.baseline_glove import TransformerGloveModel
    from tell_amd.models.pointer import TransformerPointerModel
    rb = _bpe(str(tmp_path))
    for n, cls in enumerate((TransformerPointerModel, TransformerGloveModel)):
        model = cls.__new__(cls)
        torch.nn.Module.__init__(model)
        with pytest.raises(ValueError):
            evaluate(model, [], _iterator, -1, str(tmp_path / ('refused%d' % n)), attention_maps=True, bpe=rb)
        assert not getattr(model, 'eval_attention', False)
    with pytest.raises(ValueError, match='beam'):
        evaluate(_StubModel(), _eval_batches(), _iterator, -1, str(tmp_path / 'beam'), beam_size=4, attention_maps=True, bpe=rb)

    class Ignores(_StubModel):                                              # generates, but without maps: refused, not silent
        def forward(self, context, metadata):
            out = super().forward(context, metadata)
            out['attns'] = []
            return out
    with pytest.raises(ValueError, match='without attention maps'):
        evaluate(Ignores(), _eval_batches(), _iterator, -1, str(tmp_path / 'ignores'), attention_maps=True, bpe=rb)
    m = _StubModel(fail_at=1)
    with pytest.raises(RuntimeError, match='boom'):
        evaluate(m, _eval_batches(), _iterator, -1, str(tmp_path / 'raises'), attention_maps=True, bpe=rb)
    assert m.seen == [True] and m.eval_attention is False


def test_generate_with_maps_runs_without_autograd():
    """generate(attention=True) outside a no_grad block: the cached generator is entered through _generate_cached, which
    switches autograd off as the plain path does."""
    from tell_amd.models.transformer import AttnMaps, CaptionModel

    class Conv(torch.nn.Module):
        def project_contexts(self, contexts):
            return []
    m = CaptionModel.__new__(CaptionModel)
    torch.nn.Module.__init__(m)
    m.decoder, m.sampling_topk, m.sampling_temp, m.sampling_topp, m.index = Conv(), 1, 1.0, None, 'roberta'
    seen = {}

    def steps(self, caption_ids, contexts, gen_len=100, eos=2, check_every=8, lane=0, seed=None, plan=None):
        seen['grad'], seen['attention'] = torch.is_grad_enabled(), plan.attention
        return None, None, AttnMaps({}, torch.zeros(1))
        yield                                                               # (a generator, like _greedy_steps)
    m._greedy_steps = steps.__get__(m)
    assert torch.is_grad_enabled()
    _, _, third = m._generate(torch.zeros(1, 1, dtype=torch.long), {}, attention=True)
    assert seen == {'grad': False, 'attention': True} and isinstance(third, AttnMaps)
    out = CaptionModel._attn_output({}, third)
    assert set(out) == {'attns', 'attn_steps'} and CaptionModel._attn_output({}, []) == {'attns': []}
