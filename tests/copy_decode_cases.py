"""The case tables of the static-batch copy decision (csrc/copy_decode.hip tell_copy_decide) that tests/test_copy_decode_host.py
and tests/test_gpu_copy_decode.py both walk, and its definition in terms of the float64 reference of tests/copy_ref.py:
copy_ref.copy_step called with rows = the unfinished rows; a finished row keeps its hist / copied / prob columns and its tok.
numpy only (torch for the seeded inputs, as in copy_ref)."""
import numpy as np

import copy_ref as ref

FINISHED_ROW = 1                      # of the B = 4 rows of copy_ref.STEP: STEP_ROWS = (2, 0, 3) are the unfinished ones

# further cases: id, (B, H, S, D), step p, history length L
#   X512: the LDS limit, several passes per thread; row 0 copies, row 1 is refused by the entity logits
#   X37:  ragged tails (S and D no multiple of anything); row 0 copies, row 1 is refused by hist, row 2 holds one id whose
#         positions are all improper (p < 1e-6), row 3 is finished
EXTRA = [dict(id='X512', shape=(2, 16, 512, 64), p=0, L=2), dict(id='X37', shape=(4, 3, 37, 16), p=1, L=3)]


def from_step(case, dtype):
    """a case of copy_ref.STEP as a static batch: row rows[i] holds alive row i's query, entity logits and pick"""
    def make():
        x = ref.step_inputs(case, dtype)
        Ba, B, H, S, D = case['shape']
        E = H * D
        g = ref._gen(4000 + S)
        q = ref._round(ref._randn(g, B, E) * 0.6, dtype)
        ent = np.array([[0.0, 3.0]] * B, np.float32)              # the finished row WOULD copy
        gen = np.full(B, 77, np.int64)
        fin = np.ones(B, np.uint8)
        for i, b in enumerate(x['rows']):
            q[b], ent[b], gen[b], fin[b] = x['q'][i], x['ent'][i], x['gen'][i], 0
        return dict(q=q, k=x['k'], bias_k=x['bias_k'], mask=x['mask'], proper=x['proper'], ctx=x['ctx'], ent=ent, gen=gen, fin=fin,
                    hist=x['hist'], p=x['n_hist'] - 1, L=ref.HIST_LEN - 1, H=H, tie=bool(case.get('tie')))
    return ref.cached(('decide', case['id'], dtype), make)


def extra(case, dtype):
    def make():
        import torch
        B, H, S, D = case['shape']
        E, p, L = H * D, case['p'], case['L']
        g = ref._gen(7000 + S + D)
        q, k, bk = ref._randn(g, B, E) * 0.6, ref._randn(g, S, B, E) * 0.6, ref._randn(g, E) * 0.3
        m, pr = ref._masks(B, S, 'tail', 'mixed')
        pr[:, ::2] = 1
        ctx = torch.randint(3, 40, (B, S), generator=g).numpy()
        ent = np.array([[0.0, 1.0]] * B, np.float32)
        fin = np.zeros(B, np.uint8)
        hist = np.full((B, L + 1), -1, np.int64)
        hist[:, 0] = 1000 + np.arange(B)
        if case['id'] == 'X512':
            ent[1] = [1.0, 0.5]
        x = dict(q=ref._round(q, dtype), k=ref._round(k, dtype), bias_k=ref._round(bk, dtype), mask=m, proper=pr, ctx=ctx, ent=ent,
                 gen=np.arange(B, dtype=np.int64) + 11, fin=fin, hist=hist, p=p, L=L, H=H, tie=False)
        if case['id'] == 'X37':
            ctx[2], pr[2] = 9, 0
            fin[3] = 1
            hist[1, p] = expected(x)['best_id'][1]                 # the id row 1 would copy sits in its history
        return x
    return ref.cached(('decide', case['id'], dtype), make)


def cases():
    """[(id, maker)] of every case the GPU kernel test uses"""
    return [('step_' + c['id'], (lambda dtype, c=c: from_step(c, dtype))) for c in ref.STEP] + \
        [(c['id'], (lambda dtype, c=c: extra(c, dtype))) for c in EXTRA]


def expected(x, **kw):
    """the definition: copy_ref.copy_step over the unfinished rows -> dict rows [Ba], r (copy_step's result, indexed like
    rows) and the static arrays: tok [B] (None where finished), hist [B, L + 1] int64, copied_col / prob_col [B] with
    NaN / -1 where the row is finished and the buffers keep what they held, best_id [B]"""
    rows = np.flatnonzero(np.asarray(x['fin']) == 0).astype(np.int32)
    r = ref.copy_step(x['q'][rows], x['k'], x['bias_k'], x['mask'], x['proper'], x['ctx'], rows, x['ent'][rows], x['gen'][rows],
                      x['hist'], x['p'] + 1, x['H'], **kw)
    B = len(x['fin'])
    hist = np.asarray(x['hist']).copy()
    hist[:, x['p'] + 1] = r['hist_col']
    tok, copied, prob, best = [None] * B, [None] * B, [None] * B, np.zeros(B, np.int64)
    for i, b in enumerate(rows):
        tok[b], copied[b], prob[b], best[b] = int(r['tok'][i]), bool(r['copied'][i]), i, r['best_id'][i]
    return dict(rows=rows, r=r, tok=tok, hist=hist, copied=copied, prob_index=prob, best_id=best)
