"""Hypothesis batches for the grouped copy decision (csrc/copy_decode.hip tell_copy_decide_hyp), built
from the case tables of tests/copy_decode_cases.py, and its definition: tell_copy_decide - in float64 copy_ref.copy_step - over
the batch with every image's keys, mask, proper mask and ids repeated n times.  numpy only.

A batch of n hypotheses per image: row r = b * n + j is hypothesis j of image b.  Hypothesis (b, 0) carries case row b's own
query, entity logits, gen_tok and hist, hypothesis (b, j > 0) those of case row (b + j) mod B; the keys, mask, proper mask
and ids are the case's, one row per image.  Finished flags: (b, 0) keeps the case's flag, (b, j > 0) is live, and
  n >= 2: every hypothesis of image DEAD is finished (DEAD: the case's first finished row, else its last row);
  n >= 3: of image BETWEEN (the first image besides DEAD whose case row is live) hypothesis 1 is finished, 0 and 2 are live."""
import numpy as np

import copy_decode_cases as cdc
import copy_ref as ref

N_HYP = (1, 2, 3, 5, 16)              # one chunk of every size below 4, a ragged last chunk (4 + 1), the limit (4 chunks)


def marked_images(x, n):
    """-> (DEAD, BETWEEN), None where n is too small for the pattern"""
    fin = np.asarray(x['fin'])
    B = len(fin)
    dead = (int(np.flatnonzero(fin)[0]) if fin.any() else B - 1) if n >= 2 else None
    between = next(b for b in range(B) if b != dead and not fin[b]) if n >= 3 else None
    return dead, between


def hyp_batch(x, n):
    """case x (copy_decode_cases.from_step / extra) -> the batch of n hypotheses per image: q, ent, gen, fin, hist R = B * n rows
    tall, k / mask / proper / ctx / bias_k the case's own arrays (one row per image)"""
    B = len(x['fin'])
    src = np.array([(b + j) % B for b in range(B) for j in range(n)])
    fin = np.zeros(B * n, np.uint8)
    fin[::n] = x['fin']
    dead, between = marked_images(x, n)
    if dead is not None:
        fin[dead * n:(dead + 1) * n] = 1
    if between is not None:
        fin[between * n + 1] = 1
    return dict(x, q=x['q'][src], ent=x['ent'][src], gen=x['gen'][src], hist=np.asarray(x['hist'])[src], fin=fin, n=n, src=src)


def expand(h):
    """the batch tell_copy_decide would have to be given: every image's keys, mask, proper mask and ids repeated n times"""
    n = h['n']
    rep = lambda a, axis: None if a is None else np.repeat(a, n, axis=axis)          # noqa: E731
    e = dict(h, k=rep(h['k'], 1), mask=rep(h['mask'], 0), proper=rep(h['proper'], 0), ctx=rep(h['ctx'], 0))
    del e['n'], e['src']
    return e


def expected(h):
    """the float64 definition of the hypothesis batch: copy_decode_cases.expected over the expanded batch"""
    return cdc.expected(expand(h))


def cases():
    """[(id, maker)]: the tables of copy_decode_cases, makers taking (dtype, n)"""
    def hyp(cid, make):
        return lambda dtype, n: ref.cached(('hyp', cid, dtype, n), lambda: hyp_batch(make(dtype), n))
    return [(cid, hyp(cid, make)) for cid, make in cdc.cases()]
