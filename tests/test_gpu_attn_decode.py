"""The one-query attentions of a generation step (csrc/decode.hip: attn_decode_kernel<NQ, LSE>, attn_decode_packed_kernel)
through the C ABI, element by element against the float64 reference and the bounds of tests/decode_ref.py (DESIGN.md
section 33).  Every operand and every output is a view inside a buffer of sentinels (tests/guarded.py): after each launch
the guard bands, the row gaps and the columns of the wider q / out buffers are intact.  Exact checks: a (row, head) without a
live key is +0.0 / -inf, the three cache layouts give bit-equal outputs, a second launch repeats the first bit for bit, the
exporting entry point's out is tell_attn_decode's, and a refused call launches nothing.
Run on the MI355X box:  python -m pytest tests/test_gpu_attn_decode.py -m gpu -s   (-s prints the ratios c is pinned from and
the time of the whole file)"""
import time
import types

import numpy as np
import pytest
import torch

import decode_ref as ref
from guarded import DEV, Guard

pytestmark = pytest.mark.gpu

F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
_RATIOS, _UNPINNED = {}, {}
IDS = [L['id'] for L in ref.ATTN]


@pytest.fixture(autouse=True)
def _gpu():
    import tell_amd
    tell_amd.hip.require_gpu()
    _UNPINNED.clear()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:                  # a device fault: every later launch of this process would fail the same way
        pytest.exit('GPU error, nothing more is launched: %s' % err, 3)


@pytest.fixture(scope='module', autouse=True)
def _report():
    t0 = time.time()
    yield
    for k in sorted(_RATIOS):
        print('\nlargest (|got - ref| - u_out |ref|) / (gamma 2^-24 S)  %-12s %.6f   c = %s' % (k, _RATIOS[k], ref.C.get(k)))
    print('\ntests/test_gpu_attn_decode.py: %.1f s' % (time.time() - t0))


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def bits(t):
    return t.contiguous().view(torch.int16)


def check(out, got, r, tag, extra=0.0):
    """element-wise bound of decode_ref on `out` of one context (r: its float64 reference); rows without a live key must be
    +0.0 exactly; the ratio c is pinned from is recorded"""
    got, want, S = ref.np64(got), r['out'], r['S_out']
    assert np.isfinite(got).all(), (out, tag)
    gam = ref.attn_gamma('out', r)
    rt = ref.ratio(got, want, S, 'bfloat16', gam, extra)
    _RATIOS[out] = max(_RATIOS.get(out, 0.0), rt)
    print('ratio %-12s %-44s %.6f' % (out, tag, rt))
    dead = np.repeat(~r['has'], 64, -1)
    assert not got[dead].any() and not np.signbit(got[dead]).any(), '%s %s: a row without keys is +0.0' % (out, tag)
    if out not in ref.C:
        _UNPINNED[out] = max(_UNPINNED.get(out, 0.0), rt)
        return
    err, b = np.abs(got - want), ref.bound(out, want, S, 'bfloat16', gam, extra=extra)
    bad = err > b
    assert not bad.any(), '%s %s: %d of %d outside the bound, worst error %.3g at bound %.3g (ratio %.3f, c = %g)' % (
        out, tag, bad.sum(), bad.size, err[bad].max(), b[bad][err[bad].argmax()], rt, ref.C[out])


def check_lse(got, r, tag):
    got, want = ref.np64(got), r['lse2']
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), 'ad_lse2 %s: a row without keys is -inf' % tag
    assert np.isfinite(got[fin]).all(), tag
    gam = ref.attn_gamma('lse', r)
    rt = ref.ratio(got[fin], want[fin], r['S_lse'][fin], 'float32', gam)
    _RATIOS['ad_lse2'] = max(_RATIOS.get('ad_lse2', 0.0), rt)
    print('ratio %-12s %-44s %.6f' % ('ad_lse2', tag, rt))
    if 'ad_lse2' not in ref.C:
        _UNPINNED['ad_lse2'] = max(_UNPINNED.get('ad_lse2', 0.0), rt)
        return
    err, b = np.abs(got - want)[fin], ref.bound('ad_lse2', want[fin], r['S_lse'][fin], 'float32', gam)
    assert not (err > b).any(), 'ad_lse2 %s: worst error %.3g (ratio %.3f, c = %g)' % (tag, err.max(), rt, ref.C['ad_lse2'])


def settle():
    """until c is pinned the test fails with the measured ratio in its message"""
    assert not _UNPINNED, 'constant not pinned yet, largest ratios of this case: %s' % \
        ', '.join('%s %.6f' % kv for kv in sorted(_UNPINNED.items()))


def intact(*guards):
    torch.cuda.synchronize()
    for i, g in enumerate(guards):
        assert g is None or g.intact(), 'store outside view %d of the launch' % i


def declined(name, *args):
    """the return code of a call the library declines (a negative code arrives as the RuntimeError of hip.call_rc)"""
    from tell_amd import hip
    try:
        return hip.call_rc(name, *args)
    except RuntimeError as err:
        assert name in str(err)
        return -1


class Launch:
    """the guarded operands of one launch of the table at a beam width: q and out per context (laid out as the case says),
    masks, bias rows, and the cache in the layout asked for"""

    def __init__(self, L, beams):
        self.L, self.beams = L, beams
        self.Bs, self.H = L.get('samples', 3), L['H']
        self.E, self.B = self.H * 64, self.Bs * beams
        self.x = ref.attn_inputs(L)
        E, B = self.E, self.B
        self.q_sb, self.o_sb = (2 * E if L.get('qwide') else E), (4 * E if L.get('owide') else E)
        self.q = [Guard((B, E), BF16, (self.q_sb, 1), dev(x['q'][:, :beams].reshape(B, E), BF16), off=8 * c)
                  for c, x in enumerate(self.x)]
        self.mask = [None if x['mask'] is None else Guard(x['mask'].shape, U8, fill=x['mask']) for x in self.x]
        self.bk = [Guard((E,), BF16, fill=dev(x['bias_k'], BF16)) for x in self.x]
        self.bv = [Guard((E,), BF16, fill=dev(x['bias_v'], BF16)) for x in self.x]

    def outs(self):
        return [Guard((self.B, self.E), BF16, (self.o_sb, 1)) for _ in self.x]

    def cache(self, lay):
        """-> guards, (k, v tensors), strides per context; an empty context passes q and zero strides (what the stepper does)"""
        Bs, H, E = self.Bs, self.H, self.E
        gs, kv, st = [], [], []
        for c, (S, x) in enumerate(zip(self.L['S'], self.x)):
            if S == 0:
                kv.append((self.q[c].t, self.q[c].t))
                st.append((0, 0, 64))
                continue
            if lay == 'inter':
                g = Guard((S, Bs, 2 * E), BF16, fill=dev(np.concatenate([x['k'], x['v']], -1), BF16))
                gs.append(g)
                kv.append((g.t[..., :E], g.t[..., E:]))
                st.append((2 * Bs * E, 2 * E, 64))
                continue
            shape, strides = ((S, Bs, E), None) if lay == 'row' else ((S, Bs, H, 64), (64, H * S * 64, S * 64, 1))
            gk, gv = (Guard(shape, BF16, strides, dev(x[n].reshape(shape), BF16)) for n in ('k', 'v'))
            gs += [gk, gv]
            kv.append((gk.t, gv.t))
            st.append((Bs * E, E, 64) if lay == 'row' else (64, H * S * 64, S * 64))
        return gs, kv, st

    def everything(self):
        return self.q + self.mask + self.bk + self.bv

    def valu_args(self, lay, outs, kv, st):
        from tell_amd.decode import _ints, _longs, _ptrs
        L, n, virt = self.L, len(self.x), self.L['virt']
        sh = None if lay == 'row' else _longs([s[2] for s in st])            # row-major: the null k_sh / v_sh path
        return (n, _ptrs([g.t for g in self.q]), _longs([self.q_sb] * n), _ptrs([k for k, _ in kv]), _longs([s[0] for s in st]),
                _longs([s[1] for s in st]), sh, _ptrs([v for _, v in kv]), _longs([s[0] for s in st]), _longs([s[1] for s in st]),
                sh, _ptrs([None if g is None else g.t for g in self.mask]),
                _ptrs([g.t for g in self.bk]) if 'k' in virt else None, _ptrs([g.t for g in self.bv]) if 'v' in virt else None,
                1 if 'z' in virt else 0, _ints(list(L['S'])), _ptrs([g.t for g in outs]), _longs([self.o_sb] * n), self.B, self.H,
                self.beams)


def run_valu(la, lay):
    from tell_amd import hip
    outs = la.outs()
    gs, kv, st = la.cache(lay)
    hip.call('tell_attn_decode', *la.valu_args(lay, outs, kv, st))
    intact(*(la.everything() + gs + outs))
    return outs


@pytest.mark.parametrize('which', ['two', 'wide'])
@pytest.mark.parametrize('L', ref.ATTN, ids=IDS)
def test_attn_decode(L, which):
    """NQ = 2 (beams 2) and NQ = 4 (the wide beam of the launch): bounds in the case's layout, the other two layouts and a
    second launch bit-equal"""
    beams = 2 if which == 'two' else L['wide']
    la, want = Launch(L, beams), ref.launch_ref(L, beams)
    outs = run_valu(la, L['klay'])
    name = 'ad_out_nq%d' % ref.nq_of(beams)
    for c, (o, r) in enumerate(zip(outs, want)):
        check(name, o.t, r, '%s beams %d context %d' % (L['id'], beams, c))
    for lay in ('row', 'head', 'inter'):
        again = run_valu(la, lay)
        for c, (a, o) in enumerate(zip(again, outs)):
            assert torch.equal(bits(a.t), bits(o.t)), '%s context %d: layout %s differs from %s' % (L['id'], c, lay, L['klay'])
    settle()


@pytest.mark.parametrize('L', ref.ATTN, ids=IDS)
def test_attn_decode_one_hypothesis_and_lse(L):
    """beams = 1: tell_attn_decode (NQ = 1) against the bounds, and tell_attn_decode_weights (the LSE form): its out bit-equal,
    its lse2 against the bounds; a second launch of it repeats the first"""
    from tell_amd import hip
    from tell_amd.decode import _longs, _ptrs
    la, want = Launch(L, 1), ref.launch_ref(L, 1)
    lay, n = L['klay'], len(L['S'])
    outs = run_valu(la, lay)
    for c, (o, r) in enumerate(zip(outs, want)):
        check('ad_out_nq1', o.t, r, '%s beams 1 context %d' % (L['id'], c))
    seen = []
    for _ in range(2):
        outs2, lse = la.outs(), Guard((n, la.B, la.H), F32)
        w = [Guard((1, la.B, S + 2), F32) for S in L['S']]
        gs, kv, st = la.cache(lay)
        hip.call('tell_attn_decode_weights', *la.valu_args(lay, outs2, kv, st), lse.t, _ptrs([g.t for g in w]),
                 _longs([la.B * (S + 2) for S in L['S']]), _longs([S + 2 for S in L['S']]), 0, 1, None)
        intact(*(la.everything() + gs + outs2 + w + [lse]))
        for c, (a, o) in enumerate(zip(outs2, outs)):
            assert torch.equal(bits(a.t), bits(o.t)), '%s context %d: out of the exporting entry point differs' % (L['id'], c)
        seen.append(lse.t.clone())
    assert torch.equal(seen[0].view(torch.int32), seen[1].view(torch.int32))
    for c, r in enumerate(want):
        check_lse(seen[0][c], r, '%s context %d' % (L['id'], c))
    settle()


@pytest.mark.parametrize('which', ['one', 'wide'])
@pytest.mark.parametrize('L', ref.ATTN, ids=IDS)
def test_attn_decode_packed(L, which):
    """the matrix-core kernel over decode.PackedKV (both virtual keys, always): beams 1 and the wide beam (17: two groups)"""
    from tell_amd import decode, hip
    from tell_amd.decode import _ints, _longs, _ptrs
    beams = 1 if which == 'one' else L['wide']
    la, want = Launch(L, beams), ref.launch_ref(L, beams, 'packed')
    n = len(L['S'])
    kc, vt, mk, Sp = [], [], [], []
    for S, x in zip(L['S'], la.x):
        mod = types.SimpleNamespace(num_heads=la.H, bias_k=dev(x['bias_k'], BF16).to(DEV).view(1, 1, -1),
                                    bias_v=dev(x['bias_v'], BF16).to(DEV).view(1, 1, -1))
        pk = decode.PackedKV(mod, S, la.Bs, DEV)
        pk.fill(dev(x['k'], BF16).to(DEV), dev(x['v'], BF16).to(DEV), None if x['mask'] is None else dev(x['mask'], U8).to(DEV))
        kc.append(Guard(pk.kc.shape, BF16, fill=pk.kc))
        vt.append(Guard(pk.vt.shape, BF16, fill=pk.vt))
        mk.append(Guard(pk.mask.shape, U8, fill=pk.mask))
        Sp.append(pk.Sp)
    seen = []
    for _ in range(2):
        outs = la.outs()
        hip.call('tell_attn_decode_packed', n, _ptrs([g.t for g in la.q]), _longs([la.q_sb] * n), _ptrs([g.t for g in kc]),
                 _ptrs([g.t for g in vt]), _ptrs([g.t for g in mk]), _ints(Sp), _ptrs([g.t for g in outs]), _longs([la.o_sb] * n),
                 la.B, la.H, beams)
        intact(*(la.q + kc + vt + mk + outs))
        seen.append(outs)
    for c, (a, o, r) in enumerate(zip(seen[1], seen[0], want)):
        assert torch.equal(bits(a.t), bits(o.t)), '%s context %d: the second launch differs' % (L['id'], c)
        check('pk_out', o.t, r, '%s beams %d context %d' % (L['id'], beams, c), extra=ref.PK_PROB * r['S_out'])
    settle()


def test_refused_calls_launch_nothing():
    """S = 2049, no keys at all, q_sb not a multiple of 8, Sp not a multiple of 32: an error, and the outputs stay sentinel"""
    from tell_amd.decode import _ints, _longs, _ptrs
    Bs, H = 2, 2
    E = H * 64
    q, out = Guard((Bs, 2 * E), BF16, fill=torch.zeros(Bs, 2 * E)), Guard((Bs, 2 * E), BF16)
    k = Guard((2049, Bs, E), BF16, fill=torch.zeros(2049, Bs, E))
    bk = Guard((E,), BF16, fill=torch.zeros(E))
    lse, w = Guard((1, Bs, H), F32), Guard((1, Bs, 2051), F32)

    def valu(S=8, q_sb=E, bias=True, zero=1, weights=False):
        args = (1, _ptrs([q.t]), _longs([q_sb]), _ptrs([k.t]), _longs([Bs * E]), _longs([E]), None, _ptrs([k.t]), _longs([Bs * E]),
                _longs([E]), None, None, _ptrs([bk.t]) if bias else None, _ptrs([bk.t]) if bias else None, zero, _ints([S]),
                _ptrs([out.t]), _longs([E]), Bs, H, 1)
        if weights:
            return declined('tell_attn_decode_weights', *args, lse.t, _ptrs([w.t]), _longs([Bs * 2051]), _longs([2051]), 0, 1, None)
        return declined('tell_attn_decode', *args)
    for weights in (False, True):
        assert valu(S=2049, weights=weights) != 0
        assert valu(S=0, bias=False, zero=0, weights=weights) != 0
        assert valu(q_sb=E + 4, weights=weights) != 0
    kc, mk = Guard((Bs, H, 64 * 64), BF16, fill=torch.zeros(Bs, H, 64 * 64)), Guard((Bs, 64), U8, fill=torch.ones(Bs, 64))

    def packed(Sp=64, q_sb=E):
        return declined('tell_attn_decode_packed', 1, _ptrs([q.t]), _longs([q_sb]), _ptrs([kc.t]), _ptrs([kc.t]), _ptrs([mk.t]),
                        _ints([Sp]), _ptrs([out.t]), _longs([E]), Bs, H, 1)
    assert packed(Sp=48) != 0 and packed(Sp=0) != 0 and packed(q_sb=E + 4) != 0
    torch.cuda.synchronize()
    assert out.untouched() and lse.untouched() and w.untouched()
