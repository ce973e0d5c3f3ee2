"""Guarded device buffers shared by the conformance tests that drive the C ABI (tests/test_gpu_gemm.py,
tests/test_gpu_copy.py): an operand or an output is a VIEW inside a larger allocation filled with a sentinel, so a store
(or a row stride) that is off shows in the guard bands or the row gaps without anything running out of range."""
import torch

DEV = 'cuda'
SENTINEL = -65536.0          # exact in fp32 and bf16, far from anything a case produces
PAD = 64                     # elements on each side of a view: keeps the view's 16-byte alignment


class View:
    """[rows, cols] with row stride ld >= cols inside an allocation filled with SENTINEL (also the columns cols..ld-1 of
    every row); off: extra elements in front (off = 1 takes a bf16 view 2 bytes off its 8-byte alignment)"""

    def __init__(self, rows, cols, ld, dtype, off=0, fill=None):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.lo = rows, cols, ld, PAD + off
        self.buf = torch.full((self.lo + rows * ld + PAD,), SENTINEL, dtype=dtype, device=DEV)
        self.t = torch.as_strided(self.buf, (rows, cols), (ld, 1), self.lo)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        gap = torch.as_strided(self.buf, (self.rows, self.ld - self.cols), (self.ld, 1), self.lo + self.cols)
        return bool((self.buf[:self.lo] == SENTINEL).all()) and bool((gap == SENTINEL).all()) and \
            bool((self.buf[self.lo + self.rows * self.ld:] == SENTINEL).all())


class Vec:
    """a guarded fp32 vector"""

    def __init__(self, fill):
        self.n = fill.numel()
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.t = self.buf[PAD:PAD + self.n]
        self.t.copy_(fill)

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.n:] == SENTINEL).all())


class Guard:
    """a tensor of any rank, dtype and (element) strides inside an allocation filled with a sentinel: everything of the
    allocation that is no element of the view - the bands in front and behind, and every gap the strides leave - must still
    hold the sentinel after a launch.  off: elements between the front band and the view (they count as a gap)."""

    def __init__(self, shape, dtype, strides=None, fill=None, off=0, sentinel=None):
        shape = tuple(int(n) for n in shape)
        if strides is None:
            strides, n = [], 1
            for d in reversed(shape):
                strides.insert(0, n)
                n *= max(d, 1)
        self.strides = tuple(int(s) for s in strides)
        if sentinel is None:
            sentinel = SENTINEL if dtype.is_floating_point or dtype in (torch.int32, torch.int64) else 90
        self.sentinel, self.lo = sentinel, PAD + off
        span = 1 + sum((n - 1) * s for n, s in zip(shape, self.strides)) if all(shape) else 0
        self.buf = torch.full((self.lo + span + PAD,), sentinel, dtype=dtype, device=DEV)
        self.t = torch.as_strided(self.buf, shape, self.strides, self.lo)
        self.own = torch.zeros(self.buf.numel(), dtype=torch.bool, device=DEV)
        torch.as_strided(self.own, shape, self.strides, self.lo).fill_(True)
        if fill is not None:
            if not torch.is_tensor(fill):
                fill = torch.as_tensor(fill)
            self.t.copy_(fill.reshape(shape).to(dtype))

    def intact(self):
        return bool((self.buf[~self.own] == self.sentinel).all())

    def untouched(self):
        """nothing at all was written (a view that was created without fill)"""
        return bool((self.buf == self.sentinel).all())
