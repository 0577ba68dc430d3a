"""Device buffers of the kernel-level tests (tests/test_gpu_se_gate.py, test_gpu_frm_kernels.py,
test_gpu_ffm_ctx.py, test_gpu_ifrm_kernels.py): every buffer sits between guards of a NaN bit pattern, and
a buffer that is not given a fill holds the same pattern throughout.  A stray write shows in the guard, a
stray read or an element the kernel left unwritten shows as NaN in the arithmetic."""
import torch

import rectify_cases as rc

GUARD = 64
NAN32 = 0x7FC0DEAD
NAN16 = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


class Guarded:
    """A device buffer of ``shape`` with GUARD elements of a NaN bit pattern on both sides."""

    def __init__(self, shape, dtype, dev, fill=None):
        n = 1
        for d in shape:
            n *= d
        self.n = n
        self.idt, self.pattern = (torch.int32, NAN32) if dtype != torch.bfloat16 and dtype != torch.float16 \
            else (torch.int16, NAN16[dtype])
        self.raw = torch.full((n + 2 * GUARD,), self.pattern, dtype=self.idt, device=dev)
        self.t = self.raw.view(dtype)[GUARD:GUARD + n].view(*shape)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        r = self.raw.cpu()
        return bool((r[:GUARD] == self.pattern).all() and (r[GUARD + self.n:] == self.pattern).all())

    def untouched(self):
        """an unfilled buffer still holds the pattern in every element (a refused call wrote nothing)"""
        return bool((self.raw == self.pattern).all())

    def refill(self):
        """the NaN pattern again in every element of the body (before a second launch)"""
        self.raw[GUARD:GUARD + self.n] = self.pattern


def all_intact(bufs):
    return all(b.intact() for b in bufs if b is not None)


def put(t64, dtype, dev):
    return Guarded(tuple(t64.shape), dtype, dev, t64.to(dtype))


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def twice(launch, outs, prefill=None):
    """launch, read the outputs, put them back to the NaN pattern (or their pre-fill), launch again: equal bits"""
    launch()
    torch.cuda.synchronize()
    first = [o.t.cpu().clone() for o in outs]
    for o in outs:
        o.refill()
    if prefill:
        prefill()
    launch()
    torch.cuda.synchronize()
    for o, f in zip(outs, first):
        assert bits_equal(o.t.cpu(), f), "two launches differ"
    return first


class Check:
    def __init__(self, test, case):
        self.test, self.case, self.bad = test, case, []

    def within(self, name, got, ref, e_emul, u, rowwise):
        assert not torch.isnan(got).any(), (name, "NaN left")
        err = rc.rowerr(got, ref) if rowwise else rc.tenerr(got, ref)
        bnd = rc.bound(e_emul, u)
        rc.report(self.test, self.case, name, err, bnd)
        if not err <= bnd:
            self.bad.append((name, err, bnd))

    def exact(self, name, got, want):
        same = torch.equal(got.cpu().double(), want.double())
        rc.report(self.test, self.case, name, exact=same)
        if not same:
            self.bad.append((name, "not exact"))

    def done(self):
        assert not self.bad, (self.case, self.bad)
