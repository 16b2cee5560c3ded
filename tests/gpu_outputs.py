"""Shared plumbing of the operator-level GPU tests (tests/test_small_ops_gpu.py, tests/test_sn_gpu.py): sentinel-guarded output slices, a
C-ABI call that checks them, and the error report against an fp64 reference with its fp32-CPU yardstick."""
import torch

import small_ops_reference as R

DEV = "cuda:0"
FWD_TOL, BWD_TOL = 2e-5, 1e-4
GUARD_BYTES = 256 * 4
BF16 = torch.bfloat16


def _H():
    import _hip
    return _hip


class Out:
    """An output slice between two sentinel guards."""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        n = 1
        for s in shape:
            n *= int(s)
        g = GUARD_BYTES // torch.empty(0, dtype=dtype).element_size()
        self.g, self.n, self.bits = g, n, {4: torch.int32, 2: torch.int16}[torch.empty(0, dtype=dtype).element_size()]
        sent = (torch.arange(2 * g, dtype=torch.float32) * 0.5 + 1000.25).to(dtype)
        self.buf = torch.empty(g + n + g, dtype=dtype, device=DEV)
        self.buf[:g] = sent[:g].to(DEV)
        self.buf[g + n:] = sent[g:].to(DEV)
        self.sent = sent.view(self.bits)
        self.t = self.buf[g:g + n].view(*shape)
        if fill is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(torch.as_tensor(fill, dtype=dtype).to(DEV).expand(*shape))

    def ptr(self):
        return self.t.data_ptr()

    def check(self, tag, exempt=None):
        """``exempt``: bool mask (flat, ``n`` elements) of positions the contract leaves unwritten -- they may still hold NaN."""
        b = self.buf.cpu()
        assert torch.equal(b[:self.g].view(self.bits), self.sent[:self.g]), f"{tag}: store below the output"
        assert torch.equal(b[self.g + self.n:].view(self.bits), self.sent[self.g:]), f"{tag}: store above the output"
        nan = torch.isnan(b[self.g:self.g + self.n].float())
        if exempt is not None:
            nan &= ~exempt.reshape(-1)
        assert not nan.any(), f"{tag}: {int(nan.sum())} of {self.n} elements unwritten (NaN), first at {int(nan.nonzero()[0])}"
        return self.t.cpu()


def _call(name, outs, *args):
    """One entry point; afterwards the hygiene checks of every output.  -> the outputs on the CPU."""
    H = _H()
    H.call(name, *[a.ptr() if isinstance(a, Out) else (a.data_ptr() if isinstance(a, torch.Tensor) else a) for a in args], H.stream())
    torch.cuda.synchronize()
    return [o.check(f"{name}[{k}]") for k, o in enumerate(outs)]


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _d(t):
    return None if t is None else t.double()


def _check(entry, output, case, got, ref64, ref32, tol, floor=0.0):
    """Prints the kernel's error and the fp32-CPU yardstick, then asserts the bound."""
    e, y = R.rel_err(got, ref64, floor), R.rel_err(ref32, ref64, floor)
    print(f"ERR {entry} {output} {case}: kernel {e:.3e} fp32-cpu {y:.3e} bound {tol:.0e}")
    assert e <= tol, f"{entry} {output} {case}: {e:.3e} > {tol:.0e} (fp32 on the CPU: {y:.3e})"
