"""ORACLE (test infrastructure): device tensors inside larger NaN-filled buffers, shared by the element-wise GPU suites
(tests/test_gpu_frame_kernels.py, tests/test_gpu_mrf_kernels.py).  A kernel that reads a pad column as data returns NaN;
one that writes outside its block is caught by ``Buf.get``."""
import torch

DEV = "cuda:0"
NAN = float("nan")


class Buf:
    """A [B, C, L] block at element offset ``off`` of a flat NaN-filled device buffer: row stride ld > L, batch stride
    bs > C * ld.  ``layout``: "vec" / "out" = ld % 4 == 0 and a 16-byte base, "odd_ld" = odd row stride, "shift1" = the
    base one float past a 16-byte boundary, "dense" = rows L apart (for entry points without a row stride; L % 4 == 0),
    the offset and the batch stride as for "vec"."""

    def __init__(self, t, layout="out"):
        self.B, self.C, self.L = t.shape
        l4 = (self.L + 3) // 4 * 4
        self.ld = l4 + 1 if layout == "odd_ld" else l4 + 4
        if layout == "dense":
            assert self.L % 4 == 0
            self.ld = self.L
        self.off = 9 if layout == "shift1" else 8
        self.bs = self.C * self.ld + 16
        flat = torch.full((self.off + self.B * self.bs + 8,), NAN)
        valid = torch.zeros_like(flat, dtype=torch.bool)
        self._block(flat)[:, :, :self.L] = t
        self._block(valid)[:, :, :self.L] = True
        self.flat, self.valid = flat.to(DEV), valid
        assert self.flat.data_ptr() % 16 == 0

    def _block(self, flat):
        return flat[self.off:self.off + self.B * self.bs].view(self.B, self.bs)[:, :self.C * self.ld].view(
            self.B, self.C, self.ld)

    def tail(self):
        """The buffer from the block's first element on: what a C caller passes as ``ptr + off``."""
        return self.flat[self.off:]

    def get(self):
        """The valid block on the host, after checking that nothing outside it was written."""
        torch.cuda.synchronize()
        flat = self.flat.cpu()
        assert torch.isnan(flat[~self.valid]).all(), "written outside the valid [B, C, :L] block"
        return self._block(flat)[:, :, :self.L].clone()
