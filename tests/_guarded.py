"""Poisoned device buffers with guard bands, and normalised rows with hostile neighbours, for the tests that hand the
library its workspace, its outputs and its inputs as device pointers.

A k-NN call carves all its scratch out of one caller-supplied arena and lays it out anew per call, so every region
starts with what an earlier call of another shape left there.  torch.empty gives a test memory that usually holds
benign finite data; guarded() gives it CHOSEN contents (FILLS) and a position-dependent canary in front of the payload,
behind it and in the payload's round-up tail, so that a write outside the bytes the call was promised shows as a
changed canary byte -- never as a fault.  poisoned_rows() puts NaN rows that count as real targets (zero flag 0) in
front of and behind a normalised set inside ONE allocation: a last partial tile that reads past its rows reads them."""
import numpy as np

GUARD = 4096
# mildest first; "prev" = whatever an earlier call left in the payload (Guarded.shrink re-lays the canary behind it)
FILLS = ("zeros", "word1", "ones", "prev")


def _roundup(x, m):
    return (x + m - 1) // m * m


def _canary(lo, hi):
    """bytes [lo, hi) of the canary sequence (a function of the position in the allocation, no constant run)"""
    i = np.arange(lo, hi, dtype=np.int64)
    return ((i * 167 + (i >> 8) * 59 + 0x5A) & 0xFF).astype(np.uint8)


class Guarded:
    def __init__(self, nbytes, fill, dev, guard=GUARD):
        import torch
        assert nbytes >= 0 and guard % 4096 == 0 and guard > 0
        self.guard, self.dev = guard, torch.device(dev)
        self.room = _roundup(max(nbytes, 1), 256)
        self.t = torch.empty(guard + self.room + guard, dtype=torch.uint8, device=dev)
        assert self.dev.type != "cuda" or self.t.data_ptr() % 256 == 0  # (the arena's regions are 256-byte aligned)
        self.ptr = self.t.data_ptr() + guard
        self.nbytes = nbytes
        self._lay(0, guard)
        self._lay(guard + nbytes, self.t.numel())
        self.fill(fill)

    def _lay(self, lo, hi):
        import torch
        if hi > lo:
            self.t[lo:hi] = torch.from_numpy(_canary(lo, hi)).to(self.dev)

    def _sync(self):
        import torch
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    def fill(self, fill):
        """the payload's bytes: FILLS ("prev": left as they are)"""
        import torch
        p = self.t[self.guard:self.guard + self.nbytes]
        if fill == "zeros":
            p.zero_()
        elif fill == "ones":
            p.fill_(0xFF)
        elif fill == "word1":  # every 32-bit word 0x00000001, little endian (the payload starts on a word)
            whole = self.nbytes // 4 * 4
            p[:whole].view(torch.int32).fill_(1)
            p[whole:] = 0
            p[whole:whole + 1] = 1
        else:
            assert fill == "prev", fill
        self._sync()
        return self

    def shrink(self, nbytes):
        """The payload becomes its first `nbytes` bytes, contents kept; the canary is re-laid from there on."""
        assert 0 <= nbytes <= self.nbytes
        self.nbytes = nbytes
        self._lay(self.guard + nbytes, self.t.numel())
        return self

    def payload(self):
        """host copy of the payload's bytes"""
        return self.t[self.guard:self.guard + self.nbytes].cpu().numpy()

    def view(self, dtype, shape):
        """the payload's first bytes as a device tensor of `dtype` and `shape`"""
        import torch
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        assert n <= self.nbytes
        return self.t[self.guard:self.guard + n].view(dtype).view(*shape)

    def check(self, what):
        """every canary byte unchanged; else the first changed offset, counted from the payload's start"""
        self._sync()
        end = self.guard + self.nbytes
        for lo, hi in ((0, self.guard), (end, self.t.numel())):
            got = self.t[lo:hi].cpu().numpy()
            bad = np.flatnonzero(got != _canary(lo, hi))
            assert bad.size == 0, "%s: %d byte(s) written outside its %d bytes, the first at offset %d" % (
                what, bad.size, self.nbytes, lo + int(bad[0]) - self.guard)


def guarded(nbytes, fill, dev, guard=GUARD):
    """guard + roundup(nbytes, 256) + guard bytes in one uint8 tensor: canary | payload filled with `fill` | canary from
    the payload's end on (the round-up tail and the second guard).  .ptr: the payload's start, .nbytes: its length."""
    return Guarded(int(nbytes), fill, dev, guard)


def poisoned_rows(Ehat, zero, before, after):
    """Views of the real rows of (Ehat, zero) after copying them into the middle of larger allocations whose `before`
    rows in front and `after` rows behind hold NaN, with zero flag 0: a row that gets read counts as a real target."""
    import torch
    n, dp = Ehat.shape
    big = torch.full((before + n + after, dp), float("nan"), dtype=torch.float32, device=Ehat.device)
    flags = torch.zeros((before + n + after,), dtype=torch.uint8, device=Ehat.device)
    big[before:before + n] = Ehat
    flags[before:before + n] = zero
    return big[before:before + n], flags[before:before + n]


def knn_dev_guarded(ctx, Ehat, zero, q0, nq, t_base, d, k, fill="ones", stream=0):
    """fdr_knn_dev of rows [q0, q0 + nq) of Ehat against all of them, workspace (exactly fdr_knn_workspace_bytes, filled
    with `fill`) and outputs (0xFF bytes) from guarded(); synchronises and checks the three canaries.  Returns the
    device tensors (idx int32 [nq, k], dist float32 [nq, k]) and the workspace (the call's path codes live in it)."""
    import torch
    dev, n = Ehat.device, Ehat.shape[0]
    ws = guarded(ctx.knn_workspace_bytes(nq, n, d, k), fill, dev)
    gi, gd = guarded(nq * k * 4, "ones", dev), guarded(nq * k * 4, "ones", dev)
    ctx.knn_dev(Ehat[q0].data_ptr(), zero[q0:].data_ptr(), nq, Ehat.data_ptr(), zero.data_ptr(), n, t_base, d, k,
                gi.ptr, gd.ptr, ws.ptr, ws.nbytes, stream)
    torch.cuda.synchronize(dev)
    ws.check("workspace")
    gi.check("indices")
    gd.check("distances")
    idx, dst = gi.view(torch.int32, (nq, k)), gd.view(torch.float32, (nq, k))
    return idx, dst, ws
