"""Guard-banded, poisoned buffers for kernel tests (a plain helper module; DESIGN.md, "Kernel tests allocate through guarded.py").

Every buffer a test hands to a kernel is ONE torch.uint8 allocation laid out as

    [ front guard (G bytes) | payload (nbytes) | back guard (>= G bytes) ]

G is a multiple of 512 and at least 4096, so the payload keeps the alignment of the allocation itself (the dispatcher's
aligned routes ask for 16 B; a page is kept).  The back guard begins at the FIRST byte after the payload: the payload
is flush against it, whatever its size.  The whole allocation is filled with the byte POISON = 0x7E before the payload
is copied in.  What that pattern means to a kernel that reads it:
  * as fp16 it is 0x7E7E, a NaN;
  * as fp32 it is 0x7E7E7E7E, about 8.4e37 (two of them multiplied overflow to inf; a sum with it swamps any result);
  * as a word of a bit plane (or an index) it yields arbitrary codes (0x7E7E7E7E as a row / token index is ~2.1e9).

What is detected:
  * a WRITE outside the payload: check() compares both guards with the pattern, exactly, and names the buffer, the
    side, the first and last changed byte offsets relative to the payload (negative in front, >= nbytes behind) and
    the count;
  * a READ outside an input's payload whose value is USED: the result turns into NaN or a gross mismatch with the
    oracle, which the family's own checker reports;
  * an output element that is never written, and a workspace the kernel expects to be zeroed: outputs and workspaces
    are left filled with the pattern (Guarded.empty), so an unwritten fp16 element stays NaN and an unwritten fp32
    partial is 8.4e37.
What is NOT detected: a read outside the payload whose value is discarded (masked away, multiplied by an exact zero
and so on).  That is out of scope here: the guards are the only detector, and they cannot see loads.

No payload is ever placed against the end of a mapping or next to memory the test does not own: every byte within G
of the payload, on both sides, belongs to the same allocation, so an access the guards can catch cannot fault.
"""
import numpy as np
import torch

POISON = 0x7E
GUARD = 4096  # bytes; a multiple of 512, at least 4096


class GuardViolation(AssertionError):
    pass


class Guarded:
    """One guard-banded buffer.  Guarded(payload) copies a numpy array or a torch tensor in (an input);
    Guarded.empty(nbytes) leaves the payload poisoned (an output or a workspace)."""

    def __init__(self, payload=None, nbytes=None, device="cuda:0", guard=GUARD, name=None):
        assert guard % 512 == 0 and guard >= 4096, "the front guard keeps the payload's alignment: a multiple of 512, >= 4096"
        if payload is not None:
            if isinstance(payload, np.ndarray):
                payload = torch.from_numpy(np.ascontiguousarray(payload))
            payload = payload.contiguous()
            raw = payload.reshape(-1).view(torch.uint8) if payload.numel() else torch.empty(0, dtype=torch.uint8)
            nbytes = raw.numel()
        self.name, self.G, self.nbytes = name, int(guard), int(nbytes)
        self.buf = torch.full((2 * self.G + self.nbytes, ), POISON, dtype=torch.uint8, device=device)
        if payload is not None and self.nbytes:
            self.buf[self.G:self.G + self.nbytes] = raw.to(device)

    @classmethod
    def empty(cls, nbytes, device="cuda:0", guard=GUARD, name=None):
        return cls(nbytes=nbytes, device=device, guard=guard, name=name)

    def ptr(self):
        return self.buf.data_ptr() + self.G

    def view(self, dtype, shape=None):
        """the payload as a tensor of `dtype` (a view of the allocation, not a copy)"""
        t = self.buf[self.G:self.G + self.nbytes].view(dtype)
        return t if shape is None else t.view(shape)

    def numpy(self, dtype, shape=None):
        a = self.buf[self.G:self.G + self.nbytes].cpu().numpy().view(dtype)
        return a if shape is None else a.reshape(shape)

    def check(self, name=None):
        """both guards still hold the pattern, byte for byte"""
        name = name or self.name or "buffer"
        front = self.buf[:self.G]
        back = self.buf[self.G + self.nbytes:]
        for side, g, base in (("front", front, -self.G), ("back", back, self.nbytes)):
            bad = g != POISON
            if bool(bad.any()):
                idx = torch.nonzero(bad).reshape(-1)
                raise GuardViolation(f"{name}: {side} guard overwritten: {int(idx.numel())} byte(s), payload offsets "
                                     f"[{int(idx[0]) + base}, {int(idx[-1]) + base}] (payload is {self.nbytes} bytes)")


class Guards:
    """the buffers of one launch, by name: g = Guards(); p = g.inp("x", x); o = g.out("out", N * 2); ...; g.check()"""

    def __init__(self, device="cuda:0"):
        self.device, self.bufs = device, {}

    def inp(self, name, payload):
        """an input (None stays None, for optional pointers)"""
        if payload is None:
            return None
        b = self.bufs[name] = Guarded(payload, device=self.device, name=name)
        return b

    def out(self, name, nbytes):
        b = self.bufs[name] = Guarded.empty(int(nbytes), device=self.device, name=name)
        return b

    def __getitem__(self, name):
        return self.bufs[name]

    def check(self):
        if self.device != "cpu":
            torch.cuda.synchronize()
        for name, b in self.bufs.items():
            b.check(name)


def ptr(b):
    """data pointer of an optional Guarded (None for a null pointer)"""
    return None if b is None else b.ptr()
