"""GPU: tests/guarded.py detects damage on a device buffer as it does on the CPU (tests/test_guarded_cpu.py): a guard byte dirtied
with a torch indexing store makes check() raise and name the offset; an element one past an input's payload reads as NaN."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from guarded import GUARD, Guarded, GuardViolation, Guards  # noqa: E402


def test_device_guards_detect_a_dirty_byte_on_either_side():
    b = Guarded(np.arange(10, dtype=np.float16), name="x")
    assert b.buf.is_cuda and b.ptr() == b.buf.data_ptr() + GUARD and b.ptr() % 512 == 0
    assert b.view(torch.float16).cpu().tolist() == list(range(10))
    b.check()
    for off, rel, side in ((GUARD + b.nbytes, 20, "back"), (GUARD - 1, -1, "front"), (0, -GUARD, "front"), (b.buf.numel() - 1, 20 + GUARD - 1, "back")):
        old = int(b.buf[off])
        b.buf[off] = 0
        with pytest.raises(GuardViolation, match=rf"x: {side} guard overwritten: 1 byte\(s\), payload offsets \[{rel}, {rel}\]"):
            b.check()
        b.buf[off] = old
        b.check()
    over = torch.as_strided(b.view(torch.float16), (11, ), (1, ))   # (inside the allocation)
    assert bool(torch.isnan(over[10])) and not bool(torch.isnan(over[:10]).any())


def test_device_outputs_start_poisoned_and_the_collection_names_the_buffer():
    g = Guards()
    o = g.out("out", 8)
    w = g.out("workspace", 16)
    assert bool(torch.isnan(o.view(torch.float16)).all()) and float(w.view(torch.float32).min()) > 8e37
    o.view(torch.float16)[:] = 1.0   # a kernel writing its payload
    g.check()
    w.buf[GUARD + 16:GUARD + 20] = 0   # one float behind the workspace
    with pytest.raises(GuardViolation, match=r"^workspace: back guard overwritten: 4 byte\(s\), payload offsets \[16, 19\]"):
        g.check()
