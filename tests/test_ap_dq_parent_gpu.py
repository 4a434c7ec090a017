"""GPU: the decode-to-fp16 matrix-core GEMV (csrc/ap_dq.hip::ap_gemv_dq_kernel) returns, word for word, the fp16 outputs
tests/golden/ap_dq_outputs.json records (tools/record_ap_dq_outputs.py wrote them with the library of the commit the file names --
the reference is that commit, never the library under test).  tests/test_ap_dq_gpu.py checks the kernel against an envelope; this pins
its bits: the fp32 sums of its RMSNorm statistic and of its K-split are ordered, and a refactor must not reorder them.  Cases
(tests/ap_dq_cases.py): bits 2 to 4; the smallest shape served, a ragged second row group, the two compiled-in widths, more staging
items than staging threads, the widest row; plain, residual, RMSNorm, RMSNorm + gate/up pairs and the SiLU * up prologue; guarded
buffers, the route asserted."""
import json
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ap_dq_cases  # noqa: E402
from conftest import GOLDEN  # noqa: E402

DOC = json.load(open(os.path.join(GOLDEN, "ap_dq_outputs.json")))


def test_the_record_covers_the_cases():
    assert len(DOC["parent"]) == 40 and sorted(DOC["cases"]) == sorted(ap_dq_cases.CASES) and len(ap_dq_cases.CASES) == 90
    for name, words in DOC["cases"].items():
        N = int(name.split("_")[1].split("x")[0])
        assert len(words) == 4 * (N // 2 if name.endswith("rmsnorm_pairs") else N), name


@pytest.mark.parametrize("bits", ap_dq_cases.BITS)
def test_outputs_are_the_parents(bits):
    bad = {}
    with ap_dq_cases.dq_everywhere():
        for name in ap_dq_cases.CASES:
            if name.startswith(f"b{bits}_"):
                got = ap_dq_cases.run(name)
                if got != DOC["cases"][name]:
                    bad[name] = (DOC["cases"][name], got)
    assert not bad, f"{len(bad)} cases differ from the parent's words (want, got): {dict(list(bad.items())[:3])}"
