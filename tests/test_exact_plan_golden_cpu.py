"""CPU (host logic): the exact-order planner (gq_debug_exact_plan_ex: block size, row slots, steps per block, ring depth, grid, the
blocks per CU the instance's occupancy holds, and the kernel) plans every launch of tests/golden/exact_plans.json as the commit that
file names did (tools/record_exact_plans.py wrote it with that commit's library): the Llama shapes and the edges of the K range, bits 2
to 4, the three prologues, with and without the SiLU-pairs epilogue, and the knobs that move a plan -- GQ_AP_INREG=0 among them, where
the blocks per CU are still capped with the INREG instance's occupancy (a known quirk, pinned as it is).  The reference is that commit,
never the library under test.  No device is touched (256 CUs are assumed without one)."""
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT
from guidedquant_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_exact_plans as rec  # noqa: E402

DOC = json.load(open(os.path.join(GOLDEN, "exact_plans.json")))


def test_the_record_covers_the_grid():
    assert len(DOC["parent"]) == 40 and DOC["bits"] == rec.BITS and DOC["knobs"] == rec.KNOBS
    assert [tuple(r[:5]) for r in DOC["rows"]] == rec.grid()
    plans = [p for r in DOC["rows"] for p in r[5] if isinstance(p, list)]
    assert len(plans) > 1000 and all(len(p) == 7 for p in plans) and {p[6] for p in plans} == {0, 1, 2}


@pytest.mark.parametrize("ks", range(len(rec.KNOBS)), ids=lambda i: "-".join(f"{k}={v}" for k, v in rec.KNOBS[i].items()) or "default")
def test_plans_are_the_parents(ks):
    L = _lib.lib()
    saved = {k: os.environ.get(k) for k in rec.KNOB_NAMES}
    rows = [r for r in DOC["rows"] if r[0] == ks]
    try:
        got = rec.record(L, [tuple(r[:5]) for r in rows])
    finally:
        rec.set_knobs(L, {k: v for k, v in saved.items() if v is not None})
    assert len(rows) > 0
    bad = [(w[:5], w[5], g[5]) for w, g in zip(rows, got) if w != g]
    assert not bad, f"{len(bad)} of {len(rows)} launches plan differently: {bad[:5]}"
