"""CPU (host logic): the dry AP-GEMV dispatch plans every launch of tests/golden/ap_routes.json as the commit that file names did
(tools/record_ap_routes.py wrote it with that commit's library): family, launches, variant, return code and, for the w2 form, the
workspace gq_anyprec_gemv_fused_ws_bytes asks for -- bits 2 to 8 (and 9, refused), both modes, the Llama shapes and the edges of the K range, every
launch form and the refused ones, and the knobs that move a launch.  The reference is that commit, never the library under test.  The
dry dispatch hands the kernels an aligned stand-in pointer, so the fall-backs for unaligned buffers are not covered here.  No device is
touched (256 CUs are assumed without one)."""
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT
from guidedquant_amd import _lib

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_ap_routes as rec  # noqa: E402

DOC = json.load(open(os.path.join(GOLDEN, "ap_routes.json")))


def test_the_record_covers_the_grid():
    assert len(DOC["parent"]) == 40 and DOC["bits"] == rec.BITS and DOC["knobs"] == rec.KNOBS
    assert [tuple(r[:8]) for r in DOC["rows"]] == rec.grid()


@pytest.mark.parametrize("ks", range(len(rec.KNOBS)), ids=lambda i: "-".join(f"{k}={v}" for k, v in rec.KNOBS[i].items()) or "default")
def test_routes_are_the_parents(ks):
    L = _lib.lib()
    saved = {k: os.environ.get(k) for k in rec.KNOB_NAMES}
    rows = [r for r in DOC["rows"] if r[0] == ks]
    try:
        got = rec.record(L, [tuple(r[:8]) for r in rows])
    finally:
        rec.set_knobs(L, {k: v for k, v in saved.items() if v is not None})
        L.gq_set_ap_mode(-1)
    assert len(rows) > 0
    bad = [(w[:8], w[8], g[8]) for w, g in zip(rows, got) if w != g]
    assert not bad, f"{len(bad)} of {len(rows)} launches plan differently: {bad[:5]}"
