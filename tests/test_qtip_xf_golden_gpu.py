"""GPU: the output BITS of every entry point of the QTIP transform side (tests/qtip_xf_cases.py: the cases, their shapes and inputs)
against tests/golden/qtip_xf_bits.json, recorded by tools/record_qtip_xf.py on the commit before the element-wise arithmetic moved
into csrc/qtip_xform.h.  The tests of test_qtip_gpu.py compare one form of that arithmetic with another and would not notice both
moving together; these compare SHA-256 digests of the outputs with the record.  Every case of the record is replayed."""
import json
import os

import pytest

import qtip_xf_cases

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(__file__), "golden", "qtip_xf_bits.json")) as f:
        return json.load(f)["cases"]


def test_golden_has_every_case_and_the_arms_agree(golden):
    assert sorted(golden) == sorted(qtip_xf_cases.CASES)
    for name, first in qtip_xf_cases.SAME_AS.items():
        assert golden[name] == golden[first], (name, first)


@pytest.mark.parametrize("name", list(qtip_xf_cases.CASES))
def test_call_gives_the_recorded_bits(golden, name):
    assert qtip_xf_cases.run(name) == golden[name]
