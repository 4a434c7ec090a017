"""GPU: the C-ABI calls of one eager decode step -- entry points, scalars, the role of every pointer, descriptor arrays field by field
(tests/decode_calls.py) -- against tests/golden/decode_calls.json, recorded by tools/record_decode_calls.py on the commit before the
step moved out of model.py.  Equality, every configuration: which entry point is called with which arguments in which order is pinned
for both families and every knob of guidedquant_amd/native_step.py."""
import json
import os

import pytest

import decode_calls

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(__file__), "golden", "decode_calls.json")) as f:
        return json.load(f)["configs"]


def test_golden_has_every_configuration_and_branch(golden):
    assert sorted(golden) == sorted(decode_calls.CONFIGS)
    assert decode_calls.missing_coverage(golden) == []


@pytest.mark.parametrize("name", list(decode_calls.CONFIGS))
def test_decode_step_makes_the_recorded_calls(golden, name):
    got = json.loads(json.dumps(decode_calls.record(name)))
    want = golden[name]
    assert [c[0] for c in got] == [c[0] for c in want]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
