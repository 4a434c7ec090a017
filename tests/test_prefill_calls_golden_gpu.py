"""GPU: the C-ABI calls of one eager prompt pass -- entry points, scalars, the role of every pointer, in order, and what the pass
reported (tests/prefill_calls.py) -- against tests/golden/prefill_calls.json, recorded by tools/record_prefill_calls.py on the commit
before the pass moved out of model.py into guidedquant_amd/native_prompt.py.  Equality, every configuration: which entry point is called
with which arguments in which order is pinned for every cache layout, block layout, attention choice and head of the pass."""
import json
import os

import pytest

import prefill_calls

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(__file__), "golden", "prefill_calls.json")) as f:
        return json.load(f)["configs"]


def test_golden_has_every_configuration_and_branch(golden):
    assert sorted(golden) == sorted(prefill_calls.CONFIGS)
    assert prefill_calls.missing_coverage(golden) == []


@pytest.mark.parametrize("name", list(prefill_calls.CONFIGS))
def test_prompt_pass_makes_the_recorded_calls(golden, name):
    got = json.loads(json.dumps(prefill_calls.record(name)))
    want = golden[name]
    assert [c[0] for c in got] == [c[0] for c in want]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
