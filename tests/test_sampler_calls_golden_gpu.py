"""GPU: the calls every decode route makes to the fused sampler's C ABI -- entry points, scalars, the role of every pointer
(tests/sampler_calls.py) -- against tests/golden/sampler_calls.json, recorded by tools/record_sampler_calls.py on the commit before the
routes' sampler state and C calls moved into guidedquant_amd/fused_sampler.py.  Equality, every configuration: DecodeGraph in eight
sampler configurations, routes 1 and 2 of AnyPrecisionForCausalLM.generate plain and with penalty + suppress list, the layer pipeline."""
import json
import os

import pytest

import sampler_calls

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(__file__), "golden", "sampler_calls.json")) as f:
        return json.load(f)["configs"]


def test_golden_has_every_configuration_and_entry_point(golden):
    assert sorted(golden) == sorted(sampler_calls.CONFIGS)
    assert sampler_calls.missing_coverage(golden) == []


@pytest.mark.parametrize("name", list(sampler_calls.CONFIGS))
def test_route_makes_the_recorded_sampler_calls(golden, name):
    if name.startswith("route"):
        pytest.importorskip("transformers")
    got = json.loads(json.dumps(sampler_calls.record(name)))
    want = golden[name]
    assert [c[0] for c in got] == [c[0] for c in want]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
