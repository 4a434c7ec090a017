"""Records what one eager prompt pass asks of the C ABI, per configuration of tests/prefill_calls.py, as the reference of
tests/test_prefill_calls_golden_gpu.py: a change that must not move the pass's launches is checked against the record of the commit
BEFORE it.  Needs the GPU (the pass runs for real), on a checkout of that commit with this file, tests/prefill_calls.py and the golden
test added (they use the public surface of the model only):

    python tools/record_prefill_calls.py <commit> > tests/golden/prefill_calls.json

The file: {"parent": commit, "configs": {name: [[entry point, [argument, ..]], .., ["result", [..]]]}}.  Nothing is written unless every
branch listed in prefill_calls.COVERAGE shows in the log of the configuration that is there for it.
"""
import json
import os
import sys


def main(parent):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import prefill_calls
    logs = {}
    for name in prefill_calls.CONFIGS:
        logs[name] = json.loads(json.dumps(prefill_calls.record(name)))
        print(f"{name}: {len(logs[name])} calls", file=sys.stderr)
    missing = prefill_calls.missing_coverage(logs)
    assert not missing, "branches the record does not show: " + "; ".join(missing)
    doc = json.dumps({"parent": parent, "configs": logs}, separators=(",", ":"))
    print(doc.replace('],["', '],\n["').replace('"configs":{', '"configs":{\n').replace(']]],"', ']]],\n"'))


if __name__ == "__main__":
    main(sys.argv[1])
