"""Records what one eager decode step asks of the C ABI, per configuration of tests/decode_calls.py, as the reference of
tests/test_decode_calls_golden_gpu.py: a change that must not move the step's launches is checked against the record of the commit
BEFORE it.  Needs the GPU (the step runs for real), on a checkout of that commit with this file and tests/decode_calls.py added:

    python tools/record_decode_calls.py <commit> > tests/golden/decode_calls.json

The file: {"parent": commit, "configs": {name: [[entry point, [argument, ..]], ..]}}.  Nothing is written unless every branch listed
in decode_calls.COVERAGE shows in the log of the configuration that is there for it.
"""
import json
import os
import sys


def main(parent):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import decode_calls
    logs = {}
    for name in decode_calls.CONFIGS:
        logs[name] = decode_calls.record(name)
        print(f"{name}: {len(logs[name])} calls", file=sys.stderr)
    missing = decode_calls.missing_coverage(logs)
    assert not missing, "branches the record does not show: " + "; ".join(missing)
    doc = json.dumps({"parent": parent, "configs": logs}, separators=(",", ":"))
    print(doc.replace('],["gq_', '],\n["gq_').replace('"configs":{', '"configs":{\n').replace(']]],"', ']]],\n"'))


if __name__ == "__main__":
    main(sys.argv[1])
