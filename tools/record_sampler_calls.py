"""Records what every decode route asks of the fused sampler's C ABI, per configuration of tests/sampler_calls.py, as the reference of
tests/test_sampler_calls_golden_gpu.py: a change that must not move the sampler's calls is checked against the record of the commit
BEFORE it.  Needs the GPU (the routes run for real), on a checkout of that commit with this file and tests/sampler_calls.py added:

    python tools/record_sampler_calls.py <commit> > tests/golden/sampler_calls.json

The file: {"parent": commit, "configs": {name: [[entry point, [argument, ..]], ..]}}.  Nothing is written unless every configuration's
log holds exactly the entry points sampler_calls.COVERAGE lists for it.
"""
import json
import os
import sys


def main(parent):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import sampler_calls
    logs = {}
    for name in sampler_calls.CONFIGS:
        logs[name] = sampler_calls.record(name)
        print(f"{name}: {len(logs[name])} calls", file=sys.stderr)
    missing = sampler_calls.missing_coverage(logs)
    assert not missing, "configurations whose record does not show their entry points: " + "; ".join(missing)
    doc = json.dumps({"parent": parent, "configs": logs}, separators=(",", ":"))
    print(doc.replace('],["gq_', '],\n["gq_').replace('"configs":{', '"configs":{\n').replace(']]],"', ']]],\n"'))


if __name__ == "__main__":
    main(sys.argv[1])
