"""Records the fp16 output words of every case of tests/ap_dq_cases.py, as the reference of tests/test_ap_dq_parent_gpu.py: a change
that must not move a bit of the decode-to-fp16 matrix-core GEMV (csrc/ap_dq.hip) is checked against the record of the commit BEFORE
it.  Needs the GPU and that commit's library:

    git worktree add /tmp/parent <commit> && make -C /tmp/parent/guidedquant_amd/csrc
    GQ_LIB_PATH=/tmp/parent/guidedquant_amd/libgq_hip.so python tools/record_ap_dq_outputs.py <commit> > tests/golden/ap_dq_outputs.json

The file: {"parent": commit, "cases": {name: hex}} -- the outputs themselves, four hex digits per fp16 word in row order, so that a
mismatch can be read.  Nothing is written unless every case ran on the dq route with finite outputs.
"""
import json
import os
import sys


def main(parent):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import ap_dq_cases
    cases = {}
    with ap_dq_cases.dq_everywhere():
        for name in ap_dq_cases.CASES:
            cases[name] = ap_dq_cases.run(name)
            print(f"{name}: {len(cases[name]) // 4} words", file=sys.stderr)
    doc = json.dumps({"parent": parent, "cases": cases}, separators=(",", ":"))
    print(doc.replace('","', '",\n"').replace('"cases":{', '"cases":{\n'))


if __name__ == "__main__":
    main(sys.argv[1])
