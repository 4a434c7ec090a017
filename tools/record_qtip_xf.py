"""Records the SHA-256 of the output bytes of every call of tests/qtip_xf_cases.py, as the reference of
tests/test_qtip_xf_golden_gpu.py: a change that must not move a bit of the QTIP transform-in / transform-out arithmetic is checked
against the record of the commit BEFORE it.  Needs the GPU, on a checkout of that commit with this file and tests/qtip_xf_cases.py
added:

    python tools/record_qtip_xf.py <commit> > tests/golden/qtip_xf_bits.json

The file: {"parent": commit, "cases": {name: {output name: digest}}}.  Nothing is written unless every case ran, every output is
finite and the cases that take the second arm of a kernel (qtip_xf_cases.SAME_AS) repeat the digests of the first.
"""
import json
import os
import sys


def main(parent):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import qtip_xf_cases
    cases = {}
    for name in qtip_xf_cases.CASES:
        cases[name] = qtip_xf_cases.run(name)
        print(f"{name}: {len(cases[name])} outputs", file=sys.stderr)
    for name, first in qtip_xf_cases.SAME_AS.items():
        assert cases[name] == cases[first], f"{name} differs from {first}"
    doc = json.dumps({"parent": parent, "cases": cases}, separators=(",", ":"))
    print(doc.replace('},"', '},\n"').replace('"cases":{', '"cases":{\n'))


if __name__ == "__main__":
    main(sys.argv[1])
