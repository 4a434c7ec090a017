"""Records the exact-order planner's plans (gq_debug_exact_plan_ex, all seven words) over a grid of launches, as the reference of
tests/test_exact_plan_golden_cpu.py: a change that must not move a plan is checked against the record of the commit BEFORE it.

    git worktree add /tmp/parent <commit> && make -C /tmp/parent/guidedquant_amd/csrc
    GQ_LIB_PATH=/tmp/parent/guidedquant_amd/libgq_hip.so python tools/record_exact_plans.py <commit> > tests/golden/exact_plans.json

No device is touched (256 CUs are assumed without one).  The file: {"parent": commit, "bits": [2, 3, 4], "knobs": [knob set, ..],
"rows": [..]}; a row is [knob set, N, K, prologue, epilogue, results] with one result per bit width: the plan [T, RS, SPB, D, grid,
blocks per CU the occupancy holds, kernel (0 v_perm kernel, 1 its INREG instance, 2 the pair-table kernel)], or the return code where the
planner refuses the shape.  The shapes are those of tools/record_ap_routes.py.
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import record_ap_routes as routes  # noqa: E402

BITS = [2, 3, 4]
PROLOGUES = [0, 1, 2]  # none, RMSNorm, SiLU * up
EPILOGUES = [0, routes.EPI_SILU_PAIRS]
KNOBS = [{}, {"GQ_AP_INREG": "0"}, {"GQ_AP_D": "2"}, {"GQ_AP_T": "512"}, {"GQ_AP_BPC": "1"}, {"GQ_AP_PT": "2"}]
KNOB_NAMES = sorted({k for s in KNOBS for k in s})


def shapes():
    out = []
    for model in routes.MODELS:
        out += [nk for nk in routes.shapes(model).values() if nk not in out]
    return out + [nk for nk in routes.EDGES if nk not in out]


def grid():
    """(knob set, N, K, prologue, epilogue) of every row"""
    return [(ks, N, K, pro, epi) for ks in range(len(KNOBS)) for N, K in shapes() for pro in PROLOGUES for epi in EPILOGUES]


def set_knobs(L, knobs):
    for k in KNOB_NAMES:
        os.environ.pop(k, None)
    os.environ.update(knobs)
    L.gq_reset_env_cache()


def plan(L, row, bits):
    _, N, K, pro, epi = row
    p = (ctypes.c_uint32 * 7)()
    rc = L.gq_debug_exact_plan_ex(N, K, bits, pro, epi, p)
    return rc if rc else list(p)


def record(L, rows):
    """rows with their results"""
    out, state = [], None
    for row in rows:
        if state != row[0]:
            set_knobs(L, KNOBS[row[0]])
            state = row[0]
        out.append(list(row) + [[plan(L, row, b) for b in BITS]])
    set_knobs(L, {})
    return out


def main(parent):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from guidedquant_amd import _lib
    L = _lib.lib()
    doc = {"parent": parent, "bits": BITS, "knobs": KNOBS, "rows": record(L, grid())}
    print(json.dumps(doc, separators=(",", ":")).replace("]],[", "]],\n["))


if __name__ == "__main__":
    main(sys.argv[1])
