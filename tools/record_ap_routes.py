"""Records what the dry AP-GEMV dispatch (gq_debug_ap_plan_route) plans over a grid of launches, as the reference of
tests/test_ap_route_golden_cpu.py: a change that must not move the dispatch is checked against the record of the commit BEFORE it.

    git worktree add /tmp/parent <commit> && make -C /tmp/parent/guidedquant_amd/csrc
    GQ_LIB_PATH=/tmp/parent/guidedquant_amd/libgq_hip.so python tools/record_ap_routes.py <commit> > tests/golden/ap_routes.json

No device is touched (256 CUs are assumed without one).  The file: {"parent": commit, "bits": [2..9], "knobs": [knob set, ..], "rows": [..]};
a row is [knob set, mode, N, K, M, has_norm, epilogue, ws, results] with one result per bit width (9, which is refused, included; the rows
of a knob set: 2 to 4).  ws: 0 none, 1 the workspace
gq_anyprec_gemv_fused_ws_bytes asks for at that bit width (the w2 form); its result is then [route, bytes].  A route is the return code
when that is not 0, else family + 16 * launches + 64 * variant.
"""
import ctypes
import json
import os
import sys

EPI_RESIDUAL, PRO_SILU_MUL, EPI_SILU_PAIRS = 1, 2, 4
BITS = list(range(2, 10))  # (9: refused)
# (hidden, intermediate, wqkv rows)
MODELS = {"1B": (2048, 8192, 3072), "8B": (4096, 14336, 6144), "70B": (8192, 28672, 10240), "7B": (4096, 11008, 12288),
          "405B": (16384, 53248, 18432)}
EDGES = [(100, 96), (4096, 32768), (4096, 32800), (4096, 65536), (8192, 28672)]
# the decode step's launch forms: (has_norm, epilogue, ws)
FORMS = {"wqkv": (1, 0, 0), "wo": (0, EPI_RESIDUAL, 0), "w1w3": (1, EPI_SILU_PAIRS, 0), "w2": (0, EPI_RESIDUAL, 1)}
# launches the entry points refuse: (N, K, M, has_norm, epilogue)
REJECTED = [(4096, 4096, 2, 1, 0), (4096, 4096, 2, 0, EPI_RESIDUAL), (4096, 4096, 1, 1, PRO_SILU_MUL), (4096, 4096, 1, 0, EPI_SILU_PAIRS | EPI_RESIDUAL),
            (4097, 4096, 1, 1, EPI_SILU_PAIRS), (4096, 4096, 9, 0, 0), (4096, 48, 1, 0, 0), (0, 4096, 1, 0, 0)]
KNOBS = [{}] + [{"GQ_ST": v} for v in "023"] + [{"GQ_PL_LOCAL": "0"}, {"GQ_DQ": "0"}, {"GQ_PL_MIN_MWEIGHTS": "0"}, {"GQ_PL_MAX_BITS": "2"},
                                                {"GQ_AP_FORCE_GENERIC": "1"}, {"GQ_AP_PT": "1"}, {"GQ_AP_PT": "2"}, {"GQ_ST_KSPLIT": "0"},
                                                {"GQ_PL_ONEPASS": "0"}]
KNOB_NAMES = sorted({k for s in KNOBS for k in s})


def shapes(model):
    D, F, Q = MODELS[model]
    return {"wqkv": (Q, D), "wo": (D, D), "w1w3": (2 * F, D), "w2": (D, F)}


def grid():
    """(knob set, mode, N, K, M, has_norm, epilogue, ws) of every row"""
    rows = []
    for mode in (0, 1):
        for model in MODELS:
            for name, (N, K) in shapes(model).items():
                forms = [FORMS[name]] + ([FORMS["wo"]] if name == "w2" else [])
                rows += [(0, mode, N, K, 1, *f) for f in forms] + [(0, mode, N, K, M, 0, 0, 0) for M in (1, 2, 4, 5, 8)]
        for N, K in EDGES:
            rows += [(0, mode, N, K, 1, *f) for f in FORMS.values()] + [(0, mode, N, K, M, 0, 0, 0) for M in (1, 2, 4, 5, 8)]
        rows += [(0, mode, N, K, M, norm, epi, 0) for N, K, M, norm, epi in REJECTED]
        for ks in range(1, len(KNOBS)):
            for model in ("8B", "70B"):
                for name, (N, K) in shapes(model).items():
                    forms = [FORMS[name]] + ([FORMS["wo"]] if name == "w2" else [])
                    rows += [(ks, mode, N, K, 1, *f) for f in forms] + [(ks, mode, N, K, M, 0, 0, 0) for M in (1, 4)]
    return rows


def set_knobs(L, knobs):
    for k in KNOB_NAMES:
        os.environ.pop(k, None)
    os.environ.update(knobs)
    L.gq_reset_env_cache()


def plan(L, row, bits):
    """the result of one row at one bit width, under the knob set and mode the caller has set"""
    _, _, N, K, M, norm, epi, ws = row
    need = L.gq_anyprec_gemv_fused_ws_bytes(N, K, bits, epi) if ws else 0
    r = (ctypes.c_uint32 * 3)()
    rc = L.gq_debug_ap_plan_route(N, K, bits, M, norm, epi, need, r)
    route = rc if rc else r[0] + 16 * r[1] + 64 * r[2]
    return [route, need] if ws else route


def record(L, rows):
    """rows with their results"""
    out, state = [], None
    for row in rows:
        if state != row[:2]:
            set_knobs(L, KNOBS[row[0]])
            L.gq_set_ap_mode(row[1])
            state = row[:2]
        out.append(list(row) + [[plan(L, row, b) for b in (BITS if row[0] == 0 else BITS[:3])]])
    set_knobs(L, {})
    L.gq_set_ap_mode(-1)
    return out


def main(parent):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from guidedquant_amd import _lib
    L = _lib.lib()
    doc = {"parent": parent, "bits": BITS, "knobs": KNOBS, "rows": record(L, grid())}
    print(json.dumps(doc, separators=(",", ":")).replace("]],[", "]],\n["))


if __name__ == "__main__":
    main(sys.argv[1])
