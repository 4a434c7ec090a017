"""The AP-GEMV launches the benchmark makes, in the form the decode step issues them (guidedquant_amd/native_step.py::ApStep.layers,
pair path) and as roofline_by_shape times the plain operator, each with the kernel family the default dispatch sends it to on an MI355X
(256 CUs, M = 1).  Data only: tests/test_dispatch_table_cpu.py checks the dry dispatch against it, tests/test_dispatch_parity_gpu.py
runs every row on its route against the oracle.

A row: (model, bits, name, N, K, has_norm, epilogue, ws_bytes, route).  epilogue: the GQ_EPI_* / GQ_PRO_* flags; ws_bytes: the w2
workspace the model passes (gq_anyprec_gemv_fused_ws_bytes, nonzero at 70B 2-bit only).  wqkv is listed in its fused RMSNorm form (the
decode step's q / k / v + RoPE launch runs the same stream kernel where the library serves it that way).
"""
EPI_RESIDUAL, PRO_SILU_MUL, EPI_SILU_PAIRS = 1, 2, 4

DIMS = {"8B": (4096, 14336, 6144), "70B": (8192, 28672, 10240)}  # hidden, intermediate, wqkv rows
W2_WS_BYTES = {("70B", 2): 229376}

# default-dispatch family of each launch (the w2 row of 70B 2-bit with its workspace; without one it is the two-launch plane chain)
ROUTES = {
    ("8B", 2): {"wqkv": "stream", "wo": "plane-local", "w1w3": "stream", "w2": "plane-local"},
    ("8B", 3): {"wqkv": "dq", "wo": "dq", "w1w3": "dq", "w2": "dq"},
    ("8B", 4): {"wqkv": "dq", "wo": "dq", "w1w3": "dq", "w2": "dq"},
    ("70B", 2): {"wqkv": "plane", "wo": "stream", "w1w3": "plane", "w2": "stream-ksplit"},
    ("70B", 3): {"wqkv": "dq", "wo": "dq", "w1w3": "plane", "w2": "dq"},
    ("70B", 4): {"wqkv": "dq", "wo": "dq", "w1w3": "dq", "w2": "dq"},
}
W2_NO_WS_ROUTE = "plane-chain"  # 70B 2-bit w2 without the workspace

# bench.py roofline_by_shape: the plain operator (gq_anyprec_gemv) on the 8B shapes
PLAIN_ROUTES = {
    2: {"wqkv": "plane", "wo": "plane-local", "w1w3": "stream", "w2": "plane-local"},
    3: {"wqkv": "dq", "wo": "dq", "w1w3": "dq", "w2": "dq"},
    4: {"wqkv": "dq", "wo": "dq", "w1w3": "dq", "w2": "dq"},
}


def _decode_rows():
    rows = []
    for model, (D, F, Q) in DIMS.items():
        for bits in (2, 3, 4):
            forms = {"wqkv": (Q, D, True, 0), "wo": (D, D, False, EPI_RESIDUAL), "w1w3": (2 * F, D, True, EPI_SILU_PAIRS),
                     "w2": (D, F, False, EPI_RESIDUAL)}
            for name, (N, K, norm, epi) in forms.items():
                ws = W2_WS_BYTES.get((model, bits), 0) if name == "w2" else 0
                rows.append((model, bits, name, N, K, norm, epi, ws, ROUTES[(model, bits)][name]))
    return rows


def _plain_rows():
    D, F, Q = DIMS["8B"]
    shapes = {"wqkv": (Q, D), "wo": (D, D), "w1w3": (2 * F, D), "w2": (D, F)}
    return [("8B-plain", bits, name, N, K, False, 0, 0, PLAIN_ROUTES[bits][name]) for bits in (2, 3, 4) for name, (N, K) in shapes.items()]


ROWS = _decode_rows() + _plain_rows()


def row_id(row):
    model, bits, name = row[:3]
    return f"{model}-{bits}bit-{name}"
