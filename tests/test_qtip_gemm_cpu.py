"""CPU: the QTIP prompt-path entry points (gq_qtip_decompress, gq_qtip_gemm, gq_qtip_gemm_ws) are declared, bound and exported,
and the HIP prompt pass is never offered for a QTIP model that lives on the CPU."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

NAMES = ("gq_qtip_decompress", "gq_qtip_gemm", "gq_qtip_gemm_ws", "gq_qtip_gemm_ws_bytes")


def test_qtip_gemm_entry_points_declared_and_exported():
    from guidedquant_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gq_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name


def test_qtip_gemm_ws_bytes_needs_no_split_for_unsupported_shapes():
    from guidedquant_amd import _lib
    L = _lib.lib()
    assert L.gq_qtip_gemm_ws_bytes(128, 100, 4096, 2) == 0  # M not a multiple of 32: no kernel, no workspace
    assert L.gq_qtip_gemm_ws_bytes(128, 4096, 4096, 5) == 0  # R outside 2..4
    assert L.gq_qtip_gemm_ws_bytes(0, 4096, 4096, 2) == 0


def test_qtip_gemm_rejects_unsupported_shapes_without_launching():
    from guidedquant_amd import _lib
    L = _lib.lib()
    assert L.gq_qtip_gemm(None, None, None, None, 16, 100, 4096, 2, None) == _lib.GQ_ENOTSUP
    assert L.gq_qtip_gemm(None, None, None, None, 16, 4096, 4096, 1, None) == _lib.GQ_ENOTSUP
    assert L.gq_qtip_decompress(None, None, None, 4096, 48, 2, None) == _lib.GQ_ENOTSUP


def test_cpu_qtip_model_is_not_prefill_ready():
    from guidedquant_amd import model as gm
    from guidedquant_amd.generate import load_model
    gm.transformer_configs["qtip-cpu-prefill-test"] = dict(model_name="llama-qtip-cpu-prefill-test", block_size=64, vocab_size=256,
                                                           n_layer=1, n_head=4, dim=256, intermediate_size=512, n_local_heads=4)
    try:
        m = load_model("qtip-cpu-prefill-test", "cpu", "qtip", 2, random_init=True)
    finally:
        del gm.transformer_configs["qtip-cpu-prefill-test"]
    m.setup_caches(max_batch_size=1, max_seq_length=32)
    idx = torch.arange(24, dtype=torch.int32).reshape(1, -1)
    assert not m.prefill_ready(idx)
