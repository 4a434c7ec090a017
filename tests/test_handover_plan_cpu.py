"""CPU (host logic): gq_anyprec_handover_plan runs the library's own dispatch dry -- which launches of a decode step take the
statistics hand-over (include/gq_hip.h, round 5).  No device is touched (256 CUs are assumed without one)."""
from guidedquant_amd import _lib


def test_plan_follows_the_dispatch_on_the_stream_and_plane_kernels():
    L = _lib.lib()
    L.gq_set_ap_mode(0)
    try:
        # 8B 2-bit: the stream kernel's RMSNorm prologues read, the local-image kernel's residual epilogues write
        assert L.gq_anyprec_handover_plan(6144, 4096, 2, 1, 0) == 1
        assert L.gq_anyprec_handover_plan(28672, 4096, 2, 1, 4) == 1      # gate/up pair epilogue: nothing to write
        assert L.gq_anyprec_handover_plan(4096, 4096, 2, 0, 1) == 2
        assert L.gq_anyprec_handover_plan(4096, 14336, 2, 0, 1) == 2
        # 70B: wo on the stream kernel, w2 split along K over blocks -- neither has the in-epilogue form
        assert L.gq_anyprec_handover_plan(8192, 8192, 2, 0, 1) == 0
        assert L.gq_anyprec_handover_plan(8192, 28672, 2, 0, 1) == 0
        # bad shapes plan nothing
        assert L.gq_anyprec_handover_plan(0, 4096, 2, 1, 0) == 0 and L.gq_anyprec_handover_plan(4096, 4096, 9, 0, 1) == 0
        L.gq_set_ap_mode(1)
        assert L.gq_anyprec_handover_plan(6144, 4096, 2, 1, 0) == 0 and L.gq_anyprec_handover_plan(4096, 4096, 2, 0, 1) == 0
    finally:
        L.gq_set_ap_mode(-1)


def test_plan_is_empty_where_the_dq_kernel_serves(monkeypatch):
    """8B wqkv / wo at 3 bits run the decode-to-fp16 kernel (round 6: the dispatch tries it first), which has no hand-over form --
    neither reads nor writes.  With it switched off (GQ_DQ=0) the same launches run the shared-image plane kernel (wqkv: its prologue
    has no reading form, its plain epilogue writes) and the local-image kernel (wo: two epilogue waves per block write)."""
    L = _lib.lib()
    L.gq_set_ap_mode(0)
    try:
        for N, K, norm, epi in ((6144, 4096, 1, 0), (4096, 4096, 0, 1)):
            assert _lib.ap_plan_route(N, K, 3, 1, norm, epi)[0] == "dq"
            assert L.gq_anyprec_handover_plan(N, K, 3, norm, epi) == 0
        monkeypatch.setenv("GQ_DQ", "0")
        L.gq_reset_env_cache()
        assert _lib.ap_plan_route(6144, 4096, 3, 1, True, 0)[0] == "plane"
        assert L.gq_anyprec_handover_plan(6144, 4096, 3, 1, 0) == 2
        assert _lib.ap_plan_route(4096, 4096, 3, 1, False, 1)[0] == "plane-local"
        assert L.gq_anyprec_handover_plan(4096, 4096, 3, 0, 1) == 2
    finally:
        monkeypatch.delenv("GQ_DQ", raising=False)
        L.gq_reset_env_cache()
        L.gq_set_ap_mode(-1)
