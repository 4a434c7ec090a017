"""QTIP prompt path: the batched middle step of a QTIP linear (z = x @ decode(trellis)^T, S rows) three ways -- the row loop
(S gq_qtip_matvec launches: what BitshiftLinear.forward did for every bs > 1), the reference's two steps (gq_qtip_decompress
to a dense fp16 W + torch.matmul: kernel_decompress.py:82-91) and the fused gq_qtip_gemm (plus the two steps with an fp32 output: the batched op's form from 256 rows on) -- on the Llama-2-7b shapes, R = 2/3/4,
S = 16/128/256/512/2048; then the Llama-2-7b QTIP prompt pass (random init, R = 2) at S = 128 / 512: module forward with the row
loop (GQ_QTIP_GEMM=0), module forward with the GEMM, and Transformer.prefill_native where the model is prefill-ready.
Timing: HIP events around `iters` launches, each on the next of > 512 MB of trellis copies (no launch finds its weights in the
caches); best of 3 such runs.  Prints ONE JSON line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from guidedquant_amd import _lib  # noqa: E402

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008)]


def _time_us(run, n, iters):
    run(0)
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            run((i + 1) % n)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return best


def bench_shape(M, K, R, S_list, d):
    L = _lib.lib()
    per = R * M * K // 8
    n = max(2, min(256, (512 << 20) // per + 1))
    tr = [torch.randint(-2**31, 2**31 - 1, (R * M * K // 32, ), dtype=torch.int32, device=d) for _ in range(n)]
    tl = torch.clamp(torch.randn(1024, device=d) / 16, -1, 1).half()
    W = torch.empty((M, K), dtype=torch.float16, device=d)
    rows = []
    for S in S_list:
        x = (torch.randn(S, K, device=d) / 16).half()
        y = torch.empty((S, M), dtype=torch.float32, device=d)
        nb = L.gq_qtip_gemm_ws_bytes(S, M, K, R)
        ws = torch.empty(max(nb // 4, 4), dtype=torch.float32, device=d)
        sp = _lib.current_stream_ptr()

        def gemm(i):
            rc = L.gq_qtip_gemm_ws(y.data_ptr(), tr[i].data_ptr(), x.data_ptr(), tl.data_ptr(), S, M, K, R, ws.data_ptr() if nb else None, nb, sp)
            assert rc == 0, L.gq_last_error()

        def two_step(i):
            rc = L.gq_qtip_decompress(W.data_ptr(), tr[i].data_ptr(), tl.data_ptr(), M, K, R, sp)
            assert rc == 0, L.gq_last_error()
            torch.matmul(x, W.T)

        def two_step_f32(i):  # (the form the batched op takes from GQ_QTIP_TWO_STEP_S rows on: fp32 output)
            rc = L.gq_qtip_decompress(W.data_ptr(), tr[i].data_ptr(), tl.data_ptr(), M, K, R, sp)
            assert rc == 0, L.gq_last_error()
            torch.mm(x, W.T, out_dtype=torch.float32)

        yv = torch.empty((M, ), dtype=torch.float32, device=d)

        def row_loop(i):
            for s in range(S):
                rc = L.gq_qtip_matvec(yv.data_ptr(), tr[i].data_ptr(), x[s].data_ptr(), tl.data_ptr(), M, K, R, sp)
                assert rc == 0, L.gq_last_error()

        iters = max(4, min(64, 20000 // max(S, 1)))
        t_gemm = _time_us(gemm, n, iters)
        t_two = _time_us(two_step, n, iters)
        t_two32 = _time_us(two_step_f32, n, iters)
        t_loop = _time_us(row_loop, n, max(2, min(iters, 4096 // S)))
        fl = 2.0 * S * M * K
        rows.append({"M": M, "K": K, "R": R, "S": S, "row_loop_us": round(t_loop, 2), "decompress_matmul_us": round(t_two, 2), "decompress_mm_f32out_us": round(t_two32, 2),
                     "qtip_gemm_us": round(t_gemm, 2), "qtip_gemm_tflops": round(fl / t_gemm / 1e6, 1),
                     "decompress_matmul_tflops": round(fl / t_two / 1e6, 1), "gemm_vs_loop": round(t_loop / t_gemm, 1),
                     "gemm_vs_two_step": round(t_two / t_gemm, 2), "ksplit_ws_bytes": int(nb)})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    del tr
    torch.cuda.empty_cache()
    return rows


def bench_model(d, S_list):
    from guidedquant_amd.generate import load_model
    torch.manual_seed(0)
    m = load_model("meta-llama/Llama-2-7b", d, "qtip", 2, random_init=True)
    m.setup_caches(1, max(S_list) + 8)
    out = []
    for S in S_list:
        x = torch.randint(0, 32000, (1, S), dtype=torch.int32, device=d)
        pos = torch.arange(S, dtype=torch.int32, device=d)
        res = {"S": S}
        modes = [("module_row_loop_ms", "0", lambda: m(x, pos)), ("module_gemm_ms", "1", lambda: m(x, pos))]
        if m.prefill_ready(x):
            modes.append(("prefill_native_ms", "1", lambda: m.prefill_native(x, pos, start=0, last_only=True)))
        for key, env, fn in modes:
            os.environ["GQ_QTIP_GEMM"] = env
            with torch.no_grad():
                fn()
                torch.cuda.synchronize()
                best = 1e30
                for _ in range(2 if env == "0" else 3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    lg = fn()
                    e1.record()
                    e1.synchronize()
                    best = min(best, e0.elapsed_time(e1))
            assert torch.isfinite(lg.float()).all()
            res[key] = round(best, 2)
        os.environ.pop("GQ_QTIP_GEMM", None)
        print(json.dumps(res), file=sys.stderr, flush=True)
        out.append(res)
    del m
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", default="2,3,4")
    ap.add_argument("--S", default="16,128,256,512,2048")
    ap.add_argument("--shapes", default="all", help="all | 0,1,2 (indices into the Llama-2-7b shape list)")
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    d = torch.device("cuda:0")
    shapes = SHAPES if a.shapes == "all" else [SHAPES[int(i)] for i in a.shapes.split(",")]
    res = {"bench": "qtip_prefill", "device": torch.cuda.get_device_name(d), "shapes": []}
    for M, K in shapes:
        for R in (int(r) for r in a.R.split(",")):
            res["shapes"] += bench_shape(M, K, R, [int(s) for s in a.S.split(",")], d)
    if not a.no_model:
        res["llama2_7b_R2_prompt_pass"] = bench_model(d, [128, 512])
    print(json.dumps(res), flush=True)
