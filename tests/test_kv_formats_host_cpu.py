"""No GPU: the table of KV-cache formats (`model.KV_FORMATS`) against everything it stands for -- the names `kv_cache_dtype_name` accepts,
the C entries, the shapes `KVCache` allocates, the plan suffixes of the prompt pass, and `KVCache.update` against the formats' host models."""
import pytest

torch = pytest.importorskip("torch")

from guidedquant_amd import _lib, model as gm  # noqa: E402
from guidedquant_amd.native_prompt import attention_plan  # noqa: E402

NAMES = ("fp16", "fp8", "fp8_row", "mxfp4")
B, S, H, HD = 1, 8, 2, 64
ROW_BYTES = dict(fp16=128, fp8=64, fp8_row=64, mxfp4=32)
EXP_SHAPE = dict(fp16=None, fp8=None, fp8_row=(B, H, S), mxfp4=(B, H, S, 2))


def _cache(name):
    return gm.KVCache(B, S, H, HD, torch.float16, "cpu", kv_cache_dtype=name)


def test_the_keys_are_the_names_the_validator_accepts():
    assert tuple(gm.KV_FORMATS) == NAMES and all(f.name == n for n, f in gm.KV_FORMATS.items())
    for n in NAMES:
        assert gm.kv_cache_dtype_name(n) == n
    assert gm.kv_cache_dtype_name(None) == "fp16"
    for bad in ("fp4", "int8", "FP8", ""):
        with pytest.raises(ValueError, match="kv_cache_dtype="):
            gm.kv_cache_dtype_name(bad)


@pytest.mark.parametrize("name", NAMES)
def test_every_entry_is_exported(name):
    f = gm.KV_FORMATS[name]
    assert {f.rows, f.decode, f.prompt} <= set(_lib.EXPORTS)
    sfx = {"fp16": "", "fp8": "_kv8", "fp8_row": "_kv8r", "mxfp4": "_mx4"}[name]
    assert (f.rows, f.decode, f.prompt) == ("gq_rope_cache_rows" + sfx, "gq_attn_decode_roped" + sfx, "gq_attn_prefill" + sfx)


@pytest.mark.parametrize("name", NAMES)
def test_what_the_cache_allocates(name):
    f, kc = gm.KV_FORMATS[name], _cache(name)
    for c in (kc.k_cache, kc.v_cache):
        assert tuple(c.shape[:3]) == (B, H, S) and c.shape[3] * c.element_size() == ROW_BYTES[name] == f.row_bytes(HD)
    assert f.exp_bytes(HD) == {"fp16": 0, "fp8": 0, "fp8_row": 1, "mxfp4": HD // 32}[name]
    for e in ("k_exp", "v_exp"):
        if EXP_SHAPE[name] is None:
            assert not hasattr(kc, e)
        else:
            t = getattr(kc, e)
            assert tuple(t.shape) == EXP_SHAPE[name] and t.dtype == torch.uint8 and t[0].numel() == H * S * f.exp_bytes(HD)
    for s in ("k_scale", "v_scale", "k_inv", "v_inv"):
        assert hasattr(kc, s) == (name == "fp8") == f.head_scales
    assert (kc.fp8, kc.fp8_row, kc.mxfp4) == (name == "fp8", name == "fp8_row", name == "mxfp4") and f.quantized == (name != "fp16")


def test_the_constructor_keywords_name_the_same_formats():
    for kw, name in (("fp8", "fp8"), ("fp8_row", "fp8_row"), ("mxfp4", "mxfp4")):
        a, b = gm.KVCache(B, S, H, HD, torch.float16, "cpu", **{kw: True}), _cache(name)
        assert a.fmt is b.fmt is gm.KV_FORMATS[name] and sorted(n for n, _ in a.named_buffers()) == sorted(n for n, _ in b.named_buffers())
    assert gm.KVCache(B, S, H, HD, torch.float16, "cpu").fmt is gm.KV_FORMATS["fp16"]
    with pytest.raises(AssertionError):
        gm.KVCache(B, S, H, HD, torch.float16, "cpu", fp8=True, mxfp4=True)


@pytest.mark.parametrize("name", NAMES)
def test_the_plan_ends_in_the_suffix(name):
    f = gm.KV_FORMATS[name]
    flags = dict(fp16=(False, False, False), fp8=(True, False, False), fp8_row=(True, True, False), mxfp4=(True, False, True))[name]
    assert f.suffix == {"fp16": "", "fp8": "-kv8", "fp8_row": "-kv8r", "mxfp4": "-mx4"}[name]
    for mode in ("auto", "0", "1"):
        for pieces in (1, 2):
            for sup in (False, True):
                plan = attention_plan(mode, pieces, flags[0], sup, flags[1], flags[2])
                assert plan in ("hip" + f.suffix, "sdpa" + f.suffix), plan
                assert plan.startswith("hip") == (mode != "0" and sup and (mode == "1" or pieces > 1 or f.quantized))


@pytest.mark.parametrize("name", NAMES)
def test_update_then_read_is_the_host_model_of_the_format(name):
    g = torch.Generator().manual_seed(5)
    kc = _cache(name)
    if name == "fp8":
        kc.set_scales(torch.tensor([0.5, 2.0]), torch.tensor([4.0, 0.25]))
    pos = torch.tensor([1, 2, 6])
    k = (torch.randn(B, H, 3, HD, generator=g) * 3).half()
    v = (torch.randn(B, H, 3, HD, generator=g) * 40).half()
    v[0, 1, 2, :32] *= 2.0 ** -12  # (a block far below its row's maximum)
    got_k, got_v = kc.update(pos, k, v)
    for got, x, w in ((got_k, k, "k"), (got_v, v, "v")):
        assert tuple(got.shape) == (B, H, S, HD) and got.dtype == torch.float16
        if name == "fp16":
            want = x
        elif name == "fp8":
            codes = gm.fp8_quantize(x, getattr(kc, w + "_inv"))
            assert torch.equal(getattr(kc, w + "_cache").view(torch.uint8)[:, :, pos], codes)
            want = (codes.view(torch.float8_e4m3fn).float() * getattr(kc, w + "_scale")[:, None, None]).half()
        elif name == "fp8_row":
            codes, byte = gm.fp8_row_quantize(x)
            assert torch.equal(getattr(kc, w + "_cache").view(torch.uint8)[:, :, pos], codes) and torch.equal(getattr(kc, w + "_exp")[:, :, pos], byte)
            want = (codes.view(torch.float8_e4m3fn).float() * gm.fp8_row_scale(byte)[..., None]).half()
        else:
            codes, byte = gm.mxfp4_quantize(x)
            assert torch.equal(getattr(kc, w + "_cache")[:, :, pos], codes) and torch.equal(getattr(kc, w + "_exp")[:, :, pos], byte)
            want = gm.mxfp4_dequant(codes, byte)
        assert torch.equal(got[:, :, pos], want)
        assert torch.equal(got[:, :, [0, 3, 4, 5, 7]], torch.zeros(B, H, 5, HD, dtype=torch.float16))  # (rows never written read back 0)
        assert torch.equal(kc.values(w, (slice(0, 1), slice(None), slice(0, 7))), got[:1, :, :7])
