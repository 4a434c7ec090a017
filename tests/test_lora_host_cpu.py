"""CPU: lora.LoraAdapter.from_peft -- peft's key layout and adapter_config.json fields into the stacked, padded tensors and segment tables the
kernels read (guidedquant_amd/lora.py), every refusal, and a round trip from a synthetic peft state dict to the float64 delta."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from guidedquant_amd.lora import LoraAdapter  # noqa: E402
from guidedquant_amd.model import ModelArgs, Transformer  # noqa: E402

CFG = ModelArgs(block_size=64, vocab_size=64, n_layer=2, n_head=2, dim=128, intermediate_size=256, n_local_heads=1, model_name="llama-test")
SHAPES = dict(q_proj=(128, 128), k_proj=(64, 128), v_proj=(64, 128), o_proj=(128, 128), down_proj=(128, 256), gate_proj=(256, 128))
PEFT = dict(r=5, lora_alpha=10, target_modules=["q_proj", "v_proj", "o_proj", "down_proj"], bias="none", use_dora=False, use_rslora=False,
            rank_pattern={"layers.1.self_attn.v_proj": 17}, alpha_pattern={"v_proj": 34})


def _sd(targets=("q_proj", "v_proj", "o_proj", "down_proj"), ranks=None, seed=0):
    # a peft-layout state dict of fp16-representable values: rank 5 everywhere but `ranks[(layer, name)]`
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for layer in range(CFG.n_layer):
        for name in targets:
            r = (ranks or {(1, "v_proj"): 17}).get((layer, name), 5)
            n_out, n_in = SHAPES[name]
            base = f"base_model.model.model.layers.{layer}.{'mlp' if name in ('down_proj', 'gate_proj') else 'self_attn'}.{name}"
            sd[base + ".lora_A.weight"] = torch.randn(r, n_in, generator=g).half().float()
            sd[base + ".lora_B.default.weight"] = torch.randn(n_out, r, generator=g).half().float()
    return sd


def test_from_peft_stacks_pads_and_scales():
    ad = LoraAdapter.from_peft(_sd(), PEFT, CFG)
    assert len(ad.modules) == 8 and [sorted(k for k, v in lay.items() if v) for lay in ad.layers] == [["down", "o", "qkv"]] * 2
    q0, q1 = ad.layers[0]["qkv"], ad.layers[1]["qkv"]
    # q rows [0, 128), k untargeted, v rows [192, 256); rank 5 -> 16 rows of A each; alpha_pattern gives v 34 / r
    assert q0.segments == [(0, 128, 0, 16, 0, 2.0), (192, 256, 16, 16, 128 * 16, 34 / 5)] and (q0.R, q0.K, q0.N) == (32, 128, 256)
    assert q1.segments == [(0, 128, 0, 16, 0, 2.0), (192, 256, 16, 32, 128 * 16, 2.0)] and tuple(q1.A.shape) == (48, 128)
    assert not q0.A[5:16].any() and not q0.B[:128 * 16].view(128, 16)[:, 5:].any()  # (the padding is zeros)
    assert ad.layers[0]["down"].segments == [(0, 128, 0, 16, 0, 2.0)] and ad.layers[0]["down"].K == 256
    for form in ("all-linear", r".*\.(q|v|o|down)_proj"):  # (peft's string forms of target_modules: the keys decide)
        assert len(LoraAdapter.from_peft(_sd(), dict(PEFT, target_modules=form)).modules) == 8
    first = ad.layers
    assert ad.bind(CFG, "cpu") is first and ad.bind(CFG, "meta") is not first and ad.bind(CFG, "cpu") is first  # (a binding per model kind)


def test_round_trip_to_the_float64_delta():
    sd = _sd()
    ad = LoraAdapter.from_peft(sd, PEFT, CFG)
    x = torch.randn(3, 128, generator=torch.Generator().manual_seed(1)).half()
    got = ad.layers[1]["qkv"].delta_rows(x).double().numpy()
    pre = "base_model.model.model.layers.1.self_attn."
    ref = np.zeros((3, 256))
    for name, rows, s in (("q_proj", slice(0, 128), 2.0), ("v_proj", slice(192, 256), 2.0)):
        A, B = sd[pre + name + ".lora_A.weight"].double().numpy(), sd[pre + name + ".lora_B.default.weight"].double().numpy()
        ref[:, rows] = s * (x.double().numpy() @ A.T) @ B.T
    assert np.abs(ref).max() > 1 and not got[:, 128:192].any()
    assert (np.abs(got - ref) <= 2.0**-10 * np.abs(ref) + 1e-6).all()  # (one fp16 rounding of an fp32 sum of exact inputs)


@pytest.mark.parametrize("sd,cfg,match", [
    (_sd(("q_proj", "gate_proj")), dict(PEFT, target_modules=["q_proj", "gate_proj"]), "gate_proj"),
    (_sd(), dict(PEFT, target_modules=r".*\.q_proj"), "does not match target_modules"),
    (_sd(("gate_proj", )), dict(PEFT, target_modules="all-linear"), "gate_proj.*in front of SiLU"),
    (_sd(), dict(PEFT, use_dora=True), "use_dora"),
    (_sd(), dict(PEFT, use_rslora=True), "use_rslora"),
    (_sd(), dict(PEFT, bias="all"), "bias"),
    (_sd(), dict(PEFT, modules_to_save=["lm_head"]), "modules_to_save"),
    (_sd(ranks={(0, "q_proj"): 65}), dict(PEFT, rank_pattern={"layers.0.self_attn.q_proj": 65}), "rank 65"),
    (_sd(ranks={(0, "q_proj"): 6}), dict(PEFT, rank_pattern=None), "do not match rank"),
    ({k: v for k, v in _sd().items() if "layers.0.self_attn.q_proj.lora_B" not in k}, PEFT, "pairs"),
    (dict(_sd(), **{"base_model.model.lm_head.lora_A.weight": torch.zeros(5, 128)}), PEFT, "unexpected key"),
])
def test_from_peft_refusals(sd, cfg, match):
    with pytest.raises(ValueError, match="lora: .*" + match):
        LoraAdapter.from_peft(sd, cfg, CFG)


def test_shapes_must_match_the_model_and_only_fused_models_take_an_adapter():
    ad = LoraAdapter.from_peft(_sd(), PEFT)
    wide = ModelArgs(block_size=64, vocab_size=64, n_layer=2, n_head=2, dim=256, intermediate_size=256, n_local_heads=1, model_name="llama-test")
    with pytest.raises(ValueError, match="lora: .*do not match the model"):
        ad.bind(wide, "cpu")
    m = Transformer(torch.float32, CFG, fuse_linears=False)
    with pytest.raises(NotImplementedError, match="lora: "):
        m.set_adapter(ad)
    m = Transformer(torch.float32, CFG)
    m.set_adapter(ad)
    m.setup_caches(1, 8)
    with pytest.raises(ValueError, match="lora: the module-by-module forward"):
        m(torch.zeros(1, 1, dtype=torch.long), torch.zeros(1, dtype=torch.long))
