"""CPU: the fused sampler's vocabulary limit is stated once per layer and the statements agree -- `_lib.SAMPLER_MAX_VOCAB` (what
`AnyPrecisionForCausalLM.generate` gates its fused routes on), `GQ_SAMPLER_MAX_VOCAB` of include/gq_hip.h (which csrc/sampler.hip
compiles its slices from and csrc/sampler_core.h the check every sampler entry makes) and the message of the refusal."""
import os
import re

from conftest import ROOT


def test_sampler_limit_is_262144_in_the_binding_the_header_and_the_kernel_file():
    from guidedquant_amd import _lib
    assert _lib.SAMPLER_MAX_VOCAB == 262144
    header = open(os.path.join(ROOT, "include", "gq_hip.h")).read()
    m = re.search(r"#define\s+GQ_SAMPLER_MAX_VOCAB\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.SAMPLER_MAX_VOCAB
    src = open(os.path.join(ROOT, "guidedquant_amd", "csrc", "sampler.hip")).read()
    assert "SAMP_MAX_VOCAB = GQ_SAMPLER_MAX_VOCAB" in src
    # the refusal: one check and one message for the three sampler units, compiled from the same constant
    core = open(os.path.join(ROOT, "guidedquant_amd", "csrc", "sampler_core.h")).read()
    assert "vocab > GQ_SAMPLER_MAX_VOCAB" in core and "sample_vocab_ok(vocab)" in src
    msg = re.search(r'"vocab too large for the fused sampler \(<= (\d+)\)\."', core)
    assert msg and int(msg.group(1)) == _lib.SAMPLER_MAX_VOCAB
