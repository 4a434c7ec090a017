"""CPU: a source scan of guidedquant_amd/csrc -- the device helpers the kernel files share are defined ONCE (wave_util.h: casts,
reductions, descriptors, the asm vector-memory requests; plane_mfma.h: the pieces of the plane arithmetic; qtip_xform.h: the element-wise
arithmetic of the QTIP transform-in / transform-out; ap_exact.h: the fused prologues, the row request and the ordered reduction of the
exact / wide / dq GEMV kernels; sampler_core.h: the value images, the penalty, the race, the ban list, the log-sum-exp merge, publishing and
the embedding fold of the three sampler units), under names that tell their contracts apart, and the settled build-time forks are gone.  A second copy under the same name is how wave_reduce<true> came
to mean two things (identity 0 in one file, -3e38 in another)."""
import glob
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "guidedquant_amd", "csrc")
SOURCES = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))}

# name -> the one file that defines it.  A device function's definition is a line that STARTS with __device__ and names it in front
# of its parameter list (a call never starts a line that way).  ap_core.h's gq::u2h / gq::h2u are other functions under these names:
# the packed-pair casts of the exact path, host + device (GQ_HD) because the CPU twins compile them -- not matched, not meant.
DEVICE_FUNCTIONS = {
    "wave_util.h": ["h2f", "f2h", "u2h", "h2u", "u2h2", "h22u",                                             # the casts
                    "wave_reduce_l63", "lane63", "wave_reduce_bcast", "wave_allsum", "row_sum",             # the reductions
                    "make_rsrc", "make_rsrc4",                                                              # the descriptor
                    "dma16", "aload128", "bload16s", "tie128", "tie4", "wait_vm", "wait_vm_steps", "wait_vm_units", "lds_addr"],
    "plane_mfma.h": ["mfma_f4_bf8", "bf8_split", "hot_tau_bits", "silu_mul2"],
    "qtip_xform.h": ["h16_of", "sum_parts", "sum_parts4", "xf_out", "xf_resid", "xf_in", "xf_in_unit", "xf_in_h16", "xf_in_pack",  # the elements
                     "ssq_unit", "block_rms_scale", "seg_load", "seg_signed_sum", "qtip_transform_out"],
    # the fused prologues, the row request and the ordered reduction of the exact / wide / dq GEMV kernels
    "ap_exact.h": ["silu_mul_pk", "norm_pk", "rms_scale", "stage_items", "request_row", "silu_pair", "reduce_tree", "rows_epilogue_n",
                   "stage_x_natural"],
    # what sampler.hip, sampler_full.hip and topn.hip compare bit for bit ("The sampler's shared arithmetic once")
    "sampler_core.h": ["hash32", "ordered_key16", "unordered_key16", "ordered_key32", "unordered_key32", "is_nan16", "penalise",
                       "race_u", "race_score", "better", "ban_ids", "is_banned", "lse_merge128", "sample_publish", "sample_embed"],
}
SAMPLER_UNITS = ["sampler.hip", "sampler_full.hip", "topn.hip"]
OTHER_DEFINITIONS = {  # pattern -> the one file
    r"^\s*struct HotEnt\b": "plane_mfma.h",
    r"^\s*#\s*define\s+GQ_HOT_T\b": "plane_mfma.h",
    r"0x00020000": "wave_util.h",  # the descriptor's flags word, named once (RSRC_FLAGS)
}
# names that must not come back: the reduction name that had two contracts, the second threshold, the helpers' former private spellings
RETIRED = ["wave_reduce", "gq_wave_allsum", "GQ_ST_HOT_T", "g_dma16", "g_load16", "g_wait_vm", "g_rsrc"]
# build-time forks that were decided and taken out (DESIGN.md sections 3.5 - 3.7 keep the verdicts)
REMOVED_FORKS = ["PL_SSQ_MODE", "PL_BOOB", "PL_LOOB", "ST_DPPIMG", "ST_TAU_SCALE", "ST_MAINPRIO", "ST_AUX",
                 # qtip.hip's, and the helpers nothing called
                 "QT_ABL", "QT_SB", "QT_XOOB", "QT_PF", "QT_ENGINE_STAMPS", "unit_of", "qtip_xpos", "QtipNoop", "qtip_sum_parts",
                 # the dq kernel's and the pair-table default
                 "DQ_RING", "DQ_WAVES_N", "DQ_WPE3", "DQ_WPE4", "GQ_AP_PT_DEFAULT"]
QTIP_UNITS = [f for f in SOURCES if f.startswith("qtip") and f.endswith(".hip")]


def files_matching(pattern):
    rx = re.compile(pattern, re.M)
    return sorted(f for f, text in SOURCES.items() if rx.search(text))


def test_the_scan_sees_the_tree():
    assert len(SOURCES) >= 25 and "wave_util.h" in SOURCES and "plane_mfma.h" in SOURCES and "decode_util.h" not in SOURCES


@pytest.mark.parametrize("home,name", [(h, n) for h, names in DEVICE_FUNCTIONS.items() for n in names])
def test_device_helper_is_defined_in_one_file(home, name):
    assert files_matching(r"^\s*__device__[^;=\n]*[\s\*&]" + name + r"\s*\(") == [home]


@pytest.mark.parametrize("pattern,home", sorted(OTHER_DEFINITIONS.items()))
def test_type_and_constant_are_defined_in_one_file(pattern, home):
    assert files_matching(pattern) == [home]


@pytest.mark.parametrize("name", RETIRED + REMOVED_FORKS)
def test_retired_name_is_gone(name):
    assert files_matching(r"(?<![A-Za-z0-9_])" + name + r"(?![A-Za-z0-9_])") == []


def test_the_qtip_rounding_points_stand_in_the_header_only():
    # the division of the transform-in and the SiLU of its prologue: spelled in qtip_xform.h, in no kernel file (comments included)
    assert sorted(QTIP_UNITS) == ["qtip.hip", "qtip_gemm.hip", "qtip_xf.hip"]
    for f in QTIP_UNITS:
        assert "/ 32.0f" not in SOURCES[f] and "1.0f + __expf" not in SOURCES[f], f
    assert "/ 32.0f" in SOURCES["qtip_xform.h"] and "1.0f + __expf" in SOURCES["qtip_xform.h"]
    # n^-1/2 is rounded from double in one place (gq_inv_sqrt_f)
    assert SOURCES["qtip.hip"].count("pow((double)") + SOURCES["qtip_xf.hip"].count("pow((double)") <= 1


def test_the_exact_gemv_rounding_points_stand_in_the_header_only():
    # the SiLU of the SiLU * up prologue and of the gate/up pair outputs: spelled in ap_exact.h, in no kernel file that includes it
    units = sorted(f for f, text in SOURCES.items() if f.startswith("ap_") and f.endswith(".hip") and '#include "ap_exact.h"' in text)
    assert units == ["ap_dispatch.hip", "ap_dq.hip", "ap_gemv.hip", "ap_wide.hip"]  # (the dispatcher takes the launch arguments from it)
    for f in units:
        assert "1.0f + __expf" not in SOURCES[f] and "gq_pin_f32" not in SOURCES[f], f
    assert "1.0f + __expf" in SOURCES["ap_exact.h"] and "gq_pin_f32" in SOURCES["ap_exact.h"]


def test_the_race_stands_in_the_sampler_header_only():
    # the stream's constant and the score's two logarithms: spelled in sampler_core.h, in no sampler kernel file (comments included)
    for f in SAMPLER_UNITS:
        assert "0x9E3779B9" not in SOURCES[f] and "__logf(-__logf(" not in SOURCES[f], f
    assert SOURCES["sampler_core.h"].count("0x9E3779B9") == 1 and SOURCES["sampler_core.h"].count("__logf(-__logf(") == 1


def test_the_sampler_units_include_the_header():
    assert sorted(f for f, text in SOURCES.items() if '#include "sampler_core.h"' in text) == SAMPLER_UNITS
    # a host refusal the entry points share is one string: one message per mistake
    for msg in ("vocab too large for the fused sampler", "top_p must be in (0, 1]", "repetition_penalty must be finite", "ssq_out without x_out"):
        assert files_matching(re.escape(msg)) == ["sampler_core.h"], msg


def test_plane_core_stays_host_compilable():
    # (tests/test_lane_program_cpu.py and the CPU twins compile plane_core.h with a host compiler: the device pieces live next to it)
    text = SOURCES["plane_core.h"]
    assert "wave_util.h" not in text and "plane_mfma.h" not in text and "__builtin_amdgcn" not in text
