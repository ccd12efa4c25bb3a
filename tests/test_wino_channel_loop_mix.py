"""Static check of the channel-BatchNorm form of the Winograd kernel, conv_wino_kernel<128, true,
192, 3> (tools/loop_mix.py; CPU only, hipcc cross-compile), in the style of
tests/test_wino_loop_mix.py: no scratch, 72 MFMAs per steady loop block, and no more VALU
instructions per block than measured when the form was merged.

The column form (BNM 1) has 149 and 249 VALU in its phase-1 and phase-2 loop blocks (pinned at
its earlier 350). The channel form has 150 and 250: U = med3(cx x + cc, 0, limit) does the ReLU
and the halo select in the instruction the column form spends on its max, and the one extra
instruction per block is the address of the chunk's coefficient slice (its 16 coefficients are
four LDS reads per chunk-phase, not VALU)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAG = "conv_wino_kernelILi128ELb1ELi192ELi3EE"
MOST_VALU = 250


@pytest.mark.slow
def test_channel_form_loop_mix():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from loop_mix import assembly, kernels
    mix = kernels(assembly(os.path.join(ROOT, "csrc", "hip", "conv_wino.hip")))
    hits = [k for n, k in mix.items() if FRAG in n]
    assert len(hits) == 1, len(hits)
    k = hits[0]
    assert k["scratch"] == 0, "%d bytes of scratch" % k["scratch"]
    blocks = [b for b in k["blocks"] if b["self_loop"]]
    assert len(blocks) == 2, "the phase-1 and the phase-2 loop"
    for b in blocks:
        print("%s: %d MFMA, %d VALU, %d VGPRs" % (b["label"], b["mfma"], b["valu"], k["vgprs"]))
        assert b["mfma"] == 72 and b["valu"] <= MOST_VALU, b
