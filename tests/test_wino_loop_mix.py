"""Static check of the Winograd kernels' gfx950 code (tools/loop_mix.py; CPU only, hipcc
cross-compile): the K loop's vector instructions per MFMA.

A v_mfma_f32_16x16x32_bf16 occupies the matrix pipe for 16 cycles and holds the SIMD's vector
issue for 8 of them; a plain VALU instruction costs 4 issue cycles. At r VALU per MFMA the issue
time per MFMA slot is 8 + 4 r cycles, above the pipe's 16 from r = 2.0 on: every self-looping
MFMA block of the plain forms must stay at or below that break-even (docs/KERNELS.md, "Winograd
loop: VALU per MFMA"). The fused-BatchNorm forms carry their BN arithmetic in the transform and
may not exceed the counts they had before the loop's geometry moved out of it (350 and 222 VALU
per 72 MFMAs). No instantiation that ran without scratch may use any."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mangled-name fragments: kernel<WN, one board per block, PAIRS, BN form> / chain<WN, one board>
PLAIN = {
    "conv_wino_chain_kernel<192,true>": "conv_wino_chain_kernelILi192ELb1EE",
    "conv_wino_kernel<192,true,192,0>": "conv_wino_kernelILi192ELb1ELi192ELi0EE",
    "conv_wino_kernel<192,true,96,0>": "conv_wino_kernelILi192ELb1ELi96ELi0EE",
    "conv_wino_kernel<128,true,192,0>": "conv_wino_kernelILi128ELb1ELi192ELi0EE",
    "conv_wino_chain_kernel<128,true>": "conv_wino_chain_kernelILi128ELb1EE",
}
# name: (fragment, most VALU per steady loop block of 72 MFMAs)
BN = {
    "conv_wino_kernel<128,true,192,1>": ("conv_wino_kernelILi128ELb1ELi192ELi1EE", 350),
    "conv_wino_kernel<128,true,192,2>": ("conv_wino_kernelILi128ELb1ELi192ELi2EE", 222),
}


@pytest.fixture(scope="module")
def mix():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from loop_mix import assembly, kernels
    return kernels(assembly(os.path.join(ROOT, "csrc", "hip", "conv_wino.hip")))


def kernel(mix, frag):
    hits = [k for n, k in mix.items() if frag in n]
    assert len(hits) == 1, (frag, len(hits))
    return hits[0]


def loops(k):
    blocks = [b for b in k["blocks"] if b["self_loop"]]
    assert blocks, "no self-looping MFMA block found"
    return blocks


@pytest.mark.slow
@pytest.mark.parametrize("name", list(PLAIN))
def test_k_loop_valu_per_mfma_at_most_break_even(mix, name):
    k = kernel(mix, PLAIN[name])
    assert k["scratch"] == 0, "%s: %d bytes of scratch" % (name, k["scratch"])
    for b in loops(k):
        print("%s %s: %d MFMA, %d VALU" % (name, b["label"], b["mfma"], b["valu"]))
        assert b["valu"] <= 2.0 * b["mfma"], (name, b)


@pytest.mark.slow
@pytest.mark.parametrize("name", list(BN))
def test_bn_forms_not_above_their_earlier_counts(mix, name):
    frag, most = BN[name]
    k = kernel(mix, frag)
    assert k["scratch"] == 0, "%s: %d bytes of scratch" % (name, k["scratch"])
    for b in loops(k):
        print("%s %s: %d MFMA, %d VALU" % (name, b["label"], b["mfma"], b["valu"]))
        assert b["mfma"] == 72 and b["valu"] <= most, (name, b)
