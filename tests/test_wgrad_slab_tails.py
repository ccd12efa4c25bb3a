"""Pipeline edges of the slab weight gradient's pair loop (wgrad_slab.hip): a block works through
its chunk of 64-row stages in pairs, one barrier per pair, so the batches here are the smallest
that give a block fewer stages than a pair, exactly one pair, a pair plus an odd tail, two pairs
plus one, and a last chunk that is shorter than the others. Each case runs the bit-exact
integer-operand check of test_conv_exact.run_wgrad_slab (overwrite, accumulate, deferred): a
phantom sub-stage that contributed anything, or rows counted twice, changes dW or db.

The stages per block are asserted from the library's own chunking (rag_wgrad_slab_chunks), so a
change of chunking cannot silently move the cases off the edges."""
import ctypes

import pytest

from test_conv_exact import ops, run_wgrad_slab  # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu


def stages_per_block(lib, B, S, ks, cinp, pair5):
    """(stages of every chunk but the last, stages of the last chunk)."""
    wp = S + 2 * (ks // 2)
    R = B * wp * wp
    spc = ctypes.c_int(0)
    n = lib.rag_wgrad_slab_chunks(R, cinp, ks, pair5, ctypes.byref(spc))
    steps = (R + 63) // 64
    assert n >= 1 and (n - 1) * spc.value < steps <= n * spc.value
    return spc.value, steps - (n - 1) * spc.value


# 3x3 192 -> 192 on both wave -> tile maps: (B, stages per block, stages of the last chunk)
CASES_192 = [(1, 1, 1),    # fewer stages than a pair: the prologue and a half pair only
             (12, 2, 1),   # exactly one pair; a lone sub-stage in the last chunk
             (23, 4, 3),   # two pairs; pair + odd tail in the last chunk
             (29, 5, 5)]   # two pairs + one everywhere


@pytest.mark.parametrize("wmap", [0, 1])
@pytest.mark.parametrize("B,per,last", CASES_192)
def test_wgrad_slab_tails_192(ops, B, per, last, wmap):
    lib = ops._lib()
    assert stages_per_block(lib, B, 19, 3, 192, 0) == (per, last)
    prev = lib.rag_wgrad_slab_map(wmap)
    try:
        run_wgrad_slab(ops, 19, 3, 192, 192, 192, B, seed=5000 + 2 * B + wmap)
    finally:
        lib.rag_wgrad_slab_map(prev)


# 3x3 128 -> 128 (8 waves, map 0). Its four c-tiles give 64 chunks, so B = 23 is three stages in
# every block (pair + half pair); B = 30 adds the short last chunk (4, last 3).
@pytest.mark.parametrize("B,per,last", [(23, 3, 3), (30, 4, 3)])
def test_wgrad_slab_tails_128(ops, B, per, last):
    assert stages_per_block(ops._lib(), B, 19, 3, 128, 0) == (per, last)
    run_wgrad_slab(ops, 19, 3, 128, 128, 128, B, seed=5100 + B)


# 5x5 48 -> 192: one kernel row per block, c-tile 1 row-paired (pair5)
@pytest.mark.parametrize("B,per,last", [(9, 3, 3), (23, 6, 5)])
def test_wgrad_slab_tails_5x5_pair5(ops, B, per, last):
    assert stages_per_block(ops._lib(), B, 19, 5, 64, 1) == (per, last)
    run_wgrad_slab(ops, 19, 5, 48, 64, 192, B, seed=5200 + B)
