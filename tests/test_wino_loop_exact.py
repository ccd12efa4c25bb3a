"""Bit-exact tests of every form of the Winograd kernel's K loop (csrc/hip/conv_wino.hip: the
per-block geometry of wino_geom, the fused phase-1 load pair, one transform unit per half-board
thread), with the integer operands of tests/test_conv_exact.py (GPU only).

Activations and gradients are integers in [-2, 2], weights even integers in [-4, 4], so every
product and partial sum is exact in fp32 in any order and a kernel must reproduce the float64 tap
loop (test_conv_exact.tap_conv, never a launch of the code under test) BIT FOR BIT. Every case
checks the forward (bias + ReLU) and, except the chains and the multi-board form, the dgrad (ReLU
mask at halo 1, output halo 2): every output bit, an exactly zero halo, untouched guard boards
around the output and a NaN board behind every input.

  half-board blocks    conv_wino_kernel<192,1,96>: B = 2, S = 19 and S = 14 (the smallest board
                       with more than 96 pairs: its odd block holds two real pairs), K loops of
                       one (32 -> 192: the phase-1 loop runs zero times), two and six chunks
  one-board 192        conv_wino_chain_kernel<192,1> (any_batch) at B = 3, S = 19 and the even
                       S = 18, L = 1 and 3 against the float64 reference of the composed layers;
                       conv_wino_kernel<192,1,192> at the smallest batch the selector gives it
  128-wide             conv_wino_kernel<128,1>: B = 2, S = 19, 32 / 64 / 128 -> 128;
                       conv_wino_chain_kernel<128,1>: L = 3 at B = 3
  BN forms (128-wide)  conv_wino_kernel<128,1,192,1> / <..,2> at B = 2, S = 19 (the forward with a
                       residual rounds twice, docs/KERNELS.md "Exact-arithmetic tests": held to one
                       ulp of the float64 reference and bit for bit to the two roundings)
  multi-board          conv_wino_kernel<192,0>: (B, S, C) = (5, 9, 192), forward

A chain's later layers read the layers before them, not small integers, and the Winograd
transform rounds V = d_a +- d_b to bf16: it is exact only while |d_a| + |d_b| <= 256. Their
operands keep the argument intact: biases are integers, so every activation is an integer; in a
chain of several layers the first layer's weights are sparse (one in 128 non-zero) and every
later layer's weights hold one +-2 per output channel (at a random input channel and tap), so
that every activation that feeds a layer stays at most 128 -- asserted per layer on the
reference's side, with the bound on the sum of |x| |w| of any output (below 2^24: every partial
sum exact in fp32). A later layer's output then depends on one input element each: a wrong V
row, tap, chunk or ring buffer still shows, a dropped term of a long sum is the first layer's
and the single launches' business.
"""
import pytest
import torch

from test_conv_exact import (BF, DEV, NAN, assert_bits_equal, assert_column_stats,
                             assert_guards_untouched, assert_partial_sums_exact, dgrad_weights,
                             direct_operands, gen, guarded_input, guarded_output, ints, ops,
                             round_bf16_nchw, tap_conv)  # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu


def run_layer(ops, B, S, kin, nout, seed, half=False, dgrad=True):
    """One kin -> nout layer through ops.conv_wino: the forward, and the dgrad form of the same
    shape (the input gradient of a nout -> kin layer: kin gradient channels in, nout out)."""
    assert ops.conv_wino_ok(S, 1, kin, nout, 3)
    x, w, bias, _, _, _ = direct_operands(seed, S, 3, kin, nout, B, None, wstep=2)
    assert w.abs().max().item() == 4 and bool((w % 2 == 0).all())
    uf, _ = ops.wino_weights(w.float().contiguous(), nout, kin, dgrad=False)
    ref = round_bf16_nchw(torch.relu(tap_conv(x, w) + bias))
    full, y = guarded_output(B, S, 1, nout)
    ops.conv_wino(guarded_input(x, 1, kin), uf, bias.float().contiguous(), y, B, S, kin, nout, 1,
                  True, half=half)
    assert_bits_equal(y, ref, 1, "fwd %d -> %d" % (kin, nout))
    assert_guards_untouched(full)
    if not dgrad:
        return
    xin, wl, _, _, grad, _ = direct_operands(seed + 1, S, 3, nout, kin, B, None, wstep=2)
    _, ub = ops.wino_weights(wl.float().contiguous(), kin, nout)
    xm = torch.relu(xin)
    dx = tap_conv(grad, dgrad_weights(wl))
    ref = round_bf16_nchw(torch.where(xm > 0, dx, torch.zeros_like(dx)))
    full, y = guarded_output(B, S, 2, nout)
    ops.conv_wino(guarded_input(grad, 1, kin), ub, None, y, B, S, kin, nout, 2, False,
                  mask=guarded_input(xm, 1, nout), mask_halo=1, half=half)
    assert_bits_equal(y, ref, 2, "dgrad %d -> %d" % (kin, nout))
    assert_guards_untouched(full)


@pytest.mark.parametrize("kin", [32, 64, 192])
@pytest.mark.parametrize("S", [19, 14])
def test_half_board_blocks_bit_exact(ops, S, kin):
    """Both blocks of each board: the odd block's last rows and its pad pairs included."""
    run_layer(ops, 2, S, kin, 192, seed=5000 + S + kin, half=True)


@pytest.mark.parametrize("kin", [32, 64, 128])
def test_128_wide_bit_exact(ops, kin):
    run_layer(ops, 2, 19, kin, 128, seed=5100 + kin)


def test_one_board_192_single_launch_bit_exact(ops):
    """The smallest batch that conv_wino gives to one-board blocks of the 192-wide tile (below
    it, half-board blocks fill the chip better)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = cus // 2 + 1
    assert ops.conv_wino_mode(B, 19, 192, 192) == 1
    run_layer(ops, B, 19, 192, 192, seed=5200)


def test_multi_board_blocks_forward_bit_exact(ops):
    """Four 9x9 boards per block, the last block ragged."""
    run_layer(ops, 5, 9, 192, 192, seed=5300, dgrad=False)


# ------------------------------------------------------------------------------- chains

def chain_operands(seed, B, S, C, L, device=DEV):
    """(x, [(w, bias)] * L) as float64 tensors on ``device`` from a seeded CPU generator: x
    integers in [-2, 2], integer biases in [-2, 2], first-layer weights even integers in [-4, 4]
    (dense for L = 1, one in 128 non-zero otherwise), later layers one +-2 per output channel."""
    g = gen(seed)

    def draw(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8).to(device).double()

    x = draw((B, S, S, C), -2, 2)
    layers = []
    for l in range(L):
        if l == 0:
            w = draw((C, C, 3, 3), -2, 2) * 2.0
            if L > 1:
                w = w * (torch.rand((C, C, 3, 3), generator=g) < 1.0 / 128).to(device)
        else:
            w = torch.zeros(C, C * 9, dtype=torch.float64)
            pick = torch.randint(0, C * 9, (C,), generator=g)
            w[torch.arange(C), pick] = torch.randint(0, 2, (C,), generator=g).double() * 4 - 2
            w = w.view(C, C, 3, 3).to(device)
        layers.append((w, draw((C,), -2, 2)))
    return x, layers


def chain_reference(x, layers):
    """The composed layers in float64, each output rounded to bf16 as it is stored (NHWC, one
    tensor per layer), after the exactness preconditions (properties of the operands): integer
    inputs of at most 128 (V = d_a +- d_b exact in bf16) and the largest sum of |x| |w|
    (+ |bias|) of any output below 2^24."""
    outs = []
    for w, bias in layers:
        assert bool((x == x.round()).all()) and x.abs().max().item() <= 128
        bound = (tap_conv(x.abs(), w.abs()) + bias.abs()).max().item()
        assert bound < 2 ** 24, bound
        x = torch.relu(tap_conv(x, w) + bias).float().to(torch.bfloat16).double()
        outs.append(x)
    return outs


@pytest.mark.parametrize("S,C,L", [(19, 192, 1), (19, 192, 3), (18, 192, 1), (18, 192, 3),
                                   (19, 128, 3)])
def test_chain_bit_exact(ops, S, C, L):
    B = 3
    x, layers = chain_operands(6000 + S + C + L, B, S, C, L)
    refs = chain_reference(x, layers)
    assert all(float((r != 0).double().mean()) > 0.25 for r in refs)  # (not a dead comparison)
    us = [ops.wino_weights(w.float().contiguous(), C, C, dgrad=False)[0] for w, _ in layers]
    # every later activation is an output and an input: 7.0 before the batch, NaN behind it
    acts = [guarded_input(x, 1, C)]
    fulls = []
    for _ in range(L):
        full, y = guarded_output(B, S, 1, C)
        full[-1] = NAN
        fulls.append(full)
        acts.append(y)
    ops.conv_wino_chain([(acts[l], us[l], layers[l][1].float().contiguous(), acts[l + 1], True)
                         for l in range(L)], B, S, any_batch=True)
    for l in range(L):
        assert_bits_equal(acts[l + 1], refs[l].permute(0, 3, 1, 2).to(BF).contiguous(), 1,
                          "chain layer %d of %d" % (l + 1, L))
        assert bool((fulls[l][0] == 7.0).all()), "the board before the batch was written"
        assert bool(torch.isnan(fulls[l][-1]).all()), "the board after the batch was written"


# ------------------------------------------------------------------- fused BatchNorm forms

def test_bn_forms_bit_exact(ops):
    """conv_wino_bn at B = 2 (one board per block at any batch whose grid fits the chip), the
    operands of test_conv_exact.test_bn_fused_forms_bit_exact: power-of-two column coefficients,
    U = ReLU(cx x + cc) exact in bf16, cc > 0 on the first and last column."""
    B, S, C = 2, 19, 128
    assert ops.conv_wino_bn_ok(B, S, C, C)
    x, w, bias, res, grad, _ = direct_operands(5400, S, 3, C, C, B, None, wstep=2)
    col = torch.arange(S, device=DEV)
    cx = torch.tensor([0.5, 1.0, 2.0], device=DEV)[(col // 3) % 3]
    cc = torch.tensor([2.0, -1.0, 0.0], device=DEV)[col % 3]
    assert cc[0] > 0 and cc[-1] > 0
    coef = torch.zeros(3, S, device=DEV)
    coef[0], coef[2] = cx, cc
    pre = x * cx.double().view(1, 1, S, 1) + cc.double().view(1, 1, S, 1)
    U = torch.relu(pre)  # multiples of 0.5 up to 6
    assert_partial_sums_exact(3, C, 6, 4)
    b32 = bias.float().contiguous()
    wfwd, wbwd = ops.wino_weights(w.float().contiguous(), C, C)
    blk = torch.arange(B, device=DEV).view(B, 1, 1).expand(B, S, S)
    conv = tap_conv(U, w)
    # forward: bias + residual (two roundings), statistics of the stored output
    full, y = guarded_output(B, S, 1, C)
    part = torch.full((B, 2, S), 7.0, device=DEV)
    ops.conv_wino_bn(guarded_input(x, 1, C), wfwd, b32, y, B, S, C, C, False, bn_coef=coef,
                     residual=guarded_input(res, 1, C), stat_part=part)
    assert_bits_equal(y, round_bf16_nchw(conv + bias + res), 1, "wino_bn fwd + residual",
                      one_ulp_store=True)
    twice = (conv + bias).float().to(BF).double() + res
    assert_bits_equal(y, round_bf16_nchw(twice), 1, "wino_bn fwd + residual, two roundings")
    assert_guards_untouched(full)
    stored = y[:, 1:-1, 1:-1, :].double()
    assert assert_column_stats(part[:, 0], stored, blk, 0.25, "sum y")
    assert_column_stats(part[:, 1], stored * stored, blk, 1.0 / 16, "sum y^2")
    # forward: bias + ReLU, no residual
    full, y = guarded_output(B, S, 1, C)
    ops.conv_wino_bn(guarded_input(x, 1, C), wfwd, b32, y, B, S, C, C, True, bn_coef=coef)
    assert_bits_equal(y, round_bf16_nchw(torch.relu(conv + bias)), 1, "wino_bn fwd + relu")
    assert_guards_untouched(full)
    # dgrad: the mask U > 0 recomputed from x, statistics sum dU and sum dU (x - mean)
    dx = tap_conv(grad, dgrad_weights(w))
    ref = round_bf16_nchw(torch.where(pre > 0, dx, torch.zeros_like(dx)))
    mean = ints(gen(5401), (S,), -2, 2, 0.5).float()
    full, y = guarded_output(B, S, 1, C)
    part = torch.full((B, 2, S), 7.0, device=DEV)
    ops.conv_wino_bn(guarded_input(grad, 1, C), wbwd, None, y, B, S, C, C, False,
                     mask=guarded_input(x, 1, C), mask_coef=coef, stat_part=part, stat_mean=mean)
    assert_bits_equal(y, ref, 1, "wino_bn dgrad")
    assert_guards_untouched(full)
    stored = y[:, 1:-1, 1:-1, :].double()
    assert assert_column_stats(part[:, 0], stored, blk, 1.0, "sum dU")
    assert assert_column_stats(part[:, 1], stored * (x - mean.double().view(1, 1, S, 1)), blk,
                               0.5, "sum dU (x - mean)")
