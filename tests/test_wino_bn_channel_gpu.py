"""The channel-BatchNorm forward form of the Winograd kernel (csrc/hip/conv_wino.hip BNM 3,
ops.conv_wino_bn(bn_axis=1)) and its finalize (ops.bn_ch_finalize_fwd), GPU only.

  bit-exact     the integer operands of tests/test_wino_loop_exact.py::test_bn_forms_bit_exact
                with per-CHANNEL power-of-two coefficients (cx in {0.5, 1, 2}, cc in {2, -1, 0},
                mixed inside every 8-channel slice and every 32-channel chunk; cc > 0 on a third
                of the channels, so a halo pixel that became ReLU(cc) instead of 0 changes the
                border outputs): every output bit against the float64 tap loop, an exactly zero
                halo, untouched guard boards, and the per-board channel statistics against float64
                sums of the stored output; S = 19, and the even S = 14 whose last transform unit
                of a row addresses d3 differently
  determinism   two launches into differently pre-filled buffers: equal bits (the statistics are
                reduced in a fixed order, no float atomics)
  fp32 PyTorch  random operands at B = 3 with test_resnet_gpu.test_wino_bn_kernels_match_torch's
                bounds
  finalize      bn_ch_finalize_fwd on those partials against bn_ch_train_fwd on the stored output
"""
import pytest
import torch
import torch.nn.functional as F

from test_conv_exact import (BF, DEV, assert_bits_equal, assert_guards_untouched,
                             assert_partial_sums_exact, direct_operands, guarded_input,
                             guarded_output, ops, round_bf16_nchw, tap_conv)  # noqa: F401
from test_resnet_gpu import bfr

pytestmark = pytest.mark.gpu

C = 128


def assert_channel_stats(part, terms, granule, what):
    """Per-board fp32 channel partials ``part`` [B, C] against the float64 sums of ``terms``
    [B, S, S, C] (multiples of ``granule``) over each board's pixels: the channel twin of
    test_conv_exact.assert_column_stats (one block per board). If the largest per-(board,
    channel) sum of |terms| is below 2^24 granules every fp32 partial is exact in any order and
    the comparison is exact; otherwise it is relative 1e-6. Returns which one applied."""
    want = terms.sum((1, 2))
    mag = terms.abs().sum((1, 2)).max().item() / granule
    exact = mag < 2 ** 24
    print("%s: %s comparison (largest board partial bound %.3g granules)"
          % (what, "exact" if exact else "relative 1e-6", mag))
    got = part.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    if exact:
        assert torch.equal(got, want), what
    else:
        assert torch.allclose(got, want, rtol=1e-6, atol=0), what
    return exact


def channel_coef():
    """Power-of-two coefficients per channel, all three values of each inside every 8-channel
    slice; coef [3, C] (row 1, the dy multiplier, is unused by the forward and left non-zero)."""
    c = torch.arange(C, device=DEV)
    cx = torch.tensor([0.5, 1.0, 2.0], device=DEV)[(c // 3) % 3]
    cc = torch.tensor([2.0, -1.0, 0.0], device=DEV)[c % 3]
    for k in range(0, C, 8):
        assert len(set(cx[k:k + 8].tolist())) == 3 and len(set(cc[k:k + 8].tolist())) == 3
    assert int((cc > 0).sum()) >= C // 3
    coef = torch.full((3, C), 3.0, device=DEV)
    coef[0], coef[2] = cx, cc
    return cx, cc, coef


@pytest.mark.parametrize("S", [19, 14])
def test_channel_form_bit_exact(ops, S):
    """B = 2 (one board per block). U = ReLU(cx x + cc) holds multiples of 0.5 up to 6, zero
    outside the board: the reference pads U, not x, so a kernel that applied the affine to a
    halo pixel (x = 0 there) would add ReLU(cc) = 2 on a third of the channels to the border
    outputs. conv_wino_bn_ok(2, 14, 128, 128) holds on the device (98 pairs: one board per
    block), so the even board runs the same checks."""
    B = 2
    assert ops.conv_wino_bn_ok(B, S, C, C)
    x, w, bias, res, _, _ = direct_operands(5400 + S, S, 3, C, C, B, None, wstep=2)
    cx, cc, coef = channel_coef()
    U = torch.relu(x * cx.double() + cc.double())
    assert U.max().item() <= 6 and bool(((U * 2) == (U * 2).round()).all())
    assert_partial_sums_exact(3, C, 6, 4)
    b32 = bias.float().contiguous()
    wfwd, _ = ops.wino_weights(w.float().contiguous(), C, C, dgrad=False)
    conv = tap_conv(U, w)
    # (not a dead comparison: a halo of ReLU(cc) around U changes the reference's border)
    halo = torch.relu(cc.double()).expand(B, S + 2, S + 2, C).clone()
    halo[:, 1:-1, 1:-1] = U
    assert not torch.equal(tap_conv_padded(halo, w)[:, 0], conv[:, 0])
    # forward: bias + residual (two roundings), statistics of the stored output
    full, y = guarded_output(B, S, 1, C)
    part = torch.full((B + 1, 2, C), 7.0, device=DEV)
    ops.conv_wino_bn(guarded_input(x, 1, C), wfwd, b32, y, B, S, C, C, False, bn_coef=coef,
                     residual=guarded_input(res, 1, C), stat_part=part, bn_axis=1)
    twice = (conv + bias).float().to(BF).double() + res
    assert_bits_equal(y, round_bf16_nchw(twice), 1, "channel wino_bn fwd + residual")
    assert_guards_untouched(full)
    assert bool((part[B] == 7.0).all()), "a partial row past the batch was written"
    stored = y[:, 1:-1, 1:-1, :].double()
    assert assert_channel_stats(part[:B, 0], stored, 0.25, "sum y")
    assert_channel_stats(part[:B, 1], stored * stored, 1.0 / 16, "sum y^2")
    # forward: bias + ReLU, no residual, no statistics
    full, y = guarded_output(B, S, 1, C)
    ops.conv_wino_bn(guarded_input(x, 1, C), wfwd, b32, y, B, S, C, C, True, bn_coef=coef,
                     bn_axis=1)
    assert_bits_equal(y, round_bf16_nchw(torch.relu(conv + bias)), 1, "channel wino_bn fwd + relu")
    assert_guards_untouched(full)


def tap_conv_padded(up, w):
    """tap_conv of an already padded input [B, S + 2, S + 2, cin] (its border is used as is)."""
    B, WI, _, cin = up.shape
    S = WI - 2
    out = torch.zeros(B * S * S, w.shape[0], dtype=torch.float64, device=up.device)
    for ky in range(3):
        for kx in range(3):
            out += up[:, ky:ky + S, kx:kx + S, :].reshape(-1, cin) @ w[:, :, ky, kx].t()
    return out.view(B, S, S, w.shape[0])


def test_channel_form_is_deterministic(ops):
    """The same launch twice, outputs and partials pre-filled with different junk."""
    B, S = 2, 19
    x, w, bias, res, _, _ = direct_operands(5500, S, 3, C, C, B, None, wstep=2)
    _, _, coef = channel_coef()
    coef[0] = torch.rand(C, generator=torch.Generator().manual_seed(1)).to(DEV) + 0.5
    coef[2] = torch.randn(C, generator=torch.Generator().manual_seed(2)).to(DEV) * 0.3
    wfwd, _ = ops.wino_weights((w * 0.01).float().contiguous(), C, C, dgrad=False)
    xin, rin = guarded_input(x * 0.37, 1, C), guarded_input(res * 0.21, 1, C)
    b32 = bias.float().contiguous()
    outs = []
    for junk in (7.0, -3.0e5):
        y = ops.alloc_padded(B, S, 1, C, DEV)
        y[:, 1:-1, 1:-1] = junk
        part = torch.full((B, 2, C), junk, device=DEV)
        ops.conv_wino_bn(xin, wfwd, b32, y, B, S, C, C, False, bn_coef=coef, residual=rin,
                         stat_part=part, bn_axis=1)
        outs.append((y, part))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    assert bool(torch.isfinite(outs[0][1]).all()) and float(outs[0][1][:, 1].min()) > 0


@pytest.fixture(scope="module")
def torch_case(ops):
    """One launch at B = 3 on random operands, shared by the fp32 comparison and the finalize."""
    torch.manual_seed(23)
    B, S = 3, 19
    assert ops.conv_wino_bn_ok(B, S, C, C)
    x = bfr(torch.randn(B, C, S, S, device=DEV) * 1.5)
    coef = torch.zeros(3, C, device=DEV)
    coef[0] = torch.rand(C, device=DEV) + 0.5
    coef[2] = torch.randn(C, device=DEV) * 0.3
    U = F.relu(x * coef[0].view(1, C, 1, 1) + coef[2].view(1, C, 1, 1))
    w = torch.randn(C, C, 3, 3, device=DEV) * 0.05
    b = torch.randn(C, device=DEV) * 0.1
    r = bfr(torch.randn(B, C, S, S, device=DEV))
    xp, rp = ops.pack_nchw(x, 1, C), ops.pack_nchw(r, 1, C)
    uf, _ = ops.wino_weights(w, C, C, dgrad=False)
    y = ops.alloc_padded(B, S, 1, C, DEV)
    part = torch.full((B, 2, C), 7.0, device=DEV)
    ops.conv_wino_bn(xp, uf, b, y, B, S, C, C, False, bn_coef=coef, residual=rp, stat_part=part,
                     bn_axis=1)
    ref = F.conv2d(U, w, b, padding=1) + r
    return B, S, y, part, ref


def test_channel_form_matches_torch(ops, torch_case):
    B, S, y, part, ref = torch_case
    got = ops.unpack(y, C, 1)
    e_max, e_norm = (got - ref).abs().max().item(), (got - ref).norm().item()
    print("max error %.4g of max |ref| %.4g; error norm %.4g of %.4g"
          % (e_max, ref.abs().max().item(), e_norm, ref.norm().item()))
    assert e_max < 2e-2 * ref.abs().max().item()
    assert e_norm < 6e-3 * ref.norm().item()
    sums = part.double().sum(0)
    assert torch.allclose(sums[0], got.double().sum((0, 2, 3)), rtol=1e-4, atol=1e-1)
    assert torch.allclose(sums[1], (got.double() ** 2).sum((0, 2, 3)), rtol=1e-4, atol=1e-1)
    border = y.clone()
    border[:, 1:-1, 1:-1] = 0
    assert not bool(border.view(torch.int16).any()), "the output halo is not zero"


def test_channel_finalize_matches_train_fwd(ops, torch_case):
    """bn_ch_finalize_fwd on the conv's per-board partials against bn_ch_train_fwd's own
    statistics pass over the stored output: both sum fp32 partials in double and differ only in
    how the fp32 partials group the pixels."""
    B, S, y, part, _ = torch_case
    g = torch.Generator().manual_seed(5)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    rm0 = (torch.randn(C, generator=g) * 0.1).to(DEV)
    rv0 = (torch.rand(C, generator=g) + 0.5).to(DEV)
    eps, mom = 1e-3, 0.9
    out = []
    for fused in (False, True):
        stats, coef = torch.zeros(2, C, device=DEV), torch.zeros(3, C, device=DEV)
        rmean, rvar = rm0.clone(), rv0.clone()
        if fused:
            ops.bn_ch_finalize_fwd(part, B, B, S, C, gamma, beta, rmean, rvar, eps, mom, stats,
                                   coef)
        else:
            ops.bn_ch_train_fwd(y, B, S, C, gamma, beta, rmean, rvar, eps, mom, stats, coef)
        out.append((stats, coef, rmean, rvar))
    torch.cuda.synchronize()
    assert not torch.equal(out[0][2], rm0) and not torch.equal(out[0][3], rv0)
    for name, a, b in zip(("stats", "coef", "running mean", "running variance"), out[0], out[1]):
        rel = ((a - b).abs() / a.abs().clamp_min(1e-30)).max().item()
        print("%s: largest relative difference %.3g, absolute %.3g"
              % (name, rel, (a - b).abs().max().item()))
    for name, a, b in zip(("stats", "coef", "running mean", "running variance"), out[0], out[1]):
        assert torch.allclose(b, a, rtol=1e-5), name
