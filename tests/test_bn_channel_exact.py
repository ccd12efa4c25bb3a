"""Exact and float64 tests of the channel BatchNorm kernels (csrc/hip/bn.hip, rag_bn_ch_*), in
the style of test_bn_exact.py, whose helpers and float64 formulas they use.

One statistic per CHANNEL c, reduced over (b, h, w): N = B S S values. The buffers have one slot
per padded channel (CP of them); the first C are real, the padded ones must come out exactly 0
and gamma / beta / the running arrays have only C entries. x and dy are integers in [-3, 3] with
zero padded channels and the backward's mean is a multiple of 1/8, so every per-block fp32 partial
is exact in any order: each block's partial is compared exactly with the sum over that block's
pixels. The finalize is the column form's (double arithmetic on those sums), so the tolerances
are test_bn_exact's: mean, dbeta and the running mean equal to the float64 formula rounded to
fp32; rstd, the coefficients, dgamma and the running variance within 2 fp32 ulps under the same
operand constraints (power-of-two gamma, same-signed terms in the constant coefficients).

bn_ch_apply runs with power-of-two coefficients on integers: its bf16 output is exact, with a zero
halo, zero padded channels (pre-filled with 7.0) and guard boards.
"""
import pytest
import torch

from test_bn_exact import (DEV, EPS, F64, NAN, apply_operands, assert_padded_equal, bn_bwd_ref,
                           bn_fwd_ref, check_backward_finish, check_forward_finish, f32,
                           padded_ref, prefilled_output)
from test_conv_exact import (BF, assert_guards_untouched, gen, guarded_input, guarded_output,
                             ints)

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rocalphago_amd.ops import hipops
    return hipops


def ch_sums(t):
    """[B, S, S, C] (b, h, w, c) -> per channel c."""
    return t.sum((0, 1, 2))


# name: (B, S, C, CP, halo of x, halo of dy)
STAT_CASES = {
    "b3_s5_c24in32": (3, 5, 24, 32, 1, 2),
    "b2_s9_c40in64": (2, 9, 40, 64, 2, 1),      # 24 padded channels
    "b2_s9_c192": (2, 9, 192, 192, 1, 2),       # 24 vectors per pixel: 240 active threads
    "b2_s19_c128": (2, 19, 128, 128, 2, 1),
    # 10469 pixels: capped at 1024 blocks of 11 pixels, more than the 10 pixel lanes of a block
    # at 192 channels, so a thread's walk takes a second trip; the last blocks are empty
    "b29_s19_c192_second_trip": (29, 19, 192, 192, 1, 1),
}


def ch_operands(seed, B, S, C):
    """test_bn_exact.stat_operands with one slot per channel: x, dy integers in [-3, 3]; gamma a
    power of two; |beta|, |mean| dyadic with the signs that keep both constant coefficients free
    of cancellation (sign(beta) = -sign(sum x); sign(mean) = -sign(sum dy * sum dy x))."""
    g = gen(seed)
    x = ints(g, (B, S, S, C), -3, 3)
    dy = ints(g, (B, S, S, C), -3, 3)
    gamma = 2.0 ** ints(g, (C,), -1, 2)
    beta = ints(g, (C,), 1, 8, 0.125)
    beta = torch.where(ch_sums(x) > 0, -beta, beta)
    mean = ints(g, (C,), 1, 8, 0.125)
    mean = torch.where(ch_sums(dy) * ch_sums(dy * x) > 0, -mean, mean)
    rmean = ints(g, (C,), -8, 8, 0.25)
    rvar = ints(g, (C,), 1, 8, 0.25)
    return x, dy, gamma, beta, mean, rmean, rvar


def reduce_geometry(ops, B, S, CP):
    """(blocks, pixels per block) of bn_ch_reduce_kernel: one block per pixel up to 1024 blocks,
    then equal runs of consecutive pixels (b, h, w)."""
    npix = B * S * S
    nblk = min(npix, 1024)
    assert ops._lib().rag_bn_ch_workspace(B, S, CP) == nblk * 2 * CP
    return nblk, (npix + nblk - 1) // nblk


def block_sums(terms, nblk, ppb, CP):
    """float64 [nblk, CP]: the sum of ``terms`` [B, S, S, C] over each block's pixels."""
    B, S, _, C = terms.shape
    want = torch.zeros(nblk, CP, dtype=F64, device=DEV)
    blk = torch.arange(B * S * S, device=DEV) // ppb
    want[:, :C].index_add_(0, blk, terms.reshape(-1, C))
    return want


def assert_partials(part, terms, ppb, what):
    """Every per-block fp32 partial [nblk, CP] exactly: sums of at most 2^24 granules of 1/8."""
    nblk, CP = part.shape
    assert terms.abs().max().item() * ppb * 8 < 2 ** 24
    want = block_sums(terms, nblk, ppb, CP)
    assert torch.equal(part.double(), want), what


def tail_of(values, n=4096):
    """fp32 copy of ``values`` in the last elements of a larger tensor: an index past the C
    entries would read past the tensor."""
    if values is None:
        return None
    buf = torch.full((n,), NAN, device=DEV)
    buf[n - values.numel():] = values.float()
    return buf[n - values.numel():]


def padded(v, CP):
    out = torch.zeros(CP, dtype=v.dtype, device=v.device)
    out[:v.numel()] = v
    return out


def workspace(ops, x, B, S, CP, nblk):
    """The per-block partials the last reduction on ``x``'s device left in its workspace."""
    return ops.bn_ch_workspace(B, S, CP, x.device)[:nblk * 2 * CP].view(nblk, 2, CP).clone()


def run_statistics(ops, name, affine):
    B, S, C, CP, hx, hd = STAT_CASES[name]
    x, dy, gamma, beta, mean, rmean0, rvar0 = ch_operands(
        9500 + list(STAT_CASES).index(name), B, S, C)
    if not affine:
        gamma = beta = rmean0 = rvar0 = None
    N, mom = B * S * S, 0.75
    nblk, ppb = reduce_geometry(ops, B, S, CP)
    if name.endswith("second_trip"):
        assert (nblk, ppb) == (1024, 11) and ppb > 256 // (CP // 8)
    xp, dyp = guarded_input(x, hx, CP), guarded_input(dy, hd, CP)
    # forward
    stats = torch.full((2, CP), NAN, device=DEV)
    coef = torch.full((3, CP), NAN, device=DEV)
    rmean, rvar = tail_of(rmean0), tail_of(rvar0)
    ga, be = tail_of(gamma), tail_of(beta)
    ops.bn_ch_train_fwd(xp, B, S, C, ga, be, rmean, rvar, EPS, mom, stats, coef)
    part = workspace(ops, xp, B, S, CP, nblk)
    assert_partials(part[:, 0], x, ppb, "sum x")
    assert_partials(part[:, 1], x * x, ppb, "sum x^2")
    # determinism: a second run gives bit-identical partials
    stats2, coef2 = torch.empty_like(stats), torch.empty_like(coef)
    ops.bn_ch_train_fwd(xp, B, S, C, ga, be, None, None, EPS, mom, stats2, coef2)
    again = workspace(ops, xp, B, S, CP, nblk)
    assert torch.equal(again.view(torch.int32), part.view(torch.int32))
    assert torch.equal(stats2.view(torch.int32), stats.view(torch.int32))
    assert torch.equal(coef2.view(torch.int32), coef.view(torch.int32))
    ref = bn_fwd_ref(ch_sums(x), ch_sums(x * x), N, gamma, beta, EPS, rmean0, rvar0, mom)
    check_forward_finish((stats[:, :C], coef[:, :C], rmean, rvar), ref, affine)
    # padded channels: statistics and coefficients exactly 0 (no gamma / beta entry exists)
    assert not bool(stats[:, C:].view(torch.int32).any())
    assert not bool(coef[:, C:].view(torch.int32).any())
    # backward, from a hand-made dyadic mean (x - mean stays exact) and the forward's rstd
    bstats = torch.stack([padded(mean.float(), CP), stats[1]]).contiguous()
    dgamma = torch.full((C,), NAN, device=DEV)
    dbeta = torch.full((C,), NAN, device=DEV)
    bcoef = torch.full((3, CP), NAN, device=DEV)
    ops.bn_ch_bwd_coef(xp, dyp, B, S, C, ga, bstats, dgamma, dbeta, bcoef)
    part = workspace(ops, xp, B, S, CP, nblk)
    centred = dy * (x - mean.view(1, 1, 1, C))
    assert_partials(part[:, 0], dy, ppb, "sum dy")
    assert_partials(part[:, 1], centred, ppb, "sum dy (x - mean)")
    ops.bn_ch_bwd_coef(xp, dyp, B, S, C, ga, bstats, None, None, torch.empty_like(bcoef))
    again = workspace(ops, xp, B, S, CP, nblk)
    assert torch.equal(again.view(torch.int32), part.view(torch.int32))
    ref = bn_bwd_ref(ch_sums(dy), ch_sums(centred), N, gamma, bstats[0, :C], bstats[1, :C])
    check_backward_finish((dgamma, dbeta, bcoef[:, :C]), ref)
    assert not bool(bcoef[:, C:].view(torch.int32).any())


@gpu
@pytest.mark.parametrize("name", list(STAT_CASES))
def test_bn_ch_statistics(ops, name):
    """bn_ch_train_fwd and bn_ch_bwd_coef (bn_ch_reduce_kernel<0 / 1>, then the shared
    bn_finalize_kernel with CP slots): every per-block partial exactly, twice (determinism), the
    finish against the float64 formulas with N = B S S, the padded slots exactly zero with
    gamma / beta / running arrays of C entries at the very end of a tensor."""
    run_statistics(ops, name, True)


@gpu
def test_bn_ch_statistics_null_affine(ops):
    """gamma, beta and the running averages null: gamma counts as 1, beta as 0, no running
    average is written."""
    run_statistics(ops, "b2_s9_c40in64", False)


@gpu
@pytest.mark.parametrize("B,S,C,CP", [(3, 5, 24, 32), (2, 9, 40, 64), (2, 9, 192, 192)])
def test_bn_ch_infer_coef(ops, B, S, C, CP):
    """bn_ch_infer_coef runs the column form's finish (bn.hip bn_finish_col<2>) per channel: bit
    for bit the coefficients bn_infer_coef gives for the same arrays taken as columns (at most 64
    at a time), and, as a check of the values, the float64 formula to 1e-6; padded slots 0."""
    g = gen(9600 + C)
    gamma = f32(2.0 ** ints(g, (C,), -1, 2))
    rvar = f32(ints(g, (C,), 1, 8, 0.25))
    rmean = f32(ints(g, (C,), -8, 8, 0.25))
    beta = f32(ints(g, (C,), -8, 8, 0.125))
    coef = torch.full((3, CP), NAN, device=DEV)
    ops.bn_ch_infer_coef(tail_of(gamma), tail_of(beta), tail_of(rmean), tail_of(rvar), EPS, C, CP,
                         coef)
    for a in range(0, C, 64):
        n = min(64, C - a)
        col = torch.full((3, n), NAN, device=DEV)
        ops.bn_infer_coef(gamma[a:a + n].clone(), beta[a:a + n].clone(), rmean[a:a + n].clone(),
                          rvar[a:a + n].clone(), EPS, n, col)
        assert torch.equal(coef[:, a:a + n].contiguous().view(torch.int32), col.view(torch.int32))
    rstd = 1.0 / torch.sqrt(rvar.double() + EPS)
    assert torch.allclose(coef[0, :C].double(), gamma.double() * rstd, rtol=1e-6, atol=0)
    assert torch.allclose(coef[2, :C].double(), beta.double() - rmean.double() * gamma * rstd,
                          rtol=1e-6, atol=1e-6)
    assert not bool(coef[1].view(torch.int32).any())
    assert not bool(coef[:, C:].view(torch.int32).any())


# --------------------------------------------------------------------------- bn_ch_apply

def pow2_coef_ch(C, CP):
    """[3, CP] power-of-two channel coefficients: cx in {0.5, 1, 2}, cd in {0.5, 1},
    cc in {-1, 0, 2} (cc > 0 on channel 0 and C - 1: a halo pixel that wrongly became act(cc)
    would show); the padded slots hold 0, as the finalize leaves them."""
    ch = torch.arange(C, device=DEV)
    cx = torch.tensor([0.5, 1.0, 2.0], device=DEV)[(ch // 3) % 3]
    cd = torch.tensor([1.0, 0.5], device=DEV)[ch % 2]
    cc = torch.tensor([2.0, -1.0, 0.0], device=DEV)[ch % 3]
    cc[-1] = 2.0
    out = torch.zeros(3, CP, device=DEV)
    out[:, :C] = torch.stack([cx, cd, cc])
    return out


def apply_ref_ch(x, coef, relu, dy=None, res=None):
    """bn_ch_apply in float64: act(c0[c] x + c1[c] dy + c2[c] + res) on [B, S, S, C]."""
    C = x.shape[-1]
    c = coef[:, :C].double().view(3, 1, 1, 1, C)
    v = c[0] * x + c[2]
    if dy is not None:
        v = v + c[1] * dy
    if res is not None:
        v = v + res
    return torch.relu(v) if relu else v


@gpu
@pytest.mark.parametrize("halos", [(1, 2, 2, 1), (2, 1, 1, 2), (1, 1, 2, 2)],
                         ids=["h1221", "h2112", "h1122"])
@pytest.mark.parametrize("B,S,C,CP", [(3, 5, 24, 32), (2, 9, 40, 64), (2, 9, 192, 192),
                                      (2, 19, 128, 128)])
def test_bn_ch_apply_forms_exact(ops, B, S, C, CP, halos):
    """bn_ch_apply_kernel with power-of-two coefficients on integers, halos (x, dy, residual,
    out) drawn from {1, 2}: forward BN + ReLU (c0 x + c2); the backward form
    c0 x + c1 dy + c2 + residual without ReLU, also with the residual aliasing the output.
    C = 40 in CP = 64: the padded channels are written as zero."""
    hx, hd, hr, ho = halos
    x, dy, res = apply_operands(9700 + S + C, B, C, S)
    coef = pow2_coef_ch(C, CP)
    xp, dyp, resp = guarded_input(x, hx, CP), guarded_input(dy, hd, CP), guarded_input(res, hr, CP)
    full, out = prefilled_output(B, S, ho, CP)
    ops.bn_ch_apply(xp, out, B, S, C, coef, relu=True)
    assert_padded_equal(out, padded_ref(apply_ref_ch(x, coef, True), CP), ho, "BN + ReLU")
    assert_guards_untouched(full)
    want = padded_ref(apply_ref_ch(x, coef, False, dy=dy, res=res), CP)
    full, out = prefilled_output(B, S, ho, CP)
    ops.bn_ch_apply(xp, out, B, S, C, coef, relu=False, dy=dyp, residual=resp)
    assert_padded_equal(out, want, ho, "backward + residual")
    assert_guards_untouched(full)
    # in place: the residual is the output buffer (its padded channels hold zero)
    full, out = guarded_output(B, S, ho, CP)
    out[:, ho:ho + S, ho:ho + S, :C] = res.to(BF)
    ops.bn_ch_apply(xp, out, B, S, C, coef, relu=False, dy=dyp, residual=out)
    assert_padded_equal(out, want, ho, "backward + residual in place")
    assert_guards_untouched(full)


@gpu
def test_bn_ch_rejects_bad_shapes(ops):
    """The launchers refuse (no launch) a channel count above the padded one, a padded count
    that is no multiple of 8, and the wrappers a coefficient buffer without CP slots."""
    x = torch.zeros(1, 7, 7, 32, dtype=BF, device=DEV)
    coef = torch.zeros(3, 32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.bn_ch_apply(x, torch.zeros_like(x), 1, 5, 40, coef)
    with pytest.raises(ValueError):
        ops.bn_ch_apply(x, torch.zeros_like(x), 1, 5, 24, coef[:, :24].contiguous())
    with pytest.raises(ValueError):
        ops.bn_ch_train_fwd(x, 1, 5, 24, None, None, None, None, EPS, 0.9,
                            torch.zeros(2, 5, device=DEV), coef)
    x12 = torch.zeros(1, 7, 7, 12, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):
        ops.bn_ch_train_fwd(x12, 1, 5, 12, None, None, None, None, EPS, 0.9,
                            torch.zeros(2, 12, device=DEV), torch.zeros(3, 12, device=DEV))
