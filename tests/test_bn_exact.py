"""Exact and float64 tests of the stand-alone column BatchNorm kernels (csrc/hip/bn.hip), in the
style of test_conv_exact.py.

One statistic per board COLUMN w, reduced over (b, h, c): N = B S C values (the real channels,
not the padded CP). x and dy are integers in [-3, 3] with zero padded channels, the backward's
mean is a multiple of 1/8, so every per-block fp32 partial (sum x, sum x^2, sum dy,
sum dy (x - mean)) is exact in any order: the partials are compared exactly (the helper of
test_conv_exact asserts the 2^24-granule bound itself). The finalize is double arithmetic on
those sums; against the float64 formulas of the file header (bn.hip:42-90)

* mean, dbeta and the running mean (of the stored fp32 mean, with a dyadic momentum) are
  equal to the formula rounded to fp32;
* rstd, the three coefficients, dgamma and the running variance are within 2 fp32 ulps: the
  kernel rounds mean, rstd, dgamma and k1 to fp32 before it combines them in fp32. So that
  2 ulps is a bound and not luck, gamma is a power of two (products with it are exact) and
  the two terms of the constant coefficient have the same sign (beta's sign in the forward,
  the mean's in the backward, are chosen from the operands' sums): no cancellation.

bn_apply runs with power-of-two coefficients on integers: its bf16 output is exact and compared
in value, with a zero halo, zero padded channels (pre-filled with 7.0) and guard boards.
bn_apply_bwd_part must equal bn_finalize_bwd + bn_apply bit for bit, and the float64 formula
where N is a power of two (all coefficients exact), else within one bf16 ulp.

The float64 formulas are tested on the CPU (not marked gpu) against autograd of
test_resnet_gpu.col_bn_ref.
"""
import numpy as np
import pytest
import torch

from test_conv_exact import (BF, DEV, NAN, assert_column_stats, assert_guards_untouched, gen,
                             guarded_input, guarded_output, ints, round_bf16_nchw)

gpu = pytest.mark.gpu
F64 = torch.float64
EPS = float(np.float32(1e-3))  # as the kernel receives it


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rocalphago_amd.ops import hipops
    return hipops


def _ints(g, shape, lo, hi, step=1.0, dev=DEV):
    """test_conv_exact.ints on ``dev``: the CPU self-checks draw the same values."""
    if dev == DEV:
        return ints(g, shape, lo, hi, step)
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8).double() * step


# ------------------------------------------------------------------- float64 references

def bn_fwd_ref(s0, s1, N, gamma, beta, eps, rmean=None, rvar=None, momentum=None):
    """The training forward's column finish (bn.hip:60-72) in float64 from the column sums
    s0 = sum x, s1 = sum x^2 over N values: mean, var, rstd, the coefficients of
    y = c0 x + c2 (c1, dy's, is zero) and the running averages (the mean's from the mean as
    stored in fp32)."""
    S = s0.numel()
    ga = torch.ones(S, dtype=F64, device=s0.device) if gamma is None else gamma.double()
    be = torch.zeros(S, dtype=F64, device=s0.device) if beta is None else beta.double()
    mean = s0 / N
    var = (s1 / N - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    out = dict(mean=mean, var=var, rstd=rstd,
               coef=torch.stack([ga * rstd, torch.zeros_like(mean), be - mean * ga * rstd]))
    if rmean is not None:
        out["rmean"] = momentum * rmean.double() + (1 - momentum) * mean.float().double()
        out["rvar"] = momentum * rvar.double() + (1 - momentum) * var
    return out


def bn_bwd_ref(s0, s1, N, gamma, mean, rstd):
    """The backward's column finish (bn.hip:78-89) in float64 from s0 = sum dy,
    s1 = sum dy (x - mean) and the stored mean / rstd: dbeta, dgamma and the coefficients of
    dx = c0 x + c1 dy + c2 = ga rstd dy - k1 (dbeta + xhat dgamma), k1 = ga rstd / N,
    xhat = (x - mean) rstd."""
    ga = torch.ones_like(s0) if gamma is None else gamma.double()
    mean, rstd = mean.double(), rstd.double()
    dg = s1 * rstd
    k1 = ga * rstd / N
    cx = -k1 * dg * rstd
    return dict(dbeta=s0, dgamma=dg, coef=torch.stack([cx, ga * rstd, -k1 * s0 - cx * mean]))


def col_sums(t):
    """[B, S, S, C] (b, h, w, c) -> per column w."""
    return t.sum((0, 1, 3))


def ulp32(ref):
    """The fp32 spacing at |ref| (float64 tensor)."""
    a = ref.float().abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def assert_ulps(got, ref, ulps, what):
    """fp32 ``got`` against the float64 ``ref``: equal to ref rounded to fp32 (ulps = 0) or
    within ``ulps`` fp32 ulps of it. Prints the figure."""
    assert got.dtype == torch.float32 and got.shape == ref.shape, what
    assert not bool(torch.isnan(got).any()), what
    if ulps == 0:
        assert torch.equal(got, ref.float()), (what, got.tolist(), ref.tolist())
        return
    err = ((got.double() - ref).abs() / ulp32(ref)).max().item()
    print("%s: %.2f ulps" % (what, err))
    assert err <= ulps, (what, err)


def apply_ref(x, coef=None, relu=True, dy=None, res=None):
    """bn_apply in float64: act(c0[w] x + c1[w] dy + c2[w] + res) on [B, S, S, C]."""
    S = x.shape[2]
    v = x.clone()
    if coef is not None:
        c = coef.double().view(3, 1, 1, S, 1)
        v = c[0] * x + c[2]
        if dy is not None:
            v = v + c[1] * dy
    if res is not None:
        v = v + res
    return torch.relu(v) if relu else v


# -------------------------------------------------------------- CPU self-checks (no GPU)

def stat_operands(seed, B, C, S, dev=DEV):
    """x, dy integers in [-3, 3]; gamma a power of two; |beta|, |mean| dyadic; the signs of beta
    and of the backward's mean chosen so that neither constant coefficient cancels:
    c2 = beta - mean_x ga rstd wants sign(beta) = -sign(sum x); the backward's
    c2 = -k1 (db - dg rstd mean) with dg rstd = (A - mean db) rstd^2, A = sum dy x, wants
    sign(mean) = -sign(db A)."""
    g = gen(seed)
    x = _ints(g, (B, S, S, C), -3, 3, dev=dev)
    dy = _ints(g, (B, S, S, C), -3, 3, dev=dev)
    gamma = 2.0 ** _ints(g, (S,), -1, 2, dev=dev)
    beta = _ints(g, (S,), 1, 8, 0.125, dev=dev)
    beta = torch.where(col_sums(x) > 0, -beta, beta)
    mean = _ints(g, (S,), 1, 8, 0.125, dev=dev)
    mean = torch.where(col_sums(dy) * col_sums(dy * x) > 0, -mean, mean)
    rmean = _ints(g, (S,), -8, 8, 0.25, dev=dev)
    rvar = _ints(g, (S,), 1, 8, 0.25, dev=dev)
    return x, dy, gamma, beta, mean, rmean, rvar


@pytest.mark.parametrize("B,C,S", [(2, 3, 5), (3, 4, 7)])
def test_bn_reference_matches_autograd(B, C, S):
    """bn_fwd_ref / bn_bwd_ref against test_resnet_gpu.col_bn_ref (Keras-1 BN over the last
    axis of (B, C, H, W)) and its autograd in float64: the output c0 x + c2, mean and variance,
    dx = c0 x + c1 dy + c2, dgamma, dbeta, with N = B S C; and the no-cancellation choice of
    the operands' signs."""
    from test_resnet_gpu import col_bn_ref
    x, dy, gamma, beta, _, rmean, rvar = stat_operands(9000 + S, B, C, S, "cpu")
    N = B * S * C
    f = bn_fwd_ref(col_sums(x), col_sums(x * x), N, gamma, beta, EPS, rmean, rvar, 0.75)
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_()  # (B, C, H, W)
    gr, br = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y, mean, var = col_bn_ref(xn, gr, br, EPS)
    assert torch.allclose(f["mean"], mean.detach(), rtol=1e-13, atol=1e-15)
    assert torch.allclose(f["var"], var.detach(), rtol=1e-12)
    assert torch.allclose(apply_ref(x, f["coef"], relu=False).permute(0, 3, 1, 2), y.detach(),
                          rtol=1e-12, atol=1e-13)
    assert torch.allclose(f["rvar"], 0.75 * rvar + 0.25 * var.detach(), rtol=1e-12)
    assert torch.allclose(f["rmean"], 0.75 * rmean + 0.25 * mean.detach(), rtol=1e-7, atol=1e-7)
    y.backward(dy.permute(0, 3, 1, 2))
    b = bn_bwd_ref(col_sums(dy), col_sums(dy * (x - f["mean"].view(1, 1, S, 1))), N, gamma,
                   f["mean"], f["rstd"])
    assert torch.allclose(b["dbeta"], br.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(b["dgamma"], gr.grad, rtol=1e-11, atol=1e-11)
    dx = apply_ref(x, b["coef"], relu=False, dy=dy)
    assert torch.allclose(dx.permute(0, 3, 1, 2), xn.grad, rtol=1e-10, atol=1e-12)
    # same-signed terms in both constant coefficients (stat_operands)
    assert bool((beta * (f["mean"] * gamma) <= 0).all())
    x, dy, gamma, _, m, _, _ = stat_operands(9000 + S, B, C, S, "cpu")
    s1 = col_sums(dy * (x - m.view(1, 1, S, 1)))
    rstd = torch.full((S,), 0.7, dtype=F64)
    b = bn_bwd_ref(col_sums(dy), s1, N, gamma, m, rstd)
    t1, t2 = -(gamma * rstd / N) * col_sums(dy), -b["coef"][0] * m
    assert bool((t1 * t2 >= 0).all())


# ------------------------------------------------------------------------- statistics

# name: (B, C, CP, S)
STAT_CASES = {
    "b5_c40in64_s9": (5, 40, 64, 9),
    "b3_c36in64_s7": (3, 36, 64, 7),
    "b2_c192_s13": (2, 192, 192, 13),
    "b3_c128_s19": (3, 128, 128, 19),
    "b60_c128_s19_capped": (60, 128, 128, 19),
}


def reduce_geometry(ops, B, S):
    """(blocks, rows per block, block of each (b, h) board row as [B, S, S]) of bn_reduce_kernel
    (bn.hip:291, 303-304): one block per board row up to 1024 blocks, then several rows each."""
    R = B * S
    nblk = min(R, 1024)
    assert ops._lib().rag_bn_workspace(B, S) == nblk * 2 * S
    rpb = (R + nblk - 1) // nblk
    blk = (torch.arange(R, device=DEV) // rpb).view(B, S, 1).expand(B, S, S)
    return nblk, rpb, blk


def check_forward_finish(got, ref, with_running):
    stats, coef, rmean, rvar = got
    assert_ulps(stats[0], ref["mean"], 0, "mean")
    assert_ulps(stats[1], ref["rstd"], 2, "rstd")
    assert_ulps(coef[0], ref["coef"][0], 2, "fwd coef[0]")
    assert bool((coef[1] == 0).all())
    assert_ulps(coef[2], ref["coef"][2], 2, "fwd coef[2]")
    if with_running:
        assert_ulps(rmean, ref["rmean"], 0, "running mean")
        assert_ulps(rvar, ref["rvar"], 2, "running variance")


def check_backward_finish(got, ref):
    dgamma, dbeta, coef = got
    assert_ulps(dbeta, ref["dbeta"], 0, "dbeta")
    assert_ulps(dgamma, ref["dgamma"], 2, "dgamma")
    for k in range(3):
        assert_ulps(coef[k], ref["coef"][k], 2, "bwd coef[%d]" % k)


def f32(t):
    return None if t is None else t.float().contiguous()


def run_statistics(ops, name, affine):
    B, C, CP, S = STAT_CASES[name]
    x, dy, gamma, beta, mean, rmean0, rvar0 = stat_operands(
        9100 + list(STAT_CASES).index(name), B, C, S)
    if not affine:
        gamma = beta = rmean0 = rvar0 = None
    N, mom = B * S * C, 0.75
    nblk, rpb, blk = reduce_geometry(ops, B, S)
    if name.endswith("capped"):
        assert (nblk, rpb) == (1024, 2) and nblk - (B * S + 1) // 2 == 454
    xp, dyp = guarded_input(x, 1, CP), guarded_input(dy, 2, CP)
    # forward
    stats = torch.full((2, S), NAN, device=DEV)
    coef = torch.full((3, S), NAN, device=DEV)
    rmean, rvar = f32(rmean0), f32(rvar0)
    if affine:
        rmean, rvar = rmean.clone(), rvar.clone()
    ops.bn_train_fwd(xp, B, S, C, f32(gamma), f32(beta), rmean, rvar, EPS, mom, stats, coef)
    part = ops.bn_workspace(B, S, xp.device)[:nblk * 2 * S].view(nblk, 2, S).clone()
    assert assert_column_stats(part[:, 0], x, blk, 1.0, "sum x")
    assert assert_column_stats(part[:, 1], x * x, blk, 1.0, "sum x^2")
    ref = bn_fwd_ref(col_sums(x), col_sums(x * x), N, gamma, beta, EPS, rmean0, rvar0, mom)
    check_forward_finish((stats, coef, rmean, rvar), ref, affine)
    # backward, from a hand-made dyadic mean (x - mean stays exact) and the forward's rstd
    bstats = torch.stack([mean.float(), stats[1]])
    dgamma = torch.full((S,), NAN, device=DEV)
    dbeta = torch.full((S,), NAN, device=DEV)
    bcoef = torch.full((3, S), NAN, device=DEV)
    ops.bn_bwd_coef(xp, dyp, B, S, C, f32(gamma), bstats, dgamma, dbeta, bcoef)
    part = ops.bn_workspace(B, S, xp.device)[:nblk * 2 * S].view(nblk, 2, S).clone()
    centred = dy * (x - mean.view(1, 1, S, 1))
    assert assert_column_stats(part[:, 0], dy, blk, 1.0, "sum dy")
    assert assert_column_stats(part[:, 1], centred, blk, 0.125, "sum dy (x - mean)")
    ref = bn_bwd_ref(col_sums(dy), col_sums(centred), N, gamma, bstats[0], bstats[1])
    check_backward_finish((dgamma, dbeta, bcoef), ref)


@gpu
@pytest.mark.parametrize("name", list(STAT_CASES))
def test_bn_statistics(ops, name):
    """bn_train_fwd and bn_bwd_coef (bn_reduce_kernel<0 / 1>, bn.hip:96-156, then
    bn_finalize_kernel, bn.hip:160-182): the per-block partials exactly, the finish against
    the float64 formulas with N = B S C. x at halo 1, dy at halo 2; C = 36 is no multiple of 8
    (the padded channels are zero: the layout's invariant). (60, 128, 19) has 1140 board rows:
    reduce_blocks caps at 1024 (bn.hip:291), two rows per block, 454 empty blocks that write zero
    partials."""
    run_statistics(ops, name, True)


@gpu
def test_bn_statistics_null_affine(ops):
    """gamma, beta and the running averages null (bn.hip:59, 68-69): gamma counts as 1, beta as
    0, no running average is written."""
    run_statistics(ops, "b5_c40in64_s9", False)


@gpu
@pytest.mark.parametrize("nblk", [1, 61, 300])
def test_bn_finalize_from_partials(ops, nblk):
    """bn_finalize_fwd / bn_finalize_bwd on hand-made integer partials [nblk, 2, S] (the
    BN-fused conv epilogues' form): the 256-thread loop over the partials (bn.hip:167-170) takes
    a second trip at nblk = 300; the sums are exact in double, the finish as above."""
    B, C, S = 2, 40, 9
    N, mom = B * S * C, 0.75
    g = gen(9200 + nblk)
    gamma = 2.0 ** ints(g, (S,), -1, 2)
    rmean0, rvar0 = ints(g, (S,), -8, 8, 0.25), ints(g, (S,), 1, 8, 0.25)
    part = torch.stack([ints(g, (nblk, S), -20, 20), ints(g, (nblk, S), 40, 120) * (720 // nblk)],
                       1).float().contiguous()
    s0, s1 = part[:, 0].double().sum(0), part[:, 1].double().sum(0)
    beta = ints(g, (S,), 1, 8, 0.125)
    beta = torch.where(s0 > 0, -beta, beta)
    stats = torch.full((2, S), NAN, device=DEV)
    coef = torch.full((3, S), NAN, device=DEV)
    rmean, rvar = f32(rmean0).clone(), f32(rvar0).clone()
    ops.bn_finalize_fwd(part, nblk, B, S, C, f32(gamma), f32(beta), rmean, rvar, EPS, mom, stats,
                        coef)
    ref = bn_fwd_ref(s0, s1, N, gamma, beta, EPS, rmean0, rvar0, mom)
    assert bool((ref["var"] > 1).all())
    check_forward_finish((stats, coef, rmean, rvar), ref, True)
    # backward: s1 stands for sum dy (x - mean); the mean's sign from the sums (no cancellation:
    # sign(mean) = -sign(db dg))
    bpart = torch.stack([ints(g, (nblk, S), -20, 20), ints(g, (nblk, S), -40, 40)],
                        1).float().contiguous()
    d0, d1 = bpart[:, 0].double().sum(0), bpart[:, 1].double().sum(0)
    mean = ints(g, (S,), 1, 8, 0.125)
    mean = torch.where(d0 * d1 > 0, -mean, mean)
    bstats = torch.stack([mean.float(), stats[1]])
    dgamma = torch.full((S,), NAN, device=DEV)
    dbeta = torch.full((S,), NAN, device=DEV)
    bcoef = torch.full((3, S), NAN, device=DEV)
    ops.bn_finalize_bwd(bpart, nblk, B, S, C, f32(gamma), bstats, dgamma, dbeta, bcoef)
    check_backward_finish((dgamma, dbeta, bcoef),
                          bn_bwd_ref(d0, d1, N, gamma, bstats[0], bstats[1]))


# ------------------------------------------------------------------------------ bn_apply

def pow2_coef(S):
    """[3, S] power-of-two column coefficients: cx in {0.5, 1, 2}, cd in {0.5, 1},
    cc in {-1, 0, 2}, cc > 0 on the first and last column (a halo pixel that wrongly became
    act(cc) would show)."""
    col = torch.arange(S, device=DEV)
    cx = torch.tensor([0.5, 1.0, 2.0], device=DEV)[(col // 3) % 3]
    cd = torch.tensor([1.0, 0.5], device=DEV)[col % 2]
    cc = torch.tensor([2.0, -1.0, 0.0], device=DEV)[col % 3]
    cc[-1] = 2.0
    return torch.stack([cx, cd, cc]).contiguous()


def apply_operands(seed, B, C, S):
    g = gen(seed)
    return tuple(ints(g, (B, S, S, C), -3, 3) for _ in range(3))


def prefilled_output(B, S, halo, CP):
    """guarded_output whose interior (all CP channels) is pre-filled with 7.0: every interior
    element must be written, the padded channels with zero."""
    full, out = guarded_output(B, S, halo, CP)
    out[:, halo:halo + S, halo:halo + S, :] = 7.0
    return full, out


def padded_ref(ref, CP):
    B, S, _, C = ref.shape
    out = torch.zeros(B, S, S, CP, dtype=F64, device=DEV)
    out[..., :C] = ref
    return out


def assert_padded_equal(got, ref_nhwc, halo, what):
    """As test_head_exact.assert_padded_equal: value equality with the float64 reference (exact
    in bf16), no NaN, an exactly zero halo."""
    B, S, _, C = ref_nhwc.shape
    assert got.shape == (B, S + 2 * halo, S + 2 * halo, C), got.shape
    assert not bool(torch.isnan(got).any()), "%s: NaN in the output" % what
    border = got.clone()
    border[:, halo:halo + S, halo:halo + S] = 0
    assert not bool(border.view(torch.int16).any()), "%s: the output halo is not zero" % what
    inner = got[:, halo:halo + S, halo:halo + S, :].permute(0, 3, 1, 2).float()
    want = round_bf16_nchw(ref_nhwc).float()
    assert bool((want.double() == ref_nhwc.permute(0, 3, 1, 2)).all()), "reference not bf16-exact"
    if not torch.equal(inner, want):
        bad = inner != want
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d values differ, first at (b, c, i, j) = %s: got %r, "
                             "want %r" % (what, int(bad.sum()), bad.numel(), first,
                                          inner[first].item(), want[first].item()))


@gpu
@pytest.mark.parametrize("halos", [(1, 2, 2, 1), (2, 1, 1, 2), (1, 1, 2, 2)],
                         ids=["h1221", "h2112", "h1122"])
@pytest.mark.parametrize("B,C,CP,S", [(3, 36, 64, 9), (2, 128, 128, 13), (2, 32, 32, 7)])
def test_bn_apply_forms_exact(ops, B, C, CP, S, halos):
    """bn_apply_kernel (bn.hip:191-246) with power-of-two coefficients on integers, halos
    (x, dy, residual, out) drawn from {1, 2} and never all equal: forward BN + ReLU
    (c0 x + c2); the plain ReLU without coefficients (of x + residual); the backward form
    c0 x + c1 dy + c2 + residual without ReLU, also with the residual aliasing the output (in
    place, bn.hip:243). C = 36 in CP = 64: the padded channels are written as zero
    (bn.hip:207-209, 234)."""
    hx, hd, hr, ho = halos
    x, dy, res = apply_operands(9300 + S, B, C, S)
    coef = pow2_coef(S)
    xp, dyp, resp = guarded_input(x, hx, CP), guarded_input(dy, hd, CP), guarded_input(res, hr, CP)
    full, out = prefilled_output(B, S, ho, CP)
    ops.bn_apply(xp, out, B, S, C, coef=coef, relu=True)
    assert_padded_equal(out, padded_ref(apply_ref(x, coef, True), CP), ho, "BN + ReLU")
    assert_guards_untouched(full)
    full, out = prefilled_output(B, S, ho, CP)
    ops.bn_apply(xp, out, B, S, C, coef=None, relu=True, residual=resp)
    assert_padded_equal(out, padded_ref(apply_ref(x, None, True, res=res), CP), ho, "ReLU")
    assert_guards_untouched(full)
    want = padded_ref(apply_ref(x, coef, False, dy=dy, res=res), CP)
    full, out = prefilled_output(B, S, ho, CP)
    ops.bn_apply(xp, out, B, S, C, coef=coef, relu=False, dy=dyp, residual=resp)
    assert_padded_equal(out, want, ho, "backward + residual")
    assert_guards_untouched(full)
    # in place: the residual is the output buffer (its padded channels hold zero, as the layout
    # has them)
    full, out = guarded_output(B, S, ho, CP)
    out[:, ho:ho + S, ho:ho + S, :C] = res.to(BF)
    ops.bn_apply(xp, out, B, S, C, coef=coef, relu=False, dy=dyp, residual=out)
    assert_padded_equal(out, want, ho, "backward + residual in place")
    assert_guards_untouched(full)


@gpu
def test_bn_apply_grid_stride_second_trip(ops):
    """B = 256, C = CP = 192 at 19x19: 2.2 M vectors, the grid of 8192 blocks x 256 threads
    (bn.hip:364-365) takes a second trip of the loop at bn.hip:198. Forward BN + ReLU."""
    B, C, S = 256, 192, 19
    assert B * S * S * (C // 8) > 8192 * 256
    x = ints(gen(9400), (B, S, S, C), -3, 3)
    coef = pow2_coef(S)
    full, out = prefilled_output(B, S, 1, C)
    ops.bn_apply(guarded_input(x, 2, C), out, B, S, C, coef=coef, relu=True)
    assert_padded_equal(out, apply_ref(x, coef, True), 1, "BN + ReLU, B = 256")
    assert_guards_untouched(full)


# ----------------------------------------------------------------------- folded finalize

@gpu
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("B,C,S", [(64, 128, 19), (2, 32, 7), (4, 128, 16)])
def test_bn_apply_bwd_part_equals_two_launches(ops, B, C, S, with_res):
    """bn_apply_part_kernel (bn.hip:254-289) on integer partials [61, 2, S] with gamma and rstd
    powers of two and a dyadic mean: dx, dgamma and dbeta are bit-equal to bn_finalize_bwd +
    bn_apply. (64, 128, 19): 369 664 vectors, the grid is capped at 1024 blocks (bn.hip:385);
    (2, 32, 7): four blocks. At (4, 128, 16) N = B S C = 2^13 and the column sums are multiples
    of N, so every coefficient is a small dyadic number and dx equals the float64 formula
    exactly; at the other two N is no power of two, k1 = ga rstd / N is rounded, and dx is held
    to one bf16 ulp of the float64 formula."""
    nblk = 61 if S != 16 else 64
    N = B * S * C
    g = gen(9500 + B + S)
    x, dy, res = apply_operands(9500 + B, B, C, S)
    gamma = 2.0 ** ints(g, (S,), -1, 1)
    stats = torch.stack([ints(g, (S,), -4, 4, 0.5), 2.0 ** ints(g, (S,), -1, 1)]).float()
    if S == 16:
        # gamma in {1, 2}, rstd in {0.5, 1}, mean in {-1, 0, 1}, column sums t * N with t in
        # {-1, 0, 1} (64 partials of t * N / 64 each): dx is a multiple of 1/8 below 32
        gamma = 2.0 ** ints(g, (S,), 0, 1)
        stats = torch.stack([ints(g, (S,), -1, 1), 2.0 ** ints(g, (S,), -1, 0)]).float()
        part = torch.stack([ints(g, (1, S), -1, 1).expand(nblk, S),
                            ints(g, (1, S), -1, 1).expand(nblk, S)], 1) * (N // nblk)
    else:
        part = torch.stack([ints(g, (nblk, S), -20, 20), ints(g, (nblk, S), -40, 40)], 1)
    part = part.float().contiguous()
    xp, dyp = guarded_input(x, 1, C), guarded_input(dy, 2, C)
    resp = guarded_input(res, 1, C) if with_res else None
    # two launches
    dg2 = torch.full((S,), NAN, device=DEV)
    db2 = torch.full((S,), NAN, device=DEV)
    coef = torch.full((3, S), NAN, device=DEV)
    ops.bn_finalize_bwd(part, nblk, B, S, C, f32(gamma), stats, dg2, db2, coef)
    full2, out2 = prefilled_output(B, S, 2, C)
    ops.bn_apply(xp, out2, B, S, C, coef=coef, relu=False, dy=dyp, residual=resp)
    # one launch
    dg1 = torch.full((S,), NAN, device=DEV)
    db1 = torch.full((S,), NAN, device=DEV)
    full1, out1 = prefilled_output(B, S, 2, C)
    ops.bn_apply_bwd_part(part, nblk, xp, out1, B, S, C, f32(gamma), stats, dg1, db1, dyp,
                          residual=resp)
    assert_guards_untouched(full1)
    assert_guards_untouched(full2)
    assert not bool(torch.isnan(out1).any())
    assert torch.equal(out1.view(torch.int16), out2.view(torch.int16))
    assert torch.equal(dg1, dg2) and torch.equal(db1, db2)
    # the float64 formula
    ref = bn_bwd_ref(part[:, 0].double().sum(0), part[:, 1].double().sum(0), N, gamma, stats[0],
                     stats[1])
    assert_ulps(db1, ref["dbeta"], 0, "dbeta")
    assert_ulps(dg1, ref["dgamma"], 0, "dgamma")  # integer sum times a power of two
    want = apply_ref(x, ref["coef"], False, dy=dy, res=res if with_res else None)
    if S == 16:
        assert_ulps(coef, ref["coef"], 0, "coefficients")
        assert_padded_equal(out1, want, 2, "dx")
    else:
        # the kernel's fp32 chain (fp32 coefficients, two fmaf and an add) is within a few
        # fp32 ulps of the largest term of the float64 value; the store adds half a bf16 ulp
        border = out1.clone()
        border[:, 2:2 + S, 2:2 + S] = 0
        assert not bool(border.view(torch.int16).any())
        c = ref["coef"].view(3, 1, 1, S, 1)
        terms = (c[0] * x).abs() + (c[1] * dy).abs() + c[2].abs() + (res.abs() if with_res else 0)
        _, e = torch.frexp(want.abs())
        ulp = torch.where(want == 0, torch.zeros_like(want), 2.0 ** (e - 8).double())
        err = (out1[:, 2:-2, 2:-2, :].double() - want).abs()
        assert bool((err <= ulp + 8 * 2.0 ** -23 * terms).all()), (err - ulp).max().item()
