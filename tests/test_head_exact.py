"""Exact and float64 tests of the head kernels (csrc/hip/head.hip) and of the input packer's
dihedral transforms (csrc/hip/conv.hip), in the style of test_conv_exact.py.

Operands: the last trunk activation H holds integers {0, 1, 2} (a third zeros, so the ReLU mask
matters), the head weights, biases and the pass weights are multiples of 1/64 in [-8/64, 8/64],
dz holds integers in [-2, 2]. Then

* head_bwd's dH = dz w (H > 0) is a multiple of 1/64 with at most five significant bits (exact
  in bf16) and dw, dpbias, db0 are sums of small integers: all four must EQUAL the float64
  reference cast to the output type;
* head_linear's and policy_head_fwd's position logits are multiples of 1/64, the pass logit
  pass_w . z + pass_b a multiple of 1/4096, all far below 2^24 granules: bit-equal to float64;
* what is left of policy_head_fwd is the softmax, the loss and its gradient on exact logits:
  held to 8x the error of the same formulas evaluated in float32 on the CPU (fp32_figures:
  a property of the number format, not of the kernel), never more than the 1e-5 / 1e-4 the
  project's other fp32 head kernels are held to (test_value_mlp_train).

Every bf16 input is a view of an allocation whose next board is NaN, every padded bf16 output
has a board of 7.0 before and after it and a halo that must stay exactly zero; "equal" compares
values (a masked or zero-weight product may be -0.0).

The float64 references are themselves tested on the CPU (not marked gpu): head_fwd_ref against
torch.autograd through the project's own objectives (kerasish.categorical_crossentropy,
reinforcement.log_loss), including a row whose label probability lies outside the objectives'
clip range [1e-7, 1 - 1e-7]: autograd through the clamp gives such a row a zero gradient, and
the kernel must agree (docs/PARITY.md Q16).
"""
import functools

import numpy as np
import pytest
import torch

from test_conv_exact import (BF, DEV, NAN, assert_guards_untouched, gen, guarded_input,
                             guarded_output, ints, round_bf16_nchw)

gpu = pytest.mark.gpu
F64 = torch.float64

# the objectives' clip limits as fp32 holds them (kernel and fp32 executor alike)
CLIP_LO = float(np.float32(1e-7))
CLIP_HI = float(np.float32(1.0) - np.float32(1e-7))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rocalphago_amd.ops import hipops
    return hipops


# ------------------------------------------------------------------------------- operands

def _ints(g, shape, lo, hi, step=1.0, dev=DEV):
    """test_conv_exact.ints on ``dev``: the CPU self-checks draw the same values."""
    if dev == DEV:
        return ints(g, shape, lo, hi, step)
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8).double() * step


def head_operands(seed, S, K, B, dev=DEV):
    """H [B, S, S, K] in {0, 1, 2}, w [K] and b0 [1] in 1/64 steps, dz [B, S*S] in [-2, 2]."""
    g = gen(seed)
    H = _ints(g, (B, S, S, K), 0, 2, dev=dev)
    w = _ints(g, (K,), -8, 8, 1.0 / 64, dev=dev)
    b0 = _ints(g, (1,), -8, 8, 1.0 / 64, dev=dev)
    dz = _ints(g, (B, S * S), -2, 2, dev=dev)
    return H, w, b0, dz


def packed_h(H, KP):
    """The padded bf16 head input (halo 1) of H [B, S, S, K] behind a NaN board; the padded
    channels K..KP hold 1.0 everywhere: the kernels must not let them into any result."""
    K = H.shape[-1]
    hp = guarded_input(H, 1, KP)
    if KP > K:
        hp[..., K:] = 1.0
    return hp


def guarded_rows(B, n, fill=NAN):
    """(whole allocation, its middle B rows) of an fp32 [B + 2, n] buffer: rows of 7.0 around
    ``fill``."""
    full = torch.full((B + 2, n), fill, device=DEV)
    full[0] = 7.0
    full[-1] = 7.0
    return full, full[1:B + 1]


def assert_padded_equal(got, ref_nhwc, halo, what):
    """The padded bf16 output equals the float64 NHWC reference in value, holds no NaN and has
    an exactly zero halo."""
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


# ------------------------------------------------------------------- float64 references

def head_logits(H, w, b0, pbias=None):
    """z[b, p] = sum_k w[k] H[b, p, k] + b0 (+ pbias[p]) in float64, after the exactness
    precondition: every partial sum is below 2^24 granules of 1/64."""
    B, S, _, K = H.shape
    bound = (H.abs() * w.abs()).sum(-1).max().item() + b0.abs().item()
    if pbias is not None:
        bound += pbias.abs().max().item()
    assert bound * 64 < 2 ** 24, bound
    z = (H.reshape(B, S * S, K) * w).sum(-1) + b0
    return z if pbias is None else z + pbias


def head_bwd_ref(H, w, dz, relu_mask=True):
    """dH [B, S, S, K], dw [K], dpbias [S*S], db0 of z = head_logits(H, w, b0, pbias) for
    dL/dz = dz, with the ReLU derivative of H folded into dH (head.hip:169-176), and the
    exactness precondition: sum |dz| |H| < 2^24 (integers), dH exact in bf16."""
    B, S, _, K = H.shape
    g = dz.view(B, S, S, 1)
    dH = g * w
    if relu_mask:
        dH = torch.where(H > 0, dH, torch.zeros_like(dH))
    assert (g.abs() * H).sum((0, 1, 2)).max().item() < 2 ** 24
    assert dz.abs().sum().item() < 2 ** 24
    assert bool((dH.float().to(BF).double() == dH).all())
    return dH, (g * H).sum((0, 1, 2)), dz.sum(0), dz.sum()


def lowest_argmax(z):
    """argmax over the last axis with ties resolved to the lowest index."""
    C = z.shape[-1]
    idx = torch.arange(C, device=z.device).expand_as(z)
    top = z == z.max(-1, keepdim=True).values
    return torch.where(top, idx, torch.full_like(idx, C)).min(-1).values


def _rowsum(t):
    """Sum over the last axis: float64 as torch sums it; float32 term by term in index order,
    every addition rounded to fp32 (torch.sum's order depends on the CPU's vector width and
    cumsum accumulates in double: neither is the same number on every machine)."""
    if t.dtype == F64:
        return t.sum(-1)
    s = torch.zeros_like(t[..., 0])
    for i in range(t.shape[-1]):
        s = s + t[..., i]
    return s


def _rounded(fn, t):
    """fn(t) correctly rounded to t's type (through float64): no libm in the float32 figure."""
    return fn(t.double()).to(t.dtype)


def head_fwd_ref(z, labels, sw, mode, gscale, pass_w=None, pass_b=None, lo=CLIP_LO,
                 hi=CLIP_HI, dtype=F64):
    """Softmax, per-board loss, top-1 hit and d(sum_b gscale loss_b)/d(logits) of the fused
    head in closed form, evaluated in ``dtype`` (float64: the reference; float32: the same
    formulas for fp32_figures, with correctly rounded exp / log and term-by-term sums, so that
    the figure is the same number on every machine). z [B, S*S] position logits; with pass_w /
    pass_b the softmax runs over S*S + 1 classes (pass last, logit pass_w . z + pass_b) and dz
    carries dpass * pass_w.
    Mode 1: Keras categorical cross-entropy -log clip(p_label); mode 2: REINFORCE log_loss
    -y log clip(p) averaged over the C classes; both times the sample weight. A board whose
    label probability lies outside [lo, hi] has loss -log(limit) and a zero gradient, as
    autograd through the objectives' clamp gives (test_head_reference_matches_autograd)."""
    z = z.to(dtype)
    B, S2 = z.shape
    zz = z
    if pass_w is not None:
        pw = pass_w.to(dtype)
        zz = torch.cat([z, _rowsum(z * pw).unsqueeze(1) + pass_b.to(dtype)], 1)
    C = zz.shape[1]
    e = _rounded(torch.exp, zz - zz.max(-1, keepdim=True).values)
    p = e / _rowsum(e).unsqueeze(1)
    out = {"probs": p, "hit": (lowest_argmax(zz) == labels).to(dtype)}
    if not mode:
        return out
    sw = torch.ones(B, dtype=dtype, device=z.device) if sw is None else sw.to(dtype)
    cls = 1.0 / C if mode == 2 else 1.0
    plab = p.gather(1, labels.view(B, 1)).squeeze(1)
    clipped = (plab < lo) | (plab > hi)
    y = torch.zeros_like(p)
    y.scatter_(1, labels.view(B, 1), 1.0)
    g = (p - y) * (sw * cls * gscale).view(B, 1)
    g = torch.where(clipped.view(B, 1), torch.zeros_like(g), g)
    dz = g[:, :S2]
    if pass_w is not None:
        out["dpass"] = g[:, S2]
        dz = dz + g[:, S2:] * pw
    loss = -_rounded(torch.log, plab.clamp(lo, hi)) * sw * cls
    out.update(loss=loss, dz=dz, dzsum=_rowsum(dz),
               plab=plab, clipped=clipped, scale=sw * cls)
    return out


# ----------------------------------------------------------------- policy head: the cases

# name: (S, K, KP, B)
HEAD_CASES = {
    "s19_k192_b6": (19, 192, 192, 6),
    "s19_k128_b3": (19, 128, 128, 3),
    "s13_k64_b5": (13, 64, 64, 5),
    "s9_k32_b4": (9, 32, 32, 4),
    "s7_k40in64_b2": (7, 40, 64, 2),
}
TIE_A = 3  # the two tied pixels are TIE_A and S*S - 5


@functools.lru_cache(maxsize=None)
def head_case(name, with_pass, dev=DEV):
    """Operands and launches of one policy_head_fwd case (computed once, never modified).

    Ties: pixels a < b of boards 0 and 1 carry identical channel rows and equal pbias (raised
    just enough to make the pair each board's maximum). Without a pass logit board 0 is labelled a
    (a hit) and board 1 b (no hit: argmax takes the lowest index). With one, pass_b is set (in
    1/4096 steps) so that board 1's pass logit equals its maximum too and board 1 is labelled
    pass: a three-way tie that the lowest index wins; the last board is labelled pass as well.
    Launches: gscale 1 and 1/B without sample weights; signed weights with zeros and
    gscale 1/(B norm), norm the non-zero fraction (models/fused.py train_step); "clip":
    pbias of board 0's best point q raised by 24, so that every label but q has
    p_label ~ e^-24 < 1e-7 (board 0, labelled q, has p_label > 1 - 1e-7)."""
    S, K, KP, B = HEAD_CASES[name]
    S2 = S * S
    C = S2 + (1 if with_pass else 0)
    seed = 7000 + 10 * list(HEAD_CASES).index(name) + int(with_pass)
    H, w, b0, _ = head_operands(seed, S, K, B, dev)
    g = gen(seed + 5)
    pbias = _ints(g, (S2,), -8, 8, 1.0 / 64, dev=dev)
    pass_w = _ints(g, (S2,), -8, 8, 1.0 / 64, dev=dev) if with_pass else None
    pass_b = _ints(g, (1,), -8, 8, 1.0 / 64, dev=dev) if with_pass else None
    labels = torch.randint(0, C, (B,), generator=g).to(dev)
    a, b = TIE_A, S2 - 5
    Hf = H.view(B, S2, K)
    Hf[0, b] = Hf[0, a]
    Hf[1, b] = Hf[1, a]
    pbias[a] = pbias[b] = 0.0
    z = head_logits(H, w, b0, pbias)
    # the smallest bias (in 1/64 steps) that makes the pair the maximum of boards 0 and 1
    pbias[a] = pbias[b] = (z[:2].max(-1).values - z[:2, a]).max() + 1.0 / 64
    labels[labels == a] = a + 1  # only the clip launch labels a board with q = a
    labels[0] = a
    labels[1] = b
    z = head_logits(H, w, b0, pbias)
    assert lowest_argmax(z)[0].item() == a and z[0, a] == z[0, b] and z[1, a] == z[1, b]
    assert lowest_argmax(z)[1].item() == a
    if with_pass:
        pass_b = (z[1, a] - (z[1] * pass_w).sum()).view(1)
        assert bool((pass_b * 4096 == (pass_b * 4096).round()).all())
        labels[1] = S2
        labels[B - 1] = S2
    sw = _ints(gen(seed + 6), (B,), -6, 6, 0.25, dev=dev)
    sw[0] = 0.0
    sw[B - 1] = -1.25
    norm = (sw != 0).double().mean().item()
    q = a
    pclip = pbias.clone()
    pclip[q] += 24.0
    lclip = labels.clone()
    lclip[0] = q

    def f32(v):
        return float(np.float32(v))

    launches = [("g1", pbias, labels, None, 1.0), ("gB", pbias, labels, None, f32(1.0 / B)),
                ("sw", pbias, labels, sw, f32(1.0 / (B * norm))),
                ("clip", pclip, lclip, None, f32(1.0 / B))]
    # preconditions on the reference: exact pass logits, label probabilities well inside the
    # clip range (ordinary launches) or well outside it (the clip launch)
    for tag, pb, lab, _, _ in launches:
        zl = head_logits(H, w, b0, pb)
        if with_pass:
            assert ((zl.abs() * pass_w.abs()).sum(-1).max().item()
                    + pass_b.abs().item()) * 4096 < 2 ** 24
        ref = head_fwd_ref(zl, lab, None, 1, 1.0, pass_w, pass_b)
        if tag == "clip":
            assert bool(((ref["plab"] < 1e-8) | (ref["plab"] > 1 - 3e-8)).all()), ref["plab"]
            assert bool(ref["clipped"].all()) and ref["plab"][0] > 0.5 and ref["plab"][1] < 0.5
        else:
            assert bool(((ref["plab"] >= 1e-6) & (ref["plab"] <= 1 - 1e-6)).all()), ref["plab"]
    return dict(S=S, K=K, KP=KP, B=B, C=C, H=H, w=w, b0=b0, pass_w=pass_w, pass_b=pass_b,
                launches=launches)


def head_errors(ref, got):
    """Error figures of ``got`` against the float64 ``ref`` (both dicts as head_fwd_ref's):
    "val": the largest of the probabilities' relative error, |row sum - 1|, the loss's relative
    error (for a board clipped at the upper limit, where the loss is ~1e-7 and d(-log p) = dp / p
    with p ~ 1, the error relative to weight / C instead) and |dzsum - sum dz| / sum |dz|;
    "grad": the largest error of dz and dpass relative to the board's largest |gradient|. A board
    whose reference gradient is zero (zero weight, clipped label) must have an exactly zero one:
    it counts as inf otherwise."""
    def d(t):
        return t.detach().double().cpu()

    inf = torch.tensor(float("inf"), dtype=F64)
    p, pr = d(got["probs"]), d(ref["probs"])
    val = [((p - pr).abs() / pr).max(), (p.sum(-1) - 1).abs().max()]
    grad = []
    if "loss" in ref:
        scale = d(ref["scale"]).abs()
        upper = d(ref["plab"]) > 0.5
        den = torch.where(ref["clipped"].cpu() & upper, scale, d(ref["loss"]).abs())
        err = (d(got["loss"]) - d(ref["loss"])).abs()
        val.append(torch.where(den > 0, err / den.clamp_min(1e-300),
                               torch.where(err > 0, inf, 0 * err)).max())
        dz, dzr = d(got["dz"]), d(ref["dz"])
        rowmax = dzr.abs().max(-1).values
        rowerr = (dz - dzr).abs().max(-1).values
        if "dpass" in ref:
            rowmax = torch.maximum(rowmax, d(ref["dpass"]).abs())
            rowerr = torch.maximum(rowerr, (d(got["dpass"]) - d(ref["dpass"])).abs())
        grad.append(torch.where(rowmax > 0, rowerr / rowmax.clamp_min(1e-300),
                                torch.where(rowerr > 0, inf, 0 * rowerr)).max())
        if got.get("dzsum") is not None:
            tot = dzr.abs().sum(-1)
            serr = (d(got["dzsum"]) - dzr.sum(-1)).abs()
            val.append(torch.where(tot > 0, serr / tot.clamp_min(1e-300),
                                   torch.where(serr > 0, inf, 0 * serr)).max())
    return {"val": max(v.item() for v in val), "grad": max([v.item() for v in grad] or [0.0])}


@functools.lru_cache(maxsize=None)
def fp32_figures():
    """The largest head_errors of head_fwd_ref evaluated in float32 on the CPU against its
    float64 self, over every case, mode, pass form and launch of this file: what fp32 with a
    correctly rounded exp / log and plain sums of up to 362 terms loses on these (exact)
    logits."""
    val = grad = 0.0
    for name in HEAD_CASES:
        for with_pass in (False, True):
            c = head_case(name, with_pass, "cpu")
            for _, pb, lab, sw, gs in c["launches"]:
                z = head_logits(c["H"], c["w"], c["b0"], pb)
                for mode in (1, 2):
                    ref = head_fwd_ref(z, lab, sw, mode, gs, c["pass_w"], c["pass_b"])
                    f32 = head_fwd_ref(z, lab, sw, mode, gs, c["pass_w"], c["pass_b"],
                                       dtype=torch.float32)
                    e = head_errors(ref, f32)
                    val, grad = max(val, e["val"]), max(grad, e["grad"])
    return val, grad


def head_bounds():
    """(values, gradients): 8x the float32 figures (fast intrinsics are a few ulps looser than
    libm and the summation order differs), capped by what the project holds its other fp32 head
    kernels to (test_value_mlp_train: 1e-5 on values, 1e-4 relative on gradients)."""
    val, grad = fp32_figures()
    return min(8 * val, 1e-5), min(8 * grad, 1e-4)


# -------------------------------------------------------------- CPU self-checks (no GPU)

@pytest.mark.parametrize("with_pass", [False, True], ids=["nopass", "pass"])
@pytest.mark.parametrize("mode", [1, 2])
def test_head_reference_matches_autograd(mode, with_pass):
    """head_fwd_ref against torch.autograd through the project's own objectives on a 3x3 board:
    kerasish.categorical_crossentropy (mode 1) and reinforcement.log_loss with Keras's mean over
    the classes (mode 2) of one-hot targets, times the sample weight; the gradient of
    sum_b gscale loss_b with respect to the position logits (the pass logit's share arrives
    through pass_w) and to the pass logit. Board 2's label probability is ~e^-24 and board 3's
    ~1 - 8 e^-24: the clamp gives both a zero gradient."""
    from rocalphago_amd.models import kerasish
    from rocalphago_amd.training import reinforcement
    B, S2 = 5, 9
    g = gen(41 + mode)
    z = _ints(g, (B, S2), -64, 64, 1.0 / 64, dev="cpu")
    labels = torch.tensor([0, 4, 1, 7, 8 + int(with_pass)])
    z[2, 7] += 24.0
    z[3, 7] += 24.0
    pass_w = _ints(g, (S2,), -8, 8, 1.0 / 64, dev="cpu") if with_pass else None
    pass_b = _ints(g, (1,), -8, 8, 1.0 / 64, dev="cpu") if with_pass else None
    sw = torch.tensor([1.5, -0.75, 2.0, 1.0, 0.5], dtype=F64)
    gscale = 0.2
    lo, hi = kerasish.EPSILON, 1.0 - kerasish.EPSILON
    ref = head_fwd_ref(z, labels, sw, mode, gscale, pass_w, pass_b, lo=lo, hi=hi)
    assert ref["clipped"].tolist() == [False, False, True, True, False]
    zr = z.clone().requires_grad_()
    zz = zr
    if with_pass:
        zp = (zr * pass_w).sum(-1, keepdim=True) + pass_b
        zp.retain_grad()
        zz = torch.cat([zr, zp], 1)
    y_pred = torch.softmax(zz, -1)
    y_true = torch.zeros_like(y_pred)
    y_true[torch.arange(B), labels] = 1.0
    if mode == 1:
        loss = kerasish.categorical_crossentropy(y_true, y_pred) * sw
    else:
        loss = reinforcement.log_loss(y_true, y_pred).mean(-1) * sw
    (gscale * loss).sum().backward()
    assert torch.allclose(ref["loss"], loss.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(ref["probs"], y_pred.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(ref["dz"], zr.grad, rtol=1e-11, atol=1e-18)
    assert bool((zr.grad[2:4] == 0).all()) and bool((ref["dz"][2:4] == 0).all())
    assert bool((zr.grad[:2] != 0).all())
    if with_pass:
        assert torch.allclose(ref["dpass"], zp.grad.squeeze(1), rtol=1e-11, atol=1e-18)
    assert ref["hit"].tolist() == (zz.argmax(-1) == labels).double().tolist()
    # the fp32-rounded clip limits of the default reference move the clipped loss by < 1e-8
    dflt = head_fwd_ref(z, labels, sw, mode, gscale, pass_w, pass_b)
    assert torch.equal(dflt["dz"], ref["dz"])
    assert torch.allclose(dflt["loss"][[0, 1, 2, 4]], ref["loss"][[0, 1, 2, 4]], rtol=1e-8)


def test_head_reference_ties_take_the_lowest_index():
    z = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, 1.0, 0.0, 5.0]])
    assert lowest_argmax(z).tolist() == [1, 0, 3]


def test_head_bwd_reference_matches_autograd():
    """head_bwd_ref against autograd of z = sum_k w[k] relu(x)[., k] + b0 + pbias on a 3x3 board
    (x = H where H > 0, negative elsewhere: the mask is the ReLU's derivative)."""
    S, K, B = 3, 8, 2
    H, w, b0, dz = head_operands(11, S, K, B, "cpu")
    x = torch.where(H > 0, H, -torch.ones_like(H)).requires_grad_()
    wr, br = w.clone().requires_grad_(), b0.clone().requires_grad_()
    pb = torch.zeros(S * S, dtype=F64, requires_grad=True)
    z = (torch.relu(x).view(B, S * S, K) * wr).sum(-1) + br + pb
    (z * dz).sum().backward()
    dH, dw, dpb, db0 = head_bwd_ref(H, w, dz)
    assert torch.equal(dH, x.grad) and torch.equal(dw, wr.grad)
    assert torch.equal(dpb, pb.grad) and torch.equal(db0.view(1), br.grad)
    assert 0.2 < (H == 0).double().mean().item() < 0.45
    assert torch.equal(head_logits(H, w, b0), (z - pb).detach())


def test_fp32_reference_error_keeps_the_bound_below_the_cap():
    """The float32-vs-float64 figure of the softmax / loss / gradient formulas on this file's
    logits: below 1e-6, so that the 8x bound of the GPU tests stays under the project's caps."""
    val, grad = fp32_figures()
    print("float32 reference error: values %.3g, gradients %.3g -> bounds %.3g, %.3g" %
          ((val, grad) + head_bounds()))
    assert 0 < val < 1e-6 and 0 < grad < 1e-6
    assert head_bounds() == (8 * val, 8 * grad)


# ------------------------------------------------------------------- head_bwd, bit-exact

def run_head_bwd(ops, S, K, KP, B, seed, relu_mask=True, null_dh=False, null_dpbias=False,
                 from_dzsum=False, unaligned=False, metrics=False, w_kernel=None):
    """One head_bwd launch against head_bwd_ref: dH, dw, dpbias, db0 equal the float64 values,
    dw past K untouched (NaN), dH's padded channels and halo zero, guard boards untouched.
    Returns (dH view, float64 operands) for the comparator self-check."""
    H, w, _, dz = head_operands(seed, S, K, B)
    S2 = S * S
    ref_dh, ref_dw, ref_dpb, ref_db0 = head_bwd_ref(H, w, dz, relu_mask)
    hp = packed_h(H, KP)
    if unaligned:  # a contiguous view one float into its storage: not 16-byte aligned
        store = torch.full((B * S2 + 1,), NAN, device=DEV)
        dzk = store[1:].view(B, S2)
        dzk.copy_(dz)
        assert dzk.is_contiguous() and dzk.data_ptr() % 16 == 4 and (B * S2) % 4
    else:
        dzk = dz.float().contiguous()
    full, dh = (None, None) if null_dh else guarded_output(B, S, 1, KP)
    dw = torch.full((KP,), NAN, device=DEV)
    db0 = torch.full((1,), NAN, device=DEV)
    dpb = None if null_dpbias else torch.full((S2,), NAN, device=DEV)
    dzsum = m = None
    if from_dzsum:  # deliberately not the row sums of dz: db0 must come from here
        dzsum = ints(gen(seed + 1), (B,), -3, 3).float()
        ref_db0 = dzsum.double().sum()
        assert ref_db0.item() != dz.sum().item()
    if metrics:
        g = gen(seed + 2)
        m = (ints(g, (B,), 0, 5).float(), ints(g, (B,), 0, 1).float(),
             torch.tensor([3.0, 5.0], device=DEV))
    wk = w if w_kernel is None else w_kernel
    ops.head_bwd(hp, wk.float().contiguous(), dzk, dh, dw, db0, dpb, K, relu_mask=relu_mask,
                 metrics=m, dzsum=dzsum)
    assert torch.equal(dw[:K], ref_dw.float()), "dw"
    assert bool(torch.isnan(dw[K:]).all()), "dw past K was written"
    assert torch.equal(db0, ref_db0.float().view(1)), (db0.item(), ref_db0.item())
    if dpb is not None:
        assert torch.equal(dpb, ref_dpb.float()), "dpbias"
    if metrics:
        want = torch.stack([3.0 + m[0].double().sum(), 5.0 + m[1].double().sum()]).float()
        assert torch.equal(m[2], want), (m[2].tolist(), want.tolist())
    if dh is not None and w_kernel is None:
        padded = torch.zeros(B, S, S, KP, dtype=F64, device=DEV)
        padded[..., :K] = ref_dh
        assert_padded_equal(dh, padded, 1, "dH")
    if full is not None:
        assert_guards_untouched(full)
    return dh, (H, w, dz)


# id: (S, K, KP, B, options of run_head_bwd)
HEAD_BWD_CASES = dict(
    [("kp%d" % kp, (9, kp, kp, 3, {})) for kp in (32, 64, 96, 128, 192, 256, 384, 512)] + [
        ("k59_in_kp64", (9, 59, 64, 3, {})),
        ("k187_in_kp192", (9, 187, 192, 3, {})),
        ("one_7x7_board", (7, 64, 64, 1, {})),
        ("block_cap_b35", (19, 192, 192, 35, {})),
        ("b1030", (9, 32, 32, 1030, {})),
        ("b1030_dzsum_metrics", (9, 32, 32, 1030, dict(from_dzsum=True, metrics=True))),
        ("no_relu_mask", (9, 64, 64, 3, dict(relu_mask=False))),
        ("null_dh", (9, 64, 64, 3, dict(null_dh=True))),
        ("null_dpbias", (9, 64, 64, 3, dict(null_dpbias=True))),
        ("db0_from_dzsum", (9, 64, 64, 7, dict(from_dzsum=True))),
        ("unaligned_dz", (19, 64, 64, 7, dict(unaligned=True))),
        ("metrics_b7", (9, 32, 32, 7, dict(metrics=True))),
        ("metrics_b1030", (9, 32, 32, 1030, dict(metrics=True))),
    ])


@gpu
@pytest.mark.parametrize("name", list(HEAD_BWD_CASES))
def test_head_bwd_exact(ops, name):
    """head_bwd_kernel<CH> + head_bwd_reduce_kernel against head_bwd_ref, each case the
    smallest that reaches its branch:

    kp32 .. kp512    each head_bwd_kernel<CH>, CH = KP / 8 (the switch at head.hip:580-583),
                     K = KP, B = 3 at 9x9: 243 pixels in six blocks; PPI = 256 / CH pixel lanes,
                     for CH = 12, 24, 48 with idle threads (head.hip:185, 201)
    k59_in_kp64, k187_in_kp192   K = KP - 5 with 1.0 in the input's padded channels: the weights
                     past K are zero in LDS (head.hip:188), so dH[..., K:] is zero, and the reduce
                     writes dw[:K] only (head.hip:343-345): dw past K stays NaN
    one_7x7_board    B = 1 at 7x7: 49 pixels, two blocks of 25 and 24 (head.hip:571-573)
    block_cap_b35    B = 35 at 19x19, KP = 192: 12 635 pixels want 264 blocks, the cap
                     kHeadBwdBlocks = 256 holds (head.hip:572), 50 pixels per block, blocks
                     253..255 are empty (head.hip:199-200) and still write zero dw partials
    b1030, b1030_dzsum_metrics   B = 1030 at 9x9, KP = 32: the dpbias columns sum 1030 rows
                     (head.hip:328-335); with dzsum and metrics the last reduce block's loops over
                     the boards take a second trip (head.hip:265, 290)
    no_relu_mask     relu_mask = 0 (head.hip:224): dH = dz w also where H is zero
    null_dh          dH = null (head.hip:228): dw, dpbias and db0 are still exact
    null_dpbias      dpbias = null (head.hip:346): nothing else changes
    db0_from_dzsum   db0 is the sum of the per-board dzsum (head.hip:264-265), here a vector that
                     is not the row sums of dz, so the documented source is proven
    unaligned_dz     dz one float into its storage, B S^2 = 2527 not a multiple of 4: the 16-byte
                     sum of db0 falls back to scalar loads for all of it (n4 = 0,
                     head.hip:270, 286)
    metrics_b7, metrics_b1030   metrics = (loss, hit, acc) with integer losses, 0 / 1 hits and
                     acc starting at [3, 5]: acc ends at [3 + sum loss, 5 + sum hit] exactly
                     (head.hip:289-293, 311-314)"""
    S, K, KP, B, opts = HEAD_BWD_CASES[name]
    run_head_bwd(ops, S, K, KP, B, seed=6000 + list(HEAD_BWD_CASES).index(name), **opts)


@gpu
def test_head_bwd_comparator_sees_one_wrong_weight(ops):
    """Self-check of the comparison: w[k] raised by 1/64 on the kernel's side only changes dH
    exactly at channel k where dz != 0 and H > 0, and leaves dw, dpbias, db0 unchanged."""
    S, K, B, k = 9, 64, 3, 37
    H, w, _, dz = head_operands(6990, S, K, B)
    w_bad = w.clone()
    w_bad[k] += 1.0 / 64
    dh, _ = run_head_bwd(ops, S, K, K, B, seed=6990, w_kernel=w_bad)
    good, _ = run_head_bwd(ops, S, K, K, B, seed=6990)
    differs = dh[:, 1:-1, 1:-1, :].float() != good[:, 1:-1, 1:-1, :].float()
    want = torch.zeros_like(differs)
    want[..., k] = (dz.view(B, S, S) != 0) & (H[..., k] > 0)
    assert 0.3 < want[..., k].double().mean().item() < 0.7
    assert torch.equal(differs, want)


# --------------------------------------------------------------------------- head_linear

@gpu
@pytest.mark.parametrize("S", [7, 19])
@pytest.mark.parametrize("K,KP", [(192, 192), (128, 128), (256, 256), (40, 40), (36, 40),
                                  (320, 320)])
def test_head_linear_bit_exact(ops, K, KP, S):
    """head_linear_kernel<NM> (head.hip:603-610): NM = 3, 2, 4, 1 with the weights in registers,
    NM = 0 for K = 36 (not a multiple of 8) and for K = 320 (> 256); 1.0 in the padded channels
    of (36, 40). z is bit-equal to the float64 logits; the rows around z stay untouched."""
    B = 3
    H, w, b0, _ = head_operands(6000 + K + S, S, K, B)
    full, z = guarded_rows(B, S * S)
    ops.head_linear(packed_h(H, KP), w.float(), b0.float(), z, K)
    assert torch.equal(z, head_logits(H, w, b0).float())
    assert_guards_untouched(full)


# ----------------------------------------------------------------------- policy_head_fwd

def launch_policy_head(ops, c, hp, pbias, labels, sw, gscale, mode, with_dzsum=True, acc=None):
    """One policy_head_fwd launch into NaN-filled buffers between guard rows; returns the
    outputs and the guard allocations."""
    B, S2, C = c["B"], c["S"] ** 2, c["C"]
    has_pass = c["pass_w"] is not None
    bufs = {"probs": guarded_rows(B, C), "dz": guarded_rows(B, S2), "loss": guarded_rows(B, 1),
            "hit": guarded_rows(B, 1)}
    if has_pass:
        bufs.update(zout=guarded_rows(B, S2), dpass=guarded_rows(B, 1))
    elif with_dzsum:
        bufs["dzsum"] = guarded_rows(B, 1)
    out = {k: v[1] for k, v in bufs.items()}

    def flat(k):
        return out[k].view(B) if k in out else None

    def f32(t):
        return None if t is None else t.float().contiguous()

    ops.policy_head_fwd(hp, f32(c["w"]), f32(c["b0"]), f32(pbias), out["probs"], c["K"],
                        labels=labels, sweight=f32(sw), loss=flat("loss"), dz=out["dz"],
                        hit=flat("hit"), mode=mode, gscale=gscale, pass_w=f32(c["pass_w"]),
                        pass_b=f32(c["pass_b"]), zout=out.get("zout"), dpass=flat("dpass"),
                        acc=acc, dzsum=flat("dzsum"))
    for k in ("loss", "hit", "dpass", "dzsum"):
        if k in out:
            out[k] = out[k].view(B)
    return out, [v[0] for v in bufs.values()]


@gpu
@pytest.mark.parametrize("with_pass", [False, True], ids=["nopass", "pass"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_policy_head_fwd(ops, name, mode, with_pass):
    """policy_head_fwd_kernel (head.hip:37-167) on head_case's four launches: the position logits
    (zout, head.hip:87) bit-equal to float64 and to head_linear + pbias; probabilities, loss
    (head.hip:143-148), dz / dpass (head.hip:118-137) and dzsum (head.hip:139-142) within
    head_bounds of head_fwd_ref; hit (head.hip:153-165) equal, ties to the lowest index; the
    PassLogit dW, db of pass_grads (head.hip:498-527) chained from dpass. Mode 0 writes probs
    (and zout) only: the NaN-filled loss, dz, hit, dpass, dzsum buffers stay NaN. In the "clip"
    launch every board's label probability is outside [1e-7, 1 - 1e-7] (the flag of
    head.hip:107-116): its loss is -log(limit) times the weight (over C in mode 2) and its dz,
    dpass, dzsum are exactly zero."""
    c = head_case(name, with_pass)
    B, S2 = c["B"], c["S"] ** 2
    hp = packed_h(c["H"], c["KP"])
    bval, bgrad = head_bounds()
    zlin = torch.empty(B, S2, device=DEV)
    ops.head_linear(hp, c["w"].float(), c["b0"].float(), zlin, c["K"])
    for tag, pbias, labels, sw, gscale in c["launches"]:
        z = head_logits(c["H"], c["w"], c["b0"], pbias)
        ref = head_fwd_ref(z, labels, sw, mode, gscale, c["pass_w"], c["pass_b"])
        got, fulls = launch_policy_head(ops, c, hp, pbias, labels, sw, gscale, mode)
        for full in fulls:
            assert_guards_untouched(full)
        what = "%s mode %d %s" % (name, mode, tag)
        if with_pass:
            assert torch.equal(got["zout"], z.float()), what
            assert torch.equal(got["zout"], zlin + pbias.float()), what
        assert not bool(torch.isnan(got["probs"]).any()), what
        if mode == 0:
            for k in ("loss", "dz", "hit", "dpass", "dzsum"):
                assert k not in got or bool(torch.isnan(got[k]).all()), what + ": wrote " + k
        err = head_errors(ref, got)
        print("%s: values %.3g (bound %.3g), gradients %.3g (bound %.3g)" %
              (what, err["val"], bval, err["grad"], bgrad))
        assert err["val"] <= bval and err["grad"] <= bgrad, (what, err)
        if mode == 0:
            continue
        assert torch.equal(got["hit"].double(), ref["hit"]), what
        if tag == "clip":
            assert bool(ref["clipped"].all())
            for k in ("dz", "dpass", "dzsum"):
                assert k not in got or bool((got[k] == 0).all()), what + ": " + k
        if with_pass:
            # dW[j] = sum_b dpass[b] z[b, j], db = sum_b dpass[b]: dpass's error (bgrad of the
            # board's largest gradient M_b) times |z|, plus an fp32 sum of B terms
            dW = torch.full((S2,), NAN, device=DEV)
            db = torch.full((1,), NAN, device=DEV)
            ops.pass_grads(got["zout"], got["dpass"], dW, db)
            M = torch.maximum(ref["dz"].abs().max(-1).values, ref["dpass"].abs())
            tol = bgrad * (z.abs() * M.view(B, 1)).sum(0) \
                + 1e-6 * (z * ref["dpass"].view(B, 1)).abs().sum(0)
            assert bool(((dW.double() - (z * ref["dpass"].view(B, 1)).sum(0)).abs() <= tol).all())
            assert abs(db.item() - ref["dpass"].sum().item()) <= \
                bgrad * M.sum().item() + 1e-6 * ref["dpass"].abs().sum().item()


@gpu
def test_policy_head_fwd_in_kernel_metrics(ops):
    """acc (head.hip:148, 164; the engine passes None in training): mode 1, acc starting at
    [3, 5] ends at [3 + sum loss, 5 + hits]; the loss sum within head_bounds of sum |loss| (its
    atomic adds come in any order), the hit count exactly."""
    c = head_case("s9_k32_b4", False)
    _, pbias, labels, sw, gscale = c["launches"][2]
    acc = torch.tensor([3.0, 5.0], device=DEV)
    got, _ = launch_policy_head(ops, c, packed_h(c["H"], c["KP"]), pbias, labels, sw, gscale, 1,
                                acc=acc)
    ref = head_fwd_ref(head_logits(c["H"], c["w"], c["b0"], pbias), labels, sw, 1, gscale)
    assert ref["hit"].sum().item() >= 1
    assert acc[1].item() == 5.0 + ref["hit"].sum().item()
    assert abs(acc[0].item() - 3.0 - ref["loss"].sum().item()) <= \
        head_bounds()[0] * (3.0 + ref["loss"].abs().sum().item())


@gpu
def test_policy_head_fwd_refuses_dzsum_with_pass_logit(ops):
    """dzsum has no pass-logit form (hipops.policy_head_fwd): the wrapper raises."""
    c = head_case("s9_k32_b4", True)
    _, pbias, labels, _, _ = c["launches"][0]
    B, S2 = c["B"], c["S"] ** 2
    with pytest.raises(ValueError):
        ops.policy_head_fwd(packed_h(c["H"], c["KP"]), c["w"].float(), c["b0"].float(),
                            pbias.float(), torch.empty(B, S2 + 1, device=DEV), c["K"],
                            labels=labels, dz=torch.empty(B, S2, device=DEV), mode=1,
                            pass_w=c["pass_w"].float(), pass_b=c["pass_b"].float(),
                            zout=torch.empty(B, S2, device=DEV),
                            dpass=torch.empty(B, device=DEV),
                            dzsum=torch.empty(B, device=DEV))


# ------------------------------------------------------- planes and labels move together

def plane_dataset(S, F, N, seed):
    """uint8 planes [N, F, S, S] on the CPU: random bits, plane 0 of position n one-hot at point
    n % S^2 (so a moved plane names its own label)."""
    g = gen(seed)
    planes = (torch.rand((N, F, S, S), generator=g) < 0.4).to(torch.uint8)
    planes[:, 0] = 0
    planes[:, 0].view(N, S * S)[torch.arange(N), torch.arange(N) % (S * S)] = 1
    return planes


@gpu
@pytest.mark.parametrize("S,F", [(7, 48), (9, 48), (13, 48), (19, 48), (19, 49)])
def test_pack_input_matches_host_transforms(ops, S, F):
    """pack_input of uint8, float32 and bit-packed planes into CP = 64 at halo 1 and 2, with an
    index that repeats and all eight transforms (the device map dihedral(), conv.hip:424-437,
    through pack_input_lds_kernel and pack_input_bits_kernel): every plane equals
    training.data.apply_transform_np, the host definition; the three forms are bit-equal; the
    padded channels and the halo are zero; ``nplanes`` < F packs only the leading planes of
    the two dense forms. F = 49 (an odd position stride: the byte-wise staging loop,
    conv.hip:501-505) runs at 19x19."""
    from rocalphago_amd.training.data import apply_transform_np
    from rocalphago_amd.training.replay import pack_bits
    N, CP = 6, 64
    planes = plane_dataset(S, F, N, 8000 + S + F)
    index = torch.tensor([5, 1, 4, 1, 0, 5, 2, 3, 3, 1, 0, 2, 4, 4, 5, 0])
    tf = torch.arange(16, dtype=torch.int32) % 8
    tf[8:] = torch.tensor([3, 7, 1, 6, 0, 5, 2, 4], dtype=torch.int32)
    B = index.numel()
    want = np.stack([apply_transform_np(planes[n].numpy(), int(t))
                     for n, t in zip(index.tolist(), tf.tolist())])
    want = torch.from_numpy(want).to(DEV)
    src = {"u8": planes.to(DEV), "f32": planes.to(DEV).float(),
           "bits": pack_bits(planes).to(DEV)}
    for halo in (1, 2):
        outs = {}
        for form, feats in src.items():
            full, out = guarded_output(B, S, halo, CP)
            out[:] = 7.0  # every element of the batch's boards' interior must be written
            out[:, :halo] = 0
            out[:, -halo:] = 0
            out[:, :, :halo] = 0
            out[:, :, -halo:] = 0
            ops.pack_input(feats, out, halo, index=index.to(DEV), transforms=tf.to(DEV),
                           nplanes=F if form == "bits" else None)
            assert_guards_untouched(full)
            ref = torch.zeros(B, S, S, CP, dtype=F64, device=DEV)
            ref[..., :F] = want.permute(0, 2, 3, 1).double()
            assert_padded_equal(out, ref, halo, "%s halo %d" % (form, halo))
            outs[form] = out
        assert torch.equal(outs["u8"].view(torch.int16), outs["f32"].view(torch.int16))
        assert torch.equal(outs["u8"].view(torch.int16), outs["bits"].view(torch.int16))
    for form in ("u8", "f32"):  # nplanes < F: the leading planes only
        full, out = guarded_output(B, S, 1, CP)
        ops.pack_input(src[form], out, 1, index=index.to(DEV), transforms=tf.to(DEV),
                       nplanes=F - 7)
        ref = torch.zeros(B, S, S, CP, dtype=F64, device=DEV)
        ref[..., :F - 7] = want.permute(0, 2, 3, 1)[..., :F - 7].double()
        assert_padded_equal(out, ref, 1, form + " nplanes")
        assert_guards_untouched(full)


@gpu
@pytest.mark.parametrize("S", [7, 9, 13, 19])
def test_labels_follow_their_planes(ops, S):
    """One position per board point, its plane one-hot at that point and its label that point:
    sl_batch (batch.hip:20-32, with the host label_transform_table) draws a transform per row
    from all eight and returns the moved label; pack_input with the same transforms moves the
    plane (conv.hip:424-437). The packed plane's argmax must be the returned label at all S^2
    points, under every transform."""
    from rocalphago_amd.training.data import label_transform_table
    S2 = S * S
    planes = torch.zeros(S2, 1, S, S, dtype=torch.uint8)
    planes.view(S2, S2)[torch.arange(S2), torch.arange(S2)] = 1
    labels = torch.arange(S2, device=DEV)
    table = torch.from_numpy(label_transform_table(S)).to(DEV)
    sym = torch.arange(8, dtype=torch.int32, device=DEV)
    seen = set()
    for step in range(3):  # ~S^2 / 8 draws per transform and step
        index = torch.arange(S2, device=DEV)
        tf, lab = ops.sl_batch(index, labels, table, sym, seed=5, step=step)
        full, out = guarded_output(S2, S, 1, 32)
        ops.pack_input(planes.to(DEV), out, 1, index=index, transforms=tf)
        got = out[:, 1:-1, 1:-1, 0].reshape(S2, S2).float()
        assert bool((got.sum(-1) == 1).all())
        assert torch.equal(got.argmax(-1), lab), "step %d" % step
        assert_guards_untouched(full)
        seen |= set(tf.cpu().tolist())
    assert seen == set(range(8))
