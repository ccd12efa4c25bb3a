"""The policy head on dense targets (csrc/hip/head.hip policy_head_soft_kernel): Keras
categorical cross-entropy on a dense y_true, in the style of test_head_exact.py, whose operands
(exact logits), guarded buffers and error figures this file reuses.

head_soft_ref is the closed form. With p = softmax(z), m_k = [lo <= p_k <= hi] (the objective's
clamp, per class) and Tm = sum_k t_k m_k:

    loss = -sw sum_k t_k log clamp(p_k),    d_k = (Tm p_k - t_k m_k) sw gscale

(every class, pass included; dz = d + d_pass pass_w). It is tested on the CPU against autograd
through kerasish.categorical_crossentropy, and the kernel against it within 8x the error of its
own float32 evaluation (soft_fp32_figures: computed on the CPU, never taken from the kernel),
capped at the 1e-5 / 1e-4 of the project's other fp32 head kernels. Rows equal to one-hot labels
are held to the label kernel's reference head_fwd_ref within head_bounds().

An all-zero target row has no argmax: its hit is 0 (and its loss and gradients are exactly 0).
"""
import functools

import numpy as np
import pytest
import torch

from test_conv_exact import DEV, assert_guards_untouched, gen
from test_head_exact import (CLIP_HI, CLIP_LO, F64, HEAD_CASES, TIE_A, _ints, _rounded, _rowsum,
                             guarded_rows, head_bounds, head_case, head_errors, head_fwd_ref,
                             head_logits, lowest_argmax, packed_h)

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rocalphago_amd.ops import hipops
    return hipops


# --------------------------------------------------------------------------- the reference

def head_soft_ref(z, t, sw, gscale, pass_w=None, pass_b=None, lo=CLIP_LO, hi=CLIP_HI, dtype=F64):
    """Softmax, per-board loss, hit and d(sum_b gscale loss_b)/d(logits) of the head under
    categorical cross-entropy on dense targets t [B, C], in closed form, evaluated in ``dtype``
    (float64: the reference; float32: the figure, with head_fwd_ref's correctly rounded exp / log
    and term-by-term sums). Returns head_fwd_ref's keys, so that head_errors applies ("clipped"
    is all False: the loss error is relative to the loss)."""
    z = z.to(dtype)
    B, S2 = z.shape
    zz = z
    if pass_w is not None:
        pw = pass_w.to(dtype)
        zz = torch.cat([z, _rowsum(z * pw).unsqueeze(1) + pass_b.to(dtype)], 1)
    t = t.to(dtype)
    assert t.shape == zz.shape
    e = _rounded(torch.exp, zz - zz.max(-1, keepdim=True).values)
    p = e / _rowsum(e).unsqueeze(1)
    m = ((p >= lo) & (p <= hi)).to(dtype)
    sw = torch.ones(B, dtype=dtype, device=z.device) if sw is None else sw.to(dtype)
    loss = -_rowsum(t * _rounded(torch.log, p.clamp(lo, hi))) * sw
    Tm = _rowsum(t * m)
    g = (Tm.unsqueeze(1) * p - t * m) * (sw * gscale).view(B, 1)
    dz = g[:, :S2]
    out = {}
    if pass_w is not None:
        out["dpass"] = g[:, S2]
        dz = dz + g[:, S2:] * pw
    hit = (lowest_argmax(zz) == lowest_argmax(t)) & (t.max(-1).values > 0)
    out.update(probs=p, hit=hit.to(dtype), loss=loss, dz=dz, dzsum=_rowsum(dz), mask=m, Tm=Tm,
               plab=torch.zeros_like(loss), clipped=torch.zeros(B, dtype=torch.bool,
                                                                device=z.device), scale=sw)
    return out


def one_hot(labels, C):
    y = torch.zeros(labels.numel(), C, dtype=F64, device=labels.device)
    y.scatter_(1, labels.view(-1, 1), 1.0)
    return y


# ------------------------------------------------------------- CPU: reference vs autograd

@pytest.mark.parametrize("with_pass", [False, True], ids=["nopass", "pass"])
def test_soft_reference_matches_autograd(with_pass):
    """head_soft_ref against torch.autograd through kerasish.categorical_crossentropy (with its
    y_pred / sum renormalisation) on a 3x3 board, signed sample weights, gscale 0.2. Rows: dense;
    unnormalised (sum 2.5); all zero; two live classes (p ~ 1/2 each, the other classes' p ~
    e^-24 clipped low) with half the target mass on clipped classes: Tm = 0.5, a gradient that
    is neither zero nor the unmasked p sum(t) - t; a row whose one class of any probability is
    clipped high, every other clipped low: exactly zero gradient."""
    from rocalphago_amd.models import kerasish
    B, S2 = 5, 9
    C = S2 + int(with_pass)
    g = gen(77 + int(with_pass))
    z = _ints(g, (B, S2), -64, 64, 1.0 / 64, dev="cpu")
    z[3, 7] += 24.0
    z[3, 2] += 24.0
    z[4, 7] += 24.0
    pass_w = _ints(g, (S2,), -8, 8, 1.0 / 64, dev="cpu") if with_pass else None
    pass_b = _ints(g, (1,), -8, 8, 1.0 / 64, dev="cpu") if with_pass else None
    t = torch.zeros(B, C, dtype=F64)
    t[0] = torch.rand(C, generator=g, dtype=F64)
    t[0] /= t[0].sum()
    t[1, [1, 3, 4, 6, C - 1]] = 0.5
    t[3, [7, 2, 0, 4]] = torch.tensor([0.3, 0.2, 0.25, 0.25], dtype=F64)
    t[4] = t[0]
    sw = torch.tensor([1.5, -0.75, 2.0, 1.25, 0.5], dtype=F64)
    gscale = 0.2
    lo, hi = kerasish.EPSILON, 1.0 - kerasish.EPSILON
    ref = head_soft_ref(z, t, sw, gscale, pass_w, pass_b, lo=lo, hi=hi)
    assert ref["mask"][:2].bool().all() and ref["mask"][3].sum() == 2 and ref["mask"][4].sum() == 0
    assert abs(ref["Tm"][3].item() - 0.5) < 1e-15 and abs(ref["Tm"][1].item() - 2.5) < 1e-15
    zr = z.clone().requires_grad_()
    zz = zr
    if with_pass:
        zp = (zr * pass_w).sum(-1, keepdim=True) + pass_b
        zp.retain_grad()
        zz = torch.cat([zr, zp], 1)
    y_pred = torch.softmax(zz, -1)
    loss = kerasish.categorical_crossentropy(t, y_pred) * sw
    (gscale * loss).sum().backward()
    assert torch.allclose(ref["loss"], loss.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(ref["probs"], y_pred.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(ref["dz"], zr.grad, rtol=1e-11, atol=1e-18)
    if with_pass:
        assert torch.allclose(ref["dpass"], zp.grad.squeeze(1), rtol=1e-11, atol=1e-18)
    # the all-zero row and the fully clipped row: exactly zero, in both
    for r in (2, 4):
        assert bool((zr.grad[r] == 0).all()) and bool((ref["dz"][r] == 0).all())
    assert ref["loss"][2].item() == 0 and ref["hit"][2].item() == 0
    # the partially clipped row: not zero, and not the unmasked formula
    assert zr.grad[3].abs().max().item() > 1e-3
    if not with_pass:
        pz = ref["probs"]
        unmasked = (pz[3] * t[3].sum() - t[3]) * sw[3] * gscale
        assert (zr.grad[3] - unmasked).abs().max().item() > 0.01
        want = (0.5 * pz[3, 7].item() - 0.3) * sw[3].item() * gscale
        assert abs(zr.grad[3, 7].item() - want) < 1e-12
    # a one-hot row reduces to the label reference, clipped boards included
    labels = torch.tensor([0, 4, 1, 7, 7])
    a = head_soft_ref(z, one_hot(labels, C), sw, gscale, pass_w, pass_b, lo=lo, hi=hi)
    b = head_fwd_ref(z, labels, sw, 1, gscale, pass_w, pass_b, lo=lo, hi=hi)
    for k in ("loss", "dz", "hit", "probs"):
        assert torch.allclose(a[k], b[k], rtol=1e-13, atol=1e-18), k
    assert bool((a["dz"][4] == 0).all()) and bool(b["clipped"][4])


# --------------------------------------------------------------------- GPU: the launches

def _visit_row(rng, C, n_classes, with_pass):
    """Counts over ~n_classes random classes (the pass class among them) that sum to 256."""
    k = min(n_classes, C)
    cls = rng.choice(C, size=k, replace=False)
    if with_pass and C - 1 not in cls:
        cls[0] = C - 1
    counts = rng.multinomial(256 - k, np.ones(k) / k) + 1
    row = np.zeros(C)
    row[cls] = counts
    assert row.sum() == 256
    return row / 256.0


@functools.lru_cache(maxsize=None)
def soft_case(name, with_pass, dev=DEV):
    """head_case(name, with_pass) with dense targets: a list of launches
    (tag, pbias, targets [B, C], labels or None, sw, gscale).

    "<launch>/onehot"   head_case's four launches ("clip" among them) with one-hot rows at its
                        labels: labels is given, the reference is head_fwd_ref
    "<launch>/mixA|B"   the three ordinary launches with row b of kind (b + shift) % 4:
                        0 visit-like (counts over ~40 classes, pass included, / 256: exact),
                        1 five classes of 0.5 (sum 2.5), 2 all zero, 3 a target tie between the
                        board's best logit m and another class j (0.375 each, 0.25 elsewhere):
                        j > m on even boards (hit), j < m on odd ones (no hit); shift 0 and 2,
                        so that boards 0 and 1 see every kind
    "partial"           pbias raised by 24 at q1 = TIE_A and q2 = S*S - 5, every row 0.5 on q1
                        and 0.25 on each of two other points (p ~ e^-24: clipped low): Tm = 0.5

    Preconditions (on the float64 reference): every class with t > 0 has p in [1e-6, 1 - 1e-6],
    or below 1e-8, or above 1 - 3e-8: fp32 cannot flip a mask; every target is exact in fp32."""
    c = head_case(name, with_pass, "cpu")
    S, B, C = c["S"], c["B"], c["C"]
    S2 = S * S
    rng = np.random.RandomState(9000 + 10 * list(HEAD_CASES).index(name) + int(with_pass))
    launches = []
    for tag, pb, lab, sw, gs in c["launches"]:
        launches.append((tag + "/onehot", pb, one_hot(lab, C), lab, sw, gs))
    base_pb = c["launches"][0][1]
    z = head_logits(c["H"], c["w"], c["b0"], base_pb)
    zz = z if not with_pass else torch.cat(
        [z, (z * c["pass_w"]).sum(-1, keepdim=True) + c["pass_b"]], 1)
    best = lowest_argmax(zz).tolist()
    mixes = {}
    for shift, mix in ((0, "mixA"), (2, "mixB")):
        t = np.zeros((B, C))
        for b in range(B):
            kind = (b + shift) % 4
            if kind == 0:
                t[b] = _visit_row(rng, C, 40, with_pass)
            elif kind == 1:
                t[b, rng.choice(C, size=5, replace=False)] = 0.5
            elif kind == 3:
                m = best[b]
                j = m + 7 if m + 7 < C and (b % 2 == 0 or m == 0) else m - 1
                other = (m + 20) % S2
                assert len({m, j, other}) == 3 and j < C
                t[b, [m, j]] = 0.375
                t[b, other] = 0.25
        mixes[mix] = torch.from_numpy(t)
    for tag, pb, _, sw, gs in c["launches"][:3]:
        for mix, t in mixes.items():
            launches.append(("%s/%s" % (tag, mix), pb, t, None, sw, gs))
    q1, q2 = TIE_A, S2 - 5
    pp = base_pb.clone()
    pp[q1] += 24.0
    pp[q2] += 24.0
    t = torch.zeros(B, C, dtype=F64)
    t[:, q1] = 0.5
    t[:, [q1 + 2, q2 - 2]] = 0.25
    launches.append(("partial", pp, t, None, c["launches"][2][3], c["launches"][2][4]))
    for tag, pb, t, lab, _, _ in launches:
        zl = head_logits(c["H"], c["w"], c["b0"], pb)
        if with_pass:
            assert ((zl.abs() * c["pass_w"].abs()).sum(-1).max().item()
                    + c["pass_b"].abs().item()) * 4096 < 2 ** 24
        assert torch.equal(t.float().double(), t), "targets not exact in float32"
        p = head_soft_ref(zl, t, None, 1.0, c["pass_w"], c["pass_b"])["probs"][t > 0]
        ok = ((p >= 1e-6) & (p <= 1 - 1e-6)) | (p < 1e-8) | (p > 1 - 3e-8)
        assert bool(ok.all()), (name, with_pass, tag, p[~ok])
        if tag == "partial":
            r = head_soft_ref(zl, t, None, 1.0, c["pass_w"], c["pass_b"])
            assert bool((r["Tm"] == 0.5).all()) and r["dz"].abs().max().item() > 0.1

    def mv(v):
        return v.to(dev) if torch.is_tensor(v) else v

    out = {k: mv(v) for k, v in c.items() if k != "launches"}
    out["launches"] = [tuple(mv(v) for v in ln) for ln in launches]
    return out


def soft_reference(c, ln, dtype=F64):
    """The reference of one launch: head_fwd_ref for one-hot rows, head_soft_ref otherwise."""
    _, pb, t, lab, sw, gs = ln
    z = head_logits(c["H"], c["w"], c["b0"], pb)
    if lab is not None and dtype == F64:
        return z, head_fwd_ref(z, lab, sw, 1, gs, c["pass_w"], c["pass_b"])
    return z, head_soft_ref(z, t, sw, gs, c["pass_w"], c["pass_b"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def soft_fp32_figures():
    """The largest head_errors of head_soft_ref evaluated in float32 on the CPU against its
    float64 self over every case, pass form and launch of this file."""
    val = grad = 0.0
    for name in HEAD_CASES:
        for with_pass in (False, True):
            c = soft_case(name, with_pass, "cpu")
            for ln in c["launches"]:
                z = head_logits(c["H"], c["w"], c["b0"], ln[1])
                ref = head_soft_ref(z, ln[2], ln[4], ln[5], c["pass_w"], c["pass_b"])
                f32 = head_soft_ref(z, ln[2], ln[4], ln[5], c["pass_w"], c["pass_b"],
                                    dtype=torch.float32)
                e = head_errors(ref, f32)
                val, grad = max(val, e["val"]), max(grad, e["grad"])
    return val, grad


def soft_bounds():
    """(values, gradients): head_bounds()'s recipe on this file's figures."""
    val, grad = soft_fp32_figures()
    return min(8 * val, 1e-5), min(8 * grad, 1e-4)


def test_soft_fp32_reference_error_keeps_the_bound_below_the_cap():
    val, grad = soft_fp32_figures()
    print("float32 soft reference error: values %.3g, gradients %.3g -> bounds %.3g, %.3g" %
          ((val, grad) + soft_bounds()))
    assert 0 < val < 1e-6 and 0 < grad < 1e-6
    assert soft_bounds() == (8 * val, 8 * grad)


def launch_policy_head_soft(ops, c, hp, pbias, targets, sw, gscale, with_dzsum=True):
    """One policy_head_soft launch into NaN-filled buffers between guard rows."""
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

    ops.policy_head_soft(hp, f32(c["w"]), f32(c["b0"]), f32(pbias), out["probs"], c["K"],
                         f32(targets), sweight=f32(sw), loss=flat("loss"), dz=out["dz"],
                         hit=flat("hit"), gscale=gscale, pass_w=f32(c["pass_w"]),
                         pass_b=f32(c["pass_b"]), zout=out.get("zout"), dpass=flat("dpass"),
                         dzsum=flat("dzsum"))
    for k in ("loss", "hit", "dpass", "dzsum"):
        if k in out:
            out[k] = out[k].view(B)
    return out, [v[0] for v in bufs.values()]


@gpu
@pytest.mark.parametrize("with_pass", [False, True], ids=["nopass", "pass"])
@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_policy_head_soft(ops, name, with_pass):
    """policy_head_soft_kernel on soft_case's launches: zout bit-equal to the float64 logits;
    probabilities, loss, dz / dpass, dzsum within the bounds of the reference (head_fwd_ref and
    head_bounds for one-hot rows, head_soft_ref and soft_bounds otherwise); hits equal; boards
    with a zero reference gradient (zero weight, all-zero row, every board of the clip launch)
    exactly zero; guards untouched."""
    c = soft_case(name, with_pass)
    hp = packed_h(c["H"], c["KP"])
    for ln in c["launches"]:
        tag, pbias, t, lab, sw, gscale = ln
        z, ref = soft_reference(c, ln)
        bval, bgrad = head_bounds() if lab is not None else soft_bounds()
        got, fulls = launch_policy_head_soft(ops, c, hp, pbias, t, sw, gscale)
        for full in fulls:
            assert_guards_untouched(full)
        what = "%s %s %s" % (name, "pass" if with_pass else "nopass", tag)
        if with_pass:
            assert torch.equal(got["zout"], z.float()), what
        for k, v in got.items():
            assert not bool(torch.isnan(v).any()), what + ": NaN in " + k
        err = head_errors(ref, got)
        print("%s: values %.3g (bound %.3g), gradients %.3g (bound %.3g)" %
              (what, err["val"], bval, err["grad"], bgrad))
        assert err["val"] <= bval and err["grad"] <= bgrad, (what, err)
        assert torch.equal(got["hit"].double(), ref["hit"]), what
        zero = ref["dz"].abs().max(-1).values == 0
        if with_pass:
            zero &= ref["dpass"] == 0
        if tag.startswith("clip"):
            assert bool(zero.all())
        for k in ("dz", "dpass", "dzsum"):
            if k in got:
                assert bool((got[k][zero] == 0).all()), what + ": " + k
        allzero = t.sum(-1) == 0
        assert bool((got["loss"][allzero] == 0).all()) and bool((got["hit"][allzero] == 0).all())


@gpu
def test_policy_head_soft_without_optional_outputs(ops):
    """dzsum = null: the other outputs are unchanged (bit for bit)."""
    c = soft_case("s9_k32_b4", False)
    hp = packed_h(c["H"], c["KP"])
    _, pbias, t, _, sw, gscale = c["launches"][4]
    a, _ = launch_policy_head_soft(ops, c, hp, pbias, t, sw, gscale)
    b, _ = launch_policy_head_soft(ops, c, hp, pbias, t, sw, gscale, with_dzsum=False)
    for k in ("probs", "dz", "loss", "hit"):
        assert torch.equal(a[k], b[k]), k


@gpu
def test_policy_head_soft_wrapper_checks(ops):
    """dzsum has no pass-logit form; targets must be fp32 [B, C]."""
    c = soft_case("s9_k32_b4", True)
    _, pbias, t, _, _, _ = c["launches"][0]
    B, S2 = c["B"], c["S"] ** 2
    hp = packed_h(c["H"], c["KP"])
    kw = dict(dz=torch.empty(B, S2, device=DEV), pass_w=c["pass_w"].float(),
              pass_b=c["pass_b"].float(), zout=torch.empty(B, S2, device=DEV),
              dpass=torch.empty(B, device=DEV))
    args = (hp, c["w"].float(), c["b0"].float(), pbias.float(),
            torch.empty(B, S2 + 1, device=DEV), c["K"])
    with pytest.raises(ValueError):
        ops.policy_head_soft(*args, t.float(), dzsum=torch.empty(B, device=DEV), **kw)
    with pytest.raises(ValueError):  # the no-pass width
        ops.policy_head_soft(*args, t.float()[:, :S2].contiguous(), **kw)
    with pytest.raises(ValueError):  # one board short
        ops.policy_head_soft(*args, t.float()[:B - 1].contiguous(), **kw)
    with pytest.raises(ValueError):  # float64
        ops.policy_head_soft(*args, t, **kw)
    ops.policy_head_soft(*args, t.float(), **kw)
    torch.cuda.synchronize()
