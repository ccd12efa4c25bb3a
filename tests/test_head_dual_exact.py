"""Exact tests of the policy-value network's two head kernels (csrc/hip/head.hip): the dual
head forward (ops.policy_head_dual: the DUAL forms of policy_head_fwd_kernel and
policy_head_soft_kernel) and the two-head backward (ops.head_bwd2: head_bwd2_kernel<CH> +
head_bwd_reduce_kernel<true>), in the style of test_head_exact.py, whose operands, guarded
buffers and bounds this file reuses.

Operands: H in {0, 1, 2}, both heads' weights and biases multiples of 1/64 in [-8/64, 8/64], both
dz integers in [-2, 2]; the second head's come from head_operands with another seed. Then
dzp wp + dzv wv is an integer number of 1/64 granules of magnitude <= 32: exact in fp32 in any
order and exact in bf16, so dH, dwp, dwv, dpbias, db0p and db0v must EQUAL the float64 reference
(test_multi_output.head_bwd2_ref, itself checked against autograd on the CPU) cast to the
output type, and the value logits zv must be bit-equal to head_logits(H, wv, b0v).

The policy outputs of the dual forward are held to what the single-head tests hold theirs to
(head_bounds() against head_fwd_ref for labels and one-hot rows, soft_bounds() against
head_soft_ref for dense rows, as test_policy_head_soft), and, the logits being exact and the
rest the same code on the same inputs, to bit-identity with the single-head kernels."""
import pytest
import torch

from test_conv_exact import DEV, NAN, assert_guards_untouched, gen, guarded_output, ints
from test_head_exact import (F64, HEAD_BWD_CASES, HEAD_CASES, assert_padded_equal, guarded_rows,
                             head_bounds, head_case, head_errors, head_fwd_ref, head_logits,
                             head_operands, launch_policy_head, packed_h)
from test_head_soft import (launch_policy_head_soft, soft_bounds, soft_case, soft_reference)
from test_multi_output import head_bwd2_ref

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rocalphago_amd.ops import hipops
    return hipops


def f32(t):
    return None if t is None else t.float().contiguous()


# ------------------------------------------------------------------- head_bwd2, bit-exact

def run_head_bwd2(ops, S, K, KP, B, seed, relu_mask=True, from_dzsum=False, unaligned=False,
                  metrics=False, wv_kernel=None, degenerate=False):
    """One head_bwd2 launch against head_bwd2_ref: dH, dwp, dwv, dpbias, db0p, db0v equal the
    float64 values, both dw past K untouched (NaN), dH's padded channels and halo zero, guard
    boards untouched. Returns (dH view, operands, outputs)."""
    H, wp, _, dzp = head_operands(seed, S, K, B)
    _, wv, _, dzv = head_operands(seed + 500, S, K, B)
    if degenerate:
        wv, dzv = torch.zeros_like(wv), torch.zeros_like(dzv)
    S2 = S * S
    ref_dh, ref_dwp, ref_dwv, ref_dpb, ref_db0p, ref_db0v = head_bwd2_ref(H, wp, wv, dzp, dzv,
                                                                          relu_mask)
    hp = packed_h(H, KP)
    dzvk = f32(dzv)
    if unaligned:  # a contiguous view one float into its storage: not 16-byte aligned
        store = torch.full((B * S2 + 1,), NAN, device=DEV)
        dzvk = store[1:].view(B, S2)
        dzvk.copy_(dzv)
        assert dzvk.is_contiguous() and dzvk.data_ptr() % 16 == 4 and (B * S2) % 4
    full, dh = guarded_output(B, S, 1, KP)
    dwp = torch.full((KP,), NAN, device=DEV)
    dwv = torch.full((KP,), NAN, device=DEV)
    db0p = torch.full((1,), NAN, device=DEV)
    db0v = torch.full((1,), NAN, device=DEV)
    dpb = torch.full((S2,), NAN, device=DEV)
    dzsum = m = None
    if from_dzsum:  # deliberately not the row sums of dzp: db0p must come from here
        dzsum = ints(gen(seed + 1), (B,), -3, 3).float()
        ref_db0p = dzsum.double().sum()
        assert ref_db0p.item() != dzp.sum().item()
    if metrics:
        g = gen(seed + 2)
        m = (ints(g, (B,), 0, 5).float(), ints(g, (B,), 0, 1).float(),
             torch.tensor([3.0, 5.0], device=DEV))
    wvk = wv if wv_kernel is None else wv_kernel
    ops.head_bwd2(hp, f32(wp), f32(wvk), f32(dzp), dzvk, dh, dwp, dwv, db0p, db0v, dpb, K,
                  relu_mask=relu_mask, metrics=m, dzsum=dzsum)
    assert torch.equal(dwp[:K], ref_dwp.float()), "dwp"
    assert torch.equal(dwv[:K], ref_dwv.float()), "dwv"
    assert bool(torch.isnan(dwp[K:]).all()) and bool(torch.isnan(dwv[K:]).all()), \
        "dw past K was written"
    assert torch.equal(db0p, ref_db0p.float().view(1)), (db0p.item(), ref_db0p.item())
    assert torch.equal(db0v, ref_db0v.float().view(1)), (db0v.item(), ref_db0v.item())
    assert torch.equal(dpb, ref_dpb.float()), "dpbias"
    if metrics:
        want = torch.stack([3.0 + m[0].double().sum(), 5.0 + m[1].double().sum()]).float()
        assert torch.equal(m[2], want), (m[2].tolist(), want.tolist())
    if wv_kernel is None:
        padded = torch.zeros(B, S, S, KP, dtype=F64, device=DEV)
        padded[..., :K] = ref_dh
        assert_padded_equal(dh, padded, 1, "dH")
    assert_guards_untouched(full)
    return dh, (H, wp, wv, dzp, dzv), dict(dwp=dwp, dwv=dwv, db0p=db0p, db0v=db0v, dpb=dpb)


# id: (S, K, KP, B, options of run_head_bwd2): HEAD_BWD_CASES' shapes, each the smallest that
# reaches its branch (test_head_bwd_exact's docstring names the branches)
HEAD_BWD2_CASES = dict(
    [(name, HEAD_BWD_CASES[name][:4] + ({},)) for name in
     ["kp%d" % kp for kp in (32, 64, 96, 128, 192, 256, 384, 512)] +
     ["k59_in_kp64", "k187_in_kp192", "one_7x7_board", "block_cap_b35"]] + [
        ("b1030_dzsum_metrics", (9, 32, 32, 1030, dict(from_dzsum=True, metrics=True))),
        ("no_relu_mask", (9, 64, 64, 3, dict(relu_mask=False))),
        ("db0p_from_dzsum", (9, 64, 64, 7, dict(from_dzsum=True))),
        ("unaligned_dzv", (19, 64, 64, 7, dict(unaligned=True))),
    ])


def test_head_bwd2_cases_mirror_head_bwd():
    """The shapes are HEAD_BWD_CASES' own (not marked gpu: a table check)."""
    assert HEAD_BWD2_CASES["k59_in_kp64"][:4] == (9, 59, 64, 3)
    assert HEAD_BWD2_CASES["k187_in_kp192"][:4] == (9, 187, 192, 3)
    assert HEAD_BWD2_CASES["one_7x7_board"][:4] == (7, 64, 64, 1)
    assert HEAD_BWD2_CASES["block_cap_b35"][:4] == (19, 192, 192, 35)
    for kp in (32, 64, 96, 128, 192, 256, 384, 512):
        assert HEAD_BWD2_CASES["kp%d" % kp][:4] == (9, kp, kp, 3)


@gpu
@pytest.mark.parametrize("name", list(HEAD_BWD2_CASES))
def test_head_bwd2_exact(ops, name):
    """head_bwd2_kernel<CH> + head_bwd_reduce_kernel<true> against head_bwd2_ref:

    kp32 .. kp512    each head_bwd2_kernel<CH>, CH = KP / 8, K = KP, B = 3 at 9x9
    k59_in_kp64, k187_in_kp192   K = KP - 5 with 1.0 in the input's padded channels: both heads'
                     weights past K are zero in LDS, so dH[..., K:] is zero, and the reduce writes
                     dwp[:K], dwv[:K] only: both dw past K stay NaN
    one_7x7_board    B = 1 at 7x7: 49 pixels in two blocks
    block_cap_b35    B = 35 at 19x19, KP = 192: the block cap holds, the last blocks are empty and
                     still write zero partials of both heads
    b1030_dzsum_metrics   B = 1030 at 9x9: the dpbias columns sum 1030 rows, the last reduce
                     block's loops over dzsum, the metrics and dzv take further trips
    no_relu_mask     relu_mask = 0: dH = dzp wp + dzv wv also where H is zero
    db0p_from_dzsum  db0p is the sum of dzsum, a vector that is not the row sums of dzp; db0v
                     still the sum of dzv
    unaligned_dzv    dzv one float into its storage at 19x19, B = 7 (B S^2 = 2527): db0v's
                     16-byte sum falls back to scalar loads"""
    S, K, KP, B, opts = HEAD_BWD2_CASES[name]
    run_head_bwd2(ops, S, K, KP, B, seed=6500 + list(HEAD_BWD2_CASES).index(name), **opts)


@gpu
def test_head_bwd2_degenerate_equals_head_bwd(ops):
    """wv = 0 and dzv = 0: every output equals ops.head_bwd's on the same operands (values:
    a zero product may be -0.0 in one and +0.0 in the other)."""
    S, K, KP, B, seed = 9, 59, 64, 5, 6600
    dh2, (H, wp, _, dzp, _), out = run_head_bwd2(ops, S, K, KP, B, seed, degenerate=True)
    full, dh = guarded_output(B, S, 1, KP)
    dw = torch.full((KP,), NAN, device=DEV)
    db0 = torch.full((1,), NAN, device=DEV)
    dpb = torch.full((S * S,), NAN, device=DEV)
    ops.head_bwd(packed_h(H, KP), f32(wp), f32(dzp), dh, dw, db0, dpb, K)
    assert torch.equal(dh2.float(), dh.float())
    assert torch.equal(out["dwp"][:K], dw[:K]) and torch.equal(out["db0p"], db0)
    assert torch.equal(out["dpb"], dpb)
    assert bool((out["dwv"][:K] == 0).all()) and out["db0v"].item() == 0


@gpu
def test_head_bwd2_comparator_sees_one_wrong_value_weight(ops):
    """Self-check of the comparison: wv[k] raised by 1/64 on the kernel's side only changes dH
    exactly at channel k where dzv != 0 and H > 0 (a share between 0.3 and 0.7), and leaves
    dwp, dwv, dpbias, db0p, db0v (asserted in run_head_bwd2) unchanged."""
    S, K, B, k = 9, 64, 3, 37
    H, _, _, _ = head_operands(6990, S, K, B)
    _, wv, _, dzv = head_operands(6990 + 500, S, K, B)
    wv_bad = wv.clone()
    wv_bad[k] += 1.0 / 64
    dh, _, _ = run_head_bwd2(ops, S, K, K, B, seed=6990, wv_kernel=wv_bad)
    good, _, _ = run_head_bwd2(ops, S, K, K, B, seed=6990)
    differs = dh[:, 1:-1, 1:-1, :].float() != good[:, 1:-1, 1:-1, :].float()
    want = torch.zeros_like(differs)
    want[..., k] = (dzv.view(B, S, S) != 0) & (H[..., k] > 0)
    assert 0.3 < want[..., k].double().mean().item() < 0.7
    assert torch.equal(differs, want)


@gpu
def test_head_bwd2_wrapper_checks(ops):
    S, K, B = 9, 32, 2
    H, wp, _, dzp = head_operands(6700, S, K, B)
    hp = packed_h(H, K)
    o = [torch.empty(K, device=DEV), torch.empty(K, device=DEV), torch.empty(1, device=DEV),
         torch.empty(1, device=DEV)]
    with pytest.raises(ValueError):  # float64 dz
        ops.head_bwd2(hp, f32(wp), f32(wp), dzp, f32(dzp), None, *o, None, K)
    with pytest.raises(ValueError):  # a workspace that is too small
        ops.head_bwd2(hp, f32(wp), f32(wp), f32(dzp), f32(dzp), None, *o, None, K,
                      work=torch.empty(8, device=DEV))
    ops.head_bwd2(hp, f32(wp), f32(wp), f32(dzp), f32(dzp), None, *o, None, K)  # null dH, dpbias
    torch.cuda.synchronize()
    assert torch.equal(o[0], o[1]) and torch.equal(o[2], o[3])


# ------------------------------------------------------------------------ the dual forward

def second_head(c, seed):
    """The value head's (wv [K], b0v [1]) for a head_case / soft_case, another seed's draw."""
    _, wv, b0v, _ = head_operands(seed, c["S"], c["K"], 1)
    return wv, b0v


def launch_dual(ops, c, hp, wv, b0v, pbias, labels, targets, sw, gscale, mode):
    """One policy_head_dual launch into NaN-filled buffers between guard rows."""
    B, S2 = c["B"], c["S"] ** 2
    bufs = {k: guarded_rows(B, n) for k, n in (("probs", S2), ("dz", S2), ("loss", 1),
                                               ("hit", 1), ("dzsum", 1), ("zv", S2))}
    out = {k: v[1] for k, v in bufs.items()}
    ops.policy_head_dual(hp, f32(c["w"]), f32(c["b0"]), f32(pbias), f32(wv), f32(b0v),
                         out["probs"], out["zv"], c["K"], labels=labels, targets=f32(targets),
                         sweight=f32(sw), loss=out["loss"].view(B), dz=out["dz"],
                         hit=out["hit"].view(B), mode=mode, gscale=gscale,
                         dzsum=out["dzsum"].view(B))
    for k in ("loss", "hit", "dzsum"):
        out[k] = out[k].view(B)
    return out, [v[0] for v in bufs.values()]


def check_dual(what, got, fulls, single, ref, zv_ref, bounds, mode):
    for full in fulls:
        assert_guards_untouched(full)
    assert torch.equal(got["zv"], zv_ref.float()), what + ": zv"
    assert not bool(torch.isnan(got["probs"]).any()), what
    keys = ("probs",) if mode == 0 else ("probs", "loss", "dz", "hit", "dzsum")
    if mode == 0:
        for k in ("loss", "dz", "hit", "dzsum"):
            assert bool(torch.isnan(got[k]).all()), what + ": wrote " + k
    err = head_errors(ref, got if mode else {"probs": got["probs"]})
    print("%s: values %.3g (bound %.3g), gradients %.3g (bound %.3g)" %
          (what, err["val"], bounds[0], err["grad"], bounds[1]))
    assert err["val"] <= bounds[0] and err["grad"] <= bounds[1], (what, err)
    if mode:
        assert torch.equal(got["hit"].double(), ref["hit"]), what
    for k in keys:  # the same code on the same (exact) logits as the single-head kernel
        assert torch.equal(got[k].view(torch.int32), single[k].view(torch.int32)), \
            "%s: %s differs from the single-head kernel" % (what, k)


@gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_dual_head_fwd_labels(ops, name, mode):
    """policy_head_fwd_kernel<true> on head_case's four launches (no pass logit), modes 0, 1, 2:
    zv bit-equal to the float64 value logits, guard rows untouched, the policy outputs within
    head_bounds of head_fwd_ref, hits equal, mode 0 writes probs and zv only, and every policy
    output bit-identical to policy_head_fwd's."""
    c = head_case(name, False)
    hp = packed_h(c["H"], c["KP"])
    wv, b0v = second_head(c, 7500 + list(HEAD_CASES).index(name))
    zv_ref = head_logits(c["H"], wv, b0v)
    for tag, pbias, labels, sw, gscale in c["launches"]:
        z = head_logits(c["H"], c["w"], c["b0"], pbias)
        ref = head_fwd_ref(z, labels, sw, mode, gscale)
        got, fulls = launch_dual(ops, c, hp, wv, b0v, pbias, labels, None, sw, gscale, mode)
        single, _ = launch_policy_head(ops, c, hp, pbias, labels, sw, gscale, mode)
        check_dual("%s mode %d %s" % (name, mode, tag), got, fulls, single, ref, zv_ref,
                   head_bounds(), mode)
        if mode and tag == "clip":
            assert bool((got["dz"] == 0).all()) and bool((got["dzsum"] == 0).all())


@gpu
@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_dual_head_fwd_dense_targets(ops, name):
    """policy_head_soft_kernel<true> on soft_case's launches (no pass logit), as
    test_policy_head_soft holds the single head: head_fwd_ref / head_bounds for one-hot rows,
    head_soft_ref / soft_bounds otherwise; bit-identical to policy_head_soft; zv exact."""
    c = soft_case(name, False)
    hp = packed_h(c["H"], c["KP"])
    wv, b0v = second_head(c, 7600 + list(HEAD_CASES).index(name))
    zv_ref = head_logits(c["H"], wv, b0v)
    for ln in c["launches"]:
        tag, pbias, t, lab, sw, gscale = ln
        _, ref = soft_reference(c, ln)
        got, fulls = launch_dual(ops, c, hp, wv, b0v, pbias, None, t, sw, gscale, 1)
        single, _ = launch_policy_head_soft(ops, c, hp, pbias, t, sw, gscale)
        check_dual("%s soft %s" % (name, tag), got, fulls, single, ref, zv_ref,
                   head_bounds() if lab is not None else soft_bounds(), 1)
        zero = ref["dz"].abs().max(-1).values == 0
        assert bool((got["dz"][zero] == 0).all()) and bool((got["dzsum"][zero] == 0).all())


def extra_case(S, K, KP, B, seed):
    """A plain case outside HEAD_CASES: random labels, pbias in 1/64 steps, one launch."""
    H, w, b0, _ = head_operands(seed, S, K, B)
    g = gen(seed + 5)
    pbias = ints(g, (S * S,), -8, 8, 1.0 / 64)
    labels = torch.randint(0, S * S, (B,), generator=g).to(DEV)
    return dict(S=S, K=K, KP=KP, B=B, C=S * S, H=H, w=w, b0=b0, pass_w=None, pass_b=None), \
        pbias, labels


@gpu
@pytest.mark.parametrize("S,K,KP,B", [(9, 59, 64, 3), (7, 32, 32, 2)],
                         ids=["k59_in_kp64", "one_7x7"])
def test_dual_head_fwd_extra_shapes(ops, S, K, KP, B):
    """K < KP (1.0 in the padded channels must reach neither head) and a 7x7 board: modes 0 and
    1 with labels, and mode 1 with the labels' one-hot rows as dense targets."""
    c, pbias, labels = extra_case(S, K, KP, B, 7700 + S)
    hp = packed_h(c["H"], KP)
    wv, b0v = second_head(c, 7750 + S)
    zv_ref = head_logits(c["H"], wv, b0v)
    z = head_logits(c["H"], c["w"], c["b0"], pbias)
    gscale = 1.0 / B
    for mode in (0, 1):
        ref = head_fwd_ref(z, labels, None, mode, gscale)
        got, fulls = launch_dual(ops, c, hp, wv, b0v, pbias, labels, None, None, gscale, mode)
        single, _ = launch_policy_head(ops, c, hp, pbias, labels, None, gscale, mode)
        check_dual("S%d K%d mode %d" % (S, K, mode), got, fulls, single, ref, zv_ref,
                   head_bounds(), mode)
    t = torch.zeros(B, S * S, dtype=F64, device=DEV)
    t.scatter_(1, labels.view(-1, 1), 1.0)
    ref = head_fwd_ref(z, labels, None, 1, gscale)
    got, fulls = launch_dual(ops, c, hp, wv, b0v, pbias, None, t, None, gscale, 1)
    single, _ = launch_policy_head_soft(ops, c, hp, pbias, t, None, gscale)
    check_dual("S%d K%d soft" % (S, K), got, fulls, single, ref, zv_ref, head_bounds(), 1)


@gpu
def test_policy_head_dual_wrapper_checks(ops):
    c, pbias, labels = extra_case(7, 32, 32, 2, 7800)
    hp = packed_h(c["H"], 32)
    wv, b0v = second_head(c, 7801)
    B, S2 = 2, 49
    probs, zv = torch.empty(B, S2, device=DEV), torch.empty(B, S2, device=DEV)
    args = (hp, f32(c["w"]), f32(c["b0"]), f32(pbias), f32(wv), f32(b0v), probs)
    t = torch.zeros(B, S2, device=DEV)
    with pytest.raises(ValueError):  # targets exclude labels
        ops.policy_head_dual(*args, zv, 32, labels=labels, targets=t, mode=1)
    with pytest.raises(ValueError):  # targets need mode 1
        ops.policy_head_dual(*args, zv, 32, targets=t, mode=2)
    with pytest.raises(ValueError):  # zv of the wrong shape
        ops.policy_head_dual(*args, zv[:1], 32)
    ops.policy_head_dual(*args, zv, 32)
    torch.cuda.synchronize()
    assert torch.equal(zv, head_logits(c["H"], wv, b0v).float())
