"""ResnetPolicyValue on the fused HIP plan (models/fused.py ResnetDualPlan): the raw-top head
kernels bit for bit against the existing ones on a materialised ReLU, detection, the forward
against ResnetPlan and float64 heads, the head gradients against fp32 autograd on the same trunk
output, the whole step against the CPU generic executor, the trainer and the search's wave path.
Bounds: those of tests/test_dual_plan_gpu.py and tests/test_resnet_gpu.py, as named per test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rocalphago_amd.features.preprocessing import DEFAULT_FEATURES
from rocalphago_amd.models import kerasish as K
from rocalphago_amd.models.policy import ResnetPolicy
from rocalphago_amd.models.policy_value import ResnetPolicyValue
from test_soft_training import soft_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(board=9, filters_per_layer=32, layers=4, n_skip_1=2)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rocalphago_amd.ops import hipops
    return hipops


@pytest.fixture(params=[True, False], ids=["raw_top", "materialised"])
def raw_top(request, monkeypatch):
    from rocalphago_amd.models.fused import ResnetDualPlan
    monkeypatch.setattr(ResnetDualPlan, "RAW_TOP", request.param)
    return request.param


def planes(rng, B, S, F=48):
    return (rng.rand(B, F, S, S) > 0.6).astype(np.float32)


def one_hot_rows(rng, B, C):
    Y = np.zeros((B, C), np.float32)
    Y[np.arange(B), rng.randint(0, C, B)] = 1
    return Y


def randomised(model, seed):
    """tests/test_resnet_gpu.py::_pair's recipe for the BN parameters, the running statistics
    and the Bias, and noise on every conv / Dense bias and on both heads' weights (zero biases
    would hide a mixed-up head)."""
    rng = np.random.RandomState(seed)
    names = model.net.weight_names
    first_head = next(i for i, (_, wn, _) in enumerate(names) if wn == "param_0") - 2
    ws = []
    for i, ((lname, wname, shape), v) in enumerate(zip(names, model.get_weights())):
        if "running_std" in wname:
            v = (rng.rand(*shape) * 2 + 0.5).astype(np.float32)
        elif "running_mean" in wname or "beta" in wname:
            v = (rng.randn(*shape) * 0.1).astype(np.float32)
        elif "gamma" in wname:
            v = (rng.rand(*shape) + 0.5).astype(np.float32)
        elif "param_0" in wname:
            v = (rng.randn(*shape) * 0.1).astype(np.float32)
        elif wname.endswith("_b") or i >= first_head:
            v = v + rng.uniform(-0.05, 0.05, shape).astype(np.float32)
        ws.append(v)
    return ws


def n_policy_weights(model):
    """Weight arrays of the trunk and the policy branch (a ResnetPolicy's)."""
    return next(i for i, (_, wn, _) in enumerate(model.net.weight_names) if wn == "param_0") + 1


# ------------------------------------------------------------------ 1. the raw heads, exact

def raw_operands(ops, B, S, K, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(B, K, S, S, generator=g).to(torch.bfloat16)
    A[torch.rand(A.shape, generator=g) < 0.05] = 0.0
    A[0, 0, 0, 0] = -0.0
    A[-1, K - 1, S - 1, S - 1] = -0.0
    A = A.cuda()
    KP = ops.pad_channels(K)
    Ap = ops.pack_nchw(A.float(), 1, KP)
    assert torch.equal(ops.unpack(Ap, K, 1), A.float())
    Hp = ops.alloc_padded(B, S, 1, KP, "cuda")
    ops.bn_apply(Ap, Hp, B, S, K, coef=None, relu=True)
    assert torch.equal(ops.unpack(Hp, K, 1), torch.relu(A.float()))
    frac = float((A.float() < 0).float().mean())
    assert 0.4 < frac < 0.55 and int((A == 0).sum()) > 2

    def r(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).cuda()
    par = dict(w=r(K, scale=0.2), b0=r(1), pb=r(S * S, scale=0.3), wv=r(K, scale=0.2), b0v=r(1))
    return A, Ap, Hp, KP, par, g


@pytest.mark.parametrize("B,S,K", [(3, 9, 40), (2, 19, 128), (5, 13, 192)])
def test_raw_heads_equal_the_heads_on_a_materialised_relu(ops, B, S, K):
    """relu_in=True on A against the existing entry points on ReLU(A) written by bn_apply:
    torch.equal on every output of the dual forward (inference, labels, dense targets) and of
    head_bwd2. ReLU of a bf16 value is exact and the kernels do the same fp32 operations in the
    same order, so nothing short of identity is expected. Anchors that do not involve the old
    kernels: zv against float64 relu(A) . wv + b0v (1e-5 of the largest value: fp32 sums of
    K <= 192 products), and dH exactly zero wherever A <= 0."""
    A, Ap, Hp, KP, par, g = raw_operands(ops, B, S, K, 8100 + K)
    assert (KP > K) == (K == 40)
    S2 = S * S
    labels = torch.randint(0, S2, (B,), generator=g).cuda()
    targets = torch.from_numpy(soft_rows(np.random.RandomState(K), B, S2)).cuda()
    sw = (torch.rand(B, generator=g) + 0.5).cuda()

    def fwd(h, relu_in, **kw):
        out = dict(probs=torch.zeros(B, S2, device="cuda"), zv=torch.zeros(B, S2, device="cuda"))
        tr = {}
        if kw.get("mode"):
            tr = dict(loss=torch.zeros(B, device="cuda"), dz=torch.zeros(B, S2, device="cuda"),
                      hit=torch.zeros(B, device="cuda"), dzsum=torch.zeros(B, device="cuda"))
        ops.policy_head_dual(h, par["w"], par["b0"], par["pb"], par["wv"], par["b0v"],
                             out["probs"], out["zv"], K, relu_in=relu_in, **tr, **kw)
        out.update(tr)
        return out

    cases = {"inference": {}, "labels": dict(labels=labels, mode=1, gscale=1.0 / B, sweight=sw),
             "dense": dict(targets=targets, mode=1, gscale=1.0 / B)}
    kept = None
    for name, kw in cases.items():
        raw, mat = fwd(Ap, True, **kw), fwd(Hp, False, **kw)
        for k in raw:
            assert torch.equal(raw[k], mat[k]), (name, k)
        assert float(raw["probs"].sum(1).sub(1).abs().max()) < 1e-5
        if name == "dense":
            kept = raw
    ref = (torch.relu(A.double()) * par["wv"].double().view(1, K, 1, 1)).sum(1).reshape(B, S2) \
        + par["b0v"].double()
    err = float((kept["zv"].double() - ref).abs().max()) / float(ref.abs().max())
    print("zv against float64: %.3g" % err)
    assert err <= 1e-5

    dzv = (torch.randn(B, S2, generator=g) * 0.1).cuda()
    acc0 = torch.tensor([3.0, 5.0], device="cuda")

    def bwd(h, relu_in):
        o = dict(dH=torch.zeros_like(Ap), dwp=torch.zeros(KP, device="cuda"),
                 dwv=torch.zeros(KP, device="cuda"), db0p=torch.zeros(1, device="cuda"),
                 db0v=torch.zeros(1, device="cuda"), dpbias=torch.zeros(S2, device="cuda"),
                 acc=acc0.clone())
        ops.head_bwd2(h, par["w"], par["wv"], kept["dz"], dzv, o["dH"], o["dwp"], o["dwv"],
                      o["db0p"], o["db0v"], o["dpbias"], K, dzsum=kept["dzsum"],
                      metrics=(kept["loss"], kept["hit"], o["acc"]), relu_in=relu_in)
        return o

    raw, mat = bwd(Ap, True), bwd(Hp, False)
    for k in raw:
        assert torch.equal(raw[k], mat[k]), k
    dH = ops.unpack(raw["dH"], K, 1)
    assert float(dH.abs().max()) > 0 and float(raw["dwv"][:K].abs().max()) > 0
    assert int((dH[A.float() <= 0] != 0).sum()) == 0
    assert int((dH[A.float() > 0] != 0).sum()) > 0.9 * int((A.float() > 0).sum())
    with pytest.raises(ValueError):
        ops.head_bwd2(Ap, par["w"], par["wv"], kept["dz"], dzv, None, raw["dwp"], raw["dwv"],
                      raw["db0p"], raw["db0v"], None, K, relu_mask=False, relu_in=True)


# ------------------------------------------------------------------ 2. detection

def test_detect_plan(cuda, raw_top):
    from rocalphago_amd.models.fused import DualPlan, ResnetDualPlan, detect_plan
    net = ResnetPolicyValue(DEFAULT_FEATURES, device="cuda", seed=3, **SMALL)
    plan = net.model._plan_for()
    assert type(plan) is ResnetDualPlan and isinstance(plan, DualPlan)
    assert plan.multi_output and plan.pass_name is None and plan.vhead_name
    assert type(plan.trunk).__doc__
    offs = plan.layer_offsets()
    assert offs == sorted(offs) and offs[0] == 0 and len(offs) == len(plan.conv_names)
    # the head parameters sit behind the trunk's in the flat buffer
    base = net.model.net.flat.data_ptr()
    for name in (plan.head_name, plan.bias_name, plan.vhead_name, plan.d1, plan.d2):
        assert (net.model.net.params_of(name)[0].data_ptr() - base) // 4 > offs[-1]
    # the head's input: the last residual sum itself with RAW_TOP, and no H is written
    B = 4
    x = torch.from_numpy(planes(np.random.RandomState(0), B, 9)).cuda()
    plan.prepare(x)
    t = plan.trunk
    assert t.top_relu_in == raw_top
    t.H.fill_(7.0)
    plan.forward(x)
    torch.cuda.synchronize()
    if raw_top:
        assert t.output(B).data_ptr() == t.A[-1].data_ptr()
        assert bool((t.H == 7.0).all())
    else:
        from rocalphago_amd.ops import hipops
        assert t.output(B).data_ptr() == t.H.data_ptr()
        assert torch.equal(hipops.unpack(t.H[:B], t.K, 1),
                           torch.relu(hipops.unpack(t.A[-1][:B], t.K, 1)))
    # the value branch's hidden Dense missing: the generic executor
    L = list(net.model.layers)
    dropped = L.pop(-2)
    L[-1].inbound = list(dropped.inbound)
    m = K.Model(L, functional=True, inputs=net.model.net.input_names,
                outputs=net.model.net.output_names, device="cuda", seed=1)
    assert detect_plan(m) is None and m._plan_for() is None
    # a pass logit in the policy branch: the generic executor
    net2 = ResnetPolicyValue(DEFAULT_FEATURES, device="cuda", seed=3, **SMALL)
    L = list(net2.model.layers)
    i = next(k for k, ld in enumerate(L) if ld.class_name == "Bias")
    pl = K.PassLogit()
    pl.inbound = [L[i].name]
    L[i + 1].inbound = [pl.name]
    L.insert(i + 1, pl)
    m = K.Model(L, functional=True, inputs=net2.model.net.input_names,
                outputs=net2.model.net.output_names, device="cuda", seed=1)
    assert detect_plan(m) is None
    # and on the CPU / in fp32 there is no plan either
    assert ResnetPolicyValue(DEFAULT_FEATURES, device="cpu", **SMALL).model._plan_for() is None
    assert ResnetPolicyValue(DEFAULT_FEATURES, device="cuda", **SMALL).set_dtype("fp32") \
        .model._plan_for() is None


# ------------------------------------------------------------------ 3. forward

def head_values(ops, plan, B):
    """The value output in float64 torch from the plan's own (unpacked) trunk output."""
    H = torch.relu(ops.unpack(plan.trunk.output(B), plan.K, 1)).double()
    wv, b0v = plan.head_params(plan.vhead_name)
    W1, b1, W2, b2 = [t.double() for t in plan._dense_params()]
    zv = (H * wv.double().view(1, -1, 1, 1)).sum(1).reshape(B, -1) + b0v.double()
    h = zv @ W1 + b1
    h = torch.relu(h) if plan.act1 == "relu" else torch.tanh(h) if plan.act1 == "tanh" else h
    return torch.tanh(h @ W2 + b2).reshape(-1)


@pytest.mark.parametrize("cfg", [SMALL, dict(board=19, filters_per_layer=128, layers=5)],
                         ids=["k32_l4_s9", "k128_l5_s19"])
def test_forward_matches_resnet_plan_and_float64_heads(ops, cfg, monkeypatch):
    """Probabilities against ResnetPlan.forward of a ResnetPolicy with the same weights (the same
    kernels on the same weights) and values against float64 torch on the unpacked trunk output:
    1e-5 absolute, test_dual_forward_matches_the_two_plans' bounds; both RAW_TOP settings give
    the same bits."""
    from rocalphago_amd.models.fused import ResnetDualPlan, ResnetPlan
    S = cfg["board"]
    nets = {}
    for raw in (True, False):
        monkeypatch.setattr(ResnetDualPlan, "RAW_TOP", raw)
        nets[raw] = ResnetPolicyValue(DEFAULT_FEATURES, device="cuda", seed=3, **cfg)
        if raw:
            w = randomised(nets[raw].model, 5)
        nets[raw].model.set_weights(w)
        assert nets[raw].model._plan_for().trunk.top_relu_in == raw
    pol = ResnetPolicy(DEFAULT_FEATURES, device="cuda", seed=3, **cfg)
    pol.model.set_weights(w[:n_policy_weights(nets[True].model)])
    assert isinstance(pol.model._plan_for(), ResnetPlan)
    rng = np.random.RandomState(6)
    for B in (16, 5):
        x = torch.from_numpy(planes(rng, B, S)).cuda()
        plan = nets[True].model._plan_for()
        p, v = plan.forward(x)
        want_v = head_values(ops, plan, B)
        pp = pol.model._plan_for().forward(x)
        assert p.shape == (B, S * S) and v.shape == (B,)
        ep, evl = float((p - pp).abs().max()), float((v.double() - want_v).abs().max())
        print("B = %d: probabilities %.3g, values %.3g" % (B, ep, evl))
        assert ep <= 1e-5 and evl <= 1e-5
        assert float(v.abs().max()) > 1e-3
        p2, v2 = nets[False].model._plan_for().forward(x)
        assert torch.equal(p, p2) and torch.equal(v, v2)
        fp, fv = nets[True].forward_both(x.cpu().numpy())
        assert np.array_equal(fp, p.cpu().numpy()) and np.array_equal(fv, v.cpu().numpy())


# ------------------------------------------------------------------ 4. head gradients

@pytest.mark.parametrize("targets", ["onehot", "dense"])
def test_head_gradients_match_fp32_on_same_trunk(ops, raw_top, targets, monkeypatch):
    """test_dual_head_gradients_match_fp32_on_same_trunk (tests/test_dual_plan_gpu.py) on the
    residual trunk's output, its bounds and target recipe: relative L2 error below 1e-5 for
    every fp32 head gradient (the policy conv's scalar bias relative to sum |dz|), below 5e-3
    for dH, the losses within 1e-4 max(1, |loss|), value targets from [0.5, 1] and the
    cancellation ratio of the value conv's scalar bias asserted below 100."""
    net = ResnetPolicyValue(DEFAULT_FEATURES, device="cuda", seed=3, **SMALL)
    net.model.set_weights(randomised(net.model, 4))
    plan = net.model._plan_for()
    flat = net.model.net
    S2 = 81
    rng = np.random.RandomState(4)
    B, vw = 16, 0.5
    X = torch.from_numpy(planes(rng, B, 9)).cuda()
    Yv = torch.from_numpy(rng.uniform(0.5, 1, (B, 1)).astype(np.float32)).cuda()
    Yp = torch.from_numpy(one_hot_rows(rng, B, S2) if targets == "onehot"
                          else soft_rows(rng, B, S2)).cuda()
    flat.flat_grad.zero_()
    Bp = plan.prepare(X)
    # the residual trunk's backward reuses the top-gradient buffer for the units below (its BN
    # backward writes dL/dA_u in place when the halos agree): keep what the heads wrote
    kept = {}
    trunk_backward = plan.trunk.backward

    def keep_top_grad(Bb, *a, **k):
        kept["top"] = plan.trunk.top_grad(Bb).clone()
        return trunk_backward(Bb, *a, **k)
    monkeypatch.setattr(plan.trunk, "backward", keep_top_grad)
    if targets == "onehot":
        lv = plan.fwd_bwd(Bp, Yp.argmax(1), None, 1, 1.0 / B, Yv, vw)
    else:
        lv = plan.fwd_bwd(Bp, None, None, 1, 1.0 / B, Yv, vw, targets=Yp)
    torch.cuda.synchronize()
    total = float(plan.head.loss[:B].mean()) + vw * float(lv)
    Kc = plan.K
    raw = ops.unpack(plan.trunk.output(B), Kc, 1)
    assert (float(raw.min()) < 0) == raw_top
    H = torch.relu(raw).detach().clone().requires_grad_()
    leaf = [t.detach().clone().requires_grad_() for t in
            plan.head_params() + plan.head_params(plan.vhead_name) +
            (flat.params_of(plan.bias_name)[0],) + tuple(plan._dense_params())]
    wp, b0p, wv, b0v, pb, W1, b1, W2, b2 = leaf
    zp = (H * wp.reshape(1, Kc, 1, 1)).sum(1).reshape(B, -1) + b0p + pb
    zv = (H * wv.reshape(1, Kc, 1, 1)).sum(1).reshape(B, -1) + b0v
    v = torch.tanh(torch.relu(zv @ W1 + b1) @ W2 + b2)
    lp = K.categorical_crossentropy(Yp, torch.softmax(zp, -1)).mean()
    lval = ((v - Yv) ** 2).mean()
    loss = lp + vw * lval
    loss.backward()
    assert abs(total - loss.item()) < 1e-4 * max(1.0, abs(loss.item())), (total, loss.item())
    assert abs(float(lv) - lval.item()) < 1e-4 * max(1.0, lval.item())

    def rel(a, b):
        return float((a - b).norm() / max(float(b.norm()), 1e-12))
    gW1, gb1, gW2, gb2 = flat.grads_of(plan.d1) + flat.grads_of(plan.d2)
    gwp, gbp = flat.grads_of(plan.head_name)
    gwv, gbv = flat.grads_of(plan.vhead_name)
    gpb = flat.grads_of(plan.bias_name)[0]
    errs = {"W1": rel(gW1, W1.grad), "b1": rel(gb1, b1.grad), "W2": rel(gW2, W2.grad),
            "b2": rel(gb2, b2.grad), "policy_w": rel(gwp.reshape(-1), wp.grad.reshape(-1)),
            "value_w": rel(gwv.reshape(-1), wv.grad.reshape(-1)),
            "value_b": rel(gbv.reshape(-1), b0v.grad.reshape(-1)),
            "Bias": rel(gpb, pb.grad)}
    errs["policy_b"] = abs(float(gbp) - float(b0p.grad)) / float(plan.head.dz[:B].abs().sum())
    top = ops.unpack(kept["top"], Kc, 1)
    errs["dH"] = rel(top, H.grad * (H > 0))
    cond = float(plan.head.dzv[:B].abs().sum()) / abs(float(b0v.grad))
    print("sum|dzv| / |sum dzv| = %.3g" % cond)
    assert cond < 100, cond
    print(targets, raw_top, errs)
    for k in errs:
        if k != "dH":
            assert errs[k] < 1e-5, (k, errs)
    assert errs["dH"] < 5e-3, errs
    assert float(W1.grad.norm()) > 0 and float(wv.grad.norm()) > 0


# ------------------------------------------------------------------ 5. the whole step

@pytest.mark.parametrize("cfg", [dict(board=19, filters_per_layer=64, layers=5), SMALL],
                         ids=["k64_l5_s19", "k32_l4_s9"])
def test_train_step_matches_generic(ops, cfg):
    """One (categorical_crossentropy, 0.5 mse) step at lr = 0 against the CPU generic executor,
    test_resnet_plan_train_step_matches_generic's bounds: each loss within 5 %, per-tensor
    gradient cosine above 0.98, norm ratio within 8 %, running statistics rtol 1e-2 /
    atol 2e-3."""
    S = cfg["board"]
    gpu = ResnetPolicyValue(DEFAULT_FEATURES, device="cuda", seed=3, **cfg)
    cpu = ResnetPolicyValue(DEFAULT_FEATURES, device="cpu", seed=3, **cfg)
    ws = randomised(cpu.model, 3)
    cpu.model.set_weights(ws)
    gpu.model.set_weights(ws)
    B = 16
    rng = np.random.RandomState(1)
    X = planes(rng, B, S)
    Yp = one_hot_rows(rng, B, S * S)
    # value targets from [0.5, 1], test_head_gradients_match_fp32_on_same_trunk's recipe and
    # reason: the value conv's scalar bias gradient is the sum of all B S^2 values dzv, and
    # under targets of both signs the boards' sums cancel, so that a relative bound on it
    # measures the cancellation and not the step (measured with targets of +-1: that one
    # scalar at a norm ratio of 0.80 on the 19x19 case and 1.004 on the 9x9 one, every other
    # tensor inside the bounds; with these targets sum |dzv| / |sum dzv| = 15 and 1.008)
    Yv = rng.uniform(0.5, 1, (B, 1)).astype(np.float32)
    for m in (cpu.model, gpu.model):
        m.compile(loss=["categorical_crossentropy", "mse"], optimizer=K.SGD(lr=0.0),
                  loss_weights=[1.0, 0.5])
    assert gpu.model._plan_for() is not None
    r_cpu = cpu.model.train_on_batch(X, [Yp, Yv])
    r_gpu = gpu.model.train_on_batch(X, [Yp, Yv])
    print("losses cpu %r gpu %r" % (r_cpu, r_gpu))
    for a, b in zip(r_cpu[:3], r_gpu[:3]):
        assert abs(a - b) < 0.05 * abs(a), (r_cpu, r_gpu)
    net_c, net_g = cpu.model.net, gpu.model.net
    plan = gpu.model._plan_for()
    dzv = plan.head.dzv[:B]
    print("value conv scalar bias: sum|dzv| / |sum dzv| = %.3g"
          % (float(dzv.abs().sum()) / abs(float(dzv.sum()))))
    seen, bad = 0, []
    for (lname, wname, shape), gc, gg, pc, pg in zip(net_c.weight_names, net_c._gviews,
                                                     net_g._gviews, net_c._views, net_g._views):
        gc, gg = gc.detach().reshape(-1), gg.detach().cpu().reshape(-1)
        if "running" in wname:
            assert torch.allclose(pc.detach().cpu(), pg.detach().cpu(), rtol=1e-2, atol=2e-3), \
                wname
            continue
        nc = gc.norm().item()
        if nc < 1e-6:
            assert gg.norm().item() < 1e-3, wname
            continue
        cos = torch.dot(gc, gg).item() / (nc * gg.norm().item() + 1e-12)
        ratio = gg.norm().item() / nc
        print("%s %s cos %.5f norm ratio %.4f" % (wname, tuple(shape), cos, ratio))
        if not (cos > 0.98 and abs(ratio - 1) < 0.08):
            bad.append((wname, cos, ratio))
        seen += 1
    assert seen >= len(net_c.weight_names) // 2
    assert not bad, bad


# ------------------------------------------------------------------ 6. trainer and search

def test_policy_value_trainer_step_and_evaluate(cuda, raw_top):
    from rocalphago_amd.models.fused import ResnetDualPlan
    from rocalphago_amd.training import supervised as sl
    from rocalphago_amd.training.data import DeviceDataset
    S, B = 9, 8
    net = ResnetPolicyValue(DEFAULT_FEATURES, dense=64, device=cuda, seed=5, **SMALL)
    model = net.model
    model.compile(loss=["categorical_crossentropy", "mse"], optimizer=K.SGD(lr=0.01),
                  loss_weights=[1.0, 0.5], metrics=["accuracy"])
    ds = DeviceDataset.synthetic(32, 48, S, cuda, seed=7, visits=True, outcomes=True)
    tr = sl.PolicyValueTrainer(model, ds, B, ["noop", "rot90", "fliplr", "diag2"], None,
                               seed=3, targets="visits", value_weight=0.5)
    assert type(tr.plan) is ResnetDualPlan and tr.plan.trunk.top_relu_in == raw_top
    before = model.net.flat.clone()
    index = torch.tensor([5, 0, 31, 7, 7, 12, 20, 1], device=cuda)
    tr.step(index)
    tr.step(index.flip(0))
    m = tr.pop_metrics()
    assert len(m) == 3 and all(np.isfinite(m)) and m[0] > 0 and 0 <= m[1] <= 1
    assert 0 < m[2] < 4
    assert not torch.equal(before, model.net.flat)
    ev = tr.evaluate(index)
    assert len(ev) == 3 and all(np.isfinite(ev)) and 0 <= ev[2] < 4
    # the "actions" mode: evaluate's policy loss and value loss against a manual plan forward
    tr2 = sl.PolicyValueTrainer(model, ds, B, None, None, seed=3, value_weight=0.5)
    tr2.step(index)
    assert all(np.isfinite(tr2.pop_metrics()))
    lp, acc, lv = tr2.evaluate(index)
    p, v = tr2.plan.forward(ds.states, index=index)
    lab = ds.labels[index].long()
    pl = p.double()[torch.arange(B, device=cuda), lab].clamp(1e-7, 1 - 1e-7)
    want = float(-pl.log().mean())
    print("evaluate policy loss %.8g manual %.8g" % (lp, want))
    assert abs(lp - want) <= 1e-5
    assert abs(lv - float(((v - ds.outcomes[index].reshape(-1)) ** 2).mean())) <= 1e-5
    assert acc == float((p.argmax(1) == lab).float().mean())


@pytest.mark.parametrize("graph", ["0", "1"])
def test_packed_wave_matches_board_path(cuda, graph):
    """submit_wave with a 9x9 residual policy-value network gives the board path's priors /
    values / sensible masks, eagerly and graph-replayed (tests/resnet_dual_wave_job.py, a
    process of its own under a time limit), as test_dual_packed_wave_matches_board_path."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "resnet_dual_wave_job.py"), graph]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=180, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-3000:]
    assert json.loads(lines[-1]) == {"ok": True, "graph": graph == "1"}
