"""The policy-value network on the fused HIP plan (models/fused.py DualPlan): detection, the
forward against the two single-head plans, the head gradients against fp32 autograd on the same
trunk output, the whole step against the CPU model, the trainer, and the search's wave path.
Shapes: those of the existing plan tests (19x19, 32 filters, 3 layers, B = 8 or 16)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rocalphago_amd.features.preprocessing import DEFAULT_FEATURES, VALUE_FEATURES
from rocalphago_amd.models import kerasish as K
from rocalphago_amd.models.policy import CNNPolicy
from rocalphago_amd.models.policy_value import CNNPolicyValue
from rocalphago_amd.models.value import CNNValue
from test_soft_training import soft_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(filters_per_layer=32, layers=3, seed=3)


def planes(rng, B, F=49, S=19):
    return (rng.rand(B, F, S, S) > 0.6).astype(np.float32)


def one_hot_rows(rng, B, C=361):
    Y = np.zeros((B, C), np.float32)
    Y[np.arange(B), rng.randint(0, C, B)] = 1
    return Y


def test_detect_plan(cuda):
    from rocalphago_amd.models.fused import DualPlan, detect_plan
    net = CNNPolicyValue(VALUE_FEATURES, device="cuda", **KW)
    plan = net.model._plan_for()
    assert isinstance(plan, DualPlan) and plan.head.gen == 0
    assert plan.layer_offsets() == sorted(plan.layer_offsets()) and plan.layer_offsets()[0] == 0
    # the value branch's hidden Dense missing: the generic executor
    L = list(net.model.layers)
    dropped = L.pop(-2)
    L[-1].inbound = list(dropped.inbound)
    m = K.Model(L, functional=True, inputs=net.model.net.input_names,
                outputs=net.model.net.output_names, device="cuda", seed=1)
    assert detect_plan(m) is None and m._plan_for() is None
    # and on the CPU / in fp32 there is no plan either
    assert CNNPolicyValue(VALUE_FEATURES, device="cpu", **KW).model._plan_for() is None
    assert CNNPolicyValue(VALUE_FEATURES, device="cuda", **KW).set_dtype("fp32") \
        .model._plan_for() is None


def test_dual_forward_matches_the_two_plans(cuda):
    """The dual forward against PolicyPlan.forward and ValuePlan.forward of a CNNPolicy and a
    CNNValue carrying the same trunk and head weights: 1e-5 absolute, the cap the project holds
    its fp32 head kernels to (the trunks run the same kernels on the same weights)."""
    dual = CNNPolicyValue(VALUE_FEATURES, device="cuda", **KW)
    pol = CNNPolicy(VALUE_FEATURES, device="cuda", **KW)
    val = CNNValue(VALUE_FEATURES, device="cuda", **KW)
    w = dual.model.get_weights()
    rng = np.random.RandomState(5)
    # the zero-initialised biases and Bias would hide a mixed-up head: randomise them all
    w = [a + rng.uniform(-0.05, 0.05, a.shape).astype(np.float32) for a in w]
    dual.model.set_weights(w)
    pol.model.set_weights(w[:9])
    val.model.set_weights(w[:6] + w[9:])
    for B in (16, 5):
        x = torch.from_numpy(planes(rng, B)).cuda()
        p, v = dual.model._plan_for().forward(x)
        pp = pol.model._plan_for().forward(x)
        vv = val.model._plan_for().forward(x).reshape(-1)
        assert p.shape == (B, 361) and v.shape == (B,)
        ep, evl = float((p - pp).abs().max()), float((v - vv).abs().max())
        print("B = %d: probabilities %.3g, values %.3g" % (B, ep, evl))
        assert ep <= 1e-5 and evl <= 1e-5
        assert float(v.abs().max()) > 1e-3  # not a trivially zero value head
        fp, fv = dual.forward_both(x.cpu().numpy())
        assert np.array_equal(fp, p.cpu().numpy()) and np.array_equal(fv, v.cpu().numpy())
        assert np.array_equal(dual.forward(x.cpu().numpy()), fp)


@pytest.mark.parametrize("targets", ["onehot", "dense"])
@pytest.mark.parametrize("dense_act", ["relu", "linear", "tanh"])
def test_dual_head_gradients_match_fp32_on_same_trunk(cuda, dense_act, targets):
    """Both heads' HIP training tail (the dual head forward, value_mlp_train, head_bwd2) against
    fp32 torch autograd applied to the SAME bf16 trunk output, the policy head under categorical
    cross-entropy and the value head under value_weight * MSE, value_weight = 0.5;
    test_value_head_gradients_match_fp32_on_same_trunk's bounds: relative L2 error below 1e-5
    for every fp32 head gradient, below 5e-3 for dH (bf16 storage), the total loss within
    1e-4 max(1, |loss|).

    The policy head conv's scalar bias is the one exception in form: its gradient is the sum of
    dz over the batch, and softmax gradients sum to zero over each board, so the true value is
    0 and a relative error of it means nothing. It is held to the same 1e-5, relative to the
    sum of |dz| (the terms it is the sum of).

    The value conv's scalar bias gradient is the sum of the B S^2 values dzv, which cancel
    within a board (W1 has zero mean) and, under targets of both signs, between boards. An fp32
    sum is good to about 6e-8 of the sum of |terms|, so its error relative to the result is
    6e-8 c with c = sum |dzv| / |sum dzv|: a bound of 1e-5 relative to the result tests the
    kernel only while c stays below ~100 (measured with targets drawn from [-1, 1]: c = 41 and
    an error of 4e-7 in one draw; c = 4000 in another, where the kernel was 8e-6 .. 4e-5 and
    fp32 autograd itself 2e-5 .. 3e-5 from float64). The targets are therefore drawn from
    [0.5, 1] (every board pulls the value up: no cancellation between boards), before the
    policy targets (both target kinds see the same values), and c < 100 is asserted."""
    from rocalphago_amd.ops import hipops as ops
    net = CNNPolicyValue(VALUE_FEATURES, device="cuda", dense_activation=dense_act, **KW)
    plan = net.model._plan_for()
    flat = net.model.net
    rng = np.random.RandomState(4)
    w = [a + rng.uniform(-0.05, 0.05, a.shape).astype(np.float32) if i >= 6 else a
         for i, a in enumerate(net.model.get_weights())]
    net.model.set_weights(w)
    B, vw = 16, 0.5
    X = torch.from_numpy(planes(rng, B)).cuda()
    Yv = torch.from_numpy(rng.uniform(0.5, 1, (B, 1)).astype(np.float32)).cuda()
    Yp = torch.from_numpy(one_hot_rows(rng, B) if targets == "onehot"
                          else soft_rows(rng, B, 361)).cuda()
    flat.flat_grad.zero_()
    Bp = plan.prepare(X)
    if targets == "onehot":
        lv = plan.fwd_bwd(Bp, Yp.argmax(1), None, 1, 1.0 / B, Yv, vw)
    else:
        lv = plan.fwd_bwd(Bp, None, None, 1, 1.0 / B, Yv, vw, targets=Yp)
    torch.cuda.synchronize()
    total = float(plan.head.loss[:B].mean()) + vw * float(lv)
    Kc = plan.K
    H = ops.unpack(plan.trunk.output(B), Kc, 1).detach().clone().requires_grad_()
    leaf = [t.detach().clone().requires_grad_() for t in
            plan.head_params() + plan.head_params(plan.vhead_name) +
            (flat.params_of(plan.bias_name)[0],) + tuple(plan._dense_params())]
    wp, b0p, wv, b0v, pb, W1, b1, W2, b2 = leaf
    zp = (H * wp.reshape(1, Kc, 1, 1)).sum(1).reshape(B, -1) + b0p + pb
    zv = (H * wv.reshape(1, Kc, 1, 1)).sum(1).reshape(B, -1) + b0v
    h = zv @ W1 + b1
    h = torch.relu(h) if dense_act == "relu" else torch.tanh(h) if dense_act == "tanh" else h
    v = torch.tanh(h @ W2 + b2)
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
    dzsum_abs = float(plan.head.dz[:B].abs().sum())
    errs["policy_b"] = abs(float(gbp) - float(b0p.grad)) / dzsum_abs
    top = ops.unpack(plan.trunk.top_grad(B), Kc, 1)
    assert plan.trunk.top_relu
    errs["dH"] = rel(top, H.grad * (H > 0))
    # precondition of the relative bound on the value conv's scalar bias (see the docstring)
    cond = float(plan.head.dzv[:B].abs().sum()) / abs(float(b0v.grad))
    print("value_b: kernel %.9g reference %.9g, sum|dzv| / |sum dzv| = %.3g" %
          (float(gbv), float(b0v.grad), cond))
    assert cond < 100, cond
    print(dense_act, targets, errs)
    for k in errs:
        if k != "dH":
            assert errs[k] < 1e-5, (k, errs)
    assert errs["dH"] < 5e-3, errs
    # both heads reach dH: without the value term it is a different tensor
    assert float(W1.grad.norm()) > 0 and float(wv.grad.norm()) > 0
    with pytest.raises(ValueError):
        plan.fwd_bwd(Bp, Yp.argmax(1), None, 1, 1.0 / B, Yv, 0.0)


@pytest.mark.parametrize("targets", ["onehot", "dense"])
@pytest.mark.parametrize("dense_act", ["linear", "tanh"])
def test_dual_train_step_matches_cpu(cuda, targets, dense_act):
    """train_on_batch(X, [Yp, Yv]) on the fused plan against the CPU model at SGD(lr=0.01),
    test_policy_soft_train_step_matches_cpu's tolerances (its docstring gives the reason for
    the learning rate): the total loss within 1e-2 relative, every tensor within
    2e-2 max(1e-3, max|b|). train_step returns a value (None would mean the generic path), and
    None for a pair of losses that is not (categorical_crossentropy, mse).

    The value MLP's hidden layer is linear or tanh here. With ReLU, bf16-level differences of
    the trunk output flip the mask of hidden units near zero, which moves the value head's
    updates by ~8 % between the bf16 plan and the fp32 CPU model
    (test_gpu_models.test_value_train_step_matches_cpu allows its ReLU case 15 % for that
    reason). One flipped unit j moves its hidden bias by lr * vw * 2 |v - y| / B * |W2[j]| =
    0.01 * 0.125 * 0.05 = 6e-5, three times this test's absolute floor of 2e-5. Measured here
    with ReLU: 3.7e-5 on the hidden bias and 3.9e-5 on the value conv's scalar bias (4.21e-4 on
    the GPU, 4.60e-4 on the CPU), every other tensor inside the tolerance; with the linear and
    tanh tails both are below 2e-9. The ReLU tail's kernels are held on the same trunk
    output by test_dual_head_gradients_match_fp32_on_same_trunk, its whole step by
    test_policy_value_trainer_step."""
    g = CNNPolicyValue(VALUE_FEATURES, device="cuda", dense_activation=dense_act, **KW)
    c = CNNPolicyValue(VALUE_FEATURES, device="cpu", dense_activation=dense_act, **KW)
    c.model.set_weights(g.model.get_weights())
    for m in (g, c):
        m.model.compile(loss=["categorical_crossentropy", "mse"], optimizer=K.SGD(lr=0.01),
                        loss_weights=[1.0, 0.5], metrics=["accuracy"])
    rng = np.random.RandomState(0)
    X = planes(rng, 8)
    Yp = one_hot_rows(rng, 8) if targets == "onehot" else soft_rows(rng, 8, 361)
    Yv = (rng.randint(0, 2, (8, 1)) * 2 - 1).astype(np.float32)
    plan = g.model._plan_for()
    dev = [torch.from_numpy(a).cuda() for a in (X, Yp, Yv)]
    before = g.model.net.flat.clone()
    r = plan.train_step(dev[0], dev[1:], ["categorical_crossentropy", "mse"],
                        loss_weights=[1.0, 0.5], want_acc=True)
    assert r is not None, "the (CE, MSE) pair left the fused plan"
    assert torch.equal(before, g.model.net.flat)  # train_step alone applies no update
    assert plan.train_step(dev[0], dev[1:], ["mse", "mse"]) is None
    assert plan.train_step(dev[0], dev[1:], ["categorical_crossentropy",
                                             "binary_crossentropy"]) is None
    rg_ = g.model.train_on_batch(X, [Yp, Yv])
    rc = c.model.train_on_batch(X, [Yp, Yv])
    assert len(rg_) == 4 and len(rc) == 4
    assert abs(rg_[1] - r[0][0]) < 1e-6 * abs(rg_[1]) and abs(rg_[2] - r[0][1]) < 1e-6
    assert abs(rg_[0] - (rg_[1] + 0.5 * rg_[2])) < 1e-6
    print("loss gpu %r cpu %r" % (rg_, rc))
    assert abs(rg_[0] - rc[0]) < 1e-2 * abs(rc[0])
    names = [ln + "/" + wn for ln, wn, _ in g.model.net.weight_names]
    diffs = [(n, float(np.abs(a - b).max()), 2e-2 * max(1e-3, float(np.abs(b).max())))
             for n, a, b in zip(names, g.model.get_weights(), c.model.get_weights())]
    print(" ".join("%s=%.3g(%.3g)" % d for d in diffs))
    for n, d, tol in diffs:
        assert d < tol, (n, d, tol)
    t = g.model.test_on_batch(X, [Yp, Yv])
    assert len(t) == 4 and all(np.isfinite(t))


def test_policy_value_trainer_step(cuda):
    """One PolicyValueTrainer.step on a 9x9 synthetic dataset with visits and outcomes: finite
    metrics, changed weights, and a second trainer with the same seed reproduces net.flat bit
    for bit (every summation order in the step is fixed)."""
    from rocalphago_amd.training import supervised as sl
    from rocalphago_amd.training.data import DeviceDataset
    S, B = 9, 8
    flats = []
    for rep in range(2):
        net = CNNPolicyValue(DEFAULT_FEATURES, board=S, filters_per_layer=32, layers=3,
                             dense=64, device=cuda, seed=5)
        model = net.model
        model.compile(loss=["categorical_crossentropy", "mse"], optimizer=K.SGD(lr=0.01),
                      loss_weights=[1.0, 0.5], metrics=["accuracy"])
        ds = DeviceDataset.synthetic(32, 48, S, cuda, seed=7, visits=True, outcomes=True)
        assert ds.outcomes.shape == (32, 1) and bool((ds.outcomes.abs() == 1).all())
        tr = sl.PolicyValueTrainer(model, ds, B, ["noop", "rot90", "fliplr", "diag2"], None,
                                   seed=3, targets="visits", value_weight=0.5)
        assert tr.plan is not None and tr.classes == S * S
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
        flats.append(model.net.flat.clone())
        if rep == 0:  # the "actions" mode runs the label kernel
            tr2 = sl.PolicyValueTrainer(model, ds, B, None, None, seed=3, value_weight=0.5)
            tr2.step(index)
            assert all(np.isfinite(tr2.pop_metrics()))
            with pytest.raises(ValueError):
                sl.PolicyValueTrainer(model, DeviceDataset.synthetic(8, 48, S, cuda), B)
    assert torch.equal(flats[0], flats[1])


@pytest.mark.parametrize("graph", ["0", "1"])
def test_dual_packed_wave_matches_board_path(cuda, graph):
    """submit_wave with a policy-value network (one DualPlan forward per wave, no side stream)
    gives the board path's priors / values / sensible masks, eagerly and graph-replayed
    (tests/dual_wave_job.py, a process of its own under a time limit)."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "dual_wave_job.py"), graph]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=180, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-3000:]
    assert json.loads(lines[-1]) == {"ok": True, "graph": graph == "1"}
