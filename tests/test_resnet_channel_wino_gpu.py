"""128-wide residual networks with channel BatchNormalization (bn_axis=1) whose 3x3 layers run
the channel form of the Winograd BN kernel forward (ResTrunk.CH_WINO, conv_wino.hip BNM 3):
against the generic executor on the CPU in fp32 with the same weights, against the same model
with the switch off (the unfused sequence on the direct kernel), and a column-BN model of the same
width before and after. Bounds and helpers of tests/test_resnet_channel_bn_gpu.py."""
import numpy as np
import pytest
import torch

from rocalphago_amd.features.preprocessing import DEFAULT_FEATURES
from rocalphago_amd.models import kerasish as KZ
from rocalphago_amd.models.engine import ResTrunk
from rocalphago_amd.models.policy import ResnetPolicy
from rocalphago_amd.models.policy_value import ResnetPolicyValue
from test_resnet_channel_bn_gpu import assert_grads_close, assert_policy_close
from test_resnet_dual_gpu import one_hot_rows, planes, randomised

pytestmark = pytest.mark.gpu

S = 19
WIDE = dict(board=S, filters_per_layer=128, layers=4)
CH = dict(WIDE, bn_axis=1)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rocalphago_amd.ops import hipops
    return hipops


@pytest.fixture(scope="module")
def column_before(ops):
    """A 128-wide column-BN network and its prediction; every test asks for it first, so it
    exists before any channel model of this module."""
    net = ResnetPolicy(DEFAULT_FEATURES, device="cuda", seed=11, **WIDE)
    net.model.set_weights(randomised(net.model, 12))
    X = planes(np.random.RandomState(5), 6, S)
    return net.model.get_weights(), X, net.model.predict(X)


@pytest.fixture(scope="module")
def references(column_before):
    """Per network class: the CPU model (generic fp32 executor), its initial weights and its
    outputs on the B = 6 planes, computed once (a train step moves the CPU model's running
    statistics afterwards, the saved weights and outputs are the initial ones)."""
    X = planes(np.random.RandomState(6), 6, S)
    out = {}
    for cls in (ResnetPolicy, ResnetPolicyValue):
        cpu = cls(DEFAULT_FEATURES, device="cpu", seed=3, **CH)
        ws = randomised(cpu.model, 3)
        cpu.model.set_weights(ws)
        ref = cpu.forward_both(X) if cls is ResnetPolicyValue else cpu.model.predict(X)
        out[cls] = (cpu, ws, ref)
    return X, out


def build(cls, ws, switch, monkeypatch):
    """The GPU model with ``ws`` and its trunk, built with ResTrunk.CH_WINO = ``switch``."""
    monkeypatch.setattr(ResTrunk, "CH_WINO", switch)
    net = cls(DEFAULT_FEATURES, device="cuda", seed=3, **CH)
    net.model.set_weights(ws)
    trunk = net.model._plan_for().trunk
    assert trunk.bn_axis == 1
    return net, trunk


def poison_U(trunk, B):
    """NaN in the interior of every stored U (each has its consumer's halo, 2 in front of the
    first unit's 5x5 conv; the halo stays the zero the kernels rely on)."""
    trunk.ensure_batch(B)
    for U in trunk.U:
        interior(U)[:] = float("nan")


def interior(U):
    h = (U.shape[1] - S) // 2
    return U[:, h:h + S, h:h + S]


def outputs(net, X):
    if isinstance(net, ResnetPolicyValue):
        p, v = net.forward_both(X)
        return np.asarray(p), np.asarray(v).reshape(-1)
    return np.asarray(net.model.predict(X)), None


@pytest.mark.parametrize("cls", [ResnetPolicy, ResnetPolicyValue])
def test_inference_runs_channel_winograd_and_stores_no_U(ops, column_before, references, cls,
                                                         monkeypatch):
    X, refs = references
    _, ws, ref = refs[cls]
    rp, rv = (np.asarray(ref[0]), np.asarray(ref[1]).reshape(-1)) if cls is ResnetPolicyValue \
        else (np.asarray(ref), None)
    net, t = build(cls, ws, True, monkeypatch)
    assert any(t._wino) and any(t._plan(6)[1]) and not any(t._plan(6)[0])
    poison_U(t, 6)
    gp, gv = outputs(net, X)
    assert not any(t._fused)
    # the U in front of every Winograd layer is still the poison: nothing wrote it, and the
    # finite outputs below did not need it (a 5x5 layer's U is written and read as before)
    wino = t._plan(6)[1]
    fed = [j for j in range(len(t.bns)) if wino[j + 1]]
    assert fed and all(s.ks != 3 for l, s in enumerate(t.specs) if l > 0 and not wino[l])
    assert all(bool(torch.isnan(interior(t.U[j])[:6]).all()) for j in fed), "inference wrote a U"
    assert np.isfinite(gp).all()
    assert_policy_close(rp, gp)
    off, toff = build(cls, ws, False, monkeypatch)
    assert not any(toff._wino) and not any(toff._plan(6)[1])
    op, ov = outputs(off, X)
    assert_policy_close(op, gp)
    if gv is not None:
        print("values: %.3g against generic, %.3g against the switch off"
              % (np.abs(rv - gv).max(), np.abs(ov - gv).max()))
        assert np.abs(rv - gv).max() < 2e-2 and np.abs(ov - gv).max() < 2e-2
        assert np.abs(gv).max() > 1e-3


@pytest.mark.parametrize("cls", [ResnetPolicy, ResnetPolicyValue])
def test_train_step_matches_generic_and_stores_U(ops, column_before, references, cls,
                                                 monkeypatch):
    """One step at lr = 0, B = 16: the forward runs the channel Winograd form with the next BN's
    statistics from its epilogue (bn_ch_finalize_fwd), the backward the direct kernels on the
    stored U."""
    _, refs = references
    cpu, ws, _ = refs[cls]
    cpu.model.set_weights(ws)
    net, t = build(cls, ws, True, monkeypatch)
    B = 16
    rng = np.random.RandomState(1)
    X = planes(rng, B, S)
    Yp = one_hot_rows(rng, B, S * S)
    if cls is ResnetPolicyValue:
        Y = [Yp, rng.uniform(0.5, 1, (B, 1)).astype(np.float32)]
        kw = dict(loss=["categorical_crossentropy", "mse"], loss_weights=[1.0, 0.5])
    else:
        Y, kw = Yp, dict(loss="categorical_crossentropy")
    for m in (cpu.model, net.model):
        m.compile(optimizer=KZ.SGD(lr=0.0), **kw)
    assert any(t._plan(B)[1])
    poison_U(t, B)
    r_cpu = cpu.model.train_on_batch(X, Y)
    r_gpu = net.model.train_on_batch(X, Y)
    print("losses cpu %r gpu %r" % (r_cpu, r_gpu))
    for a, b in zip(np.atleast_1d(r_cpu)[:3], np.atleast_1d(r_gpu)[:3]):
        assert abs(a - b) < 0.05 * abs(a), (r_cpu, r_gpu)
    assert_grads_close(cpu.model.net, net.model.net, slots=128)
    assert not any(t._fused)
    for U in t.U:
        assert bool(torch.isfinite(U[:B].float()).all()), "the training forward stored no U"
        assert float(U[:B].float().abs().max()) > 0


def test_column_model_unaffected_by_channel_winograd_models(ops, column_before, references,
                                                            monkeypatch):
    from rocalphago_amd.models.fused import ResnetPlan
    ws, X, before = column_before
    _, refs = references
    ch, t = build(ResnetPolicy, refs[ResnetPolicy][1], True, monkeypatch)
    assert any(t._plan(6)[1])
    ch.model.predict(X)
    ch.model.compile(loss="categorical_crossentropy", optimizer=KZ.SGD(lr=0.0))
    ch.model.train_on_batch(X, one_hot_rows(np.random.RandomState(2), 6, S * S))
    net = ResnetPolicy(DEFAULT_FEATURES, device="cuda", seed=11, **WIDE)
    net.model.set_weights(ws)
    plan = net.model._plan_for()
    assert isinstance(plan, ResnetPlan) and plan.trunk.bn_axis == -1
    assert np.array_equal(net.model.predict(X), before)
    assert tuple(plan.trunk.coef.shape[1:]) == (3, S)
