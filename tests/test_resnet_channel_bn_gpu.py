"""The residual networks with channel BatchNormalization (bn_axis=1) on the fused HIP path,
against the generic executor on the CPU in fp32 with the same weights (the bounds of
tests/test_resnet_gpu.py and tests/test_resnet_dual_gpu.py, whose helpers these tests use)."""
import numpy as np
import pytest
import torch

from rocalphago_amd.features.preprocessing import DEFAULT_FEATURES
from rocalphago_amd.models import kerasish as KZ
from rocalphago_amd.models.policy import ResnetPolicy
from rocalphago_amd.models.policy_value import ResnetPolicyValue
from test_resnet_dual_gpu import head_values, one_hot_rows, planes, randomised
from test_resnet_gpu import _pair, _planes

pytestmark = pytest.mark.gpu

SMALL = dict(board=9, filters_per_layer=32, layers=4)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rocalphago_amd.ops import hipops
    return hipops


@pytest.fixture(scope="module")
def column_before(ops):
    """A column-BN network and its prediction; the module's first fixture user asks for it before
    any channel model exists in this module."""
    net = ResnetPolicy(DEFAULT_FEATURES, device="cuda", seed=11, **SMALL)
    net.model.set_weights(randomised(net.model, 12))
    X = _planes(6, 9, 5)
    return net.model.get_weights(), X, net.model.predict(X)


def channel_pair(K, layers, board, n_skip):
    return _pair(K, layers, board, dict(n_skip, bn_axis=1))


def assert_policy_close(ref, got):
    """test_resnet_plan_forward_matches_generic's bounds (bf16 activations through every
    layer)."""
    lr, lg = np.log(ref + 1e-12), np.log(got + 1e-12)
    sel = ref > 1e-3
    e_log, e_p = np.abs(lr - lg)[sel].max(), np.abs(ref - got).max()
    print("log-probabilities %.4g, probabilities %.4g" % (e_log, e_p))
    assert e_log < 0.15
    assert e_p < 2e-2


def assert_grads_close(net_c, net_g, slots=None):
    """test_resnet_plan_train_step_matches_generic's bounds per array; BN arrays have ``slots``
    entries."""
    seen, bad = 0, []
    for (lname, wname, shape), gc, gg, pc, pg in zip(net_c.weight_names, net_c._gviews,
                                                     net_g._gviews, net_c._views, net_g._views):
        if slots is not None and lname.startswith("batchnormalization"):
            assert tuple(shape) == (slots,) and gg.numel() == slots and pg.numel() == slots
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
        print("%s %s %s cos %.5f norm ratio %.4f" % (lname, wname, tuple(shape), cos, ratio))
        if not (cos > 0.98 and abs(ratio - 1) < 0.08):
            bad.append((lname, wname, cos, ratio))
        seen += 1
    assert seen >= len(net_c.weight_names) // 2
    assert not bad, bad


def test_column_model_unaffected_by_channel_models(ops, column_before):
    """A column-BN model built after channel models ran in the same process still gets a column
    trunk and predicts what the same weights predicted before any channel model existed: no
    shared state (workspaces, packing tables, class attributes) leaked."""
    from rocalphago_amd.models.fused import ResnetPlan
    ws, X, before = column_before
    _, ch = channel_pair(32, 4, 9, {})
    assert ch.model._plan_for().trunk.bn_axis == 1
    ch.model.predict(X)
    ch.model.compile(loss="categorical_crossentropy", optimizer=KZ.SGD(lr=0.0))
    Y = np.zeros((6, 81), np.float32)
    Y[:, 3] = 1
    ch.model.train_on_batch(X, Y)
    net = ResnetPolicy(DEFAULT_FEATURES, device="cuda", seed=11, **SMALL)
    net.model.set_weights(ws)
    plan = net.model._plan_for()
    assert isinstance(plan, ResnetPlan) and plan.trunk.bn_axis == -1
    assert np.array_equal(net.model.predict(X), before)
    assert tuple(plan.trunk.coef.shape[1:]) == (3, 9)


@pytest.mark.parametrize("K,layers,board,n_skip", [(64, 5, 19, {}), (32, 4, 9, {"n_skip_1": 2}),
                                                   (40, 4, 9, {})])
def test_channel_plan_forward_matches_generic(ops, column_before, K, layers, board, n_skip):
    from rocalphago_amd.models.fused import ResnetPlan
    cpu, gpu = channel_pair(K, layers, board, n_skip)
    plan = gpu.model._plan_for()
    assert isinstance(plan, ResnetPlan) and plan.trunk.bn_axis == 1
    t = plan.trunk
    assert not any(t._wino)
    X = _planes(6, board)
    ref = cpu.model.predict(X)
    got = gpu.model.predict(X)
    assert tuple(t.coef.shape[1:]) == (3, t.KP) and tuple(t.stats.shape[1:]) == (2, t.KP)
    assert not any(t._fused) and t._plan(6) == ([False] * len(t.bns), [False] * t.L)
    assert_policy_close(ref, got)


@pytest.mark.parametrize("K,layers,board,n_skip", [(64, 5, 19, {}), (32, 4, 9, {"n_skip_1": 2}),
                                                   (40, 4, 9, {})])
def test_channel_plan_train_step_matches_generic(ops, column_before, K, layers, board, n_skip):
    cpu, gpu = channel_pair(K, layers, board, n_skip)
    B = 16
    X = _planes(B, board, 1)
    lab = np.random.RandomState(2).randint(0, board * board, B)
    Y = np.zeros((B, board * board), np.float32)
    Y[np.arange(B), lab] = 1
    for m in (cpu.model, gpu.model):
        m.compile(loss="categorical_crossentropy", optimizer=KZ.SGD(lr=0.0))
    assert gpu.model._plan_for().trunk.bn_axis == 1
    r_cpu = cpu.model.train_on_batch(X, Y)
    r_gpu = gpu.model.train_on_batch(X, Y)
    print("loss cpu %.6f gpu %.6f" % (r_cpu, r_gpu))
    assert abs(r_cpu - r_gpu) < 0.05 * abs(r_cpu)
    assert_grads_close(cpu.model.net, gpu.model.net, slots=K)


def dual_pair(seed=3):
    cfg = dict(SMALL, bn_axis=1)
    gpu = ResnetPolicyValue(DEFAULT_FEATURES, device="cuda", seed=seed, **cfg)
    cpu = ResnetPolicyValue(DEFAULT_FEATURES, device="cpu", seed=seed, **cfg)
    ws = randomised(cpu.model, seed)
    cpu.model.set_weights(ws)
    gpu.model.set_weights(ws)
    return cpu, gpu


def test_channel_dual_forward_matches_generic(ops, column_before):
    """forward_both against the generic executor: the policy within the ResNet bounds; the value
    within 1e-5 (tests/test_resnet_dual_gpu.py's bound) of the float64 heads on the plan's own
    trunk output, and within 2e-2 of the generic executor's: the value is a tanh (slope <= 1) of
    the same bf16 trunk output whose softmax is held to 2e-2."""
    from rocalphago_amd.models.fused import ResnetDualPlan
    cpu, gpu = dual_pair()
    plan = gpu.model._plan_for()
    assert type(plan) is ResnetDualPlan and plan.trunk.bn_axis == 1
    B = 6
    X = planes(np.random.RandomState(6), B, 9)
    rp, rv = cpu.forward_both(X)
    gp, gv = gpu.forward_both(X)
    assert_policy_close(np.asarray(rp), np.asarray(gp))
    own = float((torch.from_numpy(np.asarray(gv)).double()
                 - head_values(ops, plan, B).cpu()).abs().max())
    err = np.abs(np.asarray(rv).reshape(-1) - np.asarray(gv).reshape(-1)).max()
    print("values: %.3g against float64 heads on the plan's trunk, %.3g against generic"
          % (own, err))
    assert own <= 1e-5
    assert err < 2e-2
    assert np.abs(np.asarray(gv)).max() > 1e-3


def test_channel_dual_train_step_matches_generic(ops, column_before):
    """One (categorical_crossentropy, 0.5 mse) step at lr = 0, as
    test_resnet_dual_gpu.test_train_step_matches_generic with its targets and bounds."""
    cpu, gpu = dual_pair()
    B, S = 16, 9
    rng = np.random.RandomState(1)
    X = planes(rng, B, S)
    Yp = one_hot_rows(rng, B, S * S)
    Yv = rng.uniform(0.5, 1, (B, 1)).astype(np.float32)
    for m in (cpu.model, gpu.model):
        m.compile(loss=["categorical_crossentropy", "mse"], optimizer=KZ.SGD(lr=0.0),
                  loss_weights=[1.0, 0.5])
    assert gpu.model._plan_for().trunk.bn_axis == 1
    r_cpu = cpu.model.train_on_batch(X, [Yp, Yv])
    r_gpu = gpu.model.train_on_batch(X, [Yp, Yv])
    print("losses cpu %r gpu %r" % (r_cpu, r_gpu))
    for a, b in zip(r_cpu[:3], r_gpu[:3]):
        assert abs(a - b) < 0.05 * abs(a), (r_cpu, r_gpu)
    assert_grads_close(cpu.model.net, gpu.model.net, slots=32)


def test_policy_value_trainer_runs_channel_model(ops, column_before):
    """The SL trainer with visit targets and a value weight takes the channel model as it is:
    the fused plan, finite metrics, weights that move."""
    from rocalphago_amd.models.fused import ResnetDualPlan
    from rocalphago_amd.training import supervised as sl
    from rocalphago_amd.training.data import DeviceDataset
    dev = torch.device("cuda")
    net = ResnetPolicyValue(DEFAULT_FEATURES, dense=64, device=dev, seed=5, bn_axis=1, **SMALL)
    model = net.model
    model.compile(loss=["categorical_crossentropy", "mse"], optimizer=KZ.SGD(lr=0.01),
                  loss_weights=[1.0, 0.5], metrics=["accuracy"])
    ds = DeviceDataset.synthetic(32, 48, 9, dev, seed=7, visits=True, outcomes=True)
    tr = sl.PolicyValueTrainer(model, ds, 8, ["noop", "rot90"], None, seed=3, targets="visits",
                               value_weight=0.5)
    assert type(tr.plan) is ResnetDualPlan and tr.plan.trunk.bn_axis == 1
    before = model.net.flat.clone()
    index = torch.tensor([5, 0, 31, 7, 7, 12, 20, 1], device=dev)
    tr.step(index)
    tr.step(index.flip(0))
    m = tr.pop_metrics()
    assert len(m) == 3 and all(np.isfinite(m)) and m[0] > 0
    assert not torch.equal(before, model.net.flat)


def test_mixed_axes_run_the_generic_executor(ops, column_before):
    from rocalphago_amd.models.fused import detect_plan
    net = ResnetPolicy(DEFAULT_FEATURES, device="cuda", seed=3, **SMALL)
    L = list(net.model.layers)
    bns = [ld for ld in L if ld.class_name == "BatchNormalization"]
    bns[1].config["axis"] = 1
    m = KZ.Model(L, functional=True, inputs=net.model.net.input_names,
                 outputs=net.model.net.output_names, device="cuda", seed=1)
    assert detect_plan(m) is None
    for ld in bns:
        ld.config["axis"] = -3
    m = KZ.Model(L, functional=True, inputs=net.model.net.input_names,
                 outputs=net.model.net.output_names, device="cuda", seed=1)
    assert detect_plan(m).trunk.bn_axis == 1


def test_column_checkpoint_in_channel_model_raises(ops, column_before):
    """A column checkpoint (board 19, width 64: BN arrays of 19) loaded into a channel model of
    another board and width (9, 32: BN arrays of 32) raises; nothing runs."""
    col = ResnetPolicy(DEFAULT_FEATURES, device="cuda", seed=3, board=19, filters_per_layer=64,
                       layers=4)
    ch = ResnetPolicy(DEFAULT_FEATURES, device="cuda", seed=3, bn_axis=1, **SMALL)
    with pytest.raises(ValueError):
        ch.model.set_weights(col.model.get_weights())
    # and a trunk handed arrays of the other kind refuses to be built
    from rocalphago_amd.models.engine import BNSpec, ConvSpec, ResTrunk
    dev = torch.device("cuda")
    specs = [ConvSpec(3, 48, 32, False), ConvSpec(3, 32, 32, False)]
    nine = [torch.ones(9, device=dev) for _ in range(4)]
    with pytest.raises(ValueError):
        ResTrunk(specs, [1], [BNSpec(1e-3, 0.99, nine, nine[:2])], 9, dev, bn_axis=1)
    wide = [torch.ones(32, device=dev) for _ in range(4)]
    with pytest.raises(ValueError):
        ResTrunk(specs, [1], [BNSpec(1e-3, 0.99, wide, wide[:2])], 9, dev, bn_axis=-1)
    ResTrunk(specs, [1], [BNSpec(1e-3, 0.99, wide, wide[:2])], 9, dev, bn_axis=1)
