"""ResnetPolicyValue (models/policy_value.py) on the CPU: the residual trunk under the two
policy-value heads, through the generic fp32 executor (the fused plan is checked in
tests/test_resnet_dual_gpu.py). Shapes: board 9, 16 filters, 5 layers, n_skip_1 = 2."""
import math
import os

import numpy as np
import pytest

from rocalphago_amd.engine.gamestate import GameState
from rocalphago_amd.io import h5lite
from rocalphago_amd.models.policy import CNNPolicy, ResnetPolicy
from rocalphago_amd.models.policy_value import CNNPolicyValue, ResnetPolicyValue
from rocalphago_amd.search.apv import ParallelMCTS, is_dual
from rocalphago_amd.training import supervised

S = 9
FEATURES = ["board", "ones", "sensibleness", "color"]
ARGS = dict(board=S, filters_per_layer=16, layers=5, n_skip_1=2, device="cpu")


@pytest.fixture(scope="module")
def net():
    return ResnetPolicyValue(FEATURES, dense=16, seed=7, **ARGS)


def planes(n, seed):
    rng = np.random.RandomState(seed)
    return (rng.rand(n, 6, S, S) < 0.35).astype(np.float32)


def test_is_a_registered_policy_value_network(net):
    import AlphaGo.models.policy_value as compat
    assert compat.ResnetPolicyValue is ResnetPolicyValue
    assert isinstance(net, CNNPolicyValue) and is_dual(net)
    assert ResnetPolicyValue(board=S, filters_per_layer=4, layers=3, dense=4, device="cpu") \
        .preprocessor.feature_list == CNNPolicyValue(board=S, filters_per_layer=4, layers=2,
                                                     dense=4, device="cpu") \
        .preprocessor.feature_list  # VALUE_FEATURES by default
    names = [ld.class_name for ld in net.model.layers]
    assert names.count("BatchNormalization") == 4 and names.count("Merge") == 3
    assert names[-8:] == ["Convolution2D", "Flatten", "Bias", "Activation",
                          "Convolution2D", "Flatten", "Dense", "Dense"]
    assert net.model.layers[-1].config["activation"] == "tanh"
    assert net.model.layers[-2].config["output_dim"] == 16


def test_pass_logit_raises():
    with pytest.raises(ValueError):
        ResnetPolicyValue(FEATURES, pass_logit=True, **ARGS)


def test_save_and_load_round_trip(net, tmp_path):
    jf, wf = str(tmp_path / "m.json"), str(tmp_path / "w.hdf5")
    net.save_model(jf, wf)
    back = CNNPolicy.load_model(jf, device="cpu")
    assert type(back) is ResnetPolicyValue
    a, b = net.model.get_weights(), back.model.get_weights()
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_outputs_and_the_policy_half_is_a_resnet_policy(net):
    x = planes(5, 1)
    p, v = net.forward_both(x)
    assert p.shape == (5, S * S) and v.shape == (5,)
    pm, vm = net.model.predict(x)
    assert np.asarray(pm).shape == (5, S * S) and np.asarray(vm).shape == (5, 1)
    assert np.allclose(p.sum(1), 1.0, atol=1e-5) and (np.abs(v) < 1).all()
    # the leading weight arrays are a ResnetPolicy's of the same arguments: copied over, that
    # policy computes output 0 (the same fp32 executor)
    pol = ResnetPolicy(FEATURES, seed=3, **ARGS)
    wp = pol.model.get_weights()
    wn = net.model.get_weights()
    assert [w.shape for w in wn[:len(wp)]] == [w.shape for w in wp]
    pol.model.set_weights([w.copy() for w in wn[:len(wp)]])
    assert np.abs(np.asarray(pol.forward(x)) - p).max() <= 1e-6
    assert np.array_equal(np.asarray(net.forward(x)), p)  # a drop-in policy


def test_training_lowers_the_loss_and_moves_a_running_mean():
    from rocalphago_amd.models import kerasish as K
    net = ResnetPolicyValue(FEATURES, dense=16, seed=5, **ARGS)
    model = net.model
    model.compile(loss=["categorical_crossentropy", "mse"], optimizer=K.SGD(lr=0.05))
    rng = np.random.RandomState(2)
    x = planes(8, 4)
    yp = np.zeros((8, S * S), np.float32)
    yp[np.arange(8), rng.randint(0, S * S, 8)] = 1
    yv = rng.choice([-1.0, 1.0], (8, 1)).astype(np.float32)
    bn = next(ld.name for ld in model.layers if ld.class_name == "BatchNormalization")
    mean0 = model.net.params_of(bn)[2].clone()
    losses = [model.train_on_batch(x, [yp, yv])[0] for _ in range(4)]
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    assert not np.array_equal(mean0.numpy(), model.net.params_of(bn)[2].numpy())


def test_search_with_the_network_alone(net):
    mcts = ParallelMCTS(net, value=None, lmbda=0.0, n_playout=16, batch=8, seed=2)
    assert mcts.lmbda == 0.0 and mcts.lmbda < 1  # the value head is searched with
    assert mcts.evaluator.dual
    st = GameState(size=S)
    st.do_move((4, 4))
    move = mcts.get_move(st)
    assert move is not None and st.is_legal(move)


def test_sl_command_line_takes_a_value_weight(tmp_path, monkeypatch):
    monkeypatch.setenv("RAG_DEVICE", "cpu")
    feats = ["board", "ones", "sensibleness"]
    model = ResnetPolicyValue(feats, dense=8, seed=2, board=S, filters_per_layer=4, layers=3,
                              device="cpu")
    jf = str(tmp_path / "model.json")
    model.save_model(jf, str(tmp_path / "init.hdf5"))
    rng = np.random.RandomState(9)
    n = 12
    data = str(tmp_path / "data.h5")
    with h5lite.File(data, "w") as f:
        f["states"] = (rng.rand(n, 5, S, S) < 0.3).astype(np.uint8)
        f["actions"] = rng.randint(0, S, (n, 2)).astype(np.int32)
        f["outcomes"] = rng.choice([-1, 1], n).astype(np.int8)
        f["features"] = np.bytes_(",".join(feats))
    out = str(tmp_path / "out")
    meta = supervised.run_training([jf, data, out, "--epochs", "1", "--minibatch", "4",
                                    "--value-weight", "0.5", "--train-val-test", "0.7", "0.3",
                                    "0", "--seed", "1"])
    assert meta["value_weight"] == 0.5
    ep = meta["epochs"][0]
    for k in ("loss", "acc", "value_loss", "val_loss", "val_value_loss"):
        assert math.isfinite(ep[k]), (k, ep)
    assert os.path.exists(os.path.join(out, "weights.00000.hdf5"))
