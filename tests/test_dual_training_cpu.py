"""Game outcomes in the search dataset and training a policy-value network on them, on the
CPU (the generic executor; the fused step is checked in tests/test_dual_plan_gpu.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from rocalphago_amd.io import h5lite
from rocalphago_amd.models.policy import CNNPolicy
from rocalphago_amd.models.policy_value import CNNPolicyValue
from rocalphago_amd.training import search_data, supervised
from rocalphago_amd.training.data import DeviceDataset

S = 7
FEATURES = ["board", "ones", "sensibleness"]


@pytest.fixture(scope="module")
def search_file(tmp_path_factory):
    """test_search_data_generator's set-up: 7x7, uniform priors, 2 games of 32 playouts."""
    from test_apv import UniformEval
    from rocalphago_amd.search.apv import ParallelMCTS
    mcts = ParallelMCTS(evaluator=UniformEval(lambda b: 0.0), lmbda=0.0, n_playout=32, batch=8,
                        seed=3)
    out = str(tmp_path_factory.mktemp("dual") / "search.h5")
    n = search_data.generate_search_data(mcts, 2, out, size=S, features=FEATURES,
                                         temperature_moves=4, seed=1, move_limit=20)
    return out, n


def test_search_data_records_outcomes(search_file):
    out, n = search_file
    assert n > 10
    with h5lite.File(out) as f:
        o = f["outcomes"][()]
        states = f["states"][()]
        ds = DeviceDataset.from_hdf5(f, "cpu")
    assert o.shape == (n,) and o.dtype == np.int8
    assert set(np.unique(o).tolist()) <= {-1, 0, 1}
    assert ds.outcomes.shape == (n, 1) and ds.outcomes.dtype == torch.float32
    assert np.array_equal(ds.outcomes.numpy().reshape(-1), o.astype(np.float32))
    # a game starts from the empty board; within it the mover alternates between consecutive
    # recorded plies unless a pass (not recorded) came between: stones on the board grow by
    # one per recorded ply of the same game when no pass and no capture intervened
    stones = (states[:, 0] + states[:, 1]).reshape(n, -1).sum(1)
    starts = [i for i in range(n) if stones[i] == 0]
    assert len(starts) == 2 and starts[0] == 0
    checked = 0
    for g, a in enumerate(starts):
        b = starts[g + 1] if g + 1 < len(starts) else n
        game = o[a:b]
        assert len(set(np.abs(game).tolist())) == 1  # one result per game
        for i in range(a, b - 1):
            if stones[i + 1] == stones[i] + 1 and o[i] != 0:  # alternating movers
                assert o[i + 1] == -o[i]
                checked += 1
    assert checked > 5


def dual_model(tmp_path, cls=CNNPolicyValue, **kw):
    net = cls(FEATURES, board=S, layers=2, filters_per_layer=4, device="cpu", seed=2, **kw)
    jf = str(tmp_path / "model.json")
    net.save_model(jf, str(tmp_path / "init.hdf5"))
    return jf


def test_run_training_on_outcomes(search_file, tmp_path, monkeypatch):
    monkeypatch.setenv("RAG_DEVICE", "cpu")
    data, n = search_file
    jf = dual_model(tmp_path, dense=8)
    out = str(tmp_path / "out")
    meta = supervised.run_training([jf, data, out, "--epochs", "1", "--minibatch", "4",
                                    "--value-weight", "0.5", "--targets", "visits",
                                    "--train-val-test", "0.7", "0.3", "0", "--seed", "1"])
    with open(os.path.join(out, "metadata.json")) as f:
        disk = json.load(f)
    assert disk == json.loads(json.dumps(meta))
    assert disk["value_weight"] == 0.5
    ep = disk["epochs"][0]
    for k in ("loss", "acc", "value_loss", "val_loss", "val_acc", "val_value_loss"):
        assert math.isfinite(ep[k]), (k, ep)
    assert 0 <= ep["value_loss"] <= 4 and 0 <= ep["val_value_loss"] <= 4
    assert os.path.exists(os.path.join(out, "weights.00000.hdf5"))
    # the weights moved, both heads' included
    net0 = CNNPolicy.load_model(jf, device="cpu")
    net1 = CNNPolicy.load_model(jf, device="cpu")
    net1.model.load_weights(os.path.join(out, "weights.00000.hdf5"))
    moved = [not np.array_equal(a, b) for a, b in zip(net0.model.get_weights(),
                                                      net1.model.get_weights())]
    assert all(moved), moved


def test_dataset_without_outcomes_raises(search_file, tmp_path, monkeypatch):
    monkeypatch.setenv("RAG_DEVICE", "cpu")
    data, n = search_file
    bare = str(tmp_path / "bare.h5")
    with h5lite.File(data) as f, h5lite.File(bare, "w") as g:
        g["states"] = f["states"][()]
        g["actions"] = f["actions"][()]
        g["features"] = np.bytes_(",".join(FEATURES))
    jf = dual_model(tmp_path, dense=8)
    with pytest.raises(ValueError, match="outcomes"):
        supervised.run_training([jf, bare, str(tmp_path / "out"), "--epochs", "1"])
    ds = DeviceDataset.synthetic(8, 5, S, "cpu")
    net = CNNPolicy.load_model(jf, device="cpu")
    with pytest.raises(ValueError, match="outcomes"):
        supervised.PolicyValueTrainer(net.model, ds, 4)
    assert DeviceDataset.synthetic(8, 5, S, "cpu", outcomes=True).outcomes.abs().eq(1).all()


def test_value_weight_needs_a_policy_value_network(search_file, tmp_path, monkeypatch):
    monkeypatch.setenv("RAG_DEVICE", "cpu")
    data, n = search_file
    jf = dual_model(tmp_path, cls=CNNPolicy)
    with pytest.raises(ValueError, match="value-weight"):
        supervised.run_training([jf, data, str(tmp_path / "out"), "--epochs", "1",
                                 "--value-weight", "0.5"])
    # and without the flag the metadata of a plain policy names no value weight
    meta = supervised.run_training([jf, data, str(tmp_path / "out"), "--epochs", "1",
                                    "--minibatch", "4", "--train-val-test", "1", "0", "0"])
    assert "value_weight" not in meta and "value_weight" not in meta["cmd_line_args"][-1]
    assert "value_loss" not in meta["epochs"][0]
