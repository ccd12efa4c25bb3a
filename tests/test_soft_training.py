"""Training the policy on search visit distributions: the fused plan's dense-target step
(models/fused.py), the trainer's ``--targets visits`` mode (training/supervised.py) and the
self-play generator that writes the visit rows (training/search_data.py)."""
import json
import os

import numpy as np
import pytest
import torch

from rocalphago_amd.features.preprocessing import DEFAULT_FEATURES
from rocalphago_amd.io import h5lite
from rocalphago_amd.models import kerasish as K
from rocalphago_amd.models.policy import CNNPolicy
from rocalphago_amd.training import search_data
from rocalphago_amd.training import supervised as sl
from rocalphago_amd.training.data import DeviceDataset, label_transform_table, soft_targets_np

gpu = pytest.mark.gpu


def soft_rows(rng, B, C, points=10):
    """Rows that sum to 1 over ``points`` random classes."""
    Y = np.zeros((B, C), np.float32)
    for b in range(B):
        w = rng.rand(points) + 0.1
        Y[b, rng.choice(C, size=points, replace=False)] = w / w.sum()
    return Y


# ----------------------------------------------------------------------------------- GPU

@gpu
@pytest.mark.parametrize("pass_logit", [False, True], ids=["nopass", "pass"])
def test_policy_soft_train_step_matches_cpu(cuda, pass_logit):
    """A dense y under categorical cross-entropy stays on the fused plan (train_step returns a
    value: before the soft head it returned None and the generic executor ran), and the step
    matches the CPU model within test_policy_train_step_matches_cpu's tolerances.

    The learning rate is 0.01, not that test's 0.1. The tolerance's floor, 2e-2 * 1e-3 = 2e-5,
    is absolute, and the bf16 trunk's ReLU masks differ from the fp32 CPU model's at a few
    activations near zero, whatever the targets. One flipped mask under a target point moves
    a last-layer bias by lr (t / B) |w_head| <= lr * (0.18 / 8) * 0.05 = 1.1e-3 lr: at lr 0.1
    five times the floor for one flip, and dense rows put 80 target points x 32 channels at risk
    where one-hot rows put 8 x 32 (measured at lr 0.1: 7.8e-5 on that bias, while the head's
    own arrays agreed to 0.4 %). lr 0.01 keeps a flip at half the floor. What the floor then no
    longer sees is asked of the arrays no mask lies behind (head conv, Bias, PassLogit): within
    2e-2 of their own largest update."""
    kw = dict(filters_per_layer=32, layers=3, seed=3, pass_logit=pass_logit)
    g = CNNPolicy(DEFAULT_FEATURES, device="cuda", **kw)
    c = CNNPolicy(DEFAULT_FEATURES, device="cpu", **kw)
    c.model.set_weights(g.model.get_weights())
    for m in (g, c):
        m.model.compile(loss="categorical_crossentropy", optimizer=K.SGD(lr=0.01))
    w0 = [w.copy() for w in c.model.get_weights()]
    rng = np.random.RandomState(0)
    X = (rng.rand(8, 48, 19, 19) > 0.6).astype(np.float32)
    Y = soft_rows(rng, 8, 361 + int(pass_logit))
    plan = g.model._plan_for()
    assert plan is not None
    before = g.model.net.flat.clone()
    r = plan.train_step(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(),
                        "categorical_crossentropy")
    assert r is not None, "a dense target left the fused plan"
    assert torch.equal(before, g.model.net.flat)  # train_step alone applies no update
    assert plan.train_step(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), "mse") is None
    lg = g.model.train_on_batch(X, Y)
    lc = c.model.train_on_batch(X, Y)
    assert abs(r[0] - lg) < 1e-6 * abs(lg)
    assert abs(lg - lc) < 1e-2 * abs(lc)
    wg, wc = g.model.get_weights(), c.model.get_weights()
    for a, b in zip(wg, wc):
        assert np.abs(a - b).max() < 2e-2 * max(1e-3, np.abs(b).max())
    checked = 0
    for a, b, w in list(zip(wg, wc, w0))[2 * 3:]:  # past the three trunk layers' (W, b)
        update = np.abs(b - w).max()
        if update > 1e-3 * 0.01:  # (the head conv's scalar bias: sum dz = 0 without a pass logit)
            assert np.abs(a - b).max() < 2e-2 * update, (a.shape, update)
            checked += 1
    assert checked >= 2


@gpu
def test_trainer_step_on_visits(cuda):
    """One SupervisedTrainer.step in visits mode on a 9x9 synthetic dataset: the head's loss and
    dz equal head_soft_ref on the logits head_linear(trunk output) + pbias and the host-built
    targets (visits[index] through soft_targets_np with sl_batch's transforms for the same seed
    and iteration), within the soft head's bounds."""
    from test_head_exact import head_errors
    from test_head_soft import head_soft_ref, soft_bounds
    from rocalphago_amd.ops import hipops as ops
    S, B = 9, 8
    policy = CNNPolicy(DEFAULT_FEATURES, board=S, filters_per_layer=32, layers=3, device=cuda,
                       seed=5)
    model = policy.model
    model.compile(loss="categorical_crossentropy", optimizer=K.SGD(lr=0.01), metrics=["accuracy"])
    ds = DeviceDataset.synthetic(32, 48, S, cuda, seed=7, visits=True)
    assert ds.visits.shape == (32, S * S + 1) and ds.visits.dtype == torch.uint16
    tr = sl.SupervisedTrainer(model, ds, B, ["noop", "rot90", "fliplr", "diag2"], None, seed=3,
                              targets="visits")
    plan = tr.plan
    assert plan is not None and tr.classes == S * S
    index = torch.tensor([5, 0, 31, 7, 7, 12, 20, 1], device=cuda)
    w, b0 = (t.clone() for t in plan.head_params())
    pb = model.net.params_of(plan.bias_name)[0].clone()
    it = model.optimizer.iterations
    tf, _ = ops.sl_batch(index, ds.labels, ds.tf_table, tr.sym, tr.seed, it)
    tr.step(index)
    zlin = torch.empty(B, S * S, device=cuda)
    ops.head_linear(plan.trunk.output(B), w, b0, zlin, plan.K)
    z = (zlin + pb).double()
    rows = ds.visits.cpu().numpy()[index.cpu().numpy()]
    t = soft_targets_np(rows, tf.cpu().numpy(), label_transform_table(S), S * S)
    assert np.allclose(t.sum(1), 1, atol=1e-6)
    ref = head_soft_ref(z, torch.from_numpy(t).to(cuda), None, float(np.float32(1.0 / B)))
    got = dict(probs=plan.head.probs[:B], loss=plan.head.loss[:B], dz=plan.head.dz[:B],
               hit=plan.head.hit[:B], dzsum=plan.head.dzsum[:B])
    err = head_errors(ref, got)
    bval, bgrad = soft_bounds()
    print("trainer step: values %.3g (bound %.3g), gradients %.3g (bound %.3g)" %
          (err["val"], bval, err["grad"], bgrad))
    assert err["val"] <= bval and err["grad"] <= bgrad, err
    assert torch.equal(got["hit"].double(), ref["hit"])
    loss, acc = tr.pop_metrics()
    assert abs(loss - ref["loss"].mean().item()) < 1e-5 * loss
    assert acc == ref["hit"].mean().item()
    # evaluate(): the soft loss and the argmax agreement, no augmentation
    vl, va = tr.evaluate(index)
    assert vl > 0 and 0 <= va <= 1
    with pytest.raises(ValueError):
        sl.SupervisedTrainer(model, DeviceDataset.synthetic(8, 48, S, cuda), B, None, None,
                             targets="visits")


# ----------------------------------------------------------------------------------- CPU

def _tiny_file(path, S, n, visits, seed=0):
    rng = np.random.RandomState(seed)
    F = 3 + 1 + 1  # board, ones, sensibleness
    with h5lite.File(path, "w") as f:
        f["states"] = (rng.rand(n, F, S, S) < 0.4).astype(np.uint8)
        acts = np.stack([rng.randint(0, S, n), rng.randint(0, S, n)], 1).astype(np.uint8)
        f["actions"] = acts
        if visits:
            v = (rng.randint(1, 30, (n, S * S + 1)) * (rng.rand(n, S * S + 1) < 0.2))
            v[np.arange(n), acts[:, 0] * S + acts[:, 1]] += 30
            f["visits"] = v.astype(np.uint16)
        f["features"] = np.bytes_("board,ones,sensibleness")


def test_run_training_on_visits(tmp_path, monkeypatch):
    """--targets visits for 2 epochs on a tiny file (CPU): metadata.json records the mode; a
    file without visits fails with the message; --targets actions on the visits file behaves as
    before."""
    monkeypatch.setenv("RAG_DEVICE", "cpu")
    S = 7
    pol = CNNPolicy(["board", "ones", "sensibleness"], board=S, filters_per_layer=8, layers=2,
                    device="cpu", seed=1)
    spec = str(tmp_path / "p.json")
    pol.save_model(spec, str(tmp_path / "p.hdf5"))
    data, plain = str(tmp_path / "v.h5"), str(tmp_path / "a.h5")
    _tiny_file(data, S, 24, True)
    _tiny_file(plain, S, 24, False)
    common = ["--epochs", "2", "--minibatch", "4", "--train-val-test", "0.7", "0.3", "0.0",
              "--seed", "1"]
    out = str(tmp_path / "out_v")
    meta = sl.run_training([spec, data, out, "--targets", "visits"] + common)
    assert meta["targets"] == "visits" and len(meta["epochs"]) == 2
    saved = json.load(open(os.path.join(out, "metadata.json")))
    assert saved["targets"] == "visits"
    assert saved["cmd_line_args"][-1]["targets"] == "visits"
    for e in saved["epochs"]:
        assert e["loss"] > 0 and e["val_loss"] > 0 and 0 <= e["val_acc"] <= 1
    assert os.path.exists(os.path.join(out, "weights.00001.hdf5"))
    with pytest.raises(ValueError, match="visits"):
        sl.run_training([spec, plain, str(tmp_path / "out_x"), "--targets", "visits"] + common)
    # actions mode: the same results from the file with and without the visits array
    ma = sl.run_training([spec, data, str(tmp_path / "out_a")] + common)
    mb = sl.run_training([spec, plain, str(tmp_path / "out_b")] + common)
    assert ma["targets"] == "actions"
    assert ma["epochs"] == mb["epochs"]
    assert ma["epochs"] != meta["epochs"]


def test_search_data_generator(tmp_path):
    """search_data on a 7x7 board, uniform priors, 2 games of 32 playouts: the file loads
    through DeviceDataset.from_hdf5; every visits row has a positive sum of at most the playout
    count, is zero on occupied points, holds the move played in its support; no pass is
    recorded."""
    from test_apv import UniformEval
    from rocalphago_amd.search.apv import ParallelMCTS
    S, playouts = 7, 32
    feats = ["board", "ones", "sensibleness"]
    mcts = ParallelMCTS(evaluator=UniformEval(lambda b: 0.0), lmbda=0.0, n_playout=playouts,
                        batch=8, seed=3)
    out = str(tmp_path / "search.h5")
    n = search_data.generate_search_data(mcts, 2, out, size=S, features=feats,
                                         temperature_moves=4, seed=1, move_limit=20)
    assert n > 10
    with h5lite.File(out) as f:
        assert f["visits"].shape == (n, S * S + 1) and f["visits"][()].dtype == np.uint16
        assert f["actions"].shape == (n, 2)
        ds = DeviceDataset.from_hdf5(f, "cpu")
    assert ds.N == n and ds.visits.shape == (n, S * S + 1) and ds.visits.dtype == torch.uint16
    v = ds.visits.numpy().astype(np.int64)
    states = ds.states.numpy()
    labels = ds.labels.numpy()
    assert (v.sum(1) > 0).all() and (v.sum(1) <= playouts).all()
    occupied = (states[:, 0] + states[:, 1]).reshape(n, S * S) > 0  # board: own, opponent stones
    assert occupied.any() and (v[:, :S * S][occupied] == 0).all()
    assert (labels < S * S).all()
    assert (v[np.arange(n), labels] > 0).all()
    X, Y = ds.host_batch(torch.arange(n), torch.zeros(n, dtype=torch.int32), soft=True,
                         classes=S * S + 1)
    assert np.allclose(Y.sum(1), 1, atol=1e-6)
