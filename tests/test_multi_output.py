"""Multi-output functional models on the generic executor, CNNPolicyValue, and the float64
reference of the two-head backward kernel (ops.head_bwd2) that tests/test_head_dual_exact.py
holds the GPU kernel to. Nothing here needs a GPU."""
import json

import numpy as np
import pytest
import torch

from rocalphago_amd.models import kerasish as K
from rocalphago_amd.models.nn_util import Bias, NeuralNetBase
from rocalphago_amd.models.policy import CNNPolicy
from rocalphago_amd.models.policy_value import CNNPolicyValue
from test_head_exact import F64, head_bwd_ref, head_logits, head_operands

FEATURES = ["board", "ones", "sensibleness", "color"]


# ------------------------------------------------------------- a two-output functional model

def two_output_model(seed=3, S=5, F=3, C=4, D=6):
    """Input -> conv 3x3 relu -> {1x1 conv, Flatten, Bias, softmax | 1x1 conv, Flatten,
    Dense(D, relu), Dense(1, tanh)} on the CPU."""
    layers = []

    def add(layer, inbound):
        layer.inbound = list(inbound)
        layers.append(layer)
        return layer.name

    inp = K.Layer("InputLayer", {"name": K._auto_name("input"),
                                 "batch_input_shape": [None, F, S, S]})
    layers.append(inp)
    t = add(K.Convolution2D(C, 3, 3, init="uniform", activation="relu", border_mode="same"),
            [inp.name])
    p = add(K.Convolution2D(1, 1, 1, init="uniform", border_mode="same"), [t])
    p = add(K.Flatten(), [p])
    p = add(Bias(), [p])
    p = add(K.Activation("softmax"), [p])
    v = add(K.Convolution2D(1, 1, 1, init="uniform", border_mode="same"), [t])
    v = add(K.Flatten(), [v])
    v = add(K.Dense(D, init="uniform", activation="relu"), [v])
    v = add(K.Dense(1, init="uniform", activation="tanh"), [v])
    return K.Model(layers, functional=True, inputs=[inp.name], outputs=[p, v], device="cpu",
                   seed=seed)


def batch(B=6, S=5, F=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand((B, F, S, S), generator=g)
    Yp = torch.rand((B, S * S), generator=g)
    Yp = Yp / Yp.sum(1, keepdim=True)
    Yv = torch.randint(0, 2, (B, 1), generator=g).float() * 2 - 1
    return X.numpy(), Yp.numpy(), Yv.numpy()


def hand_forward(params, x):
    """The same graph written out in torch."""
    Wt, bt, Wp, bp, pb, Wv, bv, W1, b1, W2, b2 = params
    h = torch.relu(torch.nn.functional.conv2d(x, Wt, bt, padding=1))
    zp = torch.nn.functional.conv2d(h, Wp, bp).reshape(x.shape[0], -1) + pb
    zv = torch.nn.functional.conv2d(h, Wv, bv).reshape(x.shape[0], -1)
    v = torch.tanh(torch.relu(zv @ W1 + b1) @ W2 + b2)
    return torch.softmax(zp, -1), v


def test_forward_returns_outputs_in_order():
    m = two_output_model()
    X, _, _ = batch()
    outs = m.net.forward(torch.from_numpy(X))
    assert isinstance(outs, list) and len(outs) == 2
    p, v = hand_forward([w.clone() for w in m.net._views], torch.from_numpy(X))
    assert torch.allclose(outs[0], p, atol=1e-7) and torch.allclose(outs[1], v, atol=1e-7)
    pred = m.predict(X, batch_size=4)  # chunked: 4 + 2 rows
    assert isinstance(pred, list) and pred[0].shape == (6, 25) and pred[1].shape == (6, 1)
    assert np.allclose(pred[0], p.numpy(), atol=1e-7) and np.allclose(pred[1], v.numpy(),
                                                                      atol=1e-7)
    assert m.output_shape == [(None, 25), (None, 1)]


def test_train_on_batch_total_and_gradients_match_autograd():
    m = two_output_model()
    wts = [2.0, 0.5]
    m.compile(loss=["categorical_crossentropy", "mse"], optimizer=K.SGD(lr=0.1),
              loss_weights=wts, metrics=["accuracy"])
    X, Yp, Yv = batch()
    before = [w.clone() for w in m.net._views]
    params = [w.clone().requires_grad_() for w in before]
    p, v = hand_forward(params, torch.from_numpy(X))
    lp = -(torch.from_numpy(Yp) * torch.log(p.clamp(1e-7, 1 - 1e-7))).sum(-1).mean()
    lv = ((v - torch.from_numpy(Yv)) ** 2).mean()
    total = wts[0] * lp + wts[1] * lv
    grads = torch.autograd.grad(total, params)
    lp, lv, total = lp.item(), lv.item(), total.item()
    r = m.train_on_batch(X, [Yp, Yv])
    assert len(r) == 4
    assert abs(r[1] - lp) < 1e-6 and abs(r[2] - lv) < 1e-6
    assert abs(r[0] - (wts[0] * r[1] + wts[1] * r[2])) < 1e-6
    assert abs(r[0] - total) < 1e-6
    assert r[3] == float((torch.from_numpy(Yp).argmax(-1) == p.argmax(-1)).float().mean())
    for gv, g, w0, w1 in zip(m.net._gviews, grads, before, m.net._views):
        assert float((gv - g).abs().max()) < 1e-6
        assert torch.allclose(w1, w0 - 0.1 * g, atol=1e-6)
    t = m.test_on_batch(X, [Yp, Yv])
    assert len(t) == 4 and abs(t[0] - (wts[0] * t[1] + wts[1] * t[2])) < 1e-6


def test_loss_weights_default_to_one():
    m = two_output_model()
    m.compile(loss=["categorical_crossentropy", "mse"], optimizer=K.SGD(lr=0.0))
    X, Yp, Yv = batch()
    r = m.train_on_batch(X, [Yp, Yv])
    assert len(r) == 3 and abs(r[0] - (r[1] + r[2])) < 1e-6


def test_single_loss_for_two_outputs_raises():
    m = two_output_model()
    with pytest.raises(ValueError):
        m.compile(loss="categorical_crossentropy", optimizer=K.SGD())
    with pytest.raises(ValueError):
        m.compile(loss=["categorical_crossentropy"], optimizer=K.SGD())
    with pytest.raises(ValueError):
        m.compile(loss=["categorical_crossentropy", "mse"], optimizer=K.SGD(),
                  loss_weights=[1.0])


def test_json_and_weights_round_trip(tmp_path):
    m = two_output_model()
    spec = json.loads(m.to_json())
    assert len(spec["config"]["output_layers"]) == 2
    m2 = K.model_from_json(m.to_json(), device="cpu")
    assert m2.net.output_names == m.net.output_names
    path = str(tmp_path / "w.hdf5")
    m.save_weights(path)
    m2.load_weights(path)
    X, _, _ = batch()
    a, b = m.predict(X), m2.predict(X)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert m2.to_json() == m.to_json()


# --------------------------------------------------------------------------- CNNPolicyValue

def small_dual(**kw):
    args = dict(board=7, layers=2, filters_per_layer=8, dense=16, device="cpu", seed=5)
    args.update(kw)
    return CNNPolicyValue(FEATURES, **args)


def test_policy_value_layer_order():
    net = small_dual(layers=3)
    classes = [ld.class_name for ld in net.model.layers]
    assert classes == ["InputLayer", "Convolution2D", "Convolution2D", "Convolution2D",
                       "Convolution2D", "Flatten", "Bias", "Activation",
                       "Convolution2D", "Flatten", "Dense", "Dense"]
    L = net.model.layers
    assert L[1].config["nb_row"] == 5 and L[2].config["nb_row"] == 3
    assert L[4].inbound == [L[3].name] and L[8].inbound == [L[3].name]
    assert L[7].config["activation"] == "softmax" and L[11].config["activation"] == "tanh"
    assert L[10].config["output_dim"] == 16 and L[10].config["activation"] == "relu"
    assert net.model.net.output_names == [L[7].name, L[11].name]
    assert net.model.output_shape == [(None, 49), (None, 1)]
    # trunk parameters first in the flat buffer
    names = [ln for ln, _, _ in net.model.net.weight_names]
    assert names[:6] == [L[1].name] * 2 + [L[2].name] * 2 + [L[3].name] * 2
    assert isinstance(net, CNNPolicy) and "CNNPolicyValue" in NeuralNetBase.subclasses
    assert net.preprocessor.feature_list == FEATURES
    from rocalphago_amd.features.preprocessing import VALUE_FEATURES
    assert CNNPolicyValue(init_network=False).preprocessor.feature_list == VALUE_FEATURES
    import AlphaGo.models.policy_value as shim
    assert shim.CNNPolicyValue is CNNPolicyValue


def test_policy_value_forward_and_eval():
    from rocalphago_amd.engine.gamestate import GameState
    net = small_dual()
    st = GameState(size=7)
    st.do_move((3, 3))
    x = net.preprocessor.states_to_tensor_u8([st, GameState(size=7)])
    p, v = net.forward_both(x)
    assert p.shape == (2, 49) and v.shape == (2,)
    assert np.allclose(p.sum(1), 1, atol=1e-6) and bool((np.abs(v) <= 1).all())
    assert np.array_equal(net.forward(x), p)
    assert np.array_equal(net.forward_device(torch.from_numpy(x)).numpy(), p)
    moves = net.eval_state(st)
    assert len(moves) == len(st.get_legal_moves())
    assert abs(sum(pr for _, pr in moves) - 1) < 1e-6
    assert abs(net.eval_value(st) - float(v[0])) < 1e-7
    assert np.allclose(net.batch_eval_value([st, GameState(size=7)]), v, atol=1e-7)
    assert net.batch_eval_value([]).shape == (0,)


def test_policy_value_save_load(tmp_path):
    net = small_dual()
    jf, wf = str(tmp_path / "pv.json"), str(tmp_path / "pv.hdf5")
    net.save_model(jf, wf)
    net2 = NeuralNetBase.load_model(jf, device="cpu")
    assert type(net2) is CNNPolicyValue
    x = np.random.RandomState(0).randint(0, 2, (3, net.preprocessor.output_dim, 7, 7))
    x = x.astype(np.uint8)
    a, b = net.forward_both(x), net2.forward_both(x)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(net2.forward(x), a[0])


def test_policy_value_refuses_pass_logit():
    with pytest.raises(ValueError):
        small_dual(pass_logit=True)


# ------------------------------------------------- the float64 reference of ops.head_bwd2

def head_bwd2_ref(H, wp, wv, dzp, dzv, relu_mask=True):
    """head_bwd_ref with two (w, dz) pairs on one H: dH = (dzp wp + dzv wv) (H > 0),
    (dwp, dwv), dpbias = sum_b dzp, db0p = sum dzp, db0v = sum dzv; the sum of the two heads'
    dH must itself be exact in bf16 (|.| <= 32/64 in 1/64 steps on head_operands)."""
    dhp, dwp, dpb, db0p = head_bwd_ref(H, wp, dzp, relu_mask)
    dhv, dwv, _, db0v = head_bwd_ref(H, wv, dzv, relu_mask)
    dH = dhp + dhv
    assert bool((dH.float().to(torch.bfloat16).double() == dH).all())
    assert dH.abs().max().item() <= 0.5
    return dH, dwp, dwv, dpb, db0p, db0v


def test_head_bwd2_reference_matches_autograd():
    """The closed form against autograd of zp = relu(x) . wp + b0p + pbias and
    zv = relu(x) . wv + b0v on 3x3 boards (x = H where H > 0, negative elsewhere)."""
    S, K, B = 3, 8, 2
    H, wp, b0p, dzp = head_operands(21, S, K, B, "cpu")
    _, wv, b0v, dzv = head_operands(22, S, K, B, "cpu")
    assert not torch.equal(wp, wv) and not torch.equal(dzp, dzv)
    x = torch.where(H > 0, H, -torch.ones_like(H)).requires_grad_()
    ps = [t.clone().requires_grad_() for t in (wp, wv, b0p, b0v)]
    pb = torch.zeros(S * S, dtype=F64, requires_grad=True)
    hr = torch.relu(x).view(B, S * S, K)
    zp = (hr * ps[0]).sum(-1) + ps[2] + pb
    zv = (hr * ps[1]).sum(-1) + ps[3]
    ((zp * dzp).sum() + (zv * dzv).sum()).backward()
    dH, dwp, dwv, dpb, db0p, db0v = head_bwd2_ref(H, wp, wv, dzp, dzv)
    assert torch.equal(dH, x.grad)
    assert torch.equal(dwp, ps[0].grad) and torch.equal(dwv, ps[1].grad)
    assert torch.equal(dpb, pb.grad)
    assert torch.equal(db0p.view(1), ps[2].grad) and torch.equal(db0v.view(1), ps[3].grad)
    assert torch.equal(head_logits(H, wv, b0v), zv.detach())
    # without the mask: the plain sum of the two outer products
    dHn = head_bwd2_ref(H, wp, wv, dzp, dzv, relu_mask=False)[0]
    assert torch.equal(dHn, dzp.view(B, S, S, 1) * wp + dzv.view(B, S, S, 1) * wv)
    assert bool((dHn != dH).any())
