"""The policy-value network in the search, on the CPU: one evaluation per leaf fills priors and
values, lmbda is not forced to rollouts, and a separate value network is refused."""
import numpy as np
import pytest

from rocalphago_amd._native import engine
from rocalphago_amd.engine.gamestate import GameState
from rocalphago_amd.models.policy_value import CNNPolicyValue
from rocalphago_amd.models.value import CNNValue
from rocalphago_amd.search.apv import NetworkEvaluator, ParallelMCTS, ParallelMCTSPlayer

rg = engine()
FEATURES = ["board", "ones", "sensibleness", "color"]
S = 7


@pytest.fixture(scope="module")
def dual():
    return CNNPolicyValue(FEATURES, board=S, layers=2, filters_per_layer=8, dense=16,
                          device="cpu", seed=11)


def positions():
    out = []
    for moves in ([], [(3, 3)], [(3, 3), (2, 4), (4, 4)], [(0, 0), (6, 6), (1, 5), (5, 1)]):
        st = GameState(size=S)
        for mv in moves:
            st.do_move(mv)
        out.append(st)
    return out


def test_evaluator_returns_both_heads_from_one_forward(dual, monkeypatch):
    states = positions()
    boards = [st.native for st in states]
    planes = dual.preprocessor.states_to_tensor_u8(states)
    want_p, want_v = dual.forward_both(planes)
    calls = []
    predict = dual.model.predict
    monkeypatch.setattr(dual.model, "predict",
                        lambda X, *a, **k: calls.append(len(X)) or predict(X, *a, **k))
    ev = NetworkEvaluator(policy=dual)
    assert ev.dual and ev.value is dual
    for rep in range(2):
        priors, values, sens = ev(boards)
        assert len(calls) == rep + 1 and calls[-1] == len(boards)
        assert priors.shape == (len(boards), S * S) and values.shape == (len(boards),)
        assert priors.dtype == np.float32 and values.dtype == np.float32
        assert np.array_equal(priors, want_p) and np.array_equal(values, want_v)
        assert np.array_equal(sens, planes[:, 4].reshape(len(boards), -1))
    got = ev.submit(boards).result()  # no fused plan on the CPU: the same synchronous pass
    assert len(calls) == 3
    assert np.array_equal(got[0], want_p) and np.array_equal(got[1], want_v)


def test_search_uses_the_value_head(dual):
    mcts = ParallelMCTS(policy=dual, lmbda=0.0, n_playout=32, batch=8, seed=2)
    assert mcts.lmbda == 0.0  # a value head is present: not forced to rollouts only
    assert mcts.evaluator.dual
    st = GameState(size=S)
    st.do_move((3, 3))
    move = mcts.get_move(st)
    assert move is None or st.is_legal(move)
    assert move is not None
    player = ParallelMCTSPlayer(dual, lmbda=0.25, n_playout=16, batch=8)
    assert player.mcts.lmbda == 0.25


def test_dual_policy_with_a_value_network_raises(dual):
    val = CNNValue(FEATURES, board=S, layers=2, filters_per_layer=8, dense=16, device="cpu",
                   seed=1)
    with pytest.raises(ValueError):
        NetworkEvaluator(policy=dual, value=val)
    with pytest.raises(ValueError):
        ParallelMCTS(policy=dual, value=val, n_playout=8, batch=8)
