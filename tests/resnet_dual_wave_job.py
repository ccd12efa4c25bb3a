"""One case of tests/test_resnet_dual_gpu.py::test_packed_wave_matches_board_path, run as a
process of its own (under the caller's time limit): submit_wave of a 9x9 residual policy-value
network against the board path, as tests/dual_wave_job.py does for CNNPolicyValue.
Usage: resnet_dual_wave_job.py <graph 0|1>; prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rocalphago_amd._native import engine  # noqa: E402
from rocalphago_amd.engine.gamestate import GameState  # noqa: E402
from rocalphago_amd.features.preprocessing import VALUE_FEATURES  # noqa: E402
from rocalphago_amd.models.fused import ResnetDualPlan  # noqa: E402
from rocalphago_amd.models.policy_value import ResnetPolicyValue  # noqa: E402
from rocalphago_amd.search.apv import NetworkEvaluator, _Slots  # noqa: E402

S = 9


def main(graph):
    rg = engine()
    dev = torch.device("cuda")
    net = ResnetPolicyValue(VALUE_FEATURES, board=S, filters_per_layer=32, layers=4, n_skip_1=2,
                            device=dev, seed=5)
    root = GameState(size=S)
    for mv in [(4, 4), (2, 6), (6, 2), (2, 2)]:  # an early position: 64 distinct leaves exist
        root.do_move(mv)
    ev = NetworkEvaluator(net, graph=graph)
    assert ev.wave_capable(S)
    ppol, pval = ev._plans()
    assert ppol is pval and type(ppol) is ResnetDualPlan
    slots = _Slots(dev, 2)
    s = rg.Search(root.native, 4)
    s.lmbda = 0.0
    s.parallel_select_min = 1 << 20  # serial, deterministic descents
    rs = np.random.RandomState(0)
    wid, n = s.select(1)  # expand the root first
    r0 = ev.submit(s.leaf_boards(wid)).result()
    s.backup_value(wid, np.ascontiguousarray(r0[0]), r0[1], r0[2])
    W = 64  # a full slot (slots hold at least 64 leaves): the size a graph is captured for
    for rep in range(4):  # eager, eager (graph: capture), replay, replay
        wid, n = s.select(W)
        assert n == W, n
        boards = s.leaf_boards(wid)
        ref = ev.submit(boards).result()
        got = ev.submit_wave(s, wid, n, slots, W).result()
        for g, e in zip(got, ref):
            assert g.shape == e.shape
            assert np.array_equal(g, e), rep
        if rep == 0:  # and both are the network's own outputs on these positions
            planes = ev.gpu["p"](boards)
            p, v = net.forward_both_device(planes)
            assert np.array_equal(p.cpu().numpy(), got[0])
            assert np.array_equal(v.cpu().numpy(), got[1])
            assert np.abs(got[1]).max() <= 1 and np.ptp(got[1]) > 0
        s.backup_value(wid, np.ascontiguousarray(got[0]),
                       rs.uniform(-1, 1, n).astype(np.float32), got[2])
    if graph:
        assert any(getattr(sl, "graphs", None) for sl in slots.pool), "no graph was captured"
    torch.cuda.synchronize()
    print(json.dumps({"ok": True, "graph": graph}))


if __name__ == "__main__":
    main(sys.argv[1] == "1")
