"""The residual policy-value network (ResnetPolicyValue, fused.ResnetDualPlan): its fused SL
step, the raw-top head kernels next to the ReLU pass they fold in, and the search.

  python benchmarks/resdual_bench.py [--batch 256] [--filters 128] [--layers 20] [--steps 100]
                                     [--playouts 8192] [--moves 6] [--skip-search]
                                     [--bn-axis {-1,1}]

One JSON line:
  * resdual_step_positions_per_s: PolicyValueTrainer.step (visit targets + outcomes, 49 planes)
    at B x 19 x 19 under ResnetDualPlan.RAW_TOP as it stands, resdual_step_other_top the same
    with the other setting, resnet_policy_step_positions_per_s the ResnetPolicy step
    (SupervisedTrainer, visit targets, 48 planes) of the same width, all in this process;
  * head_us[B] for B = 256 and 512 at K = --filters: the raw dual forward (labels) against
    bn_apply(relu) + the plain dual forward, and raw head_bwd2 against bn_apply(relu) +
    head_bwd2 (the pass is charged to the forward in the plan; here each pair carries it, so
    the two rows bracket its cost). The candidates alternate in the same process
    (dual_bench.alternate); ``spread`` is the largest max - min over a candidate's rounds;
  * --bn-axis 1 builds the networks with channel BatchNormalization (one statistic per
    channel; ResTrunk's channel kernels, unfused but for the Winograd forward of 128-wide
    trunks). resdual_step_column_unfused_positions_per_s is
    always the column network's step with ``bn_prologue = False`` and ``WINO_MODE = "0"``, the
    launch-for-launch counterpart of the channel step, and with --bn-axis 1
    resdual_step_column_fused_positions_per_s the column step as it ships (the distance a fused
    channel kernel would have to close);
  * bn_us: at B = 256, K = --filters, S = 19 the column and the channel form of the train-forward
    statistics, the BN + ReLU apply, the backward coefficients and the backward apply with the
    residual, each pair alternating in this process (``spread`` as above);
  * wino_bn_us[B] for B = 256 and 512 at K = 128, S = 19: the fused-BN Winograd forward forms
    with bias and residual -- the column form, the channel form without and with the next BN's
    statistics -- and the unfused channel sequence the channel form replaces (bn_ch_apply into a
    stored U + the direct 3x3 kernel), alternating in this process (``spread`` as above);
  * search_sims_per_s: ParallelMCTS(net, None) at mcts_bench.py --moves 6 --dual's geometry
    (8192 playouts, waves of 512, lambda 0.5, GPU rollouts, from the empty board);
  * with --bn-axis 1, resdual_step_ch_wino_positions_per_s and search_ch_wino_sims_per_s: the
    step and the search with the channel Winograd forward (ResTrunk.CH_WINO) ``on`` and ``off``
    in this process, taking turns (medians; ``spread`` the largest max - min over a setting's
    rounds).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from benchmarks.dual_bench import alternate, timed  # noqa: E402
from rocalphago_amd.ops import hipops as ops  # noqa: E402


def alternate_with_spread(cands, rounds=7, iters=300, warmup=20):
    """dual_bench.alternate's medians plus the largest max - min over a candidate's rounds
    (one ``alternate`` round per call, so the candidates still take turns)."""
    runs = {k: [] for k in cands}
    for r in range(rounds):
        one = alternate(cands, rounds=1, iters=iters, warmup=warmup if r == 0 else 2)
        for k, v in one.items():
            runs[k].append(v)
    med = {k: round(statistics.median(v), 2) for k, v in runs.items()}
    med["spread"] = round(max(max(v) - min(v) for v in runs.values()), 2)
    return med


def head_kernels(B, K, dev):
    S, S2 = 19, 361
    KP = ops.pad_channels(K)
    a = ops.pack_nchw(torch.randn(B, K, S, S, device=dev), 1, KP)  # the last residual sum
    h = ops.alloc_padded(B, S, 1, KP, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    wp, wv = (torch.randn(K, device=dev, generator=g) * 0.05 for _ in range(2))
    b0, pb = torch.zeros(1, device=dev), torch.zeros(S2, device=dev)
    lab = torch.randint(0, S2, (B,), device=dev, generator=g)
    probs, dz, zv = (torch.empty(B, S2, device=dev) for _ in range(3))
    loss, hit, dzsum = (torch.empty(B, device=dev) for _ in range(3))
    kw = dict(labels=lab, mode=1, loss=loss, dz=dz, hit=hit, gscale=1.0 / B, dzsum=dzsum)

    def relu_pass():
        ops.bn_apply(a, h, B, S, K, coef=None, relu=True)

    def mat_fwd():
        relu_pass()
        ops.policy_head_dual(h, wp, b0, pb, wv, b0, probs, zv, K, **kw)

    fwd = alternate_with_spread({
        "raw_dual_fwd": lambda: ops.policy_head_dual(a, wp, b0, pb, wv, b0, probs, zv, K,
                                                     relu_in=True, **kw),
        "relu_pass_plus_dual_fwd": mat_fwd,
        "dual_fwd_alone": lambda: ops.policy_head_dual(h, wp, b0, pb, wv, b0, probs, zv, K, **kw),
    })
    dzv = torch.randn(B, S2, device=dev, generator=g) / B
    dh = torch.zeros_like(h)
    dwp, dwv = torch.empty(K, device=dev), torch.empty(K, device=dev)
    dbp, dbv, dpb = torch.empty(1, device=dev), torch.empty(1, device=dev), torch.empty_like(pb)

    def bwd2(src, relu_in):
        ops.head_bwd2(src, wp, wv, dz, dzv, dh, dwp, dwv, dbp, dbv, dpb, K, dzsum=dzsum,
                      relu_in=relu_in)

    def mat_bwd():
        relu_pass()
        bwd2(h, False)

    bwd = alternate_with_spread({
        "raw_head_bwd2": lambda: bwd2(a, True),
        "relu_pass_plus_head_bwd2": mat_bwd,
        "head_bwd2_alone": lambda: bwd2(h, False),
    })
    return {"fwd": fwd, "bwd": bwd}


def bn_kernels(K, dev, B=256, S=19):
    """us per call of the four stand-alone BN kernels' column and channel forms on the same
    activations (bn.hip rag_bn_* / rag_bn_ch_*)."""
    KP = ops.pad_channels(K)
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    x, dy, res = (ops.pack_nchw(torch.randn(B, K, S, S, device=dev, generator=g), 1, KP)
                  for _ in range(3))
    out = ops.alloc_padded(B, S, 1, KP, dev)
    forms = {}
    for name, n, slots in (("column", S, S), ("channel", K, KP)):
        gamma, rvar = torch.ones(n, device=dev), torch.ones(n, device=dev)
        beta, rmean = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        forms[name] = dict(gamma=gamma, beta=beta, rmean=rmean, rvar=rvar,
                           dgamma=torch.empty(n, device=dev), dbeta=torch.empty(n, device=dev),
                           stats=torch.zeros(2, slots, device=dev),
                           coef=torch.zeros(3, slots, device=dev),
                           bcoef=torch.zeros(3, slots, device=dev))

    def train_fwd(fn, f):
        return lambda: fn(x, B, S, K, f["gamma"], f["beta"], f["rmean"], f["rvar"], 1e-3, 0.99,
                          f["stats"], f["coef"])

    def bwd_coef(fn, f):
        return lambda: fn(x, dy, B, S, K, f["gamma"], f["stats"], f["dgamma"], f["dbeta"],
                          f["bcoef"])

    def apply_relu(fn, f):
        return lambda: fn(x, out, B, S, K, coef=f["coef"], relu=True)

    def bwd_apply(fn, f):
        return lambda: fn(x, out, B, S, K, coef=f["bcoef"], relu=False, dy=dy, residual=res)

    col, ch = forms["column"], forms["channel"]
    res_us = {}
    for key, make, fcol, fch in (("train_fwd", train_fwd, ops.bn_train_fwd, ops.bn_ch_train_fwd),
                                 ("apply_relu", apply_relu, ops.bn_apply, ops.bn_ch_apply),
                                 ("bwd_coef", bwd_coef, ops.bn_bwd_coef, ops.bn_ch_bwd_coef),
                                 ("bwd_apply_residual", bwd_apply, ops.bn_apply,
                                  ops.bn_ch_apply)):
        res_us[key] = alternate_with_spread({"column": make(fcol, col), "channel": make(fch, ch)})
    return res_us


def wino_bn_kernels(dev, K=128, S=19):
    """us per call at B = 256 and 512 of the fused-BN Winograd forward forms on the same
    activations and weights (conv_wino.hip): the column form (BNM 1), the channel form (BNM 3)
    without and with the next BN's statistics, and the unfused channel sequence the channel form
    replaces (bn_ch_apply into a stored U + the direct 3x3 kernel), every one with bias and
    residual. The candidates alternate in this process."""
    out = {}
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    w = torch.randn(K, K, 3, 3, device=dev, generator=g) * 0.05
    b = torch.randn(K, device=dev, generator=g) * 0.1
    uf, _ = ops.wino_weights(w, K, K, dgrad=False)
    wf, _ = ops.pack_weights(w, K, K)
    col = torch.zeros(3, S, device=dev)
    col[0] = torch.rand(S, device=dev, generator=g) + 0.5
    col[2] = torch.randn(S, device=dev, generator=g) * 0.3
    ch = torch.zeros(3, K, device=dev)
    ch[0] = torch.rand(K, device=dev, generator=g) + 0.5
    ch[2] = torch.randn(K, device=dev, generator=g) * 0.3
    for B in (256, 512):
        assert ops.conv_wino_bn_ok(B, S, K, K), B
        x, r = (ops.pack_nchw(torch.randn(B, K, S, S, device=dev, generator=g), 1, K)
                for _ in range(2))
        y, U = ops.alloc_padded(B, S, 1, K, dev), ops.alloc_padded(B, S, 1, K, dev)
        part = torch.zeros(B, 2, K, device=dev)

        def fused(coef, B=B, x=x, r=r, y=y, **kw):
            return lambda: ops.conv_wino_bn(x, uf, b, y, B, S, K, K, False, bn_coef=coef,
                                            residual=r, **kw)

        def unfused(B=B, x=x, r=r, y=y, U=U):
            ops.bn_ch_apply(x, U, B, S, K, coef=ch, relu=True)
            ops.conv_igemm(U, wf, b, y, B, S, 1, 1, K, K, 3, False, residual=r)

        out[str(B)] = alternate_with_spread({
            "column_fwd": fused(col),
            "channel_fwd": fused(ch, bn_axis=1),
            "channel_fwd_stats": fused(ch, bn_axis=1, stat_part=part),
            "channel_apply_plus_direct": unfused,
        })
    return out


def ab_rates(make, rate, rounds=3):
    """{"on": .., "off": .., "spread": ..}: ``rate(make(switch))`` with ResTrunk.CH_WINO on and
    off, both built once and measured in alternating rounds in this process; the medians and the
    largest max - min over a setting's rounds."""
    cands = {"on": make(True), "off": make(False)}
    runs = {k: [] for k in cands}
    for _ in range(rounds):
        for k, c in cands.items():
            runs[k].append(rate(c))
    res = {k: round(statistics.median(v), 1) for k, v in runs.items()}
    res["spread"] = round(max(max(v) - min(v) for v in runs.values()), 1)
    return res


def sl_steps(B, filters, layers, steps, warmup, dev, bn_axis=-1):
    from rocalphago_amd.features.preprocessing import DEFAULT_FEATURES, VALUE_FEATURES
    from rocalphago_amd.models import kerasish as K
    from rocalphago_amd.models.engine import ResTrunk
    from rocalphago_amd.models.fused import ResnetDualPlan
    from rocalphago_amd.models.policy import ResnetPolicy
    from rocalphago_amd.models.policy_value import ResnetPolicyValue
    from rocalphago_amd.training.data import TRANSFORM_NAMES, DeviceDataset
    from rocalphago_amd.training.supervised import PolicyValueTrainer, SupervisedTrainer
    col_kw = dict(board=19, filters_per_layer=filters, layers=layers, device=dev, seed=1)
    kw = dict(col_kw, bn_axis=bn_axis)
    n = 4 * B
    out = {"raw_top": bool(ResnetDualPlan.RAW_TOP), "bn_axis": bn_axis}
    index = [torch.randperm(n, device=dev)[:B] for _ in range(4)]

    def rate(step):
        k = [0]

        def one():
            step(index[k[0] % 4])
            k[0] += 1
        return round(B / (timed(one, steps, warmup) * 1e-6), 1)

    ds = DeviceDataset.synthetic(n, 49, 19, dev, seed=3, visits=True, outcomes=True)
    default = ResnetDualPlan.RAW_TOP
    for key, raw in (("resdual_step_positions_per_s", default),
                     ("resdual_step_other_top_positions_per_s", not default)):
        ResnetDualPlan.RAW_TOP = raw
        try:
            dual = ResnetPolicyValue(VALUE_FEATURES, **kw).model
            dual.compile(loss=["categorical_crossentropy", "mse"], optimizer=K.SGD(lr=0.003),
                         metrics=["accuracy"])
            tr = PolicyValueTrainer(dual, ds, B, TRANSFORM_NAMES, None, seed=1, targets="visits")
        finally:
            ResnetDualPlan.RAW_TOP = default
        assert type(tr.plan) is ResnetDualPlan and tr.plan.trunk.top_relu_in == raw
        assert tr.plan.trunk.bn_axis == bn_axis
        out[key] = rate(tr.step)
        m = tr.pop_metrics()
        assert all(v == v for v in m), m
        del tr, dual

    # the column network without its fused BN kernels (every BN the statistics / apply / conv
    # sequence the channel trunk runs), and, next to a channel run, as it ships
    for key, fused in (("resdual_step_column_unfused_positions_per_s", False),
                       ("resdual_step_column_fused_positions_per_s", True)):
        if fused and bn_axis != 1:
            continue
        mode = ResTrunk.WINO_MODE
        ResTrunk.WINO_MODE = mode if fused else "0"
        try:
            dual = ResnetPolicyValue(VALUE_FEATURES, **col_kw).model
            dual.compile(loss=["categorical_crossentropy", "mse"], optimizer=K.SGD(lr=0.003),
                         metrics=["accuracy"])
            tr = PolicyValueTrainer(dual, ds, B, TRANSFORM_NAMES, None, seed=1, targets="visits")
        finally:
            ResTrunk.WINO_MODE = mode
        trunk = tr.plan.trunk
        assert trunk.bn_axis == -1
        if not fused:
            assert not any(trunk._wino)
            trunk.bn_prologue = False
            trunk._wino_plans.clear()
        out[key] = rate(tr.step)
        assert fused or not any(trunk._fused)
        del tr, dual, trunk

    pol = ResnetPolicy(DEFAULT_FEATURES, **kw).model
    pol.compile(loss="categorical_crossentropy", optimizer=K.SGD(lr=0.003), metrics=["accuracy"])
    dsp = DeviceDataset.synthetic(n, 48, 19, dev, seed=3, visits=True)
    trp = SupervisedTrainer(pol, dsp, B, TRANSFORM_NAMES, None, seed=1, targets="visits")
    assert trp.plan is not None, "HIP fused plan not active"
    out["resnet_policy_step_positions_per_s"] = rate(trp.step)
    del trp, pol

    if bn_axis == 1:
        # the channel Winograd forward (ResTrunk.CH_WINO) on and off: two trainers of the same
        # network, alternating rounds in this process
        def dual_trainer(switch):
            saved = ResTrunk.CH_WINO
            ResTrunk.CH_WINO = switch
            try:
                dual = ResnetPolicyValue(VALUE_FEATURES, **kw).model
                dual.compile(loss=["categorical_crossentropy", "mse"],
                             optimizer=K.SGD(lr=0.003), metrics=["accuracy"])
                tr = PolicyValueTrainer(dual, ds, B, TRANSFORM_NAMES, None, seed=1,
                                        targets="visits")
            finally:
                ResTrunk.CH_WINO = saved
            assert tr.plan.trunk.bn_axis == 1
            assert any(tr.plan.trunk._plan(B)[1]) == (switch and filters == 128)
            return tr
        out["resdual_step_ch_wino_positions_per_s"] = ab_rates(dual_trainer,
                                                               lambda tr: rate(tr.step))
    return out


def search(filters, layers, playouts, moves, dev, bn_axis=-1, ch_wino=None):
    """mcts_bench.measure's loop (it builds its own networks, so the loop is repeated here) on
    a ParallelMCTS with the residual policy-value network. ``ch_wino``: ResTrunk.CH_WINO while
    the network's plan is built (None: as it stands)."""
    from rocalphago_amd.engine.gamestate import GameState
    from rocalphago_amd.features.preprocessing import DEFAULT_FEATURES
    from rocalphago_amd.models.engine import ResTrunk
    from rocalphago_amd.models.policy_value import ResnetPolicyValue
    from rocalphago_amd.search.apv import ParallelMCTS
    saved = ResTrunk.CH_WINO
    if ch_wino is not None:
        ResTrunk.CH_WINO = ch_wino
    try:
        net = ResnetPolicyValue(DEFAULT_FEATURES + ["color"], board=19,
                                filters_per_layer=filters, layers=layers, device=dev, seed=1,
                                bn_axis=bn_axis)
        mc = ParallelMCTS(net, None, lmbda=0.5, batch=512, rollout_device="gpu",
                          rollouts_per_leaf=1, nthreads=16, seed=1, pipeline=3, max_inflight=8,
                          rollout_group=8)
        mc.n_playout = playouts
        st = GameState()
        mc.search(st, 512)  # compiles / allocates (builds the plan); discarded tree
    finally:
        ResTrunk.CH_WINO = saved
    mc._search = None
    mc.stats = {"waves": 0, "sims": 0}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(moves):
        mv = mc.get_move(st)
        st.do_move(mv)
        mc.update_with_move(mv)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"search_sims_per_s": round(mc.stats["sims"] / dt, 1), "search_sims": mc.stats["sims"],
            "search_moves": moves}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--layers", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--playouts", type=int, default=8192)
    ap.add_argument("--moves", type=int, default=6)
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-heads", action="store_true")
    ap.add_argument("--bn-axis", type=int, choices=[-1, 1], default=-1,
                    help="BatchNormalization axis of the networks: -1 column, 1 channel")
    args = ap.parse_args()
    dev = torch.device("cuda")
    res = {"metric": "residual policy-value network (19x19, B = %d, %d filters, %d layers)"
           % (args.batch, args.filters, args.layers), "batch": args.batch}
    if not args.skip_heads:
        res["head_us"] = {str(B): head_kernels(B, args.filters, dev) for B in (256, 512)}
    res["bn_us"] = bn_kernels(args.filters, dev)
    res["wino_bn_us"] = wino_bn_kernels(dev)
    if not args.skip_steps:
        res.update(sl_steps(args.batch, args.filters, args.layers, args.steps, args.warmup, dev,
                            args.bn_axis))
    if not args.skip_search:
        res.update(search(args.filters, args.layers, args.playouts, args.moves, dev,
                          args.bn_axis))
        if args.bn_axis == 1:
            # the channel Winograd forward on and off, a fresh search each, taking turns
            runs = {"on": [], "off": []}
            for _ in range(2):
                for k in runs:
                    runs[k].append(search(args.filters, args.layers, args.playouts, args.moves,
                                          dev, 1, ch_wino=k == "on")["search_sims_per_s"])
            ab = {k: round(statistics.median(v), 1) for k, v in runs.items()}
            ab["spread"] = round(max(max(v) - min(v) for v in runs.values()), 1)
            res["search_ch_wino_sims_per_s"] = ab
    print(json.dumps(res))


if __name__ == "__main__":
    main()
