"""The policy-value network's fused SL step and its two head kernels next to what they replace.

  python benchmarks/dual_bench.py [--batch 256] [--filters 192] [--layers 12] [--steps 200]

One JSON line:
  * dual_step_positions_per_s: PolicyValueTrainer.step (visit targets + outcomes) at B x 19 x 19,
    device events around ``--steps`` steps after a warm-up; policy_step / value_step: the same
    loop for a CNNPolicy (SupervisedTrainer, visit targets) and for a CNNValue plan
    (fwd_bwd + SGD) of the same width, i.e. the two networks one dual step trains;
  * head_fwd_us: one dual head forward (label and dense-target forms) against the launches it
    replaces, policy_head_fwd / policy_head_soft + head_linear; head_bwd_us: head_bwd2 against
    two head_bwd launches (which cannot share a dH: the second overwrites the first). The
    candidates alternate in the same process, several rounds, and the median round is reported.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rocalphago_amd.ops import hipops as ops  # noqa: E402


def timed(fn, iters, warmup):
    """us per call, device events around ``iters`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def alternate(cands, rounds=7, iters=500, warmup=20):
    """{name: median us} of candidates timed in turn, ``rounds`` times over."""
    runs = {k: [] for k in cands}
    for r in range(rounds):
        for k, fn in cands.items():
            runs[k].append(timed(fn, iters, warmup if r == 0 else 2))
    return {k: round(statistics.median(v), 2) for k, v in runs.items()}


def head_kernels(B, K, dev):
    S, S2 = 19, 361
    h = ops.pack_nchw(torch.randn(B, K, S, S, device=dev).relu(), 1, ops.pad_channels(K))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    wp, wv = (torch.randn(K, device=dev, generator=g) * 0.05 for _ in range(2))
    b0, pb = torch.zeros(1, device=dev), torch.zeros(S2, device=dev)
    lab = torch.randint(0, S2, (B,), device=dev, generator=g)
    t = torch.rand(B, S2, device=dev, generator=g)
    t = (t / t.sum(1, keepdim=True)).contiguous()
    probs, dz, zv = (torch.empty(B, S2, device=dev) for _ in range(3))
    loss, hit, dzsum = (torch.empty(B, device=dev) for _ in range(3))
    kw = dict(loss=loss, dz=dz, hit=hit, gscale=1.0 / B, dzsum=dzsum)

    def single_labels():
        ops.policy_head_fwd(h, wp, b0, pb, probs, K, labels=lab, mode=1, **kw)
        ops.head_linear(h, wv, b0, zv, K)

    def single_dense():
        ops.policy_head_soft(h, wp, b0, pb, probs, K, t, **kw)
        ops.head_linear(h, wv, b0, zv, K)

    fwd = alternate({
        "dual_labels": lambda: ops.policy_head_dual(h, wp, b0, pb, wv, b0, probs, zv, K,
                                                    labels=lab, mode=1, **kw),
        "single_labels_plus_linear": single_labels,
        "dual_dense": lambda: ops.policy_head_dual(h, wp, b0, pb, wv, b0, probs, zv, K,
                                                   targets=t, mode=1, **kw),
        "single_dense_plus_linear": single_dense,
    })
    dzv = torch.randn(B, S2, device=dev, generator=g) / B
    ops.policy_head_dual(h, wp, b0, pb, wv, b0, probs, zv, K, labels=lab, mode=1, **kw)
    dh, dh2 = torch.zeros_like(h), torch.zeros_like(h)
    dwp, dwv = torch.empty(K, device=dev), torch.empty(K, device=dev)
    dbp, dbv, dpb = torch.empty(1, device=dev), torch.empty(1, device=dev), torch.empty_like(pb)

    def two_single():
        ops.head_bwd(h, wp, dz, dh, dwp, dbp, dpb, K, dzsum=dzsum)
        ops.head_bwd(h, wv, dzv, dh2, dwv, dbv, None, K)

    bwd = alternate({
        "head_bwd2": lambda: ops.head_bwd2(h, wp, wv, dz, dzv, dh, dwp, dwv, dbp, dbv, dpb, K,
                                           dzsum=dzsum),
        "two_head_bwd": two_single,
    })
    return fwd, bwd


def sl_steps(B, filters, layers, steps, warmup, dev):
    from rocalphago_amd.features.preprocessing import DEFAULT_FEATURES, VALUE_FEATURES
    from rocalphago_amd.models import kerasish as K
    from rocalphago_amd.models.policy import CNNPolicy
    from rocalphago_amd.models.policy_value import CNNPolicyValue
    from rocalphago_amd.models.value import CNNValue
    from rocalphago_amd.training.data import TRANSFORM_NAMES, DeviceDataset
    from rocalphago_amd.training.supervised import PolicyValueTrainer, SupervisedTrainer
    kw = dict(board=19, filters_per_layer=filters, layers=layers, device=dev, seed=1)
    n = 4 * B
    out = {}
    index = [torch.randperm(n, device=dev)[:B] for _ in range(4)]

    def rate(step):
        k = [0]

        def one():
            step(index[k[0] % 4])
            k[0] += 1
        return round(B / (timed(one, steps, warmup) * 1e-6), 1)

    dual = CNNPolicyValue(VALUE_FEATURES, **kw).model
    dual.compile(loss=["categorical_crossentropy", "mse"], optimizer=K.SGD(lr=0.003),
                 metrics=["accuracy"])
    ds = DeviceDataset.synthetic(n, 49, 19, dev, seed=3, visits=True, outcomes=True)
    tr = PolicyValueTrainer(dual, ds, B, TRANSFORM_NAMES, None, seed=1, targets="visits")
    assert tr.plan is not None, "HIP fused plan not active"
    out["dual_step_positions_per_s"] = rate(tr.step)
    m = tr.pop_metrics()
    assert all(v == v for v in m), m
    del tr, dual

    pol = CNNPolicy(DEFAULT_FEATURES, **kw).model
    pol.compile(loss="categorical_crossentropy", optimizer=K.SGD(lr=0.003), metrics=["accuracy"])
    dsp = DeviceDataset.synthetic(n, 48, 19, dev, seed=3, visits=True)
    trp = SupervisedTrainer(pol, dsp, B, TRANSFORM_NAMES, None, seed=1, targets="visits")
    out["policy_step_positions_per_s"] = rate(trp.step)
    del trp, pol

    val = CNNValue(VALUE_FEATURES, **kw).model
    val.compile(loss="mse", optimizer=K.SGD(lr=0.003))
    plan = val._plan_for()

    def vstep(idx):
        Bp = plan.prepare(ds.states, index=idx)
        plan.fwd_bwd(Bp, ds.outcomes[idx])
        val.optimizer.apply(val.net)
    out["value_step_positions_per_s"] = rate(vstep)
    p, v = out["policy_step_positions_per_s"], out["value_step_positions_per_s"]
    out["two_networks_positions_per_s"] = round(1.0 / (1.0 / p + 1.0 / v), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--filters", type=int, default=192)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda")
    res = {"metric": "policy-value SL step (19x19, B = %d, %d filters, %d + 1 layers)"
           % (args.batch, args.filters, args.layers), "batch": args.batch}
    res.update(sl_steps(args.batch, args.filters, args.layers, args.steps, args.warmup, dev))
    fwd, bwd = head_kernels(args.batch, args.filters, dev)
    res["head_fwd_us"] = fwd
    res["head_bwd_us"] = bwd
    print(json.dumps(res))


if __name__ == "__main__":
    main()
