"""The SL batch kernel for visit-count targets (csrc/hip/batch.hip sl_batch_soft_kernel) and its
host definition (training/data.py soft_targets_np / DeviceDataset.host_batch(soft=True))."""
import numpy as np
import pytest
import torch

from rocalphago_amd.training.data import (DeviceDataset, apply_transform_np,
                                          label_transform_table, soft_targets_np)

gpu = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rocalphago_amd.ops import hipops
    return hipops


def visit_rows(S, N, CD, seed):
    """uint16 [N, CD]: sparse counts, a saturated one, row 1 all zero, row 2 with its only
    count in the pass column (when there is one)."""
    rng = np.random.RandomState(seed)
    v = (rng.randint(0, 300, (N, CD)) * (rng.rand(N, CD) < 0.3)).astype(np.uint16)
    v[0, 3] = 65535
    v[1] = 0
    if CD == S * S + 1:
        v[2] = 0
        v[2, -1] = 9
    return v


def reference(v, tf, table, C):
    """The float64 quotient scattered through the table, in numpy."""
    N, CD = v.shape
    P = table.shape[1]
    n = min(CD, C)
    out = np.zeros((N, C), np.float64)
    for i in range(N):
        s = v[i, :n].astype(np.float64).sum()
        if s == 0:
            continue
        for p in range(n):
            out[i, table[tf[i], p] if p < P else p] = v[i, p] / s
    return out


@gpu
@pytest.mark.parametrize("nsym", [8, 1])
@pytest.mark.parametrize("form", ["both", "drop_pass", "no_count"])
@pytest.mark.parametrize("S,B", [(5, 3), (19, 5)])
def test_sl_batch_soft(ops, S, B, form, nsym):
    """(CD, C) = (P + 1, P + 1) and (P, P) ("both"), (P + 1, P) and (P, P + 1): tf_out equals
    sl_batch's for the same (seed, step); every element within 2 fp32 ulp of the float64
    quotient at the transformed point (the pass column in place); zero counts, the zero-sum
    row and, with the pass count dropped, the pass-only row exactly 0; the rows around the
    output untouched."""
    P = S * S
    table = label_transform_table(S)
    tab = torch.from_numpy(table).to(DEV)
    sym = (torch.arange(8, dtype=torch.int32) if nsym == 8
           else torch.tensor([6], dtype=torch.int32)).to(DEV)
    pairs = {"both": [(P + 1, P + 1), (P, P)], "drop_pass": [(P + 1, P)],
             "no_count": [(P, P + 1)]}[form]
    N = 7
    index = torch.tensor([4, 1, 2, 6, 1][:B], device=DEV)
    for CD, C in pairs:
        v = visit_rows(S, N, CD, 100 + S + CD)
        for step in (0, 3):
            tf_ref, _ = ops.sl_batch(index, torch.zeros(N, dtype=torch.int64, device=DEV), tab,
                                     sym, seed=11, step=step)
            full = torch.full((B + 2, C), float("nan"), device=DEV)
            full[0] = 7.0
            full[-1] = 7.0
            tf_full = torch.full((B + 2,), 77, dtype=torch.int32, device=DEV)
            tf, out = ops.sl_batch_soft(index, torch.from_numpy(v).to(DEV), tab, sym, 11, step,
                                        C, tf_out=tf_full[1:B + 1], targets_out=full[1:B + 1])
            assert torch.equal(tf, tf_ref)
            assert bool((full[0] == 7.0).all()) and bool((full[-1] == 7.0).all())
            assert tf_full[0].item() == 77 and tf_full[-1].item() == 77
            rows = v[index.cpu().numpy()]
            want = reference(rows, tf.cpu().numpy(), table, C)
            got = out.cpu().numpy()
            assert not np.isnan(got).any()
            assert ((got == 0) == (want == 0)).all()
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert (np.abs(got.astype(np.float64) - want) <= 2 * ulp).all()
            assert (got[index.cpu().numpy() == 1] == 0).all()
            if form == "drop_pass":
                assert (got[index.cpu().numpy() == 2] == 0).all()
            # the host definition agrees
            host = soft_targets_np(rows, tf.cpu().numpy(), table, C)
            assert (np.abs(host.astype(np.float64) - want) <= ulp).all()
            if nsym == 1:
                assert bool((tf == 6).all())
    if nsym == 8:
        seen = set()
        for step in range(6):
            seen |= set(ops.sl_batch_soft(index, torch.from_numpy(v).to(DEV), tab, sym, 11,
                                          step, C)[0].cpu().tolist())
        assert len(seen) > 4


@gpu
def test_sl_batch_soft_refuses_bad_widths(ops):
    """CD and C must each be S*S or S*S + 1: the wrapper raises, the C entry returns -1."""
    from rocalphago_amd import _native
    S, P = 5, 25
    tab = torch.from_numpy(label_transform_table(S)).to(DEV)
    sym = torch.zeros(1, dtype=torch.int32, device=DEV)
    index = torch.zeros(2, dtype=torch.int64, device=DEV)
    v = torch.zeros(3, P + 2, dtype=torch.int32).to(torch.uint16).to(DEV)
    with pytest.raises(ValueError):
        ops.sl_batch_soft(index, v, tab, sym, 0, 0, P)
    with pytest.raises(ValueError):
        ops.sl_batch_soft(index, v[:, :P].contiguous(), tab, sym, 0, 0, P + 2)
    with pytest.raises(ValueError):  # int32 counts
        ops.sl_batch_soft(index, torch.zeros(3, P, dtype=torch.int32, device=DEV), tab, sym, 0,
                          0, P)
    lib = _native.hip(required=True)
    tf = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, P + 2, device=DEV)
    for CD, C in ((P + 2, P), (P, P + 2), (P - 1, P), (P, P - 1)):
        rc = lib.rag_sl_batch_soft(index.data_ptr(), v.data_ptr(), CD, tab.data_ptr(), P,
                                   sym.data_ptr(), 1, 0, 0, tf.data_ptr(), out.data_ptr(), C, 2,
                                   None)
        assert rc == -1, (CD, C)


# ----------------------------------------------------------------------------------- CPU

def test_host_soft_batch_follows_the_planes():
    """host_batch(soft=True) under each of the 8 transforms: the target row, viewed as an S x S
    plane, equals apply_transform_np of the visit row's plane, normalised (the planes'
    direction of the permutation, not its inverse); the pass column stays in place."""
    S, N = 5, 8
    P = S * S
    rng = np.random.RandomState(5)
    v = rng.randint(0, 50, (N, P + 1)).astype(np.uint16)
    states = (rng.rand(N, 3, S, S) < 0.4).astype(np.uint8)
    ds = DeviceDataset(states, np.zeros((N, 2), np.int64), "cpu", visits=v)
    index = torch.arange(N)
    tf = torch.arange(8, dtype=torch.int32)
    X, Y = ds.host_batch(index, tf, soft=True, classes=P + 1)
    assert Y.shape == (N, P + 1) and Y.dtype == np.float32
    for i in range(N):
        q = v[i].astype(np.float64) / v[i].sum()
        plane = apply_transform_np(q[:P].reshape(1, S, S), i)[0]
        assert np.allclose(Y[i, :P].reshape(S, S), plane, rtol=1e-7, atol=0)
        assert np.isclose(Y[i, P], q[P], rtol=1e-7)
        assert np.array_equal(X[i], apply_transform_np(states[i], i).astype(np.float32))
    # without a pass class the pass count is dropped before normalising
    _, Y2 = ds.host_batch(index, tf, soft=True)
    assert Y2.shape == (N, P)
    for i in range(N):
        q = v[i, :P].astype(np.float64) / v[i, :P].sum()
        assert np.allclose(Y2[i].reshape(S, S), apply_transform_np(q.reshape(1, S, S), i)[0],
                           rtol=1e-7, atol=0)
    # the one-hot path is unchanged, and a dataset without visits refuses
    _, Y1 = ds.host_batch(index, tf)
    assert Y1.shape == (N, P) and (Y1.sum(1) == 1).all()
    plain = DeviceDataset(states, np.zeros((N, 2), np.int64), "cpu")
    assert plain.visits is None
    with pytest.raises(ValueError):
        plain.host_batch(index, tf, soft=True)
    with pytest.raises(ValueError):
        DeviceDataset(states, np.zeros((N, 2), np.int64), "cpu", visits=v[:, :P - 1])
