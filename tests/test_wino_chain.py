"""conv_wino_chain (csrc/hip/conv_wino.hip conv_wino_chain_kernel): a run of consecutive Winograd
forward layers in one launch, every block looping over the layers of its own boards.

Reference: the same layers through ops.conv_wino, one launch per layer. The arithmetic and its
order are the same, so every activation buffer must be EQUAL (torch.equal, halos included), not
close. Every buffer is the middle B boards of a B + 2 board allocation whose outer boards are
NaN: a read of them would poison the outputs, a write to them is seen.

Shapes: the smallest at which each form of the kernel can go wrong (one board per block at two
widths, four small boards per block with a ragged last block, more blocks than the chip has
CUs), chains of 1 (must equal the plain launch), 3 (two layer boundaries, both parities of the
V ring) and 11 layers (the trunk's depth). The kernel-level cases run with ``any_batch``: their
batches are ones the selector (conv_wino_mode) gives to half-board blocks or the direct kernel,
which the host entry otherwise refuses (the last test).

Weights are He-scaled (std sqrt(2 / (9 C))) so that activations neither die nor blow up over 11
layers; the per-layer reference alone must have more than a quarter of every layer's outputs
non-zero and all of them finite, or the comparison would be vacuous. (Checked on the CPU with
fp32 F.conv2d and these seeds: 0.45 - 1.0 non-zero at every layer of every case.)"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rocalphago_amd.ops import hipops
    return hipops


def layer_params(C, L, seed):
    """(input maker, per-layer (OIHW fp32 weight, bias or None, relu)) from a seeded CPU
    generator: the same values on every machine. ReLU is off on every third layer, and the
    second layer has no bias."""
    g = torch.Generator()
    g.manual_seed(seed)
    std = math.sqrt(2.0 / (9 * C))
    layers = []
    for l in range(L):
        w = torch.randn(C, C, 3, 3, generator=g) * std
        b = None if l == 1 else torch.randn(C, generator=g) * 0.1
        layers.append((w, b, l % 3 != 2))
    return g, layers


def guarded(B, S, C):
    """(whole allocation, view of its middle B boards): zero boards with halo 1 between one NaN
    board on either side."""
    full = torch.zeros(B + 2, S + 2, S + 2, C, dtype=BF, device=DEV)
    full[0] = NAN
    full[-1] = NAN
    return full, full[1:B + 1]


def assert_guards_and_halo(full, what):
    assert bool(torch.isnan(full[0]).all()), "%s: the board before the batch was written" % what
    assert bool(torch.isnan(full[-1]).all()), "%s: the board after the batch was written" % what
    v = full[1:-1]
    halo = (v[:, 0].abs().sum() + v[:, -1].abs().sum() + v[:, :, 0].abs().sum() +
            v[:, :, -1].abs().sum())
    assert float(halo) == 0.0, "%s: halo written" % what


def build(ops, B, S, C, L, seed):
    """Device operands of a case: the input in two guarded buffers (reference and chain), L
    guarded output buffers for each, Winograd weights, biases, ReLU flags."""
    g, layers = layer_params(C, L, seed)
    x = torch.randn(B, S, S, C, generator=g).to(BF).to(DEV)
    bufs = {}
    for k in ("ref", "chain"):
        bufs[k] = [guarded(B, S, C) for _ in range(L + 1)]
        bufs[k][0][1][:, 1:S + 1, 1:S + 1] = x
    us = [ops.wino_weights(w.to(DEV), C, C, dgrad=False)[0] for w, _, _ in layers]
    bs = [None if b is None else b.to(DEV) for _, b, _ in layers]
    relus = [r for _, _, r in layers]
    return bufs, us, bs, relus


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


CASES = [
    # (B, S, C, L): B None = CUs + 3
    (3, 19, 192, 1), (3, 19, 192, 3), (3, 19, 192, 11),   # <192, one board per block>
    (5, 9, 192, 3),                                       # <192, four boards>, last block ragged
    (3, 19, 128, 3),                                      # <128, one board per block>
    (None, 19, 192, 2),                                   # blocks in a second round
]


@pytest.mark.parametrize("B,S,C,L", CASES)
def test_chain_equals_single_launches(ops, B, S, C, L):
    B = cu_count() + 3 if B is None else B
    bufs, us, bs, relus = build(ops, B, S, C, L, seed=100 * L + C + S)
    ref, ch = bufs["ref"], bufs["chain"]
    for l in range(L):
        ops.conv_wino(ref[l][1], us[l], bs[l], ref[l + 1][1], B, S, C, C, 1, relus[l])
    ops.conv_wino_chain([(ch[l][1], us[l], bs[l], ch[l + 1][1], relus[l]) for l in range(L)],
                        B, S, any_batch=True)
    torch.cuda.synchronize()
    for l in range(1, L + 1):
        inner = ref[l][1][:, 1:S + 1, 1:S + 1].float()
        assert bool(torch.isfinite(inner).all()), "reference layer %d not finite" % l
        nz = float((inner != 0).float().mean())
        print("layer %d: %.3f of the reference outputs non-zero" % (l, nz))
        assert nz > 0.25, "reference layer %d: only %.3f non-zero" % (l, nz)
    for l in range(L + 1):
        assert_guards_and_halo(ref[l][0], "reference buffer %d" % l)
        assert_guards_and_halo(ch[l][0], "chain buffer %d" % l)
        assert torch.equal(ch[l][1], ref[l][1]), "activation %d differs" % l


def test_host_entry_refuses_what_the_kernel_cannot_run(ops):
    B, S, C = 3, 19, 192
    bufs, us, bs, relus = build(ops, B, S, C, 2, seed=7)
    a = [v for _, v in bufs["chain"]]

    def refused(layers, **kw):
        with pytest.raises(RuntimeError):
            ops.conv_wino_chain(layers, B, S, **kw)

    # an aliased ping-pong pair: layer 1 writes the buffer layer 0 read
    refused([(a[0], us[0], bs[0], a[1], True), (a[1], us[1], None, a[0], True)], any_batch=True)
    # overlapping (not only identical) buffers
    big = torch.zeros(B + 1, S + 2, S + 2, C, dtype=BF, device=DEV)
    refused([(big[:B], us[0], bs[0], big[1:], True)], any_batch=True)
    # a layer whose input is not the previous layer's output
    refused([(a[0], us[0], bs[0], a[1], True), (a[0], us[1], None, a[2], True)], any_batch=True)
    # unequal widths
    narrow = torch.zeros(B, S + 2, S + 2, 128, dtype=BF, device=DEV)
    refused([(a[0], us[0], bs[0], a[1], True), (a[1], us[1], None, narrow, True)],
            any_batch=True)
    # a batch the selector runs in half-board blocks
    assert ops.conv_wino_mode(B, S, C, C) == 2
    refused([(a[0], us[0], bs[0], a[1], True), (a[1], us[1], None, a[2], True)])
    # more than 16 layers
    many = [torch.zeros(B, S + 2, S + 2, C, dtype=BF, device=DEV) for _ in range(18)]
    refused([(many[l], us[0], None, many[l + 1], True) for l in range(17)], any_batch=True)
    torch.cuda.synchronize()
    # nothing ran
    assert float(a[1].abs().sum()) == 0.0 and float(a[2].abs().sum()) == 0.0
    assert float(big[B].abs().sum()) == 0.0 and float(narrow.abs().sum()) == 0.0
    assert all(float(m.abs().sum()) == 0.0 for m in many)
    # and the same 16 are taken
    ops.conv_wino_chain([(many[l], us[0], None, many[l + 1], True) for l in range(16)], B, S,
                        any_batch=True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,filters", [(3, 128), (200, 192)])
def test_trunk_forward_same_with_and_without_chain(ops, B, filters):
    """HipTrunk.forward with WINO_CHAIN on and off: equal activations at every boundary, at
    batches whose 3x3 layers run one-board Winograd blocks (so that the chain really runs)."""
    from rocalphago_amd.models.engine import ConvSpec, HipTrunk
    dev = torch.device("cuda")
    S = 19
    specs = [ConvSpec(5, 48, filters, True)] + [ConvSpec(3, filters, filters, True)] * 4 + \
        [ConvSpec(1, filters, 1, False)]
    g = torch.Generator()
    g.manual_seed(filters)
    ws = [(torch.randn(s.cout, s.cin, s.ks, s.ks, generator=g) *
           math.sqrt(2.0 / (s.ks * s.ks * s.cin))).to(dev) for s in specs]
    bs = [(torch.randn(s.cout, generator=g) * 0.1).to(dev) for s in specs]
    x = torch.randn(B, S, S, 48, generator=g).to(BF).to(dev)
    outs = {}
    for chain in (False, True):
        tr = HipTrunk(specs, S, dev)
        assert tr.wino_chain is HipTrunk.WINO_CHAIN
        tr.wino_chain = chain
        tr.ensure_batch(B)
        tr.sync_weights(ws, bs, 1)
        assert tr.chain_plan(B) == {1: 5}
        h = tr.halo[0]
        tr.input_buffer(B)[:, h:h + S, h:h + S, :48] = x
        tr.forward(B)
        torch.cuda.synchronize()
        outs[chain] = [a[:B].clone() for a in tr.acts]
    for l, (p, q) in enumerate(zip(outs[False], outs[True])):
        assert torch.equal(p, q), "activation %d differs" % l
    inner = outs[True][5][:, 1:S + 1, 1:S + 1].float()
    assert bool(torch.isfinite(inner).all()) and float((inner != 0).float().mean()) > 0.25
