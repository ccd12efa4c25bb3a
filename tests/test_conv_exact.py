"""Bit-exact tests of every convolution route with small-integer operands (GPU only).

Activations, gradients and residuals are integers in [-2, 2], weights integers in [-2, 2] (even
integers in [-4, 4] where the Winograd kernel takes part), biases multiples of 0.25 in [-2, 2].
Every product and every partial sum is then exactly representable in fp32 whatever the summation
order, the MFMA shape or the Winograd transform (U = (g0 +- g1 + g2) / 2 of even g is an integer,
V = d_a +- d_b a small one, the butterfly only adds), so the only rounding left is the final
fp32 -> bf16 store and a kernel must reproduce a float64 tap loop BIT FOR BIT: one dropped, doubled
or mis-addressed term anywhere shows. The weight-gradient kernels' block-scaled fp16 partials are
exact as long as a block's largest |partial| stays below 2^11 (11 significant bits); those cases
use sparse {-1, 0, 1} operands and assert that bound themselves.

Around every output: the halo is exactly zero, one spare board before and one after the batch
(pre-filled with 7.0) is untouched, and every input is a view into a larger allocation whose
next board is NaN, so that a read past the last board that reaches an output shows up as NaN.

Routes (from the dispatch code in csrc/hip/conv.hip, conv_tap.hip, conv_fwd.hip, conv_wino.hip,
wgrad*.hip at this commit; a dgrad of a cin -> cout row runs as the cout -> cin convolution).
conv_tap_pp_kernel's arguments are <NB, NT, BNP, KS, MT, SPREAD, PRIO, PAIR>, conv_pipe_kernel's
and conv_igemm_kernel's <KS, NT(, MT)>, conv_wino_kernel's <WN, one board per block, PAIRS, BN
form>. Thresholds as read from the code: the 384-pixel ping-pong kernel needs >= 200 blocks and a
slab of <= 640 rows (3x3) / 768 (5x5), the 192-pixel one >= 200 blocks and <= 320 / 448 rows,
conv_tap_kernel <= 320 rows.

  case (S, ks, cin -> cout, B)        forward / residual forward          dgrad
  ----------------------------------  ----------------------------------  -------------------------
  pp384_13   13 3 192->192 455        conv_tap_pp<3,6,0,3,6,1,1,0>        the same (201 blocks,
                                                                          last one 95 pixels)
  pp384_9     9 3 192->192 1024       conv_tap_pp<3,6,0,3,6,1,1,0>        the same (216 full blocks)
  pp384_2n   19 3 192->384 107        conv_tap_pp<3,6,0,3,6,1,1,0> x 2 N  conv_tap_pp<3,6,0,3,3>
                                                                          (192-pixel, 12 K chunks)
  pp384_k2   19 3  64->192 213        conv_tap_pp<3,6,0,3,6,1,1,0>        conv_pipe<3,2,6>
  pp384w128_13 13 3 128->128 455      conv_tap_pp<3,4,0,3,6>              the same
  pp384w128_2n 19 3 128->256 107      conv_tap_pp<3,4,0,3,6> x 2 N        conv_pipe<3,4,4>
  pp192_13   13 3 192->192 227        conv_tap_pp<3,6,0,3,3> (200 blocks) the same
  tap_2n     19 3 192->384 3          conv_tap_kernel x 2 N tiles         conv_tap_kernel
  pipe_9      9 3 192->192 500        conv_pipe<3,6,4> (324 > 320 rows)   the same
  pipe_13x5  13 5 64(48)->192 455     conv_pipe<5,6,6> (780 > 768 rows)   conv_pipe<5,2,6>
  pipe_w128  19 3 128->128 100        conv_pipe<3,4,4> (95 < 200 blocks)  the same
  pp384x5_pair_2n 19 5 64(48)->384 107  conv_tap_pp<3,6,0,5,6,0,0,1> x 2 N  conv_pipe<5,2,4>
  pp192x5    19 5  64->192 110        conv_tap_pp<3,6,0,5,3> (207 blocks) conv_pipe<5,2,4>
  igemm_nt1  19 3  32->32  2          conv_igemm<3,1>                     the same
  pipe_7x7    7 7  32->64  2          conv_pipe<7,2,8> (64-multiples go   conv_igemm<7,1>
                                      to conv_pipe, not to conv_igemm)
  igemm_7x7   7 7  32->96  2          conv_igemm<7,3>                     conv_igemm<7,1>
  seam 19 3 192->192 B = 105          conv_tap_kernel (198 blocks of 192 pixels)
                     B = 106, 107, 211  conv_tap_pp<3,6,0,3,3> (>= 200 blocks of 192 pixels)
                     B = 212, 213     conv_tap_pp<3,6,0,3,6,1,1,0> (>= 200 blocks of 384 pixels)
  self-check 19 3 192->192 3          conv_tap_kernel
  wino (B, S, C) = (3, 19, 192), (128, 19, 192)  conv_wino<192,1,96> (half-board blocks, 256 CUs)
                   (5, 9, 192)        conv_wino<192,0> (four boards per block, the last ragged)
                   (200, 19, 192)     conv_wino<192,1>
                   (3, 19, 128)       conv_wino<128,1>
  BN forms 19 3 128->128 256          conv_tap_pp<3,4,1,3,6> (forward), <3,4,0,3,6> with mask
                                      coefficients (dgrad); conv_wino<128,1,192,1> / <..,2>
                                      (<..,1> with a residual rounds twice: held to one ulp)
                   their conv_igemm counterparts: conv_tap_kernel, conv_pipe<3,6,6>,
                   conv_tap_pp<3,6,0,3,3> (B = 200, 128), conv_pipe<3,4,8>
  wgrad slab 3x3 192->192 (map 0 / 1) wgrad_slab_kernel<3,1,map,192,0,3> + wgrad_slab_reduce<4>
             3x3 128->128             wgrad_slab_kernel<3,1,0,128,0,3>
             5x5 48->192 / 128->128   wgrad_slab_kernel<3,1,0,192|128,0,5> (pair5 for 48 -> 192)
  wgrad all taps 3x3 64->128, 5x5 192->384   wgrad_taps_kernel<3,3,2> / <5,1,2> + wgrad_reduce<4>
  wgrad gather (hi != hg) 3x3 192->192, 5x5 32->192   conv_wgrad_kernel<3,6,3> / <5,6,1>

Confirmed once by a kernel trace of this file on an MI355X (256 CUs):
profiles/conv_exact_routes.txt.
"""
import pytest
import torch
import torch.nn.functional as F

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


# ------------------------------------------------------------------------------- operands

def gen(seed):
    """Operands come from a seeded CPU generator: the same values on every machine."""
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def ints(g, shape, lo, hi, step=1.0):
    """float64 device tensor of step * (integers in [lo, hi])."""
    t = torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8)
    return t.to(DEV).double() * step


def sparse_signs(g, shape, density):
    """float64 device tensor of values in {-1, 0, 1}, non-zero with probability ``density``."""
    keep = torch.rand(shape, generator=g) < density
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int8) * 2 - 1
    return (sign * keep).to(DEV).double()


def guarded_input(t, halo, cp):
    """Padded bf16 activation of the NHWC float64 tensor ``t`` as a view of the first B boards
    of a B + 1 board allocation whose last board is NaN."""
    B, S, _, C = t.shape
    buf = torch.zeros(B + 1, S + 2 * halo, S + 2 * halo, cp, dtype=BF, device=DEV)
    buf[B] = NAN
    buf[:B, halo:halo + S, halo:halo + S, :C] = t.to(BF)
    return buf[:B]


def guarded_output(B, S, halo, cp):
    """(whole allocation, view of its middle B boards): one spare board of 7.0 on either side."""
    full = torch.zeros(B + 2, S + 2 * halo, S + 2 * halo, cp, dtype=BF, device=DEV)
    full[0] = 7.0
    full[-1] = 7.0
    return full, full[1:B + 1]


def assert_guards_untouched(full):
    assert bool((full[0] == 7.0).all()), "the board before the batch was written"
    assert bool((full[-1] == 7.0).all()), "the board after the batch was written"


# ------------------------------------------------------------------------------ reference

def tap_conv(x, w):
    """The convolution as a plain tap loop in float64: x [B, S, S, cin], w [cout, cin, ks, ks]
    -> [B, S, S, cout]; per tap one matmul of the shifted zero-padded input with
    w[:, :, ky, kx]^T."""
    B, S, _, cin = x.shape
    cout, _, ks, _ = w.shape
    p = ks // 2
    xp = F.pad(x, (0, 0, p, p, p, p))
    out = torch.zeros(B * S * S, cout, dtype=torch.float64, device=x.device)
    for ky in range(ks):
        for kx in range(ks):
            out += xp[:, ky:ky + S, kx:kx + S, :].reshape(-1, cin) @ w[:, :, ky, kx].t()
    return out.view(B, S, S, cout)


def dgrad_weights(w):
    """w' with tap_conv(g, w') = dL/dx of y = tap_conv(x, w): flipped taps, transposed channels."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def tap_wgrad(x, g, ks):
    """dW [cout, cin, ks, ks] of y = tap_conv(x, w) for dL/dy = g: the transposed tap loop."""
    B, S, _, cin = x.shape
    cout = g.shape[-1]
    p = ks // 2
    xp = F.pad(x, (0, 0, p, p, p, p))
    gt = g.reshape(-1, cout).t().contiguous()
    dw = torch.empty(cout, cin, ks, ks, dtype=torch.float64, device=x.device)
    for ky in range(ks):
        for kx in range(ks):
            dw[:, :, ky, kx] = gt @ xp[:, ky:ky + S, kx:kx + S, :].reshape(-1, cin)
    return dw


def round_bf16_nchw(ref):
    """float64 NHWC reference -> bf16 NCHW, after the exactness precondition (a property of the
    operands, not of the kernel): every value below 2^24 in magnitude."""
    assert ref.abs().max().item() < 2 ** 24
    return ref.float().to(BF).permute(0, 3, 1, 2).contiguous()


def assert_partial_sums_exact(ks, cin, xmax, wmax):
    """Every partial sum of products (plus a quarter-step bias and a residual, each at most 2)
    is a multiple of 0.25 below 2^22: exact in fp32 in any summation order."""
    assert ks * ks * cin * xmax * wmax + 4 < 2 ** 22


# ----------------------------------------------------------------------------- comparison

def _ordered(bits):
    """bf16 bit patterns (int16) -> integers ordered like the values they encode."""
    u = bits.int() & 0xFFFF
    return torch.where(u >= 0x8000, 0x8000 - u, u)


def assert_bits_equal(got_padded, ref_nchw, halo, route="", one_ulp_store=False):
    """The padded bf16 kernel output equals the bf16 NCHW reference bit for bit, holds no NaN
    and has an exactly zero halo. Never a tolerance: on a mismatch it reports how many values
    differ, the first (b, c, i, j) and whether all of them are within one bf16 ulp (then route's
    store rounds other than to nearest even; otherwise a term is wrong).
    ``one_ulp_store``: only for a route whose store is documented to round twice (docs/KERNELS.md,
    "Exact-arithmetic tests"): every value within one bf16 ulp of the reference."""
    B, C, S, _ = ref_nchw.shape
    assert got_padded.shape == (B, S + 2 * halo, S + 2 * halo, C), got_padded.shape
    assert not bool(torch.isnan(got_padded).any()), "%s: NaN in the output" % route
    border = got_padded.clone()
    border[:, halo:halo + S, halo:halo + S] = 0
    assert not bool(border.view(torch.int16).any()), "%s: the output halo is not zero" % route
    inner = got_padded[:, halo:halo + S, halo:halo + S, :].permute(0, 3, 1, 2).contiguous()
    gb, rb = inner.view(torch.int16), ref_nchw.contiguous().view(torch.int16)
    if torch.equal(gb, rb):
        return
    bad = gb != rb
    first = tuple(bad.nonzero()[0].tolist())
    one_ulp = bool(((_ordered(gb) - _ordered(rb)).abs()[bad] <= 1).all())
    if one_ulp and one_ulp_store:
        return
    raise AssertionError(
        "%s: %d of %d values differ, first at (b, c, i, j) = %s: got %r, want %r; %s" %
        (route, int(bad.sum()), bad.numel(), first, inner[first].item(), ref_nchw[first].item(),
         "all within one bf16 ulp: this route's store does not round to nearest even"
         if one_ulp else "not all within one ulp: a term is wrong"))


# ------------------------------------------------------------------- direct kernels (igemm)

# name: (S, ks, cinp, cout, B, real input channels or None)
DIRECT = {
    "pp384_13": (13, 3, 192, 192, 455, None),
    "pp384_9": (9, 3, 192, 192, 1024, None),
    "pp384_2n": (19, 3, 192, 384, 107, None),
    "pp384_k2": (19, 3, 64, 192, 213, None),
    "pp384w128_13": (13, 3, 128, 128, 455, None),
    "pp384w128_2n": (19, 3, 128, 256, 107, None),
    "pp192_13": (13, 3, 192, 192, 227, None),
    "tap_2n": (19, 3, 192, 384, 3, None),
    "pipe_9": (9, 3, 192, 192, 500, None),
    "pipe_13x5": (13, 5, 64, 192, 455, 48),
    "pipe_w128": (19, 3, 128, 128, 100, None),
    "pp384x5_pair_2n": (19, 5, 64, 384, 107, 48),
    "pp192x5": (19, 5, 64, 192, 110, None),
    "igemm_nt1": (19, 3, 32, 32, 2, None),
    "pipe_7x7": (7, 7, 32, 64, 2, None),
    "igemm_7x7": (7, 7, 32, 96, 2, None),
}


def direct_operands(seed, S, ks, cinp, cout, B, cin_real, wstep=1):
    """x (ReLU'd where it serves as a mask), w, bias, residual, g as float64 device tensors; the
    input channels past ``cin_real`` are zero in x and w (the padded layout)."""
    g = gen(seed)
    cin = cin_real or cinp
    x = torch.zeros(B, S, S, cinp, dtype=torch.float64, device=DEV)
    x[..., :cin] = ints(g, (B, S, S, cin), -2, 2)
    w = torch.zeros(cout, cinp, ks, ks, dtype=torch.float64, device=DEV)
    w[:, :cin] = ints(g, (cout, cin, ks, ks), -2, 2, wstep)
    bias = ints(g, (cout,), -8, 8, 0.25)
    res = ints(g, (B, S, S, cout), -2, 2)
    grad = ints(g, (B, S, S, cout), -2, 2)
    assert_partial_sums_exact(ks, max(cinp, cout), 2, 2 * wstep)
    return x, w, bias, res, grad, cin


def packed_weights(ops, w, cin, dgrad):
    """The kernels' forward (or dgrad) weight layout of the float64 OIHW weights (real input
    channels only: the packer pads)."""
    cout, cinp, ks, _ = w.shape
    w32 = w[:, :cin].float().contiguous()
    wb = torch.empty(ks * ks, cinp, cout, dtype=BF, device=DEV) if dgrad else None
    wf, wb = ops.pack_weights(w32, cout, cinp, wb=wb)
    return wb if dgrad else wf


def run_direct(ops, name, form, seed):
    S, ks, cinp, cout, B, cin_real = DIRECT[name]
    x, w, bias, res, grad, cin = direct_operands(seed, S, ks, cinp, cout, B, cin_real)
    hi = ks // 2
    b32 = bias.float().contiguous()
    route = "%s/%s" % (name, form)
    if form == "fwd":  # bias + ReLU, output halo 1
        ref = round_bf16_nchw(torch.relu(tap_conv(x, w) + bias))
        full, y = guarded_output(B, S, 1, cout)
        ops.conv_igemm(guarded_input(x, hi, cinp), packed_weights(ops, w, cin, False), b32, y,
                       B, S, hi, 1, cinp, cout, ks, relu=True, cin=cin_real)
        assert_bits_equal(y, ref, 1, route)
    elif form == "res":  # bias + residual, no activation, output halo 2
        ref = round_bf16_nchw(tap_conv(x, w) + bias + res)
        full, y = guarded_output(B, S, 2, cout)
        ops.conv_igemm(guarded_input(x, hi, cinp), packed_weights(ops, w, cin, False), b32, y,
                       B, S, hi, 2, cinp, cout, ks, relu=False, cin=cin_real,
                       residual=guarded_input(res, 2, cout))
        assert_bits_equal(y, ref, 2, route)
    else:  # dgrad: output halo 2, the ReLU mask (the layer input) at its own halo 1
        xm = torch.relu(x)
        dx = tap_conv(grad, dgrad_weights(w))
        # (where, not a product: -3 * 0 is -0.0, whose bits differ from the kernel's +0.0)
        ref = round_bf16_nchw(torch.where(xm > 0, dx, torch.zeros_like(dx)))
        full, y = guarded_output(B, S, 2, cinp)
        ops.conv_igemm(guarded_input(grad, hi, cout), packed_weights(ops, w, cin, True), None, y,
                       B, S, hi, 2, cout, cinp, ks, relu=False, mask=guarded_input(xm, 1, cinp),
                       mask_halo=1)
        assert_bits_equal(y, ref, 2, route)
    assert_guards_untouched(full)


@pytest.mark.parametrize("form", ["fwd", "res", "dgrad"])
@pytest.mark.parametrize("name", list(DIRECT))
def test_direct_routes_bit_exact(ops, name, form):
    run_direct(ops, name, form, seed=1000 + list(DIRECT).index(name))


@pytest.mark.parametrize("B", [105, 106, 107, 211, 212, 213])
def test_dispatch_seams_bit_exact(ops, B):
    """3x3 192 -> 192 at 19x19 on either side of the two batch sizes where the dispatcher changes
    kernel: 198 -> 200 blocks of 192 pixels between B = 105 and 106 (conv_tap_kernel -> 192-pixel
    ping-pong), 199 -> 200 blocks of 384 pixels between B = 211 and 212 (-> 384-pixel ping-pong).
    All of them equal the same float64 reference of the same leading boards, so both sides of
    a seam give identical bits."""
    S, C = 19, 192
    x, w, bias, _, _, _ = direct_operands(77, S, 3, C, C, 213, None)
    x = x[:B].contiguous()
    ref = round_bf16_nchw(torch.relu(tap_conv(x, w) + bias))
    full, y = guarded_output(B, S, 1, C)
    ops.conv_igemm(guarded_input(x, 1, C), packed_weights(ops, w, C, False),
                   bias.float().contiguous(), y, B, S, 1, 1, C, C, 3, relu=True)
    assert_bits_equal(y, ref, 1, "seam B=%d" % B)
    assert_guards_untouched(full)


def test_comparator_sees_one_wrong_term(ops):
    """Self-check of the comparison: one weight element (n, c, ky, kx) raised by 1 on the kernel's
    side only changes channel n only, and exactly at the pixels where the float64 tap loop says
    that term is non-zero: the operands are dense enough for a single wrong term to be seen."""
    S, C, B = 19, 192, 3
    x, w, _, _, _, _ = direct_operands(5, S, 3, C, C, B, None)
    base = tap_conv(x, w)
    # the channel whose values stay smallest: below 256 every integer is a bf16 value, so the
    # extra term (at most 2) can never vanish in the output rounding (reference side only)
    n = int(base.abs().amax((0, 1, 2)).argmin())
    assert base[..., n].abs().max().item() + 2 <= 256
    c, ky, kx = 101, 2, 0
    w_bad = w.clone()
    w_bad[n, c, ky, kx] += 1
    delta = torch.zeros_like(w)
    delta[n, c, ky, kx] = 1
    term = tap_conv(x, delta)  # x shifted by the tap, on channel n
    assert 0.5 < (term[..., n] != 0).double().mean().item() < 0.9
    full, y = guarded_output(B, S, 1, C)
    ops.conv_igemm(guarded_input(x, 1, C), packed_weights(ops, w_bad, C, False), None, y, B, S, 1,
                   1, C, C, 3, relu=False)
    assert_bits_equal(y, round_bf16_nchw(base + term), 1, "self-check")
    assert_guards_untouched(full)
    got = y[:, 1:-1, 1:-1, :].view(torch.int16)
    want = base.float().to(BF).view(torch.int16)
    differs = got != want
    assert torch.equal(differs.any(0).any(0).any(0).nonzero().flatten(),
                       torch.tensor([n], device=DEV))
    assert torch.equal(differs[..., n], term[..., n] != 0)
    with pytest.raises(AssertionError, match="a term is wrong"):
        assert_bits_equal(y, round_bf16_nchw(base), 1, "self-check")


# ------------------------------------------------------------------------------- Winograd

@pytest.mark.parametrize("B,S,C", [(3, 19, 192), (5, 9, 192), (200, 19, 192), (128, 19, 192),
                                   (3, 19, 128)])
def test_wino_bit_exact(ops, B, S, C):
    """conv_wino forward (bias + ReLU) and dgrad (ReLU mask, output halo 2) with even integer
    weights: exact against the float64 tap loop and bit-equal to conv_igemm on the same inputs."""
    if B == 128 and ops.conv_wino_mode(B, S, C, C) != 2:
        pytest.skip("half-board blocks are chosen for B = 128 on 256 CUs only")
    assert ops.conv_wino_ok(S, 1, C, C, 3)
    x, w, bias, _, grad, _ = direct_operands(2000 + B + S + C, S, 3, C, C, B, None, wstep=2)
    assert w.abs().max().item() == 4 and bool((w % 2 == 0).all())
    w32, b32 = w.float().contiguous(), bias.float().contiguous()
    uf, ub = ops.wino_weights(w32, C, C)
    wf, wb = ops.pack_weights(w32, C, C, wb=torch.empty(9, C, C, dtype=BF, device=DEV))
    # forward
    ref = round_bf16_nchw(torch.relu(tap_conv(x, w) + bias))
    full, y = guarded_output(B, S, 1, C)
    ops.conv_wino(guarded_input(x, 1, C), uf, b32, y, B, S, C, C, 1, True)
    assert_bits_equal(y, ref, 1, "wino fwd")
    assert_guards_untouched(full)
    fulld, yd = guarded_output(B, S, 1, C)
    ops.conv_igemm(guarded_input(x, 1, C), wf, b32, yd, B, S, 1, 1, C, C, 3, relu=True)
    assert_bits_equal(yd, ref, 1, "direct fwd")
    assert torch.equal(y.view(torch.int16), yd.view(torch.int16))
    # dgrad with the mask at halo 1, output halo 2
    xm = torch.relu(x)
    dx = tap_conv(grad, dgrad_weights(w))
    ref = round_bf16_nchw(torch.where(xm > 0, dx, torch.zeros_like(dx)))
    full, y = guarded_output(B, S, 2, C)
    ops.conv_wino(guarded_input(grad, 1, C), ub, None, y, B, S, C, C, 2, False,
                  mask=guarded_input(xm, 1, C), mask_halo=1)
    assert_bits_equal(y, ref, 2, "wino dgrad")
    assert_guards_untouched(full)
    fulld, yd = guarded_output(B, S, 2, C)
    ops.conv_igemm(guarded_input(grad, 1, C), wb, None, yd, B, S, 1, 2, C, C, 3, relu=False,
                   mask=guarded_input(xm, 1, C), mask_halo=1)
    assert_bits_equal(yd, ref, 2, "direct dgrad")
    assert_guards_untouched(fulld)
    assert torch.equal(y.view(torch.int16), yd.view(torch.int16))


# ------------------------------------------------------------------- fused BatchNorm forms

def assert_column_stats(part, terms, blk, granule, what):
    """Per-block fp32 column partials ``part`` [nblk, S], summed over blocks in float64, against
    the float64 column sums of ``terms`` [B, S, S, C] (multiples of ``granule``). ``blk`` [B, S, S]
    is the block of each pixel. If the largest per-(block, column) sum of |terms| is below
    2^24 granules every fp32 partial is exact in any order and the comparison is exact; otherwise
    it is relative 1e-6. Returns which one applied."""
    B, S, _, _ = terms.shape
    nblk = part.shape[0]
    col = torch.arange(S, device=DEV).view(1, 1, S).expand(B, S, S)
    mag = torch.zeros(nblk * S, dtype=torch.float64, device=DEV)
    mag.index_add_(0, (blk * S + col).reshape(-1), terms.abs().sum(-1).reshape(-1))
    exact = mag.max().item() / granule < 2 ** 24
    got, want = part.double().sum(0), terms.sum((0, 1, 3))
    print("%s: %s comparison (largest block partial bound %.3g granules)" %
          (what, "exact" if exact else "relative 1e-6", mag.max().item() / granule))
    if exact:
        assert torch.equal(got, want), what
    else:
        assert torch.allclose(got, want, rtol=1e-6, atol=0), what
    return exact


@pytest.mark.parametrize("kernel", ["igemm", "wino"])
def test_bn_fused_forms_bit_exact(ops, kernel):
    """conv_igemm_bn / conv_wino_bn at B = 256, 19x19, 128 -> 128 with power-of-two column
    coefficients: U = ReLU(cx x + cc) (cx in {0.5, 1, 2}, cc in {-1, 0, 2}, cc > 0 on the first
    and last column, so a halo pixel that wrongly became ReLU(cc) would change the border) is exact
    in bf16. Forward with and without the residual, dgrad with the mask recomputed from x, and
    the column statistics partials of both: the sums are exact for these operands (the helper's
    own bound), the sums of squares exceed 2^24 per block and are compared to relative 1e-6.
    One route rounds twice and is held to one ulp: conv_wino_bn's forward with a residual."""
    B, S, C = 256, 19, 128
    if kernel == "igemm":
        assert ops.conv_bn_fusable(B, S, 1, C, C, 3)
    else:
        assert ops.conv_wino_bn_ok(B, S, C, C)
    x, w, bias, res, grad, _ = direct_operands(3000, S, 3, C, C, B, None, wstep=2)
    col = torch.arange(S, device=DEV)
    cx = torch.tensor([0.5, 1.0, 2.0], device=DEV)[(col // 3) % 3]
    cc = torch.tensor([2.0, -1.0, 0.0], device=DEV)[col % 3]
    assert cc[0] > 0 and cc[-1] > 0
    coef = torch.zeros(3, S, device=DEV)
    coef[0], coef[2] = cx, cc
    pre = x * cx.double().view(1, 1, S, 1) + cc.double().view(1, 1, S, 1)
    U = torch.relu(pre)  # multiples of 0.5 up to 6
    assert_partial_sums_exact(3, C, 6, 4)  # half steps times even weights: integers
    w32, b32 = w.float().contiguous(), bias.float().contiguous()
    if kernel == "igemm":
        wfwd, wbwd = ops.pack_weights(w32, C, C, wb=torch.empty(9, C, C, dtype=BF, device=DEV))
        nblk = ops.conv_bn_stat_blocks(B, S, C)
        # block of pixel m = (b, i, j): runs of 384 pixels
        blk = (torch.arange(B * S * S, device=DEV) // 384).view(B, S, S)

        def launch(*a, **k):
            return ops.conv_igemm_bn(*a, **k)
    else:
        wfwd, wbwd = ops.wino_weights(w32, C, C)
        nblk = B
        blk = torch.arange(B, device=DEV).view(B, 1, 1).expand(B, S, S)

        def launch(xin, wt, b, y, B_, S_, cin, cout, relu, **k):
            return ops.conv_wino_bn(xin, wt, b, y, B_, S_, cin, cout, relu, **k)
    conv = tap_conv(U, w)
    # forward: bias + residual, statistics of the stored output
    ref = round_bf16_nchw(conv + bias + res)
    full, y = guarded_output(B, S, 1, C)
    part = torch.full((nblk, 2, S), 7.0, device=DEV)
    launch(guarded_input(x, 1, C), wfwd, b32, y, B, S, C, C, False, bn_coef=coef,
           residual=guarded_input(res, 1, C), stat_part=part)
    if kernel == "igemm":
        assert_bits_equal(y, ref, 1, "igemm_bn fwd + residual")
    else:
        # conv_wino_kernel<128, true, 192, 1> rounds twice when it has a residual: conv + bias
        # goes through its bf16 LDS image, the residual is added to that in its coalesced row
        # pass and the sum is rounded again (adding it in fp32 ahead of the image measured
        # 38.7-39.4 -> 41.8-42.0 us per launch: docs/KERNELS.md "Exact-arithmetic tests"). So
        # this route alone is held to one ulp of the float64 reference -- and bit for bit to
        # that documented arithmetic, so a wrong term still shows.
        assert_bits_equal(y, ref, 1, "wino_bn fwd + residual", one_ulp_store=True)
        twice = (conv + bias).float().to(BF).double() + res
        assert_bits_equal(y, round_bf16_nchw(twice), 1, "wino_bn fwd + residual, two roundings")
    assert_guards_untouched(full)
    stored = y[:, 1:-1, 1:-1, :].double()
    assert assert_column_stats(part[:, 0], stored, blk, 0.25, "sum y")
    assert_column_stats(part[:, 1], stored * stored, blk, 1.0 / 16, "sum y^2")
    # forward: bias + ReLU, no residual
    ref = round_bf16_nchw(torch.relu(conv + bias))
    full, y = guarded_output(B, S, 1, C)
    launch(guarded_input(x, 1, C), wfwd, b32, y, B, S, C, C, True, bn_coef=coef)
    assert_bits_equal(y, ref, 1, kernel + "_bn fwd + relu")
    assert_guards_untouched(full)
    # dgrad: the mask U > 0 recomputed from x, statistics sum dU and sum dU (x - mean)
    dx = tap_conv(grad, dgrad_weights(w))
    ref = round_bf16_nchw(torch.where(pre > 0, dx, torch.zeros_like(dx)))
    mean = ints(gen(3001), (S,), -2, 2, 0.5).float()
    full, y = guarded_output(B, S, 1, C)
    part = torch.full((nblk, 2, S), 7.0, device=DEV)
    launch(guarded_input(grad, 1, C), wbwd, None, y, B, S, C, C, False,
           mask=guarded_input(x, 1, C), mask_coef=coef, stat_part=part, stat_mean=mean)
    assert_bits_equal(y, ref, 1, kernel + "_bn dgrad")
    assert_guards_untouched(full)
    stored = y[:, 1:-1, 1:-1, :].double()
    assert assert_column_stats(part[:, 0], stored, blk, 1.0, "sum dU")
    assert assert_column_stats(part[:, 1], stored * (x - mean.double().view(1, 1, S, 1)), blk,
                               0.5, "sum dU (x - mean)")


# ------------------------------------------------------------------------ weight gradient

def wgrad_case(ops, S, ks, cin, cinp, cout, B, hi, hg, seed, density=None):
    """Operands and float64 references of one conv_wgrad case. ``density``: sparse {-1, 0, 1}
    operands for the fp16-partial slab kernels (and their < 2^11 bound asserted here), None:
    dense integers in [-2, 2] (fp32 partials)."""
    g = gen(seed)
    x = torch.zeros(B, S, S, cinp, dtype=torch.float64, device=DEV)
    if density is None:
        x[..., :cin] = ints(g, (B, S, S, cin), -2, 2)
        grad = ints(g, (B, S, S, cout), -2, 2)
        assert B * S * S * 4 < 2 ** 24
    else:
        x[..., :cin] = sparse_signs(g, (B, S, S, cin), density)
        grad = sparse_signs(g, (B, S, S, cout), density)
        # the block-scaled fp16 partials hold 11 significant bits: every chunk's |partial| is at
        # most sum |g| |x| over the whole batch, however the rows are chunked (input condition)
        bound = tap_wgrad(x.abs(), grad.abs(), ks).max().item()
        assert bound < 2048, bound
    ref_dw = tap_wgrad(x, grad, ks)[:, :cin]
    ref_db = grad.sum((0, 1, 2))
    assert ref_dw.abs().max().item() < 2 ** 24
    xp, gp = guarded_input(x, hi, cinp), guarded_input(grad, hg, cout)
    return xp, gp, ref_dw.float().contiguous(), ref_db.float()


def slab_density(B, S):
    """Non-zero probability of x and of g that keeps sum |g| |x| near 1500 (max over ~3e5
    (n, c, tap) sums: + 5 sigma ~ 1700 < 2048)."""
    return min(1.0, (1500.0 / (B * S * S)) ** 0.5)


def run_wgrad_slab(ops, S, ks, cin, cinp, cout, B, seed):
    """Overwrite, accumulate on a non-zero integer dW, and the deferred form flushed with
    wgrad_flush: dW and db equal the float64 reference cast to fp32, bit for bit."""
    h = ks // 2
    xp, gp, ref_dw, ref_db = wgrad_case(ops, S, ks, cin, cinp, cout, B, h, h, seed,
                                        density=slab_density(B, S))
    dw = torch.full((cout, cin, ks, ks), NAN, device=DEV)
    db = torch.full((cout,), NAN, device=DEV)
    ops.conv_wgrad(gp, xp, dw, db, B, S, h, cout, cout, cin, cinp, ks, hg=h)
    assert torch.equal(dw, ref_dw) and torch.equal(db, ref_db)
    dw0 = ints(gen(seed + 1), (cout, cin, ks, ks), -3, 3).float()
    db0 = ints(gen(seed + 2), (cout,), -3, 3).float()
    dw, db = dw0.clone(), db0.clone()
    ops.conv_wgrad(gp, xp, dw, db, B, S, h, cout, cout, cin, cinp, ks, accumulate=True, hg=h)
    assert torch.equal(dw, dw0 + ref_dw) and torch.equal(db, db0 + ref_db)
    pend = ops.PendingReduction()
    ops.conv_wgrad(gp, xp, dw, db, B, S, h, cout, cout, cin, cinp, ks, accumulate=True, hg=h,
                   defer=True, pending=pend)
    ops.wgrad_flush(pend)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw0 + 2 * ref_dw) and torch.equal(db, db0 + 2 * ref_db)


@pytest.mark.parametrize("C,B,S,wmap", [(192, 7, 19, 0), (192, 7, 19, 1), (192, 256, 19, 0),
                                        (192, 256, 19, 1), (128, 7, 19, None),
                                        (128, 256, 19, None), (192, 227, 13, None)])
def test_wgrad_slab_3x3_exact(ops, C, B, S, wmap):
    """The slab kernel's fp16 partials (3x3, 192 -> 192 with both wave -> tile maps, 128 -> 128,
    and 13x13 boards at B = 227)."""
    lib = ops._lib()
    prev = lib.rag_wgrad_slab_map(wmap) if wmap is not None else None
    try:
        run_wgrad_slab(ops, S, 3, C, C, C, B, seed=4000 + B + C + S)
    finally:
        if wmap is not None:
            lib.rag_wgrad_slab_map(prev)


@pytest.mark.parametrize("cin,cinp,cout", [(48, 64, 192), (128, 128, 128)])
def test_wgrad_slab_5x5_rows_exact(ops, cin, cinp, cout):
    """5x5 rows on the slab kernel at B = 7: 48 -> 192 (row-paired c-tile 1) and 128 -> 128."""
    run_wgrad_slab(ops, 19, 5, cin, cinp, cout, 7, seed=4100 + cin)


@pytest.mark.parametrize("ks,cin,cout,hi,hg", [(3, 64, 128, 1, 1), (5, 192, 384, 2, 2),
                                               (3, 192, 192, 2, 1), (5, 32, 192, 2, 1)])
def test_wgrad_fp32_partial_kernels_exact(ops, ks, cin, cout, hi, hg):
    """The all-taps kernel (hi == hg, widths outside 128 / 192) and the gather kernel (hi != hg),
    dense integer operands: their partials are fp32."""
    B, S = 3, 19
    xp, gp, ref_dw, ref_db = wgrad_case(ops, S, ks, cin, cin, cout, B, hi, hg, 4200 + ks + cin)
    dw = torch.full((cout, cin, ks, ks), NAN, device=DEV)
    db = torch.full((cout,), NAN, device=DEV)
    ops.conv_wgrad(gp, xp, dw, db, B, S, hi, cout, cout, cin, cin, ks, hg=hg)
    assert torch.equal(dw, ref_dw) and torch.equal(db, ref_db)
    ops.conv_wgrad(gp, xp, dw, db, B, S, hi, cout, cout, cin, cin, ks, accumulate=True, hg=hg)
    assert torch.equal(dw, 2 * ref_dw) and torch.equal(db, 2 * ref_db)
