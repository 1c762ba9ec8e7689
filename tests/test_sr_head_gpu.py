"""-m gpu: the four kernels of the super-resolution head (csrc/vision.hip, K12) -- sr_fused_fwd/bwd_kernel (mode 0, f32 stencils) and
sr_pair_fwd/bwd_kernel (mode 1, 4x4x4 matrix cores, what every 16-bit training step runs) -- against float64, element by element.

test_kernels_gpu.py judges the head by max|err| / max|ref| (mode 0) and by mean errors on the bfloat16 build (mode 1), at no more
than 108 tiles.  Neither can see a halo off by one in the thin gradient band next to the window, a tile cursor that loses a carry, a
skipped tile that is not zero-filled, or the IEEE-half build.  Here every element is held to |got - ref| <= K u A:
  ref  the float64 autograd graph of tests/_sr_ref.py (proven in tests/test_sr_reference_cpu.py),
  A    the same graph on absolute values without the ReLUs: the sum of the magnitudes of every term that reaches the element;
       A == 0 is a structural zero and must be +0.0 in the output,
  u    2^-24 for mode 0; for mode 1 the figure the 16-bit format is held to, 2^-9 on the bfloat16 build and 2^-12 on the IEEE-half
       build (half a rounding of either format),
  K    max(1, 4 K_yard) per quantity: K_yard is the largest err / (u A) of a yardstick on the same inputs -- for mode 0 the head in
       float32 on the CPU (sums chained tile by tile, as atomics chain workgroups), for mode 1 the float64 head with u, c1, ds, dc1
       and the tap weights rounded to 16 bits.  Nothing is a fixed number; every case prints K_yard and the kernel's own figure
       (profiles/sr_head_float64.txt is that output on an MI355X).
The shapes (tests/_sr_ref.py: SHAPES) are the smallest that run what the workload runs: one tile holding all four image borders, a
full ring of neighbour tiles and a clipped window, the production geometry (G = 14, win 12), and one shape above each launcher's grid
cap -- 576 and 588 tiles for the pair backward's 512 workgroups (every carry of its cursor, zero-filled skips between reachable
tiles, the cross-iteration prefetch, accumulators that live across tiles), 1044 for the fused backward's 1024, 2052 for the forwards'
2048.  The mixed regime (half the gates closed) is checked per element in mode 0 only, with the elements that an undecided gate can
reach excluded (at most 2 %); at 16 bits a few percent of all gates are within rounding of zero and the aggregate test
test_kernels_gpu.py::test_sr_head_matrix_core_mode stays the judge.

Measured on an MI355X (every line: profiles/sr_head_float64.txt), kernel err / (u A) against the yardstick's, largest over the cases:
    mode 0  s 4.95 / 1.76 (bound 7.0)   dsr 1.53 / 0.93 (3.7)   gw 3.2 / 6.6 (26; production, 588 chained workgroups)   loss 0.35 / 0.35
    mode 1  bfloat16  dsr 1.28 / 1.28   gw 0.157 / 0.157   loss 0.055 / 0.055        IEEE half  dsr 0.889 / 0.889   gw 0.154   loss 0.035
The mode-1 kernels reproduce the rounding model to three digits on both builds.  The sums that leave the workgroups through float
atomics (loss, gw) are measured against a float32 CHAIN of the per-tile sums, not against torch's own reductions: those are pairwise
(or accumulate in double) and sit 10x closer to float64 than any chain of as many float32 additions can -- the first run of this file
had the fused backward at 6.1 against a pairwise yardstick of 0.46 at the production shape, which is the chain's own rounding
(0.29 ulp x sqrt(432 additions)), not an error of the kernel."""
import os

import pytest
import torch

import _sr_ref as S

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif("ECAMP_SR_BLOCKS" in os.environ, reason="ECAMP_SR_BLOCKS overrides the grid these shapes are sized for")]

ALL = list(S.SHAPES)
MODE1 = [s for s in ALL if s != "fused-bwd-trips"]


def ops():
    from ecamp_amd import hip_ops
    return hip_ops


def hip_error():
    from ecamp_amd._lib import EcampHipError
    return EcampHipError


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def on_device(H, dev, u8=False):
    return dict(p=H.p.to(dev), big=(H.big_u8 if u8 else H.big).to(dev), column=H.column.to(dev), row=H.row.to(dev),
                ws=[t.to(dev).contiguous() for t in H.ws])


def run(H, dev, mode, u8=False, image=False):
    """What the kernels give for the case: loss (and s from ecamp_sr_image) if the shape checks the forward, dsr and gw if the backward."""
    o, d, out = ops(), on_device(H, dev, u8), {}
    if "fwd" in H.what:
        loss = torch.zeros(1, device=dev)
        o.sr_fwd(d["p"], d["big"], d["column"], d["row"], *d["ws"], loss, S.SRT, H.win, mode)
        out["loss"] = loss.cpu().double()[0]
        if image:
            out["s"] = o.sr_image(d["p"], *d["ws"]).cpu()
    if H.bwd:
        gw = torch.zeros(168, device=dev)
        out["dsr"] = o.sr_bwd(d["p"], d["big"], d["column"], d["row"], *d["ws"], gw, S.SRT, H.win, mode).cpu()
        out["gw"] = gw.cpu()
    return out


def judge(tag, H, got, u, k_yard, keep={}, allowance={}, ref=None, A=None):
    """Every quantity of `got` per element against K u A, K = max(1, 4 K_yard); structural zeros exactly +0.0.  Prints before it asserts."""
    ref, A, bad = ref or H.ref, A or H.A, []
    for q, g in got.items():
        k = S.k_of(g, ref[q], A[q], u, keep.get(q), allowance.get(q))
        K = S.bound_k(k_yard[q])
        print("  %-44s %-4s  K_yard %7.3f   kernel %7.3f   bound %6.2f" % (tag, q, k_yard[q], k, K))
        if not k <= K:
            bad.append("%s %s: err / (u A) = %.3f > %.2f (yardstick %.3f)" % (tag, q, k, K, k_yard[q]))
        if torch.is_tensor(g) and g.dim() > 0:
            if not torch.isfinite(g).all():
                bad.append("%s %s: not finite" % (tag, q))
            zero = (A[q] == 0).expand_as(g)
            if not (bits(g)[zero] == 0).all():
                bad.append("%s %s: %d structurally zero elements are not +0.0" % (tag, q, int((bits(g)[zero] != 0).sum())))
    assert not bad, "\n".join(bad)


def open_host(shape, u8=False):
    H = S.host(shape, "open", u8)
    z1, z2 = H.margins()
    assert z1 > 1 and z2 > 1, "the open regime is not open at %s: min z1 %.2f, min z2 %.2f" % (shape, z1, z2)
    return H


# ================================================================================================ mode 0: the f32 stencils
@pytest.mark.parametrize("shape", ALL)
def test_mode0_open_regime(dev, shape):
    """sr_image at every pixel of every tile, the loss, dsr and the 168 gradients; every gate open, nothing excluded."""
    H = open_host(shape)
    judge("mode 0 open %s" % shape, H, run(H, dev, 0, image=True), S.U32, H.k32)


@pytest.mark.parametrize("shape", ALL)
def test_mode0_mixed_regime(dev, shape):
    """The weights of test_kernels_gpu.py: about half the gates closed.  The forward is continuous in every gate and is checked
    everywhere.  dsr is checked outside the stencil reach of the gates that float64 cannot decide at this K (the share is printed and
    capped at 2 %); the 168 sums are allowed what those gates can contribute, summed in float64, on top of K u A."""
    H = S.host(shape, "mixed")
    keep, allowance = {}, {}
    if H.bwd:
        U = H.undecided()
        print("  mode 0 mixed %s: gate K %.2f, undecided z2 %d, z1 %d, excluded share of dsr %.4f" % (shape, U["K"], int(U["z2"].sum()), int(U["z1"].sum()), U["share"]))
        assert U["share"] <= S.EXCLUDED_SHARE_CAP
        keep, allowance = {"dsr": ~U["dsr"]}, {"gw": U["gw_allowance"]}
    judge("mode 0 mixed %s" % shape, H, run(H, dev, 0, image=True), S.U32, H.k32, keep, allowance)


# ================================================================================================ mode 1: the matrix-core pixel pairs
@pytest.mark.parametrize("shape", MODE1)
def test_mode1_open_regime(dev, both_halves, shape):
    """sr_pair_fwd_kernel and sr_pair_bwd_kernel on both 16-bit builds: the loss, dsr and the 168 gradients per element against
    float64, the yardstick being the float64 head with the kernels' roundings in place."""
    H = open_host(shape)
    judge("mode 1 %s open %s" % (both_halves, shape), H, run(H, dev, 1), S.U16[both_halves], H.k16(both_halves))


# ================================================================================================ closed: exact zeros
def chain_bound(H, cap):
    """The loss of the closed regime is sum_window big^2 with nothing else in it.  A workgroup's thread adds at most 16 terms per tile it
    visits, a block sum adds 8 levels, and at most min(tiles, cap) workgroups add into the one float: each addition rounds the running
    sum once, so the relative error is at most that many u (every term is positive)."""
    T = S.tiles(H.shape)
    return (16 * -(-T // cap) + 8 + min(T, cap)) * S.U32


@pytest.mark.parametrize("shape", ["ring-w2", "pair-bwd-trips"])
@pytest.mark.parametrize("mode", [0, 1])
def test_closed_regime_is_exactly_zero(dev, both_halves, mode, shape):
    """b2 = -40, w2 = 0: s == 0 everywhere, so dsr and all 168 gradients are exactly zero -- within reach of the window too, where the
    kernels run all their stages -- and the loss is sum_window big^2."""
    H = S.host(shape, "closed")
    got = run(H, dev, mode, image=mode == 0)
    for q in ("s", "dsr", "gw"):
        if q in got:
            assert (got[q] == 0).all(), "%s: %d non-zero elements" % (q, int((got[q] != 0).sum()))
    want = float((H.mask * H.big.double() ** 2).sum())
    rel = abs(float(got["loss"]) - want) / want
    print("  closed mode %d %s %s: loss rel err %.2e (bound %.2e)" % (mode, both_halves, shape, rel, chain_bound(H, S.CAP_FWD)))
    assert rel <= chain_bound(H, S.CAP_FWD)


# ================================================================================================ ownership
@pytest.mark.parametrize("mode", [0, 1])
def test_outputs_are_owned_and_sums_accumulate(dev, both_halves, mode):
    """ecamp_sr_bwd through the C ABI with dsr pre-filled with NaN (hip_ops.sr_bwd hands it torch.empty) and gw_ws holding seeded values
    of the size of what it is about to receive: every dsr element is written (finite; +0.0 where no window pixel is within reach),
    gw_ws holds its old value plus the gradient, and ecamp_sr_fwd adds to a non-zero loss_sum.  The old values enter the magnitude."""
    from ecamp_amd._lib import call
    o = ops()
    H = open_host("pair-bwd-trips")
    d = on_device(H, dev)
    u, ky = (S.U32, H.k32) if mode == 0 else (S.U16[both_halves], H.k16(both_halves))
    sign = torch.where(S.randn((168,), 11) < 0, -1.0, 1.0)
    gw0 = (0.5 * H.A["gw"] * sign).float()
    loss0 = (0.5 * H.ref["loss"]).float().reshape(1)
    dsr = torch.full((H.B, 3, H.R, H.R), float("nan"), device=dev)
    gw, loss = gw0.to(dev), loss0.to(dev)
    call("ecamp_sr_bwd", o.ptr(d["p"]), o.ptr(d["big"]), o.ptr(None), o.ptr(d["column"]), o.ptr(d["row"]), *[o.ptr(t) for t in d["ws"]],
         o.ptr(dsr), o.ptr(gw), H.B, H.R, S.SRT, H.win, mode, o.stream())
    o.sr_fwd(d["p"], d["big"], d["column"], d["row"], *d["ws"], loss, S.SRT, H.win, mode)
    got = dict(dsr=dsr.cpu(), gw=gw.cpu(), loss=loss.cpu().double()[0])
    assert torch.isfinite(got["dsr"]).all(), "%d dsr elements were never written" % int((~torch.isfinite(got["dsr"])).sum())
    ref = dict(dsr=H.ref["dsr"], gw=H.ref["gw"] + gw0.double(), loss=H.ref["loss"] + loss0.double()[0])
    A = dict(dsr=H.A["dsr"], gw=H.A["gw"] + gw0.double().abs(), loss=H.A["loss"] + loss0.double()[0])
    judge("ownership mode %d %s" % (mode, both_halves), H, got, u, ky, ref=ref, A=A)


# ================================================================================================ the uint8 target
@pytest.mark.parametrize("shape", ["ring-w2", "production"])
@pytest.mark.parametrize("mode", [0, 1])
def test_uint8_target(dev, both_halves, mode, shape):
    """BigSrc::at / at2: `big` as uint8 [B, 2R, 2R] against normalise_u8 of the same bytes as f32 [B, 3, 2R, 2R].  dsr has no atomics
    in it and must be the same bits; the loss and the 168 sums are each held to float64 as everywhere else."""
    H = open_host(shape, u8=True)
    u, ky = (S.U32, H.k32) if mode == 0 else (S.U16[both_halves], H.k16(both_halves))
    f32, u8 = run(H, dev, mode), run(H, dev, mode, u8=True)
    assert torch.equal(bits(f32["dsr"]), bits(u8["dsr"])), "dsr differs between the uint8 target and its f32 counterpart"
    judge("u8 mode %d %s %s (f32)" % (mode, both_halves, shape), H, f32, u, ky)
    judge("u8 mode %d %s %s (u8) " % (mode, both_halves, shape), H, u8, u, ky)


def test_uint8_target_at_an_odd_address_is_refused(dev):
    """at2 reads two bytes at once: both entry points refuse a uint8 target that is not 2-byte aligned, in either mode."""
    o = ops()
    H = S.host("one-tile-w1", "open", True)
    d = on_device(H, dev, u8=True)
    n = d["big"].numel()
    store = torch.zeros(n + 2, dtype=torch.uint8, device=dev)
    odd = store[1 - store.data_ptr() % 2:][:n].view_as(d["big"])
    odd.copy_(d["big"])
    assert odd.data_ptr() % 2 == 1
    for mode in (0, 1):
        with pytest.raises(hip_error(), match="2-byte aligned"):
            o.sr_fwd(d["p"], odd, d["column"], d["row"], *d["ws"], torch.zeros(1, device=dev), S.SRT, H.win, mode)
        with pytest.raises(hip_error(), match="2-byte aligned"):
            o.sr_bwd(d["p"], odd, d["column"], d["row"], *d["ws"], torch.zeros(168, device=dev), S.SRT, H.win, mode)
