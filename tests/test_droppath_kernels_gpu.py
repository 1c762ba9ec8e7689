"""-m gpu: ecamp_drop_path_fwd / ecamp_drop_path_bwd (csrc/droppath.hip) against float64, per element, in every dtype form, with the kept
set taken from the development ABI's mask under the same (seed, offset).

Bounds (s = 1 / (1 - float32(p)) in float64; inputs N(0, 1)):
  f32 output      |err| <= 2^-21 (|res| + |s y|)               two f32 roundings and one ulp of s
  16-bit output   that + u max(|exact|, smallest normal), u = 2^-8 (bfloat16) or 2^-11 (IEEE half)   one rounding to the format
  backward        the same with res = 0
The rounding term has the format's floor because a relative bound cannot hold below the smallest normal number (2^-14 in IEEE half):
there the spacing is 2^-24 whatever the value, a correctly rounded result is off by up to 2^-25 = u 2^-14, and NO 16-bit output can do
better.  N(0, 1) gradients reach that range: at p = 0.1 (s = 1.11, not a power of two) the backward of (16, 197, 192) in IEEE half has 17
elements, and (3, 50, 768) 2, whose correctly rounded value misses u |exact| (CPU emulation of the same arithmetic); the forward of
(40, 197, 1024) has one.  With the floor the bound is exactly "one correct rounding", everywhere.  Each case prints how many of its
elements lie below the smallest normal.
Exact statements: a dropped sample's rows are the residual's bits (forward) or +0 (backward); p = 0 is the plain sum; two calls give equal
bits; out = y gives the bits of the unaliased call; canary rows behind the last row are untouched.

Shapes: the vector paths (D % 8 == 0, D % 4 == 0 only), one vector, several samples in one workgroup column, a sample longer than one
pass of its column of workgroups (the stride loop over vectors wraps from T * D / 8 > 1024), (40, 197, 1024), and (4100, 1, 8): more
samples than the launch has rows of workgroups (4096), so the stride loop over samples wraps too."""
import numpy as np
import pytest
import torch
from conftest import h16

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8), (5, 3, 8), (7, 5, 12), (16, 197, 192), (3, 50, 768), (40, 197, 1024), (4100, 1, 8)]
RATES = [0.0, 0.1, 0.5]
CANARY = 2          # rows
SEED, OFFSET = 0x1234ABCD5678EF01, 77


def _rounding(exact, dtype):
    """Error of one correct rounding of `exact` (float64) to `dtype`, as a bound: u max(|exact|, smallest normal); 0 for float32, whose
    roundings the 2^-21 term covers."""
    if dtype == torch.float32:
        return torch.zeros_like(exact)
    u, tiny = (2.0 ** -8, 2.0 ** -126) if dtype == torch.bfloat16 else (2.0 ** -11, 2.0 ** -14)
    return u * exact.abs().clamp_min(tiny)


def _below_normal(exact, dtype):
    tiny = {torch.float32: 2.0 ** -126, torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}[dtype]
    return int(((exact != 0) & (exact.abs() < tiny)).sum())


def _inputs(B, T, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * T, D, generator=g), torch.randn(B * T, D, generator=g)


def _keep(dev, B, p, seed, offset):
    """The kept samples, from the library's own mask.  At p = 0.5 and B >= 16 both kinds must occur (2^-15 that they do not): a failed
    precondition is reported as such -- choose another SEED -- never skipped."""
    from ecamp_amd import hip_ops as ops
    keep = ops.dropout_mask((B,), dev, p, seed, offset).cpu().bool()
    if p == 0:
        assert bool(keep.all())
    if p == 0.5 and B >= 16:
        assert 0 < int(keep.sum()) < B, "precondition: the seed keeps %d of %d samples at p = 0.5 -- choose another SEED" % (int(keep.sum()), B)
    return keep


def _with_canary(t, dev, fill):
    """`t` on the device, followed in the same buffer by CANARY rows of `fill`: -> (the view that is passed, the canary view)."""
    rows, D = t.shape
    buf = torch.full((rows + CANARY, D), fill, dtype=t.dtype, device=dev)
    buf[:rows].copy_(t)
    return buf[:rows], buf[rows:]


SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]


def _form_dtypes(form):
    r, y = form.split("-")
    return (h16() if r == "h16" else torch.float32), (h16() if y == "h16" else torch.float32)


@pytest.mark.parametrize("form", ["h16-h16", "f32-h16"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_forward_with_a_16_bit_branch_against_float64(dev, both_halves, shape, form):
    _forward(dev, both_halves, shape, form)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_forward_in_f32_against_float64(dev, shape):
    _forward(dev, "f32", shape, "f32-f32")


def _forward(dev, both_halves, shape, form):
    from ecamp_amd import hip_ops as ops
    B, T, D = shape
    rdt, ydt = _form_dtypes(form)
    res32, y32 = _inputs(B, T, D, seed=B * 1000 + D)
    res_h, y_h = res32.to(rdt), y32.to(ydt)                      # what the kernel reads, exactly
    res, _ = _with_canary(res_h, dev, 3.0)
    y, _ = _with_canary(y_h, dev, 5.0)
    R, Y = res_h.double(), y_h.double()
    for p in RATES:
        keep = _keep(dev, B, p, SEED, OFFSET)
        out, canary = _with_canary(torch.zeros_like(res_h), dev, 7.0)
        got = ops.drop_path_fwd(res, y, B, T, p, SEED, OFFSET, out=out)
        assert got is out
        s = 1.0 / (1.0 - float(np.float32(p)))
        rows = keep.repeat_interleave(T)
        sy = torch.where(rows[:, None], s * Y, torch.zeros_like(Y))
        exact = R + sy
        err = (out.cpu().double() - exact).abs()
        bound = 2.0 ** -21 * (R.abs() + sy.abs()) + _rounding(exact, rdt)
        worst = float((err / bound.clamp_min(1e-300)).max())
        print("[droppath] fwd %s %s p=%.1f %s: kept %d / %d, worst error / bound %.3f, %d results below the smallest normal"
              % (form, both_halves, p, shape, int(keep.sum()), B, worst, _below_normal(exact, rdt)))
        assert bool((err <= bound).all()), (p, worst)
        assert torch.equal(canary.cpu(), torch.full((CANARY, D), 7.0, dtype=rdt)), "rows behind the last row were written"
        if not bool(keep.all()):      # a dropped sample: the residual's bits
            assert torch.equal(out.cpu()[~rows], res_h[~rows])
        if p == 0:
            assert torch.equal(out.cpu(), (res_h.float() + y_h.float()).to(rdt))
        again = ops.drop_path_fwd(res, y, B, T, p, SEED, OFFSET)
        assert torch.equal(again, out), "two calls must give the same bits"
        if rdt == ydt:                # out may be y itself
            ya = y.clone()
            assert ops.drop_path_fwd(res, ya, B, T, p, SEED, OFFSET, out=ya) is ya
            assert torch.equal(ya, out), "the aliased call must give the bits of the unaliased one"
    assert torch.equal(res.cpu(), res_h) and torch.equal(y.cpu(), y_h)        # inputs are left alone


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_backward_in_16_bits_against_float64(dev, both_halves, shape):
    _backward(dev, both_halves, shape, "h16")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_backward_in_f32_against_float64(dev, shape):
    _backward(dev, "f32", shape, "f32")


def _backward(dev, both_halves, shape, fmt):
    from ecamp_amd import hip_ops as ops
    B, T, D = shape
    dt = h16() if fmt == "h16" else torch.float32
    d32, _ = _inputs(B, T, D, seed=B * 1000 + D + 1)
    d_h = d32.to(dt)
    dout, _ = _with_canary(d_h, dev, 3.0)
    G = d_h.double()
    for p in RATES:
        keep = _keep(dev, B, p, SEED, OFFSET + 1)
        dy = ops.drop_path_bwd(dout, B, T, p, SEED, OFFSET + 1)
        assert dy.dtype == dt and dy.data_ptr() != dout.data_ptr()
        s = 1.0 / (1.0 - float(np.float32(p)))
        rows = keep.repeat_interleave(T)
        exact = torch.where(rows[:, None], s * G, torch.zeros_like(G))
        err = (dy.cpu().double() - exact).abs()
        bound = 2.0 ** -21 * exact.abs() + _rounding(exact, dt)
        worst = float((err / bound.clamp_min(1e-300)).max())
        print("[droppath] bwd %s %s p=%.1f %s: kept %d / %d, worst error / bound %.3f, %d results below the smallest normal"
              % (fmt, both_halves, p, shape, int(keep.sum()), B, worst, _below_normal(exact, dt)))
        assert bool((err <= bound).all()), (p, worst)
        if not bool(keep.all()):      # a dropped sample: exact +0 (every bit clear)
            z = dy.cpu()[~rows]
            assert not bool((z.view(torch.int16 if dt != torch.float32 else torch.int32) != 0).any())
        if p == 0:
            assert torch.equal(dy.cpu(), d_h)
        assert torch.equal(ops.drop_path_bwd(dout, B, T, p, SEED, OFFSET + 1), dy), "two calls must give the same bits"
    assert torch.equal(dout.cpu(), d_h)


def test_backward_leaves_rows_behind_the_last_row_alone(dev, both_halves):
    """ecamp_drop_path_bwd through the C ABI into a buffer with canary rows (the wrapper allocates dy itself)."""
    from ecamp_amd import _lib
    from ecamp_amd import hip_ops as ops
    for B, T, D in ((5, 3, 8), (7, 5, 12), (3, 50, 768)):
        for dt in (h16(), torch.float32):
            d_h = _inputs(B, T, D, seed=9)[0].to(dt)
            dout = d_h.to(dev)
            dy, canary = _with_canary(torch.zeros_like(d_h), dev, 7.0)
            _lib.call("ecamp_drop_path_bwd", ops.ptr(dout), ops.ptr(dy), B, T, D, 0.5, SEED, OFFSET, ops.code(dt), ops.stream())
            assert torch.equal(dy, ops.drop_path_bwd(dout, B, T, 0.5, SEED, OFFSET))
            assert torch.equal(canary.cpu(), torch.full((CANARY, D), 7.0, dtype=dt))


def test_the_mask_depends_on_seed_and_offset_and_nothing_else(dev):
    """Sample b's fate is element b of the dropout convention: the same for every T and D, other under another offset or seed."""
    from ecamp_amd import hip_ops as ops
    B, p = 64, 0.5

    def dropped(T, D, seed, offset):
        res, y = (t.to(dev) for t in _inputs(B, T, D, seed=3))
        out = ops.drop_path_fwd(res, y, B, T, p, seed, offset)
        return (out == res).view(B, -1).all(dim=1).cpu()

    a = dropped(3, 8, SEED, OFFSET)
    assert torch.equal(a, ~ops.dropout_mask((B,), dev, p, SEED, OFFSET).cpu().bool())
    assert torch.equal(a, dropped(2, 12, SEED, OFFSET))
    assert not torch.equal(a, dropped(3, 8, SEED, OFFSET + 1)) and not torch.equal(a, dropped(3, 8, SEED + 1, OFFSET))
