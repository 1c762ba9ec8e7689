"""-m gpu: the five LayerNorm entries at the smallest shapes that reach every layout their host side selects (csrc/norm.hip), against
F.layer_norm and its autograd in float64 on identical inputs.

Rows: 5 (one whole forward workgroup of 4 rows and a partial one; less than one backward workgroup) and 4117 (more than 256 x 16, so
every backward form makes a second, ragged trip through its row loop).  Columns, and what each selects:

  cols   16-bit forward                  16-bit backward                            f32 rows (forward and backward)
   196   4-wide, 1 chunk, partly filled  4-wide x 16 waves, 1 chunk                 1 chunk
   264   8-wide, 1 chunk (33 lanes)      8-wide x 16 waves, gamma in registers      2 chunks
   520   8-wide, 2 chunks                4-wide, 3 chunks                           3 chunks
   776   8-wide, 2 chunks                8-wide two-chunk x 12 waves, gamma in LDS  4 chunks
  1032   8-wide, 4 chunks                4-wide, 8 chunks                           8 chunks

Misaligned 16-bit cases (520 and 776 columns): the row tensors the caller owns start exactly 4 elements = 8 bytes into a larger
buffer, which sends both passes to the 4-wide forms (3 and 4 chunks).  Never less: the 4-wide forms make 8-byte accesses.  f32 tensors
are never misaligned: the f32 kernels make 16-byte accesses and the library does not check that alignment.

Tolerances are those of the tests that hold the same quantities at round sizes: test_kernels_gpu.py (test_layernorm,
test_layernorm_dropout_residual_matches_pytorch_under_the_same_mask, test_fp8_delayed_scaling_kernels) for the plain entries and
test_f32_residual_gpu.py for the f32-stream entries.  The per-element float64 bounds on every quantity of these entries (rstd and
nonzero prior contents of dgamma / dbeta included) live in test_ln_float64_gpu.py, which also checks the table above against
ecamp_layernorm_layout for every case it runs."""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import h16
from test_f32_residual_gpu import _eps16
from test_kernels_gpu import DT, TOL, check

pytestmark = pytest.mark.gpu

ROWS = (5, 4117)
COLS = (196, 264, 520, 776, 1032)
MISALIGNED_COLS = (520, 776)
# (rows, cols, misaligned): a misaligned case follows its aligned twin, so the two share one reference
SHAPES = [(r, c, mis) for r in ROWS for c in COLS for mis in ((False, True) if c in MISALIGNED_COLS else (False,))]
PLAIN = [(dt, r, c, mis) for dt in DT for (r, c, mis) in SHAPES if not (mis and dt == torch.float32)]   # f32 rows are never misaligned
DROP_COLS = (264, 776)


def ops():
    from ecamp_amd import hip_ops
    return hip_ops


def shifted(t):
    """A contiguous copy of the 16-bit tensor `t` that starts 4 elements (8 bytes) into a larger buffer."""
    assert t.element_size() == 2
    buf = torch.empty(t.numel() + 8, device=t.device, dtype=t.dtype)
    v = buf[4:4 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 8
    return v


def place(t, misaligned):
    return shifted(t) if misaligned else t


def _randn(dev, seed, *shape):
    return torch.randn(*shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


@functools.lru_cache(maxsize=1)
def plain_case(dev, dtype, rows, cols, eps):
    """Inputs rounded to `dtype` and the float64 results: LN(x) with its gradients under dy, and LN(round(x + res))."""
    c = {}
    c["x"] = (_randn(dev, 1, rows, cols) * 2 + 0.3).to(dtype)
    c["res"] = _randn(dev, 2, rows, cols).to(dtype)
    c["g"], c["b"] = 1 + 0.1 * _randn(dev, 3, cols), 0.1 * _randn(dev, 4, cols)
    c["dy"] = _randn(dev, 5, rows, cols).to(dtype)
    c["dres"] = _randn(dev, 6, rows, cols).to(dtype)
    xr = c["x"].double().requires_grad_(True)
    gr, br = c["g"].double().requires_grad_(True), c["b"].double().requires_grad_(True)
    yr = F.layer_norm(xr, (cols,), gr, br, eps)
    yr.backward(c["dy"].double())
    c["y"], c["mean"], c["dx"], c["dgamma"], c["dbeta"] = yr.detach(), c["x"].double().mean(1), xr.grad, gr.grad, br.grad
    c["zz"] = (c["x"].double() + c["res"].double()).to(dtype).double()
    c["y_zz"] = F.layer_norm(c["zz"], (cols,), c["g"].double(), c["b"].double(), eps)
    return c


@pytest.mark.parametrize("dtype,rows,cols,misaligned", PLAIN)
def test_layernorm_fwd_bwd_layouts(dev, dtype, rows, cols, misaligned):
    """ecamp_layernorm_fwd / ecamp_layernorm_bwd with and without residual / dres (test_layernorm's quantities and bounds).  Misaligned:
    x and residual in the forward, dy and dres in the backward."""
    o = ops()
    eps = 1e-6
    c = plain_case(dev, dtype, rows, cols, eps)
    tol = TOL[dtype]
    gtol = 2e-5 if dtype == torch.float32 else 1e-2
    x, res, dy, dres = (place(c[k], misaligned) for k in ("x", "res", "dy", "dres"))
    y, z, mean, rstd = o.layernorm_fwd(x, c["g"], c["b"], eps)
    assert z is x
    check("ln y", y, c["y"], tol)
    check("ln mean", mean, c["mean"], 1e-5)
    for with_dres in (True, False):
        gg, gb = torch.zeros(cols, device=dev), torch.zeros(cols, device=dev)
        dz = o.layernorm_bwd(dy, c["x"], mean, rstd, c["g"], gg, gb, dres=dres if with_dres else None)
        check("ln dx(+dres)" if with_dres else "ln dx", dz, c["dx"] + c["dres"].double() if with_dres else c["dx"], tol)
        check("ln dgamma", gg, c["dgamma"], gtol)
        check("ln dbeta", gb, c["dbeta"], gtol)
    y2, z2, _, _ = o.layernorm_fwd(x, c["g"], c["b"], eps, residual=res)
    check("ln(x+res) z", z2, c["zz"], tol)
    check("ln(x+res) y", y2, c["y_zz"], tol)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("cols", DROP_COLS)
def test_layernorm_dropout_layouts(dev, dtype, rows, cols):
    """LN(dropout(x) + residual), p = 0.1, and its backward with the gradient through the mask (want_drop), under the same keep-mask."""
    o = ops()
    p, seed, offset, eps = 0.1, 987654321, 17, 1e-12
    x, res, dy = (_randn(dev, s, rows, cols).to(dtype) for s in (1, 2, 5))
    g, b = 1 + 0.1 * _randn(dev, 3, cols), 0.1 * _randn(dev, 4, cols)
    keep = o.dropout_mask((rows, cols), dev, p, seed, offset).double()
    assert abs(keep.mean().item() - (1 - p)) < 0.03
    xr, rr = x.double().requires_grad_(True), res.double().requires_grad_(True)
    gr, br = g.double().requires_grad_(True), b.double().requires_grad_(True)
    z_ref = xr * keep / (1 - p) + rr
    y_ref = F.layer_norm(z_ref, (cols,), gr, br, eps)
    y_ref.backward(dy.double())
    y, z, mean, rstd = o.layernorm_fwd(x, g, b, eps, residual=res, drop_p=p, seed=seed, offset=offset)
    tol = TOL[dtype]
    check("ln dropout z", z, z_ref, tol)
    check("ln dropout y", y, y_ref, tol * 2)
    gg, gb = torch.zeros(cols, device=dev), torch.zeros(cols, device=dev)
    dz, dxd = o.layernorm_bwd(dy, z, mean, rstd, g, gg, gb, drop_p=p, seed=seed, offset=offset, want_drop=True)
    check("ln dropout d residual", dz, rr.grad, tol * 2)
    check("ln dropout d dense-out", dxd, xr.grad, tol * 2)
    ptol = 1e-2 if dtype != torch.float32 else 2e-5
    check("ln dropout dgamma", gg, gr.grad, ptol)
    check("ln dropout dbeta", gb, br.grad, ptol)


Q8_SHAPES = [(c, r) for r in ROWS for c in DROP_COLS] + [(768, 5), (2048, 5)]   # + the production width and the documented maximum


@pytest.mark.parametrize("cols,rows", Q8_SHAPES)
def test_layernorm_q8_layouts(dev, rows, cols):
    """ecamp_layernorm_fwd_q8 (bf16): y is the plain entry's, the e4m3 copy is bit-identical to quantising that y afterwards and the
    site's amax slots hold max|y| -- with and without the fused residual + dropout.  (The plain entry itself is held to float64 per
    element in test_ln_float64_gpu.py.)"""
    o = ops()
    assert h16() == torch.bfloat16
    xx, rr = _randn(dev, 3, rows, cols).to(h16()), _randn(dev, 4, rows, cols).to(h16())
    g, b = 1.0 + 0.1 * _randn(dev, 5, cols), 0.1 * _randn(dev, 6, cols)
    for kw in ({}, dict(residual=rr, drop_p=0.1, seed=7, offset=9)):
        sc, sl = torch.tensor([0.011], device=dev), torch.zeros(512, device=dev)
        y, z, mean, rstd, y8 = o.layernorm_fwd(xx, g, b, 1e-6, q8_site=(sc, sl), **kw)
        y0 = o.layernorm_fwd(xx, g, b, 1e-6, **kw)[0]
        assert torch.equal(y, y0)
        sl0 = torch.zeros(512, device=dev)
        assert torch.equal(y8, o.quantize_fp8_site(y0, sc, sl0, True))
        assert sl.view(16, 32)[:, 0].max().item() == y0.float().abs().max().item()


# ---- the f32-stream entries: f32 LayerNorm input, every other row 16-bit
@functools.lru_cache(maxsize=1)
def stream_case(dev, dtype, rows, cols):
    """f32 rows at 2048 + N(0, 1), 16-bit dy / dres, and the float64 results."""
    c = {}
    c["z"] = 2048.0 + _randn(dev, 7, rows, cols)
    c["g"], c["b"] = 1.0 + 0.1 * _randn(dev, 8, cols), 0.1 * _randn(dev, 9, cols)
    c["dy"], c["dres"] = _randn(dev, 10, rows, cols).to(dtype), _randn(dev, 11, rows, cols).to(dtype)
    zr = c["z"].double().requires_grad_(True)
    gr, br = c["g"].double().requires_grad_(True), c["b"].double().requires_grad_(True)
    yr = F.layer_norm(zr, (cols,), gr, br, 1e-6)
    yr.backward(c["dy"].double())
    var = c["z"].double().var(1, unbiased=False)
    c["y"], c["mean"], c["rstd"] = yr.detach(), c["z"].double().mean(1), (var + 1e-6).rsqrt()
    c["dz"], c["dgamma"], c["dbeta"] = zr.grad, gr.grad, br.grad
    return c


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows,cols,misaligned", SHAPES)
def test_layernorm_x32_z32_layouts(dev, dtype, rows, cols, misaligned):
    """ecamp_layernorm_fwd_x32 and ecamp_layernorm_bwd_z32 with and without dres; misaligned: dy and dres (z stays aligned, the entry
    requires it; the forward's only 16-bit row is the output the wrapper allocates, so the forward runs once per shape)."""
    o = ops()
    c = stream_case(dev, dtype, rows, cols)
    y, z, mean, rstd = o.layernorm_fwd_x32(c["z"], c["g"], c["b"], 1e-6, dtype)
    if not misaligned:
        assert y.dtype == dtype and z is c["z"]
        err = (y.double() - c["y"]).abs().max().item() / c["y"].abs().max().item()
        emu = (mean.double() - c["mean"]).abs().max().item()
        ers = ((rstd.double() - c["rstd"]) / c["rstd"]).abs().max().item()
        print("ln_fwd_x32 %s %d x %d: y rel err %.2e, mean abs err %.2e, rstd rel err %.2e" % (dtype, rows, cols, err, emu, ers))
        assert err < 2 * _eps16(dtype)
        assert emu < 1e-3
        assert ers < 1e-3
    dy, dres = place(c["dy"], misaligned), place(c["dres"], misaligned)
    for with_dres in (True, False):
        gg, gb = torch.zeros(cols, device=dev), torch.zeros(cols, device=dev)
        dz = o.layernorm_bwd_z32(dy, c["z"], mean, rstd, c["g"], gg, gb, dres=dres if with_dres else None)
        ref = c["dz"] + c["dres"].double() if with_dres else c["dz"]
        err = (dz.double() - ref).abs().max().item() / ref.abs().max().item()
        eg = (gg.double() - c["dgamma"]).norm().item() / c["dgamma"].norm().item()
        eb = (gb.double() - c["dbeta"]).norm().item() / c["dbeta"].norm().item()
        print("ln_bwd_z32 %s %d x %d (dres %d, misaligned %d): dz rel err %.2e, dgamma %.2e, dbeta %.2e"
              % (dtype, rows, cols, with_dres, misaligned, err, eg, eb))
        assert dz.dtype == dtype
        assert err < 2 * _eps16(dtype)
        assert eg < 1e-3 and eb < 1e-5
