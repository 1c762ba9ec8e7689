"""-m gpu: the LayerNorm kernels of csrc/norm.hip -- ecamp_layernorm_fwd / ecamp_layernorm_bwd on f32, bfloat16 and IEEE-half rows,
ecamp_layernorm_fwd_x32 / ecamp_layernorm_bwd_z32 on the f32 stream beside 16-bit rows -- against float64, element by element.

test_kernels_gpu.py, test_layernorm_layouts_gpu.py and test_f32_residual_gpu.py judge them by max|err| / max|ref| per tensor, from
zeroed dgamma / dbeta, at two trips of the backward's row loop, and never look at rstd.  Here every element of y, z, mean, rstd, dz,
dx_drop, dgamma and dbeta is held to |got - ref| <= K u A (tests/_ln_ref.py, proven in tests/test_ln_reference_cpu.py):
  ref  float64 on the values the kernel was given; everything downstream of z on the z the kernel stored,
  A    the same arithmetic on magnitudes; A == 0 is a structural zero and must compare equal to zero,
  u    2^-24, 2^-9 or 2^-12 for the rows, 2^-24 for mean, rstd, dgamma, dbeta,
  K    max(1, 4 K_yard), K_yard the figure of the same arithmetic in float32 on the CPU (dgamma / dbeta: rows in at most 256 groups,
       the groups chained onto the prior contents in several orders, the worst of which counts).  Nothing is a fixed number.
Regimes: plain, offset (mean far above spread), scales (2^-6 rows beside 2^6 rows), special (a constant row whose mean and y must be
exact, a row whose dy is zero, a zero and negative gammas).  dgamma / dbeta always start from nonzero contents; one case calls the
backward twice into the same buffers; dx_drop runs under the forward's mask at p = 0.1 and, at p = 0, must be dz bit for bit.
Columns: both sides of every rung of the layout selection, one active lane, the maximum of 2048; rows 1 and 5 everywhere, and
R_BIG = 8197 (three trips of every backward form: the middle one consumes a prefetched row and issues the next prefetch; the last is
ragged) once per backward instantiation and at the production width of 768.  For every case ecamp_layernorm_layout must return
what the mirror of the selection in _ln_ref.py returns, and that must be the instantiation the case is listed for.

Every case prints K_yard, the kernel's figure and the bound per quantity before it asserts; profiles/layernorm_float64.txt is a
digest of one such run on an MI355X (tools/ln_float64_digest.py): the largest figures over all lines and every case at 8197 rows.
Largest kernel figure over the cases there, with the K_yard and the bound of the case it occurred in:
    plain + fused  f32        z 2.73 / 2.73 (10.9)  y 3.35 / 3.93 (15.7)  mean 2.29 / 2.29 (9.2)  rstd 0.92 / 1.21 (4.8)  dz 2.61 / 3.08 (12.3)
                              dx_drop 1.75 / 1.75 (7.0)  dgamma 3.58 / 3.58 (14.3)  dbeta 3.22 / 3.22 (12.9)
                   bfloat16   z 1.99 / 1.99 (8.0)   y 1.83 / 1.83 (7.3)   mean 0.77 / 0.77 (3.1)  rstd 0.92 / 1.15 (4.6)  dz 1.66 / 1.66 (6.6)
                              dx_drop 1.76 / 1.76 (7.0)  dgamma 3.27 / 2.73 (10.9)  dbeta 2.65 / 2.43 (9.7)
                   IEEE half  z 2.00 / 2.00 (8.0)   y 1.69 / 1.69 (6.8)   mean 0.95 / 0.95 (3.8)  rstd 0.98 / 1.14 (4.6)  dz 1.64 / 1.64 (6.6)
                              dx_drop 1.78 / 1.78 (7.1)  dgamma 3.70 / 3.70 (14.8)  dbeta 2.61 / 2.77 (11.1)
    f32 stream     bfloat16   y 1.83 / 1.83 (7.3)   mean 2.41 / 3.17 (12.7)  rstd 0.90 / 1.21 (4.8)  dz 1.62 / 1.62 (6.5)  dgamma 2.88 / 2.96 (11.8)
                              dbeta 2.65 / 2.43 (9.7)
                   IEEE half  y 1.71 / 1.71 (6.9)   mean 2.41 / 3.17 (12.7)  rstd 0.90 / 1.21 (4.8)  dz 1.60 / 1.60 (6.4)  dgamma 2.90 / 2.52 (10.1)
                              dbeta 2.61 / 2.77 (11.1)
No figure is above its bound; the line that comes closest to its own is mean at 0.771 of 1.00 (f32, offset, 1 x 776), then rstd at
0.81 of 1.07 (bfloat16, scales, 5 x 776).  The 16-bit rows reproduce the yardstick's roundings to three digits; rstd (the same rsqrtf
as the embedding kernel, 0.47 to 0.78 there) stays below one.  In the offset regime of the f32 stream A carries |z| + mean|z| = 4096
twice where y and dz are of order one, so a 16-bit y or dz row cannot fail there (figures of 0.001) and rstd hardly can: the stream
entries therefore make their three trips at 8197 rows in the special regime, where A is about three times |dz|, and offset rides along
at 768 columns for mean, dgamma and dbeta; the variance faults of test_ln_reference_cpu.py are caught through rstd at 5 rows."""
import os

import pytest
import torch

import _ln_ref as L

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif("ECAMP_LN_BWD" in os.environ, reason="ECAMP_LN_BWD overrides the selection these shapes are sized for")]

DT16 = [torch.bfloat16, torch.float16]
DT = [torch.float32] + DT16


def ops():
    from ecamp_amd import hip_ops
    return hip_ops


def shifted(t):
    """A contiguous copy of the 16-bit tensor `t` that starts 4 elements (8 bytes) into a larger buffer (as test_layernorm_layouts_gpu.py
    builds them: the 4-wide forms make 8-byte accesses, never less)."""
    assert t.element_size() == 2
    buf = torch.empty(t.numel() + 8, device=t.device, dtype=t.dtype)
    v = buf[4:4 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 8
    return v


def put(t, dev, dtype, misaligned=False):
    v = t.to(dev, dtype)
    assert v.data_ptr() % 16 == 0
    return shifted(v) if misaligned else v


def check_layout(rows16, cols, mis_fwd, mis_bwd):
    """The library's selection == the mirror's == the instantiation the case is listed for."""
    o = ops()
    for backward, mis in ((False, mis_fwd), (True, mis_bwd)):
        got, want = o.layernorm_layout(backward, rows16, cols, not mis), L.ln_layout(backward, rows16, cols, not mis)
        assert got == want, "layout of %s cols %d: the library says %s, the mirror %s" % ("bwd" if backward else "fwd", cols, got, want)
        form = L.intended(rows16, cols, mis)[1 if backward else 0]
        assert got[:len(form)] == form, "cols %d reaches %s, listed for %s" % (cols, got, form)


def report(lines, bad):
    for ln in lines:
        print(ln)
    assert not bad, "\n".join(bad)


def name(fmt, regime, rows, cols, mis=False, eps=L.EPS, extra=""):
    return "%s-%s-%dx%d%s%s%s" % (fmt, regime, rows, cols, "-mis" if mis else "", "" if eps == L.EPS else "-eps%g" % eps, extra)


# ================================================================================================ ecamp_layernorm_fwd / ecamp_layernorm_bwd
def _plain_cases():
    out = []
    for dt in DT:
        twins = lambda cols: (False, True) if (cols in L.MISALIGNED_COLS and dt != torch.float32) else (False,)   # f32 rows are never misaligned
        for regime in L.REGIMES:
            for cols in L.COLS:
                for rows in L.SMALL_ROWS:
                    out += [(dt, regime, rows, cols, mis, L.EPS) for mis in twins(cols)]     # a twin follows its sibling: one reference
        out.append((dt, "plain", 5, 768, False, L.EPS_BERT))
        out += [(dt, "special", L.R_BIG, cols, mis, L.EPS) for cols, mis in (L.BIG_32 if dt == torch.float32 else L.BIG_16)]
        out.append((dt, "plain", L.R_BIG, 768, False, L.EPS))
    return out


PLAIN = _plain_cases()


@pytest.mark.parametrize("dtype,regime,rows,cols,misaligned,eps", PLAIN, ids=[name(L.fmt_of(c[0]), *c[1:]) for c in PLAIN])
def test_plain_entries(dev, dtype, regime, rows, cols, misaligned, eps):
    """ecamp_layernorm_fwd without fusion (z is x) and ecamp_layernorm_bwd on its mean and rstd: without dres, then with dres and
    want_drop at p == 0 (dx_drop must be dz bit for bit), from nonzero dgamma / dbeta; at 768 columns of the plain regime a second
    call into the same buffers.  Misaligned: x in the forward; x, dy and dres in the backward."""
    o, fmt = ops(), L.fmt_of(dtype)
    c = L.case(fmt, regime, rows, cols)
    G = c.graph_x(eps)
    check_layout(fmt != L.F32, cols, misaligned, misaligned)
    tag = name(fmt, regime, rows, cols, misaligned, eps)
    x, dy, dres = (put(t, dev, dtype, misaligned) for t in (c.x, c.dy, c.dres))
    g, b = c.gamma.to(dev), c.beta.to(dev)
    y, z, mean, rstd = o.layernorm_fwd(x, g, b, eps)
    assert z is x and y.dtype == dtype
    lines, bad = L.judge(tag, G, dict(y=y.cpu(), mean=mean.cpu(), rstd=rstd.cpu()))
    for with_dres in (False, True):
        gg, gb = c.prior_g.to(dev), c.prior_b.to(dev)
        if with_dres:
            dz, dxd = o.layernorm_bwd(dy, x, mean, rstd, g, gg, gb, dres=dres, want_drop=True)
            got = dict(dz=dz.cpu(), dx_drop=dxd.cpu(), dgamma=gg.cpu(), dbeta=gb.cpu())
        else:
            got = dict(dz=o.layernorm_bwd(dy, x, mean, rstd, g, gg, gb).cpu(), dgamma=gg.cpu(), dbeta=gb.cpu())
        more = L.judge(tag + (" +dres" if with_dres else ""), G, got, dres=with_dres)
        lines, bad = lines + more[0], bad + more[1]
    if regime == "plain" and cols == 768:
        o.layernorm_bwd(dy, x, mean, rstd, g, gg, gb, dres=dres)
        more = L.judge(tag + " twice", G, dict(dgamma=gg.cpu(), dbeta=gb.cpu()), dres=True, times=2)
        lines, bad = lines + more[0], bad + more[1]
    report(lines, bad)


FUSED = [(dt, fused, rows, cols, L.EPS) for dt in DT for cols in L.FUSED_COLS for rows in (5, L.R_BIG) for fused in ("res", "drop")]
FUSED += [(dt, fused, 5, 768, L.EPS_BERT) for dt in DT for fused in ("res", "drop")]


@pytest.mark.parametrize("dtype,fused,rows,cols,eps", FUSED, ids=[name(L.fmt_of(c[0]), "plain", c[2], c[3], False, c[4], "-" + c[1]) for c in FUSED])
def test_fused_entries(dev, dtype, fused, rows, cols, eps):
    """LN(x + res) and LN(dropout(x) + res) at p = 0.1: z against x keep / (1 - p) + res, everything else on the z the kernel stored;
    the backward with dres and want_drop under the forward's mask (hip_ops.dropout_mask), from nonzero dgamma / dbeta."""
    o, fmt = ops(), L.fmt_of(dtype)
    c = L.case(fmt, "plain", rows, cols)
    check_layout(fmt != L.F32, cols, False, False)
    tag = name(fmt, "plain", rows, cols, False, eps, "-" + fused)
    p = L.DROP_P if fused == "drop" else 0.0
    kw = dict(drop_p=p, seed=L.DROP_SEED, offset=L.DROP_OFFSET) if p else {}
    keep = o.dropout_mask((rows, cols), dev, p, L.DROP_SEED, L.DROP_OFFSET).cpu() if p else None
    if p:
        assert abs(float(keep.float().mean()) - (1 - p)) < 0.03 and (keep == 0).any()
    x, res, dy, dres = (put(t, dev, dtype) for t in (c.x, c.res, c.dy, c.dres))
    g, b = c.gamma.to(dev), c.beta.to(dev)
    y, z, mean, rstd = o.layernorm_fwd(x, g, b, eps, residual=res, **kw)
    assert z is not x and z.dtype == dtype
    lines, bad = L.judge_z(tag, c, z.cpu(), keep, p)
    G = L.Graph(c, z.float().cpu(), eps)
    more = L.judge(tag, G, dict(y=y.cpu(), mean=mean.cpu(), rstd=rstd.cpu()))
    lines, bad = lines + more[0], bad + more[1]
    gg, gb = c.prior_g.to(dev), c.prior_b.to(dev)
    dz, dxd = o.layernorm_bwd(dy, z, mean, rstd, g, gg, gb, dres=dres, want_drop=True, **kw)
    more = L.judge(tag + " +dres", G, dict(dz=dz.cpu(), dx_drop=dxd.cpu(), dgamma=gg.cpu(), dbeta=gb.cpu()), dres=True, keep=keep, p=p)
    report(lines + more[0], bad + more[1])


# ================================================================================================ the f32 stream
def _stream_cases():
    out = []
    for dt in DT16:
        twins = lambda cols: (False, True) if cols in L.MISALIGNED_COLS else (False,)
        for regime in L.STREAM_REGIMES:
            for cols in L.COLS:
                for rows in L.SMALL_ROWS:
                    out += [(dt, regime, rows, cols, mis) for mis in twins(cols)]
        # 8197 rows in `special`: in `offset` A holds |z| + mean|z| = 4096 twice and a 16-bit dz row cannot fail (test_ln_reference_cpu.py
        # seeds three row-loop faults in both); `offset` rides along at the production width for mean, rstd, dgamma and dbeta
        out += [(dt, "special", L.R_BIG, cols, mis) for cols, mis in L.BIG_16]
        out.append((dt, "offset", L.R_BIG, 768, False))
    return out


STREAM = _stream_cases()


@pytest.mark.parametrize("dtype,regime,rows,cols,misaligned", STREAM, ids=[name(L.fmt_of(c[0]), *c[1:], extra="-stream") for c in STREAM])
def test_stream_entries(dev, dtype, regime, rows, cols, misaligned):
    """ecamp_layernorm_fwd_x32 and ecamp_layernorm_bwd_z32 without and with dres, from nonzero dgamma / dbeta.  Misaligned: dy and
    dres (z stays aligned, the entry requires it; the forward's only 16-bit row is the output the wrapper allocates, so the forward
    is the aligned twin's and is judged there)."""
    o, fmt = ops(), L.fmt_of(dtype)
    c = L.case(fmt, regime, rows, cols, True)
    G = c.graph_x(L.EPS)
    check_layout(True, cols, False, misaligned)
    tag = name(fmt, regime, rows, cols, misaligned, extra="-stream")
    zf = put(c.x, dev, torch.float32)
    dy, dres = put(c.dy, dev, dtype, misaligned), put(c.dres, dev, dtype, misaligned)
    g, b = c.gamma.to(dev), c.beta.to(dev)
    y, z, mean, rstd = o.layernorm_fwd_x32(zf, g, b, L.EPS, dtype)
    assert z is zf and y.dtype == dtype
    lines, bad = ([], []) if misaligned else L.judge(tag, G, dict(y=y.cpu(), mean=mean.cpu(), rstd=rstd.cpu()))
    for with_dres in (False, True):
        gg, gb = c.prior_g.to(dev), c.prior_b.to(dev)
        dz = o.layernorm_bwd_z32(dy, zf, mean, rstd, g, gg, gb, dres=dres if with_dres else None)
        assert dz.dtype == dtype
        more = L.judge(tag + (" +dres" if with_dres else ""), G, dict(dz=dz.cpu(), dgamma=gg.cpu(), dbeta=gb.cpu()), dres=with_dres)
        lines, bad = lines + more[0], bad + more[1]
    report(lines, bad)
