"""No GPU: the reference of tests/_ln_ref.py is what it claims to be -- F.layer_norm and its autograd in float64, the dropout + residual
graph, dres and dx_drop included --, its magnitudes bound it and vanish only at the structural zeros, every regime has its defining
property, every case names the instantiation the selection sends it to, and the judge refuses an output that is subtly wrong while it
accepts the yardstick itself.  For every seeded fault the test prints whether the older yardstick (max|err| / max|ref| per tensor at
the tolerances of test_kernels_gpu.py and test_layernorm_layouts_gpu.py) would have seen it."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _ln_ref as L

FMTS = (L.F32, L.BF16, L.F16)
OLD_TOL = {L.F32: 2e-5, L.BF16: 2e-2, L.F16: 3e-3}       # TOL of test_kernels_gpu.py: y, z, dz, dx_drop
OLD_GTOL = {L.F32: 2e-5, L.BF16: 1e-2, L.F16: 1e-2}      # dgamma, dbeta
OLD_MEAN = 1e-5


def old_check(name, got, ref, tol):
    """check() of test_kernels_gpu.py as a predicate, printed: True when the old yardstick lets `got` pass."""
    err = float((got.double() - ref.double()).abs().max()) / (float(ref.double().abs().max()) + 1e-20)
    print("    old check %-44s rel-err %.3e (tol %.1e): %s" % (name, err, tol, "PASSES" if err <= tol else "seen"))
    return err <= tol


# ================================================================================================ the reference is autograd
@pytest.mark.parametrize("eps", [L.EPS, L.EPS_BERT])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("rows,cols", [(1, 4), (5, 8), (7, 196), (3, 264)])
def test_reference_is_layer_norm_and_its_autograd(rows, cols, regime, p, eps):
    c = L.case(L.F32, regime, rows, cols)
    keep = (torch.rand(rows, cols, generator=torch.Generator().manual_seed(5)) >= p).to(torch.uint8) if p else None
    ks = L.keep_scale(keep, p, torch.float64)
    xr, rr = c.x.double().requires_grad_(True), c.res.double().requires_grad_(True)
    gr, br = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    z = xr * ks + rr
    zref, zA = L.z_reference(c, keep, p)
    assert float((zref - z.detach()).abs().max()) == 0 and (zA >= zref.abs()).all()
    zs = L.stored(zref, L.F32)                                         # what a kernel would have stored
    zu = z + (zs.double() - z).detach()                                # its value, z's gradient
    y = F.layer_norm(zu, (cols,), gr, br, L.eps_given(eps))
    ((y * c.dy.double()).sum() + (zu * c.dres.double()).sum()).backward()
    G = L.Graph(c, zs, eps)
    want = dict(y=y.detach(), mean=zs.double().mean(1), rstd=1 / torch.sqrt(zs.double().var(1, unbiased=False) + L.eps_given(eps)),
                dz=rr.grad, dgamma=c.prior_g.double() + gr.grad, dbeta=c.prior_b.double() + br.grad)
    for q, w in want.items():
        ref, A = G.ref(q, dres=True)
        assert ((ref - w).abs() <= 1e-12 * A).all(), "%s: %.3e of A apart" % (q, float(((ref - w).abs() / A.clamp_min(1e-300)).max()))
    dzr, dzA = G.ref("dz", dres=True)
    assert ((dzr * ks - xr.grad).abs() <= 1e-12 * dzA).all()            # dx_drop: the gradient reaching x through the mask
    nodres = G.ref("dz")[0]
    assert ((nodres + c.dres.double() - rr.grad).abs() <= 1e-12 * dzA).all()
    twice, twiceA = G.ref("dgamma", times=2)
    assert ((twice - c.prior_g.double() - 2 * gr.grad).abs() <= 1e-12 * twiceA).all()


@pytest.mark.parametrize("regime", L.REGIMES)
@pytest.mark.parametrize("rows,cols", [(1, 4), (5, 264), (29, 776)])
def test_magnitudes_bound_the_reference_and_vanish_only_at_structural_zeros(rows, cols, regime):
    c = L.case(L.BF16, regime, rows, cols)
    G = c.graph_x(L.EPS)
    for dres in (False, True):
        for q in ("y", "mean", "rstd", "dz", "dgamma", "dbeta"):
            ref, A = G.ref(q, dres)
            assert (A >= ref.abs() * (1 - 1e-12)).all(), q
            zero = torch.zeros_like(A, dtype=torch.bool)
            if q == "dz" and regime == "special":
                zero[rows - 1] = c.dres[rows - 1] == 0 if dres else True
            assert torch.equal(A == 0, zero), q
            assert (ref[zero] == 0).all(), q
    keep = (torch.rand(rows, cols, generator=torch.Generator().manual_seed(6)) >= 0.1).to(torch.uint8)
    assert (keep == 0).any() or rows * cols < 16
    ref, A = L.z_reference(c, keep, 0.1)
    assert (A >= ref.abs()).all() and (A > 0).all()


# ================================================================================================ regimes, shapes, layouts
@pytest.mark.parametrize("fmt", FMTS)
def test_every_regime_holds_its_property_and_the_yardstick_is_exact_on_the_constant_row(fmt):
    """Building a case runs its generator's assertions.  The constant row: its float32 sum is exact (cols 2^-3 <= 2^8), so the
    yardstick's mean is the constant, d == 0, and y = 0 gamma + beta = beta, rounded once to the format."""
    for stream in ((False, True) if fmt != L.F32 else (False,)):
        for regime in (L.STREAM_REGIMES if stream else L.REGIMES):
            for cols in L.COLS:
                for rows in L.SMALL_ROWS + (29,):
                    c = L.LnCase(fmt, regime, rows, cols, stream)
                    assert c.x.shape == (rows, cols) and c.zfmt == (L.F32 if stream else fmt)
                    if regime == "offset":
                        assert abs(float(c.x.mean()) - (2048.0 if c.zfmt == L.F32 else 4.0)) < 1.0
                    if regime == "special":
                        G = L.Graph(c, c.x, L.EPS)
                        assert float(G.yard("mean")[0]) == L.CONST == float(G.ref("mean")[0][0])
                        assert torch.equal(G.yard("y")[0], L.stored(c.beta, fmt))
                        assert (G.yard("dz")[rows - 1] == 0).all() and (G.ref("dz")[1][rows - 1] == 0).all()
                        out = G.yard_outputs()
                        assert not L.judge("yardstick", G, out)[1]
                        # and the judge holds a kernel to both equalities
                        bent = dict(out, mean=out["mean"].clone())
                        bent["mean"][0] = torch.nextafter(bent["mean"][0], torch.tensor(1.0))
                        assert any("constant row" in b for b in L.judge("bent mean", G, bent)[1])
                        bent = dict(out, y=out["y"].clone())
                        bent["y"][0, 0] = L.stored(bent["y"][0, 0] * (1 + 4 * L.U[fmt]), fmt)       # the next value of the format
                        assert bent["y"][0, 0] != out["y"][0, 0]
                        assert any("stored(beta)" in b for b in L.judge("bent y", G, bent)[1])
    k = L.scale_k(13)
    assert sorted(k.tolist()) == list(range(-6, 7))


def test_every_case_names_the_form_the_selection_sends_it_to():
    cdiv = lambda a, b: -(-a // b)
    for (rows16, mis), table in L.INTENDED.items():
        assert set(table) == (set(L.MISALIGNED_COLS) if mis else set(L.COLS))
        for cols, (fwd, bwd) in table.items():
            lf, lb = L.ln_layout(False, rows16, cols, not mis), L.ln_layout(True, rows16, cols, not mis)
            assert lf[:2] == fwd and lf[2:] == (4, True, 0, 0), (rows16, mis, cols, lf)
            assert lb[:4] == bwd and lb[5] == L.BWD_CAP, (rows16, mis, cols, lb)
            assert lb[4] == (9 if not lb[3] else 8) * cols * 4 <= 64 * 1024
            for vec, chunks in (fwd, bwd[:2]):
                need = cdiv(cols // vec, 64)                       # accesses a lane makes to cover the row
                assert cols % vec == 0 and need <= chunks and chunks == {1: 1, 2: 2, 3: 3 if vec == 4 else 4, 4: 4}.get(need, 8)
                assert rows16 or vec == 4
            assert cols <= 2 * bwd[2] * 64                         # two columns per thread in the backward's workgroup reduction
    lanes = lambda cols, vec: (cols // vec - 1) % 64 + 1           # lanes in use in a row's last access
    assert lanes(4, 4) == 1 and lanes(8, 8) == 1 and lanes(8, 4) == 2 and lanes(264, 8) == 33 and lanes(196, 4) == 49
    assert lanes(264, 4) == 2 and lanes(776, 4) == 2 and lanes(776, 8) == 33 and lanes(1032, 4) == 2 and lanes(520, 8) == 1
    for cols in (512, 768, 1024, 2048):                            # the full side of each rung
        assert lanes(cols, 4) == 64 or cols == 768 and lanes(cols, 8) == 32
    # R_BIG: three trips of every backward form, the last ragged
    assert L.R_BIG == 8197 and L.trips(L.R_BIG, 16) == (3, 5) and L.trips(L.R_BIG, 12) == (3, 2053) and L.R_BIG == 2 * 3072 + 2053
    assert L.trips(5, 16) == (1, 5) and L.trips(4117, 16) == (2, 21)
    # once per backward instantiation, at the smallest column count that reaches it, and at the production width
    for rows16, big in ((True, L.BIG_16), (False, L.BIG_32)):
        reached = [L.intended(rows16, cols, mis)[1] for cols, mis in big if cols != 768]
        every = {v[1] for (r16, _), t in L.INTENDED.items() if r16 == rows16 for v in t.values()}
        assert len(set(reached)) == len(reached) and set(reached) == every
        for (cols, mis), form in zip(big, reached):
            smaller = [c for c in (L.MISALIGNED_COLS if mis else L.COLS) if c < cols and c > 8]    # 4 and 8: one lane, rows 1 and 5 only
            assert all(L.intended(rows16, c, mis)[1] != form for c in smaller), (cols, mis)
        assert (768, False) in big
    assert L.R_BIG * 1032 * 4 < 35e6 and L.R_BIG * 2048 < 2 ** 30
    # the development switch: what the file skips under
    assert L.ln_layout(True, True, 776, True, 1)[:4] == (4, 4, 16, True) and L.ln_layout(True, True, 768, True, 2)[:4] == (8, 2, 12, False)


def test_layout_query_equals_the_mirror_without_a_device():
    """ecamp_layernorm_layout is host arithmetic: both builds answer without a GPU, and refuse what the kernels refuse."""
    import ctypes
    import os
    from ecamp_amd import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        from ecamp_amd import build
        build.build(verbose=False, half="both")
    for fmt in ("bf16", "f16"):
        lib = _lib.load(fmt)
        out = (ctypes.c_int32 * 6)()
        po = ctypes.cast(out, ctypes.c_void_p)
        for backward in (0, 1):
            for rows16 in (0, 1):
                for al16 in (0, 1):
                    for opt in (0, 1, 2):
                        for cols in range(4, 2049, 4):
                            assert lib.ecamp_layernorm_layout(backward, rows16, cols, al16, opt, po) == 0
                            want = L.ln_layout(backward, rows16, cols, al16, opt)
                            assert tuple(out) == tuple(int(v) for v in want), (backward, rows16, cols, al16, opt, tuple(out), want)
        for cols in (0, -4, 6, 2052):
            assert lib.ecamp_layernorm_layout(1, 1, cols, 1, 0, po) < 0 and b"multiple of 4" in lib.ecamp_last_error()
        assert lib.ecamp_layernorm_layout(1, 1, 768, 1, 0, None) < 0 and b"null pointer" in lib.ecamp_last_error()


# ================================================================================================ the judge accepts the yardstick
def _accepts(c, eps=L.EPS):
    G = c.graph_x(eps)
    for dres, times in ((False, 1), (True, 1), (True, 2)):
        out = G.yard_outputs(dres, times)
        lines, bad = L.judge("yardstick", G, out, dres, times)
        assert not bad and len(lines) == 7, bad
        for q in ("dgamma", "dbeta"):                              # another evaluation, in other chaining orders
            ref, A = G.ref(q, dres, times)
            ky = L.k_of(G.yard(q, dres, times).double(), ref, A, L.U[L.F32], allowance=L.TINY[L.F32])
            k2 = L.k_of(G.yard(q, dres, times, seed=99).double(), ref, A, L.U[L.F32], allowance=L.TINY[L.F32])
            assert k2 <= L.bound_k(ky), (q, k2, ky)


@pytest.mark.parametrize("fmt", FMTS)
def test_judge_accepts_the_yardstick_at_every_small_case(fmt):
    for stream in ((False, True) if fmt != L.F32 else (False,)):
        for regime in (L.STREAM_REGIMES if stream else L.REGIMES):
            for cols in L.COLS:
                for rows in L.SMALL_ROWS:
                    _accepts(L.case(fmt, regime, rows, cols, stream))
    c = L.case(fmt, "plain", 5, 768)
    _accepts(c, L.EPS_BERT)
    keep = (torch.rand(5, 768, generator=torch.Generator().manual_seed(7)) >= L.DROP_P).to(torch.uint8)
    z = L.z_float32(c, keep, L.DROP_P)
    assert not L.judge_z("yardstick", c, z, keep, L.DROP_P)[1]
    G = L.Graph(c, z, L.EPS_BERT)
    out = G.yard_outputs(True, 1, keep, L.DROP_P)
    assert not L.judge("yardstick", G, out, True, 1, keep, L.DROP_P)[1]
    assert (out["dx_drop"][keep == 0] == 0).all() and (keep == 0).any()


# ================================================================================================ the judge rejects seeded faults
@functools.lru_cache(maxsize=1)
def big768():
    c = L.case(L.BF16, "plain", L.R_BIG, 768)
    return c, c.graph_x(L.EPS)


def rejected(name, G, out, quantities, must=None, **kw):
    lines, bad = L.judge(name, G, {q: out[q] for q in quantities}, **kw)
    print("  fault: %s" % name)
    for b in bad:
        print("    judge: " + b)
    assert bad, name + ": the judge let it pass"
    if must is not None:
        assert any((" %s:" % must) in b for b in bad), "%s: not caught through %s" % (name, must)


def test_judge_rejects_a_row_added_twice_or_left_out_at_8197_rows():
    """One row's share of a column is about 1 / sqrt(8197) of that column's sum: 14 000 and 9 000 times the bound here.  The older
    yardstick divides the largest error of any of the 768 columns (the row's largest |dy xh|, about 9, or |dy|, about 3.5) by the
    largest column sum (about 300): 3.0e-2 for the doubled row and 9.3e-3 to 1.1e-2 for the five rows of the last trip, as printed.
    So its 1e-2 still sees the doubled row at this row count and lets three of the five dropped rows pass; the ratio falls with the
    square root of the rows, and dgamma passes from about 70 000."""
    c, G = big768()
    out = G.yard_outputs()
    assert not L.judge("yardstick", G, out)[1]
    r = L.BWD_CAP * L.BWD_WAVES + 7                                    # a row of the middle trip
    twice = dict(out, dgamma=out["dgamma"] + G.y32["dgamma"][r])
    rejected("row %d added twice to dgamma, %d x 768 %s" % (r, c.rows, c.fmt), G, twice, ("dgamma",), must="dgamma")
    old_check("dgamma with a row added twice", twice["dgamma"], G.ref("dgamma")[0], OLD_GTOL[c.fmt])
    for r in range(2 * L.BWD_CAP * L.BWD_WAVES, c.rows):               # each of the five rows of the ragged last trip
        left = dict(out, dbeta=out["dbeta"] - G.y32["dbeta"][r])
        rejected("row %d left out of dbeta, %d x 768 %s" % (r, c.rows, c.fmt), G, left, ("dbeta",), must="dbeta")
        old_check("dbeta with row %d left out" % r, left["dbeta"], G.ref("dbeta")[0], OLD_GTOL[c.fmt])


def test_judge_rejects_a_stale_prefetch_and_a_residual_gradient_lost_on_the_ragged_trip():
    c, G = big768()
    stride = L.BWD_CAP * L.BWD_WAVES
    out = G.yard_outputs(dres=True)
    stale = dict(out, dz=out["dz"].clone())
    stale["dz"][c.rows - 1] = out["dz"][c.rows - 1 - stride]
    rejected("dz of the last row is the row one stride before it", G, stale, ("dz",), must="dz", dres=True)
    old_check("dz with a stale last row", stale["dz"], G.ref("dz", True)[0], OLD_TOL[c.fmt])
    lost = dict(out, dz=out["dz"].clone())
    lost["dz"][2 * stride:] = G.yard("dz")[2 * stride:]
    assert c.rows - 2 * stride == 5
    rejected("dres dropped on the ragged last trip only", G, lost, ("dz",), must="dz", dres=True)
    old_check("dz without dres on the last trip", lost["dz"], G.ref("dz", True)[0], OLD_TOL[c.fmt])


def test_stream_row_loop_faults_show_in_the_special_regime_and_not_in_offset():
    """Why the f32-stream backward runs its 8197 rows in `special`: at 2048 + N(0, 1) A carries |z| + mean|z| = 4096 twice where dz is
    of order one, and a 16-bit dz row may be anything.  The same three faults of the pipelined row loop at 8197 x 264, both regimes."""
    stride = L.BWD_CAP * L.BWD_WAVES
    for regime in ("special", "offset"):
        c = L.case(L.BF16, regime, L.R_BIG, 264, True)
        G = c.graph_x(L.EPS)
        out = G.yard_outputs(dres=True)
        assert not L.judge("yardstick", G, out, dres=True)[1]
        lost, stale, blank = (dict(out, dz=out["dz"].clone()) for _ in range(3))
        lost["dz"][2 * stride:] = G.yard("dz")[2 * stride:]
        stale["dz"][c.rows - 1] = out["dz"][c.rows - 1 - stride]
        blank["dz"][stride + 7] = 0.0
        for fault, got in (("dres dropped on the last trip", lost), ("stale last row", stale), ("a middle-trip row of zeros", blank)):
            if regime == "special":
                rejected("%s, stream %s 8197 x 264" % (fault, regime), G, got, ("dz",), must="dz", dres=True)
            else:
                print("  fault: %s, stream offset 8197 x 264: %s" % (fault, "rejected" if L.judge(fault, G, dict(dz=got["dz"]), dres=True)[1] else "ACCEPTED"))


def _forward32(c, eps, mean=None, var=None):
    """The yardstick's forward in float32 with a mean or a variance of the fault's own."""
    z, H = c.x, c.cols
    mu = z.sum(1, keepdim=True) / H if mean is None else mean(z)
    d = z - mu
    v = (d * d).sum(1, keepdim=True) / H if var is None else var(z, mu, d)
    rs = 1.0 / torch.sqrt(v + L.eps_given(eps))
    return dict(mean=mu[:, 0], rstd=rs[:, 0], y=L.stored(d * rs * c.gamma + c.beta, c.fmt))


@pytest.mark.parametrize("fmt", FMTS)
def test_judge_rejects_a_variance_divided_by_cols_minus_one(fmt):
    """At 2048 columns rstd is off by 2.4e-4 of itself: far below a 16-bit rounding of y, 4000 roundings of an f32 statistic."""
    c = L.case(fmt, "plain", 5, 2048)
    G = c.graph_x(L.EPS)
    assert _forward32(c, L.EPS)["y"].equal(G.yard("y"))
    out = _forward32(c, L.EPS, var=lambda z, mu, d: (d * d).sum(1, keepdim=True) / (c.cols - 1))
    rejected("variance / (cols - 1), 5 x 2048 %s" % fmt, G, out, ("y", "mean", "rstd"), must="rstd")
    y_alone = L.judge("y alone", G, dict(y=out["y"]))[1]
    print("    the per-element bound on y alone: %s" % ("rejects it" if y_alone else "cannot show it"))
    passes = old_check("y with variance / (cols - 1)", out["y"], G.ref("y")[0], OLD_TOL[fmt])
    print("    old check: rstd is not compared with anything")
    assert passes or fmt == L.F32


@pytest.mark.parametrize("stream", [False, True])
def test_judge_rejects_a_one_pass_variance_in_the_offset_regime(stream):
    """E[z^2] - mu^2 in float32 on rows at 2048 + N(0, 1): z^2 is 4e6 with a spacing of 0.25 to 0.5, the variance is 1."""
    fmt = L.BF16 if stream else L.F32
    c = L.case(fmt, "offset", 5, 768, stream)
    G = c.graph_x(L.EPS)
    out = _forward32(c, L.EPS, var=lambda z, mu, d: ((z * z).sum(1, keepdim=True) / c.cols - mu * mu).clamp_min(0))
    rejected("one-pass variance, offset 5 x 768 %s%s" % (fmt, " stream" if stream else ""), G, out, ("y", "mean", "rstd"), must="rstd")
    old_check("y with a one-pass variance", out["y"], G.ref("y")[0], OLD_TOL[fmt])


@pytest.mark.parametrize("fmt", FMTS)
def test_judge_rejects_a_chunk_left_out_of_the_mean(fmt):
    c = L.case(fmt, "plain", 5, 196)
    G = c.graph_x(L.EPS)
    out = _forward32(c, L.EPS, mean=lambda z: z[:, :192].sum(1, keepdim=True) / c.cols)
    rejected("the last chunk of a 196-column row left out of the mean, %s" % fmt, G, out, ("y", "mean", "rstd"), must="mean")
    old_check("mean without the last chunk", out["mean"], G.ref("mean")[0], OLD_MEAN)
    old_check("y with that mean", out["y"], G.ref("y")[0], OLD_TOL[fmt])


@pytest.mark.parametrize("fmt,percent", [(L.F32, 1), (L.F16, 1), (L.BF16, 2)])
def test_judge_rejects_one_percent_on_a_small_row(fmt, percent):
    """scales: row 13 carries 2^-6, its neighbours 2^-1 and 2^4, the largest rows 2^6.  One percent of it is 2^-12 of one percent of
    the tensor's maximum.  bfloat16 is where the method ends: one percent is five of its roundings of |dz| and A is three to ten times
    |dz|, so the fault sits at the format's own noise (in IEEE half it is forty roundings).  The limit is recorded, not only described:
    in bfloat16 one percent is accepted (5.1 against a bound of 5.5) and two percent are rejected (8.9)."""
    c = L.case(fmt, "scales", 29, 768)
    G = c.graph_x(L.EPS)
    assert int(L.scale_k(29)[13]) == -6 and int(L.scale_k(29).max()) == 6
    out = G.yard_outputs(dres=True)
    assert not L.judge("yardstick", G, out, dres=True)[1]

    def bent(pc):
        off = dict(out, dz=out["dz"].clone())
        off["dz"][13] = L.stored(out["dz"][13] * (1 + pc / 100), fmt)
        return off
    rejected("dz of the 2^-6 row 13 off by %d %%, scales 29 x 768 %s" % (percent, fmt), G, bent(percent), ("dz",), must="dz", dres=True)
    assert old_check("dz with %d %% on a 2^-6 row" % percent, bent(percent)["dz"], G.ref("dz", True)[0], OLD_TOL[fmt])
    if fmt == L.BF16:
        lines, bad = L.judge("1 %% in %s" % fmt, G, dict(dz=bent(1)["dz"]), dres=True)
        print(lines[0])
        assert not bad, "bfloat16 now rejects 1 %: move the recorded limit"


@pytest.mark.parametrize("fmt", FMTS)
def test_judge_rejects_prior_contents_overwritten(fmt):
    c = L.case(fmt, "special", 5, 768)
    G = c.graph_x(L.EPS)
    out = G.yard_outputs()
    fresh = dict(out, dgamma=out["dgamma"] - c.prior_g)
    rejected("dgamma stored over its prior contents, 5 x 768 %s" % fmt, G, fresh, ("dgamma",), must="dgamma")
    old_check("dgamma without its prior contents", fresh["dgamma"], G.ref("dgamma")[0], OLD_GTOL[fmt])
