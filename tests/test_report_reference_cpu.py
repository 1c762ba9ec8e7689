"""No GPU: the references of tests/_report_ref.py are what they claim to be -- torch.autograd in float64 on the same cases -- and the
conditions tests/test_report_kernels_gpu.py relies on hold: every cross-entropy case reaches the kernel it is listed under and carries
the rows the old metric could not see, every embedding shape reaches the launch geometry it is listed under, the float32 chain rounds
after every addition, and the judges refuse an output that is subtly wrong."""
import pytest
import torch
import torch.nn.functional as F

import _report_ref as R


def close(name, got, ref, rel=1e-12):
    d = float((got - ref).abs().max())
    assert d <= rel * max(1.0, float(ref.abs().max())), "%s: %.3e apart" % (name, d)


# ================================================================================================ weighted cross-entropy
@pytest.mark.parametrize("gain", [1.0, 256.0 * R.CE_M])
@pytest.mark.parametrize("V,fmt", [(4, R.F32), (8, R.BF16), (1020, R.F32), (4104, R.F16), (30000, R.BF16)])
def test_cross_entropy_reference_is_autograd(V, fmt, gain):
    """gain * mean over ALL M rows of F.cross_entropy(reduction="none") * w, ignored rows counted in the denominator."""
    x, labels, w = R.ce_case(V, fmt)
    ref, A, zero = R.ce_reference(x, labels, w, gain)
    xr = x.double().requires_grad_(True)
    lab = torch.where((labels >= 0) & (labels < V), labels, torch.full_like(labels, -100))
    ce = F.cross_entropy(xr, lab, reduction="none") * w.double()
    (gain * ce.sum() / R.CE_M).backward()
    close("grad", ref["grad"], xr.grad)
    close("loss", ref["loss"], ce.sum().detach())
    assert (ref["grad"][zero] == 0).all() and (A["grad"][zero] == 0).all() and (A["grad"][~zero] > 0).all()
    assert (A["grad"] >= ref["grad"].abs()).all() and float(A["loss"]) >= float(ref["loss"]) > 0
    assert zero.tolist() == [i in (0, 1, 7, 9, 15, 20, 21, 27, 33) for i in range(R.CE_M)]


@pytest.mark.parametrize("fmt", [R.F32, R.BF16, R.F16])
def test_cross_entropy_cases_carry_their_rows(fmt):
    for V in sorted(set(R.V_REG + R.V_GENERIC + R.V_F32)):
        x, labels, w = R.ce_case(V, fmt)
        assert x.shape == (R.CE_M, V) and torch.equal(R.stored(x, fmt), x) and torch.isfinite(x).all()
        assert labels[:4].tolist() == [-100, V, 0, V - 1] and int(labels[5]) == V - 2 and float(w[7]) == 0 == float(w[20])
        others = x[4].clone()
        others[labels[4]] = -1e9
        assert 30 <= float(x[4, labels[4]] - others.max()) < 31
        lead = int(x[6].argmax())
        others = x[6].clone()
        others[lead] = -1e9
        assert lead != int(labels[6]) and 30 <= float(x[6, lead] - others.max()) < 31
        assert float(x[8].min()) == float(x[8].max()) and float((x[10] - R.CE_OFFSET).abs().max()) < 20
        # the property max|err| / max|ref| could not see: the judge asserts it again on every case it is given
        ref, A, zero = R.ce_reference(x, labels, w)
        assert float((ref["grad"][6].abs() < 2.0 ** -10 * ref["grad"][6, labels[6]].abs()).float().mean()) > 0.4


def test_cross_entropy_cases_reach_every_dispatch_branch():
    reached = {R.ce_kernel_of(V, R.BF16) for V in R.V_REG}
    assert reached == {"row<1,512>", "row<2,512>", "row<4,512>", "row<4,1024>"}
    assert [R.ce_kernel_of(V, R.BF16) for V in R.V_REG] == ["row<1,512>"] * 2 + ["row<2,512>"] * 2 + ["row<4,512>"] * 2 + ["row<4,1024>"] * 3
    assert {R.ce_kernel_of(V, R.F16) for V in R.V_GENERIC} == {"generic<16>"}
    assert {R.ce_kernel_of(V, R.F32) for V in R.V_F32} == {"generic<f32>"}
    assert R.ce_kernel_of(4096, R.BF16, ld=4104) == "row<1,512>" and R.ce_kernel_of(4096, R.BF16, ld=4100) == "generic<16>"
    assert R.ce_kernel_of(30000, R.BF16, ld=30004) == "generic<16>" and R.ce_kernel_of(4096, R.BF16, aligned=False) == "generic<16>"


def test_float32_chain_rounds_after_every_addition():
    got = R.chain32(torch.tensor([2.0 ** 24, 1.0, 1.0]))
    assert got.shape == (R.LOSS_ORDERS,) and float(got[0]) == 2.0 ** 24            # order 0: the terms as they stand
    assert set(got.tolist()) == {2.0 ** 24, 2.0 ** 24 + 2}                         # 1 + 1 first is exact
    assert float(R.chain32(torch.tensor([1.0, 1.0, 2.0 ** 24]))[0]) == 2.0 ** 24 + 2


@pytest.mark.parametrize("fmt", [R.F32, R.BF16, R.F16])
def test_cross_entropy_judge_bites(fmt):
    """The yardstick's own output passes; a softmax part that is half of what it should be, a label column off by one, a non-zero in
    a row without a weight and a loss short of one row's share are all refused."""
    V = 4104
    x, labels, w = R.ce_case(V, fmt)
    ref, A, zero = R.ce_reference(x, labels, w)
    good = ref["grad"].to(R.DTYPE[fmt])
    lines, bad = R.ce_judge("yardstick", fmt, x, labels, w, 1.0, good, float(ref["loss"]))
    assert not bad and len(lines) == 2
    onehot = (A["grad"] - ref["grad"]) / 2
    half = (ref["grad"] + onehot) / 2 - onehot
    assert R.ce_judge("half", fmt, x, labels, w, 1.0, half.to(R.DTYPE[fmt]), float(ref["loss"]))[1]
    moved = ref["grad"] + onehot - onehot.roll(1, 1)
    assert R.ce_judge("moved", fmt, x, labels, w, 1.0, moved.to(R.DTYPE[fmt]), float(ref["loss"]))[1]
    dirty = good.clone()
    dirty[7, 5] = 2.0 ** -20
    assert R.ce_judge("dirty", fmt, x, labels, w, 1.0, dirty, float(ref["loss"]))[1]
    assert R.ce_judge("loss", fmt, x, labels, w, 1.0, good, float(ref["loss"]) * (1 - 1e-4))[1]


# ================================================================================================ BertEmbeddings
def _autograd(c, keep):
    """BertEmbeddings by autograd in float64: F.embedding (padding_idx for the word table) + F.layer_norm + the keep-mask."""
    word, pos, typ, gamma, beta = [t.double().clone().requires_grad_(True) for t in (c.word, c.pos, c.typ, c.gamma, c.beta)]
    z = F.embedding(c.ids, word, padding_idx=c.pad_id) + F.embedding(c.ty, typ) + pos[None]
    e = F.layer_norm(z, (c.H,), gamma, beta, R.EMB_EPS)
    if keep is not None:
        e = e * keep.double().view(c.B, c.S, c.H) / (1 - c.p)
    e.backward(c.de.double().view(c.B, c.S, c.H))
    return z.detach().reshape(-1, c.H), e.detach().reshape(-1, c.H), dict(gword=word.grad, gpos=pos.grad, gtype=typ.grad, dgamma=gamma.grad, dbeta=beta.grad)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("variant", R.EMB_VARIANTS)
@pytest.mark.parametrize("shape", ["6x5x768", "70x3x260", "5x3x4"])
def test_embedding_reference_is_autograd(shape, variant, p):
    c = R.emb_case(shape, R.F32, variant, p)
    keep = (torch.rand(c.B * c.S, c.H, generator=torch.Generator().manual_seed(5)) >= p).to(torch.uint8) if p else None
    z, e, grads = _autograd(c, keep)
    zr, zA = c.z_reference()
    close("z", zr, z)
    assert (zA >= zr.abs()).all()
    ref, A = c.reference(z, keep)                      # the stored z = the exact one: the whole graph is autograd's
    close("e", ref["e"], e)
    close("mean", ref["mean"], z.mean(1))
    close("rstd", ref["rstd"], 1 / torch.sqrt(z.var(1, unbiased=False) + R.EMB_EPS))
    for q, g in grads.items():
        close(q, ref[q], c.prior[q].double() + g)
    for q in ref:
        assert (A[q] >= ref[q].abs() * (1 - 1e-12)).all(), q
    # structurally unchanged: the PAD row, unused words, an unused token type -- and nothing else
    un = c.untouched()
    for q, g in grads.items():
        assert torch.equal(ref[q][un[q]], c.prior[q].double()[un[q]]), q
        assert (g[un[q]] == 0).all(), q
    assert un["gword"][c.pad_id].all() and not un["gword"][7].any() and not un["gpos"].any() and not un["dgamma"].any()
    assert un["gword"][2].all() == (variant == "nohot") and un["gtype"][1].all() == (variant == "type0") and not un["gtype"][0].any()


def test_embedding_shapes_reach_their_launch_geometry():
    it = lambda cols: -(-(cols // 4) // 64)
    geo = {s: (R.emb_fwd_grid_y(B), R.emb_bwd_grid_y(B), it(H), (H // 4) % 64, B % 4) for s, (B, S, H) in R.EMB_SHAPES.items()}
    assert geo["6x5x768"] == (2, 1, 3, 0, 2)
    assert geo["70x3x260"] == (16, 2, 2, 1, 2) and 70 > 64          # a second trip of the forward's batch loop, one lane in the last trip
    assert geo["260x2x64"] == (16, 8, 1, 16, 0) and 260 // 32 >= 8 and -(-260 // 32) == 9
    assert geo["9x4x1024"] == (3, 1, 4, 0, 1)
    assert geo["5x3x4"] == (2, 1, 1, 1, 1)
    assert geo["33x2x512"] == (9, 1, 2, 0, 1)
    assert {g[2] for g in geo.values()} == {1, 2, 3, 4}
    assert R.emb_case("70x3x260", R.F32).chained()[-1] == "gpos" and "gpos" not in R.emb_case("6x5x768", R.F32).chained()


@pytest.mark.parametrize("fmt", [R.F32, R.BF16])
def test_embedding_judge_bites(fmt):
    """The yardstick's own output passes; a position-table row that lost half its batch (a plain store where an atomic belongs), a
    touched PAD row and a dropped prior are refused."""
    c = R.emb_case("70x3x260", fmt)
    z = c.z_float32()
    y = c.float32(z, None)
    got = {q: (v[0] if v.dim() > c.prior[q].dim() else v).clone() for q, v in y.items() if q in c.prior}
    got.update(z=z.to(R.DTYPE[fmt]), e=y["e"].to(R.DTYPE[fmt]), mean=y["mean"], rstd=y["rstd"])
    quantities = ("z", "mean", "rstd", "e", "gword", "gpos", "gtype", "dgamma", "dbeta")
    lines, bad = R.emb_judge("yardstick", c, got, z, None, quantities)
    assert not bad and len(lines) == len(quantities)
    r = c.rows(z, None, torch.float32)
    lost = dict(got, gpos=c.prior["gpos"] + r["dz"].view(c.B, c.S, c.H)[4:8].sum(0))
    assert R.emb_judge("lost", c, lost, z, None, ("gpos",))[1]
    pad = dict(got, gword=got["gword"].clone())
    pad["gword"][c.pad_id, 3] = torch.nextafter(pad["gword"][c.pad_id, 3], torch.tensor(9.0))     # one bit
    assert R.emb_judge("pad", c, pad, z, None, ("gword",))[1]
    fresh = dict(got, dbeta=got["dbeta"] - c.prior["dbeta"])
    assert R.emb_judge("fresh", c, fresh, z, None, ("dbeta",))[1]


# ================================================================================================ the argument checks need no device
def test_ce_fwd_bwd_refuses_bad_arguments_on_both_builds():
    """ecamp_ce_fwd_bwd checks what ecamp_ce_eval checks, before any launch: both builds answer without a GPU."""
    import ctypes
    import os
    from ecamp_amd import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        from ecamp_amd import build
        build.build(verbose=False, half="both")
    one = ctypes.c_void_p(16)
    for fmt in ("bf16", "f16"):
        lib = _lib.load(fmt)
        call = lambda M, V, ld, code, loss=one: lib.ecamp_ce_fwd_bwd(one, one, one, loss, M, V, ld, 1.0, code, None)
        for args, msg in (((4, 6, 8, 1), b"multiples of 4"), ((4, 8, 10, 1), b"multiples of 4"), ((4, 8, 4, 1), b"ld >= V > 0"),
                          ((4, 0, 8, 1), b"ld >= V > 0"), ((4, -8, 8, 0), b"ld >= V > 0"), ((-1, 8, 8, 1), b"do not fit one launch"),
                          ((2 ** 31, 8, 8, 0), b"do not fit one launch"), ((4, 8, 8, 2), b"dtype 2"), ((4, 8, 8, 1, None), b"null pointer")):
            assert call(*args) < 0 and msg in lib.ecamp_last_error(), (fmt, args, lib.ecamp_last_error())
        assert call(0, 8, 8, 1) == 0 and call(0, 8, 12, 0) == 0          # no rows: 0 without a launch
