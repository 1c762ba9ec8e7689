"""What tests/_gemm_ref.py can prove without a GPU, before any kernel is judged by it (tests/test_gemm_float64_gpu.py):

  * the EPS figures of its docstring are what float32 restatements of gelu_fast_f, gelu_both_fast_f and gelu_grad_fast_f give over
    every finite input of each 16-bit format, and gelu_fast_f's is the 7.0e-7 csrc/common.h claims;
  * one rounding of a 16-bit format is 2 U: the float64 reference rounded once misses the bound written with U and meets it with R;
  * for every shape, form, epilogue and regime of the GPU tables the yardstick meets the bound with the bare K_yard, and Kacc >= 1;
  * the restated kernel selection (route, suggest_split, tag_of) gives, for 256 CUs, the (family, tile width) written down by hand
    for every GPU case -- and every shape of test_gemm_q16_forward_and_data_gradient_ragged takes the 192-column tile;
  * seven wrong kernels, each built from the float64 reference and rounded as the kernels round, are all rejected by the judge, and
    check() of tests/test_kernels_gpu.py at its TOL accepts at least the three the issue names: the gap this file closes."""
import pytest
import torch

import _gemm_ref as G
from _gemm_ref import BF16, F16, F32, R, TINY, U, U32, Case, Slab, stored

HALVES = (BF16, F16)


# ---------------------------------------------------------------------------------------------------------------- EPS
@pytest.mark.parametrize("fmt", HALVES)
def test_eps_of_the_fast_gelu_forms(fmt):
    v = G.all_finite(fmt)
    assert v.numel() == {BF16: 65280, F16: 63488}[fmt]
    y, (y2, g), gg = G.gelu_fast32(v), G.gelu_both_fast32(v), G.gelu_grad_fast32(v)
    assert torch.equal(y, y2), "gelu_both_fast_f's y is gelu_fast_f's bit for bit"
    assert torch.isfinite(y).all() and torch.isfinite(g).all() and torch.isfinite(gg).all()
    got = {"gelu": float((y.double() - G.gelu64(v)).abs().max()), "both": float((g.double() - G.dgelu64(v)).abs().max()),
           "grad": float((gg.double() - G.dgelu64(v)).abs().max())}
    for which, m in got.items():
        print("  %s %-4s max |error| %.4e (docstring %.3e, allowance %.3e)" % (fmt, which, m, G.EPS_MEASURED[(fmt, which)], G.eps_of(fmt, which)))
        assert abs(m - G.EPS_MEASURED[(fmt, which)]) <= 5e-4 * m, (fmt, which, m)
        assert G.eps_of(fmt, which) == 2.0 * G.EPS_MEASURED[(fmt, which)]
    assert 6.95e-7 <= got["gelu"] < 7.05e-7, "csrc/common.h: max |error| 7.0e-7 over all finite inputs"


def test_float64_gelu_and_its_derivative():
    x = torch.linspace(-9, 9, 3601, dtype=torch.float64).requires_grad_(True)
    y = torch.nn.functional.gelu(x)
    y.sum().backward()
    assert float((G.gelu64(x.detach()) - y.detach()).abs().max()) < 1e-15
    assert float((G.dgelu64(x.detach()) - x.grad).abs().max()) < 1e-15
    assert 1.128 < float(G.dgelu64(x.detach()).abs().max()) < G.GELU_SLOPE


# ---------------------------------------------------------------------------------------------------------------- the rounding term
@pytest.mark.parametrize("fmt", HALVES)
def test_one_rounding_is_two_U(fmt):
    c = Case(fmt, "f", G.BASE_M, G.BASE_N, 136, "scales", "bias")
    got = stored(c.ref.float(), fmt).double()
    err = (got - c.ref).abs()
    assert bool((err > U[fmt] * c.ref.abs() + TINY[fmt]).any()), "the correctly rounded reference misses the bound written with U"
    assert bool((err <= R[fmt] * c.ref.abs() + TINY[fmt]).all()), "and meets it with one rounding, R = 2 U"
    worst, bad = G.judge(c, c.ideal(), kacc=0.0)
    assert not bad and worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("fmt", (BF16, F16, F32))
def test_yardstick_meets_the_bound_with_its_bare_k_yard(fmt):
    n, ky = 0, {}
    for kw in G.all_cases(fmt):
        c = Case(fmt, **kw)
        assert c.kacc >= 1.0 and c.kacc == max(1.0, 4.0 * c.k_yard)
        up = 1.0 + 2.0 ** -40                  # (the float64 roundings of forming err / (U32 A) and K U32 A at the element that defines K_yard)
        worst, bad = G.judge(c, c.yardstick(), kacc=c.k_yard * up, rs_kacc=c.rs_k_yard * up if c.rowsum else None, step=c.step)
        assert not bad, bad
        worst_i, bad_i = G.judge(c, c.ideal())
        assert not bad_i and worst_i <= 1.0, bad_i
        ky.setdefault((c.form, c.K), []).append(c.k_yard)
        n += 1
    for key, v in sorted(ky.items()):
        print("  %s %s K %4d: K_yard %.2f .. %.2f over %d cases" % (fmt, key[0], key[1], min(v), max(v), len(v)))
    assert n == sum(1 for _ in G.all_cases(fmt))


# ---------------------------------------------------------------------------------------------------------------- the selection mirror
def test_mirror_gives_the_intended_kernel_of_every_gpu_case():
    for fmt in HALVES:
        for force in ("t128", "q8", "q16"):
            for K in G.BASE_KS:
                for epi in G.FWD_EPIS:
                    assert G.route("f", G.BASE_M, G.BASE_N, K, fmt, epi, force=force) == G.INTENDED["f"][force][epi], (force, K, epi)
                for epi in G.DGRAD_EPIS:
                    assert G.route("d", G.BASE_M, G.BASE_N, K, fmt, epi, force=force) == G.INTENDED["d"][force][epi], (force, K, epi)
            for epi in G.FWD_EPIS:
                assert G.route("f", *G.ODD, fmt, epi, force=force) == G.INTENDED["odd"]
            for (K, split), want in G.INTENDED["w"][force].items():
                for rs in (False, True):
                    assert G.route("w", G.BASE_M, G.BASE_N, K, fmt, "wgrad", split=split, rowsum=rs, force=force) == want, (force, K, split)
            # the dense variant (leading dimension == width) changes nothing at these widths
            assert G.route("f", G.BASE_M, G.BASE_N, 128, fmt, "bias", force=force, pad=0) == G.INTENDED["f"][force]["bias"]
        for force in ("q8", "q16"):
            assert G.route("f", *G.WALK, fmt, "bias", force=force) == G.INTENDED["walk"][force]
        for form, epi in G.WIDE_CASES:
            assert G.route(form, *G.WIDE, fmt, epi, force="q16") == G.INTENDED["wide"]
    for form, (M, N, K), epi in G.F32_CASES:
        for force in ("t128", "q8", "q16"):
            assert G.route(form, M, N, K, F32, epi, force=force) == G.INTENDED["f32"]
    for K, want in G.SUGGESTED_SPLIT.items():
        for q8_mode in (-1, 0, 2):
            assert G.suggest_split(G.BASE_M, G.BASE_N, K, "w", BF16, q8_mode) == want
        assert G.suggest_split(G.BASE_M, G.BASE_N, K, "w", F32) == want
    assert G.SUGGESTED_SPLIT[4104] > 1
    # the suggested split's last slice holds 8 of the 4104 rows: the persistent kernels refuse it, WGRAD_EXTRA_SPLIT is legal
    assert G.eff_split(4104, 17, BF16) == (256, 17) and G.eff_split(4104, G.WGRAD_EXTRA_SPLIT, BF16) == (576, 8)
    assert not G.q8_legal("w", G.BASE_M, G.BASE_N, 4104, BF16, "wgrad", 17) and G.q8_legal("w", G.BASE_M, G.BASE_N, 4104, BF16, "wgrad", 8)


def test_tile_walks_and_the_256_column_tile_on_256_cus():
    cd = G.cdiv
    assert cd(G.WALK[0], 256) * cd(G.WALK[1], 256) == 258 and cd(G.WALK[0], 256) * cd(G.WALK[1], 192) == 258
    assert cd(G.WIDE[0], 256) * cd(G.WIDE[1], 256) == 129 and cd(G.WIDE[0], 256) * cd(G.WIDE[1], 192) == 258
    # no smaller output reaches the 256-column form: it needs tiles256 <= CUs < tiles192
    for N in range(8, 1100, 8):
        for m in range(1, 300):
            M = (m - 1) * 256 + 8
            if G.route("f", M, N, 136, BF16, "plain", force="q16") == ("q16", 256):
                assert M * N >= G.WIDE[0] * G.WIDE[1], (M, N)
                break
    # every shape of test_gemm_q16_forward_and_data_gradient_ragged and of the two bit-identity tests takes the 192-column tile
    for M, N, K in [(394, 768, 192), (1000, 520, 200), (512, 1536, 136), (300, 2304, 768), (2048, 192, 1088), (777 * 8, 768, 264)]:
        assert G.route("f", M, N, K, BF16, "bias", force="q16", pad=0) == ("q16", 192)
        assert G.route("d", M, K, N, BF16, "plain", force="q16", pad=0) == ("q16", 192)
    for M, N, K in [(12800, 768, 3072), (1000, 520, 264), (32768, 768, 1536)]:
        assert G.route("d", M, N, K, BF16, "plain", force="q16", pad=0) == ("q16", 192)
    # the default selection: the 768-wide outputs on the four-wave kernel, the others on the eight-wave one
    for M, N, K, want in ((12800, 768, 3072, ("q16", 192)), (32768, 768, 768, ("q16", 192)), (12800, 3072, 768, ("q8", 256)), (32768, 1536, 768, ("q8", 256))):
        assert G.route("f", M, N, K, BF16, "plain", pad=0) == want
    assert G.tag_of("q16", 256, "f", *G.WIDE, BF16, "res32") == "q16:f:e5:32776:200:136:w256"
    assert G.tag_of("t128", 128, "w", 264, 264, 4104, BF16, "wgrad", 17) == "t128:w:e-:264:264:4104:s17"
    assert G.tag_of("q16", 256, "w", 264, 264, 4104, BF16, "wgrad", 8) == "q16:w:e4:264:264:4104:s8"


# ---------------------------------------------------------------------------------------------------------------- mutants
def _max_norm_accepts(got, ref, fmt):
    """check() of tests/test_kernels_gpu.py at its TOL."""
    from test_kernels_gpu import TOL, check
    try:
        check("mutant", got, ref, TOL[G.DTYPE[fmt]])
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("fmt", HALVES)
def test_mutants_are_rejected_and_the_max_norm_check_accepts_three(fmt):
    M, N, K = G.BASE_M, G.BASE_N, 136
    plain, bias, gelu = (Case(fmt, "f", M, N, K, "scales", e) for e in ("plain", "bias", "bias_gelu_pre"))
    o = plain.o
    a64, b64 = o.a.double(), o.b.double()
    k = G.scale_k(M)
    accepted = {}

    def rejected(name, c, got, ref_for_check):
        for q in got:
            assert torch.equal(stored(got[q].float(), c.fmt), got[q].float()) or not torch.isfinite(got[q]).all()
        worst, bad = G.judge(c, got)
        assert bad, "%s passes the judge (worst err / bound %.3f)" % (name, worst)
        accepted[name] = _max_norm_accepts(got["C"], ref_for_check, fmt)
        print("  %s %-34s judge: err / bound %10.3g   max-norm check at TOL: %s" % (fmt, name, worst, "ACCEPTS" if accepted[name] else "rejects"))

    for c in (plain, bias, gelu):                  # what every mutant is derived from passes
        assert not G.judge(c, c.ideal())[1]

    # 1: the last 8-wide K chunk dropped in one 2^-6 row
    row = int((k == -6).nonzero()[-1])
    acc = o.acc.clone()
    acc[row] = a64[row, :K - 8] @ b64[:, :K - 8].T
    rejected("K tail dropped in a 2^-6 row", plain, {"C": stored(acc.float(), fmt)}, plain.ref)
    # 2: acc rounded to 16 bits before the bias is added
    rejected("acc rounded before the bias", bias, {"C": stored(stored(o.acc.float(), fmt) + o.bias, fmt)}, bias.ref)
    # 3: the bias shifted by 4 columns in the last column group only
    b3 = o.bias.clone()
    b3[N - 4:] = o.bias[N - 8:N - 4]
    rejected("bias shifted in the last group", bias, {"C": stored((o.acc + b3.double()).float(), fmt)}, bias.ref)
    # 4: GELU of the unrounded pre-activation while pre_out is given
    pre = stored(gelu.ref.float(), fmt)
    rejected("GELU of the unrounded pre", gelu, {"C": stored(G.gelu64(gelu.ref).float(), fmt), "pre": pre, "pre1": pre}, G.gelu64(pre))
    # 5: GELU with an absolute error of 1e-4 for x < -3
    assert int((pre < -3).sum()) > 100
    y5 = G.gelu64(pre) + 1e-4 * (pre < -3)
    rejected("GELU off by 1e-4 below -3", gelu, {"C": stored(y5.float(), fmt), "pre": pre, "pre1": pre}, G.gelu64(pre))
    # 7: one NaN pad element let into one sum
    c7 = stored(bias.ref.float(), fmt)
    c7[row, N - 1] = float("nan")
    worst, bad = G.judge(bias, {"C": c7})
    assert bad and worst == float("inf")
    print("  %s %-34s judge: err / bound %10.3g" % (fmt, "a NaN pad element in one sum", worst))

    # 6: one pad word of C overwritten (and: a logical word never written, a guard row written)
    slab = Slab(M, N, G.DTYPE[fmt])
    clean = slab.output()
    slab.logical(clean).copy_(stored(bias.ref.float(), fmt).to(G.DTYPE[fmt]))
    bad = []
    slab.check("C", clean, bad)
    assert not bad
    for r, col in ((G.GUARD + row, N), (G.GUARD + M - 1, N + G.PAD - 1), (G.GUARD - 1, 3), (G.GUARD + M, 0)):
        buf, bad = clean.clone(), []
        buf[r, col] = 1.0
        slab.check("C", buf, bad)
        assert len(bad) == 1 and "pad / guard" in bad[0], (r, col, bad)
    buf, bad = clean.clone(), []
    slab.logical(buf)[5, 8:12] = slab.poison()[0, :4]
    slab.check("C", buf, bad)
    assert len(bad) == 1 and "never written" in bad[0]
    print("  %s %-34s layout check: rejected" % (fmt, "a pad word of C overwritten"))

    # the gap: the per-tensor max-norm check lets these through
    for name in ("K tail dropped in a 2^-6 row", "acc rounded before the bias", "GELU off by 1e-4 below -3"):
        assert accepted[name], name


def test_slab_layout():
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        s = Slab(5, 12, dtype)
        t = torch.arange(60, dtype=torch.float32).reshape(5, 12).to(dtype)
        buf = s.input(t)
        assert buf.shape == (5 + 2 * G.GUARD, 12 + G.PAD) and s.ld == 20 and s.offset() == G.GUARD * 20
        assert torch.equal(s.logical(buf), t) and int(torch.isnan(buf).sum()) == buf.numel() - 60
        assert torch.equal(buf.reshape(-1)[s.offset():s.offset() + 12], t[0])
        out = s.output()
        assert bool((out.contiguous().view(torch.int32) == G.PATTERN).all())
        out = s.output(prior=t)
        assert torch.equal(s.logical(out), t)
    v = Slab(1, 264, torch.float32, guard=0)
    assert v.input(torch.zeros(264)).shape == (1, 272) and v.offset() == 0
    d = Slab(5, 16, torch.bfloat16, pad=0)
    assert d.ld == 16
