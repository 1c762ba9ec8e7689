"""No GPU: what tests/_attn_ref.py claims, proved on the host (read its docstring first).

  * the float32 yardstick meets the bound with its bare K_yard and the correctly rounded float64 result meets it with K = 1, in every GPU
    case and regime, in f32 and both 16-bit formats (the backward is handed the yardstick's own O and lse);
  * select() equals the table written by hand in GPU_CASES / F32_CASES, including the LDS edges;
  * eight mutants of the reference's own outputs, each a plausible kernel fault, are rejected at the case named for them with the K
    the GPU test would use there.

What check() of tests/test_kernels_gpu.py (max|got - ref| / max|ref| at 2e-2 bfloat16, 3e-3 half, 2e-5 f32, doubled for gradients) says
to the same mutants, measured here (test_old_check_accepts_what_the_bound_rejects prints the figures; A = accepted, R = rejected, the
figure is the largest of the pass's tensors; the bound rejects every line but the two marked *):
      mutant     case                          bfloat16      half          f32
      rowsum     (1,2,70,300,128) masked       A 1.10e-02    R 1.00e-02    R 9.90e-03
      inv_keep   (2,2,128,49,128) p .1         R 8.73e-02    R 8.54e-02    R 8.52e-02
      row        (2,3,50,50,32)                R 5.33e-01    R 5.32e-01    R 5.32e-01
      scale      (3,2,33,17,32) masked p .3    A 2.61e-03    A 1.39e-03    R 1.29e-03
      lse        (2,2,197,197,64)              R 6.36e-02    R 6.42e-02    R 6.42e-02    (bfloat16: dK alone is accepted, 3.83e-02)
      delta      (2,2,50,50,64)                A 4.28e-03 *  A 6.44e-04 *  R 8.93e-04
      dv_leak    (3,2,100,100,64) masked       A 2.81e-03    A 3.24e-04    A 4.69e-06
      dk_scale   (3,2,48,48,64) masked         R 2.14e+00    R 2.14e+00    R 2.14e+00
  Forward: the old check accepts `rowsum` in bfloat16 and `scale` in both 16-bit formats; the bound rejects them -- asserted below.
  `scale` (2^-9) is below one bfloat16 rounding of O (err / bound of O: 0.30 in bfloat16, 1.5 in half); it is lse, an f32 output judged
  in f32 units, that rejects it by three orders of magnitude in every format, as it does `rowsum` (O alone: 1.24 in bfloat16).
  Backward: the old gradient tolerance is doubled and accepts `dv_leak` everywhere (1e-6 of a value is invisible to a max norm; the
  bound wants an exact zero) and `delta` in both 16-bit formats.
  * `delta` -- O rounded a second time, one bit short of the format (f32 operands: to bfloat16) -- is also BELOW the 16-bit bound (err /
  bound 0.19 / 0.21): the error is a fraction of the one rounding of dS that the bound must allow.  It is named for f32 operands, where
  a 16-bit detour of O is hundreds of f32 units (err / bound 153)."""
import pytest
import torch

import _attn_ref as A
from _attn_ref import BF16, F16, F32, Case

FMTS = (BF16, F16, F32)


def _case(fmt, case_id, regime="plain"):
    layout, (B, H, Tq, Tk, hd), masked, p, *_ = A.intended(case_id)
    return Case(fmt, B, H, Tq, Tk, hd, regime, masked, p)


def _runs():
    half, f32 = A.gpu_runs()
    return [(f, i, r) for f in (BF16, F16) for i, r in half] + [(F32, i, r) for i, r in f32]


@pytest.mark.parametrize("fmt,case_id,regime", _runs())
def test_yardstick_meets_its_bare_k_and_float64_meets_k_1(fmt, case_id, regime):
    c = _case(fmt, case_id, regime)
    keep = c.host_keep()
    ref = c.forward(keep)
    yard, ideal = c.fwd_outputs(keep, yard=True), c.fwd_outputs(keep)
    ky = A.k_yard_of(c, ref, yard)
    worst_i, bad_i = A.judge(c, ref, ideal, 1.0)
    worst_y, bad_y = A.judge(c, ref, yard, {n: v * (1 + 1e-9) + 1e-12 for n, v in ky.items()})
    assert not bad_i and not bad_y, (bad_i, bad_y)
    refb = c.backward(yard["O"], yard["lse"], keep)
    yb, ib = c.bwd_outputs(yard["O"], yard["lse"], keep, yard=True), c.bwd_outputs(yard["O"], yard["lse"], keep)
    kyb = A.k_yard_of(c, refb, yb)
    worst_ib, bad_ib = A.judge(c, refb, ib, 1.0)
    _, bad_yb = A.judge(c, refb, yb, {n: v * (1 + 1e-9) + 1e-12 for n, v in kyb.items()})
    assert not bad_ib and not bad_yb, (bad_ib, bad_yb)
    ky.update(kyb)
    print("  %-44s K_yard %s" % (c.name(), "  ".join("%s %.3f" % kv for kv in ky.items())))
    assert all(0 <= v < 8 for v in ky.values()), ky          # a yardstick far outside its own magnitudes would make K meaningless
    if c.masked:       # structural zeros: the rows of the keys behind the mask
        pad = ~c.att.expand(c.B, c.H, 1, c.Tk)[:, :, 0]
        for n in ("dK", "dV"):
            assert float(refb[n].Afmt[pad].abs().max()) == 0.0 and float(yb[n][pad].abs().max()) == 0.0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case_id", sorted(A.PROBS_CASES))
def test_probs_yardstick(fmt, case_id):
    (B, H, Tq, Tk, hd), masked = A.PROBS_CASES[case_id]
    c = Case(fmt, B, H, Tq, Tk, hd, "plain", masked)
    ref, yard = c.probs(), c.probs_yard()
    ky = A.k_yard_of(c, ref, yard)
    _, bad = A.judge(c, ref, yard, {n: v * (1 + 1e-9) + 1e-12 for n, v in ky.items()})
    _, bad_i = A.judge(c, ref, {"probs": ref["probs"].ref.float()}, 1.0)
    assert not bad and not bad_i and ky["probs"] < 8, (bad, bad_i, ky)
    if masked:
        assert float(ref["probs"].ref.masked_select(~c.att.expand_as(ref["probs"].ref)).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- selection
def test_selection_mirror_equals_the_hand_written_table():
    for case_id in list(A.GPU_CASES) + list(A.F32_CASES):
        layout, (B, H, Tq, Tk, hd), masked, p, head, fwd, bwd_bits, bwd_regen = A.intended(case_id)
        fmt = F32 if case_id in A.F32_CASES else BF16
        flags = masked or p > 0
        nb = A.mask_bytes(B, H, Tq, Tk, hd, fmt, head)
        bits = p > 0 and nb > 0
        assert A.select(fmt, Tq, Tk, hd, flags, bits, False, head) == fwd, case_id
        assert (bwd_bits is not None) == bits, case_id
        if bits:
            assert A.select(fmt, Tq, Tk, hd, flags, True, True, head) == bwd_bits, case_id
        assert A.select(fmt, Tq, Tk, hd, flags, False, True, head) == bwd_regen, case_id
        for sel, back in ((fwd, False), (bwd_regen, True)):
            assert len(A.tag_of(sel, back, hd, Tq, Tk)) < 40, "the tag must fit ProfRec::tag"
    assert len(A.tag_of(A.Sel("resident", 2, 1, 0, 4), False, 128, 99999, 128)) < 40
    assert len(A.tag_of(A.Sel("stream", 0, 1, 0, 4), True, 128, 99999, 99999)) < 40


def test_selection_lds_edges():
    # hd 128: head-resident up to 288 keys (148 608 B forward, 150 912 B backward), not at 300 (320 rows: 165 120 B)
    assert A.head_lds_bytes(40, 288, 128, False, False) == 148608 and A.head_lds_bytes(40, 288, 128, True, False) == 150912
    assert A.select(BF16, 40, 288, 128, False, False, False).family == "head" and A.select(BF16, 40, 288, 128, False, False, True).family == "head"
    assert A.head_lds_bytes(40, 300, 128, False, False) == 165120 > A.LDS_MAX
    assert A.select(BF16, 40, 300, 128, False, False, False) == A.Sel("long", None, 0, 0, 4)
    assert A.select(BF16, 40, 300, 128, False, False, True) == A.Sel("stream", 0, 0, 0, 4)
    # Tq 300, Tk 70, hd 128: the forward image is the keys' (96 rows), the backward image the queries' (320 rows)
    assert A.select(BF16, 300, 70, 128, True, True, False) == A.Sel("head", None, 1, 1, 8)
    assert A.mask_bytes(1, 2, 300, 70, 128, BF16) == 2 * 300 * 32
    for bits in (True, False):
        assert A.head_lds_bytes(300, 70, 128, True, bits) > A.LDS_MAX
        assert A.select(BF16, 300, 70, 128, True, bits, True) == A.Sel("stream", 2, 1, 0, 4)
    # saved bits exist up to 256 keys only, and never for f32 operands or with the head kernels switched off
    assert A.mask_bytes(2, 2, 40, 256, 64, BF16) > 0 and A.mask_bytes(2, 2, 40, 257, 64, BF16) == 0 and A.mask_bytes(1, 2, 40, 288, 128, BF16) == 0
    assert A.mask_bytes(2, 2, 40, 49, 64, F32) == 0 and A.mask_bytes(2, 2, 40, 49, 64, BF16, head=0) == 0
    assert [A.attn_kch(t) for t in (64, 65, 128, 129, 256, 257)] == [1, 2, 2, 4, 4, 0]


def test_token_buffers_respect_the_stride_rules():
    for dense in (False, True):
        t = A.Tokens(3, 50, 3 * 2 * 64, torch.bfloat16, dense)
        assert all(s % 8 == 0 for s in t.strides(64)) and t.offset(1, 128) % 8 == 0
        buf = t.nan()
        x = torch.randn(3, 2, 17, 64)
        t.put(buf, x, 1, 128)
        assert torch.equal(t.get(buf, 1, 17, 128, 2, 64), x.bfloat16().float()) and int(torch.isfinite(buf.float()).sum()) == x.numel()
        out, bad = t.poison(), []
        t.check("untouched", out, [], bad)
        assert not bad
        t.check("unwritten", out, [(0, 50, 0, 128)], bad)
        assert len(bad) == 1
        out[0, 0] = 1.0
        t.check("guard", out, [], bad)
        assert len(bad) == 2


# ---------------------------------------------------------------------------------------------------------------- mutants
#         mutant      pass   case: shape, masked, p, regime                                formats it is named for
MUTANTS = {
    "rowsum":   ("fwd", ((1, 2, 70, 300, 128), True, 0.0, "plain"), FMTS),
    "inv_keep": ("fwd", ((2, 2, 128, 49, 128), False, 0.1, "plain"), FMTS),
    "row":      ("fwd", ((2, 3, 50, 50, 32), False, 0.0, "plain"), FMTS),
    "scale":    ("fwd", ((3, 2, 33, 17, 32), True, 0.3, "plain"), FMTS),
    "lse":      ("bwd", ((2, 2, 197, 197, 64), False, 0.0, "plain"), FMTS),
    "delta":    ("bwd", ((2, 2, 50, 50, 64), False, 0.0, "plain"), (F32,)),
    "dv_leak":  ("bwd", ((3, 2, 100, 100, 64), True, 0.0, "plain"), FMTS),
    "dk_scale": ("bwd", ((3, 2, 48, 48, 64), True, 0.0, "plain"), FMTS),
}


def _mutate(fmt, mut, spec):
    """-> (the bound's violations with the case's own K, {quantity: (old check accepted, its figure)})."""
    which, ((B, H, Tq, Tk, hd), masked, p, regime), _ = spec
    c = Case(fmt, B, H, Tq, Tk, hd, regime, masked, p)
    keep = c.host_keep()
    ref = c.forward(keep)
    yard = c.fwd_outputs(keep, yard=True)
    if which == "fwd":
        K = {n: A.bound_k(v) for n, v in A.k_yard_of(c, ref, yard).items()}
        got = c.fwd_outputs(keep, mut=mut)
    else:
        ideal = c.fwd_outputs(keep)
        ref = c.backward(ideal["O"], ideal["lse"], keep)
        K = {n: A.bound_k(v) for n, v in A.k_yard_of(c, ref, c.bwd_outputs(ideal["O"], ideal["lse"], keep, yard=True)).items()}
        got = c.bwd_outputs(ideal["O"], ideal["lse"], keep, mut=mut)
    worst, bad = A.judge(c, ref, got, K)
    old = {n: A.old_check(got[n], ref[n].ref, fmt, grad=which == "bwd") for n in got if n != "lse"}
    return worst, bad, old


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutants_are_rejected_where_they_are_named(mut):
    for spec in [MUTANTS[mut]]:
        for fmt in spec[2]:
            worst, bad, old = _mutate(fmt, mut, spec)
            print("  %-9s %-4s %-6s worst err / bound %s   old check %s" % (mut, fmt, spec[1][3], {n: "%.3g" % v for n, v in worst.items()},
                                                                            {n: ("A" if a else "R", "%.2e" % e) for n, (a, e) in old.items()}))
            assert bad, "%s in %s slipped through the bound: %s" % (mut, fmt, worst)


def test_old_check_accepts_what_the_bound_rejects():
    """In each 16-bit format at least one FORWARD mutant passes the old max-norm check at its own tolerance and is rejected by the bound;
    the unmutated reference passes both.  Every mutant's figures are printed in every format (the docstring's table)."""
    both = {BF16: [], F16: []}
    for mut, spec in sorted(MUTANTS.items()):
        for fmt in FMTS:
            worst, bad, old = _mutate(fmt, mut, spec)
            accepted = all(a for a, _ in old.values())
            print("  %-9s %-4s bound %s (worst %.3g)   old check %s %s" % (mut, fmt, "rejects" if bad else "ACCEPTS", max(worst.values()),
                                                                           "accepts" if accepted else "rejects", {n: "%.2e" % e for n, (_, e) in old.items()}))
            if spec[0] == "fwd" and fmt in both and accepted and bad:
                both[fmt].append(mut)
    assert both[BF16] and both[F16], both
    for fmt in (BF16, F16):
        worst, bad, old = _mutate(fmt, None, MUTANTS["rowsum"])
        assert not bad and all(a for a, _ in old.values())
