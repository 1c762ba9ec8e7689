"""The 16-bit (and f32 parity) GEMM kernels of csrc/gemm.hip, gemm_q8.h and gemm_q16.h in plain torch on the CPU: what
tests/test_gemm_float64_gpu.py holds ecamp_gemm / ecamp_gemm_res32 to, element by element, and what tests/test_gemm_reference_cpu.py
proves about it without a GPU.  The method and vocabulary are those of tests/_sr_ref.py and tests/_report_ref.py, whose U, TINY, stored,
fmt_of, k_of and bound_k are used as they are.

Everything is float64 on the values the kernel is given (the stored 16-bit operands, the f32 bias), in ecamp_gemm terms (M, N, K = the
contraction): opA [M, K], opB [N, K] whatever the storage order of the form (f: x [M, K], w [N, K]; d: dy [M, K], w stored [K, N];
w: dy stored [K, M], x stored [K, N]).
    acc = sum_k opA opB                Aacc = sum_k |opA| |opB|
    pre = a acc + bias                 Apre = |a| Aacc + |bias|            a = alpha * alpha_dev
    a residual and prior contents (accumulate) add their value to ref and their absolute value to the magnitude
    rowsum[m] = prior + a sum_k opA[m, k]                                  A = |prior| + |a| sum_k |opA[m, k]|

Bound of a stored output (C, pre_out), EVERY element:
    e = Kacc U32 A + extra,      |got - ref| <= e + R[fmt] (|ref| + e) + TINY[fmt]
  the first term judges the accumulation at the f32 unit against the magnitude sum, the second is one rounding of the value itself (the
  form of _hold in tests/test_flat_kernels_gpu.py); f32 outputs (out_f32, res32, weight gradients, rowsum) have e + TINY only.
  R is ONE rounding of the format, 2^-8 for bfloat16 and 2^-11 for half: U of _report_ref.py is HALF a rounding of a 16-bit format
  (its docstring: the K u A form carries a K >= 1 next to it), so R = 2 U there, and R = U for f32.  With U itself in that place no
  kernel could pass: test_one_rounding_is_two_U shows the float64 reference rounded once to the format -- the best a kernel can
  return -- outside that form and inside this one with e = 0.
  Kacc = bound_k(K_yard) = max(1, 4 K_yard), K_yard the yardstick's largest (err - extra) / (U32 A) on the same inputs.
Yardstick: a float32 chain in k order, one product per step (acc = acc + x[:, k:k+1] @ w[:, k:k+1].T), then the epilogue in float32;
  for split-K every slice is chained and the slices are chained.  Never torch.matmul: it sums blockwise and sits closer to float64 than
  a chain can.  On the two large shapes the yardstick runs on every 16th row; every row is judged.

GELU.  With pre_out the kernels apply GELU to the ROUNDED pre-activation (gemm_args.h, epilogue4): y is judged against float64 GELU of
  the pre_out the kernel returned, bound EPS + R (|ref| + EPS) + TINY, the accumulation is not charged twice.  Without pre_out (128^2
  kernel only) A = 1.13 Apre (max |gelu'| = 1.129) and extra = EPS.  The saved derivative (act 2) is judged against float64 gelu' of
  the pre_out an act 1 call on the same inputs returned.  The data gradient's gmul epilogue with act 0 multiplies by
  g = gelu'64(gmul), extra = |a acc| EPS'; with act 2 g = gmul exactly.
  EPS / EPS' are twice what tests/test_gemm_reference_cpu.py measures for float32 restatements of gelu_fast_f, gelu_both_fast_f and
  gelu_grad_fast_f (csrc/common.h) over every finite input of the format (v_rcp_f32 and v_exp_f32 are 1-ulp approximations where the
  CPU divides and exponentiates exactly, and the compiler may contract); measured maxima (65 280 bfloat16 / 63 488 half inputs):
      gelu_fast_f 7.047e-07 / 7.047e-07    gelu' of gelu_both_fast_f 1.072e-06 / 1.259e-06    gelu_grad_fast_f 2.279e-07 / 2.654e-07
  (the first is the 7.0e-7 of the comment above gelu_fast_f2).  f32 operands run erff: the 2e-6 of test_mul_gelu_grad.

Regimes (each generator asserts its own property):
  plain   N(0,1) activations, weights times K^-0.5, as the older tests.
  scales  row m of the M-side operand, of the residual and of the prior contents times 2^k, k = (5 m mod 13) - 6: an error confined
          to a 2^-6 row is 2^-12 of the tensor's maximum.  gmul is not scaled.
  Every draw is floored to |value| >= 2^-8 before scaling and no stored operand is subnormal in its format: subnormal MFMA inputs are
  out of scope.  Outputs may be subnormal, hence TINY.

Pads and guards (Slab): every matrix sits with leading dimension width + 8 inside an allocation with 8 guard rows before and after;
  input pads and guards hold NaN, output pads, guards and every logical element the call overwrites hold 0x5A5A5A5A.  After the call
  every pad and guard word is intact and no logical 32-bit word still carries the pattern (a 16-bit output is looked at in pairs: the
  kernels store at least four columns at a time, and one element may well BE 0x5A5A, 203.25 in half)."""
import functools
import math

import torch

from _report_ref import BF16, DTYPE, F16, F32, TINY, U, fmt_of, stored  # noqa: F401
from _sr_ref import bound_k, k_of  # noqa: F401

U32 = U[F32]
R = {F32: U[F32], BF16: 2 * U[BF16], F16: 2 * U[F16]}      # one rounding of the format
MIN_NORMAL = {F32: 2.0 ** -126, BF16: 2.0 ** -126, F16: 2.0 ** -14}
FLOOR = 2.0 ** -8
PATTERN = 0x5A5A5A5A
PAD, GUARD = 8, 8
GELU_SLOPE = 1.13
YARD_ROWS_LARGE = 16

# measured by test_gemm_reference_cpu.py::test_eps_of_the_fast_gelu_forms, which holds these figures to what it measures
EPS_MEASURED = {(BF16, "gelu"): 7.047e-07, (BF16, "both"): 1.072e-06, (BF16, "grad"): 2.279e-07,
                (F16, "gelu"): 7.047e-07, (F16, "both"): 1.259e-06, (F16, "grad"): 2.654e-07}
EPS_F32 = 2e-6


def eps_of(fmt, which):
    """The allowance of the GELU (`gelu`), of the derivative gelu_both_fast_f saves (`both`) and of gelu_grad_fast_f (`grad`)."""
    return EPS_F32 if fmt == F32 else 2.0 * EPS_MEASURED[(fmt, which)]


# ================================================================================================ GELU
def gelu64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _c(v):
    return torch.tensor(v, dtype=torch.float32)


def _fma(a, b, c):
    return torch.addcmul(c, a, b)


def _fast_q(x):
    """q = 1/2 - erfc(|x| / sqrt 2) / 2 of gelu_fast_f (Abramowitz-Stegun 7.1.28), float32."""
    x2 = x * x
    E = _fma(_fma(_fma(_c(5.3829750000e-06), x2, _c(3.8003575000e-05)), x2, _c(2.1141006150e-02)), x2, _c(1.0))
    O = _fma(_fma(_c(4.8890635643e-05), x2, _c(3.2776263241e-03)), x2, _c(4.9867346967e-02))
    s = _fma(x.abs(), O, E)
    for _ in range(4):
        s = s * s
    return _fma(_c(-0.5), 1.0 / s, _c(0.5))


def gelu_fast32(x):
    """gelu_fast_f of csrc/common.h in float32 torch."""
    x = x.float()
    return _fma(x.abs(), _fast_q(x), x * 0.5)


def gelu_both_fast32(x):
    """gelu_both_fast_f -> (y, gelu')."""
    x = x.float()
    q = _fast_q(x)
    e = torch.exp2((x * x) * _c(-0.72134752044448170368))
    phi = 0.5 + torch.copysign(q, x)
    return _fma(x.abs(), q, x * 0.5), _fma(x * _c(0.39894228040143267794), e, phi)


def gelu_grad_fast32(x):
    """gelu_grad_fast_f (erf_as_f: Abramowitz-Stegun 7.1.26)."""
    x = x.float()
    z = x * _c(0.70710678118654752440)
    a = z.abs()
    t = 1.0 / _fma(_c(0.3275911), a, _c(1.0))
    p = _fma(_c(1.061405429), t, _c(-1.453152027))
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = _fma(p, t, _c(c))
    p = p * t
    e = torch.exp2((_c(-1.4426950408889634) * a) * a)
    erf = torch.copysign(_fma(-p, e, _c(1.0)), z)
    return _fma(x * _c(0.39894228040143267794), e, 0.5 * (1.0 + erf))


def all_finite(fmt):
    """Every finite value of a 16-bit format, as float32."""
    v = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(DTYPE[fmt]).float()
    return v[torch.isfinite(v)]


# ================================================================================================ the kernel selection, restated
FORCE = {   # the switches that force a family where it is legal
    "t128": dict(q8_mode=0, q16_mode=0, q16_wgrad=0),
    "q8": dict(q8_mode=2, q16_mode=0, q16_wgrad=0),
    "q16": dict(q8_mode=2, q16_mode=3, q16_wgrad=2),
}
DEFAULTS = dict(q8_mode=-1, q16_mode=-1, q16_wgrad=-1, q8_bwd_grid=0)     # what ecamp_set_option takes as "back to the default"
WIDTH = {"t128": 128, "q8": 256}

#      name            bias   res    pre    act gmul   out_f32 alpha alpha_dev
EPI = {
    "plain":         (False, None,  False, 0, False, False, 1.0,  None),
    "bias":          (True,  None,  False, 0, False, False, 1.0,  None),
    "res":           (False, "h",   False, 0, False, False, 1.0,  None),
    "bias_res":      (True,  "h",   False, 0, False, False, 1.0,  None),
    "bias_gelu_pre": (True,  None,  True,  1, False, False, 1.0,  None),
    "bias_der":      (True,  None,  True,  2, False, False, 1.0,  None),
    "bias_gelu":     (True,  None,  False, 1, False, False, 1.0,  None),
    "out_f32":       (True,  None,  False, 0, False, True,  1.0,  None),
    "res32":         (True,  "f32", False, 0, False, True,  1.0,  None),
    "alpha":         (False, None,  False, 0, False, False, 0.25, None),
    "alpha_dev":     (False, None,  False, 0, False, False, 1.0,  0.75),
    "gmul0":         (False, None,  False, 0, True,  False, 1.0,  None),
    "gmul2":         (False, None,  False, 2, True,  False, 1.0,  None),
    "gmul0_res":     (False, "h",   False, 0, True,  False, 1.0,  None),
    "wgrad":         (False, None,  False, 0, False, True,  1.0,  0.75),
}


def cdiv(a, b):
    return -(-a // b)


def q8_epi(epi):
    """q8_epi of csrc/gemm.hip: the epilogue variant of the persistent kernels, -1 where none fits."""
    bias, res, pre, act, gmul, out_f32, _, _ = EPI[epi]
    if res == "f32":
        return 5 if (out_f32 and not pre and not gmul and not act) else -1
    if out_f32:
        return 4 if not (bias or res or pre or gmul or act) else -1
    if gmul:
        return 3 if (not bias and not pre and act in (0, 2)) else -1
    if pre or act:
        return 1 if (pre and act in (1, 2) and not res) else -1
    return 2 if res else 0


Q8_FORMS = {"f": (0, 1, 2, 5), "d": (0, 2, 3), "w": (4,)}      # q8_pick: the instantiations that exist


def eff_split(K, split, fmt):
    """gemm_call: whole K tiles per slice, the split count only ever goes down -> (slice length, slices)."""
    ktile = 16 if fmt == F32 else 64
    kps = cdiv(cdiv(K, max(1, split)), ktile) * ktile
    return kps, cdiv(K, kps)


def q8_legal(form, M, N, K, fmt, epi, split, pad=PAD):
    """q8_legal's shape conditions (every pointer of the tests is 16-B aligned; nothing here is near 2 GB)."""
    e = q8_epi(epi)
    if fmt == F32 or e < 0 or e not in Q8_FORMS[form]:
        return False
    _, ns = eff_split(K, split, fmt)
    if ns > 1 and e != 4:
        return False
    kps = cdiv(cdiv(K, ns), 64) * 64
    ns2 = cdiv(K, kps)
    if kps < 128 or K - (ns2 - 1) * kps <= 64:
        return False
    lda = (K if form != "w" else M) + pad
    ldb = (K if form == "f" else N) + pad
    if N % 8 or lda % 8 or ldb % 8 or (form == "w" and M % 8):
        return False
    return ns > 1 or (N + pad) % 8 == 0          # ldc, ldp, ldg and ldr are all N + pad here


def q16_cost(M, N, tn, ncu):
    return cdiv(cdiv(M, 256) * cdiv(N, tn), ncu) * (0.79 if tn == 192 else 1.0)


def route(form, M, N, K, fmt, epi, split=1, rowsum=False, force=None, ncu=256, pad=PAD, q8_mode=-1, q16_mode=1, q16_wgrad=1):
    """gemm_select of csrc/gemm.hip as plain arithmetic -> (family, tile width).  force: a key of FORCE, else the switches as given."""
    if force is not None:
        sw = FORCE[force]
        q8_mode, q16_mode, q16_wgrad = sw["q8_mode"], sw["q16_mode"], sw["q16_wgrad"]
    _, ns = eff_split(K, split, fmt)
    items8 = cdiv(M, 256) * cdiv(N, 256) * ns
    min_items = ncu // 2
    w16 = form == "w" and q16_wgrad == 2
    if q8_mode == 0 or not (q8_mode == 2 or items8 >= min_items or q16_mode == 3 or w16) or not q8_legal(form, M, N, K, fmt, epi, split, pad):
        return "t128", 128
    e = q8_epi(epi)
    if q16_mode > 0 and form != "w" and e in (0, 2, 5) and ns == 1 and not rowsum:
        nw = 6 if q16_cost(M, N, 192, ncu) <= 0.9 * q16_cost(M, N, 256, ncu) else 8
        if q16_mode >= 2 or nw == 6:
            return "q16", nw * 32
    if form == "w" and e == 4:
        on = q16_wgrad >= 2 or (q16_wgrad == 1 and q16_mode != 0 and M >= 256 and N >= 256 and items8 >= min_items)
        if on:
            return "q16", 256
    return "q8", 256


def suggest_split(M, N, K, form, fmt, q8_mode=-1, ncu=256):
    """ecamp_gemm_suggest_split for 256 CUs and no CU reserve."""
    s_old = max(1, 1024 // (cdiv(M, 128) * cdiv(N, 128)))
    s_old = min(s_old, cdiv(K, 256))
    if fmt == F32 or q8_mode == 0 or form != "w":
        return s_old
    t8 = cdiv(M, 256) * cdiv(N, 256)
    best, best_score = 1, -1.0
    for sp in range(1, 33):
        if sp > 1 and K // sp < 512:
            break
        items = t8 * sp
        score = items / (cdiv(items, ncu) * ncu) - 0.012 * (sp - 1)
        if score > best_score + 1e-9:
            best, best_score = sp, score
    return best if t8 * best >= ncu // 2 else s_old


def tag_of(family, width, form, M, N, K, fmt, epi, split=1):
    """The profiler tag of the launch: name:form:e<epi>:M:N:K:w<tile> (four-wave forward / data gradient) | s<split>."""
    _, ns = eff_split(K, split, fmt)
    e = "-" if family == "t128" else str(q8_epi(epi))
    tail = "w%d" % width if (family == "q16" and form != "w") else "s%d" % ns
    return "%s:%s:e%s:%d:%d:%d:%s" % (family, form, e, M, N, K, tail)


# ---- the case tables of tests/test_gemm_float64_gpu.py and the kernel every case is MEANT to reach, written down by hand
BASE_M, BASE_N, BASE_KS = 264, 264, (128, 136, 392)
ODD = (133, 260, 72)                       # 128^2 only: groups of 4 past N, M a multiple of nothing
WALK = (32776, 264, 136)                   # 258 tiles of either width: on 256 CUs two workgroups walk two tiles
WIDE = (32776, 200, 136)                   # 129 tiles of 256 columns against 258 of 192: the only way to the four-wave kernel's 256-column form
WGRAD_KS = (136, 4104)
WGRAD_EXTRA_SPLIT = 8                      # the suggested split (17) leaves a last slice of 8 < 64: the persistent kernels refuse it (q8_legal)
REGIMES = ("plain", "scales")
FWD_EPIS = ("plain", "bias", "bias_res", "bias_gelu_pre", "bias_der", "res32", "bias_gelu", "out_f32")
DGRAD_EPIS = ("plain", "alpha", "alpha_dev", "res", "gmul0", "gmul2", "gmul0_res")
WIDE_CASES = (("f", "bias"), ("f", "res"), ("f", "res32"), ("d", "plain"), ("d", "res"))
F32_CASES = (("f", ODD, "plain"), ("f", ODD, "bias_res"), ("f", ODD, "bias_gelu_pre"), ("f", ODD, "bias_gelu"),
             ("f", (BASE_M, BASE_N, 136), "bias"), ("d", (BASE_M, BASE_N, 136), "plain"), ("d", (BASE_M, BASE_N, 136), "gmul0"),
             ("d", (BASE_M, BASE_N, 136), "gmul0_res"))

_T, _Q8, _W192, _W256 = ("t128", 128), ("q8", 256), ("q16", 192), ("q16", 256)
INTENDED = {
    # base shape, every K of BASE_KS, both formats: {forced family: {epilogue: (family, tile width)}}
    "f": {
        "t128": {"plain": _T, "bias": _T, "bias_res": _T, "bias_gelu_pre": _T, "bias_der": _T, "res32": _T, "bias_gelu": _T, "out_f32": _T},
        "q8": {"plain": _Q8, "bias": _Q8, "bias_res": _Q8, "bias_gelu_pre": _Q8, "bias_der": _Q8, "res32": _Q8, "bias_gelu": _T, "out_f32": _T},
        "q16": {"plain": _W192, "bias": _W192, "bias_res": _W192, "bias_gelu_pre": _Q8, "bias_der": _Q8, "res32": _W192, "bias_gelu": _T,
                "out_f32": _T},
    },
    "d": {
        "t128": {"plain": _T, "alpha": _T, "alpha_dev": _T, "res": _T, "gmul0": _T, "gmul2": _T, "gmul0_res": _T},
        "q8": {"plain": _Q8, "alpha": _Q8, "alpha_dev": _Q8, "res": _Q8, "gmul0": _Q8, "gmul2": _Q8, "gmul0_res": _Q8},
        "q16": {"plain": _W192, "alpha": _W192, "alpha_dev": _W192, "res": _W192, "gmul0": _Q8, "gmul2": _Q8, "gmul0_res": _Q8},
    },
    # weight gradient out 264 x 264: {forced family: {(contraction, split asked for): (family, tile width)}}; 17 is the suggested split
    "w": {
        "t128": {(136, 1): _T, (4104, 1): _T, (4104, 17): _T, (4104, 8): _T},
        "q8": {(136, 1): _Q8, (4104, 1): _Q8, (4104, 17): _T, (4104, 8): _Q8},
        "q16": {(136, 1): _W256, (4104, 1): _W256, (4104, 17): _T, (4104, 8): _W256},
    },
    "odd": _T,                                # every epilogue of ODD, whatever is forced: N % 8
    "walk": {"q8": _Q8, "q16": _W192},
    "wide": _W256,
    "f32": _T,
}
SUGGESTED_SPLIT = {136: 1, 4104: 17}


def wgrad_calls(K):
    """(split asked for, accumulate, rowsum) of the weight-gradient calls at contraction K: every split with overwrite and accumulate,
    with and without the row sums."""
    splits = [1] + ([SUGGESTED_SPLIT[K]] if SUGGESTED_SPLIT[K] > 1 else []) + ([WGRAD_EXTRA_SPLIT] if K == 4104 else [])
    return [(sp, acc, rs) for sp in splits for acc in (False, True) for rs in (False, True)]


def all_cases(fmt):
    """The arguments of every Case of the GPU tables in one format (test_gemm_reference_cpu.py walks them)."""
    L = YARD_ROWS_LARGE
    if fmt == F32:
        for form, (M, N, K), epi in F32_CASES:
            yield dict(form=form, M=M, N=N, K=K, epi=epi)
        for sp, acc, rs in ((1, False, True), (SUGGESTED_SPLIT[4104], True, True)):
            yield dict(form="w", M=BASE_M, N=BASE_N, K=4104, epi="wgrad", split=sp, accumulate=acc, rowsum=rs)
        return
    for regime in REGIMES:
        for K in BASE_KS:
            for form, epis in (("f", FWD_EPIS), ("d", DGRAD_EPIS)):
                for epi in epis:
                    yield dict(form=form, M=BASE_M, N=BASE_N, K=K, regime=regime, epi=epi)
        for epi in FWD_EPIS:
            yield dict(form="f", M=ODD[0], N=ODD[1], K=ODD[2], regime=regime, epi=epi)
        for K in WGRAD_KS:
            for sp, acc, rs in wgrad_calls(K):
                yield dict(form="w", M=BASE_M, N=BASE_N, K=K, regime=regime, epi="wgrad", split=sp, accumulate=acc, rowsum=rs)
    yield dict(form="f", M=WALK[0], N=WALK[1], K=WALK[2], epi="bias", yard_step=L)
    for form, epi in WIDE_CASES:
        yield dict(form=form, M=WIDE[0], N=WIDE[1], K=WIDE[2], epi=epi, yard_step=L)


# ================================================================================================ inputs
def scale_k(rows):
    return (5 * torch.arange(rows)) % 13 - 6


def _draw(g, *shape):
    t = torch.randn(*shape, generator=g)
    return torch.where(t.abs() < FLOOR, torch.copysign(torch.full_like(t, FLOOR), t), t)


def _normal(t, fmt):
    return bool(((t.abs() >= MIN_NORMAL[fmt]) & torch.isfinite(t)).all())


class Operands:
    """The inputs of one (format, form, shape, regime), the float64 products and the float32 chains, computed once."""

    def __init__(self, fmt, form, M, N, K, regime):
        assert form in "fdw" and regime in REGIMES
        self.fmt, self.form, self.M, self.N, self.K, self.regime = fmt, form, M, N, K, regime
        g = torch.Generator().manual_seed(1000003 * REGIMES.index(regime) + 7919 * "fdw".index(form) + 31 * M + 17 * N + K)
        a, b = _draw(g, M, K), _draw(g, N, K)
        if form != "w":
            b = b * K ** -0.5
        res, prior, res32 = _draw(g, M, N), _draw(g, M, N), _draw(g, M, N)
        self.bias, self.gmul = _draw(g, N), stored(_draw(g, M, N), fmt)
        self.rs_prior = torch.ones(M)
        if regime == "scales":
            k = scale_k(M)
            s = (2.0 ** k.double()).float()[:, None]
            a, res, prior, res32 = a * s, res * s, prior * s, res32 * s
            assert len(set(k.tolist())) == min(M, 13) and int(k.min()) == -6 and int(k.max()) <= 6 and int(k[0]) == -6
            assert M == 1 or int((k[1:] - k[:-1]).abs().min()) >= 5, "scales: neighbouring rows less than five binades apart"
        self.a, self.b, self.res = stored(a, fmt), stored(b, fmt), stored(res, fmt)
        self.prior, self.res32 = prior, res32
        for t in (self.a, self.b, self.res, self.gmul):
            assert _normal(t, fmt), "a stored operand is zero, subnormal or not finite"
        if regime == "scales":       # a power of two commutes with the rounding of a normal value
            assert torch.equal(self.a, stored(self.a / s, fmt) * s)
        a64, b64 = self.a.double(), self.b.double()
        self.acc, self.Aacc = a64 @ b64.T, a64.abs() @ b64.abs().T
        self.asum, self.Aasum = a64.sum(1), a64.abs().sum(1)
        self._chains = {}

    def chain(self, kps, step):
        """-> (float32 chain of the products of rows ::step, of the row sums of opA): slices of kps chained, then the slices."""
        key = (kps, step)
        if key not in self._chains:
            a, b = self.a[::step].contiguous(), self.b
            total = rs = None
            for k0 in range(0, self.K, kps):
                acc = torch.zeros(a.shape[0], self.N)
                r = torch.zeros(a.shape[0])
                for k in range(k0, min(self.K, k0 + kps)):
                    acc = acc + a[:, k:k + 1] @ b[:, k:k + 1].T
                    r = r + a[:, k]
                total, rs = (acc, r) if total is None else (total + acc, rs + r)
            self._chains[key] = (total, rs)
        return self._chains[key]


@functools.lru_cache(maxsize=3)
def operands(fmt, form, M, N, K, regime):
    return Operands(fmt, form, M, N, K, regime)


class Case:
    """One call on the host: the reference, the magnitudes, the yardstick and K_yard of every output."""

    def __init__(self, fmt, form, M, N, K, regime="plain", epi="plain", split=1, accumulate=False, rowsum=False, yard_step=1):
        o = self.o = operands(fmt, form, M, N, K, regime)
        self.fmt, self.form, self.M, self.N, self.K, self.regime, self.epi = fmt, form, M, N, K, regime, epi
        self.split, self.accumulate, self.rowsum, self.step = split, accumulate, rowsum, yard_step
        self.has_bias, self.res_kind, self.pre_out, self.act, self.has_gmul, out_f32, self.alpha, self.alpha_dev = EPI[epi]
        assert (form == "w") == (epi == "wgrad") and (split == 1 or form == "w") and not ((accumulate or rowsum) and form != "w")
        self.out_fmt = F32 if (out_f32 or fmt == F32) else fmt
        a = self.a_s = self.alpha * (self.alpha_dev if self.alpha_dev is not None else 1.0)
        a32 = torch.tensor(self.alpha, dtype=torch.float32) * (1.0 if self.alpha_dev is None else torch.tensor(self.alpha_dev, dtype=torch.float32))
        self.kps, self.nsplit = eff_split(K, split, fmt)
        chain, rs_chain = o.chain(self.kps, yard_step)
        s = slice(None, None, yard_step)
        bias = o.bias if self.has_bias else torch.zeros(N)
        res = {None: torch.zeros(1, 1), "h": o.res, "f32": o.res32}[self.res_kind]
        prior = o.prior if accumulate else torch.zeros(1, 1)
        lin, Alin = a * o.acc + bias.double(), abs(a) * o.Aacc + bias.double().abs()
        v32 = chain * a32 + bias
        self.extra = 0.0
        if self.pre_out:                       # the stored pre-activation; y and the saved derivative are judged from what the kernel stored
            self.ref, self.A, yard = lin, Alin, v32
        elif self.act == 1:                    # GELU of the unrounded pre-activation
            self.ref, self.A, self.extra = gelu64(lin), GELU_SLOPE * Alin, eps_of(fmt, "gelu")
            yard = gelu64(v32).float()
        elif self.has_gmul:
            g = dgelu64(o.gmul) if self.act == 0 else o.gmul.double()
            self.ref, self.A = lin * g + res.double(), Alin * g.abs() + res.double().abs()
            self.extra = (a * o.acc).abs() * eps_of(fmt, "grad") if self.act == 0 else 0.0
            yard = v32 * g.float()[s] + res[s]
        else:
            self.ref, self.A = lin + res.double() + prior.double(), Alin + res.double().abs() + prior.double().abs()
            yard = v32 + res[s] + prior[s]
        self.ref, self.A = self.ref.expand(M, N), self.A.expand(M, N)
        self.yard = yard
        ex = self.extra[s] if torch.is_tensor(self.extra) else self.extra
        self.k_yard = k_of(yard, self.ref[s], self.A[s], U32, allowance=ex)
        self.kacc = bound_k(self.k_yard)
        if rowsum:
            self.rs_ref, self.rs_A = o.rs_prior.double() + a * o.asum, o.rs_prior.double().abs() + abs(a) * o.Aasum
            self.rs_yard = rs_chain * a32 + o.rs_prior[s]
            self.rs_k_yard = k_of(self.rs_yard, self.rs_ref[s], self.rs_A[s], U32)
            self.rs_kacc = bound_k(self.rs_k_yard)

    def name(self):
        extra = "" if self.form != "w" else " split %d acc %d rowsum %d" % (self.split, self.accumulate, self.rowsum)
        return "%s %s %dx%dx%d %-13s %-6s%s" % (self.fmt, self.form, self.M, self.N, self.K, self.epi, self.regime, extra)

    def ideal(self):
        """What a kernel that computes in float64 and rounds where the kernels store would return."""
        out = {"C": stored(self.ref.float(), self.out_fmt) if self.out_fmt != F32 else self.ref.float()}
        if self.pre_out:
            pre = stored(self.ref.float(), self.fmt)
            out["pre1"] = pre
            out["C"] = stored(gelu64(pre).float(), self.fmt)
            out["pre"] = pre if self.act == 1 else stored(dgelu64(pre).float(), self.fmt)
        if self.rowsum:
            out["rowsum"] = self.rs_ref.float()
        return out

    def yardstick(self):
        """What a kernel that IS the yardstick would return (the rows ::step the yardstick ran on)."""
        v = self.yard
        out = {"C": v if self.out_fmt == F32 else stored(v, self.out_fmt)}
        if self.pre_out:
            pre = stored(v, self.fmt)
            out["pre1"] = pre
            out["C"] = stored(gelu64(pre).float(), self.fmt)
            out["pre"] = pre if self.act == 1 else stored(dgelu64(pre).float(), self.fmt)
        if self.rowsum:
            out["rowsum"] = self.rs_yard
        return out


# ================================================================================================ the judge
def _hold(tag, q, got, ref, A, K, fmt, extra, bad):
    """Every element of one output against its bound -> the worst err / bound."""
    e = K * U32 * A + extra
    bound = e + TINY[fmt] if fmt == F32 else e + R[fmt] * (ref.abs() + e) + TINY[fmt]
    g = got.double().reshape(ref.shape)
    err = (g - ref).abs()
    ok = err <= bound                      # (False for a NaN)
    worst = float(torch.nan_to_num(err / bound, nan=float("inf")).max())
    if not bool(ok.all()):
        i = int(torch.nan_to_num(err / bound, nan=float("inf")).argmax())
        bad.append("%s %s: %d of %d elements outside the bound; the worst, at %s: got %r ref %r bound %.3e (err / bound %.3f)"
                   % (tag, q, int((~ok).sum()), ok.numel(), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ref.shape)),
                      float(g.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(bound.reshape(-1)[i]), worst))
    return worst


def judge(c, got, kacc=None, rs_kacc=None, step=1):
    """got: host tensors as the kernel stored them -- C; pre (what pre_out received) and pre1 (the pre_out of the act = 1 call, pre itself
    when act == 1) with pre_out; rowsum.  -> (worst err / bound, violations).  kacc: another K than the case's own, step: `got` holds
    rows ::step only (both for the yardstick's own test)."""
    bad, tag = [], c.name()
    K = c.kacc if kacc is None else kacc
    s = slice(None, None, step)
    ref, A, extra = c.ref[s], c.A[s], c.extra[s] if torch.is_tensor(c.extra) else c.extra
    if c.pre_out:
        pre1 = got["pre1"].double()
        worst = _hold(tag, "pre_out", got["pre1"], ref, A, K, c.fmt, 0.0, bad)
        worst = max(worst, _hold(tag, "y", got["C"], gelu64(pre1), torch.zeros_like(pre1), 0.0, c.fmt, eps_of(c.fmt, "gelu"), bad))
        if c.act == 2:
            worst = max(worst, _hold(tag, "gelu'", got["pre"], dgelu64(pre1), torch.zeros_like(pre1), 0.0, c.fmt, eps_of(c.fmt, "both"), bad))
    else:
        worst = _hold(tag, "C", got["C"], ref, A, K, c.out_fmt, extra, bad)
    if c.rowsum:
        worst = max(worst, _hold(tag, "rowsum", got["rowsum"], c.rs_ref[s], c.rs_A[s], c.rs_kacc if rs_kacc is None else rs_kacc, F32, 0.0, bad))
    return worst, bad


def line(c, family, width, worst):
    return "  %-7s w%-3d %-62s K_yard %6.3f  Kacc %6.2f  worst err / bound %6.3f" % (family, width, c.name(), c.k_yard, c.kacc, worst)


# ================================================================================================ pads and guards
class Slab:
    """A logical [rows, width] matrix at leading dimension width + pad inside an allocation with `guard` rows before and after
    (a vector: rows = 1, guard = 0: `pad` elements past its end)."""

    def __init__(self, rows, width, dtype, pad=PAD, guard=GUARD):
        self.rows, self.width, self.dtype, self.pad, self.guard, self.ld = rows, width, dtype, pad, guard, width + pad
        self.es = 4 if dtype == torch.float32 else 2
        assert (width * self.es) % 4 == 0 and (self.ld * self.es) % 4 == 0

    def poison(self):
        idt = torch.int32 if self.es == 4 else torch.int16
        return torch.full((self.rows + 2 * self.guard, self.ld), PATTERN if self.es == 4 else PATTERN & 0xFFFF, dtype=idt).view(self.dtype)

    def input(self, t):
        """The allocation of an input: NaN around the values."""
        buf = torch.full((self.rows + 2 * self.guard, self.ld), float("nan"), dtype=self.dtype)
        self.logical(buf).copy_(t.reshape(self.rows, self.width))
        return buf

    def output(self, prior=None):
        """The allocation of an output: the pattern everywhere, but for prior contents the call reads."""
        buf = self.poison()
        if prior is not None:
            self.logical(buf).copy_(prior.reshape(self.rows, self.width))
        return buf

    def logical(self, buf):
        return buf[self.guard:self.guard + self.rows, :self.width]

    def offset(self):
        """Elements from the start of the allocation to the first logical element."""
        return self.guard * self.ld

    def check(self, tag, buf, bad):
        """buf: the whole allocation on the host after the call."""
        idt = torch.int32 if self.es == 4 else torch.int16
        outside = torch.ones(buf.shape, dtype=torch.bool)
        self.logical(outside).fill_(False)
        touched = (buf.view(idt) != self.poison().view(idt)) & outside
        if bool(touched.any()):
            r, col = [int(x[0]) for x in torch.nonzero(touched, as_tuple=True)]
            bad.append("%s: %d pad / guard words were written, the first at allocation row %d (logical row %d), column %d"
                       % (tag, int(touched.sum()), r, r - self.guard, col))
        words = self.logical(buf).contiguous().view(torch.int32)
        if bool((words == PATTERN).any()):
            bad.append("%s: %d logical 32-bit words still carry the pattern (never written)" % (tag, int((words == PATTERN).sum())))
