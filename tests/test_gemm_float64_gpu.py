"""-m gpu: the GEMM kernels behind ecamp_gemm / ecamp_gemm_res32 -- the 128^2 kernels of csrc/gemm.hip, the eight-wave persistent kernel
of csrc/gemm_q8.h and the four-wave kernel of csrc/gemm_q16.h (192- and 256-column tiles, weight-gradient form) -- held to float64
element by element.  Reference, magnitudes, yardstick, bounds, regimes, case tables and the restated kernel selection are those of
tests/_gemm_ref.py (read its docstring first); tests/test_gemm_reference_cpu.py proves them without a GPU.

Every call
  * runs with every matrix at leading dimension width + 8 inside an allocation with 8 guard rows before and after, inputs surrounded by
    NaN (8 floats past bias[N] too), outputs -- C, pre_out, rowsum past M, the split-K workspace past its size -- by 0x5A5A5A5A, which
    also fills every logical element the call overwrites; afterwards every pad and guard word is intact, no logical word carries the
    pattern and nothing is NaN.  One dense call (leading dimension == width) per family and form keeps the wrap-around layout covered;
  * is forced to its family with the switches q8_mode / q16_mode / q16_wgrad (restored by the `switches` fixture) and proves what ran
    twice: by the launch counters (neither moving means the 128^2 kernel) and by the profiler tag name:form:e<epi>:M:N:K:w<tile>|s<split>,
    which must be the one _gemm_ref.route gives for this device's CU count -- and, on 256 CUs, the one written down by hand in
    _gemm_ref.INTENDED;
  * prints K_yard, Kacc and its worst err / bound (profiles/gemm_float64.txt is one run's output).
No element is left out of any judgement.

Out of scope: the e4m3 GEMM; the grouped weight-gradient launch (tests/test_gemm_q16_wgrad_gpu.py); the 2 GB split paths;
subnormal operands."""
import ctypes

import pytest
import torch

import _gemm_ref as G
from _gemm_ref import BF16, DTYPE, F16, F32, Case, Slab  # noqa: F401

pytestmark = pytest.mark.gpu


def _ops():
    from ecamp_amd import hip_ops
    return hip_ops


def _lib():
    from ecamp_amd import _lib as L
    return L.load()


def _fmt():
    from ecamp_amd import _lib as L
    return F16 if L.half() == "f16" else BF16


@pytest.fixture
def switches():
    """set(**switches) on the build in use; everything back to its default afterwards."""
    o = _ops()

    def set_(**kw):
        for k, v in kw.items():
            o.set_option(k, v)
    try:
        yield set_
    finally:
        set_(**G.DEFAULTS)


def _counts():
    lib = _lib()
    return int(lib.ecamp_gemm_q8_launches()), int(lib.ecamp_gemm_q16_launches())


def _tags():
    lib = _lib()
    n = int(lib.ecamp_prof_dump(None, 0))
    buf = ctypes.create_string_buffer(n + 16)
    lib.ecamp_prof_dump(buf, len(buf))
    return [ln.split()[0] for ln in buf.value.decode().splitlines() if ln.strip() and not ln.startswith("attn:")]   # attention tags its launches too


def _ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


class _Buf:
    """A Slab on the device."""

    def __init__(self, dev, slab, host):
        self.slab, self.t = slab, host.to(dev)

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + self.slab.offset() * self.slab.es)

    def host(self):
        return self.t.cpu()


_NULL = ctypes.c_void_p(0)


def run(dev, c, force, intended=None, pad=G.PAD, grid=None):
    """One call of the case `c` under the forced family -> (got, (family, width)): launches, proves what ran, checks every pad and guard."""
    from ecamp_amd import _lib as L
    o, lib = _ops(), _lib()
    M, N, K, form, dt = c.M, c.N, c.K, c.form, DTYPE[c.fmt]
    odt = DTYPE[c.out_fmt]
    ops = c.o
    a_st, b_st = (ops.a if form != "w" else ops.a.T), (ops.b if form == "f" else ops.b.T)

    def inp(t, dtype):
        s = Slab(t.shape[0], t.shape[1], dtype, pad=pad)
        return _Buf(dev, s, s.input(t.to(dtype)))

    def vec_in(t):
        s = Slab(1, t.numel(), torch.float32, guard=0)
        return _Buf(dev, s, s.input(t))

    A, B = inp(a_st, dt), inp(b_st, dt)
    cs = Slab(M, N, odt, pad=pad)
    C = _Buf(dev, cs, cs.output(ops.prior if c.accumulate else None))
    bias = vec_in(ops.bias) if c.has_bias else None
    res = None if c.res_kind is None else inp(ops.res, dt) if c.res_kind == "h" else inp(ops.res32, torch.float32)
    gm = inp(ops.gmul, dt) if c.has_gmul else None
    pre = None
    if c.pre_out:
        ps = Slab(M, N, dt, pad=pad)
        pre = _Buf(dev, ps, ps.output())
    rsum = None
    if c.rowsum:
        rs = Slab(1, M, torch.float32, guard=0)
        rsum = _Buf(dev, rs, rs.output(ops.rs_prior))
    ws = None
    if c.split > 1:
        assert int(lib.ecamp_gemm_workspace_bytes(M, N, K, c.split)) == c.split * M * N * 4
        wsl = Slab(1, c.split * M * N, torch.float32, guard=0)
        ws = _Buf(dev, wsl, wsl.output())
    adev = torch.tensor([c.alpha_dev], device=dev) if c.alpha_dev is not None else None
    p = lambda b: b.ptr() if b is not None else _NULL      # noqa: E731
    ld = lambda b: b.slab.ld if b is not None else 0       # noqa: E731

    q8_0, q16_0 = _counts()
    lib.ecamp_prof_collect(-1, None, None, None)
    lib.ecamp_prof_enable(1)
    try:
        if c.epi == "res32":
            L.call("ecamp_gemm_res32", A.ptr(), B.ptr(), C.ptr(), M, N, K, A.slab.ld, B.slab.ld, C.slab.ld, p(bias), p(res), ld(res), o.code(dt), o.stream())
        else:
            L.call("ecamp_gemm", A.ptr(), B.ptr(), C.ptr(), M, N, K, int(form != "w"), A.slab.ld, int(form == "f"), B.slab.ld, C.slab.ld, p(bias), p(res),
                   ld(res), p(pre), ld(pre), p(gm), ld(gm), c.act, float(c.alpha), ctypes.c_void_p(adev.data_ptr()) if adev is not None else _NULL,
                   o.code(dt), int(c.out_fmt == F32 and c.fmt != F32), int(c.accumulate), c.split, p(ws), p(rsum), o.stream())
        torch.cuda.synchronize()
    finally:
        lib.ecamp_prof_enable(0)
    tags = _tags()
    lib.ecamp_prof_collect(-1, None, None, None)
    q8_1, q16_1 = _counts()

    # what ran: the mirror for this device, the hand-written table on 256 CUs, the counters and the tag
    want = G.route(form, M, N, K, c.fmt, c.epi, split=c.split, rowsum=c.rowsum, force=force, ncu=_ncu(dev), pad=pad)
    if intended is not None and _ncu(dev) == 256:
        assert want == intended, (c.name(), force, want, intended)
    moved = {"t128": (0, 0), "q8": (1, 0), "q16": (0, 1)}[want[0]]
    assert (q8_1 - q8_0, q16_1 - q16_0) == moved, "%s forced %s: launch counters moved by %s, %s expected" % (c.name(), force, (q8_1 - q8_0, q16_1 - q16_0), want)
    assert tags == [G.tag_of(want[0], want[1], form, M, N, K, c.fmt, c.epi, c.split)], (c.name(), force, tags, want)

    bad, got = [], {}
    for name, b in (("C", C), ("pre", pre), ("rowsum", rsum)):
        if b is not None:
            h = b.host()
            b.slab.check("%s %s" % (c.name(), name), h, bad)
            got[name] = b.slab.logical(h).clone()
    if ws is not None:       # the workspace's own contents are the kernel's business; what lies past its size is not
        h = ws.host()
        assert bool((h[0, ws.slab.width:].view(torch.int32) == G.PATTERN).all()), "%s: the split-K workspace was overrun" % c.name()
    assert not bad, bad
    if c.rowsum:
        got["rowsum"] = got["rowsum"].reshape(-1)
    return got, want


def hold(c, got, want):
    worst, bad = G.judge(c, got)
    print(G.line(c, want[0], want[1], worst))
    assert not bad, bad


def run_forward(dev, fmt, force, shape, regime, epis, intended_of, dense_epi=None, yard_step=1):
    M, N, K = shape
    gelu = None
    for epi in epis:
        c = Case(fmt, "f", M, N, K, regime, epi, yard_step=yard_step)
        got, want = run(dev, c, force, intended_of(epi))
        if epi == "bias_gelu_pre":
            gelu = got
            got["pre1"] = got["pre"]
        if epi == "bias_der":     # the saved derivative: y must not depend on what is saved beside it, gelu' is judged from the act = 1 call's pre_out
            if gelu is None:
                gelu, _ = run(dev, Case(fmt, "f", M, N, K, regime, "bias_gelu_pre", yard_step=yard_step), force, intended_of("bias_gelu_pre"))
            assert torch.equal(got["C"].view(torch.int16), gelu["C"].view(torch.int16)), "act = 2 changed y"
            got["pre1"] = gelu["pre"]
        hold(c, got, want)
        if epi == dense_epi:
            got, want = run(dev, c, force, intended_of(epi), pad=0)
            hold(c, got, want)


# ---------------------------------------------------------------------------------------------------------------- base shape
@pytest.mark.parametrize("regime", G.REGIMES)
@pytest.mark.parametrize("K", G.BASE_KS)
@pytest.mark.parametrize("force", ["t128", "q8", "q16"])
def test_forward_epilogues(dev, both_halves, switches, force, K, regime):
    """264 x 264: 2 x 2 tiles of 256 (3 x 3 of 128; 192 + 72 columns on the four-wave kernel); K tiles: 2 exact, 3 with an 8-wide tail, 7
    (past the 5-slot ring).  bias + GELU without pre_out and out_f32 go to the 128^2 kernel whatever is forced (q8_epi refuses them), the
    GELU epilogues of the forced four-wave kernel to the eight-wave one."""
    switches(**G.FORCE[force])
    run_forward(dev, _fmt(), force, (G.BASE_M, G.BASE_N, K), regime, G.FWD_EPIS, lambda e: G.INTENDED["f"][force][e], dense_epi="bias" if K == 128 else None)


@pytest.mark.parametrize("regime", G.REGIMES)
@pytest.mark.parametrize("K", G.BASE_KS)
@pytest.mark.parametrize("force", ["t128", "q8", "q16"])
def test_data_gradient_epilogues(dev, both_halves, switches, force, K, regime):
    """dx = alpha alpha_dev dy w [* gelu'(gmul) | * gmul] [+ residual], w stored [K, N]: the four-wave kernel has the plain and residual
    forms, the gmul forms fall to the eight-wave kernel."""
    switches(**G.FORCE[force])
    fmt = _fmt()
    for epi in G.DGRAD_EPIS:
        c = Case(fmt, "d", G.BASE_M, G.BASE_N, K, regime, epi)
        got, want = run(dev, c, force, G.INTENDED["d"][force][epi])
        hold(c, got, want)
        if K == 128 and epi == "res":
            got, want = run(dev, c, force, G.INTENDED["d"][force][epi], pad=0)
            hold(c, got, want)


@pytest.mark.parametrize("regime", G.REGIMES)
def test_forward_epilogues_n_not_a_multiple_of_8(dev, both_halves, switches, regime):
    """133 x 260 x 72 on the 128^2 kernel (the only one that takes N % 8 != 0): groups of 4 past N, M a multiple of nothing."""
    switches(**G.FORCE["q16"])
    run_forward(dev, _fmt(), "q16", G.ODD, regime, G.FWD_EPIS, lambda e: G.INTENDED["odd"])


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("force", ["q8", "q16"])
def test_data_gradient_tile_walk_is_bit_identical(dev, both_halves, switches, force, grid):
    """q8_bwd_grid 1 / 3: one workgroup walks all four tiles of the base shape (three walk one or two): the same bits as the default grid,
    and the same bounds."""
    switches(**G.FORCE[force])
    fmt = _fmt()
    for epi in ("plain", "res") + (("gmul0",) if force == "q8" else ()):
        c = Case(fmt, "d", G.BASE_M, G.BASE_N, 136, "scales", epi)
        switches(q8_bwd_grid=0)
        base, want = run(dev, c, force, G.INTENDED["d"][force][epi])
        switches(q8_bwd_grid=grid)
        got, want2 = run(dev, c, force, G.INTENDED["d"][force][epi])
        assert want2 == want and torch.equal(got["C"].view(torch.int16), base["C"].view(torch.int16)), (force, grid, epi)
        hold(c, got, want)


# ---------------------------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("regime", G.REGIMES)
@pytest.mark.parametrize("K", G.WGRAD_KS)
@pytest.mark.parametrize("force", ["t128", "q8", "q16"])
def test_weight_gradient(dev, both_halves, switches, force, K, regime):
    """dW [264, 264] (f32) (+)= 0.75 dy^T x over K rows, both operands strided: split 1, the library's suggested split (17 at 4104: its
    last slice holds 8 rows, which the persistent kernels refuse -- the call falls to the 128^2 kernel, asserted) and split 8 (the
    persistent kernels' slabs and the split-K reduce); overwrite and accumulate onto nonzero prior contents; with and without the
    row sums (the bias gradient), which start from ones."""
    switches(**G.FORCE[force])
    fmt = _fmt()
    sug = max(1, int(_lib().ecamp_gemm_suggest_split(G.BASE_M, G.BASE_N, K, 0, 0, 1)))
    assert sug == G.suggest_split(G.BASE_M, G.BASE_N, K, "w", fmt, G.FORCE[force]["q8_mode"], ncu=_ncu(dev))
    if _ncu(dev) == 256:
        assert sug == G.SUGGESTED_SPLIT[K]
    assert (sug > 1) == (K == 4104)
    first = True
    for split, acc, rs in G.wgrad_calls(K):
        c = Case(fmt, "w", G.BASE_M, G.BASE_N, K, regime, "wgrad", split=split, accumulate=acc, rowsum=rs)
        got, want = run(dev, c, force, G.INTENDED["w"][force][(K, split)])
        hold(c, got, want)
        if first and K == 136:
            got, want = run(dev, c, force, G.INTENDED["w"][force][(K, split)], pad=0)
            hold(c, got, want)
        first = False


# ---------------------------------------------------------------------------------------------------------------- large shapes
@pytest.mark.parametrize("force", ["q8", "q16"])
def test_forward_tile_walk(dev, both_halves, switches, force):
    """32776 x 264 x 136: 258 tiles on either kernel (256- and 192-column tiles alike): on 256 CUs two workgroups walk two tiles each, the
    forward form's only walk below 12800 x 3072."""
    M, N, K = G.WALK
    tiles = G.cdiv(M, 256) * G.cdiv(N, G.INTENDED["walk"][force][1])
    if not tiles > _ncu(dev):
        pytest.skip("%d tiles on %d CUs: no workgroup walks a second tile" % (tiles, _ncu(dev)))
    switches(**G.FORCE[force])
    run_forward(dev, _fmt(), force, G.WALK, "plain", ("bias",), lambda e: G.INTENDED["walk"][force], yard_step=G.YARD_ROWS_LARGE)


@pytest.mark.parametrize("form,epi", G.WIDE_CASES)
def test_four_wave_256_column_tile(dev, both_halves, switches, form, epi):
    """32776 x 200 x 136: 129 tiles of 256 columns fit one round of 256 CUs where 258 of 192 need two, so q16_cost picks the 256-column form
    of the four-wave kernel -- gemm_bf16_q16_kernel<EPI, 8, B_KC>, which no smaller output reaches; the tag must say w256."""
    M, N, K = G.WIDE
    if not G.cdiv(M, 256) * G.cdiv(N, 256) <= _ncu(dev) < G.cdiv(M, 256) * G.cdiv(N, 192):
        pytest.skip("on %d CUs this shape does not take the 256-column tile" % _ncu(dev))
    switches(**G.FORCE["q16"])
    c = Case(_fmt(), form, M, N, K, "plain", epi, yard_step=G.YARD_ROWS_LARGE)
    got, want = run(dev, c, "q16", G.INTENDED["wide"])
    assert want == ("q16", 256)
    hold(c, got, want)


# ---------------------------------------------------------------------------------------------------------------- f32 operands
def test_f32_operands_on_the_128_kernel(dev, switches):
    """The f32 parity kernel (exact-f32 MFMA, erff GELU): its own short list, the persistent kernels forced and refused."""
    switches(**G.FORCE["q16"])
    for form, (M, N, K), epi in G.F32_CASES:
        c = Case(F32, form, M, N, K, "plain", epi)
        got, want = run(dev, c, "q16", G.INTENDED["f32"])
        if epi == "bias_gelu_pre":
            got["pre1"] = got["pre"]
        hold(c, got, want)
    for split, acc, rs in ((1, False, True), (G.SUGGESTED_SPLIT[4104], True, True)):
        c = Case(F32, "w", G.BASE_M, G.BASE_N, 4104, "plain", "wgrad", split=split, accumulate=acc, rowsum=rs)
        got, want = run(dev, c, "q16", G.INTENDED["f32"])
        hold(c, got, want)
