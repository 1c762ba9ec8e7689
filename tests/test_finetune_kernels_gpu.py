"""-m gpu: the four kernels of csrc/finetune.hip against float64 on the CPU.  Error is max |a - b| / max |b| unless a line says otherwise;
every case prints what it measured (recorded in profiles/finetune.txt)."""
import pytest
import torch
import torch.nn.functional as F

import _finetune_ref as R
from conftest import h16

pytestmark = pytest.mark.gpu


def worst(got, ref):
    """max |got - ref| / max |ref|"""
    ref = ref.double().cpu()
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------- cls_head_dgrad
DGRAD_GRID_CAP = 2048 * 256            # (sample, 16-byte vector) items one pass of the launch covers: B * D / 4 above it loops
DGRAD_SHAPES = [(B, C, D) for C in (1, 3, 64) for D in (64, 192, 1028) for B in (1, 5)] + [(32800, 3, 64)]


@pytest.mark.parametrize("B,C,D", DGRAD_SHAPES)
def test_cls_head_dgrad_against_float64(dev, B, C, D):
    from ecamp_amd import hip_ops as ops
    if B > 5:
        assert B * (D // 4) > DGRAD_GRID_CAP
    g = torch.Generator().manual_seed(B + 31 * C + D)
    dlogits, W = torch.randn(B, C, generator=g), torch.randn(C, D, generator=g)
    ref = dlogits.double() @ W.double()
    a = ops.cls_head_dgrad(dlogits.to(dev), W.to(dev))
    b = ops.cls_head_dgrad(dlogits.to(dev), W.to(dev))
    assert a.shape == (B, D) and a.dtype == torch.float32 and torch.equal(a, b), "two calls must give the same bits"
    e = worst(a, ref)
    print("[finetune] cls_head_dgrad B=%d C=%d D=%d: %.2e (bar 1e-6)" % (B, C, D, e))
    assert e <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- pool_norm_bwd
def _pool_case(B, T, D, t0, t1, dtype, affine, scale=1.0):
    """x on a coarse grid (1/64; 1/8 in 16 bits, where |x| <= 5 then needs 6 bits) whose token noise cancels in pairs: every float64 sum
    below is exact, so the mean over [t0, t1) IS the f32 `pooled` the kernel is handed, and what is compared is the backward's arithmetic
    alone.  -> (x, pooled f32, dfeat f32, gamma, beta,
    float64 references dx, dgamma, dbeta from autograd through layer_norm(x[:, t0:t1].mean(1)))."""
    g = torch.Generator().manual_seed(B * 1000 + T * 7 + D)
    q = 64 if dtype == torch.float32 else 8
    row = torch.randint(-4 * q, 4 * q + 1, (B, 1, D), generator=g).double() / q      # a few units per column
    n = t1 - t0
    half = torch.randint(-q, q + 1, (B, n // 2, D), generator=g).double() / q
    noise = torch.cat([half, -half] + ([torch.zeros(B, 1, D, dtype=torch.float64)] if n % 2 else []), dim=1)
    x = torch.zeros(B, T, D, dtype=torch.float64)
    x[:, t0:t1] = row + noise
    x[:, :t0] = 3.0                                                                  # rows outside the range: anything
    x[:, t1:] = -2.0
    assert torch.equal(x.to(dtype).double(), x)
    x = x.to(dtype)
    gamma = (1 + 0.5 * torch.randn(D, generator=g)) if affine else None
    beta = torch.randn(D, generator=g) if affine else None
    dfeat = torch.randn(B, D, generator=g) * scale
    xd = x.double().requires_grad_(True)
    gd = gamma.double().requires_grad_(True) if affine else None
    bd = beta.double().requires_grad_(True) if affine else None
    pooled = xd[:, t0:t1].mean(dim=1)
    F.layer_norm(pooled, (D,), gd, bd, 1e-6).backward(dfeat.double())
    assert torch.equal(pooled.detach().float().double(), pooled.detach()) and torch.equal(pooled.detach(), row[:, 0])   # exact, as promised
    if not affine:   # the identity affine's own gradients, for the kernel's dgamma / dbeta outputs
        xh = F.layer_norm(pooled.detach(), (D,), None, None, 1e-6)
        dg, db = (dfeat.double() * xh).sum(0), dfeat.double().sum(0)
    else:
        dg, db = gd.grad, bd.grad
    return x, pooled.detach().float(), dfeat, gamma, xd.grad, dg, db


def _run_pool_bwd(dev, case, t0, t1, T, dtype):
    from ecamp_amd import hip_ops as ops
    x, pooled, dfeat, gamma, dx_ref, dg_ref, db_ref = case
    args = (dfeat.to(dev), pooled.to(dev), gamma.to(dev) if gamma is not None else None, t0, t1, T, 1e-6, dtype)
    a, b = ops.pool_norm_bwd(*args), ops.pool_norm_bwd(*args)
    for u, v in zip(a, b):
        assert torch.equal(u, v), "two calls must give the same bits"
    dx, dg, db = a
    assert dx.shape == dx_ref.shape and dx.dtype == dtype and dg.dtype == db.dtype == torch.float32
    out = torch.ones(T, dtype=torch.bool)
    out[t0:t1] = False
    assert torch.all(dx.cpu()[:, out] == 0), "rows outside [t0, t1) must be exactly zero"
    assert torch.all(dx_ref[:, out] == 0)
    return dx, dg, db


PNB_STORE_GRID_CAP, PNB_ROW_GRID_CAP = 2048, 256   # workgroups of the dx store / of the per-sample stage: B = 2100 is above both


@pytest.mark.parametrize("B,T,D,t0,t1,affine", [(3, 5, 64, 1, 5, True), (2, 197, 192, 1, 197, True), (2, 9, 64, 0, 9, False), (2100, 3, 64, 1, 3, True)])
def test_pool_norm_bwd_in_f32_against_float64_autograd(dev, B, T, D, t0, t1, affine):
    assert B <= 3 or B > max(PNB_STORE_GRID_CAP, PNB_ROW_GRID_CAP)
    case = _pool_case(B, T, D, t0, t1, torch.float32, affine)
    dx, dg, db = _run_pool_bwd(dev, case, t0, t1, T, torch.float32)
    e = (worst(dx, case[4]), worst(dg, case[5]), worst(db, case[6]))
    print("[finetune] pool_norm_bwd f32 B=%d T=%d D=%d [%d,%d) %s: dx %.2e dgamma %.2e dbeta %.2e (bar 2e-6)"
          % (B, T, D, t0, t1, "affine" if affine else "null affine", *e))
    assert max(e) <= 2e-6


@pytest.mark.parametrize("B,T,D,t0,t1", [(2, 197, 192, 1, 197), (2, 50, 772, 1, 50)])
def test_pool_norm_bwd_in_16_bits_is_one_rounding_of_each_element(dev, both_halves, B, T, D, t0, t1):
    """dx in the build's 16-bit format: every element within one rounding of the format -- 2^-8 (bf16) / 2^-11 (half) -- of ITS float64
    value.  The upstream gradient carries a factor 2^16, as a loss-scaled one does, which keeps IEEE half's dx in its normal range; that
    is asserted on the float64 side."""
    dtype = h16()
    case = _pool_case(B, T, D, t0, t1, dtype, True, scale=65536.0)
    dx, dg, db = _run_pool_bwd(dev, case, t0, t1, T, dtype)
    ref = case[4][:, t0:t1]
    assert float(ref.abs().min()) >= 2.0 ** -14 and float(ref.abs().max()) < 6e4
    bar = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    err = float(((dx.double().cpu()[:, t0:t1] - ref).abs() / ref.abs()).max())
    e = (worst(dg, case[5]), worst(db, case[6]))
    print("[finetune] pool_norm_bwd %s B=%d T=%d D=%d: dx worst per-element relative error %.2e (bar %.2e) dgamma %.2e dbeta %.2e (bar 2e-6)"
          % (str(dtype).split(".")[-1], B, T, D, err, bar, *e))
    assert err <= bar and max(e) <= 2e-6


def test_pool_norm_bwd_is_the_backward_of_the_forward_kernel(dev):
    """The pair as PoolNormFn uses it: `pooled` from ecamp_pool_norm itself on a random 16-bit x."""
    from ecamp_amd import hip_ops as ops
    B, T, D = 3, 50, 192
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, T, D, generator=g).to(h16())
    gamma, beta, dfeat = 1 + 0.3 * torch.randn(D, generator=g), torch.randn(D, generator=g), torch.randn(B, D, generator=g)
    pooled, _ = ops.pool_norm(x.to(dev), 1, T, gamma.to(dev), beta.to(dev), 1e-6)
    dx, dg, db = ops.pool_norm_bwd(dfeat.to(dev), pooled, gamma.to(dev), 1, T, T, 1e-6, torch.float32)
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.layer_norm(xd[:, 1:].mean(1), (D,), gd, bd, 1e-6).backward(dfeat.double())
    e = (worst(dx, xd.grad), worst(dg, gd.grad), worst(db, bd.grad))
    print("[finetune] pool_norm -> pool_norm_bwd: dx %.2e dgamma %.2e dbeta %.2e (bar 1e-5: `pooled` is an f32 mean)" % e)
    assert max(e) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- sumsq_grouped + sgd_grouped
SGD_GRID_CAP = 8192 * 256 * 4          # elements one grid-stride pass of ecamp_sgd_grouped covers
SUMSQ_PASS = 2048 * 256 * 4 * 4        # ... and one unrolled pass of ecamp_sumsq_grouped (2048 slots x 256 threads x four 16-byte loads)


def _steps(dev, p0, grads, table, max_norm, p16_dtype=None, grad_scale=1.0, ctl=None, wds=R.GROUP_WD):
    """Run the fused step once per gradient from (p0, zero momentum) -> (p, buf, p16 or None, [norm per step]) on the CPU."""
    from ecamp_amd import hip_ops as ops
    n = p0.numel()
    p, buf, tab = p0.to(dev).clone(), torch.zeros(n, device=dev), table.to(dev)
    p16 = torch.full((n,), 7.0, device=dev, dtype=p16_dtype) if p16_dtype is not None else None
    slots = ops.sumsq_grouped_slots(n)
    assert 1 <= slots <= ops.SUMSQ_MAX_SLOTS
    partials = torch.full((slots + 3,), float("nan"), device=dev)      # (a launch fills exactly `slots`: the rest stays NaN and unread)
    norm_out = torch.full((1,), -1.0, device=dev)
    norms = []
    for g in grads:
        assert ops.sumsq_grouped(g.to(dev), tab, partials) == slots
        ops.sgd_grouped(p, g.to(dev), buf, p16, tab, R.GROUP_LR, wds, R.MOMENTUM, max_norm, partials, slots, grad_scale, ctl, norm_out)
        norms.append(float(norm_out.item()))
    assert bool(torch.isnan(partials[slots:]).all()) and not bool(torch.isnan(partials[:slots]).any())
    return p.cpu(), buf.cpu(), (p16.cpu() if p16 is not None else None), norms


def _reference(p0, grads, table, max_norm, dtype, wds=R.GROUP_WD, grad_scale=1.0):
    p, buf = p0.to(dtype).clone(), torch.zeros_like(p0, dtype=dtype)
    out = [R.clip_sgd_step(p, g, buf, table, R.GROUP_LR, wds, R.MOMENTUM, max_norm, grad_scale) for g in grads]
    return p, buf, [o[0] for o in out], [o[1] for o in out]


def test_four_clipped_sgd_steps_against_float64_with_torchs_float32_as_the_yardstick(dev, both_halves):
    n = 64 * 40
    table = R.block_table(40, seed=1)
    live = R.element_groups(table) < 8
    assert set(table.tolist()) == {0, 1, 2, R.FROZEN}
    p0, grads = R.trajectory(n, steps=4, seed=2)
    norms0 = [float(torch.sqrt((g[live].double() ** 2).sum())) for g in grads]
    max_norm = R.f32((norms0[1] * norms0[2]) ** 0.5)
    p64, buf64, norms64, coefs64 = _reference(p0, grads, table, max_norm, torch.float64)
    assert coefs64[0] < 1.0 and coefs64[-1] == 1.0, "the first step must clip and a later one must not"
    # the yardstick: the same four steps by torch itself in float32 on the CPU
    p32, buf32, _, _ = R.torch_clip_sgd(p0, grads, table, R.GROUP_LR, R.GROUP_WD, R.MOMENTUM, max_norm, torch.float32)
    yp, yb = worst(p32[live], p64[live]), worst(buf32[live], buf64[live])
    p, buf, p16, norms = _steps(dev, p0, grads, table, max_norm, p16_dtype=h16())
    ep, eb = worst(p[live], p64[live]), worst(buf[live], buf64[live])
    en = max(abs(a - b) / b for a, b in zip(norms, norms64))
    print("[finetune] sgd_grouped 4 steps: p %.2e (torch f32 %.2e) buf %.2e (torch f32 %.2e) norm %.2e (bar 1e-5); coefficients %s"
          % (ep, yp, eb, yb, en, ["%.3f" % c for c in coefs64]))
    assert yp > 0 and yb > 0
    assert ep <= 4 * yp and eb <= 4 * yb
    assert en <= 1e-5
    assert torch.equal(p16[live], p[live].to(h16())), "the 16-bit shadow is the master, cast"
    # blocks of group 255 keep their bits: parameter, momentum, shadow
    assert torch.equal(p[~live], p0[~live]) and torch.all(buf[~live] == 0) and torch.all(p16[~live] == 7.0)
    assert float((p[live] - p0[live]).abs().max()) > 1e-2
    again = _steps(dev, p0, grads, table, max_norm, p16_dtype=h16())
    assert torch.equal(again[0], p) and torch.equal(again[1], buf) and torch.equal(again[2], p16) and again[3] == norms, "two runs, the same bits"


def test_ctl_replaces_the_gradient_scale_and_its_skip_flag_leaves_every_byte_alone(dev):
    n = 64 * 40
    table = R.block_table(40, seed=1)
    p0, grads = R.trajectory(n, steps=2, seed=3)
    grads = [g * 2 for g in grads]
    max_norm = 20.0
    want = _steps(dev, p0, grads, table, max_norm, p16_dtype=torch.bfloat16, grad_scale=0.5)
    ctl = torch.tensor([0.5, 0.0, 9.0, 9.0], device=dev)
    got = _steps(dev, p0, grads, table, max_norm, p16_dtype=torch.bfloat16, grad_scale=123.0, ctl=ctl)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]) and got[3] == want[3]
    p64, _, norms64, _ = _reference(p0, grads, table, max_norm, torch.float64, grad_scale=0.5)
    live = R.element_groups(table) < 8
    assert worst(got[0][live], p64[live]) <= 1e-5 and abs(got[3][0] - norms64[0]) / norms64[0] <= 1e-5    # (the scale took effect)
    skip = torch.tensor([0.5, 1.0, 9.0, 9.0], device=dev)
    p, buf, p16, norms = _steps(dev, p0, grads, table, max_norm, p16_dtype=torch.bfloat16, ctl=skip)
    assert torch.equal(p, p0) and torch.all(buf == 0) and torch.all(p16 == 7.0) and norms == [-1.0, -1.0]


def test_no_clipping_without_a_max_norm_and_two_launches_share_one_partials_buffer(dev):
    """max_norm = 0 leaves the gradients alone; an arena and a tail buffer fill disjoint ranges of one partials buffer and see ONE norm."""
    from ecamp_amd import hip_ops as ops
    na, nt = 64 * 40, 64 * 6
    ta, tt = R.block_table(40, seed=1), R.block_table(6, seed=2)
    pa, ga = R.trajectory(na, steps=1, seed=5)
    pt, gt = R.trajectory(nt, steps=1, seed=6)
    live_a, live_t = R.element_groups(ta) < 8, R.element_groups(tt) < 8
    p, buf, _, norms = _steps(dev, pa, ga, ta, 0.0)
    p64, buf64, norms64, coefs = _reference(pa, ga, ta, 0.0, torch.float64)
    assert coefs == [1.0] and worst(p[live_a], p64[live_a]) <= 1e-6 and abs(norms[0] - norms64[0]) / norms64[0] <= 1e-5
    # the joint step against float64 over the concatenation
    table, p0, g = torch.cat([ta, tt]), torch.cat([pa, pt]), torch.cat([ga[0], gt[0]])
    live = torch.cat([live_a, live_t])
    max_norm = R.f32(0.5 * float(torch.sqrt((g[live].double() ** 2).sum())))
    q64, b64, n64, c64 = _reference(p0, [g], table, max_norm, torch.float64)
    assert c64[0] < 1.0
    sa, st = ops.sumsq_grouped_slots(na), ops.sumsq_grouped_slots(nt)
    partials = torch.zeros(sa + st, device=dev)
    bufs = [(pa.to(dev).clone(), ga[0].to(dev), torch.zeros(na, device=dev), ta.to(dev)), (pt.to(dev).clone(), gt[0].to(dev), torch.zeros(nt, device=dev), tt.to(dev))]
    ops.sumsq_grouped(bufs[0][1], bufs[0][3], partials)
    ops.sumsq_grouped(bufs[1][1], bufs[1][3], partials[sa:])
    norm = torch.zeros(2, device=dev)
    for k, (pp, gg, bb, tb) in enumerate(bufs):
        ops.sgd_grouped(pp, gg, bb, None, tb, R.GROUP_LR, R.GROUP_WD, R.MOMENTUM, max_norm, partials, sa + st, 1.0, None, norm[k:k + 1])
    got = torch.cat([bufs[0][0].cpu(), bufs[1][0].cpu()])
    assert float(norm[0]) == float(norm[1]) and abs(float(norm[0]) - n64[0]) / n64[0] <= 1e-5
    e = worst(got[live], q64[live])
    print("[finetune] arena + tail, one norm: p %.2e" % e)
    assert e <= 1e-6


def test_one_step_over_more_elements_than_one_grid_stride_pass(dev):
    """n = 64 * 140000 = 8 960 000 elements: above the 8192 x 256 x 4 = 8 388 608 one pass of ecamp_sgd_grouped covers, and above the
    8 388 608 of ecamp_sumsq_grouped's unrolled pass -- both kernels loop, the second through its remainder loop as well."""
    nblk = 140000
    n = 64 * nblk
    assert n > SGD_GRID_CAP and n > SUMSQ_PASS and n < 2 * SGD_GRID_CAP
    table = R.block_table(nblk, seed=7)
    live = R.element_groups(table) < 8
    p0, grads = R.trajectory(n, steps=1, seed=8)
    max_norm = R.f32(0.5 * float(torch.sqrt((grads[0][live].double() ** 2).sum())))
    p64, buf64, norms64, coefs = _reference(p0, grads, table, max_norm, torch.float64)
    assert coefs[0] < 1.0
    p32, buf32, _, _ = R.torch_clip_sgd(p0, grads, table, R.GROUP_LR, R.GROUP_WD, R.MOMENTUM, max_norm, torch.float32)
    yp, yb = worst(p32[live], p64[live]), worst(buf32[live], buf64[live])
    p, buf, _, norms = _steps(dev, p0, grads, table, max_norm)
    ep, eb, en = worst(p[live], p64[live]), worst(buf[live], buf64[live]), abs(norms[0] - norms64[0]) / norms64[0]
    print("[finetune] sgd_grouped n=%d: p %.2e (torch f32 %.2e) buf %.2e (torch f32 %.2e) norm %.2e" % (n, ep, yp, eb, yb, en))
    assert ep <= 4 * yp and eb <= 4 * yb and en <= 1e-5
    assert torch.equal(p[~live], p0[~live]) and torch.all(buf[~live] == 0)
    # the tail of the buffer was reached: the last live block moved
    assert table[-1] == 2 and float((p[-64:] - p0[-64:]).abs().max()) > 0
