"""-m gpu: the kernels every training step ends with -- csrc/optim.hip, csrc/elementwise.hip and scaled_accum_kernel of csrc/vision.hip --
against float64 / plain PyTorch on the CPU, at the sizes production hands them: ABOVE the grid cap of each grid-stride kernel (so that
the stride expression runs, with a partial last trip), at ragged edges, on both 16-bit builds.

The optimizer kernels are held to tests/_optim_ref.py (proven against torch in tests/test_optim_reference_cpu.py).  Their bound is not a
number: torch.optim.AdamW in float32 on the CPU is run on the same inputs, its distance from the float64 reference is the yardstick, and
the kernel may be at most 4x as far (it orders its operations differently: * 1/sqrt(bc2) for torch's division, (lr / bc1) * (m / denom)
for addcdiv -- a few ulp per step against a yardstick that is itself ~0.5 ulp(p) per step accumulated).  Measured on an MI355X
(profiles/optim_kernel_vs_f32_yardstick.txt): see the docstring of test_adamw_grouped_trajectory.
"""
import fractions
import functools
import math

import numpy as np
import pytest
import torch

import _optim_ref as R
from conftest import h16
from test_kernels_gpu import DT, TOL, check, rnd

pytestmark = pytest.mark.gpu

SMALL = 3 * 50 * 768                      # what test_small_ops hands the flat kernels: one partial trip
MID = 64 * 128 * 768                      # 1.5 trips of the 4096-block grid (4 194 304 elements per trip)
BIG = 5 * 4194304 // 2 + 4 * 11           # 2.5 trips and a ragged tail
FLAT = [SMALL, MID, BIG]


def ops():
    from ecamp_amd import hip_ops
    return hip_ops


def hip_error():
    from ecamp_amd._lib import EcampHipError
    return EcampHipError


def bits(t):
    """The tensor's bytes as integers: equality that sees NaN payloads and the sign of zero."""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


@functools.lru_cache(maxsize=None)
def _randn(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def flat(n, seed, dtype):
    """n seeded normal values, pre-rounded to `dtype` (so that only the kernel's own rounding is measured), as float32 on the CPU."""
    return rnd(_randn(BIG, seed)[:n], dtype)


# ================================================================================================ B. AdamW
RATIO = 4.0   # the kernel may be this many times as far from float64 as torch's float32 AdamW is (module docstring)


class _Host:
    """The host side of one AdamW case, computed once and shared by both builds: the float64 reference and the float32 yardstick after
    every step in `check_at`.  `single` = the ecamp_adamw entry point: one group, no table."""

    def __init__(self, nblocks, steps, check_at, seed, single=False):
        self.n, self.steps, self.check_at, self.seed, self.single = nblocks * 64, steps, check_at, seed, single
        n = self.n
        self.table = torch.zeros(nblocks, dtype=torch.uint8) if single else R.make_table(nblocks, seed)
        self.wds = [R.f32(0.05)] if single else list(R.GROUP_WD)
        self.p0, self.mag = R.make_params(n, seed + 1), R.make_magnitudes(n, seed + 2)
        self.sel = R.element_groups(self.table) < 8
        p, m, v = self.p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        yard = R.TorchGroupedAdamW(self.p0, self.table, self.wds, R.B1, R.B2, R.EPS, torch.float32)
        self.ref, self.yard, self.sumsq = {}, {}, {}
        for t in range(1, steps + 1):
            g, lrs = self.grad(t), self.lrs(t)
            self.sumsq[t] = R.ref_adamw_grouped(p, g, m, v, self.table, lrs, self.wds, R.B1, R.B2, R.EPS, t, 1.0)
            yard.step(g, lrs)
            if t in check_at:
                self.ref[t] = (p.clone(), m.clone(), v.clone())
                self.yard[t] = R.distances(*yard.arena(self.p0), self.ref[t], self.sel)

    def lrs(self, t):
        return R.group_lrs(t, self.steps)[:1] if self.single else R.group_lrs(t, self.steps)

    def grad(self, t):
        g = R.make_grad(self.mag, self.seed + 3, t)
        return g if self.single else R.plant_nonfinite(g, self.table)


@functools.lru_cache(maxsize=3)
def _host(nblocks, steps, check_at, seed, single=False):
    return _Host(nblocks, steps, check_at, seed, single)


class _Device:
    """p, m, v, the 16-bit shadow and the table on the device.  The shadow starts as random bits, the moments of frozen blocks as NaN / -0
    patterns: whatever a frozen block holds must come back bit for bit."""

    def __init__(self, H, dev):
        self.H, self.dev = H, dev
        g = torch.Generator().manual_seed(H.seed + 9)
        self.p = H.p0.to(dev)
        m0, v0 = torch.zeros(H.n), torch.zeros(H.n)
        m0[~H.sel], v0[~H.sel] = float("nan"), -0.0
        self.m, self.v = m0.to(dev), v0.to(dev)
        self.p16 = torch.randint(-32768, 32767, (H.n,), generator=g, dtype=torch.int16).view(h16()).to(dev)
        self.table = H.table.to(dev)
        self.before = [bits(t)[~H.sel] for t in (self.p, self.m, self.v, self.p16)]

    def step(self, t, **kw):
        H, o = self.H, ops()
        g = H.grad(t).to(self.dev)
        if H.single:
            o.adamw(self.p, g, self.m, self.v, self.p16, H.lrs(t)[0], R.B1, R.B2, R.EPS, H.wds[0], t)
            return None
        start = R.f32(0.5 * H.sumsq[t])        # grad_sumsq ACCUMULATES: it starts from a value of the size of what it is about to gather
        ss = torch.full((1,), start, device=self.dev)
        o.adamw_grouped(self.p, g, self.m, self.v, self.p16, self.table, H.lrs(t), H.wds, R.B1, R.B2, R.EPS, t, grad_sumsq=ss, **kw)
        return float(ss) - start

    def compare(self, t, tag, gathered=None):
        """Everything that must hold after a step: the three distances against 4x the yardstick, the frozen blocks, the shadow, the sum."""
        H = self.H
        p, m, v, p16 = self.p.cpu(), self.m.cpu(), self.v.cpu(), self.p16.cpu()
        for name, now, was in zip(("p", "m", "v", "p16"), (p, m, v, p16), self.before):
            assert torch.equal(bits(now)[~H.sel], was), "%s step %d: frozen blocks of %s changed" % (tag, t, name)
        assert torch.equal(bits(p16)[H.sel], bits(p.to(h16()))[H.sel]), "%s step %d: the 16-bit shadow is not p rounded once" % (tag, t)
        assert torch.isfinite(p).all() and torch.isfinite(m[H.sel]).all() and torch.isfinite(v[H.sel]).all()
        dk = R.distances(p.double(), m.double(), v.double(), H.ref[t], H.sel)
        ratios = [k / y for k, y in zip(dk, H.yard[t])]
        print("  %-22s step %3d  kernel/yardstick  p %.2e/%.2e = %.2f   m %.2e/%.2e = %.2f   v %.2e/%.2e = %.2f"
              % (tag, t, dk[0], H.yard[t][0], ratios[0], dk[1], H.yard[t][1], ratios[1], dk[2], H.yard[t][2], ratios[2]))
        for name, k, y in zip("pmv", dk, H.yard[t]):
            assert k <= RATIO * y, "%s step %d: %s is %.3e from float64, torch's float32 AdamW %.3e (x%.1f > x%.0f)" % (tag, t, name, k, y, k / y, RATIO)
        if gathered is not None:
            assert abs(gathered - H.sumsq[t]) <= 1e-5 * H.sumsq[t], "%s step %d: grad_sumsq %.9g, reference %.9g" % (tag, t, gathered, H.sumsq[t])
        return ratios


TRAJ = (4099, 50, (1, 2, 3, 10, 50), 11)    # 262 336 elements, 50 steps


def test_adamw_grouped_trajectory(dev, both_halves):
    """ecamp_adamw_grouped, the production optimizer, over 50 steps of a warm-up + cosine schedule on five groups (+ frozen runs, a
    group index beyond the groups, the edge byte 8), p / m / v carried on the device, compared after steps 1, 2, 3, 10 and 50.

    Measured on an MI355X, both builds alike (the 16-bit format only touches the shadow), kernel / yardstick distance from float64:
        step  1: p 5.11e-09 / 8.33e-09 = 0.61   m 5.68e-08 / 5.68e-08 = 1.00   v 1.02e-07 / 1.02e-07 = 1.00
        step 10: p 2.47e-08 / 2.47e-08 = 1.00   m 1.88e-07 / 2.07e-07 = 0.91   v 2.15e-07 / 2.93e-07 = 0.74
        step 50: p 5.23e-08 / 7.69e-08 = 0.68   m 2.76e-07 / 2.92e-07 = 0.94   v 3.95e-07 / 5.89e-07 = 0.67
    Over every case of this file (21 M elements, ecamp_adamw, the gradient-scale runs) the largest ratios were p 1.00, m 1.09, v 1.00
    against the bound of 4: the kernel is as close to float64 as torch's own float32 step.  Every line: profiles/optim_kernel_vs_f32_yardstick.txt."""
    H = _host(*TRAJ)
    D = _Device(H, dev)
    for t in range(1, H.steps + 1):
        gathered = D.step(t)
        if t in H.check_at:
            D.compare(t, "grouped " + both_halves, gathered)


def test_adamw_grouped_above_the_grid_cap(dev, both_halves):
    """n = 2.5 x 8 388 608 + 64 x 37: every trip of the stride loop of the 8192-block grid and a partial last one, three steps, each
    compared in full (the float64 reference works through the arena in chunks on the host)."""
    H = _host((5 * 8388608 // 2) // 64 + 37, 3, (1, 2, 3), 21)
    assert H.n == 20973888
    D = _Device(H, dev)
    for t in (1, 2, 3):
        D.compare(t, "grouped 21M " + both_halves, D.step(t))


@pytest.mark.parametrize("nblocks,steps,check_at", [(4099, 20, (1, 2, 3, 10, 20)), (MID // 64, 2, (1, 2))])
def test_adamw_single_group_entry_point(dev, both_halves, nblocks, steps, check_at):
    """ecamp_adamw through the same harness (one group, weight decay 0.05): a trajectory, and 1.5 trips of its 4096-block grid."""
    H = _host(nblocks, steps, check_at, 31, True)
    D = _Device(H, dev)
    for t in range(1, steps + 1):
        D.step(t)
        if t in check_at:
            D.compare(t, "single %d %s" % (H.n, both_halves))


def test_adamw_grouped_gradient_scale_host_and_ctl(dev, both_halves):
    """The loss scale reaches the kernel two ways and both must give the same bits: grad_scale = 1/65536 from the host, and ctl =
    [1/65536, 0, bc1, 1/sqrt(bc2)] from the device -- the latter with a WRONG host step and grad_scale, which ctl overrides.  Gradients
    are pre-multiplied by 65536 (exact), so both must also match the reference on the unscaled gradients, m and v included."""
    H = _host(*TRAJ)
    A, B = _Device(H, dev), _Device(H, dev)
    o = ops()
    for t in (1, 2, 3):
        g = (H.grad(t) * 65536.0).to(dev)
        got = []
        for D, kw in ((A, dict(step=t, grad_scale=1.0 / 65536.0)),
                      (B, dict(step=7, grad_scale=123.0, ctl=torch.tensor([1.0 / 65536.0, 0.0, 1.0 - R.B1 ** t, 1.0 / math.sqrt(1.0 - R.B2 ** t)], device=dev)))):
            ss = torch.full((1,), 3.0, device=dev)
            o.adamw_grouped(D.p, g, D.m, D.v, D.p16, D.table, H.lrs(t), H.wds, R.B1, R.B2, R.EPS, grad_sumsq=ss, **kw)
            got.append(float(ss) - 3.0)
        for name in ("p", "m", "v", "p16"):
            assert torch.equal(bits(getattr(A, name)), bits(getattr(B, name))), "step %d: %s differs between grad_scale and ctl" % (t, name)
        # (the two sums are NOT compared bit for bit: 8192 blocks add into grad_sumsq with float atomics, in whatever order they finish)
        A.compare(t, "grad_scale " + both_halves, got[0])
        B.compare(t, "ctl " + both_halves, got[1])


def test_adamw_grouped_skipped_step_writes_nothing(dev, both_halves):
    H = _host(*TRAJ)
    D = _Device(H, dev)
    D.step(1)
    D.m[5], D.v[6], D.p[7] = float("nan"), -0.0, -0.0      # in updated blocks: a skipped step may not even normalise them
    ss = torch.tensor([-0.0], device=dev)
    before = [bits(t) for t in (D.p, D.m, D.v, D.p16, ss)]
    ctl = torch.tensor([1.0 / 65536.0, 1.0, 0.5, 2.0], device=dev)
    ops().adamw_grouped(D.p, H.grad(2).to(dev), D.m, D.v, D.p16, D.table, H.lrs(2), H.wds, R.B1, R.B2, R.EPS, 2, grad_sumsq=ss, ctl=ctl)
    for name, now, was in zip(("p", "m", "v", "p16", "grad_sumsq"), (D.p, D.m, D.v, D.p16, ss), before):
        assert torch.equal(bits(now), was), "ctl[1] = 1: %s changed" % name


def test_adamw_grouped_refuses_bad_arguments(dev):
    o, z = ops(), torch.zeros(128, device=dev)
    tb = torch.zeros(2, dtype=torch.uint8, device=dev)
    with pytest.raises(hip_error()):
        o.adamw_grouped(z[:100], z[:100], z[:100], z[:100], None, tb, [1e-3], [0.0], R.B1, R.B2, R.EPS, 1)     # n % 64
    with pytest.raises(hip_error()):
        o.adamw_grouped(z, z, z, z, None, tb, [1e-3] * 9, [0.0] * 9, R.B1, R.B2, R.EPS, 1)                     # nine groups
    with pytest.raises(hip_error()):
        o.adamw_grouped(z, z, z, z, None, tb, [1e-3], [0.0], R.B1, R.B2, R.EPS, 0)                             # step 0


# ================================================================================================ C. sumsq
SUMSQ_BIG = 5 * 2097152 // 2 + 4 * 13     # 2.5 trips of the 2048-block grid and a ragged tail


@functools.lru_cache(maxsize=None)
def _sumsq_input(n):
    g = torch.Generator().manual_seed(41)
    x = torch.pow(10.0, torch.rand(n, generator=g, dtype=torch.float64) * 9.0 - 6.0).float()
    return x * (torch.randint(0, 2, (n,), generator=g).float() * 2.0 - 1.0)


@pytest.mark.parametrize("n", [4096 * 3, SUMSQ_BIG])
def test_sumsq_against_float64(dev, n):
    x = _sumsq_input(n)
    ref = float((x.double() ** 2).sum())
    start = R.f32(0.5 * ref)
    s = torch.full((1,), start, device=dev)
    ops().sumsq(x.to(dev), s)
    got = float(s) - start
    print("  sumsq n=%d: rel err %.2e (tol 1e-5)" % (n, abs(got - ref) / ref))
    assert abs(got - ref) <= 1e-5 * ref


@pytest.mark.parametrize("n", [4096 * 3, SUMSQ_BIG])
def test_sumsq_one_nonfinite_element_makes_the_sum_nonfinite(dev, n):
    """What the device-side GradScaler rests on: one inf, -inf or nan anywhere -- first element, last element, an element that only the
    second trip of the stride loop reaches -- and the result is not finite."""
    xd = _sumsq_input(n).to(dev)
    where = [0, n - 1] + ([2097152 + 12345] if n > 2097152 else [n // 2 + 1])
    for bad in (float("inf"), float("-inf"), float("nan")):
        for i in where:
            y = xd.clone()
            y[i] = bad
            s = torch.full((1,), 5.0, device=dev)
            ops().sumsq(y, s)
            assert not math.isfinite(float(s)), "sumsq missed %r at element %d of %d" % (bad, i, n)


def test_sumsq_refuses_a_length_that_is_not_a_multiple_of_four(dev):
    with pytest.raises(hip_error()):
        ops().sumsq(torch.zeros(1022, device=dev), torch.zeros(1, device=dev))


# ================================================================================================ D. the device-side GradScaler
class _Scaler:
    """state[4] | opt_step[1] | ctl[4] | norm[1] | sumsq[1] in ONE device buffer, so that a step is one launch and one read-back."""

    def __init__(self, dev, scale, tracker=0.0, skipped=0.0, opt_step=0.0, ctl23=(-7.0, -9.0)):
        self.buf = torch.tensor([scale, tracker, skipped, 0.0, opt_step, 0.0, 0.0, ctl23[0], ctl23[1], 0.0, 0.0], device=dev)
        self.state, self.opt_step, self.ctl, self.norm, self.sumsq = self.buf[0:4], self.buf[4:5], self.buf[5:9], self.buf[9:10], self.buf[10:11]

    def step(self, s, growth, backoff, interval, norm=True):
        self.sumsq.fill_(s)
        ops().loss_scale_update(self.sumsq, self.state, self.opt_step, self.ctl, self.norm if norm else None, growth, backoff, interval, R.B1, R.B2)
        b = self.buf.tolist()
        return tuple(b[0:3]), b[4], b[5:9], b[9]


def _same(a, b):
    return a == b or (a != a and b != b)


def _check_scaler_step(tag, got, want, ctl_before):
    (state, opt_step, ctl, norm), (rstate, rstep, rctl, rnorm) = got, want
    assert state == rstate and opt_step == rstep, "%s: state %r step %r, reference %r %r" % (tag, state, opt_step, rstate, rstep)
    assert _same(ctl[0], rctl[0]) and ctl[1] == rctl[1], (tag, ctl, rctl)
    if rctl[1]:
        assert ctl[2:] == ctl_before[2:], "%s: a skipped step rewrote the bias corrections" % tag
        assert not math.isfinite(norm), tag
    else:
        for k in (2, 3):   # computed in double and rounded once by the kernel: within 1 ulp of float32 of the float64 value
            assert abs(ctl[k] - rctl[k]) <= R.ulp32(rctl[k]), "%s: ctl[%d] = %.9g, reference %.17g" % (tag, k, ctl[k], rctl[k])
        assert math.isfinite(norm) and abs(norm - rnorm) <= 1e-6 * rnorm, "%s: norm %.9g, reference %.9g" % (tag, norm, rnorm)


@pytest.mark.parametrize("interval,growth,backoff", [(1, 2.0, 0.5), (2, 2.0, 0.5), (2000, 2.0, 0.5), (3, 1.5, 0.75)])
def test_loss_scale_update_state_machine(dev, interval, growth, backoff):
    """300 seeded steps of finite / inf / -inf / nan sums per configuration against ref_scaler_step: scale, tracker and skipped count
    exactly, opt_step only on clean steps, ctl and the norm as _check_scaler_step lists them.  (interval = 1 doubles the
    scale on every clean step and so walks into the 2^127 guard on its own.)"""
    S = _Scaler(dev, 65536.0)
    state, opt_step, ctl = (65536.0, 0.0, 0.0), 0.0, [0.0, 0.0, -7.0, -9.0]
    clean = 0
    for i, s in enumerate(R.sumsq_sequence(300, 1000 + interval)):
        if interval == 1 and state[0] >= 2.0 ** 100:
            s = float("inf") if i % 3 else s          # keep 1 / scale and the norm inside float32's normal range for this test
        want = R.ref_scaler_step(s, state, opt_step, growth, backoff, interval, R.B1, R.B2)
        got = S.step(s, growth, backoff, interval)
        _check_scaler_step("step %d (sumsq %r)" % (i, s), got, want, ctl)
        state, opt_step, ctl = got[0], got[1], got[2]
        clean += want[2][1] == 0.0
    assert state[2] >= 20 and clean >= 100 and opt_step == clean


@pytest.mark.parametrize("step", [1, 2, 10, 1000, 100000])
def test_loss_scale_update_bias_corrections_late_in_training(dev, step):
    S = _Scaler(dev, 1024.0, opt_step=float(step - 1))
    want = R.ref_scaler_step(4.0, (1024.0, 0.0, 0.0), float(step - 1), 2.0, 0.5, 2000, R.B1, R.B2)
    got = S.step(4.0, 2.0, 0.5, 2000)
    _check_scaler_step("opt_step %d" % step, got, want, None)
    assert got[1] == float(step) and abs(got[2][2] - (1.0 - R.B1 ** step)) <= R.ulp32(1.0) and got[3] == 2.0 / 1024.0


def test_loss_scale_update_edges(dev):
    # -inf and nan are overflows like inf
    for s in (float("-inf"), float("nan"), float("inf")):
        got = _Scaler(dev, 1024.0, tracker=5.0, opt_step=3.0).step(s, 2.0, 0.5, 2000)
        assert got[0] == (512.0, 0.0, 1.0) and got[1] == 3.0 and got[2] == [1.0 / 1024.0, 1.0, -7.0, -9.0] and not math.isfinite(got[3])
    # a growth step whose result is not finite keeps the scale, like torch._amp_update_scale_; the tracker restarts
    top = 2.0 ** 127
    S = _Scaler(dev, top)
    for k in range(3):
        state, opt_step, ctl, _ = S.step(1.0, 2.0, 0.5, 1)
        assert state == (top, 0.0, 0.0) and opt_step == k + 1.0 and ctl[1] == 0.0, (state, opt_step, ctl)
    assert _Scaler(dev, top / 2, tracker=1.0).step(1.0, 2.0, 0.5, 2)[0] == (top, 0.0, 0.0)
    # backing off through the subnormals to zero: float32 multiplication, the same as torch's (test_optim_reference_cpu)
    for start, backoff, n in ((2.0 ** -120, 0.5, 40), (2.0 ** -140, 0.75, 12)):
        S, state = _Scaler(dev, start), (start, 0.0, 0.0)
        for k in range(n):
            want = R.ref_scaler_step(float("inf"), state, 0.0, 2.0, backoff, 2000, R.B1, R.B2)
            got = S.step(float("inf"), 2.0, backoff, 2000)
            assert got[0] == want[0] and got[2][0] == want[2][0], (k, got, want)
            state = got[0]
    # a null norm_out is accepted
    got = _Scaler(dev, 8.0).step(16.0, 2.0, 0.5, 2000, norm=False)
    assert got[0] == (8.0, 1.0, 0.0) and got[3] == 0.0


@pytest.mark.parametrize("growth,backoff,interval", [(1.0, 0.5, 2000), (0.5, 0.5, 2000), (2.0, 0.0, 2000), (2.0, 1.0, 2000), (2.0, 1.5, 2000), (2.0, 0.5, 0)])
def test_loss_scale_update_refuses_bad_factors(dev, growth, backoff, interval):
    with pytest.raises(hip_error()):
        _Scaler(dev, 8.0).step(1.0, growth, backoff, interval)


# ================================================================================================ E. the elementwise family
def _exact_or_tol(name, got, ref, dtype):
    """float32: one IEEE operation per element on both sides, so the bits agree; 16 bits: test_kernels_gpu's TOL."""
    if dtype == torch.float32:
        assert torch.equal(got.cpu(), ref), name + ": float32 result is not the IEEE result"
    else:
        check(name, got, ref, TOL[dtype])


@pytest.mark.parametrize("n", FLAT)
@pytest.mark.parametrize("dtype", DT)
def test_add(dev, dtype, n):
    a, b = flat(n, 1, dtype), flat(n, 2, dtype)
    _exact_or_tol("add n=%d" % n, ops().add(a.to(dev, dtype), b.to(dev, dtype)), a + b, dtype)


@pytest.mark.parametrize("n", FLAT)
@pytest.mark.parametrize("dtype", DT)
def test_scale_in_place(dev, dtype, n):
    x = flat(n, 3, dtype)
    xd = x.to(dev, dtype)
    assert ops().scale_(xd, alpha=1.7) is xd
    _exact_or_tol("scale_ n=%d" % n, xd, x * torch.tensor(1.7, dtype=torch.float32), dtype)
    xd = x.to(dev, dtype)
    a = torch.tensor(2.0, dtype=torch.float32) * torch.tensor(0.3, dtype=torch.float32)    # alpha * alpha_dev[0] in float32, as the kernel forms it
    ops().scale_(xd, alpha=2.0, alpha_dev=torch.tensor([0.3], device=dev))
    _exact_or_tol("scale_ alpha_dev n=%d" % n, xd, x * a, dtype)


def _gelu_grad64(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


@pytest.mark.parametrize("n", FLAT)
@pytest.mark.parametrize("dtype", DT)
def test_mul_gelu_grad(dev, dtype, n):
    """dx = dy * gelu'(pre): float32 (erff) against the float64 erf derivative at 2e-6; the 16-bit builds use the Abramowitz-Stegun 7.1.26
    erf of gelu_grad_fast_f (absolute error <= 1.5e-7 before the 16-bit rounding), so TOL.  pre covers [-8, 8], 0 and +-large, where
    gelu' is exactly 0 or 1."""
    g = torch.Generator().manual_seed(5)
    pre = (torch.rand(n, generator=g) * 16.0 - 8.0)
    edge = torch.tensor([0.0, 30.0, -30.0, 1e4, -1e4, 8.0, -8.0, 0.0])
    for at in (0, n // 2 + 4, n - 8):
        pre[at:at + 8] = edge
    pre, dy = rnd(pre, dtype), flat(n, 6, dtype)
    for at in (0, n // 2 + 4, n - 8):
        dy[at:at + 8] = 1.0
    dx = ops().mul_gelu_grad(dy.to(dev, dtype), pre.to(dev, dtype))
    check("mul_gelu_grad n=%d" % n, dx, (dy.double() * _gelu_grad64(pre)).float(), 2e-6 if dtype == torch.float32 else TOL[dtype])
    got = dx.float().cpu()
    for at in (0, n // 2 + 4, n - 8):
        assert got[at:at + 5].tolist() == [0.5, 1.0, 0.0, 1.0, 0.0], (at, got[at:at + 8].tolist())


# ---- cast ----
def _h16_bits(n, seed):
    """n random 16-bit patterns (every exponent, subnormals, infinities) with the NaN patterns replaced by 1.0."""
    raw = torch.randint(-32768, 32768, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32).to(torch.int16)
    x = raw.view(h16())
    one = torch.ones((), dtype=h16()).view(torch.int16)
    return torch.where(torch.isnan(x.float()), one, raw).view(h16())


def _rounding_edges():
    """float32 values on and around the rounding boundaries of the build's 16-bit format: exact ties (both parities), their float32
    neighbours, the largest mantissa of a binade (rounds up into the next), +-0, subnormals, infinities, and the overflow edge."""
    t = h16()
    g = torch.Generator().manual_seed(7)
    lo = torch.randint(0, 0x7BFF if t == torch.float16 else 0x7F7E, (4096,), generator=g, dtype=torch.int32).to(torch.int16)
    top = torch.tensor([0x3BFF, 0x3FFF, 0x0001, 0x03FF] if t == torch.float16 else [0x3FFF, 0x407F, 0x0001, 0x007F], dtype=torch.int16)
    lo = torch.cat([lo, top])
    a, b = lo.view(t).float(), (lo + 1).view(t).float()
    tie = (a + b) / 2                                         # exact in float32: 16-bit neighbours differ in one low bit
    inf = torch.tensor(float("inf"))
    vals = [a, tie, torch.nextafter(tie, inf), torch.nextafter(tie, -inf)]
    fin = torch.finfo(t)
    over = torch.tensor([fin.max, 65519.996, 65520.0, 65536.0, 3.3961775e38, 3.4e38, torch.finfo(torch.float32).max, float("inf"), 0.0,
                         fin.tiny, fin.tiny / 2, fin.smallest_normal * 2.0 ** -10, 1e-45])
    out = torch.cat(vals + [over])
    return torch.cat([out, -out])


@pytest.mark.parametrize("n", FLAT)
def test_cast_f32_to_16_is_round_to_nearest_even(dev, both_halves, n):
    x = _randn(BIG, 8)[:n].clone() * 3.0
    e = _rounding_edges()
    ne = e.numel() - e.numel() % 4
    for at in (0, (n // 2) // 4 * 4, n - ne):
        x[at:at + ne] = e[:ne]
    if n > 4194304 + ne:
        x[4194304:4194304 + ne] = e[:ne]                      # the first elements of the second trip
    dst = torch.full((n,), 7.0, device=dev, dtype=h16())
    ops().cast(x.to(dev), dst)
    want = x.to(h16())
    bad = (bits(dst) != bits(want)).nonzero().flatten()
    assert bad.numel() == 0, "f32 -> %s differs from round-to-nearest-even at %d elements, first %r -> %r (torch %r)" % (
        both_halves, bad.numel(), x[bad[0]].item(), dst[bad[0]].item(), want[bad[0]].item())


@pytest.mark.parametrize("n", FLAT)
def test_cast_16_to_f32_is_exact_and_16_to_16_copies(dev, both_halves, n):
    src = _h16_bits(n, 9)
    sd = src.to(dev)
    dst = torch.full((n,), 7.0, device=dev)
    ops().cast(sd, dst)
    assert torch.equal(bits(dst), bits(src.float())), "16 -> f32 is not exact"
    cp = torch.zeros(n, device=dev, dtype=h16())
    ops().cast(sd, cp)
    assert torch.equal(bits(cp), bits(src)), "16 -> 16 is not a copy"     # (NaN patterns are left out: a conversion may quiet them)


@pytest.mark.parametrize("n", FLAT)
def test_cast_f32_to_f32_copies_every_bit(dev, n):
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=torch.Generator().manual_seed(10), dtype=torch.int64).to(torch.int32).view(torch.float32)
    dst = torch.zeros(n, device=dev)
    ops().cast(src.to(dev), dst)
    assert torch.equal(bits(dst), bits(src))


# ---- broadcasts over [B, S, H] ----
SHAPES = [(64, 128, 768), (3, 50, 132)]


@pytest.mark.parametrize("B,S,H", SHAPES)
@pytest.mark.parametrize("dtype", DT)
def test_bcast_add(dev, dtype, B, S, H):
    x, g = flat(B * S * H, 11, dtype).view(B, S, H), flat(B * H, 12, dtype).view(B, H)
    _exact_or_tol("bcast_add", ops().bcast_add(x.to(dev, dtype), g.to(dev, dtype)), x + g[:, None], dtype)


@pytest.mark.parametrize("B,S,H", SHAPES)
@pytest.mark.parametrize("dtype", DT)
def test_seq_bcast(dev, dtype, B, S, H):
    g, y0 = flat(B * H, 13, dtype).view(B, H), flat(B * S * H, 14, dtype).view(B, S, H)
    gd = g.to(dev, dtype)
    for mode, s0, s1, scale in ((0, 1, S, 0.5), (0, 2, S - 5, 1.0), (1, 0, S, 1.0), (1, 3, S - 7, 0.25), (0, 7, 7, 1.0), (1, 7, 7, 1.0)):
        y = y0.to(dev, dtype)
        ops().seq_bcast(gd, y, s0, s1, scale, mode)
        ref = y0.clone() if mode == 1 else torch.zeros(B, S, H)
        ref[:, s0:s1] += (g * torch.tensor(scale, dtype=torch.float32))[:, None]
        check("seq_bcast mode %d [%d, %d)" % (mode, s0, s1), y, ref, TOL[dtype])
        out = torch.ones(S, dtype=torch.bool)
        out[s0:s1] = False
        got = y.float().cpu()
        assert torch.equal(got[:, out], ref[:, out]), "rows outside [s0, s1) must be exactly zero (mode 0) / what they were (mode 1)"


def _ulp16(x, dtype):
    mant = 10 if dtype == torch.float16 else 7
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-30))) - mant)


@pytest.mark.parametrize("H", [132, 768])
@pytest.mark.parametrize("dtype", DT)
def test_seq_sum(dev, dtype, H):
    """B = 256 rows of blocks, S - s0 not a multiple of the 8 rows a block strides by.  Per element: float32 within summation error of
    the float64 sum; 16 bits within half a 16-bit ulp of it (ONE rounding of the float32 sum) plus that summation error.  The allowance
    for the summation, 1e-6 sum|x|: at most 7 additions per row lane, 7 across the 8 lanes, the scale and nothing else -- 15 roundings
    of 2^-24 each = 8.9e-7 of sum|x| in the worst case."""
    B, S = 256, 50
    x = flat(B * S * H, 15, dtype).view(B, S, H)
    xd = x.to(dev, dtype)
    for s0, s1, scale in ((1, S, 1.0 / (S - 1)), (3, S - 2, 1.0), (5, 6, 2.0)):
        got = ops().seq_sum(xd, s0, s1, scale).float().cpu().double()
        ref = x[:, s0:s1].double().sum(1) * scale
        slack = 1e-6 * x[:, s0:s1].double().abs().sum(1) * scale + 1e-30
        if dtype != torch.float32:
            slack = slack + 0.5 * _ulp16(ref, dtype)
        worst = ((got - ref).abs() / slack).max().item()
        print("  seq_sum %s H=%d [%d, %d): worst error / allowance %.3f" % (dtype, H, s0, s1, worst))
        assert got.shape == (B, H) and worst <= 1.0
        check("seq_sum", got, ref, TOL[dtype])


# ---- colsum ----
@functools.lru_cache(maxsize=2)
def _colsum_block(rows, N):
    return torch.randn(rows, N, generator=torch.Generator().manual_seed(16))


def _colsum_case(dev, dtype, M, N, ld=None, period=0, lo=0, hi=0, alpha=1.0, alpha_dev=None):
    """X = a seeded [1024, N] block repeated down the rows, each row times a power of two of its own (exact in every format), built on the
    device; the float64 reference is summed block by block on the host."""
    rows = min(M, 1024)
    reps = M // rows
    assert reps * rows == M
    blk = rnd(_colsum_block(rows, N), dtype)
    fac = torch.tensor([1.0, -0.5, 2.0, 0.25, -1.0, 0.5, -2.0, 1.0])[torch.arange(M) % 5 + torch.arange(M) % 3]
    ld = ld or N
    wide = torch.full((M, ld), 3.0, device=dev, dtype=dtype)            # columns outside the slice hold a value that would show
    X = wide[:, ld - N:]
    X.copy_((blk.to(dev).repeat(reps, 1) * fac.to(dev)[:, None]).to(dtype))
    keep = torch.ones(M, dtype=torch.bool)
    if period > 0:
        t = torch.arange(M) % period
        keep = (t >= lo) & (t < hi)
    ref = torch.zeros(N, dtype=torch.float64)
    for r in range(reps):
        w = (fac * keep)[r * rows:(r + 1) * rows].double()
        ref += (blk.double() * w[:, None]).sum(0)
    a = alpha * (0.3 if alpha_dev else 1.0)
    start = flat(N, 17, torch.float32)
    out = start.to(dev)
    ops().colsum(X, out, alpha, period, lo, hi, torch.tensor([0.3], device=dev) if alpha_dev else None)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    check("colsum M=%d N=%d ld=%d period=%d [%d, %d)" % (M, N, ld, period, lo, hi), out.cpu().double() - start.double(), a * ref, tol)


@pytest.mark.parametrize("dtype", DT)
def test_colsum_many_rows(dev, dtype):
    _colsum_case(dev, dtype, 32768, 768)                                      # 256 row blocks
    _colsum_case(dev, dtype, 32768, 768, period=128, lo=0, hi=1)              # the cls row of every sample
    _colsum_case(dev, dtype, 32768, 768, period=128, lo=1, hi=128, alpha=0.5, alpha_dev=True)
    _colsum_case(dev, dtype, 32768, 768, ld=1024)                             # a column slice of a wider matrix
    _colsum_case(dev, dtype, 3072, 132, period=3, lo=1, hi=2)                 # two column blocks, the second 4 columns wide
    _colsum_case(dev, dtype, 3072, 132, ld=264, alpha_dev=True)


@pytest.mark.parametrize("dtype", DT)
def test_colsum_row_block_cap(dev, dtype):
    """N = 30 000 is 235 column blocks, which caps the row blocks at 2048 / 235 = 8: each thread strides over 128 of the 8192 rows."""
    _colsum_case(dev, dtype, 8192, 30000)


# ---- zero_blocks ----
def test_zero_blocks(dev):
    n = 5 * 4194304 // 2 + 64 * 11
    g = torch.Generator().manual_seed(18)
    flags = (torch.rand(n // 64, generator=g) < 0.4).to(torch.uint8) * torch.randint(1, 256, (n // 64,), generator=g, dtype=torch.int32).to(torch.uint8)
    x = _randn(BIG, 19).repeat(2)[:n].clone()
    x[::97], x[5::193], x[7::389] = float("nan"), -0.0, float("inf")
    xd = x.to(dev)
    ops().zero_blocks_(xd, flags.to(dev))
    sel = flags.repeat_interleave(64) != 0
    assert 0.3 < sel.float().mean() < 0.5 and torch.isnan(x[sel]).any() and torch.isnan(x[~sel]).any()
    got = bits(xd)
    assert (got[sel] == 0).all(), "a flagged block must be +0 everywhere"
    assert torch.equal(got[~sel], bits(x)[~sel]), "an unflagged block must not change by a bit"
    with pytest.raises(hip_error()):
        ops().zero_blocks_(xd[:n - 32], flags.to(dev))


# ---- scaled_accum ----
def _is_a_nearest_float32(got, exact):
    got = np.float32(got)
    d = abs(fractions.Fraction(float(got)) - exact)
    return all(d <= abs(fractions.Fraction(float(np.nextafter(got, np.float32(s)))) - exact) for s in (np.inf, -np.inf))


def _check_fma(name, got, grad, scale, ws):
    """grad + scale * ws as ONE rounding (hipcc contracts scaled_accum_kernel's multiply-add to v_fmac_f32).  float64 holds the product of
    two float32 exactly and rounds the sum once more, so float64 -> float32 is the fused result except on a double-rounding tie (about one
    element in 2^29); any element that differs is settled with exact rational arithmetic."""
    want = (grad.double() + float(scale) * ws.double()).float()
    got = got.cpu()
    bad = (bits(got) != bits(want)).nonzero().flatten().tolist()
    assert len(bad) <= 8, "%s: %d elements differ from fma(scale, ws, grad)" % (name, len(bad))
    for i in bad:
        exact = fractions.Fraction(float(grad[i])) + fractions.Fraction(float(scale)) * fractions.Fraction(float(ws[i]))
        assert _is_a_nearest_float32(got[i].item(), exact), "%s: element %d is %r, fma gives %r" % (name, i, got[i].item(), want[i].item())


def test_scaled_accum(dev):
    o = ops()
    scales = torch.tensor([0.37, -1.0 / 3.0])
    sd = scales.to(dev)
    ws = _randn(BIG, 20)[:168].clone()
    for idx in (0, 1):        # the four slices of the SR head's 168-float workspace, as functions.py folds them
        for a, b in ((0, 81), (81, 84), (84, 165), (165, 168)):
            grad = _randn(BIG, 21)[a:b].clone()
            gd = grad.to(dev)
            o.scaled_accum(ws.to(dev)[a:b], gd, sd, idx)
            _check_fma("scaled_accum [%d:%d] idx %d" % (a, b, idx), gd, grad, scales[idx], ws[a:b])
    n = 30000 * 768           # the chunked MLM head's decoder weight gradient, onto a non-zero grad
    ws, grad = _randn(BIG, 22).repeat(3)[:n], _randn(BIG, 23).repeat(3)[:n].roll(12345)
    gd = grad.to(dev)
    o.scaled_accum(ws.to(dev), gd, sd, 1)
    _check_fma("scaled_accum n=%d" % n, gd, grad, scales[1], ws)
