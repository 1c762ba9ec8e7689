"""not gpu: the float64 references of tests/_optim_ref.py, proven against torch before any kernel is held to them
(tests/test_optim_elementwise_gpu.py): grouped AdamW against torch.optim.AdamW(float64) with the same groups, the scaler step against
torch._amp_update_scale_ on CPU tensors, and the float32 yardstick of the kernel tests checked to be rounding-sized (a yardstick that
is far from the reference would make "at most 4x the yardstick" an empty bound)."""
import math

import numpy as np
import pytest
import torch

import _optim_ref as R


def _arena(nblocks, seed):
    table = R.make_table(nblocks, seed)
    n = nblocks * 64
    return table, n, R.make_params(n, seed + 1), R.make_magnitudes(n, seed + 2)


def test_the_inputs_hold_every_case_they_are_meant_to():
    table = R.make_table(4099, 11)
    assert set(table.tolist()) == {0, 1, 2, 3, 4, R.BEYOND, R.EDGE, R.FROZEN}
    cuts = (table[1:] != table[:-1]).nonzero().flatten() + 1
    assert cuts.numel() > 100 and (cuts % 16 != 0).sum() > cuts.numel() // 2, "group boundaries must fall inside a 1024-element thread-block span"
    assert {R.GROUP_WD[0], R.GROUP_WD[1]} == {R.f32(0.05), 0.0} and 0.0 in R.GROUP_LR_SCALE and 0.65 in R.GROUP_LR_SCALE
    lrs = [R.group_lrs(t, 50) for t in range(1, 51)]
    assert lrs[0][0] == R.f32(6e-5) and lrs[9][0] == R.f32(6e-4) and lrs[49][0] == R.f32(1e-6)   # warm-up, peak, the cosine's end
    assert all(l[3] == 0.0 for l in lrs) and abs(lrs[20][2] / lrs[20][0] - 0.65) < 1e-6 and abs(lrs[20][4] / lrs[20][0] - 0.1) < 1e-6
    mag = R.make_magnitudes(64 * 4099, 13)
    nz = mag[mag != 0].abs()
    assert (mag[::7] == 0).all() and 1e-12 <= nz.min() < 1e-11 and 1e1 < nz.max() <= 1e2 and (mag < 0).any() and (mag > 0).any()


def test_ref_adamw_grouped_equals_torch_adamw_in_float64():
    """50 steps, five groups + a group index beyond them + frozen blocks, a schedule that moves the lr every step, a gradient scale of
    1/65536 on gradients pre-multiplied by 65536 (exact): p, m, v within 1e-12 of the largest update."""
    table, n, p0, mag = _arena(613, 3)
    steps = 50
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    opt = R.TorchGroupedAdamW(p0, table, R.GROUP_WD, R.B1, R.B2, R.EPS, torch.float64)
    upd = R.element_groups(table) < 8
    for t in range(1, steps + 1):
        g = R.plant_nonfinite(R.make_grad(mag, 5, t), table)
        lrs = R.group_lrs(t, steps)
        total = R.ref_adamw_grouped(p, g * 65536.0, m, v, table, lrs, list(R.GROUP_WD), R.B1, R.B2, R.EPS, t, 1.0 / 65536.0)
        opt.step(g, lrs)
        want = float((g.double()[upd] ** 2).sum())
        assert math.isfinite(total) and abs(total - want) <= 1e-12 * want
    pt, mt, vt = opt.arena(p0)
    biggest = (pt - p0.double()).abs().max().item()
    assert biggest > 1e-3, "the trajectory must move the parameters"
    err = (p - pt).abs().max().item()
    print("  f64 reference vs torch f64 AdamW: %.2e of the largest update" % (err / biggest))
    assert err <= 1e-12 * biggest
    assert ((m - mt).abs() <= 1e-12 * mt.abs()).all() and ((v - vt).abs() <= 1e-12 * vt.abs()).all()
    # blocks with a table byte >= 8: not a bit of p, m, v moves, whatever their gradient holds
    assert torch.equal(p[~upd], p0.double()[~upd]) and (m[~upd] == 0).all() and (v[~upd] == 0).all()
    # a group index >= the number of groups: the moments gather, the parameter stays
    beyond = R.element_groups(table) == R.BEYOND
    assert torch.equal(p[beyond], p0.double()[beyond]) and (v[beyond][mag[beyond] != 0] > 0).all()
    # lr = 0 with weight decay set: the same
    g3 = R.element_groups(table) == 3
    assert torch.equal(p[g3], p0.double()[g3])


def test_ref_adamw_grouped_chunks_do_not_matter():
    table, n, p0, mag = _arena(613, 3)
    outs = []
    for chunk in (64, 64 * 100, 1 << 21):
        p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        s = [R.ref_adamw_grouped(p, R.make_grad(mag, 5, t), m, v, table, R.group_lrs(t, 3), list(R.GROUP_WD), R.B1, R.B2, R.EPS, t, 1.0,
                                 chunk=chunk) for t in (1, 2, 3)]
        outs.append((p, m, v, s))
    for p, m, v, s in outs[1:]:
        assert torch.equal(p, outs[0][0]) and torch.equal(m, outs[0][1]) and torch.equal(v, outs[0][2])
        assert all(abs(a - b) <= 1e-12 * b for a, b in zip(s, outs[0][3]))


def test_the_float32_yardstick_is_rounding_sized():
    """torch.optim.AdamW in float32 on the CPU -- the yardstick the kernel may be at most 4x as far from the reference as -- sits where
    float32 rounding puts it: a few ulp of the largest |p| after 50 steps, a few 1e-7 on the moments."""
    table, n, p0, mag = _arena(4099, 11)
    steps = 50
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    yard = R.TorchGroupedAdamW(p0, table, R.GROUP_WD, R.B1, R.B2, R.EPS, torch.float32)
    sel = R.element_groups(table) < 8
    for t in range(1, steps + 1):
        g = R.make_grad(mag, 5, t)
        lrs = R.group_lrs(t, steps)
        R.ref_adamw_grouped(p, g, m, v, table, lrs, list(R.GROUP_WD), R.B1, R.B2, R.EPS, t, 1.0)
        yard.step(g, lrs)
        if t in (1, 50):
            dp, dm, dv = R.distances(*yard.arena(p0), (p, m, v), sel)
            print("  step %2d: yardstick p %.2e (%.1f ulp of max|p|)  m %.2e  v %.2e" % (t, dp, dp / R.ulp32(p.abs().max().item()), dm, dv))
            assert 0.0 < dp <= 16 * R.ulp32(p.abs().max().item()) and 0.0 < dm <= 2e-6 and 0.0 < dv <= 2e-6


# ------------------------------------------------------------------------------------------------ the scaler step
def _torch_scaler(scale, tracker, sumsq, growth, backoff, interval):
    s, tr = torch.tensor([scale], dtype=torch.float32), torch.tensor([int(tracker)], dtype=torch.int32)
    found = torch.tensor([0.0 if math.isfinite(float(np.float32(sumsq))) else 1.0])
    torch._amp_update_scale_(s, tr, found, growth, backoff, interval)
    return float(s), float(tr)


@pytest.mark.parametrize("interval,growth,backoff", [(1, 2.0, 0.5), (2, 2.0, 0.5), (2000, 2.0, 0.5), (3, 1.5, 0.75)])
def test_ref_scaler_step_equals_torch_amp_update_scale(interval, growth, backoff):
    for seed in range(3):
        state, opt_step = (65536.0, 0.0, 0.0), 0.0
        for s in R.sumsq_sequence(150, 100 * interval + seed):
            new, step2, ctl, norm = R.ref_scaler_step(s, state, opt_step, growth, backoff, interval, R.B1, R.B2)
            want = _torch_scaler(state[0], state[1], s, growth, backoff, interval)
            assert new[:2] == want, (s, state, new, want)
            bad = not math.isfinite(s)
            assert new[2] == state[2] + bad and step2 == opt_step + (not bad) and ctl[1] == float(bad)
            assert ctl[0] == R.f32(1.0 / state[0]) and math.isfinite(norm) != bad
            assert (ctl[2] is None and ctl[3] is None) if bad else (ctl[2] == 1.0 - R.B1 ** step2 and ctl[3] == 1.0 / math.sqrt(1.0 - R.B2 ** step2))
            state, opt_step = new, step2
        assert state[2] > 5 and opt_step > 100


def test_ref_scaler_step_edges_equal_torch():
    # a growth step that would overflow keeps the scale (and restarts the tracker)
    top = 2.0 ** 127
    assert _torch_scaler(top, 0, 1.0, 2.0, 0.5, 1) == (top, 0.0)
    assert R.ref_scaler_step(1.0, (top, 0.0, 0.0), 0.0, 2.0, 0.5, 1, R.B1, R.B2)[0] == (top, 0.0, 0.0)
    assert R.ref_scaler_step(1.0, (top / 2, 1.0, 0.0), 0.0, 2.0, 0.5, 2, R.B1, R.B2)[0] == (top, 0.0, 0.0)
    # backing off through the subnormals down to zero: whatever float32 multiplication does, on both sides
    state = (2.0 ** -120, 5.0, 0.0)
    for k in range(40):
        new = R.ref_scaler_step(float("nan") if k % 2 else float("-inf"), state, 7.0, 2.0, 0.5, 2000, R.B1, R.B2)[0]
        assert new[:2] == _torch_scaler(state[0], state[1], float("inf"), 2.0, 0.5, 2000)
        state = new
    assert state == (0.0, 0.0, 40.0)
    state = (2.0 ** -140, 0.0, 0.0)
    for k in range(12):   # an odd back-off factor on subnormals rounds (to nearest even) at every step
        new = R.ref_scaler_step(float("inf"), state, 0.0, 2.0, 0.75, 2000, R.B1, R.B2)[0]
        assert new[:2] == _torch_scaler(state[0], state[1], float("inf"), 2.0, 0.75, 2000)
        state = new
