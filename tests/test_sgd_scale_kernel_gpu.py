"""-m gpu: ecamp_sgd_scale_update (csrc/finetune.hip), the loss scaler's decision on the device, on both 16-bit builds: its norm against
float64 and -- bit for bit -- against the norm ecamp_sgd_grouped forms from the same partials under the `ctl` just written; the three ways
a sum of squares stops being finite (inf and nan are VALUES of f32 arithmetic here; every address stays in range); the state against
`SGDLossScaler.host_update` after every update of a scripted sequence; the cap, the static scale and the host-side refusals.
npart in {1, 255, 256, 257, 4096}: one slot, either side of the 256-thread stride, and the cap of two full ecamp_sumsq_grouped launches."""
import ctypes

import pytest
import torch

import _finetune_ref as R
from conftest import h16

pytestmark = pytest.mark.gpu

NPARTS = [1, 255, 256, 257, 4096]
N = 64 * 12                              # elements of the flat buffer the step under `ctl` runs over


def _partials(npart, seed=0):
    """Random positive slots, as sums of squares are."""
    g = torch.Generator().manual_seed(1000 + npart + seed)
    return (0.25 + torch.rand(npart, generator=g)) * 1.0e5


def _state(dev, scale, clean=0.0, skipped=0.0, row=0.0):
    return torch.tensor([scale, clean, skipped, row], device=dev, dtype=torch.float32)


def _update(part, state, growth=2.0, backoff=0.5, window=2000, max_scale=2.0 ** 24):
    """One launch -> (ctl, norm) as host lists / floats (state is updated in place on the device)."""
    from ecamp_amd import hip_ops as ops
    ctl = torch.full((4,), -7.0, device=part.device)
    norm = torch.full((1,), -7.0, device=part.device)
    ops.sgd_scale_update(part, part.numel(), state, ctl, norm, growth, backoff, window, max_scale)
    return ctl, norm


def _sgd_under(dev, part, ctl, max_norm=1.0):
    """ecamp_sgd_grouped over a small flat buffer with `part` as its partials, under `ctl` -> (before, after, norm_out); before / after
    are (p, buf, p16)."""
    from ecamp_amd import hip_ops as ops
    table = R.block_table(N // 64, seed=3).to(dev)
    p0, grads = R.trajectory(N, steps=1, seed=4)
    p, g = p0.to(dev), grads[0].to(dev)
    buf = torch.randn(N, generator=torch.Generator().manual_seed(9)).to(dev)
    p16 = p.to(h16())
    before = (p.clone(), buf.clone(), p16.clone())
    norm = torch.full((1,), -3.0, device=dev)
    ops.sgd_grouped(p, g, buf, p16, table, R.GROUP_LR, R.GROUP_WD, R.MOMENTUM, max_norm, part, part.numel(), 1.0, ctl, norm)
    torch.cuda.synchronize()
    return before, (p, buf, p16), norm


@pytest.mark.parametrize("scale", [65536.0, 1000.0], ids=["2^16", "1000"])
@pytest.mark.parametrize("npart", NPARTS)
def test_norm_against_float64_and_bit_equal_to_the_norm_of_the_step(dev, both_halves, npart, scale):
    """1e-6 relative to sqrt(float64 sum) / scale; and the same BITS as ecamp_sgd_grouped's norm_out from the same partials under the
    `ctl` this launch wrote: the scaler and every workgroup of the step add the slots in one order and form the norm by one expression."""
    part = _partials(npart).to(dev)
    state = _state(dev, scale)
    ctl, norm = _update(part, state)
    want = float(torch.sqrt(part.double().sum()).cpu()) / scale
    e = abs(float(norm.item()) - want) / want
    print("[fp16-finetune] sgd_scale_update npart=%d scale=%g (%s build): norm %.2e of sqrt(float64 sum) / scale (bar 1e-6)" % (npart, scale, both_halves, e))
    assert e <= 1e-6
    assert ctl.tolist() == [float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(scale, dtype=torch.float32)), 0.0, 0.0, 0.0]
    assert state.tolist() == [scale, 1.0, 0.0, 0.0]
    before, after, step_norm = _sgd_under(dev, part, ctl)
    assert torch.equal(step_norm.view(torch.int32), norm.view(torch.int32)), (step_norm.item(), norm.item())
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1]) and not torch.equal(after[2], before[2])   # a clean step is taken
    # two launches on equal inputs: equal bits
    state2 = _state(dev, scale)
    ctl2, norm2 = _update(part, state2)
    assert torch.equal(norm2.view(torch.int32), norm.view(torch.int32)) and torch.equal(ctl2, ctl) and torch.equal(state2, state)


def _overflow(form, npart):
    part = _partials(npart, seed=1)
    if form == "inf-last":
        part[-1] = float("inf")
    elif form == "nan-first":
        part[0] = float("nan")
    else:                                  # two finite slots whose sum leaves f32 (3.0e38 + 3.0e38 > FLT_MAX = 3.4e38)
        part[0], part[1] = 3.0e38, 3.0e38
        assert bool(torch.isfinite(part).all())
    return part


@pytest.mark.parametrize("form,npart", [(f, n) for f in ("inf-last", "nan-first", "finite-sum") for n in NPARTS if not (f == "finite-sum" and n == 1)])
def test_a_sum_that_is_not_finite_is_found_backs_off_and_the_step_under_its_ctl_writes_nothing(dev, both_halves, form, npart):
    part = _overflow(form, npart).to(dev)
    state = _state(dev, 2.0 ** 20, clean=5.0, skipped=3.0, row=0.0)
    ctl, norm = _update(part, state)
    assert ctl.tolist() == [2.0 ** -20, 1.0, 0.0, 0.0]
    assert state.tolist() == [2.0 ** 19, 0.0, 4.0, 1.0]                   # halved; the clean count starts again; both skipped counters + 1
    assert not bool(torch.isfinite(norm).all())
    before, after, step_norm = _sgd_under(dev, part, ctl)
    for b, a, name in zip(before, after, ("p", "buf", "p16")):
        assert torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32)), name
    assert float(step_norm.item()) == -3.0                                  # a skipped step writes no norm either
    ctl, norm = _update(part, state)                                        # a second overflow in a row
    assert state.tolist() == [2.0 ** 18, 0.0, 5.0, 2.0] and ctl.tolist() == [2.0 ** -19, 1.0, 0.0, 0.0]


def test_a_scripted_sequence_equals_host_update_after_every_update(dev, both_halves):
    """window = 3, 2 * window + 3 = 9 updates, overflows at updates 3 (one short of the window) and 8; growth exactly at the window."""
    from ecamp_amd.optim import SGDLossScaler
    window = 3
    flags = [0, 0, 1, 0, 0, 0, 0, 1, 0]
    assert len(flags) == 2 * window + 3
    host = SGDLossScaler(init_scale=2.0 ** 10, window=window, max_scale=2.0 ** 24)
    clean, bad = _partials(257).to(dev), _overflow("inf-last", 257).to(dev)
    state = _state(dev, 2.0 ** 10)
    seen = []
    for f in flags:
        ctl, _ = _update(bad if f else clean, state, window=window)
        host.host_update(f)
        want = [host.scale, float(host.clean_steps), float(host.skipped_steps), float(host.skipped_in_a_row)]
        assert state.tolist() == want, (len(seen), state.tolist(), want)
        assert ctl[1].item() == float(f)
        seen.append(state[0].item())
    assert seen == [1024.0, 1024.0, 512.0, 512.0, 512.0, 1024.0, 1024.0, 512.0, 512.0]
    # the same through the scaler's own device state
    dev_scaler = SGDLossScaler(init_scale=2.0 ** 10, window=window, max_scale=2.0 ** 24)
    for f in flags:
        c = dev_scaler.update(bad if f else clean, 257)
        assert c is dev_scaler.ctl
    assert (dev_scaler.scale, dev_scaler.clean_steps, dev_scaler.skipped_steps, dev_scaler.skipped_in_a_row, dev_scaler.last_found_inf) == (512.0, 1, 2, 0, False)
    loss = torch.tensor(0.75, device=dev)
    assert float(dev_scaler.scale_loss(loss).item()) == 0.75 * 512.0
    with pytest.raises(RuntimeError):
        dev_scaler.host_update(False)


def test_growth_stops_at_max_scale_and_a_window_of_zero_is_a_static_scale(dev, both_halves):
    clean, bad = _partials(256).to(dev), _overflow("finite-sum", 256).to(dev)
    state = _state(dev, 2.0 ** 12, clean=1.0)
    _update(clean, state, window=2, max_scale=2.0 ** 12)
    assert state.tolist() == [2.0 ** 12, 0.0, 0.0, 0.0]                     # a growth step at the cap: the scale stays, the count starts again
    state = _state(dev, 2.0 ** 12, clean=1.0)
    _update(clean, state, window=2, max_scale=2.0 ** 24)
    assert state.tolist() == [2.0 ** 13, 0.0, 0.0, 0.0]
    # window = 0: never grows, never backs off; an overflow still tells the step to skip
    state = _state(dev, 2.0 ** 12)
    for k in range(3):
        ctl, _ = _update(clean, state, window=0)
        assert state.tolist() == [2.0 ** 12, float(k + 1), 0.0, 0.0] and ctl.tolist() == [2.0 ** -12, 0.0, 0.0, 0.0]
    ctl, norm = _update(bad, state, window=0)
    assert state.tolist() == [2.0 ** 12, 0.0, 1.0, 1.0] and ctl.tolist() == [2.0 ** -12, 1.0, 0.0, 0.0] and not bool(torch.isfinite(norm).all())
    before, after, _ = _sgd_under(dev, bad, ctl)
    assert all(torch.equal(a, b) for a, b in zip(after, before))


def test_what_the_host_refuses_returns_an_error_and_launches_nothing(dev, both_halves):
    from ecamp_amd import _lib
    lib = _lib.load()
    part = _partials(8).to(dev)
    state, ctl, norm = _state(dev, 1024.0), torch.full((4,), -7.0, device=dev), torch.full((1,), -7.0, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda part_=P(part), npart=8, state_=P(state), ctl_=P(ctl), growth=2.0, backoff=0.5, window=3, max_scale=2.0 ** 24: lib.ecamp_sgd_scale_update(
        part_, npart, state_, ctl_, P(norm), growth, backoff, window, max_scale, stream)
    err = lambda: lib.ecamp_last_error().decode()
    for kw, word in (({"part_": None}, "null pointer"), ({"state_": None}, "null pointer"), ({"ctl_": None}, "null pointer"), ({"npart": 0}, "npart=0"),
                     ({"npart": 4097}, "npart=4097"), ({"backoff": 0.0}, "backoff=0"), ({"window": -1}, "window=-1"), ({"growth": 0.5}, "growth=0.5"),
                     ({"max_scale": 0.0}, "max_scale=0")):
        assert call(**kw) != 0 and word in err(), (kw, err())
    torch.cuda.synchronize()
    assert state.tolist() == [1024.0, 0.0, 0.0, 0.0] and ctl.tolist() == [-7.0] * 4 and norm.item() == -7.0
    assert call() == 0                                                     # and the same arguments, all valid, do launch
    torch.cuda.synchronize()
    assert state.tolist() == [1024.0, 1.0, 0.0, 0.0] and ctl.tolist() == [2.0 ** -10, 0.0, 0.0, 0.0] and norm.item() > 0
