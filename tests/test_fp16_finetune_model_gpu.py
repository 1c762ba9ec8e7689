"""-m gpu: encoder fine-tuning in IEEE half under the on-device loss scaler, at the model, engine and driver level.  Model, weights, batches
and the float64 references are those of tests/test_finetune_model_gpu.py (ecamp_tiny with the oracle's recipe weights, B = 4, C = 3),
imported from it and shared: three engine steps beside the same steps in bfloat16, steps that must be skipped, the scale finding its
level, a freshly initialised head (the case the reference's 2^20 exists for), the collapse of the scale, and the driver."""
import functools
import os

import numpy as np
import pytest
import torch

import test_finetune_model_gpu as M

pytestmark = pytest.mark.gpu

B, C = M.B, M.C


def _scaler_of(monkeypatch, **kw):
    """A scaler of the test's own making behind engine_finetune.make_scaler -> the scaler."""
    from ecamp_amd import engine_finetune as engine
    from ecamp_amd.optim import SGDLossScaler
    scaler = SGDLossScaler(**kw)
    monkeypatch.setattr(engine, "make_scaler", lambda args: scaler)
    return scaler


def _trained_state(clf, opt):
    """Every byte a step may write: masters, 16-bit shadows and momentum of the arena, parameters and momentum of the tail."""
    A, T = clf.encoder.arena, clf.tail()
    return [A.flat_p, A.flat_p16, opt._buf, T.flat_p, T.flat_buf]


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32))


# ---------------------------------------------------------------------------------------------------------------- three engine steps
def _three_steps(dev, dtype, compute):
    from ecamp_amd import engine_finetune as engine
    losses_r, upd_r, _ = M._replay()
    clf = M._build(dtype, dev)
    clf.encoder.prepare()
    named = M._named(clf)
    p0 = {k: p.detach().clone() for k, p in named.items()}
    xs, ys = M._batches()
    out = engine.train(clf, list(zip(xs, ys)), None, M._engine_args(compute_dtype=compute), log=lambda m: None, keep_losses=True)
    assert out["global_step"] == 3
    losses = [float(t.item()) for t in out["losses"]]
    el = max(abs(a - r) / abs(r) for a, r in zip(losses, losses_r))
    errs = {k: M.rel(named[k].detach() - p0[k], upd_r[k]) for k in upd_r}
    worst = max(errs, key=errs.get)
    return el, errs[worst], worst, float(np.median(list(errs.values())))


def test_three_engine_steps_in_half_are_no_further_from_float64_than_in_bfloat16(dev, monkeypatch):
    """lr 3e-2, warm-up 1, weight decay 1e-4, max_grad_norm 1, loss scale 2^16 (no step skipped) against the float64 replay.  The bar is
    the bfloat16 path on the same three steps: half has three more mantissa bits and un-scaling by a power of two is exact, so the worst
    per-tensor update error (max |a - b| / max |b| of p3 - p0) and the loss error must each be no larger than bfloat16's; the loss
    error also <= 1e-3, the half bar of the one-backward test.  Measured values: profiles/finetune_fp16.txt."""
    scaler = _scaler_of(monkeypatch, init_scale=2.0 ** 16)
    el_b, eu_b, worst_b, med_b = _three_steps(dev, torch.bfloat16, "bf16")
    assert scaler._dev is None, "the bfloat16 path must not touch a loss scaler"
    el_h, eu_h, worst_h, med_h = _three_steps(dev, torch.float16, "fp16")
    print("[fp16-finetune] 3 engine steps vs float64 replay: fp16 (scale 2^16) losses %.2e updates worst %.2e (%s) median %.2e; "
          "bf16 losses %.2e updates worst %.2e (%s) median %.2e; skipped %d, scale after %g"
          % (el_h, eu_h, worst_h, med_h, el_b, eu_b, worst_b, med_b, scaler.skipped_steps, scaler.scale))
    assert scaler.skipped_steps == 0 and scaler.clean_steps == 3 and scaler.scale == 2.0 ** 16
    assert eu_h <= eu_b and el_h <= el_b, (eu_h, eu_b, el_h, el_b)
    assert el_h <= 1e-3


# ---------------------------------------------------------------------------------------------------------------- steps that are skipped
def test_steps_whose_gradients_overflow_half_are_skipped_and_leave_every_byte_alone(dev, monkeypatch):
    """Loss scale 2^40: dx enters the encoder at about 0.08 * 0.1 / 196 * 2^40 = 4.5e7, above half's largest number 65504 (inf and nan
    VALUES in the gradients; nothing is out of range in memory).  Both steps are skipped, the schedule still advances."""
    from ecamp_amd import engine_finetune as engine
    scaler = _scaler_of(monkeypatch, init_scale=2.0 ** 40, max_scale=2.0 ** 40)
    made = []
    real = engine.make_optimizer
    monkeypatch.setattr(engine, "make_optimizer", lambda model, args: made.append(real(model, args)) or made[-1])
    clf = M._build(torch.float16, dev)
    A = clf.encoder.prepare()
    clf.tail()
    before = None
    xs, ys = M._batches()

    class Loader(list):      # the state the first step starts from exists once the optimizer is made: taken at the first batch
        def __iter__(self):
            nonlocal before
            if before is None:
                before = [t.clone() for t in _trained_state(clf, made[0])]
            return super().__iter__()

    out = engine.train(clf, Loader(zip(xs[:2], ys[:2])), None, M._engine_args(compute_dtype="fp16", num_steps=2), log=lambda m: None, keep_losses=True)
    assert out["global_step"] == 2 and len(made) == 1 and made[0].loss_scaler is scaler and made[0]._steps == 2
    assert all(np.isfinite(float(t.item())) for t in out["losses"])                   # the forward pass and the un-scaled loss are fine
    after = _trained_state(clf, made[0])
    for name, a, b in zip(("flat_p", "flat_p16", "momentum", "tail p", "tail momentum"), after, before):
        assert _bits_equal(a, b), name
    assert float(made[0]._buf.abs().max()) == 0 and clf.encoder.arena is A
    assert (scaler.scale, scaler.skipped_steps, scaler.skipped_in_a_row, scaler.clean_steps, scaler.last_found_inf) == (2.0 ** 38, 2, 2, 0, True)
    assert not np.isfinite(float(made[0].last_norm.item()))


def test_the_scale_finds_its_level_from_two_to_the_32(dev, monkeypatch):
    """2^32 puts dx at about 2e5, above 65504: the first step is skipped; at most sixteen halvings reach 2^16, where the gradients fit.
    window 2, twenty steps over rotating batches; the skip flag of every step stays on the device and is read once at the end.  A
    skipped step left every trained byte alone, a taken one changed every trained tensor; scale and counters equal host_update
    replayed over the recorded flags.  (The schedule's horizon is 40 steps, so that no step runs at a zero learning rate.)"""
    from ecamp_amd import engine_finetune as engine
    from ecamp_amd.optim import SGDLossScaler
    steps, kw = 20, dict(init_scale=2.0 ** 32, window=2, max_scale=2.0 ** 32)
    scaler = _scaler_of(monkeypatch, **kw)
    clf = M._build(torch.float16, dev)
    clf.encoder.prepare()
    args = M._engine_args(compute_dtype="fp16", num_steps=2 * steps)
    opt = engine.make_optimizer(clf, args)
    opt.zero_grad(set_to_none=True)
    named = M._named(clf)
    xs, ys = M._batches()
    flags = torch.zeros(steps, device=dev)
    same_bytes = torch.zeros(steps, device=dev, dtype=torch.bool)       # every trained byte as before the step
    all_moved = torch.zeros(steps, device=dev, dtype=torch.bool)        # every trained tensor differs from before the step
    for s in range(steps):
        prev = [t.clone() for t in _trained_state(clf, opt)]
        prev_p = {k: p.detach().clone() for k, p in named.items()}
        engine.train_step(clf, opt, xs[s % 3], ys[s % 3], s, args)
        flags[s] = scaler.ctl[1]
        same_bytes[s] = torch.stack([(a.view(torch.uint8) == b.view(torch.uint8)).all() for a, b in zip(_trained_state(clf, opt), prev)]).all()
        all_moved[s] = torch.stack([(named[k].detach() != prev_p[k]).any() for k in named]).all()
    flags, same_bytes, all_moved = flags.cpu().tolist(), same_bytes.cpu().tolist(), all_moved.cpu().tolist()
    host = SGDLossScaler(**kw)
    for f in flags:
        host.host_update(f != 0)
    print("[fp16-finetune] from 2^32, window 2, 20 steps: skip flags %s; scale %g, %d skipped" % ("".join(str(int(f)) for f in flags), scaler.scale, scaler.skipped_steps))
    assert flags[0] == 1.0 and set(flags) <= {0.0, 1.0}
    for s, f in enumerate(flags):
        assert (same_bytes[s] and not all_moved[s]) if f else (all_moved[s] and not same_bytes[s]), (s, f, same_bytes[s], all_moved[s])
    assert (scaler.scale, scaler.clean_steps, scaler.skipped_steps, scaler.skipped_in_a_row) == (host.scale, host.clean_steps, host.skipped_steps, host.skipped_in_a_row)
    assert steps - scaler.skipped_steps >= 4 and scaler.skipped_steps == int(sum(flags)) and opt._steps == steps


# ---------------------------------------------------------------------------------------------------------------- a fresh head
def _fresh_tail():
    """The classifier's tail as a run starts with it: head.weight ~ trunc_normal(std=2e-5) (train.py:148), zero bias, identity fc_norm."""
    w = torch.empty(C, 192)
    torch.manual_seed(7)
    torch.nn.init.trunc_normal_(w, std=2e-5)
    return {"fc_norm.weight": torch.ones(192), "fc_norm.bias": torch.zeros(192), "head.weight": w, "head.bias": torch.zeros(C)}


@functools.lru_cache(maxsize=None)
@M._with_threads
def _fresh_reference():
    """One float64 backward on the test batch with the fresh tail -> {name: gradient norm}; computed once."""
    P, cfg = M._ref_params("avg")
    with torch.no_grad():
        for k, v in _fresh_tail().items():
            P[k].copy_(v.double())
    M._ref_loss(P, cfg, M._imgs(), M._labels(True), True, "avg").backward()
    return {k: float(P[k].grad.norm()) for k in M._trained_names("avg")}


def _fresh_norm_errors(dev, scale):
    """One backward in half with the loss scaled by `scale` -> per-tensor gradient-norm errors against float64, over (a) the encoder's
    tensors above 1e-3 of the largest encoder norm, (b) every trained tensor above 1e-3 of the largest norm of all."""
    from ecamp_amd.optim import SGDLossScaler
    ref = _fresh_reference()
    clf = M._build(torch.float16, dev)
    with torch.no_grad():
        for k, v in _fresh_tail().items():
            clf.get_parameter(k).copy_(v)
    clf.encoder.prepare()
    clf.tail()
    clf.train()
    scaler = SGDLossScaler(init_scale=scale)
    scaler.scale_loss(clf.loss(clf(M._imgs()), M._labels(True))).backward()
    torch.cuda.synchronize()
    named = M._named(clf)
    names = sorted(ref)
    want = np.array([ref[k] for k in names])
    got = np.array([float(named[k].grad.double().norm()) / scale for k in names])
    enc = np.array([not k.startswith(("head.", "fc_norm.")) for k in names])
    err = np.abs(got - want) / want
    big_enc = enc & (want > 1e-3 * want[enc].max())
    big_all = want > 1e-3 * want.max()
    return err[big_enc], err[big_all], int(big_enc.sum()), int(big_all.sum())


def test_a_fresh_head_needs_the_scale_the_reference_sets(dev):
    """head.weight ~ 2e-5: dfeat is of order 1e-7 and dx, divided by 196 tokens, 1e-9 per element -- below half's smallest subnormal
    2^-24 = 6e-8.  At loss scale 2^20 the per-tensor gradient norms meet the half bars of the one-backward test (median 2e-3, worst 1e-2
    over tensors above 1e-3 of the largest norm).  With this head the largest norm of ALL trained tensors is the head's own (f32, never
    through half) and every encoder tensor lies below 1e-3 of it, so the bars are held over the encoder's tensors relative to the
    largest encoder norm -- the tensors the scale exists for -- and over the literal set as well.  At scale 1 the same two figures are
    recorded, not asserted: the measured reason for the mode (profiles/finetune_fp16.txt)."""
    enc, lit, n_enc, n_lit = _fresh_norm_errors(dev, 2.0 ** 20)
    print("[fp16-finetune] fresh head, scale 2^20: encoder gradient norms of %d tensors: median %.2e (bar 2e-3) worst %.2e (bar 1e-2); "
          "all trained tensors above 1e-3 of the largest (%d): median %.2e worst %.2e" % (n_enc, np.median(enc), enc.max(), n_lit, np.median(lit), lit.max()))
    enc1, lit1, n_enc1, _ = _fresh_norm_errors(dev, 1.0)
    print("[fp16-finetune] fresh head, scale 1 (recorded, not asserted): encoder gradient norms of %d tensors: median %.2e worst %.2e"
          % (n_enc1, np.median(enc1), enc1.max()))
    assert n_enc > 60 and n_lit >= 1
    assert np.median(enc) <= 2e-3 and enc.max() <= 1e-2
    assert np.median(lit) <= 2e-3 and lit.max() <= 1e-2


# ---------------------------------------------------------------------------------------------------------------- collapse
def test_a_scale_below_one_ends_the_run_and_names_the_f32_residual(dev, monkeypatch):
    from ecamp_amd import engine_finetune as engine
    _scaler_of(monkeypatch, init_scale=0.5)               # the device state reads 0.5 at the first print step
    clf = M._build(torch.float16, dev)
    xs, ys = M._batches()
    lines = []
    with pytest.raises(SystemExit) as e:
        engine.train(clf, list(zip(xs, ys)), None, M._engine_args(compute_dtype="fp16", print_freq=1), log=lines.append)
    assert e.value.code not in (0, None) and "--f32_residual" in str(e.value) and "0.5" in str(e.value)
    assert any("loss scale 0.5" in l for l in lines) and sum("Training (" in l for l in lines) == 1      # it ended at the first print step
    assert clf.training is False


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_driver_fine_tunes_in_half_with_the_reference_flags_and_the_flag_added(dev, tmp_path):
    from ecamp_amd import main_finetune
    out = str(tmp_path / "run")
    common = ["--name", "t", "--model", "vit_tiny_patch16", "--task", "CheXpert", "--num_classes", "5", "--output_dir", out, "--img_size", "224",
              "--train_batch_size", "8", "--eval_batch_size", "16", "--learning_rate", "3e-2", "--warmup_steps", "1", "--fp16", "--fp16_opt_level", "O2",
              "--fp16_loss_scale", "dynamic", "--synthetic", "--synthetic_len", "16", "--num_workers", "0", "--print_freq", "2"]
    parse = main_finetune.get_args_parser().parse_args
    res = main_finetune.main(parse(common + ["--stage", "train", "--num_steps", "4"]))
    log = open(os.path.join(out, "log.txt")).read()
    first = log.splitlines()[0]
    assert first.startswith(main_finetune.DEVIATIONS) and "IEEE half" in first and "1048576 (2^20)" in first and "f32_residual" in first
    assert "End Training!" in log and "Training (4 / 4 Steps)" in log
    scale_lines = [l for l in log.splitlines() if l.startswith("  loss scale ")]
    assert len(scale_lines) == 2 and all("steps skipped" in l for l in scale_lines)             # print_freq 2 over 4 steps
    path = os.path.join(out, "t_bestauc_checkpoint.bin")
    assert os.path.exists(path)
    sd = torch.load(path, map_location="cpu")
    assert sd["head.weight"].shape == (5, 192)
    for k, v in sd.items():
        assert v.dtype == torch.float32 and bool(torch.isfinite(v).all()), k
    res2 = main_finetune.main(parse(common + ["--stage", "test"]))
    assert res2["loss"] == res["loss"] and np.isfinite(res2["loss"])
    np.testing.assert_array_equal(np.array(res2["aurocs"]), np.array(res["aurocs"]))
