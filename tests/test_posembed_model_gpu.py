"""-m gpu: a trained position table (`train_pos_embed=True`, `--train_pos_embed`) at the model, engine and driver level, on ecamp_tiny
with the oracle's recipe weights (B = 4, R = 224, C = 3), as tests/test_finetune_model_gpu.py tests fine-tuning without it.  The reference
is the float64 classifier of tests/_posembed_ref.py with `pos_embed` among the tensors that require a gradient, computed once per case.

Measured on an MI355X (profiles/finetune_pos_embed.txt holds the full lines): see that file; the bars below are the project's existing
ones and none was widened for this feature."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

import _posembed_ref as R
from _posembed_ref import B, C, rel

pytestmark = pytest.mark.gpu

STEM = ("pos_embed", "cls_token", "patch_embed.proj.bias")
OTHERS = ("blocks.0.attn.qkv.weight", "blocks.6.mlp.fc1.bias", "blocks.11.norm2.weight")      # one tensor per block region


# ---------------------------------------------------------------------------------------------------------------- one backward
@pytest.mark.parametrize("pool", ["avg", "cls"])
def test_one_backward_in_f32_against_float64_autograd(dev, pool):
    """The three gradients ecamp_pos_embed_grad forms, and three tensors elsewhere, to the project's 1e-3 of the largest element; a second
    backward accumulates; the arena holds the table like any trained tensor."""
    loss_ref, grads_ref = R.reference(pool)
    clf = R.build(torch.float32, dev, pool=pool)
    loss = R.backward(clf)
    named = dict(clf.finetune_parameters())
    assert sorted(named) == sorted(grads_ref) and "pos_embed" in named
    A = clf.encoder.arena
    pe = clf.encoder.pos_embed
    assert id(pe) in A.index and pe.grad.data_ptr() == A.grad(pe).data_ptr() and pe.data.data_ptr() == A.flat_p.data_ptr() + 4 * A.span(pe)[0]
    errs = {k: rel(named[k].grad, grads_ref[k]) for k in STEM + OTHERS}
    el = abs(loss - loss_ref) / abs(loss_ref)
    print("[pos_embed] one backward f32 %s: loss %.2e (bar 2e-4); gradient worst element / max (bar 1e-3): %s"
          % (pool, el, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert el <= 2e-4 and max(errs.values()) <= 1e-3, errs
    assert float(grads_ref["pos_embed"].abs().max()) > 0 and float(grads_ref["pos_embed"][0, 1:].abs().max()) > 0
    R.backward(clf)
    for k in STEM:
        assert rel(named[k].grad, 2 * grads_ref[k]) <= 1e-3, k


@pytest.mark.parametrize("dtype,f32_residual,med_tol,max_tol,ltol,lscale",
                         [(torch.bfloat16, False, 1e-2, 6e-2, 3e-2, 1.0), (torch.float16, False, 2e-3, 1e-2, 1e-3, 65536.0),
                          (torch.bfloat16, True, 1e-2, 6e-2, 3e-2, 1.0)], ids=["bf16", "f16", "bf16-f32residual"])
def test_one_backward_in_16_bits_within_the_formats_gradient_norm_bars(dev, dtype, f32_residual, med_tol, max_tol, ltol, lscale):
    """Per-tensor gradient norms, pos_embed included, against float64 (tensors above 1e-3 of the largest norm): bfloat16 median 1e-2 /
    worst 6e-2, IEEE half median 2e-3 / worst 1e-2 with the loss scaled by 65536.  Measured values: profiles/finetune_pos_embed.txt."""
    loss_ref, grads_ref = R.reference("avg")
    clf = R.build(dtype, dev, f32_residual=f32_residual)
    loss = R.backward(clf, scale=lscale)
    named = dict(clf.finetune_parameters())
    names = sorted(grads_ref)
    ref = np.array([float(grads_ref[k].norm()) for k in names])
    got = np.array([float(named[k].grad.double().norm()) / lscale for k in names])
    big = ref > 1e-3 * ref.max()
    e = np.abs(got - ref) / ref
    el = abs(loss - loss_ref) / abs(loss_ref)
    ip = names.index("pos_embed")
    print("[pos_embed] one backward %s%s: loss %.2e (bar %.0e); gradient norms of %d tensors: median %.2e (bar %.0e) worst %.2e (bar %.0e, %s); "
          "pos_embed %.2e, elementwise %.2e of its largest"
          % (str(dtype).split(".")[-1], " f32_residual" if f32_residual else "", el, ltol, int(big.sum()), np.median(e[big]), med_tol, e[big].max(),
             max_tol, np.array(names)[big][int(e[big].argmax())], e[ip], rel(named["pos_embed"].grad / lscale, grads_ref["pos_embed"])))
    assert big[ip], "pos_embed's gradient norm is among the ones that count"
    assert big.sum() > 60 and el <= ltol
    assert np.median(e[big]) <= med_tol and e[big].max() <= max_tol and e[ip] <= max_tol


# ---------------------------------------------------------------------------------------------------------------- three engine steps
def _engine_args(**kw):
    a = argparse.Namespace(learning_rate=3e-2, weight_decay=1e-4, decay_type="cosine", warmup_steps=1, num_steps=3, max_grad_norm=1.0,
                           train_batch_size=B, print_freq=100, output_dir="", name="t", ratio=1.0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _batches():
    return [R.imgs(B, seed=20 + i) for i in range(3)], [R.labels(seed=30 + i) for i in range(3)]


@functools.lru_cache(maxsize=None)
@R.with_threads
def _replay():
    """The three steps on the CPU in float64 over the trained list INCLUDING pos_embed: clip_grad_norm_, torch.optim.SGD(momentum 0.9,
    weight decay), the schedule stepped first -> (losses, {name: p3 - p0}, clip coefficients, the first step's norm before clipping)."""
    from ecamp_amd import engine_linprobe as lp
    args = _engine_args()
    P, cfg = R.ref_params("avg")
    names = R.trained_names("avg")
    p0 = {k: P[k].detach().clone() for k in names}
    opt = torch.optim.SGD([P[k] for k in names], lr=args.learning_rate, momentum=0.9, weight_decay=args.weight_decay)
    xs, ys = _batches()
    losses, coefs, norms = [], [], []
    for step in range(args.num_steps):
        loss = R.ref_loss(P, cfg, xs[step], ys[step], "avg")
        loss.backward()
        norm = float(torch.nn.utils.clip_grad_norm_([P[k] for k in names], args.max_grad_norm))
        norms.append(norm)
        coefs.append(min(1.0, args.max_grad_norm / (norm + 1e-6)))
        for grp in opt.param_groups:
            grp["lr"] = args.learning_rate * lp.lr_factor(args.decay_type, step + 1, args.warmup_steps, args.num_steps)
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
    return losses, {k: P[k].detach() - p0[k] for k in names}, coefs, norms[0]


def test_three_engine_steps_replay_on_the_cpu_in_float64(dev):
    """f32 compute; lr 3e-2, warm-up 1, weight decay 1e-4, max_grad_norm 1.  Losses to 2e-4; per-tensor parameter UPDATES (p3 - p0),
    pos_embed's among them, to 3e-3 of their largest element; the forward reads the trained table (or the losses of steps 2 and 3 would
    not match)."""
    from ecamp_amd import engine_finetune as engine
    losses_r, upd_r, coefs, _ = _replay()
    print("[pos_embed] replay clip coefficients:", ["%.3f" % c for c in coefs])
    assert any(c < 1.0 for c in coefs), "at least one step must clip on the reference side"
    clf = R.build(torch.float32, dev)
    clf.encoder.prepare()
    named = dict(clf.finetune_parameters())
    p0 = {k: p.detach().clone() for k, p in named.items()}
    xs, ys = _batches()
    out = engine.train(clf, list(zip(xs, ys)), None, _engine_args(), log=lambda m: None, keep_losses=True)
    assert out["global_step"] == 3 and len(out["losses"]) == 3
    losses = [float(t.item()) for t in out["losses"]]
    el = max(abs(a - r) / abs(r) for a, r in zip(losses, losses_r))
    errs = {k: rel(named[k].detach() - p0[k], upd_r[k]) for k in upd_r}
    worst = max(errs, key=errs.get)
    print("[pos_embed] engine vs float64 replay after 3 steps: losses %.2e (bar 2e-4); updates worst %.2e (%s), median %.2e, pos_embed %.2e (bar 3e-3)"
          % (el, errs[worst], worst, float(np.median(list(errs.values()))), errs["pos_embed"]))
    assert sorted(errs) == sorted(named) and el <= 2e-4 and errs[worst] <= 3e-3, (el, worst, errs[worst])
    assert float((named["pos_embed"].detach() - p0["pos_embed"]).abs().max()) > 0, "pos_embed has moved"
    assert clf.encoder.decoder_pos_embed.requires_grad is False


def test_last_norm_is_the_global_norm_over_the_trained_list_with_pos_embed(dev):
    """A single hand-run step: the norm torch computes in float64 over the .grad of finetune_parameters(), taken before the step's
    zero_grad, against optimizer.last_norm to 1e-5 -- and it is not the norm without pos_embed."""
    from ecamp_amd import engine_finetune as engine
    clf = R.build(torch.float32, dev)
    opt = engine.make_optimizer(clf, _engine_args())
    assert any(p is clf.encoder.pos_embed for g in opt.param_groups for p in g["params"])
    xs, ys = _batches()
    R.backward(clf, x=xs[0], y=ys[0])
    clf.encoder.arena.flush_fresh()
    grads = {k: p.grad.detach().double().cpu() for k, p in clf.finetune_parameters()}
    want = float(torch.sqrt(sum((g ** 2).sum() for g in grads.values())))
    without = float(torch.sqrt(sum((g ** 2).sum() for k, g in grads.items() if k != "pos_embed")))
    before = clf.encoder.pos_embed.detach().clone()
    opt.step()
    got = float(opt.last_norm.item())
    ref_norm = _replay()[3]
    print("[pos_embed] last_norm %.8e; float64 norm of the engine's gradients %.8e (rel %.2e, bar 1e-5); without pos_embed %.8e; replay's %.8e"
          % (got, want, abs(got - want) / want, without, ref_norm))
    assert abs(got - want) <= 1e-5 * want
    assert abs(without - want) > 2e-5 * want, "pos_embed's gradient must weigh more in the norm than the bar, for this check to tell"
    assert not torch.equal(clf.encoder.pos_embed.detach(), before)


def test_the_16_bit_shadows_follow_the_masters_and_the_table_survives_a_move(dev):
    from ecamp_amd import engine_finetune as engine
    clf = R.build(torch.bfloat16, dev)
    A = clf.encoder.prepare()
    pos0 = clf.encoder.pos_embed.detach().clone()
    xs, ys = _batches()
    out = engine.train(clf, list(zip(xs, ys)), None, _engine_args(), log=lambda m: None, keep_losses=True)
    assert out["global_step"] == 3 and all(np.isfinite(float(t.item())) for t in out["losses"])
    live = torch.zeros(A.total, dtype=torch.bool)
    for p, o, n in zip(A.params, A.offsets, A.sizes):
        live[o:o + n] = True
    live = live.to(dev)
    assert torch.equal(A.flat_p16[live], A.flat_p[live].to(torch.bfloat16)), "the 16-bit shadows must equal the masters, cast"
    trained = clf.encoder.pos_embed.detach().clone()
    assert not torch.equal(trained, pos0)
    # .to() re-materialises the parameters and drops the arena: the next one is built with pos_embed again, from the trained values,
    # and the forward reads them
    clf.eval()
    with torch.no_grad():
        before = clf(R.imgs())
    clf.to("cpu").to(dev)
    assert clf.encoder.arena is None and clf.encoder.pos_embed.requires_grad is True
    with torch.no_grad():
        after = clf(R.imgs())
    A2 = clf.encoder.arena
    assert A2 is not A and id(clf.encoder.pos_embed) in A2.index and torch.equal(clf.encoder.pos_embed.detach(), trained)
    assert clf.encoder.pos_embed.data_ptr() == A2.flat_p.data_ptr() + 4 * A2.span(clf.encoder.pos_embed)[0]
    assert torch.equal(before, after)


# ---------------------------------------------------------------------------------------------------------------- checkpoint round trip
def test_checkpoint_carries_the_trained_table_and_a_default_classifier_scores_it(dev):
    from ecamp_amd import engine_finetune as engine
    clf = R.build(torch.bfloat16, dev)
    sincos = clf.encoder.pos_embed.detach().cpu().clone()
    xs, ys = _batches()
    engine.train(clf, list(zip(xs, ys)), None, _engine_args(), log=lambda m: None)
    sd = clf.reference_state_dict()
    assert torch.equal(sd["pos_embed"], clf.encoder.pos_embed.detach().cpu().float()) and not torch.equal(sd["pos_embed"], sincos)
    assert sd["pos_embed"].shape == (1, 197, 192) and sd["pos_embed"].dtype == torch.float32
    clf.eval()
    with torch.no_grad():
        want = clf(R.imgs())
    fresh = R.build(torch.bfloat16, "cpu", train_pos_embed=False, train_encoder=False)      # a default classifier: the table is data to it
    assert "pos_embed" in fresh.load_pretrained(sd)
    fresh.to(dev).eval()
    assert fresh.encoder.pos_embed.requires_grad is False
    with torch.no_grad():
        got = fresh(R.imgs())
    assert torch.equal(got, want), "eval logits of the reloaded checkpoint must be the trained model's bits"


# ---------------------------------------------------------------------------------------------------------------- the default
def test_without_the_flag_nothing_changes_and_the_two_stem_backwards_agree(dev):
    """The default path keeps its two colsum launches; the fixed-order kernel sums the same numbers in another order: cls_token and bias
    gradients within 1e-5 relative (f32 rounding of a few hundred terms)."""
    off = R.build(torch.float32, dev, train_pos_embed=False)
    on = R.build(torch.float32, dev)
    assert off.encoder.pos_embed.requires_grad is False and "pos_embed" not in dict(off.finetune_parameters())
    la, lb = R.backward(off), R.backward(on)
    assert la == lb, "the forward is the same computation"
    assert id(off.encoder.pos_embed) not in off.encoder.arena.index and off.encoder.pos_embed.grad is None
    for k in ("cls_token", "patch_embed.proj.bias"):
        a, b = dict(off.finetune_parameters())[k].grad, dict(on.finetune_parameters())[k].grad
        e = rel(a, b)
        print("[pos_embed] %s gradient, colsum path vs pos_embed_grad path: %.2e (bar 1e-5)" % (k, e))
        assert e <= 1e-5, k


def test_a_built_arena_without_the_table_is_refused_and_masking_is_refused(dev):
    from ecamp_amd.module.classifier import ECAMPClassifier
    off = R.build(torch.float32, dev, train_pos_embed=False)
    off.encoder.prepare()
    with pytest.raises(RuntimeError, match="already built without pos_embed"):
        ECAMPClassifier(off.encoder, C, train_encoder=True, train_pos_embed=True)
    assert off.encoder.pos_embed.requires_grad is False
    # a masked pass (pre-training's) through a stem whose table is trained: the backward refuses, it does not mis-place rows
    from ecamp_amd.functions import StemFn
    on = R.build(torch.float32, dev)
    m = on.encoder
    m.prepare()
    x = StemFn.apply(R.imgs(2).to(dev), None, m, 0.75, m.cls_token)[0]
    with pytest.raises(RuntimeError, match="every patch kept in place"):
        x.float().sum().backward()


def test_the_pass_after_a_backward_that_raised_joins_the_weight_gradient_stream_once(dev, monkeypatch):
    """The refused masked pass above launches the stem's weight gradient on the weight-gradient stream, asks for the join at the end of
    the pass and then raises: the engine drops that callback.  The next, ordinary pass must ask again and be joined exactly once
    (streams.at_backward_end remembers the pass, not a flag that only the dropped callback would have cleared)."""
    from ecamp_amd import hip_ops, streams
    from ecamp_amd.functions import StemFn
    monkeypatch.setattr(hip_ops, "OVERLAP_WGRAD", True)
    clf = R.build(torch.float32, dev)
    m = clf.encoder
    m.prepare()
    x = StemFn.apply(R.imgs(2).to(dev), None, m, 0.75, m.cls_token)[0]
    with pytest.raises(RuntimeError, match="every patch kept in place"):
        x.float().sum().backward()
    joins, join = [], streams.join
    monkeypatch.setattr(streams, "join", lambda: (joins.append(1), join())[1])
    R.backward(clf)
    assert len(joins) == 1


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_driver_trains_the_table_writes_it_and_tests_the_checkpoint(dev, tmp_path):
    from ecamp_amd import main_finetune
    out = str(tmp_path / "run")
    common = ["--name", "t", "--model", "vit_tiny_patch16", "--task", "CheXpert", "--num_classes", "5", "--output_dir", out, "--img_size", "224",
              "--train_batch_size", "8", "--eval_batch_size", "16", "--learning_rate", "3e-2", "--warmup_steps", "1",
              "--synthetic", "--synthetic_len", "16", "--num_workers", "0", "--print_freq", "2", "--train_pos_embed"]
    parse = main_finetune.get_args_parser().parse_args
    res = main_finetune.main(parse(common + ["--stage", "train", "--num_steps", "4"]))
    path = os.path.join(out, "t_bestauc_checkpoint.bin")
    assert os.path.exists(path) and len(res["aurocs"]) == 5
    sd = torch.load(path, map_location="cpu")
    model = main_finetune.build_model(main_finetune.check_args(parse(common + ["--stage", "test"])))
    assert model.train_pos_embed is True
    sincos = model.encoder.pos_embed.detach().clone()
    assert sd["pos_embed"].shape == sincos.shape and not torch.equal(sd["pos_embed"], sincos), "the checkpoint holds a trained table"
    res2 = main_finetune.main(parse(common + ["--stage", "test"]))
    assert res2["loss"] == res["loss"]
    np.testing.assert_array_equal(np.array(res2["aurocs"]), np.array(res["aurocs"]))
    log = open(os.path.join(out, "log.txt")).read()
    first = log.splitlines()[0]
    assert "pos_embed" in first and "IS trained" in first and "fixed" not in first and "NOT applied" in first
    n_on = sum(p.numel() for _, p in model.finetune_parameters())
    assert "Total Parameter: \t%2.4fM" % (n_on / 1e6) in log and n_on == sum(v.numel() for v in sd.values())
    for line in ("Training (4 / 4 Steps)", "Saved model checkpoint", "Test Loss:"):
        assert line in log, line
