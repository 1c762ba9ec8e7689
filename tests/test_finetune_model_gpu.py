"""-m gpu: encoder fine-tuning at the model, engine and driver level, on ecamp_tiny with the oracle's recipe weights (B = 4, R = 224,
C = 3).  The reference is the oracle's `vit_block` chain under torch autograd in float64 on the CPU, computed once per (loss, pooling)
and shared: one backward in every format, three engine steps against a float64 replay, what must not change, and the driver."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, C = 4, 3


def rel(a, b):
    """max |a - b| / max |b|"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _imgs(n=B, seed=11):
    return torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


def _labels(multilabel, n=B, seed=2):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, C, generator=g) < 0.5).float() if multilabel else torch.randint(0, C, (n, 1), generator=g).float()


def _tail_values():
    """fc_norm and head of a classifier in mid-training: no identity norm, no vanishing head."""
    g = torch.Generator().manual_seed(5)
    return {"fc_norm.weight": 1 + 0.2 * torch.randn(192, generator=g), "fc_norm.bias": 0.1 * torch.randn(192, generator=g),
            "head.weight": 0.1 * torch.randn(C, 192, generator=g), "head.bias": 0.1 * torch.randn(C, generator=g)}


def _build(dtype, dev, multilabel=True, pool="avg", train_encoder=True, **kw):
    from ecamp_amd.module import model_ecamp as me
    from ecamp_amd.module.classifier import ECAMPClassifier
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    torch.manual_seed(0)
    enc = me.ecamp_tiny(compute_dtype=dtype, **kw)
    enc.load_state_dict(recipe.recipe_state(orc.cfg_tiny(), seed=0), strict=True)
    clf = ECAMPClassifier(enc, C, multilabel=multilabel, pool=pool, train_encoder=train_encoder)
    tv = _tail_values()
    with torch.no_grad():
        clf.fc_norm.weight.copy_(tv["fc_norm.weight"])
        clf.fc_norm.bias.copy_(tv["fc_norm.bias"])
        clf.head.weight.copy_(tv["head.weight"])
        clf.head.bias.copy_(tv["head.bias"])
    return clf.to(dev)


# ---------------------------------------------------------------------------------------------------------------- the float64 reference
def _trained_names(pool):
    names = ["cls_token", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    for i in range(12):
        for n in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2"):
            names += ["blocks.%d.%s.weight" % (i, n), "blocks.%d.%s.bias" % (i, n)]
    names += ["norm.weight", "norm.bias"] if pool == "cls" else ["fc_norm.weight", "fc_norm.bias"]
    return names + ["head.weight", "head.bias"]


def _ref_params(pool):
    """The oracle's parameters and the classifier's tail in float64; the trained ones require a gradient."""
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    cfg = orc.cfg_tiny()
    P = {k: v.double() for k, v in orc.load_state(orc.new_params(cfg), recipe.recipe_state(cfg, seed=0)).items()}
    P.update({k: v.double() for k, v in _tail_values().items()})
    for k in _trained_names(pool):
        P[k].requires_grad_(True)
    return P, cfg


def _ref_loss(P, cfg, imgs, y, multilabel, pool):
    from oracle import ecamp_oracle as orc
    n = imgs.shape[0]
    x = F.conv2d(imgs.double(), P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=cfg.patch_size).flatten(2).transpose(1, 2)
    x = x + P["pos_embed"][:, 1:, :]
    x = torch.cat(((P["cls_token"] + P["pos_embed"][:, :1, :]).expand(n, -1, -1), x), dim=1)
    for i in range(cfg.depth):
        x = orc.vit_block(P, "blocks.%d" % i, x, cfg.num_heads, cfg.ln_eps)
    if pool == "avg":
        feat = F.layer_norm(x[:, 1:, :].mean(dim=1), (x.shape[-1],), P["fc_norm.weight"], P["fc_norm.bias"], 1e-6)
    else:
        feat = F.layer_norm(x, (x.shape[-1],), P["norm.weight"], P["norm.bias"], cfg.ln_eps)[:, 0]
    logits = feat @ P["head.weight"].t() + P["head.bias"]
    return F.binary_cross_entropy_with_logits(logits, y.double()) if multilabel else F.cross_entropy(logits, y.reshape(-1).long())


def _with_threads(fn):
    @functools.wraps(fn)
    def wrapped(*a, **k):
        threads = torch.get_num_threads()
        torch.set_num_threads(min(os.cpu_count() or 1, 16))
        try:
            return fn(*a, **k)
        finally:
            torch.set_num_threads(threads)     # (process-wide: given back for the tests that follow)
    return wrapped


@functools.lru_cache(maxsize=None)
@_with_threads
def _reference(multilabel, pool):
    """One backward on the test batch -> (loss, {name: gradient}) in float64; computed once per case, shared, never changed."""
    P, cfg = _ref_params(pool)
    loss = _ref_loss(P, cfg, _imgs(), _labels(multilabel), multilabel, pool)
    loss.backward()
    return float(loss.detach()), {k: P[k].grad.clone() for k in _trained_names(pool)}


def _named(clf):
    return dict(clf.finetune_parameters())


def _backward(clf, multilabel, scale=1.0):
    clf.train()
    loss = clf.loss(clf(_imgs()), _labels(multilabel))
    (loss * scale if scale != 1.0 else loss).backward()
    clf.check_labels()
    torch.cuda.synchronize()
    return float(loss.item())


def _untrained_arena_mask(clf):
    """bool [arena.total]: the elements of arena parameters that fine-tuning does not train."""
    A = clf.encoder.arena
    trained = {id(p) for _, p in clf.finetune_parameters()}
    m = torch.zeros(A.total, dtype=torch.bool)
    for p, o, n in zip(A.params, A.offsets, A.sizes):
        if id(p) not in trained:
            m[o:o + n] = True
    return m


# ---------------------------------------------------------------------------------------------------------------- one backward
F32_CASES = [(torch.float32, True, "avg", False), (torch.float32, False, "avg", False), (torch.float32, True, "cls", False),
             (torch.bfloat16, True, "avg", True)]


@pytest.mark.parametrize("dtype,multilabel,pool,f32_residual", F32_CASES, ids=["f32-bce-avg", "f32-ce-avg", "f32-bce-cls", "bf16-f32residual"])
def test_one_backward_against_float64_autograd(dev, dtype, multilabel, pool, f32_residual):
    """f32 compute: loss to 2e-4, every trained tensor's gradient to 1e-3 of its largest element (the project's f32 bars); everything else
    in the arena keeps a zero gradient.  The 16-bit format with the f32 residual stream is held to the bfloat16 bars of
    tests/test_model_gpu.py on the per-tensor gradient norms (median 1e-2, worst 6e-2; loss 3e-2)."""
    loss_ref, grads_ref = _reference(multilabel, pool)
    clf = _build(dtype, dev, multilabel=multilabel, pool=pool, f32_residual=f32_residual)
    loss = _backward(clf, multilabel)
    named = _named(clf)
    assert sorted(named) == sorted(grads_ref)
    el = abs(loss - loss_ref) / abs(loss_ref)
    errs = {k: rel(named[k].grad, grads_ref[k]) for k in grads_ref}
    nerr = {k: abs(float(named[k].grad.double().norm()) - float(grads_ref[k].norm())) / float(grads_ref[k].norm()) for k in grads_ref}
    worst = max(errs, key=errs.get)
    print("[finetune] one backward %s %s %s%s: loss %.2e; gradients worst element / max %.2e (%s), median %.2e; norms median %.2e worst %.2e"
          % (str(dtype).split(".")[-1], "bce" if multilabel else "ce", pool, " f32_residual" if f32_residual else "", el, errs[worst], worst,
             float(np.median(list(errs.values()))), float(np.median(list(nerr.values()))), max(nerr.values())))
    if dtype == torch.float32:
        assert el <= 2e-4 and errs[worst] <= 1e-3, (el, worst, errs[worst])
    else:
        assert el <= 3e-2 and float(np.median(list(nerr.values()))) <= 1e-2 and max(nerr.values()) <= 6e-2
    A = clf.encoder.arena
    A.flush_fresh()
    others = _untrained_arena_mask(clf)
    assert bool(others.any()) and torch.all(A.flat_g.cpu()[others] == 0), "decoder / report-side gradients must stay zero"
    if pool == "cls":
        assert torch.all(clf.fc_norm.weight.grad == 0) and torch.all(clf.fc_norm.bias.grad == 0)
    if dtype == torch.float32:   # a second backward accumulates, as autograd does for any parameter
        _backward(clf, multilabel)
        for k in ("blocks.11.mlp.fc2.weight", "blocks.0.norm1.bias", "head.weight"):
            assert rel(named[k].grad, 2 * grads_ref[k]) <= 1e-3, k


@pytest.mark.parametrize("dtype,med_tol,max_tol,ltol,lscale", [(torch.bfloat16, 1e-2, 6e-2, 3e-2, 1.0), (torch.float16, 2e-3, 1e-2, 1e-3, 65536.0)],
                         ids=["bf16", "f16"])
def test_one_backward_in_16_bits_within_the_formats_gradient_norm_bars(dev, dtype, med_tol, max_tol, ltol, lscale):
    """Per-tensor gradient norms against the oracle, as tests/test_model_gpu.py measures them (tensors above 1e-3 of the largest norm):
    bfloat16 median 1e-2 / worst 6e-2, IEEE half median 2e-3 / worst 1e-2 with the loss scaled by 65536.  Measured values:
    profiles/finetune.txt."""
    loss_ref, grads_ref = _reference(True, "avg")
    clf = _build(dtype, dev)
    loss = _backward(clf, True, scale=lscale)
    named = _named(clf)
    names = sorted(grads_ref)
    ref = np.array([float(grads_ref[k].norm()) for k in names])
    got = np.array([float(named[k].grad.double().norm()) / lscale for k in names])
    big = ref > 1e-3 * ref.max()
    e = np.abs(got - ref)[big] / ref[big]
    el = abs(loss - loss_ref) / abs(loss_ref)
    print("[finetune] one backward %s: loss %.2e (bar %.0e); gradient norms of %d tensors: median %.2e (bar %.0e) worst %.2e (bar %.0e, %s)"
          % (str(dtype).split(".")[-1], el, ltol, int(big.sum()), np.median(e), med_tol, e.max(), max_tol, np.array(names)[big][int(e.argmax())]))
    assert big.sum() > 60 and el <= ltol
    assert np.median(e) <= med_tol and e.max() <= max_tol


# ---------------------------------------------------------------------------------------------------------------- three engine steps
def _engine_args(**kw):
    a = argparse.Namespace(learning_rate=3e-2, weight_decay=1e-4, decay_type="cosine", warmup_steps=1, num_steps=3, max_grad_norm=1.0,
                           train_batch_size=B, print_freq=100, output_dir="", name="t", ratio=1.0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _batches():
    return [_imgs(B, seed=20 + i) for i in range(3)], [_labels(True, seed=30 + i) for i in range(3)]


@functools.lru_cache(maxsize=None)
@_with_threads
def _replay():
    """The three steps on the CPU in float64: clip_grad_norm_, torch.optim.SGD(momentum 0.9, weight decay), the schedule stepped first
    -> (losses, {name: p3 - p0}, clip coefficients)."""
    from ecamp_amd import engine_linprobe as lp
    args = _engine_args()
    P, cfg = _ref_params("avg")
    names = _trained_names("avg")
    p0 = {k: P[k].detach().clone() for k in names}
    opt = torch.optim.SGD([P[k] for k in names], lr=args.learning_rate, momentum=0.9, weight_decay=args.weight_decay)
    xs, ys = _batches()
    losses, coefs = [], []
    for step in range(args.num_steps):
        loss = _ref_loss(P, cfg, xs[step], ys[step], True, "avg")
        loss.backward()
        norm = float(torch.nn.utils.clip_grad_norm_([P[k] for k in names], args.max_grad_norm))
        coefs.append(min(1.0, args.max_grad_norm / (norm + 1e-6)))
        for grp in opt.param_groups:
            grp["lr"] = args.learning_rate * lp.lr_factor(args.decay_type, step + 1, args.warmup_steps, args.num_steps)
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
    return losses, {k: P[k].detach() - p0[k] for k in names}, coefs


def test_three_engine_steps_replay_on_the_cpu_in_float64(dev):
    """f32 compute; lr 3e-2, warm-up 1, weight decay 1e-4, max_grad_norm 1.  Losses to 2e-4; per-tensor parameter UPDATES (p3 - p0) to
    3e-3 of their largest element -- three steps, each adding at most the 1e-3 gradient bar."""
    from ecamp_amd import engine_finetune as engine
    losses_r, upd_r, coefs = _replay()
    print("[finetune] replay clip coefficients:", ["%.3f" % c for c in coefs])
    assert any(c < 1.0 for c in coefs), "at least one step must clip on the reference side"
    clf = _build(torch.float32, dev)
    A = clf.encoder.prepare()
    named = _named(clf)
    p0 = {k: p.detach().clone() for k, p in named.items()}
    flat0, pos0 = A.flat_p.clone(), clf.encoder.pos_embed.detach().clone()
    xs, ys = _batches()
    out = engine.train(clf, list(zip(xs, ys)), None, _engine_args(), log=lambda m: None, keep_losses=True)
    assert out["global_step"] == 3 and len(out["losses"]) == 3
    losses = [float(t.item()) for t in out["losses"]]
    el = max(abs(a - r) / abs(r) for a, r in zip(losses, losses_r))
    errs = {k: rel(named[k].detach() - p0[k], upd_r[k]) for k in upd_r}
    worst = max(errs, key=errs.get)
    print("[finetune] engine vs float64 replay after 3 steps: losses %.2e (bar 2e-4); updates worst %.2e (%s), median %.2e (bar 3e-3)"
          % (el, errs[worst], worst, float(np.median(list(errs.values())))))
    assert el <= 2e-4 and errs[worst] <= 3e-3, (el, worst, errs[worst])
    others = _untrained_arena_mask(clf).to(dev)
    assert clf.encoder.arena is A and torch.equal(A.flat_p[others], flat0[others]), "decoder / report side must keep their bits"
    assert torch.equal(clf.encoder.pos_embed, pos0) and clf.encoder.pos_embed.requires_grad is False
    assert all(float((named[k].detach() - p0[k]).abs().max()) > 0 for k in named), "every trained tensor moved"
    assert clf.training is False                       # the engine hands the model back in eval mode


def test_the_16_bit_shadows_follow_the_masters_through_engine_steps(dev):
    from ecamp_amd import engine_finetune as engine
    clf = _build(torch.bfloat16, dev)
    A = clf.encoder.prepare()
    flat0 = A.flat_p.clone()
    xs, ys = _batches()
    out = engine.train(clf, list(zip(xs, ys)), None, _engine_args(), log=lambda m: None, keep_losses=True)
    assert out["global_step"] == 3 and all(np.isfinite(float(t.item())) for t in out["losses"])
    assert not torch.equal(A.flat_p, flat0)
    live = torch.zeros(A.total, dtype=torch.bool)
    for p, o, n in zip(A.params, A.offsets, A.sizes):
        live[o:o + n] = True
    live = live.to(dev)
    assert torch.equal(A.flat_p16[live], A.flat_p[live].to(torch.bfloat16)), "the 16-bit shadows must equal the masters, cast"
    # the optimizer state in torch SGD's layout
    from ecamp_amd.optim import FusedSGD
    opt = FusedSGD([p for _, p in clf.finetune_parameters()], lr=0.1, momentum=0.9)
    assert opt.state_dict()["state"] == {}
    loss = clf.train().loss(clf(xs[0]), ys[0])
    loss.backward()
    opt.step()
    sd = opt.state_dict()
    assert len(sd["state"]) == len(clf.finetune_parameters()) and sd["param_groups"][0]["momentum"] == 0.9
    assert all(set(v) == {"momentum_buffer"} and v["momentum_buffer"].shape == p.shape for v, (_, p) in zip(sd["state"].values(), clf.finetune_parameters()))
    assert opt.last_norm.shape == (1,) and float(opt.last_norm.item()) > 0
    other = _build(torch.bfloat16, dev)
    other.encoder.prepare()
    other.tail()
    with pytest.raises(RuntimeError, match="different arenas"):
        FusedSGD([clf.head.weight, other.head.weight, clf.encoder.cls_token], lr=0.1).step()
    with pytest.raises(RuntimeError, match="different arenas"):
        FusedSGD([clf.encoder.cls_token, other.encoder.cls_token], lr=0.1).step()


# ---------------------------------------------------------------------------------------------------------------- what must not change
def test_the_default_is_still_the_probe_and_eval_runs_the_forward_only_path(dev):
    imgs = _imgs()
    probe = _build(torch.bfloat16, dev, train_encoder=False)
    ft = _build(torch.bfloat16, dev, train_encoder=True)
    probe.train()
    # the probe's forward: the forward-only features through the head, bit for bit, and a gradient for the head only
    from ecamp_amd import hip_ops as ops
    logits = probe(imgs)
    feats = probe.forward_features(imgs)
    assert torch.equal(logits.detach(), ops.cls_head_fwd(feats, probe.head.weight.data, probe.head.bias.data))
    A = probe.encoder.arena
    flat_g = A.flat_g.clone()
    probe.loss(logits, _labels(True)).backward()
    assert probe.head.weight.grad is not None and probe.head.bias.grad is not None
    assert probe.fc_norm.weight.grad is None and probe.fc_norm.bias.grad is None and torch.equal(A.flat_g, flat_g)
    assert probe._tail is None
    # a train_encoder model: the same bits in training mode (differentiable path), in eval mode and under no_grad (forward-only path)
    ft.train()
    a = ft(imgs)
    assert a.requires_grad and a.grad_fn is not None
    with torch.no_grad():
        b = ft(imgs)
    ft.eval()
    c = ft(imgs)
    with torch.no_grad():
        f = ft.forward_features(imgs)
        d = ft(imgs)
    assert torch.equal(a.detach(), logits.detach()) and torch.equal(b, logits.detach()) and torch.equal(c.detach(), logits.detach()) and torch.equal(d, b)
    assert torch.equal(f, feats)
    assert float(ft.encoder.arena.flat_g.abs().sum()) == 0       # nothing ran backward


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("f32_residual", [False, True], ids=["res16", "res32"])
@pytest.mark.parametrize("pool", ["avg", "cls"])
def test_forward_only_bits_equal_the_differentiable_path_bits(dev, pool, f32_residual, dtype):
    """One encoder body (ECAMPClassifier._features) with and without gradients: the logits of the training-mode forward are the bits of
    `forward_features` through the head.  vit_tiny_patch16 at 32 x 32 pixels: four patches, five tokens, B = 3."""
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module.classifier import build_classifier
    torch.manual_seed(0)
    clf = build_classifier("vit_tiny_patch16", C, True, img_size=32, pool=pool, train_encoder=True, compute_dtype=dtype, f32_residual=f32_residual)
    with torch.no_grad():
        for k, v in _tail_values().items():
            clf.get_parameter(k).copy_(v)
    clf.to(dev).train()
    imgs = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(11))
    a = clf(imgs)
    assert a.requires_grad and a.grad_fn is not None
    feats = clf.forward_features(imgs)
    assert not feats.requires_grad and feats.shape == (3, 192)
    b = ops.cls_head_fwd(feats, clf.head.weight.data, clf.head.bias.data)
    assert torch.isfinite(b).all() and float(b.abs().max()) > 0
    assert torch.equal(a.detach(), b)


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_driver_trains_writes_the_flat_checkpoint_and_tests_it(dev, tmp_path, monkeypatch):
    from ecamp_amd import main_finetune
    from ecamp_amd.module.classifier import ECAMPClassifier
    out = str(tmp_path / "run")
    common = ["--name", "t", "--model", "vit_tiny_patch16", "--task", "CheXpert", "--num_classes", "5", "--output_dir", out, "--img_size", "224",
              "--train_batch_size", "8", "--eval_batch_size", "16", "--learning_rate", "3e-2", "--warmup_steps", "1",
              "--synthetic", "--synthetic_len", "16", "--num_workers", "0", "--print_freq", "2"]
    probe_imgs = _imgs(3, seed=77)
    built, initial, at_save = [], [], []
    real_build, real_sd = main_finetune.build_model, ECAMPClassifier.reference_state_dict

    def build_model(args):
        m = real_build(args)
        built.append(m)
        initial.append(real_sd(m))
        return m

    def reference_state_dict(self):      # what the in-memory model computes at the moment its checkpoint is written
        with torch.no_grad():
            at_save.append(self(probe_imgs).clone())
        return real_sd(self)

    monkeypatch.setattr(main_finetune, "build_model", build_model)
    monkeypatch.setattr(ECAMPClassifier, "reference_state_dict", reference_state_dict)
    parse = main_finetune.get_args_parser().parse_args
    res = main_finetune.main(parse(common + ["--stage", "train", "--num_steps", "4"]))
    path = os.path.join(out, "t_bestauc_checkpoint.bin")
    assert os.path.exists(path) and len(res["aurocs"]) == 5 and len(built) == 2 and built[0].train_encoder and len(at_save) >= 1
    sd = torch.load(path, map_location="cpu")
    assert sd["head.weight"].shape == (5, 192) and "fc_norm.weight" in sd and not any(k.startswith(("decoder", "bert", "norm.")) for k in sd)
    # the encoder was trained: a probe run's checkpoint would hold the initial encoder
    moved = [k for k in sd if k.startswith("blocks.") and not torch.equal(sd[k], initial[0][k])]
    assert len(moved) == sum(k.startswith("blocks.") for k in sd) and not torch.equal(sd["cls_token"], initial[0]["cls_token"])
    assert torch.equal(sd["pos_embed"], initial[0]["pos_embed"])
    # the reloaded model (the second one built: the test stage) computes the bits of the in-memory one
    with torch.no_grad():
        reloaded = built[1](probe_imgs)
    assert torch.equal(reloaded, at_save[-1])
    res2 = main_finetune.main(parse(common + ["--stage", "test"]))
    assert res2["loss"] == res["loss"] and len(built) == 3
    np.testing.assert_array_equal(np.array(res2["aurocs"]), np.array(res["aurocs"]))
    with torch.no_grad():
        assert torch.equal(built[2](probe_imgs), reloaded)
    log = open(os.path.join(out, "log.txt")).read()
    first = log.splitlines()[0]
    assert "stochastic depth" in first and "NOT applied" in first and "pos_embed" in first and "fixed" in first
    for line in ("Training (4 / 4 Steps)", "Valid Loss:", "Valid Auc:", "Saved model checkpoint", "Test Loss:", "Test Accuracy:", "The average AUROC is",
                 "The AUROC of class 4 is", "Total Parameter: \t%2.4fM" % (sum(p.numel() for _, p in built[0].finetune_parameters()) / 1e6)):
        assert line in log, line
    assert log.count("Test Loss:") == 2 and log.count("Valid Auc:") == 2             # 16 samples / 8 = two passes of two steps
