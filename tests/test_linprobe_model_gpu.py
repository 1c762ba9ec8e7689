"""-m gpu: the linear probe at the model, engine and driver level, on ecamp_tiny with the oracle's recipe weights (B = 4, R = 224):
ECAMPClassifier.forward_features against the oracle's encoder, its isolation from the pre-training state, the head's gradient
against torch autograd in float64, six engine steps against a float64 replay on the CPU, and the checkpoint / driver round trip."""
import argparse
import os

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


def _build(dtype, dev, multilabel=True, pool="avg", **kw):
    from ecamp_amd.module import model_ecamp as me
    from ecamp_amd.module.classifier import ECAMPClassifier
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    torch.manual_seed(0)
    enc = me.ecamp_tiny(compute_dtype=dtype, **kw)
    enc.load_state_dict(recipe.recipe_state(orc.cfg_tiny(), seed=0), strict=True)
    clf = ECAMPClassifier(enc, C, multilabel=multilabel, pool=pool)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():   # a probe in mid-training: no identity norm, no vanishing head
        clf.fc_norm.weight.copy_(1 + 0.2 * torch.randn(192, generator=g))
        clf.fc_norm.bias.copy_(0.1 * torch.randn(192, generator=g))
        clf.head.weight.copy_(0.1 * torch.randn(C, 192, generator=g))
        clf.head.bias.copy_(0.1 * torch.randn(C, generator=g))
    return clf.to(dev)


@pytest.fixture(scope="module")
def oracle():
    """The oracle's encoder on the test images, once: tokens before `norm` (stem, vit_block x depth with every patch kept in place), the
    float64 pool-and-norm of them under the test's fc_norm, and image_encoder's own output (after `norm`)."""
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    cfg = orc.cfg_tiny()
    P = orc.load_state(orc.new_params(cfg), recipe.recipe_state(cfg, seed=0))
    imgs = _imgs()
    threads = torch.get_num_threads()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    with torch.no_grad():
        x = F.conv2d(imgs, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=cfg.patch_size).flatten(2).transpose(1, 2)
        x = x + P["pos_embed"][:, 1:, :]
        x = torch.cat(((P["cls_token"] + P["pos_embed"][:, :1, :]).expand(B, -1, -1), x), dim=1)
        for i in range(cfg.depth):
            x = orc.vit_block(P, "blocks.%d" % i, x, cfg.num_heads, cfg.ln_eps)
        noise = (torch.arange(cfg.num_patches, dtype=torch.float32) / cfg.num_patches).expand(B, -1).contiguous()
        latent = orc.image_encoder(P, cfg, imgs, 0.0, noise)[0]
    torch.set_num_threads(threads)   # (process-wide: given back for the tests that follow)
    assert rel(F.layer_norm(x, (192,), P["norm.weight"], P["norm.bias"], cfg.ln_eps), latent) < 1e-6   # the same tokens, in place
    return {"imgs": imgs, "tokens": x, "latent": latent, "noise": noise}


def _feat_ref(clf, tokens):
    w, b = clf.fc_norm.weight.detach().double().cpu(), clf.fc_norm.bias.detach().double().cpu()
    return F.layer_norm(tokens.double()[:, 1:, :].mean(dim=1), (tokens.shape[-1],), w, b, 1e-6)


def test_features_against_the_oracle_in_f32(dev, oracle):
    clf = _build(torch.float32, dev)
    f = clf.forward_features(oracle["imgs"])
    assert f.shape == (B, 192) and f.dtype == torch.float32
    e = rel(f, _feat_ref(clf, oracle["tokens"]))
    print("[linprobe] f32 features (avg) vs oracle: %.2e (bar 2e-4)" % e)
    assert e <= 2e-4
    c = clf.forward_features(oracle["imgs"], pool="cls")
    ec = rel(c, oracle["latent"][:, 0])
    print("[linprobe] f32 features (cls) vs oracle: %.2e (bar 2e-4)" % ec)
    assert c.shape == (B, 192) and c.dtype == torch.float32 and ec <= 2e-4
    assert torch.equal(f, clf.forward_features(oracle["imgs"])) and torch.equal(c, clf.forward_features(oracle["imgs"], pool="cls"))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_features_in_16_bits_stay_within_twice_the_encoders_own_error(dev, oracle, dtype):
    """The bar is not fixed in advance: it is twice the error, on the same relative scale, of the existing `image_encoder(mask_ratio=0)`
    output against the oracle in this format.  Measured on an MI355X (profiles/linprobe.txt)."""
    clf = _build(dtype, dev)
    with torch.no_grad():
        lat = clf.encoder.image_encoder(oracle["imgs"], 0.0, noise=oracle["noise"])[0]
    e_enc = rel(lat.float(), oracle["latent"])
    ref = _feat_ref(clf, oracle["tokens"])
    f = clf.forward_features(oracle["imgs"])
    e_feat = rel(f, ref)
    res = _build(dtype, dev, f32_residual=True)
    f_res = res.forward_features(oracle["imgs"])
    e_res = rel(f_res, ref)
    e_cls = rel(clf.forward_features(oracle["imgs"], pool="cls"), oracle["latent"][:, 0])
    name = str(dtype).split(".")[-1]
    print("[linprobe] %s encoder output vs oracle %.3e | features (avg) %.3e | with f32_residual %.3e | (cls) %.3e | bar 2 x encoder = %.3e"
          % (name, e_enc, e_feat, e_res, e_cls, 2 * e_enc))
    assert f.dtype == f_res.dtype == torch.float32
    assert torch.equal(f, clf.forward_features(oracle["imgs"])) and torch.equal(f_res, res.forward_features(oracle["imgs"]))
    assert e_feat <= 2 * e_enc, (e_feat, e_enc)
    assert e_res <= 2 * e_enc, (e_res, e_enc)


def _recipe_batch():
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    return recipe.recipe_batch(orc.cfg_tiny(), 2, 64, seed=5)


def test_a_probe_call_leaves_the_pretraining_state_alone(dev):
    """Two identical models in train mode (dropout draws from the model's Philox counter): one probes between its steps.  Counter,
    modes, gradient arena and every .grad are as they were; the next forward / forward_eval give the losses of the model that never
    probed (to 1e-5: their sums are float-atomic)."""
    batch, imgs = _recipe_batch(), _imgs(2, seed=3)
    runs = []
    for probe in (False, True):
        clf = _build(torch.bfloat16, dev)
        m = clf.encoder
        clf.train()
        clf.fc_norm.eval()
        m.blocks[2].eval()
        sum(m(batch)).backward()
        if probe:
            A = m.arena
            ctr, modes = m._rng_ctr, [(mod, mod.training) for mod in clf.modules()]
            flat_g, ptr_g = A.flat_g.clone(), A.flat_g.data_ptr()
            grads = [(p, p.grad.data_ptr()) for p in m.parameters() if p.grad is not None]
            assert float(flat_g.abs().sum()) > 0 and len(grads) > 100
            f = clf.forward_features(imgs)
            f2 = clf.forward_features(imgs, pool="cls")
            torch.cuda.synchronize()
            assert f.requires_grad is False and f2.requires_grad is False
            assert m._rng_ctr == ctr and ctr > 0
            assert all(mod.training is mode for mod, mode in modes) and m.training and not m.blocks[2].training and not clf.fc_norm.training
            assert m.arena is A and A.flat_g.data_ptr() == ptr_g and torch.equal(A.flat_g, flat_g)
            assert all(p.grad is not None and p.grad.data_ptr() == q for p, q in grads)
            assert all(p.grad is None for p in (clf.head.weight, clf.head.bias, clf.fc_norm.weight, clf.fc_norm.bias))
        nxt = [t.item() for t in m(batch)]
        ev = m.forward_eval(batch)
        runs.append(nxt + [ev["mim_loss"].item(), ev["res_loss"].item(), ev["mlm_loss"].item(), int(ev["mlm_counts"][0])])
    print("[linprobe] losses without / with a probe call in between:", runs)
    assert runs[1][:6] == pytest.approx(runs[0][:6], rel=1e-5) and runs[1][6] == runs[0][6]


@pytest.mark.parametrize("multilabel", [True, False], ids=["bce", "ce"])
def test_head_gradient_matches_autograd_in_float64(dev, multilabel):
    clf = _build(torch.bfloat16, dev, multilabel=multilabel)
    imgs = _imgs()
    g = torch.Generator().manual_seed(2)
    y = (torch.rand(B, C, generator=g) < 0.5).float() if multilabel else torch.randint(0, C, (B, 1), generator=g).float()   # (as the dataset hands them over)
    feats = clf.forward_features(imgs)
    A = clf.encoder.arena
    flat_g = A.flat_g.clone()
    logits = clf(imgs)
    loss = clf.loss(logits, y)
    loss.backward()
    clf.check_labels()
    assert logits.shape == (B, C) and logits.dtype == torch.float32 and loss.dim() == 0
    assert clf.fc_norm.weight.grad is None and clf.fc_norm.bias.grad is None and torch.equal(A.flat_g, flat_g)
    W = clf.head.weight.detach().double().cpu().requires_grad_(True)
    b = clf.head.bias.detach().double().cpu().requires_grad_(True)
    lr = feats.double().cpu() @ W.t() + b
    ref = F.binary_cross_entropy_with_logits(lr, y.double()) if multilabel else F.cross_entropy(lr, y.reshape(-1).long())
    ref.backward()
    e = (rel(logits, lr), rel(loss, ref), rel(clf.head.weight.grad, W.grad), rel(clf.head.bias.grad, b.grad))
    print("[linprobe] head (%s) vs float64 autograd: logits %.2e loss %.2e dW %.2e db %.2e" % ((("bce" if multilabel else "ce"),) + e))
    assert e[0] <= 2e-4 and e[1] <= 2e-4 and e[2] <= 1e-3 and e[3] <= 1e-3
    assert clf.last_counts.tolist()[0] == B
    # a second backward accumulates, as autograd does for any parameter
    clf.loss(clf(imgs), y).backward()
    assert rel(clf.head.weight.grad, 2 * W.grad) <= 1e-3
    if not multilabel:
        clf.loss(clf(imgs), torch.tensor([0, 1, C, 0]))
        with pytest.raises(Exception, match="outside"):
            clf.check_labels()


def _engine_args(**kw):
    a = argparse.Namespace(learning_rate=0.05, weight_decay=0.0, decay_type="cosine", warmup_steps=2, num_steps=6, max_grad_norm=1.0,
                           train_batch_size=8, print_freq=100, output_dir="", name="t", ratio=1.0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _replay(feats, ys, W0, b0, args):
    """The six steps on the CPU in float64: torch's BCEWithLogitsLoss, clip_grad_norm_, SGD with momentum 0.9, the schedule stepped first."""
    from ecamp_amd import engine_linprobe as engine
    W, b = W0.clone().double().requires_grad_(True), b0.clone().double().requires_grad_(True)
    opt = torch.optim.SGD([W, b], lr=args.learning_rate, momentum=0.9, weight_decay=args.weight_decay)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: engine.lr_factor(args.decay_type, s, args.warmup_steps, args.num_steps))
    loss_fct = torch.nn.BCEWithLogitsLoss()
    losses, coefs, norms = [], [], []
    for step in range(args.num_steps):
        f, y = feats[step % len(feats)], ys[step % len(ys)]
        loss = loss_fct(f @ W.t() + b, y.double())
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_([W, b], args.max_grad_norm)
        norms.append(float(norm))
        coefs.append(min(1.0, args.max_grad_norm / (float(norm) + 1e-6)))
        sched.step()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss))
    return W.detach(), b.detach(), losses, coefs, norms


def test_six_engine_steps_replay_on_the_cpu_in_float64(dev):
    from ecamp_amd import engine_linprobe as engine
    clf = _build(torch.bfloat16, dev)
    g = torch.Generator().manual_seed(9)
    xs = [_imgs(8, seed=20 + i) for i in range(3)]                        # a fixed tensor dataset, no augmentation: two passes of three batches
    ys = [(torch.rand(8, C, generator=g) < 0.5).float() for _ in range(3)]
    feats = [clf.forward_features(x).double().cpu() for x in xs]
    W0, b0 = clf.head.weight.detach().cpu().clone(), clf.head.bias.detach().cpu().clone()
    # a clip threshold between two of the gradient norms an unclipped dry replay meets -- the first such midpoint (from the largest norms
    # down) under which the replay proper shows the coefficient below 1 on some step and equal to 1 on another; both are asserted
    # below, so neither branch of the clip goes untested
    dry = _replay(feats, ys, W0, b0, _engine_args(max_grad_norm=1e9))
    assert all(c == 1.0 for c in dry[3])
    ordered = sorted(dry[4], reverse=True)
    args = None
    for hi, lo in zip(ordered, ordered[1:]):
        cand = _engine_args(max_grad_norm=(hi * lo) ** 0.5)
        coefs = _replay(feats, ys, W0, b0, cand)[3]
        if any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs):
            args = cand
            break
    assert args is not None, ("no threshold between the dry replay's norms exercises both branches", dry[4])
    Wr, br, losses_r, coefs, norms = _replay(feats, ys, W0, b0, args)
    print("[linprobe] replay clip coefficients:", ["%.3f" % c for c in coefs], "gradient norms:", ["%.3f" % n for n in norms], "max_grad_norm %.3f" % args.max_grad_norm)
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs)
    out = engine.train(clf, list(zip(xs, ys)), None, args, log=lambda m: None, keep_losses=True)
    assert out["global_step"] == 6 and len(out["losses"]) == 6
    losses = [float(t.item()) for t in out["losses"]]
    eW, eb = rel(clf.head.weight, Wr), rel(clf.head.bias, br)
    el = max(abs(a - r) / abs(r) for a, r in zip(losses, losses_r))
    print("[linprobe] engine vs float64 replay after 6 steps: head.weight %.2e head.bias %.2e losses %.2e (bar 1e-4)" % (eW, eb, el))
    assert eW <= 1e-4 and eb <= 1e-4 and el <= 1e-4
    assert rel(clf.head.weight, W0) > 1e-2 and losses_r[3] < losses_r[0]           # it moved, and downhill: the first batch again, one pass later
    assert clf.head.weight.grad is None and all(p.grad is None for p in clf.fc_norm.parameters())


def test_a_bad_label_in_any_batch_is_reported_not_only_in_the_last(dev):
    """The kernel's label flag is folded into a running device flag: a class index outside [0, C) in the FIRST of three batches raises
    where the engine reads the loss (here: at the last step, and at the end of an evaluation pass), and the flag is cleared by the report."""
    from ecamp_amd import engine_linprobe as engine
    clf = _build(torch.bfloat16, dev, multilabel=False)
    xs = [_imgs(4, seed=40 + i) for i in range(3)]
    good = [torch.tensor([[0.0], [1.0], [2.0], [1.0]]) for _ in range(3)]
    bad = [torch.tensor([[0.0], [float(C)], [2.0], [1.0]])] + good[1:]
    args = _engine_args(num_steps=3, train_batch_size=4)
    with pytest.raises(Exception, match="outside"):
        engine.train(clf, list(zip(xs, bad)), None, args, log=lambda m: None)
    assert clf.bad_label is None                                   # reported once, then cleared
    with pytest.raises(Exception, match="outside"):
        engine.evaluate(clf, list(zip(xs, bad)), log=lambda m: None)
    out = engine.evaluate(clf, list(zip(xs, good)), log=lambda m: None)
    assert 0.0 <= out["accuracy"] <= 1.0 and out["confusion"].sum() == 12
    engine.train(clf, list(zip(xs, good)), None, args, log=lambda m: None)


def test_reference_checkpoint_round_trip_gives_the_same_bits(dev, tmp_path):
    clf = _build(torch.bfloat16, dev)
    imgs = _imgs()
    with torch.no_grad():
        want = clf(imgs)
    path = str(tmp_path / "t_bestauc_checkpoint.bin")
    torch.save(clf.reference_state_dict(), path)
    from ecamp_amd.module.classifier import build_classifier
    torch.manual_seed(123)
    fresh = build_classifier("vit_tiny_patch16", C, True, img_size=224, compute_dtype=torch.bfloat16)
    fresh.load_pretrained(path)
    fresh.to(dev)
    with torch.no_grad():
        got = fresh(imgs)
    assert torch.equal(got, want)


def test_driver_trains_and_tests_on_the_synthetic_stand_in(dev, tmp_path):
    from ecamp_amd import main_linprobe
    out = str(tmp_path / "run")
    common = ["--name", "t", "--model", "vit_tiny_patch16", "--task", "CheXpert", "--num_classes", "5", "--output_dir", out, "--img_size", "224",
              "--train_batch_size", "8", "--eval_batch_size", "16", "--learning_rate", "3e-2", "--warmup_steps", "1", "--mode", "LinearProbe",
              "--synthetic", "--synthetic_len", "16", "--num_workers", "0", "--print_freq", "2"]
    res = main_linprobe.main(main_linprobe.get_args_parser().parse_args(common + ["--stage", "train", "--num_steps", "4"]))
    assert os.path.exists(os.path.join(out, "t_bestauc_checkpoint.bin")) and len(res["aurocs"]) == 5
    sd = torch.load(os.path.join(out, "t_bestauc_checkpoint.bin"), map_location="cpu")
    assert sd["head.weight"].shape == (5, 192) and "fc_norm.weight" in sd and not any(k.startswith(("decoder", "bert")) for k in sd)
    res2 = main_linprobe.main(main_linprobe.get_args_parser().parse_args(common + ["--stage", "test"]))
    import numpy as np
    assert res2["loss"] == res["loss"]
    np.testing.assert_array_equal(np.array(res2["aurocs"]), np.array(res["aurocs"]))          # the same checkpoint on the same test set: the same bits
    log = open(os.path.join(out, "log.txt")).read()
    for line in ("Training (4 / 4 Steps)", "Valid Loss:", "Valid Auc:", "Saved model checkpoint", "Test Loss:", "Test Accuracy:", "The average AUROC is",
                 "The AUROC of class 4 is"):
        assert line in log, line
    assert log.count("Test Loss:") == 2 and log.count("Valid Auc:") == 2             # 16 samples / 8 = two passes of two steps
