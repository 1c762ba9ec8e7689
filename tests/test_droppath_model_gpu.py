"""-m gpu: stochastic depth in encoder fine-tuning at the model and driver level, on ecamp_tiny with the oracle's recipe weights (B = 4,
R = 224, C = 3), built as tests/test_finetune_model_gpu.py builds it.  The reference is the float64 block of tests/_droppath_ref.py under
torch autograd on the CPU, run under the SAME keep masks: they are rebuilt from the model's Philox trace through the development ABI
(hip_ops.dropout_mask).  drop_path_rate = 0.5 so that a batch of four really drops samples; the bars are the project's own
(tests/test_finetune_model_gpu.py), not new ones.  Measured values: profiles/finetune_droppath.txt."""
import functools
import os

import _droppath_ref as ref
import numpy as np
import pytest
import test_finetune_model_gpu as ft
import torch

pytestmark = pytest.mark.gpu

B, C = ft.B, ft.C
RATE = 0.5
DEPTH = 12


def _build(dtype, dev, rate=RATE, seed=0, **kw):
    """ft._build with a stochastic-depth rate (`rate` None: the constructor argument is not passed at all)."""
    from ecamp_amd.module import model_ecamp as me
    from ecamp_amd.module.classifier import ECAMPClassifier
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    pool, multilabel = kw.pop("pool", "avg"), kw.pop("multilabel", True)
    torch.manual_seed(seed)
    enc = me.ecamp_tiny(compute_dtype=dtype, **kw)
    enc.load_state_dict(recipe.recipe_state(orc.cfg_tiny(), seed=0), strict=True)
    extra = {} if rate is None else {"drop_path_rate": rate}
    clf = ECAMPClassifier(enc, C, multilabel=multilabel, pool=pool, train_encoder=True, **extra)
    with torch.no_grad():
        for k, v in ft._tail_values().items():
            clf.get_parameter(k).copy_(v)
    clf = clf.to(dev)
    clf.encoder.prepare()          # the Philox key is taken from torch.initial_seed() here: under THIS build's torch.manual_seed
    return clf


def _masks_from_trace(clf, trace, dev):
    """{block: (keep of the attention branch, keep of the MLP branch)} as float64 [B] on the CPU, from the (seed, offset) pairs one
    forward drew: two per block of a rate above 0, in block order, attention first."""
    from ecamp_amd import hip_ops as ops
    active = [i for i, r in enumerate(clf.drop_path_rates) if r > 0]
    assert len(trace) == 2 * len(active)
    masks, it = {}, iter(trace)
    for i in active:
        pair = []
        for _ in range(2):
            seed, off = next(it)
            pair.append(ops.dropout_mask((B,), dev, clf.drop_path_rates[i], seed, off).cpu().double())
        masks[i] = tuple(pair)
    return masks


@functools.lru_cache(maxsize=None)
@ft._with_threads
def _reference(pool, rates, mask_key):
    """One float64 backward under the given masks -> (loss, {name: gradient}); keyed by the masks' bytes, computed once per distinct set."""
    masks = {i: (torch.tensor(a, dtype=torch.float64), torch.tensor(m, dtype=torch.float64)) for i, a, m in mask_key}
    P, cfg = ft._ref_params(pool)
    loss = ref.classifier_loss(P, cfg, ft._imgs(), ft._labels(True), True, pool, list(rates), masks)
    loss.backward()
    return float(loss.detach()), {k: P[k].grad.clone() for k in ft._trained_names(pool)}


def _traced_backward(clf, dev, scale=1.0):
    clf.encoder.prepare()
    clf.encoder._rng_trace = []
    loss = ft._backward(clf, True, scale=scale)
    trace, clf.encoder._rng_trace = clf.encoder._rng_trace, None
    masks = _masks_from_trace(clf, trace, dev)
    dropped = sum(int((1 - a).sum() + (1 - m).sum()) for a, m in masks.values())
    mixed = sum(0 < float(k.sum()) < B for pair in masks.values() for k in pair)
    print("[droppath] rate %.2f: %d of %d sample-branches dropped over %d sites, %d sites with both kinds" % (clf.drop_path_rate, dropped, 2 * 11 * B, len(trace), mixed))
    # precondition, reported and never skipped: the draw must exercise both the dropped and the kept path (another torch.manual_seed otherwise)
    assert dropped >= 8 and mixed >= 1, "precondition: the seed drops %d sample-branches (%d mixed sites) -- build with another seed" % (dropped, mixed)
    key = tuple((i, tuple(a.tolist()), tuple(m.tolist())) for i, (a, m) in sorted(masks.items()))
    return loss, trace, key


CASES = [(torch.float32, "avg", False), (torch.float32, "cls", False), (torch.bfloat16, "avg", False), (torch.bfloat16, "avg", True), (torch.float16, "avg", False)]


@pytest.mark.parametrize("dtype,pool,f32_residual", CASES, ids=["f32-avg", "f32-cls", "bf16", "bf16-f32residual", "f16"])
def test_one_backward_against_float64_under_the_same_masks(dev, dtype, pool, f32_residual):
    """f32 compute: loss 2e-4, every trained tensor's gradient 1e-3 of its largest element.  bf16 and bf16 with the f32 residual stream:
    loss 3e-2, per-tensor gradient norms median 1e-2 / worst 6e-2.  IEEE half with the loss scaled by 65536: 1e-3, 2e-3 / 1e-2 (norms of
    the tensors above 1e-3 of the largest norm, as tests/test_finetune_model_gpu.py takes them).  Decoder and report side keep a zero
    gradient."""
    lscale = 65536.0 if dtype == torch.float16 else 1.0
    clf = _build(dtype, dev, pool=pool, f32_residual=f32_residual)
    ctr0 = clf.encoder._rng_ctr
    loss, trace, key = _traced_backward(clf, dev, scale=lscale)
    assert clf.encoder._rng_ctr == ctr0 + 22 and [o for _, o in trace] == list(range(ctr0 + 1, ctr0 + 23))
    loss_ref, grads_ref = _reference(pool, tuple(clf.drop_path_rates), key)
    named = ft._named(clf)
    assert sorted(named) == sorted(grads_ref)
    el = abs(loss - loss_ref) / abs(loss_ref)
    names = sorted(grads_ref)
    rn = np.array([float(grads_ref[k].norm()) for k in names])
    gn = np.array([float(named[k].grad.double().norm()) / lscale for k in names])
    big = rn > 1e-3 * rn.max()
    nerr = np.abs(gn - rn)[big] / rn[big]
    tag = "%s %s%s" % (str(dtype).split(".")[-1], pool, " f32_residual" if f32_residual else "")
    if dtype == torch.float32:
        errs = {k: ft.rel(named[k].grad, grads_ref[k]) for k in grads_ref}
        worst = max(errs, key=errs.get)
        print("[droppath] one backward %s: loss %.2e (bar 2e-4); gradients worst element / max %.2e (%s; bar 1e-3), median %.2e"
              % (tag, el, errs[worst], worst, float(np.median(list(errs.values())))))
        assert el <= 2e-4 and errs[worst] <= 1e-3, (el, worst, errs[worst])
    else:
        ltol, med_tol, max_tol = (1e-3, 2e-3, 1e-2) if dtype == torch.float16 else (3e-2, 1e-2, 6e-2)
        print("[droppath] one backward %s: loss %.2e (bar %.0e); gradient norms of %d tensors: median %.2e (bar %.0e) worst %.2e (bar %.0e, %s)"
              % (tag, el, ltol, int(big.sum()), np.median(nerr), med_tol, nerr.max(), max_tol, np.array(names)[big][int(nerr.argmax())]))
        assert big.sum() > 60 and el <= ltol
        assert np.median(nerr) <= med_tol and nerr.max() <= max_tol
    A = clf.encoder.arena
    A.flush_fresh()
    others = ft._untrained_arena_mask(clf)
    assert bool(others.any()) and torch.all(A.flat_g.cpu()[others] == 0), "decoder / report-side gradients must stay zero"


def test_the_trace_has_two_pairs_per_active_block_in_block_order(dev):
    """Rates linspace(0, r, 12): block 0 has rate 0 and draws nothing, every other block draws two pairs per forward, attention then MLP;
    the counter moves by exactly that.  The masks of one site differ between its two branches and between two forwards."""
    clf = _build(torch.bfloat16, dev, rate=0.5)
    m = clf.encoder
    m.prepare()
    assert clf.drop_path_rates[0] == 0.0 and all(r > 0 for r in clf.drop_path_rates[1:])
    clf.train()
    ctr0, m._rng_trace = m._rng_ctr, []
    clf(ft._imgs())
    first, m._rng_trace = m._rng_trace, []
    clf(ft._imgs())
    second, m._rng_trace = m._rng_trace, None
    assert len(first) == len(second) == 2 * (DEPTH - 1)
    assert [o for _, o in first + second] == list(range(ctr0 + 1, ctr0 + 1 + 4 * (DEPTH - 1))) and len({s for s, _ in first + second}) == 1
    a, b = _masks_from_trace(clf, first, dev), _masks_from_trace(clf, second, dev)
    assert any(not torch.equal(a[i][0], a[i][1]) for i in a) and any(not torch.equal(a[i][0], b[i][0]) for i in a)


def _logits_and_grads(clf, train=True):
    clf.train(train)
    logits = clf(ft._imgs())
    clf.loss(logits, ft._labels(True)).backward()
    torch.cuda.synchronize()
    clf.encoder.arena.flush_fresh()
    return logits.detach().clone(), {k: p.grad.detach().clone() for k, p in clf.finetune_parameters()}


def _gemm_written(k, g):
    """The gradients that a weight-gradient GEMM WRITES, in one fixed order: the matrices.  Biases, LayerNorm parameters and cls_token are
    ACCUMULATED with float atomics (bias row sums of the GEMMs, ecamp_layernorm_bwd, ecamp_colsum), whose order -- and so whose last bits --
    vary between two backwards of ONE model."""
    return g.dim() >= 2 and k != "cls_token"


def _assert_same_backward(ga, gb, gc, what):
    """gb against ga.  Matrices: the same bits.  Atomically accumulated tensors have no bits of their own to equal, so they are held to the
    reference's own error: `gc` is a second backward of the reference model, and gb may differ from ga by at most four times the largest
    relative difference (of a tensor's largest element) that ga and gc show over all such tensors, plus one f32 ulp."""
    assert sorted(ga) == sorted(gb) == sorted(gc)
    acc = [k for k in ga if not _gemm_written(k, ga[k])]
    assert len(acc) > 60 and len(acc) < len(ga)
    spread = max(float((ga[k] - gc[k]).abs().max() / ga[k].abs().max()) for k in acc)
    worst = 0.0
    for k in ga:
        if _gemm_written(k, ga[k]):
            assert torch.equal(ga[k], gb[k]), (what, k)
        else:
            d = float((ga[k] - gb[k]).abs().max() / ga[k].abs().max())
            worst = max(worst, d)
            assert d <= 4 * spread + 2.0 ** -23, (what, k, d, spread)
    print("[droppath] %s: matrices bit-equal; accumulated tensors differ by %.2e of their largest element (the reference against itself: %.2e)"
          % (what, worst, spread))


@pytest.mark.parametrize("dtype,f32_residual", [(torch.bfloat16, False), (torch.bfloat16, True), (torch.float32, False)], ids=["bf16", "bf16-f32residual", "f32"])
def test_rate_zero_is_the_model_built_without_the_argument(dev, dtype, f32_residual, monkeypatch):
    """Logits, the Philox counter and every matrix gradient: the same bits.  Every VitBlockFn call of the rate-0 model has the six
    arguments it always had, so the same kernels see the same inputs; the gradients that are accumulated with float atomics are compared
    as _assert_same_backward says (two backwards of the model built WITHOUT the argument do not agree in their last bits either)."""
    from ecamp_amd.functions import VitBlockFn
    plain = _build(dtype, dev, rate=None, f32_residual=f32_residual)
    again = _build(dtype, dev, rate=None, f32_residual=f32_residual)
    zero = _build(dtype, dev, rate=0.0, f32_residual=f32_residual)
    c0 = zero.encoder._rng_ctr
    assert c0 == plain.encoder._rng_ctr and zero.encoder._rng_seed == plain.encoder._rng_seed
    la, ga = _logits_and_grads(plain)
    lc, gc = _logits_and_grads(again)
    nargs, real = [], VitBlockFn.apply
    monkeypatch.setattr(VitBlockFn, "apply", lambda *a: (nargs.append(len(a)), real(*a))[1])
    lb, gb = _logits_and_grads(zero)
    monkeypatch.undo()
    assert nargs == [6] * DEPTH
    assert torch.equal(la, lb) and torch.equal(la, lc)
    _assert_same_backward(ga, gb, gc, "rate 0 against no argument, %s%s" % (str(dtype).split(".")[-1], " f32_residual" if f32_residual else ""))
    assert zero.encoder._rng_ctr == c0 == plain.encoder._rng_ctr, "a rate-0 model draws nothing"


def test_outside_training_a_rate_05_model_is_the_rate_0_model(dev):
    """eval(), no_grad and forward_features apply no stochastic depth: the bits of the rate-0 model, and the Philox counter stays."""
    imgs = ft._imgs()
    zero = _build(torch.bfloat16, dev, rate=0.0)
    half = _build(torch.bfloat16, dev, rate=0.5)
    zero.eval()
    want, feats = zero(imgs).detach(), zero.forward_features(imgs)
    half.encoder.prepare()
    c0 = half.encoder._rng_ctr
    half.train()
    with torch.no_grad():
        a = half(imgs)
    f = half.forward_features(imgs)
    fc = half.forward_features(imgs, pool="cls")
    half.eval()
    b = half(imgs)
    with torch.no_grad():
        c = half(imgs)
    assert torch.equal(a, want) and torch.equal(b.detach(), want) and torch.equal(c, want) and torch.equal(f, feats)
    assert torch.equal(fc, zero.forward_features(imgs, pool="cls"))
    assert half.encoder._rng_ctr == c0
    half.train()                                   # ... and in training it is another function, which draws
    d = half(imgs)
    assert half.encoder._rng_ctr == c0 + 22 and not torch.equal(d.detach(), want)


def test_the_draw_follows_torch_manual_seed(dev):
    imgs = ft._imgs()
    a, b, c = (_build(torch.bfloat16, dev, rate=0.5, seed=s) for s in (3, 3, 4))
    for m in (a, b, c):
        m.train()
    la, ga = _logits_and_grads(a)
    lb, gb = _logits_and_grads(b)
    assert torch.equal(la, lb), "the same seed gives the same bits"
    assert all(torch.equal(ga[k], gb[k]) for k in ga if _gemm_written(k, ga[k])), "the same seed gives the same matrix gradients, bit for bit"
    assert not torch.equal(la, c(imgs).detach()), "another seed draws other masks"


def test_vit_block_refuses_stochastic_depth_beside_the_fp8_forward(dev):
    from ecamp_amd.functions import VitBlockFn
    clf = _build(torch.bfloat16, dev, rate=0.0)
    m = clf.encoder
    m.prepare()
    x = torch.zeros(2 * 5, 192, dtype=torch.bfloat16, device=dev)
    m.fp8_forward = True
    try:
        with pytest.raises(RuntimeError, match="fp8"):
            VitBlockFn.apply(x, m.blocks[0], m, 2, 5, m.num_heads, 0.25)
    finally:
        m.fp8_forward = False


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_driver_trains_with_stochastic_depth_and_tests_the_checkpoint(dev, tmp_path):
    from ecamp_amd import main_finetune
    out = str(tmp_path / "run")
    common = ["--name", "t", "--model", "vit_tiny_patch16", "--task", "CheXpert", "--num_classes", "5", "--output_dir", out, "--img_size", "224",
              "--train_batch_size", "8", "--eval_batch_size", "16", "--learning_rate", "3e-2", "--warmup_steps", "1",
              "--synthetic", "--synthetic_len", "16", "--num_workers", "0", "--print_freq", "2", "--drop_path_rate", "0.1"]
    parse = main_finetune.get_args_parser().parse_args
    res = main_finetune.main(parse(common + ["--stage", "train", "--num_steps", "4"]))
    path = os.path.join(out, "t_bestauc_checkpoint.bin")
    assert os.path.exists(path) and len(res["aurocs"]) == 5 and np.isfinite(res["loss"])
    sd = torch.load(path, map_location="cpu")
    assert sd["head.weight"].shape == (5, 192) and "fc_norm.weight" in sd and not any(k.startswith(("decoder", "bert", "norm.")) for k in sd)
    res2 = main_finetune.main(parse(common + ["--stage", "test"]))      # evaluation is deterministic: no stochastic depth outside training
    assert res2["loss"] == res["loss"]
    np.testing.assert_array_equal(np.array(res2["aurocs"]), np.array(res["aurocs"]))
    log = open(os.path.join(out, "log.txt")).read()
    first = log.splitlines()[0]
    assert "stochastic depth" in first and "IS applied" in first and "0.1" in first and "NOT applied" not in first and "pos_embed" in first
    for line in ("Training (4 / 4 Steps)", "Valid Auc:", "Saved model checkpoint", "Test Loss:"):
        assert line in log, line
    assert log.count("Test Loss:") == 2
