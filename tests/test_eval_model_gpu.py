"""-m gpu: held-out evaluation at the model, engine and driver level -- `ECAMP.forward_eval` against the reference's golden losses
(tests/golden/tiny_b4_s128.npz, the inputs of oracle.recipe) and against counts formed on the host from its own logits,
`engine_pretrain.evaluate` against separate `forward_eval` calls, its isolation from the training state, and the driver's flags."""
import argparse
import json
import os
import random

import numpy as np
import pytest
import torch

from conftest import h16

pytestmark = pytest.mark.gpu

NAME = "tiny_b4_s128"
KEYS = ("val_mim_loss", "val_res_loss", "val_mlm_loss", "val_mlm_top1", "val_mlm_top5", "val_mlm_tokens")


def _gold():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", NAME + ".npz"), allow_pickle=False)


def _build(dtype, dev):
    from ecamp_amd.module import model_ecamp as me
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    cfg = orc.cfg_tiny()
    torch.manual_seed(0)
    model = me.ecamp_tiny(compute_dtype=dtype)
    model.load_state_dict(recipe.recipe_state(cfg, seed=0), strict=True)
    model.to(dev)
    return model, cfg


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def host_counts(logits, labels):
    """[scored, top1, top5] from logits [M, V] and labels [M] with the kernel's rank rule: logits strictly above the label's."""
    x = logits.detach().float().cpu().double()
    labels = labels.reshape(-1).cpu()
    V = x.shape[1]
    valid = (labels >= 0) & (labels < V)
    xl = x.gather(1, labels.clamp(0, V - 1)[:, None])
    rank = (x > xl).sum(1)
    return [int(valid.sum()), int((valid & (rank == 0)).sum()), int((valid & (rank < 5)).sum())]


def _losses(out):
    return np.array([out["mim_loss"].item(), out["res_loss"].item(), out["mlm_loss"].item()])


def _eval_golden_case(dev, dtype, tol):
    from oracle import recipe
    g = _gold()
    B, S = int(g["meta/B"]), int(g["meta/S"])
    model, cfg = _build(dtype, dev)
    model.train()              # evaluation semantics whatever the mode: the reference's dropout (p = 0.1) must not run
    model.keep_aux = True
    batch = recipe.recipe_batch(cfg, B, S, seed=0)
    noise = recipe.recipe_noise(B, cfg.num_patches, seed=0)
    out = model.forward_eval(batch, mask_ratio=0.75, noise=noise)
    assert set(out) == {"mim_loss", "res_loss", "mlm_loss", "mlm_counts"}
    assert all(out[k].is_cuda and out[k].dim() == 0 and not out[k].requires_grad for k in ("mim_loss", "res_loss", "mlm_loss"))
    assert out["mlm_counts"].dtype == torch.int64 and out["mlm_counts"].shape == (3,) and out["mlm_counts"].is_cuda
    assert model.training
    losses = _losses(out)
    print(NAME, dtype, "losses", losses, "golden", g["losses"], "rel", rel(losses, g["losses"]))
    assert rel(losses, g["losses"]) < tol
    assert (model._aux["ids_keep"].cpu().numpy() == g["ids_keep"]).all()
    logits = model._aux["logits"]
    assert logits.shape == (B * S, cfg.bert.vocab_size) and logits.dtype == dtype
    want = host_counts(logits, batch["labels"])
    got = out["mlm_counts"].cpu().tolist()
    print("  counts", got, "host", want)
    assert got == want and want[0] == B * S       # (the recipe labels every position)
    return model, cfg


def test_forward_eval_matches_reference_fp32(dev):
    _eval_golden_case(dev, torch.float32, 2e-4)


def test_forward_eval_16bit_within_tolerance(dev, both_halves):
    dtype = h16()
    _eval_golden_case(dev, dtype, 3e-2 if dtype == torch.bfloat16 else 1e-3)


def test_forward_eval_skips_ignored_labels(dev):
    """Labels of -100 (what the dataset's masker gives every unmasked position): the counts cover the labelled rows only, and the loss is
    the labelled rows' share of the same sum."""
    from oracle import recipe
    model, cfg = _build(torch.float32, dev)
    model.eval()
    model.keep_aux = True
    batch = recipe.recipe_batch(cfg, 4, 128, seed=0)
    noise = recipe.recipe_noise(4, cfg.num_patches, seed=0)
    keep = torch.zeros(4, 128, dtype=torch.bool)
    keep[:, 3::7] = True
    batch["labels"] = torch.where(keep, batch["labels"], torch.full_like(batch["labels"], -100))
    out = model.forward_eval(batch, noise=noise)
    logits = model._aux["logits"]
    want = host_counts(logits, batch["labels"])
    assert out["mlm_counts"].cpu().tolist() == want and want[0] == int(keep.sum())
    x = logits.float().cpu().double()
    lab = batch["labels"].reshape(-1)
    ce = torch.logsumexp(x, 1) - x.gather(1, lab.clamp(min=0)[:, None])[:, 0]
    ref = float((ce * batch["weights"].reshape(-1).double())[lab >= 0].sum() / lab.numel())
    assert abs(out["mlm_loss"].item() - ref) <= 1e-5 * abs(ref)


def _labels_near_the_top(logits, B, S):
    """Labels whose rank under `logits` cycles through 0..7 from row to row (lower where 16-bit logits tie), every third position
    ignored: random weights never rank a random label near the top, and counts of zero would check nothing."""
    top = logits.float().topk(8, dim=1).indices.cpu()
    r = torch.arange(top.shape[0]) % 8
    labels = top.gather(1, r[:, None]).view(B, S).clone()
    labels[:, 2::3] = -100
    return labels


def _three_batches(cfg, model, dev):
    """Recipe batches of 4, 4 and 2 samples, relabelled with `_labels_near_the_top` under the noise `evaluate` masks batch i with
    (labels do not enter the logits) -> (batches, host counts [scored, top1, top5] pooled over the three)."""
    from ecamp_amd import hip_ops
    from ecamp_amd.engine_pretrain import eval_noise_key
    from oracle import recipe
    batches = [recipe.recipe_batch(cfg, n, 128, seed=s) for n, s in ((4, 0), (4, 1), (2, 2))]
    keep_aux, model.keep_aux = model.keep_aux, True
    pooled = np.zeros(3, dtype=np.int64)
    for i, b in enumerate(batches):
        n = b["labels"].shape[0]
        model.forward_eval(b, mask_ratio=0.75, noise=hip_ops.uniform((n, cfg.num_patches), dev, *eval_noise_key(0, i)))
        b["labels"] = _labels_near_the_top(model._aux["logits"], n, 128)
        pooled += np.array(host_counts(model._aux["logits"], b["labels"]), dtype=np.int64)
    model.keep_aux = keep_aux
    assert 0 < pooled[1] < pooled[2] < pooled[0] < 10 * 128, pooled
    return batches, pooled


def test_forward_eval_counts_labels_near_the_top(dev, both_halves):
    """Labels placed at ranks 0..7 of the model's own logits: top-1 and top-5 are neither zero nor everything, and ties between 16-bit
    logits resolve by the strictly-greater rule."""
    from oracle import recipe
    model, cfg = _build(h16(), dev)
    model.keep_aux = True
    batch = recipe.recipe_batch(cfg, 4, 128, seed=3)
    noise = recipe.recipe_noise(4, cfg.num_patches, seed=3)
    model.forward_eval(batch, noise=noise)
    batch["labels"] = _labels_near_the_top(model._aux["logits"], 4, 128)
    out = model.forward_eval(batch, noise=noise)
    want = host_counts(model._aux["logits"], batch["labels"])
    got = out["mlm_counts"].cpu().tolist()
    print("  counts", got, "host", want)
    assert got == want and 0 < want[1] < want[2] < want[0] < 4 * 128


def test_evaluate_is_the_sample_weighted_mean_and_the_pooled_counts(dev):
    from ecamp_amd import hip_ops
    from ecamp_amd.engine_pretrain import eval_noise_key, evaluate
    model, cfg = _build(torch.bfloat16, dev)
    model.eval()
    batches, pooled = _three_batches(cfg, model, dev)
    stats = evaluate(model, batches, dev, epoch=3, args=argparse.Namespace(mask_ratio=0.75, prefetch=True))
    assert tuple(stats) == KEYS
    n_all, lsum, csum = 0, np.zeros(3), np.zeros(3, dtype=np.int64)
    for i, b in enumerate(batches):
        n = b["labels"].shape[0]
        noise = hip_ops.uniform((n, cfg.num_patches), dev, *eval_noise_key(0, i))
        out = model.forward_eval(b, mask_ratio=0.75, noise=noise)
        lsum += n * _losses(out)
        csum += np.array(out["mlm_counts"].cpu().tolist(), dtype=np.int64)
        n_all += n
    want = lsum / n_all
    got = np.array([stats["val_mim_loss"], stats["val_res_loss"], stats["val_mlm_loss"]])
    print("evaluate", got, "separate calls", want, "counts", csum)
    assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want))
    assert csum.tolist() == pooled.tolist()
    assert stats["val_mlm_tokens"] == int(csum[0])
    assert stats["val_mlm_top1"] == int(csum[1]) / int(csum[0]) and stats["val_mlm_top5"] == int(csum[2]) / int(csum[0])
    assert 0.0 <= stats["val_mlm_top1"] <= stats["val_mlm_top5"] <= 1.0


class _Writer:
    def __init__(self):
        self.rows = []

    def add_scalar(self, name, value, step):
        self.rows.append((name, value, step))


def test_evaluate_is_repeatable_and_leaves_the_training_state_alone(dev):
    from ecamp_amd.engine_pretrain import evaluate
    model, cfg = _build(torch.bfloat16, dev)
    batches, pooled = _three_batches(cfg, model, dev)
    model.train()
    model.keep_aux = True
    A = model.prepare()
    sentinel = torch.arange(A.flat_g.numel(), device=dev, dtype=torch.float32) * 0.5 - 7.0
    A.flat_g.copy_(sentinel)
    grads = [(p.grad.data_ptr(), tuple(p.grad.shape)) if p.grad is not None else None for p in model.parameters()]
    model.next_rng()
    model.next_rng()
    random.seed(11)
    np.random.seed(12)
    torch.manual_seed(13)
    before = (model._rng_seed, model._rng_ctr, random.getstate(), np.random.get_state(), torch.get_rng_state())
    args = argparse.Namespace(mask_ratio=0.75, prefetch=True)
    w = _Writer()
    a = evaluate(model, batches, dev, epoch=2, log_writer=w, args=args)
    keep_a = model._aux["ids_keep"].clone()
    b = evaluate(model, batches, dev, epoch=2, args=args)
    keep_b = model._aux["ids_keep"].clone()
    for k in ("val_mlm_top1", "val_mlm_top5", "val_mlm_tokens"):
        assert a[k] == b[k], k
    assert (a["val_mlm_tokens"], a["val_mlm_top1"], a["val_mlm_top5"]) == (int(pooled[0]), pooled[1] / pooled[0], pooled[2] / pooled[0])
    assert torch.equal(keep_a, keep_b)
    assert sorted(w.rows) == sorted((k, a[k], 2000) for k in KEYS)
    # nothing the next training step depends on has moved
    assert model.training and all(mod.training for mod in model.modules())
    assert (model._rng_seed, model._rng_ctr) == before[:2]
    assert random.getstate() == before[2]
    now = np.random.get_state()
    assert now[0] == before[3][0] and (now[1] == before[3][1]).all() and now[2:] == before[3][2:]
    assert torch.equal(torch.get_rng_state(), before[4])
    assert torch.equal(A.flat_g.view(torch.int32), sentinel.view(torch.int32))
    assert [(p.grad.data_ptr(), tuple(p.grad.shape)) if p.grad is not None else None for p in model.parameters()] == grads
    # and the noise does not come from the model's stream: another position of the counter gives the same pass
    model.next_rng()
    c = evaluate(model, batches, dev, epoch=2, args=args)
    assert (c["val_mlm_top1"], c["val_mlm_top5"], c["val_mlm_tokens"]) == (a["val_mlm_top1"], a["val_mlm_top5"], a["val_mlm_tokens"])
    assert torch.equal(model._aux["ids_keep"], keep_a)


def test_evaluate_unwraps_a_data_parallel_wrapper(dev):
    from ecamp_amd.engine_pretrain import evaluate
    model, cfg = _build(torch.bfloat16, dev)
    batches = _three_batches(cfg, model, dev)[0][2:]
    args = argparse.Namespace(mask_ratio=0.75, prefetch=False)
    plain = evaluate(model, batches, dev, epoch=0, args=args)
    wrapped = evaluate(argparse.Namespace(module=model), batches, dev, epoch=0, args=args)
    assert (plain["val_mlm_top1"], plain["val_mlm_top5"], plain["val_mlm_tokens"]) == (wrapped["val_mlm_top1"], wrapped["val_mlm_top5"], wrapped["val_mlm_tokens"])


# ------------------------------------------------------------------------------------------------ driver
def _args(tmp, extra=()):
    from ecamp_amd.main_pretrain import get_args_parser
    argv = ["--synthetic", "--model", "ecamp_tiny", "--epochs", "1", "--batch_size", "4", "--synthetic_len", "8", "--accum_iter", "1",
            "--warmup_epochs", "1", "--lr", "5e-4", "--num_workers", "0", "--max_caption_length", "64", "--output_dir", str(tmp),
            "--data_path", str(tmp)] + list(extra)
    return argparse.ArgumentParser(parents=[get_args_parser()]).parse_args(argv)


def _log(tmp):
    lines = open(os.path.join(tmp, "log.txt")).read().strip().split("\n")
    return [json.loads(l) for l in lines if l.startswith("{")]


def _check_val(s):
    for k in KEYS:
        assert k in s and np.isfinite(s[k]), k
    assert 0.0 <= s["val_mlm_top1"] <= s["val_mlm_top5"] <= 1.0
    assert s["val_mlm_tokens"] == 8 * 64     # the synthetic stand-in labels every position of its 8 held-out samples


def test_main_pretrain_eval_freq_and_eval_only(dev, tmp_path, capsys):
    from ecamp_amd import main_pretrain
    main_pretrain.main(_args(tmp_path, ["--eval_freq", "1"]))
    stats = _log(tmp_path)
    assert [s["epoch"] for s in stats] == [0]
    _check_val(stats[0])
    assert "train_mlm_loss" in stats[0]
    ck = os.path.join(tmp_path, "checkpoint-0.pth")
    assert os.path.exists(ck)
    capsys.readouterr()
    ret = main_pretrain.main(_args(tmp_path, ["--eval_only", "--resume", ck]))
    printed = [l[l.index("{"):] for l in capsys.readouterr().out.split("\n") if '"val_mlm_top1"' in l]
    assert len(printed) == 1
    shown = json.loads(printed[0])
    _check_val(shown)
    assert shown == ret
    # the same weights, the same held-out samples, the same masks: the checkpoint scores what the run scored after its last epoch
    assert (shown["val_mlm_top1"], shown["val_mlm_top5"], shown["val_mlm_tokens"]) == tuple(stats[0][k] for k in KEYS[3:])
    assert _log(tmp_path)[-1]["eval_only"] == ck


def test_main_pretrain_without_eval_freq_logs_no_val_key(dev, tmp_path):
    from ecamp_amd import main_pretrain
    main_pretrain.main(_args(tmp_path))
    stats = _log(tmp_path)
    assert [s["epoch"] for s in stats] == [0]
    assert not any(k.startswith("val_") for k in stats[0])
    assert set(stats[0]) == {"train_mim_loss", "train_res_loss", "train_mlm_loss", "train_lr", "epoch", "data"}
