"""-m gpu: masked-token evaluation at the model, engine and driver level -- `ECAMP.forward_eval(score="masked")` with the MLM head run on
the gathered rows alone, against counts and losses formed on the host from its own compacted logits, against the uncompacted head on the
same batch relabelled on the host, `engine_pretrain.evaluate` with `args.eval_score = "masked"` and the driver's `--eval_score`.
The tiny model and the recipe state of tests/test_eval_model_gpu.py, B = 4, S = 128."""
import argparse
import json
import random

import numpy as np
import pytest
import torch

from conftest import h16
from test_eval_model_gpu import KEYS, _args, _build, _labels_near_the_top, _log, _losses, _three_batches, host_counts

pytestmark = pytest.mark.gpu

B, S = 4, 128
MASK = 3
LOSS_TOL = {torch.float32: 2e-4, torch.bfloat16: 3e-2, torch.float16: 1e-3}     # the project's bars of forward_eval against the reference


def _batch(model, cfg, seed):
    """A recipe batch whose labels sit near the top of the model's own logits (ranks 0..7, every third position -100) -> (batch, noise,
    the uncompacted logits [B*S, V] the labels were placed under)."""
    from oracle import recipe
    batch = recipe.recipe_batch(cfg, B, S, seed=seed)
    noise = recipe.recipe_noise(B, cfg.num_patches, seed=seed)
    keep, model.keep_aux = model.keep_aux, True
    model.forward_eval(batch, noise=noise)
    logits = model._aux["logits"]
    model.keep_aux = keep
    batch["labels"] = _labels_near_the_top(logits, B, S)
    return batch, noise, logits


def _masked(batch, V):
    """bool [B*S]: the positions score="masked" covers."""
    ids, labels = batch["ids"].reshape(-1), batch["labels"].reshape(-1)
    return (ids == MASK) & (labels >= 0) & (labels < V)


def _relabelled(batch, V):
    """The same batch with -100 outside the masked positions: what the uncompacted path scores is then the masked scope."""
    m = _masked(batch, V).view(batch["labels"].shape)
    return dict(batch, labels=torch.where(m, batch["labels"], torch.full_like(batch["labels"], -100)))


def test_default_path_is_unchanged(dev):
    """`forward_eval(batch)` and `forward_eval(batch, score="all")` are one path: the same keys, the same `_aux`, bit-identical logits,
    image masks and counts.  The three losses are f32 sums accumulated with floating-point atomics whose order is not fixed, so two calls
    of the very same path may differ in the last bits (measured: res_loss, one ulp, between two default calls); they are held to 1e-5
    relative, the bar tests/test_eval_model_gpu.py sets for `evaluate` against separate calls of the same pass."""
    model, cfg = _build(torch.bfloat16, dev)
    model.keep_aux = True
    batch, noise, _ = _batch(model, cfg, 3)
    a = model.forward_eval(batch, noise=noise)
    aux_a = dict(model._aux)
    b = model.forward_eval(batch, noise=noise, score="all")
    assert set(a) == set(b) == {"mim_loss", "res_loss", "mlm_loss", "mlm_counts"}
    assert torch.equal(a["mlm_counts"], b["mlm_counts"])
    la, lb = _losses(a), _losses(b)
    print("default", la, "score=all", lb, "bitwise", [torch.equal(a[k], b[k]) for k in ("mim_loss", "res_loss", "mlm_loss")])
    assert np.all(np.abs(la - lb) <= 1e-5 * np.abs(la))
    assert set(aux_a) == set(model._aux) and "mlm_rows" not in model._aux
    assert model._aux["logits"].shape == (B * S, cfg.bert.vocab_size)
    for k in ("logits", "ids_keep", "mask", "latent"):
        assert torch.equal(aux_a[k], model._aux[k]), k
    with pytest.raises(ValueError):
        model.forward_eval(batch, noise=noise, score="visible")


def _check_compacted(model, cfg, batch, out, dtype):
    """A compacted pass against the host: the rows it gathered, its counts and its loss from its own logits."""
    from ecamp_amd import hip_ops
    V = cfg.bert.vocab_size
    masked = _masked(batch, V)
    n = int(masked.sum())
    cap = hip_ops.compact_cap(n)
    logits, rows = model._aux["logits"], model._aux["mlm_rows"].cpu().long()
    assert 0 < n and cap < B * S
    assert logits.shape == (cap, V) and logits.dtype == dtype and rows.shape == (cap,)
    assert torch.equal(rows[:n], masked.nonzero()[:, 0]) and (rows[n:] == -1).all()          # exactly the masked positions, in order
    assert int(out["mlm_rows_found"].item()) == n
    labels_c = torch.where(rows >= 0, batch["labels"].reshape(-1)[rows.clamp(min=0)], torch.full_like(rows, -100))
    weights_c = torch.where(rows >= 0, batch["weights"].reshape(-1)[rows.clamp(min=0)], torch.zeros(cap))
    want = host_counts(logits, labels_c)
    got = out["mlm_counts"].cpu().tolist()
    print("  counts", got, "host", want, "rows", n, "cap", cap)
    assert got == want and want[0] == n and 0 < want[1] < want[2] < want[0]
    x = logits.float().cpu().double()
    ce = torch.logsumexp(x, 1) - x.gather(1, labels_c.clamp(min=0)[:, None])[:, 0]
    ref = float((ce * weights_c.double())[labels_c >= 0].sum() / (B * S))
    print("  mlm_loss", out["mlm_loss"].item(), "host", ref)
    assert abs(out["mlm_loss"].item() - ref) <= 1e-5 * abs(ref)


def test_masked_scope_runs_the_head_on_the_gathered_rows(dev, both_halves):
    """score="masked": the logits kept are [cap, V] with cap below B*S, `mlm_rows` lists the masked positions, and the counts and the
    loss are those of the compacted logits -- with the row count handed over as a hint and read back from the device."""
    from ecamp_amd.engine_pretrain import eval_scored_rows
    for dtype in (torch.float32, h16()):
        model, cfg = _build(dtype, dev)
        model.keep_aux = True
        batch, noise, _ = _batch(model, cfg, 3)
        hint = eval_scored_rows(batch, "masked", cfg.bert.vocab_size)
        assert hint == int(_masked(batch, cfg.bert.vocab_size).sum())
        out_h = model.forward_eval(dict(batch, mlm_rows=hint), noise=noise, score="masked")
        assert set(out_h) == {"mim_loss", "res_loss", "mlm_loss", "mlm_counts", "mlm_rows_found"}
        _check_compacted(model, cfg, batch, out_h, dtype)
        out_r = model.forward_eval(batch, noise=noise, score="masked")                     # no hint: one read-back
        _check_compacted(model, cfg, batch, out_r, dtype)
        assert torch.equal(out_h["mlm_counts"], out_r["mlm_counts"]) and out_h["mlm_counts"][0].item() == hint


def _precondition_failures(logits, labels, scored):
    """Rows whose top-1 / top-5 verdict a rounding difference of 1e-4 max|logit| could flip: the label's logit within that distance of
    one of the other six largest, or (label outside the six largest) less than that below the fifth largest."""
    x = logits.float().cpu().double()
    eps = 1e-4 * float(x.abs().max())
    val, idx = x.topk(7, dim=1)
    lab = labels.reshape(-1).clamp(min=0)
    xl = x.gather(1, lab[:, None])[:, 0]
    in6 = (idx[:, :6] == lab[:, None]).any(1)
    own = idx == lab[:, None]
    near = ((val - xl[:, None]).abs() <= eps) & ~own
    bad_in = in6 & near.any(1)
    bad_out = ~in6 & (xl > val[:, 4] - eps)
    return int(((bad_in | bad_out) & scored).sum())


def _cross_path(dev, dtype):
    model, cfg = _build(dtype, dev)
    model.keep_aux = True
    V = cfg.bert.vocab_size
    fails = None
    for seed in (3, 4, 5):
        batch, noise, logits = _batch(model, cfg, seed)
        fails = _precondition_failures(logits, batch["labels"], _masked(batch, V))
        if dtype != torch.float32 or fails == 0:
            break
    held = _relabelled(batch, V)
    n = int(_masked(batch, V).sum())
    ref = model.forward_eval(held, noise=noise)                                             # the uncompacted head, relabelled on the host
    assert model._aux["logits"].shape[0] == B * S
    modes = {"masked": model.forward_eval(batch, noise=noise, score="masked"),
             "masked, compact=False": model.forward_eval(batch, noise=noise, score="masked", compact=False),
             "all on -100 labels, compact=True": model.forward_eval(held, noise=noise, score="all", compact=True)}
    rc, rl = ref["mlm_counts"].cpu().tolist(), ref["mlm_loss"].item()
    print(dtype, "seed", seed, "scored", n, "uncompacted counts", rc, "loss", rl, "precondition failures", fails)
    assert rc[0] == n and 0 < rc[1] < rc[2] < rc[0]
    for name, out in modes.items():
        c, l = out["mlm_counts"].cpu().tolist(), out["mlm_loss"].item()
        print("  %-34s counts %s loss %.8f rel %.2e" % (name, c, l, abs(l - rl) / abs(rl)))
        assert c[0] == n, name
        assert abs(l - rl) <= LOSS_TOL[dtype] * abs(rl), name
        if dtype == torch.float32:
            if fails == 0:
                assert c == rc, name
            else:   # no seed met the precondition: at most the rows that could flip, and few of them
                assert fails <= 0.05 * n and abs(c[1] - rc[1]) <= fails and abs(c[2] - rc[2]) <= fails, (name, fails)
    assert "mlm_rows_found" not in modes["masked, compact=False"] and "mlm_rows_found" in modes["masked"]


def test_compacted_and_uncompacted_heads_agree_fp32(dev):
    _cross_path(dev, torch.float32)


def test_compacted_and_uncompacted_heads_agree_16bit(dev, both_halves):
    _cross_path(dev, h16())


def _masked_args(**kw):
    return argparse.Namespace(mask_ratio=0.75, prefetch=True, eval_score="masked", **kw)


def test_evaluate_masked_is_the_pooled_forward_eval_calls(dev, monkeypatch):
    from ecamp_amd import engine_pretrain, hip_ops
    from ecamp_amd.engine_pretrain import eval_noise_key, evaluate
    model, cfg = _build(torch.bfloat16, dev)
    V = cfg.bert.vocab_size
    batches, _ = _three_batches(cfg, model, dev)
    model.train()
    A = model.prepare()
    sentinel = torch.arange(A.flat_g.numel(), device=dev, dtype=torch.float32) * 0.5 - 7.0
    A.flat_g.copy_(sentinel)
    grads = [(p.grad.data_ptr(), tuple(p.grad.shape)) if p.grad is not None else None for p in model.parameters()]
    model.next_rng()
    random.seed(11)
    np.random.seed(12)
    torch.manual_seed(13)
    before = (model._rng_seed, model._rng_ctr, random.getstate(), np.random.get_state(), torch.get_rng_state())
    seen = []
    inner = model.forward_eval

    def spy(batch, **kw):
        seen.append((batch.get("mlm_rows"), kw.get("score"), batch["labels"].is_cuda))
        return inner(batch, **kw)

    monkeypatch.setattr(model, "forward_eval", spy)
    stats = evaluate(model, batches, dev, epoch=3, args=_masked_args())
    monkeypatch.undo()
    assert tuple(stats) == KEYS
    hints = [int(_masked(b, V).sum()) for b in batches]
    assert seen == [(h, "masked", True) for h in hints]                        # the count rides in the staged batch, a plain int
    assert all(isinstance(s[0], int) for s in seen)
    # nothing the next training step depends on has moved
    assert model.training and all(mod.training for mod in model.modules())
    assert (model._rng_seed, model._rng_ctr) == before[:2]
    assert random.getstate() == before[2]
    now = np.random.get_state()
    assert now[0] == before[3][0] and (now[1] == before[3][1]).all() and now[2:] == before[3][2:]
    assert torch.equal(torch.get_rng_state(), before[4])
    assert torch.equal(A.flat_g.view(torch.int32), sentinel.view(torch.int32))
    assert [(p.grad.data_ptr(), tuple(p.grad.shape)) if p.grad is not None else None for p in model.parameters()] == grads
    # the pooled separate calls
    n_all, lsum, csum = 0, np.zeros(3), np.zeros(3, dtype=np.int64)
    for i, b in enumerate(batches):
        n = b["labels"].shape[0]
        out = model.forward_eval(b, mask_ratio=0.75, noise=hip_ops.uniform((n, cfg.num_patches), dev, *eval_noise_key(0, i)), score="masked")
        lsum += n * _losses(out)
        csum += np.array(out["mlm_counts"].cpu().tolist(), dtype=np.int64)
        n_all += n
    want = lsum / n_all
    got = np.array([stats["val_mim_loss"], stats["val_res_loss"], stats["val_mlm_loss"]])
    print("evaluate", got, "separate calls", want, "counts", csum, "hints", hints)
    assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want))
    assert stats["val_mlm_tokens"] == int(csum[0]) == sum(hints) and 0 < csum[1] < csum[2] < csum[0]
    assert stats["val_mlm_top1"] == int(csum[1]) / int(csum[0]) and stats["val_mlm_top5"] == int(csum[2]) / int(csum[0])
    everything = evaluate(model, batches, dev, epoch=3, args=argparse.Namespace(mask_ratio=0.75, prefetch=True))
    assert everything["val_mlm_tokens"] > stats["val_mlm_tokens"]              # the default scope pools every labelled position
    # a wrong hint -- one row short, and far short -- is caught at the read-back
    true_count, ctr = engine_pretrain.eval_scored_rows, model._rng_ctr
    for wrong in (lambda b, s, v: true_count(b, s, v) - 1, lambda b, s, v: 1):
        monkeypatch.setattr(engine_pretrain, "eval_scored_rows", wrong)
        with pytest.raises(RuntimeError, match="mlm_rows"):
            evaluate(model, batches, dev, epoch=3, args=_masked_args())
        monkeypatch.undo()
    assert model.training and model._rng_ctr == ctr                             # also when the pass ends in the error


def _masked_tokens_of_the_synthetic_validation_set(args):
    from ecamp_amd.data import SyntheticContextBertDataset
    ds = SyntheticContextBertDataset(min(args.synthetic_len, 1024), args.max_caption_length, args.input_size, seed=args.seed + 1)
    n = 0
    for i in range(len(ds)):
        item = ds[i]
        n += int(((item["ids"] == MASK) & (item["labels"] >= 0) & (item["labels"] < 30000)).sum())
    return n


def test_main_pretrain_eval_score_masked(dev, tmp_path, capsys):
    from ecamp_amd import main_pretrain
    args = _args(tmp_path, ["--eval_freq", "1", "--eval_score", "masked"])
    masked = _masked_tokens_of_the_synthetic_validation_set(args)
    assert 0 < masked < 8 * 64
    main_pretrain.main(args)
    stats = _log(tmp_path)
    assert [s["epoch"] for s in stats] == [0]
    for k in KEYS:
        assert k in stats[0] and np.isfinite(stats[0][k]), k
    assert set(k for k in stats[0] if k.startswith("val_")) == set(KEYS)        # the same keys in both scopes
    assert stats[0]["val_mlm_tokens"] == masked
    assert 0.0 <= stats[0]["val_mlm_top1"] <= stats[0]["val_mlm_top5"] <= 1.0
    ck = str(tmp_path / "checkpoint-0.pth")
    capsys.readouterr()
    ret = main_pretrain.main(_args(tmp_path, ["--eval_only", "--resume", ck, "--eval_score", "masked"]))
    printed = [l[l.index("{"):] for l in capsys.readouterr().out.split("\n") if '"val_mlm_top1"' in l]
    assert len(printed) == 1
    shown = json.loads(printed[0])
    assert shown == ret and tuple(shown) == KEYS
    # the same weights, the same held-out samples, the same masks: the checkpoint scores what the run scored after its last epoch
    assert (shown["val_mlm_top1"], shown["val_mlm_top5"], shown["val_mlm_tokens"]) == tuple(stats[0][k] for k in KEYS[3:])
    assert all(abs(shown[k] - stats[0][k]) <= 1e-5 * abs(stats[0][k]) for k in KEYS[:3])
