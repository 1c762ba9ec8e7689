"""`train_one_epoch` -- the MAE-style engine step of ECAMP/Pre-training/main_pretrain.py:116-180 (the reference
defines it inline in main_pretrain.py; this module is the MAE-conventional home and main_pretrain re-exports it).

Same signature, same per-iteration LR schedule, same `(mim+res+mlm)/accum_iter` loss, same meters
(`mim_loss, res_loss, mlm_loss, lr`) and return value.  What changed is when the host waits for the device:
the reference calls `.item()` x3 + `torch.cuda.synchronize()` + three scalar all-reduces every micro-step
(:143-145,155,164-166); here the three losses stay on the device, are all-reduced as ONE 3-float message, and
are only read back when a meter is printed (every `print_freq` steps) or averaged at the end of the epoch.
Gradient all-reduce runs once per optimizer step (not per micro-step), overlapped with backward.

`evaluate` (no reference counterpart: the reference has no validation loop) is the held-out pass: `ECAMP.forward_eval` over a loader,
the three losses and the top-1 / top-5 accuracy of the MLM head summed on the device, one all-reduce and one read-back at the end; over every
labelled position, or (`args.eval_score = "masked"`) over the [MASK]ed ones with the head run on those rows alone.
"""
import contextlib
import ctypes
import math
import random
from typing import Iterable

import numpy as np
import torch

from .util import lr_sched, misc


@contextlib.contextmanager
def _range(on, name):
    """roctx range (torch.cuda.nvtx is roctx on ROCm builds) when profiling is on; free otherwise."""
    if not on:
        yield
        return
    try:
        torch.cuda.nvtx.range_push(name)
        pushed = True
    except Exception:   # a build without roctx: profiling ranges are best effort
        pushed = False
    try:
        yield
    finally:
        if pushed:
            torch.cuda.nvtx.range_pop()


def _flush_tb(log_writer, pending):
    """Write the buffered (epoch_1000x, [mim, res, mlm] on the device, lr) records: ONE device read-back for all of them."""
    if not pending:
        return
    vals = torch.stack([r for _, r, _ in pending]).tolist()
    for (x, _, lr), r in zip(pending, vals):
        if not all(math.isfinite(v) for v in r):
            print("warning: non-finite loss {}".format(r))
        log_writer.add_scalar("mim_loss", r[0], x)
        log_writer.add_scalar("res_loss", r[1], x)
        log_writer.add_scalar("mlm_loss", r[2], x)
        log_writer.add_scalar("lr", lr, x)
    del pending[:]


def train_one_epoch(model: torch.nn.Module, data_loader: Iterable, optimizer: torch.optim.Optimizer, device: torch.device,
                    epoch: int, loss_scaler, log_writer=None, args=None):
    model.train(True)
    metric_logger = misc.MetricLogger(delimiter="  ")
    metric_logger.add_meter("lr", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    header = "Epoch: [{}]".format(epoch)
    print_freq = getattr(args, "print_freq", 20)
    accum_iter = args.accum_iter
    optimizer.zero_grad()
    if log_writer is not None:
        print("log_dir: {}".format(log_writer.log_dir))
    n_iter = len(data_loader)
    tb_pending = []
    prof = bool(getattr(args, "profile", False))
    if prof:
        from . import _lib
        lib = _lib.load()
        lib.ecamp_prof_collect(-1, None, None, None)
        lib.ecamp_prof_enable(1)   # HIP events around every GEMM / attention launch (csrc/profile.hip)
    if torch.device(device).type == "cuda" and getattr(args, "prefetch", True):
        from .data import DevicePrefetcher
        data_loader = DevicePrefetcher(data_loader, device)   # batch i+1 crosses PCIe while step i computes
    for data_iter_step, batch in enumerate(metric_logger.log_every(data_loader, print_freq, header)):
        # per-iteration (not per-epoch) lr schedule, updated at accumulation boundaries only (main_pretrain.py:137-138)
        if data_iter_step % accum_iter == 0:
            lr_sched.adjust_learning_rate(optimizer, data_iter_step / n_iter + epoch, args)
        update_grad = (data_iter_step + 1) % accum_iter == 0
        if hasattr(model, "set_grad_sync"):
            model.set_grad_sync(update_grad)
        with _range(prof, "ecamp/step %d" % data_iter_step):
            with _range(prof, "ecamp/forward"):
                mim_loss, res_loss, mlm_loss = model(batch, mask_ratio=args.mask_ratio)
                loss = (mim_loss + res_loss + mlm_loss) / accum_iter
            with _range(prof, "ecamp/backward+allreduce+adamw" if update_grad else "ecamp/backward"):
                loss_scaler(loss, optimizer, parameters=model.parameters(), update_grad=update_grad)
                if update_grad:
                    optimizer.zero_grad()
        losses = torch.stack([mim_loss.detach(), res_loss.detach(), mlm_loss.detach()])
        metric_logger.update(mim_loss=losses[0], res_loss=losses[1], mlm_loss=losses[2])
        lr = optimizer.param_groups[0]["lr"]
        metric_logger.update(lr=lr)
        reduced = misc.all_reduce_mean(losses)
        if log_writer is not None and update_grad:
            # epoch_1000x as the x-axis calibrates curves across batch sizes (main_pretrain.py:168-175).  The values stay on the device
            # until the meters are printed anyway (every `print_freq` steps) or the epoch ends: no host synchronisation per optimizer step
            tb_pending.append((int((data_iter_step / n_iter + epoch) * 1000), reduced, lr))
            if (data_iter_step + 1) % print_freq == 0 or data_iter_step == n_iter - 1:
                _flush_tb(log_writer, tb_pending)
        if getattr(loss_scaler, "dynamic", False) and ((data_iter_step + 1) % print_freq == 0 or data_iter_step == n_iter - 1):
            # GradScaler's state is on the device; it is read back where the meters are printed anyway.  A scale below 1 means every recent
            # step overflowed whatever the scale -- in IEEE half that is an activation past 65504 in the FORWARD pass (the residual stream is
            # stored in half here unless --f32_residual, f32 under the reference's autocast: INTEGRATION.md), and training is no longer making progress
            sc = loss_scaler.get_scale()
            metric_logger.update(loss_scale=sc)
            if sc < 1.0:
                print("warning: the dynamic loss scale has fallen to %g after %d skipped steps -- every step overflows; fp16 activations out of range? "
                      "(--f32_residual keeps the ViT residual stream in f32, as autocast does)" % (sc, loss_scaler.skipped_steps))
    if log_writer is not None:
        _flush_tb(log_writer, tb_pending)
    if prof:
        torch.cuda.synchronize()
        lib.ecamp_prof_enable(0)
        for cat, name in ((0, "bf16 GEMM"), (1, "f32 GEMM"), (2, "attention")):
            ms, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
            lib.ecamp_prof_collect(cat, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(n))
            if n.value:
                print("profile: %-10s %7d launches  %9.2f ms/step  %7.1f TFLOP/s (HIP events on the launch stream)"
                      % (name, n.value, ms.value / max(n_iter, 1), fl.value / max(ms.value, 1e-9) / 1e9))
    metric_logger.synchronize_between_processes()
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


# --------------------------------------------------------------------------------------------- held-out evaluation
EVAL_SEED = 0x45434D50   # the masking noise (and the host-side draws of a validation dataset) of every evaluation pass: the same at every epoch
EVAL_KEYS = ("val_mim_loss", "val_res_loss", "val_mlm_loss", "val_mlm_top1", "val_mlm_top5", "val_mlm_tokens")


def eval_noise_key(rank, batch_index):
    """(seed, offset) of the Philox stream that masks the images of batch `batch_index` on rank `rank` in an evaluation pass."""
    return EVAL_SEED, (int(rank) << 32) | int(batch_index)


def eval_batch_sums(losses, counts, n):
    """One batch's contribution to the sums of an evaluation pass, f64[7]: [n, n * mim, n * res, n * mlm, tokens scored, top-1, top-5] --
    `losses` the three batch means, `counts` the head's int64[3], `n` the batch's samples (a short last batch counts by its size).
    Sums of such vectors -- over batches, then over ranks -- are what `eval_stats` reads; f64 keeps the counts exact below 2^53."""
    losses = losses.to(torch.float64)
    return torch.cat([losses.new_full((1,), float(n)), losses * float(n), counts.to(torch.float64)])


def eval_stats(sums):
    """The sums of `eval_batch_sums` over the whole loader and every rank (7 numbers) -> the `val_*` dict: sample-weighted mean losses,
    accuracies as pooled counts (sum of hits / sum of scored tokens; 0.0 when no token was scored) and the token count."""
    n, mim, res, mlm, tok, top1, top5 = (float(v) for v in sums)
    per = lambda v: v / n if n > 0 else 0.0
    acc = lambda v: v / tok if tok > 0 else 0.0
    return {"val_mim_loss": per(mim), "val_res_loss": per(res), "val_mlm_loss": per(mlm), "val_mlm_top1": acc(top1), "val_mlm_top5": acc(top5),
            "val_mlm_tokens": int(round(tok))}


def eval_scored_rows(batch, score, vocab):
    """The positions of `batch` that `ECAMP.forward_eval(batch, score=score)` scores, as a plain int: labels in [0, vocab), for
    score "masked" only where the input token is [MASK].  On CPU tensors this is host arithmetic -- `evaluate` carries it in the batch
    as `"mlm_rows"`, the row count of the compacted head, which the GEMMs need on the host; on device tensors it synchronises."""
    from .data import MASK
    if score not in ("all", "masked"):
        raise ValueError("score must be 'all' or 'masked', got %r" % (score,))
    labels = batch["labels"]
    scored = (labels >= 0) & (labels < vocab)
    if score == "masked":
        scored &= batch["ids"] == MASK
    return int(scored.sum())


def _with_row_hints(loader, score, vocab):
    """The loader's batches, each host-resident one carrying its scored-row count under "mlm_rows" (a device-resident batch goes through
    as it is: `forward_eval` reads the count back itself)."""
    for batch in loader:
        if batch["labels"].device.type == "cpu":
            batch = dict(batch, mlm_rows=eval_scored_rows(batch, score, vocab))
        yield batch


def evaluate(model, data_loader, device, epoch, log_writer=None, args=None):
    """One pass of `ECAMP.forward_eval` over `data_loader` (held-out data) -> {val_mim_loss, val_res_loss, val_mlm_loss, val_mlm_top1,
    val_mlm_top5, val_mlm_tokens}; TensorBoard scalars under the same names at `epoch * 1000`.

    `args.eval_score` ("all", the default, or "masked") is `forward_eval`'s `score`: the same keys in both scopes, `val_mlm_tokens` says
    which ran.  "masked" runs the head on the scored rows alone; their count per batch is formed on the host before the batch is staged
    (`eval_scored_rows`) and checked at the pass's read-back against what the device found -- a short count would drop rows.
    `args.eval_compact` (absent = None: compact exactly when the scope is "masked") is `forward_eval`'s `compact`, for measurements.

    Comparable across epochs: batch i on rank r is masked with `ops.uniform` noise keyed by `eval_noise_key(r, i)`, handed over as
    `noise=`; a loader with a generator of its own has it re-seeded, and the host generators a dataset may draw from (`random`, NumPy,
    torch) are seeded for the loop.  Without effect on training: on return the model's mode, its Philox counter, those three host
    generators, the gradient arena and every `.grad` are what they were."""
    from . import hip_ops as ops
    m = model.module if hasattr(model, "module") else model   # parallel.DistributedDataParallel: evaluation needs no reducer
    mask_ratio = getattr(args, "mask_ratio", 0.75)
    score = getattr(args, "eval_score", "all")
    compact = getattr(args, "eval_compact", None)
    compact = (score == "masked") if compact is None else bool(compact)
    rank = misc.get_rank()
    m.prepare()
    saved = (m._rng_ctr, m._rng_trace, random.getstate(), np.random.get_state(), torch.get_rng_state())
    try:
        m._rng_trace = None
        random.seed(EVAL_SEED + rank)
        np.random.seed((EVAL_SEED + rank) & 0xFFFFFFFF)
        torch.default_generator.manual_seed(EVAL_SEED + rank)
        if getattr(data_loader, "generator", None) is not None:
            data_loader.generator.manual_seed(EVAL_SEED + rank)
        if compact:
            data_loader = _with_row_hints(data_loader, score, m.bert_config.vocab_size)
        if torch.device(device).type == "cuda" and getattr(args, "prefetch", True):
            from .data import DevicePrefetcher
            data_loader = DevicePrefetcher(data_loader, device)   # (passes the hint, a non-tensor, through)
        dev = m.arena.device
        total = torch.zeros(7, dtype=torch.float64, device=dev)
        found = torch.zeros(1, dtype=torch.float64, device=dev)   # rows the gathers found in the hinted batches, against the hints' sum
        hinted = 0
        for i, batch in enumerate(data_loader):
            n = batch["labels"].shape[0] if batch["labels"].dim() > 1 else 1
            noise = ops.uniform((n, m.num_patches), dev, *eval_noise_key(rank, i))
            out = m.forward_eval(batch, mask_ratio=mask_ratio, noise=noise, score=score, compact=compact)
            total += eval_batch_sums(torch.stack([out["mim_loss"], out["res_loss"], out["mlm_loss"]]), out["mlm_counts"], n)
            if batch.get("mlm_rows") is not None and "mlm_rows_found" in out:
                hinted += int(batch["mlm_rows"])
                found += out["mlm_rows_found"]
        sums = torch.cat([total, found, found.new_full((1,), float(hinted))])
        if misc.get_world_size() > 1:
            torch.distributed.all_reduce(sums)
        sums = sums.tolist()   # the pass's one read-back
        if sums[7] != sums[8]:
            raise RuntimeError("evaluate: the batches' \"mlm_rows\" hints sum to %d scored rows, the device found %d -- a hint below the true "
                               "count drops rows from the compacted head (engine_pretrain.eval_scored_rows gives the count)" % (sums[8], sums[7]))
        stats = eval_stats(sums[:7])
    finally:
        m._rng_ctr, m._rng_trace = saved[0], saved[1]
        random.setstate(saved[2])
        np.random.set_state(saved[3])
        torch.set_rng_state(saved[4])
    if log_writer is not None:
        for k in EVAL_KEYS:
            log_writer.add_scalar(k, stats[k], epoch * 1000)
    print("Evaluation [{}]: {}".format(epoch, "  ".join(("{} {:d}" if isinstance(stats[k], int) else "{} {:.4f}").format(k, stats[k]) for k in EVAL_KEYS)))
    return stats
