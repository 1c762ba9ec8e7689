"""Training and evaluation loops of the linear probe -- the reference's Fine-tuning/Classification/train.py:182-509 restricted to the
head (`--mode LinearProbe`), and its learning-rate schedules (utils/scheduler.py) restated.

The frozen encoder and the head's forward, loss and weight gradient are HIP kernels (module/classifier.py); the clip and the SGD
step of the head's two tensors (at most 64 x 1280 values) are plain torch ops on the device.  Nothing is read back per step: the
loss is read where the loop prints.
"""
import math
import os

import numpy as np
import torch

from .util import metrics

PATIENCE = 20   # train.py:427


def _progress(step, warmup_steps, t_total):
    """Share of the decay phase behind `step`: 0 at the end of the warm-up, 1 at `t_total`."""
    return (step - warmup_steps) / max(1, t_total - warmup_steps)


def warmup_linear_factor(step, warmup_steps, t_total):
    """Learning-rate factor of the reference's WarmupLinearSchedule (utils/scheduler.py): a ramp from 0 to 1 over the warm-up, then a
    straight line down to 0 at `t_total` (and 0 beyond)."""
    if step < warmup_steps:
        return step / warmup_steps
    return max(0.0, 1.0 - _progress(step, warmup_steps, t_total))


def warmup_cosine_factor(step, warmup_steps, t_total):
    """Learning-rate factor of the reference's WarmupCosineSchedule with its default half cycle: the same ramp, then
    (1 + cos(pi * progress)) / 2 down to 0 at `t_total`."""
    if step < warmup_steps:
        return step / warmup_steps
    return max(0.0, (1.0 + math.cos(math.pi * _progress(step, warmup_steps, t_total))) / 2.0)


def lr_factor(decay_type, step, warmup_steps, t_total):
    if decay_type not in ("cosine", "linear"):
        raise ValueError("decay_type must be cosine or linear, got %r" % (decay_type,))
    return (warmup_cosine_factor if decay_type == "cosine" else warmup_linear_factor)(step, warmup_steps, t_total)


def head_parameters(model):
    return [model.head.weight, model.head.bias]


def make_optimizer(model, args):
    """train.py:377-384: SGD with momentum 0.9 -- over the head alone, the only tensors with a gradient."""
    return torch.optim.SGD(head_parameters(model), lr=args.learning_rate, momentum=0.9, weight_decay=args.weight_decay)


def _train_step(model, optimizer, x, y, global_step, args, clip=None, scaler=None):
    """One iteration of train.py:438-465 -> (the loss as a device scalar, the learning rate of this step).  The scheduler is stepped
    before the optimizer (train.py:462-463), so optimizer step k (1-based) runs at learning_rate * factor(k).  `clip()` runs between
    backward and the step, for an optimizer that does not clip inside its step.  (set_to_none: the fused optimizers keep `.grad` as views
    whatever is asked.)  `scaler` (optim.SGDLossScaler, engine_finetune's IEEE-half mode): the loss is multiplied by its scale before
    backward and the optimizer takes `step_scaled(scaler)`; the loss returned is the un-scaled one."""
    loss = model.loss(model(x), y)
    (loss if scaler is None else scaler.scale_loss(loss)).backward()
    if clip is not None:
        clip()
    lr = args.learning_rate * lr_factor(args.decay_type, global_step + 1, args.warmup_steps, args.num_steps)
    for grp in optimizer.param_groups:
        grp["lr"] = lr
    if scaler is None:
        optimizer.step()
    else:
        optimizer.step_scaled(scaler)
    optimizer.zero_grad(set_to_none=True)
    return loss.detach(), lr


def train_step(model, optimizer, x, y, global_step, args):
    """One probe iteration -> (loss as a device scalar, learning rate): `_train_step` with the head's gradients clipped before the step."""
    return _train_step(model, optimizer, x, y, global_step, args, clip=lambda: torch.nn.utils.clip_grad_norm_(head_parameters(model), args.max_grad_norm))


@torch.no_grad()
def evaluate(model, loader, log=print):
    """train.py:182-264 / :267-361 without the printing -> dict: `loss` (mean of the batch losses, as the reference's AverageMeter),
    `accuracy` (simple_accuracy), and for a multilabel task `aurocs` (per class, NaN where undefined) and `auroc` (their mean over the
    defined ones), else `confusion`.  Logits and labels stay on the device until the pass is over: one transfer."""
    losses, all_logits, all_y = [], [], []
    for x, y in loader:
        logits = model(x)
        losses.append(model.loss(logits, y))
        all_logits.append(logits)
        all_y.append(y.to(logits.device, non_blocking=True))
    if not losses:
        raise ValueError("evaluate: the loader is empty")
    model.check_labels()
    logits = torch.cat(all_logits).cpu()
    out = {"loss": float(torch.stack(losses).mean().item())}
    if model.multilabel:
        y = torch.cat(all_y).cpu().numpy().reshape(logits.shape)
        prob = logits.sigmoid().numpy()                        # train.py:220,228
        preds = (prob > 0.5) * 1
        out["aurocs"] = metrics.auroc_per_class(prob, y)
        out["auroc"] = metrics.mean_auroc(out["aurocs"], log=log)
        out["accuracy"] = metrics.simple_accuracy(preds, y)
        out["result"] = out["auroc"]
    else:
        y = torch.cat([t.reshape(-1) for t in all_y]).cpu().numpy().astype(np.int64)   # train.py:214-215
        preds = torch.argmax(logits, dim=-1).numpy()
        out["accuracy"] = metrics.simple_accuracy(preds, y)
        out["confusion"] = metrics.confusion_matrix(y, preds, model.num_classes)
        out["result"] = out["accuracy"]
    return out


def checkpoint_path(args, multilabel):
    """train.py:84-95,150-153."""
    return os.path.join(args.output_dir, "%s_%s_checkpoint.bin" % (args.name, "bestauc" if multilabel else "bestacc"))


def train(model, train_loader, val_loader, args, log=print, writer=None, keep_losses=False):
    """Train the head (train.py:364-509) -> dict(global_step, best, losses): `_train` with this module's optimizer and step."""
    return _train(model, train_loader, val_loader, args, log, writer, keep_losses, make_optimizer, train_step)


def _train(model, train_loader, val_loader, args, log, writer, keep_losses, make_optimizer, train_step, report=None):
    """train.py:364-509 under the optimizer and step of the calling engine: passes over `train_loader` until `num_steps` optimizer steps
    are done or the validation result has not improved for PATIENCE validations; validation after every pass; the best checkpoint (mean
    AUROC, ties replace: `<=`; accuracy: `<`) is written in the reference's flat layout.  `report(optimizer, log)` (optional) runs where
    the loop reads the loss anyway, behind its line: an engine's own device values go to the log there.  -> dict(global_step, best, losses
    (device scalars, keep_losses only))."""
    optimizer = make_optimizer(model, args)
    optimizer.zero_grad(set_to_none=True)
    print_freq = max(1, int(getattr(args, "print_freq", 50)))
    global_step, best, down = 0, 0.0, 0
    kept = []
    t_total = args.num_steps
    log("***** Running training *****")
    log("  Total optimization steps = %d" % t_total)
    log("  Instantaneous batch size per GPU = %d" % args.train_batch_size)
    while True:
        n_batches = 0
        for x, y in train_loader:
            loss, lr = train_step(model, optimizer, x, y, global_step, args)
            global_step += 1
            n_batches += 1
            if keep_losses:
                kept.append(loss)
            if global_step % print_freq == 0 or global_step == t_total:
                model.check_labels()   # (where the loss is read anyway)
                val = float(loss.item())
                log("Training (%d / %d Steps) (loss=%2.5f) (lr=%.3e)" % (global_step, t_total, val, lr))
                if writer is not None:
                    writer.add_scalar("train/loss", scalar_value=val, global_step=global_step)
                    writer.add_scalar("train/lr", scalar_value=lr, global_step=global_step)
                if report is not None:
                    report(optimizer, log)
            if global_step >= t_total:
                break
        if n_batches == 0:
            raise ValueError("train: the training loader is empty")
        if val_loader is not None:
            res = evaluate(model, val_loader, log=log)
            log("Validation Results")
            log("Global Steps: %d" % global_step)
            log("Valid Loss: %2.5f" % res["loss"])
            log(("Valid Auc: %2.5f" if model.multilabel else "Valid Accuracy: %2.5f") % res["result"])
            if writer is not None:
                writer.add_scalar("valid/loss", scalar_value=res["loss"], global_step=global_step)
                writer.add_scalar("auroc" if model.multilabel else "accuracy", scalar_value=res["result"], global_step=global_step)
            r = res["result"]
            better = (best <= r) if model.multilabel else (best < r)   # train.py:484,492
            if better and not math.isnan(r):
                torch.save(model.reference_state_dict(), checkpoint_path(args, model.multilabel))
                log("Saved model checkpoint to [DIR: %s]" % args.output_dir)
                best, down = r, 0
            else:
                down += 1
        if global_step >= t_total or down >= PATIENCE:
            break
    log("End Training!")
    return {"global_step": global_step, "best": best, "losses": kept}


def test(model, test_loader, args, log=print, class_names=None):
    """train.py:267-361 on a model that holds the best checkpoint: the test lines, with one AUROC line per class."""
    res = evaluate(model, test_loader, log=log)
    log("Test Results")
    log("Crop ratio: %0.4f" % args.ratio)
    log("Test Loss: %2.5f" % res["loss"])
    log("Test Accuracy: %2.5f" % res["accuracy"])
    if model.multilabel:
        log("The average AUROC is {auroc_avg:.5f}".format(auroc_avg=res["auroc"]))
        for i, a in enumerate(res["aurocs"]):
            log("The AUROC of {} is {}".format(class_names[i] if class_names else "class %d" % i, a))
    else:
        log("Confusion matrix (rows: label, columns: prediction):\n%s" % res["confusion"])
    return res
