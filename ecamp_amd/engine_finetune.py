"""Training and evaluation loops of encoder fine-tuning -- the reference's Fine-tuning/Classification/train.py:364-509 in its default
`--mode Finetune`.  Loop, schedule factors, patience, best-checkpoint rule, log lines and checkpoint layout are engine_linprobe's; what
differs is the optimizer: one fused SGD step over the parameter arena and the classifier's tail buffer (optim.FusedSGD), with the
reference's global-norm clip inside that step.  Nothing is read back per step: the loss is read where the loop prints, the gradient
norm stays on the device (`optimizer.last_norm`).

With `args.compute_dtype == "fp16"` (IEEE half: the reference's apex `--fp16 --fp16_opt_level O2`) the loss is multiplied by a loss scale
before backward and the step is `FusedSGD.step_scaled`: whether the scaled gradients overflowed, the skip and the next scale are decided
on the device (optim.SGDLossScaler).  Where the loop reads the loss it also logs the scale and the skipped steps, and ends the run when
the scale has fallen below 1.
"""
from . import engine_linprobe as _lp
from .engine_linprobe import PATIENCE, checkpoint_path, evaluate, lr_factor, test  # noqa: F401  (the same functions, re-exported)


def make_scaler(args):
    """The loss scaler of the IEEE-half mode, from `args.fp16_loss_scale`: "dynamic" (or unset) is the reference's recipe -- apex's dynamic
    rule started at 2^20 (train.py:398) -- and a number is a static scale."""
    from .optim import SGDLossScaler
    v = getattr(args, "fp16_loss_scale", None)
    if v in (None, "dynamic"):
        return SGDLossScaler()
    return SGDLossScaler(init_scale=float(v), window=0, max_scale=float(v))


def make_optimizer(model, args):
    """train.py:377-380: SGD with momentum 0.9 and one weight decay over every trained tensor; the clip of train.py:458-461 is part of
    the fused step.  In the IEEE-half mode the optimizer carries the loss scaler (`optimizer.loss_scaler`, else None)."""
    from .optim import FusedSGD
    if not getattr(model, "train_encoder", False):
        raise ValueError("engine_finetune needs an ECAMPClassifier(train_encoder=True); the linear probe is engine_linprobe's")
    model.encoder.prepare()
    model.tail()
    opt = FusedSGD([p for _, p in model.finetune_parameters()], lr=args.learning_rate, momentum=0.9, weight_decay=args.weight_decay,
                   max_grad_norm=args.max_grad_norm)
    opt.loss_scaler = make_scaler(args) if getattr(args, "compute_dtype", None) == "fp16" else None
    return opt


def train_step(model, optimizer, x, y, global_step, args):
    """One fine-tune iteration in training mode -> (loss as a device scalar, learning rate): engine_linprobe._train_step; the clip is
    inside the fused step, and so is the loss scaler's decision when the optimizer carries one."""
    model.train()
    return _lp._train_step(model, optimizer, x, y, global_step, args, scaler=getattr(optimizer, "loss_scaler", None))


def report_scaler(optimizer, log):
    """Where the loop reads the loss: the loss scale and the skipped steps, and the end of a run whose scale has collapsed.  From 2^20 a
    scale below 1 is 21 net halvings; gradients that the bf16 path carries cannot need that, so the forward pass itself is not finite."""
    scaler = getattr(optimizer, "loss_scaler", None)
    if scaler is None:
        return
    scale = scaler.scale
    log("  loss scale %.10g, %d steps skipped (%d in a row)" % (scale, scaler.skipped_steps, scaler.skipped_in_a_row))
    if not scale >= 1.0:
        raise SystemExit("fp16 fine-tuning: the loss scale has fallen to %.10g after %d skipped steps (%d in a row): no scale makes the gradients "
                         "finite, so the forward pass itself overflows IEEE half -- run with --f32_residual (the residual stream in f32) "
                         "or --compute_dtype bf16" % (scale, scaler.skipped_steps, scaler.skipped_in_a_row))


def train(model, train_loader, val_loader, args, log=print, writer=None, keep_losses=False):
    """engine_linprobe's loop with the fused optimizer and step of this module.  Validation runs the forward-only path (`evaluate`
    is under no_grad) and the model is back in training mode at the next step."""
    model.train()
    try:
        return _lp._train(model, train_loader, val_loader, args, log, writer, keep_losses, make_optimizer, train_step, report=report_scaler)
    finally:
        model.eval()
