"""Training and evaluation loops of encoder fine-tuning -- the reference's Fine-tuning/Classification/train.py:364-509 in its default
`--mode Finetune`.  Loop, schedule factors, patience, best-checkpoint rule, log lines and checkpoint layout are engine_linprobe's; what
differs is the optimizer: one fused SGD step over the parameter arena and the classifier's tail buffer (optim.FusedSGD), with the
reference's global-norm clip inside that step.  Nothing is read back per step: the loss is read where the loop prints, the gradient
norm stays on the device (`optimizer.last_norm`).
"""
from . import engine_linprobe as _lp
from .engine_linprobe import PATIENCE, checkpoint_path, evaluate, lr_factor, test  # noqa: F401  (the same functions, re-exported)


def make_optimizer(model, args):
    """train.py:377-380: SGD with momentum 0.9 and one weight decay over every trained tensor; the clip of train.py:458-461 is part of
    the fused step."""
    from .optim import FusedSGD
    if not getattr(model, "train_encoder", False):
        raise ValueError("engine_finetune needs an ECAMPClassifier(train_encoder=True); the linear probe is engine_linprobe's")
    model.encoder.prepare()
    model.tail()
    return FusedSGD([p for _, p in model.finetune_parameters()], lr=args.learning_rate, momentum=0.9, weight_decay=args.weight_decay,
                    max_grad_norm=args.max_grad_norm)


def train_step(model, optimizer, x, y, global_step, args):
    """One fine-tune iteration in training mode -> (loss as a device scalar, learning rate): engine_linprobe._train_step; the clip is
    inside the fused step."""
    model.train()
    return _lp._train_step(model, optimizer, x, y, global_step, args)


def train(model, train_loader, val_loader, args, log=print, writer=None, keep_losses=False):
    """engine_linprobe's loop with the fused optimizer and step of this module.  Validation runs the forward-only path (`evaluate`
    is under no_grad) and the model is back in training mode at the next step."""
    model.train()
    try:
        return _lp._train(model, train_loader, val_loader, args, log, writer, keep_losses, make_optimizer, train_step)
    finally:
        model.eval()
