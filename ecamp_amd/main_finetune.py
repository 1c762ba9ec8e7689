"""Fine-tuning the pre-trained encoder on a classification task -- drop-in for `python train.py` of
ECAMP/Fine-tuning/Classification in its default `--mode Finetune` (run_ft.sh), on one MI355X:

    python -m ecamp_amd.main_finetune --name ecamp --stage train --model vit_base_patch16 --task ChestX-ray14 --num_classes 14 \
        --pretrained_path <pre-training checkpoint> --dataset_path <images> --list_dir <directory of the list files> \
        --output_dir output/ChestX-ray14/1/ --data_volume 1 --num_steps 3000 --eval_batch_size 512 --img_size 224 \
        --learning_rate 3e-2 --warmup_steps 50 --train_batch_size 96 --compute_dtype bf16 --drop_path_rate 0.1 \
        --train_pos_embed
    python -m ecamp_amd.main_finetune --name ecamp --stage test ... (scores <output_dir>/<name>_best{auc,acc}_checkpoint.bin)

The flags are main_linprobe's (the reference's names and its additions); `--mode` defaults to Finetune, and `--mode LinearProbe` hands
over to main_linprobe.  `--drop_path_rate R` applies stochastic depth at rates linear over the blocks from 0 to R (timm's rule); the
reference hard-codes R = 0.1 (train.py:127), the default here is 0.0.  `--train_pos_embed` (default off) trains `pos_embed` as the
reference does (timm's is a parameter: in the SGD, in the clip, in the checkpoint); without it the table stays the fixed sin-cos one.
`--drop_path_rate 0.1 --train_pos_embed` is the reference's model-side recipe.  The first log line of every run states what deviates from
the reference: stochastic depth when it is off, and `pos_embed` when it is held fixed.

`--fp16_loss_scale {dynamic,<power of two>}` (default: none) makes `--fp16` / `--compute_dtype fp16` fine-tune in IEEE half, the format of
the reference's `--fp16 --fp16_opt_level O2`: half activations and 16-bit weight shadows over f32 masters (the head stays f32, where apex
O2's is half), the loss multiplied by a scale before backward, the gradients un-scaled inside the fused SGD step.  `dynamic` is apex's rule
from the reference's start of 2^20 (train.py:398): a step whose scaled gradients are not finite is skipped and the scale halved, 2000 clean
steps in a row double it (at most 2^24); the decision is taken on the device and the schedule advances over a skipped step, as the
reference's does.  A number is a static scale (a power of two, so that un-scaling is exact).  A run_ft.sh line then needs only
`--fp16_loss_scale dynamic` (and the list and dataset paths) added.  The log carries the scale and the skipped steps wherever it carries
the loss; a scale that has fallen below 1 ends the run (the forward pass overflows half: `--f32_residual`).

NOT implemented, and refused with a message before any device work: data-parallel fine-tuning (`--local_rank` other than -1),
`--gradient_accumulation_steps` other than 1, and `--fp16` / `--compute_dtype fp16` WITHOUT `--fp16_loss_scale` (IEEE half needs loss
scaling: opt in, or use `--compute_dtype bf16`).
"""
import torch

from . import main_linprobe
from .main_linprobe import build_loader, get_args_parser  # noqa: F401  (one parser: run_ft.sh's command lines parse unchanged)

DEVIATIONS = ("NOTE: stochastic depth (the reference's drop_path_rate=0.1) is NOT applied, and pos_embed is held fixed at the sin-cos table "
              "(the reference trains it)")


def opening_line(args):
    """The first log line of a run, a function of `args` alone: what deviates from the reference's recipe."""
    rate = float(getattr(args, "drop_path_rate", 0.0))
    depth = ("stochastic depth (the reference's drop_path_rate=0.1) is NOT applied" if rate == 0 else
             "stochastic depth IS applied at drop_path_rate=%g, rising linearly over the blocks from 0 (the reference's is 0.1)" % rate)
    pos = ("pos_embed IS trained (as the reference does)" if getattr(args, "train_pos_embed", False) else
           "pos_embed is held fixed at the sin-cos table (the reference trains it)")
    line = "NOTE: %s, and %s" % (depth, pos)
    if getattr(args, "fp16_loss_scale", None) is not None and (getattr(args, "fp16", False) or getattr(args, "compute_dtype", None) == "fp16"):
        from . import engine_finetune
        line += ("; IEEE half (fp16) activations and 16-bit weight shadows over f32 masters and an f32 head (apex O2's head is half), under %s; "
                 "the residual stream is %s" % (engine_finetune.make_scaler(args).describe(),
                                                "f32 (--f32_residual)" if getattr(args, "f32_residual", False) else "half (--f32_residual keeps it in f32)"))
    return line


def loss_scale_of(text):
    """`--fp16_loss_scale`: "dynamic", or a static scale 2^k >= 1 (un-scaling by a power of two is exact in f32) -> "dynamic" / float."""
    if text == "dynamic":
        return text
    try:
        v = float(text)
    except ValueError:
        v = 0.0
    import math
    if not (1.0 <= v < float("inf")) or math.frexp(v)[0] != 0.5:
        raise SystemExit("--fp16_loss_scale %s: must be `dynamic` or a positive power of two (1, 2, 4, ... 65536 ...: un-scaling is then exact)" % text)
    return v


def check_args(args):
    """Refuse what is not implemented before any device or dataset is touched; the checks behind are main_linprobe's shared ones."""
    if args.mode != "Finetune":
        raise SystemExit("--mode %s: this driver fine-tunes the encoder (--mode Finetune) or hands --mode LinearProbe to main_linprobe" % args.mode)
    if args.local_rank != -1:
        raise SystemExit("--local_rank %d: data-parallel fine-tuning is not implemented here; run on one device (--local_rank -1)" % args.local_rank)
    if args.gradient_accumulation_steps != 1:
        raise SystemExit("--gradient_accumulation_steps %d: gradient accumulation is not implemented here (only 1)" % args.gradient_accumulation_steps)
    half = args.fp16 or args.compute_dtype == "fp16"
    if getattr(args, "fp16_loss_scale", None) is not None:
        loss_scale_of(args.fp16_loss_scale)
        if not half:
            raise SystemExit("--fp16_loss_scale %s with --compute_dtype %s: a loss scale belongs to IEEE half (--fp16 / --compute_dtype fp16); "
                             "bf16 and fp32 need none" % (args.fp16_loss_scale, args.compute_dtype or "bf16"))
    elif half:
        raise SystemExit("--fp16 --mode Finetune is not implemented here without a loss scale (IEEE half needs loss scaling around the fused SGD "
                         "step): add --fp16_loss_scale dynamic (the reference's apex recipe), or use --compute_dtype bf16 (or fp32)")
    rate = float(getattr(args, "drop_path_rate", 0.0))
    if not 0.0 <= rate < 1.0:
        raise SystemExit("--drop_path_rate %g must lie in [0, 1)" % rate)
    return main_linprobe.check_common(args)


def build_model(args):
    from .module.classifier import build_classifier
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.compute_dtype]
    return build_classifier(args.model, args.num_classes, args.is_multilabel, img_size=args.img_size, pool=args.pool, train_encoder=True,
                            drop_path_rate=getattr(args, "drop_path_rate", 0.0), train_pos_embed=getattr(args, "train_pos_embed", False),
                            compute_dtype=dtype, f32_residual=args.f32_residual)


def main(args):
    if args.mode == "LinearProbe":
        return main_linprobe.main(args)
    args = check_args(args)
    from . import engine_finetune as engine
    return main_linprobe.run(args, engine, build_model, lambda model: sum(p.numel() for _, p in model.finetune_parameters()),
                             [opening_line(args)] + (["WARNING: --synthetic: fine-tuning on RANDOM images (no dataset is read); the numbers are meaningless"]
                                             if args.synthetic else []), eval_mode=True)


if __name__ == "__main__":
    main(get_args_parser().parse_args())
