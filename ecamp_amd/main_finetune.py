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

NOT implemented, and refused with a message before any device work: data-parallel fine-tuning (`--local_rank` other than -1),
`--gradient_accumulation_steps` other than 1, and `--fp16` (IEEE half with loss scaling): use `--compute_dtype bf16`.
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
    return "NOTE: %s, and %s" % (depth, pos)


def check_args(args):
    """Refuse what is not implemented before any device or dataset is touched; the checks behind are main_linprobe's shared ones."""
    if args.mode != "Finetune":
        raise SystemExit("--mode %s: this driver fine-tunes the encoder (--mode Finetune) or hands --mode LinearProbe to main_linprobe" % args.mode)
    if args.local_rank != -1:
        raise SystemExit("--local_rank %d: data-parallel fine-tuning is not implemented here; run on one device (--local_rank -1)" % args.local_rank)
    if args.gradient_accumulation_steps != 1:
        raise SystemExit("--gradient_accumulation_steps %d: gradient accumulation is not implemented here (only 1)" % args.gradient_accumulation_steps)
    if args.fp16 or args.compute_dtype == "fp16":
        raise SystemExit("--fp16 --mode Finetune is not implemented here (IEEE half needs loss scaling around the fused SGD step): "
                         "use --compute_dtype bf16 (or fp32)")
    rate = float(getattr(args, "drop_path_rate", 0.0))
    if not 0.0 <= rate < 1.0:
        raise SystemExit("--drop_path_rate %g must lie in [0, 1)" % rate)
    return main_linprobe.check_common(args)


def build_model(args):
    from .module.classifier import build_classifier
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[args.compute_dtype]
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
