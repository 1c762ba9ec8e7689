"""Linear-probe classification on a frozen pre-trained encoder -- drop-in for `python train.py --mode LinearProbe` of
ECAMP/Fine-tuning/Classification (run_lp.sh), on one MI355X:

    python -m ecamp_amd.main_linprobe --name ecamp --stage train --model vit_base_patch16 --task ChestX-ray14 --num_classes 14 \
        --pretrained_path <pre-training checkpoint> --dataset_path <images> --list_dir <directory of the list files> \
        --output_dir output/ChestX-ray14/1/ --data_volume 1 --num_steps 3000 --eval_batch_size 1024 --img_size 224 \
        --learning_rate 3e-2 --warmup_steps 50 --train_batch_size 96 --mode LinearProbe
    python -m ecamp_amd.main_linprobe --name ecamp --stage test ... (scores <output_dir>/<name>_best{auc,acc}_checkpoint.bin)

The reference's flag names are kept.  Added: --list_dir (the reference hard-codes ./datasets/<task>), --compute_dtype {bf16,fp16,fp32}
(--fp16 is --compute_dtype fp16; --fp16_opt_level is accepted and ignored), --pool {avg,cls}, --f32_residual, --synthetic,
--synthetic_len, --num_workers, --print_freq, --image_shard_dir (the image pipeline on the device, over pre-decoded uint8 shards; see its
help), --image_shard_resident / --image_shard_resident_max_gb (keep those shards in device memory: workers then send table rows, no pixels),
--drop_path_rate (main_finetune's stochastic depth; refused here unless 0: the frozen
encoder of the probe is deterministic), --train_pos_embed (main_finetune's trained position table; refused here), --fp16_loss_scale (main_finetune's loss scale of IEEE-half
fine-tuning; ignored here: the head and its gradient are f32).  `--stage train` trains, then tests the best checkpoint, as the reference does.

NOT implemented here, and refused with a message: `--mode Finetune` (main_finetune's), data-parallel probing (`--local_rank` other
than -1); segmentation and detection fine-tuning have no counterpart in this project.
"""
import argparse
import os
import random

import numpy as np
import torch

TASKS = ["ChestX-ray14", "CheXpert", "RSNA", "SIIM", "COVIDx", "Aptos", "SpineXR", "ODIR5K", "MURED"]
SINGLE_LABEL_TASKS = ("COVIDx", "Aptos")   # train.py:118-121: everything else is multilabel
IMAGE_PIPELINE_LINE = ("NOTE: the image pipeline runs on the device (--image_shard_dir %s): crop, BILINEAR resample, flip and normalisation of the "
                       "pre-decoded uint8 shards; the bytes of the host transforms -- a colour image of a colour shard (make_image_shard.py --colour) is "
                       "resampled as three planes and folded to luma behind the resample, as Pillow's Grayscale after the resize")


def get_args_parser():
    p = argparse.ArgumentParser("ECAMP linear probe", add_help=True)
    p.add_argument("--model", choices=["vit_tiny_patch16", "vit_base_patch16", "vit_large_patch16"], default="vit_large_patch16", type=str)
    p.add_argument("--name", required=True, help="name of this run (prefix of the checkpoint files)")
    p.add_argument("--stage", type=str, default="train", choices=["train", "test"])
    p.add_argument("--task", choices=TASKS, default="ChestX-ray14")
    p.add_argument("--num_classes", default=14, type=int)
    p.add_argument("--pretrained_path", type=str, default="", help="pre-training checkpoint ({'model': ...}) whose encoder is probed (--stage train)")
    p.add_argument("--output_dir", default="output", type=str)
    p.add_argument("--img_size", default=384, type=int)
    p.add_argument("--train_batch_size", default=512, type=int)
    p.add_argument("--eval_batch_size", default=64, type=int)
    p.add_argument("--eval_every", default=100, type=int, help="accepted as in the reference, which does not use it either: validation runs after every pass")
    p.add_argument("--learning_rate", default=3e-2, type=float)
    p.add_argument("--weight_decay", default=0, type=float)
    p.add_argument("--num_steps", default=10000, type=int)
    p.add_argument("--data_volume", type=str, default="100", help="1, 10 or 100: train_list_1.txt, train_list_10.txt or train_list.txt")
    p.add_argument("--gpu", type=str, default="", help="accepted and ignored (the reference does not use it either)")
    p.add_argument("--decay_type", choices=["cosine", "linear"], default="cosine")
    p.add_argument("--warmup_steps", default=500, type=int)
    p.add_argument("--max_grad_norm", default=1.0, type=float)
    p.add_argument("--local_rank", type=int, default=-1)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--gradient_accumulation_steps", type=int, default=1)
    p.add_argument("--fp16", action="store_true", help="the same as --compute_dtype fp16")
    p.add_argument("--fp16_opt_level", type=str, default="O2", help="accepted and ignored (apex)")
    p.add_argument("--loss_scale", type=float, default=0, help="accepted and ignored: the head and its gradient are f32")
    p.add_argument("--dataset_path", type=str, default="")
    p.add_argument("--ratio", type=float, default=1)
    p.add_argument("--mode", type=str, default="Finetune", help="LinearProbe (main_linprobe) or Finetune (main_finetune, the reference's default); each driver refuses the other's")
    # additions
    p.add_argument("--list_dir", type=str, default="", help="directory of train_list*.txt / val_list.txt / test_list.txt (default ./datasets/<task>)")
    p.add_argument("--compute_dtype", choices=["bf16", "fp16", "fp32"], default=None, help="format of the frozen encoder (default bf16)")
    p.add_argument("--f32_residual", action="store_true", help="keep the encoder's residual stream in f32 (16-bit formats)")
    p.add_argument("--pool", choices=["avg", "cls"], default="avg", help="avg: mean of the patch tokens + fc_norm (the reference's global_pool=True)")
    p.add_argument("--synthetic", action="store_true", help="random images whose label is a function of the image, instead of a dataset")
    p.add_argument("--synthetic_len", default=64, type=int, help="samples of the synthetic training set (validation and test: half)")
    p.add_argument("--num_workers", default=8, type=int)
    p.add_argument("--print_freq", default=50, type=int, help="steps between two reads of the training loss")
    p.add_argument("--drop_path_rate", default=0.0, type=float,
                   help="--mode Finetune: stochastic depth, the rate of the last block (linear over the blocks from 0); the reference hard-codes 0.1 "
                        "(train.py:127), the default here is 0.0: none")
    p.add_argument("--train_pos_embed", action="store_true",
                   help="--mode Finetune: train pos_embed as the reference does (timm's is a parameter among model.parameters()); the default "
                        "here holds it at the fixed sin-cos table")
    p.add_argument("--fp16_loss_scale", type=str, default=None, metavar="{dynamic,<power of two>}",
                   help="--mode Finetune with --fp16 / --compute_dtype fp16: fine-tune in IEEE half under a loss scale.  dynamic: the reference's "
                        "apex recipe (from 2^20, halved when a step overflows and that step skipped, doubled after 2000 clean steps); a power "
                        "of two: that scale, static.  Without it fp16 fine-tuning is refused; --mode LinearProbe ignores it")
    p.add_argument("--image_shard_dir", type=str, default="", metavar="DIR",
                   help="run the image pipeline on the device: DIR holds one uint8 shard per list file (<list file name>.u8 + .idx.npy, made by "
                        "tools/make_image_shard.py --list_dir ... --dataset_path ... --out_dir DIR); loader workers send the bytes of the crop box, "
                        "the device resamples them with Pillow's BILINEAR arithmetic and the model reads uint8 images.  The same bytes as the "
                        "host transforms.  Colour sources (Aptos, ODIR5K, MURED): make the shards with --colour; a colour shard is recognised from "
                        "its index, its colour images travel as three planes and the device folds them to luma behind the resample, as "
                        "Grayscale after the resize does (without --colour the tool ends at the first colour image)")
    p.add_argument("--image_shard_resident", action="store_true",
                   help="with --image_shard_dir: upload the shard of every split this run reads into device memory once, when its loader is "
                        "built, and resample each crop box where it lies in the stored image; a loader worker then sends one table row per "
                        "sample and no pixels.  The same bytes as without the flag.  A shard must fit in half of the memory that is free when "
                        "it is uploaded (or in --image_shard_resident_max_gb); one that does not ends the run with a message.  "
                        "Classification shards only: pre-training's --image_shard is not covered")
    p.add_argument("--image_shard_resident_max_gb", type=float, default=None, metavar="N",
                   help="with --image_shard_resident: a shard may hold at most N GB (10^9 bytes), in place of the one-half rule")
    return p


def check_args(args):
    """Refuse what is not implemented before any device or dataset is touched."""
    if args.mode != "LinearProbe":
        raise SystemExit("--mode %s is not implemented here: this driver trains the linear probe only (--mode LinearProbe); fine-tuning the "
                         "encoder needs stochastic depth, SGD and clipping over the parameter arena and an unmasked encoder backward" % args.mode)
    if getattr(args, "drop_path_rate", 0.0) != 0:
        raise SystemExit("--drop_path_rate %g with --mode LinearProbe: the probe's encoder is frozen and deterministic, stochastic depth belongs to "
                         "--mode Finetune (main_finetune)" % args.drop_path_rate)
    if getattr(args, "train_pos_embed", False):
        raise SystemExit("--train_pos_embed with --mode LinearProbe: the probe's encoder is frozen, pos_embed included; a trained position table "
                         "belongs to --mode Finetune (main_finetune)")
    if args.local_rank != -1:
        raise SystemExit("--local_rank %d: data-parallel probing is not implemented here; run on one device (--local_rank -1)" % args.local_rank)
    if args.gradient_accumulation_steps != 1:
        raise SystemExit("--gradient_accumulation_steps other than 1 is not implemented here")
    return check_common(args)


def check_common(args):
    """The checks and defaults that do not depend on `--mode` (main_finetune runs them behind its own refusals)."""
    if not 1 <= args.num_classes <= 64:
        raise SystemExit("--num_classes must lie in [1, 64]")
    if args.fp16 and args.compute_dtype not in (None, "fp16"):
        raise SystemExit("--fp16 contradicts --compute_dtype %s" % args.compute_dtype)
    args.compute_dtype = "fp16" if args.fp16 else (args.compute_dtype or "bf16")
    args.is_multilabel = args.task not in SINGLE_LABEL_TASKS
    if args.stage == "train" and not (args.pretrained_path or args.synthetic):
        raise SystemExit("--stage train needs --pretrained_path <pre-training checkpoint> (or --synthetic, which probes a random encoder)")
    shard_dir = getattr(args, "image_shard_dir", "")
    if shard_dir and args.synthetic:
        raise SystemExit("--image_shard_dir with --synthetic: the synthetic stand-in reads no images, there is nothing to resample on the device")
    if getattr(args, "image_shard_resident", False):
        if args.synthetic:
            raise SystemExit("--image_shard_resident with --synthetic: the synthetic stand-in reads no images, there is no shard to keep on the device")
        if not shard_dir:
            raise SystemExit("--image_shard_resident needs --image_shard_dir DIR: it keeps the shards of DIR in device memory")
    elif getattr(args, "image_shard_resident_max_gb", None) is not None:
        raise SystemExit("--image_shard_resident_max_gb without --image_shard_resident: there is no resident shard to limit")
    if getattr(args, "image_shard_resident_max_gb", None) is not None and not args.image_shard_resident_max_gb > 0:
        raise SystemExit("--image_shard_resident_max_gb must be positive, got %g" % args.image_shard_resident_max_gb)
    if not args.synthetic and not args.dataset_path and not shard_dir:   # (the shards hold the images: --dataset_path is then not read)
        raise SystemExit("--dataset_path is required (or --synthetic)")
    if not args.list_dir:
        args.list_dir = os.path.join("datasets", args.task)
    if shard_dir:
        check_image_shards(args)
    return args


def check_image_shards(args):
    """`--image_shard_dir`: every split this run reads needs its shard, with as many images as its list has lines -- found out here,
    from two small files per split, before any device work."""
    from .module import finetune_datasets as fd
    for split in (("train", "val", "test") if args.stage == "train" else ("test",)):
        try:
            fd.check_shard(fd.shard_path(args.image_shard_dir, split, args.data_volume), os.path.join(args.list_dir, fd.list_file(split, args.data_volume)))
        except (FileNotFoundError, ValueError) as e:
            raise SystemExit("--image_shard_dir %s, %s split: %s" % (args.image_shard_dir, split, e))


def build_model(args):
    from .module.classifier import build_classifier
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.compute_dtype]
    return build_classifier(args.model, args.num_classes, args.is_multilabel, img_size=args.img_size, pool=args.pool, compute_dtype=dtype,
                            f32_residual=args.f32_residual)


def resident_max_bytes(args):
    gb = getattr(args, "image_shard_resident_max_gb", None)
    return None if gb is None else int(gb * 1e9)


def check_resident_shards(args, device):
    """`--image_shard_resident`: refuse a shard that does not fit before the model is built (each is checked again when it is uploaded)."""
    from .module import finetune_datasets as fd
    for split in (("train", "val", "test") if args.stage == "train" else ("test",)):
        try:
            fd.ResidentShard.check_fits(fd.shard_path(args.image_shard_dir, split, args.data_volume), device, resident_max_bytes(args))
        except MemoryError as e:
            raise SystemExit("--image_shard_resident, %s split: %s" % (split, e))


def build_loader(args, split, log=print):
    from torch.utils.data import DataLoader

    from .module import finetune_datasets as fd
    train = split == "train"
    batch_size = args.train_batch_size if train else args.eval_batch_size
    if getattr(args, "image_shard_dir", "") and getattr(args, "image_shard_resident", False):
        ds = fd.ShardListDataset(args.image_shard_dir, args.list_dir, split, data_volume=args.data_volume, img_size=args.img_size, ratio=args.ratio,
                                 resident=True)
        print("%s set: %d samples (image shard %s)" % (split, len(ds), ds.shard_path))
        try:
            shard = fd.ResidentShard(ds.shard_path, torch.device("cuda"), resident_max_bytes(args))
        except MemoryError as e:
            raise SystemExit("--image_shard_resident, %s split: %s" % (split, e))
        log("%s set: image shard %s resident on the device: %d bytes uploaded in %.3f s" % (split, shard.path, shard.nbytes, shard.seconds))
        loader = DataLoader(ds, shuffle=train, batch_size=batch_size, num_workers=args.num_workers, pin_memory=True, collate_fn=fd.collate_resident)
        return fd.DeviceImageLoader(loader, torch.device("cuda"), args.img_size, shard=shard)
    if getattr(args, "image_shard_dir", ""):
        ds = fd.ShardListDataset(args.image_shard_dir, args.list_dir, split, data_volume=args.data_volume, img_size=args.img_size, ratio=args.ratio)
        print("%s set: %d samples (image shard %s)" % (split, len(ds), ds.shard_path))
        loader = DataLoader(ds, shuffle=train, batch_size=batch_size, num_workers=args.num_workers, pin_memory=True, collate_fn=fd.collate_boxes)
        return fd.DeviceImageLoader(loader, torch.device("cuda"), args.img_size)
    if args.synthetic:
        n = args.synthetic_len if train else max(1, args.synthetic_len // 2)
        ds = fd.SyntheticClassificationDataset(n, args.img_size, args.num_classes, args.is_multilabel, seed=args.seed + {"train": 0, "val": 1, "test": 2}[split])
    else:
        tf = fd.train_transform(args.img_size) if train else fd.eval_transform(args.img_size, args.ratio)
        ds = fd.ListDataset(args.dataset_path, args.list_dir, split, data_volume=args.data_volume, transform=tf)
    print("%s set: %d samples" % (split, len(ds)))
    return DataLoader(ds, shuffle=train, batch_size=batch_size, num_workers=args.num_workers, pin_memory=True)


def run(args, engine, build_model, count_parameters, opening, eval_mode=False):
    """`--stage train` (train, then test the best checkpoint, as the reference does) or `--stage test` of checked `args`, under `engine`
    (engine_linprobe or engine_finetune).  `count_parameters(model)`: the elements being trained; `opening`: the first log lines;
    `eval_mode`: put the model under test into eval() (a train_encoder model's forward reads `training`)."""
    if not torch.cuda.is_available():
        raise SystemExit("an MI355X is required: the encoder and the head are HIP kernels, there is no CPU path")
    device = torch.device("cuda")
    os.makedirs(args.output_dir, exist_ok=True)
    log_path = os.path.join(args.output_dir, "log.txt")

    def log(msg):
        print(msg, flush=True)
        with open(log_path, mode="a", encoding="utf-8") as f:
            f.write(str(msg) + "\n")

    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    for line in opening:
        log(line)
    if getattr(args, "image_shard_dir", ""):
        log(IMAGE_PIPELINE_LINE % args.image_shard_dir)
    if getattr(args, "image_shard_resident", False):
        check_resident_shards(args, device)
    if args.stage == "train":
        writer = None
        try:
            from torch.utils.tensorboard import SummaryWriter
            writer = SummaryWriter(log_dir=os.path.join(args.output_dir, "logs"))
        except Exception:   # tensorboard is optional
            print("tensorboard not available: scalars go to log.txt only")
        model = build_model(args)
        if args.pretrained_path:
            loaded = model.load_pretrained(args.pretrained_path)
            log("loaded %d tensors from %s" % (len(loaded), args.pretrained_path))
        model.to(device)
        log("Training parameters %s" % args)
        log("Total Parameter: \t%2.4fM" % (count_parameters(model) / 1e6))
        engine.train(model, build_loader(args, "train", log), build_loader(args, "val", log), args, log=log, writer=writer)
        if writer is not None:
            writer.close()
        del model
    # test the best checkpoint (train.py:616-618: also after training)
    path = engine.checkpoint_path(args, args.is_multilabel)
    if not os.path.exists(path):
        raise SystemExit("%s not found: --stage test scores the best checkpoint of a --stage train run with the same --name and --output_dir" % path)
    model = build_model(args)
    model.load_pretrained(path)
    model.to(device)
    if eval_mode:
        model.eval()
    return engine.test(model, build_loader(args, "test", log), args, log=log)


def main(args):
    args = check_args(args)
    from . import engine_linprobe as engine
    return run(args, engine, build_model, lambda model: sum(p.numel() for p in engine.head_parameters(model)),
               ["WARNING: --synthetic: probing on RANDOM images (no dataset is read); the numbers are meaningless"] if args.synthetic else [])


if __name__ == "__main__":
    main(get_args_parser().parse_args())
