#!/usr/bin/env python3
"""Decode images ONCE into uint8 shards for the device image pipelines (module/pretrain_datasets.py: U8ShardWriter).

Pre-training -- the radiographs of <data_path>/mimic-cxr-2.0.0-entity-llm.csv, for `main_pretrain.py --image_shard`:

    python tools/make_image_shard.py --data_path <dir> --out <dir>/images.u8 [--max_side 1024] [--workers 16]

Without --max_side the shard holds the JPEGs' own pixels (7.8 MB per 2544 x 3056 radiograph: the crops are then exactly the reference's);
--max_side shrinks the longer side first (Pillow bicubic) -- smaller files and host -> HBM copies, crops from the shrunk image.

Classification -- one shard per list file of a task, for `main_linprobe.py / main_finetune.py --image_shard_dir`:

    python tools/make_image_shard.py --list_dir <lists> --dataset_path <images> --out_dir <dir> [--splits train_list.txt val_list.txt ...] [--colour]

writes <out_dir>/<list file name>.u8 (+ .idx.npy) with the list's images in list order, opened through `pil_loader` as the dataset opens
them.  --splits: list file names (default: every one of train_list.txt, train_list_1.txt, train_list_10.txt, val_list.txt, test_list.txt
that exists).  An image whose three channels are equal keeps that property through the resample, and Grayscale returns the common value:
one plane is the whole source.  Grayscale after the resample of a colour image is NOT the resample of its gray plane, so without
--colour an image whose channels differ ends the run, naming the file.  --colour (Aptos, ODIR5K, MURED: colour fundus photographs, or
any list with a colour file in it) writes every shard through the colour writer: a grayscale file still costs one plane, a colour file
three (R, G, B), and the index gains a fourth column, the plane count, from which the drivers recognise the shard.  The device then
resamples the three planes and folds them as Pillow's convert("L") does -- byte for byte the host transforms either way.  --max_side
is not offered in this mode."""
import argparse
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIST_FILES = ("train_list.txt", "train_list_1.txt", "train_list_10.txt", "val_list.txt", "test_list.txt")


def decode(args):
    path, max_side = args
    from PIL import Image
    img = Image.open(path).convert("L")
    if max_side and max(img.size) > max_side:
        r = max_side / float(max(img.size))
        img = img.resize((max(1, int(round(img.size[0] * r))), max(1, int(round(img.size[1] * r)))), Image.BICUBIC)
    return np.asarray(img, dtype=np.uint8)


def decode_gray(path):
    """The dataset's `pil_loader` image as one uint8 plane, or None if its three channels differ (a colour source)."""
    from ecamp_amd.module.pretrain_datasets import pil_loader
    a = np.asarray(pil_loader(path), dtype=np.uint8)
    if not (np.array_equal(a[..., 0], a[..., 1]) and np.array_equal(a[..., 0], a[..., 2])):
        return None
    return np.ascontiguousarray(a[..., 0])


def decode_planes(path):
    """The dataset's `pil_loader` image as uint8 [H, W, 3] (`U8ShardWriter(colour=True).add` keeps one plane if the channels are equal)."""
    from ecamp_amd.module.pretrain_datasets import pil_loader
    return np.asarray(pil_loader(path), dtype=np.uint8)


def shard_lists(list_dir, dataset_path, out_dir, splits, workers, keep_colour=False):
    from ecamp_amd.module.finetune_datasets import read_list
    from ecamp_amd.module.pretrain_datasets import U8ShardWriter
    names = list(splits) if splits else [n for n in LIST_FILES if os.path.exists(os.path.join(list_dir, n))]
    if not names:
        raise SystemExit("no list file (%s) in %s" % (", ".join(LIST_FILES), list_dir))
    os.makedirs(out_dir, exist_ok=True)
    for name in names:
        lp = os.path.join(list_dir, name)
        if not os.path.exists(lp):
            raise SystemExit("%s not found" % lp)
        paths = [os.path.join(dataset_path, r) for r in read_list(lp)[0]]
        out = os.path.join(out_dir, name + ".u8")
        colour = None
        with U8ShardWriter(out, colour=keep_colour) as w, ProcessPoolExecutor(workers) as ex:
            for n, arr in enumerate(ex.map(decode_planes if keep_colour else decode_gray, paths, chunksize=8)):
                if arr is None:
                    colour = paths[n]
                    break
                w.add(arr)
                if n % 1000 == 0:
                    print("%s: %d / %d" % (name, n, len(paths)), flush=True)
        if colour is not None:   # no partial shard is left behind
            os.remove(out)
            os.remove(out + ".idx.npy")
            raise SystemExit("%s is a COLOUR image (its three channels differ): the device image pipeline equals the host transforms "
                             "for grayscale sources only (Grayscale after the resample is not the resample of the gray plane) -- "
                             "keep this dataset on the host transforms (no --image_shard_dir), or pass --colour to store colour "
                             "images as three planes, which the device resamples and folds to luma as Pillow does" % colour)
        if keep_colour:
            n3 = sum(1 for row in w.index if row[3] == 3)
            print("wrote %s (%d images: %d grayscale of one plane, %d colour of three; %.3f GB) + .idx.npy"
                  % (out, len(paths), len(paths) - n3, n3, os.path.getsize(out) / 1e9))
        else:
            print("wrote %s (%d images, %.3f GB) + .idx.npy" % (out, len(paths), os.path.getsize(out) / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_path", help="pre-training: the directory of mimic-cxr-2.0.0-entity-llm.csv")
    ap.add_argument("--out", help="pre-training: the shard file to write")
    ap.add_argument("--max_side", type=int, default=0)
    ap.add_argument("--workers", type=int, default=os.cpu_count() or 1)
    ap.add_argument("--list_dir", help="classification: the directory of train_list*.txt / val_list.txt / test_list.txt")
    ap.add_argument("--dataset_path", help="classification: the root the lists' relative paths start from")
    ap.add_argument("--out_dir", help="classification: where <list file name>.u8 go (default: --list_dir)")
    ap.add_argument("--splits", nargs="*", default=None, help="classification: list file names (default: every known one that exists)")
    ap.add_argument("--colour", action="store_true", help="classification (--list_dir): keep colour images as three planes (grayscale ones stay one plane) "
                                                          "instead of ending the run at the first; the device folds them to luma behind the resample")
    a = ap.parse_args()
    if a.colour and not a.list_dir:
        ap.error("--colour goes with --list_dir (the classification shards); the pre-training shard is grayscale")
    if a.list_dir:
        if a.dataset_path is None or a.data_path or a.out or a.max_side:
            ap.error("--list_dir goes with --dataset_path [--out_dir] [--splits]; --data_path / --out / --max_side belong to the pre-training mode")
        return shard_lists(a.list_dir, a.dataset_path, a.out_dir or a.list_dir, a.splits, a.workers, a.colour)
    if not (a.data_path and a.out):
        ap.error("--data_path and --out are required (or --list_dir and --dataset_path)")
    import pandas as pd
    from ecamp_amd.module.pretrain_datasets import U8ShardWriter
    paths = list(pd.read_csv(os.path.join(a.data_path, "mimic-cxr-2.0.0-entity-llm.csv"))["img_path"])
    with U8ShardWriter(a.out) as w, ProcessPoolExecutor(a.workers) as ex:
        for n, arr in enumerate(ex.map(decode, [(p, a.max_side) for p in paths], chunksize=8)):
            w.add(arr)
            if n % 1000 == 0:
                print("%d / %d" % (n, len(paths)), flush=True)
    print("wrote %s (%.1f GB) + .idx.npy" % (a.out, os.path.getsize(a.out) / 1e9))


if __name__ == "__main__":
    main()
