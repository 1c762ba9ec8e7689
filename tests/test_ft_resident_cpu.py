"""The host half of `--image_shard_resident` (module/finetune_datasets.py: `resident_item`, `pack_resident`, `ResidentShard.fits`; the
drivers' flags), without a device: a resident dataset draws the boxes of the non-resident one from the index alone, its table rows address
in the shard file exactly the bytes `pack_boxes` copies, and the drivers refuse the flag where it has no shard to keep.  Every comparison
is equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ft_colour_ref as C  # noqa: E402
import _ft_image_ref as R  # noqa: E402

from ecamp_amd.module import finetune_datasets as fd  # noqa: E402
from ecamp_amd.module.pretrain_datasets import U8ShardWriter  # noqa: E402

SIZE = 16
# (h, w) of the stored images; in the colour shard every second one has three planes (the others are gray sources: one plane)
SHAPES = [(37, 53), (64, 64), (5, 7), (90, 16), (11, 40), (200, 150), (20, 90), (9, 11)]


def _write_task(root, colour):
    """lists + one shard per split under `root`, written with `U8ShardWriter` -> (shard_dir, list_dir)."""
    shards, lists = os.path.join(root, "shards"), os.path.join(root, "lists")
    os.makedirs(shards), os.makedirs(lists)
    for name, seed in (("train_list.txt", 0), ("val_list.txt", 50), ("test_list.txt", 90)):
        with open(os.path.join(lists, name), "w") as f:
            for n in range(len(SHAPES)):
                f.write("img_%d.png %d %d\n" % (n, n % 2, (n // 2) % 2))
        with U8ShardWriter(os.path.join(shards, name + ".u8"), colour=colour) as w:
            for n, (h, wd) in enumerate(SHAPES):
                if colour:
                    g = R.gray_image(h, wd, seed + n)
                    w.add(C.colour_image(h, wd, seed + n).transpose(1, 2, 0) if n % 2 else np.stack([g, g, g], axis=-1))
                else:
                    w.add(R.gray_image(h, wd, seed + n))
    return shards, lists


@pytest.fixture(scope="module", params=[False, True], ids=["gray", "colour"])
def task(request, tmp_path_factory):
    shards, lists = _write_task(str(tmp_path_factory.mktemp("resident_cpu")), request.param)
    return shards, lists, request.param


def _items(task, split, resident, seed=7):
    shards, lists, _ = task
    ds = fd.ShardListDataset(shards, lists, split, data_volume="100", img_size=SIZE, ratio=1.3, resident=resident)
    torch.manual_seed(seed)
    return ds, [ds[n] for n in range(len(ds))]


@pytest.mark.parametrize("split", ["train", "val"])
def test_resident_rows_hold_the_boxes_of_the_non_resident_dataset(task, split):
    ds, host = _items(task, split, False)
    rds, rows = _items(task, split, True)
    assert rds.shard is None and len(rows) == len(host) == len(SHAPES)          # the file is never mapped
    flips = []
    for (box, flip, geom), y in host:
        flips.append(bool(flip))
    for n, (((box, flip, geom), y), (row, ry)) in enumerate(zip(host, rows)):
        assert row.dtype == np.int64 and row.shape == (12,)
        assert (int(row[1]), int(row[2]), bool(row[3]), tuple(int(v) for v in row[5:9])) == (box.shape[-2], box.shape[-1], bool(flip), tuple(geom)), n
        assert (row[9] == 3) == (box.ndim == 3) and torch.equal(y, ry)
        H, W = SHAPES[n]
        assert (int(row[10]), int(row[11])) == (W, H * W)
    if split == "train":
        assert any(flips) and not all(flips)                                        # the flip is drawn, and drawn alike
        assert any(int(r[1]) < SHAPES[n][0] and int(r[2]) < SHAPES[n][1] for n, (r, _) in enumerate(rows))   # boxes strictly smaller than their images
    else:
        assert not any(flips) and all((int(r[1]), int(r[2])) == SHAPES[n] for n, (r, _) in enumerate(rows))  # evaluation: the whole image
    if task[2]:
        assert [int(r[9]) for r, _ in rows] == [3 if n % 2 else 0 for n in range(len(SHAPES))]


@pytest.mark.parametrize("split", ["train", "test"])
def test_table_and_meta_equal_pack_boxes_and_the_rows_gather_its_bytes(task, split):
    _, host = _items(task, split, False)
    _, rows = _items(task, split, True)
    flat, table, meta = fd.pack_boxes([it for it, _ in host])
    rtable, rmeta = fd.pack_resident([r for r, _ in rows])
    assert rtable.dtype == torch.int64 and tuple(rtable.shape) == (len(SHAPES), 12)
    assert torch.equal(rtable[:, 1:10], table[:, 1:10]) and rmeta == meta
    assert (len(meta) == 4) == task[2]
    ct, cmeta, cy = fd.collate_resident(rows)
    assert torch.equal(ct, rtable) and cmeta == meta and torch.equal(cy, torch.stack([y for _, y in rows]))
    # gather every box from the shard FILE by off / pitch / plane_pitch: the bytes that pack_boxes copied, in its order
    data = np.fromfile(fd.shard_path(task[0], split, "100"), dtype=np.uint8)
    flat, got = flat.numpy(), []
    for off, h, w, _, _, _, _, _, _, c, pitch, plane_pitch in rtable.tolist():
        for p in range(3 if c == 3 else 1):
            for r in range(h):
                a = off + p * plane_pitch + r * pitch
                got.append(data[a:a + w])
        assert off + ((3 if c == 3 else 1) - 1) * plane_pitch + (h - 1) * pitch + w <= data.size        # the device's range guard holds
    assert np.array_equal(np.concatenate(got), flat)


def test_fits_at_its_boundaries():
    fits = fd.ResidentShard.fits
    assert fd.ResidentShard.FREE_DIVISOR == 2
    assert fits(500, 1000) and fits(500, 1001) and not fits(501, 1001) and not fits(501, 1000) and fits(0, 0)   # one half of what is free, rounded down
    assert fits(1000, 10, max_bytes=1000) and not fits(1001, 10 ** 12, max_bytes=1000)                             # max_bytes replaces the rule
    assert fits(900, 1000, max_bytes=900) and not fits(400, 1000, max_bytes=399)


def _parse(mod, *extra):
    return mod.get_args_parser().parse_args(["--name", "t", "--pretrained_path", "x.pth"] + list(extra))


@pytest.mark.parametrize("driver,mode", [("main_linprobe", "LinearProbe"), ("main_finetune", "Finetune")])
def test_driver_refusals(task, driver, mode):
    import importlib
    mod = importlib.import_module("ecamp_amd." + driver)
    shards, lists, _ = task
    common = ("--mode", mode, "--list_dir", lists)
    with pytest.raises(SystemExit, match=r"--image_shard_resident needs --image_shard_dir"):
        mod.check_args(_parse(mod, *common, "--dataset_path", "D", "--image_shard_resident"))
    with pytest.raises(SystemExit, match=r"--image_shard_resident with --synthetic"):
        mod.check_args(_parse(mod, *common, "--synthetic", "--image_shard_resident"))
    with pytest.raises(SystemExit, match=r"with --synthetic"):
        mod.check_args(_parse(mod, *common, "--synthetic", "--image_shard_resident", "--image_shard_dir", shards))
    with pytest.raises(SystemExit, match=r"--image_shard_resident_max_gb without --image_shard_resident"):
        mod.check_args(_parse(mod, *common, "--image_shard_dir", shards, "--image_shard_resident_max_gb", "1"))
    a = mod.check_args(_parse(mod, *common, "--image_shard_dir", shards, "--image_shard_resident", "--image_shard_resident_max_gb", "0.5"))
    assert a.image_shard_resident is True and a.image_shard_resident_max_gb == 0.5
    from ecamp_amd import main_linprobe
    assert main_linprobe.resident_max_bytes(a) == 500_000_000
    plain = mod.check_args(_parse(mod, *common, "--dataset_path", "D"))                       # a plain command line parses as before
    assert plain.image_shard_resident is False and plain.image_shard_resident_max_gb is None and plain.image_shard_dir == ""
    assert main_linprobe.resident_max_bytes(plain) is None
    assert mod.check_args(_parse(mod, *common, "--image_shard_dir", shards)).image_shard_resident is False


def test_the_binding_declares_the_entry_point():
    import ctypes
    from ecamp_amd import _lib, hip_ops
    ret, args = _lib.parse_header()["ecamp_resample_shard_u8"]
    assert ret is ctypes.c_int32
    assert [a[1] for a in args] == ["shard", "shard_bytes", "table", "dst", "B", "out", "kmax", "tmp_rows", "max_h", "filter", "ws", "ws_bytes", "err_flag", "stream"]
    assert args[1][0] is ctypes.c_int64 and args[0][0] is ctypes.c_void_p
    assert callable(hip_ops.resample_shard_u8)
    for name in ("ecamp_resample_crops_u8", "ecamp_resample_boxes_u8", "ecamp_resample_boxes_rgb_u8"):   # the three before it keep their lists
        assert [a[1] for a in _lib.parse_header()[name][1]][:3] ==["src", "table", "dst"]
    assert _lib.abi_version_of_header() == 5
