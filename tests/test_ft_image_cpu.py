"""The classification image pipeline's host side, without a device: the restatement of ecamp_resample_boxes_u8 (tests/_ft_image_ref.py)
against Pillow's own bytes, the worker-side items (module/finetune_datasets.py), the normalisation table, the shard tool, the drivers'
refusals and the header."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ft_image_ref as R  # noqa: E402


@pytest.mark.parametrize("h,w,size,ratio", R.EVAL_CASES)
def test_restatement_and_eval_item_give_the_bytes_of_eval_transform(h, w, size, ratio):
    """Resize(int(size / ratio)) + CenterCrop((size, size)) by Pillow, against ONE resample per axis with `device_eval_item`'s full / shift."""
    from ecamp_amd.module import finetune_datasets as fd
    img = R.gray_image(h, w, seed=h * 100 + w)
    want = R.pil_eval_bytes(img, size, ratio)
    box, flip, geom = fd.device_eval_item(img, size, ratio)
    assert flip is False and box.dtype == np.uint8 and np.array_equal(box, img)
    assert all(isinstance(v, int) for v in geom) and geom == fd.eval_geometry(w, h, size, ratio)
    got = R.resample_box(box, size, geom)
    assert np.array_equal(got, want), (geom, int((got != want).sum()))
    # and the f32 item of the host path is the table applied to these bytes
    assert torch.equal(fd.eval_transform(size, ratio)(R.as_rgb(img)), R.normalise(want))


def test_eval_geometry_of_the_padding_and_shift_cases():
    from ecamp_amd.module import finetune_datasets as fd
    assert fd.eval_geometry(47, 61, 16, 2) == (8, -4, 10, -3)           # S = 8: (nw, nh) = (8, 10), padding on both axes
    fw, sw, fh, sh = fd.eval_geometry(90, 20, 16, 1.3)                   # S = 12: (54, 12): shift 19 on the long axis, padding on the other
    assert (fw, sw, fh, sh) == (54, 19, 12, -2)
    assert fd.eval_geometry(16, 16, 16, 1) == (16, 0, 16, 0)             # short == S: no resize
    assert fd.eval_geometry(16, 40, 16, 1) == (16, 0, 40, 12)
    for d in range(0, 41):                                               # Python's round(d / 2.0), in integers
        assert fd._round_half_even_of_half(d) == int(round(d / 2.0))


@pytest.mark.parametrize("h,w,out", R.TRAIN_CASES)
@pytest.mark.parametrize("flip", [False, True])
def test_restatement_gives_the_bytes_of_a_training_crop(h, w, out, flip):
    img = R.gray_image(h, w, seed=h + w)
    want = R.pil_train_bytes(img, out, flip)
    got = R.resample_box(img, out, (out, 0, out, 0), flip=flip)
    assert np.array_equal(got, want), int((got != want).sum())


def test_bicubic_restatement_equals_pillow():
    from PIL import Image
    for h, w in ((37, 53), (5, 7), (200, 150)):
        img = R.gray_image(h, w, seed=3)
        want = np.asarray(Image.fromarray(img, "L").resize((16, 16), Image.BICUBIC))
        assert np.array_equal(R.resample_box(img, 16, (16, 0, 16, 0), filt=R.BICUBIC), want)


@pytest.mark.parametrize("seed", [0, 1, 7, 11])
def test_train_item_draws_what_train_transform_draws(seed):
    """One torch seed: the same box, the same flip, the generator left in the same state -- and the item's resample IS the host item."""
    from ecamp_amd.module import finetune_datasets as fd
    from ecamp_amd.module.pretrain_datasets import random_flip, random_resized_crop_params
    img = R.gray_image(83, 61, seed)
    torch.manual_seed(seed)
    want = fd.train_transform(16)(R.as_rgb(img))
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    box, flip, geom = fd.device_train_item(img, 16)
    assert torch.equal(torch.get_rng_state(), state)
    torch.manual_seed(seed)
    i, j, h, w = random_resized_crop_params(61, 83, scale=(0.08, 1.0))
    assert flip == random_flip() and np.array_equal(box, img[i:i + h, j:j + w]) and box.dtype == np.uint8
    assert geom == (16, 0, 16, 0)
    assert torch.equal(R.normalise(R.resample_box(box, 16, geom, flip=flip)), want)


def test_pack_boxes_lays_out_table_bytes_and_meta():
    from ecamp_amd.module import finetune_datasets as fd
    items = [fd.device_eval_item(R.gray_image(61, 47, 1), 16, 2), fd.device_eval_item(R.gray_image(20, 90, 2), 16, 1.3),
             (R.gray_image(200, 150, 3), True, (16, 0, 16, 0))]
    flat, table, meta = fd.pack_boxes(items)
    assert table.dtype == torch.int64 and table.shape == (3, 10) and flat.dtype == torch.uint8
    off = row = 0
    for n, (c, flip, g) in enumerate(items):
        h, w = c.shape
        assert table[n].tolist() == [off, h, w, int(flip), row] + list(g) + [0]
        assert np.array_equal(flat[off:off + h * w].numpy().reshape(h, w), c)
        off += h * w
        row += h
    assert meta == (max(R.ksize(200, 16), R.ksize(47, 8), R.ksize(90, 54)), 61 + 20 + 200, 200) and all(isinstance(v, int) for v in meta)
    f2, t2, m2, y = fd.collate_boxes([(it, torch.FloatTensor([n, 1])) for n, it in enumerate(items)])
    assert torch.equal(f2, flat) and torch.equal(t2, table) and m2 == meta and y.tolist() == [[0, 1], [1, 1], [2, 1]]


def test_normalisation_table_is_the_host_arithmetic_on_every_byte():
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import finetune_datasets as fd
    from PIL import Image
    u = np.arange(256, dtype=np.uint8).reshape(16, 16)
    want = fd._to_normalised_gray3(Image.fromarray(u, "L"), 16)[0].reshape(-1)
    lut = ops.image_lut("cpu", fd.FT_MEAN, fd.FT_STD)
    assert lut.dtype == torch.float32 and torch.equal(lut.view(torch.int32), want.view(torch.int32))
    # keyed by the constants: the default stays pre-training's pair, and is another table
    pre = ops.image_lut("cpu")
    assert torch.equal(pre, torch.arange(256, dtype=torch.float32).div(255.0).sub(0.4721).div(0.3037)) and not torch.equal(pre, lut)
    assert ops.image_lut("cpu", fd.FT_MEAN, fd.FT_STD) is lut and ops.image_lut("cpu") is pre


def test_tap_formula_covers_pillows_tap_count():
    """`bilinear_taps` (integers, the host's size of the device tap tables) == Pillow's ksize, scales below, at and above 1; and every
    restated tap row fits it and sums to 2^22 up to rounding."""
    from ecamp_amd.module import finetune_datasets as fd
    for n, full in ((1, 16), (5, 16), (15, 16), (16, 16), (17, 16), (31, 16), (32, 16), (33, 16), (200, 16), (1024, 224), (3056, 224), (224, 224), (90, 54), (47, 8)):
        k = R.ksize(n, full)
        assert fd.bilinear_taps(n, full) == k, (n, full)
        bounds, kk = R.coeffs(n, full, 0, full)
        assert kk.shape[1] == k and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= k).all() and (bounds.sum(1) <= n).all()
        assert np.abs(kk.sum(1) - (1 << 22)).max() <= k


def _write_task(root, n_per_list=(5, 3, 4), colour_at=None):
    """A data root with grayscale PNGs (lossless) and the three list files; -> {list file name: [uint8 arrays]}."""
    from PIL import Image
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    os.makedirs(os.path.join(root, "lists"), exist_ok=True)
    out, k = {}, 0
    for name, n in zip(("train_list.txt", "val_list.txt", "test_list.txt"), n_per_list):
        lines, arrs = [], []
        for _ in range(n):
            a = R.gray_image(40 + 7 * k, 52 - 3 * k, 20 + k)
            rel = "img/i%d.png" % k
            if colour_at == k:
                rgb = np.stack([a, a, a], -1)
                rgb[3, 4, 1] ^= 1
                Image.fromarray(rgb, "RGB").save(os.path.join(root, rel))
            else:
                Image.fromarray(a, "L").save(os.path.join(root, rel))
            lines.append("%s %d %d %d" % (rel, k % 2, (k // 2) % 2, (k + 1) % 2))
            arrs.append(a)
            k += 1
        open(os.path.join(root, "lists", name), "w").write("\n".join(lines) + "\n")
        out[name] = arrs
    return out


def _make_shards(root, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_image_shard.py"), "--list_dir", os.path.join(root, "lists"), "--dataset_path", root,
                           "--out_dir", os.path.join(root, "shards"), "--workers", "2"] + list(extra), capture_output=True, text=True, timeout=300)


def test_shard_tool_round_trips_a_task_and_the_dataset_reads_it(tmp_path):
    from ecamp_amd.module import finetune_datasets as fd
    from ecamp_amd.module.pretrain_datasets import U8ShardReader
    root = str(tmp_path)
    arrs = _write_task(root)
    r = _make_shards(root)
    assert r.returncode == 0, r.stderr[-1500:]
    for name, want in arrs.items():
        rd = U8ShardReader(os.path.join(root, "shards", name + ".u8"))
        assert len(rd) == len(want) and all(np.array_equal(rd[k], want[k]) for k in range(len(want)))
    ds = fd.ShardListDataset(os.path.join(root, "shards"), os.path.join(root, "lists"), "val", img_size=16, ratio=1.0)
    host = fd.ListDataset(root, os.path.join(root, "lists"), "val", transform=fd.eval_transform(16, 1.0))
    assert len(ds) == len(host) == 3
    for k in range(3):
        (box, flip, geom), y = ds[k]
        img, yh = host[k]
        assert torch.equal(y, yh) and torch.equal(R.normalise(R.resample_box(box, 16, geom, flip)), img)
    tr = fd.ShardListDataset(os.path.join(root, "shards"), os.path.join(root, "lists"), "train", data_volume="100", img_size=16)
    th = fd.ListDataset(root, os.path.join(root, "lists"), "train", data_volume="100", transform=fd.train_transform(16))
    torch.manual_seed(5)
    (box, flip, geom), y = tr[2]
    torch.manual_seed(5)
    img, yh = th[2]
    assert torch.equal(y, yh) and torch.equal(R.normalise(R.resample_box(box, 16, geom, flip)), img)
    # through loader workers (the packed bytes are laid out in shared memory there): the batches of the in-process loader
    from torch.utils.data import DataLoader
    test = fd.ShardListDataset(os.path.join(root, "shards"), os.path.join(root, "lists"), "test", img_size=16, ratio=1.3)
    for a, b in zip(DataLoader(test, batch_size=3, num_workers=0, collate_fn=fd.collate_boxes), DataLoader(test, batch_size=3, num_workers=2, collate_fn=fd.collate_boxes)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and tuple(a[2]) == tuple(b[2]) and torch.equal(a[3], b[3])
    # --splits: one list only
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_image_shard.py"), "--list_dir", os.path.join(root, "lists"), "--dataset_path", root,
                        "--out_dir", os.path.join(root, "one"), "--splits", "test_list.txt", "--workers", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and sorted(os.listdir(os.path.join(root, "one"))) == ["test_list.txt.u8", "test_list.txt.u8.idx.npy"]


def test_shard_tool_refuses_a_colour_image_by_name(tmp_path):
    root = str(tmp_path)
    _write_task(root, colour_at=6)          # the second image of val_list.txt: one bit of one channel
    r = _make_shards(root)
    assert r.returncode != 0
    assert "img/i6.png" in r.stderr and "COLOUR" in r.stderr and "grayscale sources only" in r.stderr
    assert not os.path.exists(os.path.join(root, "shards", "val_list.txt.u8"))      # no partial shard


def _driver_args(module, root, *extra):
    return module.get_args_parser().parse_args(["--name", "t", "--model", "vit_tiny_patch16", "--task", "CheXpert", "--num_classes", "3", "--img_size", "224",
                                                "--pretrained_path", "x.pth", "--dataset_path", root, "--list_dir", os.path.join(root, "lists"),
                                                "--output_dir", os.path.join(root, "out")] + list(extra))


@pytest.mark.parametrize("driver", ["linprobe", "finetune"])
def test_drivers_refuse_bad_shards_before_any_device_work(tmp_path, driver):
    from ecamp_amd import main_finetune, main_linprobe
    mod, mode = (main_linprobe, "LinearProbe") if driver == "linprobe" else (main_finetune, "Finetune")
    root = str(tmp_path)
    _write_task(root)
    shards = os.path.join(root, "shards")
    with pytest.raises(SystemExit, match=r"--image_shard_dir .*train split.*train_list\.txt\.u8.*not found"):     # no shard at all
        mod.check_args(_driver_args(mod, root, "--mode", mode, "--image_shard_dir", shards))
    assert _make_shards(root).returncode == 0
    a = mod.check_args(_driver_args(mod, root, "--mode", mode, "--image_shard_dir", shards))                    # complete: accepted
    assert a.image_shard_dir == shards
    os.remove(os.path.join(shards, "test_list.txt.u8"))
    with pytest.raises(SystemExit, match=r"test split.*test_list\.txt\.u8.*not found"):                            # one split's shard missing
        mod.check_args(_driver_args(mod, root, "--mode", mode, "--image_shard_dir", shards, "--stage", "test"))
    assert _make_shards(root).returncode == 0
    with open(os.path.join(root, "lists", "val_list.txt"), "a") as f:                                              # the list grew after the shard was made
        f.write("img/i0.png 1 0 1\n")
    with pytest.raises(SystemExit, match=r"val split.*holds 3 images.*lists 4"):
        mod.check_args(_driver_args(mod, root, "--mode", mode, "--image_shard_dir", shards))
    mod.check_args(_driver_args(mod, root, "--mode", mode, "--image_shard_dir", shards, "--stage", "test"))      # --stage test reads the test split alone
    with pytest.raises(SystemExit, match=r"--image_shard_dir with --synthetic"):
        mod.check_args(_driver_args(mod, root, "--mode", mode, "--image_shard_dir", shards, "--synthetic"))
    assert mod.check_args(_driver_args(mod, root, "--mode", mode)).image_shard_dir == ""                          # opt-in: off by default


def test_header_declares_the_two_entry_points_at_abi_5():
    from ecamp_amd import _lib
    protos = _lib.parse_header()
    assert _lib.abi_version_of_header() == 5          # entry points were added, no signature changed
    names = [a[1] for a in protos["ecamp_resample_boxes_u8"][1]]
    assert names == ["src", "table", "dst", "B", "out", "kmax", "tmp_rows", "max_h", "filter", "ws", "ws_bytes", "err_flag", "stream"]
    assert [a[1] for a in protos["ecamp_resample_boxes_workspace_bytes"][1]] == ["B", "out", "kmax", "tmp_rows"]
    assert [a[1] for a in protos["ecamp_im2col_u8"][1]] == ["img", "lut", "ids_keep", "out", "B", "Lk", "R", "p", "dtype", "stream"]
    # the old entry point keeps its signature
    assert [a[1] for a in protos["ecamp_resample_crops_u8"][1]] == ["src", "table", "dst", "B", "out", "kmax", "tmp_rows", "max_h", "ws", "ws_bytes", "err_flag", "stream"]
