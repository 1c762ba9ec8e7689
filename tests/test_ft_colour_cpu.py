"""Colour sources in the classification image pipeline, without a device: the restatement of ecamp_resample_boxes_rgb_u8
(tests/_ft_colour_ref.py: per-plane resample, then Pillow's luma fold) against Pillow's own bytes through the product's host transforms,
the colour shard writer / reader, the worker-side items and `pack_boxes` on mixed batches, the shard tool's --colour, and the header."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ft_colour_ref as C  # noqa: E402
import _ft_image_ref as R  # noqa: E402


@pytest.mark.parametrize("out", C.OUTS)
@pytest.mark.parametrize("h,w", C.SIZES)
def test_restatement_gives_the_bytes_of_eval_transform_on_a_colour_image(h, w, out):
    """Resize + CenterCrop + Grayscale by Pillow on the RGB image, against per-plane resample + fold with `device_eval_item`'s geometry:
    ratios 0.5, 0.875, 1 and 2 -- among them padding on one axis and on both."""
    from ecamp_amd.module import finetune_datasets as fd
    img = C.colour_image(h, w, seed=h * 100 + w)
    for ratio in C.RATIOS:
        want = C.pil_eval_bytes(img, out, ratio)
        box, flip, geom = fd.device_eval_item(img, out, ratio)
        assert flip is False and box.shape == (3, h, w) and np.array_equal(box, img) and geom == fd.eval_geometry(w, h, out, ratio)
        got = C.resample_colour_box(box, out, geom)
        assert np.array_equal(got, want), (ratio, geom, int((got != want).sum()))
        assert torch.equal(fd.eval_transform(out, ratio)(C.as_pil(img)), R.normalise(want))          # the host's f32 item is the table on these bytes


def test_eval_cases_hold_padding_on_one_axis_and_on_both():
    from ecamp_amd.module import finetune_datasets as fd
    seen = set()
    for h, w in C.SIZES:
        for out in C.OUTS:
            for ratio in C.RATIOS:
                _, sw, _, sh = fd.eval_geometry(w, h, out, ratio)
                seen.add((sw < 0) + (sh < 0))
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("out", C.OUTS)
@pytest.mark.parametrize("h,w", C.SIZES)
def test_restatement_gives_the_bytes_of_train_transform_on_a_colour_image(h, w, out):
    """Through `train_transform` itself: one seed, the drawn box and flip of `device_train_item`, the host's f32 item; both flip values are
    met over the seeds."""
    from ecamp_amd.module import finetune_datasets as fd
    img = C.colour_image(h, w, seed=h + w)
    flips = set()
    for seed in range(6):
        torch.manual_seed(seed)
        want = fd.train_transform(out)(C.as_pil(img))
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        box, flip, geom = fd.device_train_item(img, out)
        assert torch.equal(torch.get_rng_state(), state) and box.ndim == 3 and box.shape[0] == 3 and geom == (out, 0, out, 0)
        got = C.resample_colour_box(box, out, geom, flip)
        assert np.array_equal(got, C.pil_train_bytes(box, out, flip))
        assert torch.equal(R.normalise(got), want), seed
        flips.add(bool(flip))
    assert flips == {False, True}


def test_fold_of_pure_colours_and_white():
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]], dtype=np.uint8).T      # [3, 5]
    assert C.luma(px).tolist() == [76, 150, 29, 255, 0]
    from PIL import Image
    assert np.asarray(Image.fromarray(px.T[None].copy(), "RGB").convert("L")).tolist() == [[76, 150, 29, 255, 0]]
    # an image of one pure colour stays that colour's luma through the resample
    for p, v in enumerate((76, 150, 29)):
        img = np.zeros((3, 37, 53), dtype=np.uint8)
        img[p] = 255
        assert (C.resample_colour_box(img, 16, (16, 0, 16, 0)) == v).all()


def test_gray_plane_first_is_not_pillows_order():
    """Why the fold sits behind the vertical pass: resampling the folded plane differs from Pillow on these images, by 1."""
    differing = 0
    for h, w in C.SIZES:
        img = C.colour_image(h, w, seed=h + w)
        want = C.pil_train_bytes(img, 16)
        assert np.array_equal(C.resample_colour_box(img, 16, (16, 0, 16, 0)), want)
        wrong = C.gray_first_box(img, 16, (16, 0, 16, 0))
        d = np.abs(wrong.astype(int) - want.astype(int))
        assert d.max() <= 1
        differing += int(d.sum())
    assert differing > 0


def test_bicubic_restatement_equals_pillow_on_a_colour_image():
    from PIL import Image
    for h, w in ((37, 53), (5, 7), (200, 150)):
        img = C.colour_image(h, w, seed=3)
        assert np.array_equal(C.resample_colour_box(img, 16, (16, 0, 16, 0), filt=R.BICUBIC), C.pil_train_bytes(img, 16, filt=Image.BICUBIC))


# ------------------------------------------------------------------------------------------------------------------------ shards
def test_colour_writer_and_reader_round_trip_a_mixed_shard(tmp_path):
    from PIL import Image
    from ecamp_amd.module.pretrain_datasets import U8ShardReader, U8ShardWriter
    g0, c1, g2, c3 = R.gray_image(9, 13, 1), C.colour_image(7, 5, 2), R.gray_image(4, 6, 3), C.colour_image(11, 3, 4)
    path = str(tmp_path / "mixed.u8")
    with U8ShardWriter(path, colour=True) as w:
        assert w.add(np.stack([g0, g0, g0], -1)) == 0               # [H, W, 3] with equal channels: one plane
        assert w.add(C.as_pil(c1)) == 1                            # an RGB PIL image
        assert w.add(R.as_rgb(g2)) == 2                            # what pil_loader makes of a grayscale file
        assert w.add(np.ascontiguousarray(c3.transpose(1, 2, 0))) == 3
        with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
            w.add(g0)
    idx = np.load(path + ".idx.npy")
    assert idx.dtype == np.int64 and idx.tolist() == [[0, 9, 13, 1], [117, 7, 5, 3], [117 + 105, 4, 6, 1], [117 + 105 + 24, 11, 3, 3]]
    assert os.path.getsize(path) == 117 + 105 + 24 + 99
    rd = U8ShardReader(path)
    assert len(rd) == 4 and [rd.planes(i) for i in range(4)] == [1, 3, 1, 3]
    for i, want in enumerate((g0, c1, g2, c3)):
        assert rd[i].dtype == np.uint8 and rd[i].shape == want.shape and np.array_equal(rd[i], want)
    with pytest.raises(ValueError, match="max_side"):
        U8ShardWriter(str(tmp_path / "x.u8"), max_side=8, colour=True)
    # the planes of a colour image lie back to back: R, G, B
    raw = np.fromfile(path, dtype=np.uint8)
    assert np.array_equal(raw[117:117 + 35].reshape(7, 5), c1[0]) and np.array_equal(raw[117 + 70:117 + 105].reshape(7, 5), c1[2])
    assert Image.fromarray(np.ascontiguousarray(rd[1].transpose(1, 2, 0)), "RGB").tobytes() == C.as_pil(c1).tobytes()


def test_default_writer_is_unchanged_and_a_three_column_index_reads_as_gray(tmp_path):
    from ecamp_amd.module.pretrain_datasets import U8ShardReader, U8ShardWriter
    imgs = [R.gray_image(9, 13, 1), R.gray_image(4, 6, 3)]
    path = str(tmp_path / "gray.u8")
    with U8ShardWriter(path) as w:
        w.add(imgs[0])
        w.add(R.as_rgb(imgs[1]))                                   # colour inputs go through convert("L"), as before
    # the plain writer's files, restated: the planes back to back, and an int64 [N, 3] index of (offset, H, W)
    assert open(path, "rb").read() == imgs[0].tobytes() + imgs[1].tobytes()
    idx = np.load(path + ".idx.npy")
    assert idx.dtype == np.int64 and idx.shape == (2, 3) and idx.tolist() == [[0, 9, 13], [117, 4, 6]]
    want_npy = str(tmp_path / "want.npy")
    np.save(want_npy, np.asarray([(0, 9, 13), (117, 4, 6)], dtype=np.int64).reshape(-1, 3))
    assert open(path + ".idx.npy", "rb").read() == open(want_npy, "rb").read()
    rd = U8ShardReader(path)
    assert [rd.planes(i) for i in range(2)] == [1, 1]
    assert all(rd[i].shape == imgs[i].shape and np.array_equal(rd[i], imgs[i]) for i in range(2))


# ------------------------------------------------------------------------------------------------------------------- loader side
def _mixed_items():
    from ecamp_amd.module import finetune_datasets as fd
    return [fd.device_eval_item(R.gray_image(61, 47, 1), 16, 2), fd.device_eval_item(C.colour_image(20, 90, 2), 16, 1.3),
            (C.colour_image(200, 150, 3)[:, 10:43, 5:100], True, (16, 0, 16, 0)),      # a non-contiguous colour view, as a training box is
            (R.gray_image(11, 40, 4), False, (16, 0, 16, 0)), (C.colour_image(11, 40, 5), False, (16, 0, 16, 0))]


def test_pack_boxes_on_a_mixed_batch():
    from ecamp_amd.module import finetune_datasets as fd
    items = _mixed_items()
    flat, table, meta = fd.pack_boxes(items)
    assert table.dtype == torch.int64 and table.shape == (5, 10) and flat.dtype == torch.uint8
    off = row = max_h = 0
    for n, (c, flip, g) in enumerate(items):
        planes = 3 if c.ndim == 3 else 1
        h, w = c.shape[-2:]
        assert table[n].tolist() == [off, h, w, int(flip), row] + list(g) + [3 if planes == 3 else 0]
        assert np.array_equal(flat[off:off + planes * h * w].numpy().reshape(c.shape), c)          # planes contiguous, R then G then B
        off += planes * h * w
        row += planes * h
        max_h = max(max_h, planes * h)
    assert flat.numel() == off
    assert table[:, 9].tolist() == [0, 3, 3, 0, 3] and table[:, 4].tolist() == [0, 61, 61 + 60, 61 + 60 + 99, 61 + 60 + 99 + 11]
    assert max_h == 99 and row == 61 + 60 + 99 + 11 + 33
    taps = max(max(R.ksize(c.shape[-1], g[0]), R.ksize(c.shape[-2], g[2])) for c, _, g in items)
    assert taps == R.ksize(61, 10) == 15
    assert tuple(meta) == (taps, row, max_h, True) and all(isinstance(v, int) for v in meta)
    f2, t2, m2, y = fd.collate_boxes([(it, torch.FloatTensor([n])) for n, it in enumerate(items)])
    assert torch.equal(f2, flat) and torch.equal(t2, table) and tuple(m2) == tuple(meta) and y.shape == (5, 1)


def test_pack_boxes_on_gray_items_is_the_parents():
    """Restated: boxes back to back, rows of (off, h, w, flip, row0, full_w, shift_w, full_h, shift_h, 0), meta = (taps, sum h, max h) -- and
    no colour flag, so `DeviceBoxResampler` takes the one-plane call."""
    from ecamp_amd.module import finetune_datasets as fd
    items = [fd.device_eval_item(R.gray_image(61, 47, 1), 16, 2), fd.device_eval_item(R.gray_image(20, 90, 2), 16, 1.3),
             (R.gray_image(200, 150, 3)[3:150, 7:99], True, (16, 0, 16, 0))]
    flat, table, meta = fd.pack_boxes(items)
    want_flat = np.concatenate([np.ascontiguousarray(c).reshape(-1) for c, _, _ in items])
    assert flat.dtype == torch.uint8 and np.array_equal(flat.numpy(), want_flat)
    want = [[0, 61, 47, 0, 0, 8, -4, 10, -3, 0], [61 * 47, 20, 90, 0, 61, 54, 19, 12, -2, 0], [61 * 47 + 20 * 90, 147, 92, 1, 81, 16, 0, 16, 0, 0]]
    assert table.dtype == torch.int64 and table.tolist() == want
    assert tuple(meta[:3]) == (max(R.ksize(147, 16), R.ksize(47, 8), R.ksize(90, 54)), 61 + 20 + 147, 147)
    assert not any(meta[3:])


@pytest.mark.parametrize("seed", [0, 1, 7, 11])
def test_train_item_draws_the_same_box_and_flip_for_colour_and_gray(seed):
    from ecamp_amd.module import finetune_datasets as fd
    col = C.colour_image(83, 61, seed)
    torch.manual_seed(seed)
    gbox, gflip, ggeom = fd.device_train_item(col[0], 16)
    gstate = torch.get_rng_state()
    torch.manual_seed(seed)
    cbox, cflip, cgeom = fd.device_train_item(col, 16)
    assert torch.equal(torch.get_rng_state(), gstate)                      # the same number of RNG calls
    assert cflip == gflip and cgeom == ggeom and cbox.shape == (3,) + gbox.shape and np.array_equal(cbox[0], gbox)
    assert np.shares_memory(cbox, col)                                     # a view: `pack_boxes` makes the one copy
    # a PIL image: colour keeps three planes, equal channels fold to one
    torch.manual_seed(seed)
    pbox, pflip, _ = fd.device_train_item(C.as_pil(col), 16)
    assert pflip == cflip and np.array_equal(pbox, cbox)
    torch.manual_seed(seed)
    qbox, _, _ = fd.device_train_item(R.as_rgb(col[0]), 16)
    assert np.array_equal(qbox, gbox)


# --------------------------------------------------------------------------------------------------------------------------- tool
def _write_task(root, colour_at):
    """`test_ft_image_cpu._write_task` with really different planes in the colour file -> {list file name: [uint8 [H, W] or [3, H, W]]}."""
    from PIL import Image
    os.makedirs(os.path.join(root, "img"), exist_ok=True)
    os.makedirs(os.path.join(root, "lists"), exist_ok=True)
    out, k = {}, 0
    for name, n in zip(("train_list.txt", "val_list.txt", "test_list.txt"), (5, 3, 4)):
        lines, arrs = [], []
        for _ in range(n):
            rel = "img/i%d.png" % k
            if k in colour_at:
                a = C.colour_image(40 + 7 * k, 52 - 3 * k, 20 + k)
                C.as_pil(a).save(os.path.join(root, rel))
            else:
                a = R.gray_image(40 + 7 * k, 52 - 3 * k, 20 + k)
                Image.fromarray(a, "L").save(os.path.join(root, rel))
            lines.append("%s %d %d %d" % (rel, k % 2, (k // 2) % 2, (k + 1) % 2))
            arrs.append(a)
            k += 1
        open(os.path.join(root, "lists", name), "w").write("\n".join(lines) + "\n")
        out[name] = arrs
    return out


def _tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_image_shard.py")] + list(args), capture_output=True, text=True, timeout=300)


def test_shard_tool_with_colour_keeps_three_planes_of_the_colour_file_alone(tmp_path):
    from ecamp_amd.module import finetune_datasets as fd
    from ecamp_amd.module.pretrain_datasets import U8ShardReader
    root = str(tmp_path)
    arrs = _write_task(root, colour_at={6})                     # the second image of val_list.txt
    lists, shards = os.path.join(root, "lists"), os.path.join(root, "shards")
    r = _tool("--list_dir", lists, "--dataset_path", root, "--out_dir", shards, "--workers", "2", "--colour")
    assert r.returncode == 0, r.stderr[-1500:]
    assert "val_list.txt.u8 (3 images: 2 grayscale of one plane, 1 colour of three" in r.stdout
    assert "train_list.txt.u8 (5 images: 5 grayscale of one plane, 0 colour of three" in r.stdout
    for name, want in arrs.items():
        rd = U8ShardReader(os.path.join(shards, name + ".u8"))
        assert rd.index.shape == (len(want), 4) and len(rd) == len(want)
        assert [rd.planes(k) for k in range(len(want))] == [3 if a.ndim == 3 else 1 for a in want]
        assert all(rd[k].shape == want[k].shape and np.array_equal(rd[k], want[k]) for k in range(len(want)))
    # the dataset over the colour shard yields the host item's bytes, colour and gray rows alike
    ds = fd.ShardListDataset(shards, lists, "val", img_size=16, ratio=1.0)
    host = fd.ListDataset(root, lists, "val", transform=fd.eval_transform(16, 1.0))
    for k in range(3):
        (box, flip, geom), y = ds[k]
        img, yh = host[k]
        got = C.resample_colour_box(box, 16, geom, flip) if box.ndim == 3 else R.resample_box(box, 16, geom, flip)
        assert box.ndim == (3 if k == 1 else 2) and torch.equal(y, yh) and torch.equal(R.normalise(got), img)
    batch = fd.collate_boxes([ds[k] for k in range(3)])
    assert batch[1][:, 9].tolist() == [0, 3, 0] and tuple(batch[2])[3] is True
    # without the flag: the present refusal, by name, now pointing at --colour
    r = _tool("--list_dir", lists, "--dataset_path", root, "--out_dir", os.path.join(root, "plain"), "--workers", "2")
    assert r.returncode != 0 and "img/i6.png" in r.stderr and "COLOUR" in r.stderr and "--colour" in r.stderr
    assert not os.path.exists(os.path.join(root, "plain", "val_list.txt.u8"))


def test_shard_tool_refuses_colour_outside_the_list_mode_and_with_max_side(tmp_path):
    r = _tool("--data_path", str(tmp_path), "--out", str(tmp_path / "x.u8"), "--colour")
    assert r.returncode == 2 and "--colour goes with --list_dir" in r.stderr
    r = _tool("--list_dir", str(tmp_path), "--dataset_path", str(tmp_path), "--colour", "--max_side", "512")
    assert r.returncode == 2 and "--max_side" in r.stderr


# ------------------------------------------------------------------------------------------------------------------------- header
@pytest.fixture(scope="module")
def libs():
    from ecamp_amd import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        from ecamp_amd import build
        build.build(verbose=False, half="both")
    return _lib.load("bf16"), _lib.load("f16")


def test_header_declares_the_colour_entry_point_and_both_builds_export_it(libs):
    from ecamp_amd import _lib
    protos = _lib.parse_header()
    assert _lib.abi_version_of_header() == 5          # an entry point was added, no signature changed
    assert "ecamp_resample_boxes_rgb_u8" in protos
    assert [a[1] for a in protos["ecamp_resample_boxes_rgb_u8"][1]] == [a[1] for a in protos["ecamp_resample_boxes_u8"][1]]
    assert [a[0] for a in protos["ecamp_resample_boxes_rgb_u8"][1]] == [a[0] for a in protos["ecamp_resample_boxes_u8"][1]]
    assert "data_utils.py:20-34" in open(_lib.HEADER).read().split("ecamp_resample_boxes_rgb_u8(")[0].rsplit("/*", 1)[1]
    for lib in libs:
        assert hasattr(lib, "ecamp_resample_boxes_rgb_u8")


def test_colour_entry_point_refuses_bad_arguments_without_a_device(libs):
    one = ctypes.c_void_p(16)   # never dereferenced: the argument checks fail first
    for lib in libs:
        rc = lib.ecamp_resample_boxes_rgb_u8(one, one, None, 2, 16, 5, 64, 32, 0, one, 1 << 30, one, None)
        assert rc < 0 and b"resample_boxes_rgb_u8: null argument" in lib.ecamp_last_error()
        rc = lib.ecamp_resample_boxes_rgb_u8(one, one, one, 2, 513, 5, 64, 32, 0, one, 1 << 30, one, None)
        assert rc < 0 and b"out=513 (<= 512)" in lib.ecamp_last_error()
        rc = lib.ecamp_resample_boxes_rgb_u8(one, one, one, 2, 16, 5, 64, 32, 2, one, 1 << 30, one, None)
        assert rc < 0 and b"filter 2" in lib.ecamp_last_error()
        rc = lib.ecamp_resample_boxes_rgb_u8(one, one, one, 2, 16, 5, 64, 32, 0, one, 16, one, None)
        assert rc < 0 and b"too small" in lib.ecamp_last_error()


# ------------------------------------------------------------------------------- the one launch path of the three resample entry points
# name -> (the filters it takes, None: no filter argument; its workspace size function)
ENTRY_POINTS = {"ecamp_resample_crops_u8": ((None,), "ecamp_resample_crops_workspace_bytes"),
                "ecamp_resample_boxes_u8": ((0, 1), "ecamp_resample_boxes_workspace_bytes"),
                "ecamp_resample_boxes_rgb_u8": ((0, 1), "ecamp_resample_boxes_workspace_bytes")}
ONE = ctypes.c_void_p(16)   # never dereferenced: the argument checks fail first


def _refused(lib, name, filt, match, src=ONE, table=ONE, dst=ONE, B=2, out=16, kmax=5, rows=64, max_h=32, ws=ONE, ws_bytes=1 << 40, err=ONE):
    """One call that the argument checks must refuse, with the entry point's own name in front of a message that holds `match`."""
    rc = getattr(lib, name)(src, table, dst, B, out, kmax, rows, max_h, *(() if filt is None else (filt,)), ws, ws_bytes, err, None)
    msg = lib.ecamp_last_error()
    assert rc < 0 and msg.startswith(name[len("ecamp_"):].encode() + b": ") and match in msg, (name, filt, rc, msg)


@pytest.mark.parametrize("build", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_every_resample_entry_point_refuses_bad_arguments_under_its_own_name(libs, name, build):
    lib = libs[build]
    filters, size_fn = ENTRY_POINTS[name]
    for filt in filters:
        for null in ("src", "table", "dst", "ws", "err"):
            _refused(lib, name, filt, b"null argument", **{null: None})
        _refused(lib, name, filt, b"out=513 (<= 512)", out=513)
        low = 4 if filt in (None, 1) else 2                               # one below Pillow's tap count at scale 1: 5 bicubic, 3 bilinear
        _refused(lib, name, filt, b"kmax=%d " % low, kmax=low)
        _refused(lib, name, filt, b"LDS", out=512, kmax=81)               # 81 * 512 * 4 = 165888 > 160 KB
        _refused(lib, name, filt, b"max_h=65", rows=64, max_h=65)
        _refused(lib, name, filt, b"too small", ws_bytes=getattr(lib, size_fn)(2, 16, 5, 64) - 1)
        _refused(lib, name, filt, b"B=65536 (<= 65535)", B=65536)         # gridDim.y of the passes: crops included
    if filters != (None,):
        _refused(lib, name, 2, b"filter 2")


def _align256(v):
    return (v + 255) // 256 * 256


def test_workspace_sizes_are_the_layout_restated(libs):
    """bounds int2 [B][2][out] | coef int32 [B][2][out][kmax] | 256 spare | intermediate [rows][out], + RsTab [B] (48 B) for the boxes."""
    grid = [(B, out, kmax, rows) for B in (1, 3, 16) for out in (7, 16) for kmax in (5, 32) for rows in (16, 40)]
    terms = [(B * 2 * out * 8, B * 2 * out * kmax * 4, rows * out, B * 48) for B, out, kmax, rows in grid]
    for n in range(4):                                                    # every term both is and is not a multiple of 256 somewhere
        assert {t[n] % 256 == 0 for t in terms} == {True, False}, n
    for lib in libs:
        assert lib.ecamp_resample_crops_workspace_bytes(3, 16, 5, 40) == 3840 and lib.ecamp_resample_boxes_workspace_bytes(3, 16, 5, 40) == 4096
        for args, (bounds, coef, tmp, tab) in zip(grid, terms):
            crops = _align256(bounds) + _align256(coef) + 256 + _align256(tmp)
            assert lib.ecamp_resample_crops_workspace_bytes(*args) == crops, args
            assert lib.ecamp_resample_boxes_workspace_bytes(*args) == crops + _align256(tab), args
        for n in range(4):
            for bad in (0, -1):
                args = [3, 16, 5, 40]
                args[n] = bad
                assert lib.ecamp_resample_crops_workspace_bytes(*args) == 0 and lib.ecamp_resample_boxes_workspace_bytes(*args) == 0, args


def test_the_two_resampler_objects_share_one_base_and_choose_only_the_op_and_the_taps(monkeypatch):
    """hip_ops recorded instead of called, tensors on the host: which op each object calls with which tap count, and the grow-only workspace."""
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import finetune_datasets as fd
    from ecamp_amd.module import pretrain_datasets as pd
    calls, need = [], {"bytes": 1000}
    for name in ("resample_crops_u8", "resample_boxes_u8", "resample_boxes_rgb_u8"):
        def op(flat, table, out_t, out, kmax, tmp_rows, max_h, ws, err, name=name, **kw):
            calls.append((name, tuple(out_t.shape), out, kmax, tmp_rows, max_h, ws, err, kw))
        op.__name__ = name
        monkeypatch.setattr(ops, name, op)
    for name in ("resample_crops_workspace_bytes", "resample_boxes_workspace_bytes"):
        monkeypatch.setattr(ops, name, lambda B, out, kmax, rows, name=name: calls.append((name, B, out, kmax, rows)) or need["bytes"])
    assert issubclass(pd.DeviceAugmenter, pd.DeviceResampler) and issubclass(fd.DeviceBoxResampler, pd.DeviceResampler)
    assert "__call__" not in vars(pd.DeviceResampler) and pd.DeviceAugmenter.run is fd.DeviceBoxResampler.run

    crops = [(R.gray_image(h, w, seed=h), False) for h, w in ((70, 20), (9, 33), (16, 16))]
    cflat, t6 = pd.pack_crops(crops)
    aug = pd.DeviceAugmenter("cpu", 16)
    for meta in (pd.crops_meta(t6), None):                                # None: the augmenter alone reads the table itself
        del calls[:]
        got = aug(cflat, t6, meta)
        kmax = pd.DeviceAugmenter.taps(70, 16)
        assert kmax == 19 and got.shape == (3, 16, 16) and got.dtype == torch.uint8
        assert calls[0] == ("resample_crops_workspace_bytes", 3, 16, kmax, 95)
        assert calls[1][:6] == ("resample_crops_u8", (3, 16, 16), 16, kmax, 95, 70) and calls[1][6] is aug.ws and calls[1][7] is aug.err and calls[1][8] == {}
    assert pd.DeviceAugmenter("cpu").size == 448

    gray = [(R.gray_image(20, 30, seed=1), True, (16, 0, 16, 0)), (R.gray_image(40, 12, seed=2), False, (16, 0, 16, 0))]
    colour = gray + [(np.stack([R.gray_image(8, 8, seed=s) for s in (3, 4, 5)]), False, (16, 0, 16, 0))]
    box = fd.DeviceBoxResampler("cpu", 16)
    for items, meta4, want in ((gray, None, "resample_boxes_u8"), (colour, None, "resample_boxes_rgb_u8"), (gray, False, "resample_boxes_u8"),
                               (gray, True, "resample_boxes_rgb_u8")):
        flat, t10, meta = fd.pack_boxes(items)
        meta = meta if meta4 is None else tuple(meta[:3]) + (meta4,)
        del calls[:]
        got = box(flat, t10, meta)
        assert calls[0] == ("resample_boxes_workspace_bytes", len(items), 16, meta[0], meta[1])
        assert calls[1][:6] == (want, (len(items), 16, 16), 16, meta[0], meta[1], meta[2]) and calls[1][6] is box.ws and calls[1][7] is box.err
        assert calls[1][8] in ({}, {"filter": ops.BILINEAR}) and got.shape == (len(items), 16, 16)

    flat, t10, meta = fd.pack_boxes(gray)
    for obj, args in ((aug, (cflat, t6, pd.crops_meta(t6))), (box, (flat, t10, meta))):
        need["bytes"] = 1000
        obj(*args)
        first = obj.ws
        assert first.numel() == 1000 and first.dtype == torch.uint8
        need["bytes"] = 800
        obj(*args)
        assert obj.ws is first                                            # large enough: reused
        need["bytes"] = 2000
        obj(*args)
        assert obj.ws is not first and obj.ws.numel() == 2000             # too small: reallocated
