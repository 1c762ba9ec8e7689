"""-m gpu: the drivers' `--image_shard_resident` on ecamp_tiny (R = 224, batch 4) with the oracle's recipe weights, over a tiny task whose
shards are written here: the loaders with and without the flag yield the same uint8 batches and labels under one seed, a `--stage train`
run of either driver writes the same loss and score lines, a limit below the shard's size ends the run before the model is built, and a
table row that points outside the shard makes the loader raise at the end of its pass.  Every comparison is equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ft_colour_ref as C  # noqa: E402
import _ft_image_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [(300, 260), (240, 330), (180, 200), (224, 224), (410, 250), (203, 500), (260, 260), (150, 420)]
GRAY_AT = (2, 9)      # the colour task: one grayscale source in the train list, one in the val list -- mixed batches


def _write_task(root, colour):
    """The three list files, a pre-training checkpoint and one shard per list (`U8ShardWriter`; up- and down-scaling, padding at --ratio 1.1)."""
    from ecamp_amd.module.pretrain_datasets import U8ShardWriter
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    os.makedirs(os.path.join(root, "lists"))
    os.makedirs(os.path.join(root, "shards"))
    k = 0
    for name, n in (("train_list.txt", 8), ("val_list.txt", 4), ("test_list.txt", 4)):
        lines = []
        with U8ShardWriter(os.path.join(root, "shards", name + ".u8"), colour=colour) as w:
            for _ in range(n):
                h, wd = SIZES[k % len(SIZES)]
                if not colour:
                    w.add(R.gray_image(h, wd, 40 + k))
                elif k in GRAY_AT:
                    g = R.gray_image(h, wd, 40 + k)
                    w.add(np.stack([g, g, g], axis=-1))
                else:
                    w.add(np.ascontiguousarray(C.colour_image(h, wd, 40 + k).transpose(1, 2, 0)))
                lines.append("img/i%d.png %d %d %d" % (k, k % 2, (k // 2) % 2, (k + 1) % 2))
                k += 1
        open(os.path.join(root, "lists", name), "w").write("\n".join(lines) + "\n")
    torch.save({"model": recipe.recipe_state(orc.cfg_tiny(), seed=0)}, os.path.join(root, "pre.pth"))
    return root


@pytest.fixture(scope="module")
def gray_task(tmp_path_factory):
    return _write_task(str(tmp_path_factory.mktemp("ft_resident_gray")), False)


@pytest.fixture(scope="module")
def colour_task(tmp_path_factory):
    return _write_task(str(tmp_path_factory.mktemp("ft_resident_colour")), True)


def _argv(root, out, *extra):
    return ["--name", "t", "--model", "vit_tiny_patch16", "--task", "CheXpert", "--num_classes", "3", "--output_dir", out, "--img_size", "224",
            "--train_batch_size", "4", "--eval_batch_size", "4", "--learning_rate", "3e-2", "--warmup_steps", "1", "--num_workers", "0", "--print_freq", "1",
            "--ratio", "1.1", "--pretrained_path", os.path.join(root, "pre.pth"), "--list_dir", os.path.join(root, "lists"),
            "--image_shard_dir", os.path.join(root, "shards")] + list(extra)


def _loaders(task, out, split, workers):
    from ecamp_amd import main_linprobe
    parse = main_linprobe.get_args_parser().parse_args
    a = main_linprobe.check_args(parse(_argv(task, out, "--mode", "LinearProbe", "--num_workers", str(workers))))
    b = main_linprobe.check_args(parse(_argv(task, out, "--mode", "LinearProbe", "--num_workers", str(workers), "--image_shard_resident")))
    return main_linprobe.build_loader(a, split), main_linprobe.build_loader(b, split)


@pytest.mark.parametrize("workers", [0, 2])
@pytest.mark.parametrize("colour", [False, True], ids=["gray", "colour"])
def test_loaders_with_and_without_the_flag_yield_the_same_batches(dev, gray_task, colour_task, tmp_path, colour, workers):
    from ecamp_amd.module import finetune_datasets as fd
    task = colour_task if colour else gray_task
    for split, batches in (("train", 2), ("val", 1)):
        dl, rl = _loaders(task, str(tmp_path), split, workers)
        assert isinstance(rl, fd.DeviceImageLoader) and isinstance(rl.shard, fd.ResidentShard) and dl.shard is None and len(rl) == len(dl) == batches
        path = fd.shard_path(os.path.join(task, "shards"), split, "100")
        assert rl.shard.nbytes == os.path.getsize(path) == rl.shard.tensor.numel() and rl.shard.tensor.is_cuda and rl.dataset.shard is None
        assert np.array_equal(rl.shard.tensor.cpu().numpy(), np.fromfile(path, dtype=np.uint8))        # the upload is the file
        for seed in (123, 124):                                                                        # two passes: the end-of-pass check lets a clean one through
            torch.manual_seed(seed)
            want = list(dl)
            torch.manual_seed(seed)
            got = list(rl)
            assert len(want) == len(got) == batches
            for (xw, yw), (xg, yg) in zip(want, got):
                assert xg.dtype == torch.uint8 and xg.is_cuda and tuple(xg.shape) == (4, 224, 224)
                assert torch.equal(xg, xw) and torch.equal(yg, yw)
                assert int(xg.max()) > 0


def _scored(path):
    keep = ("Training (", "Valid Loss:", "Valid Auc:", "Test Loss:", "Test Accuracy:", "The average AUROC", "The AUROC of")
    return [ln for ln in open(path).read().splitlines() if ln.startswith(keep)]


@pytest.mark.parametrize("driver,mode", [("main_linprobe", "LinearProbe"), ("main_finetune", "Finetune")])
def test_a_train_run_with_the_flag_writes_the_loss_and_score_lines_of_the_run_without_it(dev, colour_task, tmp_path, driver, mode):
    import importlib
    mod = importlib.import_module("ecamp_amd." + driver)
    parse = mod.get_args_parser().parse_args
    res, lines = [], []
    for flag in ((), ("--image_shard_resident",)):
        out = str(tmp_path / ("run%d" % len(flag)))
        res.append(mod.main(parse(_argv(colour_task, out, "--mode", mode, "--stage", "train", "--num_steps", "2", *flag))))
        lines.append(_scored(os.path.join(out, "log.txt")))
        log = open(os.path.join(out, "log.txt")).read()
        assert log.count("resident on the device") == (3 if flag else 0)                               # one line per split: train, val, test
    assert lines[0] == lines[1] and len(lines[0]) >= 2 + 2 + 3 + 3, lines
    assert any(ln.startswith("Training (2 / 2 Steps)") for ln in lines[0])
    assert res[0]["loss"] == res[1]["loss"] and res[0]["accuracy"] == res[1]["accuracy"]
    np.testing.assert_array_equal(np.array(res[0]["aurocs"]), np.array(res[1]["aurocs"]))
    log = open(os.path.join(str(tmp_path / "run1"), "log.txt")).read()
    for name in ("train_list.txt.u8", "val_list.txt.u8", "test_list.txt.u8"):
        size = os.path.getsize(os.path.join(colour_task, "shards", name))
        assert any(name in ln and "%d bytes uploaded in" % size in ln for ln in log.splitlines()), name


def test_a_limit_below_the_shards_size_ends_the_run_before_the_model_is_built(dev, gray_task, tmp_path, monkeypatch):
    from ecamp_amd import main_linprobe

    def no_model(args):
        raise AssertionError("the model was built")

    monkeypatch.setattr(main_linprobe, "build_model", no_model)
    parse = main_linprobe.get_args_parser().parse_args
    size = os.path.getsize(os.path.join(gray_task, "shards", "train_list.txt.u8"))
    gb = (size - 1) / 1e9
    with pytest.raises(SystemExit) as e:
        main_linprobe.main(parse(_argv(gray_task, str(tmp_path), "--mode", "LinearProbe", "--stage", "train", "--num_steps", "1", "--image_shard_resident",
                                       "--image_shard_resident_max_gb", repr(gb))))
    msg = str(e.value)
    assert "train split" in msg and "train_list.txt.u8" in msg and "holds %d bytes" % size in msg and "bytes are free" in msg
    assert "--image_shard_resident_max_gb) is %d bytes" % int(gb * 1e9) in msg and "works without --image_shard_resident" in msg


def test_a_row_outside_the_shard_raises_at_the_end_of_the_pass(dev, gray_task, tmp_path):
    """The last image of the val shard claims one row more than it has: its whole-image box ends one image row (224 bytes) past the shard.  The shard's tensor is
    made a view of a larger allocation of the test's own first, so that even an unguarded read would stay inside it."""
    _, rl = _loaders(gray_task, str(tmp_path), "val", 0)
    n = rl.shard.nbytes
    alloc = torch.cat([rl.shard.tensor, torch.zeros((65536,), dtype=torch.uint8, device=dev)])
    rl.shard.tensor = alloc[:n]
    torch.manual_seed(5)
    clean = list(rl)                                                            # a clean pass ends without a word
    off, H, W = (int(v) for v in rl.dataset.index[3][:3])
    assert off + H * W == n and (H, W) == (224, 224)
    rl.dataset.index[3, 1] = H + 1
    it = iter(rl)
    x, y = next(it)                                                             # the batch itself is delivered: the refused sample is zeros
    assert bool((x[3] == 0).all()) and torch.equal(x[:3], clean[0][0][:3])
    with pytest.raises(RuntimeError, match=r"resample_shard_u8 on .*val_list\.txt\.u8: err_flag = 2: a table row pointed outside the resident shard"):
        next(it)
    rl.dataset.index[3, 1] = H
    again = list(rl)                                                            # the flag was cleared with the report
    assert torch.equal(again[0][0], clean[0][0])
