"""-m gpu: colour sources through the drivers' `--image_shard_dir`, on ecamp_tiny (R = 224) with the oracle's recipe weights.  Over a task
of colour PNGs (and two grayscale ones among them) the loaders of `build_loader` with and without the flag yield the same uint8 items
under the same seed; eval logits, and the loss and the updated parameters of a training step, on the device item are BITWISE those on the
host item; `main_finetune --stage train` then `--stage test` over the colour shard writes the host path's test lines."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ft_colour_ref as C  # noqa: E402
import _ft_image_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

B, NC = 4, 3


def _build(dtype, dev, train_encoder=False):
    from ecamp_amd.module import model_ecamp as me
    from ecamp_amd.module.classifier import ECAMPClassifier
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    torch.manual_seed(0)
    enc = me.ecamp_tiny(compute_dtype=dtype)
    enc.load_state_dict(recipe.recipe_state(orc.cfg_tiny(), seed=0), strict=True)
    clf = ECAMPClassifier(enc, NC, multilabel=True, pool="avg", train_encoder=train_encoder)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():   # a classifier in mid-training: no identity norm, no vanishing head
        clf.fc_norm.weight.copy_(1 + 0.2 * torch.randn(192, generator=g))
        clf.fc_norm.bias.copy_(0.1 * torch.randn(192, generator=g))
        clf.head.weight.copy_(0.1 * torch.randn(NC, 192, generator=g))
        clf.head.bias.copy_(0.1 * torch.randn(NC, generator=g))
    return clf.to(dev)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


GRAY_AT = (2, 9)      # one grayscale file in the train list, one in the val list: mixed batches


def _write_task(root):
    """Colour PNGs of several sizes (up- and down-scaling, padding at --ratio 1.1) with two grayscale ones among them, the three list files,
    a pre-training checkpoint and the colour shards."""
    from PIL import Image
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    os.makedirs(os.path.join(root, "img"))
    os.makedirs(os.path.join(root, "lists"))
    sizes = [(300, 260), (240, 330), (180, 200), (224, 224), (410, 250), (203, 500), (260, 260), (150, 420)]
    k = 0
    for name, n in (("train_list.txt", 8), ("val_list.txt", 4), ("test_list.txt", 4)):
        lines = []
        for _ in range(n):
            h, w = sizes[k % len(sizes)]
            path = os.path.join(root, "img", "i%d.png" % k)
            if k in GRAY_AT:
                Image.fromarray(R.gray_image(h, w, 40 + k), "L").save(path)
            else:
                C.as_pil(C.colour_image(h, w, 40 + k)).save(path)
            lines.append("img/i%d.png %d %d %d" % (k, k % 2, (k // 2) % 2, (k + 1) % 2))
            k += 1
        open(os.path.join(root, "lists", name), "w").write("\n".join(lines) + "\n")
    torch.save({"model": recipe.recipe_state(orc.cfg_tiny(), seed=0)}, os.path.join(root, "pre.pth"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_image_shard.py"), "--list_dir", os.path.join(root, "lists"), "--dataset_path", root,
                        "--out_dir", os.path.join(root, "shards"), "--workers", "2", "--colour"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    assert "train_list.txt.u8 (8 images: 1 grayscale of one plane, 7 colour of three" in r.stdout


@pytest.fixture(scope="module")
def task(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("ft_colour_task"))
    _write_task(root)
    return root


def _argv(root, out, *extra):
    return ["--name", "t", "--model", "vit_tiny_patch16", "--task", "CheXpert", "--num_classes", "3", "--output_dir", out, "--img_size", "224",
            "--train_batch_size", "4", "--eval_batch_size", "4", "--learning_rate", "3e-2", "--warmup_steps", "1", "--num_workers", "0", "--print_freq", "1",
            "--ratio", "1.1", "--pretrained_path", os.path.join(root, "pre.pth"), "--dataset_path", root, "--list_dir", os.path.join(root, "lists")] + list(extra)


def _loaders(task, out, split):
    from ecamp_amd import main_linprobe
    parse = main_linprobe.get_args_parser().parse_args
    host_args = main_linprobe.check_args(parse(_argv(task, out, "--mode", "LinearProbe")))
    dev_args = main_linprobe.check_args(parse(_argv(task, out, "--mode", "LinearProbe", "--image_shard_dir", os.path.join(task, "shards"))))
    return main_linprobe.build_loader(host_args, split), main_linprobe.build_loader(dev_args, split)


@pytest.fixture(scope="module")
def batch(dev, task, tmp_path_factory):
    """The first training batch either way under one seed: (f32 [B, 3, R, R] of the host transforms, uint8 [B, R, R] of the device, labels)."""
    hl, dl = _loaders(task, str(tmp_path_factory.mktemp("ft_colour_batch")), "train")
    torch.manual_seed(77)
    xh, yh = next(iter(hl))
    torch.manual_seed(77)
    xd, yd = next(iter(dl))
    assert torch.equal(yh, yd.cpu())
    return xh, xd, yh


def test_loaders_with_and_without_the_flag_yield_the_same_items(dev, task, tmp_path):
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import finetune_datasets as fd
    lut = ops.image_lut(dev, fd.FT_MEAN, fd.FT_STD)
    for split, batches in (("train", 2), ("val", 1), ("test", 1)):
        hl, dl = _loaders(task, str(tmp_path), split)
        assert isinstance(dl, fd.DeviceImageLoader) and len(dl) == len(hl) == batches
        assert [dl.dataset.shard.planes(k) for k in range(len(dl.dataset))].count(3) >= 3
        torch.manual_seed(123)
        host = list(hl)
        torch.manual_seed(123)
        device = list(dl)
        assert len(host) == len(device) == batches
        for (xh, yh), (xd, yd) in zip(host, device):
            assert xd.dtype == torch.uint8 and xd.is_cuda and tuple(xd.shape) == (4, 224, 224) and tuple(xh.shape) == (4, 3, 224, 224)
            assert torch.equal(yh, yd.cpu())
            assert _bits(R.normalise(xd.cpu().numpy()), xh)                                   # the host arithmetic on the device's bytes
            assert _bits(lut[xd.long()][:, None].expand(4, 3, 224, 224).contiguous().cpu(), xh)   # and the table the stem reads


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_eval_logits_and_a_probe_step_on_the_device_item_are_bitwise_those_on_the_host_item(dev, batch, dtype):
    """Forward-only logits; then one engine_linprobe step (SGD with momentum on the head, clipped): the loss and the updated parameters."""
    from ecamp_amd import engine_linprobe as lp
    xh, xd, y = batch
    clf = _build(dtype, dev).eval()
    with torch.no_grad():
        assert _bits(clf(xd), clf(xh))
    args = argparse.Namespace(learning_rate=3e-2, weight_decay=1e-4, decay_type="cosine", warmup_steps=1, num_steps=3, max_grad_norm=1.0)
    out = []
    for x in (xh, xd):
        clf = _build(dtype, dev)
        opt = lp.make_optimizer(clf, args)
        before = [p.detach().clone() for p in lp.head_parameters(clf)]
        loss, _ = lp.train_step(clf, opt, x, y, 0, args)
        torch.cuda.synchronize()
        after = [p.detach().clone() for p in lp.head_parameters(clf)]
        assert all(not torch.equal(a, b) for a, b in zip(after, before))
        out.append((loss.clone(), after))
    assert _bits(out[0][0], out[1][0])
    assert all(_bits(a, b) for a, b in zip(out[0][1], out[1][1]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_fine_tune_step_on_the_device_item_gives_the_bits_of_the_step_on_the_host_item(dev, batch, dtype):
    """`train_encoder` training mode at drop-path 0: logits and loss bitwise (what `test_ft_image_model_gpu` holds the uint8 stem to)."""
    xh, xd, y = batch
    out = []
    for x in (xh, xd):
        clf = _build(dtype, dev, train_encoder=True)
        clf.train()
        logits = clf(x)
        loss = clf.loss(logits, y)
        loss.backward()
        clf.check_labels()
        torch.cuda.synchronize()
        out.append((logits.detach().clone(), loss.detach().clone()))
    assert _bits(out[0][0], out[1][0]) and _bits(out[0][1], out[1][1])


def test_train_then_test_over_a_colour_shard_writes_the_host_paths_test_lines(dev, task, tmp_path):
    from ecamp_amd import main_finetune
    out = str(tmp_path / "run")
    shards = os.path.join(task, "shards")
    parse = main_finetune.get_args_parser().parse_args
    res = main_finetune.main(parse(_argv(task, out, "--stage", "train", "--num_steps", "2", "--image_shard_dir", shards)))
    assert os.path.exists(os.path.join(out, "t_bestauc_checkpoint.bin"))
    log = open(os.path.join(out, "log.txt")).read()
    assert log.count("the image pipeline runs on the device") == 1 and "colour" in log and "Training (2 / 2 Steps)" in log
    n0 = len(log.splitlines())
    res_host = main_finetune.main(parse(_argv(task, out, "--stage", "test")))
    n1 = len(open(os.path.join(out, "log.txt")).read().splitlines())
    res_dev = main_finetune.main(parse(_argv(task, out, "--stage", "test", "--image_shard_dir", shards)))
    lines = open(os.path.join(out, "log.txt")).read().splitlines()

    def scored(seg):
        return [ln for ln in seg if ln.startswith(("Test Loss:", "Test Accuracy:", "The average AUROC", "The AUROC of"))]

    a, b = scored(lines[n0:n1]), scored(lines[n1:])
    assert len(a) == 3 + NC and a == b, (a, b)
    assert scored(lines[:n0]) == a                                                   # and the test pass that closed the training run
    assert res_host["loss"] == res_dev["loss"] == res["loss"] and res_host["accuracy"] == res_dev["accuracy"]
    np.testing.assert_array_equal(np.array(res_host["aurocs"]), np.array(res_dev["aurocs"]))
