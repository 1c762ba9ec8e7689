"""-m gpu: the classifier reading uint8 images, and the drivers' `--image_shard_dir`, on ecamp_tiny (R = 224) with the oracle's recipe weights:
features, logits and the loss of a training step on the device pipeline's uint8 item are BITWISE those on the host-normalised f32 item;
the loaders of `build_loader` with and without the flag yield the same labels and, after normalisation, the same images; `--stage test`
logs the same lines either way; a short `--stage train` run on the device pipeline completes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ft_image_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

B, C = 4, 3


def _build(dtype, dev, train_encoder=False, pool="avg", **kw):
    from ecamp_amd.module import model_ecamp as me
    from ecamp_amd.module.classifier import ECAMPClassifier
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    torch.manual_seed(0)
    enc = me.ecamp_tiny(compute_dtype=dtype, **kw)
    enc.load_state_dict(recipe.recipe_state(orc.cfg_tiny(), seed=0), strict=True)
    clf = ECAMPClassifier(enc, C, multilabel=True, pool=pool, train_encoder=train_encoder)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():   # a classifier in mid-training: no identity norm, no vanishing head
        clf.fc_norm.weight.copy_(1 + 0.2 * torch.randn(192, generator=g))
        clf.fc_norm.bias.copy_(0.1 * torch.randn(192, generator=g))
        clf.head.weight.copy_(0.1 * torch.randn(C, 192, generator=g))
        clf.head.bias.copy_(0.1 * torch.randn(C, generator=g))
    return clf.to(dev)


def _u8(n=B, seed=11):
    return torch.from_numpy(np.stack([R.gray_image(224, 224, seed + k) for k in range(n)]))


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_eval_features_and_logits_on_uint8_are_bitwise_those_on_the_host_item(dev, dtype):
    clf = _build(dtype, dev).eval()
    u8 = _u8()
    f32 = R.normalise(u8.numpy())                      # `_to_normalised_gray3`'s arithmetic: what the host loader hands over
    assert f32.shape == (B, 3, 224, 224)
    for pool in ("avg", "cls"):
        want = clf.forward_features(f32, pool=pool)
        assert _bits(clf.forward_features(u8, pool=pool), want)
        assert _bits(clf.forward_features(u8[:, None].to(dev), pool=pool), want)         # [B, 1, R, R], already on the device
    with torch.no_grad():
        assert _bits(clf(u8), clf(f32))
    with pytest.raises(ValueError, match="uint8 imgs must be"):
        clf.forward_features(u8[:, :200])
    with pytest.raises(ValueError, match="uint8 imgs must be"):
        clf.forward_features(u8[:, None].expand(B, 3, 224, 224))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_training_step_on_uint8_gives_the_bits_of_the_step_on_the_host_item(dev, dtype):
    """`train_encoder` training mode at drop-path 0: logits and loss bitwise; the patch embedding's weight gradient -- formed from `ctx.cols`,
    the same tensor either way -- agrees to the summation order of its reduction (1e-5 of its largest element)."""
    u8 = _u8(seed=31)
    f32 = R.normalise(u8.numpy())
    y = (torch.rand(B, C, generator=torch.Generator().manual_seed(2)) < 0.5).float()
    out = []
    for x in (f32, u8):
        clf = _build(dtype, dev, train_encoder=True)
        clf.train()
        logits = clf(x)
        loss = clf.loss(logits, y)
        loss.backward()
        clf.check_labels()
        torch.cuda.synchronize()
        assert logits.requires_grad
        out.append((logits.detach().clone(), loss.detach().clone(), clf.encoder.arena.grad(clf.encoder.patch_embed.proj.weight).detach().float().clone()))
    assert _bits(out[0][0], out[1][0]) and _bits(out[0][1], out[1][1])
    ga, gb = out
    assert float(ga[2].abs().max()) > 0
    assert float((ga[2] - gb[2]).abs().max()) <= 1e-5 * float(ga[2].abs().max())


# ---------------------------------------------------------------------------------------------------------------- loaders and drivers
def _write_task(root):
    """Grayscale PNGs of several sizes (up- and down-scaling, padding at --ratio 1.1), the three list files, a pre-training checkpoint and
    the shards."""
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
            Image.fromarray(R.gray_image(h, w, 40 + k), "L").save(os.path.join(root, "img", "i%d.png" % k))
            lines.append("img/i%d.png %d %d %d" % (k, k % 2, (k // 2) % 2, (k + 1) % 2))
            k += 1
        open(os.path.join(root, "lists", name), "w").write("\n".join(lines) + "\n")
    torch.save({"model": recipe.recipe_state(orc.cfg_tiny(), seed=0)}, os.path.join(root, "pre.pth"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_image_shard.py"), "--list_dir", os.path.join(root, "lists"), "--dataset_path", root,
                        "--out_dir", os.path.join(root, "shards"), "--workers", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]


@pytest.fixture(scope="module")
def task(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("ft_image_task"))
    _write_task(root)
    return root


def _argv(root, out, *extra):
    return ["--name", "t", "--model", "vit_tiny_patch16", "--task", "CheXpert", "--num_classes", "3", "--output_dir", out, "--img_size", "224",
            "--train_batch_size", "4", "--eval_batch_size", "4", "--learning_rate", "3e-2", "--warmup_steps", "1", "--num_workers", "0", "--print_freq", "1",
            "--ratio", "1.1", "--pretrained_path", os.path.join(root, "pre.pth"), "--dataset_path", root, "--list_dir", os.path.join(root, "lists")] + list(extra)


def test_loaders_with_and_without_the_flag_yield_the_same_items(dev, task, tmp_path):
    from ecamp_amd import hip_ops as ops
    from ecamp_amd import main_linprobe
    from ecamp_amd.module import finetune_datasets as fd
    parse = main_linprobe.get_args_parser().parse_args
    host_args = main_linprobe.check_args(parse(_argv(task, str(tmp_path), "--mode", "LinearProbe")))
    dev_args = main_linprobe.check_args(parse(_argv(task, str(tmp_path), "--mode", "LinearProbe", "--image_shard_dir", os.path.join(task, "shards"))))
    lut = ops.image_lut(dev, fd.FT_MEAN, fd.FT_STD)
    for split, batches in (("train", 2), ("val", 1), ("test", 1)):
        hl, dl = main_linprobe.build_loader(host_args, split), main_linprobe.build_loader(dev_args, split)
        assert isinstance(dl, fd.DeviceImageLoader) and len(dl) == len(hl) == batches
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


def test_train_stage_on_the_device_pipeline_and_identical_test_lines_either_way(dev, task, tmp_path):
    from ecamp_amd import main_finetune
    out = str(tmp_path / "run")
    shards = os.path.join(task, "shards")
    parse = main_finetune.get_args_parser().parse_args
    res = main_finetune.main(parse(_argv(task, out, "--stage", "train", "--num_steps", "2", "--image_shard_dir", shards)))
    assert os.path.exists(os.path.join(out, "t_bestauc_checkpoint.bin"))
    log = open(os.path.join(out, "log.txt")).read()
    assert log.count("the image pipeline runs on the device") == 1 and "Training (2 / 2 Steps)" in log and "Saved model checkpoint" in log
    n0 = len(log.splitlines())
    res_host = main_finetune.main(parse(_argv(task, out, "--stage", "test")))
    n1 = len(open(os.path.join(out, "log.txt")).read().splitlines())
    res_dev = main_finetune.main(parse(_argv(task, out, "--stage", "test", "--image_shard_dir", shards)))
    lines = open(os.path.join(out, "log.txt")).read().splitlines()

    def scored(seg):
        return [ln for ln in seg if ln.startswith(("Test Loss:", "Test Accuracy:", "The average AUROC", "The AUROC of"))]

    a, b = scored(lines[n0:n1]), scored(lines[n1:])
    assert len(a) == 3 + C and a == b, (a, b)
    assert scored(lines[:n0]) == a                                                   # and the test pass that closed the training run
    assert res_host["loss"] == res_dev["loss"] == res["loss"] and res_host["accuracy"] == res_dev["accuracy"]
    np.testing.assert_array_equal(np.array(res_host["aurocs"]), np.array(res_dev["aurocs"]))
    assert not any("image pipeline" in ln for ln in lines[n0:n1]) and any("image pipeline" in ln for ln in lines[n1:])
