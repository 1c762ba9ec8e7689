"""not gpu: the host side of the linear probe -- metrics (ecamp_amd.util.metrics), the learning-rate schedules, the list dataset and
its transforms, ECAMPClassifier's construction and checkpoint layouts, the declaration / export / argument checks of the four
classification kernels, and the driver's flags."""
import argparse
import ctypes
import math
import os

import numpy as np
import pytest
import torch


# ---------------------------------------------------------------------------------------------------------------- metrics
def _auroc_pairs(y, s):
    """The definition: (concordant + tied / 2) over positive x negative pairs."""
    pos, neg = s[y == 1], s[y == 0]
    d = pos[:, None] - neg[None, :]
    return ((d > 0).sum() + 0.5 * (d == 0).sum()) / float(len(pos) * len(neg))


@pytest.mark.parametrize("C", [1, 3, 14])
def test_auroc_equals_the_pairwise_definition_with_ties(C):
    from ecamp_amd.util import metrics
    rng = np.random.RandomState(C)
    N = 211
    y = (rng.rand(N, C) < 0.3).astype(np.int64)
    s = np.round(rng.rand(N, C) + 0.3 * y, 1)          # one decimal: many ties
    assert all(len(np.unique(s[:, i])) < N // 4 for i in range(C))
    got = metrics.auroc_per_class(s, y)
    assert len(got) == C
    for i in range(C):
        assert got[i] == pytest.approx(_auroc_pairs(y[:, i], s[:, i]), abs=1e-12)
    assert metrics.mean_auroc(got, log=None) == pytest.approx(np.mean(got), abs=1e-15)


def test_auroc_of_a_single_valued_class_is_nan_and_left_out_of_the_mean():
    from ecamp_amd.util import metrics
    y = np.array([[1, 0, 1], [0, 0, 1], [1, 0, 1], [0, 0, 1]])
    s = np.array([[0.9, 0.1, 0.3], [0.2, 0.4, 0.2], [0.8, 0.3, 0.9], [0.1, 0.2, 0.5]])
    a = metrics.auroc_per_class(s, y)
    assert a[0] == 1.0 and math.isnan(a[1]) and math.isnan(a[2])
    said = []
    assert metrics.mean_auroc(a, log=said.append) == 1.0
    assert len(said) == 1 and "1, 2" in said[0]
    assert math.isnan(metrics.mean_auroc([float("nan")], log=None))


def test_rank_ties_share_the_average_rank():
    from ecamp_amd.util import metrics
    assert metrics.rankdata_average(np.array([3.0, 1.0, 3.0, 2.0, 3.0])).tolist() == [4.0, 1.0, 4.0, 2.0, 4.0]


def test_accuracy_and_confusion_matrix_by_hand():
    from ecamp_amd.util import metrics
    labels = np.array([0, 0, 1, 2, 2, 2])
    preds = np.array([0, 1, 1, 2, 0, 2])
    assert metrics.simple_accuracy(preds, labels) == pytest.approx(4 / 6)
    assert metrics.confusion_matrix(labels, preds, 3).tolist() == [[1, 1, 0], [0, 1, 0], [1, 0, 2]]
    assert metrics.confusion_matrix(labels, preds).shape == (3, 3)
    # multilabel: elementwise agreement (train.py:74-77 on [N, C] arrays)
    assert metrics.simple_accuracy(np.array([[1, 0], [1, 1]]), np.array([[1, 1], [1, 1]])) == 0.75


# ---------------------------------------------------------------------------------------------------------------- schedules
def test_learning_rate_factors_equal_the_formulas():
    from ecamp_amd import engine_linprobe as e
    W, T = 10, 110
    mid = (W + T) // 2
    for step in (0, 1, W - 1):
        assert e.warmup_cosine_factor(step, W, T) == step / W
        assert e.warmup_linear_factor(step, W, T) == step / W
    assert e.warmup_cosine_factor(W, W, T) == 1.0 and e.warmup_linear_factor(W, W, T) == 1.0
    assert e.warmup_cosine_factor(mid, W, T) == pytest.approx(0.5 * (1 + math.cos(math.pi * (mid - W) / (T - W))), abs=1e-15)
    assert e.warmup_cosine_factor(mid, W, T) == pytest.approx(0.5, abs=1e-12)
    assert e.warmup_linear_factor(mid, W, T) == (T - mid) / (T - W) == 0.5
    assert e.warmup_cosine_factor(T, W, T) == pytest.approx(0.0, abs=1e-15) and e.warmup_linear_factor(T, W, T) == 0.0
    assert e.warmup_linear_factor(T + 5, W, T) == 0.0
    assert e.lr_factor("cosine", 3, W, T) == 0.3 and e.lr_factor("linear", 60, W, T) == 0.5
    with pytest.raises(ValueError):
        e.lr_factor("step", 0, W, T)
    # no warm-up: the first value is 1, not 0 / 0
    assert e.warmup_cosine_factor(0, 0, T) == 1.0 and e.warmup_linear_factor(0, 0, T) == 1.0


# ---------------------------------------------------------------------------------------------------------------- dataset
def _gradient_image(w=300, h=200):
    from PIL import Image
    yy, xx = np.mgrid[0:h, 0:w]
    rgb = np.stack([(xx * 255 // (w - 1)), (yy * 255 // (h - 1)), ((xx + yy) % 256)], -1).astype(np.uint8)
    return Image.fromarray(rgb, "RGB")


def _write_lists(tmp_path, rows):
    d = tmp_path / "lists"
    d.mkdir()
    for name, lines in rows.items():
        (d / name).write_text("\n".join(lines) + "\n")
    return str(d)


def test_list_parsing_and_data_volume(tmp_path):
    from ecamp_amd.module import finetune_datasets as fd
    img_dir = tmp_path / "images"
    (img_dir / "sub").mkdir(parents=True)
    _gradient_image(40, 30).save(str(img_dir / "sub" / "a.png"))
    _gradient_image(30, 40).save(str(img_dir / "b.png"))
    lists = _write_lists(tmp_path, {
        "train_list.txt": ["sub/a.png 1 0 1", "b.png 0 0 0", "b.png 0 1 1"],
        "train_list_10.txt": ["sub/a.png 1 0 1", "b.png 0 1 0 "],      # trailing blank, as the reference's RSNA lists have
        "train_list_1.txt": ["b.png 0 0 1", ""],
        "val_list.txt": ["sub/a.png 2"],
        "test_list.txt": ["b.png 0", "sub/a.png 1"],
    })
    assert fd.list_file("train", "1") == "train_list_1.txt" and fd.list_file("train", "10") == "train_list_10.txt"
    assert fd.list_file("train", "100") == "train_list.txt" and fd.list_file("val") == "val_list.txt" and fd.list_file("test") == "test_list.txt"
    with pytest.raises(ValueError):
        fd.list_file("train", "50")
    for vol, n in (("100", 3), ("10", 2), ("1", 1)):
        assert len(fd.ListDataset(str(img_dir), lists, "train", data_volume=vol)) == n
    ds = fd.ListDataset(str(img_dir), lists, "train", data_volume="10", transform=fd.eval_transform(16))
    assert ds.labels == [[1, 0, 1], [0, 1, 0]] and ds.paths[0] == os.path.join(str(img_dir), "sub/a.png")
    x, y = ds[0]
    assert x.shape == (3, 16, 16) and x.dtype == torch.float32 and y.dtype == torch.float32 and y.tolist() == [1.0, 0.0, 1.0]
    val = fd.ListDataset(str(img_dir), lists, "val", transform=fd.eval_transform(16))
    assert val[0][1].tolist() == [2.0] and len(fd.ListDataset(str(img_dir), lists, "test")) == 2   # a single class index
    with pytest.raises(FileNotFoundError):
        fd.ListDataset(str(img_dir), str(tmp_path), "val")


def _expected_tensor(img):
    g = np.asarray(img.convert("L"), dtype=np.float32) / 255.0
    return torch.from_numpy((g - 0.4722) / 0.3028)[None].expand(3, *g.shape)


def test_normalisation_constants_differ_from_pretraining_as_in_the_reference():
    from ecamp_amd.module import finetune_datasets as fd
    assert (fd.FT_MEAN, fd.FT_STD) == (0.4722, 0.3028)


@pytest.mark.parametrize("ratio,resized,box", [(1.0, (96, 64), (16, 0, 80, 64)), (0.875, (109, 73), (22, 4, 86, 68))])
def test_eval_transform_is_pils_resize_and_centre_crop(ratio, resized, box):
    from PIL import Image
    from ecamp_amd.module import finetune_datasets as fd
    img = _gradient_image(300, 200)
    got = fd.eval_transform(64, ratio)(img)
    want = _expected_tensor(img.resize(resized, Image.BILINEAR).crop(box))
    assert got.shape == (3, 64, 64) and torch.equal(got, want)
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    tall = fd.eval_transform(64, ratio)(_gradient_image(200, 300))       # the short side is the width
    assert tall.shape == (3, 64, 64)
    small = fd.center_crop(_gradient_image(10, 20), 16)                   # smaller than the crop: zero padding, as torchvision
    assert small.size == (16, 16) and small.getpixel((2, 8)) == (0, 0, 0) and small.getpixel((13, 8)) == (0, 0, 0)   # columns 3..12 hold the image
    assert small.getpixel((3, 0)) == _gradient_image(10, 20).getpixel((0, 2)) and small.getpixel((12, 15)) == _gradient_image(10, 20).getpixel((9, 17))


def test_train_transform_draws_crop_then_flip_from_the_torch_generator(monkeypatch):
    from PIL import Image
    from ecamp_amd.module import finetune_datasets as fd
    from ecamp_amd.module import pretrain_datasets as pd
    img = _gradient_image(300, 200)
    calls = []
    real_crop, real_flip = fd.random_resized_crop_params, fd.random_flip
    monkeypatch.setattr(fd, "random_resized_crop_params", lambda *a, **k: (calls.append(("crop", a, k)), real_crop(*a, **k))[1])
    monkeypatch.setattr(fd, "random_flip", lambda: (calls.append(("flip",)), real_flip())[1])
    assert real_crop is pd.random_resized_crop_params and real_flip is pd.random_flip
    flips = 0
    for seed in range(6):
        del calls[:]
        torch.manual_seed(seed)
        got = fd.train_transform(32)(img)
        after = torch.rand(1)
        assert [c[0] for c in calls] == ["crop", "flip"]
        assert calls[0][1] == (300, 200) and calls[0][2] == {"scale": (0.08, 1.0)}
        # the same draws by hand, in the same order, leave the generator where the transform left it
        torch.manual_seed(seed)
        i, j, h, w = pd.random_resized_crop_params(300, 200, scale=(0.08, 1.0))
        flip = pd.random_flip()
        assert torch.equal(torch.rand(1), after)
        ref = img.crop((j, i, j + w, i + h)).resize((32, 32), Image.BILINEAR)
        if flip:
            ref = ref.transpose(Image.FLIP_LEFT_RIGHT)
        flips += flip
        assert torch.equal(got, _expected_tensor(ref))
    assert 0 < flips < 6


def test_synthetic_dataset_labels_are_a_function_of_the_image():
    from ecamp_amd.module import finetune_datasets as fd
    ds = fd.SyntheticClassificationDataset(8, 32, 4, True, seed=3)
    x, y = ds[5]
    x2, y2 = ds[5]
    assert torch.equal(x, x2) and torch.equal(y, y2) and x.shape == (3, 32, 32) and y.shape == (4,)
    bands = x[0].reshape(4, 8, 32).mean(dim=(1, 2))
    assert torch.equal((bands > 0).float(), y)
    single = fd.SyntheticClassificationDataset(8, 32, 4, False, seed=3)
    x, y = single[2]
    assert y.shape == (1,) and int(x[0].reshape(4, 8, 32).mean(dim=(1, 2)).argmax()) == int(y[0])


# ---------------------------------------------------------------------------------------------------------------- classifier
FLAT = ("cls_token", "pos_embed", "patch_embed.proj.", "blocks.", "fc_norm.", "head.")


@pytest.fixture(scope="module")
def clf():
    from ecamp_amd.module.classifier import build_classifier
    torch.manual_seed(0)
    return build_classifier("vit_tiny_patch16", 3, True, img_size=224)


def test_classifier_construction_leaves_the_wrapped_model_alone(clf):
    from ecamp_amd.module import model_ecamp as me
    assert list(clf.encoder.state_dict().keys()) == list(me.ecamp_tiny().state_dict().keys())
    assert clf.fc_norm.eps == 1e-6 and torch.all(clf.fc_norm.weight == 1) and torch.all(clf.fc_norm.bias == 0)
    assert clf.head.weight.shape == (3, 192) and clf.head.weight.dtype == torch.float32 and torch.all(clf.head.bias == 0)
    assert 0 < clf.head.weight.abs().max() <= 2 * 2e-5 * 2 + 1e-12 and clf.head.weight.std() < 1e-4     # trunc_normal_(std=2e-5)
    own = [k for k in clf.state_dict() if not k.startswith("encoder.")]
    assert own == ["fc_norm.weight", "fc_norm.bias", "head.weight", "head.bias"]
    with pytest.raises(ValueError):
        type(clf)(clf.encoder, 65)
    with pytest.raises(ValueError):
        type(clf)(clf.encoder, 3, pool="max")


def test_reference_state_dict_is_the_flat_timm_layout(clf):
    sd = clf.reference_state_dict()
    assert all(k.startswith(FLAT) for k in sd) and not any(k.startswith(("bert_encoder", "decoder", "super_res", "norm.", "mask_token")) for k in sd)
    want = {"cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "fc_norm.weight", "fc_norm.bias", "head.weight", "head.bias"}
    for i in range(12):
        for n in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2"):
            want |= {"blocks.%d.%s.weight" % (i, n), "blocks.%d.%s.bias" % (i, n)}
    assert set(sd) == want
    assert all(v.dtype == torch.float32 and v.device.type == "cpu" for v in sd.values())
    assert sd["head.weight"].data_ptr() != clf.head.weight.data_ptr()     # copies, not views


def test_load_pretrained_takes_a_pretraining_checkpoint_and_its_own_flat_layout(tmp_path):
    from ecamp_amd.module import model_ecamp as me
    from ecamp_amd.module.classifier import build_classifier
    torch.manual_seed(1)
    src = me.ecamp_tiny()
    with torch.no_grad():
        src.blocks[3].mlp.fc1.weight.normal_()
        src.norm.weight.fill_(1.5)
    keys_before = list(src.state_dict().keys())
    path = str(tmp_path / "pretrain.pth")
    # what util/misc.save_model writes: the weights beside the optimizer state, the epoch, the scaler and the run's argparse.Namespace
    opt = torch.optim.AdamW(src.parameters(), lr=1e-3)
    torch.save({"model": src.state_dict(), "optimizer": opt.state_dict(), "epoch": 3, "scaler": {"scale": 65536.0},
                "args": argparse.Namespace(lr=1e-3, data_path="/data", compute_dtype="bf16")}, path)
    a = build_classifier("vit_tiny_patch16", 3, True)
    dec_before = a.encoder.decoder_embed.weight.clone()
    loaded = a.load_pretrained(path)
    assert torch.equal(a.encoder.blocks[3].mlp.fc1.weight, src.blocks[3].mlp.fc1.weight) and torch.equal(a.encoder.cls_token, src.cls_token)
    assert torch.equal(a.encoder.decoder_embed.weight, dec_before)          # not an encoder key: keeps its initialisation
    assert not any(k.startswith(("decoder", "bert", "super_res", "head", "fc_norm")) for k in loaded)
    assert list(a.encoder.state_dict().keys()) == keys_before
    a.load_pretrained({"model": src.state_dict()})                          # a state in memory as well
    # its own flat layout, through a file, into a fresh classifier
    with torch.no_grad():
        a.head.weight.normal_()
        a.head.bias.normal_()
        a.fc_norm.weight.normal_()
    flat = str(tmp_path / "x_bestauc_checkpoint.bin")
    torch.save(a.reference_state_dict(), flat)
    b = build_classifier("vit_tiny_patch16", 3, True)
    loaded = b.load_pretrained(flat)
    assert {"fc_norm.weight", "fc_norm.bias", "head.weight", "head.bias"} <= set(loaded)
    for k, v in a.reference_state_dict().items():
        assert torch.equal(b.reference_state_dict()[k], v), k
    with pytest.raises(ValueError):
        b.load_pretrained({"model": {"head.weight": torch.zeros(3, 192)}})


def test_load_pretrained_drops_a_head_of_another_shape(clf, capsys):
    from ecamp_amd.module.classifier import build_classifier
    sd = clf.reference_state_dict()
    sd["head.weight"], sd["head.bias"] = torch.ones(14, 192), torch.ones(14)
    sd["fc_norm.bias"] = torch.full((192,), 0.25)
    b = build_classifier("vit_tiny_patch16", 3, True)
    w0 = b.head.weight.clone()
    loaded = b.load_pretrained(sd)
    out = capsys.readouterr().out
    assert "Removing key head.weight" in out and "Removing key head.bias" in out
    assert torch.equal(b.head.weight, w0) and torch.all(b.head.bias == 0) and "head.weight" not in loaded
    assert torch.all(b.fc_norm.bias == 0.25)


# ---------------------------------------------------------------------------------------------------------------- ABI
SYMBOLS = ("ecamp_pool_norm", "ecamp_cls_head_fwd", "ecamp_cls_loss", "ecamp_cls_head_wgrad")


def test_header_declares_the_four_kernels_and_both_builds_export_and_check_them():
    from ecamp_amd import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        from ecamp_amd import build
        build.build(verbose=False, half="both")
    protos = _lib.parse_header()
    assert _lib.abi_version_of_header() == 5
    for s in SYMBOLS:
        assert s in protos and protos[s][0] is ctypes.c_int32, s
    assert [n for _, n in protos["ecamp_pool_norm"][1]] == ["x", "gamma", "beta", "pooled", "feat", "B", "T", "D", "t0", "t1", "eps", "ws", "dtype", "stream"]
    assert [n for _, n in protos["ecamp_cls_loss"][1]] == ["logits", "targets", "kind", "loss", "dlogits", "counts", "bad_label", "B", "C", "stream"]
    one, null = ctypes.c_void_p(64), None
    for fmt in ("bf16", "f16"):
        lib = _lib.load(fmt)
        err = lambda: lib.ecamp_last_error().decode()
        for s in SYMBOLS:
            assert hasattr(lib, s), (fmt, s)
        # argument errors are reported without a device: nothing is launched
        pn = lambda x=one, pooled=one, D=8, t0=1, t1=5, dtype=1: lib.ecamp_pool_norm(x, null, null, pooled, one, 2, 5, D, t0, t1, 1e-6, one, dtype, None)
        assert pn(x=null) < 0 and "null pointer" in err()
        assert pn(pooled=null) < 0 and "null pointer" in err()
        assert lib.ecamp_pool_norm(one, one, null, one, one, 2, 5, 8, 1, 5, 1e-6, one, 1, None) < 0 and "null pointer" in err()
        assert pn(D=6) < 0 and "multiple of 4" in err()
        assert pn(t0=5, t1=5) < 0 and "t0" in err()
        assert pn(t0=3, t1=2) < 0 and "t0" in err()
        assert pn(t1=6) < 0 and "t0" in err()
        assert pn(dtype=7) < 0 and "dtype" in err()
        assert lib.ecamp_pool_norm_workspace_bytes(2, 5, 8, 1, 5, 1) >= 2 * 8 * 4 and lib.ecamp_pool_norm_workspace_bytes(2, 5, 6, 1, 5, 1) == 0
        for name, call in (("cls_head_fwd", lambda C, D, p=one: lib.ecamp_cls_head_fwd(one, one, p, one, 4, C, D, None)),
                           ("cls_head_wgrad", lambda C, D, p=one: lib.ecamp_cls_head_wgrad(one, one, one, p, 4, C, D, None)),
                           ("cls_loss", lambda C, D, p=one: lib.ecamp_cls_loss(one, one, 1, one, one, one, p, 4, C, None))):
            assert call(0, 8) < 0 and "C=0" in err(), name
            assert call(65, 8) < 0 and "C=65" in err(), name
            assert call(3, 8, null) < 0 and "null pointer" in err(), name
            if name != "cls_loss":
                assert call(3, 10) < 0 and "multiple of 4" in err(), name
        assert lib.ecamp_cls_loss(one, one, 2, one, one, one, one, 4, 3, None) < 0 and "kind" in err()


# ---------------------------------------------------------------------------------------------------------------- driver
RUN_LP_FIRST = ["--name", "ecamp", "--stage", "train", "--model", "vit_base_patch16", "--task", "ChestX-ray14", "--num_classes", "14",
                "--pretrained_path", "ECAMP_ViT_Base_16.pth", "--dataset_path", "ChestX-ray14", "--output_dir", "output/ChestX-ray14/1/",
                "--data_volume", "1", "--num_steps", "3000", "--eval_batch_size", "1024", "--img_size", "224", "--learning_rate", "3e-2",
                "--warmup_steps", "50", "--fp16", "--fp16_opt_level", "O2", "--train_batch_size", "96"]


def _parse(argv):
    from ecamp_amd.main_linprobe import get_args_parser
    return get_args_parser().parse_args(argv)


def test_driver_parses_the_references_command_line():
    from ecamp_amd.main_linprobe import check_args
    a = _parse(RUN_LP_FIRST)
    assert (a.name, a.stage, a.model, a.task, a.num_classes, a.data_volume) == ("ecamp", "train", "vit_base_patch16", "ChestX-ray14", 14, "1")
    assert (a.num_steps, a.eval_batch_size, a.img_size, a.learning_rate, a.warmup_steps, a.train_batch_size) == (3000, 1024, 224, 3e-2, 50, 96)
    assert a.fp16 and a.fp16_opt_level == "O2" and a.decay_type == "cosine" and a.max_grad_norm == 1.0 and a.seed == 42 and a.ratio == 1
    assert a.mode == "Finetune" and a.local_rank == -1            # the reference's defaults
    a = check_args(_parse(RUN_LP_FIRST + ["--mode", "LinearProbe"]))
    assert a.compute_dtype == "fp16" and a.is_multilabel and a.list_dir == os.path.join("datasets", "ChestX-ray14") and a.pool == "avg"
    for task, multi in (("COVIDx", False), ("Aptos", False), ("RSNA", True), ("CheXpert", True), ("MURED", True)):
        b = check_args(_parse(["--name", "x", "--task", task, "--mode", "LinearProbe", "--synthetic", "--list_dir", "/lists"]))
        assert b.is_multilabel is multi and b.compute_dtype == "bf16" and b.list_dir == "/lists"


@pytest.mark.parametrize("extra,word", [(["--mode", "Finetune"], "--mode Finetune is not implemented"), ([], "--mode Finetune is not implemented"),
                                        (["--mode", "LinearProbe", "--local_rank", "0"], "data-parallel probing is not implemented")])
def test_driver_refuses_what_is_not_implemented_before_any_device_work(extra, word, monkeypatch):
    from ecamp_amd import main_linprobe

    def no_device(*a, **k):
        raise AssertionError("the flags must be refused before a model is built")

    monkeypatch.setattr(main_linprobe, "build_model", no_device)
    with pytest.raises(SystemExit) as e:
        main_linprobe.main(_parse(RUN_LP_FIRST + extra))
    assert e.value.code not in (0, None) and word in str(e.value)
