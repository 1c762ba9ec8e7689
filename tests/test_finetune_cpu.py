"""not gpu: the host side of encoder fine-tuning -- declaration / export / argument checks of the four kernels of csrc/finetune.hip, the
driver's flags (every command line of the reference's run_ft.sh), the float64 reference of the fused clip + SGD step
(tests/_finetune_ref.py) against torch, and the set of tensors `ECAMPClassifier.finetune_parameters()` names."""
import ctypes
import os

import pytest
import torch

import _finetune_ref as R

# ---------------------------------------------------------------------------------------------------------------- ABI
SYMBOLS = ("ecamp_cls_head_dgrad", "ecamp_pool_norm_bwd", "ecamp_sumsq_grouped", "ecamp_sgd_grouped")


def test_header_declares_the_four_kernels_and_both_builds_export_and_check_them():
    from ecamp_amd import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        from ecamp_amd import build
        build.build(verbose=False, half="both")
    protos = _lib.parse_header()
    assert _lib.abi_version_of_header() == 5          # entry points were added, no signature changed
    for s in SYMBOLS:
        assert s in protos and protos[s][0] is ctypes.c_int32, s
    assert protos["ecamp_pool_norm_bwd_workspace_bytes"][0] is ctypes.c_int64 and protos["ecamp_sumsq_grouped_slots"][0] is ctypes.c_int64
    assert [n for _, n in protos["ecamp_cls_head_dgrad"][1]] == ["dlogits", "W", "dfeat", "B", "C", "D", "stream"]
    assert [n for _, n in protos["ecamp_pool_norm_bwd"][1]] == ["dfeat", "pooled", "gamma", "dgamma", "dbeta", "dx", "B", "T", "D", "t0", "t1", "eps",
                                                                 "ws", "dtype", "stream"]
    assert [n for _, n in protos["ecamp_sumsq_grouped"][1]] == ["g", "block_group", "n", "partials", "npart_out", "stream"]
    assert [n for _, n in protos["ecamp_sgd_grouped"][1]] == ["p", "g", "buf", "p16", "block_group", "n", "ngroups", "lr_host", "wd_host", "momentum",
                                                               "max_norm", "partials", "npart", "grad_scale", "ctl", "norm_out", "stream"]
    one, null = ctypes.c_void_p(64), None
    hyper = (ctypes.c_float * 8)(*([0.1] * 8))
    for fmt in ("bf16", "f16"):
        lib = _lib.load(fmt)
        err = lambda: lib.ecamp_last_error().decode()
        for s in SYMBOLS + ("ecamp_pool_norm_bwd_workspace_bytes", "ecamp_sumsq_grouped_slots"):
            assert hasattr(lib, s), (fmt, s)
        # argument errors are reported without a device: nothing is launched
        dg = lambda C=3, D=8, a=one, w=one, o=one: lib.ecamp_cls_head_dgrad(a, w, o, 4, C, D, None)
        assert dg(C=65) < 0 and "C=65" in err()
        assert dg(C=0) < 0 and "C=0" in err()
        assert dg(D=10) < 0 and "D=10" in err() and "multiple of 4" in err()
        for kw in ({"a": null}, {"w": null}, {"o": null}):
            assert dg(**kw) < 0 and "null pointer" in err()
        pb = lambda dfeat=one, pooled=one, dgamma=one, dbeta=one, dx=one, D=8, t0=1, t1=5, ws=one, dtype=1: lib.ecamp_pool_norm_bwd(
            dfeat, pooled, null, dgamma, dbeta, dx, 2, 5, D, t0, t1, 1e-6, ws, dtype, None)
        for kw in ({"dfeat": null}, {"pooled": null}, {"dx": null}, {"ws": null}, {"dgamma": null}, {"dbeta": null}):
            assert pb(**kw) < 0 and "null pointer" in err(), kw
        assert pb(D=6) < 0 and "D=6" in err()
        assert pb(t0=5, t1=5) < 0 and "t0=5" in err() and "t1=5" in err()
        assert pb(t0=3, t1=2) < 0 and "t0=3" in err()
        assert pb(t1=6) < 0 and "t1=6" in err()
        assert pb(dtype=7) < 0 and "dtype 7" in err()
        assert lib.ecamp_pool_norm_bwd_workspace_bytes(2, 5, 8, 1, 5, 1) >= 2 * 8 * 4 + 2 * 2 * 8 * 4
        assert lib.ecamp_pool_norm_bwd_workspace_bytes(2, 5, 6, 1, 5, 1) == 0 and lib.ecamp_pool_norm_bwd_workspace_bytes(2, 5, 8, 5, 5, 1) == 0
        sq = lambda n=128, g=one, t=one, part=one: lib.ecamp_sumsq_grouped(g, t, n, part, null, None)
        assert sq(n=100) < 0 and "n=100" in err()
        assert sq(n=0) < 0 and "n=0" in err()
        for kw in ({"g": null}, {"t": null}, {"part": null}):
            assert sq(**kw) < 0 and "null pointer" in err()
        assert lib.ecamp_sumsq_grouped_slots(100) == 0 and lib.ecamp_sumsq_grouped_slots(64) == 1
        assert 1 <= lib.ecamp_sumsq_grouped_slots(64 * 40) <= 2048 and lib.ecamp_sumsq_grouped_slots(1 << 34) == 2048
        sg = lambda n=128, p=one, g=one, buf=one, t=one, ng=3, part=one, npart=1, max_norm=1.0: lib.ecamp_sgd_grouped(
            p, g, buf, null, t, n, ng, hyper, hyper, 0.9, max_norm, part, npart, 1.0, null, null, None)
        assert sg(n=100) < 0 and "n=100" in err()
        assert sg(ng=9) < 0 and "ngroups=9" in err()
        assert sg(ng=0) < 0 and "ngroups=0" in err()
        assert sg(npart=-1) < 0 and "npart=-1" in err()
        assert sg(part=null) < 0 and "null pointer" in err()
        assert sg(part=null, npart=0) < 0 and "max_norm=1" in err()      # a clip without the partials it needs
        for kw in ({"p": null}, {"g": null}, {"buf": null}, {"t": null}):
            assert sg(**kw) < 0 and "null pointer" in err()


# ---------------------------------------------------------------------------------------------------------------- driver
def _run_ft_command_lines():
    """Every command line of the reference's run_ft.sh, restated: (task, classes, data volume, steps, eval batch, lr, warm-up, batch)."""
    rows = [("ChestX-ray14", 14, "1", 3000, 512, "3e-2", 50, 96), ("ChestX-ray14", 14, "10", 3000, 1024, "2.4e-2", 50, 768),
            ("ChestX-ray14", 14, "100", 30000, 1024, "1e-2", 500, 768),
            ("CheXpert", 5, "1", 30000, 1024, "3e-3", 50, 768), ("CheXpert", 5, "10", 90000, 1024, "5e-3", 1500, 768),
            ("CheXpert", 5, "100", 90000, 1024, "4e-3", 1500, 768),
            ("RSNA", 1, "1", 2000, 1024, "3e-3", 50, 256), ("RSNA", 1, "10", 9000, 1024, "3e-3", 50, 768), ("RSNA", 1, "100", 90000, 1024, "3e-3", 150, 768),
            ("COVIDx", 3, "1", 30000, 512, "3e-2", 50, 256), ("COVIDx", 3, "10", 30000, 512, "1e-2", 50, 768), ("COVIDx", 3, "100", 30000, 512, "1e-2", 50, 768)]
    out = []
    for task, C, vol, steps, eb, lr, wu, tb in rows:
        out.append((["--name", "ecamp", "--stage", "train", "--model", "vit_base_patch16", "--task", task, "--num_classes", str(C),
                     "--pretrained_path", "ECAMP_ViT_Base_16.pth", "--dataset_path", task, "--output_dir", "output/%s/%s/" % (task, vol),
                     "--data_volume", vol, "--num_steps", str(steps), "--eval_batch_size", str(eb), "--img_size", "224", "--learning_rate", lr,
                     "--warmup_steps", str(wu), "--fp16", "--fp16_opt_level", "O2", "--train_batch_size", str(tb)],
                    (task, C, vol, steps, eb, float(lr), wu, tb)))
    return out


def test_every_command_line_of_run_ft_parses_with_finetune_as_the_mode():
    from ecamp_amd import main_finetune
    lines = _run_ft_command_lines()
    assert len(lines) == 12
    for argv, (task, C, vol, steps, eb, lr, wu, tb) in lines:
        a = main_finetune.get_args_parser().parse_args(argv)
        assert (a.task, a.num_classes, a.data_volume, a.num_steps, a.eval_batch_size, a.learning_rate, a.warmup_steps, a.train_batch_size) == \
            (task, C, vol, steps, eb, lr, wu, tb)
        assert a.mode == "Finetune" and a.fp16 and a.local_rank == -1 and a.gradient_accumulation_steps == 1 and a.max_grad_norm == 1.0
    # without --fp16 such a line passes the checks: bf16, the task's label kind, the default list directory
    argv = [x for x in lines[9][0] if x != "--fp16"]
    a = main_finetune.check_args(main_finetune.get_args_parser().parse_args(argv))
    assert a.mode == "Finetune" and a.compute_dtype == "bf16" and a.is_multilabel is False and a.list_dir == os.path.join("datasets", "COVIDx")
    a = main_finetune.check_args(main_finetune.get_args_parser().parse_args([x for x in lines[0][0] if x != "--fp16"] + ["--compute_dtype", "fp32"]))
    assert a.compute_dtype == "fp32" and a.is_multilabel is True


@pytest.mark.parametrize("extra,words", [(["--local_rank", "0"], ("--local_rank 0", "data-parallel")),
                                         (["--gradient_accumulation_steps", "2"], ("--gradient_accumulation_steps 2",)),
                                         (["--fp16"], ("--fp16", "--compute_dtype bf16")),
                                         (["--compute_dtype", "fp16"], ("--compute_dtype bf16",)),
                                         (["--mode", "Other"], ("--mode Other",))])
def test_driver_refuses_what_is_not_implemented_before_any_device_work(extra, words, monkeypatch):
    from ecamp_amd import main_finetune

    def no_device(*a, **k):
        raise AssertionError("the flags must be refused before a model is built")

    monkeypatch.setattr(main_finetune, "build_model", no_device)
    argv = [x for x in _run_ft_command_lines()[0][0] if x != "--fp16"] + extra
    with pytest.raises(SystemExit) as e:
        main_finetune.main(main_finetune.get_args_parser().parse_args(argv))
    assert e.value.code not in (0, None)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_linear_probe_mode_is_handed_to_the_probe_driver(monkeypatch):
    from ecamp_amd import main_finetune, main_linprobe
    seen = []
    monkeypatch.setattr(main_linprobe, "main", lambda args: seen.append(args) or "probe")
    monkeypatch.setattr(main_finetune, "build_model", lambda *a, **k: (_ for _ in ()).throw(AssertionError("not the fine-tuning path")))
    a = main_finetune.get_args_parser().parse_args(_run_ft_command_lines()[0][0] + ["--mode", "LinearProbe"])
    assert main_finetune.main(a) == "probe" and seen == [a] and a.mode == "LinearProbe"


def test_the_probe_driver_still_refuses_finetune_with_its_own_words():
    from ecamp_amd import main_linprobe
    with pytest.raises(SystemExit) as e:
        main_linprobe.check_args(main_linprobe.get_args_parser().parse_args(_run_ft_command_lines()[0][0]))
    assert "--mode Finetune is not implemented here" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- the float64 reference
@pytest.mark.parametrize("wds", [R.GROUP_WD, (0.0, 0.0, 0.0)], ids=["decay", "no-decay"])
def test_float64_reference_equals_clip_grad_norm_and_torch_sgd_over_five_steps(wds):
    n = 64 * 12
    table = R.block_table(n // 64, seed=3)
    p0, grads = R.trajectory(n, steps=5, seed=4)
    live = R.element_groups(table) < 8
    assert bool(live.any()) and not bool(live.all()) and set(table.tolist()) == {0, 1, 2, R.FROZEN}
    # a threshold between the norms of the second and third gradient: two steps clip, three do not
    norms = [float(torch.sqrt((g[live].double() ** 2).sum())) for g in grads]
    max_norm = (norms[1] * norms[2]) ** 0.5
    want_p, want_buf, want_norms, want_coefs = R.torch_clip_sgd(p0, grads, table, R.GROUP_LR, wds, R.MOMENTUM, max_norm, torch.float64)
    assert any(c < 1.0 for c in want_coefs) and any(c == 1.0 for c in want_coefs)       # a norm above max_norm, and one below
    p, buf = p0.double().clone(), torch.zeros(n, dtype=torch.float64)
    for s, g in enumerate(grads):
        norm, coef = R.clip_sgd_step(p, g, buf, table, R.GROUP_LR, wds, R.MOMENTUM, max_norm)
        assert norm == pytest.approx(want_norms[s], rel=1e-13) and coef == pytest.approx(want_coefs[s], rel=1e-13)
    assert float((p - want_p).abs().max()) <= 1e-13 and float((buf - want_buf).abs().max()) <= 1e-13
    assert torch.equal(p[~live], p0.double()[~live]) and torch.all(buf[~live] == 0)         # frozen blocks: untouched
    assert float((p[live] - p0.double()[live]).abs().max()) > 1e-3
    # max_norm <= 0: no clipping at all
    p2, buf2 = p0.double().clone(), torch.zeros(n, dtype=torch.float64)
    assert R.clip_sgd_step(p2, grads[0], buf2, table, R.GROUP_LR, wds, R.MOMENTUM, 0.0)[1] == 1.0
    # grad_scale folds into the gradient before the norm
    p3, buf3 = p0.double().clone(), torch.zeros(n, dtype=torch.float64)
    n3, c3 = R.clip_sgd_step(p3, grads[0] * 4, buf3, table, R.GROUP_LR, wds, R.MOMENTUM, max_norm, grad_scale=0.25)
    p4, buf4 = p0.double().clone(), torch.zeros(n, dtype=torch.float64)
    n4, c4 = R.clip_sgd_step(p4, grads[0], buf4, table, R.GROUP_LR, wds, R.MOMENTUM, max_norm)
    assert n3 == pytest.approx(n4, rel=1e-14) and float((p3 - p4).abs().max()) <= 1e-14


# ---------------------------------------------------------------------------------------------------------------- what is trained
def _expected_names(pool):
    want = ["cls_token", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    for i in range(12):
        for n in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2"):
            want += ["blocks.%d.%s.weight" % (i, n), "blocks.%d.%s.bias" % (i, n)]
    want += ["norm.weight", "norm.bias"] if pool == "cls" else ["fc_norm.weight", "fc_norm.bias"]
    return want + ["head.weight", "head.bias"]


@pytest.mark.parametrize("pool", ["avg", "cls"])
def test_finetune_parameters_names_exactly_the_trained_tensors(pool):
    from ecamp_amd.module.classifier import build_classifier
    torch.manual_seed(0)
    clf = build_classifier("vit_tiny_patch16", 3, True, img_size=224, pool=pool, train_encoder=True)
    named = clf.finetune_parameters()
    assert sorted(k for k, _ in named) == sorted(_expected_names(pool))
    assert len({id(p) for _, p in named}) == len(named) and all(p.requires_grad for _, p in named)
    enc = dict(clf.encoder.named_parameters())
    for k, p in named:
        own = {"fc_norm.weight": clf.fc_norm.weight, "fc_norm.bias": clf.fc_norm.bias, "head.weight": clf.head.weight, "head.bias": clf.head.bias}
        assert p is (own[k] if k in own else enc[k]), k
    assert clf.encoder.pos_embed.requires_grad is False and not any(k == "pos_embed" or k.startswith(("decoder", "bert", "super_res", "mask_token")) for k, _ in named)
    # the default stays the probe: same construction, same state dict, no tail buffer
    probe = build_classifier("vit_tiny_patch16", 3, True, img_size=224, pool=pool)
    assert probe.train_encoder is False and clf.train_encoder is True and list(probe.state_dict()) == list(clf.state_dict())
    with pytest.raises(RuntimeError):
        probe.tail()


def test_fused_sgd_refuses_what_it_cannot_update():
    from ecamp_amd.optim import FusedSGD
    w = torch.nn.Parameter(torch.zeros(4))
    opt = FusedSGD([w], lr=0.1, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0)
    assert opt.param_groups[0]["momentum"] == 0.9 and opt.param_groups[0]["nesterov"] is False and opt.max_grad_norm == 1.0
    with pytest.raises(RuntimeError, match="not in an ecamp_amd arena"):
        opt.step()
    with pytest.raises(ValueError):
        FusedSGD([{"params": [w], "momentum": 0.5}, {"params": [torch.nn.Parameter(torch.zeros(2))]}], lr=0.1)
    with pytest.raises(ValueError):
        FusedSGD([{"params": [w], "nesterov": True}], lr=0.1)
