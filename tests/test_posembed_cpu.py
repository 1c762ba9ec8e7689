"""not gpu: the host side of a trained position table (`--train_pos_embed`) -- the driver's flag and first log line, the classifier's
argument and what it adds to `finetune_parameters()`, declaration / export / argument checks of ecamp_pos_embed_grad, and the float64
reference of its sums (tests/_posembed_ref.py) against torch autograd."""
import ctypes
import os

import pytest
import torch

import _posembed_ref as R

BASE = ["--name", "t", "--stage", "train", "--model", "vit_tiny_patch16", "--task", "ChestX-ray14", "--num_classes", "14", "--synthetic"]


# ---------------------------------------------------------------------------------------------------------------- driver
def test_the_flag_parses_passes_the_finetune_checks_and_defaults_to_off():
    from ecamp_amd import main_finetune
    parse = main_finetune.get_args_parser().parse_args
    assert parse(BASE).train_pos_embed is False and parse(BASE + ["--train_pos_embed"]).train_pos_embed is True
    a = main_finetune.check_args(parse(BASE + ["--train_pos_embed"]))
    assert a.train_pos_embed is True and a.mode == "Finetune" and a.compute_dtype == "bf16"


def test_the_probe_driver_refuses_the_flag_in_its_own_words_before_any_device_work(monkeypatch):
    from ecamp_amd import main_linprobe
    monkeypatch.setattr(main_linprobe, "build_model", lambda *a, **k: (_ for _ in ()).throw(AssertionError("refuse before a model is built")))
    parse = main_linprobe.get_args_parser().parse_args
    with pytest.raises(SystemExit) as e:
        main_linprobe.main(parse(BASE + ["--mode", "LinearProbe", "--train_pos_embed"]))
    assert e.value.code not in (0, None) and "--train_pos_embed" in str(e.value) and "LinearProbe" in str(e.value) and "frozen" in str(e.value)
    with pytest.raises(SystemExit) as e:
        main_linprobe.check_args(parse(BASE + ["--mode", "LinearProbe", "--drop_path_rate", "0.1"]))
    assert "--drop_path_rate" in str(e.value)
    main_linprobe.check_args(parse(BASE + ["--mode", "LinearProbe"]))       # without either flag the probe's checks pass


def test_build_model_passes_the_flag_on(monkeypatch):
    from ecamp_amd import main_finetune
    from ecamp_amd.module import classifier
    seen = []
    monkeypatch.setattr(classifier, "build_classifier", lambda *a, **k: seen.append(k) or "model")
    parse = main_finetune.get_args_parser().parse_args
    for extra, want in (([], False), (["--train_pos_embed"], True)):
        assert main_finetune.build_model(main_finetune.check_args(parse(BASE + extra))) == "model"
        assert seen[-1]["train_pos_embed"] is want and seen[-1]["train_encoder"] is True


def test_opening_line_says_what_still_deviates():
    from ecamp_amd import main_finetune as mf
    parse = mf.get_args_parser().parse_args
    assert mf.opening_line(parse(BASE)) == mf.DEVIATIONS
    assert "NOT applied" in mf.DEVIATIONS and "pos_embed is held fixed at the sin-cos table" in mf.DEVIATIONS
    on = mf.opening_line(parse(BASE + ["--train_pos_embed"]))
    assert "pos_embed" in on and "IS trained (as the reference does)" in on and "fixed" not in on and "NOT applied" in on
    both = mf.opening_line(parse(BASE + ["--train_pos_embed", "--drop_path_rate", "0.1"]))
    assert "pos_embed" in both and "IS trained" in both and "NOT applied" not in both and "fixed" not in both and "drop_path_rate=0.1" in both
    rate_only = mf.opening_line(parse(BASE + ["--drop_path_rate", "0.1"]))
    assert "IS applied" in rate_only and "fixed" in rate_only and "IS trained" not in rate_only


# ---------------------------------------------------------------------------------------------------------------- classifier
def test_classifier_argument_turns_the_gradient_on_and_names_the_table_among_the_trained():
    from ecamp_amd.module.classifier import ECAMPClassifier, build_classifier
    torch.manual_seed(0)
    with pytest.raises(ValueError, match="train_encoder"):
        build_classifier("vit_tiny_patch16", 3, True, img_size=32, train_pos_embed=True)
    probe = build_classifier("vit_tiny_patch16", 3, True, img_size=32)
    with pytest.raises(ValueError, match="train_encoder"):
        ECAMPClassifier(probe.encoder, 3, train_pos_embed=True)
    assert probe.encoder.pos_embed.requires_grad is False          # a refused construction changed nothing
    off = build_classifier("vit_tiny_patch16", 3, True, img_size=32, train_encoder=True)
    assert off.train_pos_embed is False and off.encoder.pos_embed.requires_grad is False
    assert "pos_embed" not in dict(off.finetune_parameters())
    on = build_classifier("vit_tiny_patch16", 3, True, img_size=32, train_encoder=True, train_pos_embed=True)
    named = dict(on.finetune_parameters())
    assert on.train_pos_embed is True and on.encoder.pos_embed.requires_grad is True and named["pos_embed"] is on.encoder.pos_embed
    assert sorted(named) == sorted(list(dict(off.finetune_parameters())) + ["pos_embed"])
    assert not any(k.startswith(("decoder", "bert", "mask_token")) for k in named) and on.encoder.decoder_pos_embed.requires_grad is False
    assert list(on.state_dict()) == list(off.state_dict())          # the same checkpoint layout either way


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_declares_the_entry_points_and_both_builds_export_and_check_them():
    from ecamp_amd import _lib
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        from ecamp_amd import build
        build.build(verbose=False, half="both")
    protos = _lib.parse_header()
    assert _lib.abi_version_of_header() == 5          # entry points were added, no signature changed
    assert protos["ecamp_pos_embed_grad"][0] is ctypes.c_int32 and protos["ecamp_pos_embed_grad_workspace_bytes"][0] is ctypes.c_int64
    assert [n for _, n in protos["ecamp_pos_embed_grad"][1]] == ["dx", "dpos", "dcls", "dbias", "B", "T", "D", "ws", "dtype", "stream"]
    assert [n for _, n in protos["ecamp_pos_embed_grad_workspace_bytes"][1]] == ["B", "T", "D", "dtype"]
    one, odd, null = ctypes.c_void_p(64), ctypes.c_void_p(72), None
    for fmt in ("bf16", "f16"):
        lib = _lib.load(fmt)
        err = lambda: lib.ecamp_last_error().decode()
        assert hasattr(lib, "ecamp_pos_embed_grad") and hasattr(lib, "ecamp_pos_embed_grad_workspace_bytes")
        # argument errors are reported without a device: nothing is launched
        pg = lambda dx=one, dpos=one, dcls=one, dbias=one, B=4, T=5, D=16, ws=one, dtype=1: lib.ecamp_pos_embed_grad(
            dx, dpos, dcls, dbias, B, T, D, ws, dtype, None)
        for kw in ({"dx": null}, {"dpos": null}, {"ws": null}):
            assert pg(**kw) < 0 and "null pointer" in err(), kw
        assert pg(dbias=null) < 0 and "given together" in err()
        assert pg(dcls=null) < 0 and "given together" in err()
        assert pg(B=0) < 0 and "B=0" in err()
        assert pg(T=1) < 0 and "T=1" in err()
        assert pg(D=12) < 0 and "D=12" in err() and "multiple of 8" in err()
        assert pg(D=10, dtype=0) < 0 and "D=10" in err() and "multiple of 4" in err()
        assert pg(D=0) < 0 and "D=0" in err()
        assert pg(dtype=7) < 0 and "dtype 7" in err()
        for kw in ({"dpos": odd}, {"dx": odd}, {"dcls": odd}, {"dbias": odd}, {"ws": odd}):
            assert pg(**kw) < 0 and "16-byte aligned" in err(), kw
        wsb = lib.ecamp_pos_embed_grad_workspace_bytes
        assert wsb(0, 5, 16, 1) == 0 and wsb(4, 1, 16, 1) == 0 and wsb(4, 5, 12, 1) == 0 and wsb(4, 5, 10, 0) == 0 and wsb(4, 5, 16, 7) == 0
        assert wsb(4, 5, 16, 1) >= 5 * 16 * 4 and wsb(4, 5, 12, 0) >= 5 * 12 * 4 and wsb(4, 5, 16, 1) % 16 == 0
        assert wsb(96, 197, 768, 1) >= 197 * 768 * 4 and wsb(96, 197, 768, 1) % (197 * 768 * 4) == 0     # whole [T, D] partial tables


# ---------------------------------------------------------------------------------------------------------------- the float64 reference
@pytest.mark.parametrize("Bn,T,D", [(1, 2, 8), (5, 5, 24), (3, 17, 16)])
def test_float64_reference_equals_autograd_through_the_token_assembly(Bn, T, D):
    g = torch.Generator().manual_seed(Bn * 100 + T)
    cls = torch.randn(1, 1, D, generator=g, dtype=torch.float64, requires_grad=True)
    pos = torch.randn(1, T, D, generator=g, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(D, generator=g, dtype=torch.float64, requires_grad=True)
    patches = torch.randn(Bn, T - 1, D, generator=g, dtype=torch.float64)
    x = torch.cat(((cls + pos[:, :1]).expand(Bn, -1, -1), patches + bias + pos[:, 1:]), dim=1)
    dx = R.representable((Bn, T, D), seed=7)
    x.backward(dx.double())
    dpos, dcls, dbias = R.stem_grads(dx)
    assert dpos.dtype == torch.float64 and dpos.shape == (T, D) and dcls.shape == (D,) and dbias.shape == (D,)
    tol = 1e-13 * float(dx.abs().sum())
    assert float((dpos - pos.grad[0]).abs().max()) <= tol and float((dcls - cls.grad.view(-1)).abs().max()) <= tol
    assert float((dbias - bias.grad).abs().max()) <= tol
    # the bounds' sums of |terms| dominate the sums themselves, and the inputs are exact in every format under test
    A, A0, Ab = R.stem_abs_sums(dx)
    assert torch.all(A >= dpos.abs()) and torch.all(A0 >= dcls.abs()) and torch.all(Ab >= dbias.abs())
    assert torch.equal(dx.to(torch.bfloat16).float(), dx) and torch.equal(dx.to(torch.float16).float(), dx)
    bp, bc, bb = R.stem_bounds(dx, torch.ones(T, D), torch.ones(D), torch.ones(D))
    assert torch.equal(bp, (Bn + 1) * R.U32 * (1 + A)) and torch.equal(bc, (Bn + 1) * R.U32 * (1 + A0)) and torch.equal(bb, (Bn + T) * R.U32 * (1 + Ab))
