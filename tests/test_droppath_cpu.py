"""not gpu: stochastic depth for encoder fine-tuning, everything that needs no device -- the float64 helper against the oracle's block,
the per-block rates, the flag and its refusals, the opening log line, and the new entry points' argument checks."""
import ctypes
import os

import _droppath_ref as ref
import pytest
import torch

from ecamp_amd import _lib

F32, H16 = 0, 1


# ---------------------------------------------------------------------------------------------------------------- the float64 helper
def _tiny_block():
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    cfg = orc.cfg_tiny()
    P = {k: v.double() for k, v in orc.load_state(orc.new_params(cfg), recipe.recipe_state(cfg, seed=0)).items()}
    x = torch.randn(3, 5, cfg.embed_dim, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    return P, cfg, x


def test_helper_with_every_sample_kept_is_the_oracles_block_exactly():
    from oracle import ecamp_oracle as orc
    P, cfg, x = _tiny_block()
    ones = torch.ones(3)
    want = orc.vit_block(P, "blocks.1", x, cfg.num_heads, cfg.ln_eps)
    got = ref.vit_block_droppath(P, "blocks.1", x, cfg.num_heads, cfg.ln_eps, ones, ones, 0.0)
    assert torch.equal(got, want)


def test_helper_with_hand_written_masks():
    """A sample dropped on both branches leaves the block as it entered; one dropped on the MLP branch only carries the attention
    branch scaled by 1 / (1 - p); samples do not see each other."""
    from oracle import ecamp_oracle as orc
    P, cfg, x = _tiny_block()
    p = 0.25
    ka, km = torch.tensor([1.0, 0.0, 1.0]), torch.tensor([1.0, 0.0, 0.0])
    got = ref.vit_block_droppath(P, "blocks.1", x, cfg.num_heads, cfg.ln_eps, ka, km, p)
    assert torch.equal(got[1], x[1])
    full = orc.vit_block(P, "blocks.1", x, cfg.num_heads, cfg.ln_eps)
    assert not torch.equal(got[0], full[0])          # kept, but scaled
    # sample 2: x + attention branch / (1 - p), no MLP branch -- the attention branch taken from a run with the MLP branch switched off
    only_attn = ref.vit_block_droppath(P, "blocks.1", x, cfg.num_heads, cfg.ln_eps, torch.ones(3), torch.zeros(3), 0.0)
    want2 = x[2] + (only_attn[2] - x[2]) / (1 - p)
    assert torch.allclose(got[2], want2, rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- per-block rates
@pytest.mark.parametrize("depth", [12, 24])
@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_rates_are_timms_linspace(depth, rate):
    from ecamp_amd.module.classifier import ECAMPClassifier
    import torch.nn as nn

    class Enc(nn.Module):
        def __init__(self):
            super().__init__()
            self.embed_dim, self.fp8_forward = 16, False
            self.blocks = nn.ModuleList(nn.Identity() for _ in range(depth))

    clf = ECAMPClassifier(Enc(), 3, drop_path_rate=rate)
    want = torch.linspace(0, rate, depth)
    assert isinstance(clf.drop_path_rates, list) and all(type(v) is float for v in clf.drop_path_rates)
    assert torch.equal(torch.tensor(clf.drop_path_rates, dtype=torch.float64), want.double())     # each value IS a float32
    assert clf.drop_path_rates[0] == 0.0 and clf.drop_path_rates[-1] == ref.f32(rate)
    assert ECAMPClassifier(Enc(), 3).drop_path_rates == [0.0] * depth


def test_rates_of_depth_one_and_refusals():
    from ecamp_amd.module.classifier import ECAMPClassifier, build_classifier
    import torch.nn as nn

    class Enc(nn.Module):
        def __init__(self, depth=1, fp8=False):
            super().__init__()
            self.embed_dim, self.fp8_forward = 16, fp8
            self.blocks = nn.ModuleList(nn.Identity() for _ in range(depth))

    assert ECAMPClassifier(Enc(), 3, drop_path_rate=0.3).drop_path_rates == [0.0]
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="drop_path_rate"):
            ECAMPClassifier(Enc(4), 3, drop_path_rate=bad)
        with pytest.raises(ValueError, match="drop_path_rate"):
            build_classifier("vit_tiny_patch16", 3, True, img_size=32, drop_path_rate=bad)
    with pytest.raises(ValueError, match="fp8_forward"):
        ECAMPClassifier(Enc(4, fp8=True), 3, drop_path_rate=0.1)
    assert ECAMPClassifier(Enc(4, fp8=True), 3).drop_path_rates == [0.0] * 4        # rate 0 beside fp8_forward stays legal
    clf = build_classifier("vit_tiny_patch16", 3, True, img_size=32, train_encoder=True, drop_path_rate=0.1)
    assert len(clf.drop_path_rates) == 12 and clf.drop_path_rate == 0.1


# ---------------------------------------------------------------------------------------------------------------- flag and log line
_COMMON = ["--name", "t", "--synthetic", "--num_classes", "3"]


def test_parser_default_and_the_probes_refusal(monkeypatch):
    from ecamp_amd import main_finetune, main_linprobe
    assert main_linprobe.get_args_parser().parse_args(_COMMON).drop_path_rate == 0.0
    assert main_finetune.get_args_parser().parse_args(_COMMON + ["--drop_path_rate", "0.1"]).drop_path_rate == 0.1
    assert "0.1" in main_linprobe.get_args_parser().format_help().split("--drop_path_rate")[-1][:400]
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was asked for before the refusal"))
    probe = main_linprobe.get_args_parser().parse_args(_COMMON + ["--mode", "LinearProbe", "--drop_path_rate", "0.1"])
    with pytest.raises(SystemExit, match="drop_path_rate"):
        main_linprobe.main(probe)
    with pytest.raises(SystemExit, match="drop_path_rate"):
        main_finetune.main(probe)                      # hands over to main_linprobe, which refuses
    main_linprobe.check_args(main_linprobe.get_args_parser().parse_args(_COMMON + ["--mode", "LinearProbe"]))   # rate 0: accepted
    for bad in ("1.0", "-0.2"):
        with pytest.raises(SystemExit, match="drop_path_rate"):
            main_finetune.main(main_finetune.get_args_parser().parse_args(_COMMON + ["--drop_path_rate", bad]))
    ok = main_finetune.check_args(main_finetune.get_args_parser().parse_args(_COMMON + ["--drop_path_rate", "0.1"]))
    assert ok.drop_path_rate == 0.1


def test_opening_line():
    from ecamp_amd import main_finetune
    parse = main_finetune.get_args_parser().parse_args
    at0 = main_finetune.opening_line(parse(_COMMON))
    assert at0 == main_finetune.DEVIATIONS == ("NOTE: stochastic depth (the reference's drop_path_rate=0.1) is NOT applied, and pos_embed is held fixed at "
                                                "the sin-cos table (the reference trains it)")
    at1 = main_finetune.opening_line(parse(_COMMON + ["--drop_path_rate", "0.1"]))
    assert "stochastic depth" in at1 and "IS applied" in at1 and "0.1" in at1 and "linearly" in at1 and "NOT applied" not in at1
    assert "pos_embed" in at1 and "fixed" in at1
    assert "0.25" in main_finetune.opening_line(parse(_COMMON + ["--drop_path_rate", "0.25"]))


# ---------------------------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def libs():
    if not all(os.path.exists(p) for p in _lib.LIB_PATHS.values()):
        from ecamp_amd import build
        build.build(verbose=False, half="both")
    return _lib.load("bf16"), _lib.load("f16")


def test_both_builds_declare_and_export_the_entry_points(libs):
    protos = _lib.parse_header()
    for name, nargs in (("ecamp_drop_path_fwd", 12), ("ecamp_drop_path_bwd", 10)):
        assert name in protos and len(protos[name][1]) == nargs
        for lib in libs:
            assert hasattr(lib, name)
    assert [a[1] for a in protos["ecamp_drop_path_fwd"][1]] == ["res", "y", "out", "B", "T", "D", "p", "seed", "offset", "res_dtype", "y_dtype", "stream"]
    assert "train.py:127" in open(_lib.HEADER).read()       # the reference call site, as every prototype cites one


def test_argument_errors_are_reported_without_a_device(libs):
    a, b, c = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)   # never dereferenced: a check fails first
    for lib in libs:
        err = lib.ecamp_last_error
        fwd, bwd = lib.ecamp_drop_path_fwd, lib.ecamp_drop_path_bwd
        assert fwd(None, b, c, 2, 3, 8, 0.1, 1, 2, H16, H16, None) < 0 and b"null pointer" in err()
        assert fwd(a, b, None, 2, 3, 8, 0.1, 1, 2, H16, H16, None) < 0 and b"null pointer" in err()
        assert bwd(a, None, 2, 3, 8, 0.1, 1, 2, H16, None) < 0 and b"null pointer" in err()
        assert fwd(a, b, c, 2, 3, 6, 0.1, 1, 2, H16, H16, None) < 0 and b"multiple of 4" in err()
        assert bwd(a, b, 2, 3, 6, 0.1, 1, 2, F32, None) < 0 and b"multiple of 4" in err()
        assert fwd(a, b, c, 0, 3, 8, 0.1, 1, 2, H16, H16, None) < 0 and b"positive" in err()
        assert bwd(a, b, 2, 0, 8, 0.1, 1, 2, H16, None) < 0 and b"positive" in err()
        assert fwd(a, b, c, 2, 3, 8, 1.0, 1, 2, H16, H16, None) < 0 and b"[0, 1)" in err()
        assert fwd(a, b, c, 2, 3, 8, -0.5, 1, 2, F32, F32, None) < 0 and b"[0, 1)" in err()
        assert bwd(a, b, 2, 3, 8, 1.0, 1, 2, H16, None) < 0 and b"[0, 1)" in err()
        assert fwd(a, b, c, 2, 3, 8, 0.1, 1, 2, H16, F32, None) < 0 and b"dtype pair" in err()       # a 16-bit residual with an f32 branch
        assert fwd(a, b, c, 2, 3, 8, 0.1, 1, 2, 2, H16, None) < 0 and b"dtype pair" in err()
        assert bwd(a, b, 2, 3, 8, 0.1, 1, 2, 7, None) < 0 and b"dtype" in err()
        assert fwd(a, b, b, 2, 3, 8, 0.1, 1, 2, F32, H16, None) < 0 and b"aliasing" in err()         # out is y, but in another format
        assert fwd(a, b, a, 2, 3, 8, 0.1, 1, 2, H16, H16, None) < 0 and b"aliasing" in err()         # out is res
        assert fwd(a, b, ctypes.c_void_p((2 << 20) + 16), 2, 3, 8, 0.1, 1, 2, H16, H16, None) < 0 and b"aliasing" in err()   # a partial overlap
        assert bwd(a, a, 2, 3, 8, 0.1, 1, 2, H16, None) < 0 and b"aliasing" in err()
        assert fwd(ctypes.c_void_p((1 << 20) + 8), b, c, 2, 3, 8, 0.1, 1, 2, H16, H16, None) < 0 and b"aligned" in err()
