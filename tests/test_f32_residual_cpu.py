"""not gpu: the host side of ECAMP(f32_residual=True) -- the command-line flag, the constructor's validation, the carrier that takes the f32
stream across autograd edges, and the new entry points of both builds of the library."""
import pytest
import torch


def test_cli_flag_reaches_the_constructor():
    from ecamp_amd.main_pretrain import build_model, get_args_parser
    args = get_args_parser().parse_args(["--model", "ecamp_tiny", "--amp", "fp16", "--f32_residual"])
    model = build_model(args)
    assert model.f32_residual is True and model.compute_dtype == torch.float16 and args.loss_scale == "dynamic"
    args = get_args_parser().parse_args(["--model", "ecamp_tiny"])
    assert args.f32_residual is False
    model = build_model(args)
    assert model.f32_residual is False and model.compute_dtype == torch.bfloat16


def test_constructor_validation():
    from ecamp_amd.module import model_ecamp as me
    with pytest.raises(ValueError, match="f32_residual"):
        me.ecamp_tiny(compute_dtype=torch.bfloat16, fp8_forward=True, f32_residual=True)
    # the f32 parity mode accepts the flag; its stream is f32 already, so nothing changes
    assert me.ecamp_tiny(compute_dtype=torch.float32, f32_residual=True).f32_residual is False
    assert me.ecamp_tiny(compute_dtype=torch.bfloat16, f32_residual=True).f32_residual is True
    assert me.ecamp_tiny(compute_dtype=torch.bfloat16).f32_residual is False


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_f32_carrier_round_trip_and_16_bit_gradients(dtype):
    """The carrier is a 16-bit [M, D] view over the f32 rows: f32_stream recovers them exactly, and autograd hands the stage before it a
    16-bit gradient (an f32 edge would make autograd insert a cast of every gradient)."""
    from ecamp_amd.functions import f32_carrier, f32_stream
    x = 2048.0 + torch.randn(6, 8)
    c = f32_carrier(x, dtype)
    assert c.dtype == dtype and c.shape == x.shape
    y = f32_stream(c)
    assert y.dtype == torch.float32 and y.data_ptr() == x.data_ptr() and torch.equal(y, x)
    assert f32_stream(x) is x
    seen = []

    class Produce(torch.autograd.Function):
        @staticmethod
        def forward(ctx, w):
            return f32_carrier(x + w, dtype)

        @staticmethod
        def backward(ctx, g):
            seen.append(g.dtype)
            return g.float().sum()

    class Consume(torch.autograd.Function):
        @staticmethod
        def forward(ctx, c):
            return f32_stream(c).sum()

        @staticmethod
        def backward(ctx, g):
            return torch.ones(6, 8, dtype=dtype) * g.to(dtype)

    w = torch.zeros((), requires_grad=True)
    Consume.apply(Produce.apply(w)).backward()
    assert seen == [dtype] and w.grad.item() == 48.0


def test_new_entry_points_exported_by_both_builds():
    from ecamp_amd import _lib
    if not all(__import__("os").path.exists(p) for p in _lib.LIB_PATHS.values()):
        from ecamp_amd import build
        build.build(verbose=False, half="both")
    protos = _lib.parse_header()
    new = ["ecamp_gemm_res32", "ecamp_layernorm_fwd_x32", "ecamp_layernorm_bwd_z32", "ecamp_assemble_tokens_x32", "ecamp_unshuffle_fwd_x32"]
    for fmt in ("bf16", "f16"):
        lib = _lib.load(fmt)
        assert lib.ecamp_abi_version() == _lib.abi_version_of_header() == 5
        for name in new:
            assert name in protos and hasattr(lib, name), (fmt, name)
