"""-m gpu: ecamp_pos_embed_grad (csrc/finetune.hip) against the float64 sums of tests/_posembed_ref.py, per element and to a DERIVED
bound -- an f32 sum in any fixed order errs by at most (additions per term) * 2^-24 * sum |terms| -- with preloaded outputs (the call
accumulates), guard bands around every buffer it writes, two calls for determinism, and the form without dcls / dbias.  Every case
prints its worst ratio to the bound."""
import pytest
import torch

import _posembed_ref as R
from conftest import h16

pytestmark = pytest.mark.gpu

PEG_GRID_CAP = 2048     # workgroups of the streaming launch; an item is 64 16-byte column vectors x one batch range
PEG_APPLY_CAP = 1024    # workgroups of either kind in the second launch; its dpos kind takes T * D / 4 / 256 items
# (B, T, D): no reduction at the smallest T and D; an odd batch and 3 column vectors; the tiny model; a batch cut into several ranges
# (five of 14 samples); and 1100 * 1024 / 8 / 64 = 2200 items (4400 in f32) above the streaming launch's cap, 1100 above the second
# launch's, with dx at 6.8 MB (13.5 MB in f32)
SHAPES = [(1, 2, 8), (5, 5, 24), (7, 197, 192), (70, 17, 192), (3, 1100, 1024)]
GUARD = 64              # floats on either side of a buffer: 256 bytes keep the payload's alignment
PATTERN = -1234.5


def _guarded(dev, payload):
    buf = torch.full((payload.numel() + 2 * GUARD,), PATTERN, dtype=torch.float32, device=dev)
    buf[GUARD:GUARD + payload.numel()] = payload.reshape(-1).to(dev)
    return buf


def _intact(buf):
    return bool(torch.all(buf[:GUARD] == PATTERN)) and bool(torch.all(buf[-GUARD:] == PATTERN))


def _call(dev, dx, pos0, cls0, bias0, with_vectors=True):
    """One call through the C ABI on freshly preloaded, guarded buffers -> (dpos, dcls, dbias payloads, guards intact?)."""
    from ecamp_amd import _lib
    from ecamp_amd import hip_ops as ops
    Bn, T, D = dx.shape
    dt = ops.code(dx.dtype)
    nws = int(_lib.load().ecamp_pos_embed_grad_workspace_bytes(Bn, T, D, dt))
    assert nws >= T * D * 4 and nws % 16 == 0
    gp, gc, gb = _guarded(dev, pos0), _guarded(dev, cls0), _guarded(dev, bias0)
    ws = _guarded(dev, torch.zeros(nws // 4))
    view = lambda g: g[GUARD:-GUARD]
    _lib.call("ecamp_pos_embed_grad", ops.ptr(dx), ops.ptr(view(gp)), ops.ptr(view(gc)) if with_vectors else None,
              ops.ptr(view(gb)) if with_vectors else None, Bn, T, D, ops.ptr(view(ws)), dt, ops.stream())
    torch.cuda.synchronize()
    return view(gp).clone().view(T, D), view(gc).clone(), view(gb).clone(), all(_intact(g) for g in (gp, gc, gb, ws))


def _check(dev, dtype, Bn, T, D):
    dx = R.representable((Bn, T, D), seed=Bn * 7 + T)
    assert torch.equal(dx.to(dtype).float(), dx), "the inputs are exact in the format under test"
    pos0, cls0, bias0 = R.representable((T, D), seed=1), R.representable((D,), seed=2), R.representable((D,), seed=3)
    pos0[pos0 == 0], cls0[cls0 == 0], bias0[bias0 == 0] = 0.5, 0.5, 0.5          # non-zero priors: accumulation itself is tested
    S, S0, Sb = R.stem_grads(dx)
    want = (pos0.double() + S, cls0.double() + S0, bias0.double() + Sb)
    bounds = R.stem_bounds(dx, pos0, cls0, bias0)
    dxd = dx.to(dtype).to(dev)
    a = _call(dev, dxd, pos0, cls0, bias0)
    assert a[3], "guard bands around dpos, dcls, dbias and ws must keep their pattern"
    ratios = [float(((got.double().cpu() - w).abs() / b).max()) for got, w, b in zip(a[:3], want, bounds)]
    print("[pos_embed] %s B=%d T=%d D=%d: worst |got - exact| / bound: dpos %.2e dcls %.2e dbias %.2e (bar 1)"
          % (str(dtype).split(".")[-1], Bn, T, D, *ratios))
    assert max(ratios) <= 1.0, ratios
    assert all(float((got.cpu() - p).abs().max()) > 0 for got, p in zip(a[:3], (pos0, cls0, bias0))), "every output moved"
    b = _call(dev, dxd, pos0, cls0, bias0)
    assert b[3] and all(torch.equal(u, v) for u, v in zip(a[:3], b[:3])), "two calls on equal inputs must give the same bits"
    c = _call(dev, dxd, pos0, cls0, bias0, with_vectors=False)
    assert c[3] and torch.equal(c[0], a[0]), "dcls = dbias = NULL: the same dpos bits"
    assert torch.equal(c[1].cpu(), cls0) and torch.equal(c[2].cpu(), bias0), "dcls = dbias = NULL: nothing else is written"


@pytest.mark.parametrize("Bn,T,D", SHAPES)
def test_pos_embed_grad_in_16_bits_within_the_derived_bound(dev, both_halves, Bn, T, D):
    if T > 197:
        assert T * D // 8 // 64 > PEG_GRID_CAP and T * D // 4 // 256 > PEG_APPLY_CAP and Bn * T * D * 2 < 64 << 20
    _check(dev, h16(), Bn, T, D)


@pytest.mark.parametrize("Bn,T,D", SHAPES + [(5, 5, 12)])
def test_pos_embed_grad_in_f32_within_the_derived_bound(dev, Bn, T, D):
    """(5, 5, 12): a D that only the f32 form takes (a multiple of 4, not of 8)."""
    if T > 197:
        assert T * D // 4 // 64 > PEG_GRID_CAP and T * D // 4 // 256 > PEG_APPLY_CAP and Bn * T * D * 4 < 64 << 20
    _check(dev, torch.float32, Bn, T, D)


def test_the_wrapper_accumulates_into_arena_style_views(dev):
    """hip_ops.pos_embed_grad as StemFn.backward calls it: [1, T, D] / [1, 1, D] parameter-shaped views of one flat f32 buffer, the
    workspace from the caching allocator; two calls add twice."""
    from ecamp_amd import hip_ops as ops
    Bn, T, D = 6, 5, 192
    dx = R.representable((Bn, T, D), seed=9)
    flat = torch.zeros(T * D + 64 + 2 * 192, device=dev)          # pos_embed | pad to 64 | cls_token | bias
    o = (T * D + 63) // 64 * 64
    dpos, dcls, dbias = flat[:T * D].view(1, T, D), flat[o:o + D].view(1, 1, D), flat[o + 192:o + 192 + D]
    for _ in range(2):
        ops.pos_embed_grad(dx.to(dev).to(torch.bfloat16), dpos.view(T, D), dcls.view(-1), dbias)
    S, S0, Sb = R.stem_grads(dx)
    zero = torch.zeros(D)
    bounds = R.stem_bounds(dx, torch.zeros(T, D), zero, zero)       # of one call; two calls: twice the terms through twice the additions
    for got, w, b in ((dpos.view(T, D), 2 * S, bounds[0]), (dcls.view(-1), 2 * S0, bounds[1]), (dbias, 2 * Sb, bounds[2])):
        assert bool(torch.all((got.double().cpu() - w).abs() <= 4 * b))
    with pytest.raises(AssertionError):
        ops.pos_embed_grad(dx.to(dev), dpos.view(T, D), dcls.view(-1), None)
