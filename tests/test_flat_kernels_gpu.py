"""The bandwidth-bound helpers behind the one flat launch path (csrc/common.h: Vec, flat_grid, launch_typed, col_tile_sum).

Merged kernels (assemble_tokens / unshuffle_fwd: one template for the in-place / same-dtype entry and the f32-stream `_x32` entry), bit for
bit against plain torch: the f32 sum of a 16-bit value and an f32 table entry is one correctly rounded f32 addition in the kernel and in
torch alike, and the 16-bit store is one round-to-nearest-even, which is `.to(dtype)`.

Column reductions (colsum, seq_sum, the mask-token gradient of unshuffle_bwd: one shared LDS tail) against float64 sums, every element held
to the any-order f32 summation bound  |got - ref| <= M * 2^-24 * sum|x|  over the M rows that enter that column (Higham, Accuracy and
Stability of Numerical Algorithms, eq. 4.4 with u = 2^-24: (M - 1) u / (1 - (M - 1) u) <= M u for the M used here), plus one rounding of
the output where it is 16-bit.  The scales used (2, 0.5) are powers of two, so they add no rounding.  The inputs are drawn on the CPU from a
fixed seed, and a float32 torch sum of the same data is put to the same bound first: the bound is one the reference itself meets.

dtype refusal: the twelve flat entries and the two report-side embedding entries that used to run any dtype code other than 0 as 16-bit
now refuse an unknown code before any launch; ecamp_cast and ecamp_scale refuse through the same path.  An empty flat call is a no-op."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
U24 = 2.0 ** -24


def _half_ulp(dtype):
    """(relative, absolute) size of one round-to-nearest of the output format: its unit roundoff 2^-p (p = 8 significant bits in bfloat16,
    11 in half: half an ulp of a normal value), and half the spacing of its subnormals."""
    if dtype == torch.bfloat16:
        return 2.0 ** -8, 2.0 ** -134
    if dtype == torch.float16:
        return 2.0 ** -11, 2.0 ** -25
    return 0.0, 0.0


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------- merged kernels
def _perm_ids(B, L, g):
    """[B, L] int32: an independent permutation of 0 .. L-1 per sample."""
    return torch.stack([torch.randperm(L, generator=g) for _ in range(B)]).to(torch.int32)


# (B, Lk, D, L): the smallest shape with a non-monotone ids_keep, and 256 * 49 * 192 = 2 408 448 vectors, above the 8192 x 256 threads of the
# capped grid (a thread takes a second vector)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,Lk,D,L", [(2, 3, 8, 5), (256, 48, 768, 196)])
def test_assemble_tokens_bits(dev, dtype, B, Lk, D, L):
    from ecamp_amd import hip_ops as ops
    g = _gen(B + Lk + D)
    x = torch.randn(B, Lk + 1, D, generator=g).to(dtype).to(dev)
    cls = torch.randn(D, generator=g).to(dev)
    pos = torch.randn(L + 1, D, generator=g).to(dev)
    if B == 2:
        ids = torch.tensor([[3, 0, 2], [4, 1, 0]], dtype=torch.int32)
    else:
        ids = _perm_ids(B, L, g)[:, :Lk].contiguous()
        assert bool((ids[:, 1:] < ids[:, :-1]).any())
    ids = ids.to(dev)
    ref = torch.empty(B, Lk + 1, D, device=dev, dtype=torch.float32)
    ref[:, 0] = cls + pos[0]
    ref[:, 1:] = x[:, 1:].float() + pos[1 + ids.long()]
    if dtype != torch.float32:
        x32 = ops.assemble_tokens_x32(x, cls, pos, ids, B, Lk, D)
        torch.cuda.synchronize()
        assert _bits_equal(x32, ref), "f32-stream output != f32 sum"
    inplace = ops.assemble_tokens_(x.clone(), cls, pos, ids, B, Lk, D)
    torch.cuda.synchronize()
    assert _bits_equal(inplace, ref.to(dtype)), "in place != (x.float() + pos[...]).to(dtype)"
    if dtype != torch.float32:
        assert _bits_equal(inplace, x32.to(dtype)), "in place != f32-stream .to(dtype)"


# (B, L, Lk, D): one kept and three masked slots per sample; the decoder's shape at B = 192 (above the grid cap: 192 * 197 * 128 vectors)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,L,Lk,D", [(2, 4, 1, 8), (192, 196, 49, 512)])
def test_unshuffle_fwd_bits(dev, dtype, B, L, Lk, D):
    from ecamp_amd import hip_ops as ops
    g = _gen(B + L + Lk + D)
    y = torch.randn(B, Lk + 1, D, generator=g).to(dtype).to(dev)
    mtok = torch.randn(D, generator=g).to(dev)
    dpos = torch.randn(L + 1, D, generator=g).to(dev)
    ids = _perm_ids(B, L, g).to(dev)
    kept = ids < Lk
    assert bool(kept.any()) and bool((~kept).any())
    yf = y.float()
    src = torch.cat([yf[:, 1:], mtok.expand(B, L - Lk, D)], dim=1)                       # [B, L, D]: kept tokens, then mask tokens
    ref = torch.cat([yf[:, :1], torch.gather(src, 1, ids.long()[:, :, None].expand(B, L, D))], dim=1) + dpos   # the cls row, then slot j
    out = ops.unshuffle_fwd(y, ids, mtok, dpos, B, L, Lk, D)
    torch.cuda.synchronize()
    assert _bits_equal(out, ref.to(dtype)), "unshuffle_fwd != (gathered + dpos).to(dtype)"
    if dtype != torch.float32:
        out32 = ops.unshuffle_fwd_x32(y, ids, mtok, dpos, B, L, Lk, D)
        torch.cuda.synchronize()
        assert _bits_equal(out32, ref), "unshuffle_fwd_x32 != f32 sum"


# ---------------------------------------------------------------------------------------------------------------- column reductions
def _hold(name, got, ref64, absx64, rows, out_dtype=torch.float32):
    """every element: |got - ref| <= rows * 2^-24 * sum|x| (+ one rounding of a 16-bit output)"""
    bound = rows * U24 * absx64
    rel, sub = _half_ulp(out_dtype)
    if rel:
        bound = bound + rel * (ref64.abs() + bound) + sub
    err = (got.double().cpu() - ref64).abs()
    worst = float((err - bound).max())
    print("%s: max err %.3e, max bound %.3e, worst err - bound %.3e" % (name, float(err.max()), float(bound.max()), worst))
    assert bool((err <= bound).all()), (name, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("select", [False, True])
@pytest.mark.parametrize("M,N", [(1, 4), (9, 132), (1025, 132)])
def test_colsum_against_float64(dev, dtype, select, M, N):
    from ecamp_amd import hip_ops as ops
    x = torch.randn(M, N, generator=_gen(M * 1000 + N)).to(dtype)
    period, lo, hi = (3, 1, 3) if select else (0, 0, 0)
    rows = torch.arange(M)
    sel = (rows % period >= lo) & (rows % period < hi) if select else torch.ones(M, dtype=torch.bool)
    xs = x[sel]
    nsel = int(sel.sum())
    alpha = 2.0
    ref = alpha * xs.double().sum(0)
    absx = alpha * xs.double().abs().sum(0)
    _hold("cpu f32 sum", alpha * xs.float().sum(0), ref, absx, nsel)
    out = torch.zeros(N, device=dev)
    ops.colsum(x.to(dev), out, alpha=alpha, period=period, lo=lo, hi=hi)
    torch.cuda.synchronize()
    _hold("colsum %s %dx%d select=%s" % (dtype, M, N, select), out, ref, absx, nsel)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,s0,s1", [(1, 0, 1), (9, 0, 9), (9, 2, 9)])
@pytest.mark.parametrize("H", [4, 132])
def test_seq_sum_against_float64(dev, dtype, S, s0, s1, H):
    from ecamp_amd import hip_ops as ops
    B = 3
    x = torch.randn(B, S, H, generator=_gen(S * 100 + H + s0)).to(dtype)
    scale = 0.5
    xs = x[:, s0:s1]
    ref = scale * xs.double().sum(1)
    absx = scale * xs.double().abs().sum(1)
    _hold("cpu f32 sum", (scale * xs.float().sum(1)).to(dtype), ref, absx, s1 - s0, dtype)
    out = ops.seq_sum(x.to(dev), s0, s1, scale)
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == (B, H)
    _hold("seq_sum %s S=%d [%d, %d) H=%d" % (dtype, S, s0, s1, H), out, ref, absx, s1 - s0, dtype)


# Lk = L: no slot masked, L - 1: one per sample, 0: all of them.  The kernel ACCUMULATES into the gradient, so `out` starts from nonzero
# contents, which enter the bound as one more row of the sum.
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masked", ["none", "one", "all"])
@pytest.mark.parametrize("D", [4, 132])
def test_unshuffle_bwd_mask_token_grad_against_float64(dev, dtype, masked, D):
    from ecamp_amd import _lib, hip_ops as ops
    B, L = 2, 4
    Lk = {"none": L, "one": L - 1, "all": 0}[masked]
    g = _gen(D + Lk)
    dxd = torch.randn(B, L + 1, D, generator=g).to(dtype)
    ids_restore = _perm_ids(B, L, g)
    ids_keep = torch.argsort(ids_restore, dim=1)[:, :Lk].to(torch.int32)
    out0 = torch.randn(D, generator=g)
    is_masked = ids_restore >= Lk                                                       # [B, L]
    xs = dxd[:, 1:].double() * is_masked[:, :, None]                                      # the rows that enter, zeros elsewhere
    nrows = int(is_masked.sum())
    assert nrows == B * (L - Lk)
    ref = out0.double() + xs.sum((0, 1))
    absx = out0.double().abs() + xs.abs().sum((0, 1))
    _hold("cpu f32 sum", out0 + (dxd[:, 1:].float() * is_masked[:, :, None]).sum((0, 1)), ref, absx, nrows + 1)
    out = out0.clone().to(dev)
    keep_dev = torch.zeros(max(1, B * Lk), dtype=torch.int32, device=dev)   # (never a null pointer, even with nothing kept)
    keep_dev[:B * Lk] = ids_keep.reshape(-1).to(dev)
    dy = torch.empty(B, Lk + 1, D, device=dev, dtype=dtype)
    dxd_dev, restore_dev = dxd.to(dev), ids_restore.to(dev)   # (held until the kernel has run)
    _lib.call("ecamp_unshuffle_bwd", ops.ptr(dxd_dev), ops.ptr(restore_dev), ops.ptr(keep_dev), ops.ptr(dy), ops.ptr(out), B, L, Lk, D,
              ops.code(dtype), ops.stream())
    torch.cuda.synchronize()
    _hold("masktok_grad %s D=%d masked=%s" % (dtype, D, masked), out, ref, absx, nrows + 1)
    if masked == "none":
        assert _bits_equal(out.cpu(), out0)
    want_dy = torch.cat([dxd[:, :1], torch.gather(dxd[:, 1:], 1, ids_keep.long()[:, :, None].expand(B, Lk, D))], dim=1)
    assert _bits_equal(dy.cpu(), want_dy), "dy is a copy of the kept rows"


# ---------------------------------------------------------------------------------------------------------------- dtype refusal
PATTERN = 0x5A5A5A5A


def _refusal_cases(dev):
    """name -> (error prefix, argument list with DTYPE where the dtype code goes, output buffers).  Smallest legal shapes; EVERY buffer is
    allocated at its f32 size, so that no reading of the dtype code could leave it."""
    f = lambda *shape: torch.zeros(*shape, device=dev)                      # noqa: E731  an input
    o = lambda *shape: torch.zeros(*shape, device=dev).view(torch.int32).fill_(PATTERN).view(torch.float32)   # noqa: E731  an output
    i0 = lambda: torch.zeros(1, 1, dtype=torch.int32, device=dev)           # noqa: E731  ids_keep / ids_restore = [[0]]
    DT = "DTYPE"
    c = {}
    y = o(4); c["ecamp_add"] = ("ecamp_add", [f(4), f(4), y, 4, DT], [y])
    y = o(1, 1, 4); c["ecamp_bcast_add"] = ("ecamp_bcast_add", [f(1, 1, 4), f(1, 4), y, 1, 1, 4, DT], [y])
    y = o(1, 4); c["ecamp_seq_sum"] = ("ecamp_seq_sum", [f(1, 1, 4), y, 1, 1, 4, 0, 1, 1.0, DT], [y])
    y = o(1, 1, 4); c["ecamp_seq_bcast"] = ("ecamp_seq_bcast", [f(1, 4), y, 1, 1, 4, 0, 1, 1.0, 0, DT], [y])
    y = o(4); c["ecamp_colsum"] = ("ecamp_colsum", [f(1, 4), 4, 1, 4, 1.0, None, 0, 0, 0, y, DT], [y])
    y = o(4); c["ecamp_gelu_bwd"] = ("ecamp_gelu_bwd", [f(4), f(4), y, 4, DT], [y])
    y = o(2, 16); c["ecamp_im2col_gather"] = ("im2col_gather", [f(1, 1, 4, 4), i0(), y, 1, 1, 1, 4, 4, DT], [y])
    y = o(1, 2, 4); c["ecamp_assemble_tokens"] = ("assemble_tokens", [y, f(4), f(2, 4), i0(), 1, 1, 4, DT], [y])
    y = o(1, 2, 4); c["ecamp_unshuffle_fwd"] = ("unshuffle_fwd", [f(1, 2, 4), i0(), f(4), f(2, 4), y, 1, 1, 1, 4, DT], [y])
    y, m = o(1, 2, 4), o(4); c["ecamp_unshuffle_bwd"] = ("unshuffle_bwd", [f(1, 2, 4), i0(), i0(), y, m, 1, 1, 1, 4, DT], [y, m])
    y, s = o(1, 3, 4, 4), o(1)
    c["ecamp_unpatchify_mim"] = ("unpatchify_mim", [f(1, 2, 48), f(1, 3, 4, 4), f(1, 1), y, s, 1, 4, 4, DT], [y, s])
    y = o(2, 48); c["ecamp_img_loss_bwd"] = ("img_loss_bwd", [f(1, 3, 4, 4), f(1, 3, 4, 4), f(1, 1), f(1, 3, 4, 4), f(2), y, 1, 4, 4, DT], [y])
    # the report-side embedding (csrc/text.hip) ran an unknown code as 16-bit as well: B = S = 1, four columns, token 0 = the padding id
    l0 = lambda: torch.zeros(1, 1, dtype=torch.int64, device=dev)           # noqa: E731  ids / type_ids = [[0]]
    z, e, mu, rs = o(1, 4), o(1, 4), o(1), o(1)
    c["ecamp_bert_embed_fwd"] = ("bert_embed_fwd", [l0(), l0(), f(1, 4), f(1, 4), f(1, 4), f(4), f(4), z, e, mu, rs, 1, 1, 4, 1e-12, 0.0, 0, 0, DT],
                                 [z, e, mu, rs])
    gw, gp, gt, dg, db = o(1, 4), o(1, 4), o(1, 4), o(4), o(4)
    c["ecamp_bert_embed_bwd"] = ("bert_embed_bwd", [f(1, 4), f(1, 4), f(1), f(1), f(4), l0(), l0(), gw, gp, gt, dg, db, 1, 1, 4, 0, 0, 0, 0.0, 0, 0, DT],
                                 [gw, gp, gt, dg, db])
    return c


ENTRIES = ["ecamp_add", "ecamp_bcast_add", "ecamp_seq_sum", "ecamp_seq_bcast", "ecamp_colsum", "ecamp_gelu_bwd", "ecamp_im2col_gather",
           "ecamp_assemble_tokens", "ecamp_unshuffle_fwd", "ecamp_unshuffle_bwd", "ecamp_unpatchify_mim", "ecamp_img_loss_bwd", "ecamp_bert_embed_fwd", "ecamp_bert_embed_bwd"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_unknown_dtype_is_refused_before_any_launch(dev, both_halves, entry):
    from ecamp_amd import _lib, hip_ops as ops
    lib = _lib.load()
    prefix, args, outs = _refusal_cases(dev)[entry]
    for bad in (2, -1):
        cargs = [ops.ptr(a) if (a is None or torch.is_tensor(a)) else bad if a == "DTYPE" else a for a in args]
        rc = getattr(lib, entry)(*cargs, ops.stream())
        torch.cuda.synchronize()
        msg = lib.ecamp_last_error().decode()
        assert rc < 0, (entry, bad, rc)
        assert msg.startswith(prefix + ":") and ("dtype %d" % bad) in msg, (entry, bad, msg)
        for t in outs:
            assert bool((t.view(torch.int32) == PATTERN).all()), (entry, bad, "an output was written")
    # and the entry still serves the dtypes it knows at this shape
    cargs = [ops.ptr(a) if (a is None or torch.is_tensor(a)) else 0 if a == "DTYPE" else a for a in args]
    assert getattr(lib, entry)(*cargs, ops.stream()) == 0, lib.ecamp_last_error().decode()
    torch.cuda.synchronize()


def test_cast_and_scale_refuse_unknown_dtypes(dev, both_halves):
    """ecamp_cast reads two codes: either unknown one is refused (the destination's is looked at first), nothing is written."""
    from ecamp_amd import _lib, hip_ops as ops
    lib = _lib.load()
    src = torch.zeros(4, device=dev)
    dst = torch.zeros(4, device=dev).view(torch.int32).fill_(PATTERN).view(torch.float32)
    for sd, dd, named in ((2, 0, 2), (0, 2, 2), (1, -1, -1), (3, 5, 5)):
        rc = lib.ecamp_cast(ops.ptr(src), ops.ptr(dst), 4, sd, dd, ops.stream())
        msg = lib.ecamp_last_error().decode()
        assert rc < 0 and msg == "ecamp_cast: dtype %d" % named, (sd, dd, rc, msg)
    for bad in (2, -1):
        rc = lib.ecamp_scale(ops.ptr(src), ops.ptr(dst), 4, 2.0, None, bad, ops.stream())
        msg = lib.ecamp_last_error().decode()
        assert rc < 0 and msg == "ecamp_scale: dtype %d" % bad, (bad, rc, msg)
    torch.cuda.synchronize()
    assert bool((dst.view(torch.int32) == PATTERN).all())
    assert lib.ecamp_cast(ops.ptr(src), ops.ptr(dst), 4, 0, 0, ops.stream()) == 0
    torch.cuda.synchronize()
    assert bool((dst == 0).all())


def test_an_empty_flat_call_is_a_no_op(dev):
    """flat_grid never asks for zero workgroups: a call over no elements launches one idle workgroup and returns 0, writing nothing."""
    from ecamp_amd import _lib, hip_ops as ops
    lib = _lib.load()
    a = torch.zeros(4, device=dev)
    y = torch.zeros(4, device=dev).view(torch.int32).fill_(PATTERN).view(torch.float32)
    assert lib.ecamp_add(ops.ptr(a), ops.ptr(a), ops.ptr(y), 0, 0, ops.stream()) == 0, lib.ecamp_last_error().decode()
    assert lib.ecamp_gelu_bwd(ops.ptr(a), ops.ptr(a), ops.ptr(y), 0, 0, ops.stream()) == 0, lib.ecamp_last_error().decode()
    torch.cuda.synchronize()
    assert bool((y.view(torch.int32) == PATTERN).all())
