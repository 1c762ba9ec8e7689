"""-m gpu: `ecamp_compact_rows` (csrc/text.hip), the gather of the scored rows in front of the evaluation head, against plain torch
indexing on the host -- bitwise, this is data movement.  f32 and the 16-bit format of both builds; row counts around the 256-row
segment, a count that spans more than one 1024-segment super-segment, every scored pattern with and without `ids`, a capacity below
the count with canary rows behind every output, and argument errors that launch nothing."""
import ctypes

import pytest
import torch

from conftest import h16

pytestmark = pytest.mark.gpu

V = 1000
MASK = 3
CANARY = 5          # rows allocated behind each output; the call must leave them alone
PATTERNS = ("none", "all", "first", "last", "p15", "p50")


def _case(M, cols, dtype, pattern, with_ids, seed, ldx=None):
    """Host tensors of one case -> (x [M, cols] (a view with row stride ldx), labels, weights, ids or None, scored bool[M])."""
    g = torch.Generator().manual_seed(seed)
    ldx = cols if ldx is None else ldx
    x = torch.randn(M, ldx, generator=g).to(dtype)[:, :cols]
    if pattern == "none":
        scored = torch.zeros(M, dtype=torch.bool)
    elif pattern == "all":
        scored = torch.ones(M, dtype=torch.bool)
    elif pattern in ("first", "last"):
        scored = torch.zeros(M, dtype=torch.bool)
        scored[0 if pattern == "first" else M - 1] = True
    else:
        scored = torch.rand(M, generator=g) < (0.15 if pattern == "p15" else 0.5)
    valid = torch.randint(0, V, (M,), generator=g)
    valid[::7] = V - 1
    valid[1::7] = 0                                                      # both ends of [0, V) are labels
    invalid = torch.tensor([-100, -1, V, V + 5, -2 ** 40])[torch.randint(0, 5, (M,), generator=g)]
    weights = torch.rand(M, generator=g) * 2 + 0.01
    if not with_ids:
        return x, torch.where(scored, valid, invalid), weights, None, scored
    # unscored rows are a mix of: [MASK] under an invalid label, a valid label under another token, neither
    how = torch.randint(0, 3, (M,), generator=g)
    labels = torch.where(scored | (how == 1), valid, invalid)
    other = torch.randint(4, V, (M,), generator=g)
    ids = torch.where(scored | (how == 0), torch.full((M,), MASK), other)
    return x, labels, weights, ids, scored


def _reference(x, labels, weights, ids, cap):
    """Plain torch indexing -> (x_c, labels_c, weights_c, rows, count): the first `cap` scored rows in order, padding behind them."""
    scored = (labels >= 0) & (labels < V)
    if ids is not None:
        scored &= ids == MASK
    idx = scored.nonzero()[:, 0]
    k = min(idx.numel(), cap)
    x_c = torch.zeros(cap, x.shape[1], dtype=x.dtype)
    labels_c = torch.full((cap,), -100, dtype=torch.int64)
    weights_c = torch.zeros(cap)
    rows = torch.full((cap,), -1, dtype=torch.int32)
    x_c[:k], labels_c[:k], weights_c[:k], rows[:k] = x[idx[:k]], labels[idx[:k]], weights[idx[:k]], idx[:k].to(torch.int32)
    return x_c, labels_c, weights_c, rows, idx.numel()


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _run_and_check(dev, x, labels, weights, ids, scored, cap):
    """The C entry point on buffers of its own with CANARY rows behind each output: everything against `_reference`, bit for bit."""
    from ecamp_amd import _lib, hip_ops
    M, cols = x.shape
    xd = torch.empty(M, x.stride(0), dtype=x.dtype, device=dev)[:, :cols]
    xd.copy_(x)
    ld, wd = labels.to(dev), weights.to(dev)
    idd = ids.to(dev) if ids is not None else None
    g = torch.Generator().manual_seed(99)
    outs = [torch.randn(cap + CANARY, cols, generator=g).to(x.dtype), torch.randint(-9, 9, (cap + CANARY,), generator=g),
            torch.randn(cap + CANARY, generator=g), torch.randint(-9, 9, (cap + CANARY,), generator=g).to(torch.int32),
            torch.full((1 + CANARY,), -77, dtype=torch.int64)]
    od = [o.to(dev) for o in outs]
    nws = _lib.load().ecamp_compact_rows_workspace_bytes(M)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    p = hip_ops.ptr
    _lib.call("ecamp_compact_rows", p(xd), xd.stride(0), p(ld), p(wd), p(idd), MASK, M, cols, V, cap, p(od[0]), p(od[1]), p(od[2]), p(od[3]),
              p(od[4]), p(ws), hip_ops.code(x.dtype), hip_ops.stream())
    torch.cuda.synchronize()
    got = [o.cpu() for o in od]
    want = _reference(x, labels, weights, ids, cap)
    assert want[4] == int(scored.sum())
    assert int(got[4][0]) == want[4], "count_out"
    k = min(want[4], cap)
    assert torch.equal(got[3][:cap], want[3]), "rows_out: order / padding"
    assert torch.equal(got[1][:cap], want[1]), "labels_out"
    assert torch.equal(_bits(got[2][:cap]), _bits(want[2])), "weights_out"
    assert torch.equal(_bits(got[0][:cap]), _bits(want[0])), "x_out"
    assert (got[3][k:cap] == -1).all() and (got[1][k:cap] == -100).all() and (_bits(got[2][k:cap]) == 0).all() and (_bits(got[0][k:cap]) == 0).all()
    for name, a, b, n in (("x_out", got[0], outs[0], cap), ("labels_out", got[1], outs[1], cap), ("weights_out", got[2], outs[2], cap),
                          ("rows_out", got[3], outs[3], cap), ("count_out", got[4], outs[4], 1)):
        assert torch.equal(_bits(a[n:]), _bits(b[n:])), "written at or beyond row cap: " + name
    return want[4]


@pytest.mark.parametrize("M", [1, 255, 256, 257, 4 * 128, 769, 1000])
def test_compact_rows_matches_torch_indexing(dev, both_halves, M):
    """Every pattern, with and without ids, three row widths, f32 and this build's 16-bit format; the capacity is the count rounded
    up to the head's granule (so padding exists), and M itself."""
    from ecamp_amd import hip_ops
    seed = 0
    for dtype in (torch.float32, h16()):
        for cols in (8, 192, 768):
            for pattern in PATTERNS:
                for with_ids in (False, True):
                    seed += 1
                    x, labels, weights, ids, scored = _case(M, cols, dtype, pattern, with_ids, seed)
                    n = int(scored.sum())
                    _run_and_check(dev, x, labels, weights, ids, scored, hip_ops.compact_cap(n))
                    if cols == 192:
                        _run_and_check(dev, x, labels, weights, ids, scored, M)


def test_compact_rows_capacity_below_the_count(dev, both_halves):
    """cap < count: exactly the first cap scored rows, the true count in count_out, nothing behind row cap -- with the cut inside the
    first segment, on a segment boundary and inside a later segment."""
    for dtype in (torch.float32, h16()):
        for pattern, with_ids in (("all", False), ("p50", True)):
            x, labels, weights, ids, scored = _case(1000, 192, dtype, pattern, with_ids, 7)
            n = int(scored.sum())
            for cap in (1, 100, 256, 300, n - 1):
                assert cap < n
                assert _run_and_check(dev, x, labels, weights, ids, scored, cap) == n


def test_compact_rows_strided_input_rows(dev, both_halves):
    for dtype in (torch.float32, h16()):
        x, labels, weights, ids, scored = _case(600, 192, dtype, "p50", True, 11, ldx=200)
        assert x.stride(0) == 200
        _run_and_check(dev, x, labels, weights, ids, scored, 512)


def test_compact_rows_across_super_segments(dev):
    """300 000 rows = 1172 segments, more than one super-segment of 1024: offsets come from the super-segment sums plus the counts
    inside the last one.  f32 with 8 columns keeps it small."""
    M = 300000
    for pattern, with_ids in (("p15", True), ("all", False), ("last", False), ("none", True)):
        x, labels, weights, ids, scored = _case(M, 8, torch.float32, pattern, with_ids, 13)
        n = int(scored.sum())
        _run_and_check(dev, x, labels, weights, ids, scored, -(-max(n, 1) // 256) * 256)
    x, labels, weights, ids, scored = _case(M, 8, torch.float32, "p50", False, 14)
    n = int(scored.sum())
    assert 140000 + 1000 < n < 155000
    _run_and_check(dev, x, labels, weights, ids, scored, 140000 + 77)       # the cut lies in the second super-segment (near source row 280 000)


def test_hip_ops_compact_rows_wrapper(dev, both_halves):
    from ecamp_amd import _lib, hip_ops
    for dtype in (torch.float32, h16()):
        x, labels, weights, ids, scored = _case(4 * 128, 192, dtype, "p15", True, 21)
        n = int(scored.sum())
        for cap in (hip_ops.compact_cap(n), None):
            out = hip_ops.compact_rows(x.to(dev), labels.to(dev), weights.to(dev), ids.to(dev), mask_id=MASK, vocab=V, cap=cap)
            want = _reference(x, labels, weights, ids, 512 if cap is None else cap)
            assert out[0].dtype == dtype and out[1].dtype == torch.int64 and out[2].dtype == torch.float32 and out[3].dtype == torch.int32
            assert out[4].dtype == torch.int64 and out[4].shape == (1,) and int(out[4].item()) == n
            for a, b in zip(out[:4], want[:4]):
                assert torch.equal(_bits(a.cpu()), _bits(b))
        noids = hip_ops.compact_rows(x.to(dev), labels.to(dev), weights.to(dev), vocab=V, cap=512)
        assert int(noids[4].item()) == int(((labels >= 0) & (labels < V)).sum()) > n
    with pytest.raises(_lib.EcampHipError):
        hip_ops.compact_rows(x, labels, weights, ids, vocab=V, cap=256)                  # CPU tensors: there is no fallback


def test_compact_rows_refuses_bad_arguments_without_a_launch(dev):
    """A row that is no multiple of 16 bytes is an argument error, and nothing is launched: the outputs keep their contents."""
    from ecamp_amd import _lib
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    labels = torch.zeros(16, dtype=torch.int64, device=dev)
    w = torch.ones(16, device=dev)
    ws = torch.zeros(64, dtype=torch.uint8, device=dev)
    for dtype, code, cols in ((torch.float32, 0, 6), (torch.bfloat16, 1, 4), (torch.bfloat16, 1, 12)):
        x = torch.ones(16, cols, dtype=dtype, device=dev)
        outs = [torch.full((16, cols), 5.0, dtype=dtype, device=dev), torch.full((16,), 5, dtype=torch.int64, device=dev),
                torch.full((16,), 5.0, device=dev), torch.full((16,), 5, dtype=torch.int32, device=dev), torch.full((1,), 5, dtype=torch.int64, device=dev)]
        rc = lib.ecamp_compact_rows(p(x), cols, p(labels), p(w), None, MASK, 16, cols, V, 16, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(outs[4]),
                                    p(ws), code, s)
        assert rc < 0 and b"multiples of 16 bytes" in lib.ecamp_last_error()
        torch.cuda.synchronize()
        assert all(bool((o == 5).all()) for o in outs)
    x = torch.ones(16, 8, device=dev)
    outs = [torch.full((16, 8), 5.0, device=dev), torch.full((16,), 5, dtype=torch.int64, device=dev), torch.full((16,), 5.0, device=dev),
            torch.full((16,), 5, dtype=torch.int32, device=dev), torch.full((1,), 5, dtype=torch.int64, device=dev)]
    rc = lib.ecamp_compact_rows(p(x), 8, p(labels), p(w), None, MASK, 16, 8, V, 16, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None, p(ws), 0, s)
    assert rc < 0 and b"null pointer" in lib.ecamp_last_error()
    rc = lib.ecamp_compact_rows(p(x), 8, p(labels), p(w), None, MASK, 16, 8, V, 16, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(outs[4]), p(ws), 7, s)
    assert rc < 0 and b"dtype" in lib.ecamp_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 5).all()) for o in outs)
