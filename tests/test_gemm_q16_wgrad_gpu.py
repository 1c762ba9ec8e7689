"""The weight-gradient form of the four-wave v_mfma_f32_16x16x32 kernel (csrc/gemm_q16.h, q16w_body; switch "q16_wgrad"): both operands
strided and read through transpose reads, the bias gradient summed from the M-side fragments, per-layer launches (C or split-K slabs)
and the grouped item-table launch.  Every case forces the kernel with "q16_wgrad" = 2 and proves by the launch counters that it ran.

Bounds.  Inputs are exact in the 16-bit format, products are exact in f32, so the only error is f32 accumulation over the contraction
(<= 16392 terms here: ~sqrt(K) * 2^-24 relative to the row's magnitude, about 1e-5 of max|ref|) and the f32 sums of the slabs; the
existing grouped test's bound, 1e-4 * max|ref| + 1e-3 for weights and 1e-3 * max|ref| + 1e-2 for bias sums, is taken against an
exact float64 product."""
import pytest
import torch

from conftest import h16

pytestmark = pytest.mark.gpu


def ops():
    from ecamp_amd import hip_ops
    return hip_ops


def _counts():
    from ecamp_amd import _lib
    lib = _lib.load()
    return int(lib.ecamp_gemm_q16_launches()), int(lib.ecamp_gemm_q8_launches()), int(lib.ecamp_wgrad_group_launches())


@pytest.fixture
def wgrad16():
    """set(mode): the "q16_wgrad" switch; back to the default afterwards."""
    o = ops()
    yield lambda mode: o.set_option("q16_wgrad", mode)
    o.set_option("q16_wgrad", -1)


def _group(dev, rows, shapes, seed):
    """items [(dy, x, base gw, base gb or None, accumulate)] and their float64 references (weights, bias sums) of ONE call."""
    gen_ = torch.Generator().manual_seed(seed)
    items, refs = [], []
    for i, (n_out, k_in) in enumerate(shapes):
        dy = (torch.randn(rows, n_out, generator=gen_) * 0.5).to(dev, h16())
        x = torch.randn(rows, k_in, generator=gen_).to(dev, h16())
        acc = i % 2 == 1
        base = torch.randn(n_out, k_in, generator=gen_).to(dev) if acc else torch.full((n_out, k_in), 7.0, device=dev)   # (overwritten)
        gb = torch.ones(n_out, device=dev) if i != 1 else None
        prod = dy.double().t() @ x.double()
        items.append((dy, x, base, gb, acc))
        refs.append((prod, dy.double().sum(0)))
    return items, refs


def _wb(ref):
    return 1e-4 * ref.abs().max().item() + 1e-3


def _bb(ref):
    return 1e-3 * ref.abs().max().item() + 1e-2


@pytest.mark.usefixtures("both_halves")
@pytest.mark.parametrize("workgroups", [64, 0])
@pytest.mark.parametrize("rows", [1000, 1280])
def test_grouped_against_float64(dev, wgrad16, rows, workgroups):
    """Grouped form: ragged M and N edges, 28 tiles, K ranges cut into segments (at these sizes both workgroup counts get the
    segment-major plan, one piece per workgroup: 4-5 segments per tile for 0, 2 for 64; the dealing is walked by the test below), a
    partial last K tile (rows 1000), overwrite and accumulate, layers with and without a bias.  The eight-wave kernel's item-table
    form ("q16_wgrad" 0) runs on the same inputs and is held to the same bound; both maximum errors are printed."""
    o = ops()
    shapes = [(1000, 520), (264, 264), (520, 1000)]
    items, refs = _group(dev, rows, shapes, seed=rows)
    assert o.wgrad_group_supported(items)
    err = {}
    for mode in (0, 2):
        wgrad16(mode)
        run = [(dy, x, gw.clone(), gb.clone() if gb is not None else None, acc) for dy, x, gw, gb, acc in items]
        q0, _, w0 = _counts()
        o.wgrad_group(run, workgroups=workgroups)
        torch.cuda.synchronize()
        q1, _, w1 = _counts()
        assert w1 - w0 == 1 and q1 - q0 == (1 if mode == 2 else 0)
        ew = eb = 0.0
        for (dy, x, gw, gb, acc), (dy0, x0, base, gb0, _), (prod, bsum) in zip(run, items, refs):
            ref = prod + base.double() if acc else prod
            dw = (gw.double() - ref).abs().max().item()
            ew = max(ew, dw / _wb(ref))
            assert dw < _wb(ref), (mode, dw, _wb(ref))
            if gb is not None:
                refb = bsum + 1.0
                db = (gb.double() - refb).abs().max().item()
                eb = max(eb, db / _bb(refb))
                assert db < _bb(refb), (mode, db, _bb(refb))
        err[mode] = (ew, eb)
        if mode == 2:   # a second call accumulates on top of the first where asked to and overwrites elsewhere
            o.wgrad_group(run, workgroups=workgroups)
            torch.cuda.synchronize()
            for (dy, x, gw, gb, acc), (dy0, x0, base, gb0, _), (prod, bsum) in zip(run, items, refs):
                ref = 2.0 * prod + base.double() if acc else prod
                assert (gw.double() - ref).abs().max().item() < _wb(ref)
                if gb is not None:
                    refb = 2.0 * bsum + 1.0
                    assert (gb.double() - refb).abs().max().item() < _bb(refb)
    print("  grouped rows %d workgroups %d: max error / bound (weights, bias): eight-wave %.3f %.3f, four-wave %.3f %.3f"
          % (rows, workgroups, err[0][0], err[0][1], err[2][0], err[2][1]))


@pytest.mark.usefixtures("both_halves")
def test_grouped_dealing_plan_against_float64(dev, wgrad16):
    """More tiles than workgroups (324 on 200): the plan deals K-tile pairs out in tile order, so a workgroup walks SEVERAL items whose
    ranges run across tile boundaries (5 units of 3 per tile), operands and leading dimensions change between a workgroup's items, and
    the 7th, partial K tile (rows 392) rides on a tile's last unit."""
    o = ops()
    rows, shapes = 392, [(2296, 2304), (2304, 2296), (2304, 2304), (2304, 2304)]
    items, refs = _group(dev, rows, shapes, seed=11)
    wgrad16(2)
    q0, _, w0 = _counts()
    o.wgrad_group(items, workgroups=200)
    torch.cuda.synchronize()
    q1, _, w1 = _counts()
    assert (q1 - q0, w1 - w0) == (1, 1)
    for (dy, x, gw, gb, acc), (prod, bsum) in zip(items, refs):
        if acc:
            continue
        assert (gw.double() - prod).abs().max().item() < _wb(prod)
        if gb is not None:
            assert (gb.double() - (bsum + 1.0)).abs().max().item() < _bb(bsum + 1.0)
    # the accumulating layers hold base + product: their bases were drawn before the call
    items2, refs2 = _group(dev, rows, shapes, seed=11)
    for (dy, x, gw, gb, acc), (_, _, base, _, _), (prod, bsum) in zip(items, items2, refs2):
        if acc:
            assert (gw.double() - (prod + base.double())).abs().max().item() < _wb(prod + base.double())


@pytest.mark.usefixtures("both_halves")
@pytest.mark.parametrize("K,split", [(4104, 1), (16392, None)])
def test_per_layer_against_float64(dev, wgrad16, K, split):
    """Per-layer form dW[264, 520]: 65 K tiles (odd, partial last one) written straight into C with alpha_dev, and K = 16392 with the split
    count the library chooses (f32 slabs + the split-K reduce); with and without a bias, overwrite and accumulate."""
    o = ops()
    from ecamp_amd import _lib
    wgrad16(2)
    n_out, k_in = 264, 520
    gen_ = torch.Generator().manual_seed(K)
    dy = (torch.randn(K, n_out, generator=gen_) * 0.5).to(dev, h16())
    x = torch.randn(K, k_in, generator=gen_).to(dev, h16())
    base = torch.randn(n_out, k_in, generator=gen_).to(dev)
    ad = torch.tensor([0.75], device=dev)
    prod = 0.75 * (dy.double().t() @ x.double())
    bsum = 0.75 * dy.double().sum(0)
    if split is None:
        split = max(1, int(_lib.load().ecamp_gemm_suggest_split(n_out, k_in, K, 0, 0, 1)))
        assert split > 1
    for bias in (False, True):
        for acc in (False, True):
            gw = base.clone()
            gb = torch.ones(n_out, device=dev) if bias else None
            q0, e0, _ = _counts()
            o.gemm(dy, x, gw, n_out, k_in, K, False, n_out, False, k_in, k_in, alpha_dev=ad, out_f32=True, accumulate=acc, split_k=split, rowsum=gb)
            torch.cuda.synchronize()
            q1, e1, _ = _counts()
            assert q1 - q0 == 1 and e1 == e0, "the four-wave weight-gradient kernel did not run"
            ref = prod + base.double() if acc else prod
            dw = (gw.double() - ref).abs().max().item()
            print("  per-layer K %d split %d bias %d acc %d: weights %.3e (bound %.3e)" % (K, split, bias, acc, dw, _wb(ref)))
            assert dw < _wb(ref)
            if bias:
                db = (gb.double() - (bsum + 1.0)).abs().max().item()
                print("    bias sums %.3e (bound %.3e)" % (db, _bb(bsum + 1.0)))
                assert db < _bb(bsum + 1.0)


@pytest.mark.usefixtures("both_halves")
def test_encoder_block_group_matches_per_layer_launches(dev, wgrad16):
    """One encoder-block group at rows 1280 with the production widths on the four-wave kernel against the per-layer launches of the
    eight-wave kernel (as the existing grouped test compares them)."""
    o = ops()
    rows, shapes = 1280, [(2304, 768), (768, 768), (3072, 768), (768, 3072)]
    items, _ = _group(dev, rows, shapes, seed=7)
    refs = []
    wgrad16(0)
    for dy, x, gw, gb, acc in items:
        gw_ref, gb_ref = gw.clone(), gb.clone() if gb is not None else None
        o.linear_wgrad(dy, x, gw_ref, gb=gb_ref, accumulate=acc)
        refs.append((gw_ref, gb_ref))
    wgrad16(2)
    q0, _, w0 = _counts()
    o.wgrad_group(items)
    torch.cuda.synchronize()
    q1, _, w1 = _counts()
    assert (q1 - q0, w1 - w0) == (1, 1)
    for (dy, x, gw, gb, acc), (gw_ref, gb_ref) in zip(items, refs):
        assert (gw - gw_ref).abs().max() < 1e-4 * gw_ref.abs().max() + 1e-3, (gw - gw_ref).abs().max()
        if gb is not None:
            assert (gb - gb_ref).abs().max() < 1e-3 * gb_ref.abs().max() + 1e-2


@pytest.mark.usefixtures("both_halves")
def test_routing_follows_the_switch(dev, wgrad16):
    """"q16_wgrad" 0: no four-wave launch from a grouped or a per-layer weight-gradient call; 2: one per grouped call and one per per-layer
    call."""
    o = ops()
    items, _ = _group(dev, 512, [(520, 520), (520, 520), (520, 520)], seed=3)   # 27 tiles
    dy, x = items[0][0], items[0][1]
    for mode in (0, 2):
        wgrad16(mode)
        q0, e0, w0 = _counts()
        o.wgrad_group(items)
        q1, e1, w1 = _counts()
        assert w1 - w0 == 1
        assert (q1 - q0, e1 - e0) == ((1 if mode == 2 else 0), len(items))   # (the layers of a grouped launch count as persistent GEMM calls either way)
        gw = torch.zeros(520, 520, device=dev)
        o.gemm(dy, x, gw, 520, 520, 512, False, 520, False, 520, 520, out_f32=True, split_k=1)
        q2, _, _ = _counts()
        assert q2 - q1 == (1 if mode == 2 else 0)
    torch.cuda.synchronize()
