"""No GPU: the reference of tests/_sr_ref.py is what it claims to be, and the conditions tests/test_sr_head_gpu.py relies on hold --
the hand-written backward is autograd's, the open regime is open at every shape, every multi-tile shape exceeds the grid cap it is
meant to exceed with every carry of the pair backward's tile cursor in use, and the mixed regime loses at most 2 % of its elements
to undecided gates at the K the GPU test uses."""
import pytest
import torch

import _sr_ref as S


def close(name, got, ref, rel=1e-12):
    d = float((got - ref).abs().max())
    assert d <= rel * max(1.0, float(ref.abs().max())), "%s: %.3e apart" % (name, d)


@pytest.mark.parametrize("regime", ["open", "mixed", "closed"])
@pytest.mark.parametrize("shape", ["one-tile-w3", "ring-w2", "pair-bwd-trips"])
def test_hand_written_backward_is_autograd(shape, regime):
    """model() with no rounding == graph() (F.interpolate, autograd) to 1e-12 of each quantity's largest value: the bilinear matrix and
    its transpose, both transposed convolutions, the gates, the per-tile sums in the kernels' order."""
    H = S.host(shape, regime)
    m = S.model(*H.args)
    for q in ("u", "z1", "z2", "s", "loss", "dsr", "gw"):
        close("%s %s %s" % (shape, regime, q), m[q], H.ref[q])


def test_gradient_order_is_the_kernels():
    """gw = {dW1[o][i][ky][kx], db1, dW2, db2}: a central difference of 0.5 * loss in one weight of each block (exact up
    to rounding in the open regime, where the loss is quadratic) lands on its index."""
    H = S.host("one-tile-w1", "open")
    for blk, idx, at in ((0, (2, 1, 0, 2), 2 * 27 + 1 * 9 + 0 * 3 + 2), (1, (1,), 81 + 1), (2, (0, 2, 2, 1), 84 + 2 * 9 + 2 * 3 + 1), (3, (2,), 165 + 2)):
        ws = [t.double().clone() for t in H.ws]
        ws[blk][idx] += 1e-3
        up = S.graph(H.p, ws, H.big, H.mask, backward=False)["loss"]
        ws[blk][idx] -= 2e-3
        dn = S.graph(H.p, ws, H.big, H.mask, backward=False)["loss"]
        fd = float(0.5 * (up - dn) / 2e-3)
        assert abs(fd - float(H.ref["gw"][at])) <= 1e-9 * float(H.A["gw"][at]), (blk, fd, float(H.ref["gw"][at]))


def test_float32_chain_rounds_after_every_addition():
    """The yardstick of the atomically gathered sums (loss, gw) is a chain of float32 additions, one rounding each: 2^24 + 1 + 1 stays
    2^24 (torch.cumsum on the CPU accumulates float32 in double and would give 2^24 + 2).  In float64 the model sums plainly."""
    parts = torch.tensor([[2.0 ** 24], [0.0], [1.0], [1.0]], dtype=torch.float32)
    got = S.chain(parts)
    assert got.shape == (S.ORDERS, 1) and float(got[0, 0]) == 2.0 ** 24
    assert set(got[:, 0].tolist()) <= {2.0 ** 24, 2.0 ** 24 + 2}       # 1 + 1 first is exact
    H = S.host("ring-w2", "open")
    m = S.model(*H.args, dtype=torch.float32)
    assert m["gw"].shape == (S.ORDERS, 168) and m["loss"].shape == (S.ORDERS,) and m["gw"].dtype == torch.float32


def test_rounding_model_rounds_where_the_kernels_do():
    """u, c1, ds, dc1 come out of the model as 16-bit values; the skip connection keeps s unrounded."""
    H = S.host("ring-w2", "open")
    for half in ("bf16", "f16"):
        rnd = S.rounder(half)
        m = S.model(*H.args, half=half)
        assert torch.equal(rnd(m["ds"]), m["ds"]) and torch.equal(rnd(m["dc1"]), m["dc1"])
        assert not torch.equal(rnd(m["s"]), m["s"]) and not torch.equal(m["s"], H.ref["s"])
        assert float((m["s"] - H.ref["s"]).abs().max()) < 40 * S.U16[half] * float(H.A["s"].max())


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_open_regime_is_open(shape):
    """min z1 > 1 and min z2 > 1 in float64: no gate is within any rounding of zero, the head is affine."""
    z1, z2 = S.host(shape, "open").margins()
    print("%s: min z1 %.2f, min z2 %.2f" % (shape, z1, z2))
    assert z1 > 1 and z2 > 1


def test_closed_regime_is_closed():
    for shape in ("ring-w2", "pair-bwd-trips"):
        H = S.host(shape, "closed")
        assert float(H.ref["s"].abs().max()) == 0 and float(H.ref["dsr"].abs().max()) == 0 and float(H.ref["gw"].abs().max()) == 0
        want = (H.mask * H.big.double() ** 2).sum()
        assert abs(float(H.ref["loss"] - want)) <= 1e-12 * float(want)


def test_shapes_exceed_their_grid_caps_and_use_every_cursor_carry():
    assert S.tiles("production") == 588 > S.CAP_BWD1 and S.tiles("pair-bwd-trips") == 576 > S.CAP_BWD1
    assert S.tiles("fused-bwd-trips") == 1044 > S.CAP_BWD0
    assert S.tiles("fwd-trips") == 2052 > S.CAP_FWD
    for shape in ("production", "pair-bwd-trips"):
        G = 2 * S.SHAPES[shape][1] // S.SRT
        assert all(v > 0 for v in S.cursor_steps(S.CAP_BWD1, G)), (shape, S.cursor_steps(S.CAP_BWD1, G))
    # the cursor itself: stepping by the grid size with carries lands on t = b G G + ty G + tx
    G, grid = 6, S.CAP_BWD1
    sb, sy, sx = S.cursor_steps(grid, G)
    for t0 in (0, 35, 511):
        b, ty, tx = t0 // (G * G), (t0 // G) % G, t0 % G
        t = t0
        for _ in range(3):
            t, tx = t + grid, tx + sx
            if tx >= G:
                tx, ty = tx - G, ty + 1
            ty += sy
            if ty >= G:
                ty, b = ty - G, b + 1
            b += sb
            assert (b, ty, tx) == (t // (G * G), (t // G) % G, t % G)


def test_seeded_windows_hold_an_interior_and_a_clipped_one():
    for shape in ("pair-bwd-trips", "fused-bwd-trips", "fwd-trips"):
        B, R, win, column, row, _ = S.geometry(shape)
        G = 2 * R // S.SRT
        cr = list(zip(column.tolist(), row.tolist()))
        assert (2, 2) in cr and (G - 1, G - 1) in cr and len(set(cr)) > 4
        assert int(column.max()) < G and int(row.max()) < G


def test_structural_zeros_are_the_tiles_out_of_reach():
    """A == 0 exactly on the pred_img tiles further than one tile from the window, A > 0 on every element of the others."""
    H = S.host("pair-bwd-trips", "open")
    G, PT = 2 * H.R // S.SRT, S.SRT // 2
    for b in range(H.B):
        c0, r0 = int(H.column[b]), int(H.row[b])
        for ty in range(G):
            for tx in range(G):
                a = H.A["dsr"][b, :, ty * PT:(ty + 1) * PT, tx * PT:(tx + 1) * PT]
                far = ty < c0 - 1 or ty > c0 + H.win or tx < r0 - 1 or tx > r0 + H.win
                if far:
                    assert float(a.abs().max()) == 0 and float(H.ref["dsr"][b, :, ty * PT:(ty + 1) * PT, tx * PT:(tx + 1) * PT].abs().max()) == 0
                elif c0 <= ty < c0 + H.win and r0 <= tx < r0 + H.win:
                    assert float(a.min()) > 0
    thin = (H.A["dsr"] > 0) & (H.ref["dsr"].abs() < 1e-3 * H.ref["dsr"].abs().max())
    assert 0.005 < float(thin.sum()) / float((H.A["dsr"] > 0).sum()) < 0.5      # the thin band a max-norm cannot see


@pytest.mark.parametrize("shape", [s for s in S.SHAPES if "bwd" in S.SHAPES[s][4]])
def test_mixed_regime_excludes_at_most_two_percent(shape):
    H = S.host(shape, "mixed")
    U = H.undecided()
    print("%s: K %.2f, undecided z2 %d z1 %d, excluded share %.4f, largest gw allowance / A %.2e"
          % (shape, U["K"], int(U["z2"].sum()), int(U["z1"].sum()), U["share"], float((U["gw_allowance"] / H.A["gw"]).max())))
    assert U["share"] <= S.EXCLUDED_SHARE_CAP
    closed = float((H.ref["z2"] <= 0).double().mean())
    assert 0.2 < closed < 0.8           # "about half the gates are closed"
