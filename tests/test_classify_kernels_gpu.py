"""-m gpu: the four classification kernels (csrc/classify.hip) against float64 computed here from the same, already-rounded inputs, so
that only the kernels' f32 arithmetic is under test.  Bars: the project's f32 ones -- 2e-4 of the tensor's largest magnitude for values,
1e-3 for gradients.  Every case prints its measured worst error (recorded in profiles/linprobe.txt)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import h16

pytestmark = pytest.mark.gpu

VALUE_BAR, GRAD_BAR = 2e-4, 1e-3


def worst(got, ref):
    """max |got - ref| / max |ref|"""
    ref = ref.double()
    return float((got.double().cpu() - ref.cpu()).abs().max() / ref.abs().max().clamp_min(1e-300))


def report(what, case, err, bar):
    print("[classify] %-14s %-44s worst error / max magnitude %.2e (bar %.0e)" % (what, case, err, bar))
    assert err <= bar, (what, case, err)


# ---------------------------------------------------------------------------------------------------------------- pool_norm
# the smallest shapes that cross each boundary: one sample; several samples with two token lanes per column vector (768 / 8 = 96
# vectors); a long sequence of 1024 columns (f32: 256 vectors = one lane); the cls row included (t0 = 0) with ten lanes of 24 vectors;
# many samples of few tokens; more (sample, chunk) items than the launch has workgroups, so that a workgroup takes several; and a width
# that is no multiple of 8 (16-bit rows read 8 bytes at a time) nor of 64
POOL_SHAPES = [(1, 197, 192, 1, 197), (3, 197, 768, 1, 197), (2, 785, 1024, 1, 785), (5, 50, 192, 0, 50), (300, 5, 768, 1, 5), (2100, 3, 192, 1, 3),
               (3, 7, 100, 1, 7)]


@pytest.mark.parametrize("affine", [False, True], ids=["identity", "affine"])
@pytest.mark.parametrize("xkind", ["h16", "f32"])
@pytest.mark.parametrize("B,T,D,t0,t1", POOL_SHAPES)
def test_pool_norm_against_float64(dev, both_halves, B, T, D, t0, t1, xkind, affine):
    from ecamp_amd import hip_ops as ops
    g = torch.Generator().manual_seed(B * 1000 + T + D)
    offset = torch.rand(D, generator=g) * 8 - 4          # a few units per column: a mean kept in 16 bits would miss the bar
    x = (torch.randn(B, T, D, generator=g) + offset).to(h16() if xkind == "h16" else torch.float32)
    gamma = (1 + 0.5 * torch.randn(D, generator=g)) if affine else None
    beta = torch.randn(D, generator=g) if affine else None
    xd = x.double()
    pooled_ref = xd[:, t0:t1].mean(dim=1)
    feat_ref = F.layer_norm(pooled_ref, (D,), gamma.double() if affine else None, beta.double() if affine else None, 1e-6)
    xg = x.to(dev)
    a = ops.pool_norm(xg, t0, t1, gamma.to(dev) if affine else None, beta.to(dev) if affine else None, 1e-6)
    b = ops.pool_norm(xg, t0, t1, gamma.to(dev) if affine else None, beta.to(dev) if affine else None, 1e-6)
    assert a[0].dtype == a[1].dtype == torch.float32 and a[0].shape == a[1].shape == (B, D)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "two calls must give the same bits"
    case = "B=%d T=%d D=%d [%d,%d) %s %s" % (B, T, D, t0, t1, str(x.dtype).split(".")[-1], "affine" if affine else "identity")
    report("pool_norm mean", case, worst(a[0], pooled_ref), VALUE_BAR)
    report("pool_norm feat", case, worst(a[1], feat_ref), VALUE_BAR)
    # what the bar is worth here: the same mean rounded to the 16-bit format misses it
    if xkind == "h16":
        assert worst(pooled_ref.to(h16()).double(), pooled_ref) > VALUE_BAR


def test_pool_norm_refuses_bad_arguments(dev):
    from ecamp_amd import _lib
    from ecamp_amd import hip_ops as ops
    x = torch.zeros(2, 5, 8, device=dev, dtype=torch.float32)
    with pytest.raises(_lib.EcampHipError, match="t0"):
        ops.pool_norm(x, 3, 3)
    with pytest.raises(_lib.EcampHipError, match="t0"):
        ops.pool_norm(x, 1, 6)
    with pytest.raises(_lib.EcampHipError, match="multiple of 4"):
        ops.pool_norm(torch.zeros(2, 5, 6, device=dev), 1, 5)


# ---------------------------------------------------------------------------------------------------------------- head, loss, wgrad
# (the last: D = 100 -- fewer 16-byte vectors than a wave has lanes in the forward, a partly filled 64-column tile in the weight gradient)
HEAD_SHAPES = [(1, 1, 192), (5, 3, 768), (37, 14, 768), (256, 20, 1024), (1500, 5, 192), (9, 3, 100)]


def _head_inputs(B, C, D):
    g = torch.Generator().manual_seed(B + 31 * C + D)
    feat = torch.randn(B, D, generator=g)
    w = torch.randn(C, D, generator=g) * D ** -0.5
    bias = torch.randn(C, generator=g)
    return feat, w, bias, g


@pytest.mark.parametrize("B,C,D", HEAD_SHAPES)
def test_head_forward_against_float64(dev, B, C, D):
    from ecamp_amd import hip_ops as ops
    feat, w, bias, _ = _head_inputs(B, C, D)
    ref = feat.double() @ w.double().t() + bias.double()
    a = ops.cls_head_fwd(feat.to(dev), w.to(dev), bias.to(dev))
    b = ops.cls_head_fwd(feat.to(dev), w.to(dev), bias.to(dev))
    assert a.shape == (B, C) and a.dtype == torch.float32 and torch.equal(a, b)
    report("cls_head_fwd", "B=%d C=%d D=%d" % (B, C, D), worst(a, ref), VALUE_BAR)


@pytest.mark.parametrize("B,C,D", HEAD_SHAPES)
def test_head_weight_gradient_against_float64(dev, B, C, D):
    from ecamp_amd import hip_ops as ops
    feat, _, _, g = _head_inputs(B, C, D)
    dl = torch.randn(B, C, generator=g) / B
    dw_ref, db_ref = dl.double().t() @ feat.double(), dl.double().sum(0)
    a = ops.cls_head_wgrad(dl.to(dev), feat.to(dev))
    b = ops.cls_head_wgrad(dl.to(dev), feat.to(dev))
    assert a[0].shape == (C, D) and a[1].shape == (C,) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    case = "B=%d C=%d D=%d" % (B, C, D)
    report("wgrad dW", case, worst(a[0], dw_ref), GRAD_BAR)
    report("wgrad db", case, worst(a[1], db_ref), GRAD_BAR)
    # overwriting: a second call into tensors that held something else gives the same result (the outputs are fresh here; the
    # kernel itself never reads them)


def _loss_ref(x, y, kind):
    xd = x.double().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(xd, y.double()) if kind == 0 else F.cross_entropy(xd, y)
    loss.backward()
    return loss.detach(), xd.grad


def _host_counts(x, y, kind):
    if kind == 0:
        return [x.shape[0], int((((x > 0) == (y > 0.5)).all(dim=1)).sum())]
    return [x.shape[0], int((torch.argmax(x, dim=-1) == y).sum())]


def _targets(B, C, kind, g):
    return (torch.rand(B, C, generator=g) < 0.4).float() if kind == 0 else torch.randint(0, C, (B,), generator=g)


@pytest.mark.parametrize("kind", [0, 1], ids=["bce", "ce"])
@pytest.mark.parametrize("B,C,D", HEAD_SHAPES)
def test_loss_gradient_and_counts_against_float64(dev, B, C, D, kind):
    from ecamp_amd import hip_ops as ops
    g = torch.Generator().manual_seed(7 * B + C + kind)
    x = torch.randn(B, C, generator=g) * 3
    y = _targets(B, C, kind, g)
    loss_ref, grad_ref = _loss_ref(x, y, kind)
    a = ops.cls_loss(x.to(dev), y.to(dev), kind, check=True)
    b = ops.cls_loss(x.to(dev), y.to(dev), kind)
    assert all(torch.equal(p, q) for p, q in zip(a, b)), "two calls must give the same bits"
    loss, dlogits, counts, bad = a
    assert loss.shape == (1,) and dlogits.shape == (B, C) and counts.dtype == torch.int64 and int(bad.item()) == 0
    case = "B=%d C=%d kind=%d" % (B, C, kind)
    report("cls_loss", case, worst(loss, loss_ref.reshape(1)), VALUE_BAR)
    report("cls_loss grad", case, worst(dlogits, grad_ref), GRAD_BAR)
    assert counts.tolist() == _host_counts(x, y, kind)


@pytest.mark.parametrize("kind", [0, 1], ids=["bce", "ce"])
def test_loss_stays_finite_at_logits_of_80(dev, kind):
    """exp(80) overflows nothing in f32 yet, but exp(80) * exp(80) / the naive log(1 + exp(x)) and softmax without the row maximum do."""
    from ecamp_amd import hip_ops as ops
    g = torch.Generator().manual_seed(80 + kind)
    B, C = 37, 14
    x = (torch.randint(0, 2, (B, C), generator=g).float() * 2 - 1) * 80
    x[0] = 80.0
    x[1] = -80.0
    y = _targets(B, C, kind, g)
    loss_ref, grad_ref = _loss_ref(x, y, kind)
    loss, dlogits, counts, _ = ops.cls_loss(x.to(dev), y.to(dev), kind, check=True)
    assert torch.isfinite(loss).all() and torch.isfinite(dlogits).all()
    report("cls_loss +-80", "B=%d C=%d kind=%d" % (B, C, kind), worst(loss, loss_ref.reshape(1)), VALUE_BAR)
    report("grad +-80", "B=%d C=%d kind=%d" % (B, C, kind), worst(dlogits, grad_ref), GRAD_BAR)
    assert counts.tolist() == _host_counts(x, y, kind)


def test_counts_break_an_argmax_tie_towards_the_lowest_index(dev):
    from ecamp_amd import hip_ops as ops
    x = torch.tensor([[2.0, 1.0, 2.0], [2.0, 1.0, 2.0], [0.5, 0.5, 0.5], [0.0, 3.0, 3.0], [1.0, 2.0, 3.0]])
    y = torch.tensor([0, 2, 0, 2, 2])
    assert torch.argmax(x, dim=-1).tolist() == [0, 0, 0, 1, 2]
    counts = ops.cls_loss(x.to(dev), y.to(dev), 1, check=True)[2]
    assert counts.tolist() == [5, 3] == _host_counts(x, y, 1)
    # kind 0: a logit of exactly 0 predicts "absent" (sigmoid(0) = 0.5 is not > 0.5)
    x0 = torch.tensor([[0.0, 1.0], [0.0, -1.0], [2.0, -2.0]])
    y0 = torch.tensor([[0.0, 1.0], [1.0, 0.0], [1.0, 0.0]])
    assert ops.cls_loss(x0.to(dev), y0.to(dev), 0)[2].tolist() == [3, 2] == _host_counts(x0, y0, 0)


@pytest.mark.parametrize("label", [3, -1, 2 ** 40])
def test_an_out_of_range_label_raises_and_reads_nothing(dev, label):
    from ecamp_amd import _lib
    from ecamp_amd import hip_ops as ops
    x = torch.randn(6, 3, generator=torch.Generator().manual_seed(1))
    y = torch.tensor([0, 1, label, 2, 1, 0])
    with pytest.raises(_lib.EcampHipError, match="outside"):
        ops.cls_loss(x.to(dev), y.to(dev), 1, check=True)
    loss, dlogits, counts, bad = ops.cls_loss(x.to(dev), y.to(dev), 1)       # unchecked: the flag is there to be read later
    assert int(bad.item()) == 1 and torch.isfinite(loss).all() and torch.all(dlogits[2] == 0) and counts[0].item() == 6
    keep = [0, 1, 3, 4, 5]
    ref = F.cross_entropy(x[keep].double(), y[keep], reduction="sum") / 6
    assert worst(loss, ref.reshape(1)) <= VALUE_BAR
    ops.cls_check_labels(ops.cls_loss(x.to(dev), torch.tensor([0, 1, 2, 2, 1, 0], device=dev), 1)[3], 3)   # a clean call clears it
