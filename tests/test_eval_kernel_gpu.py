"""-m gpu: `ecamp_ce_eval` (csrc/text.hip), the evaluation form of the MLM head's loss, through hip_ops.ce_eval against float64
arithmetic on the stored values.

Logits are multiples of 0.25 in [-8, 8]: exact in bfloat16, IEEE half and f32, and full of ties.  Contract checked per case:
  counts  int64[3] = [rows whose label lies in [0, V), label ranks first, label within the first five], rank = logits STRICTLY above the
          label's -- equal to the reference as integers
  loss    loss_sum / M within 1e-5 relative of sum_i w_i (logsumexp_i - x_i[label_i]) / M (the bound test_kernels_gpu.py holds
          ecamp_ce_fwd_bwd's loss to)
  logits  bitwise unchanged by the call
Every case carries rows that pin the rank rule (label tied with the maximum; exactly four / exactly five logits above the label; label
in the row's last 16-byte group; label at column 0; ten rows with 0..9 logits above the label at random columns and thousands tied
with it), ignored labels (-100 and V), and weights of zero."""
import ctypes
import functools

import pytest
import torch

from conftest import h16

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("both_halves")]

M = 37
# the (NG, NT) rungs of the row-in-registers form end at 4096, 8192, 16384 and 32768; 30000 is the vocabulary
V_REG = [8, 4096, 4104, 8192, 16384, 16392, 30000]
V_GENERIC = [30004, 32776]      # V % 8 != 0, V > 32768: refused by the register form
V_F32 = [8, 4100, 30000]


def _spread(V, label, k):
    """k distinct columns other than `label`, spread over the row (first, last, middle, ...)."""
    cand = []
    for c in (0, V - 1, V // 2, 1, V - 2, V // 3, 2 * V // 3, 3, 5, 6):
        if c != label and c not in cand:
            cand.append(c)
    assert len(cand) >= k
    return cand[:k]


@functools.lru_cache(maxsize=None)
def case(V, seed=0, all_ignored=False):
    """-> (logits f32 [M, V], labels int64 [M], weights f32 [M]) on the host."""
    g = torch.Generator().manual_seed(1000 * seed + V)
    x = torch.randint(-32, 33, (M, V), generator=g).float() * 0.25
    labels = torch.randint(0, V, (M,), generator=g)
    w = torch.rand(M, generator=g) * 2
    w[7] = 0.0
    w[20] = 0.0
    labels[0], labels[1], labels[2], labels[3] = -100, V, 0, V - 1
    labels[9::6] = -100
    # row 4: the label tied with the maximum -> first
    labels[4] = V // 2
    x[4, V // 2] = 8.0
    x[4, _spread(V, V // 2, 1)[0]] = 8.0
    # rows 5 / 6: exactly four / exactly five logits above the label (in the last 16-byte group / at column 0), the rest at or below it
    for r, lab, k in ((5, V - 2, 4), (6, 0, 5)):
        labels[r] = lab
        x[r].clamp_(max=1.0)
        x[r, lab] = 1.0
        x[r, _spread(V, lab, k)] = 2.0
    # rows 10..19: 0..9 logits above the label at random columns, a quarter of the row TIED with it (rank counts strictly greater only)
    for r in range(10, 20):
        k = min(r - 10, V - 2)
        lab = int(labels[r])
        if lab < 0:     # (row 15 is one of the ignored ones)
            continue
        x[r].clamp_(max=4.0)
        x[r, lab] = 4.0
        cols = [c for c in torch.randperm(V, generator=g).tolist()[:k + 1] if c != lab][:k]
        x[r, cols] = 6.0
    if all_ignored:
        labels[0::2] = -100
        labels[1::2] = V
    return x, labels, w


@functools.lru_cache(maxsize=None)
def reference(V, seed=0, all_ignored=False):
    """float64 on the stored values -> (loss_sum / M, [scored, top1, top5])."""
    x, labels, w = case(V, seed, all_ignored)
    x = x.double()
    valid = (labels >= 0) & (labels < V)
    idx = labels.clamp(0, V - 1)
    xl = x.gather(1, idx[:, None])[:, 0]
    rank = (x > xl[:, None]).sum(1)
    ce = torch.logsumexp(x, 1) - xl
    loss = float((ce * w.double())[valid].sum() / M)
    counts = [int(valid.sum()), int((valid & (rank == 0)).sum()), int((valid & (rank < 5)).sum())]
    return loss, counts


def _check(dev, dtype, V, place, seed=0, all_ignored=False):
    from ecamp_amd import hip_ops
    x, labels, w = case(V, seed, all_ignored)
    ref_loss, ref_counts = reference(V, seed, all_ignored)
    if not all_ignored:
        # on the reference alone: a kernel that returns constants cannot pass
        assert 0 < ref_counts[1] < ref_counts[2] < ref_counts[0] < M, ref_counts
        r = (x[4:7].double() > x[4:7].double().gather(1, labels[4:7, None])).sum(1).tolist()
        assert r == [0, 4, 5]
    assert torch.equal(x.to(dtype).float(), x), "the inputs must be exact in the format under test"
    xd = place(x.to(dtype), dev)
    before = xd.clone()
    loss_sum, counts = hip_ops.ce_eval(xd, labels.to(dev), w.to(dev))
    torch.cuda.synchronize()
    got = counts.cpu().tolist()
    loss = float(loss_sum.item()) / M
    err = abs(loss - ref_loss) / max(abs(ref_loss), 1e-30) if ref_loss != 0 else abs(loss)
    print("  V=%d %s counts %s (ref %s) loss %.7f (ref %.7f) rel err %.2e" % (V, str(dtype).split(".")[-1], got, ref_counts, loss, ref_loss, err))
    assert loss_sum.dtype == torch.float32 and loss_sum.shape == (1,) and counts.dtype == torch.int64 and counts.shape == (3,)
    assert got == ref_counts
    assert err <= 1e-5
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(xd.view(bits), before.view(bits)), "ecamp_ce_eval wrote to the logits"


def _dense(x, dev):
    return x.to(dev)


def _strided(x, dev):
    """ld = V + 8: a column slice of a wider buffer (its other columns would be scored as +inf if they were read)."""
    buf = torch.full((x.shape[0], x.shape[1] + 8), float("inf"), dtype=x.dtype, device=dev)
    buf[:, :x.shape[1]] = x.to(dev)
    return buf[:, :x.shape[1]]


def _misaligned(x, dev):
    """A base 4 elements past a 16-byte boundary: refused by the 16-byte loads of the register form."""
    flat = torch.empty(x.numel() + 8, dtype=x.dtype, device=dev)
    v = flat[4:4 + x.numel()].view(x.shape)
    v.copy_(x.to(dev))
    assert v.data_ptr() % 16 == 8 and flat.data_ptr() % 16 == 0
    return v


@pytest.mark.parametrize("V", V_REG + V_GENERIC)
def test_ce_eval_16bit(dev, V):
    _check(dev, h16(), V, _dense)


@pytest.mark.parametrize("V", [4096, 30000, 30004])
def test_ce_eval_16bit_strided_rows(dev, V):
    _check(dev, h16(), V, _strided, seed=1)


def test_ce_eval_16bit_misaligned_base(dev):
    _check(dev, h16(), 4096, _misaligned, seed=2)


@pytest.mark.parametrize("V", V_F32)
def test_ce_eval_f32(dev, V):
    _check(dev, torch.float32, V, _dense, seed=3)


def test_ce_eval_f32_strided_rows(dev):
    _check(dev, torch.float32, 4100, _strided, seed=4)


@pytest.mark.parametrize("V,f32", [(30000, False), (30004, False), (4100, True)])
def test_ce_eval_every_row_ignored(dev, V, f32):
    """Labels of -100 and V only: nothing is scored, and both outputs stay exactly zero."""
    from ecamp_amd import hip_ops
    _check(dev, torch.float32 if f32 else h16(), V, _dense, seed=5, all_ignored=True)
    x, labels, w = case(V, 5, True)
    loss_sum, counts = hip_ops.ce_eval(x.to(dev, torch.float32 if f32 else h16()), labels.to(dev), w.to(dev))
    assert counts.cpu().tolist() == [0, 0, 0] and float(loss_sum.item()) == 0.0


def test_ce_eval_refuses_bad_arguments_without_a_launch(dev):
    from ecamp_amd import _lib, hip_ops
    lib = _lib.load()
    x = torch.zeros(4, 8, dtype=h16(), device=dev)
    labels = torch.zeros(4, dtype=torch.int64, device=dev)
    w = torch.ones(4, device=dev)
    loss = torch.full((1,), 7.0, device=dev)
    counts = torch.full((3,), 7, dtype=torch.int64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = hip_ops.stream()
    rc = lib.ecamp_ce_eval(p(x), p(labels), p(w), p(loss), p(counts), 4, 6, 8, 1, s)
    assert rc != 0 and b"multiples of 4" in lib.ecamp_last_error()
    rc = lib.ecamp_ce_eval(p(x), p(labels), p(w), p(loss), None, 4, 8, 8, 1, s)
    assert rc != 0 and b"null pointer" in lib.ecamp_last_error()
    rc = lib.ecamp_ce_eval(p(x), p(labels), p(w), p(loss), p(counts), 4, 8, 6, 1, s)
    assert rc != 0 and lib.ecamp_last_error() != b""
    torch.cuda.synchronize()
    assert float(loss.item()) == 7.0 and counts.cpu().tolist() == [7, 7, 7]      # nothing ran
    with pytest.raises(_lib.EcampHipError, match="CPU tensor"):
        hip_ops.ce_eval(x.cpu(), labels.cpu(), w.cpu())
    with pytest.raises(TypeError):
        hip_ops.ce_eval(x.to(torch.float64), labels, w)
