"""-m gpu: the report-side training kernels of csrc/text.hip -- ecamp_ce_fwd_bwd (the weighted cross-entropy that writes its gradient
over the logits) and ecamp_bert_embed_fwd / ecamp_bert_embed_bwd -- against float64, element by element, on all three formats.

test_kernels_gpu.py judges them by max|err| / max|ref| at workload shapes: the label column of a cross-entropy row is three to four
orders of magnitude above the rest of it, so a softmax part wrong by half passes, and its shapes reach two of the six cross-entropy
kernels and one of the embedding kernels' launch geometries.  Here every element is held to |got - ref| <= K u A (tests/_report_ref.py,
proven against autograd in tests/test_report_reference_cpu.py): ref in float64, A the same arithmetic on magnitudes, u half a rounding
of the stored format, K = max(1, 4 K_yard) with K_yard measured on a CPU yardstick of the same case; rows without a weight are zero,
and what no row reaches keeps its prior contents bit for bit.  Nothing is a fixed number; every case prints K_yard and the kernel's
own figure (profiles/report_side_float64.txt is that output on an MI355X).

Cross-entropy, M = 37 rows, finite logits; which V reaches which kernel (the dispatch of ecamp_ce_fwd_bwd: 16-bit rows with V % 8 == 0,
ld % 8 == 0, V <= 32768 and a 16-byte aligned base go to the row-in-registers form, whose rungs end at 4096 / 8192 / 16384 / 32768):
    ce_fwd_bwd_row_kernel<1, 512>    V = 8, 4096            ce_fwd_bwd_row_kernel<2, 512>    V = 4104, 8192
    ce_fwd_bwd_row_kernel<4, 512>    V = 8200, 16384        ce_fwd_bwd_row_kernel<4, 1024>   V = 16392, 30000, 32768
    ce_fwd_bwd_kernel<16-bit>        V = 4, 30004 (V % 8), 32776 (V > 32768); V = 4096 / 30000 at ld = V + 4 (ld % 8); V = 4096 at a
                                     base 8 bytes past a 16-byte boundary
    ce_fwd_bwd_kernel<float>         V = 4, 1020, 4100, 30000
Strided rows (ld = V + 8 and V + 4) and the misaligned base sit in a buffer filled with a bit pattern, one guard row (or 24 bytes) in
front and behind: every bit outside the [M, V] view is unchanged after the call.  Embedding shapes: _report_ref.EMB_SHAPES.

Measured on an MI355X (every line: profiles/report_side_float64.txt), kernel err / (u A) against the yardstick's, largest over the cases:
    ce row form     bfloat16  grad 1.99 / 1.99 (bound 7.97)   loss 0.80 / 1.46 (5.82)      IEEE half  grad 1.98 / 1.98 (7.93)   loss 1.08 / 1.68 (6.71)
    ce generic      bfloat16  grad 1.99 / 1.99 (7.97)   loss 0.84 / 0.84 (3.37)            IEEE half  grad 1.90 / 1.90 (7.59)   loss 1.24 / 0.90 (3.60)
                    f32       grad 88.7 / 34.5 (138; V = 30000)   loss 0.68 / 0.68 (2.71)
    embed bfloat16  z 1.98 / 1.98   mean 0.16 / 0.16   rstd 0.68 / 0.94   e 1.52 / 1.52   gword 1.99 / 2.67   gpos 0.99 / 0.78   gtype 0.66 / 1.26   dgamma 1.04 / 1.94   dbeta 1.72 / 2.45
    embed IEEE half z 1.99 / 1.99   mean 0.32 / 0.32   rstd 0.64 / 0.76   e 1.57 / 1.57   gword 2.50 / 2.50   gpos 0.95 / 0.84   gtype 0.82 / 0.63   dgamma 0.96 / 1.97   dbeta 1.32 / 2.65
    embed f32       z 1.92 / 1.92   mean 1.54 / 0.72   rstd 0.78 / 0.73   e 3.10 / 2.98   gword 2.54 / 2.54   gpos 1.03 / 0.93   gtype 0.68 / 1.12   dgamma 1.02 / 1.57   dbeta 1.73 / 2.30
The 16-bit gradients reproduce one rounding of the float64 value to three digits on every kernel.  The f32 gradient stands at 2.6 times
its yardstick where one logit leads a row by 30: __expf multiplies x - max by log2(e) in float32 before the hardware exp2, which costs
|x - max| 2^-24 of relative accuracy (22 u at 30) on top of the 2^-20 the float32 difference x - max has already lost in either
computation -- within the factor 4, and far below what the optimizer sees.  The loss leaves through one float atomic per row in no
particular order: its yardstick is the worst of 16 seeded orders of the same float32 chain (tests/_report_ref.py says why row order
alone is not a yardstick: the first run of this file had one loss at 1.14 against a row-order figure of 0.115, and passed the next time).
Rows without a weight may come out as zeros of either sign (the generic kernel multiplies 0 by a negative softmax term); they compare
equal to zero, which is what is asserted."""
import ctypes

import pytest
import torch

import _report_ref as R
from conftest import h16

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16, torch.float16]
PATTERN = {2: 0x5A5A, 4: 0x5A5A5A5A}       # finite in every format; no kernel output looks like it


def ops():
    from ecamp_amd import hip_ops
    return hip_ops


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def patterned(n, dtype, dev):
    t = torch.empty(n, dtype=dtype, device=dev)
    bits(t).fill_(PATTERN[t.element_size()])
    return t


# ---- where the [M, V] logits live: -> (the view the kernel gets, a check of everything around it) ------------------------------------
def dense(x, dev):
    return x.to(dev), lambda: None


def strided(extra):
    """Rows ld = V + extra apart inside a patterned buffer with one guard row in front and one behind."""
    def place(x, dev):
        M, V = x.shape
        ld = V + extra
        buf = patterned((M + 2) * ld, x.dtype, dev).view(M + 2, ld)
        v = buf[1:M + 1, :V]
        v.copy_(x.to(dev))
        assert v.stride(0) == ld and v.stride(1) == 1
        outside = torch.ones(M + 2, ld, dtype=torch.bool, device=dev)
        outside[1:M + 1, :V] = False

        def check():
            n = int((bits(buf)[outside] != PATTERN[x.element_size()]).sum())
            assert n == 0, "%d elements outside the [M, V] view of a buffer with ld = V + %d were written" % (n, extra)
        return v, check
    return place


def misaligned(x, dev):
    """A base 8 bytes past a 16-byte boundary (16-bit rows: refused by the 16-byte loads of the register form), 24 bytes of guard in
    front and behind."""
    n, g = x.numel(), 12
    flat = patterned(n + 2 * g, x.dtype, dev)
    v = flat[g:g + n].view(x.shape)
    v.copy_(x.to(dev))
    assert flat.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 8

    def check():
        b = bits(flat)
        assert bool((b[:g] == PATTERN[2]).all()) and bool((b[g + n:] == PATTERN[2]).all()), "the guards around a misaligned base were written"
    return v, check


def run_ce(dev, dtype, V, place=dense, seed=0, gain=1.0, where="dense"):
    fmt = R.fmt_of(dtype)
    x, labels, w = R.ce_case(V, fmt, seed)
    xd, check_guards = place(x.to(dtype), dev)
    loss = torch.zeros(1, device=dev)
    out = ops().ce_fwd_bwd_(xd, labels.to(dev), w.to(dev), loss, gain=gain)
    torch.cuda.synchronize()
    assert out is xd
    ld, aligned = xd.stride(0), xd.data_ptr() % 16 == 0
    tag = "ce %s V=%d %s%s -> %s" % (fmt, V, where, "" if gain == 1.0 else " gain", R.ce_kernel_of(V, fmt, ld, aligned))
    lines, bad = R.ce_judge(tag, fmt, x, labels, w, gain, xd.cpu(), loss.item())
    print("\n".join(lines))
    check_guards()
    assert not bad, "\n".join(bad)


# ================================================================================================ weighted cross-entropy
@pytest.mark.parametrize("V", R.V_REG)
def test_ce_16bit_register_form(dev, both_halves, V):
    """ce_fwd_bwd_row_kernel at <1,512>, <2,512>, <4,512> and <4,1024>: both sides of every rung and the top of the last one."""
    assert R.ce_kernel_of(V, both_halves).startswith("row<")
    run_ce(dev, h16(), V)


@pytest.mark.parametrize("V", R.V_GENERIC)
def test_ce_16bit_generic(dev, both_halves, V):
    """The two-pass kernel on the 16-bit rows the register form refuses: V % 8 != 0 (one lane holds the whole row at V = 4), V > 32768."""
    assert R.ce_kernel_of(V, both_halves) == "generic<16>"
    run_ce(dev, h16(), V, seed=1)


@pytest.mark.parametrize("V", R.V_F32)
def test_ce_f32(dev, V):
    run_ce(dev, torch.float32, V, seed=2)


@pytest.mark.parametrize("extra", [8, 4])
@pytest.mark.parametrize("V", [4096, 30000, 30004])
@pytest.mark.parametrize("dtype", DT)
def test_ce_strided_rows_leave_the_other_columns_alone(dev, dtype, V, extra):
    """A column slice of a wider buffer: ld = V + 8 keeps a 16-bit row in the register form, ld = V + 4 sends it to the generic kernel.
    Columns [V, ld) and a guard row on either side hold a bit pattern and must hold it afterwards."""
    run_ce(dev, dtype, V, strided(extra), seed=3, where="ld=V+%d" % extra)


def test_ce_16bit_misaligned_base(dev, both_halves):
    run_ce(dev, h16(), 4096, misaligned, seed=4, where="base%16=8")


@pytest.mark.parametrize("V", [4096, 30000])
@pytest.mark.parametrize("dtype", DT)
def test_ce_gain(dev, dtype, V):
    """MlmHeadFn's call: gain = 256 M on the IEEE-half build (the softmax part would vanish below its subnormals), 1 on the others.
    The reference scales by the same power of two; nothing else changes."""
    run_ce(dev, dtype, V, seed=5, gain=256.0 * R.CE_M if dtype == torch.float16 else 1.0)


def test_ce_refuses_bad_arguments_without_a_launch(dev):
    from ecamp_amd import _lib
    o, lib = ops(), _lib.load()
    x = torch.full((8, 16), 7.0, dtype=h16(), device=dev)        # large enough for any (M, V, ld) below, were one of them launched
    labels = torch.zeros(4, dtype=torch.int64, device=dev)
    w = torch.ones(4, device=dev)
    loss = torch.full((1,), 7.0, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = o.stream()
    for (M, V, ld, code), msg in (((4, 6, 8, 1), b"multiples of 4"), ((4, 8, 10, 1), b"multiples of 4"), ((4, 8, 4, 1), b"ld >= V > 0"),
                                  ((4, 0, 8, 1), b"ld >= V > 0"), ((4, -4, 8, 1), b"ld >= V > 0"), ((4, 8, 8, 2), b"dtype 2"),
                                  ((4, 8, 8, -1), b"dtype -1")):
        rc = lib.ecamp_ce_fwd_bwd(p(x), p(labels), p(w), p(loss), M, V, ld, 0.25, code, s)
        assert rc != 0 and msg in lib.ecamp_last_error(), (M, V, ld, code, lib.ecamp_last_error())
    for args in ((None, p(labels), p(w), p(loss)), (p(x), None, p(w), p(loss)), (p(x), p(labels), None, p(loss)), (p(x), p(labels), p(w), None)):
        rc = lib.ecamp_ce_fwd_bwd(*args, 4, 8, 8, 0.25, 1, s)
        assert rc != 0 and b"null pointer" in lib.ecamp_last_error()
    assert lib.ecamp_ce_fwd_bwd(p(x), p(labels), p(w), p(loss), 0, 8, 8, 0.25, 1, s) == 0          # no rows: nothing to do, no launch
    empty = torch.empty(0, 8, dtype=h16(), device=dev)
    o.ce_fwd_bwd_(empty, labels[:0], w[:0], loss)
    torch.cuda.synchronize()
    assert float(loss.item()) == 7.0 and bool((x == 7).all())      # nothing ran
    with pytest.raises(_lib.EcampHipError, match="CPU tensor"):
        o.ce_fwd_bwd_(x.cpu(), labels.cpu(), w.cpu(), loss.cpu())
    with pytest.raises(TypeError):
        o.ce_fwd_bwd_(x[:4, :8].to(torch.float64), labels, w, loss)
    with pytest.raises(AssertionError):
        o.ce_fwd_bwd_(x[:4, ::2], labels, w, loss)                 # stride(1) != 1
    with pytest.raises(AssertionError):
        o.ce_fwd_bwd_(x[:4], labels[:3], w, loss)


# ================================================================================================ BertEmbeddings
EMB_Q = ("z", "mean", "rstd", "e", "gword", "gpos", "gtype", "dgamma", "dbeta")


def run_emb(dev, dtype, shape, variant="plain", p=0.0):
    o, fmt = ops(), R.fmt_of(dtype)
    c = R.emb_case(shape, fmt, variant, p)
    seed, offset = 4242, 5
    d = lambda t: t.to(dev)
    keep = o.dropout_mask((c.B * c.S, c.H), dev, p, seed, offset).cpu() if p else None
    e, z, mean, rstd = o.bert_embed_fwd(d(c.ids), d(c.ty), d(c.word), d(c.pos), d(c.typ), d(c.gamma), d(c.beta), R.EMB_EPS, dtype,
                                        drop_p=p, seed=seed, offset=offset)
    buf = {q: d(t).clone() for q, t in c.prior.items()}
    o.bert_embed_bwd(d(c.de).to(dtype), z, mean, rstd, d(c.gamma), d(c.ids), d(c.ty), buf["gword"], buf["gpos"], buf["gtype"], buf["dgamma"],
                     buf["dbeta"], c.B, c.S, c.H, drop_p=p, seed=seed, offset=offset, pad_id=c.pad_id, hot=c.hot)
    torch.cuda.synchronize()
    got = dict(z=z.cpu(), mean=mean.cpu(), rstd=rstd.cpu(), e=e.cpu(), **{q: t.cpu() for q, t in buf.items()})
    if p:
        kept = float(keep.float().mean())
        assert 0.8 < kept < 0.97, kept
    tag = "embed %s %s %s%s (fwd y=%d, bwd y=%d)" % (fmt, shape, variant, " p=%.1f" % p if p else "", R.emb_fwd_grid_y(c.B), R.emb_bwd_grid_y(c.B))
    lines, bad = R.emb_judge(tag, c, got, got["z"].float(), keep, EMB_Q)
    print("\n".join(lines))
    assert not bad, "\n".join(bad)
    return c, got


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape", list(R.EMB_SHAPES))
@pytest.mark.parametrize("dtype", DT)
def test_bert_embeddings(dev, dtype, shape, p):
    """Every template rung (IT = 1..4), partial last trips, one active lane, the forward's grid cap and second trip, and the backward
    with its batch split over 2 and 8 workgroups per position (the position row through atomics): z, mean, rstd, e and the five
    accumulated gradients, with and without dropout under the kernels' own keep-mask."""
    run_emb(dev, dtype, shape, p=p)


@pytest.mark.parametrize("variant", ["hot03", "nohot", "type0"])
@pytest.mark.parametrize("dtype", DT)
def test_bert_embeddings_hot_and_pad_guards(dev, dtype, variant):
    """hot = (0, 3) with PAD 0: the guard hot0 != pad_id keeps the PAD row at its prior contents.  hot = (2, 3) that no token carries:
    rows 2 and 3 are not touched.  Every token of type 0: the type-1 row is not touched."""
    c, got = run_emb(dev, dtype, "6x5x768", variant)
    same = lambda q, row: torch.equal(got[q][row].view(torch.int32), c.prior[q][row].view(torch.int32))
    assert same("gword", c.pad_id)
    if variant == "nohot":
        assert same("gword", 2) and same("gword", 3)
    if variant == "type0":
        assert same("gtype", 1) and not same("gtype", 0)


def test_bert_embeddings_refuse_bad_arguments_without_a_launch(dev):
    from ecamp_amd import _lib
    o, lib = ops(), _lib.load()
    B, S, H = 2, 2, 1028
    seven = lambda *shape, dtype=torch.float32: torch.full(shape, 7.0, dtype=dtype, device=dev)
    ids, ty = torch.ones(B, S, dtype=torch.int64, device=dev), torch.zeros(B, S, dtype=torch.int64, device=dev)
    word, pos, typ, gamma, beta = seven(4, H), seven(S, H), seven(2, H), seven(H), seven(H)
    z, e, de = seven(B * S, H, dtype=h16()), seven(B * S, H, dtype=h16()), seven(B * S, H, dtype=h16())
    mean, rstd = seven(B * S), seven(B * S)
    gword, gpos, gtype, dgamma, dbeta = seven(4, H), seven(S, H), seven(2, H), seven(H), seven(H)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    s = o.stream()

    def fwd(cols, z_=z):
        return lib.ecamp_bert_embed_fwd(p(ids), p(ty), p(word), p(pos), p(typ), p(gamma), p(beta), p(z_), p(e), p(mean), p(rstd), B, S, cols,
                                        1e-12, 0.0, 0, 0, 1, s)

    def bwd(cols, gpos_=gpos):
        return lib.ecamp_bert_embed_bwd(p(de), p(z), p(mean), p(rstd), p(gamma), p(ids), p(ty), p(gword), p(gpos_), p(gtype), p(dgamma), p(dbeta),
                                        B, S, cols, 0, 2, 3, 0.0, 0, 0, 1, s)
    for f in (fwd, bwd):
        for cols in (1028, 6):
            assert f(cols) != 0 and b"multiple of 4 and <= 1024" in lib.ecamp_last_error()
        assert f(768, None) != 0 and b"null pointer" in lib.ecamp_last_error()
    torch.cuda.synchronize()
    for t in (word, pos, typ, gamma, beta, z, e, de, mean, rstd, gword, gpos, gtype, dgamma, dbeta):
        assert bool((t == 7).all())      # nothing ran
