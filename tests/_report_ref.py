"""The report-side training kernels of csrc/text.hip in plain torch on the CPU: what tests/test_report_kernels_gpu.py holds
ecamp_ce_fwd_bwd and ecamp_bert_embed_fwd / ecamp_bert_embed_bwd to, element by element, and what tests/test_report_reference_cpu.py
proves about it without a GPU.  The method is that of tests/_sr_ref.py: every element is judged by |got - ref| <= K u A with
  ref  float64 on the values the kernel was given,
  A    the same arithmetic on magnitudes: the sum of the absolute values of every term that reaches the element,
  u    half a rounding of the format the quantity is stored in (U below; f32 for every sum, statistic and table gradient),
  K    max(1, 4 K_yard), K_yard the largest err / (u A) of a yardstick on the same inputs (bound_k of _sr_ref), never a fixed number.

Weighted cross-entropy over [M, V] logits, w_i = 0 for a label outside [0, V), c = gain / M:
    ref[i, j] = c w_i (p_ij - [j == label_i])      A[i, j] = c w_i (p_ij + [j == label_i])      p = softmax of the row
    loss = sum_i w_i (lse_i - x_i[label_i])        A    = sum_i w_i (|lse_i| + |x_i[label_i]|)
  A row with w_i == 0 is structurally zero: every element must compare equal to zero.  Yardsticks: a 16-bit gradient is the float64
  gradient rounded once to the format; the f32 gradient is the same formula in float32 (exp(x - max) / sum); the loss is a float32
  CHAIN of the float32 per-row terms -- the kernels leave through one float atomic per row, and torch's pairwise sums sit closer to
  float64 than any such chain can (see the docstring of tests/test_sr_head_gpu.py) -- in row order and in 15 seeded orders, of which
  the worst counts: the atomics land in no particular order, and the rounding of ONE order of 37 terms is a single draw (row order
  alone gave K_yard between 0.05 and 1.7 over the cases, and a kernel figure of 1.14 met a bound of 1.00 in one run and passed in the
  next).  Half of the format's smallest
  subnormal is allowed on top of K u A: it matters for IEEE half without `gain` only, where most of the softmax part lies below 2^-14.

BertEmbeddings, rows r = b S + s, z = word[id] + type[ty] + pos[s] stored in the activation format:
    z     against the float64 sum of the three table rows, A = the sum of their magnitudes.
    everything else takes the STORED z as its input, so that its rounding is not charged twice:
    mu = mean(z), d = z - mu, rs = (mean(d^2) + eps)^-1/2, xh = d rs, e = (xh gamma + beta) keep / (1 - p)
    dd = de keep / (1 - p), g = dd gamma, dz = rs (g - mean(g) - xh mean(g xh))
    dgamma += sum_r dd xh, dbeta += sum_r dd, gpos[s] += sum_b dz, gtype[ty] += dz, gword[id] += dz (id != pad)
  On magnitudes: |z| for z, mean|z| for mu, |z| + mean|z| for d, every product of magnitudes and every sum without a minus sign; rs is a
  positive factor and stays (for rs itself A = rs (1 + mean(|d| d_A) / (var + eps)): what a relative error u of d does to the
  variance).  Every gradient buffer starts from prior contents, which enter ref and A; an element that no row reaches is structurally
  unchanged and must be the prior value bit for bit (the PAD row of gword, a word or a token type that no token uses).  Yardstick: the
  same arithmetic in float32, rounded where the kernels store 16 bits (z, e), the sums over rows chained one row after the other in
  several seeded orders (the worst counts) where the kernel gathers them with float atomics -- gword, gtype, dgamma, dbeta, and gpos
  when ecamp_bert_embed_bwd splits the batch of a position over several workgroups (B >= 64); index_add_ otherwise."""
import functools

import torch

from _sr_ref import bound_k, k_of  # noqa: F401  (K = max(1, 4 K_yard); the largest (|got - ref| - allowance) / (u A))

F32, BF16, F16 = "f32", "bf16", "f16"
DTYPE = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
U = {F32: 2.0 ** -24, BF16: 2.0 ** -9, F16: 2.0 ** -12}
TINY = {F32: 2.0 ** -150, BF16: 2.0 ** -134, F16: 2.0 ** -25}      # half of the smallest subnormal
ORDERS = 4          # row orders of the chained embedding sums
LOSS_ORDERS = 16    # row orders of the chained cross-entropy loss


def fmt_of(dtype):
    return {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}[dtype]


def stored(t, fmt):
    """t rounded to the format, as float32 (exact: every format embeds in float32)."""
    return t.to(DTYPE[fmt]).to(torch.float32)


# ================================================================================================ weighted cross-entropy
CE_M = 37
CE_OFFSET = 256.0      # the common offset of row 10: a power of two, exact in every format
V_REG = [8, 4096, 4104, 8192, 8200, 16384, 16392, 30000, 32768]     # 16-bit rows the register form takes: both sides of every rung
V_GENERIC = [4, 30004, 32776]                                       # 16-bit rows it refuses: V % 8 != 0, V > 32768
V_F32 = [4, 1020, 4100, 30000]


def ce_kernel_of(V, fmt, ld=None, aligned=True):
    """Which kernel ecamp_ce_fwd_bwd launches at its default selection (the conditions of its dispatch, restated)."""
    ld = V if ld is None else ld
    if fmt == F32:
        return "generic<f32>"
    if V % 8 or ld % 8 or V > 32768 or not aligned:
        return "generic<16>"
    return "row<1,512>" if V <= 4096 else "row<2,512>" if V <= 8192 else "row<4,512>" if V <= 16384 else "row<4,1024>"


@functools.lru_cache(maxsize=4)
def ce_case(V, fmt, seed=0):
    """-> (logits f32 [M, V], exact in `fmt`; labels int64 [M]; weights f32 [M]) on the host.  Finite logits only."""
    M = CE_M
    g = torch.Generator().manual_seed(7919 * seed + V)
    x = stored(torch.randn(M, V, generator=g) * 3, fmt)
    labels = torch.randint(0, V, (M,), generator=g)
    w = torch.rand(M, generator=g) * 2 + 0.05
    labels[0], labels[1] = -100, V                       # ignored
    labels[2], labels[3], labels[5] = 0, V - 1, V - 2    # column 0, the last column, inside the last 16-byte group
    labels[9::6] = -100
    w[7], w[20] = 0.0, 0.0                               # scored labels, weight zero
    top = lambda r: float(torch.ceil(x[r].max())) + 30.0     # an integer below 128: exact in every format
    x[4, int(labels[4])] = top(4)                        # the label's logit leads by 30: p ~ 1, cancellation at the label
    x[6, (int(labels[6]) + V // 2) % V] = top(6)         # another column leads by 30: a large loss, every other p ~ e^-30
    x[8] = 1.5                                           # all equal
    x[10] = stored(torch.randn(V, generator=g) * 3 + CE_OFFSET, fmt)
    assert torch.equal(stored(x, fmt), x) and torch.isfinite(x).all()
    return x, labels, w


def ce_reference(x, labels, w, gain=1.0):
    """float64 on the given values -> dict(grad [M, V], loss) x 2: ref and A, and `zero` [M]: the structurally zero rows."""
    M, V = x.shape
    x = x.double()
    valid = (labels >= 0) & (labels < V)
    wv = torch.where(valid, w.double(), torch.zeros((), dtype=torch.float64))
    lse = torch.logsumexp(x, 1)
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x)
    onehot[valid, labels[valid]] = 1.0
    sc = (wv * (gain / M))[:, None]
    xl = x.gather(1, labels.clamp(0, V - 1)[:, None])[:, 0]
    ref = dict(grad=sc * (p - onehot), loss=(wv * (lse - xl)).sum())
    A = dict(grad=sc * (p + onehot), loss=(wv * (lse.abs() + xl.abs())).sum())
    return ref, A, wv == 0


def chain32(terms, orders=LOSS_ORDERS):
    """float32 terms added one after the other, one rounding per addition (torch.cumsum accumulates float32 in double on the CPU), in
    `orders` orders -> [orders]: order 0 is the terms as they stand, the others are seeded permutations."""
    terms = terms.to(torch.float32)
    g = torch.Generator().manual_seed(13)
    P = torch.stack([terms] + [terms[torch.randperm(terms.numel(), generator=g)] for _ in range(orders - 1)])
    acc = torch.zeros(orders, dtype=torch.float32)
    for t in range(terms.numel()):
        acc = acc + P[:, t]
    return acc


def ce_float32(x, labels, w, gain=1.0):
    """The same formulas in float32 on the CPU -> dict(grad, loss): the yardstick of the f32 gradient and of the loss of every build."""
    M, V = x.shape
    x = x.to(torch.float32)
    valid = (labels >= 0) & (labels < V)
    wv = torch.where(valid, w.to(torch.float32), torch.zeros(()))
    mx = x.max(1, keepdim=True).values
    e = torch.exp(x - mx)
    s = e.sum(1, keepdim=True)
    onehot = torch.zeros_like(x)
    onehot[valid, labels[valid]] = 1.0
    sc = (wv * torch.tensor(gain / M, dtype=torch.float32))[:, None]
    xl = x.gather(1, labels.clamp(0, V - 1)[:, None])[:, 0]
    lse = mx[:, 0] + torch.log(s[:, 0])
    return dict(grad=sc * (e / s - onehot), loss=chain32(wv * (lse - xl)))


def ce_yardsticks(x, labels, w, fmt, gain, ref, A):
    y32 = ce_float32(x, labels, w, gain)
    ygrad = y32["grad"] if fmt == F32 else ref["grad"].to(DTYPE[fmt])
    return dict(grad=k_of(ygrad, ref["grad"], A["grad"], U[fmt], allowance=TINY[fmt]),
                loss=k_of(y32["loss"], ref["loss"], A["loss"], U[F32]))


def ce_judge(tag, fmt, x, labels, w, gain, got_grad, got_loss):
    """-> (printed lines, violations).  got_grad [M, V] as stored by the kernel (any float dtype, on the host), got_loss a number."""
    M, V = x.shape
    ref, A, zero = ce_reference(x, labels, w, gain)
    # on the reference alone: the case can tell a wrong kernel from a right one
    valid = (labels >= 0) & (labels < V)
    assert valid.any() and (~valid).any() and (zero & valid).sum() >= 2 and float(ref["loss"]) > 0
    rows = torch.nonzero(~zero)[:, 0]
    at_label = ref["grad"][rows, labels[rows]].abs()[:, None]
    thin = ref["grad"][rows].abs() < 2.0 ** -10 * at_label
    assert thin.any(), "no off-label gradient below 2^-10 of its row's label entry: max|err| / max|ref| would do"
    ky = ce_yardsticks(x, labels, w, fmt, gain, ref, A)
    got = dict(grad=got_grad.double(), loss=torch.as_tensor(float(got_loss), dtype=torch.float64))
    lines, bad = [], []
    for q, u, tiny in (("grad", U[fmt], TINY[fmt]), ("loss", U[F32], None)):
        k, K = k_of(got[q], ref[q], A[q], u, allowance=tiny), bound_k(ky[q])
        lines.append("  %-46s %-5s K_yard %7.3f   kernel %7.3f   bound %6.2f" % (tag, q, ky[q], k, K))
        if not k <= K:
            bad.append("%s %s: err / (u A) = %.3f > %.2f (yardstick %.3f)" % (tag, q, k, K, ky[q]))
    if not torch.isfinite(got["grad"]).all():
        bad.append("%s grad: not finite" % tag)
    if not (got["grad"][zero] == 0).all():
        bad.append("%s grad: %d non-zero elements in rows without a weight" % (tag, int((got["grad"][zero] != 0).sum())))
    return lines, bad


# ================================================================================================ BertEmbeddings
EMB_WORDS = 50
EMB_EPS = 1e-12
#             B   S  cols
EMB_SHAPES = {
    "6x5x768":    (6, 5, 768),      # IT = 3, the backward owns its position row
    "70x3x260":   (70, 3, 260),     # fwd gridDim.y capped at 16 + a second trip; B % 4 != 0; bwd gridDim.y = 2; IT = 2, one lane in the last trip
    "260x2x64":   (260, 2, 64),     # bwd gridDim.y = 8 (its cap), nine trips; IT = 1, 48 of 64 lanes idle
    "9x4x1024":   (9, 4, 1024),     # IT = 4, full width
    "5x3x4":      (5, 3, 4),        # one active lane per wave
    "33x2x512":   (33, 2, 512),     # IT = 2 full; bwd gridDim.y = 1 with a ragged last trip
}
EMB_VARIANTS = ("plain", "hot03", "nohot", "type0")


def emb_bwd_grid_y(B):
    return max(1, min(8, B // 32))


def emb_fwd_grid_y(B):
    return min(16, (B + 3) // 4)


def ln_rows(z, de, gamma, beta, eps, sc, dt, magnitudes=False):
    """The LayerNorm row arithmetic of the docstring above on z [R, H] in `dt` (shared with tests/_ln_ref.py, where sc == 1):
    -> dict(mean, rstd [R]; e, dgamma, dbeta, dz [R, H], the parameter gradients per row).  sc: the keep-mask scale on e and de.
    magnitudes: the same on absolute values (rs from the values themselves)."""
    z, de, g, b = z.to(dt), de.to(dt), gamma.to(dt), beta.to(dt)
    H = z.shape[1]
    mu = z.sum(1, keepdim=True) / H
    d = z - mu
    var = (d * d).sum(1, keepdim=True) / H
    rs = 1.0 / torch.sqrt(var + eps)
    if not magnitudes:
        xh = d * rs
        dd = de * sc
        gg = dd * g
        dz = rs * (gg - gg.sum(1, keepdim=True) / H - xh * ((gg * xh).sum(1, keepdim=True) / H))
        return dict(mean=mu[:, 0], rstd=rs[:, 0], e=(xh * g + b) * sc, dgamma=dd * xh, dbeta=dd, dz=dz)
    muA = z.abs().sum(1, keepdim=True) / H
    dA = z.abs() + muA
    xhA = dA * rs
    ddA = de.abs() * sc
    ggA = ddA * g.abs()
    dzA = rs * (ggA + ggA.sum(1, keepdim=True) / H + xhA * ((ggA * xhA).sum(1, keepdim=True) / H))
    rsA = rs * (1.0 + (d.abs() * dA).sum(1, keepdim=True) / H / (var + eps))
    return dict(mean=muA[:, 0], rstd=rsA[:, 0], e=(xhA * g.abs() + b.abs()) * sc, dgamma=ddA * xhA, dbeta=ddA, dz=dzA)


class EmbCase:
    """One embedding case on the host.  variant: plain -- hot ids (2, 3), PAD 0; hot03 -- hot ids (0, 3), PAD 0 (the guard hot0 != pad);
    nohot -- hot ids (2, 3) that no token carries; type0 -- every token of type 0."""

    def __init__(self, shape, fmt, variant="plain", p=0.0, seed=0):
        B, S, H = EMB_SHAPES[shape]
        self.shape, self.fmt, self.variant, self.p, self.B, self.S, self.H = shape, fmt, variant, p, B, S, H
        self.pad_id, self.hot = 0, (0, 3) if variant == "hot03" else (2, 3)
        g = torch.Generator().manual_seed(100 * seed + B)
        ids = torch.randint(4, EMB_WORDS, (B, S), generator=g)
        ids[::2, 0] = 2
        ids[1::3, S - 1] = 3
        ids[4::5, S - 1] = 0                         # PAD tails
        if S > 2:
            ids[4::10, S - 2] = 0
        ids[0, 1], ids[1, 1], ids[3, 0] = 7, 7, 7    # one ordinary id twice at a position and at two positions: colliding atomics
        if variant == "nohot":
            ids[ids == 2], ids[ids == 3] = 12, 13
        ty = (torch.rand(B, S, generator=g) < 0.3).long()
        ty[0, 0], ty[1, 0] = 0, 1
        if variant == "type0":
            ty.zero_()
        self.ids, self.ty = ids, ty
        rn = lambda *s: torch.randn(*s, generator=g)
        self.word, self.pos, self.typ = rn(EMB_WORDS, H) * 0.5, rn(S, H) * 0.5, rn(2, H) * 0.5
        self.gamma, self.beta = 1 + 0.1 * rn(H), 0.1 * rn(H)
        self.de = stored(rn(B * S, H), fmt)
        self.prior = dict(gword=rn(EMB_WORDS, H) * 0.5, gpos=rn(S, H) * 0.5, gtype=rn(2, H) * 0.5, dgamma=rn(H) * 0.5, dbeta=rn(H) * 0.5)
        assert all((t != 0).all() for t in self.prior.values())
        flat = ids.reshape(-1)
        has = lambda v: bool((flat == v).any())
        assert has(0) and has(7) and (variant == "nohot") != has(2) and (variant == "nohot") != has(3)
        assert (ids[:, 1] == 7).sum() >= 2 and (ids[:, 0] == 7).any()
        assert variant == "type0" or (bool((ty == 0).any()) and bool((ty == 1).any()))

    # ---- where every row's dz goes: destination row per buffer, -1 = nowhere -------------------------------------------------------
    def dest(self):
        R = self.B * self.S
        ids, ty = self.ids.reshape(-1), self.ty.reshape(-1)
        s = torch.arange(R) % self.S
        return dict(gword=torch.where(ids == self.pad_id, torch.full_like(ids, -1), ids), gpos=s, gtype=ty,
                    dgamma=torch.zeros(R, dtype=torch.int64), dbeta=torch.zeros(R, dtype=torch.int64))

    def untouched(self):
        """Per buffer, bool like the buffer: the elements no row reaches."""
        out = {}
        for q, d in self.dest().items():
            n = self.prior[q].shape[0] if self.prior[q].dim() == 2 else 1
            hit = torch.zeros(n, dtype=torch.bool)
            hit[d[d >= 0]] = True
            out[q] = (~hit)[:, None].expand(n, self.H).reshape(self.prior[q].shape)
        return out

    def z_reference(self):
        """-> (float64 sum of the three table rows [B S, H], the sum of their magnitudes)."""
        ids, ty = self.ids.reshape(-1), self.ty.reshape(-1)
        s = torch.arange(ids.numel()) % self.S
        a, t, p = self.word.double()[ids], self.typ.double()[ty], self.pos.double()[s]
        return a + t + p, a.abs() + t.abs() + p.abs()

    def z_float32(self):
        ids, ty = self.ids.reshape(-1), self.ty.reshape(-1)
        s = torch.arange(ids.numel()) % self.S
        return stored((self.word[ids] + self.typ[ty]) + self.pos[s], self.fmt)

    def _scale(self, keep, dt):
        if keep is None:
            assert self.p == 0.0
            return torch.ones((), dtype=dt)
        return keep.reshape(self.B * self.S, self.H).to(dt) / (1.0 - self.p)

    def rows(self, z, keep, dt, magnitudes=False):
        """The per-row arithmetic on the stored z in `dt` -> dict(mean, rstd, e, dgamma, dbeta, dz), the last three per row [R, H].
        magnitudes: the same on absolute values (rs from the values themselves)."""
        return ln_rows(z, self.de, self.gamma, self.beta, EMB_EPS, self._scale(keep, dt), dt, magnitudes)

    def _gather(self, rows, dt, magnitudes=False, chained=()):
        """prior + the sum of every row's share, per buffer.  chained: the buffers whose rows are added one after the other in `dt`, in
        ORDERS seeded orders -> [ORDERS, ...]; the others by index_add_."""
        out = {}
        for q, d in self.dest().items():
            prior = self.prior[q].to(dt)
            prior = (prior.abs() if magnitudes else prior).reshape(-1, self.H)
            part = rows[q if q in ("dgamma", "dbeta") else "dz"]
            use = torch.nonzero(d >= 0)[:, 0]
            if q in chained:
                gen = torch.Generator().manual_seed(11)
                accs = []
                for o in range(ORDERS):
                    acc = prior.clone()
                    order = use if o == 0 else use[torch.randperm(use.numel(), generator=gen)]
                    for r, k in zip(order.tolist(), d[order].tolist()):
                        acc[k] += part[r]                 # one rounding per addition
                    accs.append(acc)
                out[q] = torch.stack(accs).reshape((ORDERS,) + self.prior[q].shape)
            else:
                out[q] = prior.clone().index_add_(0, d[use], part[use]).reshape(self.prior[q].shape)
        return out

    def reference(self, z, keep):
        """float64 on the stored z -> (ref, A): mean, rstd [R], e [R, H] and the five buffers (prior contents included)."""
        r, a = self.rows(z, keep, torch.float64), self.rows(z, keep, torch.float64, magnitudes=True)
        ref, A = {q: r[q] for q in ("mean", "rstd", "e")}, {q: a[q] for q in ("mean", "rstd", "e")}
        ref.update(self._gather(r, torch.float64))
        A.update(self._gather(a, torch.float64, magnitudes=True))
        return ref, A

    def chained(self):
        return ("gword", "gtype", "dgamma", "dbeta") + (("gpos",) if emb_bwd_grid_y(self.B) > 1 else ())

    def float32(self, z, keep):
        """The yardstick: the same in float32, e rounded to the format, the atomically gathered sums chained."""
        r = self.rows(z, keep, torch.float32)
        y = dict(mean=r["mean"], rstd=r["rstd"], e=stored(r["e"], self.fmt))
        y.update(self._gather(r, torch.float32, chained=self.chained()))
        return y


@functools.lru_cache(maxsize=8)
def emb_case(shape, fmt, variant="plain", p=0.0):
    return EmbCase(shape, fmt, variant, p)


EMB_UNIT = dict(z=None, e=None)     # None: the activation format; every other quantity is f32


def emb_judge(tag, c, got, z_stored, keep, quantities):
    """-> (lines, violations) for the `quantities` of `got` (host tensors).  z is judged against the tables, the rest against the
    reference on `z_stored`."""
    lines, bad = [], []
    ref, A = c.reference(z_stored, keep)
    ref["z"], A["z"] = c.z_reference()
    y = c.float32(z_stored, keep)
    y["z"] = c.z_float32()
    untouched = c.untouched()
    for q in quantities:
        fmt = c.fmt if q in EMB_UNIT else F32
        u, tiny = U[fmt], TINY[fmt]
        g = got[q].double().reshape(ref[q].shape)
        ky = k_of(y[q].double(), ref[q], A[q], u, allowance=tiny)
        k, K = k_of(g, ref[q], A[q], u, allowance=tiny), bound_k(ky)
        lines.append("  %-46s %-6s K_yard %7.3f   kernel %7.3f   bound %6.2f" % (tag, q, ky, k, K))
        if not k <= K:
            bad.append("%s %s: err / (u A) = %.3f > %.2f (yardstick %.3f)" % (tag, q, k, K, ky))
        if not torch.isfinite(g).all():
            bad.append("%s %s: not finite" % (tag, q))
        if q in untouched:
            same = got[q].reshape(c.prior[q].shape).view(torch.int32) == c.prior[q].view(torch.int32)
            n = int((~same & untouched[q]).sum())
            if n:
                bad.append("%s %s: %d elements that no row reaches differ from their prior contents" % (tag, q, n))
    return lines, bad
