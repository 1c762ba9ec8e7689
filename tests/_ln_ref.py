"""The LayerNorm kernels of csrc/norm.hip in plain torch on the CPU: what tests/test_ln_float64_gpu.py holds ecamp_layernorm_fwd /
ecamp_layernorm_bwd and ecamp_layernorm_fwd_x32 / ecamp_layernorm_bwd_z32 to, element by element, and what
tests/test_ln_reference_cpu.py proves about it without a GPU.  The method is that of tests/_sr_ref.py and tests/_report_ref.py, whose
k_of, bound_k, U, TINY, stored and fmt_of are used as they are: every element is judged by |got - ref| <= K u A (+ TINY) with
  ref  float64 on the values the kernel was given (eps included: the float32 value the entry receives),
  A    the same arithmetic on magnitudes, no minus signs (ln_rows of _report_ref.py: the graph the embedding kernel is held to),
  u    half a rounding of the format the quantity is stored in: the row format for y, z, dz and dx_drop, f32 for mean, rstd, dgamma, dbeta,
  K    max(1, 4 K_yard), K_yard the largest err / (u A) of the yardstick on the same inputs; no fixed tolerance anywhere.

    z       = x keep / (1 - p) + res                  A = |x| / (1 - p) + |res|           (the fused entry only; else z is x itself)
    everything else takes the STORED z the kernel returned as its input, so that the rounding of z is not charged twice:
    mu = mean(z), d = z - mu, rs = (mean(d^2) + eps)^-1/2, xh = d rs, y = xh gamma + beta
    g = dy gamma, dz = rs (g - mean(g) - xh mean(g xh)) + dres                            A: + |dres|
    dgamma = prior + n sum_r dy xh, dbeta = prior + n sum_r dy  (n calls into one buffer)  A: |prior| + n sum_r of the magnitudes
    dx_drop = stored(dz) keep / (1 - p): an exact product rounded once, judged against the dz the kernel stored.  A dropped element
    is a structural zero; with p == 0 dx_drop must be dz bit for bit.
  A == 0 marks a structural zero: the element must compare equal to zero (a row whose dy is all zero, without dres).

Yardstick: the same arithmetic in float32 on the CPU, rounded to the format where the kernels store 16 bits.  dgamma and dbeta leave
the kernels through one float atomic per column and workgroup, at most 256 workgroups: the yardstick splits the rows into at most 256
groups (row r in group r mod 256), chains each group's rows in float32, then chains the groups onto the prior contents in ORDERS orders
(order 0 as they stand, the others seeded), of which the worst counts.  Never torch's pairwise sum of all rows: it sits closer to
float64 than any such chain can (the docstring of tests/test_sr_head_gpu.py).

Regimes (each generator asserts its own defining property):
  plain    2 N(0,1) + 0.3, as the older tests have it.
  offset   mean far above spread: 2048 + N(0,1) for f32 rows and the f32 stream; 4 + N(0,1) / 4 for 16-bit rows.  The second has
           |mean| / std = 16 in expectation only, so a row whose sample spread exceeds 0.85 / 4 is shrunk to it; every row of the
           stored values then has |mean| / std >= 16.
  scales   row r of x, res and dres times 2^k, k = (5 r mod 13) - 6: every k of -6..6 in 13 rows, neighbours at least five binades
           apart.  dy is scaled by 2^2k: rs goes with 2^-k, so row r of dz (and of dx_drop, z, dres) is again 2^k times an
           unscaled row, and an error confined to a 2^-6 row is 2^-12 of the tensor's maximum.
  special  row 0 is constant (every element 2^-3: the row sum is exact in any order, so mean must be the constant and y must be
           stored(beta), both bit for bit; rstd = eps^-1/2 is judged like any other); the last row's dy is all zero (dz == 0 without
           dres); gamma has one zero column and negative entries.  With one row, that row is both.
  dgamma / dbeta start from nonzero prior contents in every regime."""
import functools

import torch

from _report_ref import BF16, DTYPE, F16, F32, TINY, U, fmt_of, ln_rows, stored  # noqa: F401
from _sr_ref import bound_k, k_of  # noqa: F401

ORDERS = 4
GROUPS = 256
EPS, EPS_BERT = 1e-6, 1e-12
DROP_P, DROP_SEED, DROP_OFFSET = 0.1, 987654321, 17
CONST = 2.0 ** -3

BWD_CAP, BWD_WAVES = 256, 16
R_BIG = 2 * BWD_CAP * BWD_WAVES + 5        # three trips of every backward form's row loop: the middle one consumes a prefetch and issues one
SMALL_ROWS = (1, 5)
COLS = (4, 8, 196, 264, 512, 520, 768, 776, 1024, 1032, 2048)
MISALIGNED_COLS = (264, 776)
FUSED_COLS = (264, 768, 776)
REGIMES = ("plain", "offset", "scales", "special")
STREAM_REGIMES = ("offset", "scales", "special")
# R_BIG once per backward instantiation, at the smallest column count that reaches it, and at the production width: (cols, misaligned)
BIG_16 = [(196, False), (264, False), (264, True), (520, False), (776, False), (776, True), (1032, False), (768, False)]
BIG_32 = [(196, False), (264, False), (520, False), (776, False), (1032, False), (768, False)]


def eps_given(eps):
    """The value the entry receives: eps as a float32."""
    return float(torch.tensor(eps, dtype=torch.float32))


# ================================================================================================ the layout selection, restated
def ln_layout(backward, rows16, cols, al16=True, opt_bwd=0):
    """ln_select of csrc/norm.hip -> (vec, chunks, waves, greg, lds, grid_cap); ecamp_layernorm_layout must agree for every case."""
    cdiv = lambda a, b: -(-a // b)
    wide = bool(rows16) and cols % 8 == 0 and bool(al16)
    it8, it4 = cdiv(cols // 8, 64), cdiv(cols // 4, 64)
    chunks4 = 1 if it4 <= 1 else it4 if it4 <= 4 else 8
    if not backward:
        return (8, 1 if it8 <= 1 else 2 if it8 <= 2 else 4, 4, True, 0, 0) if wide else (4, chunks4, 4, True, 0, 0)
    slices = 8 * cols * 4
    if wide and opt_bwd != 1 and cols <= 1024:
        if it8 <= 1:
            return (8, 1, 16, True, slices, BWD_CAP)
        if opt_bwd == 2 or cols > 768:
            return (8, 2, 12, False, 9 * cols * 4, BWD_CAP)
    return (4, chunks4, 16, True, slices, BWD_CAP)


# The instantiation every case is MEANT to reach, written down by hand: {(rows16, misaligned): {cols: ((vec, chunks) forward,
# (vec, chunks, waves, greg) backward)}}.  test_ln_reference_cpu.py holds the mirror above to it, the GPU test holds the library to the mirror.
_W16, _W12 = (16, True), (12, False)
INTENDED = {
    (True, False): {4: ((4, 1), (4, 1) + _W16), 8: ((8, 1), (8, 1) + _W16), 196: ((4, 1), (4, 1) + _W16), 264: ((8, 1), (8, 1) + _W16),
                    512: ((8, 1), (8, 1) + _W16), 520: ((8, 2), (4, 3) + _W16), 768: ((8, 2), (4, 3) + _W16), 776: ((8, 2), (8, 2) + _W12),
                    1024: ((8, 2), (8, 2) + _W12), 1032: ((8, 4), (4, 8) + _W16), 2048: ((8, 4), (4, 8) + _W16)},
    (True, True): {264: ((4, 2), (4, 2) + _W16), 776: ((4, 4), (4, 4) + _W16)},
    (False, False): {4: ((4, 1), (4, 1) + _W16), 8: ((4, 1), (4, 1) + _W16), 196: ((4, 1), (4, 1) + _W16), 264: ((4, 2), (4, 2) + _W16),
                     512: ((4, 2), (4, 2) + _W16), 520: ((4, 3), (4, 3) + _W16), 768: ((4, 3), (4, 3) + _W16), 776: ((4, 4), (4, 4) + _W16),
                     1024: ((4, 4), (4, 4) + _W16), 1032: ((4, 8), (4, 8) + _W16), 2048: ((4, 8), (4, 8) + _W16)},
}


def intended(rows16, cols, misaligned=False):
    """-> ((vec, chunks) of the forward, (vec, chunks, waves, greg) of the backward) the case is meant to reach."""
    return INTENDED[(bool(rows16), bool(misaligned))][cols]


def trips(rows, waves, cap=BWD_CAP):
    """Trips of the busiest wave through the backward's row loop, and the rows of the last trip."""
    stride = min(cap, -(-rows // waves)) * waves
    n = -(-rows // stride)
    return n, rows - (n - 1) * stride


# ================================================================================================ inputs
def scale_k(rows):
    return (5 * torch.arange(rows)) % 13 - 6


def _base(rows, cols, fmt, zfmt, g):
    rn = lambda *s: torch.randn(*s, generator=g)
    d = dict(x=stored(rn(rows, cols) * 2 + 0.3, zfmt), res=stored(rn(rows, cols), fmt), dy=stored(rn(rows, cols), fmt),
             dres=stored(rn(rows, cols), fmt), gamma=1 + 0.1 * rn(cols), beta=0.1 * rn(cols), prior_g=0.5 * rn(cols), prior_b=0.5 * rn(cols))
    assert (d["prior_g"] != 0).all() and (d["prior_b"] != 0).all()
    return d


def gen_plain(rows, cols, fmt, zfmt, g):
    return _base(rows, cols, fmt, zfmt, g)


def gen_offset(rows, cols, fmt, zfmt, g):
    d = _base(rows, cols, fmt, zfmt, g)
    n = torch.randn(rows, cols, generator=g)
    if zfmt == F32:
        d["x"] = 2048.0 + n
    else:
        n = n / 4
        s = n.std(1, unbiased=False, keepdim=True)
        d["x"] = stored(4.0 + n * (0.85 / 4 / s.clamp_min(1e-30)).clamp_max(1.0), zfmt)
    x = d["x"].double()
    assert (x.mean(1).abs() >= 16 * x.std(1, unbiased=False)).all(), "offset: a row with |mean| / std < 16"
    return d


def gen_scales(rows, cols, fmt, zfmt, g):
    d = _base(rows, cols, fmt, zfmt, g)
    k = scale_k(rows)
    s = (2.0 ** k.double()).float()[:, None]
    base_x = d["x"]
    d["x"], d["res"], d["dres"], d["dy"] = stored(d["x"] * s, zfmt), stored(d["res"] * s, fmt), stored(d["dres"] * s, fmt), stored(d["dy"] * s * s, fmt)
    assert torch.equal(d["x"], stored(base_x * s, zfmt)) and torch.isfinite(d["dy"]).all()
    assert len(set(k.tolist())) == min(rows, 13) and int(k.min()) >= -6 and int(k.max()) <= 6 and int(k[0]) == -6
    assert rows == 1 or int((k[1:] - k[:-1]).abs().min()) >= 5, "scales: neighbouring rows less than five binades apart"
    return d


def gen_special(rows, cols, fmt, zfmt, g):
    d = _base(rows, cols, fmt, zfmt, g)
    d["x"][0] = CONST
    d["dy"][rows - 1] = 0.0
    d["gamma"][2::5] = -d["gamma"][2::5]
    d["gamma"][1] = 0.0
    assert (d["x"][0] == CONST).all() and float(stored(torch.tensor(CONST), zfmt)) == CONST and (d["dy"][rows - 1] == 0).all()
    assert int((d["gamma"] == 0).sum()) == 1 and (d["gamma"] < 0).any() and (d["gamma"] > 0).any()
    return d


GENERATORS = dict(plain=gen_plain, offset=gen_offset, scales=gen_scales, special=gen_special)


class LnCase:
    """One case on the host.  fmt: the format of the 16-bit-or-f32 rows (y, res, dy, dres, dz); stream: the LayerNorm input is f32
    beside 16-bit rows (ecamp_layernorm_fwd_x32 / ecamp_layernorm_bwd_z32)."""

    def __init__(self, fmt, regime, rows, cols, stream=False):
        assert not (stream and fmt == F32) and cols % 4 == 0
        self.fmt, self.zfmt, self.regime, self.rows, self.cols, self.stream = fmt, F32 if stream else fmt, regime, rows, cols, stream
        g = torch.Generator().manual_seed(1000003 * REGIMES.index(regime) + 9176 * rows + cols)
        for k, v in GENERATORS[regime](rows, cols, fmt, self.zfmt, g).items():
            setattr(self, k, v)
        for t, f in ((self.x, self.zfmt), (self.res, fmt), (self.dy, fmt), (self.dres, fmt)):
            assert torch.equal(stored(t, f), t) and torch.isfinite(t).all()

    @functools.lru_cache(maxsize=2)
    def graph_x(self, eps):
        """The graph on x itself (the entries without a fused residual: z is x)."""
        return Graph(self, self.x, eps)


@functools.lru_cache(maxsize=2)
def case(fmt, regime, rows, cols, stream=False):
    return LnCase(fmt, regime, rows, cols, stream)


# ================================================================================================ z of the fused entry
def p_given(p):
    """The value the entry receives: p as a float32."""
    return float(torch.tensor(p, dtype=torch.float32))


def keep_scale(keep, p, dt):
    """keep / (1 - p) in `dt`; in float32 as the kernels form it, 1.0f / (1.0f - p) times the mask.  keep None: no dropout."""
    if keep is None:
        assert p == 0.0
        return torch.ones((), dtype=dt)
    one = torch.ones((), dtype=torch.float32)
    inv = one / (one - torch.tensor(p, dtype=torch.float32)) if dt == torch.float32 else torch.tensor(1.0 / (1.0 - p_given(p)), dtype=dt)
    return keep.to(dt) * inv


def z_reference(c, keep, p):
    """-> (x keep / (1 - p) + res in float64, |x| / (1 - p) + |res|)."""
    x, res = c.x.double(), c.res.double()
    return x * keep_scale(keep, p, torch.float64) + res, x.abs() * (1.0 / (1.0 - p_given(p))) + res.abs()


def z_float32(c, keep, p):
    return stored(c.x * keep_scale(keep, p, torch.float32) + c.res, c.fmt)


def _line(tag, q, ky, k, K):
    return "  %-52s %-7s K_yard %7.3f   kernel %7.3f   bound %6.2f" % (tag, q, ky, k, K)


def _held(tag, q, got, yard, ref, A, fmt, lines, bad):
    """One quantity: K_yard (the worst of the yardstick's leading dimension when it has one more than ref), the figure of `got`, the
    bound; finite; structural zeros."""
    u, tiny = U[fmt], TINY[fmt]
    g = got.double().reshape(ref.shape)
    ky = k_of(yard.double(), ref, A, u, allowance=tiny)
    k, K = k_of(g, ref, A, u, allowance=tiny), bound_k(ky)
    lines.append(_line(tag, q, ky, k, K))
    if not k <= K:
        bad.append("%s %s: err / (u A) = %.3f > %.2f (yardstick %.3f)" % (tag, q, k, K, ky))
    if not torch.isfinite(g).all():
        bad.append("%s %s: not finite" % (tag, q))
    zero = A == 0
    if zero.any() and not (g[zero] == 0).all():
        bad.append("%s %s: %d structurally zero elements are not zero" % (tag, q, int((g[zero] != 0).sum())))


def judge_z(tag, c, got_z, keep, p):
    """z of the fused entry as the kernel stored it -> (lines, violations)."""
    lines, bad = [], []
    ref, A = z_reference(c, keep, p)
    _held(tag, "z", got_z, z_float32(c, keep, p), ref, A, c.fmt, lines, bad)
    return lines, bad


# ================================================================================================ everything downstream of the stored z
def chain_groups(part, prior, times=1, orders=ORDERS, seed=17, first_as_is=True):
    """part [rows, cols], prior [cols], float32 -> [orders, cols]: the rows in at most GROUPS groups (row r in group r mod GROUPS), each
    group's rows added one after the other, then the groups added one after the other onto the prior contents, `times` times over
    (calls into one buffer: every group of a call lands before any of the next), one rounding per addition (torch.cumsum on the CPU
    accumulates float32 in double).  Order 0 takes the groups as they stand, the others are seeded permutations."""
    assert part.dtype == torch.float32 and prior.dtype == torch.float32
    rows, cols = part.shape
    G = min(GROUPS, rows)
    T = -(-rows // G)
    P = torch.zeros(T * G, cols, dtype=torch.float32)
    P[:rows] = part
    P = P.view(T, G, cols)
    acc = P[0].clone()
    for t in range(1, T):
        acc = acc + P[t]
    gen = torch.Generator().manual_seed(seed)
    out = prior.clone()[None].repeat(orders, 1)
    for _ in range(times):
        perms = torch.stack([torch.arange(G) if (o == 0 and first_as_is) else torch.randperm(G, generator=gen) for o in range(orders)])
        for i in range(G):
            out = out + acc[perms[:, i]]
    return out


class Graph:
    """Reference, magnitudes and yardstick of everything downstream of one stored z [rows, cols] (float32 values, exact in the z format)."""

    def __init__(self, c, z, eps):
        self.c, self.eps = c, eps_given(eps)
        assert z.dtype == torch.float32 and z.shape == (c.rows, c.cols) and torch.equal(stored(z, c.zfmt), z)
        self.z = z
        one = lambda dt: torch.ones((), dtype=dt)
        self.r = ln_rows(z, c.dy, c.gamma, c.beta, self.eps, one(torch.float64), torch.float64)
        self.a = ln_rows(z, c.dy, c.gamma, c.beta, self.eps, one(torch.float64), torch.float64, magnitudes=True)
        self.y32 = ln_rows(z, c.dy, c.gamma, c.beta, self.eps, one(torch.float32), torch.float32)

    # ---- reference and magnitude of one quantity
    def ref(self, q, dres=False, times=1):
        c, r, a = self.c, self.r, self.a
        if q == "y":
            return r["e"], a["e"]
        if q in ("mean", "rstd"):
            return r[q], a[q]
        if q == "dz":
            return (r["dz"] + c.dres.double(), a["dz"] + c.dres.double().abs()) if dres else (r["dz"], a["dz"])
        prior = (c.prior_g if q == "dgamma" else c.prior_b).double()
        return prior + times * r[q].sum(0), prior.abs() + times * a[q].sum(0)

    # ---- the yardstick of one quantity (dgamma, dbeta: [ORDERS, cols])
    def yard(self, q, dres=False, times=1, seed=None):
        """seed: another set of chaining orders for dgamma / dbeta, none of them the groups as they stand."""
        c, y = self.c, self.y32
        if q == "y":
            return stored(y["e"], c.fmt)
        if q in ("mean", "rstd"):
            return y[q]
        if q == "dz":
            return stored(y["dz"] + c.dres if dres else y["dz"], c.fmt)
        prior = c.prior_g if q == "dgamma" else c.prior_b
        return chain_groups(y[q], prior, times) if seed is None else chain_groups(y[q], prior, times, seed=seed, first_as_is=False)

    def yard_outputs(self, dres=False, times=1, keep=None, p=0.0):
        """What a kernel that is the yardstick would return: every quantity, dgamma / dbeta in order 0."""
        out = {q: self.yard(q, dres, times) for q in ("y", "mean", "rstd", "dz")}
        out["dgamma"], out["dbeta"] = self.yard("dgamma", dres, times)[0], self.yard("dbeta", dres, times)[0]
        out["dx_drop"] = stored(out["dz"] * keep_scale(keep, p, torch.float32), self.c.fmt)
        return out


def judge(tag, G, got, dres=False, times=1, keep=None, p=0.0):
    """The quantities of `got` (host tensors, as the kernels stored them; any of y, mean, rstd, dz, dx_drop, dgamma, dbeta; dx_drop
    needs dz beside it) -> (printed lines, violations)."""
    c, lines, bad = G.c, [], []
    for q in ("y", "mean", "rstd", "dz", "dgamma", "dbeta"):
        if q in got:
            ref, A = G.ref(q, dres, times)
            _held(tag, q, got[q], G.yard(q, dres, times), ref, A, c.fmt if q in ("y", "dz") else F32, lines, bad)
    if "dx_drop" in got:
        dzs = got["dz"].float()
        ks = keep_scale(keep, p, torch.float64)
        ref = dzs.double() * ks
        _held(tag, "dx_drop", got["dx_drop"], stored(dzs * keep_scale(keep, p, torch.float32), c.fmt), ref, ref.abs(), c.fmt, lines, bad)
        if p == 0.0 and not torch.equal(got["dx_drop"].float().view(torch.int32), dzs.view(torch.int32)):
            bad.append("%s dx_drop: differs from dz in its bits with p == 0" % tag)
    if c.regime == "special":
        assert (G.z[0] == CONST).all()
        if "mean" in got and float(got["mean"][0]) != CONST:
            bad.append("%s mean: the constant row's mean is %r, not %r" % (tag, float(got["mean"][0]), CONST))
        if "y" in got and not torch.equal(got["y"][0].float(), stored(c.beta, c.fmt)):
            bad.append("%s y: the constant row is not stored(beta) bit for bit" % tag)
        if "dz" in got and not dres and not (got["dz"][c.rows - 1] == 0).all():
            bad.append("%s dz: the row whose dy is zero is not zero" % tag)
    return lines, bad
