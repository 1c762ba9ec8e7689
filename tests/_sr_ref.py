"""The super-resolution head of csrc/vision.hip (K12) in plain torch on the CPU: what tests/test_sr_head_gpu.py holds the four kernels
to, element by element, and what tests/test_sr_reference_cpu.py proves about it without a GPU.

    u  = bilinear x2 (p), align_corners=False          z1 = conv1(u),      c1 = relu(z1)
    z2 = conv2(c1) + u,   s = relu(z2)                 loss = sum_window (s - big)^2
    window of sample b: rows [column_b, column_b + win) x columns [row_b, row_b + win) of 32-px super-patches, clipped by the image
    dsr = d(0.5 loss)/dp,  gw = {dW1[81], db1[3], dW2[81], db2[3]} of 0.5 loss      (the kernels' order)

Three forms of that graph:
  * `graph`     -- autograd, float64: THE reference.  With absolute=True it runs on |p|, |w|, |b|, |big| without the ReLUs and with
                   s + |big| in the loss: every output is then the sum of the absolute values of every term that reaches it, the
                   magnitude `A` an error is judged by (|got - ref| <= K u A); A == 0 marks a structurally zero output.
  * `model`     -- the same arithmetic with the backward written out (ds, dc1, du, the transposed bilinear filter, the 168 sums per
                   32 x 32 tile), so that a rounding can be put where the mode-1 kernels have one: u, c1, ds, dc1 and the tap weights
                   in the library's 16-bit format; the skip connection, the loss and every accumulation stay unrounded.
  * `model` in float32 with no rounding -- the yardstick of the mode-0 kernels.  Its sums (loss, gw) are formed per tile and then
                   chained one tile after the other in float32, in several seeded orders, the worst of which counts: the kernels add one
                   partial per workgroup into one float with atomics, and a pairwise sum (what torch's own reductions do) is closer to
                   float64 than any such chain can be.
K = max(1, RATIO * K_yard) per quantity, K_yard the yardstick's largest err / (u A) on the same inputs; the floor is one rounding of
the magnitude sum."""
import functools

import torch
import torch.nn.functional as F

SRT = 32          # a tile = one super-patch of the high-resolution image
RATIO = 4.0       # as in test_optim_elementwise_gpu.py: the kernels order their sums differently from the yardstick
U32 = 2.0 ** -24
U16 = {"bf16": 2.0 ** -9, "f16": 2.0 ** -12}
CAP_FWD, CAP_BWD0, CAP_BWD1 = 2048, 1024, 512    # grid caps of ecamp_sr_fwd / ecamp_sr_image, ecamp_sr_bwd mode 0, mode 1
EXCLUDED_SHARE_CAP = 0.02
ORDERS = 8        # tile orders of the float32 chain

#           name            B   R   win  (column, row) per sample, or None = seeded      what is checked
SHAPES = {
    "one-tile-w1":   (4, 16, 1, [(0, 0)] * 4, ("fwd", "bwd")),
    "one-tile-w3":   (4, 16, 3, [(0, 0)] * 4, ("fwd", "bwd")),
    "ring-w1":       (6, 48, 1, [(0, 0), (1, 1), (2, 2), (0, 1), (2, 1), (1, 0)], ("fwd", "bwd")),
    "ring-w2":       (6, 48, 2, [(0, 0), (1, 1), (2, 2), (0, 1), (2, 1), (1, 0)], ("fwd", "bwd")),
    "production":    (3, 224, 12, [(0, 0), (2, 2), (1, 2)], ("fwd", "bwd")),
    "pair-bwd-trips":  (16, 96, 2, None, ("fwd", "bwd")),
    "fused-bwd-trips": (29, 96, 2, None, ("bwd",)),
    "fwd-trips":       (57, 96, 2, None, ("fwd",)),
}


def geometry(shape):
    """-> B, R, win, column [B], row [B] (int64), what.  Seeded windows always hold (2, 2) and the clipped (5, 5)."""
    B, R, win, windows, what = SHAPES[shape]
    G = 2 * R // SRT
    if windows is None:
        cr = torch.randint(0, G, (B, 2), generator=torch.Generator().manual_seed(100 + B))
        cr[0], cr[1] = torch.tensor([2, 2]), torch.tensor([G - 1, G - 1])
    else:
        cr = torch.tensor(windows)
    return B, R, win, cr[:, 0].contiguous(), cr[:, 1].contiguous(), what


def tiles(shape):
    B, R = SHAPES[shape][:2]
    return B * (2 * R // SRT) ** 2


def cursor_steps(grid, G):
    """step_b, step_y, step_x of sr_pair_bwd_kernel's division-free tile cursor."""
    step_b = grid // (G * G)
    step_r = grid - step_b * G * G
    return step_b, step_r // G, step_r % G


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def weights(regime, seed=0):
    """conv1.weight, conv1.bias, conv2.weight, conv2.bias (float32) of a regime.
    open:   every ReLU gate open by a wide margin -- the head is affine and a per-element bound holds everywhere;
    closed: s == 0 everywhere -- every gradient is exactly zero and the loss is sum_window big^2;
    mixed:  the weights of test_kernels_gpu.py (scale 0.3, biases 0.1): about half the gates are closed."""
    w1, b1 = randn((3, 3, 3, 3), seed + 5, 0.3), randn((3,), seed + 6, 0.1)
    w2, b2 = randn((3, 3, 3, 3), seed + 7, 0.3), randn((3,), seed + 8, 0.1)
    if regime == "open":
        b1, w2, b2 = 8.0 + b1, randn((3, 3, 3, 3), seed + 7, 0.05), 12.0 + b2
    elif regime == "closed":
        w2, b2 = torch.zeros(3, 3, 3, 3), torch.full((3,), -40.0)
    else:
        assert regime == "mixed"
    return [w1, b1, w2, b2]


def window_mask(column, row, win, R, dtype=torch.float64):
    """[B, 1, 2R, 2R]: 1 on the loss window of each sample."""
    B, G = column.numel(), 2 * R // SRT
    sm = torch.zeros(B, G, G, dtype=dtype)
    for i in range(B):
        sm[i, int(column[i]):int(column[i]) + win, int(row[i]):int(row[i]) + win] = 1
    return torch.kron(sm, torch.ones(SRT, SRT, dtype=dtype))[:, None]


def up_matrix(R, dtype=torch.float64):
    """[2R, R]: the x2 bilinear filter with align_corners=False along one axis (torch's source-index rule); u = M p M^T."""
    M = torch.zeros(2 * R, R, dtype=torch.float64)
    for Y in range(2 * R):
        src = max((Y + 0.5) * 0.5 - 0.5, 0.0)
        y0 = int(src)
        y1 = min(y0 + 1, R - 1)
        M[Y, y0] += 1.0 - (src - y0)
        M[Y, y1] += src - y0
    return M.to(dtype)       # .25 / .75 / 1: exact in every format


def graph(p, ws, big, mask, dtype=torch.float64, absolute=False, backward=True):
    """The head and its windowed loss by autograd.  -> dict(u, z1, z2, s, loss[, dsr, gw])."""
    cv = (lambda t: t.abs()) if absolute else (lambda t: t)
    p = cv(p.to(dtype)).requires_grad_(backward)
    w1, b1, w2, b2 = [cv(t.to(dtype)).requires_grad_(backward) for t in ws]
    big, mask = cv(big.to(dtype)), mask.to(dtype)
    act = (lambda t: t) if absolute else F.relu
    u = F.interpolate(p, scale_factor=2, mode="bilinear", align_corners=False)
    z1 = F.conv2d(u, w1, b1, padding=1)
    z2 = F.conv2d(act(z1), w2, b2, padding=1) + u
    s = act(z2)
    d = s + big if absolute else s - big
    loss = (mask * d * d).sum()
    out = dict(u=u, z1=z1, z2=z2, s=s, loss=loss)
    if backward:
        (0.5 * loss).backward()
        out.update(dsr=p.grad, gw=torch.cat([w1.grad.reshape(-1), b1.grad, w2.grad.reshape(-1), b2.grad]))
    return {k: v.detach() for k, v in out.items()}


def rounder(half):
    """Round-to-nearest-even to the library's 16-bit format (through float32, as the kernels' own values are); None: no rounding."""
    if half is None:
        return lambda t: t
    h = {"bf16": torch.bfloat16, "f16": torch.float16}[half]
    return lambda t: t.to(torch.float32).to(h).to(t.dtype)


def _per_tile(t):
    B, C, H, W = t.shape
    return t.reshape(B, C, H // SRT, SRT, W // SRT, SRT)


def _corr_tiles(d, x):
    """dW[o][i][ky][kx] = sum d[o](Y, X) x[i](Y + ky - 1, X + kx - 1) (x zero outside the image), per tile: [tiles, 81]."""
    B, _, H, W = d.shape
    G = H // SRT
    xp, dt = F.pad(x, (1, 1, 1, 1)), _per_tile(d)
    out = d.new_zeros(B, G, G, 3, 3, 3, 3)
    for ky in range(3):
        for kx in range(3):
            out[..., ky, kx] = torch.einsum("bogyhx,bigyhx->bghoi", dt, _per_tile(xp[:, :, ky:ky + H, kx:kx + W]))
    return out.reshape(B * G * G, 81)


def _bias_tiles(d):
    return _per_tile(d).sum((3, 5)).permute(0, 2, 3, 1).reshape(-1, 3)


def gw_tiles(ds, dc1, u, c1):
    """[tiles, 168]: every tile's share of {dW1, db1, dW2, db2}."""
    return torch.cat([_corr_tiles(dc1, u), _bias_tiles(dc1), _corr_tiles(ds, c1), _bias_tiles(ds)], 1)


def chain(parts, orders=ORDERS):
    """[tiles, n] -> [orders, n]: the parts added one after the other in their own dtype, tile order 0 as it stands, the others seeded."""
    parts = parts[(parts != 0).any(1)]          # adding an exact zero changes nothing
    T = parts.shape[0]
    g = torch.Generator().manual_seed(7)
    perms = [torch.arange(T)] + [torch.randperm(T, generator=g) for _ in range(orders - 1)]
    P = torch.stack([parts[pm] for pm in perms])
    acc = parts.new_zeros(orders, parts.shape[1])
    for t in range(T):                          # one rounding per addition (torch.cumsum on the CPU accumulates float32 in double)
        acc = acc + P[:, t]
    return acc


def model(p, ws, big, mask, dtype=torch.float64, half=None, backward=True):
    """The head with its backward written out and the mode-1 kernels' roundings (`half`) in place.  loss and gw come back as
    [ORDERS, ...] chains in float32, as plain sums in float64."""
    rnd = rounder(half)
    p, big, mask = p.to(dtype), big.to(dtype), mask.to(dtype)
    w1, b1, w2, b2 = [t.to(dtype) for t in ws]
    w1r, w2r = rnd(w1), rnd(w2)
    M = up_matrix(p.shape[-1], dtype)
    u = M @ p @ M.T
    u16 = rnd(u)
    z1 = F.conv2d(u16, w1r, b1, padding=1)
    c1 = rnd(F.relu(z1))
    z2 = F.conv2d(c1, w2r, b2, padding=1) + u
    s = F.relu(z2)
    total = (lambda parts: chain(parts)) if dtype == torch.float32 else (lambda parts: parts.sum(0))
    out = dict(u=u, z1=z1, z2=z2, s=s, loss=total(_per_tile(mask * (s - big) ** 2).sum((1, 3, 5)).reshape(-1, 1))[..., 0])
    if backward:
        ds = rnd((s - big) * mask * (z2 > 0))
        dc1 = rnd(F.conv_transpose2d(ds, w2r, padding=1) * (z1 > 0))
        du = F.conv_transpose2d(dc1, w1r, padding=1) + ds
        out.update(ds=ds, dc1=dc1, dsr=M.T @ du @ M, gw=total(gw_tiles(ds, dc1, u16, c1)))
    return out


def k_of(got, ref, A, u, keep=None, allowance=None):
    """The largest (|got - ref| - allowance) / (u A) over the elements with A > 0 (and `keep`)."""
    got, ref, A = [torch.as_tensor(t, dtype=torch.float64) for t in (got, ref, A)]
    ref, A = ref.expand_as(got), A.expand_as(got)
    m = (A > 0) if keep is None else (A > 0) & keep
    if not m.any():
        return 0.0
    err = (got - ref).abs()
    if allowance is not None:
        err = (err - allowance).clamp_min(0)
    return float((err[m] / (u * A[m])).max())


def bound_k(k_yard):
    return max(1.0, RATIO * k_yard)


def _dilate(m, r):
    return F.max_pool2d(m, 2 * r + 1, 1, r)


class Host:
    """One case on the host, computed once: inputs (float32, what the kernels get), the float64 reference, the magnitudes A, and the
    yardsticks' K.  u8: the target is uint8 [B, 2R, 2R]; `big` is normalise_u8 of the same bytes."""
    QUANT = ("s", "loss", "dsr", "gw")

    def __init__(self, shape, regime, u8=False, seed=0):
        from ecamp_amd.data import normalise_u8
        self.shape, self.regime = shape, regime
        self.B, self.R, self.win, self.column, self.row, self.what = geometry(shape)
        B, R = self.B, self.R
        self.bwd = "bwd" in self.what
        self.p = randn((B, 3, R, R), seed + 2)
        self.big_u8 = torch.randint(0, 256, (B, 2 * R, 2 * R), generator=torch.Generator().manual_seed(seed + 4), dtype=torch.uint8) if u8 else None
        self.big = normalise_u8(self.big_u8) if u8 else randn((B, 3, 2 * R, 2 * R), seed + 3)
        self.ws = weights(regime, seed)
        self.mask = window_mask(self.column, self.row, self.win, R)
        self.args = (self.p, self.ws, self.big, self.mask)
        self.ref = graph(*self.args, backward=self.bwd)
        self.A = graph(*self.args, absolute=True, backward=self.bwd)
        y32 = model(*self.args, dtype=torch.float32, backward=self.bwd)
        self.k32 = self._yard(y32, U32)
        self.k32["z1"] = k_of(y32["z1"], self.ref["z1"], self.A["z1"], U32)

    def _yard(self, y, u):
        return {q: k_of(y[q], self.ref[q], self.A[q], u) for q in self.QUANT if q in y}

    @functools.lru_cache(maxsize=None)
    def k16(self, half):
        """K_yard of the rounding model in `half`."""
        return self._yard(model(*self.args, half=half, backward=self.bwd), U16[half])

    def margins(self):
        return float(self.ref["z1"].min()), float(self.ref["z2"].min())

    # ---- mixed regime, mode 0: what a gate within rounding of zero may change ---------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def undecided(self):
        """A gate is undecided when |z| <= K u A_z in the float64 reference, K the bound of the forward (s and z1 are computed alike):
        z2 inside the window (where ds is taken), z1 within one pixel of it (where dc1 can be non-zero).  The forward itself needs no
        exclusion -- relu is continuous, an error of z passes into c1 and s at most unchanged -- so sr_image is checked everywhere.
        -> dict(K, z2 [B,3,2R,2R] bool, z1, dsr [B,1,R,R] bool = the dsr elements whose stencil reaches one, share, gw_allowance [168])."""
        K = bound_k(max(self.k32["s"], self.k32["z1"]))
        r, A, m = self.ref, self.A, self.mask
        z2u = (r["z2"].abs() <= K * U32 * A["z2"]) & (m > 0)
        z1u = (r["z1"].abs() <= K * U32 * A["z1"]) & (_dilate(m, 1) > 0)
        # du = ds + conv1^T(dc1), dc1 = [z1 > 0] conv2^T(ds): du sees ds within 2 pixels and the z1 gates within 1; pred pixel y gathers
        # du rows 2y-1 .. 2y+2
        any2, any1 = z2u.any(1, keepdim=True).double(), z1u.any(1, keepdim=True).double()
        bad_du = torch.maximum(_dilate(any2, 2), _dilate(any1, 1))
        bad = F.max_pool2d(bad_du, 4, 2, 1) > 0
        reach = (A["dsr"] > 0).any(1, keepdim=True)
        share = float((bad & reach).sum()) / max(1, int(reach.sum()))
        # a flipped z2 gate changes its ds entry by |s - big| <= |big| + K u A; a flipped z1 gate its dc1 entry by |conv2^T(ds)|.  What
        # these reach in the 168 sums, in absolute values:
        w2 = self.ws[2].double()
        ds_f = z2u * (self.big.double().abs() + K * U32 * A["z2"])
        ds_ref = (r["s"] - self.big.double()) * m * (r["z2"] > 0)
        dc1_f = F.conv_transpose2d(ds_f, w2.abs(), padding=1) + z1u * F.conv_transpose2d(ds_ref, w2, padding=1).abs()
        allow = gw_tiles(ds_f, dc1_f, r["u"].abs(), F.relu(r["z1"])).sum(0)
        return dict(K=K, z2=z2u, z1=z1u, dsr=bad, share=share, gw_allowance=allow)


@functools.lru_cache(maxsize=8)
def host(shape, regime, u8=False):
    return Host(shape, regime, u8)
