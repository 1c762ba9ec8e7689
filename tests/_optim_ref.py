"""Float64 restatements of the optimizer-side kernels (csrc/optim.hip) and the inputs the optimizer tests drive them with.

A plain helper module, not a test file: tests/test_optim_reference_cpu.py proves what is here against torch (float64 torch.optim.AdamW,
torch._amp_update_scale_) without a GPU, tests/test_optim_elementwise_gpu.py holds the kernels to it.

Every hyper-parameter is rounded to float32 ONCE, here, before anybody uses it: the C ABI takes `float`, so the kernel, the float64
reference and the float32 yardstick then all start from the same real numbers and what is compared is arithmetic, not the rounding of 0.9.
"""
import math
import types

import numpy as np
import torch


def f32(x):
    """The float32 nearest to x, as a Python float."""
    return float(np.float32(x))


B1, B2, EPS = f32(0.9), f32(0.95), f32(1e-8)   # main_pretrain.py: AdamW(betas=(0.9, 0.95)), torch's default eps

# The param_groups of the trajectory: (lr_scale, weight_decay).  Between them: wd = 0 and wd = 0.05 (timm's decay / no-decay split), a
# scaled lr (layer decay), lr = 0 (a group that is frozen by its schedule but still gathers moments).  Neighbouring indices differ in wd
# (0 / 1) and in lr (2 / 3, 3 / 4), so that a coefficient read from the wrong slot moves something.
GROUP_LR_SCALE = (1.0, 1.0, 0.65, 0.0, 0.1)
GROUP_WD = (f32(0.05), 0.0, f32(0.05), f32(0.05), 0.0)
NGROUPS = len(GROUP_WD)
BEYOND = 6      # a table byte < 8 but >= NGROUPS: the ABI zero-fills those slots, so lr = wd = 0 -- moments move, the parameter does not
FROZEN = 255    # a table byte >= 8: the block is not read and not written
EDGE = 8        # the smallest byte that means "untouched"


def group_lrs(step, total, peak=6e-4, min_lr=1e-6, warmup=10):
    """The per-group learning rates of optimizer step `step` (1-based) of `total`: util/lr_sched.py's warm-up + half cosine, written into
    the groups the way it writes them (lr * lr_scale), then rounded to float32."""
    from ecamp_amd.util import lr_sched
    groups = [{"lr": 0.0, "lr_scale": s} for s in GROUP_LR_SCALE]
    args = types.SimpleNamespace(lr=peak, min_lr=min_lr, warmup_epochs=float(warmup), max_epoch=float(max(total, warmup + 1)))
    lr_sched.adjust_learning_rate(types.SimpleNamespace(param_groups=groups), float(step), args)
    return [f32(g["lr"]) for g in groups]


def make_table(nblocks, seed):
    """uint8[nblocks]: the group of every 64-element block.  Runs of odd length (so that group boundaries fall on 64-element blocks that are
    not multiples of the 16-block = 1024-element span of one thread block), cycling through every group, with runs of frozen blocks, one run
    of a group index beyond NGROUPS and one of the edge byte 8."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor([1, 3, 5, 7, 11, 13, 21, 37, 53, 101])
    cycle = [0, 1, FROZEN, 2, 3, 0, 4, FROZEN, 1, BEYOND, 2, EDGE, 4, 3]
    out = torch.empty(nblocks, dtype=torch.uint8)
    pos, k = 0, 0
    while pos < nblocks:
        n = int(lens[int(torch.randint(0, len(lens), (1,), generator=g))])
        if nblocks > 100000:
            n *= 97    # the 21 M-element arena: still odd, still off the thread-block span, but not thirty thousand runs
        out[pos:pos + n] = cycle[k % len(cycle)]
        pos, k = pos + n, k + 1
    assert k >= len(cycle), "the table is too short to hold every kind of run"
    return out


def element_groups(table):
    return table.repeat_interleave(64)


def make_params(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.02


def make_magnitudes(n, seed, zero_stride=7):
    """Signed per-element gradient magnitudes, log-uniform over 1e-12 ... 1e2, exact zeros every `zero_stride` elements.

    The SIGN belongs to the element, not to the step (make_grad varies the size only).  The optimizer tests measure m relative to |m|
    per element; with a fresh sign every step m is a cancelling sum, its relative rounding error is 1 / (how close to zero it happened to
    land), and the largest of 2.6e5 such numbers says nothing about a kernel.  A parameter that is pushed one way is the common case in
    training, too."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(10.0, torch.rand(n, generator=g, dtype=torch.float64) * 14.0 - 12.0).float()
    mag = mag * (torch.randint(0, 2, (n,), generator=g).float() * 2.0 - 1.0)
    mag[::zero_stride] = 0.0
    return mag


def make_grad(mag, seed, step):
    """The float32 gradient of `step`: magnitude * (0.25 + U[0, 1))."""
    g = torch.Generator().manual_seed(seed * 100003 + step)
    return mag * (torch.rand(mag.numel(), generator=g) + 0.25)


def plant_nonfinite(g, table):
    """Put a NaN at the first element of the first frozen block and an inf at the last element of the last one: a kernel that so much as
    reads them into its sum of squares shows it."""
    fr = (table >= 8).nonzero().flatten()
    assert fr.numel() >= 2
    g[int(fr[0]) * 64] = float("nan")
    g[int(fr[-1]) * 64 + 63] = float("inf")
    return g


# ------------------------------------------------------------------------------------------------ grouped AdamW in float64
def ref_adamw_grouped(p, g, m, v, table, lrs, wds, b1, b2, eps, step, gscale, chunk=1 << 21):
    """What csrc/optim.hip documents, in float64, in place on the float64 tensors p, m, v (g: any float dtype, read only):

        g' = g * gscale;  p *= 1 - lr wd;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)

    with bc1 = 1 - b1^step, bc2 = 1 - b2^step and (lr, wd) those of the block's table byte (zero for a byte >= len(lrs)); blocks whose byte
    is >= 8 are untouched and their gradient is not looked at.  Returns sum(g'^2) over the updated blocks.  Works through the arena in
    chunks so that a 21 M-element case does not hold a dozen float64 temporaries of that size."""
    assert p.dtype == m.dtype == v.dtype == torch.float64 and p.numel() % 64 == 0 and chunk % 64 == 0
    assert table.numel() * 64 == p.numel() and len(lrs) == len(wds) <= 8
    bc1, sqrt_bc2 = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    lr_of, wd_of = torch.zeros(256, dtype=torch.float64), torch.zeros(256, dtype=torch.float64)
    lr_of[:len(lrs)] = torch.tensor(lrs, dtype=torch.float64)
    wd_of[:len(wds)] = torch.tensor(wds, dtype=torch.float64)
    total = 0.0
    for a in range(0, p.numel(), chunk):
        b = min(p.numel(), a + chunk)
        gi = table[a // 64:b // 64].long().repeat_interleave(64)
        upd = gi < 8
        lr, wd = lr_of[gi], wd_of[gi]
        gs = torch.where(upd, g[a:b].double() * gscale, torch.zeros((), dtype=torch.float64))
        total += float((gs * gs).sum())
        pn = p[a:b] * (1.0 - lr * wd)
        mn = b1 * m[a:b] + (1.0 - b1) * gs
        vn = b2 * v[a:b] + (1.0 - b2) * gs * gs
        pn = pn - lr / bc1 * mn / (vn.sqrt() / sqrt_bc2 + eps)
        p[a:b] = torch.where(upd, pn, p[a:b])
        m[a:b] = torch.where(upd, mn, m[a:b])
        v[a:b] = torch.where(upd, vn, v[a:b])
    return total


class TorchGroupedAdamW:
    """torch.optim.AdamW (the single-tensor CPU implementation) over the same arena and table: one parameter tensor per table byte < 8,
    gathered from the arena.  In float64 it is what ref_adamw_grouped is proven against; in float32 it is the rounding yardstick of the
    kernel tests -- a second, independent float32 implementation of the same step."""

    def __init__(self, p0, table, wds, b1, b2, eps, dtype):
        gi = element_groups(table)
        self.dtype, self.n, self.items = dtype, p0.numel(), []
        groups = []
        for k in sorted(set(table.unique().tolist())):
            if k >= 8:
                continue
            idx = (gi == k).nonzero().flatten()
            prm = p0[idx].to(dtype).clone().requires_grad_(True)
            groups.append({"params": [prm], "lr": 0.0, "weight_decay": wds[k] if k < len(wds) else 0.0})
            self.items.append((k, idx, prm))
        self.opt = torch.optim.AdamW(groups, lr=0.0, betas=(b1, b2), eps=eps, weight_decay=0.0, foreach=False)

    def step(self, g, lrs, gscale=1.0):
        for (k, idx, prm), grp in zip(self.items, self.opt.param_groups):
            prm.grad = g[idx].to(self.dtype) * gscale
            grp["lr"] = lrs[k] if k < len(lrs) else 0.0
        self.opt.step()

    def arena(self, p0):
        """-> (p, m, v) scattered back into arena order, float64; untouched elements keep p0 and zero moments."""
        p, m, v = p0.double().clone(), torch.zeros(self.n, dtype=torch.float64), torch.zeros(self.n, dtype=torch.float64)
        for k, idx, prm in self.items:
            st = self.opt.state[prm]
            p[idx], m[idx], v[idx] = prm.detach().double(), st["exp_avg"].double(), st["exp_avg_sq"].double()
        return p, m, v


REL_TINY = 1e-30   # |ref| + REL_TINY in the relative distances of m and v: 2^24 float32-subnormal steps, so that the ABSOLUTE granularity of
                   # a subnormal v (g = 1e-12 squared and decayed) does not pose as a relative error; nothing normal is affected


def distances(p, m, v, ref, sel):
    """max |p - p_ref| (absolute) and max |x - x_ref| / (|x_ref| + REL_TINY) for m and v, over the elements `sel`; all float64."""
    pr, mr, vr = ref
    dp = (p[sel] - pr[sel]).abs().max().item()
    dm = ((m[sel] - mr[sel]).abs() / (mr[sel].abs() + REL_TINY)).max().item()
    dv = ((v[sel] - vr[sel]).abs() / (vr[sel].abs() + REL_TINY)).max().item()
    return dp, dm, dv


# ------------------------------------------------------------------------------------------------ the device-side GradScaler in float64
def _isfinite32(x):
    return bool(np.isfinite(np.float32(x)))


def ref_scaler_step(sumsq, state, opt_step, growth, backoff, interval, b1, b2):
    """One ecamp_loss_scale_update.  `state` = (scale, growth tracker, skipped steps), `opt_step` = AdamW steps taken so far; all Python
    floats holding float32 values.  -> (state', opt_step', ctl, norm) where ctl = [1 / scale, skip flag, bc1, rsqrt_bc2] with None in the
    two slots a skipped step leaves untouched, bc1 and rsqrt_bc2 in float64 (the kernel rounds them to float32 once), and norm =
    sqrt(sumsq) / scale in float64.

    The scale arithmetic is float32 (numpy), like torch._amp_update_scale_'s: back-off multiplies, growth multiplies only when the tracker
    reaches the interval and only if the product is finite, and the tracker restarts either way."""
    scale, tracker, skipped = state
    found = not _isfinite32(sumsq)
    with np.errstate(all="ignore"):
        s32, sc32 = np.float32(sumsq), np.float32(scale)
        inv = float(np.float32(1.0) / sc32)
        norm = float(np.sqrt(np.float64(s32))) / scale if scale != 0.0 else float("nan")
        if found:
            new = (float(sc32 * np.float32(backoff)), 0.0, skipped + 1.0)
            return new, opt_step, [inv, 1.0, None, None], norm
        ok = tracker + 1.0
        if ok == float(interval):
            grown = sc32 * np.float32(growth)
            new = (float(grown) if np.isfinite(grown) else scale, 0.0, skipped)
        else:
            new = (scale, ok, skipped)
    step = opt_step + 1.0
    return new, step, [inv, 0.0, 1.0 - b1 ** step, 1.0 / math.sqrt(1.0 - b2 ** step)], norm


def sumsq_sequence(n, seed, p_bad=0.15):
    """n float32 `sumsq` values: mostly finite (1e-3 ... 1e9), with inf, -inf and nan mixed in at probability p_bad."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.pow(10.0, torch.rand(n, generator=g, dtype=torch.float64) * 12.0 - 3.0).float().tolist()
    kind = torch.rand(n, generator=g).tolist()
    bad = [float("inf"), float("-inf"), float("nan")]
    which = torch.randint(0, 3, (n,), generator=g).tolist()
    return [bad[w] if k < p_bad else x for x, k, w in zip(vals, kind, which)]


def ulp32(x):
    """The spacing of float32 at |x| (x a float64 value inside float32's normal range)."""
    return float(np.spacing(np.float32(abs(x))))
