"""Float64 restatement of the fused fine-tuning step (csrc/finetune.hip: ecamp_sumsq_grouped + ecamp_sgd_grouped) and the inputs its tests use.

A plain helper module, not a test file: tests/test_finetune_cpu.py proves `clip_sgd_step` against torch.nn.utils.clip_grad_norm_ +
torch.optim.SGD on the CPU, tests/test_finetune_kernels_gpu.py holds the kernels to it.  Hyper-parameters are rounded to float32 once,
here (the C ABI takes `float`), so the kernel, this reference and the float32 yardstick start from the same real numbers.
"""
import numpy as np
import torch

FROZEN = 255    # a table byte >= 8: the block is neither read nor written


def f32(x):
    """The float32 nearest to x, as a Python float."""
    return float(np.float32(x))


MOMENTUM = f32(0.9)
GROUP_LR = (f32(3e-2), f32(1e-2), f32(5e-2))
GROUP_WD = (f32(1e-4), 0.0, f32(5e-2))


def block_table(nblk, seed=0):
    """uint8 [nblk]: groups 0..2 in runs, with runs of FROZEN blocks in between (also the first and the last block of a run boundary)."""
    rng = np.random.RandomState(seed)
    t = np.empty(nblk, dtype=np.uint8)
    i = 0
    while i < nblk:
        run = int(rng.randint(1, 5))
        t[i:i + run] = FROZEN if rng.rand() < 0.25 else rng.randint(0, 3)
        i += run
    t[1], t[nblk // 2] = FROZEN, FROZEN
    t[0], t[2], t[nblk - 1] = 0, 1, 2      # (nblk >= 6: every group and a frozen block occur)
    return torch.from_numpy(t)


def element_groups(table):
    """int64 [64 * nblk]: the group of every element."""
    return table.to(torch.int64).repeat_interleave(64)


def clip_sgd_step(p, g, buf, table, lrs, wds, momentum, max_norm, grad_scale=1.0):
    """One step in the dtype of `p` (float64: the reference; float32: the yardstick), in place on p and buf -> (norm, coef).
    norm = sqrt(sum of g^2 over the live blocks) * grad_scale; coef = min(1, max_norm / (norm + 1e-6)) when max_norm > 0;
    d = g * grad_scale * coef + wd * p; buf = momentum * buf + d; p -= lr * buf.  Blocks of a group >= 8 are left alone."""
    eg = element_groups(table)
    live = eg < 8
    dt = p.dtype
    norm = torch.sqrt((g[live].to(dt) ** 2).sum()) * grad_scale
    coef = min(1.0, max_norm / (float(norm) + 1e-6)) if max_norm > 0 else 1.0
    lr = torch.tensor(list(lrs) + [0.0] * 8, dtype=dt)[eg.clamp(max=8)]
    wd = torch.tensor(list(wds) + [0.0] * 8, dtype=dt)[eg.clamp(max=8)]
    d = g.to(dt) * grad_scale * coef + wd * p
    nb = momentum * buf + d
    buf[live] = nb[live]
    p[live] = (p - lr * nb)[live]
    return float(norm), coef


def torch_clip_sgd(p0, grads, table, lrs, wds, momentum, max_norm, dtype):
    """The same steps by torch itself on the CPU in `dtype`: one parameter per group over the live elements (clip_grad_norm_ over all of
    them, then torch.optim.SGD with per-group lr / weight decay) -> (p, buf, norms, coefs) scattered back to the flat layout; frozen
    elements keep p0 and a zero buffer."""
    eg = element_groups(table)
    ng = len(lrs)
    params = [p0[eg == k].to(dtype).clone().requires_grad_(True) for k in range(ng)]
    opt = torch.optim.SGD([{"params": [q], "lr": lrs[k], "weight_decay": wds[k]} for k, q in enumerate(params)], lr=1.0, momentum=momentum)
    norms, coefs = [], []
    for g in grads:
        for k, q in enumerate(params):
            q.grad = g[eg == k].to(dtype).clone()
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm) if max_norm > 0 else torch.sqrt(sum((q.grad ** 2).sum() for q in params))
        norms.append(float(norm))
        coefs.append(min(1.0, max_norm / (float(norm) + 1e-6)) if max_norm > 0 else 1.0)
        opt.step()
    p, buf = p0.to(dtype).clone(), torch.zeros_like(p0, dtype=dtype)
    for k, q in enumerate(params):
        p[eg == k] = q.detach()
        buf[eg == k] = opt.state[q]["momentum_buffer"]
    return p, buf, norms, coefs


def trajectory(n, steps=4, seed=0):
    """(p0 f32 [n], [g_1 .. g_steps] f32): gradients whose norm shrinks from step to step, so that one max_norm clips the first steps
    and not the last."""
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (0.5 ** s) for s in range(steps)]
    return p0, grads
