"""Held-out evaluation, measured (profiles/eval_pass.txt):

  1  the head's loss kernel alone at the benchmark's row count: `ecamp_ce_eval` against `ecamp_ce_fwd_bwd` on the same bf16 logits
     [M = 32768, V = 30000], every row labelled and at the reference's masking rate (15 % of the rows labelled, the rest -100).
     HIP events around each launch, the two kernels alternating in one loop, the logits restored (untimed) in front of every launch.
  2  one `engine_pretrain.evaluate` pass at B = 256, S = 128 over batches resident in HBM, in pairs/s, beside the forward-only protocol
     of `bench.py --full` (`forward` under no_grad, training mode, the same batch) and `forward_eval` on its own.

    python tools/eval_bench.py [--iters 20] [--batches 12] [--dtype bf16|fp16]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ms_of(pairs):
    return [a.elapsed_time(b) for a, b in pairs]


def bench_kernel(dev, dtype, iters, M=32768, V=30000):
    from ecamp_amd import hip_ops as ops
    g = torch.Generator(device="cpu").manual_seed(0)
    src = (torch.randn(1024, V, generator=g) * 3).to(dev, dtype).repeat(M // 1024, 1)
    work = torch.empty_like(src)
    w = torch.rand(M, generator=g).to(dev) * 2
    full = torch.randint(0, V, (M,), generator=g)
    sparse = torch.where(torch.rand(M, generator=g) < 0.15, full, torch.full_like(full, -100))
    nbytes = src.numel() * src.element_size()
    print("1  loss kernel alone: %s logits [%d, %d] = %.2f GB" % (str(dtype).split(".")[-1], M, V, nbytes / 1e9))
    print("   %-34s %10s %10s %10s %12s" % ("kernel / labels", "median us", "min us", "max us", "GB/s moved"))
    for name, labels in (("every row labelled", full), ("15 %% of the rows labelled (%d)" % int((sparse >= 0).sum()), sparse)):
        lab = labels.to(dev)
        scored = int((labels >= 0).sum())
        t = {"ce_fwd_bwd": [], "ce_eval": []}
        for i in range(iters + 3):
            for kind in ("ce_fwd_bwd", "ce_eval"):
                work.copy_(src)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if kind == "ce_eval":
                    ops.ce_eval(work, lab, w)      # (its two small memsets are inside the bracket: they are part of the call)
                else:
                    s = ops.zeros((1,), dev)
                    ops.ce_fwd_bwd_(work, lab, w, s)
                b.record()
                if i >= 3:
                    t[kind].append((a, b))
        torch.cuda.synchronize()
        moved = {"ce_fwd_bwd": 2 * nbytes, "ce_eval": nbytes * scored / M}   # read + write of every row; one read of the labelled rows
        for kind in ("ce_fwd_bwd", "ce_eval"):
            us = [1e3 * v for v in ms_of(t[kind])]
            med = statistics.median(us)
            print("   %-34s %10.1f %10.1f %10.1f %12.0f" % (kind + ", " + name.split(" (")[0], med, min(us), max(us), moved[kind] / med / 1e3))
        e, f = statistics.median(ms_of(t["ce_eval"])), statistics.median(ms_of(t["ce_fwd_bwd"]))
        print("   -> ce_eval takes %.2f x the time of ce_fwd_bwd (%s)" % (e / f, name))


def bench_pass(dev, dtype, nb, B=256, S=128):
    from ecamp_amd.data import synthetic_batch
    from ecamp_amd.engine_pretrain import evaluate
    from ecamp_amd.module import model_ecamp as me
    torch.manual_seed(0)
    model = me.ecamp(compute_dtype=dtype).to(dev)
    model.train()
    two = [synthetic_batch(B, S, 448, seed=s, device=dev) for s in (0, 1)]
    g = torch.Generator().manual_seed(7)
    held_out = []
    for b in two:
        keep = (torch.rand(B, S, generator=g) < 0.15).to(dev)
        held_out.append(dict(b, labels=torch.where(keep, b["labels"], torch.full_like(b["labels"], -100))))
    args = argparse.Namespace(mask_ratio=0.75, prefetch=False)

    def timed(fn, n):
        fn(2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    def fwd_no_grad(n):    # bench.py --full's `fwd_only_*`
        with torch.no_grad():
            for i in range(n):
                model(two[i % 2])

    def fwd_eval(batches):
        def run(n):
            for i in range(n):
                model.forward_eval(batches[i % 2])
        return run

    rows = [("forward, no_grad, training mode (bench.py fwd_only protocol)", timed(fwd_no_grad, nb)),
            ("forward_eval, every row labelled", timed(fwd_eval(two), nb)),
            ("forward_eval, 15 % of the rows labelled", timed(fwd_eval(held_out), nb))]
    loader = [held_out[i % 2] for i in range(nb)]
    evaluate(model, loader[:2], dev, 0, args=args)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = evaluate(model, loader, dev, 0, args=args)      # ends in its own read-back
    dt = (time.perf_counter() - t0) / nb
    rows.append(("evaluate(): %d batches, 15 %% labelled, one read-back at the end" % nb, dt))
    print("2  one pass at B = %d, S = %d, %s, batches resident in HBM (host clock around work that ends in a synchronise)" % (B, S, str(dtype).split(".")[-1]))
    print("   %-66s %10s %10s" % ("", "ms/batch", "pairs/s"))
    for name, d in rows:
        print("   %-66s %10.3f %10.0f" % (name, 1e3 * d, B / d))
    print("   evaluate() returned", stats)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/eval_bench.py measures on an MI355X; there is nothing to time without one")
    from ecamp_amd import _lib
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    _lib.set_half(dt)
    d = torch.device("cuda:0")
    print("device:", torch.cuda.get_device_name(0))
    bench_kernel(d, dt, a.iters)
    torch.cuda.empty_cache()
    bench_pass(d, dt, a.batches)
