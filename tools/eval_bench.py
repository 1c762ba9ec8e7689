"""Held-out evaluation, measured (profiles/eval_pass.txt):

  1  the head's loss kernel alone at the benchmark's row count: `ecamp_ce_eval` against `ecamp_ce_fwd_bwd` on the same bf16 logits
     [M = 32768, V = 30000], every row labelled and at the reference's masking rate (15 % of the rows labelled, the rest -100).
     HIP events around each launch, the two kernels alternating in one loop, the logits restored (untimed) in front of every launch.
  2  one `engine_pretrain.evaluate` pass at B = 256, S = 128 over batches resident in HBM, in pairs/s, beside the forward-only protocol
     of `bench.py --full` (`forward` under no_grad, training mode, the same batch) and `forward_eval` on its own.
  3  masked-token evaluation (profiles/eval_compact.txt; `--leg compact` runs this leg alone): `ecamp_compact_rows` on the head's input
     [32768, 768] against a plain copy of the bytes it moves, and one `evaluate` pass at B = 256, S = 128 on `synthetic_batch` data with
     score "masked", the head compacted and uncompacted, beside the default scope (the pass of part 2) -- the three alternating in one process.

    python tools/eval_bench.py [--iters 20] [--batches 12] [--dtype bf16|fp16] [--leg all|pass|compact]
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


def bench_compact(dev, dtype, iters, nb, rounds=5, B=256, S=128, H=768, V=30000):
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.data import MASK, synthetic_batch
    from ecamp_amd.engine_pretrain import eval_scored_rows, evaluate
    from ecamp_amd.module import model_ecamp as me
    host = [synthetic_batch(B, S, 448, seed=s) for s in (0, 1)]
    hints = [eval_scored_rows(b, "masked", V) for b in host]
    M = B * S
    print("3  masked-token evaluation: synthetic_batch data, B = %d, S = %d: %s of %d positions hold [MASK] under a label" % (B, S, hints, M))
    # a) the gather alone against a copy of the bytes it moves
    g = torch.Generator().manual_seed(3)
    h = torch.randn(M, H, generator=g).to(dev, dtype)
    labels, weights, ids = (host[0][k].to(dev).view(-1) for k in ("labels", "weights", "ids"))
    cap = ops.compact_cap(hints[0])
    src, dst = h[:cap].clone(), torch.empty((cap, H), device=dev, dtype=dtype)
    t = {"compact_rows": [], "copy": []}
    for i in range(iters + 3):
        for kind in ("compact_rows", "copy"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if kind == "copy":
                dst.copy_(src)
            else:
                out = ops.compact_rows(h, labels, weights, ids, MASK, V, cap=cap)   # (its output and workspace allocations are inside the bracket)
            b.record()
            if i >= 3:
                t[kind].append((a, b))
    torch.cuda.synchronize()
    assert int(out[4].item()) == hints[0]
    nbytes = cap * H * h.element_size()
    print("   a) %d scored rows of [%d, %d] %s -> [%d, %d] = %.2f MB written (three launches; reads %d labels, ids and the scored rows)"
          % (hints[0], M, H, str(dtype).split(".")[-1], cap, H, nbytes / 1e6, M))
    print("   %-34s %10s %10s %10s" % ("call", "median us", "min us", "max us"))
    for kind in ("compact_rows", "copy"):
        us = [1e3 * v for v in ms_of(t[kind])]
        print("   %-34s %10.1f %10.1f %10.1f" % (kind if kind != "copy" else "copy_ of the same [%d, %d]" % (cap, H), statistics.median(us), min(us), max(us)))
    # b) the pass
    torch.manual_seed(0)
    model = me.ecamp(compute_dtype=dtype).to(dev)
    model.train()
    two = [dict({k: v.to(dev) for k, v in b.items()}, mlm_rows=n) for b, n in zip(host, hints)]   # resident in HBM, the row count known on the host
    loader = [two[i % 2] for i in range(nb)]
    modes = [("score all (the default: the pass of part 2)", dict(eval_score="all")),
             ("score masked, head on every row (compact=False)", dict(eval_score="masked", eval_compact=False)),
             ("score masked, head on the gathered rows", dict(eval_score="masked", eval_compact=True))]
    ns = [argparse.Namespace(mask_ratio=0.75, prefetch=False, **kw) for _, kw in modes]
    import contextlib
    import io
    times, stats = [[] for _ in modes], [None] * len(modes)
    for r in range(rounds + 1):
        for k, a in enumerate(ns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                stats[k] = evaluate(model, loader, dev, 0, args=a)      # ends in its own read-back
            if r >= 1:
                times[k].append((time.perf_counter() - t0) / nb)
    print("   b) evaluate(): %d batches resident in HBM, %d rounds of the three modes in turn after one untimed (host clock, each pass ends in its read-back)" % (nb, rounds))
    print("   %-58s %10s %10s %10s %10s" % ("", "median ms", "min ms", "max ms", "pairs/s"))
    for (name, _), ts in zip(modes, times):
        med = statistics.median(ts)
        print("   %-58s %10.3f %10.3f %10.3f %10.0f" % (name, 1e3 * med, 1e3 * min(ts), 1e3 * max(ts), B / med))
    for (name, _), st in zip(modes, stats):
        print("   %s -> %s" % (name.split(" (")[0], st))
    base, comp = statistics.median(times[1]), statistics.median(times[2])
    print("   -> compacting the head takes %.3f ms off the %.3f ms masked pass per batch (%.3fx)" % (1e3 * (base - comp), 1e3 * base, comp / base))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--leg", default="all", choices=["all", "pass", "compact"], help="pass: parts 1 and 2; compact: part 3 alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/eval_bench.py measures on an MI355X; there is nothing to time without one")
    from ecamp_amd import _lib
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    _lib.set_half(dt)
    d = torch.device("cuda:0")
    print("device:", torch.cuda.get_device_name(0))
    if a.leg in ("all", "pass"):
        bench_kernel(d, dt, a.iters)
        torch.cuda.empty_cache()
        bench_pass(d, dt, a.batches)
        torch.cuda.empty_cache()
    if a.leg in ("all", "compact"):
        bench_compact(d, dt, a.iters, a.batches)
