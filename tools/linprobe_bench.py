"""The linear probe, measured (profiles/linprobe.txt), at B = 256, R = 224, one MI355X:

  1  `ECAMPClassifier.forward_features` (the frozen ViT-B/16 encoder, every patch kept, + token mean + fc_norm) in images/s.
  2  `ecamp_pool_norm` on the last block's output [256, 197, 768] against the two launches it replaces, `ecamp_seq_sum` +
     `ecamp_layernorm_fwd` (which round the mean to 16 bits in between), on the same tensor: HIP events around groups of 20 calls,
     the two alternating in one loop.
  3  one probe step end to end (engine_linprobe.train_step: encoder forward, head, loss, head gradient, clip, SGD) in images/s.

    python tools/linprobe_bench.py [--iters 30] [--warmup 5] [--dtype bf16|fp16] [--batch 256] [--classes 14]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


def timed(fn, iters, warmup):
    """Host clock around `iters` calls that end in a device synchronise, after `warmup` calls -> seconds per call, per repetition of 5."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        reps.append((time.perf_counter() - t0) / iters)
    return reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--classes", type=int, default=14)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linprobe_bench needs an MI355X: nothing here can be measured on a CPU")
    from ecamp_amd import engine_linprobe as engine
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module.classifier import build_classifier
    dev = torch.device("cuda")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    B, C = args.batch, args.classes
    torch.manual_seed(0)
    clf = build_classifier("vit_base_patch16", C, True, img_size=224, compute_dtype=dtype).to(dev)
    imgs = torch.randn(B, 3, 224, 224, device=dev)
    y = (torch.rand(B, C, device=dev) < 0.3).float()
    print("linear probe on %s: ViT-B/16 encoder in %s, B = %d, R = 224, %d classes; %d iterations x 5 repetitions after %d warm-up calls"
          % (torch.cuda.get_device_name(0), args.dtype, B, C, args.iters, args.warmup))

    reps = timed(lambda: clf.forward_features(imgs), args.iters, args.warmup)
    med, lo, hi = stats(reps)
    print("1  forward_features: %.2f ms per call (min %.2f, max %.2f over the repetitions) = %.0f images/s" % (1e3 * med, 1e3 * lo, 1e3 * hi, B / med))

    T, D = 197, 768
    x = (torch.randn(B, T, D, device=dev) + torch.linspace(-4, 4, D, device=dev)).to(dtype)
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    nbytes = x.numel() * x.element_size()

    def fused():
        return ops.pool_norm(x, 1, T, gamma, beta, 1e-6)

    def two():
        return ops.layernorm_fwd(ops.seq_sum(x, 1, T, 1.0 / (T - 1)), gamma, beta, 1e-6)

    # HIP events around GROUPS of 20 back-to-back calls, the two forms alternating: a single call of either form is two launches of
    # ~10-20 us, less than the host needs to queue them, so an event pair around one call would time the host
    GROUP = 20
    t = {"pool_norm": [], "seq_sum + layernorm_fwd": []}
    for i in range(args.iters + args.warmup):
        for name, fn in (("pool_norm", fused), ("seq_sum + layernorm_fwd", two)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(GROUP):
                fn()
            b.record()
            if i >= args.warmup:
                t[name].append((a, b))
        torch.cuda.synchronize()
    host = {name: 1e6 * stats(timed(fn, GROUP, args.warmup))[0] for name, fn in (("pool_norm", fused), ("seq_sum + layernorm_fwd", two))}
    print("2  token mean + norm of %s [%d, %d, %d] = %.1f MB; per call, from event pairs around %d calls (the calls include their output /"
          " workspace allocations); 'host us': the host clock around the same groups, ending in a synchronise"
          % (args.dtype, B, T, D, nbytes / 1e6, GROUP))
    print("   %-26s %10s %10s %10s %12s %10s" % ("call", "median us", "min us", "max us", "GB/s read", "host us"))
    for name, pairs in t.items():
        us = [1e3 * p.elapsed_time(q) / GROUP for p, q in pairs]
        med, lo, hi = stats(us)
        print("   %-26s %10.1f %10.1f %10.1f %12.0f %10.1f" % (name, med, lo, hi, nbytes * (T - 1) / T / (med * 1e-6) / 1e9, host[name]))
    f = fused()[1].double()
    r = torch.nn.functional.layer_norm(x.double()[:, 1:].mean(1), (D,), eps=1e-6)
    s = two()[0].double()
    print("   worst error against float64 / max magnitude: pool_norm %.2e, seq_sum + layernorm_fwd %.2e"
          % (float((f - r).abs().max() / r.abs().max()), float((s - r).abs().max() / r.abs().max())))

    step_args = argparse.Namespace(learning_rate=3e-2, weight_decay=0.0, decay_type="cosine", warmup_steps=50, num_steps=3000, max_grad_norm=1.0)
    opt = engine.make_optimizer(clf, step_args)
    n = [0]

    def step():
        engine.train_step(clf, opt, imgs, y, n[0], step_args)
        n[0] += 1

    reps = timed(step, args.iters, args.warmup)
    med, lo, hi = stats(reps)
    print("3  probe step (encoder forward + head + loss + head gradient + clip + SGD): %.2f ms (min %.2f, max %.2f) = %.0f images/s"
          % (1e3 * med, 1e3 * lo, 1e3 * hi, B / med))


if __name__ == "__main__":
    main()
