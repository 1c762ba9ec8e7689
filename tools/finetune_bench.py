"""Encoder fine-tuning, measured (profiles/finetune.txt): ViT-B/16 in bf16, R = 224, 14 classes, at B = 96 and B = 256 on one MI355X:

  1  one fine-tune step end to end (engine_finetune.train_step: differentiable encoder forward, head, loss, the whole backward, the fused
     clip + SGD step) in images/s, beside the probe step (engine_linprobe.train_step) of the same shape in the same process.
  2  `ecamp_sumsq_grouped` + `ecamp_sgd_grouped` over the parameter arena (the launches of one FusedSGD.step, with its block table)
     beside ONE `ecamp_adamw_grouped` launch over the same arena with the same table, alternating in one loop: HIP events around
     groups of calls.  The two SGD launches move about 6.5 arena-sized streams of the live blocks (g; p, g, buf in; p, buf, p16 out)
     where AdamW moves 7.5 (p, g, m, v in; p, m, v, p16 out): expected no more than 1.1 x AdamW's time.
  3  `ecamp_pool_norm_bwd` (dx [B, 197, 768] in bf16) beside a plain device copy of the same bytes.

    python tools/finetune_bench.py [--iters 20] [--warmup 3] [--batches 96,256] [--out profiles/finetune.txt]

`--droppath` runs another leg INSTEAD and writes profiles/finetune_droppath.txt (`--droppath_out`); without it nothing above changes:

  4  `ecamp_drop_path_fwd` / `ecamp_drop_path_bwd` alone on bf16 [B, 197, 768] beside `ecamp_add` on the same buffers, alternating in one
     loop, outputs allocated once.  ecamp_add moves three streams (two read, one written), and so does the forward for a kept sample (a
     dropped one moves two); the backward moves two (a dropped sample: one).  Expected: the forward at p = 0 -- the same bytes, one Philox
     call per (workgroup, sample) -- at parity with ecamp_add.
  5  the whole fine-tune step of leg 1 at drop_path_rate 0 against 0.1 on ONE model and optimizer, blocks of `--iters` steps alternating
     between the two rates.
  `--parity_log FILE`: the "[droppath]" lines that tests/test_droppath_model_gpu.py prints under `pytest -s` are copied behind the timings.

`--pos_embed` runs another leg INSTEAD and writes profiles/finetune_pos_embed.txt (`--pos_embed_out`):

  7  `ecamp_pos_embed_grad` (one fixed-order pass over dx = bf16 [B, 197, 768]: the gradients of pos_embed, cls_token and the patch
     embedding's bias) beside the two `ecamp_colsum` calls it replaces in StemFn.backward (two passes with float atomics: bias and
     cls_token only) and a plain device copy of the same bytes, alternating in one loop.
  8  the whole fine-tune step of leg 1 without and with `train_pos_embed` on TWO models of equal weights with an optimizer each (the
     arena's layout differs), blocks of `--iters` steps alternating between them.  The model without the flag runs the code of the
     commit before the flag existed, launch for launch.
  `--parity_log FILE`: the "[pos_embed]" lines that tests/test_posembed_*_gpu.py print under `pytest -s` are copied behind the timings.

`--fp16` runs another leg INSTEAD and writes profiles/finetune_fp16.txt (`--fp16_out`):

  10 the whole fine-tune step of leg 1 in bf16 beside the same step in IEEE half under the loss scaler (`--fp16 --fp16_loss_scale dynamic`:
     loss x scale, `FusedSGD.step_scaled`) on TWO models of equal weights with an optimizer each, blocks of `--iters` steps alternating.
  11 `ecamp_sgd_scale_update` alone beside an empty launch (`ecamp_dev_spin`, one workgroup, zero cycles), alternating in one loop.
  `--parity_log FILE`: the "[fp16-finetune]" lines that tests/test_sgd_scale_kernel_gpu.py and tests/test_fp16_finetune_model_gpu.py print under
  `pytest -s` are copied behind the timings.
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


def timed(fn, iters, warmup, reps=3):
    """Host clock around `iters` calls that end in a device synchronise, after `warmup` calls -> seconds per call, per repetition."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters)
    return out


def event_groups(fns, iters, warmup, group):
    """HIP events around groups of `group` back-to-back calls of each fn, the fns alternating in one loop -> {name: [us per call]}."""
    t = {name: [] for name, _ in fns}
    for i in range(iters + warmup):
        for name, fn in fns:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(group):
                fn()
            b.record()
            if i >= warmup:
                t[name].append((a, b))
        torch.cuda.synchronize()
    return {name: [1e3 * p.elapsed_time(q) / group for p, q in pairs] for name, pairs in t.items()}


def droppath_leg(args, say):
    """Legs 4 and 5 (see the module docstring)."""
    from ecamp_amd import _lib, engine_finetune
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module.classifier import build_classifier
    dev = torch.device("cuda")
    C, T, D = args.classes, 197, 768
    BF16 = _lib.BF16
    say("stochastic depth on %s: ViT-B/16 in bf16, R = 224, %d classes" % (torch.cuda.get_device_name(0), C))
    say("4  kernels alone: bf16 [B, %d, %d], per call, from event pairs around 20 calls, the kernels alternating in one loop (%d groups after %d warm-up "
        "groups); one stream = B x %d x %d x 2 bytes (at B = 96 the three streams, 87 MB, fit the 256 MB last-level cache: the rates are not HBM rates, "
        "for any of the kernels)" % (T, D, args.iters, args.warmup, T, D))
    seed, off = 0x9E3779B97F4A7C15, 5
    for B in [int(b) for b in args.batches.split(",")]:
        res = torch.randn(B * T, D, device=dev).to(torch.bfloat16)
        y = torch.randn(B * T, D, device=dev).to(torch.bfloat16)
        out = torch.empty_like(res)
        one = res.numel() * 2
        kept = int(ops.dropout_mask((B,), dev, 0.1, seed, off).sum().item())
        st = ops.stream

        def add():
            _lib.call("ecamp_add", ops.ptr(res), ops.ptr(y), ops.ptr(out), res.numel(), BF16, st())

        def fwd(p):
            return lambda: _lib.call("ecamp_drop_path_fwd", ops.ptr(res), ops.ptr(y), ops.ptr(out), B, T, D, p, seed, off, BF16, BF16, st())

        def bwd(p):
            return lambda: _lib.call("ecamp_drop_path_bwd", ops.ptr(res), ops.ptr(out), B, T, D, p, seed, off, BF16, st())

        names = [("ecamp_add", add, 3.0), ("drop_path_fwd p=0", fwd(0.0), 3.0), ("drop_path_fwd p=0.1", fwd(0.1), (3.0 * kept + 2.0 * (B - kept)) / B),
                 ("drop_path_bwd p=0", bwd(0.0), 2.0), ("drop_path_bwd p=0.1", bwd(0.1), (2.0 * kept + 1.0 * (B - kept)) / B)]
        us = event_groups([(n, f) for n, f, _ in names], args.iters, args.warmup, 20)
        say("   B = %3d: one stream = %.1f MB; at p = 0.1 this (seed, offset) keeps %d of %d samples" % (B, one / 1e6, kept, B))
        med_add, lo_add, hi_add = stats(us["ecamp_add"])
        for n, _, streams in names:
            med_u, lo_u, hi_u = stats(us[n])
            say("     %-20s median %7.1f us (min %.1f, max %.1f) = %.2f x ecamp_add; %.2f streams = %.0f GB/s"
                % (n, med_u, lo_u, hi_u, med_u / med_add, streams, streams * one / (med_u * 1e-6) / 1e9))
        gap = stats(us["drop_path_fwd p=0"])[0] - med_add
        say("     expectation: drop_path_fwd at p = 0 at parity with ecamp_add (same bytes): gap %+.1f us against ecamp_add's own min-max spread of %.1f us: %s"
            % (gap, hi_add - lo_add, "met" if gap <= hi_add - lo_add else "NOT met"))
        del res, y, out

    torch.manual_seed(0)
    clf = build_classifier("vit_base_patch16", C, True, img_size=224, compute_dtype=torch.bfloat16, train_encoder=True, drop_path_rate=0.1).to(dev)
    step_args = argparse.Namespace(learning_rate=3e-2, weight_decay=1e-4, decay_type="cosine", warmup_steps=50, num_steps=3000, max_grad_norm=1.0)
    opt = engine_finetune.make_optimizer(clf, step_args)
    rates = {0.1: list(clf.drop_path_rates), 0.0: [0.0] * len(clf.drop_path_rates)}
    say("5  the whole fine-tune step (forward + backward + clip + SGD) at drop_path_rate 0 against 0.1: one model, one optimizer, blocks of %d steps "
        "alternating between the rates, host clock around a block that ends in a device synchronise, 5 blocks each after %d warm-up steps each" % (args.iters, args.warmup))
    for B in [int(b) for b in args.batches.split(",")]:
        imgs = torch.randn(B, 3, 224, 224, device=dev)
        y = (torch.rand(B, C, device=dev) < 0.3).float()
        n = [0]

        def block(rate, steps):
            clf.drop_path_rate, clf.drop_path_rates = rate, rates[rate]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                engine_finetune.train_step(clf, opt, imgs, y, n[0], step_args)
                n[0] += 1
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps

        for rate in (0.0, 0.1):
            block(rate, args.warmup)
        ms = {0.0: [], 0.1: []}
        for _ in range(5):
            for rate in (0.0, 0.1):
                ms[rate].append(1e3 * block(rate, args.iters))
        m0, lo0, hi0 = stats(ms[0.0])
        m1, lo1, hi1 = stats(ms[0.1])
        say("   B = %3d  rate 0: %.2f ms (min %.2f, max %.2f) = %.0f images/s;  rate 0.1: %.2f ms (min %.2f, max %.2f) = %.0f images/s;  "
            "stochastic depth costs %+.2f ms = %+.1f %% (block-to-block spread at rate 0: %.2f ms)"
            % (B, m0, lo0, hi0, B / (m0 * 1e-3), m1, lo1, hi1, B / (m1 * 1e-3), m1 - m0, 100.0 * (m1 - m0) / m0, hi0 - lo0))
        sites = 2 * sum(r > 0 for r in rates[0.1])
        say("            %d active sites; from bytes alone: per site the forward adds one write and one read of a bf16 [B, 197, 768] stream to the GEMM "
            "epilogue it replaces, the backward one read and one write: about %.2f GB more per step" % (sites, sites * 4 * B * 197 * 768 * 2 / 1e9))
        del imgs, y
    if args.parity_log:
        say("6  parity of the model test (tests/test_droppath_model_gpu.py, ecamp_tiny, B = 4, drop_path_rate 0.5, float64 reference under the same masks):")
        for line in open(args.parity_log):
            if "[droppath]" in line:
                say("   " + line.strip().lstrip(".").strip())


def pos_embed_leg(args, say):
    """Legs 7 and 8 (see the module docstring)."""
    from ecamp_amd import engine_finetune
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module.classifier import build_classifier
    dev = torch.device("cuda")
    C, T, D = args.classes, 197, 768
    say("a trained pos_embed on %s: ViT-B/16 in bf16, R = 224, %d classes" % (torch.cuda.get_device_name(0), C))
    say("7  the stem's row-sum gradients from dx = bf16 [B, %d, %d], per call, from event pairs around 20 calls, alternating in one loop (%d groups after "
        "%d warm-up groups).  pos_embed_grad: ONE read of dx, fixed order, three gradients (dpos, dcls, dbias), its workspace from the caching "
        "allocator as in the product; 2 x colsum: TWO reads of dx, float atomics, two gradients (dbias, dcls) -- what StemFn.backward runs without "
        "the flag; device copy: one read and one write of the same bytes" % (T, D, args.iters, args.warmup))
    for B in [int(b) for b in args.batches.split(",")]:
        dx = torch.randn(B, T, D, device=dev).to(torch.bfloat16)
        dx2 = dx.view(B * T, D)
        dst = torch.empty_like(dx)
        dpos, dcls, dbias = ops.zeros((T, D), dev), ops.zeros((D,), dev), ops.zeros((D,), dev)
        nbytes = dx.numel() * 2

        def peg():
            ops.pos_embed_grad(dx, dpos, dcls, dbias)

        def colsums():
            ops.colsum(dx2, dbias, period=T, lo=1, hi=T)
            ops.colsum(dx2, dcls, period=T, lo=0, hi=1)

        us = event_groups([("pos_embed_grad", peg), ("2 x colsum", colsums), ("device copy", lambda: dst.copy_(dx))], args.iters, args.warmup, 20)
        say("   B = %3d: dx = %.1f MB (with the copy's destination %s the 256 MB last-level cache: %s)"
            % (B, nbytes / 1e6, "inside" if 2 * nbytes < 256e6 else "beyond", "the rates are not HBM rates" if 2 * nbytes < 256e6 else "HBM rates"))
        med_c = stats(us["2 x colsum"])[0]
        for name, reads in (("pos_embed_grad", 1.0), ("2 x colsum", 2.0), ("device copy", 1.0)):
            med_u, lo_u, hi_u = stats(us[name])
            say("     %-15s median %7.1f us (min %.1f, max %.1f) = %.2f x the two colsums; %.0f read%s of dx = %.0f GB/s read"
                % (name, med_u, lo_u, hi_u, med_u / med_c, reads, "" if reads == 1 else "s", reads * nbytes / (med_u * 1e-6) / 1e9))
        med_k = stats(us["pos_embed_grad"])[0]
        say("     pos_embed_grad against the two colsums it replaces: %+.1f us (%s)" % (med_k - med_c, "faster" if med_k < med_c else "SLOWER"))
        del dx, dx2, dst

    step_args = argparse.Namespace(learning_rate=3e-2, weight_decay=1e-4, decay_type="cosine", warmup_steps=50, num_steps=3000, max_grad_norm=1.0)
    models = {}
    for flag in (False, True):
        torch.manual_seed(0)
        clf = build_classifier("vit_base_patch16", C, True, img_size=224, compute_dtype=torch.bfloat16, train_encoder=True, train_pos_embed=flag).to(dev)
        models[flag] = (clf, engine_finetune.make_optimizer(clf, step_args))
    say("8  the whole fine-tune step (forward + backward + clip + SGD) without and with train_pos_embed: two models of equal initial weights, an optimizer "
        "each, blocks of %d steps alternating between them, host clock around a block that ends in a device synchronise, 5 blocks each after %d warm-up "
        "steps each.  `off` runs the launches of the commit before the flag existed" % (args.iters, args.warmup))
    for B in [int(b) for b in args.batches.split(",")]:
        imgs = torch.randn(B, 3, 224, 224, device=dev)
        y = (torch.rand(B, C, device=dev) < 0.3).float()
        n = {False: 0, True: 0}

        def block(flag, steps):
            clf, opt = models[flag]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                engine_finetune.train_step(clf, opt, imgs, y, n[flag], step_args)
                n[flag] += 1
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps

        for flag in (False, True):
            block(flag, args.warmup)
        ms = {False: [], True: []}
        for _ in range(5):
            for flag in (False, True):
                ms[flag].append(1e3 * block(flag, args.iters))
        m0, lo0, hi0 = stats(ms[False])
        m1, lo1, hi1 = stats(ms[True])
        say("   B = %3d  off: %.2f ms (min %.2f, max %.2f) = %.0f images/s;  on: %.2f ms (min %.2f, max %.2f) = %.0f images/s;  "
            "a trained pos_embed costs %+.2f ms = %+.2f %% (block-to-block spread of `off`: %.2f ms)"
            % (B, m0, lo0, hi0, B / (m0 * 1e-3), m1, lo1, hi1, B / (m1 * 1e-3), m1 - m0, 100.0 * (m1 - m0) / m0, hi0 - lo0))
        del imgs, y
    earlier = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "finetune_droppath.txt")
    if os.path.exists(earlier):
        say("   the same step as the commit before the flag measured it (profiles/finetune_droppath.txt, leg 5, its `rate 0` blocks: the same model, "
            "optimizer and shapes, another run on another day):")
        for line in open(earlier):
            if "rate 0:" in line:
                say("     " + line.strip().split(";  rate 0.1")[0])
    if args.parity_log:
        say("9  the GPU tests' own figures (tests/test_posembed_kernel_gpu.py: worst |got - exact| over the derived bound; tests/test_posembed_model_gpu.py: "
            "ecamp_tiny, B = 4, float64 reference with pos_embed trained):")
        for line in open(args.parity_log):
            if "[pos_embed]" in line:
                say("   " + line[line.index("[pos_embed]"):].strip())


def fp16_leg(args, say):
    """Legs 10 and 11 (see the module docstring)."""
    from ecamp_amd import _lib, engine_finetune
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module.classifier import build_classifier
    dev = torch.device("cuda")
    C = args.classes
    say("IEEE-half fine-tuning under the on-device loss scaler on %s: ViT-B/16, R = 224, %d classes" % (torch.cuda.get_device_name(0), C))
    models = {}
    for name, dtype in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        torch.manual_seed(0)
        clf = build_classifier("vit_base_patch16", C, True, img_size=224, compute_dtype=dtype, train_encoder=True).to(dev)
        step_args = argparse.Namespace(learning_rate=3e-2, weight_decay=1e-4, decay_type="cosine", warmup_steps=50, num_steps=3000, max_grad_norm=1.0,
                                       compute_dtype=name, fp16_loss_scale="dynamic" if name == "fp16" else None)
        models[name] = (clf, engine_finetune.make_optimizer(clf, step_args), step_args)
    scaler = models["fp16"][1].loss_scaler
    say("10 the whole fine-tune step (forward + backward + clip + SGD) in bf16 and in fp16 with the loss scaler (%s): two models of equal initial "
        "weights, an optimizer each, blocks of %d steps alternating between them, host clock around a block that ends in a device synchronise, 5 blocks "
        "each after %d warm-up steps each" % (scaler.describe(), args.iters, args.warmup))
    for B in [int(b) for b in args.batches.split(",")]:
        imgs = torch.randn(B, 3, 224, 224, device=dev)
        y = (torch.rand(B, C, device=dev) < 0.3).float()
        n = {"bf16": 0, "fp16": 0}

        def block(name, steps):
            clf, opt, step_args = models[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                engine_finetune.train_step(clf, opt, imgs, y, n[name], step_args)
                n[name] += 1
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps

        for name in models:
            block(name, args.warmup)
        ms = {name: [] for name in models}
        for _ in range(5):
            for name in models:
                ms[name].append(1e3 * block(name, args.iters))
        m0, lo0, hi0 = stats(ms["bf16"])
        m1, lo1, hi1 = stats(ms["fp16"])
        say("   B = %3d  bf16: %.2f ms (min %.2f, max %.2f) = %.0f images/s;  fp16 + scaler: %.2f ms (min %.2f, max %.2f) = %.0f images/s;  "
            "fp16 - bf16 = %+.2f ms = %+.2f %% (block-to-block spread of bf16: %.2f ms); after %d fp16 steps: scale %.10g, %d skipped"
            % (B, m0, lo0, hi0, B / (m0 * 1e-3), m1, lo1, hi1, B / (m1 * 1e-3), m1 - m0, 100.0 * (m1 - m0) / m0, hi0 - lo0, n["fp16"], scaler.scale,
               scaler.skipped_steps))
        del imgs, y

    opt = models["fp16"][1]
    npart = sum(opt._slots)
    part = torch.rand(npart, device=dev) + 0.5
    state = torch.tensor([2.0 ** 20, 0.0, 0.0, 0.0], device=dev)
    ctl, norm = ops.zeros((4,), dev), ops.zeros((1,), dev)
    st = ops.stream
    us = event_groups([("sgd_scale_update", lambda: ops.sgd_scale_update(part, npart, state, ctl, norm, 2.0, 0.5, 2000, 2.0 ** 24)),
                       ("empty launch", lambda: _lib.call("ecamp_dev_spin", 1, 256, 0, st()))], args.iters, args.warmup, 20)
    say("11 ecamp_sgd_scale_update alone over the %d slots of this model's step (arena %d + tail %d) beside an empty launch (ecamp_dev_spin, one "
        "workgroup of 256 threads, zero cycles: the floor of a single-workgroup kernel), per call, from event pairs around 20 back-to-back calls, "
        "alternating in one loop (%d groups after %d warm-up groups)" % (npart, opt._slots[0], opt._slots[1], args.iters, args.warmup))
    med_e = stats(us["empty launch"])[0]
    for name in ("sgd_scale_update", "empty launch"):
        med_u, lo_u, hi_u = stats(us[name])
        say("   %-17s median %6.2f us (min %.2f, max %.2f) = %.2f x the empty launch" % (name, med_u, lo_u, hi_u, med_u / med_e))
    if args.parity_log:
        say("12 the GPU tests' own figures (tests/test_sgd_scale_kernel_gpu.py; tests/test_fp16_finetune_model_gpu.py: ecamp_tiny, B = 4, float64 references):")
        for line in open(args.parity_log):
            if "[fp16-finetune]" in line:
                say("   " + line[line.index("[fp16-finetune]"):].strip())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=str, default="96,256")
    ap.add_argument("--classes", type=int, default=14)
    ap.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "finetune.txt"))
    ap.add_argument("--droppath", action="store_true", help="run the stochastic-depth leg instead (profiles/finetune_droppath.txt)")
    ap.add_argument("--droppath_out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "finetune_droppath.txt"))
    ap.add_argument("--parity_log", type=str, default="", help="--droppath / --pos_embed: a `pytest -s` log of that leg's GPU tests whose [droppath] / [pos_embed] lines are copied")
    ap.add_argument("--pos_embed", action="store_true", help="run the trained-pos_embed leg instead (profiles/finetune_pos_embed.txt)")
    ap.add_argument("--pos_embed_out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "finetune_pos_embed.txt"))
    ap.add_argument("--fp16", action="store_true", help="run the IEEE-half / loss-scaler leg instead (profiles/finetune_fp16.txt)")
    ap.add_argument("--fp16_out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "finetune_fp16.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_bench needs an MI355X: nothing here can be measured on a CPU")
    if args.fp16:
        lines = []

        def say_h(msg):
            print(msg, flush=True)
            lines.append(msg)

        fp16_leg(args, say_h)
        os.makedirs(os.path.dirname(os.path.abspath(args.fp16_out)), exist_ok=True)
        with open(args.fp16_out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if args.pos_embed:
        lines = []

        def say_pe(msg):
            print(msg, flush=True)
            lines.append(msg)

        pos_embed_leg(args, say_pe)
        os.makedirs(os.path.dirname(os.path.abspath(args.pos_embed_out)), exist_ok=True)
        with open(args.pos_embed_out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if args.droppath:
        lines = []

        def say_dp(msg):
            print(msg, flush=True)
            lines.append(msg)

        droppath_leg(args, say_dp)
        os.makedirs(os.path.dirname(os.path.abspath(args.droppath_out)), exist_ok=True)
        with open(args.droppath_out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    from ecamp_amd import engine_finetune, engine_linprobe
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module.classifier import build_classifier
    lines = []

    def say(msg):
        print(msg, flush=True)
        lines.append(msg)

    dev = torch.device("cuda")
    C = args.classes
    torch.manual_seed(0)
    clf = build_classifier("vit_base_patch16", C, True, img_size=224, compute_dtype=torch.bfloat16, train_encoder=True).to(dev)
    step_args = argparse.Namespace(learning_rate=3e-2, weight_decay=1e-4, decay_type="cosine", warmup_steps=50, num_steps=3000, max_grad_norm=1.0)
    say("encoder fine-tuning on %s: ViT-B/16 in bf16, R = 224, %d classes; %d iterations x 3 repetitions after %d warm-up calls"
        % (torch.cuda.get_device_name(0), C, args.iters, args.warmup))
    opt = engine_finetune.make_optimizer(clf, step_args)
    A = opt.arena
    live = int((opt._table < 8).sum().item()) * 64
    say("arena: %d f32 elements (%.2f GB), of which fine-tuning updates %d (%.1f %%); tail buffer %d elements"
        % (A.total, 4 * A.total / 1e9, live, 100.0 * live / A.total, opt._tail.total))

    for B in [int(b) for b in args.batches.split(",")]:
        imgs = torch.randn(B, 3, 224, 224, device=dev)
        y = (torch.rand(B, C, device=dev) < 0.3).float()
        n = [0]

        def ft_step():
            engine_finetune.train_step(clf, opt, imgs, y, n[0], step_args)
            n[0] += 1

        med, lo, hi = stats(timed(ft_step, args.iters, args.warmup))
        say("1  B = %3d  fine-tune step (forward + backward + clip + SGD): %.2f ms (min %.2f, max %.2f) = %.0f images/s"
            % (B, 1e3 * med, 1e3 * lo, 1e3 * hi, B / med))
        clf.eval()
        popt = engine_linprobe.make_optimizer(clf, step_args)
        clf.head.weight.grad = clf.head.bias.grad = None      # the probe's optimizer clips and steps plain `.grad` tensors
        m = [0]

        def probe_step():
            engine_linprobe.train_step(clf, popt, imgs, y, m[0], step_args)
            m[0] += 1

        med_p, lo_p, hi_p = stats(timed(probe_step, args.iters, args.warmup))
        clf.tail()                                            # (`.grad` back onto the tail buffer)
        say("   B = %3d  probe step (encoder forward + head + loss + head gradient + clip + SGD): %.2f ms (min %.2f, max %.2f) = %.0f images/s; "
            "fine-tune / probe = %.2f x" % (B, 1e3 * med_p, 1e3 * lo_p, 1e3 * hi_p, B / med_p, med / med_p))

        T, D = 197, 768
        pooled = torch.randn(B, D, device=dev)
        dfeat = torch.randn(B, D, device=dev)
        gamma = torch.ones(D, device=dev)
        src = torch.randn(B, T, D, device=dev).to(torch.bfloat16)
        dst = torch.empty_like(src)
        nbytes = src.numel() * 2
        us = event_groups([("pool_norm_bwd", lambda: ops.pool_norm_bwd(dfeat, pooled, gamma, 1, T, T, 1e-6, torch.bfloat16)),
                           ("device copy", lambda: dst.copy_(src))], args.iters, args.warmup, 20)
        say("3  B = %3d  dx = bf16 [%d, %d, %d] = %.1f MB; per call, from event pairs around 20 calls (pool_norm_bwd includes its output / workspace allocations)"
            % (B, B, T, D, nbytes / 1e6))
        for name in ("pool_norm_bwd", "device copy"):
            med_u, lo_u, hi_u = stats(us[name])
            say("   %-16s median %7.1f us (min %.1f, max %.1f) = %.0f GB/s written" % (name, med_u, lo_u, hi_u, nbytes / (med_u * 1e-6) / 1e9))

    # 2: the optimizer launches over the arena, same block table, same process
    mbuf, vbuf = ops.zeros((A.total,), dev), ops.zeros((A.total,), dev)
    lrs, wds = [1e-3], [1e-4]
    ops.zero_(A.flat_g)
    A.flat_g.normal_(std=1e-3)
    n0 = ops.sumsq_grouped_slots(A.total)
    partials = ops.zeros((n0,), dev)

    def sgd():
        ops.sumsq_grouped(A.flat_g, opt._table, partials)
        ops.sgd_grouped(A.flat_p, A.flat_g, opt._buf, A.flat_p16, opt._table, lrs, wds, 0.9, 1.0, partials, n0, 1.0, None, opt.last_norm)

    def sumsq_only():
        ops.sumsq_grouped(A.flat_g, opt._table, partials)

    def adamw():
        ops.adamw_grouped(A.flat_p, A.flat_g, mbuf, vbuf, A.flat_p16, opt._table, lrs, wds, 0.9, 0.95, 1e-8, 10, 1.0, None, None)

    us = event_groups([("sumsq_grouped + sgd_grouped", sgd), ("adamw_grouped", adamw), ("sumsq_grouped alone", sumsq_only)], args.iters, args.warmup, 5)
    say("2  optimizer launches over the arena (%d live f32 elements of %d), per call, from event pairs around 5 calls, alternating:" % (live, A.total))
    med_a = stats(us["adamw_grouped"])[0]
    for name in ("sumsq_grouped + sgd_grouped", "adamw_grouped", "sumsq_grouped alone"):
        med_u, lo_u, hi_u = stats(us[name])
        streams = {"sumsq_grouped + sgd_grouped": 6.5, "adamw_grouped": 7.5, "sumsq_grouped alone": 1.0}[name]
        say("   %-28s median %8.1f us (min %.1f, max %.1f) = %.2f x adamw_grouped; %.1f streams of %.2f GB = %.0f GB/s"
            % (name, med_u, lo_u, hi_u, med_u / med_a, streams, 4 * live / 1e9, streams * 4 * live / (med_u * 1e-6) / 1e9))
    say("   expectation: sumsq_grouped + sgd_grouped <= 1.10 x adamw_grouped (6.5 against 7.5 streams, a second launch): %s"
        % ("met" if stats(us["sumsq_grouped + sgd_grouped"])[0] <= 1.1 * med_a else "NOT met"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
