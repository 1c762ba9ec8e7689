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

`--image_pipeline` runs another leg INSTEAD and writes profiles/finetune_image_pipeline.txt (`--image_pipeline_out`):

  13 `ecamp_resample_boxes_u8` (BILINEAR, R = 224) on B training crops of 1024 x 1024 sources (boxes drawn by `device_train_item`), and
     `ecamp_im2col_u8` on the resulting uint8 [B, 224, 224] beside `ecamp_im2col_gather` on the f32 [B, 3, 224, 224] image, per call.
  14 the whole fine-tune step of leg 1 on a resident f32 batch -- the code of the commit before the uint8 path existed, launch for launch --
     against the same step on the resident uint8 batch of the same pixels, ONE model and optimizer, blocks alternating three times.
  15 images/s of the host loader (ListDataset + train_transform: PIL decode, crop, resample, f32 planes) and of the device loader
     (ShardListDataset + DeviceImageLoader) with the same worker count over the same generated PNG set (`--loader_images` files of
     1024 x 1024), each over one full pass after a first pass that starts the workers.

`--image_pipeline --colour` runs the resample and loader comparison of that leg on COLOUR sources instead and writes
profiles/finetune_image_pipeline_colour.txt (`--image_pipeline_colour_out`):

  16 `ecamp_resample_boxes_rgb_u8` on B three-plane training crops of 1024 x 1024 sources with three different planes, beside
     `ecamp_resample_boxes_u8` on the first planes of the same boxes (the boxes of leg 13: the same seed draws them), alternating in one loop.
  17 leg 15 over colour PNG files and a colour shard (`U8ShardWriter(colour=True)`); `--loader_images 0` skips it.

`--image_pipeline --resident` measures the shard kept in device memory (`--image_shard_resident`) on gray sources and then on colour ones
(`--colour`: colour alone) and writes profiles/finetune_image_resident.txt (`--image_resident_out`):

  (a) `ecamp_resample_shard_u8` on boxes read where they lie in the resident images beside `ecamp_resample_boxes_u8` / `_rgb_u8` on the same
      boxes packed, alternating in groups inside one process; medians, the packed call's own spread, the verdict by leg 14's rule -- once with
      the same batch in every call, once with batches in rotation whose box bytes (`--resident_fresh_mb`) exceed the 256 MB Infinity Cache.
  (b) the resident loader beside the device loader of leg 15 / 17 on the same shard and list, `--loader_workers` workers each, passes after
      the first; the fine-tune step's rate on a uint8 batch is taken in the same process, and a loader FEEDS a step by leg 15's rule.
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


def image_pipeline_leg(args, say):
    """Legs 13 to 15 (see the module docstring)."""
    import shutil
    import tempfile

    import numpy as np
    from torch.utils.data import DataLoader

    from ecamp_amd import engine_finetune
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import finetune_datasets as fd
    from ecamp_amd.module.classifier import build_classifier
    from ecamp_amd.module.pretrain_datasets import U8ShardWriter
    dev = torch.device("cuda")
    C, R, S = args.classes, 224, 1024
    batches = [int(b) for b in args.batches.split(",")]
    say("the classification image pipeline on the device, on %s: R = %d, sources %d x %d, training crop scales 0.08 to 1" % (torch.cuda.get_device_name(0), R, S, S))
    rng = np.random.default_rng(0)
    base = [np.clip(127 + 80 * np.sin(np.add.outer(np.arange(S) / (5.0 + k), np.arange(S) / (9.0 - k))) + rng.integers(-30, 31, (S, S)), 0, 255).astype(np.uint8)
            for k in range(4)]
    lut = ops.image_lut(dev, fd.FT_MEAN, fd.FT_STD)
    say("13 kernels alone, per call, from event pairs around 10 back-to-back calls, alternating in one loop (%d groups after %d warm-up groups)" % (args.iters, args.warmup))
    resident = {}
    for B in batches:
        torch.manual_seed(B)
        flat, table, meta = fd.pack_boxes([fd.device_train_item(base[b % 4], R) for b in range(B)])
        flat_d, table_d = flat.to(dev), table.to(dev)
        rs = fd.DeviceBoxResampler(dev, R)
        u8 = rs(flat_d, table_d, meta, check=True)
        ids = torch.arange(196, dtype=torch.int32, device=dev).expand(B, 196).contiguous()
        f32 = lut[u8.long()][:, None].expand(B, 3, R, R).contiguous()
        assert torch.equal(ops.im2col_u8(u8, lut, ids, 16, torch.bfloat16).view(torch.int16), ops.im2col_gather(f32, ids, 16, torch.bfloat16).view(torch.int16))
        us = event_groups([("ecamp_resample_boxes_u8", lambda: rs(flat_d, table_d, meta)),
                           ("ecamp_im2col_u8 (bf16 cols)", lambda: ops.im2col_u8(u8, lut, ids, 16, torch.bfloat16)),
                           ("ecamp_im2col_gather on f32 (bf16 cols)", lambda: ops.im2col_gather(f32, ids, 16, torch.bfloat16))], args.iters, args.warmup, 10)
        say("   B = %3d: %.1f MB of box bytes, %d taps, tallest box %d rows" % (B, flat.numel() / 1e6, meta[0], meta[2]))
        for name, xs in us.items():
            med, lo, hi = stats(xs)
            say("      %-40s median %8.1f us (min %.1f, max %.1f)" % (name, med, lo, hi))
        resident[B] = (f32, u8)
        del flat_d, table_d, rs
    torch.manual_seed(0)
    clf = build_classifier("vit_base_patch16", C, True, img_size=R, compute_dtype=torch.bfloat16, train_encoder=True).to(dev)
    step_args = argparse.Namespace(learning_rate=3e-2, weight_decay=1e-4, decay_type="cosine", warmup_steps=50, num_steps=3000, max_grad_norm=1.0)
    opt = engine_finetune.make_optimizer(clf, step_args)
    say("14 the whole fine-tune step (ViT-B/16, bf16, forward + backward + clip + SGD) on a resident f32 [B, 3, %d, %d] batch -- the parent commit's step: "
        "that path runs the parent's kernels launch for launch -- against the resident uint8 [B, %d, %d] batch of the same pixels; one model and optimizer, "
        "blocks of %d steps alternating parent / new three times, host clock around a block that ends in a device synchronise, after %d warm-up steps each"
        % (R, R, R, R, args.iters, args.warmup))
    n = [0]
    step_rate = {}
    for B in batches:
        f32, u8 = resident[B]
        y = (torch.rand(B, C, device=dev) < 0.3).float()

        def block(x, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                engine_finetune.train_step(clf, opt, x, y, n[0], step_args)
                n[0] += 1
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / steps

        block(f32, args.warmup)
        block(u8, args.warmup)
        old, new = [], []
        for _ in range(3):
            old.append(block(f32, args.iters))
            new.append(block(u8, args.iters))
        mo, mn, spread = statistics.median(old), statistics.median(new), max(old) - min(old)
        step_rate[B] = B / (mn * 1e-3)
        say("   B = %3d  parent (f32): %s ms = %.0f images/s;  new (uint8): %s ms = %.0f images/s;  new - parent = %+.3f ms (medians); the parent's own spread "
            "across its three runs: %.3f ms -> %s" % (B, " ".join("%.2f" % v for v in old), B / (mo * 1e-3), " ".join("%.2f" % v for v in new), B / (mn * 1e-3),
                                                   mn - mo, spread, "not slower" if mn - mo <= spread else "SLOWER than the parent by more than its spread"))
    del clf, opt, resident
    # leg 15: the loaders, over files written here
    from PIL import Image
    root = tempfile.mkdtemp(prefix="ecamp_image_pipeline_")
    try:
        N, W = args.loader_images, args.loader_workers
        os.makedirs(os.path.join(root, "img"))
        lines = []
        for k in range(N):
            a = np.roll(base[k % 4], 37 * k, axis=1)
            Image.fromarray(a, "L").save(os.path.join(root, "img", "i%d.png" % k), compress_level=1)
            lines.append("img/i%d.png %s" % (k, " ".join(str((k >> c) & 1) for c in range(C))))
        rep = args.loader_repeat          # the list names every file `rep` times: passes long enough to time, without writing more files
        open(os.path.join(root, "train_list.txt"), "w").write("\n".join(lines * rep) + "\n")
        with U8ShardWriter(os.path.join(root, "train_list.txt.u8")) as w:
            for _ in range(rep):
                for k in range(N):
                    w.add(np.roll(base[k % 4], 37 * k, axis=1))
        say("15 loaders: one pass over a list of %d samples (%d PNG files of %d x %d, lossless, each listed %d times; the shard holds the same pixels in list "
            "order), batch 96, %d workers each, pinned memory; the pass is timed after a first pass (worker start-up, file cache); host: ListDataset + "
            "train_transform -> f32 [96, 3, %d, %d]; device: ShardListDataset + DeviceImageLoader -> uint8 [96, %d, %d] in HBM (the resample included; the "
            "timed pass ends in a device synchronise)" % (N * rep, N, S, S, rep, W, R, R, R, R))
        host = DataLoader(fd.ListDataset(root, root, "train", data_volume="100", transform=fd.train_transform(R)), shuffle=True, batch_size=96, num_workers=W,
                          pin_memory=True, persistent_workers=W > 0)
        def device_loader(workers):
            return fd.DeviceImageLoader(DataLoader(fd.ShardListDataset(root, root, "train", data_volume="100", img_size=R), shuffle=True, batch_size=96,
                                                   num_workers=workers, pin_memory=True, collate_fn=fd.collate_boxes, persistent_workers=workers > 0), dev, R)

        rates, slowest = {}, {}
        for name, loader in (("host loader", host), ("device loader", device_loader(W)), ("device loader, %d workers" % (2 * W), device_loader(2 * W))):
            per = []
            for rep in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                seen = 0
                for x, _ in loader:
                    x = x.to(dev, non_blocking=True)
                    seen += x.shape[0]
                torch.cuda.synchronize()
                per.append(seen / (time.perf_counter() - t0))
            rates[name], slowest[name] = statistics.median(per[1:]), min(per[1:])
            say("   %-26s %8.0f images/s (passes after the first: %s)" % (name, rates[name], " ".join("%.0f" % v for v in per[1:])))
            del loader
        say("   device / host = %.1f x with the same %d workers" % (rates["device loader"] / rates["host loader"], W))
        say("   the rates these must feed: the fine-tune step of leg 14 on the uint8 batch (%s images/s), and profiles/finetune.txt / profiles/linprobe.txt: about "
            "6 600 images/s for a fine-tune step at B = 96, 19 700 images/s for a probe step.  A loader FEEDS a step when its SLOWEST timed pass is at least the "
            "step's rate:" % ", ".join("B = %d: %.0f" % (B, r) for B, r in step_rate.items()))
        for name in rates:
            verdict = ["fine-tune step at B = %d: %s" % (B, "FEEDS it" if slowest[name] >= r else "does NOT feed it") for B, r in step_rate.items()]
            verdict.append("probe step (19 700): %s" % ("FEEDS it" if slowest[name] >= 19700 else "does NOT feed it"))
            say("   %-26s slowest pass %6.0f images/s -> %s" % (name, slowest[name], "; ".join(verdict)))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def image_pipeline_colour_leg(args, say):
    """Legs 16 and 17 (see the module docstring)."""
    import shutil
    import tempfile

    import numpy as np
    from torch.utils.data import DataLoader

    from ecamp_amd.module import finetune_datasets as fd
    from ecamp_amd.module.pretrain_datasets import U8ShardWriter
    dev = torch.device("cuda")
    C, R, S = args.classes, 224, 1024
    batches = [int(b) for b in args.batches.split(",")]
    say("colour sources in the classification image pipeline on the device, on %s: R = %d, sources 3 x %d x %d (three different planes), training crop "
        "scales 0.08 to 1" % (torch.cuda.get_device_name(0), R, S, S))
    rng = np.random.default_rng(0)
    base = [np.clip(127 + 80 * np.sin(np.add.outer(np.arange(S) / (5.0 + k), np.arange(S) / (9.0 - k))) + rng.integers(-30, 31, (S, S)), 0, 255).astype(np.uint8)
            for k in range(4)]
    colour = [np.stack([base[k], base[(k + 1) % 4], base[(k + 2) % 4]]) for k in range(4)]
    say("16 kernels alone, per call (coefficients + horizontal + vertical pass), from event pairs around 10 back-to-back calls, alternating in one loop "
        "(%d groups after %d warm-up groups); the gray entry point runs on the FIRST PLANES of the same boxes" % (args.iters, args.warmup))
    PARENT_US = {96: 175.0, 256: 399.0}      # profiles/finetune_image_pipeline.txt, leg 13: the gray entry point at the parent commit
    for B in batches:
        torch.manual_seed(B)                  # leg 13's seed: the same boxes
        items = [fd.device_train_item(colour[b % 4], R) for b in range(B)]
        cf, ct, cm = fd.pack_boxes(items)
        gf, gt, gm = fd.pack_boxes([(box[0], flip, geom) for box, flip, geom in items])
        assert len(cm) == 4 and cm[3] and len(gm) == 3 and cm[0] == gm[0] and cm[1] == 3 * gm[1]
        cf, ct, gf, gt = cf.to(dev), ct.to(dev), gf.to(dev), gt.to(dev)
        rs_c, rs_g = fd.DeviceBoxResampler(dev, R), fd.DeviceBoxResampler(dev, R)
        got = rs_c(cf, ct, cm, check=True)
        from PIL import Image
        box, flip, _ = items[0]                # one sample against Pillow itself, before anything is timed
        want = Image.fromarray(np.ascontiguousarray(box.transpose(1, 2, 0)), "RGB").resize((R, R), Image.BILINEAR)
        want = np.asarray((want.transpose(Image.FLIP_LEFT_RIGHT) if flip else want).convert("L"))
        assert np.array_equal(got[0].cpu().numpy(), want)
        us = event_groups([("ecamp_resample_boxes_rgb_u8 (three planes)", lambda: rs_c(cf, ct, cm)),
                           ("ecamp_resample_boxes_u8 (first planes)", lambda: rs_g(gf, gt, gm))], args.iters, args.warmup, 10)
        say("   B = %3d: %.1f MB of colour box bytes (%.1f MB of first planes), %d taps, tallest colour sample %d intermediate rows" % (B, cf.numel() / 1e6, gf.numel() / 1e6, cm[0], cm[2]))
        med = {}
        for name, xs in us.items():
            med[name], lo, hi = stats(xs)
            say("      %-44s median %8.1f us (min %.1f, max %.1f)" % (name, med[name], lo, hi))
        c, g = med["ecamp_resample_boxes_rgb_u8 (three planes)"], med["ecamp_resample_boxes_u8 (first planes)"]
        say("      colour / gray = %.2f x (three times the source bytes and taps, one coefficient pass and one output byte: about 3 x is the expectation)" % (c / g))
        if B in PARENT_US:
            say("      the gray entry point at the parent commit (profiles/finetune_image_pipeline.txt): %.0f us; here %.1f us (this run's own spread: %.1f us)"
                % (PARENT_US[B], g, max(us["ecamp_resample_boxes_u8 (first planes)"]) - min(us["ecamp_resample_boxes_u8 (first planes)"])))
        del cf, ct, gf, gt, rs_c, rs_g
    if args.loader_images <= 0:
        return
    from PIL import Image
    root = tempfile.mkdtemp(prefix="ecamp_image_pipeline_colour_")
    try:
        N, W, rep = args.loader_images, args.loader_workers, args.loader_repeat

        def source(k):
            return np.roll(colour[k % 4], 37 * k, axis=2)

        os.makedirs(os.path.join(root, "img"))
        lines = []
        for k in range(N):
            Image.fromarray(np.ascontiguousarray(source(k).transpose(1, 2, 0)), "RGB").save(os.path.join(root, "img", "i%d.png" % k), compress_level=1)
            lines.append("img/i%d.png %s" % (k, " ".join(str((k >> c) & 1) for c in range(C))))
        open(os.path.join(root, "train_list.txt"), "w").write("\n".join(lines * rep) + "\n")
        with U8ShardWriter(os.path.join(root, "train_list.txt.u8"), colour=True) as w:
            for _ in range(rep):
                for k in range(N):
                    w.add(np.ascontiguousarray(source(k).transpose(1, 2, 0)))
        say("17 loaders: one pass over a list of %d samples (%d colour PNG files of %d x %d, lossless, each listed %d times; the colour shard holds the same "
            "pixels as three planes per image, %.1f GB, in list order), batch 96, %d workers each, pinned memory; the pass is timed after a first pass; host: "
            "ListDataset + train_transform -> f32 [96, 3, %d, %d]; device: ShardListDataset + DeviceImageLoader -> uint8 [96, %d, %d] in HBM (three-plane boxes "
            "over PCIe, the resample and the fold included; the timed pass ends in a device synchronise)"
            % (N * rep, N, S, S, rep, os.path.getsize(os.path.join(root, "train_list.txt.u8")) / 1e9, W, R, R, R, R))
        host = DataLoader(fd.ListDataset(root, root, "train", data_volume="100", transform=fd.train_transform(R)), shuffle=True, batch_size=96, num_workers=W,
                          pin_memory=True, persistent_workers=W > 0)

        def device_loader(workers):
            return fd.DeviceImageLoader(DataLoader(fd.ShardListDataset(root, root, "train", data_volume="100", img_size=R), shuffle=True, batch_size=96,
                                                   num_workers=workers, pin_memory=True, collate_fn=fd.collate_boxes, persistent_workers=workers > 0), dev, R)

        rates, slowest = {}, {}
        for name, loader in (("host loader", host), ("device loader", device_loader(W)), ("device loader, %d workers" % (2 * W), device_loader(2 * W))):
            per = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                seen = 0
                for x, _ in loader:
                    x = x.to(dev, non_blocking=True)
                    seen += x.shape[0]
                torch.cuda.synchronize()
                per.append(seen / (time.perf_counter() - t0))
            rates[name], slowest[name] = statistics.median(per[1:]), min(per[1:])
            say("   %-26s %8.0f images/s (passes after the first: %s)" % (name, rates[name], " ".join("%.0f" % v for v in per[1:])))
            del loader
        say("   device / host = %.1f x with the same %d workers" % (rates["device loader"] / rates["host loader"], W))
        say("   the rates these must feed (profiles/finetune.txt): a fine-tune step at B = 96 runs 6 600 images/s, at B = 256 7 200 images/s.  A loader FEEDS a "
            "step when its SLOWEST timed pass is at least the step's rate:")
        for name in rates:
            say("   %-26s slowest pass %6.0f images/s -> %s" % (name, slowest[name], "; ".join(
                "fine-tune step at B = %d (%d): %s" % (B, r, "FEEDS it" if slowest[name] >= r else "does NOT feed it") for B, r in ((96, 6600), (256, 7200)))))
        say("   NOT measured: real fundus photographs are larger than %d x %d (Aptos: up to 4288 x 2848).  A training box then carries up to an order of "
            "magnitude more bytes per sample, three planes each, from the shard's pages through pinned memory and PCIe; host-to-device bytes per batch and "
            "the worker-side copy grow with them, and the rates above do not speak for that." % (S, S))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def image_resident_leg(args, say):
    """Legs (a) and (b) of `--image_pipeline --resident` (see the module docstring)."""
    import shutil
    import tempfile

    import numpy as np
    from torch.utils.data import DataLoader

    from ecamp_amd import engine_finetune
    from ecamp_amd.module import finetune_datasets as fd
    from ecamp_amd.module.classifier import build_classifier
    from ecamp_amd.module.pretrain_datasets import U8ShardWriter
    dev = torch.device("cuda")
    C, R, S = args.classes, 224, args.resident_source
    batches = [int(b) for b in args.batches.split(",")]
    N, W, rep = args.loader_images, args.loader_workers, args.loader_repeat
    say("classification image shards resident in HBM (--image_shard_resident), on %s: R = %d, sources %d x %d, training crop scales 0.08 to 1"
        % (torch.cuda.get_device_name(0), R, S, S))
    rng = np.random.default_rng(0)
    base = [np.clip(127 + 80 * np.sin(np.add.outer(np.arange(S) / (5.0 + k), np.arange(S) / (9.0 - k))) + rng.integers(-30, 31, (S, S)), 0, 255).astype(np.uint8)
            for k in range(4)]
    # the fine-tune step's rate on a uint8 batch, in this process (leg 14's block: host clock around steps that end in a device synchronise)
    torch.manual_seed(0)
    clf = build_classifier("vit_base_patch16", C, True, img_size=R, compute_dtype=torch.bfloat16, train_encoder=True).to(dev)
    step_args = argparse.Namespace(learning_rate=3e-2, weight_decay=1e-4, decay_type="cosine", warmup_steps=50, num_steps=3000, max_grad_norm=1.0)
    opt = engine_finetune.make_optimizer(clf, step_args)
    step_rate, n = {}, 0
    for B in batches:
        x = torch.randint(0, 256, (B, R, R), dtype=torch.uint8, device=dev)
        y = (torch.rand(B, C, device=dev) < 0.3).float()
        per = []
        for steps in (args.warmup, args.iters, args.iters, args.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                engine_finetune.train_step(clf, opt, x, y, n, step_args)
                n += 1
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) / max(1, steps))
        step_rate[B] = B / statistics.median(per[1:])
    del clf, opt
    torch.cuda.empty_cache()
    say("the fine-tune step (ViT-B/16, bf16, forward + backward + clip + SGD) on a resident uint8 batch, this process, median of three blocks of %d steps: %s"
        % (args.iters, ", ".join("B = %d: %.0f images/s" % (B, r) for B, r in step_rate.items())))
    for colour in ((True,) if args.colour else (False, True)):
        kind = "colour" if colour else "gray"

        def source(k):
            if colour:
                return np.roll(np.stack([base[k % 4], base[(k + 1) % 4], base[(k + 2) % 4]]), 37 * k, axis=2)
            return np.roll(base[k % 4], 37 * k, axis=1)

        root = tempfile.mkdtemp(prefix="ecamp_image_resident_")
        try:
            lines = ["img/i%d.png %s" % (k, " ".join(str((k >> c) & 1) for c in range(C))) for k in range(N)]
            open(os.path.join(root, "train_list.txt"), "w").write("\n".join(lines * rep) + "\n")
            path = os.path.join(root, "train_list.txt.u8")
            with U8ShardWriter(path, colour=colour) as w:
                for _ in range(rep):
                    for k in range(N):
                        w.add(np.ascontiguousarray(source(k).transpose(1, 2, 0)) if colour else source(k))
            shard = fd.ResidentShard(path, dev)
            say("== %s sources: a shard of %d images (%d different ones, each listed %d times), %s%d x %d" % (kind, N * rep, N, rep, "3 x " if colour else "", S, S))
            say("   upload: %d bytes resident (%.2f GB) in %.2f s = %.2f GB/s, through a pinned staging buffer of %d MB"
                % (shard.nbytes, shard.nbytes / 1e9, shard.seconds, shard.nbytes / 1e9 / shard.seconds, fd.ResidentShard.CHUNK_BYTES >> 20))
            say("(a) the call, per call (coefficients + horizontal + vertical pass), from event pairs around 10 back-to-back calls, the two alternating in one "
                "loop (%d groups after %d warm-up groups); sample b of a batch is a box in image b of the shard; the packed call gets the same boxes copied "
                "back to back" % (args.iters, args.warmup))
            data = np.memmap(path, dtype=np.uint8, mode="r")
            packed_name = "ecamp_resample_boxes_rgb_u8 (packed)" if colour else "ecamp_resample_boxes_u8 (packed)"
            for B in batches:
                torch.manual_seed(B)

                def draw(first):
                    """One batch: sample b is a box in image first + b of the shard -> (resident arguments, packed arguments, box bytes)"""
                    rows = [fd.resident_item(shard.index[(first + b) % len(shard.index)], True, R) for b in range(B)]
                    table, meta = fd.pack_resident(rows)
                    items = []
                    for r in rows:
                        off, h, w, flip = (int(v) for v in r[:4])
                        planes = [np.lib.stride_tricks.as_strided(data[off + p * int(r[11]):], shape=(h, w), strides=(int(r[10]), 1)) for p in range(3 if r[9] == 3 else 1)]
                        items.append((np.stack(planes) if colour else planes[0], bool(flip), tuple(int(v) for v in r[5:9])))
                    flat, ptable, pmeta = fd.pack_boxes(items)
                    assert pmeta == meta and torch.equal(ptable[:, 1:10], table[:, 1:10])
                    return (shard, table.to(dev), meta), (flat.to(dev), ptable.to(dev), pmeta), flat.numel()

                def rotate(rs, calls):
                    at = [0]

                    def fn():
                        rs(*calls[at[0] % len(calls)])
                        at[0] += 1
                    return fn

                sets = [draw(0)]
                rs_r, rs_p = fd.DeviceBoxResampler(dev, R), fd.DeviceBoxResampler(dev, R)
                assert torch.equal(rs_r(*sets[0][0], check=True), rs_p(*sets[0][1], check=True))      # the same bytes, before anything is timed
                while sum(n for _, _, n in sets) < args.resident_fresh_mb * 1e6:
                    sets.append(draw(len(sets) * B))
                say("   B = %3d: %.1f MB of box bytes, %d taps, tallest sample %d intermediate rows" % (B, sets[0][2] / 1e6, sets[0][0][2][0], sets[0][0][2][2]))
                for what, use in (("the same batch in every call", sets[:1]),
                                  ("another batch in every call: %d batches in rotation, %.0f MB of box bytes, more than the 256 MB Infinity Cache holds"
                                   % (len(sets), sum(n for _, _, n in sets) / 1e6), sets)):
                    us = event_groups([(packed_name, rotate(rs_p, [p for _, p, _ in use])),
                                       ("ecamp_resample_shard_u8 (resident)", rotate(rs_r, [r for r, _, _ in use]))], args.iters, args.warmup, 10)
                    say("      %s" % what)
                    med = {}
                    for name, xs in us.items():
                        med[name], lo, hi = stats(xs)
                        say("         %-40s median %8.1f us (min %.1f, max %.1f)" % (name, med[name], lo, hi))
                    spread = max(us[packed_name]) - min(us[packed_name])
                    diff = med["ecamp_resample_shard_u8 (resident)"] - med[packed_name]
                    say("         resident - packed = %+.1f us (medians); the packed call's own spread across its groups: %.1f us -> %s"
                        % (diff, spread, "not slower" if diff <= spread else "SLOWER than the packed call by more than its spread"))
                del sets, rs_r, rs_p
            del data
            if N * rep < 96:
                continue
            say("(b) loaders: one pass over the list of %d samples, batch 96, %d workers each, pinned memory, shuffled; passes after the first are timed, "
                "each ends in a device synchronise; device loader: ShardListDataset + collate_boxes (box bytes from the shard's pages over PCIe); resident "
                "loader: ShardListDataset(resident=True) + collate_resident (one table row per sample) on the uploaded shard" % (N * rep, W))

            def loader(resident):
                ds = fd.ShardListDataset(root, root, "train", data_volume="100", img_size=R, resident=resident)
                dl = DataLoader(ds, shuffle=True, batch_size=96, num_workers=W, pin_memory=True, collate_fn=fd.collate_resident if resident else fd.collate_boxes,
                                persistent_workers=W > 0)
                return fd.DeviceImageLoader(dl, dev, R, shard=shard if resident else None)

            rates, slowest = {}, {}
            for name, ld in (("device loader", loader(False)), ("resident loader", loader(True))):
                per = []
                for _ in range(4):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    seen = 0
                    for x, _ in ld:
                        seen += x.shape[0]
                    torch.cuda.synchronize()
                    per.append(seen / (time.perf_counter() - t0))
                rates[name], slowest[name] = statistics.median(per[1:]), min(per[1:])
                say("   %-18s %8.0f images/s (passes after the first: %s)" % (name, rates[name], " ".join("%.0f" % v for v in per[1:])))
                del ld
            say("   resident / device = %.2f x (medians); slowest passes: resident %.0f, device %.0f images/s -> %s"
                % (rates["resident loader"] / rates["device loader"], slowest["resident loader"], slowest["device loader"],
                   "the resident loader is not below the device loader" if slowest["resident loader"] >= slowest["device loader"]
                   else "the resident loader is BELOW the device loader: the feature is not done"))
            say("   a loader FEEDS a step when its SLOWEST timed pass is at least the step's rate (fine-tune: this process, above; probe step: 19 700 images/s, "
                "profiles/linprobe.txt):")
            for name in rates:
                verdict = ["fine-tune step at B = %d (%.0f): %s" % (B, r, "FEEDS it" if slowest[name] >= r else "does NOT feed it") for B, r in step_rate.items()]
                verdict.append("probe step (19 700): %s" % ("FEEDS it" if slowest[name] >= 19700 else "does NOT feed it"))
                say("   %-18s slowest pass %6.0f images/s -> %s" % (name, slowest[name], "; ".join(verdict)))
            del shard
        finally:
            shutil.rmtree(root, ignore_errors=True)
    say("NOT covered: pre-training's --image_shard (MIMIC-CXR shards do not fit in HBM).  NOT measured: real fundus photographs, larger than %d x %d." % (S, S))


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
    ap.add_argument("--image_pipeline", action="store_true", help="run the device-image-pipeline leg instead (profiles/finetune_image_pipeline.txt)")
    ap.add_argument("--image_pipeline_out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "finetune_image_pipeline.txt"))
    ap.add_argument("--colour", action="store_true", help="--image_pipeline: the resample and loader comparison on colour sources instead "
                                                          "(profiles/finetune_image_pipeline_colour.txt)")
    ap.add_argument("--image_pipeline_colour_out", type=str,
                    default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "finetune_image_pipeline_colour.txt"))
    ap.add_argument("--loader_images", type=int, default=384, help="--image_pipeline: PNG files of the loader comparison")
    ap.add_argument("--loader_repeat", type=int, default=8, help="--image_pipeline: times the list names each file")
    ap.add_argument("--loader_workers", type=int, default=8, help="--image_pipeline: workers of both loaders (the drivers' default)")
    ap.add_argument("--resident", action="store_true", help="--image_pipeline: the shard resident in device memory beside the packed call and the device loader, "
                                                            "gray sources then colour ones (--colour: colour alone) (profiles/finetune_image_resident.txt)")
    ap.add_argument("--resident_fresh_mb", type=float, default=600.0, help="--resident, leg (a): box bytes of the batches in rotation when every call gets another batch")
    ap.add_argument("--resident_source", type=int, default=1024, help="--resident: side of the square sources (1024: the other legs'; another value moves the rows and "
                                                                        "planes of a stored image off the power-of-two pitches)")
    ap.add_argument("--image_resident_out", type=str,
                    default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "finetune_image_resident.txt"))
    args = ap.parse_args()
    if args.resident and not args.image_pipeline:
        ap.error("--resident goes with --image_pipeline")
    if args.colour and not args.image_pipeline:
        ap.error("--colour goes with --image_pipeline")
    if not torch.cuda.is_available():
        raise SystemExit("finetune_bench needs an MI355X: nothing here can be measured on a CPU")
    if args.image_pipeline:
        lines = []

        def say_ip(msg):
            print(msg, flush=True)
            lines.append(msg)

        out = args.image_resident_out if args.resident else args.image_pipeline_colour_out if args.colour else args.image_pipeline_out
        (image_resident_leg if args.resident else image_pipeline_colour_leg if args.colour else image_pipeline_leg)(args, say_ip)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
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
