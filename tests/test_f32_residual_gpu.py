"""ECAMP(f32_residual=True): the image encoder's and decoder's residual streams stored in f32, as the reference's autocast leaves them
(an f32 stream plus a half branch is f32: timm Block at model_ecamp.py:233-234,254-255, the stems at :222,228-230,245-251).

Kernel level: the mixed GEMM (16-bit operands, bias + f32 residual -> f32) on each kernel that serves the residual linear layers, the
LayerNorm forward with an f32 input and its backward with an f32 z, against torch in f32 / f64.  Model level: the precision and range
cases a 16-bit stream cannot represent, the golden vectors of the reference in the new mode, and the default mode left untouched."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def _build(name, dtype, dev, **kw):
    from ecamp_amd.module import model_ecamp as me
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    tiny = name.startswith("tiny")
    cfg = orc.cfg_tiny() if tiny else orc.cfg_base()
    torch.manual_seed(0)
    model = (me.ecamp_tiny if tiny else me.ecamp)(compute_dtype=dtype, **kw)
    model.load_state_dict(recipe.recipe_state(cfg, seed=0), strict=True)
    model.to(dev)
    return model, cfg


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _eps16(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


# ---------------------------------------------------------------------------------------------------------------- kernel level
# (M, N, K, kernel): the tiny model's D = 192 and a ragged M on the generic kernel, a decoder-like N = 512 on the eight-wave persistent
# kernel, the encoder's N = 768 at M = 12800 (configs[1]) and a ragged M on the four-wave 192-column kernel
GEMM_SHAPES = [(200, 192, 768, "generic"), (203, 192, 192, "generic"), (25216, 512, 2048, "q8"), (12800, 768, 768, "q16"),
               (12763, 768, 3072, "q16")]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K,kern", GEMM_SHAPES)
def test_gemm_res32_matches_torch(dev, dtype, M, N, K, kern):
    """y (f32) = x w^T + b + r (f32) against f64 on the device: the residual (1000 + N(0, 1): a 16-bit copy of it would be off by up to
    2 in bfloat16, 0.25 in half) must be added in f32 and the result never rounded to 16 bits."""
    from ecamp_amd import _lib, hip_ops as ops
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    x = torch.randn(M, K, device=dev, generator=g).to(dtype)
    w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(dtype)
    b = torch.randn(N, device=dev, generator=g)
    r = 1000.0 + torch.randn(M, N, device=dev, generator=g)
    q8, q16 = int(lib.ecamp_gemm_q8_launches()), int(lib.ecamp_gemm_q16_launches())
    y = ops.linear_fwd_res32(x, w, b, r)
    torch.cuda.synchronize()
    d8, d16 = int(lib.ecamp_gemm_q8_launches()) - q8, int(lib.ecamp_gemm_q16_launches()) - q16
    assert y.dtype == torch.float32 and y.shape == (M, N)
    assert (d8, d16) == {"generic": (0, 0), "q8": (1, 0), "q16": (0, 1)}[kern], (kern, d8, d16)
    ref = x.double() @ w.double().t() + b.double() + r.double()
    err = (y.double() - ref).abs().max().item()
    print("gemm_res32 %s %d x %d x %d (%s): max abs err %.3e" % (dtype, M, N, K, kern, err))
    assert err < 2e-3, err


LN_SHAPES = [(12800, 768), (25216, 512), (203, 192), (1000, 1024), (77, 196)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_fwd_x32_matches_torch(dev, dtype, rows, cols):
    """f32 rows at 2048 + N(0, 1) (a 16-bit copy would keep nothing of the deviations) -> 16-bit y, f32 mean / rstd, against
    F.layer_norm in f64: y to its own rounding, the statistics to f32 accuracy."""
    from ecamp_amd import hip_ops as ops
    g = torch.Generator(device=dev).manual_seed(rows * cols)
    x = 2048.0 + torch.randn(rows, cols, device=dev, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(cols, device=dev, generator=g)
    beta = 0.1 * torch.randn(cols, device=dev, generator=g)
    y, z, mean, rstd = ops.layernorm_fwd_x32(x, gamma, beta, 1e-6, dtype)
    assert y.dtype == dtype and z is x
    ref = F.layer_norm(x.double(), (cols,), gamma.double(), beta.double(), 1e-6)
    err = (y.double() - ref).abs().max().item() / ref.abs().max().item()
    xd = x.double()
    mu, var = xd.mean(1), xd.var(1, unbiased=False)
    print("ln_fwd_x32 %s %d x %d: y rel err %.2e" % (dtype, rows, cols, err))
    assert err < 2 * _eps16(dtype)
    assert (mean.double() - mu).abs().max().item() < 1e-3
    assert ((rstd.double() - (var + 1e-6).rsqrt()) / (var + 1e-6).rsqrt()).abs().max().item() < 1e-3


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_layernorm_bwd_z32_matches_autograd(dev, dtype, rows, cols):
    """The backward of an f32-input LayerNorm: 16-bit dy and dres, f32 z -> 16-bit dz = LN'(dy) + dres; dgamma / dbeta accumulated in
    f32; against torch autograd in f64."""
    from ecamp_amd import hip_ops as ops
    g = torch.Generator(device=dev).manual_seed(7 + rows * cols)
    z = 2048.0 + torch.randn(rows, cols, device=dev, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(cols, device=dev, generator=g)
    beta = 0.1 * torch.randn(cols, device=dev, generator=g)
    dy = torch.randn(rows, cols, device=dev, generator=g).to(dtype)
    dres = torch.randn(rows, cols, device=dev, generator=g).to(dtype)
    _, _, mean, rstd = ops.layernorm_fwd_x32(z, gamma, beta, 1e-6, dtype)
    gg = torch.zeros(cols, device=dev)
    gb = torch.zeros(cols, device=dev)
    dz = ops.layernorm_bwd_z32(dy, z, mean, rstd, gamma, gg, gb, dres=dres)
    zr = z.double().requires_grad_(True)
    gr = gamma.double().requires_grad_(True)
    br = beta.double().requires_grad_(True)
    F.layer_norm(zr, (cols,), gr, br, 1e-6).backward(dy.double())
    ref = zr.grad + dres.double()
    err = (dz.double() - ref).abs().max().item() / ref.abs().max().item()
    eg = (gg.double() - gr.grad).norm().item() / gr.grad.norm().item()
    eb = (gb.double() - br.grad).norm().item() / br.grad.norm().item()
    print("ln_bwd_z32 %s %d x %d: dz rel err %.2e, dgamma %.2e, dbeta %.2e" % (dtype, rows, cols, err, eg, eb))
    assert dz.dtype == dtype
    assert err < 2 * _eps16(dtype)
    assert eg < 1e-3 and eb < 1e-5


# ---------------------------------------------------------------------------------------------------------------- model level
@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 6e-2), (torch.float16, 1e-2)])
def test_block_update_on_a_large_stream_matches_the_oracle(dev, dtype, tol):
    """One VitBlockFn of the tiny golden model on x = 2048 + N(0, 1): the block's update x2 - x against oracle.vit_block in f32.  At that
    offset a 16-bit stream has a spacing of 2 (half) / 16 (bfloat16), larger than the update itself; the f32 stream keeps it."""
    from ecamp_amd.functions import VitBlockFn, f32_carrier, f32_stream
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    model, cfg = _build("tiny_b4_s128", dtype, dev, f32_residual=True)
    model.eval()
    model.prepare()
    B, T, D = 2, 50, cfg.embed_dim
    g = torch.Generator().manual_seed(3)
    x = 2048.0 + torch.randn(B * T, D, generator=g)
    with torch.no_grad():
        x2 = f32_stream(VitBlockFn.apply(f32_carrier(x.to(dev).contiguous(), dtype), model.blocks[0], model, B, T, model.num_heads))
        assert x2.dtype == torch.float32
        upd = (x2.cpu().double() - x.double())
        P = orc.load_state(orc.new_params(cfg, requires_grad=False), recipe.recipe_state(cfg, seed=0))
        ref = orc.vit_block(P, "blocks.0", x.view(B, T, D), cfg.num_heads, cfg.ln_eps).view(B * T, D).double() - x.double()
    err = (upd - ref).norm().item() / ref.norm().item()
    print("block update on a stream at 2048, %s: rel err %.3e (update norm %.3e)" % (dtype, err, ref.norm().item()))
    assert err < tol


def _big_bias_state(cfg):
    """The tiny golden parameters with four channels of mlp.fc2.bias raised to 4e4 in the first two encoder blocks: every linear layer's
    output stays inside +-65504, the encoder's residual stream passes it (8e4 after block 1)."""
    from oracle import recipe
    state = recipe.recipe_state(cfg, seed=0)
    for i in (0, 1):
        k = "blocks.%d.mlp.fc2.bias" % i
        state[k] = state[k].clone()
        state[k][:4] = 4e4
    return state


def test_fp16_stream_past_65504_stays_finite(dev):
    """--amp fp16 --f32_residual on a model whose encoder stream grows past half's range while every linear-layer output stays inside it
    (_big_bias_state).  The premise is checked on the device: the oracle's encoder blocks under torch.autocast(float16) keep a finite
    stream whose largest element passes 65504.  Then the product: finite losses within 1e-3 of the f32 oracle and finite gradients whose
    per-tensor norms are within the fp16 golden bounds (median 2e-3, worst 1e-2) of the oracle's."""
    from ecamp_amd.module import model_ecamp as me
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    cfg = orc.cfg_tiny()
    state = _big_bias_state(cfg)
    B, S = 4, 128
    batch = recipe.recipe_batch(cfg, B, S, seed=0)
    noise = recipe.recipe_noise(B, cfg.num_patches, seed=0)
    # the premise, on the device: autocast's f32 stream through the encoder blocks
    Pd = {k: v.to(dev) for k, v in orc.load_state(orc.new_params(cfg, requires_grad=False), state).items()}
    with torch.no_grad(), torch.autocast("cuda", torch.float16):
        imgs = orc.bicubic_resize(batch["image"].to(dev), cfg.img_size)
        w = Pd["patch_embed.proj.weight"]
        x = F.conv2d(imgs, w, Pd["patch_embed.proj.bias"], stride=cfg.patch_size).flatten(2).transpose(1, 2) + Pd["pos_embed"][:, 1:, :]
        x = torch.cat(((Pd["cls_token"] + Pd["pos_embed"][:, :1, :]).expand(B, -1, -1), x), 1)
        for i in range(cfg.depth):
            x = orc.vit_block(Pd, "blocks.%d" % i, x, cfg.num_heads, cfg.ln_eps)
    print("autocast encoder stream: dtype %s, max |x| %.4g" % (x.dtype, x.abs().max().item()))
    assert x.dtype == torch.float32 and torch.isfinite(x).all() and x.abs().max().item() > 65504.0
    # checker: the f32 oracle on the host
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    P = orc.set_requires_grad(orc.load_state(orc.new_params(cfg), state), cfg)
    ref = orc.forward(P, cfg, batch, 0.75, noise)
    sum(ref).backward()
    # product
    lscale = 65536.0
    torch.manual_seed(0)
    model = me.ecamp_tiny(compute_dtype=torch.float16, f32_residual=True)
    model.load_state_dict(state, strict=True)
    model.to(dev).eval()
    out = model(batch, noise=noise)
    losses = np.array([t.item() for t in out])
    ref_l = np.array([t.item() for t in ref])
    print("losses", losses, "oracle", ref_l)
    assert np.isfinite(losses).all()
    assert (np.abs(losses - ref_l) / np.abs(ref_l)).max() < 1e-3
    (sum(out) * lscale).backward()
    named = dict(model.named_parameters())
    errs = []
    for n, p in P.items():
        if p.grad is None or n not in named or named[n].grad is None:
            continue
        gq = named[n].grad.double().cpu() / lscale
        assert torch.isfinite(gq).all(), n
        gn = p.grad.double().norm().item()
        if gn > 1e-3 * max(q.grad.double().norm().item() for q in P.values() if q.grad is not None):
            errs.append(abs(gq.norm().item() - gn) / gn)
    errs = np.array(errs)
    print("grad-norm rel err: median %.2e worst %.2e over %d tensors" % (np.median(errs), errs.max(), len(errs)))
    assert np.median(errs) < 2e-3 and errs.max() < 1e-2


def _golden_case(dev, name, dtype, loss_tol, med_tol, max_tol, act_tol, lscale):
    """tests/test_model_gpu.py's golden case (losses, activation digests, per-tensor gradient norms) with f32_residual=True."""
    from oracle import recipe
    from oracle.make_golden import digest
    g = _load(name)
    B, S = int(g["meta/B"]), int(g["meta/S"])
    model, cfg = _build(name, dtype, dev, f32_residual=True)
    model.eval()
    model.keep_aux = True
    mim, res, mlm = model(recipe.recipe_batch(cfg, B, S, seed=0), mask_ratio=0.75, noise=recipe.recipe_noise(B, cfg.num_patches, seed=0))
    losses = np.array([mim.item(), res.item(), mlm.item()])
    print(name, dtype, "f32 residual: losses rel", np.abs(losses - g["losses"]) / g["losses"])
    assert (np.abs(losses - g["losses"]) / g["losses"]).max() < loss_tol
    aux, L = model._aux, cfg.num_patches
    acts = {"latent": aux["latent"], "pred": aux["pred"].view(B, L + 1, -1)[:, 1:], "pred_img": aux["pred_img"], "fused": aux["fused"],
            "seq_out": aux["seq_out"], "logits": aux["logits"].view(B, S, -1)}
    for k, t in acts.items():
        nm, s = digest(t.float().cpu())
        e = max(_rel(nm[0], g["act/%s/nm" % k][0]), _rel(s, g["act/%s/s" % k]))
        print("  act %-10s rel err %.2e" % (k, e))
        assert e < act_tol, (k, e)
    ((mim + res + mlm) * lscale).backward()
    names = list(g["grad/names"])
    params = dict(model.named_parameters())
    norms = np.array([params[n].grad.double().norm().item() / lscale for n in names])
    big = g["grad/norms"] > 1e-3 * g["grad/norms"].max()
    e = np.abs(norms - g["grad/norms"])[big] / g["grad/norms"][big]
    print("  grad-norm rel err: median %.2e max %.2e" % (np.median(e), e.max()))
    assert np.median(e) < med_tol and e.max() < max_tol


@pytest.mark.parametrize("name", ["tiny_b4_s128", "base_b2_s128"])
def test_golden_fp16_f32_residual(dev, name):
    """fp16 + f32 residual against the reference's golden vectors, the bounds of the fp16 golden test (losses 1e-3, activations 4e-3,
    gradient norms median 2e-3 / worst 1e-2), loss scaled by GradScaler's initial 65536."""
    _golden_case(dev, name, torch.float16, 1e-3, 2e-3, 1e-2, 4e-3, 65536.0)


@pytest.mark.parametrize("name", ["tiny_b4_s128", "base_b2_s128"])
def test_golden_bf16_f32_residual(dev, name):
    """bf16 + f32 residual against the golden vectors with the bf16 bounds (losses 3e-2, activations 3e-2, gradient norms 1e-2 / 6e-2)."""
    _golden_case(dev, name, torch.bfloat16, 3e-2, 1e-2, 6e-2, 3e-2, 1.0)


def test_engine_step_fp16_f32_residual_matches_reference(dev):
    """tests/test_model_gpu.py's fp16 engine step (accum_iter 2, device-side GradScaler, one AdamW step) with f32_residual=True against the
    golden 'engine/*' of the tiny config, with the same bounds: logged losses 1e-3, gradient norm 5e-3, sampled updates 1e-1."""
    from ecamp_amd import optim
    from ecamp_amd.util.misc import NativeScalerWithGradNormCount
    from oracle import recipe
    from oracle.make_golden import GRAD_SAMPLE_KEYS, digest
    name = "tiny_b4_s128"
    g = _load(name)
    B, S = int(g["meta/B"]), int(g["meta/S"])
    model, cfg = _build(name, torch.float16, dev, f32_residual=True)
    model.eval()
    model.prepare()
    opt = optim.FusedAdamW(optim.add_weight_decay(model, 0.05), lr=1.5e-4, betas=(0.9, 0.95))
    scaler = NativeScalerWithGradNormCount(dynamic=True)
    opt.zero_grad()
    logged, norm = [], None
    for it in range(2):
        batch = recipe.recipe_batch(cfg, B, S, seed=10 + it)
        noise = recipe.recipe_noise(B, cfg.num_patches, seed=10 + it)
        mim, res, mlm = model(batch, noise=noise)
        logged.append([mim.item(), res.item(), mlm.item()])
        norm = scaler((mim + res + mlm) / 2, opt, parameters=model.parameters(), update_grad=(it == 1))
    assert scaler.last_step_fused and scaler.skipped_steps == 0 and scaler.get_scale() == 65536.0 and opt.steps_taken == 1
    print("  logged rel", _rel(np.array(logged), g["engine/logged"]), "norm", norm.item(), float(g["engine/grad_norm"]))
    assert _rel(np.array(logged), g["engine/logged"]) < 1e-3
    assert _rel(norm.item(), float(g["engine/grad_norm"])) < 5e-3
    old = recipe.recipe_state(cfg, seed=0)
    params = dict(model.named_parameters())
    for n in GRAD_SAMPLE_KEYS:
        _, s_new = digest(params[n].detach().float().cpu())
        _, s_old = digest(old[n])
        upd, upd_ref = s_new - s_old, g["engine/param/%s/s" % n] - s_old
        e = np.linalg.norm(upd - upd_ref) / (np.linalg.norm(upd_ref) + 1e-30)
        assert e < 1e-1, (n, e)


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 6e-2), (torch.float16, 8e-3)])
def test_visualization_forward_f32_residual(dev, dtype, tol):
    """forward_visualization runs the encoder through VitBlockFn and so inherits the mode: against vis_base_b2_s128 with the bounds of
    the default-mode test."""
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    from oracle.make_golden import digest
    g = _load("vis_base_b2_s128")
    B, S = int(g["meta/B"]), int(g["meta/S"])
    model, cfg = _build("base_b2_s128", dtype, dev, f32_residual=True)
    model.eval()
    batch = recipe.recipe_batch(cfg, B, S, seed=0)
    imgs = orc.bicubic_resize(batch["image"], cfg.img_size)
    probs = model.forward_visualization(imgs, batch["ids"], batch["attention_mask"], batch["type_ids"], mask_ratio=0,
                                        noise=recipe.recipe_noise(B, cfg.num_patches, seed=0))
    p = probs.cpu()
    nm, s = digest(p)
    print("vis f32 residual", dtype, "norm rel", _rel(nm[0], g["probs/nm"][0]), "sample rel", _rel(s, g["probs/s"]))
    assert _rel(nm[0], g["probs/nm"][0]) < tol and _rel(s, g["probs/s"]) < tol and _rel(p[:, :, 4].numpy(), g["probs_tok4"]) < tol


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_flag_off_is_identical_to_the_default(dev, dtype):
    """f32_residual=False builds the model a constructor without the argument builds: the same losses and gradient arena.  The loss sums
    and a few weight gradients leave their kernels through float atomics, whose summation order varies run to run, so "identical" is
    asserted to f32 rounding of those sums (as the image-schema test of tests/test_model_gpu.py does); a 16-bit rounding anywhere on
    the way would be orders of magnitude larger."""
    from ecamp_amd.module import model_ecamp as me
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    cfg = orc.cfg_tiny()
    state = recipe.recipe_state(cfg, seed=0)
    batch = recipe.recipe_batch(cfg, 4, 64, seed=2)
    noise = recipe.recipe_noise(4, cfg.num_patches, seed=2)
    res = []
    for kw in ({}, {"f32_residual": False}):
        torch.manual_seed(0)
        m = me.ecamp_tiny(compute_dtype=dtype, **kw)
        assert m.f32_residual is False
        m.load_state_dict(state, strict=True)
        m.to(dev).eval()
        arena = m.prepare()
        arena.flat_g.zero_()
        out = m(batch, noise=noise)
        sum(out).backward()
        torch.cuda.synchronize()
        res.append((torch.stack([t.detach() for t in out]).cpu(), arena.flat_g.clone()))
    assert float(((res[0][0] - res[1][0]).abs() / res[1][0].abs()).max()) < 2e-6, (res[0][0], res[1][0])
    d = float((res[0][1] - res[1][1]).abs().max() / res[1][1].abs().max())
    print("flag off vs no argument (%s): gradient arena max rel diff %.2e" % (dtype, d))
    assert d < 1e-5
