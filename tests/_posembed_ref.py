"""Float64 references for the trained position table (`--train_pos_embed`): the batch reduction of csrc/finetune.hip's
ecamp_pos_embed_grad, and the classifier of tests/test_finetune_model_gpu.py restated with `pos_embed` among the tensors that require a
gradient.

A plain helper module, not a test file: tests/test_posembed_cpu.py proves `stem_grads` against torch autograd on the CPU,
tests/test_posembed_kernel_gpu.py holds the kernel to it, tests/test_posembed_model_gpu.py the model, the engine and the driver to the
float64 classifier.  Each reference is computed once per case, shared, and never changed.
"""
import functools
import os

import torch
import torch.nn.functional as F

B, C = 4, 3
U32 = 2.0 ** -24   # the unit round-off of float32


# ---------------------------------------------------------------------------------------------------------------- the kernel's reference
def stem_grads(dx):
    """dx [B, T, D] -> (dpos [T, D], dcls [D], dbias [D]) in float64, by plain sums: S = dx summed over the batch; dpos = S, dcls = S[0],
    dbias = S[1:] summed over the tokens."""
    S = dx.double().sum(dim=0)
    return S, S[0].clone(), S[1:].sum(dim=0)


def stem_abs_sums(dx):
    """The sums of |terms| behind each output of `stem_grads`, for the error bounds: (sum_b |dx| [T, D], its row 0, sum_{b, t>=1} |dx| [D])."""
    A = dx.double().abs().sum(dim=0)
    return A, A[0].clone(), A[1:].sum(dim=0)


def stem_bounds(dx, pos0, cls0, bias0):
    """Bounds on |got - exact| per element, derived, not measured: an f32 sum in any fixed order errs by at most
    (additions a term goes through) * 2^-24 * sum |terms| to first order.  dpos / dcls: B terms and the prior value, at most B additions:
    (B + 1) * 2^-24 * (|prior| + sum_b |dx|).  dbias: B * (T - 1) terms and the prior, in a tree whose depth stays below B + T:
    (B + T) * 2^-24 * (|prior| + sum_{b, t >= 1} |dx|)."""
    Bn, T = dx.shape[0], dx.shape[1]
    A, A0, Ab = stem_abs_sums(dx)
    return ((Bn + 1) * U32 * (pos0.double().abs() + A), (Bn + 1) * U32 * (cls0.double().abs() + A0),
            (Bn + T) * U32 * (bias0.double().abs() + Ab))


def representable(shape, seed):
    """Normal values rounded to bfloat16's eight significant bits with magnitudes in [2^-6, 4], each times 2^-6, 1 or 2^6 at random:
    magnitudes in [2^-12, 256], inside IEEE half's normal range, so every value is exact in bfloat16, IEEE half and float32 alike --
    and the exponents are spread far enough (eighteen binades over eight bits) that an f32 sum of a few of them does round."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g).to(torch.bfloat16).to(torch.float32)
    x = torch.where(x.abs() < 2.0 ** -6, torch.full_like(x, 2.0 ** -6), x).clamp(-4.0, 4.0)
    return x * torch.tensor([2.0 ** -6, 1.0, 2.0 ** 6])[torch.randint(0, 3, x.shape, generator=g)]


# ---------------------------------------------------------------------------------------------------------------- the model's reference
def rel(a, b):
    """max |a - b| / max |b|"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def imgs(n=B, seed=11):
    return torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


def labels(n=B, seed=2):
    return (torch.rand(n, C, generator=torch.Generator().manual_seed(seed)) < 0.5).float()


def tail_values():
    """fc_norm and head of a classifier in mid-training: no identity norm, no vanishing head."""
    g = torch.Generator().manual_seed(5)
    return {"fc_norm.weight": 1 + 0.2 * torch.randn(192, generator=g), "fc_norm.bias": 0.1 * torch.randn(192, generator=g),
            "head.weight": 0.1 * torch.randn(C, 192, generator=g), "head.bias": 0.1 * torch.randn(C, generator=g)}


def build(dtype, dev, pool="avg", train_pos_embed=True, train_encoder=True, **kw):
    """ecamp_tiny with the oracle's recipe weights behind a multilabel classifier (train_encoder and train_pos_embed unless told
    otherwise), on `dev`."""
    from ecamp_amd.module import model_ecamp as me
    from ecamp_amd.module.classifier import ECAMPClassifier
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    torch.manual_seed(0)
    enc = me.ecamp_tiny(compute_dtype=dtype, **kw)
    enc.load_state_dict(recipe.recipe_state(orc.cfg_tiny(), seed=0), strict=True)
    clf = ECAMPClassifier(enc, C, multilabel=True, pool=pool, train_encoder=train_encoder, train_pos_embed=train_pos_embed)
    with torch.no_grad():
        for k, v in tail_values().items():
            clf.get_parameter(k).copy_(v)
    return clf.to(dev)


def trained_names(pool):
    names = ["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    for i in range(12):
        for n in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2"):
            names += ["blocks.%d.%s.weight" % (i, n), "blocks.%d.%s.bias" % (i, n)]
    names += ["norm.weight", "norm.bias"] if pool == "cls" else ["fc_norm.weight", "fc_norm.bias"]
    return names + ["head.weight", "head.bias"]


def ref_params(pool):
    """The oracle's parameters and the classifier's tail in float64; the trained ones -- `pos_embed` among them -- require a gradient."""
    from oracle import ecamp_oracle as orc
    from oracle import recipe
    cfg = orc.cfg_tiny()
    P = {k: v.double() for k, v in orc.load_state(orc.new_params(cfg), recipe.recipe_state(cfg, seed=0)).items()}
    P.update({k: v.double() for k, v in tail_values().items()})
    for k in trained_names(pool):
        P[k].requires_grad_(True)
    return P, cfg


def ref_loss(P, cfg, x, y, pool):
    from oracle import ecamp_oracle as orc
    n = x.shape[0]
    x = F.conv2d(x.double(), P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=cfg.patch_size).flatten(2).transpose(1, 2)
    x = x + P["pos_embed"][:, 1:, :]
    x = torch.cat(((P["cls_token"] + P["pos_embed"][:, :1, :]).expand(n, -1, -1), x), dim=1)
    for i in range(cfg.depth):
        x = orc.vit_block(P, "blocks.%d" % i, x, cfg.num_heads, cfg.ln_eps)
    if pool == "avg":
        feat = F.layer_norm(x[:, 1:, :].mean(dim=1), (x.shape[-1],), P["fc_norm.weight"], P["fc_norm.bias"], 1e-6)
    else:
        feat = F.layer_norm(x, (x.shape[-1],), P["norm.weight"], P["norm.bias"], cfg.ln_eps)[:, 0]
    logits = feat @ P["head.weight"].t() + P["head.bias"]
    return F.binary_cross_entropy_with_logits(logits, y.double())


def with_threads(fn):
    @functools.wraps(fn)
    def wrapped(*a, **k):
        threads = torch.get_num_threads()
        torch.set_num_threads(min(os.cpu_count() or 1, 16))
        try:
            return fn(*a, **k)
        finally:
            torch.set_num_threads(threads)     # (process-wide: given back for the tests that follow)
    return wrapped


@functools.lru_cache(maxsize=None)
@with_threads
def reference(pool):
    """One backward on the test batch -> (loss, {name: gradient}) in float64."""
    P, cfg = ref_params(pool)
    loss = ref_loss(P, cfg, imgs(), labels(), pool)
    loss.backward()
    return float(loss.detach()), {k: P[k].grad.clone() for k in trained_names(pool)}


def backward(clf, scale=1.0, x=None, y=None):
    clf.train()
    loss = clf.loss(clf(imgs() if x is None else x), labels() if y is None else y)
    (loss * scale if scale != 1.0 else loss).backward()
    clf.check_labels()
    torch.cuda.synchronize()
    return float(loss.item())
