"""Float64 restatement of a ViT block under stochastic depth, and of the classifier's loss with it: timm's Block with
DropPath(scale_by_keep=True) on both residual branches, `x + keep[:, None, None] / (1 - p) * branch(x)`, over the oracle's parameter dict
(oracle.ecamp_oracle.vit_block is the same block without it).

A plain helper module, not a test file: tests/test_droppath_cpu.py proves it against the oracle's block, tests/test_droppath_model_gpu.py
holds the HIP path to it under the masks the kernels drew.
"""
import torch
import torch.nn.functional as F


def f32(x):
    """The float32 nearest to x, as a Python float (the C ABI takes the rate as `float`)."""
    return float(torch.tensor(x, dtype=torch.float32).item())


def vit_block_droppath(P, pre, x, heads, eps, keep_attn, keep_mlp, p):
    """oracle.vit_block with per-sample keep masks ([B], 1 = kept) on the attention and the MLP branch and rate p: a kept sample's branch
    is scaled by 1 / (1 - p), a dropped one contributes nothing.  All-ones masks and p = 0 give oracle.vit_block's operations exactly."""
    from oracle import ecamp_oracle as orc
    B, T, D = x.shape
    hd = D // heads
    s1 = (keep_attn.to(x.dtype) / (1.0 - p)).view(B, 1, 1)
    s2 = (keep_mlp.to(x.dtype) / (1.0 - p)).view(B, 1, 1)
    h = orc._ln(P, pre + ".norm1", x, eps)
    qkv = orc._lin(P, pre + ".attn.qkv", h).reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    att = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(dim=-1)
    a = (att @ v).transpose(1, 2).reshape(B, T, D)
    x = x + s1 * orc._lin(P, pre + ".attn.proj", a)
    h = orc._ln(P, pre + ".norm2", x, eps)
    x = x + s2 * orc._lin(P, pre + ".mlp.fc2", F.gelu(orc._lin(P, pre + ".mlp.fc1", h)))
    return x


def classifier_loss(P, cfg, imgs, y, multilabel, pool, rates, masks):
    """tests/test_finetune_model_gpu.py::_ref_loss with stochastic depth: `rates[i]` is block i's rate, `masks[i]` its pair of keep masks
    (attention, MLP) or None where the rate is 0 (the block then runs oracle.vit_block itself)."""
    from oracle import ecamp_oracle as orc
    n = imgs.shape[0]
    x = F.conv2d(imgs.double(), P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=cfg.patch_size).flatten(2).transpose(1, 2)
    x = x + P["pos_embed"][:, 1:, :]
    x = torch.cat(((P["cls_token"] + P["pos_embed"][:, :1, :]).expand(n, -1, -1), x), dim=1)
    for i in range(cfg.depth):
        if rates[i] > 0:
            x = vit_block_droppath(P, "blocks.%d" % i, x, cfg.num_heads, cfg.ln_eps, masks[i][0], masks[i][1], rates[i])
        else:
            x = orc.vit_block(P, "blocks.%d" % i, x, cfg.num_heads, cfg.ln_eps)
    if pool == "avg":
        feat = F.layer_norm(x[:, 1:, :].mean(dim=1), (x.shape[-1],), P["fc_norm.weight"], P["fc_norm.bias"], 1e-6)
    else:
        feat = F.layer_norm(x, (x.shape[-1],), P["norm.weight"], P["norm.bias"], cfg.ln_eps)[:, 0]
    logits = feat @ P["head.weight"].t() + P["head.bias"]
    return F.binary_cross_entropy_with_logits(logits, y.double()) if multilabel else F.cross_entropy(logits, y.reshape(-1).long())
