"""Linear-probe classifier on the frozen pre-trained image encoder -- the `--mode LinearProbe` share of
ECAMP/Fine-tuning/Classification (models_vit.py:61-97, train.py:115-166), MI355X-native.

`ECAMPClassifier` wraps an `ECAMP` instance and runs ITS encoder stages (StemFn, VitBlockFn, NormFn over the model's parameter arena)
forward only, with every patch kept; what it adds sits behind the last block: token mean + `fc_norm` in one kernel
(`ecamp_pool_norm`), the head (`ecamp_cls_head_fwd` / `ecamp_cls_head_wgrad`) and its loss (`ecamp_cls_loss`).  `fc_norm` and `head` are
plain f32 parameters of this module, outside the wrapped model's arena and state dict.

`ECAMPClassifier(..., train_encoder=True)` is the `--mode Finetune` share (train.py:144-166): in training mode `forward` runs the same
stages with their hand-written backwards (StemFn, VitBlockFn, then PoolNormFn or NormFn) so that the loss reaches every encoder
parameter; `fc_norm` and `head` then live in a small flat buffer of their own (arena.FlatTail) which the fused SGD step updates beside
the arena.  `pos_embed` stays the fixed sin-cos table unless `train_pos_embed=True` (default False; timm's pos_embed is a trained
parameter, so the reference trains it): `pos_embed.requires_grad` is then turned on before the encoder's arena is built, the arena places
it like any other trained tensor (gradient view, block table, the fused SGD step with the one clip coefficient and weight decay), and
StemFn's backward forms its gradient -- dx summed over the batch -- together with the bias and cls_token gradients in one fixed-order
pass (`ecamp_pos_embed_grad`).  Forward, eval and checkpoints read and write the trained table.

Stochastic depth: `drop_path_rate` (default 0.0: none; the reference builds its ViT with drop_path_rate=0.1, train.py:127) gives block i
the rate linspace(0, rate, depth)[i], timm's rule, and the differentiable training path hands each block its rate (VitBlockFn: timm
DropPath per sample on both residual branches, csrc/droppath.hip).  Forward-only runs -- eval(), no_grad, `forward_features` -- apply
none, as timm does outside training: they compute the bits of a rate-0 model and leave the Philox counter alone.
"""
import os

import torch
import torch.nn as nn

ENCODER_PREFIXES = ("cls_token", "pos_embed", "patch_embed.proj.", "blocks.", "norm.")


def _is_encoder_key(k):
    return k in ("cls_token", "pos_embed") or k.startswith(ENCODER_PREFIXES[2:])


class ECAMPClassifier(nn.Module):
    def __init__(self, encoder, num_classes, multilabel=True, pool="avg", train_encoder=False, drop_path_rate=0.0, train_pos_embed=False):
        super().__init__()
        if train_pos_embed and not train_encoder:
            raise ValueError("train_pos_embed=True needs train_encoder=True (the linear probe's encoder is frozen)")
        rate = float(drop_path_rate)
        if not 0.0 <= rate < 1.0:
            raise ValueError("drop_path_rate must lie in [0, 1), got %r" % (drop_path_rate,))
        if rate > 0 and getattr(encoder, "fp8_forward", False):
            raise ValueError("drop_path_rate > 0 is not implemented beside fp8_forward (fine-tuning does not use the fp8 forward)")
        if pool not in ("avg", "cls"):
            raise ValueError("pool must be 'avg' (the reference's global_pool=True) or 'cls', got %r" % (pool,))
        if not 1 <= int(num_classes) <= 64:
            raise ValueError("num_classes must lie in [1, 64] (the head kernels' range), got %r" % (num_classes,))
        self.encoder = encoder
        self.num_classes, self.multilabel, self.pool = int(num_classes), bool(multilabel), pool
        D = encoder.embed_dim
        self.fc_norm = nn.LayerNorm(D, eps=1e-6)          # models_vit.py:69-71 (identity initialisation)
        self.head = nn.Linear(D, self.num_classes)
        nn.init.trunc_normal_(self.head.weight, std=2e-5)   # train.py:148
        nn.init.zeros_(self.head.bias)
        self.last_counts = None    # int64[2] on the device after `loss`: [rows seen, rows predicted right]
        self.bad_label = None      # int32[1] on the device: 1 once ANY `loss` call since the last `check_labels` saw a label outside [0, C)
        self._noise = {}
        self.train_encoder = bool(train_encoder)   # False: the linear probe, exactly; True: `forward` is differentiable down to the stem
        # a trained pos_embed must be in the arena: the flag is turned on before `prepare()` builds it (and survives `.to()`, which keeps
        # requires_grad and drops the arena); an arena that was built without it is not rebuilt behind its owner's back
        self.train_pos_embed = bool(train_pos_embed)
        if self.train_pos_embed:
            arena = getattr(encoder, "arena", None)
            if arena is not None and id(encoder.pos_embed) not in arena.index:
                raise RuntimeError("train_pos_embed=True: the encoder's parameter arena was already built without pos_embed; wrap the model "
                                   "before its first forward / prepare()")
            encoder.pos_embed.requires_grad_(True)
        self._tail = None          # arena.FlatTail over fc_norm and head (train_encoder only; built on the device, on first use)
        # stochastic depth per block: timm's torch.linspace(0, rate, depth), each value rounded to float32 once (the C ABI takes `float`);
        # block 0 always has rate 0 and keeps the fused residual epilogues
        self.drop_path_rate = rate
        self.drop_path_rates = [float(v) for v in torch.linspace(0, rate, len(encoder.blocks), dtype=torch.float32).tolist()]

    # ---------------------------------------------------------------------------------------------
    def _identity_noise(self, B, dev):
        """Ascending masking noise: argsort is the identity, every patch is kept in place -- and the model's Philox counter is not
        advanced, so a pre-training run that probes between epochs draws the masks it would have drawn."""
        L = self.encoder.num_patches
        key = (B, L, str(dev))
        if key not in self._noise:
            self._noise = {key: (torch.arange(L, dtype=torch.float32, device=dev) / L).expand(B, L).contiguous()}
        return self._noise[key]

    def _features(self, imgs, pool, drop_path=False):
        """The encoder body, imgs f32 [B, 3, R, R] (or the uint8 grayscale bytes [B, R, R] / [B, 1, R, R] before ToTensor / Normalize: the
        same bits) -> f32 [B, D]: stem, blocks, then "avg": the mean of the patch tokens of the last
        block's output and `fc_norm` (global_pool=True; the encoder's own `norm` is not applied); "cls": `norm(x)[:, 0]`
        (models_vit.py:78-97).  Every patch is kept in place (identity noise, ratio 0: the Philox counter is not advanced).  Differentiable
        down to the stem where gradients are enabled; under no_grad the same kernels in the same order, hence the same bits.
        `drop_path`: hand every block its stochastic-depth rate (`forward` does on the differentiable training path only; a block of rate
        0 runs the body it always ran, and only blocks of a rate above 0 draw from the Philox counter, two pairs each)."""
        from ..functions import NormFn, PoolNormFn, StemFn, VitBlockFn
        m = self.encoder
        A = m.prepare()
        R = m.img_size
        lut = None
        if imgs.dtype == torch.uint8:
            # the device image pipeline's item (finetune_datasets.DeviceImageLoader): the grayscale bytes before ToTensor / Normalize; the
            # stem normalises them through the table of the classification constants while it gathers the patches (ecamp_im2col_u8)
            if tuple(imgs.shape[1:]) not in ((R, R), (1, R, R)):
                raise ValueError("uint8 imgs must be [B,%d,%d] or [B,1,%d,%d], got %s" % (R, R, R, R, tuple(imgs.shape)))
            from .. import hip_ops as ops
            from .finetune_datasets import FT_MEAN, FT_STD
            imgs = imgs.to(A.device, non_blocking=True).reshape(imgs.shape[0], R, R).contiguous()
            lut = ops.image_lut(A.device, FT_MEAN, FT_STD)
        else:
            imgs = imgs.to(A.device, dtype=torch.float32, non_blocking=True).contiguous()
            if imgs.dim() != 4 or imgs.shape[1:] != (3, R, R):
                raise ValueError("imgs must be f32 [B,3,%d,%d] (or uint8 [B,%d,%d]), got %s" % (R, R, R, R, tuple(imgs.shape)))
        B = imgs.shape[0]
        x, _, _, _, ids_keep = StemFn.apply(imgs, self._identity_noise(B, A.device), m, 0.0, m.cls_token, lut)
        T = ids_keep.shape[1] + 1
        for i, blk in enumerate(m.blocks):
            if drop_path and self.drop_path_rates[i] > 0:
                x = VitBlockFn.apply(x, blk, m, B, T, m.num_heads, self.drop_path_rates[i])
            else:
                x = VitBlockFn.apply(x, blk, m, B, T, m.num_heads)
        if pool == "cls":
            return NormFn.apply(x, m.norm, m).view(B, T, -1)[:, 0].float().contiguous()
        return PoolNormFn.apply(x, self.fc_norm.weight, self.fc_norm.bias, m, B, T, self.fc_norm.eps)

    def forward_features(self, imgs, pool=None):
        """`_features` forward only (`pool`: "avg" or "cls" instead of the model's own).  No gradient, and no stochastic depth whatever
        `training` says (timm applies DropPath in training only; the blocks have no other dropout): the bits are those of a
        drop_path_rate=0 model, and the modes, the Philox counter, the gradient arena and every `.grad` are left as they were."""
        pool = self.pool if pool is None else pool
        if pool not in ("avg", "cls"):
            raise ValueError("pool must be 'avg' or 'cls', got %r" % (pool,))
        with torch.no_grad():
            return self._features(imgs, pool)

    def forward(self, imgs):
        """-> logits f32 [B, C].  Differentiable with respect to `head` only -- except on a `train_encoder=True` model in training mode
        with gradients enabled, where the encoder stages run with their backwards and fc_norm / head sit in `tail()`.  That path alone
        depends on `training`: it is where stochastic depth (drop_path_rate > 0) is applied."""
        from ..functions import ClsHeadFn
        if self.train_encoder and self.training and torch.is_grad_enabled():
            self.tail()
            feat = self._features(imgs, self.pool, drop_path=self.drop_path_rate > 0)
        else:
            feat = self.forward_features(imgs)
        return ClsHeadFn.apply(feat, self.head.weight, self.head.bias)

    def tail(self):
        """The flat buffer of `fc_norm` and `head` (train_encoder=True only; built where the parameters are, rebuilt after `.to()`)."""
        if not self.train_encoder:
            raise RuntimeError("ECAMPClassifier.tail(): only a train_encoder=True model keeps fc_norm and head in a flat buffer")
        if self._tail is None or not self._tail.owns():
            from ..arena import FlatTail
            self.encoder.prepare()
            self._tail = FlatTail([("fc_norm.weight", self.fc_norm.weight), ("fc_norm.bias", self.fc_norm.bias),
                                   ("head.weight", self.head.weight), ("head.bias", self.head.bias)])
        else:
            self._tail.attach_grads()
        return self._tail

    def finetune_parameters(self):
        """[(name, parameter)] of what `--mode Finetune` trains, named as the reference's flat layout names them: the encoder's cls_token,
        patch_embed.proj.* and blocks.*, `norm.*` only when it is used (pool="cls"), `fc_norm.*` only when it is (pool="avg"), head.*.
        `pos_embed` only with `train_pos_embed` (otherwise it is the fixed sin-cos table: requires_grad=False, outside the arena);
        decoder and report side are not trained."""
        out = []
        for k, p in self.encoder.named_parameters():
            if k == "cls_token" or (k == "pos_embed" and self.train_pos_embed) or k.startswith(("patch_embed.proj.", "blocks.")) or (k.startswith("norm.") and self.pool == "cls"):
                out.append((k, p))
        if self.pool == "avg":
            out += [("fc_norm.weight", self.fc_norm.weight), ("fc_norm.bias", self.fc_norm.bias)]
        return out + [("head.weight", self.head.weight), ("head.bias", self.head.bias)]

    def loss(self, logits, y):
        """BCEWithLogitsLoss against multi-hot y [B, C] (multilabel) or CrossEntropyLoss against class indices y [B] / [B, 1]
        (train.py:118-121,422-425,442-447) -> scalar.  `last_counts` keeps the kernel's counts; its label flag is folded into
        `bad_label`, which stays set until `check_labels` has reported it."""
        from ..functions import ClsLossFn
        y = y.to(logits.device, non_blocking=True)
        if self.multilabel:
            y = y.to(torch.float32).reshape(logits.shape).contiguous()
        else:
            y = y.reshape(-1).to(torch.int64).contiguous()
        loss, self.last_counts, bad = ClsLossFn.apply(logits, y, 0 if self.multilabel else 1)
        self.bad_label = bad if self.bad_label is None else torch.maximum(self.bad_label, bad)   # (4 bytes on the device, no read-back)
        return loss

    def check_labels(self):
        """Raise if any `loss` call since the last check saw a class index outside [0, C) (such a row got a zero loss and gradient), and
        clear the flag.  Reads the device: call it where the loss is read."""
        from .. import hip_ops as ops
        bad, self.bad_label = self.bad_label, None
        if bad is not None:
            ops.cls_check_labels(bad, self.num_classes)

    # ---------------------------------------------------------------------------------------------
    def load_pretrained(self, path_or_state):
        """Takes (a) a pre-training checkpoint `{"model": state}` of this project or of the reference (train.py:131-142): the encoder's
        keys are loaded, the rest of the wrapped model keeps its initialisation and goes unused; (b) a flat timm-keyed state dict as
        the reference's save_model_auc / save_model_acc write it (train.py:84-95): encoder keys plus `fc_norm.*` / `head.*`.  A
        `head` of another shape is dropped with a message (train.py:136-139).  -> the list of keys that were loaded."""
        sd = path_or_state
        if isinstance(sd, (str, os.PathLike)):
            # (weights_only=False as util/misc.load_model: a pre-training checkpoint also holds its argparse.Namespace and optimizer state)
            sd = torch.load(sd, map_location="cpu", weights_only=False)
        if isinstance(sd, dict) and isinstance(sd.get("model"), dict):
            sd = sd["model"]
        enc = {k: v for k, v in sd.items() if _is_encoder_key(k)}
        if not any(k.startswith("blocks.") for k in enc):
            raise ValueError("load_pretrained: no image-encoder keys (cls_token, pos_embed, patch_embed.proj.*, blocks.*) in the checkpoint")
        want = {k for k in self.encoder.state_dict() if _is_encoder_key(k)}
        unknown = sorted(set(enc) - want)
        if unknown:
            raise ValueError("load_pretrained: encoder keys this model does not have: %s" % ", ".join(unknown[:8]))
        missing = sorted(k for k in want - set(enc) if not (k.startswith("norm.") and self.pool == "avg"))   # global_pool deletes `norm`
        if missing:
            raise ValueError("load_pretrained: the checkpoint lacks encoder keys: %s" % ", ".join(missing[:8]))
        self.encoder.load_state_dict(enc, strict=False)
        loaded = sorted(enc)
        own = self.state_dict()
        for k in ("fc_norm.weight", "fc_norm.bias", "head.weight", "head.bias"):
            if k not in sd:
                continue
            if k.startswith("head.") and tuple(sd[k].shape) != tuple(own[k].shape):
                print("Removing key %s from pretrained checkpoint (shape %s, this head has %s)" % (k, tuple(sd[k].shape), tuple(own[k].shape)))
                continue
            with torch.no_grad():
                own[k].copy_(sd[k].to(torch.float32))
            loaded.append(k)
        return loaded

    def reference_state_dict(self):
        """The flat timm-keyed layout of the reference's classifier (models_vit.VisionTransformer: cls_token, pos_embed,
        patch_embed.proj.*, blocks.*, head.*, and fc_norm.* with global pooling / norm.* without), f32 on the CPU: what the
        reference's `--stage test` loads (train.py:98-112)."""
        out = {}
        for k, v in self.encoder.state_dict().items():
            if _is_encoder_key(k) and not (k.startswith("norm.") and self.pool == "avg"):
                out[k] = v.detach().to("cpu", torch.float32).clone()
        if self.pool == "avg":
            for k, v in self.fc_norm.state_dict().items():
                out["fc_norm." + k] = v.detach().to("cpu", torch.float32).clone()
        for k, v in self.head.state_dict().items():
            out["head." + k] = v.detach().to("cpu", torch.float32).clone()
        return out


# the encoders of model_ecamp's factories (ecamp_tiny / ecamp / ecamp_large_448) under the reference's `--model` names (train.py:514;
# models_vit.py:117-143).  vit_tiny_patch16 keeps this project's 3 heads of 64: the reference's 12 heads of 16 are below the attention
# kernels' head widths, and no pre-trained tiny checkpoint of the reference exists.
_ENCODERS = {"vit_tiny_patch16": dict(embed_dim=192, depth=12, num_heads=3), "vit_base_patch16": dict(embed_dim=768, depth=12, num_heads=12),
             "vit_large_patch16": dict(embed_dim=1024, depth=24, num_heads=16)}


def build_classifier(model_name, num_classes, multilabel, img_size=224, pool="avg", train_encoder=False, drop_path_rate=0.0,
                     train_pos_embed=False, **kwargs):
    """The reference's `--model` name -> an ECAMPClassifier around an ECAMP with that encoder at `img_size` (decoder and report side
    as the pre-training factories build them, so a pre-training checkpoint's encoder keys fit).  `drop_path_rate`: the stochastic-depth
    rate of the last block (ECAMPClassifier; the reference's is 0.1, train.py:127).  `train_pos_embed`: train the position table as the
    reference does (needs train_encoder=True)."""
    from functools import partial

    from .bert_config import BertConfig
    from .model_ecamp import ECAMP
    if model_name not in _ENCODERS:
        raise ValueError("--model must be one of %s, got %r" % (", ".join(sorted(_ENCODERS)), model_name))
    if not 0.0 <= float(drop_path_rate) < 1.0:
        raise ValueError("drop_path_rate must lie in [0, 1), got %r" % (drop_path_rate,))
    if train_pos_embed and not train_encoder:
        raise ValueError("train_pos_embed=True needs train_encoder=True (the linear probe's encoder is frozen)")
    if model_name == "vit_tiny_patch16":
        kwargs.setdefault("bert_config", BertConfig(num_hidden_layers=2))
    enc = ECAMP(img_size=img_size, patch_size=16, in_chans=3, decoder_embed_dim=512, decoder_depth=4, decoder_num_heads=16, mlp_ratio=4,
                norm_layer=partial(nn.LayerNorm, eps=1e-6), **_ENCODERS[model_name], **kwargs)
    return ECAMPClassifier(enc, num_classes, multilabel=multilabel, pool=pool, train_encoder=train_encoder, drop_path_rate=drop_path_rate,
                           train_pos_embed=train_pos_embed)
