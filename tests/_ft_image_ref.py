"""NumPy restatement of what csrc/augment.hip's ecamp_resample_boxes_u8 computes, for the tests of the classification image pipeline:
Pillow's two-pass antialiased resample (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the 8bpc horizontal and
vertical passes) with a filter argument and, per axis, `full` and `shift`: output index x of an axis is index u = x + shift of a resize of
that axis from its size to `full`; u outside [0, full) has no tap and yields (2^21) >> 22 = 0.  tests/test_ft_image_cpu.py holds it to
Pillow's own bytes; the GPU tests hold the kernels to Pillow and to it."""
import math

import numpy as np

PRECISION_BITS = 22
BILINEAR, BICUBIC = 0, 1

# the cases of the issue: evaluation (h, w, size, ratio) and training (h, w, out)
EVAL_CASES = [(37, 53, 16, 1), (53, 37, 16, 1), (16, 16, 16, 1), (40, 16, 16, 1), (61, 47, 16, 2), (20, 90, 16, 1.3), (9, 11, 16, 1), (33, 33, 16, 0.7)]
TRAIN_CASES = [(37, 53, 16), (5, 7, 16), (16, 90, 16), (200, 150, 16)]


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {BILINEAR: (_bilinear, 1.0), BICUBIC: (_bicubic, 2.0)}


def ksize(in_size, full, filt=BILINEAR):
    """Pillow's tap count of a resize from in_size to full."""
    return int(math.ceil(FILTERS[filt][1] * max(1.0, in_size / full))) * 2 + 1


def coeffs(in_size, full, shift, out, filt=BILINEAR):
    """-> (bounds int [out, 2] = (first input index, tap count), taps int32 [out, ksize]) of output indices shift .. shift + out - 1 of a
    resize from in_size to full; an index outside [0, full) has tap count 0."""
    f, sup = FILTERS[filt]
    scale = in_size / full
    filterscale = max(scale, 1.0)
    support = sup * filterscale
    k = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out, 2), dtype=np.int64)
    kk = np.zeros((out, k), dtype=np.int64)
    ss = 1.0 / filterscale
    for x in range(out):
        u = x + shift
        if u < 0 or u >= full:
            continue
        center = (u + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [f((i + xmin - center + 0.5) * ss) for i in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for i, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[x, i] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[x] = (xmin, xmax)
    return bounds, kk


def _clip8(v):
    return np.clip(v >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resample_box(img, out, geom, flip=False, filt=BILINEAR):
    """img uint8 [h, w]; geom = (full_w, shift_w, full_h, shift_h) -> uint8 [out, out]: horizontal pass to a uint8 intermediate [h, out], then
    the vertical pass, then the flip."""
    h, w = img.shape
    fw, sw, fh, sh = geom
    bh, kh = coeffs(w, fw, sw, out, filt)
    bv, kv = coeffs(h, fh, sh, out, filt)
    src = img.astype(np.int64)
    tmp = np.zeros((h, out), dtype=np.uint8)
    for x in range(out):
        x0, n = bh[x]
        tmp[:, x] = _clip8((1 << (PRECISION_BITS - 1)) + src[:, x0:x0 + n] @ kh[x, :n])
    t = tmp.astype(np.int64)
    dst = np.zeros((out, out), dtype=np.uint8)
    for y in range(out):
        y0, n = bv[y]
        dst[y] = _clip8((1 << (PRECISION_BITS - 1)) + kv[y, :n] @ t[y0:y0 + n])
    return dst[:, ::-1].copy() if flip else dst


def gray_image(h, w, seed):
    """A uint8 test image with structure at every scale (so that a wrong tap or a wrong bound changes bytes)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 90 * np.sin(x / 3.1 + seed) * np.cos(y / 4.3) + rng.integers(-37, 38, (h, w))
    return np.clip(base, 0, 255).astype(np.uint8)


def as_rgb(img):
    """What `pil_loader` makes of a grayscale file: an RGB PIL image with three equal channels."""
    from PIL import Image
    return Image.fromarray(img, "L").convert("RGB")


def pil_eval_bytes(img, size, ratio):
    """`eval_transform`'s uint8 item (before ToTensor / Normalize), by Pillow itself through the product's own host functions."""
    from ecamp_amd.module import finetune_datasets as fd
    return np.asarray(fd.center_crop(fd.resize_short_side(as_rgb(img), int(size / ratio)), size).convert("L"), dtype=np.uint8)


def pil_train_bytes(img, out, flip=False):
    """`train_transform`'s resize of a crop box (+ flip), by Pillow itself."""
    from PIL import Image
    r = as_rgb(img).resize((out, out), Image.BILINEAR)
    if flip:
        r = r.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(r.convert("L"), dtype=np.uint8)


def normalise(u8):
    """`_to_normalised_gray3`'s arithmetic on a uint8 [.., R, R] array -> f32 torch tensor [.., 3, R, R]."""
    import torch
    from ecamp_amd.module.finetune_datasets import FT_MEAN, FT_STD
    g = np.asarray(u8, dtype=np.float32) / 255.0
    t = torch.from_numpy((g - FT_MEAN) / FT_STD)
    return t.unsqueeze(-3).expand(*t.shape[:-2], 3, *t.shape[-2:]).contiguous()
