"""NumPy restatement of what csrc/augment.hip's ecamp_resample_boxes_rgb_u8 computes for a colour sample: tests/_ft_image_ref.resample_box on
each of the three planes (Pillow resamples an RGB image band by band, with an L image's coefficients and uint8 intermediate), then
Pillow's convert("L"), L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16, then the flip.  tests/test_ft_colour_cpu.py holds it to Pillow's
own bytes through the product's host transforms; the GPU tests hold the kernels to Pillow and to it."""
import numpy as np

import _ft_image_ref as R

# the cases of the issue: (h, w) at out 16 and 48; evaluation at these ratios
SIZES = [(37, 53), (5, 7), (200, 150), (64, 64), (90, 16), (11, 40), (32, 32), (12, 300)]
OUTS = (16, 48)
RATIOS = (0.5, 0.875, 1, 2)


def luma(planes):
    """uint8 [3, ...] -> uint8 [...]: Pillow's convert("L") of an RGB pixel."""
    p = np.asarray(planes).astype(np.int64)
    return ((19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 0x8000) >> 16).astype(np.uint8)


def resample_colour_box(planes, out, geom, flip=False, filt=R.BILINEAR):
    """planes uint8 [3, h, w]; geom = (full_w, shift_w, full_h, shift_h) -> uint8 [out, out]: every plane through `resample_box`, the fold
    behind the vertical pass, then the flip."""
    assert planes.ndim == 3 and planes.shape[0] == 3
    dst = luma(np.stack([R.resample_box(planes[p], out, geom, flip=False, filt=filt) for p in range(3)]))
    return dst[:, ::-1].copy() if flip else dst


def gray_first_box(planes, out, geom, flip=False, filt=R.BILINEAR):
    """The WRONG order (fold, then resample the gray plane): what a one-plane shard of a colour source would give."""
    return R.resample_box(luma(planes), out, geom, flip=flip, filt=filt)


def colour_image(h, w, seed):
    """uint8 [3, h, w]: three different `gray_image` planes (R, G, B)."""
    return np.stack([R.gray_image(h, w, seed), R.gray_image(h, w, seed + 101), R.gray_image(h, w, seed + 202)])


def as_pil(planes):
    """The RGB PIL image `pil_loader` makes of a colour file with these planes."""
    from PIL import Image
    return Image.fromarray(np.ascontiguousarray(planes.transpose(1, 2, 0)), "RGB")


def pil_eval_bytes(planes, size, ratio):
    """`eval_transform`'s uint8 item (before ToTensor / Normalize) of a colour image, by Pillow through the product's own host functions."""
    from ecamp_amd.module import finetune_datasets as fd
    return np.asarray(fd.center_crop(fd.resize_short_side(as_pil(planes), int(size / ratio)), size).convert("L"), dtype=np.uint8)


def pil_train_bytes(planes, out, flip=False, filt=None):
    """`train_transform`'s resize of a colour crop box (+ flip) and Grayscale, by Pillow itself."""
    from PIL import Image
    r = as_pil(planes).resize((out, out), Image.BILINEAR if filt is None else filt)
    if flip:
        r = r.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(r.convert("L"), dtype=np.uint8)
