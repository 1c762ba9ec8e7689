"""-m gpu: ecamp_resample_boxes_rgb_u8 (csrc/augment.hip) -- three planes through the shared coefficient and horizontal passes, the luma
fold behind the new vertical pass -- against Pillow's own bytes: `eval_transform`'s Resize + CenterCrop + Grayscale and `train_transform`'s
crop().resize(BILINEAR) + flip + Grayscale on RGB images, in batches that mix one-plane and three-plane samples.  Every comparison is
byte equality.  The vertical pass launches ceil(out^2 / 256) blocks per sample, the horizontal one a block per (sample, 32-row chunk of
c * h rows): no grid cap of their own to step over."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ft_colour_ref as C  # noqa: E402
import _ft_image_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _eval(img, size, ratio):
    from ecamp_amd.module import finetune_datasets as fd
    pil = C.pil_eval_bytes if img.ndim == 3 else R.pil_eval_bytes
    return fd.device_eval_item(img, size, ratio), pil(img, size, ratio)


def _train(img, out, flip):
    pil = C.pil_train_bytes if img.ndim == 3 else R.pil_train_bytes
    return (img, flip, (out, 0, out, 0)), pil(img, out, flip)


@pytest.fixture(scope="module")
def cases():
    """The ragged mixed batch of the issue, gray and colour interleaved, each sample with Pillow's bytes: [(item, want uint8 [16, 16])]."""
    g, c = R.gray_image, C.colour_image
    return [_eval(g(61, 47, 1), 16, 2),                 # 0 gray, padding on both axes
            _train(c(200, 150, 2), 16, False),          # 1 colour, 200 rows -> 16: 27 taps
            _train(g(37, 53, 3), 16, False),            # 2 gray
            _train(c(5, 7, 4), 16, False),              # 3 colour, upscaling
            _eval(g(20, 90, 5), 16, 1.3),               # 4 gray, padding on one axis
            _train(c(37, 53, 6), 16, True),             # 5 colour, flipped training crop
            _eval(c(61, 47, 7), 16, 2),                 # 6 colour, padding on both axes
            _eval(c(20, 90, 8), 16, 1.3),               # 7 colour, padding on one axis, a shift on the other
            _train(c(11, 40, 9), 16, False),            # 8 colour, 3 h = 33: one row past a 32-row chunk
            _train(g(16, 90, 10), 16, True),            # 9 gray, flipped
            _train(c(32, 32, 11), 16, True),            # 10 colour, 3 h = 96: exactly three chunks
            _eval(g(9, 11, 12), 16, 1)]                 # 11 gray, upscaling


def _run(dev, items, size, check=True):
    from ecamp_amd.module import finetune_datasets as fd
    flat, table, meta = fd.pack_boxes(items, pin=True)
    return fd.DeviceBoxResampler(dev, size)(flat, table, meta, check=check).cpu().numpy(), meta


def _ref(item, size):
    box, flip, geom = item
    return C.resample_colour_box(box, size, geom, flip) if box.ndim == 3 else R.resample_box(box, size, geom, flip)


def test_ragged_mixed_batch_equals_pillow_and_its_gray_samples_the_gray_entry_point(dev, cases):
    items = [c[0] for c in cases]
    got, meta = _run(dev, items, 16)
    assert meta[0] == 27 and meta[3] is True and meta[2] == 600                # 200 -> 16: 2 * ceil(12.5) + 1; the tallest sample: 3 x 200 rows
    for n, (item, want) in enumerate(cases):
        assert np.array_equal(got[n], want), (n, item[0].shape, item[1:], int((got[n] != want).sum()))
        assert np.array_equal(got[n], _ref(item, 16))
    assert (got[0] == 0).any() and (got[6] == 0).any() and (got[6][:3] == 0).all() and (got[6][:, :4] == 0).all()   # the zero borders
    gray = [n for n, it in enumerate(items) if it[0].ndim == 2]
    assert gray == [0, 2, 4, 9, 11]
    alone, gmeta = _run(dev, [items[n] for n in gray], 16)
    assert len(gmeta) == 3                                                     # no colour flag: ecamp_resample_boxes_u8
    assert np.array_equal(alone, got[gray])


def test_one_colour_sample_and_an_all_colour_batch(dev, cases):
    for n in (6, 3, 5):                                                        # padding on both axes, upscaling, a flipped training crop
        got, meta = _run(dev, [cases[n][0]], 16)
        assert got.shape == (1, 16, 16) and meta[3] is True and np.array_equal(got[0], cases[n][1]), n
    colour = [c for c in cases if c[0][0].ndim == 3]
    assert len(colour) == 7
    got, _ = _run(dev, [c[0] for c in colour], 16)
    for n, (item, want) in enumerate(colour):
        assert np.array_equal(got[n], want), (n, item[0].shape)


def test_pure_red_green_and_blue_ramps(dev):
    """One plane a ramp, the others zero: a swapped plane or a swapped weight changes every non-zero byte."""
    ramp = (40 + np.add.outer(np.arange(48) * 3, np.arange(64) * 2)).clip(0, 255).astype(np.uint8)
    items, wants = [], []
    for p in range(3):
        img = np.zeros((3, 48, 64), dtype=np.uint8)
        img[p] = ramp
        items.append((img, p == 1, (16, 0, 16, 0)))
        wants.append(C.pil_train_bytes(img, 16, p == 1))
    got, _ = _run(dev, items, 16)
    for p in range(3):
        assert np.array_equal(got[p], wants[p]), p
    # the three differ from one another everywhere: the weights 19595 / 38470 / 7471 of a ramp that is never zero
    assert (got[0] != got[2]).all() and (got[0] != got[1][:, ::-1]).all() and (got[1][:, ::-1] != got[2]).all()


def test_a_1024_wide_colour_sample_at_224_uses_eleven_taps(dev):
    img = C.colour_image(300, 1024, seed=9)
    got, meta = _run(dev, [(img, True, (224, 0, 224, 0))], 224)
    assert meta[0] == 11 and meta[1] == meta[2] == 900
    assert np.array_equal(got[0], C.pil_train_bytes(img, 224, True))


def test_bicubic_through_the_colour_entry_point_equals_pillow(dev):
    from PIL import Image
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import finetune_datasets as fd
    imgs = [C.colour_image(37, 53, 1), R.gray_image(64, 64, 2), C.colour_image(5, 7, 3), C.colour_image(200, 150, 4)]
    size = 16
    flat, table, (_, rows, max_h, colour) = fd.pack_boxes([(im, n % 2 == 1, (size, 0, size, 0)) for n, im in enumerate(imgs)])
    kmax = R.ksize(200, size, R.BICUBIC)
    assert colour is True and kmax == 51
    ws = torch.empty((ops.resample_boxes_workspace_bytes(len(imgs), size, kmax, rows),), dtype=torch.uint8, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    got = torch.empty((len(imgs), size, size), dtype=torch.uint8, device=dev)
    ops.resample_boxes_rgb_u8(flat.to(dev), table.to(dev), got, size, kmax, rows, max_h, ws, err, filter=ops.BICUBIC)
    assert int(err.item()) == 0
    got = got.cpu().numpy()
    for n, im in enumerate(imgs):
        if im.ndim == 3:
            want = C.pil_train_bytes(im, size, n % 2 == 1, filt=Image.BICUBIC)
        else:
            r = Image.fromarray(im, "L").resize((size, size), Image.BICUBIC)
            want = np.asarray(r.transpose(Image.FLIP_LEFT_RIGHT) if n % 2 == 1 else r)
        assert np.array_equal(got[n], want), n


def test_undersized_tap_tables_raise_err_and_touch_nothing_out_of_bounds(dev, cases):
    """kmax = 5 where the batch needs 27: `err` is set, and the bytes before and behind `dst` and the workspace are as they were."""
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import finetune_datasets as fd
    flat, table, (kmax, rows, max_h, colour) = fd.pack_boxes([c[0] for c in cases])
    assert kmax > 5 and colour is True
    B, size, G = table.shape[0], 16, 4096
    need = ops.resample_boxes_workspace_bytes(B, size, 5, rows)
    ws_all = torch.full((G + need + G,), 0xA5, dtype=torch.uint8, device=dev)
    dst_all = torch.full((G + B * size * size + G,), 0x5A, dtype=torch.uint8, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    ops.resample_boxes_rgb_u8(flat.to(dev), table.to(dev), dst_all[G:G + B * size * size].view(B, size, size), size, 5, rows, max_h, ws_all[G:G + need], err)
    torch.cuda.synchronize()
    assert int(err.item()) == 1
    assert bool((ws_all[:G] == 0xA5).all()) and bool((ws_all[G + need:] == 0xA5).all())
    assert bool((dst_all[:G] == 0x5A).all()) and bool((dst_all[G + B * size * size:] == 0x5A).all())
    with pytest.raises(Exception, match="LDS"):                 # the LDS bound on kmax * out * 4 stays a checked argument error
        ops.resample_boxes_rgb_u8(flat.to(dev), table.to(dev), dst_all[G:G + B * size * size].view(B, size, size), size, 4096, rows, max_h, ws_all[G:G + need], err)
    with pytest.raises(RuntimeError, match="resample_boxes_rgb_u8.*more taps"):        # the loader-side object reports the flag when asked to
        fd.DeviceBoxResampler(dev, size)(flat, table, (5, rows, max_h, True), check=True)
