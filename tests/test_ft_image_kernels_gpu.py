"""-m gpu: the two kernels of the classification image pipeline.  ecamp_resample_boxes_u8 (csrc/augment.hip) against Pillow's own bytes
-- `eval_transform`'s Resize + CenterCrop with zero padding and `train_transform`'s crop().resize(BILINEAR) + flip -- and against the old
entry point for BICUBIC; ecamp_im2col_u8 (csrc/vision.hip) against ecamp_im2col_gather on the normalised image expanded to three planes,
bit for bit.  The resample launches one block per (sample, row chunk) / (sample, output row) and one thread per coefficient row: no grid
cap of its own to step over; ecamp_im2col_u8 has the 8192-block cap of im2col_gather_kernel and is run above it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ft_image_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    """The twelve shapes of the issue (+ the four training ones flipped), each with Pillow's bytes: [(item, want uint8 [16, 16])]."""
    from ecamp_amd.module import finetune_datasets as fd
    out = []
    for h, w, size, ratio in R.EVAL_CASES:
        img = R.gray_image(h, w, seed=h * 100 + w)
        out.append((fd.device_eval_item(img, size, ratio), R.pil_eval_bytes(img, size, ratio)))
    for flip in (False, True):
        for h, w, o in R.TRAIN_CASES:
            img = R.gray_image(h, w, seed=h + w)
            out.append(((img, flip, (o, 0, o, 0)), R.pil_train_bytes(img, o, flip)))
    return out


def _run(dev, items, size, check=True):
    from ecamp_amd.module import finetune_datasets as fd
    flat, table, meta = fd.pack_boxes(items, pin=True)
    return fd.DeviceBoxResampler(dev, size)(flat, table, meta, check=check).cpu().numpy(), meta


def test_ragged_batch_of_training_and_evaluation_rows_equals_pillow(dev, cases):
    got, meta = _run(dev, [c[0] for c in cases], 16)
    assert meta[0] == 27                                     # 200 -> 16: 2 * ceil(12.5) + 1
    for n, (item, want) in enumerate(cases):
        assert np.array_equal(got[n], want), (n, item[0].shape, item[1:], int((got[n] != want).sum()))
        assert np.array_equal(got[n], R.resample_box(*((item[0], 16, item[2], item[1]))))
    assert any(c[0][1] for c in cases) and (got[4] == 0).any()    # flips were in the batch; the padded case has its zero border


def test_single_samples_equal_pillow(dev, cases):
    """B = 1: each of padding-on-both-axes, upscaling, a flipped training crop."""
    for n in (4, 6, 12):
        got, _ = _run(dev, [cases[n][0]], 16)
        assert got.shape == (1, 16, 16) and np.array_equal(got[0], cases[n][1]), n


def test_a_1024_wide_sample_at_224_uses_eleven_taps(dev):
    img = R.gray_image(300, 1024, seed=9)
    got, meta = _run(dev, [(img, True, (224, 0, 224, 0)), (img[:, :700].copy(), False, (224, 0, 224, 0))], 224)
    assert meta[0] == 11
    assert np.array_equal(got[0], R.pil_train_bytes(img, 224, True))
    assert np.array_equal(got[1], R.pil_train_bytes(img[:, :700], 224, False))


def test_bicubic_through_the_new_entry_point_equals_the_old_one(dev):
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import pretrain_datasets as pd
    imgs = [R.gray_image(h, w, seed=h) for h, w in ((37, 53), (5, 7), (200, 150), (64, 64), (90, 16))]
    size = 32
    flat, t6 = pd.pack_crops([(im, n % 2 == 1) for n, im in enumerate(imgs)])
    want = pd.DeviceAugmenter(dev, size)(flat, t6, check=True)
    t10 = torch.zeros((len(imgs), 10), dtype=torch.int64)
    t10[:, :5] = t6[:, :5]
    t10[:, 5], t10[:, 7] = size, size
    max_side, rows, max_h = pd.crops_meta(t6)
    kmax = pd.DeviceAugmenter.taps(max_side, size)
    ws = torch.empty((ops.resample_boxes_workspace_bytes(len(imgs), size, kmax, rows),), dtype=torch.uint8, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    got = torch.empty_like(want)
    ops.resample_boxes_u8(flat.to(dev), t10.to(dev), got, size, kmax, rows, max_h, ws, err, filter=ops.BICUBIC)
    assert int(err.item()) == 0 and torch.equal(got, want)
    for n, im in enumerate(imgs):
        assert np.array_equal(got[n].cpu().numpy(), R.resample_box(im, size, (size, 0, size, 0), flip=n % 2 == 1, filt=R.BICUBIC))


def test_undersized_tap_tables_raise_err_and_touch_nothing_out_of_bounds(dev, cases):
    """kmax = 5 where the batch needs 27: `err` is set, and the bytes before and behind `dst` and the workspace are as they were."""
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import finetune_datasets as fd
    flat, table, (kmax, rows, max_h) = fd.pack_boxes([c[0] for c in cases])
    assert kmax > 5
    B, size, G = table.shape[0], 16, 4096
    need = ops.resample_boxes_workspace_bytes(B, size, 5, rows)
    ws_all = torch.full((G + need + G,), 0xA5, dtype=torch.uint8, device=dev)
    dst_all = torch.full((G + B * size * size + G,), 0x5A, dtype=torch.uint8, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    ops.resample_boxes_u8(flat.to(dev), table.to(dev), dst_all[G:G + B * size * size].view(B, size, size), size, 5, rows, max_h, ws_all[G:G + need], err)
    torch.cuda.synchronize()
    assert int(err.item()) == 1
    assert bool((ws_all[:G] == 0xA5).all()) and bool((ws_all[G + need:] == 0xA5).all())
    assert bool((dst_all[:G] == 0x5A).all()) and bool((dst_all[G + B * size * size:] == 0x5A).all())
    with pytest.raises(Exception, match="LDS"):                 # the LDS bound on kmax * out * 4 stays a checked argument error
        ops.resample_boxes_u8(flat.to(dev), table.to(dev), dst_all[G:G + B * size * size].view(B, size, size), size, 4096, rows, max_h, ws_all[G:G + need], err)
    with pytest.raises(RuntimeError, match="more taps"):        # and the loader-side object reports the flag when asked to
        fd.DeviceBoxResampler(dev, size)(flat, table, (5, rows, max_h), check=True)


def _im2col_case(dev, dtype, B, Rr, p, Lk, permute, seed):
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import finetune_datasets as fd
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, Rr, Rr), dtype=torch.uint8, generator=g)
    L = (Rr // p) ** 2
    if permute:
        ids = torch.stack([torch.randperm(L, generator=g)[:Lk] for _ in range(B)]).to(torch.int32)
    else:
        ids = torch.arange(Lk, dtype=torch.int32).expand(B, Lk).contiguous()
    lut = ops.image_lut(dev, fd.FT_MEAN, fd.FT_STD)
    f32 = lut[img.to(dev).long()][:, None].expand(B, 3, Rr, Rr).contiguous()
    assert torch.equal(f32.cpu(), R.normalise(img.numpy()))          # the expanded image IS the host item
    want = ops.im2col_gather(f32, ids.to(dev), p, dtype)
    got = ops.im2col_u8(img.to(dev), lut, ids.to(dev), p, dtype)
    assert got.shape == want.shape == (B * (Lk + 1), 3 * p * p) and got.dtype == dtype
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.view(bits), want.view(bits))
    assert bool((got.view(B, Lk + 1, -1)[:, 0] == 0).all()) and bool((got[:, :p * p].view(bits) == got[:, 2 * p * p:].view(bits)).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_im2col_u8_is_bit_equal_to_im2col_gather_on_the_expanded_image(dev, dtype):
    _im2col_case(dev, dtype, 3, 64, 16, 16, False, 1)            # identity ids_keep, every patch
    _im2col_case(dev, dtype, 3, 64, 16, 16, True, 2)             # permuted
    _im2col_case(dev, dtype, 2, 48, 8, 11, True, 3)              # Lk < L, another patch size
    _im2col_case(dev, dtype, 1, 32, 4, 64, False, 4)             # B = 1, the smallest patch
    _im2col_case(dev, dtype, 170, 224, 16, 196, False, 5)        # 170 * 197 * 64 work items > 8192 blocks x 256 threads: the strided loop
