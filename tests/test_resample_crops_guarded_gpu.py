"""-m gpu: ecamp_resample_crops_u8 through the launch path it shares with the boxes entry points (csrc/augment.hip: rs_run), on a workspace
of exactly ecamp_resample_crops_workspace_bytes between guard regions.  The crops workspace has no RsTab [B] tail -- the passes read the
caller's table -- so a launch path that treated crops as boxes would write behind it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ft_image_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def test_crops_on_an_exact_workspace_equal_the_restatement_and_leave_the_guards(dev):
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import pretrain_datasets as pd
    imgs = [R.gray_image(h, w, seed=h + w) for h, w in ((37, 53), (5, 7), (64, 16), (20, 45))]
    items = [(im, n % 2 == 1) for n, im in enumerate(imgs)]
    flat, table = pd.pack_crops(items)
    max_side, rows, max_h = pd.crops_meta(table)
    B, size, G = len(imgs), 16, 4096
    kmax = pd.DeviceAugmenter.taps(max_side, size)
    assert kmax == 2 * 8 + 1 and (rows, max_h) == (126, 64)               # 64 -> 16: 2 * ceil(2 * 4) + 1 taps, enough for every crop
    need = ops.resample_crops_workspace_bytes(B, size, kmax, rows)
    assert need < ops.resample_boxes_workspace_bytes(B, size, kmax, rows)  # the tail this workspace does not have
    ws_all = torch.full((G + need + G,), 0xA5, dtype=torch.uint8, device=dev)
    dst_all = torch.full((G + B * size * size + G,), 0x5A, dtype=torch.uint8, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    got = dst_all[G:G + B * size * size].view(B, size, size)
    ops.resample_crops_u8(flat.to(dev), table.to(dev), got, size, kmax, rows, max_h, ws_all[G:G + need], err)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    for n, (im, flip) in enumerate(items):
        want = R.resample_box(im, size, (size, 0, size, 0), flip=flip, filt=R.BICUBIC)
        assert np.array_equal(got[n].cpu().numpy(), want), (n, im.shape, int((got[n].cpu().numpy() != want).sum()))
    assert bool((ws_all[:G] == 0xA5).all()) and bool((ws_all[G + need:] == 0xA5).all())
    assert bool((dst_all[:G] == 0x5A).all()) and bool((dst_all[G + B * size * size:] == 0x5A).all())
