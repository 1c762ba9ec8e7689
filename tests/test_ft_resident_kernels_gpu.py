"""-m gpu: ecamp_resample_shard_u8 (csrc/augment.hip) -- the classification resample reading every crop box where it lies in an image of a
shard that stays in device memory (table [B, 12]: the stride-10 row + pitch and plane_pitch) -- against Pillow's own bytes and against the
packed entry point on the copied box; its range guard (a row that points outside the shard reads nothing, gives zeros and sets bit 2 of the
error flag) and its argument refusals.  out = 16, one shard of under 200 KB; every comparison is byte equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ft_colour_ref as C  # noqa: E402
import _ft_image_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SIZE = 16


class Stored:
    """Images uint8 [H, W] / [3, H, W] back to back behind `lead` bytes: `data` (the shard's bytes), `row` / `box` of a crop box in one."""

    def __init__(self, images, lead=3):
        self.images, self.offs, parts, at = images, [], [np.full((lead,), 0xEE, dtype=np.uint8)], lead
        for im in images:
            self.offs.append(at)
            parts.append(im.reshape(-1))
            at += im.size
        self.data = np.concatenate(parts)

    def box(self, n, y0, x0, h, w):
        return self.images[n][..., y0:y0 + h, x0:x0 + w]

    def row(self, n, y0, x0, h, w, flip, geom):
        im = self.images[n]
        H, W = im.shape[-2:]
        assert 0 <= y0 and y0 + h <= H and 0 <= x0 and x0 + w <= W
        return np.array((self.offs[n] + y0 * W + x0, h, w, int(flip), 0) + tuple(geom) + (3 if im.ndim == 3 else 0, W, H * W), dtype=np.int64)

    def train(self, n, y0, x0, h, w, flip):
        """-> (table row, the packed item of the copied box, Pillow's bytes)"""
        box = np.ascontiguousarray(self.box(n, y0, x0, h, w))
        pil = C.pil_train_bytes if box.ndim == 3 else R.pil_train_bytes
        return self.row(n, y0, x0, h, w, flip, (SIZE, 0, SIZE, 0)), (box, flip, (SIZE, 0, SIZE, 0)), pil(box, SIZE, flip)

    def eval(self, n, ratio):
        from ecamp_amd.module import finetune_datasets as fd
        im = self.images[n]
        H, W = im.shape[-2:]
        geom = fd.eval_geometry(W, H, SIZE, ratio)
        pil = C.pil_eval_bytes if im.ndim == 3 else R.pil_eval_bytes
        return self.row(n, 0, 0, H, W, False, geom), (im, False, geom), pil(im, SIZE, ratio)


def _shard(dev, data, spare=0):
    """-> the device allocation: `data` with `spare` bytes of 0xC3 before and behind it (memory the test owns, outside what it declares as the
    shard: `alloc[spare:spare + data.size]`)."""
    pad = np.full((spare,), 0xC3, dtype=np.uint8)
    return torch.from_numpy(np.concatenate([pad, data, pad])).to(dev)


def _run(dev, shard, rows, filt=0, kmax=None):
    """rows through `pack_resident` and ecamp_resample_shard_u8 on `shard` (its numel is the declared size) -> (uint8 [B, 16, 16], err, meta)"""
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import finetune_datasets as fd
    table, meta = fd.pack_resident(rows)
    kmax = meta[0] if kmax is None else kmax
    ws = torch.empty((ops.resample_boxes_workspace_bytes(len(rows), SIZE, kmax, meta[1]),), dtype=torch.uint8, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    out = torch.full((len(rows), SIZE, SIZE), 0x5A, dtype=torch.uint8, device=dev)
    ops.resample_shard_u8(shard, table.to(dev), out, SIZE, kmax, meta[1], meta[2], ws, err, filter=filt)
    return out.cpu().numpy(), int(err.item()), meta


def _packed(dev, items):
    from ecamp_amd.module import finetune_datasets as fd
    flat, table, meta = fd.pack_boxes(items)
    return fd.DeviceBoxResampler(dev, SIZE)(flat, table, meta, check=True).cpu().numpy(), meta


@pytest.fixture(scope="module")
def stored():
    g, c = R.gray_image, C.colour_image
    return Stored([g(61, 47, 1), c(230, 171, 2), g(45, 61, 3), c(9, 13, 4), g(20, 90, 5), c(41, 57, 6), c(61, 47, 7), c(15, 45, 8), g(9, 11, 9), c(13, 17, 10)])


@pytest.fixture(scope="module")
def cases(stored):
    """[(table row, packed item, Pillow's bytes)]: the boxes of the issue, one-plane and three-plane images mixed."""
    s = stored
    return [s.eval(0, 2),                            # 0 gray, the whole image, zero padding on both axes
            s.train(1, 13, 9, 200, 150, False),      # 1 colour, strictly inside: x0, y0 > 0, pitch 171 != 150, plane_pitch != h w; 200 rows -> 27 taps
            s.train(2, 3, 5, 37, 53, False),         # 2 gray, strictly inside
            s.train(3, 2, 3, 5, 7, False),           # 3 colour, an upscaled 5 x 7 box
            s.eval(4, 1.3),                          # 4 gray, the whole image, zero padding on one axis
            s.train(5, 1, 2, 37, 53, True),          # 5 colour, flipped
            s.eval(6, 2),                            # 6 colour, the whole image, zero padding on both axes
            s.train(7, 2, 3, 11, 40, False),         # 7 colour, 3 h = 33: one row past a 32-row chunk
            s.train(1, 100, 70, 32, 32, True),       # 8 colour, 3 h = 96: exactly three chunks; the image of sample 1 again, another box
            s.train(2, 0, 20, 45, 30, True),         # 9 gray, the image of sample 2 again, flipped
            s.eval(8, 1),                            # 10 gray, the whole image, upscaled
            s.train(9, 6, 8, 7, 9, False)]           # 11 colour, the box ends on the last byte of the last image: of the shard


def test_boxes_inside_larger_images_equal_pillow_and_the_packed_entry_point(dev, both_halves, stored, cases):
    assert stored.offs[0] % 2 == 1 and sum(o % 2 for o in stored.offs) >= 3 and 20_000 < stored.data.size < 200_000
    last = cases[11][0]
    assert last[0] + 2 * last[11] + (last[1] - 1) * last[10] + last[2] == stored.data.size        # the last byte of the shard
    got, err, meta = _run(dev, _shard(dev, stored.data), [c[0] for c in cases])
    assert err == 0 and meta[0] == 27 and meta[3] is True and meta[2] == 600
    packed, pmeta = _packed(dev, [c[1] for c in cases])
    assert pmeta == meta
    for n, (row, item, want) in enumerate(cases):
        assert np.array_equal(got[n], want), (n, row.tolist(), int((got[n] != want).sum()))
        assert np.array_equal(got[n], packed[n]), n
    assert (got[0] == 0).any() and (got[6][:3] == 0).all() and (got[6][:, :4] == 0).all()          # the zero borders of the evaluation rows
    assert not np.array_equal(got[1], got[8]) and not np.array_equal(got[2], got[9])              # one image, two boxes


def test_a_batch_of_one_plane_images_alone(dev, stored, cases):
    gray = [n for n, c in enumerate(cases) if c[0][9] != 3]
    assert gray == [0, 2, 4, 9, 10]
    got, err, meta = _run(dev, _shard(dev, stored.data), [cases[n][0] for n in gray])
    assert err == 0 and len(meta) == 3
    for k, n in enumerate(gray):
        assert np.array_equal(got[k], cases[n][2]), n


@pytest.mark.parametrize("filt", [0, 1], ids=["bilinear", "bicubic"])
def test_packed_source_equals_the_packed_entry_point(dev, filt):
    """pitch = w, plane_pitch = h w on the flat bytes of `pack_boxes`: the bytes of ecamp_resample_boxes_rgb_u8, for both filters."""
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import finetune_datasets as fd
    g, c = R.gray_image, C.colour_image
    imgs = [g(61, 47, 1), c(200, 150, 2), g(37, 53, 3), c(5, 7, 4), c(11, 40, 9), g(16, 90, 10), c(32, 32, 11), g(9, 11, 12)]
    items = [(im, n % 3 == 1, (SIZE, 0, SIZE, 0)) for n, im in enumerate(imgs)]
    items[0] = (imgs[0], False, fd.eval_geometry(47, 61, SIZE, 2))
    flat, table, (kmax, rows, max_h, colour) = fd.pack_boxes(items)
    kmax = max(kmax, R.ksize(200, SIZE, filt))
    assert colour is True and kmax == (27, 51)[filt]
    t12 = torch.cat([table, table[:, 2:3], table[:, 1:2] * table[:, 2:3]], dim=1).contiguous()
    ws = torch.empty((ops.resample_boxes_workspace_bytes(len(imgs), SIZE, kmax, rows),), dtype=torch.uint8, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    want = torch.empty((len(imgs), SIZE, SIZE), dtype=torch.uint8, device=dev)
    got = torch.full_like(want, 0x5A)
    ops.resample_boxes_rgb_u8(flat.to(dev), table.to(dev), want, SIZE, kmax, rows, max_h, ws, err, filter=filt)
    ops.resample_shard_u8(flat.to(dev), t12.to(dev), got, SIZE, kmax, rows, max_h, ws, err, filter=filt)
    assert int(err.item()) == 0 and torch.equal(got, want)
    if filt == 0:
        assert np.array_equal(got[1].cpu().numpy(), C.pil_train_bytes(imgs[1], SIZE, True))


def test_offsets_behind_two_to_the_31(dev):
    """One gray and one colour image behind byte 2^31 of an uninitialised allocation, at odd offsets: the byte offsets are 64-bit all the way."""
    base, total = 2 ** 31 + 1, 2 ** 31 + 8192
    s = Stored([R.gray_image(37, 53, 21), C.colour_image(21, 30, 22)], lead=0)
    s.offs = [base, base + 37 * 53 + 1]                                  # 2^31 + 1 and 2^31 + 1963: both odd, one spare byte between
    assert all(o % 2 == 1 and o > 2 ** 31 for o in s.offs) and s.offs[1] + 3 * 21 * 30 <= total
    shard = torch.empty((total,), dtype=torch.uint8, device=dev)
    for off, im in zip(s.offs, s.images):
        shard[off:off + im.size] = torch.from_numpy(im.reshape(-1)).to(dev)
    cases = [s.train(0, 4, 6, 30, 41, True), s.train(1, 2, 3, 17, 25, False), s.eval(0, 1.3), s.eval(1, 2)]
    got, err, _ = _run(dev, shard, [c[0] for c in cases])
    assert err == 0
    for n, (row, _, want) in enumerate(cases):
        assert row[0] > 2 ** 31 and np.array_equal(got[n], want), n
    del shard
    torch.cuda.empty_cache()


def test_range_guard_zeroes_the_sample_and_sets_bit_2(dev, both_halves, stored, cases):
    """The declared shard is shorter than the allocation (4096 bytes of the test's own on either side): a row that ends one byte past the
    declared size, and a row whose pitch is below its width, read nothing -- all zeros, err_flag 2 -- and the valid rows beside them are
    Pillow's.  Every refused row here would stay inside the allocation even if it were read."""
    n_bytes, G = stored.data.size, 4096
    alloc = _shard(dev, stored.data, spare=G)
    shard = alloc[G:G + n_bytes]
    good = [cases[n] for n in (2, 11, 5)]
    past = cases[11][0].copy()
    past[0] += 1                                                                     # the last plane's last row now ends at n_bytes + 1
    assert past[0] + 2 * past[11] + (past[1] - 1) * past[10] + past[2] == n_bytes + 1
    narrow = cases[2][0].copy()
    narrow[10] = narrow[2] - 1                                                       # pitch < w
    for bad in (past, narrow):
        got, err, _ = _run(dev, shard, [good[0][0], bad, good[1][0], good[2][0]])
        assert err == 2
        assert (got[1] == 0).all()
        for k, n in ((0, 0), (2, 1), (3, 2)):
            assert np.array_equal(got[k], good[n][2]), (k, n)
    got, err, _ = _run(dev, shard, [past, narrow])                                    # a batch of nothing but refused rows
    assert err == 2 and (got == 0).all()
    # the other conditions, on the gray row of sample 2 (2257 bytes from its first pixel) and the colour row of sample 3
    for n, col, value in ((2, 0, -1), (2, 1, 0), (2, 2, 0), (3, 11, -5), (2, 0, n_bytes)):
        r = cases[n][0].copy()
        r[col] = value
        got, err = _run_table(dev, shard, np.stack([good[0][0], r]), fd_table([good[0][0], cases[n][0]]))
        assert err == 2 and (got[1] == 0).all() and np.array_equal(got[0], good[0][2]), (n, col, value)
    got, err, _ = _run(dev, shard, [c[0] for c in good])
    assert err == 0                                                                  # valid rows leave the flag alone
    assert bool((alloc[:G] == 0xC3).all()) and bool((alloc[G + n_bytes:] == 0xC3).all())


def fd_table(rows):
    from ecamp_amd.module import finetune_datasets as fd
    return fd.pack_resident(rows)[0]


def _run_table(dev, shard, rows, sized_like):
    """`rows` int64 [B, 12] as they are, but column 4 and (tmp_rows, max_h) taken from the valid table `sized_like`: nothing is sized by a
    refused row."""
    from ecamp_amd import hip_ops as ops
    t = torch.from_numpy(rows.copy())
    t[:, 4] = sized_like[:, 4]
    planes = torch.where(sized_like[:, 9] == 3, 3, 1)
    ch = planes * sized_like[:, 1]
    kmax, tmp_rows, max_h = 27, int(ch.sum()), int(ch.max())
    ws = torch.empty((ops.resample_boxes_workspace_bytes(len(rows), SIZE, kmax, tmp_rows),), dtype=torch.uint8, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    out = torch.full((len(rows), SIZE, SIZE), 0x5A, dtype=torch.uint8, device=dev)
    ops.resample_shard_u8(shard, t.to(dev), out, SIZE, kmax, tmp_rows, max_h, ws, err)
    return out.cpu().numpy(), int(err.item())


def test_too_few_taps_keep_value_1(dev, stored, cases):
    got, err, _ = _run(dev, _shard(dev, stored.data), [cases[1][0], cases[2][0]], kmax=5)
    assert err == 1


def test_argument_refusals_launch_nothing(dev, stored, cases):
    from ecamp_amd import _lib
    from ecamp_amd import hip_ops as ops
    from ecamp_amd.module import finetune_datasets as fd
    shard = _shard(dev, stored.data)
    table, (kmax, rows, max_h, _) = fd.pack_resident([c[0] for c in cases])
    table = table.to(dev)
    B = table.shape[0]
    need = ops.resample_boxes_workspace_bytes(B, SIZE, kmax, rows)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    out = torch.full((B, SIZE, SIZE), 0x5A, dtype=torch.uint8, device=dev)

    def call(**over):
        a = dict(shard=ops.ptr(shard), shard_bytes=shard.numel(), table=ops.ptr(table), dst=ops.ptr(out), B=B, out=SIZE, kmax=kmax, tmp_rows=rows, max_h=max_h,
                 filter=0, ws=ops.ptr(ws), ws_bytes=need, err_flag=ops.ptr(err), stream=ops.stream())
        a.update(over)
        _lib.call("ecamp_resample_shard_u8", *a.values())

    for name in ("shard", "table", "dst", "ws", "err_flag"):
        with pytest.raises(_lib.EcampHipError, match=r"resample_shard_u8: null argument"):
            call(**{name: ops.ptr(None)})
    with pytest.raises(_lib.EcampHipError, match=r"resample_shard_u8: B=65536 \(<= 65535\)"):
        call(B=65536)
    for v in (0, -1):
        with pytest.raises(_lib.EcampHipError, match=r"resample_shard_u8: shard_bytes=%d" % v):
            call(shard_bytes=v)
    with pytest.raises(_lib.EcampHipError, match=r"resample_shard_u8: workspace of %d bytes is too small" % (need - 1)):
        call(ws_bytes=need - 1)
    with pytest.raises(_lib.EcampHipError, match=r"resample_shard_u8: filter 2"):
        call(filter=2)
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and bool((ws == 0xA5).all()) and int(err.item()) == 0      # nothing was launched
    call()                                                                                      # and the same arguments, unchanged, run
    assert int(err.item()) == 0 and np.array_equal(out[3].cpu().numpy(), cases[3][2])
