"""Classification datasets of the linear probe -- the reference's Fine-tuning/Classification/utils/my_dataset.py (list format) and
utils/data_utils.py:20-34 (transforms), with PIL and torch only (torchvision is not a dependency).

List format: one sample per line, `relative/path label label ...` with integer labels -- a multi-hot row (multilabel tasks) or one
class index (COVIDx, Aptos).  The lists are `train_list.txt` / `train_list_1.txt` / `train_list_10.txt` (picked by `--data_volume`),
`val_list.txt` and `test_list.txt` in `--list_dir` (the reference hard-codes ./datasets/<task>).
"""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from .pretrain_datasets import DeviceResampler, pil_loader, random_flip, random_resized_crop_params

# utils/data_utils.py:25,33.  NOT the pre-training constants (0.4721 / 0.3037, pretrain_datasets.py:51): the reference has both.
FT_MEAN, FT_STD = 0.4722, 0.3028
TRAIN_LISTS = {"1": "train_list_1.txt", "10": "train_list_10.txt", "100": "train_list.txt"}   # my_dataset.py:15-20


def list_file(split, data_volume=None):
    """File name of a split's list (my_dataset.py:15-40)."""
    if split == "train":
        if str(data_volume) not in TRAIN_LISTS:
            raise ValueError("--data_volume must be '1', '10' or '100', got %r" % (data_volume,))
        return TRAIN_LISTS[str(data_volume)]
    if split not in ("val", "test"):
        raise ValueError("split must be train, val or test, got %r" % (split,))
    return split + "_list.txt"


def read_list(path):
    """-> (relative paths, label rows as lists of int)  (my_dataset.py:44-62; blank lines are skipped)."""
    paths, labels = [], []
    with open(path, "r") as f:
        for line in f:
            items = line.split()
            if not items:
                continue
            paths.append(items[0])
            labels.append([int(i) for i in items[1:]])
    return paths, labels


def _to_normalised_gray3(img, size):
    """Grayscale(3) + ToTensor + Normalize(mean=[0.4722], std=[0.3028]) (data_utils.py:23-25): three identical f32 planes."""
    g = np.asarray(img.convert("L"), dtype=np.float32) / 255.0
    t = torch.from_numpy((g - FT_MEAN) / FT_STD)
    return t[None].expand(3, size, size).contiguous()


def train_transform(img_size):
    """data_utils.py:20-26: RandomResizedCrop((s, s)) with torchvision's defaults (scale 0.08-1, ratio 3/4-4/3, bilinear) /
    RandomHorizontalFlip / Grayscale(3) / ToTensor / Normalize.  Draws from torch's global generator as torchvision does:
    `random_resized_crop_params`, then `random_flip`."""
    from PIL import Image

    def tf(img):
        w, h = img.size
        i, j, ch, cw = random_resized_crop_params(w, h, scale=(0.08, 1.0))
        img = img.crop((j, i, j + cw, i + ch)).resize((img_size, img_size), Image.BILINEAR)
        if random_flip():
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        return _to_normalised_gray3(img, img_size)

    return tf


def resize_short_side(img, size):
    """torchvision `Resize(int)` on a PIL image: the short side becomes `size`, the long one int(size * long / short); bilinear."""
    from PIL import Image
    w, h = img.size
    short, long_ = (w, h) if w <= h else (h, w)
    if short == size:
        return img
    new_short, new_long = size, int(size * long_ / short)
    nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
    return img.resize((nw, nh), Image.BILINEAR)


def center_crop(img, size):
    """torchvision `CenterCrop((size, size))` on a PIL image: zero padding where the image is smaller, then the crop whose top-left
    corner is round((h - size) / 2), round((w - size) / 2)."""
    from PIL import Image
    w, h = img.size
    if size > w or size > h:
        left, top = ((size - w) // 2 if size > w else 0), ((size - h) // 2 if size > h else 0)
        canvas = Image.new(img.mode, (max(w, size), max(h, size)), 0)
        canvas.paste(img, (left, top))
        img = canvas
        w, h = img.size
    top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
    return img.crop((left, top, left + size, top + size))


def eval_transform(img_size, ratio=1.0):
    """data_utils.py:28-34: Resize(int(img_size / ratio)) / CenterCrop((s, s)) / Grayscale(3) / ToTensor / Normalize."""
    def tf(img):
        return _to_normalised_gray3(center_crop(resize_short_side(img, int(img_size / ratio)), img_size), img_size)

    return tf


class ListDataset(Dataset):
    """my_dataset.XRAY: (image f32 [3, s, s], labels FloatTensor [k]) per line of `<list_dir>/<list of the split>`; images are read from
    `root`/<relative path> and converted to RGB first, as the reference does."""

    def __init__(self, root, list_dir, split, data_volume=None, transform=None):
        self.root, self.split, self.transform = root, split, transform
        self.list_path = os.path.join(list_dir, list_file(split, data_volume))
        if not os.path.exists(self.list_path):
            raise FileNotFoundError("%s not found: check --list_dir (the directory with train_list*.txt, val_list.txt, test_list.txt)" % self.list_path)
        rel, self.labels = read_list(self.list_path)
        self.paths = [os.path.join(root, r) for r in rel]

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, index):
        img = pil_loader(self.paths[index])
        if self.transform is not None:
            img = self.transform(img)
        return img, torch.FloatTensor(self.labels[index])


class SyntheticClassificationDataset(Dataset):
    """`--synthetic`: random images whose label is a function of the image (no dataset is read).  The image is noise; the rows are cut
    into one horizontal band per class, and a band is brightened (positive class) or darkened.  Multilabel: every class draws its own
    bit, labels = the multi-hot row; single-label: one class index, its band alone is brightened.  Sample i depends on (seed, i) only."""

    def __init__(self, length, img_size, num_classes, multilabel, seed=0):
        self.length, self.img_size, self.num_classes, self.multilabel, self.seed = int(length), int(img_size), int(num_classes), bool(multilabel), int(seed)

    def __len__(self):
        return self.length

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self.seed * 1000003 + int(index))
        R, C = self.img_size, self.num_classes
        img = 0.3 * torch.randn(R, R, generator=g)
        if self.multilabel:
            bits = torch.randint(0, 2, (C,), generator=g)
            label = bits.to(torch.float32)
        else:
            k = int(torch.randint(0, C, (1,), generator=g))
            bits = torch.zeros(C, dtype=torch.int64)
            bits[k] = 1
            label = torch.FloatTensor([k])
        band = torch.arange(R) * C // R                      # the class whose band a row belongs to
        img = img + (bits[band].to(torch.float32) * 2.0 - 1.0)[:, None]
        return img[None].expand(3, R, R).contiguous(), label


# ---- the image half on the device (csrc/augment.hip: ecamp_resample_boxes_u8; csrc/vision.hip: ecamp_im2col_u8) -------------------------
# The transforms above cost a loader worker a decode, a crop, a resample and twelve bytes per pixel through pinned memory and PCIe per
# sample.  The path below keeps their RESULT and moves the work, as `--image_shard` does for pre-training: the images of a list file are
# decoded once, offline, into a uint8 shard (tools/make_image_shard.py --list_dir); a worker draws the box and the flip (training: the same
# torch-RNG calls in the same order) or works out the Resize + CenterCrop geometry in integers (evaluation) and copies bytes; the device
# resamples the batch with Pillow's own BILINEAR fixed-point arithmetic and hands the classifier uint8 [B, R, R], which its stem
# normalises through the table of FT_MEAN / FT_STD.  Byte for byte the host item: a GRAYSCALE source (three equal channels: each is
# resampled alike and Grayscale returns the common value) is one plane; Grayscale after the resample of a colour image is not the resample
# of its gray plane, so a COLOUR source (Aptos, ODIR5K, MURED; `make_image_shard.py --colour`) keeps its three planes [3, H, W] through the
# shard and the box, the device resamples each with the same taps -- Pillow resamples an RGB image band by band -- and folds them with
# Pillow's convert("L") behind the vertical pass (ecamp_resample_boxes_rgb_u8).  A batch without a colour sample takes the one-plane call.
def _as_planes(image):
    """uint8 [H, W] or [3, H, W] as it is; a PIL image -> its common channel [H, W] if the three are equal, else [3, H, W]."""
    if isinstance(image, np.ndarray):
        return image
    a = np.asarray(image.convert("RGB"), dtype=np.uint8)
    if np.array_equal(a[..., 0], a[..., 1]) and np.array_equal(a[..., 0], a[..., 2]):
        return np.ascontiguousarray(a[..., 0])
    return np.ascontiguousarray(a.transpose(2, 0, 1))


def device_train_item(image, img_size):
    """`train_transform`'s share of a loader worker: draw the crop box, then the flip (the same calls in the same order, whatever the
    number of planes) -> (the BOX's bytes, uint8 [h, w] or [3, h, w], a view of `image`; flip; (full_w, shift_w, full_h, shift_h) =
    (s, 0, s, 0): the box is resized to s x s)."""
    image = _as_planes(image)
    H, W = image.shape[-2:]
    i, j, h, w = random_resized_crop_params(W, H, scale=(0.08, 1.0))
    flip = random_flip()
    return image[..., i:i + h, j:j + w], flip, (int(img_size), 0, int(img_size), 0)   # a view: `pack_boxes` makes the one copy


def _round_half_even_of_half(d):
    """Python's round(d / 2.0) of an integer d >= 0, in integers: ties go to the even neighbour."""
    q, r = divmod(d, 2)
    return q + (r & q & 1)


def eval_geometry(w, h, img_size, ratio=1.0):
    """`eval_transform` as numbers: Resize(S = int(img_size / ratio)) makes the image (nw, nh) (`resize_short_side`: untouched when the short
    side is S already); CenterCrop pads with zeros where that is smaller than the crop and cuts at round((n' - size) / 2) of the padded
    canvas.  Per axis: `full` = n, and the crop's pixel x is pixel x + shift of the resized axis (outside [0, full): zero), with
    shift = round((max(n, size) - size) / 2) - pad, pad = (size - n) // 2 if size > n else 0.  -> (full_w, shift_w, full_h, shift_h)."""
    size, S = int(img_size), int(img_size / ratio)
    short, long_ = (w, h) if w <= h else (h, w)
    if short == S:
        nw, nh = w, h
    else:
        new_long = (S * long_) // short            # int(S * long / short): exact in integers
        nw, nh = (S, new_long) if w <= h else (new_long, S)
    out = []
    for n in (nw, nh):
        pad = (size - n) // 2 if size > n else 0
        out += [n, _round_half_even_of_half(max(n, size) - size) - pad]
    return tuple(out)


def device_eval_item(image, img_size, ratio=1.0):
    """`eval_transform`'s share of a loader worker -> (the WHOLE image's bytes, uint8 [H, W] or [3, H, W]; flip = False; `eval_geometry`)."""
    image = _as_planes(image)
    H, W = image.shape[-2:]
    return np.ascontiguousarray(image), False, eval_geometry(W, H, img_size, ratio)


def bilinear_taps(in_size, full):
    """Pillow's ksize of a BILINEAR resize of an axis from `in_size` to `full`: 2 * ceil(max(1, in / full)) + 1, in integers."""
    return 2 * max(1, -(-int(in_size) // int(full))) + 1


def pack_boxes(items, pin=False):
    """Batch of `device_train_item` / `device_eval_item` results -> (flat uint8 tensor of all boxes back to back, int64 table [B, 10] for
    ecamp_resample_boxes_u8: byte offset, h, w, flip, first intermediate row, full_w, shift_w, full_h, shift_h, 0; meta = (tap count of the
    batch's largest scale factor, sum of h, largest h) as Python ints, made here so that the step never reads the table back).
    A colour box [3, h, w] is copied as three contiguous planes, has 3 in the last column and 3 h intermediate rows (the table of
    ecamp_resample_boxes_rgb_u8; the sums and the maximum then count 3 h), and gives meta a fourth field, True: a colour sample is present."""
    total = sum(c.size for c, _, _ in items)
    if torch.utils.data.get_worker_info() is not None:
        # in a loader worker: straight into shared memory, as torch's default_collate does -- the bytes are then copied once here (from
        # the shard's pages) and once more by the pinning thread, instead of a third time when the batch is handed to the main process
        flat = torch.empty(0, dtype=torch.uint8)
        flat = flat.new(flat._typed_storage()._new_shared(total)).resize_(total)
    else:
        flat = torch.empty((total,), dtype=torch.uint8, pin_memory=pin)
    table = torch.zeros((len(items), 10), dtype=torch.int64, pin_memory=pin)
    fa, ta = flat.numpy(), table.numpy()
    off = row = max_h = 0
    kmax = 3
    colour = False
    for n, (c, flip, (fw, sw, fh, sh)) in enumerate(items):
        h, w = c.shape[-2:]
        planes = 1
        if c.ndim == 3:
            if c.shape[0] != 3:
                raise ValueError("pack_boxes: a box is uint8 [h, w] or [3, h, w], got %s" % (c.shape,))
            planes, colour = 3, True
            ta[n, 9] = 3
        fa[off:off + c.size].reshape(c.shape)[...] = c
        ta[n, :9] = (off, h, w, int(flip), row, fw, sw, fh, sh)
        kmax = max(kmax, bilinear_taps(w, fw), bilinear_taps(h, fh))
        off += c.size
        row += planes * h
        max_h = max(max_h, planes * h)
    return flat, table, ((kmax, row, max_h, True) if colour else (kmax, row, max_h))


def collate_boxes(batch):
    """collate_fn of `ShardListDataset`: [(item, labels)] -> (flat bytes, table, meta, labels [B, k])."""
    flat, table, meta = pack_boxes([item for item, _ in batch])
    return flat, table, meta, torch.stack([y for _, y in batch])


# ---- the shard in device memory (csrc/augment.hip: ecamp_resample_shard_u8) ---------------------------------------------------------------
# A classification shard is small beside the device's memory and never changes, yet the path above sends every box's bytes through a
# worker's shared memory, the pinning thread and PCIe again in every epoch.  `ResidentShard` uploads the file once; a worker then draws the
# same box from the index row alone and sends twelve numbers, and the device reads the box where it lies in the stored image (two pitches
# more per row).  The transforms and their bytes are the ones above.  Pre-training's `--image_shard` is not covered: MIMIC-CXR does not fit.
def resident_item(index_row, train, img_size, ratio=1.0):
    """`device_train_item` / `device_eval_item` on an index row (byte offset, H, W[, C]) instead of the image: the same torch-RNG calls in
    the same order (training), `eval_geometry` (evaluation) -> int64 [12], the row of ecamp_resample_shard_u8 but for column 4 (the first
    intermediate row, which `pack_resident` fills): off of the box's first pixel, h, w, flip, 0, full_w, shift_w, full_h, shift_h, C, pitch =
    W, plane_pitch = H W."""
    off, H, W = (int(v) for v in index_row[:3])
    c = int(index_row[3]) if len(index_row) > 3 else 1
    if train:
        i, j, h, w = random_resized_crop_params(W, H, scale=(0.08, 1.0))
        flip = random_flip()
        geometry = (int(img_size), 0, int(img_size), 0)
    else:
        i, j, h, w, flip = 0, 0, H, W, False
        geometry = eval_geometry(W, H, img_size, ratio)
    return np.array((off + i * W + j, h, w, int(flip), 0) + geometry + (3 if c == 3 else 0, W, H * W), dtype=np.int64)


def pack_resident(items, pin=False):
    """Batch of `resident_item` rows -> (int64 table [B, 12] for ecamp_resample_shard_u8, meta): columns 1 to 9 and meta are `pack_boxes`' on
    the same items -- the first intermediate rows are the prefix sum of c h, meta = (tap count, sum of c h, largest c h[, True: a colour
    sample is present])."""
    table = torch.zeros((len(items), 12), dtype=torch.int64, pin_memory=pin)
    ta = table.numpy()
    row = max_h = 0
    kmax = 3
    colour = False
    for n, r in enumerate(items):
        ta[n] = r
        ta[n, 4] = row
        h, w, planes = int(r[1]), int(r[2]), (3 if r[9] == 3 else 1)
        colour = colour or planes == 3
        kmax = max(kmax, bilinear_taps(w, r[5]), bilinear_taps(h, r[7]))
        row += planes * h
        max_h = max(max_h, planes * h)
    return table, ((kmax, row, max_h, True) if colour else (kmax, row, max_h))


def collate_resident(batch):
    """collate_fn of `ShardListDataset(resident=True)`: [(row, labels)] -> (table, meta, labels [B, k])."""
    table, meta = pack_resident([item for item, _ in batch])
    return table, meta, torch.stack([y for _, y in batch])


class ResidentShard:
    """A shard file (`U8ShardWriter`) uploaded once into ONE device uint8 tensor (`tensor`, `nbytes`), in chunks through a reused pinned
    staging buffer -- no whole-file host copy; the index stays on the host (`index`).  Refuses, before anything is allocated, a file that
    does not fit: `fits`.  `seconds`: what the upload took."""

    FREE_DIVISOR = 2          # without a limit of the caller's, a shard may take 1 / FREE_DIVISOR of the memory that is free when it is uploaded
    CHUNK_BYTES = 64 << 20    # the staging buffer

    @staticmethod
    def fits(nbytes, free_bytes, max_bytes=None):
        return nbytes <= max_bytes if max_bytes is not None else nbytes <= free_bytes // ResidentShard.FREE_DIVISOR

    @classmethod
    def check_fits(cls, path, device, max_bytes=None):
        """-> the file's size; raises MemoryError with the whole story if `fits` says no.  Allocates nothing."""
        nbytes = os.path.getsize(path)
        torch.cuda.empty_cache()   # what a released shard held is free again
        free = int(torch.cuda.mem_get_info(device)[0])
        if not cls.fits(nbytes, free, max_bytes):
            limit = ("the limit given (--image_shard_resident_max_gb) is %d bytes" % max_bytes if max_bytes is not None
                     else "the limit is 1/%d of the free memory, %d bytes" % (cls.FREE_DIVISOR, free // cls.FREE_DIVISOR))
            raise MemoryError("image shard %s holds %d bytes and does not fit in device memory: %d bytes are free, %s.  The run works without "
                              "--image_shard_resident (the boxes then travel from the host in every pass)" % (path, nbytes, free, limit))
        return nbytes

    def __init__(self, path, device, max_bytes=None):
        import time
        self.path, self.device = path, torch.device(device)
        self.nbytes = self.check_fits(path, self.device, max_bytes)
        t0 = time.time()
        self.index = np.load(path + ".idx.npy")
        self.tensor = torch.empty((self.nbytes,), dtype=torch.uint8, device=self.device)
        if self.nbytes:
            data = np.memmap(path, dtype=np.uint8, mode="r")
            stage = torch.empty((min(self.nbytes, self.CHUNK_BYTES),), dtype=torch.uint8, pin_memory=True)
            for a in range(0, self.nbytes, stage.numel()):
                n = min(stage.numel(), self.nbytes - a)
                stage.numpy()[:n] = data[a:a + n]
                self.tensor[a:a + n].copy_(stage[:n])   # blocking: the staging buffer is free again when it returns
            del data, stage
        self.seconds = time.time() - t0


class ShardListDataset(Dataset):
    """The labels of `<list_dir>/<list of the split>` over the shard that holds the list's images in list order
    (`<shard_dir>/<list file name>.u8`, tools/make_image_shard.py --list_dir): (`device_train_item` or `device_eval_item`, labels)."""

    def __init__(self, shard_dir, list_dir, split, data_volume=None, img_size=224, ratio=1.0, resident=False):
        """resident: the shard's bytes live in device memory (`ResidentShard`) -- an item is then `resident_item`'s table row instead of a
        box's bytes, made from the index alone: the file is never mapped here."""
        from .pretrain_datasets import U8ShardReader
        self.split, self.img_size, self.ratio, self.resident = split, int(img_size), ratio, bool(resident)
        self.list_path = os.path.join(list_dir, list_file(split, data_volume))
        self.shard_path = shard_path(shard_dir, split, data_volume)
        check_shard(self.shard_path, self.list_path)
        _, self.labels = read_list(self.list_path)
        if self.resident:
            self.shard, self.index = None, np.load(self.shard_path + ".idx.npy")
        else:
            self.shard = U8ShardReader(self.shard_path)

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, index):
        if self.resident:
            return resident_item(self.index[index], self.split == "train", self.img_size, self.ratio), torch.FloatTensor(self.labels[index])
        img = self.shard[index]
        item = device_train_item(img, self.img_size) if self.split == "train" else device_eval_item(img, self.img_size, self.ratio)
        return item, torch.FloatTensor(self.labels[index])


def shard_path(shard_dir, split, data_volume=None):
    return os.path.join(shard_dir, list_file(split, data_volume) + ".u8")


def check_shard(path, list_path):
    """Raise unless the shard `path` (+ its index) exists and holds as many images as `list_path` has lines.  Reads two small files."""
    if not os.path.exists(list_path):
        raise FileNotFoundError("%s not found: check --list_dir (the directory with train_list*.txt, val_list.txt, test_list.txt)" % list_path)
    if not (os.path.exists(path) and os.path.exists(path + ".idx.npy")):
        raise FileNotFoundError("image shard %s (+ .idx.npy) not found: make it with tools/make_image_shard.py --list_dir ... --dataset_path ... "
                                "--out_dir %s" % (path, os.path.dirname(path)))
    n, want = len(np.load(path + ".idx.npy")), len(read_list(list_path)[0])
    if n != want:
        raise ValueError("image shard %s holds %d images, %s lists %d: the shard was made from another list" % (path, n, list_path, want))


class DeviceBoxResampler(DeviceResampler):
    """boxes (flat uint8 + table [B, 10] + meta, host or device) -> uint8 [B, size, size] on the device: the classification transforms'
    resample (+ flip), Pillow-exact (ecamp_resample_boxes_u8, BILINEAR; ecamp_resample_boxes_rgb_u8 -- three planes, then Grayscale -- when
    meta's fourth field says the batch holds a colour sample).  With a `ResidentShard` in place of the flat bytes and a table [B, 12]
    (`pack_resident`): ecamp_resample_shard_u8 on the shard's tensor -- the same bytes, no box travels."""

    def __call__(self, flat, table, meta, check=False):
        from .. import hip_ops as ops
        kmax, rows, max_h = (int(v) for v in meta[:3])
        if isinstance(flat, ResidentShard):   # table [B, 12]: the boxes are read where they lie in the uploaded shard
            out = self.run(ops.resample_shard_u8, ops.resample_boxes_workspace_bytes, "box", flat.tensor, table, kmax, rows, max_h, False)
            if check:
                self.raise_on_err(flat)
            return out
        op = ops.resample_boxes_rgb_u8 if len(meta) > 3 and meta[3] else ops.resample_boxes_u8   # filter: their default, BILINEAR
        return self.run(op, ops.resample_boxes_workspace_bytes, "box", flat, table, kmax, rows, max_h, check)

    def raise_on_err(self, shard):
        """Read the flag of the resident calls made so far (one 4-byte read, a host synchronisation), clear it, and raise if it is set."""
        v = int(self.err.item())
        if v == 0:
            return
        self.err.zero_()
        said = [text for bit, text in ((1, "a box needed more taps than the table was sized for (1)"),
                                       (2, "a table row pointed outside the resident shard; its sample was zeros (2)")) if v & bit]
        raise RuntimeError("ecamp_resample_shard_u8 on %s: err_flag = %d: %s" % (shard.path, v, "; ".join(said)))


class DeviceImageLoader:
    """A DataLoader over a `ShardListDataset` (collate_fn=collate_boxes) -> (uint8 [B, R, R] on the device, labels): what
    engine_linprobe's loops iterate, the image being the bytes `ECAMPClassifier` normalises in its stem.
    shard: the `ResidentShard` of a `ShardListDataset(resident=True)` (collate_fn=collate_resident) -- the loader then yields table rows
    alone, the boxes are read from the shard in device memory, and the end of every pass reads the calls' error flag once."""

    def __init__(self, loader, device, img_size, shard=None):
        self.loader, self.dataset, self.shard = loader, loader.dataset, shard
        self.resample = DeviceBoxResampler(device, img_size)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        if self.shard is not None:
            for table, meta, y in self.loader:
                yield self.resample(self.shard, table, meta), y
            self.resample.raise_on_err(self.shard)   # once per pass: nothing else on the training path reads the flag
            return
        for flat, table, meta, y in self.loader:
            yield self.resample(flat, table, meta), y
