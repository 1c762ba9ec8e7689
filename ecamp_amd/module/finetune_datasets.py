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

from .pretrain_datasets import pil_loader, random_flip, random_resized_crop_params

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
