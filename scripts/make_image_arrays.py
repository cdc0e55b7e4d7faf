#!/usr/bin/env python
"""Turn a folder of images, one sub-folder per class, into the two arrays that ``--data_format npy`` trains on:

    {out}/{split}_images.npy   uint8 [N, S, S, 3]     {out}/{split}_labels.npy   int64 [N]
    {out}/{split}_classes.txt  the class of each label, one name per line (sorted sub-folder names)

Every image is decoded with PIL, converted to RGB, resized so that its shorter side is the store size S (bilinear,
PIL's reducing filter) and cropped to the centred S x S square.  The device pipeline crops and resizes from there
(RandomResizedCrop for training, resize + centre crop for evaluation), so S is usually a little above the training
size: 256 for 224.  The images array is written through a memory map, one image at a time.

Usage: python scripts/make_image_arrays.py SRC_DIR OUT_DIR --split train [--size 256]
"""
import argparse
import os

import numpy as np

EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".gif", ".tif", ".tiff", ".webp", ".ppm")


def list_images(src):
    """-> (class names, [(path, label)]) of ``src``, both in sorted order."""
    classes = sorted(d for d in os.listdir(src) if os.path.isdir(os.path.join(src, d)))
    if not classes:
        raise SystemExit(f"{src}: no class sub-folders")
    items = []
    for label, name in enumerate(classes):
        for root, _, files in sorted(os.walk(os.path.join(src, name))):
            items += [(os.path.join(root, f), label) for f in sorted(files) if f.lower().endswith(EXTENSIONS)]
    if not items:
        raise SystemExit(f"{src}: no images")
    return classes, items


def load_square(path, size):
    """The image at ``path`` as uint8 [size, size, 3]: shorter side resized to ``size``, then the centre crop."""
    from PIL import Image

    with Image.open(path) as im:
        im = im.convert("RGB")
        w, h = im.size
        if w <= h:
            nw, nh = size, max(size, int(round(h * size / w)))
        else:
            nw, nh = max(size, int(round(w * size / h))), size
        im = im.resize((nw, nh), resample=Image.BILINEAR)
        left, top = (nw - size) // 2, (nh - size) // 2
        return np.asarray(im.crop((left, top, left + size, top + size)), dtype=np.uint8)


def convert(src, out, split, size):
    classes, items = list_images(src)
    os.makedirs(out, exist_ok=True)
    images = np.lib.format.open_memmap(os.path.join(out, f"{split}_images.npy"), mode="w+", dtype=np.uint8,
                                       shape=(len(items), size, size, 3))
    for i, (path, _) in enumerate(items):
        images[i] = load_square(path, size)
    images.flush()
    np.save(os.path.join(out, f"{split}_labels.npy"), np.array([label for _, label in items], dtype=np.int64))
    with open(os.path.join(out, f"{split}_classes.txt"), "w") as f:
        f.write("\n".join(classes) + "\n")
    return len(items), len(classes)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src", help="folder with one sub-folder of images per class")
    ap.add_argument("out", help="folder the arrays are written to")
    ap.add_argument("--split", default="train", help="prefix of the files: train or val")
    ap.add_argument("--size", type=int, default=256, help="side of the stored square images")
    a = ap.parse_args(argv)
    if a.size < 1:
        ap.error("--size must be at least 1")
    n, k = convert(a.src, a.out, a.split, a.size)
    print(f"{a.split}: {n} images of {k} classes at {a.size} x {a.size} -> {a.out}")


if __name__ == "__main__":
    main()
