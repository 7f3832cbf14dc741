"""Writes tests/golden/augment_pil.npz: small uint8 sources and what Pillow makes of them, the expected outputs of the input pipeline's
resampling (csrc/augment.hip, tests/augment_ref.py).  Needs Pillow; run from the repository root:

    python tools/gen_augment_fixture.py

Cases: crop(...).resize((S, S)) with bilinear and bicubic, up- and down-scaling, odd sizes, a source wider than tall, a 1-pixel-wide
crop and crops touching every edge; and one torchvision Resize(256) + CenterCrop(224) (bilinear)."""
import os
import sys

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "augment_pil.npz")


def smooth_image(rng, H, W):
    """A gradient + blobs + mild noise (compresses well, still exercises every tap)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / (3 + c) + y / (5 + 2 * c)) for c in range(3)], -1)
    img += rng.integers(-12, 13, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def main():
    rng = np.random.default_rng(20261016)
    srcs = [smooth_image(rng, 37, 53), smooth_image(rng, 61, 29), smooth_image(rng, 9, 7), rng.integers(0, 256, (23, 41, 3), dtype=np.uint8),
            smooth_image(rng, 300, 260)]
    # (source, (i, j, h, w), S, filter 0 bilinear / 1 bicubic)
    cases = [(0, (0, 0, 37, 53), 24, 1), (0, (0, 0, 37, 53), 24, 0),           # whole image, down
             (0, (5, 11, 20, 30), 47, 1), (0, (5, 11, 20, 30), 47, 0),         # inner crop, up
             (0, (30, 0, 7, 53), 16, 1),                                       # bottom edge, left + right edges
             (1, (0, 28, 61, 1), 12, 1), (1, (0, 28, 61, 1), 12, 0),           # 1-pixel-wide crop at the right edge
             (1, (0, 0, 1, 29), 19, 1),                                        # 1-pixel-tall crop at the top
             (2, (0, 0, 9, 7), 31, 1), (2, (2, 1, 3, 5), 33, 0),               # tiny source, up by 4-10x
             (3, (0, 0, 23, 41), 17, 1), (3, (3, 4, 20, 37), 11, 0), (3, (0, 0, 23, 41), 64, 1),   # noise, down / up
             (4, (10, 3, 290, 251), 56, 1), (4, (0, 0, 300, 260), 56, 0)]      # down by ~5x
    arrays = {f"src{k}": s for k, s in enumerate(srcs)}
    meta = []
    for n, (k, (i, j, h, w), S, f) in enumerate(cases):
        pim = Image.fromarray(srcs[k]).crop((j, i, j + w, i + h))
        arrays[f"out{n}"] = np.asarray(pim.resize((S, S), Image.BICUBIC if f else Image.BILINEAR))
        meta.append([k, i, j, h, w, S, f])
    arrays["cases"] = np.array(meta, np.int32)
    val_src = srcs[4]
    H, W = val_src.shape[:2]
    gw, gh = (256, int(256 * H / W)) if W <= H else (int(256 * W / H), 256)
    full = np.asarray(Image.fromarray(val_src).resize((gw, gh), Image.BILINEAR))
    top, left = int(round((gh - 224) / 2.0)), int(round((gw - 224) / 2.0))
    arrays["val_src"] = np.array([4], np.int32)
    arrays["val_out"] = full[top:top + 224, left:left + 224]
    arrays["pillow_version"] = np.array(Image.__version__)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(cases)} resize cases + 1 Resize(256)+CenterCrop(224)", file=sys.stderr)


if __name__ == "__main__":
    main()
