"""Writes tests/golden/randaug_pil.npz: small uint8 images and what Pillow makes of them under timm's RandAugment ops and ColorJitter,
the expected outputs of csrc/randaug.hip and tests/randaug_ref.py.  Needs Pillow; run from the repository root:

    python tools/gen_randaug_fixture.py

Cases: each of the 15 "increasing" ops at two levels (one with the sign flipped), the five geometric ones with bilinear and bicubic;
composed two-op lists (a repeated op among them); the ColorJitter orders; on 16x16 and 19x19 images (19 * 3 row bytes are odd).
A case is a list of steps; a step is [name, t, neg, resample] (a RandAugment op at t = level / 10) or ["enhance", code, factor]."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import randaug_ref as R          # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "randaug_pil.npz")
GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")


def images(rng, S):
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    smooth = np.stack([128 + 100 * np.sin(x / (2 + c) + y / (3 + c)) for c in range(3)], -1) + rng.integers(-12, 13, (S, S, 3))
    return [rng.integers(0, 256, (S, S, 3), dtype=np.uint8), np.clip(smooth, 0, 255).astype(np.uint8),
            rng.integers(70, 180, (S, S, 3), dtype=np.uint8)]


def pil_steps(img, steps):
    for st in steps:
        img = R.pil_enhance(img, st[1], st[2]) if st[0] == "enhance" else R.pil_named(img, st[0], st[1], st[2], st[3])
    return img


def main():
    from PIL import Image
    rng = np.random.default_rng(20261017)
    arrays, cases = {}, []
    for S in (16, 19):
        for k, im in enumerate(images(rng, S)):
            arrays[f"img{S}_{k}"] = im
        lists = []
        for name in R.RAND_OPS:
            for t, neg in ((0.37, False), (0.9, True)):
                for res in ((R.BILINEAR, R.BICUBIC) if name in GEOMETRIC else (R.BICUBIC,)):
                    lists.append([[name, t, neg, res]])
        lists += [[["Rotate", 0.78, False, R.BICUBIC], ["SharpnessIncreasing", 0.9, False, 0]],
                  [["Equalize", 0.5, False, 0], ["ShearX", 0.6, True, R.BILINEAR]],
                  [["ContrastIncreasing", 0.85, True, 0], ["ContrastIncreasing", 0.4, False, 0]],
                  [["TranslateYRel", 0.5, True, R.BILINEAR], ["TranslateYRel", 0.5, True, R.BILINEAR]],
                  [["SolarizeAdd", 0.9, False, 0], ["AutoContrast", 0.9, False, 0]],
                  [["ColorIncreasing", 1.0, True, 0], ["PosterizeIncreasing", 1.0, False, 0]]]
        f = (0.71, 1.32, 0.94)
        codes = (R.OP_BRIGHTNESS, R.OP_CONTRAST, R.OP_COLOR)
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (2, 1, 0)):
            lists.append([["enhance", codes[k], f[k]] for k in order])
        for n, steps in enumerate(lists):
            k = n % 3
            arrays[f"out{S}_{n}"] = pil_steps(arrays[f"img{S}_{k}"], steps)
            cases.append(dict(S=S, img=k, n=n, steps=steps))
    arrays["cases"] = np.array(json.dumps(cases))
    arrays["pillow_version"] = np.array(Image.__version__)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(cases)} cases", file=sys.stderr)


if __name__ == "__main__":
    main()
