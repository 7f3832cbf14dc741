"""numpy restatement of RandAugment / ColorJitter as csrc/randaug.hip computes them (the checker of tests/test_randaug_*.py): Pillow's
arithmetic on uint8 RGB HWC images, op by op, and the per-image draw procedure of d2s.data.

    affine      libImaging/Geometry.c (ImagingGenericTransform with affine_transform, bilinear_filter32RGB / bicubic_filter32RGB), in double
    rotate      PIL/Image.py::rotate's matrix, then the affine
    enhance     PIL/ImageEnhance.py: Image.blend(degenerate, image, factor), libImaging/Blend.c in fp32
    SMOOTH      libImaging/Filter.c's 3x3 kernel in fp32 (the degenerate of Sharpness)
    LUT ops     PIL/ImageOps.py: autocontrast (cutoff 0), equalize, posterize, solarize, invert; timm's solarize_add

An op is the tuple (code, resample, iarg, farg, matrix) that d2s.data.pack_ops writes into the op table.
"""
import math

import numpy as np

(OP_NONE, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD, OP_AFFINE, OP_COLOR, OP_CONTRAST,
 OP_BRIGHTNESS, OP_SHARPNESS) = range(12)
BILINEAR, BICUBIC = 0, 1
FILL = (124, 116, 104)                 # round(255 * ImageNet mean)
# timm's _RAND_INCREASING_TRANSFORMS, in its order
RAND_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd", "ColorIncreasing",
            "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def rotate_matrix(angle, W, H):
    """PIL/Image.py::rotate (no expand, default centre): the six AFFINE coefficients, or None when Pillow copies (angle % 360 == 0)."""
    angle = angle % 360.0
    if angle == 0:
        return None
    assert angle not in (90, 180, 270), "Pillow's transpose paths are not reachable from RandAugment's +-30 degrees"
    cx, cy = W / 2, H / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def affine(img, m, resample, fill=FILL):
    H, W = img.shape[:2]
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    xin = (m[0] * (x + .5) + m[1] * (y + .5)) + m[2]
    yin = (m[3] * (x + .5) + m[4] * (y + .5)) + m[5]
    outside = (xin < 0) | (xin >= W) | (yin < 0) | (yin >= H)
    xin, yin = xin - .5, yin - .5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = (xin - x0)[..., None], (yin - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    src = img.astype(np.float64)
    px = lambda yy, xx: src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
    if resample == BILINEAR:
        lin = lambda a, b, d: a + (b - a) * d
        v1 = lin(px(y0, x0), px(y0, x0 + 1), dx)
        v2 = lin(px(y0 + 1, x0), px(y0 + 1, x0 + 1), dx)
        out = lin(v1, v2, dy).astype(np.uint8)                                   # within [0, 255]: the cast truncates
    else:
        def cubic(v1, v2, v3, v4, d):
            p1, p2, p3, p4 = v2, -v1 + v3, 2 * (v1 - v2) + v3 - v4, -v1 + v2 - v3 + v4
            return p1 + d * (p2 + d * (p3 + d * p4))
        rows = [cubic(px(y0 + r, x0 - 1), px(y0 + r, x0), px(y0 + r, x0 + 1), px(y0 + r, x0 + 2), dx) for r in (-1, 0, 1, 2)]
        out = np.clip(cubic(*rows, dy), 0, 255).astype(np.uint8)
    out[outside] = fill
    return out


# ---- enhance ----------------------------------------------------------------------------------------------------------------------------
def luma(img):
    v = img.astype(np.int64)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f):
    """Image.blend(deg, img, f): fp32 d + f * (x - d); truncated when 0 <= f <= 1, else clipped first."""
    f = np.float32(f)
    if f == 0:
        return np.broadcast_to(np.asarray(deg, np.uint8), img.shape).copy()
    if f == 1:
        return img.copy()
    d = np.broadcast_to(np.asarray(deg), img.shape).astype(np.float32)
    t = d + f * (img.astype(np.float32) - d)
    assert t.dtype == np.float32
    if not 0 <= f <= 1:
        t = np.clip(t, 0, 255)
    return t.astype(np.uint8)


def smooth(img):
    """ImageFilter.SMOOTH: (1,1,1; 1,5,1; 1,1,1) / 13 in fp32, summed as libImaging/Filter.c does (0.5, then the rows y+1, y, y-1, each
    a left-to-right dot product), clip, truncate; the 1-pixel border is copied."""
    H, W = img.shape[:2]
    out = img.copy()
    if H < 3 or W < 3:
        return out
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], np.float32) / np.float32(13)).astype(np.float32)
    v = img.astype(np.float32)
    ss = np.full((H - 2, W - 2, 3), 0.5, np.float32)
    for n, r in enumerate((2, 1, 0)):                                             # rows y+1, y, y-1
        row = v[r:r + H - 2]
        ss = ss + ((row[:, 0:W - 2] * k[3 * n] + row[:, 1:W - 1] * k[3 * n + 1]) + row[:, 2:W] * k[3 * n + 2])
    assert ss.dtype == np.float32
    out[1:-1, 1:-1] = np.clip(ss, 0, 255).astype(np.uint8)
    return out


def contrast_mean(img):
    """int(ImageStat.Stat(L).mean[0] + 0.5): an integer sum divided in double."""
    L = luma(img)
    return int(int(L.astype(np.int64).sum()) / L.size + 0.5)


# ---- LUT ops ----------------------------------------------------------------------------------------------------------------------------
def _apply_luts(img, luts):
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = np.clip(np.asarray(luts[c]), 0, 255).astype(np.uint8)[img[..., c]]
    return out


def autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return list(range(256))
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return [min(255, max(0, int(ix * scale + offset))) for ix in range(256)]


def equalize_lut(h):
    histo = [int(v) for v in h if v]
    if len(histo) <= 1:
        return list(range(256))
    step = (sum(histo) - histo[-1]) // 255
    if not step:
        return list(range(256))
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(255, n // step))                                          # Pillow's point() clips the table to 8 bits
        n += int(h[i])
    return lut


def static_lut(code, iarg):
    i = np.arange(256)
    if code == OP_INVERT:
        return 255 - i
    if code == OP_POSTERIZE:
        return i & ~(2 ** (8 - iarg) - 1)
    if code == OP_SOLARIZE:
        return np.where(i < iarg, i, 255 - i)
    if code == OP_SOLARIZE_ADD:
        return np.where(i < 128, np.minimum(255, i + iarg), i)
    raise ValueError(code)


# ---- one op, a list of ops --------------------------------------------------------------------------------------------------------------
def apply_op(img, op):
    code, resample, iarg, farg, m = op
    if code == OP_NONE:
        return img.copy()
    if code in (OP_AUTOCONTRAST, OP_EQUALIZE):
        f = autocontrast_lut if code == OP_AUTOCONTRAST else equalize_lut
        return _apply_luts(img, [f(np.bincount(img[..., c].reshape(-1), minlength=256)) for c in range(3)])
    if code in (OP_INVERT, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD):
        return _apply_luts(img, [static_lut(code, iarg)] * 3)
    if code == OP_AFFINE:
        return affine(img, m, resample)
    if code == OP_COLOR:
        return blend(luma(img)[..., None], img, farg)
    if code == OP_CONTRAST:
        return blend(contrast_mean(img), img, farg)
    if code == OP_BRIGHTNESS:
        return blend(0, img, farg)
    if code == OP_SHARPNESS:
        return blend(smooth(img), img, farg)
    raise ValueError(code)


def apply_ops(img, ops):
    for op in ops:
        img = apply_op(img, op)
    return img


def mk(code, resample=0, iarg=0, farg=0.0, m=None):
    return (code, resample, int(iarg), float(np.float32(farg)), tuple(m) if m is not None else (0.0,) * 6)


# ---- timm's level -> argument functions (the "increasing" set), and the op each name becomes ----------------------------------------------
def named_op(name, t, neg, S, resample=BICUBIC):
    """The op tuple of RandAugment op `name` at t = level / 10 with the coin flip `neg` (ignored by the ops that have none);
    None when the op is the identity."""
    sgn = -1.0 if neg else 1.0
    if name == "AutoContrast":
        return mk(OP_AUTOCONTRAST)
    if name == "Equalize":
        return mk(OP_EQUALIZE)
    if name == "Invert":
        return mk(OP_INVERT)
    if name == "Rotate":
        m = rotate_matrix(sgn * (30.0 * t), S, S)
        return None if m is None else mk(OP_AFFINE, resample, m=m)
    if name in ("ShearX", "ShearY"):
        v = sgn * (0.3 * t)
        return mk(OP_AFFINE, resample, m=(1, v, 0, 0, 1, 0) if name == "ShearX" else (1, 0, 0, v, 1, 0))
    if name in ("TranslateXRel", "TranslateYRel"):
        px = sgn * (0.45 * t) * S
        return mk(OP_AFFINE, resample, m=(1, 0, px, 0, 1, 0) if name == "TranslateXRel" else (1, 0, 0, 0, 1, px))
    if name == "PosterizeIncreasing":
        bits = 4 - int(4 * t)
        return None if bits >= 8 else mk(OP_POSTERIZE, iarg=bits)
    if name == "SolarizeIncreasing":
        return mk(OP_SOLARIZE, iarg=256 - int(256 * t))
    if name == "SolarizeAdd":
        return mk(OP_SOLARIZE_ADD, iarg=min(128, int(110 * t)))
    code = {"ColorIncreasing": OP_COLOR, "ContrastIncreasing": OP_CONTRAST, "BrightnessIncreasing": OP_BRIGHTNESS,
            "SharpnessIncreasing": OP_SHARPNESS}[name]
    return mk(code, farg=max(0.1, 1.0 + sgn * (0.9 * t)))


def draw_randaug(rng, cfg, S, interpolation):
    """The draw procedure of d2s.data.randaug_ops, restated: cfg = dict(m, mstd, n, p, mmax)."""
    names = [RAND_OPS[int(k)] for k in rng.integers(0, len(RAND_OPS), cfg["n"])]
    ops = []
    for name in names:
        if not rng.random() < cfg["p"]:
            continue
        m = float(rng.normal(cfg["m"], cfg["mstd"])) if cfg["mstd"] > 0 else float(cfg["m"])
        m = min(max(m, 0.0), float(cfg["mmax"]))
        neg = bool(rng.random() < 0.5)
        res = {"bilinear": BILINEAR, "bicubic": BICUBIC}.get(interpolation)
        if res is None:
            res = int(rng.integers(0, 2))
        op = named_op(name, m / 10.0, neg, S, res)
        if op is not None:
            ops.append(op)
    return ops


def draw_jitter(rng, j):
    lo, hi = max(0.0, 1.0 - j), 1.0 + j
    f = [float(rng.uniform(lo, hi)) for _ in range(3)]
    codes = (OP_BRIGHTNESS, OP_CONTRAST, OP_COLOR)
    return [mk(codes[int(k)], farg=f[int(k)]) for k in rng.permutation(3)]


# ---- live Pillow (timm's auto_augment.py calls, restated) ---------------------------------------------------------------------------------
def pil_named(img, name, t, neg, resample=BICUBIC):
    """What timm's RandAugment op `name` does to a uint8 HWC image through Pillow at t = level / 10."""
    from PIL import Image, ImageEnhance, ImageOps
    im = Image.fromarray(img)
    sgn = -1.0 if neg else 1.0
    kw = dict(resample=Image.BICUBIC if resample == BICUBIC else Image.BILINEAR, fillcolor=FILL)
    if name == "AutoContrast":
        out = ImageOps.autocontrast(im)
    elif name == "Equalize":
        out = ImageOps.equalize(im)
    elif name == "Invert":
        out = ImageOps.invert(im)
    elif name == "Rotate":
        out = im.rotate(sgn * (30.0 * t), **kw)
    elif name == "ShearX":
        out = im.transform(im.size, Image.AFFINE, (1, sgn * (0.3 * t), 0, 0, 1, 0), **kw)
    elif name == "ShearY":
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, sgn * (0.3 * t), 1, 0), **kw)
    elif name == "TranslateXRel":
        out = im.transform(im.size, Image.AFFINE, (1, 0, sgn * (0.45 * t) * im.size[0], 0, 1, 0), **kw)
    elif name == "TranslateYRel":
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, sgn * (0.45 * t) * im.size[1]), **kw)
    elif name == "PosterizeIncreasing":
        bits = 4 - int(4 * t)
        out = im if bits >= 8 else ImageOps.posterize(im, bits)
    elif name == "SolarizeIncreasing":
        out = ImageOps.solarize(im, 256 - int(256 * t))
    elif name == "SolarizeAdd":
        add = min(128, int(110 * t))
        out = im.point([min(255, i + add) if i < 128 else i for i in range(256)] * 3)
    else:
        enh = {"ColorIncreasing": ImageEnhance.Color, "ContrastIncreasing": ImageEnhance.Contrast,
               "BrightnessIncreasing": ImageEnhance.Brightness, "SharpnessIncreasing": ImageEnhance.Sharpness}[name]
        out = enh(im).enhance(max(0.1, 1.0 + sgn * (0.9 * t)))
    return np.asarray(out)


def pil_enhance(img, code, f):
    """ImageEnhance.{Color, Contrast, Brightness}(img).enhance(f) (torchvision-style ColorJitter on PIL images, as timm uses it)."""
    from PIL import Image, ImageEnhance
    enh = {OP_COLOR: ImageEnhance.Color, OP_CONTRAST: ImageEnhance.Contrast, OP_BRIGHTNESS: ImageEnhance.Brightness,
           OP_SHARPNESS: ImageEnhance.Sharpness}[code]
    return np.asarray(enh(Image.fromarray(img)).enhance(f))


# ---- the committed Pillow outputs (tools/gen_randaug_fixture.py) ----------------------------------------------------------------------------
def steps_to_ops(steps, S):
    """A fixture case's steps ([name, t, neg, resample] or ["enhance", code, factor]) as op tuples; identities are left out."""
    ops = [mk(st[1], farg=st[2]) if st[0] == "enhance" else named_op(st[0], st[1], st[2], S, st[3]) for st in steps]
    return [op for op in ops if op is not None]


def load_fixture(path):
    """-> list of (image, ops, expected output, steps)."""
    import json
    z = np.load(path)
    return [(z[f"img{c['S']}_{c['img']}"], steps_to_ops(c["steps"], c["S"]), z[f"out{c['S']}_{c['n']}"], c["steps"])
            for c in json.loads(str(z["cases"]))]
