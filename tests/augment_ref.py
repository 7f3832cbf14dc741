"""numpy restatement of the input pipeline of csrc/augment.hip (the checker of tests/test_augment_*.py).

Resampling follows Pillow's libImaging/Resample.c (8 bits per channel) line by line; torchvision crops first, so the crop is
resampled with in0 = 0, in1 = its size.  The integer sums are done as float64 matrix products: every product and partial sum is an
integer below 2**53, so they are exact.  ToTensor + Normalize, erasing and the Mixup blend are fp32, as torch computes them.
"""
import numpy as np

PREC = 22
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


def _filter(f, x):
    x = abs(x)
    if f == 0:
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size, f, first, count):
    """Fixed-point taps of output indices [first, first + count) as a dense float64 matrix [count, in_size] (precompute_coeffs +
    normalize_coeffs_8bpc)."""
    M = np.zeros((count, in_size), np.float64)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = (1.0 if f == 0 else 2.0) * fs
    ss = 1.0 / fs
    for r in range(count):
        center = (first + r + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_filter(f, (t + xmin - center + 0.5) * ss) for t in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for t, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            M[r, xmin + t] = int(-0.5 + v * (1 << PREC)) if v < 0 else int(0.5 + v * (1 << PREC))
    return M


def _clip8(acc):
    return np.clip(np.floor(acc / (1 << PREC)), 0, 255).astype(np.uint8)       # acc is an exact integer: floor == arithmetic shift


def crop_resize(img, crop, grid, win, f, S):
    """uint8 [S, S, 3]: the S x S window at `win` of img[crop] resized to `grid` (Pillow: horizontal pass, then vertical)."""
    i, j, h, w = crop
    gh, gw = grid
    wy, wx = win
    src = img[i:i + h, j:j + w].astype(np.float64)                       # [h, w, 3]
    Mh = coeffs(w, gw, f, wx, S)                                         # [S, w]
    Mv = coeffs(h, gh, f, wy, S)                                         # [S, h]
    rows = np.nonzero(Mv.any(axis=0))[0]
    lo, hi = (rows.min(), rows.max() + 1) if rows.size else (0, 1)
    inter = _clip8(np.matmul(Mh, src[lo:hi]) + (1 << (PREC - 1))).astype(np.float64)            # [rows, S, 3]
    return _clip8((Mv[:, lo:hi] @ inter.reshape(hi - lo, -1)).reshape(S, S, 3) + (1 << (PREC - 1)))


def pil_crop_resize(img, crop, size, f):
    """Live Pillow: Image.crop(...).resize((size, size), BILINEAR / BICUBIC) (what torchvision's resized_crop does)."""
    from PIL import Image
    i, j, h, w = crop
    pim = Image.fromarray(img).crop((j, i, j + w, i + h))
    return np.asarray(pim.resize((size, size), Image.BICUBIC if f == 1 else Image.BILINEAR))


def pil_val(img, S=224, resize=256):
    """Live Pillow: torchvision Resize(256) (bilinear) + CenterCrop(224)."""
    from PIL import Image
    H, W = img.shape[:2]
    short, long_ = (W, H) if W <= H else (H, W)
    ns, nl = resize, int(resize * long_ / short)
    gw, gh = (ns, nl) if W <= H else (nl, ns)
    out = np.asarray(Image.fromarray(img).resize((gw, gh), Image.BILINEAR))
    top, left = int(round((gh - S) / 2.0)), int(round((gw - S) / 2.0))
    return out[top:top + S, left:left + S]


def normalize(u8):
    """ToTensor + Normalize of a uint8 HWC image: fp32 [3, H, W], ((u / 255) - mean) / std with IEEE fp32 division."""
    x = u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    return (x - MEAN[:, None, None]) / STD[:, None, None]


def _mix64(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def erase_normal(seed, sample, c, y, x):
    """The kernel's keyed N(0, 1): splitmix64 of (sample << 40 | c << 32 | y << 16 | x), xor the seed, Box-Muller in float64 -> fp32."""
    y, x = np.asarray(y, np.uint64) & np.uint64(0xFFFF), np.asarray(x, np.uint64) & np.uint64(0xFFFF)
    key = (np.uint64(sample) << np.uint64(40)) | (np.uint64(c) << np.uint64(32)) | (y << np.uint64(16)) | x
    h1 = _mix64(np.uint64(seed) ^ _mix64(key))
    h2 = _mix64(h1)
    u1 = ((h1 >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (h2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)).astype(np.float32)


def erase(v, boxes, mode, seed, sample):
    """RandomErasing on fp32 [3, S, S] in place: later boxes overwrite earlier ones; mode 1 const (0), 2 rand (one value per channel
    and box), 3 pixel (one value per channel and pixel)."""
    S = v.shape[-1]
    for e, (t, l, h, w) in enumerate(boxes):
        ys, xs = np.meshgrid(np.arange(t, t + h), np.arange(l, l + w), indexing="ij")
        for c in range(3):
            if mode == 1:
                v[c, t:t + h, l:l + w] = 0.
            elif mode == 2:
                v[c, t:t + h, l:l + w] = erase_normal(seed, sample, c, 0xFFFF - e, 0xFFFF)
            else:
                v[c, t:t + h, l:l + w] = erase_normal(seed, sample, c, ys, xs)
    assert v.shape[-2:] == (S, S)
    return v


def mix(x, mix_p):
    """Per-sample blend with the partner B-1-i from d2s.data.mix_params' (mode, pix_a, pix_b, box, ...): fp32 [B, 3, S, S]."""
    mode, pa, pb, box = mix_p[:4]
    B = x.shape[0]
    out = x.copy()
    for i in range(B):
        j = B - 1 - i
        if mode[i] == 1:
            out[i] = (x[i] * pa[i]) + (x[j] * pb[i])
        elif mode[i] == 2:
            y0, y1, x0, x1 = box[i]
            out[i, :, y0:y1, x0:x1] = x[j, :, y0:y1, x0:x1]
    return out


def soft_labels(labels, la, lb, C, smoothing):
    """timm mixup_target with per-sample coefficients: y1 * la + y2 * lb, one-hot rows of fp32 (on, off)."""
    off = np.float32(smoothing / C)
    on = np.float32(1. - smoothing + smoothing / C)
    labels = np.asarray(labels)
    y1 = np.full((len(labels), C), off, np.float32)
    y1[np.arange(len(labels)), labels] = on
    y2 = y1[::-1]
    return (y1 * la[:, None].astype(np.float32)) + (y2 * lb[:, None].astype(np.float32))


def augment_batch(images, labels, params, S, mix_p=None, seed=0, num_classes=1000, smoothing=0.1):
    """The whole batch as the kernels compute it -> (fp32 [B, 3, S, S], labels int64 [B] or fp32 soft labels [B, C])."""
    xs = []
    for b, (im, p) in enumerate(zip(images, params)):
        u = crop_resize(im, p["crop"], p["grid"], p["win"], p["filt"], S)
        if p["flip"]:
            u = u[:, ::-1]
        v = normalize(np.ascontiguousarray(u))
        if p["boxes"]:
            erase(v, p["boxes"], p["emode"], seed, b)
        xs.append(v)
    x = np.stack(xs)
    if mix_p is None:
        return x, np.asarray(labels, np.int64)
    return mix(x, mix_p), soft_labels(labels, mix_p[4], mix_p[5], num_classes, smoothing)
