"""Image-folder input pipeline: the reference's data sets and transforms (build_data_sets.py:8-34, mask_predictor.py:234-272), with the
per-pixel work on the GPU (csrc/augment.hip) and only JPEG decode on the host.

    listing      torchvision.datasets.ImageFolder: classes = sorted sub-directories, files from a sorted walk, torchvision's extension
                 list matched case-insensitively, decoded with Pillow open(...).convert('RGB') in DataLoader workers
    split        mask_predictor.py:236-240: np.random.seed(42); shuffle(range(N)); the first 20 % is the validation set
    train        timm create_transform(is_training=True): RandomResizedCropAndInterpolation(224, scale (0.08, 1), ratio (3/4, 4/3)),
                 RandomHorizontalFlip(0.5), RandAugment (--aa rand-...) or else ColorJitter (--color-jitter), ToTensor,
                 Normalize(ImageNet mean / std), RandomErasing(reprob, remode, recount)
    val          Resize(256) (bilinear), CenterCrop(224), ToTensor, Normalize
    mix          timm Mixup (train.py:29-31) with its soft labels (mixup_target)

Every random parameter is drawn here, on the host, from numpy Generators keyed by (seed, epoch, rank, position in the epoch) for the
per-image transforms and by (seed, epoch, rank, batch index) for Mixup, so a batch does not depend on the number of workers.  Pillow
is imported only by `decode`, i.e. only when folder data is asked for.

Odd batches (the last batch of an epoch; the reference's loaders keep it, drop_last=False, and timm's Mixup asserts on it): the partner
of sample i is B-1-i, so the middle sample pairs with itself.  In 'batch' and 'elem' mode it is then mixed with itself exactly as
timm's formulas would do it; in 'pair' mode it keeps lam = 1 (no mixing, a smoothed one-hot label).
"""
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

# torchvision.datasets.folder.IMG_EXTENSIONS
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")
MAX_ERASE = 8                 # erase boxes per image in the descriptor (csrc/augment.hip)
DESC_INTS = 64
(A_OFF_LO, A_OFF_HI, A_H, A_W, A_CI, A_CJ, A_CH, A_CW, A_GH, A_GW, A_WY, A_WX, A_FILTER, A_FLIP, A_YFIRST, A_YN, A_ROWOFF, A_EMODE,
 A_ECOUNT, A_MIX, A_PIXA, A_PIXB, A_LABA, A_LABB, A_CY0, A_CY1, A_CX0, A_CX1, A_LABEL) = range(29)
A_BOXES = 32
BILINEAR, BICUBIC = 0, 1
FILTERS = {"bilinear": BILINEAR, "bicubic": BICUBIC}
ERASE_MODES = {"const": 1, "rand": 2, "pixel": 3}      # timm: anything that is not 'rand' or 'pixel' erases with zeros
MIX_NONE, MIX_MIXUP, MIX_CUTMIX = 0, 1, 2
# RandAugment / ColorJitter op table (csrc/randaug.hip): [B, RA_MAX_OPS, RA_OP_INTS] int32, an image's list ends at the first code 0
RA_MAX_OPS, RA_OP_INTS = 8, 16
(OP_NONE, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD, OP_AFFINE, OP_COLOR, OP_CONTRAST,
 OP_BRIGHTNESS, OP_SHARPNESS) = range(12)
E_CODE, E_RESAMPLE, E_IARG, E_FARG, E_MATRIX = range(5)       # E_FARG: a float32's bits; E_MATRIX: six float64 (ints 4..15)
# timm's _RAND_INCREASING_TRANSFORMS, in its order
RAND_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd", "ColorIncreasing",
            "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")


# ---- listing, split, shards -----------------------------------------------------------------------------------------------------------
def find_classes(root):
    """torchvision's find_classes: the sorted names of the sub-directories of `root`."""
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"couldn't find any class folder in {root}")
    return classes, {c: i for i, c in enumerate(classes)}


def make_dataset(root, class_to_idx, extensions=IMG_EXTENSIONS):
    """torchvision's make_dataset: (path, class index) for every file under each class folder, in a sorted walk, whose lower-cased name
    ends with one of `extensions`."""
    out = []
    for cls in sorted(class_to_idx):
        for dirpath, _, fnames in sorted(os.walk(os.path.join(root, cls), followlinks=True)):
            for fname in sorted(fnames):
                if fname.lower().endswith(extensions):
                    out.append((os.path.join(dirpath, fname), class_to_idx[cls]))
    return out


def image_folder(root):
    """(samples, classes) of torchvision.datasets.ImageFolder(root)."""
    classes, class_to_idx = find_classes(root)
    samples = make_dataset(root, class_to_idx)
    if not samples:
        raise FileNotFoundError(f"found no valid image file under {root} (extensions: {', '.join(IMG_EXTENSIONS)})")
    return samples, classes


def split_indices(n, seed=42, val_fraction=0.2):
    """mask_predictor.py:236-240 under its np.random.seed(42): (train indices, val indices)."""
    idx = list(range(n))
    np.random.RandomState(seed).shuffle(idx)
    split = int(np.floor(val_fraction * n))
    return idx[split:], idx[:split]


def epoch_order(indices, seed, epoch):
    """The training subset in a fresh random order per epoch (the reference's SubsetRandomSampler), the same on every rank."""
    perm = np.random.default_rng([seed, epoch, 0x5348]).permutation(len(indices))
    return [indices[k] for k in perm]


def shard(indices, rank, world):
    """torch DistributedSampler(shuffle=False, drop_last=False) over `indices` (ddp_training.py:15): padded by wrapping to a multiple of
    `world` so that every rank runs the same number of steps, then every world-th element from `rank`.  The shards are disjoint
    except for the (at most world-1) padding repeats and together cover the whole list."""
    indices = list(indices)
    if world <= 1:
        return indices
    total = -(-len(indices) // world) * world
    pad = total - len(indices)
    padded = indices + (indices * (pad // max(len(indices), 1) + 1))[:pad]
    return padded[rank:total:world]


# ---- per-image parameter samplers (timm 0.4.12's formulas, restated; timm is not a dependency) ------------------------------------------
def rrc_params(rng, H, W, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.)):
    """timm RandomResizedCropAndInterpolation.get_params -> (i, j, h, w):
        area = W * H; up to 10 attempts of
            target_area = U(scale) * area;  aspect = exp(U(log ratio[0], log ratio[1]))
            w = int(round(sqrt(target_area * aspect)));  h = int(round(sqrt(target_area / aspect)))
            if 0 < w <= W and 0 < h <= H:  i = randint(0, H - h);  j = randint(0, W - w)  (both inclusive)
        then the centre-crop fallback: in_ratio = W / H; below min(ratio): w = W, h = int(round(w / min(ratio))); above max(ratio):
        h = H, w = int(round(h * max(ratio))); else the whole image; i = (H - h) // 2, j = (W - w) // 2.
    (`0 < w` / `0 < h` as in later timm versions: a 1-pixel image would otherwise ask for an empty crop.)"""
    area = W * H
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target_area = rng.uniform(*scale) * area
        aspect = math.exp(rng.uniform(*log_ratio))
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= W and 0 < h <= H:
            return int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w
    in_ratio = W / H
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def erase_params(rng, prob, max_count, S, min_area=0.02, max_area=1 / 3, min_aspect=0.3):
    """timm RandomErasing._erase on an S x S image -> list of (top, left, h, w):
        nothing if random() > prob; count = 1 if max_count == 1 else randint(1, max_count); per box up to 10 attempts of
            target_area = U(min_area, max_area) * S * S / count;  aspect = exp(U(log min_aspect, log 1 / min_aspect))
            h = int(round(sqrt(target_area * aspect)));  w = int(round(sqrt(target_area / aspect)))
            if w < S and h < S:  top = randint(0, S - h);  left = randint(0, S - w)  (inclusive)."""
    if prob <= 0 or rng.random() > prob:
        return []
    count = 1 if max_count <= 1 else int(rng.integers(1, max_count + 1))
    log_aspect = (math.log(min_aspect), math.log(1 / min_aspect))
    boxes = []
    for _ in range(count):
        for _ in range(10):
            target_area = rng.uniform(min_area, max_area) * S * S / count
            aspect = math.exp(rng.uniform(*log_aspect))
            h = int(round(math.sqrt(target_area * aspect)))
            w = int(round(math.sqrt(target_area / aspect)))
            if w < S and h < S:
                boxes.append((int(rng.integers(0, S - h + 1)), int(rng.integers(0, S - w + 1)), h, w))
                break
    return boxes


# ---- RandAugment / ColorJitter (timm 0.4.12's auto_augment.py and torchvision's ColorJitter on PIL images, restated) ---------------------
def parse_auto_augment(text):
    """timm's rand_augment_transform config string `rand-mM[-mstdS][-nN][-pP][-mmaxX]-inc1` -> dict(m, mstd, n, p, mmax), or None when
    off ('', 'none', None).  Only the "increasing" op set with uniform choice is built: another policy family, inc0 (or no inc key) and
    the weighted choice `w` raise ValueError."""
    if text is None or text.strip().lower() in ("", "none"):
        return None
    parts = text.strip().lower().split("-")
    if parts[0] != "rand":
        raise ValueError(f"auto-augment policy '{text}': only RandAugment ('rand-m9-mstd0.5-inc1') is built")
    cfg, inc = dict(m=10.0, mstd=0.0, n=2, p=0.5, mmax=10.0), None
    for part in parts[1:]:
        for key in ("mstd", "mmax", "inc", "m", "n", "p", "w"):            # longer keys first
            if part.startswith(key):
                val = part[len(key):]
                break
        else:
            raise ValueError(f"auto-augment policy '{text}': unknown key in '{part}'")
        try:
            num = float(val)
        except ValueError:
            raise ValueError(f"auto-augment policy '{text}': '{part}' has no number") from None
        if key == "w":
            raise ValueError(f"auto-augment policy '{text}': weighted op choice ('w') is not built")
        if key == "inc":
            inc = bool(int(num))
        elif key == "n":
            cfg["n"] = int(num)
        else:
            cfg[key] = num
    if not inc:
        raise ValueError(f"auto-augment policy '{text}': only the increasing op set ('inc1') is built")
    if not 0 <= cfg["n"] <= RA_MAX_OPS:
        raise ValueError(f"auto-augment policy '{text}': n outside 0..{RA_MAX_OPS} (ops per image in the op table)")
    if not (0 <= cfg["p"] <= 1 and cfg["m"] >= 0 and cfg["mstd"] >= 0 and cfg["mmax"] >= 0):
        raise ValueError(f"auto-augment policy '{text}': p outside [0, 1] or a negative magnitude")
    return cfg


def rotate_matrix(angle, W, H):
    """PIL/Image.py::rotate (no expand, default centre): the six AFFINE coefficients, in double as the Python computes them; None when
    Pillow copies the image (angle % 360 == 0).  RandAugment's angles stay within +-30 degrees, so the transpose paths never apply."""
    angle = angle % 360.0
    if angle == 0:
        return None
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def _op(code, resample=0, iarg=0, farg=0.0, matrix=None):
    """One op of the table: (code, resample, int argument, float argument, six doubles)."""
    return (code, resample, int(iarg), float(np.float32(farg)), tuple(float(v) for v in matrix) if matrix is not None else (0.0,) * 6)


def randaug_op(name, t, neg, S, resample):
    """timm's level_fn of the increasing op `name` at t = level / 10 with the coin flip `neg` -> the table op, or None for an identity."""
    sgn = -1.0 if neg else 1.0
    if name == "AutoContrast":
        return _op(OP_AUTOCONTRAST)
    if name == "Equalize":
        return _op(OP_EQUALIZE)
    if name == "Invert":
        return _op(OP_INVERT)
    if name == "Rotate":
        m = rotate_matrix(sgn * (30.0 * t), S, S)
        return None if m is None else _op(OP_AFFINE, resample, matrix=m)
    if name == "ShearX":
        return _op(OP_AFFINE, resample, matrix=(1, sgn * (0.3 * t), 0, 0, 1, 0))
    if name == "ShearY":
        return _op(OP_AFFINE, resample, matrix=(1, 0, 0, sgn * (0.3 * t), 1, 0))
    if name == "TranslateXRel":
        return _op(OP_AFFINE, resample, matrix=(1, 0, sgn * (0.45 * t) * S, 0, 1, 0))
    if name == "TranslateYRel":
        return _op(OP_AFFINE, resample, matrix=(1, 0, 0, 0, 1, sgn * (0.45 * t) * S))
    if name == "PosterizeIncreasing":
        bits = 4 - int(4 * t)
        return None if bits >= 8 else _op(OP_POSTERIZE, iarg=bits)
    if name == "SolarizeIncreasing":
        return _op(OP_SOLARIZE, iarg=256 - int(256 * t))
    if name == "SolarizeAdd":
        return _op(OP_SOLARIZE_ADD, iarg=min(128, int(110 * t)))
    code = {"ColorIncreasing": OP_COLOR, "ContrastIncreasing": OP_CONTRAST, "BrightnessIncreasing": OP_BRIGHTNESS,
            "SharpnessIncreasing": OP_SHARPNESS}[name]
    return _op(code, farg=max(0.1, 1.0 + sgn * (0.9 * t)))


def randaug_ops(rng, cfg, S, interpolation):
    """One image's RandAugment: n ops chosen uniformly with replacement; each is the identity with probability 1 - p, otherwise drawn at
    level clip(gauss(m, mstd), 0, mmax) with its coin flip, and with BILINEAR or BICUBIC drawn per application when the run's
    interpolation is 'random'."""
    names = [RAND_OPS[int(k)] for k in rng.integers(0, len(RAND_OPS), cfg["n"])]
    ops = []
    for name in names:
        if not rng.random() < cfg["p"]:
            continue
        m = float(rng.normal(cfg["m"], cfg["mstd"])) if cfg["mstd"] > 0 else float(cfg["m"])
        m = min(max(m, 0.0), float(cfg["mmax"]))
        neg = bool(rng.random() < 0.5)
        resample = FILTERS.get(interpolation)
        if resample is None:
            resample = int(rng.integers(0, 2))
        op = randaug_op(name, m / 10.0, neg, S, resample)
        if op is not None:
            ops.append(op)
    return ops


def jitter_ops(rng, j):
    """ColorJitter(j, j, j): brightness, contrast and saturation factors uniform in [max(0, 1 - j), 1 + j], applied in a random order
    (ImageEnhance.Brightness / Contrast / Color).  No hue."""
    lo, hi = max(0.0, 1.0 - j), 1.0 + j
    f = [float(rng.uniform(lo, hi)) for _ in range(3)]
    codes = (OP_BRIGHTNESS, OP_CONTRAST, OP_COLOR)
    return [_op(codes[int(k)], farg=f[int(k)]) for k in rng.permutation(3)]


def pack_ops(op_lists):
    """Per-image op lists -> the int32 table [B, RA_MAX_OPS, RA_OP_INTS] of csrc/randaug.hip."""
    table = np.zeros((len(op_lists), RA_MAX_OPS, RA_OP_INTS), np.int32)
    for b, ops in enumerate(op_lists):
        if len(ops) > RA_MAX_OPS:
            raise ValueError(f"at most {RA_MAX_OPS} ops per image")
        for k, (code, resample, iarg, farg, matrix) in enumerate(ops):
            assert OP_NONE < code <= OP_SHARPNESS and resample in (BILINEAR, BICUBIC) and 0 <= iarg <= 256, (code, resample, iarg)
            table[b, k, :E_MATRIX] = (code, resample, iarg, int(np.float32(farg).view(np.int32)))
            table[b, k, E_MATRIX:E_MATRIX + 12] = np.asarray(matrix, np.float64).view(np.int32)
    return table


@dataclass
class AugmentOptions:
    """The training transform's flags (utils.parse_args: --train-interpolation, --reprob, --remode, --recount, --aa, --color-jitter)."""
    interpolation: str = "bicubic"          # bilinear | bicubic | random (one of the two per image)
    reprob: float = 0.25
    remode: str = "pixel"
    recount: int = 1
    hflip: float = 0.5
    auto_augment: str = ""                  # '' / 'none': off; else timm's 'rand-m9-mstd0.5-inc1' form (parse_auto_augment)
    color_jitter: float = 0.0               # used only when auto_augment is off, as in timm's transforms_imagenet_train


def train_params(rng, H, W, opts, S):
    """One image's RandomResizedCropAndInterpolation + RandomHorizontalFlip + RandomErasing parameters and, when the options ask for
    them, its RandAugment or ColorJitter ops (drawn last: with both off the draws are those of the transform without them)."""
    i, j, h, w = rrc_params(rng, H, W)
    interp = opts.interpolation
    if interp == "random":
        interp = ("bilinear", "bicubic")[int(rng.integers(0, 2))]
    flip = bool(rng.random() < opts.hflip)
    boxes = erase_params(rng, opts.reprob, opts.recount, S)
    p = dict(crop=(i, j, h, w), grid=(S, S), win=(0, 0), filt=FILTERS[interp], flip=flip,
             emode=ERASE_MODES.get(opts.remode.lower(), 1) if boxes else 0, boxes=boxes)
    ra = parse_auto_augment(opts.auto_augment)
    if ra is not None:
        p["ops"] = randaug_ops(rng, ra, S, opts.interpolation)
    elif opts.color_jitter > 0:
        p["ops"] = jitter_ops(rng, opts.color_jitter)
    return p


def val_params(H, W, S=224, resize=256):
    """Resize(resize) + CenterCrop(S): the short side becomes `resize`, the long side int(resize * long / short) (torchvision's
    _compute_resized_output_size); the window's top-left is int(round((grid - S) / 2.0)) (F.center_crop)."""
    short, long_ = (W, H) if W <= H else (H, W)
    new_short, new_long = resize, int(resize * long_ / short)
    gw, gh = (new_short, new_long) if W <= H else (new_long, new_short)
    return dict(crop=(0, 0, H, W), grid=(gh, gw), win=(int(round((gh - S) / 2.0)), int(round((gw - S) / 2.0))), filt=BILINEAR,
                flip=False, emode=0, boxes=[])


# ---- Mixup / CutMix parameters (timm Mixup, restated) -------------------------------------------------------------------------------------
@dataclass
class MixConfig:
    """timm Mixup(mixup_alpha, cutmix_alpha, cutmix_minmax, prob, switch_prob, mode, label_smoothing, num_classes), correct_lam=True
    (mask_predictor.py:262-267 with utils.py:305-315's flags).  cutmix_minmax, when set, forces cutmix_alpha = 1."""
    mixup_alpha: float = 0.8
    cutmix_alpha: float = 1.0
    cutmix_minmax: tuple = None
    prob: float = 1.0
    switch_prob: float = 0.5
    mode: str = "batch"
    smoothing: float = 0.1
    num_classes: int = 1000

    def __post_init__(self):
        if self.cutmix_minmax is not None:
            assert len(self.cutmix_minmax) == 2
            self.cutmix_alpha = 1.0


def rand_bbox(rng, S, lam, margin=0.):
    """timm rand_bbox on an S x S image: ratio = sqrt(1 - lam); cut = int(S * ratio); centre cy, cx = randint(0, S) (exclusive);
    box = clip(c -+ cut // 2, 0, S).  numpy arithmetic on lam's own type, as timm does it (float32 lam in elem / pair mode)."""
    ratio = np.sqrt(1 - lam)
    cut_h, cut_w = int(S * ratio), int(S * ratio)
    margin_y, margin_x = int(margin * cut_h), int(margin * cut_w)
    cy = rng.integers(0 + margin_y, S - margin_y)
    cx = rng.integers(0 + margin_x, S - margin_x)
    return (int(np.clip(cy - cut_h // 2, 0, S)), int(np.clip(cy + cut_h // 2, 0, S)),
            int(np.clip(cx - cut_w // 2, 0, S)), int(np.clip(cx + cut_w // 2, 0, S)))


def rand_bbox_minmax(rng, S, minmax):
    """timm rand_bbox_minmax: cut = randint(int(S * min), int(S * max)) (exclusive); top-left = randint(0, S - cut)."""
    cut_h = int(rng.integers(int(S * minmax[0]), int(S * minmax[1])))
    cut_w = int(rng.integers(int(S * minmax[0]), int(S * minmax[1])))
    yl = int(rng.integers(0, S - cut_h))
    xl = int(rng.integers(0, S - cut_w))
    return yl, yl + cut_h, xl, xl + cut_w


def cutmix_bbox_and_lam(rng, S, lam, minmax=None):
    """timm cutmix_bbox_and_lam with correct_lam=True: lam = 1 - box area / (S * S) (a float64)."""
    box = rand_bbox_minmax(rng, S, minmax) if minmax is not None else rand_bbox(rng, S, lam)
    yl, yu, xl, xu = box
    return box, 1. - np.int64((yu - yl) * (xu - xl)) / float(S * S)


def _params_per_elem(rng, n, cfg):
    """timm Mixup._params_per_elem: float32 lam per element and a cutmix flag."""
    lam = np.ones(n, dtype=np.float32)
    use_cutmix = np.zeros(n, dtype=bool)
    if cfg.mixup_alpha > 0. and cfg.cutmix_alpha > 0.:
        use_cutmix = rng.random(n) < cfg.switch_prob
        lam_mix = np.where(use_cutmix, rng.beta(cfg.cutmix_alpha, cfg.cutmix_alpha, size=n),
                           rng.beta(cfg.mixup_alpha, cfg.mixup_alpha, size=n))
    elif cfg.mixup_alpha > 0.:
        lam_mix = rng.beta(cfg.mixup_alpha, cfg.mixup_alpha, size=n)
    elif cfg.cutmix_alpha > 0.:
        use_cutmix = np.ones(n, dtype=bool)
        lam_mix = rng.beta(cfg.cutmix_alpha, cfg.cutmix_alpha, size=n)
    else:
        raise ValueError("mixup_alpha and cutmix_alpha are both 0")
    lam = np.where(rng.random(n) < cfg.prob, lam_mix.astype(np.float32), lam)
    return lam, use_cutmix


def _params_per_batch(rng, cfg):
    """timm Mixup._params_per_batch: a Python-float lam and a cutmix flag."""
    lam, use_cutmix = 1., False
    if rng.random() < cfg.prob:
        if cfg.mixup_alpha > 0. and cfg.cutmix_alpha > 0.:
            use_cutmix = bool(rng.random() < cfg.switch_prob)
            lam_mix = rng.beta(cfg.cutmix_alpha, cfg.cutmix_alpha) if use_cutmix else rng.beta(cfg.mixup_alpha, cfg.mixup_alpha)
        elif cfg.mixup_alpha > 0.:
            lam_mix = rng.beta(cfg.mixup_alpha, cfg.mixup_alpha)
        elif cfg.cutmix_alpha > 0.:
            use_cutmix = True
            lam_mix = rng.beta(cfg.cutmix_alpha, cfg.cutmix_alpha)
        else:
            raise ValueError("mixup_alpha and cutmix_alpha are both 0")
        lam = float(lam_mix)
    return lam, use_cutmix


def mix_params(rng, B, cfg, S):
    """Per-sample blend of timm's Mixup.__call__ ('batch', 'pair' or 'elem') on a batch of B (partner of i: B-1-i):
        mode [B] (0 none, 1 mixup, 2 cutmix), pix_a / pix_b [B] fp32 (mixup: out = fl(x * a) + fl(x' * b)), box [B, 4] (y0, y1, x0, x1),
        lab_a / lab_b [B] fp32 (label = y * a + y' * b).
    The coefficients are rounded as timm's torch ops round them: in 'batch' mode lam is a Python float, x.mul_(lam) and
    x.flip(0).mul_(1. - lam) use fl32(lam) and fl32(1 - lam); in 'elem' / 'pair' mode lam is float32 and 1 - lam is a float32
    subtraction; a cutmix lam is the box-corrected float64 lam, stored as float32 in 'elem' / 'pair' mode."""
    mode = np.zeros(B, np.int32)
    pa, pb = np.ones(B, np.float32), np.zeros(B, np.float32)
    box = np.zeros((B, 4), np.int32)
    one = np.float32(1)
    if cfg.mode == "batch":
        lam, use_cutmix = _params_per_batch(rng, cfg)
        if lam != 1.:
            if use_cutmix:
                b, lam = cutmix_bbox_and_lam(rng, S, lam, cfg.cutmix_minmax)
                mode[:], box[:] = MIX_CUTMIX, b
            else:
                mode[:], pa[:], pb[:] = MIX_MIXUP, np.float32(lam), np.float32(1. - lam)
        lam = float(lam)
        return mode, pa, pb, box, np.full(B, lam, np.float32), np.full(B, 1. - lam, np.float32)
    if cfg.mode not in ("pair", "elem"):
        raise ValueError(f"mixup mode {cfg.mode}")
    pair = cfg.mode == "pair"
    n = B // 2 if pair else B
    lam_b, use_cutmix = _params_per_elem(rng, n, cfg)
    for i in range(n):
        js = (i, B - 1 - i) if pair else (i,)
        lam = lam_b[i]
        if lam != 1.:
            if use_cutmix[i]:
                b, lam_c = cutmix_bbox_and_lam(rng, S, lam, cfg.cutmix_minmax)
                lam_b[i] = lam_c
                for k in js:
                    mode[k], box[k] = MIX_CUTMIX, b
            else:
                for k in js:
                    mode[k], pa[k], pb[k] = MIX_MIXUP, lam, one - lam
    if pair:
        lam_b = np.concatenate((lam_b, np.ones(B - 2 * n, np.float32), lam_b[::-1]))
    return mode, pa, pb, box, lam_b.astype(np.float32), (one - lam_b).astype(np.float32)


# ---- Pillow's resampling bounds (csrc/augment.hip computes the taps; the host needs the rows and the table sizes) ---------------------------
def resample_bounds(in_size, out_size, filt, xx):
    """[first, end) input indices of Pillow's filter for output index xx (precompute_coeffs, in double)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = (1.0 if filt == BILINEAR else 2.0) * fs
    center = (xx + 0.5) * scale
    return max(int(center - support + 0.5), 0), min(int(center + support + 0.5), in_size)


def resample_taps(in_size, out_size, filt):
    """Pillow's ksize = 2 * ceil(support) + 1."""
    fs = max(in_size / out_size, 1.0)
    return int(math.ceil((1.0 if filt == BILINEAR else 2.0) * fs)) * 2 + 1


# ---- packing ------------------------------------------------------------------------------------------------------------------------------
def pack_batch(images, labels, params, S=224, mix=None, seed=0):
    """images: uint8 HWC RGB arrays; params: per-image dicts of train_params / val_params; mix: None or mix_params' tuple.
    -> dict(pix=uint8 [n * 16], desc=int32 [B, DESC_INTS], labels=int64 [B], meta=dict of the host maxima and the erase seed, mixed=bool)
    and, when any image's params carry an "ops" list (RandAugment / ColorJitter), ops=int32 [B, RA_MAX_OPS, RA_OP_INTS]."""
    B = len(images)
    desc = np.zeros((B, DESC_INTS), np.int32)
    sizes = [int(im.size) for im in images]
    offs = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    total = int(-(-int(offs[-1]) // 16) * 16) or 16
    pix = np.zeros(total, np.uint8)
    row_off, max_rows, kmax_h, kmax_v, rowbytes = 0, 1, 1, 1, 32
    for b, (im, p) in enumerate(zip(images, params)):
        H, W, C = im.shape
        assert C == 3 and im.dtype == np.uint8, (im.shape, im.dtype)
        pix[offs[b]:offs[b + 1]] = im.reshape(-1)
        ci, cj, ch, cw = p["crop"]
        gh, gw = p["grid"]
        wy, wx = p["win"]
        assert 0 <= ci and 0 <= cj and 0 < ch and 0 < cw and ci + ch <= H and cj + cw <= W, (p["crop"], H, W)
        assert 0 <= wy and wy + S <= gh and 0 <= wx and wx + S <= gw, (p["win"], p["grid"], S)
        f = p["filt"]
        yfirst = resample_bounds(ch, gh, f, wy)[0]
        yend = resample_bounds(ch, gh, f, wy + S - 1)[1]
        yn = yend - yfirst
        boxes = p["boxes"]
        if len(boxes) > MAX_ERASE:
            raise ValueError(f"at most {MAX_ERASE} erase boxes per image")
        lo = int(offs[b]) & 0xFFFFFFFF
        desc[b, :A_LABEL + 1] = (lo - (1 << 32) if lo >= 1 << 31 else lo, int(offs[b]) >> 32, H, W, ci, cj, ch, cw, gh, gw, wy, wx, f,
                                 int(p["flip"]), yfirst, yn, row_off, p["emode"] if boxes else 0, len(boxes), 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                 int(labels[b]))
        for e, bx in enumerate(boxes):
            desc[b, A_BOXES + 4 * e:A_BOXES + 4 * e + 4] = bx
        row_off += yn
        max_rows = max(max_rows, yn)
        kmax_h = max(kmax_h, resample_taps(cw, gw, f))
        kmax_v = max(kmax_v, resample_taps(ch, gh, f))
        rowbytes = max(rowbytes, (cw * 3 + 32 + 15) // 16 * 16)
    one = np.float32(1)
    fl = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
    if mix is not None:
        mode, pa, pb, box, la, lb = mix
        desc[:, A_MIX], desc[:, A_PIXA], desc[:, A_PIXB] = mode, fl(pa), fl(pb)
        desc[:, A_LABA], desc[:, A_LABB] = fl(la), fl(lb)
        desc[:, A_CY0:A_CX1 + 1] = box
    else:
        desc[:, A_PIXA], desc[:, A_LABA] = fl(np.full(B, one)), fl(np.full(B, one))
    meta = dict(total_rows=row_off, max_rows=max_rows, kmax_h=kmax_h, kmax_v=kmax_v, rowbytes=rowbytes, seed=int(seed), size=S)
    hb = dict(pix=torch.from_numpy(pix), desc=torch.from_numpy(desc), labels=torch.as_tensor(np.asarray(labels, np.int64)),
              meta=meta, mixed=mix is not None)
    if any("ops" in p for p in params):
        hb["ops"] = torch.from_numpy(pack_ops([p.get("ops", []) for p in params]))
    return hb


def decode(path):
    """Pillow open(...).convert('RGB') as a uint8 HWC array (torchvision's pil_loader)."""
    from PIL import Image
    with open(path, "rb") as f:
        img = Image.open(f)
        return np.asarray(img.convert("RGB"))


def _key_seed(*key):
    """A 64-bit seed from a key tuple (numpy SeedSequence)."""
    a, b = np.random.SeedSequence(list(key)).generate_state(2, np.uint32)
    return (int(a) << 32) | int(b)


class BatchSet(torch.utils.data.Dataset):
    """Item b = the packed batch b of an epoch (decode + parameter sampling + packing), so DataLoader workers do the whole host side."""

    def __init__(self, samples, order, batch, train, S=224, opts=None, mix=None, seed=0, epoch=0, rank=0, loader=decode):
        self.samples, self.order, self.batch, self.train, self.S = samples, list(order), int(batch), bool(train), S
        self.opts, self.mix, self.seed, self.epoch, self.rank, self.loader = opts or AugmentOptions(), mix, seed, epoch, rank, loader

    def __len__(self):
        return -(-len(self.order) // self.batch)

    def __getitem__(self, b):
        idx = self.order[b * self.batch:(b + 1) * self.batch]
        images, labels, params = [], [], []
        for p, n in enumerate(idx):
            path, label = self.samples[n]
            im = self.loader(path)
            H, W = im.shape[:2]
            if self.train:
                params.append(train_params(np.random.default_rng([self.seed, self.epoch, self.rank, b * self.batch + p]), H, W, self.opts, self.S))
            else:
                params.append(val_params(H, W, self.S))
            images.append(im)
            labels.append(label)
        mix = None
        if self.train and self.mix is not None:
            mix = mix_params(np.random.default_rng([self.seed, self.epoch, self.rank, b, 0x6D6978]), len(idx), self.mix, self.S)
        return pack_batch(images, labels, params, self.S, mix, _key_seed(self.seed, self.epoch, self.rank, b, 0x6572))


def _identity(x):
    return x


def _worker_context():
    """Workers start from a fork server (a fresh interpreter with torch and this module imported), not by forking the training
    process: after a fork of a process that holds GPU mappings, its own writes to shared pages take copy-on-write faults that stall
    the next training step for seconds (measured: 6 s on the first step of every epoch at B = 128)."""
    import multiprocessing as mp
    ctx = mp.get_context("forkserver")
    ctx.set_forkserver_preload(["torch", "numpy", __name__])
    return ctx


class FolderLoader:
    """Iterates (images fp32 [B, 3, S, S], labels) on `device` like utils.SyntheticLoader: int64 labels, or fp32 [B, classes] soft
    labels when `mix` is set.  With prefetch, batch t+1's host-to-device copy is issued on a side stream before batch t is handed out,
    so it overlaps step t; batch t's kernels run on the consuming stream after an event wait.  The copies are allocated on the side
    stream and record_stream'ed to the consuming stream, which reads them last."""

    def __init__(self, samples, order, batch, device, train=True, S=224, opts=None, mix=None, seed=0, epoch=0, rank=0, num_workers=0,
                 prefetch=True, loader=decode):
        if num_workers > 16:
            raise ValueError("at most 16 loader workers")
        self.set = BatchSet(samples, order, batch, train, S, opts, mix, seed, epoch, rank, loader)
        self.device, self.num_workers, self.prefetch, self.mix, self.S = torch.device(device), int(num_workers), prefetch, mix, S
        self._side = None

    def __len__(self):
        return len(self.set)

    def host_batches(self):
        return torch.utils.data.DataLoader(self.set, batch_size=None, shuffle=False, num_workers=self.num_workers,
                                           pin_memory=self.device.type == "cuda", collate_fn=_identity,
                                           multiprocessing_context=_worker_context() if self.num_workers else None)

    def _upload(self, hb, stream=None):
        with torch.cuda.stream(stream):          # None: the current stream
            dev = {k: hb[k].to(self.device, non_blocking=True) for k in ("pix", "desc", "labels", "ops") if k in hb}
            ev = torch.cuda.Event()
            ev.record()
        return dev, ev, hb

    def _finish(self, up):
        from . import ops
        dev, ev, hb = up
        main = torch.cuda.current_stream(self.device)
        main.wait_event(ev)
        for t in dev.values():
            t.record_stream(main)
        images = ops.augment_images(dev["pix"], dev["desc"], hb["meta"], self.S, dev.get("ops"))
        labels = ops.augment_labels(dev["desc"], self.mix.num_classes, self.mix.smoothing) if hb["mixed"] else dev["labels"]
        return images, labels

    def __iter__(self):
        if not self.prefetch:
            for hb in self.host_batches():
                yield self._finish(self._upload(hb))
            return
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        prev = None
        for hb in self.host_batches():
            up = self._upload(hb, self._side)
            if prev is not None:
                yield self._finish(prev)
            prev = up
        if prev is not None:
            yield self._finish(prev)

