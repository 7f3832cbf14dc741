"""Input-pipeline measurements (csrc/augment.hip, d2s/data.py) on one GPU:

  1. the augment kernels alone (crop-resize + flip + normalize + erase + Mixup, and the soft labels) at B = 128 on ImageNet-like
     sources (about 500 x 375), timed with device events: without RandAugment / ColorJitter (the fused route), with the default
     --aa rand-m9-mstd0.5-inc1 and with --color-jitter 0.4 alone (the three-pass route around csrc/randaug.hip), and the op kernel alone;
  2. the loader's host rate (JPEG decode + parameter sampling + packing) with 8 and 16 workers, on JPEGs generated into a temp dir;
  3. mask_predictor.py --data-source folder images/s next to --data-source synthetic (fresh child processes, same model and batch).

    python tools/augment_bench.py [--batch 128] [--images 1280] [--arch deit_small] [--skip-train] [--kernels-only]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dense2sparse-vit_amd"))


def _imagenet_like(rng):
    H, W = (375, 500) if rng.random() < 0.7 else (500, 375)
    H, W = H + int(rng.integers(-40, 41)), W + int(rng.integers(-40, 41))
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 90 * np.sin(x / (7 + 3 * c) + y / (11 + c)) for c in range(3)], -1)
    return np.clip(base + rng.integers(-30, 31, (H, W, 3)), 0, 255).astype(np.uint8)


def _timed(fn, iters, repeats=5):
    """Median and spread (min, max) of `repeats` event-timed runs of `iters` calls, in ms per call."""
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return dict(median=round(float(np.median(ms)), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def kernels(B, iters=200):
    import torch
    from d2s import data, ops
    res = {}
    for tag, aa, jitter in (("off", "", 0.0), ("randaug", "rand-m9-mstd0.5-inc1", 0.4), ("jitter", "", 0.4)):
        rng = np.random.default_rng(0)
        images = [_imagenet_like(rng) for _ in range(B)]
        opts = data.AugmentOptions("bicubic", 0.25, "pixel", 1, auto_augment=aa, color_jitter=jitter)
        params = [data.train_params(np.random.default_rng([0, k]), im.shape[0], im.shape[1], opts, 224) for k, im in enumerate(images)]
        mp = data.mix_params(rng, B, data.MixConfig(), 224)
        hb = data.pack_batch(images, list(range(B)), params, 224, mp, seed=1)
        pix, desc = hb["pix"].cuda(), hb["desc"].cuda()
        table = hb["ops"].cuda() if "ops" in hb else None

        def step():
            ops.augment_images(pix, desc, hb["meta"], 224, table)
            ops.augment_labels(desc, 1000, 0.1)
        res[f"ms_per_batch_{tag}"] = _timed(step, iters)
        if table is not None:
            u8 = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device="cuda")
            res[f"ms_op_kernel_{tag}"] = _timed(lambda: ops.randaug_apply(u8, table), iters)
            res[f"ops_per_image_{tag}"] = round(float((hb["ops"][:, :, 0] != 0).sum()) / B, 2)
    src = int(sum(im.size for im in images))
    inter = int(hb["meta"]["total_rows"]) * 224 * 3
    out = B * 3 * 224 * 224 * 4
    res.update(batch=B, ms_per_batch=res["ms_per_batch_off"]["median"], src_mb=round(src / 1e6, 1), scratch_mb=round(inter / 1e6, 1),
               out_mb=round(out / 1e6, 1), u8_image_mb=round(B * 224 * 224 * 3 / 1e6, 1),
               bytes_floor_us=round((src + 2 * inter + out + B * 4000) / 8.0e12 * 1e6, 1))        # at the 8 TB/s HBM peak (fused route)
    return res


def make_folder(root, n, rng):
    from PIL import Image
    for c in range(4):
        os.makedirs(os.path.join(root, f"class{c}"), exist_ok=True)
    pool = [_imagenet_like(rng) for _ in range(64)]
    for k in range(n):
        Image.fromarray(pool[k % 64]).save(os.path.join(root, f"class{k % 4}", f"{k:06d}.jpg"), quality=90)


def loader_rate(root, B, workers):
    from d2s import data
    samples, _ = data.image_folder(root)
    ld = data.FolderLoader(samples, list(range(len(samples))), B, "cpu", train=True, opts=data.AugmentOptions(), mix=data.MixConfig(),
                           num_workers=workers)
    it = iter(ld.host_batches())
    next(it)                                           # worker start-up
    t0, n = time.time(), 0
    for hb in it:
        n += hb["desc"].shape[0]
    return round(n / (time.time() - t0), 1)


def train_rate(root, B, arch, source, epochs=2):
    cmd = [sys.executable, os.path.join(REPO, "dense2sparse-vit_amd", "mask_predictor.py"), "--arch", arch, "--pruning-locs", "3",
           "--keep-ratios", "0.5", "--topk-selection", "--epochs", str(epochs), "--warmup-steps", "0", "--batch-size", str(B),
           "--data-source", source]
    if source == "folder":
        cmd += ["--imgnet-val-dir", root, "--num-workers", "16"]
    else:
        n_train = len(os.listdir(os.path.join(root, "class0"))) * 4 * 4 // 5
        cmd += ["--steps-per-epoch", str(-(-n_train // B)), "--val-steps", "1"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError(out.stdout[-2000:] + out.stderr[-2000:])
    rates = [float(m) for m in re.findall(r"([0-9.]+) train images/s", out.stdout)]
    return rates[-1]                                   # the last epoch: warmed up


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--images", type=int, default=1280)
    ap.add_argument("--arch", default="deit_small")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="measurement 1 only")
    a = ap.parse_args()
    res = {"kernels": kernels(a.batch)}
    print(f"[augment] kernels: {res['kernels']}", flush=True)
    if a.kernels_only:
        print(json.dumps(res))
        return
    with tempfile.TemporaryDirectory() as root:
        make_folder(root, a.images, np.random.default_rng(1))
        res["decode_img_s"] = {w: loader_rate(root, a.batch, w) for w in (8, 16)}
        print(f"[augment] loader images/s by workers: {res['decode_img_s']}", flush=True)
        if not a.skip_train:
            res["train_img_s"] = {s: train_rate(root, a.batch, a.arch, s) for s in ("synthetic", "folder")}
            print(f"[augment] mask_predictor train images/s: {res['train_img_s']}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
