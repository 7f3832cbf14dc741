"""GPU tier of RandAugment / ColorJitter (csrc/randaug.hip through d2s.ops / d2s.data): the op kernel against Pillow's committed outputs
and the numpy restatement (tests/randaug_ref.py), bit for bit; the three-pass input pipeline against the existing stages of
tests/augment_ref.py composed with the restatement; and mask_predictor --data-source folder with the default --aa."""
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as A
from tests import randaug_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "randaug_pil.npz")
DEV = "cuda:0"


def _apply(images, op_lists):
    from d2s import data, ops
    table = torch.from_numpy(data.pack_ops(op_lists)).to(DEV)
    out = ops.randaug_apply(torch.from_numpy(np.stack(images)).to(DEV), table)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_op_kernel_matches_the_pillow_fixture_and_the_restatement():
    """Every op singly (both filters for the geometric ones), the composed lists and the ColorJitter orders, in batches of B = 3 images
    of 16 x 16 (the 16-byte path) and 19 x 19 (odd row bytes: the per-pixel path)."""
    cases = R.load_fixture(FIXTURE)
    for S in (16, 19):
        sub = [c for c in cases if c[0].shape[0] == S]
        for k in range(0, len(sub) - 2, 3):
            batch = sub[k:k + 3] if k + 3 <= len(sub) else sub[-3:]
            got = _apply([c[0] for c in batch], [c[1] for c in batch])
            for b, (img, ops, want, steps) in enumerate(batch):
                assert np.array_equal(got[b], want), (S, steps)
                assert np.array_equal(got[b], R.apply_ops(img, ops)), (S, steps)
        last = sub[-3:]
        got = _apply([c[0] for c in last], [c[1] for c in last])
        assert all(np.array_equal(got[b], c[2]) for b, c in enumerate(last))


def _smooth_image(rng, S):
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / (7 + 3 * c) + y / (11 + c)) for c in range(3)], -1) + rng.integers(-20, 21, (S, S, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("S", [224, 384])
def test_full_size_images(S):
    """One image at 224 (147 KiB, the size that would just fit one workgroup's LDS) and one at 384 (beyond it): both full lists of 8 ops
    with every op class, a repeated op, an empty list; two runs give the same bytes."""
    rng = np.random.default_rng(S)
    img = _smooth_image(rng, S)
    n = R.named_op
    lists = [[n("Equalize", 0, 0, S), n("Rotate", 0.78, False, S, R.BICUBIC), n("SharpnessIncreasing", 0.9, False, S), n("AutoContrast", 0, 0, S),
              n("ShearX", 0.9, True, S, R.BILINEAR), n("ContrastIncreasing", 0.6, True, S), n("ColorIncreasing", 0.9, False, S),
              n("SolarizeIncreasing", 0.4, False, S)],
             [n("Invert", 0, 0, S), n("PosterizeIncreasing", 0.6, False, S), n("SolarizeAdd", 0.9, False, S), n("BrightnessIncreasing", 0.5, True, S),
              n("TranslateXRel", 0.7, True, S, R.BICUBIC), n("TranslateYRel", 0.3, False, S, R.BILINEAR), n("Invert", 0, 0, S),
              n("Rotate", 1.0, True, S, R.BILINEAR)],
             [], [n("SharpnessIncreasing", 1.0, True, S)] * 2 + [n("ShearY", 0.5, False, S, R.BICUBIC)] * 2]
    outs = []
    for ops in lists:
        got = _apply([img], [ops])
        assert np.array_equal(got[0], R.apply_ops(img, ops)), [op[0] for op in ops]
        outs.append(got[0])
    assert np.array_equal(outs[2], img)                                       # an empty list copies
    again = _apply([img], [lists[0]])
    assert np.array_equal(again[0], outs[0])


def test_batch_of_mixed_lists_and_empty_lists():
    """B = 3 with lists of different lengths, one of them empty: images are independent, and an empty list returns its input."""
    rng = np.random.default_rng(3)
    for S in (16, 19):
        imgs = [rng.integers(0, 256, (S, S, 3), dtype=np.uint8) for _ in range(3)]
        n = R.named_op
        lists = [[n("Rotate", 0.5, True, S, R.BILINEAR), n("Rotate", 0.5, True, S, R.BILINEAR), n("Equalize", 0, 0, S)], [],
                 [n("ContrastIncreasing", 1.0, True, S)]]
        got = _apply(imgs, lists)
        for b in range(3):
            assert np.array_equal(got[b], R.apply_ops(imgs[b], lists[b])), (S, b)
        assert np.array_equal(got[1], imgs[1])
        assert np.array_equal(_apply(imgs, lists), got)
        # degenerate histograms: a constant image under AutoContrast / Equalize stays as it is
        const = [np.full((S, S, 3), 77, np.uint8)] * 3
        got = _apply(const, [[n("AutoContrast", 0, 0, S)], [n("Equalize", 0, 0, S)], [n("Equalize", 0, 0, S), n("AutoContrast", 0, 0, S)]])
        assert all(np.array_equal(g, const[0]) for g in got)


def _pipeline_batch(opts, S):
    from d2s import data
    rng = np.random.default_rng(7)
    sizes = [(61, 83), (90, 120), (120, 75), (48, 48)]
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in sizes]
    params = [data.train_params(np.random.default_rng([1, 0, 0, k]), H, W, opts, S) for k, (H, W) in enumerate(sizes)]
    return images, [3, 1, 4, 1], params


def _run(images, labels, params, S, mix, seed, table="packed"):
    from d2s import data, ops
    hb = data.pack_batch(images, labels, params, S, mix, seed)
    t = hb["ops"].to(DEV) if table == "packed" else table
    x = ops.augment_images(hb["pix"].to(DEV), hb["desc"].to(DEV), hb["meta"], S, t)
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("aa,jitter", [("rand-m9-mstd0.5-n3-p0.9-inc1", 0.4), ("", 0.4)])
def test_pipeline_matches_the_composed_restatement(aa, jitter):
    """crop, flip, ops, normalise, erase, mix on a packed batch of 4 sources: the existing stages of tests/augment_ref.py with the new
    restatement between the flip and the normalisation.  Erasing is 'const' here: the random erase values go through the device's log
    and cos (tests/test_augment_gpu.py bounds those), everything else is bit for bit."""
    from d2s import data
    S, seed = 48, 99
    opts = data.AugmentOptions("random", 1.0, "const", 2, auto_augment=aa, color_jitter=jitter)
    images, labels, params = _pipeline_batch(opts, S)
    assert all("ops" in p for p in params) and sum(len(p["ops"]) for p in params) >= 6 and any(p["boxes"] for p in params)
    mp = data.mix_params(np.random.default_rng(2), 4, data.MixConfig(mode="elem", num_classes=10), S)
    xs = []
    for b, (im, p) in enumerate(zip(images, params)):
        u = A.crop_resize(im, p["crop"], p["grid"], p["win"], p["filt"], S)
        if p["flip"]:
            u = u[:, ::-1]
        u = R.apply_ops(np.ascontiguousarray(u), p["ops"])
        v = A.normalize(u)
        if p["boxes"]:
            A.erase(v, p["boxes"], p["emode"], seed, b)
        xs.append(v)
    want = A.mix(np.stack(xs), mp)
    got = _run(images, labels, params, S, mp, seed).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(_run(images, labels, params, S, mp, seed).cpu().numpy(), got)


def test_three_pass_route_with_empty_lists_equals_the_fused_route():
    from d2s import data, ops
    S, seed = 48, 5
    opts = data.AugmentOptions("random", 1.0, "pixel", 2, auto_augment="none", color_jitter=0.0)
    images, labels, params = _pipeline_batch(opts, S)
    assert not any("ops" in p for p in params)
    for B in (4, 3):                                                          # an odd batch: the middle sample pairs with itself
        mp = data.mix_params(np.random.default_rng(2), B, data.MixConfig(mode="elem", num_classes=10), S)
        fused = _run(images[:B], labels[:B], params[:B], S, mp, seed, table=None)
        empty = torch.zeros((B, ops.RA_MAX_OPS, ops.RA_OP_INTS), dtype=torch.int32, device=DEV)
        assert torch.equal(_run(images[:B], labels[:B], params[:B], S, mp, seed, table=empty), fused)


def test_mask_predictor_two_steps_with_the_default_aa(tmp_path, capsys, monkeypatch):
    pytest.importorskip("PIL")
    from PIL import Image
    from d2s import ops
    import mask_predictor
    rng = np.random.default_rng(0)
    for c in ("cat", "dog"):
        (tmp_path / c).mkdir()
        for k in range(10):
            H, W = (int(v) for v in rng.integers(180, 300, 2))
            Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(tmp_path / c / f"{k}.jpg", quality=90)
    losses, tables = [], []
    orig_step, orig_aug = mask_predictor.train_one_epoch, ops.augment_images

    def spy_epoch(*a, **k):
        m = orig_step(*a, **k)
        losses.append(m["train_loss"])
        return m

    def spy_aug(pix, desc, meta, size, op_table=None):
        tables.append(None if op_table is None else op_table.cpu().numpy())
        return orig_aug(pix, desc, meta, size, op_table)
    monkeypatch.setattr(mask_predictor, "train_one_epoch", spy_epoch)
    monkeypatch.setattr(ops, "augment_images", spy_aug)
    mask_predictor.main(["--arch", "deit_tiny", "--pruning-locs", "3", "--keep-ratios", "0.5", "--epochs", "1", "--warmup-steps", "1",
                         "--batch-size", "8", "--topk-selection", "--data-source", "folder", "--imgnet-val-dir", str(tmp_path),
                         "--num-workers", "0"])
    out = capsys.readouterr().out
    assert "20 images in 2 classes: 16 train / 4 val" in out and "Attention: --aa" not in out
    assert len(losses) == 1 and np.isfinite(losses[0])
    train = [t for t in tables if t is not None]
    assert len(train) == 2 and all(t.shape == (8, ops.RA_MAX_OPS, ops.RA_OP_INTS) for t in train)      # two training steps of 8 images
    assert sum(int((t[:, :, 0] != 0).sum()) for t in train) > 0 and len(tables) > len(train)            # validation has no table
