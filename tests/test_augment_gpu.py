"""GPU tier of the input pipeline (csrc/augment.hip through d2s.ops / d2s.data): the kernels against the committed Pillow outputs and
the numpy restatement (tests/augment_ref.py), the soft labels, the prefetching loader, and mask_predictor --data-source folder."""
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _run(images, labels, params, S, mix=None, seed=0, num_classes=1000, smoothing=0.1):
    from d2s import data, ops
    hb = data.pack_batch(images, labels, params, S, mix, seed)
    pix, desc = hb["pix"].to(DEV), hb["desc"].to(DEV)
    x = ops.augment_images(pix, desc, hb["meta"], S)
    y = ops.augment_labels(desc, num_classes, smoothing) if mix is not None else None
    torch.cuda.synchronize()
    return x.cpu().numpy(), (None if y is None else y.cpu().numpy())


def _plain(crop, S, f):
    return dict(crop=crop, grid=(S, S), win=(0, 0), filt=f, flip=False, emode=0, boxes=[])


def test_kernel_matches_pillow_fixture():
    from d2s import data
    z = np.load(os.path.join(REPO, "tests", "golden", "augment_pil.npz"))
    srcs = [z[f"src{k}"] for k in range(5)]
    for n, (k, i, j, h, w, S, f) in enumerate(z["cases"]):
        x, _ = _run([srcs[k]], [0], [_plain((i, j, h, w), int(S), int(f))], int(S))
        assert np.array_equal(x[0], R.normalize(z[f"out{n}"])), n
    src = srcs[int(z["val_src"][0])]
    x, _ = _run([src], [0], [data.val_params(*src.shape[:2])], 224)
    assert np.array_equal(x[0], R.normalize(z["val_out"]))


def _random_batch(rng, B):
    """B sources from 1x1 to 3000x2000 with training crops (incl. 1x1 and full-image crops), validation transforms, flips and
    const / rand / pixel erasing."""
    from d2s import data
    sizes = [(1, 1), (2000, 3000), (3000, 2000), (1, 9), (375, 500), (500, 375)] + \
        [tuple(int(v) for v in rng.integers(1, 700, 2)) for _ in range(B - 6)]
    images, params, labels = [], [], []
    for b, (H, W) in enumerate(sizes[:B]):
        im = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        kind = b % 4
        if kind == 3:
            p = data.val_params(H, W)
        else:
            opts = data.AugmentOptions("random", 1.0 if kind else 0.5, ("const", "pixel", "rand")[b % 3], 1 + b % 3)
            p = data.train_params(rng, H, W, opts, 224)
            if b == 5:
                p["crop"] = (int(rng.integers(0, H)), int(rng.integers(0, W)), 1, 1)            # a 1x1 crop of a larger image
        images.append(im)
        params.append(p)
        labels.append(int(rng.integers(0, 1000)))
    return images, labels, params


def _erase_mask(params, S):
    m = np.zeros((len(params), S, S), bool)
    for b, p in enumerate(params):
        if p["emode"] in (2, 3):
            for t, l, h, w in p["boxes"]:
                m[b, t:t + h, l:l + w] = True
    return m


@pytest.mark.parametrize("B", [37, 36])
def test_kernel_matches_restatement_on_a_ragged_batch(B):
    from d2s import data
    rng = np.random.default_rng(B)
    images, labels, params = _random_batch(rng, B)
    assert any(p["flip"] for p in params) and {p["emode"] for p in params} >= {0, 1, 2, 3}
    seed = 0x1234567890ABCDEF
    base, _ = R.augment_batch(images, labels, params, 224, None, seed)
    emask = _erase_mask(params, 224)
    touched = emask | emask[::-1]                          # a value from the erase RNG may reach the partner through the blend
    x, _ = _run(images, labels, params, 224, None, seed)
    m = np.broadcast_to(emask[:, None], base.shape)
    assert np.array_equal(x[~m], base[~m])
    assert np.abs(x[m] - base[m]).max(initial=0) <= 1e-6
    for mode in ("batch", "pair", "elem"):
        for alphas in ((0.8, 1.0, None), (0.8, 0.0, None), (0.0, 1.0, None)):
            cfg = data.MixConfig(*alphas, mode=mode, num_classes=1000, smoothing=0.1)
            mp = data.mix_params(np.random.default_rng(len(mode)), B, cfg, 224)
            x, y = _run(images, labels, params, 224, mp, seed)
            want = R.mix(base, mp)
            m = np.broadcast_to(touched[:, None], want.shape)
            assert np.array_equal(x[~m], want[~m]), (mode, alphas)
            assert np.abs(x[m] - want[m]).max(initial=0) <= 1e-6, (mode, alphas)
            assert np.array_equal(y, R.soft_labels(labels, mp[4], mp[5], 1000, 0.1)), (mode, alphas)
            assert np.abs(y.sum(1) - 1).max() <= 1e-6


def test_soft_labels_bit_exact():
    from d2s import data, ops
    rng = np.random.default_rng(1)
    for B, C, mode in ((7, 10, "pair"), (128, 1000, "batch"), (33, 1000, "elem")):
        cfg = data.MixConfig(mode=mode, num_classes=C, smoothing=0.1)
        labels = rng.integers(0, C, B)
        mp = data.mix_params(rng, B, cfg, 224)
        hb = data.pack_batch([np.zeros((1, 1, 3), np.uint8)] * B, labels, [_plain((0, 0, 1, 1), 224, 0)] * B, 224, mp)
        y = ops.augment_labels(hb["desc"].to(DEV), C, 0.1).cpu().numpy()
        assert np.array_equal(y, R.soft_labels(labels, mp[4], mp[5], C, 0.1))
        assert np.abs(y.sum(1) - 1).max() <= 1e-6


def test_prefetched_batches_equal_synchronous_ones():
    from d2s import data
    rng = np.random.default_rng(2)
    arrays = {f"im{k}": rng.integers(0, 256, tuple(int(v) for v in rng.integers(40, 400, 2)) + (3,), dtype=np.uint8) for k in range(37)}
    samples = [(f"im{k}", k % 5) for k in range(37)]
    kw = dict(train=True, opts=data.AugmentOptions("random", 0.5, "pixel", 2), mix=data.MixConfig(mode="elem", num_classes=1000),
              seed=11, epoch=2, loader=arrays.__getitem__)
    sync = list(data.FolderLoader(samples, list(range(37)), 8, DEV, prefetch=False, **kw))
    pre = list(data.FolderLoader(samples, list(range(37)), 8, DEV, prefetch=True, **kw))
    assert len(sync) == len(pre) == 5 and pre[-1][0].shape == (5, 3, 224, 224)
    for (xa, ya), (xb, yb) in zip(sync, pre):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
        assert ya.shape[1] == 1000 and ya.dtype == torch.float32
    val = list(data.FolderLoader(samples, list(range(37)), 16, DEV, train=False, loader=arrays.__getitem__))
    assert val[0][1].dtype == torch.int64 and val[-1][0].shape == (5, 3, 224, 224)


def test_mask_predictor_trains_from_an_image_folder(tmp_path, capsys, monkeypatch):
    pytest.importorskip("PIL")
    from PIL import Image
    import mask_predictor
    rng = np.random.default_rng(0)
    for c in ("cat", "dog"):
        (tmp_path / c).mkdir()
        for k in range(12):
            H, W = (int(v) for v in rng.integers(180, 420, 2))
            Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(tmp_path / c / f"{k}.jpg", quality=90)
    seen = []
    orig = mask_predictor.train_one_epoch

    def spy(args, student, teacher, loader, optim, mixup_fn=None):
        from losses import BackboneLoss
        assert args.mixup > 0 and BackboneLoss(args).soft_targets           # soft-target cross entropy on the loader's labels

        class Spy:
            def __iter__(self):
                for x, y in loader:
                    seen.append((tuple(x.shape), tuple(y.shape), y.dtype))
                    yield x, y

            def __len__(self):
                return len(loader)
        m = orig(args, student, teacher, Spy(), optim, mixup_fn)
        assert np.isfinite(m["train_loss"])
        return m
    monkeypatch.setattr(mask_predictor, "train_one_epoch", spy)
    best = mask_predictor.main(["--arch", "deit_tiny", "--pruning-locs", "3", "--keep-ratios", "0.5", "--epochs", "2", "--warmup-steps", "1",
                                "--batch-size", "8", "--topk-selection", "--data-source", "folder", "--imgnet-val-dir", str(tmp_path),
                                "--num-workers", "2"])
    out = capsys.readouterr().out
    assert 0.0 <= best <= 1.0 and "Epoch 2/2" in out and "train images/s" in out
    assert "24 images in 2 classes: 20 train / 4 val" in out
    assert seen == [((8, 3, 224, 224), (8, 1000), torch.float32), ((8, 3, 224, 224), (8, 1000), torch.float32),
                    ((4, 3, 224, 224), (4, 1000), torch.float32)] * 2
