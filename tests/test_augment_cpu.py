"""Input pipeline, host side and restatement (no GPU): tests/augment_ref.py against Pillow's outputs, d2s.data's listing / split /
shards / samplers / packing, and the --data-source folder command line."""
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "augment_pil.npz")


def _fixture():
    z = np.load(FIXTURE)
    return z, [z[f"src{k}"] for k in range(5)]


def test_restatement_matches_pillow_fixture():
    z, srcs = _fixture()
    for n, (k, i, j, h, w, S, f) in enumerate(z["cases"]):
        got = R.crop_resize(srcs[k], (i, j, h, w), (S, S), (0, 0), f, S)
        assert np.array_equal(got, z[f"out{n}"]), n
    from d2s import data
    src = srcs[int(z["val_src"][0])]
    p = data.val_params(*src.shape[:2])
    assert np.array_equal(R.crop_resize(src, p["crop"], p["grid"], p["win"], p["filt"], 224), z["val_out"])


def test_restatement_matches_live_pillow():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(5)
    for _ in range(60):
        H, W = (int(v) for v in rng.integers(1, 90, 2))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        crop = (int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w)
        S, f = int(rng.integers(1, 70)), int(rng.integers(0, 2))
        assert np.array_equal(R.crop_resize(img, crop, (S, S), (0, 0), f, S), R.pil_crop_resize(img, crop, S, f)), (H, W, crop, S, f)
    from d2s import data
    for H, W in ((300, 257), (256, 256), (241, 391), (400, 299)):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        p = data.val_params(H, W)
        assert np.array_equal(R.crop_resize(img, p["crop"], p["grid"], p["win"], p["filt"], 224), R.pil_val(img))


# ---- torch restatement of timm 0.4.12's Mixup.__call__ and mixup_target (the tensor ops as timm writes them) ------------------------
def _timm_one_hot(x, C, on, off):
    return torch.full((x.size()[0], C), off).scatter_(1, x.long().view(-1, 1), on)


def _timm_mixup_target(target, C, lam, smoothing):
    off = smoothing / C
    on = 1. - smoothing + off
    y1 = _timm_one_hot(target, C, on, off)
    y2 = _timm_one_hot(target.flip(0), C, on, off)
    return y1 * lam + y2 * (1. - lam)


def _timm_mixup(x, target, rng, cfg):
    """timm Mixup.__call__ with its parameter draws taken from d2s.data's restated samplers on `rng`."""
    from d2s import data
    S = x.shape[-1]
    B = len(x)
    if cfg.mode == "batch":
        lam, use_cutmix = data._params_per_batch(rng, cfg)
        if lam != 1.:
            if use_cutmix:
                (yl, yh, xl, xh), lam = data.cutmix_bbox_and_lam(rng, S, lam, cfg.cutmix_minmax)
                x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
            else:
                x_flipped = x.flip(0).mul_(1. - lam)
                x.mul_(lam).add_(x_flipped)
    else:
        pair = cfg.mode == "pair"
        lam_batch, use_cutmix = data._params_per_elem(rng, B // 2 if pair else B, cfg)
        x_orig = x.clone()
        for i in range(B // 2 if pair else B):
            j = B - i - 1
            lam = lam_batch[i]
            if lam != 1.:
                if use_cutmix[i]:
                    (yl, yh, xl, xh), lam = data.cutmix_bbox_and_lam(rng, S, lam, cfg.cutmix_minmax)
                    x[i][:, yl:yh, xl:xh] = x_orig[j][:, yl:yh, xl:xh]
                    if pair:
                        x[j][:, yl:yh, xl:xh] = x_orig[i][:, yl:yh, xl:xh]
                    lam_batch[i] = lam
                else:
                    x[i] = x[i] * lam + x_orig[j] * (1 - lam)
                    if pair:
                        x[j] = x[j] * lam + x_orig[i] * (1 - lam)
        if pair:
            lam_batch = np.concatenate((lam_batch, lam_batch[::-1]))
        lam = torch.tensor(lam_batch, dtype=x.dtype).unsqueeze(1)
    return x, _timm_mixup_target(target, cfg.num_classes, lam, cfg.smoothing)


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
@pytest.mark.parametrize("alphas", [(0.8, 1.0), (0.8, 0.0), (1.0, 1.0, (0.2, 0.7))])
def test_restated_blend_matches_timm_mixup(mode, alphas):
    from d2s import data
    S, B, C = 20, 8, 13
    cfg = data.MixConfig(alphas[0], alphas[1], alphas[2] if len(alphas) > 2 else None, 1.0, 0.5, mode, 0.1, C)
    for seed in range(12):
        rng = np.random.default_rng(seed)
        u8 = rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
        labels = rng.integers(0, C, B)
        # ToTensor + Normalize as torchvision / timm compute them, with a const and a pixel-mode erase box on two samples
        xt = torch.stack([torch.from_numpy(u).permute(2, 0, 1).float().div(255) for u in u8])
        xt = xt.sub_(torch.tensor(R.MEAN)[:, None, None]).div_(torch.tensor(R.STD)[:, None, None])
        xn = np.stack([R.normalize(u) for u in u8])
        assert np.array_equal(xt.numpy(), xn)
        xn[1, :, 2:7, 3:9] = 0.
        xt[1, :, 2:7, 3:9] = 0.
        R.erase(xn[2], [(4, 1, 6, 5)], 3, 99, 2)
        xt[2] = torch.from_numpy(xn[2].copy())
        want_x, want_y = _timm_mixup(xt.clone(), torch.from_numpy(labels), np.random.default_rng(1000 + seed), cfg)
        mp = data.mix_params(np.random.default_rng(1000 + seed), B, cfg, S)
        got_x = R.mix(xn, mp)
        got_y = R.soft_labels(labels, mp[4], mp[5], C, cfg.smoothing)
        assert np.array_equal(got_x, want_x.numpy()), (mode, seed)
        assert np.array_equal(got_y, want_y.numpy()), (mode, seed)


def test_odd_batch_pairs_the_middle_sample_with_itself():
    from d2s import data
    for mode in ("batch", "pair", "elem"):
        cfg = data.MixConfig(0.8, 0.0, None, 1.0, 0.5, mode, 0.1, 10)
        mode_, pa, pb, box, la, lb = data.mix_params(np.random.default_rng(3), 7, cfg, 16)
        assert len(la) == 7 and len(mode_) == 7
        if mode == "pair":
            assert mode_[3] == 0 and la[3] == 1 and lb[3] == 0
            assert np.array_equal(la[:3], la[4:][::-1])


def test_samplers_stay_in_bounds_and_take_the_fallbacks():
    from d2s import data
    rng = np.random.default_rng(0)
    for _ in range(2000):
        H, W = (int(v) for v in rng.integers(1, 600, 2))
        i, j, h, w = data.rrc_params(rng, H, W)
        assert 0 < h <= H and 0 < w <= W and 0 <= i <= H - h and 0 <= j <= W - w
    # scale that can never fit: the centre-crop fallback for all three aspect branches
    assert data.rrc_params(rng, 100, 300, scale=(5, 6)) == (0, (300 - 133) // 2, 100, 133)
    assert data.rrc_params(rng, 300, 100, scale=(5, 6)) == ((300 - 133) // 2, 0, 133, 100)
    assert data.rrc_params(rng, 100, 110, scale=(5, 6)) == (0, 0, 100, 110)
    assert data.rrc_params(rng, 1, 1) == (0, 0, 1, 1)
    n_boxes = 0
    for _ in range(2000):
        boxes = data.erase_params(rng, 0.5, 3, 224)
        assert len(boxes) <= 3
        n_boxes += bool(boxes)
        for t, l, h, w in boxes:
            assert 0 < h < 224 and 0 < w < 224 and 0 <= t <= 224 - h and 0 <= l <= 224 - w
    assert 800 < n_boxes < 1200
    assert data.erase_params(rng, 0.0, 1, 224) == [] and data.erase_params(rng, 1.0, 1, 4, min_area=2, max_area=3) == []   # no fit
    for mode in ("batch", "pair", "elem"):
        for alphas in ((0.8, 1.0, None), (0.0, 1.0, None), (0.8, 0.0, None), (1.0, 1.0, (0.1, 0.9))):
            cfg = data.MixConfig(*alphas, prob=0.7, mode=mode, num_classes=5)
            for s in range(30):
                m, pa, pb, box, la, lb = data.mix_params(np.random.default_rng(s), 6, cfg, 32)
                assert np.all((la >= 0) & (la <= 1)) and np.all(np.abs(la + lb - 1) < 1e-6)
                assert np.all((box[:, 0] <= box[:, 1]) & (box[:, 2] <= box[:, 3])) and np.all((box >= 0) & (box <= 32))
                assert np.all(m[(la == 1) & (pa == 1)] != 1)


def _tree(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    names = {"b_cls": ["x.JPG", "a.png", "skip.txt", "sub/z.jpeg", "c.Webp"], "a_cls": ["2.bmp", "1.jpg"], "c_empty": []}
    for cls, files in names.items():
        (tmp_path / cls).mkdir()
        for f in files:
            p = tmp_path / cls / f
            p.parent.mkdir(exist_ok=True)
            if f.endswith(".txt"):
                p.write_text("no image")
                continue
            H, W = (int(v) for v in rng.integers(20, 60, 2))
            fmt = {"jpg": "JPEG", "jpeg": "JPEG", "png": "PNG", "webp": "WEBP", "bmp": "BMP"}[f.rsplit(".", 1)[1].lower()]
            Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(p, format=fmt)
    return tmp_path


def test_image_folder_order_and_extensions(tmp_path):
    pytest.importorskip("PIL")
    from d2s import data
    root = _tree(tmp_path)
    samples, classes = data.image_folder(str(root))
    assert classes == ["a_cls", "b_cls", "c_empty"]
    rel = [(os.path.relpath(p, root), c) for p, c in samples]
    assert rel == [("a_cls/1.jpg", 0), ("a_cls/2.bmp", 0), ("b_cls/a.png", 1), ("b_cls/c.Webp", 1), ("b_cls/x.JPG", 1),
                   ("b_cls/sub/z.jpeg", 1)]
    im = data.decode(samples[0][0])
    assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3


def test_split_is_the_references_seeded_shuffle():
    from d2s import data
    for n in (1, 7, 10, 1234):
        idx = list(range(n))
        rs = np.random.RandomState(42)
        rs.shuffle(idx)
        k = int(np.floor(0.2 * n))
        assert data.split_indices(n) == (idx[k:], idx[:k])
    np.random.seed(42)                                      # the reference's global seeding (mask_predictor.py:43-45) then shuffle
    ref = list(range(500))
    np.random.shuffle(ref)
    assert data.split_indices(500)[1] == ref[:100]


def test_ddp_shards_are_disjoint_and_cover_the_set():
    from d2s import data
    for n, world in ((12, 4), (10, 4), (7, 3), (5, 8)):
        idx = list(range(100, 100 + n))
        shards = [data.shard(idx, r, world) for r in range(world)]
        assert len({len(s) for s in shards}) == 1                               # equal step counts on every rank
        allv = [v for s in shards for v in s]
        assert set(allv) == set(idx)
        assert len(allv) - len(set(allv)) == (-n) % world                      # only DistributedSampler's padding repeats
        if n % world == 0:
            assert len(allv) == len(set(allv))


def test_packed_batches_do_not_depend_on_workers(tmp_path):
    pytest.importorskip("PIL")
    from d2s import data
    samples, _ = data.image_folder(str(_tree(tmp_path)))
    mix = data.MixConfig(mode="elem", num_classes=10)
    opts = data.AugmentOptions("random", 0.7, "pixel", 3)

    def batches(workers):
        ld = data.FolderLoader(samples, list(range(len(samples))), 4, "cpu", train=True, opts=opts, mix=mix, seed=3, epoch=1,
                               num_workers=workers)
        return list(ld.host_batches())

    a, b = batches(0), batches(2)
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        for k in ("pix", "desc", "labels"):
            assert torch.equal(x[k], y[k]), k
        assert x["meta"] == y["meta"] and x["mixed"] and y["mixed"]
    assert a[1]["desc"].shape == (2, data.DESC_INTS)


def test_pack_batch_descriptor():
    from d2s import data
    rng = np.random.default_rng(0)
    ims = [rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), rng.integers(0, 256, (300, 400, 3), dtype=np.uint8)]
    params = [data.train_params(rng, 5, 7, data.AugmentOptions(reprob=1.0), 224), data.val_params(300, 400)]
    hb = data.pack_batch(ims, [3, 4], params, 224, None, seed=7)
    d = hb["desc"].numpy()
    assert hb["pix"].numel() % 16 == 0 and hb["pix"].numel() >= 5 * 7 * 3 + 300 * 400 * 3
    assert d[1, data.A_OFF_LO] == 105 and tuple(d[1, data.A_H:data.A_W + 1]) == (300, 400)
    assert tuple(d[1, data.A_GH:data.A_WX + 1]) == (256, 341, 16, 58)
    assert d[1, data.A_ROWOFF] == d[0, data.A_YN] and hb["meta"]["total_rows"] == d[:, data.A_YN].sum()
    assert d[0, data.A_ECOUNT] == 1 and d[0, data.A_EMODE] == 3 and list(d[:, data.A_LABEL]) == [3, 4]


def test_cli_folder_source():
    import mask_predictor
    import utils
    a = utils.parse_args([])
    assert a.data_source == "synthetic" and a.num_workers == 8
    mask_predictor.check_supported(a)
    assert a.mixup == 0.0 and a.cutmix == 0.0 and a.cutmix_minmax is None
    a = utils.parse_args(["--data-source", "folder", "--imgnet-val-dir", "/data"])
    mask_predictor.check_supported(a)
    assert a.mixup == 0.8 and a.cutmix == 1.0                                   # kept on folder data
    for extra, msg in ((["--train-interpolation", "lanczos"], "train-interpolation"), (["--mixup", "0"], "--cutmix without"),
                       (["--mixup", "0", "--cutmix", "0", "--cutmix-minmax", "0.2", "0.8"], "--cutmix without"),
                       (["--num-workers", "17"], "num-workers"), (["--mixup-mode", "row"], "mixup-mode")):
        with pytest.raises(SystemExit, match=msg):
            mask_predictor.check_supported(utils.parse_args(["--data-source", "folder", "--imgnet-val-dir", "/data"] + extra))
    with pytest.raises(SystemExit, match="imgnet-val-dir"):
        mask_predictor.check_supported(utils.parse_args(["--data-source", "folder"]))
    a = utils.parse_args(["--data-source", "folder", "--imgnet-val-dir", "/data", "--mixup", "0", "--cutmix", "0"])
    mask_predictor.check_supported(a)
    assert a.mixup == 0 and a.cutmix == 0
