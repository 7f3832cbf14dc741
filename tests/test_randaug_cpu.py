"""RandAugment / ColorJitter, host side and restatement (no GPU): tests/randaug_ref.py against Pillow's committed outputs and, where
Pillow is importable, against live Pillow; d2s.data's config parser, refusals, per-image draws and op table."""
import os

import numpy as np
import pytest

from tests import randaug_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "randaug_pil.npz")
DEFAULT = dict(m=9.0, mstd=0.5, n=2, p=0.5, mmax=10.0)


def test_restatement_equals_the_pillow_fixture():
    cases = R.load_fixture(FIXTURE)
    assert len(cases) == 100 and {c[0].shape[0] for c in cases} == {16, 19}
    seen = set()
    for img, ops, want, steps in cases:
        assert np.array_equal(R.apply_ops(img, ops), want), steps
        seen |= {(op[0], op[1]) for op in ops}
    assert {c for c, _ in seen} == set(range(1, 12)) and {(R.OP_AFFINE, 0), (R.OP_AFFINE, 1)} <= seen


def test_restatement_equals_live_pillow():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(5)
    for trial in range(8):
        S = (16, 19, 33, 17)[trial % 4]
        img = [rng.integers(0, 256, (S, S, 3), dtype=np.uint8), rng.integers(100, 120, (S, S, 3), dtype=np.uint8),
               np.full((S, S, 3), int(rng.integers(0, 256)), np.uint8),                       # constant: AutoContrast / Equalize identity
               (rng.integers(0, 2, (S, S, 3)) * 255).astype(np.uint8)][trial % 4]
        for name in R.RAND_OPS:
            # level 0 (rotate by 0 copies, factor 1), posterize to 0 bits and a factor clipped to 0.1 at t = 1, and a random level
            for t in (0.0, 1.0, float(rng.uniform(0, 1))):
                for neg in (False, True):
                    for res in (R.BILINEAR, R.BICUBIC):
                        op = R.named_op(name, t, neg, S, res)
                        got = img if op is None else R.apply_op(img, op)
                        assert np.array_equal(got, R.pil_named(img, name, t, neg, res)), (trial, name, t, neg, res)
        for code in (R.OP_BRIGHTNESS, R.OP_CONTRAST, R.OP_COLOR):                             # ColorJitter's range, 0 included
            for f in (0.0, 0.6, 1.0, 1.4, float(rng.uniform(0.6, 1.4))):
                assert np.array_equal(R.apply_op(img, R.mk(code, farg=f)), R.pil_enhance(img, code, f)), (trial, code, f)
    assert R.named_op("PosterizeIncreasing", 1.0, False, 16)[2] == 0 and R.named_op("ColorIncreasing", 1.0, True, 16)[3] == np.float32(0.1)
    assert R.named_op("Rotate", 0.0, True, 16) is None


def test_config_parsing():
    from d2s import data
    assert data.parse_auto_augment("rand-m9-mstd0.5-inc1") == DEFAULT
    assert data.parse_auto_augment("rand-m7-n3-p0.25-mmax8-inc1") == dict(m=7.0, mstd=0.0, n=3, p=0.25, mmax=8.0)
    assert data.parse_auto_augment("RAND-M9-MSTD0.5-INC1") == DEFAULT
    for off in ("", "none", "None", None):
        assert data.parse_auto_augment(off) is None


@pytest.mark.parametrize("text", ["rand-m9-mstd0.5", "rand-m9-inc0", "rand-m9-w0-inc1", "augmix-m5-w4-d2", "original", "v0", "3a",
                                  "rand-m9-inc1-n9", "rand-mx-inc1", "rand-m9-q2-inc1", "rand-m9-p1.5-inc1"])
def test_refusals(text):
    from d2s import data
    import mask_predictor
    import utils
    with pytest.raises(ValueError, match="auto-augment policy"):
        data.parse_auto_augment(text)
    with pytest.raises(SystemExit, match="not on the accelerated path") as e:
        mask_predictor.check_supported(utils.parse_args(["--data-source", "folder", "--imgnet-val-dir", "x", "--mixup", "0.8", "--aa", text]))
    assert "--aa" in str(e.value)


def test_check_supported_accepts_the_recipe_without_a_notice(capsys):
    import mask_predictor
    import utils
    for extra in ([], ["--aa", "none", "--color-jitter", "0"], ["--aa", "", "--color-jitter", "0.4"]):
        mask_predictor.check_supported(utils.parse_args(["--data-source", "folder", "--imgnet-val-dir", "x", "--mixup", "0.8"] + extra))
    assert "Attention" not in capsys.readouterr().out
    with pytest.raises(SystemExit, match="color-jitter"):
        mask_predictor.check_supported(utils.parse_args(["--data-source", "folder", "--imgnet-val-dir", "x", "--mixup", "0.8",
                                                         "--color-jitter", "-0.1"]))


def _close(a, b):
    return a[:3] == b[:3] and a[3] == b[3] and a[4] == b[4]


def test_draws_are_keyed_and_follow_the_restatement():
    from d2s import data
    for interp in ("bicubic", "bilinear", "random"):
        opts = data.AugmentOptions(interp, auto_augment="rand-m9-mstd0.5-inc1", color_jitter=0.4)
        for k in range(40):
            key = [42, 3, 0, k]
            a = data.train_params(np.random.default_rng(key), 300, 400, opts, 224)
            b = data.train_params(np.random.default_rng(key), 300, 400, opts, 224)
            assert a == b                                                        # same (seed, epoch, rank, position): same draws
            # the crop / flip / erase draws are those of the transform without the stage; the ops are drawn after them
            rng = np.random.default_rng(key)
            base = data.train_params(rng, 300, 400, data.AugmentOptions(interp), 224)
            assert "ops" not in base and {k_: v for k_, v in a.items() if k_ != "ops"} == base
            want = R.draw_randaug(rng, DEFAULT, 224, interp)
            assert len(a["ops"]) == len(want) and all(_close(x, y) for x, y in zip(a["ops"], want))
    a = data.train_params(np.random.default_rng([42, 3, 0, 1]), 300, 400, opts, 224)
    b = data.train_params(np.random.default_rng([42, 4, 0, 1]), 300, 400, opts, 224)
    assert a != b


def test_randaug_draws_stay_in_range():
    from d2s import data
    rng = np.random.default_rng(0)
    cfg = data.parse_auto_augment("rand-m9-mstd0.5-n3-inc1")
    S, codes, counts, resamples = 224, set(), [], set()
    for _ in range(3000):
        ops = data.randaug_ops(rng, cfg, S, "random")
        counts.append(len(ops))
        for code, resample, iarg, farg, m in ops:
            codes.add(code)
            assert 1 <= code <= 11 and resample in (0, 1)
            if code == data.OP_POSTERIZE:
                assert 0 <= iarg <= 4
            elif code == data.OP_SOLARIZE:
                assert 0 <= iarg <= 256
            elif code == data.OP_SOLARIZE_ADD:
                assert 0 <= iarg <= 110
            elif code == data.OP_AFFINE:
                resamples.add(resample)
                assert abs(m[1]) <= 0.5 + 1e-12 and abs(m[3]) <= 0.5 + 1e-12            # shear <= 0.3, sin(30 deg) = 0.5
                if m[0] == 1 and m[4] == 1 and m[1] == 0 and m[3] == 0:
                    assert abs(m[2]) <= 0.45 * S and abs(m[5]) <= 0.45 * S              # translate
                elif m[0] != 1:
                    assert m[0] == m[4] and m[1] == -m[3] and m[0] >= np.cos(np.radians(30.0)) - 1e-15    # rotate within 30 degrees (entries rounded to 15 places)
            elif code >= data.OP_COLOR:
                assert np.float32(0.1) <= farg <= np.float32(1.9)
    assert codes == set(range(1, 12)) and resamples == {0, 1}
    assert max(counts) == 3 and min(counts) == 0 and 1.3 < np.mean(counts) < 1.7        # p = 0.5 of n = 3
    # magnitude: fixed level without mstd, clipped at mmax
    ops = data.randaug_ops(np.random.default_rng(1), dict(m=30.0, mstd=0.0, n=8, p=1.0, mmax=10.0), S, "bicubic")
    for code, _, iarg, farg, m in ops:
        if code >= data.OP_COLOR:
            assert farg in (np.float32(1.9), np.float32(0.1))
        if code == data.OP_POSTERIZE:
            assert iarg == 0


def test_jitter_draws():
    from d2s import data
    orders = set()
    for k in range(200):
        ops = data.jitter_ops(np.random.default_rng(k), 0.4)
        want = R.draw_jitter(np.random.default_rng(k), 0.4)
        assert ops == want and sorted(o[0] for o in ops) == [data.OP_COLOR, data.OP_CONTRAST, data.OP_BRIGHTNESS]
        assert all(np.float32(0.6) <= o[3] <= np.float32(1.4) for o in ops)
        orders.add(tuple(o[0] for o in ops))
    assert len(orders) == 6
    assert all(o[3] >= 0 for o in data.jitter_ops(np.random.default_rng(0), 1.5))          # the lower end stops at 0
    # timm applies only one of the two: RandAugment wins
    p = data.train_params(np.random.default_rng(0), 50, 60, data.AugmentOptions(auto_augment="", color_jitter=0.4), 32)
    assert len(p["ops"]) == 3


def test_off_means_no_table_and_packing():
    from d2s import data
    rng = np.random.default_rng(0)
    im = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    off = data.AugmentOptions(auto_augment="none", color_jitter=0.0)
    p = [data.train_params(np.random.default_rng(k), 40, 50, off, 32) for k in range(3)]
    hb = data.pack_batch([im] * 3, [0, 1, 2], p, 32)
    assert "ops" not in hb and hb["desc"].shape == (3, data.DESC_INTS) and data.DESC_INTS == 64
    on = data.AugmentOptions(auto_augment="rand-m9-mstd0.5-n4-p1-inc1")
    q = [data.train_params(np.random.default_rng(k), 40, 50, on, 32) for k in range(3)]
    hb2 = data.pack_batch([im] * 3, [0, 1, 2], q, 32)
    assert np.array_equal(hb2["desc"].numpy(), hb["desc"].numpy()) and np.array_equal(hb2["pix"].numpy(), hb["pix"].numpy())
    t = hb2["ops"].numpy()
    assert t.shape == (3, data.RA_MAX_OPS, data.RA_OP_INTS) and t.dtype == np.int32
    for b in range(3):
        ops = q[b]["ops"]
        assert (t[b, :len(ops), 0] != 0).all() and (t[b, len(ops):] == 0).all()
        for k, (code, resample, iarg, farg, m) in enumerate(ops):
            assert tuple(t[b, k, :3]) == (code, resample, iarg) and t[b, k, 3:4].view(np.float32)[0] == np.float32(farg)
            assert tuple(t[b, k, 4:16].view(np.float64)) == m
    assert data.pack_ops([[], []]).any() == False                                        # noqa: E712
    with pytest.raises(ValueError):
        data.pack_ops([[R.mk(R.OP_INVERT)] * 9])
