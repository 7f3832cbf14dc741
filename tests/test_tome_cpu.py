"""Token merging (--method tome), the parts that need no GPU: the float64 restatement in tests/tome_ref.py against a
literal transcription of the published algorithm, the key-weighted softmax identity, the clipping of r, the command line's acceptance and
refusals, the model's constructor, the library binding, and that the package imports neither oracle/ nor tests/."""
import math
import os
import re

import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import tome_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)


# ---- the published algorithm (facebookresearch/ToMe, tome/merge.py), written out: bipartite_soft_matching with class_token=True and merge_wavg
def published_bipartite_soft_matching(metric, r):
    t = metric.shape[1]
    r = min(r, (t - 1) // 2)
    if r <= 0:
        return None
    metric = metric / metric.norm(dim=-1, keepdim=True)
    a, b = metric[..., ::2, :], metric[..., 1::2, :]
    scores = a @ b.transpose(-1, -2)
    scores[..., 0, :] = -math.inf
    node_max, node_idx = scores.max(dim=-1)
    edge_idx = node_max.argsort(dim=-1, descending=True)[..., None]
    unm_idx = edge_idx[..., r:, :]
    src_idx = edge_idx[..., :r, :]
    dst_idx = node_idx[..., None].gather(dim=-2, index=src_idx)
    unm_idx = unm_idx.sort(dim=1)[0]

    def merge(x, mode="mean"):
        src, dst = x[..., ::2, :], x[..., 1::2, :]
        n, t1, c = src.shape
        unm = src.gather(dim=-2, index=unm_idx.expand(n, t1 - r, c))
        src = src.gather(dim=-2, index=src_idx.expand(n, r, c))
        dst = dst.scatter_reduce(-2, dst_idx.expand(n, r, c), src, reduce=mode)
        return torch.cat([unm, dst], dim=1)
    return merge, unm_idx[..., 0], src_idx[..., 0], dst_idx[..., 0]


def published_merge_wavg(merge, x, size=None):
    if size is None:
        size = torch.ones_like(x[..., 0, None])
    x = merge(x * size, mode="sum")
    size = merge(size, mode="sum")
    return x / size, size


@pytest.mark.parametrize("B,n,H,r", [(2, 9, 3, 2), (2, 10, 2, 4), (3, 65, 3, 16), (2, 66, 1, 32), (2, 197, 6, 13), (2, 17, 2, 100)])
def test_ref_agrees_with_the_published_algorithm(B, n, H, r):
    gen = torch.Generator().manual_seed(77 + n)
    qkv = torch.randn((B, n, 3, H, 64), generator=gen)
    x = torch.randn((B, n, 32), generator=gen, dtype=torch.float64)
    size = torch.randint(1, 6, (B, n), generator=gen).double()
    assert min(R.gaps(qkv, r)) > 1e-9                                # no ties: the published code leaves them to the framework
    merge, unm_p, src_p, dst_p = published_bipartite_soft_matching(qkv[:, :, 1].double().mean(dim=2), r)
    node_max, node_idx, unm, src, dst = R.match(qkv, r)
    re = R.clip_r(r, n)
    assert unm.shape == (B, (n + 1) // 2 - re) and src.shape == (B, re)
    assert torch.equal(unm, unm_p)
    order = src_p.argsort(dim=1)                                     # the published sources come in rank order, ours ascending
    assert torch.equal(src, src_p.gather(1, order)) and torch.equal(dst, dst_p.gather(1, order))
    assert bool((node_max[:, 0] == -math.inf).all()) and bool((node_idx[:, 0] == 0).all())
    for s in (None, size):
        want_x, want_s = published_merge_wavg(merge, x, None if s is None else s[..., None])
        got_x, got_s, group, _ = R.merge(x, s, unm, src, dst)
        torch.testing.assert_close(got_x, want_x, rtol=1e-13, atol=1e-13)
        assert torch.equal(got_s, want_s[..., 0])
        assert int(group.sum()) == B * n                             # every input row lands in exactly one output row


def test_ref_tie_rules_on_hand_made_rows():
    gen = torch.Generator().manual_seed(5)
    qkv = torch.randn((1, 10, 3, 2, 64), generator=gen)
    qkv[:, 3, 1] = qkv[:, 1, 1]                  # B rows 0 and 1 identical
    qkv[:, 2, 1] = 2.0 * qkv[:, 1, 1]            # A row 1 points exactly at them
    node_max, node_idx, _, _, _ = R.match(qkv, 0)
    assert int(node_idx[0, 1]) == 0 and 1 not in node_idx[0].tolist()
    qkv = torch.randn((1, 10, 3, 2, 64), generator=gen)
    qkv[:, 4, 1] = 3.0 * qkv[:, 1, 1]            # A rows 2 and 3 identical and the best matched of all
    qkv[:, 6, 1] = 3.0 * qkv[:, 1, 1]
    node_max, _, unm, src, dst = R.match(qkv, 1)
    assert float(node_max[0, 2]) == float(node_max[0, 3]) and src.tolist() == [[2]] and dst.tolist() == [[0]] and 3 in unm[0].tolist()
    assert R.match(qkv, 2)[3].tolist() == [[2, 3]]


def test_keyw_attention_is_softmax_of_scores_plus_log_size():
    gen = torch.Generator().manual_seed(9)
    B, n, H = 2, 13, 3
    qkv = torch.randn((B, n, 3, H, 64), generator=gen)
    w = torch.randint(1, n + 1, (B, n), generator=gen).double()
    out, lse = R.keyw_attention(qkv, w, 0.125)
    q, k, v = (qkv[:, :, i].double().transpose(1, 2) for i in range(3))
    S = (q @ k.transpose(-1, -2)) * 0.125 + torch.log(w)[:, None, None, :]
    torch.testing.assert_close(out, (torch.softmax(S, dim=-1) @ v).transpose(1, 2).reshape(B, n, H * 64), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(lse, torch.logsumexp(S, dim=-1), rtol=1e-12, atol=1e-12)


def test_clipping_of_r():
    from d2s import ops
    for n, r, want in ((17, 8, 8), (17, 100, 8), (9, 8, 4), (5, 8, 2), (3, 8, 1), (2, 8, 0), (2, 0, 0), (197, 13, 13), (196, 200, 97), (10, 0, 0)):
        assert R.clip_r(r, n) == want and ops.tome_clip_r(r, n) == want
    n, trail = 17, []
    for _ in range(4):
        n -= R.clip_r(8, n)
        trail.append(n)
    assert trail == [9, 5, 3, 2]
    qkv = torch.randn((1, 5, 3, 1, 64), generator=torch.Generator().manual_seed(1))
    assert R.match(qkv, 9)[3].shape == (1, 2) and R.match(qkv, 0)[2].tolist() == [[0, 1, 2]]


# ---- command line ----
def test_check_supported_accepts_and_refuses():
    import mask_predictor
    import utils
    a = utils.parse_args([])
    assert a.tome_r == 0 and a.method == "d2s"
    refusals = ((["--method", "tome", "--student-checkpoint", "w.pt"], "--method tome without --eval-only"),
                (["--method", "tome", "--eval-only", "--student-checkpoint", "w.pt", "--gemm-mode", "bf16"], "--method tome with --gemm-mode bf16"),
                (["--method", "tome", "--eval-only", "--student-checkpoint", "w.pt", "--tome-r", "-1"], "--tome-r -1"),
                (["--tome-r", "4"], "--tome-r 4 with --method d2s"),
                (["--tome-r", "4", "--method", "dynamicvit"], "--tome-r 4 with --method dynamicvit"),
                (["--method", "tome", "--eval-only"], "--eval-only without weights"))
    for extra, needle in refusals:
        with pytest.raises(SystemExit) as e:
            mask_predictor.check_supported(utils.parse_args(extra))
        assert str(e.value).startswith("not on the accelerated path: ") and needle in str(e.value), (extra, str(e.value))
    for mode in ("exact", "split"):
        a = utils.parse_args(["--method", "tome", "--eval-only", "--student-checkpoint", "w.pt", "--tome-r", "13", "--gemm-mode", mode])
        mask_predictor.check_supported(a)
        assert a.tome_r == 13 and a.method == "tome"
    mask_predictor.check_supported(utils.parse_args(["--method", "tome", "--eval-only", "--resume", "w.pt"]))      # r = 0: the dense model
    mask_predictor.check_supported(utils.parse_args(["--topk-selection"]))                                         # the default is untouched


# ---- model ----
def test_constructor_keys_and_refusals():
    import vit_models
    from vit_models import tome
    m = vit_models.VisionTransformerToMe(**MICRO, tome_r=3)
    t = vit_models.VisionTransformerTeacher(**MICRO)
    assert list(m.state_dict()) == list(t.state_dict()) and [tuple(v.shape) for v in m.state_dict().values()] == [tuple(v.shape) for v in t.state_dict().values()]
    assert m.tome_r == [3, 3, 3, 3] and m.prop_attn and m.tokens_per_block is None
    assert vit_models.VisionTransformerToMe(**MICRO, tome_r=[4, 3, 0, 1], prop_attn=False).tome_r == [4, 3, 0, 1]
    for bad in ([1, 2], -1, [1, 1, 1, -2]):
        with pytest.raises(ValueError):
            vit_models.VisionTransformerToMe(**MICRO, tome_r=bad)
    m.train()
    with pytest.raises(NotImplementedError) as e:      # raised before anything touches the device
        m(torch.zeros(1, 3, 64, 64))
    assert str(e.value) == tome.TOME_TRAINING_ERROR and "inference only" in str(e.value)
    small = vit_models.tome_deit_small_patch16_224(13)
    assert small.tome_r == [13] * 12 and small.embed_dim == 384
    assert vit_models.tome_deit_tiny_patch16_224(2).embed_dim == 192 and callable(vit_models.tome_deit_base_patch16_224)


# ---- binding ----
def test_library_binding_declares_the_three_entries_once():
    from d2s import lib, ops
    header = open(os.path.join(REPO, "include", "d2s_hip.h")).read()
    for name in ("d2s_tome_match", "d2s_tome_merge", "d2s_attn_keyw_fwd_f32"):
        assert name in lib.symbols("d2s_hip.h") and "int " + name + "(" in header
    assert callable(ops.tome_match) and callable(ops.tome_merge) and callable(ops.attn_keyw_fwd)


def test_the_package_imports_neither_the_oracle_nor_the_tests():
    pkg = os.path.join(REPO, "dense2sparse-vit_amd")
    pat = re.compile(r"^\s*(?:from|import)\s+(?:oracle|tests)\b", flags=re.M)
    seen = 0
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                seen += 1
                assert not pat.search(open(os.path.join(root, f)).read()), os.path.join(root, f)
    assert seen > 10
