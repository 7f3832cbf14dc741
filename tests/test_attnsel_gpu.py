"""Attention selection (attn_selection) on the GPU: the kernel of csrc/attnsel.hip against the float64 restatement
(tests/attnsel_ref.py), ties, its consistency with d2s_select_topk, the C entry's refusals, the student (one and two stages, train and
eval, max and mean over heads, the flag off, with token fusion), TrainStep, and the bf16 arithmetic mode.

Inputs of the kernel-against-ref test.  The ids must equal the reference's exactly, so values that are neighbours in rank have to be
further apart than fp32 rounding can move them.  A gap of 1e-3 of the ROW SUM between all rank neighbours exists only while
T (T - 1) / 2 <= 1000 (the values would otherwise add up to more than the sum), i.e. for the 5-token shape here; it is asserted there.  For
every shape the test asserts a gap of 1e-3 of the larger VALUE, which is 14 times the (H + T + 2) 2^-24 = 7e-5 relative error allowed
on either probability at the longest row (T = 576, H = 12)."""
import numpy as np
import pytest
import torch

from tests import attnsel_ref as R
from tests import cases
from tests import fuse_ref
from tests.test_model_gpu import build_models, make_args, _t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24

# (B, H, n, lead, T): the smallest row / under one wave / one token past a wave / DeiT-S / one token past a 256-chunk / DeiT at 384 (three
# chunks, 12 heads) / DeiT-S with two trailing carried columns
SHAPES = [(1, 1, 6, 1, 5), (3, 3, 64, 1, 63), (2, 6, 66, 1, 65), (2, 6, 197, 1, 196), (2, 12, 260, 1, 257), (1, 12, 577, 1, 576),
          (2, 6, 199, 1, 196)]


def _ops():
    from d2s import ops
    return ops


def _bound(H, T):
    """relative, per probability: an H-term mean, a T-term sum of positive values, one division"""
    return (H + T + 2) * EPS


def _check_probs(got, want, H, T, what):
    rel = ((got.double().cpu() - want).abs() / want).max()
    print(f"[attnsel {what}] largest relative error {float(rel):.3e}, bound {_bound(H, T):.3e}")
    assert bool(torch.isfinite(got).all()) and float(rel) <= _bound(H, T), what


# ---- 1. kernel against the reference ----
@pytest.mark.parametrize("B,H,n,lead,T", SHAPES)
def test_kernel_against_the_reference(B, H, n, lead, T):
    ops = _ops()
    for mean in (False, True):
        rows = R.gapped_rows(B, H, n, lead, T, mean, seed=17 * T + H)
        rel, of_sum = R.rank_gaps(R.reduce_heads(rows, lead, T, mean))
        assert rel >= 1e-3
        if T * (T - 1) // 2 <= 1000:
            assert of_sum >= 1e-3
        dev_rows = rows.to(DEV)
        for k in (0, 1, T // 2, T):
            want_p, want_k, want_d = R.select(rows, lead, T, k, mean)
            probs, kept, dropped = ops.select_cls_attn(dev_rows, lead, T, k, mean)
            torch.cuda.synchronize()
            assert probs.shape == (B, T) and kept.shape == (B, k) and dropped.shape == (B, T - k)
            assert kept.dtype == dropped.dtype == torch.int64
            assert torch.equal(kept.cpu(), want_k) and torch.equal(dropped.cpu(), want_d)
            both = torch.sort(torch.cat([kept, dropped], dim=1).cpu(), dim=1)[0]
            assert torch.equal(both, torch.arange(T).expand(B, T))
            _check_probs(probs, want_p, H, T, f"B={B} H={H} n={n} T={T} k={k} mean={mean}")


# ---- 2. ties ----
def test_ties_take_the_lowest_index_first():
    ops = _ops()
    vals = torch.tensor([8.0, 7.0, 5.0, 1.0, 2.0, 5.0, 5.0, 3.0])             # columns 2, 5, 6 are duplicates around places 3 - 5
    scale = torch.tensor([1.0, 0.5, 0.25])
    rows = torch.full((2, 3, 10), 9.0)
    rows[:, :, 1:9] = scale[None, :, None] * vals[None, None, :]              # identical in every head up to the head's scale
    for mean in (False, True):
        for k, want in ((2, [0, 1]), (3, [0, 1, 2]), (4, [0, 1, 2, 5]), (5, [0, 1, 2, 5, 6]), (6, [0, 1, 2, 5, 6, 7])):
            probs, kept, dropped = ops.select_cls_attn(rows.to(DEV), 1, 8, k, mean)
            assert kept.cpu().tolist() == [want, want]
            assert dropped.cpu().tolist() == [sorted(set(range(8)) - set(want))] * 2
            p = probs.cpu()
            assert torch.equal(p[:, 2], p[:, 5]) and torch.equal(p[:, 2], p[:, 6])
            assert torch.equal(kept.cpu(), R.select(rows, 1, 8, k, mean)[1])
    flat = torch.full((1, 2, 301), 0.25, device=DEV)                          # every token equal, across two 256-chunks
    _, kept, dropped = ops.select_cls_attn(flat, 1, 300, 130)
    assert kept.cpu().tolist() == [list(range(130))] and dropped.cpu().tolist() == [list(range(130, 300))]


# ---- 3. self-consistency ----
@pytest.mark.parametrize("B,H,n,lead,T", [(2, 6, 197, 1, 196), (2, 12, 260, 1, 257), (3, 2, 19, 1, 16)])
def test_select_topk_of_the_emitted_probs_gives_the_same_ids(B, H, n, lead, T):
    ops = _ops()
    gen = torch.Generator().manual_seed(n)
    rows = torch.softmax(torch.randn((B, H, n), generator=gen) * 3.0, dim=-1).to(DEV)
    wild = rows.clone()
    wild[:, :, :lead] = 3.0e38
    wild[:, :, lead + T:] = 3.0e38
    for mean in (False, True):
        for k in (1, T // 2, T - 1):
            probs, kept, dropped = ops.select_cls_attn(rows, lead, T, k, mean)
            k2, d2 = ops.select_topk(probs, k)
            assert torch.equal(kept, k2) and torch.equal(dropped, d2)
            again = ops.select_cls_attn(rows, lead, T, k, mean)
            other = ops.select_cls_attn(wild, lead, T, k, mean)
            for a, b, c in zip((probs, kept, dropped), again, other):
                assert torch.equal(a, b) and torch.equal(a, c)
            _check_probs(probs, R.select(rows.cpu(), lead, T, k, mean)[0], H, T, f"softmax rows n={n} k={k} mean={mean}")


# ---- 4. argument checks ----
def test_the_entry_refuses_bad_arguments_without_launching():
    from d2s import lib
    rows = torch.rand((1, 1, 16386), device=DEV) + 0.5
    probs = torch.full((1, 16386), 7.0, device=DEV)
    kept = torch.full((1, 16386), -7, dtype=torch.int64, device=DEV)
    dropped = torch.full((1, 16386), -7, dtype=torch.int64, device=DEV)
    P = lib.ptr
    # each case trips exactly one check: every other argument is legal for the 16386-wide buffers
    bad = {"lead + T > n": (P(rows), 1, 1, 8, 1, 8, 4, 0, P(probs), P(kept), P(dropped)),
           "lead + T > n at the largest T": (P(rows), 1, 1, 16384, 1, 16384, 4, 0, P(probs), P(kept), P(dropped)),
           "lead alone past n": (P(rows), 1, 1, 8, 8, 1, 1, 0, P(probs), P(kept), P(dropped)),
           "k > T": (P(rows), 1, 1, 16386, 1, 8, 9, 0, P(probs), P(kept), P(dropped)),
           "T > 16384": (P(rows), 1, 1, 16386, 1, 16385, 4, 0, P(probs), P(kept), P(dropped)),
           "null probs": (P(rows), 1, 1, 16386, 1, 8, 4, 0, None, P(kept), P(dropped))}
    for what, a in bad.items():
        with pytest.raises(lib.D2SError, match="d2s_select_cls_attn failed with code -1"):
            lib.call("d2s_select_cls_attn", *a)
    torch.cuda.synchronize()
    assert bool((probs == 7.0).all()) and bool((kept == -7).all()) and bool((dropped == -7).all())
    lib.call("d2s_select_cls_attn", P(rows), 1, 1, 16386, 1, 8, 4, 0, P(probs), P(kept), P(dropped))      # the same call, legal
    torch.cuda.synchronize()
    assert abs(float(probs[0, :8].sum()) - 1.0) < 1e-5 and sorted(kept[0, :4].tolist() + dropped[0, :4].tolist()) == list(range(8))


# ---- 5. the model ----
def _student(case, **kw):
    """The case's student weights in a student built with **kw (init_n / token_ratio / pruning_loc may be overridden)."""
    import vit_models
    cfg = case["cfg"]
    student, teacher, _, _ = build_models(case, torch.device(DEV))
    common = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                  mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
    kw.setdefault("pruning_loc", list(cfg["pruning_loc"]))
    kw.setdefault("token_ratio", list(cfg["token_ratio"]))
    kw.setdefault("init_n", cfg["init_n"])
    m = vit_models.VisionTransformerDiffPruning(distill=True, topk_selection=True, predictor_loss_type=cfg["loss_type"],
                                                small_predictor=cfg["small_predictor"], **common, **kw)
    m.load_state_dict(student.state_dict(), strict=True)
    return m.to(DEV), teacher


def _forward(student, x, train):
    """-> (logits, cls_attns, pred_logits, kept) in either mode"""
    student.train(train)
    with torch.no_grad():
        out = student(x)
    if train:
        return out[0], list(student.cls_attns), out[2], out[3]
    return out


@pytest.mark.parametrize("name", ["micro1", "micro2"])
def test_student_selects_by_its_own_cls_attention(name):
    ops = _ops()
    case = cases.MODEL_CASES[name]
    cfg = case["cfg"]
    x = _t(cases.make_images(case)).to(DEV)
    locs = list(cfg["pruning_loc"])
    ks = [int(cfg["init_n"] * r) for r in cfg["token_ratio"]]
    base, _ = _student(case)
    _, _, base_scores, base_kept = _forward(base, x, False)
    differs = False
    for train in (False, True):
        for mean in (False, True):
            student, _ = _student(case, attn_selection=True, mean_heads=mean)
            logits, cls_attns, pred, kept = _forward(student, x, train)
            assert bool(torch.isfinite(logits).all()) and len(pred) == len(kept) == len(locs) and len(cls_attns) == cfg["depth"]
            want = R.stage_loop([c.cpu() for c in cls_attns], locs, ks, mean)
            for s, (wp, wk, wd) in enumerate(want):
                T = cls_attns[locs[s] - 1].shape[-1]
                assert pred[s].shape == (case["batch"], T) and not pred[s].requires_grad
                _check_probs(pred[s], wp, cfg["heads"], T, f"{name} stage {s} train={train} mean={mean}")
                k2, d2 = ops.select_topk(pred[s].contiguous(), ks[s])
                assert torch.equal(kept[s], k2) and torch.equal(student.dropped_token_indices[s], d2)
                assert kept[s].shape == base_kept[s].shape
            differs = differs or not torch.equal(kept[0], base_kept[0])
            # replaying the recorded selection gives the same logits
            student.kept_token_override = [k.clone() for k in kept]
            assert torch.equal(_forward(student, x, train)[0], logits)
    assert differs, "attention selection kept exactly the predictor's tokens for every image: the flag does nothing"


def test_flag_off_is_the_default_forward_bit_for_bit():
    case = cases.MODEL_CASES["micro2"]
    x = _t(cases.make_images(case)).to(DEV)
    base, _ = _student(case)
    off, _ = _student(case, attn_selection=False, mean_heads=True)             # mean_heads alone has no effect
    for train in (False, True):
        a, b = _forward(base, x, train), _forward(off, x, train)
        assert torch.equal(a[0], b[0])
        assert all(torch.equal(p, q) for p, q in zip(a[2], b[2])) and all(torch.equal(p, q) for p, q in zip(a[3], b[3]))


def test_with_token_fusion_the_package_row_is_weighted_by_the_attention_probs(monkeypatch):
    """micro2: the second stage carries a package row (t = 1), which is not scored.  The bound is tests/test_fuse_gpu.py's for f:
    4 (m + 2) u sum_j |w_j x_jc| with m dropped tokens."""
    import d2s.functional as DF
    ops = _ops()
    case = cases.MODEL_CASES["micro2"]
    x = _t(cases.make_images(case)).to(DEV)
    student, _ = _student(case, attn_selection=True, fuse_dropped=True)
    student.train()
    calls = []
    orig = DF.GatherFuseFn.apply

    def spy(xs, p, kept, dropped, t):
        xs.retain_grad()
        y = orig(xs, p, kept, dropped, t)
        calls.append((xs, p, kept, dropped, t, y))
        return y
    monkeypatch.setattr(DF.GatherFuseFn, "apply", staticmethod(spy))
    logits, features, pred, kept_all = student(x)
    logits.sum().backward()
    ops.join_weight_grads()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert [c[4] for c in calls] == [0, 1]
    for s, (xs, p, kept, dropped, t, y) in enumerate(calls):
        assert p is pred[s] and not p.requires_grad and torch.equal(kept, kept_all[s])
        assert p.shape[1] == xs.shape[1] - 1 - t                              # the carried rows are not scored
        assert xs.grad is not None and bool(torch.isfinite(xs.grad).all()) and float(xs.grad.abs().max()) > 0
        xc, pc, kc, dc = xs.detach().cpu(), p.cpu(), kept.cpu(), dropped.cpu()
        want = fuse_ref.fuse_forward_f64(xc, pc, kc, dc, t)
        Bc, m, D = xc.shape[0], dc.shape[1], xc.shape[2]
        T = xc.shape[1] - 1 - t
        pd = torch.gather(pc.double(), 1, dc)
        w = pd / pd.sum(dim=1, keepdim=True)
        xd = torch.gather(xc.double()[:, 1:1 + T], 1, dc[:, :, None].expand(Bc, m, D))
        bound = 4.0 * (m + 2) * EPS * (w[:, :, None] * xd).abs().sum(dim=1)
        err = (y[:, -1].detach().cpu().double() - want[:, -1]).abs()
        print(f"[attnsel fuse stage {s}] largest fraction of the bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        assert torch.equal(y[:, :-1].detach().cpu(), want[:, :-1].float())    # CLS, kept and carried rows are copies
    assert all(p.grad is None for p in student.score_predictor.parameters())


# ---- 6. TrainStep ----
def _train(steps, warmup_steps=0):
    """micro1's weights in a student whose init_n is its own token count (16), keep 0.5: the stage keeps 8 ids and MaskLoss ranks 8"""
    from d2s.engine import TrainStep
    case = cases.MODEL_CASES["micro1"]
    student, teacher = _student(case, attn_selection=True, init_n=16, token_ratio=[0.5])
    args = make_args(case["cfg"])
    args.keep_ratios = [0.5]
    before = {n: p.detach().clone() for n, p in student.named_parameters()}
    ts = TrainStep(student, teacher, args, warmup_steps=warmup_steps, graph=False)
    x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
    torch.manual_seed(5)
    infos = []
    for _ in range(steps):
        info = ts(x, y)
        torch.cuda.synchronize()
        infos.append(dict(loss=info["loss"].detach().clone(), mask_loss=info["mask_loss"].detach().clone(),
                          kept=[k.clone() for k in info["kept"]], cls_attn=info["cls_attn"].clone()))
    return ts, student, before, infos


def test_train_steps_leave_the_predictors_alone_and_report_the_agreement():
    ts, student, before, infos = _train(3)
    after = dict(student.named_parameters())
    pred = [n for n in before if n.startswith("score_predictor.")]
    assert len(pred) == 24
    for n in pred:
        assert torch.equal(after[n].detach(), before[n]), n
        assert after[n].grad is None and not bool(ts.arena.grad_views[n].any())
    moved = [n for n in before if n.startswith("blocks.") and not torch.equal(after[n].detach(), before[n])]
    assert len(moved) == sum(n.startswith("blocks.") for n in before) and not torch.equal(after["head.weight"].detach(), before["head.weight"])
    assert all(bool(torch.isfinite(i["loss"])) for i in infos)
    assert all(float(i["mask_loss"]) == 0.0 and not i["mask_loss"].requires_grad for i in infos)
    assert float(ts.metrics["train_mask_loss"]) == 0.0
    agree = []
    for i in infos:
        assert i["kept"][0].shape == (3, 8)
        gt, _ = R.stable_topk(R.teacher_target(i["cls_attn"].cpu()), 8)
        agree.append(R.mask_agreement(i["kept"][0].cpu(), gt, 16))
    acc = float(ts.metrics["train_mask_acc_0"])
    print(f"[attnsel step] per-step agreement with the teacher target {agree}, train_mask_acc_0 {acc:.6f}")
    assert 0.0 <= acc <= 1.0 and acc == pytest.approx(sum(agree) / 3.0, abs=1e-6)
    assert set(ts.metrics) >= {"train_mask_loss", "train_mask_acc_0", "train_backbone_loss"}
    cfg = ts.config()
    assert cfg["attn_selection"] is True and cfg["mean_heads"] is False
    # a second identical run: the same bits
    ts2, _, _, infos2 = _train(3)
    assert torch.equal(ts.arena.params, ts2.arena.params)
    assert all(torch.equal(a["loss"], b["loss"]) and torch.equal(a["kept"][0], b["kept"][0]) for a, b in zip(infos, infos2))


def test_mask_accuracy_when_init_n_is_not_the_token_count():
    """micro1 with init_n = 24 at keep 0.5: the stage keeps 12 of its 16 tokens while MaskLoss ranks int(16 * 0.5) = 8 (the predictor path
    re-ranks its scores at that count too).  The accuracy is then that of the top 8 of the stage's own probabilities against the teacher
    target's top 8."""
    from d2s.engine import TrainStep
    case = cases.MODEL_CASES["micro1"]
    student, teacher = _student(case, attn_selection=True, init_n=24, token_ratio=[0.5])
    args = make_args(case["cfg"])
    args.keep_ratios = [0.5]
    ts = TrainStep(student, teacher, args, warmup_steps=0, graph=False)
    x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
    info = ts(x, y)
    torch.cuda.synchronize()
    assert info["kept"][0].shape == (3, 12) and info["pred_logits"][0].shape == (3, 16)
    pm, _ = R.stable_topk(info["pred_logits"][0].cpu(), 8)
    gt, _ = R.stable_topk(R.teacher_target(info["cls_attn"].cpu()), 8)
    assert set(pm[0].tolist()) <= set(info["kept"][0][0].tolist())           # the top 8 are among the 12 kept
    assert float(ts.metrics["train_mask_acc_0"]) == pytest.approx(R.mask_agreement(pm, gt, 16), abs=1e-6)
    assert float(info["mask_loss"]) == 0.0 and bool(torch.isfinite(info["loss"]))


def test_graph_step_is_bit_identical_to_the_eager_step():
    """nothing in an attention-selecting stage synchronises with the host: the captured step replays the same bits (micro2, two stages,
    with and without token fusion)"""
    from d2s.engine import TrainStep
    from tests.test_graph_gpu import _same_step, _batches
    case = cases.MODEL_CASES["micro2"]
    for fuse in (False, True):
        eager, graph = [TrainStep(*_student(case, attn_selection=True, fuse_dropped=fuse), make_args(case["cfg"]), warmup_steps=0, graph=gr)
                        for gr in (False, True)]
        for i, (x, y) in enumerate(_batches(case, eager.GRAPH_WARM_STEPS + 2, torch.device(DEV))):
            _same_step(eager, graph, x, y, f"fuse {fuse} step {i}")
        assert graph.last_step_captured and not eager.last_step_captured
        for k, v in eager.metrics.items():
            assert float(v) == float(graph.metrics[k]), k


def test_the_largest_row_runs():
    """T = 16384, the entry's limit: 128 KiB of dynamic LDS, above the runtime's default per-kernel limit (the entry raises it)"""
    ops = _ops()
    T = 16384
    rows = R.gapped_rows(1, 1, T + 1, 1, T, False, seed=3)
    assert R.rank_gaps(R.reduce_heads(rows, 1, T))[0] >= 1e-3
    for k in (1, T // 2):
        want_p, want_k, want_d = R.select(rows, 1, T, k)
        probs, kept, dropped = ops.select_cls_attn(rows.to(DEV), 1, T, k)
        torch.cuda.synchronize()
        assert torch.equal(kept.cpu(), want_k) and torch.equal(dropped.cpu(), want_d)
        _check_probs(probs, want_p, 1, T, f"T={T} k={k}")


def test_train_step_refuses_a_warmup():
    with pytest.raises(ValueError, match="warmup_steps"):
        _train(0, warmup_steps=1)


# ---- 7. bf16 arithmetic mode ----
def test_bf16_mode_selects_by_the_same_rule():
    import vit_models
    ops = _ops()
    ops.set_gemm_mode(ops.GEMM_BF16)
    try:
        torch.manual_seed(0)
        student = vit_models.dynamic_vit_small_patch16_224_student([3, 6], [0.5, 0.25], topk_selection=True, attn_selection=True,
                                                                   predictor_loss_type="kl_div").to(DEV)
        gen = torch.Generator().manual_seed(4)
        x = torch.randn((2, 3, 224, 224), generator=gen).to(DEV)
        logits, cls_attns, pred, kept = _forward(student, x, False)
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_mode(ops.GEMM_EXACT)
    assert bool(torch.isfinite(logits).all())
    want = R.stage_loop([c.cpu() for c in cls_attns], [3, 6], [98, 49])
    for s, (wp, _, _) in enumerate(want):
        assert cls_attns[[3, 6][s] - 1].dtype == torch.float32
        _check_probs(pred[s], wp, 6, wp.shape[1], f"bf16 stage {s}")
        k2, d2 = ops.select_topk(pred[s].contiguous(), [98, 49][s])
        assert torch.equal(kept[s], k2) and torch.equal(student.dropped_token_indices[s], d2)
