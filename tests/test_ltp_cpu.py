"""The LTP kernels, the parts that need no GPU: the properties of the float64 restatement in tests/ltp_ref.py (every
image's scores sum to 1 in the three forms; the policy form with an all-ones policy and eps = 0 is the plain form; the varlen form is the
plain form image by image), the closed-form backward of the soft mask against float64 autograd with the condition that rules out
cancellation, the decision rule at score == theta, the header and binding tables; the model cases of the GPU tests with the conditions
on their inputs asserted (the binarised soft restatement with eps = 0 is the hard one, an image alone with its pruned tokens deleted
gives the batch's logits), the command line and every refusal, build_models, the constructor and the state-dict keys, TrainStep's
refusals, the loss and the checkpoint config."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import cases  # noqa: F401  (puts the package on sys.path)
from tests import ltp_ref as R
from oracle import d2s_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["d2s_ltp_score_f32", "d2s_ltp_score_workspace_bytes", "d2s_ltp_select", "d2s_ltp_soft_mask_bwd", "d2s_ltp_soft_mask_fwd"]
SCALE = 0.125


def make_qkv(rows, H, seed, gain=1.4):
    """qkv [rows, 3, H, 64] float64 on the fp32 grid; q and k scaled so that S has a standard deviation of gain^2 = 2 and max |S| lands at about 5-10"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((rows, 3, H, 64), generator=g, dtype=torch.float64)
    qkv[:, :2] *= gain
    return qkv.float().double()


def make_policy(kind, B, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "ones":
        m = torch.ones((B, n), dtype=torch.float64)
    elif kind == "cls_only":
        m = torch.zeros((B, n), dtype=torch.float64)
    else:                                   # exact 0, exact 1 and values in between
        m = torch.rand((B, n), generator=g, dtype=torch.float64)
        pick = torch.rand((B, n), generator=g)
        m[pick < 0.3] = 0.0
        m[pick > 0.7] = 1.0
    m[:, 0] = 1.0
    return m.float().double()


# ---- the score ----
@pytest.mark.parametrize("B,n,H", [(1, 2, 1), (3, 33, 2), (2, 65, 6)])
def test_every_images_scores_sum_to_one_in_the_three_forms(B, n, H):
    qkv = make_qkv(B * n, H, 7 * n + H)
    S = (qkv.reshape(B, n, 3, H, 64)[0, :, 0, 0] @ qkv.reshape(B, n, 3, H, 64)[0, :, 1, 0].T) * SCALE
    assert 1.0 < float(S.abs().max()) < 12.0, float(S.abs().max())       # the logits are far from uniform
    plain = R.score_plain(qkv, B, n, H, SCALE)
    assert torch.allclose(plain.sum(dim=1), torch.ones(B, dtype=torch.float64), rtol=1e-12, atol=0)
    for kind in ("ones", "mixed", "cls_only"):
        for eps in (0.0, 1e-6):
            s = R.score_policy(qkv, make_policy(kind, B, n, n), B, n, H, SCALE, eps)
            assert torch.allclose(s.sum(dim=1), torch.ones(B, dtype=torch.float64), rtol=1e-12, atol=0), (kind, eps)
    assert torch.allclose(R.score_policy(qkv, make_policy("ones", B, n, 0), B, n, H, SCALE, 0.0), plain, rtol=1e-13, atol=0)
    assert torch.equal(R.score_varlen(qkv, [n] * B, H, SCALE), plain.reshape(-1))


def test_varlen_scores_sum_to_one_per_image_and_a_lone_cls_row_scores_one():
    lens = [1, 2, 17, 33]
    s = R.score_varlen(make_qkv(sum(lens), 2, 3), lens, 2, SCALE)
    r0 = 0
    for n in lens:
        assert abs(float(s[r0:r0 + n].sum()) - 1.0) < 1e-12
        r0 += n
    assert float(s[0]) == 1.0


def test_policy_statistics_reproduce_the_probabilities():
    """lse and cinv, the two statistics the policy attention saves, give back P = exp(S - lse) mk + cinv - what the score kernel computes"""
    n = 19
    qkv = make_qkv(n, 1, 11).reshape(n, 3, 1, 64)
    S = (qkv[:, 0, 0] @ qkv[:, 1, 0].T) * SCALE
    m = make_policy("mixed", 1, n, 5)[0]
    P, lse, cinv = R.policy_softmax_rows(S, m, 1e-6)
    mk = m[None, :].repeat(n, 1)
    mk[torch.arange(n), torch.arange(n)] = 1.0
    assert torch.allclose(torch.exp(S - lse[:, None]) * mk + cinv[:, None], P, rtol=1e-12, atol=1e-300)
    assert torch.allclose(P.sum(dim=1), torch.ones(n, dtype=torch.float64), rtol=1e-12)


# ---- the decision ----
def test_select_keeps_cls_and_a_score_equal_to_the_threshold():
    score = torch.tensor([0.0, 0.3, 0.5, 0.5000001, 0.1, 0.9, 0.5], dtype=torch.float64)
    keep, counts = R.select(score, [4, 1, 2], 0.5)
    assert keep.tolist() == [1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0] and counts == [2, 0, 1]
    keep, counts = R.select(score, [4, 1, 2], 1.0)           # every image becomes its CLS row alone
    assert keep.tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0] and counts == [0, 0, 0]
    keep, counts = R.select(score, [4, 1, 2], 0.0)           # nothing leaves
    assert keep.tolist() == [1.0] * 7 and counts == [3, 0, 1]


# ---- the soft mask: closed form against autograd ----
def soft_case(B, N, seed, tau=2e-3, lam=0.05):
    """Three stages on scores near 1 / N; w_k: what the loss makes of the policy after stage k (the stand-in for the policy blocks)"""
    g = torch.Generator().manual_seed(seed)
    S = 3
    theta = [0.6 / N, 1.0 / N, 1.3 / N]
    score = [(torch.rand((B, N), generator=g, dtype=torch.float64) * 2.0 / N).float().double() for _ in range(S)]
    w = [torch.randn((B, N), generator=g, dtype=torch.float64).float().double() + 0.3 for _ in range(S)]
    return dict(B=B, N=N, S=S, tau=tau, lam=lam, theta=theta, score=score, w=w)


def soft_objective(c, theta):
    """m_0 = 1, m_k = m_{k-1} * M_k; loss = sum_k <w_k, m_k> + lam * R, R = mean of every M over stages, images and patches"""
    m = torch.ones((c["B"], c["N"]), dtype=torch.float64)
    Ms, ms, R_, loss = [], [], 0.0, 0.0
    for k in range(c["S"]):
        M, m_new, msum = R.soft_mask(c["score"][k], m, theta[k], c["tau"])
        Ms.append(M), ms.append(m)
        m = m_new
        loss = loss + (c["w"][k] * m).sum()
        R_ = R_ + msum.sum()
    R_ = R_ / (c["S"] * c["B"] * (c["N"] - 1))
    return loss + c["lam"] * R_, Ms, ms


def soft_closed_form(c, Ms, ms):
    """the backward walk of section 27: gm of the last policy first, every stage hands gm_before += gm_after * M_k down"""
    greg = c["lam"] / (c["S"] * c["B"] * (c["N"] - 1))
    gm = torch.zeros((c["B"], c["N"]), dtype=torch.float64)
    out = [None] * c["S"]
    for k in reversed(range(c["S"])):
        gm_after = gm + c["w"][k]                   # the dpolicy of everything that used the policy after stage k
        gM, gm, dth, mag = R.soft_mask_bwd(gm_after, Ms[k], ms[k], c["tau"], greg)
        out[k] = (gM, gm, dth, mag)
    return out


@pytest.mark.parametrize("B,N,seed", [(4, 17, 1), (2, 50, 2)])
def test_soft_mask_closed_form_against_autograd(B, N, seed):
    c = soft_case(B, N, seed)
    theta = [torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in c["theta"]]
    loss, Ms, ms = soft_objective(c, theta)
    for M in Ms:
        M.retain_grad()
    for m in ms[1:]:
        m.retain_grad()
    loss.backward()
    with torch.no_grad():
        closed = soft_closed_form(c, [M.detach() for M in Ms], [m.detach() for m in ms])
    for k in range(c["S"]):
        gM, gm, dth, mag = closed[k]
        assert torch.allclose(gM[:, 1:], Ms[k].grad[:, 1:], rtol=1e-9, atol=1e-15), k
        assert float(gM[:, 0].abs().max()) == 0.0
        if k > 0:
            assert torch.allclose(gm + c["w"][k - 1], ms[k].grad, rtol=1e-9, atol=1e-15), k    # m_k also feeds its own loss term
        assert torch.allclose(dth, theta[k].grad, rtol=1e-9, atol=0), k
        assert abs(float(dth)) >= 1e-2 * float(mag), (k, float(dth), float(mag))         # no cancellation: dtheta is visible
        frac = float(((Ms[k][:, 1:] > 0.05) & (Ms[k][:, 1:] < 0.95)).double().mean())
        assert frac > 0.02, (k, frac)                                                     # the sigmoid is not saturated everywhere


# ---- header and binding ----
def test_ltp_header_and_binding_tables():
    from d2s import lib, ops
    text = open(os.path.join(REPO, "include", "d2s_hip_ltp.h")).read()
    assert NEW == lib.symbols("d2s_hip_ltp.h")
    assert len(re.findall(r"^/\* ", text, flags=re.M)) == 1 + len(NEW)            # the file's comment and one per entry
    assert "D2S_ERR_ARG" in text
    assert lib.signature("d2s_ltp_score_workspace_bytes")[0] is lib.Z and all(lib.signature(n)[0] is lib.I for n in NEW if n.endswith(("f32", "select", "fwd", "bwd")))
    assert lib.query("d2s_ltp_score_workspace_bytes", 197 * 128, 6) == 197 * 128 * 6 * 4
    assert lib.query("d2s_ltp_score_workspace_bytes", 0, 6) == 0 and lib.query("d2s_ltp_score_workspace_bytes", 5, 0) == 0
    src = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "ltp.hip")).read()
    for name in NEW:
        assert len(re.findall(rf"^(?:int|size_t) {name}\(", src, flags=re.M)) == 1, name
    assert "atomic" not in src.lower().replace("no atomics", "")
    assert all(callable(getattr(ops, n)) for n in ("ltp_score", "ltp_select", "ltp_soft_mask_fwd", "ltp_soft_mask_bwd"))
    mk = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "Makefile")).read()
    assert "resources-%: %.hip" in mk and "ltp (27)" in mk                        # `make resources-ltp` reports the kernels' registers


# ---- the model cases of the GPU tests ----
# Micro geometry (D 128, H 2, depth 4, N 17, B 4), stages at blocks 0, 1, 2.  Random 0.02-std weights give near-uniform attention, so the
# qkv weights are scaled by 10.  The seeds were picked on the CPU with the float64 restatement alone (the project's weight generator,
# tests/cases.py) so that check_condition holds; theta = 0 everywhere (nothing leaves) and a stage with theta = 1 (every image becomes its
# CLS row alone) are cases of their own.
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
CFG = O.make_cfg(img_size=64, dim=128, depth=4, heads=2, num_classes=10, pruning_loc=(1,), token_ratio=(0.05,))
LOCS = [0, 1, 2]
QKV_GAIN = 10.0
LTP_CASES = {
    "ltp1": dict(case=dict(cfg=CFG, batch=4, seed=320), theta=[0.045, 0.055, 0.07]),
    "ltp2": dict(case=dict(cfg=CFG, batch=4, seed=313), theta=[0.045, 0.055, 0.07]),
    "keep_all": dict(case=dict(cfg=CFG, batch=4, seed=327), theta=[0.0, 0.0, 0.0]),
    "all_cls": dict(case=dict(cfg=CFG, batch=4, seed=327), theta=[0.045, 1.0, 0.07]),
}
PRUNING = ("ltp1", "ltp2")
# the soft-gradient case: tau and lambda chosen so that dtheta is visible (the scores sit near 1 / 17, tau is a fifth of that)
SOFT = dict(tau=0.012, lam=0.5)
_BUILT = {}


def built(name):
    """(state dict fp32, images, labels, float64 hard restatement without gradients) of a model case, once"""
    if name not in _BUILT:
        c = LTP_CASES[name]
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in cases.make_weights(c["case"])[1].items()}
        for k in sd:
            if k.endswith("attn.qkv.weight"):
                sd[k] = sd[k] * QKV_GAIN
        images = torch.from_numpy(cases.make_images(c["case"]))
        labels = torch.from_numpy(cases.make_labels(c["case"])).long()
        with torch.no_grad():
            out = R.model_hard({k: v.double() for k, v in sd.items()}, images, CFG, LOCS, c["theta"])
        _BUILT[name] = (sd, images, labels, out)
    return _BUILT[name]


def check_condition(name, out):
    """The conditions on the inputs (conditions, not measurements; nothing is excluded): in float64 every live patch of every stage is at
    least 1e-3 theta_k from its threshold; every stage leaves at least two different counts across the batch; some image loses at least
    half its patches."""
    if name in PRUNING:
        assert out["margin"] >= 1e-3, out["margin"]
        counts = [live.sum(dim=1).tolist() for live in out["live"]]
        assert all(len(set(c)) >= 2 for c in counts), counts
        assert min(counts[-1]) - 1 <= 8, counts
    elif name == "keep_all":
        assert all(bool(live.all()) for live in out["live"])
    else:
        assert all(int(live.sum()) == live.shape[0] for live in out["live"][1:]) and int(out["live"][0].sum()) > out["live"][0].shape[0]


@pytest.mark.parametrize("name", sorted(LTP_CASES))
def test_the_model_cases_qualify_and_fp32_keeps_what_float64_keeps(name):
    sd, images, _, out = built(name)
    check_condition(name, out)
    with torch.no_grad():
        out32 = R.model_hard(sd, images, CFG, LOCS, LTP_CASES[name]["theta"], dtype=torch.float32)
    assert all(torch.equal(a, b) for a, b in zip(out32["live"], out["live"]))
    for s, live_before in zip(out["scores"], [torch.ones_like(out["live"][0])] + out["live"][:-1]):
        assert torch.allclose((s * live_before).sum(dim=1), torch.ones(4, dtype=torch.float64), rtol=1e-12)
    print(name, "margin", f"{out['margin']:.2e}", "rows per block", [c.tolist() for c in out["counts"]])


@pytest.mark.parametrize("name", sorted(LTP_CASES))
def test_soft_restatement_with_binarised_masks_and_eps_zero_is_the_hard_one(name):
    sd, images, _, out = built(name)
    with torch.no_grad():
        soft = R.model_soft({k: v.double() for k, v in sd.items()}, images, CFG, LOCS, LTP_CASES[name]["theta"], tau=1.0, eps=0.0, binarise=True)
    assert torch.allclose(soft["logits"], out["logits"], rtol=1e-10, atol=1e-12)
    m = torch.ones_like(soft["M"][0])
    for M, live in zip(soft["M"], out["live"]):
        m = m * M
        assert torch.equal(m.bool(), live)


@pytest.mark.parametrize("name", sorted(LTP_CASES))
def test_an_image_alone_with_its_pruned_tokens_deleted_gives_the_batch_logits(name):
    sd, images, _, out = built(name)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        for b in range(images.shape[0]):
            logits, kept = R.model_deleted(sd64, images[b:b + 1], CFG, LOCS, LTP_CASES[name]["theta"])
            assert torch.allclose(logits[0], out["logits"][b], rtol=1e-10, atol=1e-12), (name, b)
            for ids, live in zip(kept, out["live"]):
                assert ids.tolist() == torch.nonzero(live[b]).flatten().tolist()


def test_soft_gradient_case_has_a_visible_dtheta():
    """The soft-phase gradient case of the GPU tests: closed-form dtheta from the restatement's own gM against autograd, and
    |dtheta_k| >= 1e-2 sum |summands| at every stage (no cancellation)."""
    sd, images, labels, _ = built("ltp1")
    sd64 = {k: v.double() for k, v in sd.items()}
    theta = [torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in LTP_CASES["ltp1"]["theta"]]
    out = R.model_soft(sd64, images, CFG, LOCS, theta, SOFT["tau"])
    for M in out["M"]:
        M.retain_grad()
    R.objective(out["logits"], labels, out["reg"], SOFT["lam"]).backward()
    for k, (M, th) in enumerate(zip(out["M"], theta)):
        terms = (M.grad * M.detach() * (1 - M.detach()))[:, 1:] / SOFT["tau"]
        assert torch.allclose(-terms.sum(), th.grad, rtol=1e-9, atol=0), k
        assert abs(float(th.grad)) >= 1e-2 * float(terms.abs().sum()), (k, float(th.grad), float(terms.abs().sum()))
        print(f"stage {k}: dtheta {float(th.grad):.4e}, sum |summands| {float(terms.abs().sum()):.4e}")


# ---- command line ----
LTP = ["--method", "ltp", "--pruning-locs", "3", "6", "9"]


def _check(argv):
    import mask_predictor
    import utils
    args = utils.parse_args(argv)
    mask_predictor.check_supported(args)
    return args


def test_cli_accepts_ltp_and_fills_the_defaults():
    import utils
    p = utils.parse_args([])
    assert (p.ltp_phase, p.ltp_temperature, p.ltp_lambda, p.ltp_init_threshold) == (None, None, None, None)
    for mode in ("exact", "split"):
        a = _check(LTP + ["--student-checkpoint", "w.pt", "--gemm-mode", mode])
        assert a.method == "ltp" and a.warmup_steps == 0
        assert (a.ltp_phase, a.ltp_temperature, a.ltp_lambda, a.ltp_init_threshold) == ("soft", 1e-3, 0.01, 0.005)
    a = _check(LTP + ["--ltp-phase", "hard", "--ltp-temperature", "0.01", "--ltp-lambda", "0", "--ltp-init-threshold", "0.002", "--dist-weight", "0",
                      "--warmup-steps", "0"])
    assert (a.ltp_phase, a.ltp_temperature, a.ltp_lambda, a.ltp_init_threshold) == ("hard", 0.01, 0.0, 0.002)
    assert _check(["--method", "ltp", "--pruning-locs", "0", "10", "--eval-only", "--student-checkpoint", "w.pt"]).eval_only
    d = _check([])
    assert d.ltp_phase is None and d.ltp_lambda is None                              # the other methods are not handed the defaults
    assert _check(["--warmup-steps", "5"]).warmup_steps == 5


@pytest.mark.parametrize("argv,fragment", [
    (LTP + ["--topk-selection"], "--method ltp with --topk-selection"),
    (LTP + ["--topk-selection", "--attn-selection"], "--method ltp with --attn-selection"),
    (LTP + ["--topk-selection", "--fuse-dropped"], "--method ltp with --fuse-dropped"),
    (LTP + ["--topk-selection", "--squeeze-dropped"], "--method ltp with --squeeze-dropped"),
    (LTP + ["--topk-selection", "--diff-topk"], "--method ltp with --diff-topk"),
    (LTP + ["--patch-score-threshold", "0.4"], "--method ltp with --patch-score-threshold"),
    (LTP + ["--gemm-mode", "bf16"], "--method ltp with --gemm-mode bf16"),
    (LTP + ["--eval-only", "--student-checkpoint", "w.pt", "--gemm-mode", "bf16"], "--method ltp with --gemm-mode bf16"),
    (LTP + ["--drop-path", "0.1"], "--method ltp with --drop-path 0.1"),
    (LTP + ["--torch-optim"], "--method ltp with --torch-optim"),
    (LTP + ["--warmup-steps", "3"], "--method ltp with --warmup-steps 3"),
    (["--method", "ltp", "--pruning-locs", "3", "11"], "--method ltp with --pruning-locs 3 11"),
    (["--method", "ltp", "--pruning-locs", "6", "3"], "--method ltp with --pruning-locs 6 3"),
    (LTP + ["--ltp-temperature", "0"], "--ltp-temperature 0.0 (tau > 0)"),
    (LTP + ["--ltp-temperature", "-1"], "--ltp-temperature -1.0 (tau > 0)"),
    (LTP + ["--ltp-lambda", "-0.1"], "--ltp-lambda -0.1 (lambda >= 0)"),
    (["--ltp-phase", "hard"], "--ltp-phase with --method d2s"),
    (["--ltp-temperature", "0.01"], "--ltp-temperature with --method d2s"),
    (["--method", "dynamicvit", "--ltp-lambda", "0.1"], "--ltp-lambda with --method dynamicvit"),
    (["--method", "avit", "--ltp-init-threshold", "0.01"], "--ltp-init-threshold with --method avit"),
    (LTP + ["--tome-r", "2"], "--tome-r 2 with --method ltp"),
    (LTP + ["--ats-tokens", "8"], "--ats-tokens with --method ltp"),
    (LTP + ["--avit-gate-scale", "4"], "--avit-gate-scale with --method ltp"),
    (LTP + ["--evo-keep", "0.5"], "--evo-keep with --method ltp"),
])
def test_cli_refusals(argv, fragment):
    with pytest.raises(SystemExit) as e:
        _check(argv)
    assert str(e.value).startswith("not on the accelerated path: ") and fragment in str(e.value), str(e.value)


def test_build_models_builds_the_teacher_unless_dist_weight_is_zero(monkeypatch, capsys):
    import mask_predictor
    import vit_models
    seen = {}

    def factory(checkpoint_path=None, **kw):
        seen["kw"] = kw
        return vit_models.VisionTransformerLTP(**MICRO, **kw)

    def teacher_factory(checkpoint_path=None):
        seen["teacher_checkpoint"] = checkpoint_path
        return vit_models.VisionTransformerTeacher(**MICRO)
    monkeypatch.setattr(vit_models, "ltp_deit_tiny_patch16_224", factory)
    monkeypatch.setattr(vit_models, "dynamic_vit_tiny_patch16_224_teacher", teacher_factory)
    base = dict(arch="deit_tiny", method="ltp", student_checkpoint=None, resume=None, teacher_checkpoint=None, device=torch.device("cpu"),
                pruning_locs=[0, 2])
    student, teacher = mask_predictor.build_models(types.SimpleNamespace(**base, dist_weight=0.5, ltp_phase="hard", ltp_temperature=0.01,
                                                                         ltp_init_threshold=0.02))
    assert isinstance(student, vit_models.VisionTransformerLTP) and isinstance(teacher, vit_models.VisionTransformerTeacher)
    assert seen["kw"] == dict(pruning_loc=[0, 2], ltp_temperature=0.01, ltp_init_threshold=0.02, ltp_phase="hard")
    assert student.ltp_phase == "hard" and not student.ltp_threshold.requires_grad
    seen.pop("teacher_checkpoint")
    student, teacher = mask_predictor.build_models(types.SimpleNamespace(**base, dist_weight=0.0))
    assert teacher is None and "teacher_checkpoint" not in seen                      # --dist-weight 0: no teacher is built
    assert (student.ltp_phase, student.ltp_temperature, student.ltp_init_threshold) == ("soft", 1e-3, 0.005)
    assert "the trunk starts from its random initialisation" in capsys.readouterr().out


def test_a_soft_phase_checkpoint_hands_its_thresholds_to_the_hard_phase(monkeypatch, tmp_path, capsys):
    import mask_predictor
    import vit_models
    monkeypatch.setattr(vit_models, "ltp_deit_tiny_patch16_224", lambda checkpoint_path=None, **kw: vit_models.VisionTransformerLTP(**MICRO, **kw))
    soft = vit_models.VisionTransformerLTP(**MICRO, pruning_loc=[0, 2])
    with torch.no_grad():
        soft.ltp_threshold.copy_(torch.tensor([0.031, 0.047]))
    torch.save({"model": soft.state_dict(), "epoch": 0}, tmp_path / "best.pt")
    torch.save(vit_models.VisionTransformerTeacher(**MICRO).state_dict(), tmp_path / "deit.pt")
    base = dict(arch="deit_tiny", method="ltp", resume=None, teacher_checkpoint=None, device=torch.device("cpu"), pruning_locs=[0, 2],
                dist_weight=0.0, ltp_phase="hard")
    hard, _ = mask_predictor.build_models(types.SimpleNamespace(**base, student_checkpoint=str(tmp_path / "best.pt")))
    assert hard.ltp_phase == "hard" and hard.ltp_threshold.tolist() == soft.ltp_threshold.tolist() and not hard.ltp_threshold.requires_grad
    assert all(torch.equal(a, b) for a, b in zip(hard.state_dict().values(), soft.state_dict().values()))
    fresh, _ = mask_predictor.build_models(types.SimpleNamespace(**base, student_checkpoint=str(tmp_path / "deit.pt")))
    assert torch.allclose(fresh.ltp_threshold, torch.tensor([0.0025, 0.005]))      # a DeiT checkpoint: the thresholds keep their initial values
    capsys.readouterr()


# ---- constructor, TrainStep, loss, checkpoints ----
def test_constructor_and_state_dict_keys():
    import vit_models
    m = vit_models.VisionTransformerLTP(**MICRO, pruning_loc=[0, 1, 2])
    assert (m.pruning_loc, m.ltp_temperature, m.ltp_init_threshold, m.ltp_phase) == ([0, 1, 2], 1e-3, 0.005, "soft") and m.grad_ready_hook is None
    assert torch.allclose(m.ltp_threshold, torch.tensor([0.005 / 3, 0.01 / 3, 0.005])) and m.ltp_threshold.requires_grad
    assert m.ltp_threshold.dtype == torch.float32 and m.ltp_threshold.dim() == 1
    teacher = vit_models.VisionTransformerTeacher(**MICRO)
    assert sorted(set(m.state_dict()) - set(teacher.state_dict())) == ["ltp_threshold"] and set(teacher.state_dict()) <= set(m.state_dict())
    result = m.load_state_dict(teacher.state_dict())                     # strict: exactly that key may be missing
    assert list(result.missing_keys) == ["ltp_threshold"] and not result.unexpected_keys
    sd = teacher.state_dict()
    sd.pop("norm.weight")
    with pytest.raises(RuntimeError, match="norm.weight"):
        m.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="nosuch"):
        m.load_state_dict(dict(teacher.state_dict(), nosuch=torch.zeros(1)))
    from d2s import engine
    assert engine._group_of("ltp_threshold", m.ltp_threshold) == "base_no_decay"          # 1-D: no weight decay, the backbone's learning rate
    assert "ltp_threshold" in engine.execution_order(m)[0]
    h = vit_models.VisionTransformerLTP(**MICRO, pruning_loc=[1], ltp_phase="hard", ltp_temperature=0.02, ltp_init_threshold=0.03)
    assert h.ltp_phase == "hard" and not h.ltp_threshold.requires_grad and h.ltp_threshold.tolist() == [pytest.approx(0.03)]
    h.set_phase("soft")
    assert h.ltp_threshold.requires_grad
    assert len(vit_models.ltp_deit_small_patch16_224().blocks) == 12 and vit_models.ltp_deit_small_patch16_224().embed_dim == 384
    assert vit_models.ltp_deit_tiny_patch16_224(pruning_loc=(2, 5), ltp_temperature=0.5).pruning_loc == [2, 5]
    for bad, match in ((dict(pruning_loc=[3]), "pruning_loc"), (dict(pruning_loc=[]), "pruning_loc"), (dict(pruning_loc=[1, 1]), "pruning_loc"),
                       (dict(pruning_loc=[0], ltp_temperature=0.0), "ltp_temperature"), (dict(pruning_loc=[0], ltp_phase="medium"), "ltp_phase"),
                       (dict(pruning_loc=[0], drop_path_rate=0.1), "drop_path_rate")):
        with pytest.raises(ValueError, match=match):
            vit_models.VisionTransformerLTP(**MICRO, **bad)


def test_train_step_refusals_come_before_the_device():
    import vit_models
    from d2s import lib, ops
    from d2s.engine import TrainStep
    args = types.SimpleNamespace(mixup=0.0)
    m = vit_models.VisionTransformerLTP(**MICRO, pruning_loc=[0, 1])
    with pytest.raises(lib.D2SError, match="graph=True.*LTP"):
        TrainStep(m, None, args, graph=True)
    with pytest.raises(ValueError, match="warmup_steps 1 with an LTP student"):
        TrainStep(m, None, args, warmup_steps=1)
    dp = vit_models.VisionTransformerLTP(**MICRO, pruning_loc=[0, 1])
    dp.drop_path_rate = 0.1                                                       # the constructor refuses it; a model altered afterwards
    with pytest.raises(lib.D2SError, match="LTP student and drop_path_rate > 0"):
        TrainStep(dp, None, args)
    with ops.gemm_mode(ops.GEMM_BF16):
        for phase in ("soft", "hard"):
            m.set_phase(phase)
            with pytest.raises(lib.D2SError, match="LTP student in the bf16 arithmetic mode"):
                TrainStep(m, None, args)
        m.eval()
        with pytest.raises(lib.D2SError, match="fp32 arithmetic modes"):
            m(torch.zeros(1, 3, 64, 64))
    with pytest.raises(lib.D2SError) as e:                                        # the message the other students reach is what it was
        TrainStep(vit_models.VisionTransformerTeacher(**MICRO), None, args)
    assert str(e.value) == "TrainStep without a teacher: only a Token Merging student trains without one"


def test_loss_defaults_and_metric_keys():
    from losses import LTPLoss
    fn = LTPLoss(types.SimpleNamespace(mixup=0.0))
    assert (fn.ltp_lambda, fn.cls_weight, fn.dist_weight) == (0.01, 1.0, 0.5)
    assert LTPLoss(types.SimpleNamespace(mixup=0.0, ltp_lambda=None)).ltp_lambda == 0.01
    fn = LTPLoss(types.SimpleNamespace(mixup=0.0, ltp_lambda=0.3, dist_weight=0.0))
    assert (fn.ltp_lambda, fn.dist_weight) == (0.3, 0.0)
    metrics = {}
    one = torch.ones(())
    fn.accumulate(metrics, (one, one, one), (2 * one, 3 * one))
    assert sorted(metrics) == ["train_avg_tokens", "train_cls_kl_loss", "train_cls_loss", "train_ltp_loss", "train_ltp_reg"]
    assert (float(metrics["train_ltp_reg"]), float(metrics["train_avg_tokens"])) == (2.0, 3.0)


def test_checkpoint_config_records_the_class_the_phase_and_the_constants():
    import vit_models
    from d2s import engine
    cfg = lambda s, **kw: engine.TrainStep.config(types.SimpleNamespace(student=s, args=types.SimpleNamespace(mask_loss_type="kl_div", **kw)))
    a = cfg(vit_models.VisionTransformerLTP(**MICRO, pruning_loc=[0, 2], ltp_temperature=0.02, ltp_phase="hard"), ltp_lambda=0.3)
    b = cfg(vit_models.VisionTransformerLTP(**MICRO, pruning_loc=[0, 2]))
    c = cfg(vit_models.VisionTransformerTeacher(**MICRO))
    assert a["model"] == "VisionTransformerLTP" and a["pruning_loc"] == [0, 2]
    assert (a["ltp_phase"], a["ltp_temperature"], a["ltp_lambda"], a["ltp_init_threshold"]) == ("hard", 0.02, 0.3, 0.005)
    assert (b["ltp_phase"], b["ltp_temperature"], b["ltp_lambda"], b["ltp_init_threshold"]) == ("soft", 1e-3, 0.01, 0.005)
    assert {k for k in a if a[k] != b[k]} == {"ltp_phase", "ltp_temperature", "ltp_lambda"}          # another phase: a resume is refused
    assert (c["ltp_phase"], c["ltp_temperature"], c["ltp_lambda"], c["ltp_init_threshold"]) == (None, None, None, None)
    assert json.loads(json.dumps(a)) == a
    old = {k: v for k, v in c.items() if not k.startswith("ltp_")}
    assert engine.checkpoint_config(old) == c and "ltp_phase" not in old          # a checkpoint written before: no such student
    assert engine.checkpoint_config(a) == a
