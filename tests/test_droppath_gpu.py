"""Stochastic depth on the MI355X: the per-step table of draws, the row-scale epilogue of the residual GEMMs in all three arithmetic
modes, the backward's row scaling, a whole block (composite and per-op) against tests/droppath_ref.py, and the train step.

Tolerances are those of tests/test_kernels_gpu.py (test_gemm_epilogues / test_gemm_split_modes): rtol 1e-4 / atol 2e-5 for the exact and
bf16x3 arithmetic, 3e-2 / 3e-2 for bf16, atol multiplied by 1 / keep - the factor the branch, and so its error, is scaled by.

Parameter gradients are sums over all B * n rows, so their error is bounded against the float64 restatement as a full-tensor relative L2
error, the way tests/test_model_gpu.py::test_train_step_parity bounds them: no more than 4 x the error of an fp32 CPU evaluation of the
same restatement, floor 2e-4 (exact, bf16x3); for bf16 operands 3e-2, the issue's relative bound for that arithmetic.  y and dx keep the
element-wise bounds."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import droppath_ref as R
from tests.test_model_gpu import build_models, make_args, _t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("exact", "split", "bf16")


def _ops():
    from d2s import ops
    return ops


def _mode(ops, name):
    return {"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT, "bf16": ops.GEMM_BF16}[name]


def _tol(mode, keep):
    rtol, atol = (3e-2, 3e-2) if mode == "bf16" else (1e-4, 2e-5)
    return dict(rtol=rtol, atol=atol / keep)


# ---- 1. the table ----
def test_scale_table_values_rows_and_seeds():
    ops = _ops()
    rates = torch.tensor([0.0, 0.05, 0.1, 0.5, 0.0, 0.9], device=DEV)
    t = ops.drop_path_scales(rates, 128, 1234)
    torch.cuda.synchronize()
    for r, rate in enumerate(rates.cpu()):
        row = t[r].cpu()
        if rate == 0:
            assert torch.equal(row, torch.ones(128)), r
            continue
        inv = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - rate)
        assert bool(((row == 0) | (row == inv)).all()), (r, row.unique())
    assert torch.equal(t, ops.drop_path_scales(rates, 128, 1234))
    assert not torch.equal(t, ops.drop_path_scales(rates, 128, 1235))
    assert torch.equal(ops.drop_path_scales(rates, 64, 1234), t[:, :64])
    # a row is a function of (seed, rate, row index, sample): the same rows inside a longer table
    longer = ops.drop_path_scales(torch.cat([rates, rates]), 128, 1234)
    assert torch.equal(longer[:6], t)
    out = torch.full((6, 128), -1.0, device=DEV)
    assert ops.drop_path_scales(rates, 128, 1234, out=out) is out and torch.equal(out, t)


@pytest.mark.parametrize("rate", [0.05, 0.1, 0.5])
def test_scale_table_kept_count_is_binomial(rate):
    """5-sigma bound of a Binomial(N, keep) count, N = 24 * 4096 (derived, not measured), and per-row counts within 6 sigma of their own."""
    ops = _ops()
    R_, B = 24, 4096
    t = ops.drop_path_scales(torch.full((R_,), rate, device=DEV), B, 20261016)
    kept = (t > 0).sum().item()
    keep = 1.0 - float(np.float32(rate))
    N = R_ * B
    assert abs(kept - N * keep) <= 5.0 * np.sqrt(N * keep * (1 - keep)), (kept, N * keep)
    rows = (t > 0).sum(dim=1).cpu().numpy()
    assert np.all(np.abs(rows - B * keep) <= 6.0 * np.sqrt(B * keep * (1 - keep))), rows
    assert len({tuple(r.tolist()) for r in (t > 0).cpu()}) == R_, "rows must not repeat each other"


# ---- 2. the epilogue ----
EPI_SHAPES = [(197 * 3, 384, 384, 197), (99 * 5, 384, 1536, 99), (100 * 4, 384, 1536, 100), (577 * 2, 768, 3072, 577),
              (197 * 128, 384, 1536, 197), (100, 128, 4096, 50)]      # the last: small grid, long K - the split-K combine in exact mode


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,N,K,rpg", EPI_SHAPES)
def test_rowscale_epilogue(mode, M, N, K, rpg):
    ops = _ops()
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g) * 0.5
    w = torch.randn(N, K, generator=g) * 0.05
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    G = (M + rpg - 1) // rpg
    keep = 0.5
    mask = (torch.arange(G) % 2 == 0).float()          # both values inside every tile that spans two groups
    if G > 2:
        mask[1], mask[2] = 1.0, 0.0
    s = mask / keep
    if (M, N, K) == EPI_SHAPES[-1][:3]:
        assert ops.lib.query("d2s_gemm_f32_workspace_bytes", 0, M, N, K, ops.GEMM_EXACT) > 0, "expected to take the split-K path"
    ref = s.double().repeat_interleave(rpg)[:M, None] * (x.double() @ w.double().t() + b.double()) + r.double()
    with ops.gemm_mode(_mode(ops, mode)):
        y = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), epi=ops.EPI_BIAS_RESID, aux=r.to(DEV), rowscale=s.to(DEV), rows_per_group=rpg)
        plain = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), epi=ops.EPI_BIAS_RESID, aux=r.to(DEV))
        ones = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), epi=ops.EPI_BIAS_RESID, aux=r.to(DEV), rowscale=torch.ones(G, device=DEV),
                              rows_per_group=rpg)
    y, plain, ones = y.cpu(), plain.cpu(), ones.cpu()
    err = (y.double() - ref).abs().max().item()
    print(f"rowscale epilogue {mode} {M}x{N}x{K} rows/group {rpg}: max abs err {err:.3e}")
    np.testing.assert_allclose(y.numpy(), ref.float().numpy(), **_tol(mode, keep))
    dropped = s.repeat_interleave(rpg)[:M] == 0
    assert dropped.any() and (~dropped).any()
    assert torch.equal(y[dropped], r[dropped]), "a row with scale 0 is the residual, bit for bit"
    np.testing.assert_allclose(ones.numpy(), plain.numpy(), **_tol(mode, 1.0))


def test_rowscale_epilogue_scalar_store_path():
    """N not a multiple of 4: the dword epilogue (store_tile_out) instead of the LDS-staged 16-byte one."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    M, N, K, rpg = 70, 30, 64, 7
    x, w, b, r = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    s = (torch.arange(10) % 3 != 0).float() / 0.75
    ref = s.double().repeat_interleave(rpg)[:, None] * (x.double() @ w.double().t() + b.double()) + r.double()
    for mode in MODES:
        with ops.gemm_mode(_mode(ops, mode)):
            y = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), epi=ops.EPI_BIAS_RESID, aux=r.to(DEV), rowscale=s.to(DEV), rows_per_group=rpg).cpu()
        np.testing.assert_allclose(y.numpy(), ref.float().numpy(), **_tol(mode, 0.75))
        assert torch.equal(y[:rpg], r[:rpg])


def test_plain_gemm_entry_refuses_the_rowscale_code():
    ops = _ops()
    x, w, r = torch.randn(8, 16, device=DEV), torch.randn(8, 16, device=DEV), torch.randn(8, 8, device=DEV)
    out = torch.empty(8, 8, device=DEV)
    with pytest.raises(ops.lib.D2SError):
        ops.lib.call("d2s_gemm_f32", 0, x.data_ptr(), 16, w.data_ptr(), 16, out.data_ptr(), 8, 8, 8, 16, 11, None, r.data_ptr(), 8, None,
                     0, 0, 0, 0, 0, None, 0)


# ---- 3. scale_rows / drop_path_fwd ----
@pytest.mark.parametrize("M,D,rpg", [(197 * 3, 384, 197), (99 * 5 + 1, 384, 99), (7, 1536, 3), (10, 30, 4)])
def test_scale_rows_is_bit_exact(M, D, rpg):
    ops = _ops()
    g = torch.randn(M, D, generator=torch.Generator().manual_seed(M))
    G = (M + rpg - 1) // rpg
    s = torch.where(torch.arange(G) % 2 == 0, torch.tensor(1.0 / 0.9), torch.tensor(0.0))
    out = ops.scale_rows(g.to(DEV), s.to(DEV), rpg).cpu()
    assert torch.equal(out, g * s.repeat_interleave(rpg)[:M, None])


def test_drop_path_module_forward_and_backward():
    import vit_models
    ops = _ops()
    m = vit_models.DropPath(0.5).train()
    for shape in ((6, 5, 128), (6, 7)):
        x = torch.randn(*shape, device=DEV, requires_grad=True)
        torch.manual_seed(11)
        y = m(x)
        torch.manual_seed(11)
        s = m.draw(shape[0], x.device)
        assert torch.equal(y, x.detach() * s.view((-1,) + (1,) * (len(shape) - 1)))
        gy = torch.randn(*shape, device=DEV)
        y.backward(gy)
        assert torch.equal(x.grad, gy * s.view((-1,) + (1,) * (len(shape) - 1)))
    assert m.eval()(x) is x


# ---- 4. a block ----
def _block_inputs(B, n, D, hidden, seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (hidden, D), (hidden,), (D, hidden), (D,)]
    p = [torch.randn(s, generator=g) * (0.05 if len(s) == 2 else 0.1) for s in shapes]
    p[0], p[6] = p[0] + 1.0, p[6] + 1.0
    return torch.randn(B, n, D, generator=g), p, torch.randn(B, n, D, generator=g)


def _run_block(ops, x, p, gy, heads, rows, composite=True, eps=1e-6):
    from d2s import functional as DF
    ops._BLOCK_COMPOSITE = composite
    try:
        xd = x.to(DEV).requires_grad_(True)
        pd = [t.to(DEV).requires_grad_(True) for t in p]
        extra = () if rows is None else (None, rows[0], rows[1])
        y, _ = DF.run(DF.BlockFn, xd, *pd, heads, eps, False, None, *extra)
        grads = torch.autograd.grad(y, [xd] + pd, gy.to(DEV))
        ops.join_weight_grads()
        torch.cuda.synchronize()
        return y.detach().cpu(), [t.cpu() for t in grads]
    finally:
        ops._BLOCK_COMPOSITE = True


@pytest.mark.parametrize("mode", MODES)
def test_block_forward_and_all_gradients_against_float64(mode):
    ops = _ops()
    B, n, D, H, hid = 5, 99, 128, 2, 512
    x, p, gy = _block_inputs(B, n, D, hid)
    keep = 0.5
    masks = torch.tensor([[1, 0, 1, 0, 1], [1, 1, 0, 0, 1]], dtype=torch.float32)
    s = (masks / keep)
    yr, dxr, dpr = R.block_with_grads(x, p, H, 1e-6, gy, s[0], s[1])
    with ops.gemm_mode(_mode(ops, mode)):
        y, grads = _run_block(ops, x, p, gy, H, (s[0].to(DEV), s[1].to(DEV)))
    tol = _tol(mode, keep)
    np.testing.assert_allclose(y.numpy(), yr.float().numpy(), **tol)
    np.testing.assert_allclose(grads[0].numpy(), dxr.float().numpy(), **tol)
    # the same restatement evaluated in fp32 on the CPU: the yardstick's own rounding error
    x32 = x.clone().requires_grad_(True)
    p32 = [t.clone().requires_grad_(True) for t in p]
    cpu = torch.autograd.grad(R.block(x32, p32, H, 1e-6, s[0], s[1]), p32, gy)
    for name, got, want, c in zip(R.PARAM_NAMES, grads[1:], dpr, cpu):
        denom = float(want.norm())
        err = float((got.double() - want).norm()) / denom
        err_cpu = float((c.double() - want).norm()) / denom
        print(f"block {mode} d{name}: relative L2 error {err:.3e} (fp32 CPU {err_cpu:.3e})")
        assert err <= (3e-2 if mode == "bf16" else max(4.0 * err_cpu, 2e-4)), (name, err, err_cpu)


@pytest.mark.parametrize("mode", ("exact", "split"))
def test_block_composite_and_per_op_paths_are_bit_identical(mode):
    ops = _ops()
    x, p, gy = _block_inputs(4, 100, 128, 512, seed=1)
    s = torch.tensor([[2.0, 0.0, 2.0, 0.0], [0.0, 0.0, 2.0, 2.0]], device=DEV)
    with ops.gemm_mode(_mode(ops, mode)):
        a = _run_block(ops, x, p, gy, 2, (s[0], s[1]), composite=True)
        b = _run_block(ops, x, p, gy, 2, (s[0], s[1]), composite=False)
        one_row = _run_block(ops, x, p, gy, 2, (None, s[1]), composite=True), _run_block(ops, x, p, gy, 2, (None, s[1]), composite=False)
    assert torch.equal(a[0], b[0])
    for i, (ga, gb) in enumerate(zip(a[1], b[1])):
        assert torch.equal(ga, gb), i
    assert torch.equal(one_row[0][0], one_row[1][0]) and all(torch.equal(u, v) for u, v in zip(one_row[0][1], one_row[1][1]))


@pytest.mark.parametrize("mode", MODES)
def test_block_without_gradient_ignores_the_rows_and_no_rows_is_the_plain_block(mode):
    """forward-only paths are today's block whatever the rows; rows of None run the launches of a block without stochastic depth"""
    from d2s import functional as DF
    ops = _ops()
    x, p, gy = _block_inputs(3, 50, 128, 512, seed=2)
    s = torch.tensor([[2.0, 0.0, 2.0], [0.0, 2.0, 2.0]], device=DEV)
    with ops.gemm_mode(_mode(ops, mode)):
        plain = _run_block(ops, x, p, gy, 2, None)
        none_rows = _run_block(ops, x, p, gy, 2, (None, None))
        with torch.no_grad():
            pd = [t.to(DEV) for t in p]
            y_ng, _ = DF.run(DF.BlockFn, x.to(DEV), *pd, 2, 1e-6, False, None, None, s[0], s[1])
            y_plain, _ = DF.run(DF.BlockFn, x.to(DEV), *pd, 2, 1e-6, False, None)
    assert torch.equal(plain[0], none_rows[0]) and all(torch.equal(u, v) for u, v in zip(plain[1], none_rows[1]))
    assert torch.equal(y_ng, y_plain)


@pytest.mark.parametrize("mode", MODES)
def test_sample_dropped_in_both_branches_is_the_identity_and_adds_no_gradient(mode):
    ops = _ops()
    B = 4
    x, p, gy = _block_inputs(B, 99, 128, 512, seed=3)
    s = torch.tensor([[2.0, 0.0, 2.0, 2.0], [2.0, 0.0, 0.0, 2.0]], device=DEV)
    keepers = [0, 2, 3]
    with ops.gemm_mode(_mode(ops, mode)):
        y, grads = _run_block(ops, x, p, gy, 2, (s[0], s[1]))
        y3, grads3 = _run_block(ops, x[keepers], p, gy[keepers], 2, (s[0][keepers].contiguous(), s[1][keepers].contiguous()))
    assert torch.equal(y[1], x[1]), "y[b] == x[b] bit for bit"
    assert torch.equal(grads[0][1], gy[1]), "and its input gradient is the upstream gradient"
    assert torch.equal(y[keepers], y3)
    # the dropped sample's rows enter every weight-gradient sum as exact zeros; what may differ from the 3-sample run is the split-K
    # partition of the token dimension (the bound of the existing batch-independence tests)
    for name, a, b in zip(R.PARAM_NAMES, grads[1:], grads3[1:]):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, float(b.abs().max())), err_msg=name)


# ---- 5. / 6. the model and the train step ----
def _student(case, rate):
    import vit_models
    cfg = case["cfg"]
    student, teacher, _, _ = build_models(case, torch.device(DEV))
    common = dict(img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                  mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
    dp = vit_models.VisionTransformerDiffPruning(pruning_loc=list(cfg["pruning_loc"]), token_ratio=list(cfg["token_ratio"]), distill=True,
                                                 topk_selection=True, predictor_loss_type=cfg["loss_type"],
                                                 small_predictor=cfg["small_predictor"], predictor_bn=bool(cfg.get("predictor_bn")),
                                                 init_n=cfg["init_n"], drop_path_rate=rate, **common)
    dp.load_state_dict(student.state_dict(), strict=True)
    return dp.to(DEV), teacher


def test_model_rate_zero_masks_all_ones_and_eval_are_the_plain_model():
    case = cases.MODEL_CASES["micro2"]
    x = _t(cases.make_images(case)).to(DEV)
    plain, _ = _student(case, 0.0)
    dp, _ = _student(case, 0.5)
    depth = len(dp.blocks)
    plain.train(), dp.train()
    want = plain(x)[0].detach()
    dp.drop_path_masks = torch.ones(2 * depth, x.shape[0])
    rates = torch.tensor(dp._drop_path.rates)
    got = dp(x)[0].detach()
    # all kept at rate p is the branch times 1 / keep - not the plain model; with the masks set to keep (scale exactly 1) it is
    dp.drop_path_masks = (1.0 - rates)[:, None].expand(-1, x.shape[0])
    same = dp(x)[0].detach()
    assert not torch.equal(got, want)
    assert torch.equal(same, want)
    dp.drop_path_masks = None
    plain.eval(), dp.eval()
    with torch.no_grad():
        assert torch.equal(dp(x)[0], plain(x)[0])
    dp.train()
    with torch.no_grad():
        assert torch.equal(dp(x)[0], plain.train()(x)[0]), "forward-only paths ignore the rate"


def test_model_masks_follow_torch_manual_seed():
    case = cases.MODEL_CASES["micro2"]
    x = _t(cases.make_images(case)).to(DEV)
    dp, _ = _student(case, 0.5)
    dp.train()
    def run(seed):
        torch.manual_seed(seed)
        out = dp(x)[0].detach().clone()
        return out, dp._drop_path.buffers(x.shape[0], x.device)[1].clone()
    a, ta = run(1)
    b, tb = run(1)
    c, tc = run(2)
    assert torch.equal(a, b) and torch.equal(ta, tb)
    assert not torch.equal(ta, tc)
    assert torch.equal(ta[:2], torch.ones_like(ta[:2])), "block 0 has rate 0"


def _steps(case, rate, n, seed=5, resume_after=None, graph=False):
    from d2s.engine import TrainStep
    student, teacher = _student(case, rate)
    ts = TrainStep(student, teacher, make_args(case["cfg"]), warmup_steps=0, graph=graph)
    x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
    torch.manual_seed(seed)
    rec, sd = [], None
    for i in range(n):
        info = ts(x, y)
        torch.cuda.synchronize()
        rec.append((info["loss"].detach().clone(), ts.arena.params.clone()))
        if resume_after is not None and i + 1 == resume_after:
            sd = ts.state_dict(epoch=0)
    return rec, sd, ts


def test_train_step_is_reproducible_differs_from_rate_zero_and_resumes_bit_identically():
    case = cases.MODEL_CASES["micro2"]
    a, sd, _ = _steps(case, 0.1, 4, resume_after=2)
    b, _, _ = _steps(case, 0.1, 4)
    z, _, _ = _steps(case, 0.0, 4)
    for i in range(4):
        assert torch.equal(a[i][0], b[i][0]) and torch.equal(a[i][1], b[i][1]), i
    assert not torch.equal(a[3][1], z[3][1])
    # resume after step 2 in a fresh TrainStep: steps 3 and 4 are those of the uninterrupted run
    from d2s.engine import TrainStep
    from d2s import lib
    student, teacher = _student(case, 0.1)
    ts = TrainStep(student, teacher, make_args(case["cfg"]), warmup_steps=0, graph=False)
    torch.manual_seed(999)                       # the checkpoint's generator state must win
    ts.load_state_dict(sd)
    x, y = _t(cases.make_images(case)).to(DEV), _t(cases.make_labels(case)).to(DEV)
    for i in (2, 3):
        info = ts(x, y)
        torch.cuda.synchronize()
        assert torch.equal(info["loss"].detach(), a[i][0]) and torch.equal(ts.arena.params, a[i][1]), i
    # a checkpoint made at rate 0.1 is refused by a run at rate 0
    student0, teacher0 = _student(case, 0.0)
    ts0 = TrainStep(student0, teacher0, make_args(case["cfg"]), warmup_steps=0, graph=False)
    with pytest.raises(lib.D2SError, match="drop_path_rate"):
        ts0.load_state_dict(sd)


def test_graph_mode_with_a_rate_is_refused_at_construction():
    from d2s.engine import TrainStep
    from d2s import lib
    case = cases.MODEL_CASES["micro2"]
    student, teacher = _student(case, 0.1)
    with pytest.raises(lib.D2SError, match="drop_path_rate"):
        TrainStep(student, teacher, make_args(case["cfg"]), graph=True)
    student0, teacher0 = _student(case, 0.0)
    TrainStep(student0, teacher0, make_args(case["cfg"]), graph=True)


def _fixture_student(g, prefix):
    """the student of a section of tests/golden/droppath_micro.npz at the fixture's rate, its masks injected -> (student, x, case, tag)"""
    import vit_models
    from d2s import synth
    case, tag, masks, rate = R.fixture_case(g, prefix)
    cfg = case["cfg"]
    student = vit_models.VisionTransformerDiffPruning(
        img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
        mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"], pruning_loc=list(cfg["pruning_loc"]),
        token_ratio=list(cfg["token_ratio"]), distill=True, topk_selection=True, predictor_loss_type=cfg["loss_type"],
        small_predictor=cfg["small_predictor"], init_n=cfg["init_n"], drop_path_rate=rate,
        patch_score_threshold=case["threshold"] if prefix else None)
    student.load_state_dict({k: _t(v) for k, v in cases.make_weights(case)[0].items()}, strict=True)
    student = student.to(DEV).train()
    student.drop_path_masks = masks
    x = _t(synth.images(case["batch"], 3, cfg["img_size"], seed=case["seed"])).to(DEV)
    return student, x, case, tag


@pytest.mark.parametrize("prefix", ["", "thr_"])
def test_student_with_the_fixture_masks_matches_the_reference_run(prefix):
    """The student with the masks the reference drew (tests/golden/droppath_micro.npz) injected: "" = micro1 with token pruning, batch 4;
    "thr_" = policy training (patch_score_threshold set, the keep mask really masks keys) - the path of _forward_threshold with rows.
    Selection exact; logits, features, pred_logits and the gradients of the fixture's linear probe within the tolerances
    tests/test_model_gpu.py / tests/test_threshold_gpu.py apply to these cases against their rate-0 fixtures; the full gradient tensors
    against tests/droppath_ref.py in float64, no worse than 4 x the fp32 CPU evaluation of the same restatement (floor 2e-4)."""
    g = cases.load_golden("droppath_micro")
    student, x, case, tag = _fixture_student(g, prefix)
    thr = bool(prefix)
    logits, features, pred_logits, sel = student(x)
    if thr:
        pred_logits, sel = pred_logits[-1:], sel[-1:]
    for i, k in enumerate(sel):
        np.testing.assert_array_equal(k.cpu().numpy().astype(np.float64), g[f"{prefix}kept_{i}"].astype(np.float64))
        np.testing.assert_allclose(pred_logits[i].detach().cpu().numpy(), g[f"{prefix}pred_logits_{i}"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), g[prefix + "logits"], rtol=1e-4, atol=2e-5)
    assert list(features.shape) == g[prefix + "features_shape"].tolist()
    np.testing.assert_allclose(features[:, :4, :16].detach().cpu().numpy(), g[prefix + "features_slice"], rtol=1e-4, atol=3e-5)
    np.testing.assert_allclose(features.detach().double().sum(dim=(1, 2)).cpu().numpy(), g[prefix + "features_sum"], rtol=1e-4, atol=1e-2)
    loss = R.probe_loss(tag, case["seed"], logits.cpu(), features.cpu(), [p_.cpu() for p_ in pred_logits])
    np.testing.assert_allclose(float(loss), float(g[prefix + "probe_loss"]), rtol=1e-4, atol=2e-5)
    loss.backward()
    from d2s import ops
    ops.join_weight_grads()
    torch.cuda.synchronize()
    ref64 = R.run_fixture_case(g, prefix, torch.float64)
    ref32 = R.run_fixture_case(g, prefix, torch.float32)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), ref64["logits"].float().numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(features.detach().cpu().numpy(), ref64["features"].float().numpy(), rtol=1e-4, atol=3e-5)
    params = dict(student.named_parameters())
    worst = 0.0
    for n, ref_norm, ref_head in zip([str(v) for v in g[prefix + "grad_names"]], g[prefix + "grad_norms"], g[prefix + "grad_heads"]):
        pg = params[n].grad
        if ref_norm < 0:
            assert pg is None or float(pg.abs().max()) == 0.0, n
            continue
        assert pg is not None, n
        gf = pg.detach().flatten().cpu()
        np.testing.assert_allclose(float(gf.double().norm()), ref_norm, rtol=2e-3 if thr else 1e-3, atol=1e-6, err_msg=n)
        m = min(8, gf.numel())
        np.testing.assert_allclose(gf[:m].numpy(), ref_head[:m], rtol=5e-3,
                                   atol=(5e-3 if thr else 5e-4) * float(np.abs(ref_head[:m]).max()) + 2e-6, err_msg=n)
        g64 = ref64["grads"][n].flatten()
        denom = float(g64.norm())
        if denom > 1e-6:
            err_hip = float((gf.double() - g64).norm()) / denom
            err_cpu = float((ref32["grads"][n].flatten().double() - g64).norm()) / denom
            assert err_hip <= max(4.0 * err_cpu, 2e-4), (n, err_hip, err_cpu)
            worst = max(worst, err_hip)
    print(f"[droppath {tag}] worst relative gradient error vs the float64 restatement: {worst:.2e}")


def test_policy_train_step_with_injected_masks_runs_the_threshold_path():
    """TrainStep on the dynamic-keep-ratio case at rate 0.5 with the fixture's masks: the step is reproducible, its student logits are
    those of the model-level forward checked above, and it differs from the step without stochastic depth."""
    from d2s.engine import TrainStep
    from tests.test_threshold_gpu import build_threshold_models
    g = cases.load_golden("droppath_micro")
    case = cases.THRESHOLD_CASES["micro_thr1"]
    y = _t(cases.make_labels(case)).to(DEV)
    recs = []
    for rate_on in (True, True, False):
        student, x, _, _ = _fixture_student(g, "thr_")
        _, teacher, _, _ = build_threshold_models(case, torch.device(DEV))
        if not rate_on:
            student.drop_path_masks = torch.from_numpy(1.0 - g["thr_rates"]).float()[:, None].expand(-1, x.shape[0])      # every scale exactly 1
        args = make_args(case["cfg"])
        args.patch_score_threshold = case["threshold"]
        ts = TrainStep(student, teacher, args, warmup_steps=0, graph=False)
        info = ts(x, y)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(info["loss"]))
        recs.append((info["loss"].detach().clone(), info["logits_s"].detach().clone(), ts.arena.params.clone()))
    assert all(torch.equal(a, b) for a, b in zip(recs[0], recs[1]))
    np.testing.assert_allclose(recs[0][1].cpu().numpy(), g["thr_logits"], rtol=1e-4, atol=2e-5)
    assert not torch.equal(recs[0][2], recs[2][2])


# ---- 7. the entry script ----
@pytest.mark.parametrize("extra", [[], ["--torch-optim"]])
def test_mask_predictor_cli_with_drop_path(capsys, extra):
    import re
    import mask_predictor
    best = mask_predictor.main(["--arch", "deit_tiny", "--pruning-locs", "3", "--keep-ratios", "0.5", "--epochs", "2", "--warmup-steps", "1",
                                "--batch-size", "4", "--steps-per-epoch", "3", "--val-steps", "1", "--topk-selection", "--drop-path", "0.1"] + extra)
    out = capsys.readouterr().out
    assert 0.0 <= best <= 1.0
    assert "drop_path: 0.1" in out and "Epoch 2/2" in out and "Training complete" in out
    losses = [float(v) for v in re.findall(r"train loss: ([-+0-9.einfa]+)", out)]
    assert losses and all(np.isfinite(losses)), losses
