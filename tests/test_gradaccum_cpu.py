"""CPU tier of gradient accumulation and global-norm clipping: the numpy restatement of the window (tests/gradaccum_ref.py) against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, the two flags, their validation, and the C ABI of the three entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import cases, gradaccum_ref as R

REPO = cases.REPO


def _model(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.GELU(), torch.nn.Linear(16, 5))


@pytest.mark.parametrize("c,max_norm", [(2, 0.05), (3, 0.05), (3, 1e30), (1, 0.05)])
def test_window_restatement_matches_torch_clip_and_adamw(c, max_norm):
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(8, 12, generator=g) for _ in range(c)]
    ys = [torch.randint(0, 5, (8,), generator=g) for _ in range(c)]
    a, b = _model(3), _model(3)
    opt_a = torch.optim.AdamW(a.parameters(), lr=1e-3, weight_decay=0.05)
    opt_b = torch.optim.AdamW(b.parameters(), lr=1e-3, weight_decay=0.05)
    # torch: backward into .grad over the window, grad.mul_(s), clip_grad_norm_, step
    micro = []
    for x, y in zip(xs, ys):
        torch.nn.functional.cross_entropy(a(x), y).backward()
        gi = torch.autograd.grad(torch.nn.functional.cross_entropy(a(x), y), list(a.parameters()))
        micro.append(np.concatenate([t.numpy().ravel() for t in gi]))
    s = R.window_scale(c)
    S_torch = np.concatenate([p.grad.numpy().ravel() for p in a.parameters()])
    S = R.window_sum(micro)
    np.testing.assert_array_equal(S, S_torch)            # arrival-order fp32 sums: AccumulateGrad adds the same way
    for p in a.parameters():
        p.grad.mul_(float(s))
    norm_torch = float(torch.nn.utils.clip_grad_norm_(list(a.parameters()), max_norm))
    opt_a.step()
    norm = R.norm64(S, s)
    coef = R.clip_coef(norm, max_norm)
    np.testing.assert_allclose(norm, norm_torch, rtol=1e-6)
    assert (coef < 1) == (norm_torch > max_norm)
    geff = R.effective_grad(S, s, coef)
    g_torch = np.concatenate([p.grad.numpy().ravel() for p in a.parameters()])
    if c in (1, 2):      # s a power of two: fl(fl(S s) coef) and fl(S fl(s coef)) round once, identically
        np.testing.assert_array_equal(geff, g_torch)
    np.testing.assert_allclose(geff, g_torch, rtol=4 * 2 * R.F32_EPS, atol=1e-30)
    off = 0
    for p in b.parameters():
        p.grad = torch.from_numpy(geff[off:off + p.numel()].reshape(p.shape).copy())
        off += p.numel()
    opt_b.step()
    for p, q in zip(a.parameters(), b.parameters()):
        np.testing.assert_allclose(q.detach().numpy(), p.detach().numpy(), rtol=1e-6, atol=1e-8)


def test_window_sum_is_ordered_fp32():
    g = [np.float32([1.0]), np.float32([2.0 ** -24]), np.float32([2.0 ** -24])]
    assert R.window_sum(g)[0] == np.float32(1.0)                       # each tiny term is absorbed in turn
    assert R.window_sum(g[::-1])[0] == np.float32(1.0) + np.float32(2.0 ** -23)
    assert R.window_scale(3, 2) == np.float32(1.0 / 6.0) and R.window_scale(4) == np.float32(0.25)


def test_flags_parse_with_their_defaults():
    import utils
    a = utils.parse_args([])
    assert a.accum_steps == 1 and a.clip_grad is None
    a = utils.parse_args(["--accum-steps", "4", "--clip-grad", "1.5"])
    assert a.accum_steps == 4 and isinstance(a.accum_steps, int) and a.clip_grad == 1.5


@pytest.mark.parametrize("argv", [["--accum-steps", "0"], ["--accum-steps", "-2"], ["--clip-grad", "0"], ["--clip-grad", "-1"]])
def test_check_supported_rejects_bad_values(argv):
    import utils
    import mask_predictor
    mask_predictor.check_supported(utils.parse_args(["--accum-steps", "2", "--clip-grad", "1.0"]))
    with pytest.raises(SystemExit) as e:
        mask_predictor.check_supported(utils.parse_args(argv))
    assert "not on the accelerated path" in str(e.value) and argv[0] in str(e.value)


def test_header_and_binding_table_declare_the_entry_points():
    from d2s import lib
    header = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "d2s_hip.h")).read())
    for decl in ("int d2s_grad_accumulate(float* acc, float* g, const void* chunk_desc, int n_chunks, int mode, d2s_stream_t stream);",
                 "int d2s_grad_clip_coef(const float* g, const void* chunk_desc, int n_chunks, float scale, float max_norm, float* partials, "
                 "float* out, d2s_stream_t stream);",
                 "int d2s_adamw_step_clip(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const void* chunk_desc, "
                 "int n_chunks, float beta1, float beta2, float eps, int step, float grad_scale, int* chunk_steps, float* ema, "
                 "float ema_decay, const float* coef_dev, d2s_stream_t stream);",
                 "int d2s_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const void* chunk_desc, "
                 "int n_chunks, float beta1, float beta2, float eps, int step, float grad_scale, int* chunk_steps, d2s_stream_t stream);",
                 "int d2s_adamw_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const void* chunk_desc, "
                 "int n_chunks, float beta1, float beta2, float eps, int step, float grad_scale, int* chunk_steps, float* ema, "
                 "float ema_decay, d2s_stream_t stream);"):
        assert decl in header, decl
    for name in ("d2s_grad_accumulate", "d2s_grad_clip_coef", "d2s_adamw_step_clip"):
        assert name in lib.symbols("d2s_hip.h")
    handle = lib.load()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert handle.d2s_grad_accumulate.argtypes == [P, P, P, I, I, P]
    assert handle.d2s_grad_clip_coef.argtypes == [P, P, I, F, F, P, P, P]
    assert handle.d2s_adamw_step_clip.argtypes == [P, P, P, P, P, I, F, F, F, I, F, P, P, F, P, P]
    assert handle.d2s_adamw_step.argtypes == [P, P, P, P, P, I, F, F, F, I, F, P, P], "the plain entry keeps its signature"
    assert handle.d2s_adamw_step_ema.argtypes == [P, P, P, P, P, I, F, F, F, I, F, P, P, F, P], "the EMA entry keeps its signature"
    # null pointers and bad modes are argument errors, reported before anything is launched
    assert handle.d2s_grad_accumulate(None, None, None, 4, 0, None) == -1
    assert handle.d2s_grad_clip_coef(None, None, 4, 1.0, 1.0, None, None, None) == -1


def test_reference_bounds_follow_from_the_stated_depth():
    src = open(os.path.join(REPO, "dense2sparse-vit_amd", "csrc", "gradaccum.hip")).read()
    assert f"L = {R.SUMSQ_DEPTH} additions" in src, "the kernel states the depth of its fp32 tree; the test bounds are derived from it"
    assert R.SUMSQ_REL_BOUND < 12 * R.F32_EPS and R.NORM_REL_BOUND < 8 * R.F32_EPS
