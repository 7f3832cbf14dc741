"""Numpy restatement of an accumulation window of the fused step (d2s.engine.TrainStep accum_steps= / clip_grad=): the combined gradient,
its scale, the clipping norm and coefficient, and the gradient AdamW sees.  Nothing here imports the package under test."""
import numpy as np

F32_EPS = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
SUMSQ_DEPTH = 10              # additions on any path of the per-chunk fp32 tree (csrc/gradaccum.hip: 2 in the thread, 6 in the wave, 2 over waves)
# sum of squares of non-negative terms: one rounding per square + SUMSQ_DEPTH additions; the double fold adds O(2^-53 n): the 1e-3 slack
SUMSQ_REL_BOUND = (SUMSQ_DEPTH + 1) * F32_EPS * (1 + 1e-3)
# sqrt halves the relative error; then two roundings (the product with the scale, the store as fp32)
NORM_REL_BOUND = (0.5 * (SUMSQ_DEPTH + 1) + 2) * F32_EPS * (1 + 1e-3)
# coef = max_norm / (norm + 1e-6) in fp32: the norm's error, one addition, one division
COEF_REL_BOUND = NORM_REL_BOUND + 2 * F32_EPS * (1 + 1e-3)


def window_sum(grads):
    """S = fl(...fl(fl(g_1 + g_2) + g_3)... + g_c): arrival order, fp32, element by element"""
    S = np.array(grads[0], dtype=np.float32, copy=True)
    for g in grads[1:]:
        S = (S + np.asarray(g, dtype=np.float32)).astype(np.float32)
    return S


def window_scale(c, world=1):
    """s = float32(1 / (c * world)), formed in double"""
    return np.float32(1.0 / (c * world))


def norm64(S, s, mask=None):
    """s * sqrt(sum S^2) in float64 over the elements selected by mask"""
    v = np.asarray(S, dtype=np.float64)
    if mask is not None:
        v = v[mask]
    return float(np.float64(s) * np.sqrt(np.sum(v * v)))


def clip_coef(total_norm, max_norm):
    """clip_grad_norm_: min(1, max_norm / (total_norm + 1e-6)), fp32 like the norm tensor it is formed from"""
    c = np.float32(max_norm) / (np.float32(total_norm) + np.float32(1e-6))
    return np.float32(1.0) if c > 1 else np.float32(c)


def effective_grad(S, s, coef=None):
    """g' = fl(S * fl(s * coef)); without clipping fl(S * s)"""
    k = np.float32(s) if coef is None else np.float32(np.float32(s) * np.float32(coef))
    return (np.asarray(S, dtype=np.float32) * k).astype(np.float32)


def chunk_desc(lr, wd, active):
    """the per-chunk descriptor table of the AdamW / accumulate / norm launches as bytes: {float lr, float wd, int active, int pad}"""
    n = len(active)
    d = np.zeros(n, dtype=[("lr", "<f4"), ("wd", "<f4"), ("active", "<i4"), ("pad", "<i4")])
    d["lr"], d["wd"], d["active"] = lr, wd, active
    return d.view(np.uint8).copy()
