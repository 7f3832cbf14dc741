"""Pruning and squeezing at a pruning stage (squeeze_dropped), restated in plain torch in the dtype of its input.  This is the definition
(DESIGN.md section 23), the build's own: the reference has no counterpart.

A stage receives x [B, n, D] - row 0 CLS, then T = n - 1 scored tokens - and the ascending stage-relative id lists kept [B, k] /
dropped [B, m], m = T - k, of the selector.  With r_t = 1 / ||x[:, 1 + t]|| (0 for a zero norm):

    c_ij     = <x[:, 1 + dropped_i], x[:, 1 + kept_j]> r_dropped_i r_kept_j
    sim_i    = max_j c_ij,      dst_i = the lowest j that attains it            (the plan; dst is a POSITION in kept)
    w_i      = exp(sim_i),      E = exp(1)
    Z_j      = E + sum_{i: dst_i = j} w_i
    y[:, 0]  = x[:, 0]
    y[:, 1 + j] = (E x[:, 1 + kept_j] + sum_{i: dst_i = j} w_i x[:, 1 + dropped_i]) / Z_j

The plan is a constant of the backward; the ids get no gradient.  An entry with dst < 0 is in no sum."""
import math

import torch
import torch.nn.functional as F

from oracle import d2s_oracle as O

E = math.e


def rows(x, ids):
    """x [B, n, D] (CLS first), ids [B, q] stage-relative -> x[:, 1 + ids] [B, q, D]"""
    return torch.gather(x[:, 1:], 1, ids[:, :, None].expand(-1, -1, x.shape[-1]))


def cosines(x, kept, dropped):
    """-> c [B, m, k] in the dtype of x"""
    norm = x[:, 1:].pow(2).sum(-1).sqrt()
    r = torch.where(norm > 0, 1.0 / torch.where(norm > 0, norm, torch.ones_like(norm)), torch.zeros_like(norm))
    a, b = rows(x, dropped) * torch.gather(r, 1, dropped)[:, :, None], rows(x, kept) * torch.gather(r, 1, kept)[:, :, None]
    return a @ b.transpose(1, 2)


def match(x, kept, dropped):
    """-> (dst [B, m] int32, sim [B, m]): the first (lowest) position of the largest cosine, and that cosine"""
    c = cosines(x, kept, dropped)
    if c.shape[1] == 0:
        return torch.zeros(c.shape[:2], dtype=torch.int32), c.new_zeros(c.shape[:2])
    sim = c.max(dim=2)[0]
    first = (c == sim[:, :, None]).to(torch.int64).argmax(dim=2)          # argmax of a 0/1 tensor: the first 1
    return first.to(torch.int32), sim


def weights(dst, sim, k, dtype):
    """-> (w [B, m] = exp(sim) where dst is a position, 0 elsewhere; Z [B, k]; the destination index with invalid entries at 0)"""
    ok = (dst >= 0) & (dst < k)
    w = torch.where(ok, torch.exp(sim.to(dtype)), torch.zeros((), dtype=dtype))
    d = torch.where(ok, dst.long(), torch.zeros((), dtype=torch.int64))
    Z = torch.full((dst.shape[0], k), E, dtype=dtype).scatter_add(1, d, w)
    return w, Z, d


def merge(x, kept, dropped, dst, sim):
    """-> (y [B, k + 1, D], Z [B, k]) in the dtype of x; differentiable in x; a kept row without a source is x's row itself"""
    B, n, D = x.shape
    k = kept.shape[1]
    w, Z, d = weights(dst, sim, k, x.dtype)
    own = rows(x, kept)
    num = (E * own).scatter_add(1, d[:, :, None].expand(-1, -1, D), w[:, :, None] * rows(x, dropped))
    hit = torch.zeros((B, k), dtype=torch.int64).scatter_add(1, d, (w > 0).long()) > 0
    return torch.cat([x[:, :1], torch.where(hit[:, :, None], num / Z[:, :, None], own)], dim=1), Z


def merge_backward(g, kept, dropped, dst, sim, n):
    """The backward in closed form, g [B, k + 1, D] -> dx [B, n, D] in the dtype of g: dx[:, 0] = g[:, 0]; a kept token at position j gets
    (E / Z_j) g[:, 1 + j] (exactly g[:, 1 + j] without a source); a dropped token gets (w_i / Z_dst) g[:, 1 + dst_i]"""
    B, k1, D = g.shape
    k = k1 - 1
    w, Z, d = weights(dst, sim, k, g.dtype)
    hit = torch.zeros((B, k), dtype=torch.int64).scatter_add(1, d, (w > 0).long()) > 0
    ck = torch.where(hit, E / Z, torch.ones_like(Z))
    cd = w / torch.gather(Z, 1, d)
    dx = torch.zeros((B, n, D), dtype=g.dtype)
    dx[:, 0] = g[:, 0]
    tok = dx[:, 1:]
    tok.scatter_(1, kept[:, :, None].expand(-1, -1, D), ck[:, :, None] * g[:, 1:])
    tok.scatter_(1, dropped[:, :, None].expand(-1, -1, D), cd[:, :, None] * torch.gather(g[:, 1:], 1, d[:, :, None].expand(-1, -1, D)))
    return dx


def merge_autograd(x, kept, dropped, dst, sim, g):
    """-> (y, Z, dx) with dx by autograd through merge, the plan held constant"""
    x = x.detach().clone().requires_grad_(True)
    y, Z = merge(x, kept, dropped, dst, sim)
    (dx,) = torch.autograd.grad(y, x, g.to(y.dtype))
    return y.detach(), Z.detach(), dx


def complement(kept, T):
    """the ascending ids of [0, T) that are not in kept [B, k] -> [B, T - k]"""
    mask = torch.ones((kept.shape[0], T), dtype=torch.bool).scatter(1, kept, torch.zeros(kept.shape, dtype=torch.bool))
    return torch.nonzero(mask)[:, 1].reshape(kept.shape[0], T - kept.shape[1])


def student_forward(sd, images, cfg, kept_ids, plans=None, squeeze=True):
    """The fixed-ratio student (oracle.student_forward's loop) in the dtype of sd, with the selection replayed from kept_ids (one [B, k_s]
    per stage - the score predictor or the CLS attention that chose them is not evaluated: no gradient passes through a hard selection)
    and every stage squeezing its dropped tokens, by the replayed plans or, with plans None, by this file's own match.
    squeeze False: plain pruning.  -> (logits, [rows of the sequence after each stage], [(dst, sim) per stage])"""
    x = O.embed_tokens(sd, images, cfg)
    lengths, used, stage = [], [], 0
    for i in range(cfg["depth"]):
        if i in cfg["pruning_loc"]:
            kept = kept_ids[stage].long()
            if squeeze and kept.shape[1] > 0:
                dropped = complement(kept, x.shape[1] - 1)
                dst, sim = match(x.detach(), kept, dropped) if plans is None else plans[stage]
                used.append((dst, sim))
                x, _ = merge(x, kept, dropped, dst, sim.to(x.dtype))
            else:
                x = O.gather_pack(x, kept)
            lengths.append(x.shape[1])
            stage += 1
        x, _ = O.block(sd, i, x, cfg)
    x = F.layer_norm(x, (cfg["dim"],), sd["norm.weight"], sd["norm.bias"], cfg["ln_eps"])
    return F.linear(x[:, 0], sd["head.weight"], sd["head.bias"]), lengths, used


def model_grads(state_dict, images, cfg, kept_ids, plans):
    """student_forward in float64 with ids and plans replayed -> (logits, {name: d logits.sum() / d parameter or None})"""
    sd = {k: torch.as_tensor(v).double().clone().requires_grad_(True) for k, v in state_dict.items()}
    logits, _, _ = student_forward(sd, torch.as_tensor(images).double(), cfg, kept_ids, plans)
    names = list(sd)
    grads = torch.autograd.grad(logits.sum(), [sd[k] for k in names], allow_unused=True)
    return logits.detach(), dict(zip(names, grads))


# ---- the inputs the GPU tests run the kernels on; the CPU tests qualify the very same tensors ----
# (B, T, k, D): one kept and one dropped token / odd sizes inside one tile / the micro students' stage (an odd batch) / a 17-row sequence:
# two 16-row workgroups of the backward / one dropped token, a full 32-column tile of kept ones / DeiT-S stage 1 at keep 0.7 (k > 128: a
# wave of the match takes a second tile step) and at keep 0.5 (four 32-row tiles of the dropped list, the last one partial) / 384 x 384
# inputs, n = 577
SHAPES = [(2, 2, 1, 64), (2, 5, 2, 64), (3, 16, 9, 128), (2, 17, 8, 192), (2, 33, 32, 128), (2, 196, 137, 384), (2, 196, 98, 384),
          (1, 576, 288, 192)]
# seed of each shape's input: the first for which every dropped token's best cosine leads its second best by margin(D) (found on the
# CPU with find_seed, fixed here; tests/test_squeeze_cpu.py asserts the margin on every dropped token)
SEEDS = {(2, 2, 1, 64): 0, (2, 5, 2, 64): 0, (3, 16, 9, 128): 0, (2, 17, 8, 192): 0, (2, 33, 32, 128): 0, (2, 196, 137, 384): 0,
         (2, 196, 98, 384): 1, (1, 576, 288, 192): 2}


def inputs(shape):
    return make_inputs(*shape, SEEDS[tuple(shape)])


def margin(D):
    """4 x the fp32 worst case of one emitted cosine, (2 D + 8) 2^-24: a D-long dot of two unit vectors (sum |a_i b_i| <= 1: D roundings)
    and the two norms (D / 2 each), with 8 for the square roots, reciprocals and products"""
    return 4.0 * (2 * D + 8) * 2.0 ** -24


def make_inputs(B, T, k, D, seed):
    """x [B, T + 1, D]: tokens drawn from an 8-dimensional subspace plus 10 % noise, so that the cosines spread over (-1, 1) the way
    those of token features do and not over the +- 1 / sqrt(D) of white noise; kept / dropped a seeded random split, each ascending;
    g [B, k + 1, D]"""
    gen = torch.Generator().manual_seed(1_000_003 * seed + 7919 * T + 31 * k + D)
    x = torch.randn((B, T + 1, 8), generator=gen) @ torch.randn((8, D), generator=gen) + 0.1 * torch.randn((B, T + 1, D), generator=gen)
    order = torch.stack([torch.randperm(T, generator=gen) for _ in range(B)])
    kept, dropped = torch.sort(order[:, :k], dim=1)[0].contiguous(), torch.sort(order[:, k:], dim=1)[0].contiguous()
    g = torch.randn((B, k + 1, D), generator=gen)
    return x, kept, dropped, g


def gaps(x, kept, dropped):
    """float64 gap between the best and the second-best cosine of every dropped token [B, m] (inf with a single kept token)"""
    c = cosines(x.double(), kept, dropped)
    if c.shape[2] < 2:
        return torch.full(c.shape[:2], float("inf"), dtype=torch.float64)
    top = c.topk(2, dim=2)[0]
    return top[:, :, 0] - top[:, :, 1]


def find_seed(B, T, k, D, tries=200):
    for seed in range(tries):
        x, kept, dropped, _ = make_inputs(B, T, k, D, seed)
        if float(gaps(x, kept, dropped).min()) >= margin(D):
            return seed
    raise AssertionError(f"no seed below {tries} separates every match of {(B, T, k, D)}")


def duplicate_inputs(D=128, T=40, k=20, seed=3):
    """make_inputs with kept positions 4 and 11 made bit-identical rows and dropped tokens 0 and 1 placed right next to them (the shared
    row plus 1 % noise): exact ties by construction, to be resolved to position 4.  -> (x, kept, dropped, the two dropped positions)"""
    x, kept, dropped, _ = make_inputs(1, T, k, D, seed)
    gen = torch.Generator().manual_seed(99)
    x[0, 1 + kept[0, 11]] = x[0, 1 + kept[0, 4]]
    for i in (0, 1):
        x[0, 1 + dropped[0, i]] = x[0, 1 + kept[0, 4]] + 0.01 * torch.randn((D,), generator=gen)
    return x, kept, dropped, (0, 1)


# ---- the merge's error bound and an emulation of the kernel's roundings (shared by the GPU test and the CPU test that validates it) ----
U = 2.0 ** -24
# y_c of a row with s sources is N_c / Z, N_c = E x_c + sum_i w_i x_ic.  To first order in u = 2^-24, relative to M_c = (E |x_c| + sum_i w_i
# |x_ic|) / Z:
#   s + 1   the numerator chain: one rounding for the product E x_c, one per fused multiply-add (each at most u times a partial sum of
#           |terms|, so at most u Z M_c)
#   2       the weights inside N: expf is accurate to 1 ulp = 2 u on every w_i; the fp32 constant E is within u of e
#   4       Z: the same weight errors (2), and the compensated sum's own error, 2 u whatever s is (the roundings of the additions are
#           carried along and added back: what remains is the rounding of the final sum and of the carried term)
#   1       the one division
# so |y_c - ref| <= (s + 8) u M_c: C_MERGE = 8.  Z itself: |Z - ref| <= 4 u Z, inside the same rule (s + 8) u Z.
C_MERGE = 8
# a dx row is fl(fl(a / Z) g) with a = w_i (expf: 2 u) or E (u) and Z the forward's (4 u, above): 6 u on the operands, one rounding for
# the ratio and one for the product
C_BWD = 8


def merge_bounds(x, kept, dropped, dst, sim):
    """float64 inputs -> (bound on |y[:, 1:] - ref| [B, k, D], bound on |Z - ref| [B, k], sources per kept row [B, k])"""
    k, D = kept.shape[1], x.shape[-1]
    w, Z, d = weights(dst, sim, k, torch.float64)
    s = torch.zeros(kept.shape, dtype=torch.int64).scatter_add(1, d, (w > 0).long())
    mag = (E * rows(x, kept).abs()).scatter_add(1, d[:, :, None].expand(-1, -1, D), w[:, :, None] * rows(x, dropped).abs()) / Z[:, :, None]
    units = (s + C_MERGE).double() * U
    return units[:, :, None] * mag, units * Z, s


def emulate_merge(x, kept, dropped, dst, sim, expf_ulps=0):
    """The forward kernel's arithmetic on fp32 inputs, rounding for rounding (numpy float32; a fused multiply-add is the float64 value of
    w x + acc, exact for fp32 operands up to float64's own rounding, rounded once to fp32): w_i = expf(sim_i), taken as the correctly
    rounded value moved by expf_ulps units in the last place; acc = E x, then one fma per source in ascending i; Z by Fast2Sum with the
    carried term added at the end; y = acc / Z.  -> (y [B, k + 1, D], Z [B, k]) as float32 tensors"""
    import numpy as np
    f32, f64 = np.float32, np.float64
    xn, simn = x.numpy().astype(f32), sim.numpy().astype(f32)
    B, n, D = xn.shape
    k = kept.shape[1]
    E32 = f32(2.71828174591064453125)
    w = np.exp(simn.astype(f64)).astype(f32)
    for _ in range(abs(expf_ulps)):
        w = np.nextafter(w, f32(np.inf if expf_ulps > 0 else -np.inf))
    y, Z = np.empty((B, k + 1, D), dtype=f32), np.full((B, k), E32, dtype=f32)
    y[:, 0] = xn[:, 0]
    for b in range(B):
        for j in range(k):
            own = xn[b, 1 + int(kept[b, j])]
            src = [i for i in range(dst.shape[1]) if int(dst[b, i]) == j]
            if not src:
                y[b, 1 + j] = own
                continue
            acc, zs, zc = E32 * own, E32, f32(0)
            for i in src:
                t = f32(zs + w[b, i])
                zc = f32(zc + f32(w[b, i] - f32(t - zs)))
                zs = t
                acc = (f64(w[b, i]) * xn[b, 1 + int(dropped[b, i])].astype(f64) + acc.astype(f64)).astype(f32)
            zs = f32(zs + zc)
            Z[b, j] = zs
            y[b, 1 + j] = acc / zs
    return torch.from_numpy(y), torch.from_numpy(Z)
