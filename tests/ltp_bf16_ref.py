"""Float64 restatement of the LTP score on the bf16 data path ("In the bf16 arithmetic mode"): the quantity of
tests/ltp_ref.py on the operands the bf16 kernels multiply - q as it lies in the bf16 qkv, k as bf16(fp32(k) * scale), the scale inside
the rounded key - and the soft model with a stage's scores handed in as constants.  Nothing here imports the package; every result is
float64."""
import torch

from tests import ltp_ref as R


def make_qkv(rows, H, seed, gain=1.4):
    """tests/test_ltp_cpu.py's make_qkv on the bf16 grid: qkv [rows, 3, H, 64] float64 holding bf16 values, max |S| at about 5-10"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((rows, 3, H, 64), generator=g, dtype=torch.float64)
    qkv[:, :2] *= gain
    return qkv.float().bfloat16().double()


def round_operands(qkv, scale):
    """qkv [rows, 3, H, 64] float64 holding bf16 values -> (q, ks) [rows, H, 64] float64: q as it is, ks = bf16(fp32(k) * fp32(scale)),
    the kernel's two roundings in the kernel's order"""
    q, k = qkv[:, 0], qkv[:, 1]
    assert torch.equal(q.float().bfloat16().double(), q) and torch.equal(k.float().bfloat16().double(), k), "operands off the bf16 grid"
    ks = (k.float() * torch.tensor(scale, dtype=torch.float32)).bfloat16().double()
    return q, ks


def _scores(q, ks, h):
    """S [n, n] of head h from the rounded operands of one image; the scale is inside ks"""
    return q[:, h] @ ks[:, h].T


def stats_plain(qkv, B, n, H, scale):
    """-> lse [B, H, n] of the plain softmax on the rounded operands"""
    q, ks = round_operands(qkv, scale)
    q, ks = q.reshape(B, n, H, 64), ks.reshape(B, n, H, 64)
    return torch.stack([torch.stack([R.softmax_rows(_scores(q[b], ks[b], h))[1] for h in range(H)]) for b in range(B)])


def stats_policy(qkv, policy, B, n, H, scale, eps):
    """-> (lse, cinv) [B, H, n] of the policy softmax on the rounded operands"""
    q, ks = round_operands(qkv, scale)
    q, ks = q.reshape(B, n, H, 64), ks.reshape(B, n, H, 64)
    lse, cinv = torch.zeros((B, H, n), dtype=torch.float64), torch.zeros((B, H, n), dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            _, lse[b, h], cinv[b, h] = R.policy_softmax_rows(_scores(q[b], ks[b], h), policy[b], eps)
    return lse, cinv


def stats_varlen(qkv, lens, H, scale):
    """-> lse [H, total], the layout of the varlen attention"""
    total = sum(lens)
    lse, r0 = torch.zeros((H, total), dtype=torch.float64), 0
    for n in lens:
        lse[:, r0:r0 + n] = stats_plain(qkv[r0:r0 + n], 1, n, H, scale)[0]
        r0 += n
    return lse


def score_from_stats(qkv, B, n, H, scale, lse, policy=None, cinv=None):
    """The score from given statistics (lse and cinv [B, H, n], float64 or the GPU's own): s[b, j] = sum_h sum_i w_i (exp(S_ij - lse_i)
    mk_ij + cinv_i) / (H sum_i w_i), w = 1 and mk = 1, cinv = 0 without a policy -> [B, n]"""
    q, ks = round_operands(qkv, scale)
    q, ks = q.reshape(B, n, H, 64), ks.reshape(B, n, H, 64)
    out = torch.zeros((B, n), dtype=torch.float64)
    for b in range(B):
        w = torch.ones(n, dtype=torch.float64) if policy is None else policy[b].double()
        for h in range(H):
            P = torch.exp(_scores(q[b], ks[b], h) - lse[b, h].double()[:, None])
            if policy is not None:
                mk = w[None, :].repeat(n, 1)
                mk[torch.arange(n), torch.arange(n)] = 1.0
                P = P * mk + cinv[b, h].double()[:, None]
            out[b] += (w[:, None] * P).sum(dim=0)
        out[b] /= H * w.sum()
    return out


def score_plain(qkv, B, n, H, scale):
    return score_from_stats(qkv, B, n, H, scale, stats_plain(qkv, B, n, H, scale))


def score_policy(qkv, policy, B, n, H, scale, eps):
    lse, cinv = stats_policy(qkv, policy, B, n, H, scale, eps)
    return score_from_stats(qkv, B, n, H, scale, lse, policy, cinv)


def score_varlen(qkv, lens, H, scale, lse=None):
    """qkv [total, 3, H, 64] packed -> s [total]; lse [H, total]: given statistics instead of the restatement's own"""
    out, r0 = torch.zeros((qkv.shape[0],), dtype=torch.float64), 0
    for n in lens:
        one = qkv[r0:r0 + n]
        st = stats_plain(one, 1, n, H, scale) if lse is None else lse[:, r0:r0 + n].double()[None]
        out[r0:r0 + n] = score_from_stats(one, 1, n, H, scale, st)[0]
        r0 += n
    return out


def model_soft_given(sd, images, cfg, locs, theta, tau, scores, eps=1e-6, dtype=torch.float64):
    """tests/ltp_ref.py's model_soft with every stage's score a given constant (scores: per stage [B, N]) instead of the restatement's own
    column means - by definition the score carries no gradient, so the objective is differentiated with exactly these numbers in the masks.
    -> dict: logits, M (per stage), reg"""
    from oracle import d2s_oracle as O
    x = O.embed_tokens(sd, images.to(dtype), cfg)
    B, N, _ = x.shape
    m = torch.ones((B, N), dtype=dtype)
    out = dict(M=[])
    stage, reg = 0, 0.0
    eye = torch.eye(N, dtype=dtype)

    def policy_probs(S, m, first):
        if first:
            return S.softmax(dim=-1)
        mk = m[:, None, None, :] * (1.0 - eye) + eye
        e = torch.exp(S - S.max(dim=-1, keepdim=True).values.detach()) * mk
        return (e + eps / N) / (e.sum(dim=-1, keepdim=True) + eps)

    for l in range(cfg["depth"]):
        pol, first = m, stage == 0
        x, _ = R._block(sd, l, x, cfg, lambda S: policy_probs(S, pol, first))
        if stage < len(locs) and l == locs[stage]:
            s = scores[stage].to(dtype).detach()
            M = torch.sigmoid((s - theta[stage]) / tau)
            M = torch.cat((torch.ones_like(M[:, :1]), M[:, 1:]), dim=1)
            out["M"].append(M)
            reg = reg + M[:, 1:].sum()
            m = m * M
            stage += 1
    out["logits"] = R._logits(sd, x, cfg)
    out["reg"] = reg / (len(locs) * B * (N - 1))
    return out
