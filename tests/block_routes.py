"""What the transformer block's host code does, per configuration, through the public entry points only (DF.run(DF.BlockFn, ...),
DF.ragged_block_forward, DF.AttnCoreFn.apply, the token-merging block's TF.tome_block_forward, TF.tome_block_forward_bf16 and
TF.tome_block_train, AF.ragged_block_train, and the blocks with a tap or a stage: GF.rank_block, SF.metric_block, LF.soft_block,
LF.stage_block): the C-ABI entries it issues (forward, backward), the bytes it saves for the backward and its peak of allocated
memory.  Shared by tools/gen_block_routes.py, which records tests/golden/block_routes.json, and
tests/test_block_routes_gpu.py, which compares a fresh recording with it.

Geometry: the block of tests/test_ragged_bf16_gpu.py (D 128, 2 heads, hidden 512), B = 2, n = 33 (one key tile plus a remainder);
the ragged case packs the lengths (5, 33); the token-merging block merges r = 5 of the 33 tokens away (28 rows per image in its MLP
half) or none, with every token one patch (size None) or the fixed patch counts of _size().  The attention configurations appended
last run longer sequences: n = 70 (two full key tiles plus a 6-row remainder; the dense bf16 forward takes its 32-key-tile kernel there)
and n = 161 (a second workgroup, of 33 queries), and the packed lengths (70, 161).  The tap and stage configurations behind them are
back at B = 2, n = 33 and the packed lengths (5, 33); their stages leave the 5-row image whole and shorten the 33-row one."""
import torch

from tests.test_ragged_bf16_gpu import BLOCK_D, BLOCK_H, SCALE, _block_params, _cu, _t

DEV = "cuda:0"
B, N = 2, 33
RAGGED_LENGTHS = (5, 33)
EPS = 1e-6
TOME_R = 5
ATTN_LENGTHS = (70, 161)
MODES = ("exact", "split", "bf16", "bf16_noio")          # bf16_noio: bf16 arithmetic with the bf16 data path switched off


def configurations():
    """[(name, dict)] in the order they are run"""
    out = []
    for mode in MODES:
        for train in (False, True):
            for policy in ("none", "const", "grad"):
                for dp in (False, True):
                    composites = (True, False) if (mode in ("exact", "split") and policy == "none") else (True,)
                    for composite in composites:
                        name = f"block/{mode}/{'train' if train else 'nograd'}/policy_{policy}/{'dp' if dp else 'nodp'}"
                        out.append((name + ("" if composite else "/percall"),
                                    dict(kind="block", mode=mode, train=train, policy=policy, dp=dp, composite=composite, grads="all")))
    for mode in ("exact", "bf16"):          # the backward prunes its launches by what wants a gradient
        for grads in ("x", "params"):
            for composite in ((True, False) if mode == "exact" else (True,)):
                out.append((f"block/{mode}/train/only_{grads}" + ("" if composite else "/percall"),
                            dict(kind="block", mode=mode, train=True, policy="none", dp=False, composite=composite, grads=grads)))
    for mode in MODES:
        for want_cls in (True, False):
            out.append((f"ragged/{mode}/{'cls' if want_cls else 'nocls'}", dict(kind="ragged", mode=mode, want_cls=want_cls)))
    for mode in ("exact", "bf16"):
        for policy in ("none", "const", "grad"):
            out.append((f"attn/{mode}/policy_{policy}", dict(kind="attn", mode=mode, policy=policy)))
    # appended: the caching allocator rounds for the ones above as it did at their recording
    return out + _tome_configurations() + _attention_configurations() + _tap_and_stage_configurations()


def _tome_configurations():
    out = []

    def add(mode, train, r, size, **kw):
        cfg = dict(kind="tome", mode=mode, train=train, r=r, size=size, replay=False, prop_attn=True, grads="all",
                   entry="train" if train else "forward")
        cfg.update(kw)
        tags = [t for t, on in (("replay", cfg["replay"]), ("noprop", not cfg["prop_attn"]), (f"only_{cfg['grads']}", cfg["grads"] != "all"),
                                ("fn_nograd", cfg["entry"] == "train" and not train)) if on]
        out.append(("/".join([f"tome/{mode}/{'train' if train else 'nograd'}/r{r}/size_{'given' if size else 'none'}"] + tags), cfg))
    for mode in ("exact", "split"):
        for train in (False, True):
            for r in (0, TOME_R):
                for size in (False, True):
                    add(mode, train, r, size)
    for train in (False, True):
        add("exact", train, TOME_R, True, replay=True)
        add("exact", train, TOME_R, True, prop_attn=False)
    for grads in ("x", "params"):          # the backward prunes its launches by what wants a gradient
        add("exact", True, TOME_R, True, grads=grads)
    add("exact", False, TOME_R, True, entry="train")          # ToMeBlockFn with nothing to keep for a backward
    for r in (0, TOME_R):          # the bf16 data path, forward only
        for size in (False, True):
            add("bf16", False, r, size)
    add("bf16", False, TOME_R, True, replay=True)
    return out


def _attention_configurations():
    """every instantiation of the attention kernels past one key tile and past one workgroup, the varlen backward among them"""
    out = []
    for n in ATTN_LENGTHS:
        for mode in ("exact", "bf16"):
            for policy in ("none", "const", "grad"):
                out.append((f"attn/{mode}/policy_{policy}/n{n}", dict(kind="attn", mode=mode, policy=policy, n=n)))
    for mode in ("exact", "bf16"):
        out.append((f"ragged/{mode}/cls/n70_161", dict(kind="ragged", mode=mode, want_cls=True, lengths=ATTN_LENGTHS)))
    for lengths in (RAGGED_LENGTHS, ATTN_LENGTHS):          # RaggedBlockFn without a sampling stage: the varlen forward with lse and its backward
        out.append((f"ragged_train/exact/n{lengths[0]}_{lengths[1]}", dict(kind="ragged_train", mode="exact", train=True, lengths=lengths)))
    for mode in ("bf16", "bf16_noio"):          # the dense bf16 kernels on bf16 and on fp32 qkv, the forward on 32-key tiles
        out.append((f"block/{mode}/train/policy_none/nodp/n70",
                    dict(kind="block", mode=mode, train=True, policy="none", dp=False, composite=True, grads="all", n=70)))
    return out


def _tap_and_stage_configurations():
    """the per-op routes with a tap behind the attention forward (graph rank, key metric, the LTP score) and the ragged blocks with a stage
    between their halves (an LTP threshold, ATS sampling), through GF.rank_block, SF.metric_block, LF.soft_block, LF.stage_block and
    AF.ragged_block_train"""
    out = []
    tg = lambda train: "train" if train else "nograd"
    for mode in ("exact", "split"):
        for train in (False, True):
            for dp in (False, True):
                out.append((f"rank/{mode}/{tg(train)}/{'dp' if dp else 'nodp'}", dict(kind="rank", mode=mode, train=train, dp=dp, iters=3)))
    for iters in (0, 3):
        for train in (False, True):
            for dp in (False, True):
                out.append((f"metric/exact/iters{iters}/{tg(train)}/{'dp' if dp else 'nodp'}",
                            dict(kind="metric", mode="exact", train=train, dp=dp, iters=iters)))
    for mode, bf16 in (("exact", False), ("split", False), ("exact", True), ("bf16", True)):
        for policy in ("none", "const", "grad"):
            for score in (True, False):
                for train in (False, True):
                    out.append((f"ltp_soft/{mode}{'/bf16flag' if bf16 else ''}/{tg(train)}/policy_{policy}/{'score' if score else 'noscore'}",
                                dict(kind="ltp_soft", mode=mode, bf16=bf16, policy=policy, score=score, train=train)))
    for kind in ("ltp_stage", "ragged_stage"):          # ragged_stage: an ATS stage of K = 8, 33 -> 9 rows and 5 stays 5
        for mode in ("exact", "bf16"):
            for train, replay in ((False, False), (True, False), (True, True)):
                out.append((f"{kind}/{mode}/{tg(train)}" + ("/replay" if replay else ""),
                            dict(kind=kind, mode=mode, bf16=mode == "bf16", train=train, replay=replay)))
    for train in (False, True):          # the stage-less ragged block on the bf16 data path
        out.append((f"ragged_train/bf16/{tg(train)}", dict(kind="ragged_stage", mode="bf16", bf16=True, train=train, replay=False, stage=False)))
    return out


_HOST = {}


def _synth(tag, shape):
    """a fresh device tensor per call; the values are made once"""
    from d2s import synth
    if (tag, shape) not in _HOST:
        _HOST[tag, shape] = _t(synth.normal(f"routes/{tag}", shape, seed=21))
    return _HOST[tag, shape].to(DEV)


def _params():
    if "params" not in _HOST:
        _HOST["params"] = _block_params()
    return [t.to(DEV) for t in _HOST["params"]]


def _policy(kind, n=N):
    if kind == "none":
        return None
    p = torch.ones(B, n, device=DEV)
    p[0, 3::4] = 0.0
    p[1, 2::3] = 0.0
    return p.requires_grad_(kind == "grad")


def _size():
    """patches per token: 1s with some 2s and 3s, CLS at 1"""
    s = torch.ones(B, N, device=DEV)
    s[0, 2::5] = 2.0
    s[1, 3::4] = 3.0
    s[1, 4::7] = 2.0
    return s


def _make_tome_call(cfg):
    from d2s import functional_tome as TF, ops
    r = cfg["r"]
    size = _size() if cfg["size"] else None
    # a replayed plan is a recorded one of another input: the match of the synthetic qkv of the attn configurations
    plan = tuple(ops.tome_match(_synth("qkv", (B * N, 3 * BLOCK_D)), B, N, BLOCK_H, r)[2:]) if cfg["replay"] else None
    x = _synth("x", (B, N, BLOCK_D)).requires_grad_(cfg["train"] and cfg["grads"] in ("all", "x"))
    p = [t.requires_grad_(cfg["train"] and cfg["grads"] in ("all", "params")) for t in _params()]
    leaves = dict(dx=x, **{f"dp{i}": t for i, t in enumerate(p)}) if cfg["train"] else {}

    def outputs(y, size_out, used):
        unm, src, dst = used if used is not None else (None, None, None)
        return dict(y=y, size_out=size_out, unm=unm, src=src, dst=dst)

    def call():
        if cfg["entry"] == "train":
            with torch.enable_grad() if cfg["train"] else torch.no_grad():
                y, size_out, used = TF.tome_block_train(x, size, p, BLOCK_H, EPS, SCALE, r, cfg["prop_attn"], plan)
            return outputs(y, size_out, used), (y if cfg["train"] else None)
        forward = TF.tome_block_forward_bf16 if cfg["mode"] == "bf16" else TF.tome_block_forward
        with torch.no_grad():
            y, size_out, used = forward(x.view(B * N, BLOCK_D), size, p, B, N, BLOCK_H, EPS, SCALE, r, cfg["prop_attn"], plan)
        return outputs(y, size_out, used), None
    return call, leaves


def _ltp_theta():
    """The threshold of the ltp_stage configurations, from the float64 restatement (tests/ltp_ref.py) on the synthetic packed input: the
    middle of the widest gap between two neighbouring patch scores of the 33-row image, so that image drops some of its patches and keeps
    the others in every arithmetic mode.  One threshold cannot also split the 5-row image: an image's scores sum to 1, its four patches
    score about 1 / 5 each, above every patch of the longer image - it keeps them all."""
    if "theta" not in _HOST:
        import torch.nn.functional as F
        from tests import ltp_ref
        p = [t.double() for t in _block_params()]
        x = _synth("xr", (sum(RAGGED_LENGTHS), BLOCK_D)).cpu().double()          # the input of _make_stage_call
        qkv = F.linear(F.layer_norm(x, (BLOCK_D,), p[0], p[1], EPS), p[2], p[3])
        s = ltp_ref.score_varlen(qkv, RAGGED_LENGTHS, BLOCK_H, SCALE)[RAGGED_LENGTHS[0] + 1:].sort().values
        i = int((s[1:] - s[:-1]).argmax())
        _HOST["theta"] = float(s[i] + s[i + 1]) / 2
    return torch.full((1,), _HOST["theta"], device=DEV)


def _make_tap_call(cfg):
    """rank_block, metric_block and soft_block on the dense [B, N, D] input"""
    from d2s import functional_graph_rank as GF, functional_ltp as LF, functional_sim_prune as SF
    x = _synth("x", (B, N, BLOCK_D)).requires_grad_(True)
    p = [t.requires_grad_(True) for t in _params()]
    leaves = dict(dx=x, **{f"dp{i}": t for i, t in enumerate(p)})
    if cfg["kind"] == "ltp_soft":
        policy = _policy(cfg["policy"])
        if policy is not None and policy.requires_grad:
            leaves["dpolicy"] = policy
    else:
        rows = (torch.tensor([1.25, 0.0], device=DEV), torch.tensor([0.0, 1.25], device=DEV)) if cfg["dp"] else None

    def call():
        with torch.enable_grad() if cfg["train"] else torch.no_grad():
            if cfg["kind"] == "rank":
                y, cls_row, rank = GF.rank_block(x, p, BLOCK_H, EPS, SCALE, cfg["iters"], drop_path_rows=rows)
                outs = dict(y=y, cls=cls_row, rank=rank)
            elif cfg["kind"] == "metric":
                y, cls_row, metric, rank = SF.metric_block(x, p, BLOCK_H, EPS, SCALE, cfg["iters"], drop_path_rows=rows)
                outs = dict(y=y, cls=cls_row, metric=metric, rank=rank)
            else:
                y, score = LF.soft_block(x, p, BLOCK_H, EPS, SCALE, policy, cfg["score"], bf16=cfg["bf16"])
                outs = dict(y=y, score=score)
        return outs, (y if cfg["train"] else None)
    return call, leaves


def _make_stage_call(cfg):
    """stage_block and ragged_block_train on the packed lengths (5, 33); a replaying configuration replays, in its measured call, the plan
    its warm-up call decided"""
    from d2s import functional_ats as AF, functional_ltp as LF
    lengths, plans = RAGGED_LENGTHS, []
    xp, cu = _synth("xr", (sum(lengths), BLOCK_D)).requires_grad_(True), _cu(lengths).to(DEV)
    p = [t.requires_grad_(True) for t in _params()]
    row_src = torch.cat([torch.arange(n, dtype=torch.int32) for n in lengths]).to(DEV)
    theta = _ltp_theta() if cfg["kind"] == "ltp_stage" else None
    geom = (cu, len(lengths), max(lengths), BLOCK_H, SCALE)

    def call():
        plan = plans[0] if (cfg["replay"] and plans) else None
        with torch.enable_grad() if cfg["train"] else torch.no_grad():
            if cfg["kind"] == "ltp_stage":
                r = LF._RaggedLTP(*geom, row_src, theta, max(lengths) - 1, plan, bf16=cfg["bf16"])
                y = LF.stage_block(xp, p, EPS, r)
            elif cfg.get("stage", True):
                r = AF._Ragged(*geom, row_src, 8, max(lengths) - 1, plan, bf16=cfg["bf16"], stage_bf16=cfg["bf16"])
                y = AF.ragged_block_train(xp, p, EPS, r)
            else:
                r = AF._Ragged(*geom, bf16=cfg["bf16"])
                y = AF.ragged_block_train(xp, p, EPS, r)
        plans.append(r.plan)
        keep, counts = r.plan if r.plan is not None else (None, None)
        return dict(y=y, cu_new=r.cu_new, row_src_new=r.row_src_new, keep=keep, counts=counts, score=r.score, dense=r.dense), \
            (y if cfg["train"] else None)
    return call, dict(dx=xp, **{f"dp{i}": t for i, t in enumerate(p)})


def _make_call(cfg):
    """-> (call, leaves): call() runs the forward and returns (outputs, the output to run the backward from or None); leaves: the named
    tensors whose .grad the backward fills"""
    from d2s import functional as DF
    leaves = {}
    if cfg["kind"] == "tome":
        return _make_tome_call(cfg)
    if cfg["kind"] in ("rank", "metric", "ltp_soft"):
        return _make_tap_call(cfg)
    if cfg["kind"] in ("ltp_stage", "ragged_stage"):
        return _make_stage_call(cfg)
    if cfg["kind"] in ("ragged", "ragged_train"):
        p = _params()
        lengths = cfg.get("lengths", RAGGED_LENGTHS)
        total = sum(lengths)
        xp, cu = _synth("xr", (total, BLOCK_D)), _cu(lengths).to(DEV)
        if cfg["kind"] == "ragged_train":
            from d2s import functional_ats as AF
            xp.requires_grad_(True)
            p = [t.requires_grad_(True) for t in p]
            leaves.update(dx=xp, **{f"dp{i}": t for i, t in enumerate(p)})

            def call():
                y = AF.ragged_block_train(xp, p, EPS, AF._Ragged(cu, len(lengths), max(lengths), BLOCK_H, SCALE))
                return dict(y=y), y
            return call, leaves

        def call():
            with torch.no_grad():
                y, cls_rows = DF.ragged_block_forward(xp, cu, len(lengths), max(lengths), p, BLOCK_H, EPS, SCALE, want_cls=cfg["want_cls"])
            return dict(y=y, cls=cls_rows), None
        return call, leaves
    n = cfg.get("n", N)
    policy = _policy(cfg["policy"], n)
    if policy is not None and policy.requires_grad:
        leaves["dpolicy"] = policy
    if cfg["kind"] == "attn":
        qkv = _synth("qkv", (B * n, 3 * BLOCK_D)).requires_grad_(True)
        leaves["dqkv"] = qkv
        extra = () if policy is None else (policy,)

        def call():
            out, cls_row = DF.AttnCoreFn.apply(qkv, B, n, BLOCK_H, SCALE, True, *extra)
            return dict(y=out, cls=cls_row), out
        return call, leaves
    x = _synth("x", (B, n, BLOCK_D)).requires_grad_(cfg["grads"] in ("all", "x"))
    p = [t.requires_grad_(cfg["grads"] in ("all", "params")) for t in _params()]
    leaves.update(dx=x, **{f"dp{i}": t for i, t in enumerate(p)})
    rows = (torch.tensor([1.25, 0.0], device=DEV), torch.tensor([0.0, 1.25], device=DEV)) if cfg["dp"] else ()
    extra = (policy,) + rows if (rows or policy is not None) else ()

    def call():
        if cfg["train"]:
            y, cls_row = DF.run(DF.BlockFn, x, *p, BLOCK_H, EPS, True, None, *extra)
            return dict(y=y, cls=cls_row), y
        with torch.no_grad():
            y, cls_row = DF.run(DF.BlockFn, x, *p, BLOCK_H, EPS, True, None, *extra)
        return dict(y=y, cls=cls_row), None
    return call, leaves


def _run(call, leaves, gy, names, distinct=False):
    saved, seen = [0], set()

    def pack(t):
        if not (distinct and t.data_ptr() in seen):          # distinct: a storage saved in two slots (a placeholder) counts once
            saved[0] += t.numel() * t.element_size()
        seen.add(t.data_ptr())
        return t
    for t in leaves.values():
        t.grad = None
    del names[:]
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        outs, root = call()
    fwd = [s for s in names if s != "d2s_convert_bf16"]          # a weight's bf16 form is made once, on its first use
    del names[:]
    if root is not None:
        if root.grad_fn is None:
            saved[0] = 0
        else:
            # behind a stage the output has fewer rows than went in: how many is known only here
            torch.autograd.backward([root], [gy if gy.shape[0] == root.shape[0] else gy[:root.shape[0]]])
    else:
        saved[0] = 0
    bwd = [s for s in names if s != "d2s_convert_bf16"]
    torch.cuda.synchronize()
    outs.update({k: t.grad for k, t in leaves.items() if t.grad is not None})
    return dict(forward=fwd, backward=bwd, saved_bytes=saved[0]), outs


def record(cfg):
    """One configuration of configurations().  -> ({forward, backward, saved_bytes, peak_bytes}, {name: output or gradient tensor})"""
    def make():
        call, leaves = _make_call(cfg)
        if cfg["kind"] == "tome":          # the merged block's output: n - r rows per image
            gy = _synth("gy", (B * (N - cfg["r"]), BLOCK_D)).view(B, N - cfg["r"], BLOCK_D)
        elif cfg["kind"] == "ragged_train":
            gy = _synth("gy", (sum(cfg["lengths"]), BLOCK_D))
        elif cfg["kind"] in ("ltp_stage", "ragged_stage"):          # the rows that entered; _run takes as many as left the stage
            gy = _synth("gy", (sum(RAGGED_LENGTHS), BLOCK_D))
        else:
            n = cfg.get("n", N)
            gy = _synth("gy", (B * n, BLOCK_D)) if cfg["kind"] == "attn" else _synth("gy", (B * n, BLOCK_D)).view(B, n, BLOCK_D)
        return call, leaves, gy
    return record_call(make, cfg["mode"], cfg.get("composite", True))


def record_call(make, mode, composite=True, distinct=False):
    """The spy on the C-ABI and the allocator discipline, shared with tests/predictor_routes.py: make() -> (call, leaves, gy) as of
    _make_call, run in the arithmetic mode `mode` (one of MODES): a warm-up call, then the measured one from an emptied allocator cache.
    distinct: count the saved bytes once per storage.  -> (route, tensors) as record's"""
    from d2s import lib, ops
    gmode = {"exact": ops.GEMM_EXACT, "split": ops.GEMM_SPLIT}.get(mode, ops.GEMM_BF16)
    switches = ops._BF16_IO, ops._BLOCK_COMPOSITE
    names, real = [], lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    lib.call = spy
    try:
        ops._BF16_IO = mode != "bf16_noio"
        ops._BLOCK_COMPOSITE = composite
        call, leaves, gy = make()
        with ops.gemm_mode(gmode):
            _run(call, leaves, gy, names, distinct)
            for t in leaves.values():
                t.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            route, outs = _run(call, leaves, gy, names, distinct)
            route["peak_bytes"] = torch.cuda.max_memory_allocated() - base
    finally:
        lib.call = real
        ops._BF16_IO, ops._BLOCK_COMPOSITE = switches
    return route, outs


def record_all():
    """-> ({name: route}, {name: {tensor name: tensor}})"""
    routes, tensors = {}, {}
    for name, cfg in configurations():
        routes[name], outs = record(cfg)
        tensors[name] = {k: t.detach().cpu() for k, t in outs.items() if t is not None}
    return routes, tensors
