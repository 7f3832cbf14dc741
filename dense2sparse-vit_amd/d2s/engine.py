"""Training engine for the accelerated step: flat parameter / gradient arenas in HBM, fused AdamW, the step of
train.py:40-57, and the data-parallel gradient exchange (ddp_training.py:93 intent) as bucketed RCCL all-reduces on a
side stream that overlap the rest of backward.

Layout: every student parameter lives in ONE fp32 arena (each tensor padded to 1024 elements); gradients, exp_avg and
exp_avg_sq have arenas of the same layout.  The Functions in d2s.functional write parameter gradients straight into
the gradient arena (ops.grad_buffer), so the optimiser is a single kernel launch and a DDP bucket is a contiguous
slice - there is no flatten/unflatten copy anywhere.
"""
import contextlib
import math

import numpy as np
import torch
import torch.distributed as dist

import methods

from . import lib, ops


def _group_of(name, p):
    """utils.get_param_groups, utils.py:67-90 -> 'predictor' | 'base_no_decay' | 'base_decay' | None (never optimised)."""
    if "predictor" in name or "dist" in name:
        return "predictor"
    if "early_exit" in name:
        return "early_exit"
    if "cls_token" in name or "pos_embed" in name:
        return None
    if p.dim() == 1 or name.endswith(".bias"):
        return "base_no_decay"
    return "base_decay"


class ParamArena:
    """Moves the parameters of `model` into one flat fp32 buffer (in registration order) and owns the matching
    gradient buffer.  param.data becomes a view; state_dict()/load_state_dict() keep working."""

    def __init__(self, model, order=None):
        self.chunk = lib.query("d2s_adamw_chunk_elems")
        named = [(n, p) for n, p in model.named_parameters()]
        if order is not None:
            byname = dict(named)
            assert sorted(order) == sorted(byname), "order must list every parameter exactly once"
            named = [(n, byname[n]) for n in order]
        assert named and all(p.is_cuda and p.dtype == torch.float32 for _, p in named), "move the model to the GPU first"
        dev = named[0][1].device
        self.names, self.offsets, self.sizes, self.params_list = [], [], [], []
        off = 0
        for n, p in named:
            self.names.append(n)
            self.offsets.append(off)
            self.sizes.append(p.numel())
            self.params_list.append(p)
            off += ((p.numel() + self.chunk - 1) // self.chunk) * self.chunk
        self.total = off
        self.n_chunks = off // self.chunk
        self.params = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad_views = {}
        for n, p, o, s in zip(self.names, self.params_list, self.offsets, self.sizes):
            v = self.params[o:o + s].view(p.shape)
            v.copy_(p.data)
            p.data = v
            gv = self.grads[o:o + s].view(p.shape)
            self.grad_views[n] = gv
            ops.register_grad_buffer(p, gv)
        ops.register_weight_arena(self.params)       # weights at stable addresses: their W^T copies may be cached (ops.linear_dgrad)

    def chunk_range(self, i):
        o = self.offsets[i]
        return o // self.chunk, (o + ((self.sizes[i] + self.chunk - 1) // self.chunk) * self.chunk) // self.chunk

    def check_alias(self):
        """The optimiser updates the arena; a parameter whose .data was re-assigned afterwards (.to(), .half(), load into a new
        tensor) would silently stop following it."""
        base = self.params.data_ptr()
        for n, p, o in zip(self.names, self.params_list, self.offsets):
            if p.data_ptr() != base + 4 * o:
                raise lib.D2SError(f"parameter {n} no longer aliases the parameter arena (re-assigned after TrainStep was built)")

    def collect_grads(self):
        """Make sure every live gradient sits in the arena (it does when the Functions produced it; a gradient that
        autograd materialised elsewhere is copied in) and detach .grad from autograd's bookkeeping."""
        for n, p in zip(self.names, self.params_list):
            if p.grad is not None and p.grad.data_ptr() != self.grad_views[n].data_ptr():
                self.grad_views[n].copy_(p.grad)


class FusedAdamW:
    """torch.optim.AdamW semantics (decoupled weight decay, bias correction) over a ParamArena in one kernel launch.
    Groups and learning rates follow utils.get_param_groups / utils.adjust_learning_rate (utils.py:67-147)."""

    def __init__(self, arena, lr=5e-4, weight_decay=0.05, betas=(0.9, 0.999), eps=1e-8):
        self.arena, self.betas, self.eps = arena, betas, eps
        self.exp_avg = torch.zeros_like(arena.params)
        self.exp_avg_sq = torch.zeros_like(arena.params)
        self.groups = [_group_of(n, p) for n, p in zip(arena.names, arena.params_list)]
        self.group_lr = {"predictor": lr, "base_no_decay": lr, "base_decay": lr, "early_exit": lr}
        self.group_wd = {"predictor": weight_decay, "base_no_decay": 0.0, "base_decay": weight_decay, "early_exit": weight_decay}
        self.steps = 0
        # torch.optim.AdamW counts updates per parameter (state['step'] advances only when the parameter has a gradient), so a tensor
        # frozen during the warm-up epochs starts its bias correction at t = 1 afterwards: one counter per arena chunk, on the device
        self.chunk_steps = torch.zeros(arena.n_chunks, dtype=torch.int32, device=arena.params.device)
        self._desc = None
        self._dirty = True
        self._wt = None
        # exponential moving average of the weights (enable_ema): a fifth arena, advanced inside the AdamW launch; None = off, and then
        # neither the buffer nor the EMA entry point is ever touched
        self.ema, self.ema_decay, self._ema_primed = None, None, False

    def enable_ema(self, decay):
        """Keep ema = decay * ema + (1 - decay) * p after every step (timm ModelEmaV2), in the launch that updates p.  The average
        starts from the parameters as they are immediately before the NEXT step - not from what the arena holds now - so a broadcast
        into the arena or a load_state_dict that follows this call is what it starts from."""
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise lib.D2SError(f"ema decay {decay}: expected 0 <= decay < 1")
        if self.ema is None:
            self.ema = torch.zeros_like(self.arena.params)
        self.ema_decay, self._ema_primed = decay, False

    def ema_flat(self):
        """The EMA arena as it counts right now: before the first step after enable_ema it IS the parameters."""
        if self.ema is None:
            raise lib.D2SError("no EMA weights: call enable_ema(decay) first")
        return self.ema if self._ema_primed else self.arena.params

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the parameter arena holds the EMA weights (and the EMA arena the live ones): the model evaluates its moving
        average without a second copy of itself.  Swapped on the device and swapped back on exit, bit for bit.  No step inside."""
        if self.ema is None:
            raise lib.D2SError("no EMA weights: call enable_ema(decay) first")
        swap = self._ema_primed              # not started yet: the average equals the parameters, nothing to exchange
        if swap:
            self._swap_ema()
        try:
            yield self
        finally:
            if swap:
                self._swap_ema()

    def _swap_ema(self):
        a = self.arena
        tmp = a.params.clone()
        a.params.copy_(self.ema)
        self.ema.copy_(tmp)
        ops.bump_weights_epoch()        # raw write into the arena: cached W^T copies and bf16 mirrors of the weights are stale

    def set_lrs(self, predictor_lr, backbone_lr):
        self.group_lr.update(predictor=predictor_lr, base_no_decay=backbone_lr, base_decay=backbone_lr)
        self._dirty = True

    def _build_desc(self):
        a = self.arena
        desc = np.zeros(a.n_chunks, dtype=[("lr", "<f4"), ("wd", "<f4"), ("active", "<i4"), ("pad", "<i4")])
        for i, (g, p) in enumerate(zip(self.groups, a.params_list)):
            c0, c1 = a.chunk_range(i)
            if g is None or g == "early_exit" or not p.requires_grad:
                continue      # early_exit: the head is never called (dynamic_vit.py:752-758), its gradients stay None and torch's AdamW
                              # skips such parameters entirely - so does this one
            desc["lr"][c0:c1] = self.group_lr[g]
            desc["wd"][c0:c1] = self.group_wd[g]
            desc["active"][c0:c1] = 1
        new = torch.from_numpy(desc.view(np.uint8).copy())
        if self._desc is None:
            self._desc = new.to(a.params.device)
        else:                           # in place: a captured step (TrainStep graph mode) keeps reading this buffer
            self._desc.copy_(new, non_blocking=False)
        self._dirty = False

    def mark_dirty(self):
        self._dirty = True

    def desc(self):
        """The per-chunk {lr, wd, active} table on the device, rebuilt when learning rates or the frozen set changed."""
        if self._dirty:
            self._build_desc()
        return self._desc

    def step(self, grad_scale=1.0, clip_coef=None):
        """clip_coef: None, or a one-float device tensor - the gradient scale is then fl(grad_scale * clip_coef[0]), formed on the device
        (d2s_adamw_step_clip); without it d2s_adamw_step / d2s_adamw_step_ema are launched with the host scale."""
        if self._dirty:
            self._build_desc()
        self.steps += 1
        a = self.arena
        if self.ema is not None and not self._ema_primed:
            self.ema.copy_(a.params)
            self._ema_primed = True
        if clip_coef is not None:
            ops.adamw_step_clip(a.params, a.grads, self.exp_avg, self.exp_avg_sq, self._desc, a.n_chunks, self.betas[0], self.betas[1],
                                self.eps, self.steps, clip_coef, ema=self.ema, ema_decay=self.ema_decay or 0.0, grad_scale=grad_scale,
                                chunk_steps=self.chunk_steps)
        elif self.ema is None:
            ops.adamw_step(a.params, a.grads, self.exp_avg, self.exp_avg_sq, self._desc, a.n_chunks, self.betas[0], self.betas[1],
                           self.eps, self.steps, grad_scale, chunk_steps=self.chunk_steps)
        else:
            ops.adamw_step_ema(a.params, a.grads, self.exp_avg, self.exp_avg_sq, self._desc, a.n_chunks, self.betas[0], self.betas[1],
                               self.eps, self.steps, self.ema, self.ema_decay, grad_scale, chunk_steps=self.chunk_steps)
        ops.bump_weights_epoch()        # the kernel wrote the parameters through raw pointers: cached W^T copies are stale

    def refresh_transposed_weights(self):
        """Rebuild the W^T copies of every weight of the arena in one launch (the input-gradient GEMMs read them, ops.linear_dgrad).
        TrainStep calls this at the START of every step, so whatever wrote the parameters since the last step - the fused AdamW, a
        broadcast into the arena, load_state_dict, a raw `.data` edit that no version counter sees - is picked up."""
        a = self.arena
        ops.bump_weights_epoch()
        if self._wt is None:
            self._wt = ops.TransposedArena(a.params, list(zip(a.params_list, a.offsets)))
        self._wt.refresh()
        if ops.bf16_io():      # bf16 mode: the GEMMs read bf16 mirrors of W and W^T made here, once per step
            if getattr(self, "_w16", None) is None:
                self._w16 = ops.Bf16Weights(a.params, list(zip(a.params_list, a.offsets)), self._wt)
            self._w16.refresh()

    def zero_grad(self):
        for p in self.arena.params_list:
            p.grad = None

    # ---- state in and out: per parameter NAME and in the parameter's own shape; offsets, padding and the arena order stay inside ----
    def _unflatten(self, flat):
        """device arena -> {name: CPU tensor of the parameter's shape, with storage of its own} (one device-to-host copy)"""
        a = self.arena
        host = flat.detach().cpu()
        return {n: host[o:o + sz].reshape(p.shape).clone() for n, p, o, sz in zip(a.names, a.params_list, a.offsets, a.sizes)}

    def _flatten(self, tensors):
        """{name: tensor} -> CPU tensor in arena layout (padding zero)"""
        a = self.arena
        host = torch.zeros(a.total, dtype=torch.float32)
        for n, o, sz in zip(a.names, a.offsets, a.sizes):
            host[o:o + sz] = tensors[n].detach().to(dtype=torch.float32, device="cpu").reshape(-1)
        return host

    def state_dict(self):
        a = self.arena
        m, v = self._unflatten(self.exp_avg), self._unflatten(self.exp_avg_sq)
        counts = self.chunk_steps.cpu().tolist()
        state = {n: {"exp_avg": m[n], "exp_avg_sq": v[n], "step": int(counts[a.chunk_range(i)[0]])} for i, n in enumerate(a.names)}
        return {"state": state, "betas": [float(self.betas[0]), float(self.betas[1])], "eps": float(self.eps), "steps": int(self.steps)}

    def check_state_dict(self, sd, what="optimizer"):
        a = self.arena
        state = sd.get("state") if isinstance(sd, dict) else None
        if not isinstance(state, dict):
            raise lib.D2SError(f"checkpoint {what}: no per-parameter 'state'")
        _check_names_shapes(what, {n: tuple(p.shape) for n, p in zip(a.names, a.params_list)},
                            {n: tuple(e["exp_avg"].shape) for n, e in state.items()})
        for n, e in state.items():
            if tuple(e["exp_avg_sq"].shape) != tuple(e["exp_avg"].shape):
                raise lib.D2SError(f"checkpoint {what}: exp_avg_sq of {n} has shape {tuple(e['exp_avg_sq'].shape)}, exp_avg {tuple(e['exp_avg'].shape)}")
        if [float(b) for b in sd["betas"]] != [float(b) for b in self.betas] or float(sd["eps"]) != float(self.eps):
            raise lib.D2SError(f"checkpoint {what}: betas / eps {sd['betas']} / {sd['eps']}, this optimiser has {list(self.betas)} / {self.eps}")

    def load_state_dict(self, sd):
        """Copies INTO the existing arenas (call check_state_dict first: this method assumes names and shapes fit)."""
        a = self.arena
        state = sd["state"]
        self.exp_avg.copy_(self._flatten({n: state[n]["exp_avg"] for n in a.names}))
        self.exp_avg_sq.copy_(self._flatten({n: state[n]["exp_avg_sq"] for n in a.names}))
        counts = torch.zeros(a.n_chunks, dtype=torch.int32)
        for i, n in enumerate(a.names):
            c0, c1 = a.chunk_range(i)
            counts[c0:c1] = int(state[n]["step"])
        self.chunk_steps.copy_(counts)
        self.steps = int(sd.get("steps", 0))
        self._dirty = True


def _check_names_shapes(what, want, got):
    """want / got: {name: shape}.  One D2SError naming the first difference."""
    for n in want:
        if n not in got:
            raise lib.D2SError(f"checkpoint {what}: {n} is missing")
    for n in got:
        if n not in want:
            raise lib.D2SError(f"checkpoint {what}: unexpected entry {n}")
    for n, shape in want.items():
        if tuple(got[n]) != tuple(shape):
            raise lib.D2SError(f"checkpoint {what}: {n} has shape {tuple(got[n])}, this model has {tuple(shape)}")


CHECKPOINT_FORMAT = 1


def checkpoint_config(config):
    """A checkpoint's 'config' with the keys that later features added filled in as the checkpoint's run had them: off."""
    theirs = dict(config)
    theirs.setdefault("drop_path_rate", 0.0)       # checkpoints written before stochastic depth existed were trained without it
    theirs.setdefault("diff_topk", False)          # ... and before the perturbed top-k mode existed: hard selection
    theirs.setdefault("topk_num_samples", 0)
    theirs.setdefault("fuse_dropped", False)       # ... and before token fusion existed: dropped tokens were discarded
    theirs.setdefault("attn_selection", False)     # ... and before attention selection existed: the score predictor selected
    theirs.setdefault("mean_heads", False)
    theirs.setdefault("tome_r", [])                # ... and before a Token Merging student could be trained: no such student
    theirs.setdefault("prop_attn", False)
    theirs.setdefault("train_merge", False)
    theirs.setdefault("ats_locs", [])              # ... and before an Adaptive Token Sampling student could be trained: no such student
    theirs.setdefault("ats_tokens", [])
    theirs.setdefault("train_sample", False)
    for m in methods.METHODS:                      # ... and before the A-ViT, Evo-ViT or LTP baseline existed: no such student
        for k in m.config_keys:
            theirs.setdefault(k, None)
    theirs.setdefault("squeeze_dropped", False)    # ... and before pruning and squeezing existed: dropped tokens were discarded
    theirs.setdefault("ragged_train", False)       # ... and before the dynamic keep ratio could train on the ragged batch: policy attention
    theirs.setdefault("ragged_bf16", False)        # ... and before it could do so in the bf16 arithmetic mode: fp32 modes only
    return theirs


def graph_rank_iters(config):
    """The PageRank iterations of a checkpoint's (or a run's) 'config': the key is recorded only when positive, so a
    config without it - every other run, every checkpoint written before graph ranking existed - reads as 0"""
    return int(config.get("graph_rank_iters", 0))


def sim_prune(config):
    """The similarity-pruning count of a checkpoint's (or a run's) 'config': the key is recorded only when positive (DESIGN.md section
    30), so a config without it - every other run, every checkpoint written before the similarity stage existed - reads as 0"""
    return int(config.get("sim_prune", 0))


def adjust_learning_rate(optimizer, model, step, epochs, lr, min_lr, warmup_steps, frozen=()):
    """utils.adjust_learning_rate (utils.py:93-147): cosine schedule, backbone frozen for the first `warmup_steps`
    epochs (requires_grad toggled exactly like the reference), backbone lr = min(0.01 lr, cos) afterwards."""
    cos_lr = (math.cos(step / epochs * math.pi) + 1) * 0.5
    cos_lr = min_lr + cos_lr * (lr - min_lr)
    predictor_lr = cos_lr
    backbone_lr = 0.0 if step < warmup_steps else min(lr * 0.01, cos_lr)
    for n, p in model.named_parameters():
        if n in frozen:     # frozen by construction (T2T's sinusoid pos_embed, the performer's random features): never trained
            continue
        is_pred = "dist" in n or "predictor" in n
        g = _group_of(n, p)
        if g is None:                       # cls_token / pos_embed: in no param group, follow the first loop of the reference
            p.requires_grad_(True if step >= warmup_steps else is_pred)
        elif g == "predictor":
            p.requires_grad_(predictor_lr != 0)
        else:
            p.requires_grad_(backbone_lr != 0)
    optimizer.set_lrs(predictor_lr, backbone_lr)
    return predictor_lr, backbone_lr


def execution_order(student):
    """Parameter names in forward-execution order (embed, then per block: the predictor that runs before it, the block;
    then norm / head).  Autograd runs backward in exactly the reverse order, so gradients become final from the END of
    an arena laid out this way towards its start - which is what makes a DDP bucket a contiguous tail slice."""
    names = [n for n, _ in student.named_parameters()]
    pre = [n for n in names if not (n.startswith("blocks.") or n.startswith("score_predictor.") or n.startswith("norm.")
                                    or n.startswith("head."))]
    order, starts = list(pre), {}
    locs = list(getattr(student, "pruning_loc", []))
    for i in range(len(student.blocks)):
        starts[i] = len(order)
        if i in locs:
            s_ = locs.index(i)
            order += [n for n in names if n.startswith(f"score_predictor.{s_}.")]
        order += [n for n in names if n.startswith(f"blocks.{i}.")]
    order += [n for n in names if n.startswith("norm.") or n.startswith("head.")]
    assert sorted(order) == sorted(names)
    return order, starts


class GradReducer:
    """Data-parallel gradient averaging (the DDP of ddp_training.py:93): tail slices of the gradient arena are
    all-reduced with RCCL on a side stream as soon as autograd has finished the layers that own them (reverse layer
    order), so the exchange overlaps the remaining backward; joined before the optimiser step."""

    def __init__(self, arena, group=None, bucket_mb=None, collective=None):
        """bucket_mb (default: D2S_DDP_BUCKET_MB, else 16): smallest slice worth a collective of its own.
        collective (default: D2S_DDP_COLLECTIVE, else "allreduce"): "allreduce" = one all_reduce per bucket; "rs_ag" = reduce_scatter
        into this rank's 1/world shard of the bucket followed by an all_gather of the shards - the two halves of a direct
        all-reduce over the fully connected xGMI mesh (SURVEY 8d sizes both forms); same sums, same result layout."""
        import os
        self.arena, self.group = arena, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        # its waits on the weight-gradient stream sit in its hardware queue: on the main stream's queue they would stall the backward itself
        self.stream = ops.concurrent_stream([torch.cuda.current_stream()], "gradient exchange") if arena.params.is_cuda else None
        if bucket_mb is None:
            bucket_mb = float(os.environ.get("D2S_DDP_BUCKET_MB", "16"))
        self.collective = collective or os.environ.get("D2S_DDP_COLLECTIVE", "allreduce")
        if self.collective not in ("allreduce", "rs_ag"):
            raise ValueError(f"collective {self.collective!r}: expected 'allreduce' or 'rs_ag'")
        self.bucket_mb = bucket_mb
        self.bucket_elems = int(bucket_mb * (1 << 20) / 4)
        self._hi = arena.total
        # arena ranges [lo, hi) whose gradients exist this epoch (ascending, merged); None = the whole arena.  requires_grad flips
        # between epochs (utils.py:112-147): in the warm-up epochs only the predictors train, and cls_token / pos_embed are never
        # optimised (utils.py:79-80), so their slices are not exchanged either (set_live_ranges, called from TrainStep.set_epoch)
        self.live = None
        self.force = False      # rehearsal: issue the collectives even with a single rank
        self.paused = False
        self.timing = False     # bench: bracket every collective with events on the side stream
        self._events, self._exposed, self._bytes, self._launched = [], [], 0, False
        self._n_collectives = 0

    def set_live_ranges(self, ranges):
        """ranges: iterable of (lo, hi) arena offsets holding live gradients; merged when they touch."""
        merged = []
        for lo, hi in sorted(ranges):
            if merged and lo <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], hi)
            elif hi > lo:
                merged.append([lo, hi])
        self.live = [tuple(r) for r in merged]

    def live_elems(self):
        return self.arena.total if self.live is None else sum(hi - lo for lo, hi in self.live)

    def _launch(self, lo):
        hi, self._hi = self._hi, lo
        if (self.world == 1 and not self.force) or lo >= hi:
            return
        if self.live is None:
            self._reduce(lo, hi)
        else:       # only the parts of [lo, hi) that hold live gradients, from the arena's end towards its start
            for a, b in reversed(self.live):
                a, b = max(a, lo), min(b, hi)
                if b > a:
                    self._reduce(a, b)

    def _collective(self, buf, async_op):
        """SUM of `buf` over the ranks, result in `buf` on every rank.  -> list of work handles (async_op) or []"""
        n = buf.numel()
        if self.collective == "rs_ag" and self.world > 1 and n % self.world == 0:
            per = n // self.world
            shard = torch.empty(per, dtype=buf.dtype, device=buf.device)    # a buffer of its own: gloo on device tensors returns wrong sums
            w1 = dist.reduce_scatter_tensor(shard, buf, op=dist.ReduceOp.SUM, group=self.group, async_op=async_op)   # for an aliased output
            if async_op:
                w1.wait()            # RCCL: a stream-level dependency, no host block; gloo's worker threads would otherwise start the
                                     # gather before the scatter has written the shard
            w2 = dist.all_gather_into_tensor(buf, shard, group=self.group, async_op=async_op)
            self._n_collectives += 2
            return [w2] if async_op else []
        w = dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=async_op)     # also rs_ag's path for a slice the world does not divide
        self._n_collectives += 1
        return [w] if async_op else []

    def _reduce(self, lo, hi):
        buf = self.arena.grads[lo:hi]
        self._launched = True
        if self.stream is None:          # CPU tensors (gloo rehearsal): blocking
            self._collective(buf, False)
            return
        self.stream.wait_stream(torch.cuda.current_stream())
        wg = ops.weight_grad_stream()
        if wg is not None:                          # the weight gradients of this bucket were written on their own stream
            self.stream.wait_stream(wg)
        with torch.cuda.stream(self.stream):
            if self.timing:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            for w in self._collective(buf, True):
                w.wait()                 # stream-level wait: the side stream follows RCCL's stream
            if self.timing:
                e1.record()
                self._events.append((e0, e1))
                self._bytes += buf.numel() * 4

    def ready_from(self, lo):
        """Every gradient at arena offset >= lo is final."""
        if self.paused:          # a step that is being captured into a hipGraph: no collective from inside; finish() sends everything
            return
        if self._pending(lo) >= self.bucket_elems:
            self._launch(lo)

    def _pending(self, lo):
        if self.live is None:
            return self._hi - lo
        return sum(max(0, min(b, self._hi) - max(a, lo)) for a, b in self.live)

    def finish(self):
        """Flush the remainder, join, and return 1/world (folded into the optimiser's gradient scale)."""
        self._launch(0)
        if self._launched and self.stream is not None:
            cur = torch.cuda.current_stream()
            if self.timing:
                arrived, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                arrived.record(cur)
                done.record(self.stream)
                self._exposed.append((arrived, done))
            cur.wait_stream(self.stream)
        self._launched = False
        self._hi = self.arena.total
        return 1.0 / self.world

    def comm_summary(self, steps):
        """Per-step communication figures from the recorded events (call after a device synchronize): bytes all-reduced, time
        the collectives occupied the side stream, bus bandwidth 2(N-1)/N * bytes / time, and the exposed part = how long the
        main stream had to wait in finish() after the backward was already done."""
        if not self._events:
            return None
        t_ms = sum(a.elapsed_time(b) for a, b in self._events)
        exposed = sum(max(0.0, a.elapsed_time(b)) for a, b in self._exposed)
        n = max(self.world, 1)
        out = {"allreduce_bytes_per_step": self._bytes / steps, "buckets_per_step": len(self._events) / steps,
               "collectives_per_step": round(self._n_collectives / steps, 2), "collective": self.collective, "bucket_mb": self.bucket_mb,
               "allreduce_ms_per_step": round(t_ms / steps, 3), "exposed_ms_per_step": round(exposed / steps, 3),
               "bus_GBps": round(2.0 * (n - 1) / n * self._bytes / (t_ms * 1e-3) / 1e9, 1) if t_ms > 0 else None,
               "backend": "nccl (RCCL)", "world": n}
        self._events, self._exposed, self._bytes, self._n_collectives = [], [], 0, 0
        return out


class TrainStep:
    """One optimiser step as train.py:40-57 defines it: teacher forward (no grad), student forward, MaskLoss +
    BackboneLoss, warm-up switch (train.py:50-53), zero_grad / backward / step."""

    GRAPH_WARM_STEPS = 2        # eager steps of a given shape before it is captured (lazy one-time work happens there)

    def __init__(self, student, teacher, args, lr=5e-4, min_lr=1e-5, weight_decay=0.05, epochs=25, warmup_steps=0,
                 distributed=False, bucket_mb=None, collective=None, graph=None, accum_steps=1, clip_grad=None):
        """accum_steps = A: an optimiser step is computed from a window of A calls.  Every call runs forward, losses and backward on its own
        batch; the first A - 1 add their gradient to a second arena and return, the last one combines (fp32, arrival order), exchanges,
        clips and updates with the scale 1 / (A * world).  flush() closes a shorter window.  clip_grad = M: the gradient the optimiser sees
        is clipped to the global L2 norm M (torch.nn.utils.clip_grad_norm_ over the parameters it updates); norm and coefficient stay on the
        device (last_clip).  With A = 1 and no clipping the step is launch for launch what it is without these keywords.
        graph: capture the step into a hipGraph and replay it (None: D2S_STEP_GRAPH = 0 | 1 | auto, default 0; see _use_graph).
        Off by default: on ROCm 7.2 the replay of the ~1400-node graph is SLOWER than issuing the kernels (config 3, 32 images per GPU:
        2064 vs 2310 images/s; the replay call itself keeps the host busy for 11.4 ms against 12.5 ms of eager enqueue, and the GPU side
        gains nothing: profiles/r03_a_graph_vs_eager.txt) - the runtime walks the graph node by node on the host."""
        if int(accum_steps) != accum_steps or accum_steps < 1:
            raise lib.D2SError(f"accum_steps {accum_steps!r}: expected an integer >= 1")
        if clip_grad is not None and not float(clip_grad) > 0.0:
            raise lib.D2SError(f"clip_grad {clip_grad!r}: expected a norm > 0 (None = no clipping)")
        self.accum_steps, self.clip_grad = int(accum_steps), None if clip_grad is None else float(clip_grad)
        self._pending = 0                   # micro-steps of the open window whose gradients have not reached the optimiser yet
        self._acc = None                    # accumulation arena, partial sums of squares: allocated on first use
        self._partials = None
        self.last_clip = None               # device floats {pre-clip norm, coefficient} of the last clipped optimiser step
        self._norm_sum, self._norm_steps = None, 0
        self.student, self.teacher, self.args = student, teacher, args
        # a student that selects by its own CLS attention never calls its score predictors: like the early-exit head
        # they are created for the state-dict keys only, get no gradient, and the optimiser must not move them (no update, no weight decay)
        self.attn_selection = bool(getattr(student, "attn_selection", False))
        if self.attn_selection:
            if warmup_steps > 0:
                raise ValueError(f"warmup_steps {warmup_steps} with an attention-selecting student: the warm-up epochs train the score "
                                 "predictors only (train.py:50-53), and attention selection has none to train - pass warmup_steps=0")
            for p in student.score_predictor.parameters():
                p.requires_grad_(False)       # listed in self.frozen below: the epoch schedule leaves them alone, AdamW marks their chunks idle
            # ... and one that ranks by PageRank over the attention graph needs the block's fp32 qkv
            if int(getattr(student, "graph_rank_iters", 0)) > 0 and ops.get_gemm_mode() == ops.GEMM_BF16:
                from .functional_graph_rank import GRAPH_RANK_BF16_ERROR
                raise lib.D2SError(GRAPH_RANK_BF16_ERROR)
            # ... and so does one that prunes similar candidates: the key metric is computed from it
            if int(getattr(student, "sim_prune", 0)) > 0 and ops.get_gemm_mode() == ops.GEMM_BF16:
                from .functional_sim_prune import SIM_PRUNE_BF16_ERROR
                raise lib.D2SError(SIM_PRUNE_BF16_ERROR)
        # the logits-only families (methods.py; DESIGN.md sections 22 and 24 to 27) return logits alone and train with one objective of their
        # own; the teacher is optional (None: no teacher forward, no side stream).  Every refusal comes before anything touches the device.
        # A step is captured only where no block reads a row count on the host and the captured step is built: the Evo-ViT baseline's.
        self.method = m = methods.of(student)
        self.logits_only = m.logits_only
        if m.logits_only:
            if warmup_steps > 0:
                raise ValueError(f"warmup_steps {warmup_steps} with {m.student}: the warm-up epochs train the score predictors only "
                                 f"(train.py:50-53), and {m.has_none} - pass warmup_steps=0")
            if graph is True and m.no_graph:
                raise lib.D2SError(f"TrainStep(graph=True) with {m.student} is not supported: {m.no_graph}; run the step eagerly (graph=False)")
            if m.opt_in and m.opt_in[1](student) and not getattr(student, m.opt_in[0], False):
                raise lib.D2SError(f"TrainStep with {m.opt_in[2]}")
            if float(getattr(student, "drop_path_rate", 0.0)) > 0.:
                raise lib.D2SError(f"TrainStep with {m.student} and drop_path_rate > 0: stochastic depth is not built for {m.block}")
            if m.bf16_refusal and ops.get_gemm_mode() == ops.GEMM_BF16 and not getattr(student, "train_bf16", False):
                raise lib.D2SError(f"TrainStep with {m.student} in the bf16 arithmetic mode: " + m.bf16_refusal())
            if m.no_graph:
                graph = False
        # a dynamic-keep-ratio student that trains on the ragged packed batch (ragged_train=True): the ordinary
        # route - both losses, warm-up epochs, the freeze schedule - with the packed outputs handed to the losses; the refusals are those
        # of a ragged block
        self.ragged_train = bool(getattr(student, "ragged_train", False))
        if self.ragged_train != bool(getattr(args, "ragged_train", False)):
            raise lib.D2SError(f"TrainStep: the student was built with ragged_train={self.ragged_train}, args.ragged_train is "
                               f"{bool(getattr(args, 'ragged_train', False))}: the losses follow args, both must agree")
        if self.ragged_train:
            if graph is True:
                raise lib.D2SError("TrainStep(graph=True) with ragged_train is not supported: every threshold stage reads its row count on "
                                   "the host (one host read per stage), which a captured step cannot; run the step eagerly (graph=False)")
            if float(getattr(student, "drop_path_rate", 0.0)) > 0.:
                raise lib.D2SError("TrainStep with ragged_train and drop_path_rate > 0: stochastic depth is not built for a ragged block")
            graph = False
        if not self.logits_only and teacher is None:
            raise lib.D2SError("TrainStep without a teacher: only a Token Merging student trains without one")
        if self.teacher is not None:
            self.teacher.eval()
            for p in self.teacher.parameters():
                p.requires_grad_(False)
        order, starts = execution_order(student)
        self.arena = ParamArena(student, order)
        self.block_offset = {i: self.arena.offsets[starts[i]] for i in starts}
        self.opt = FusedAdamW(self.arena, lr=lr, weight_decay=weight_decay)
        # the DynamicViT baseline (vit_models/default_dynamic_vit.py) returns (logits, features, decision, [decision per stage]) and is
        # trained with its own objective, the full one in every epoch; the freeze / learning-rate schedule is the d2s one
        if m.name == "dynamicvit" and not getattr(student, "distill", False):
            raise lib.D2SError("TrainStep with the DynamicViT baseline needs distill=True: the objective reads the student's features")
        self.fresh_losses(args)
        self.metrics = {}
        self.lr, self.min_lr, self.epochs, self.warmup_steps = lr, min_lr, epochs, warmup_steps
        self.reducer = GradReducer(self.arena, bucket_mb=bucket_mb, collective=collective) if distributed else None
        if self.reducer is not None:
            student.grad_ready_hook = lambda i: self.reducer.ready_from(self.block_offset[i])
        self.frozen = frozenset(n for n, p in student.named_parameters() if not p.requires_grad)
        import os
        # the frozen teacher's forward runs on a second HIP stream beside the student's forward (independent until the losses):
        # +2.6 % images/s, identical losses (profiles/r02_f_teacher_stream_ab.txt).  D2S_TEACHER_STREAM=0 serialises them.
        two = os.environ.get("D2S_TEACHER_STREAM", "1") == "1" and self.arena.params.is_cuda and self.teacher is not None
        # chosen, not just created: it must sit on another hardware queue than the stream the step is issued on (ops.concurrent_stream)
        self._teacher_stream = ops.concurrent_stream([torch.cuda.current_stream()], "teacher forward") if two else None
        if graph is None:
            graph = {"0": False, "1": True, "auto": "auto"}[os.environ.get("D2S_STEP_GRAPH", "0")]
        self.graph = None if graph == "auto" else bool(graph)      # True | False | None (auto: small per-rank batches only)
        if float(getattr(student, "drop_path_rate", 0.0)) > 0.:
            # the table of draws is filled inside the model's forward (seed from the CPU generator, one launch): a captured step would
            # replay the masks of the step it was captured in.  Refilling the persistent table outside the captured region is not built.
            if self.graph is True:
                raise lib.D2SError("TrainStep(graph=True) with drop_path_rate > 0 is not supported: a replayed step would reuse the "
                                   "stochastic-depth masks it was captured with; run the step eagerly (graph=False)")
            self.graph = False
        if bool(getattr(student, "diff_topk", False)):
            # same reason: the perturbation noise comes from a seed drawn on the host inside the model's forward (one draw per step), and
            # sigma changes per epoch as a launch argument: a replayed step would repeat the noise and the sigma it was captured with
            if self.graph is True:
                raise lib.D2SError("TrainStep(graph=True) with diff_topk is not supported: a replayed step would reuse the perturbation "
                                   "noise and the sigma it was captured with; run the step eagerly (graph=False)")
            self.graph = False
        if m.name == "dynamicvit":
            # same reason: the Gumbel noise of every stage comes from a seed drawn on the host inside the model's forward (one draw per step)
            if self.graph is True:
                raise lib.D2SError("TrainStep(graph=True) with the DynamicViT baseline is not supported: a replayed step would reuse the "
                                   "Gumbel noise it was captured with; run the step eagerly (graph=False)")
            self.graph = False
        if self.accum_steps > 1:
            # a captured step overwrites the gradient arena on every replay, and which launches follow the backward (accumulate, or
            # combine + exchange + update) changes from call to call within a window
            if self.graph is True:
                raise lib.D2SError("TrainStep(graph=True) with accum_steps > 1 is not supported: accumulation inside a captured step is "
                                   "not built; run the step eagerly (graph=False)")
            self.graph = False
            if self.reducer is not None:
                self.reducer.paused = True      # no exchange from inside backward: finish() sends the combined gradient, once per window
        if self.clip_grad is not None:
            if self.graph is True:
                raise lib.D2SError("TrainStep(graph=True) with clip_grad is not supported: the clipped update after a replayed step is "
                                   "not covered by a test; run the step eagerly (graph=False)")
            self.graph = False
        self.graph_auto_max_rows = int(os.environ.get("D2S_STEP_GRAPH_AUTO_ROWS", "16384"))
        self._graphs = {}                   # key -> entry (see _graph_step)
        self._capture_stream = None
        self._ahead = None                  # teacher outputs of the next batch, issued one step early (_teacher_ahead)
        self._steps_seen = 0
        self._step_on_side = False          # the step is issued on a stream of its own choice (see _place_beside_process_group)
        self.pg_probe = None
        self.last_step_captured = False     # diagnostic: did the last call replay a graph
        self.set_epoch(0)

    def _no_open_window(self, what):
        if self._pending:
            raise lib.D2SError(f"{what} with {self._pending} of {self.accum_steps} micro-steps of an accumulation window pending: "
                               "call flush() first (a window never crosses an epoch or a checkpoint)")

    def fresh_losses(self, args):
        """New loss modules, the family's own: their running means start over (train.py:14-15; train_one_epoch calls this once per epoch)."""
        from losses import MaskLoss, BackboneLoss
        m = self.method
        self.tome_loss_fn = m.loss(args) if m.logits_only else None
        self.dynamicvit_loss_fn = m.loss(args) if m.name == "dynamicvit" else None
        self.mask_loss_fn, self.backbone_loss_fn = (None, None) if m.loss else (MaskLoss(args, "train"), BackboneLoss(args))
        self._loss_extras, self._token_record = m.loss_extras, m.token_record

    def set_epoch(self, epoch):
        self._no_open_window("set_epoch")
        self.epoch = epoch
        self.args.step = epoch
        out = adjust_learning_rate(self.opt, self.student, epoch, self.epochs, self.lr, self.min_lr, self.warmup_steps, self.frozen)
        if self.reducer is not None:       # the live gradient set changed: rebuild the bucket plan (SURVEY 8e caveat ii)
            a = self.arena
            chunk = a.chunk
            self.reducer.set_live_ranges(
                (o, o + ((sz + chunk - 1) // chunk) * chunk)
                for o, sz, p, g in zip(a.offsets, a.sizes, a.params_list, self.opt.groups)
                if p.requires_grad and g is not None and g != "early_exit")
        return out

    # ---- exponential moving average of the weights (FusedAdamW.enable_ema) ----
    def enable_ema(self, decay):
        self.opt.enable_ema(decay)

    def ema_weights(self):
        """Context manager: the student holds its EMA weights inside the block (FusedAdamW.ema_weights)."""
        return self.opt.ema_weights()

    def ema_state_dict(self):
        """The student's state dict with the EMA weights for its parameters (CPU tensors); buffers - the running statistics of
        --predictor-bn - are the live model's: only parameters are averaged.  Call it outside ema_weights()."""
        return self._model_state(self.opt.ema_flat())

    def _model_state(self, flat):
        byname = self.opt._unflatten(flat)
        return {k: (byname[k] if k in byname else v.detach().cpu().clone()) for k, v in self.student.state_dict().items()}

    # ---- checkpoints ----
    def config(self):
        """What a checkpoint must agree on with the run that loads it (schedule lengths and learning rates may differ: a resumed job may
        be given more epochs)."""
        s = self.student
        pe = getattr(s, "patch_embed", None)
        pred = s.score_predictor[0] if len(getattr(s, "score_predictor", [])) else None
        thr = getattr(s, "patch_score_threshold", None)
        own = methods.of(s)
        return {
            "format": CHECKPOINT_FORMAT,
            "model": type(s).__name__,
            "embed_dim": int(getattr(s, "embed_dim", 0)),
            "depth": len(s.blocks),
            "num_heads": int(getattr(getattr(s.blocks[0], "attn", None), "num_heads", 0)),
            "num_classes": int(getattr(s, "num_classes", 0)),
            "img_size": [int(v) for v in getattr(pe, "img_size", ())],
            "patch_size": [int(v) for v in getattr(pe, "patch_size", ())],
            "pruning_loc": [int(v) for v in getattr(s, "pruning_loc", [])],
            "token_ratio": [float(v) for v in getattr(s, "token_ratio", [])],
            "init_n": int(getattr(s, "init_n", 0)),
            "topk_selection": bool(getattr(s, "topk_selection", False)),
            "small_predictor": bool(getattr(pred, "small_predictor", False)),
            "predictor_bn": bool(getattr(pred, "use_bn", False)),
            "mask_loss_type": str(getattr(self.args, "mask_loss_type", "")),
            "fuse_dropped": bool(getattr(s, "fuse_dropped", False)),
            "patch_score_threshold": None if thr is None else float(thr),
            "gemm_mode": int(ops.get_gemm_mode()),
            "drop_path_rate": float(getattr(s, "drop_path_rate", 0.0)),
            "diff_topk": bool(getattr(s, "diff_topk", False)),
            "topk_num_samples": int(getattr(s, "topk_num_samples", 500)) if getattr(s, "diff_topk", False) else 0,
            "attn_selection": bool(getattr(s, "attn_selection", False)),
            "mean_heads": bool(getattr(s, "mean_heads", False)) if getattr(s, "attn_selection", False) else False,
            "tome_r": [int(v) for v in getattr(s, "tome_r", [])],
            "prop_attn": bool(getattr(s, "prop_attn", False)),
            "train_merge": bool(getattr(s, "train_merge", False)),
            "ats_locs": [int(v) for v in getattr(s, "ats_locs", [])],
            "ats_tokens": [int(v) for v in getattr(s, "ats_tokens", [])],
            "train_sample": bool(getattr(s, "train_sample", False)),
            "ragged_train": bool(getattr(s, "ragged_train", False)),
            "ragged_bf16": bool(getattr(s, "ragged_bf16", False)),
            # every family's own keys: its values for the student's family, None for the others
            **{k: v for m in methods.METHODS if m.config_keys
               for k, v in zip(m.config_keys, m.config(s, self.args) if m is own else (None,) * len(m.config_keys))},
            "squeeze_dropped": bool(getattr(s, "squeeze_dropped", False)),
            # recorded only when on: a config without the key - every other run, every older checkpoint - counts as off
            **({"train_bf16": True} if getattr(s, "train_bf16", False) else {}),
            **({"graph_rank_iters": int(s.graph_rank_iters)} if int(getattr(s, "graph_rank_iters", 0)) > 0 else {}),
            **({"sim_prune": int(s.sim_prune)} if int(getattr(s, "sim_prune", 0)) > 0 else {}),
        }

    def state_dict(self, best_acc=0.0, epoch=None):
        """Everything a later process needs to continue this run after the epoch that just ended, or to evaluate the student: a plain
        nested dict of CPU tensors, numbers, strings and lists (torch.load(..., weights_only=True) reads it back).  Keys are the
        student's parameter names and every tensor has its parameter's own shape - the arena layout stays an implementation detail.
        epoch: the last finished one (default: the epoch set_epoch was last called with)."""
        self._no_open_window("state_dict")
        dev = self.arena.params.device
        sd = {
            "model": self._model_state(self.arena.params),
            "optimizer": self.opt.state_dict(),
            "epoch": int(self.epoch if epoch is None else epoch),
            "best_acc": float(best_acc),
            "rng": {"cpu": torch.get_rng_state().clone()},
            "config": self.config(),
        }
        if dev.type == "cuda":
            sd["rng"]["device"] = torch.cuda.get_rng_state(dev).clone()
        if self.opt.ema is not None:
            sd["model_ema"] = self.ema_state_dict()
            sd["ema_decay"] = float(self.opt.ema_decay)
        return sd

    def load_state_dict(self, sd):
        """Continue from TrainStep.state_dict(): config, then names and shapes are checked BEFORE anything is written (one D2SError names
        the first mismatch and leaves this step as it was); the tensors are then copied INTO the arenas this step already owns, the
        per-tensor AdamW counters rebuilt, EMA weights and RNG states restored, and everything that remembers the old weights (captured
        step graphs, a teacher pass issued ahead, cached W^T / bf16 copies) dropped.  The caller continues with set_epoch(sd["epoch"] + 1)."""
        self._no_open_window("load_state_dict")
        if not isinstance(sd, dict) or not isinstance(sd.get("config"), dict) or "model" not in sd or "optimizer" not in sd:
            raise lib.D2SError("not a training checkpoint: 'config', 'model' and 'optimizer' are expected (a weights-only file goes "
                               "through --student-checkpoint)")
        theirs, ours = checkpoint_config(sd["config"]), self.config()
        for k in ours:
            if k not in theirs or theirs[k] != ours[k]:
                raise lib.D2SError(f"checkpoint config mismatch: {k}: the checkpoint has {theirs.get(k)!r}, this run has {ours[k]!r}")
        if bool(theirs.get("train_bf16", False)) and not ours.get("train_bf16", False):      # the key exists only where it is on
            raise lib.D2SError("checkpoint config mismatch: train_bf16: the checkpoint has True, this run has False")
        if graph_rank_iters(theirs) != graph_rank_iters(ours):                               # likewise; a config without the key ranks by the CLS row
            raise lib.D2SError(f"checkpoint config mismatch: graph_rank_iters: the checkpoint has {graph_rank_iters(theirs)}, this run has "
                               f"{graph_rank_iters(ours)}")
        if sim_prune(theirs) != sim_prune(ours):                                             # likewise; a config without the key prunes by importance alone
            raise lib.D2SError(f"checkpoint config mismatch: sim_prune: the checkpoint has {sim_prune(theirs)}, this run has {sim_prune(ours)}")
        own = self.student.state_dict()
        _check_names_shapes("model", {k: tuple(v.shape) for k, v in own.items()}, {k: tuple(v.shape) for k, v in sd["model"].items()})
        self.opt.check_state_dict(sd["optimizer"])
        ema = sd.get("model_ema") if self.opt.ema is not None else None
        if ema is not None:
            _check_names_shapes("model_ema", {k: tuple(v.shape) for k, v in own.items()}, {k: tuple(v.shape) for k, v in ema.items()})
        # ---- checked; from here on only copies into existing storage (parameters keep aliasing the arena) ----
        a = self.arena
        a.params.copy_(self.opt._flatten(sd["model"]))
        for k, v in own.items():
            if k not in a.grad_views:                  # buffers (BatchNorm running statistics): in place too
                v.copy_(sd["model"][k])
        self.opt.load_state_dict(sd["optimizer"])
        if ema is not None:
            self.opt.ema.copy_(self.opt._flatten(ema))
            self.opt._ema_primed = True
        elif self.opt.ema is not None:
            self.opt._ema_primed = False               # a checkpoint without an average: it starts from the loaded weights
        rng = sd.get("rng", {})
        if "cpu" in rng:
            torch.set_rng_state(rng["cpu"])
        if "device" in rng and a.params.device.type == "cuda":
            torch.cuda.set_rng_state(rng["device"], a.params.device)
        ops.bump_weights_epoch()
        self.opt.mark_dirty()
        self.drop_graphs()
        self._ahead = None
        a.check_alias()
        return int(sd["epoch"])

    @staticmethod
    def _batch_key(images):
        return (images.data_ptr(), images._version, tuple(images.shape))

    def _teacher_ahead(self, images, ready):
        """Issue the frozen teacher's forward for the NEXT batch on the teacher stream now (it depends on nothing this step computes),
        so that it shares the GPU with this step's backward instead of with the next step's student forward.  `ready`: event on the
        caller's stream after which `images` is valid."""
        side = self._teacher_stream
        side.wait_event(ready)
        with torch.cuda.stream(side), torch.no_grad():
            out = self.teacher(images)
            done = side.record_event()
        images.record_stream(side)
        self._ahead = dict(key=self._batch_key(images), images=images, out=out, done=done)

    def _tome_losses(self, logits_s, out_t, labels, accumulate):
        """ToMeLoss on the merging student's logits; 'mask_loss' reports the weighted distillation term (0 without a teacher)."""
        fn = self.tome_loss_fn
        logits_t = None if out_t is None else out_t[0]
        s = self.student
        loss = fn(logits_s, logits_t, labels, self.metrics, *self._loss_extras(s), accumulate=accumulate)      # what the forward left on the model
        per_block = list(getattr(s, self._token_record))
        dist_term = fn.dist_weight * fn.last[2]
        return loss, dict(mask_loss=dist_term, backbone_loss=fn.last[0] - dist_term, kept=None, logits_s=logits_s, token_s=None,
                          pred_logits=None, logits_t=logits_t, token_t=None, cls_attn=None, tokens_per_block=per_block)

    def forward_losses(self, images, labels, accumulate=True, next_images=None):
        if self.teacher is None:
            return self._tome_losses(self.student(images), None, labels, accumulate)
        ahead, self._ahead = self._ahead, None
        if ahead is not None and (self._teacher_stream is None or ahead["key"] != self._batch_key(images)):
            ahead = None                                # a different batch arrived than the one announced: its teacher pass is dropped
        if self._teacher_stream is not None:
            # The frozen teacher's forward and the student's forward are independent until the losses: the teacher runs on a second
            # HIP stream so that its kernels fill the CUs the student's kernels leave idle in their ramp-up / last residency round
            # (and vice versa).  Scratch buffers are per stream (ops.workspace), so the two forwards never share one.
            from .functional import shared_patch_columns, prime_patch_columns
            side, main = self._teacher_stream, torch.cuda.current_stream()
            ready = main.record_event() if next_images is not None else None
            if ahead is not None:                       # issued during the previous step (_teacher_ahead)
                out_t = ahead["out"]
                out_s = self.student(images)
                main.wait_event(ahead["done"])
            else:
                with shared_patch_columns():
                    pe = getattr(self.student, "patch_embed", None)
                    if pe is not None and images.is_contiguous() and hasattr(pe, "patch_size") and getattr(self.teacher, "patch_embed", None) is not None:
                        prime_patch_columns(images, pe.patch_size[0])       # one im2col for both, built before the fork
                    side.wait_stream(main)
                    with torch.cuda.stream(side), torch.no_grad():
                        out_t = self.teacher(images)
                    out_s = self.student(images)
                    main.wait_stream(side)
            for t in out_t:                              # produced on the side stream, consumed (and later freed) on the main one
                t.record_stream(main)
            if next_images is not None:
                self._teacher_ahead(next_images, ready)
        else:
            from .functional import shared_patch_columns
            with shared_patch_columns():       # teacher and student embed the same images: one im2col pass for both
                with torch.no_grad():
                    out_t = self.teacher(images)
                out_s = self.student(images)
        if self.logits_only:
            return self._tome_losses(out_s, out_t, labels, accumulate)
        if self.dynamicvit_loss_fn is not None:
            return self._baseline_losses(out_s, out_t, labels, accumulate)
        logits_t, token_t, cls_attn = out_t
        logits_s, token_s, pred_logits, kept = out_s
        if self.ragged_train:       # the packed outputs: every stage's offsets for the mask loss, the last packed batch's for the distillation
            s = self.student
            mask_loss = self.mask_loss_fn(pred_logits, cls_attn, kept, self.metrics, accumulate=accumulate,
                                          ragged=(list(s.cu_seqlens_per_stage), list(s.ragged_row_src_per_stage)))
            backbone_loss = self.backbone_loss_fn(logits_s, token_s, logits_t, token_t, kept, labels, self.metrics, accumulate=accumulate,
                                                  ragged=(s.cu_seqlens, s.ragged_row_src))
            loss = mask_loss if self.epoch < self.warmup_steps else backbone_loss + mask_loss
            return loss, dict(mask_loss=mask_loss, backbone_loss=backbone_loss, kept=kept, logits_s=logits_s, token_s=token_s,
                              pred_logits=pred_logits, logits_t=logits_t, token_t=token_t, cls_attn=cls_attn)
        mask_loss = self.mask_loss_fn(pred_logits, cls_attn, kept, self.metrics, accumulate=accumulate, attn_selection=self.attn_selection)
        backbone_loss = self.backbone_loss_fn(logits_s, token_s, logits_t, token_t, kept, labels, self.metrics, accumulate=accumulate)
        loss = mask_loss if self.epoch < self.warmup_steps else backbone_loss + mask_loss     # train.py:50-53
        return loss, dict(mask_loss=mask_loss, backbone_loss=backbone_loss, kept=kept, logits_s=logits_s, token_s=token_s,
                          pred_logits=pred_logits, logits_t=logits_t, token_t=token_t, cls_attn=cls_attn)

    def _baseline_losses(self, out_s, out_t, labels, accumulate):
        """DynamicViTLoss on the baseline's outputs.  The teacher is this file's dense one ((logits, tokens)) or a d2s teacher, whose third
        output is not used.  'mask_loss' reports the weighted ratio term - the part only the predictors see - and 'backbone_loss' the rest."""
        logits_s, token_s, decision, stages = out_s
        logits_t, token_t = out_t[0], out_t[1]
        fn = self.dynamicvit_loss_fn
        loss = fn(logits_s, token_s, decision, stages, logits_t, token_t, labels, self.metrics, accumulate=accumulate)
        ratio = fn.ratio_weight * fn.last[2]
        return loss, dict(mask_loss=ratio, backbone_loss=fn.last[0] - ratio, kept=stages, logits_s=logits_s, token_s=token_s,
                          pred_logits=stages, logits_t=logits_t, token_t=token_t, cls_attn=None)

    def __call__(self, images, labels, next_images=None):
        """next_images: the batch of the FOLLOWING call, if the caller already has it (a prefetching loader does).  The frozen teacher's
        forward for it is then issued during this step (see _teacher_ahead) - every step still runs exactly one teacher forward, the
        results are bit-identical, and a following call with any other batch simply recomputes.  Eager steps only."""
        self.arena.check_alias()
        if images.is_cuda and self._steps_seen == 0 and self.reducer is not None:
            self._place_beside_process_group()
        if images.is_cuda and self.graph is False and self._steps_seen in (1, 2):
            # the side streams were picked before anything else had run; an RCCL communicator (and whatever else creates streams late)
            # can have moved onto their hardware queues since: verify once the first step(s) are behind us
            main = self._capture_stream if self._step_on_side else torch.cuda.current_stream()
            self._teacher_stream = ops.recheck_stream(self._teacher_stream, [main], "teacher forward")
            ops.recheck_weight_grad_stream([main])
        self._steps_seen += 1
        if (self.graph is False and not self._step_on_side) or not images.is_cuda:
            return self._eager_step(images, labels, next_images)
        # Graph-capable mode: EVERY step - the eager warm-up steps, the capture, the replays, and steps of shapes that stay eager - is
        # issued on one side stream of this TrainStep.  Autograd pins a parameter's AccumulateGrad node to the stream of the forward that
        # created it, and such a node outlives its step whenever anything still references that step's graph (the model's own
        # `pred_logits` list does); a node pinned to the legacy default stream pulls that stream into a later capture, which then cannot
        # end.  The caller's stream waits for the side stream before this returns, so the caller sees an ordinary in-order step.
        cur = torch.cuda.current_stream()
        if self._capture_stream is None:
            self._capture_stream = torch.cuda.Stream()
        side = self._capture_stream
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            info = self._graph_step(images, labels) if self._use_graph(images) else self._eager_step(images, labels, next_images)
        cur.wait_stream(side)
        if not self.last_step_captured:
            for v in info.values():            # allocated on the side stream, consumed (and freed) by the caller on its own stream
                for t in (v if isinstance(v, (list, tuple)) else (v,)):
                    if torch.is_tensor(t) and t.is_cuda:
                        t.record_stream(cur)
        return info

    def _place_beside_process_group(self):
        """First call of a data-parallel TrainStep: make sure the stream the step is issued on does not share a hardware queue with the
        process group's RCCL stream (ops.pg_stream_shares_queue).  If it does on ANY rank, every rank probes the same three candidate
        streams (the probes are collectives), and a rank whose stream collided moves its steps to the first candidate that does not -
        issued there the way the graph-capable mode issues them, the caller's stream waiting at both ends."""
        if not (dist.is_initialized() and dist.get_backend(self.reducer.group) == "nccl") or self.graph is not False:
            return
        cur = torch.cuda.current_stream()
        bad = ops.pg_stream_shares_queue(cur, self.reducer.group)
        flag = torch.tensor([1.0 if bad else 0.0], device=self.arena.params.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.reducer.group)
        self.pg_probe = {"caller_stream_shares_rccl_queue": bool(bad), "moved": False}
        if float(flag.item()) != 0.0:
            chosen = None
            for _ in range(3):
                cand = torch.cuda.Stream()
                if not ops.pg_stream_shares_queue(cand, self.reducer.group) and chosen is None:
                    chosen = cand
            if bad and chosen is not None:
                self._capture_stream, self._step_on_side = chosen, True
                self._teacher_stream = ops.recheck_stream(self._teacher_stream, [chosen], "teacher forward")
                self.reducer.stream = ops.recheck_stream(self.reducer.stream, [chosen], "gradient exchange")
                ops.recheck_weight_grad_stream([chosen])
                self.pg_probe["moved"] = True
        # the weight-gradient stream must not sit behind RCCL either: every bucket's collective would hold up the weight gradients issued
        # after it for as long as the exchange takes (the same fixed number of probes on every rank)
        if not ops._WGRAD_ENABLED:
            return
        step_stream = self._capture_stream if self._step_on_side else cur
        wg = ops.ensure_weight_grad_stream([step_stream])
        bad_wg = ops.pg_stream_shares_queue(wg, self.reducer.group)
        flag.fill_(1.0 if bad_wg else 0.0)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.reducer.group)
        self.pg_probe["weight_grad_stream_shares_rccl_queue"] = bool(bad_wg)
        if float(flag.item()) != 0.0:
            chosen = None
            for _ in range(3):
                cand = ops.concurrent_stream([step_stream], "weight gradients (off the RCCL queue)")
                if not ops.pg_stream_shares_queue(cand, self.reducer.group) and chosen is None:
                    chosen = cand
            if bad_wg and chosen is not None:
                ops.set_weight_grad_stream(chosen)
                self.pg_probe["weight_grad_stream_moved"] = True

    def _eager_step(self, images, labels, next_images=None):
        self.last_step_captured = False
        loss, info = self._forward_backward(images, labels, accumulate=True, next_images=next_images)
        info["loss"] = loss.detach()
        if self.accum_steps == 1 and self.clip_grad is None:
            scale = self.reducer.finish() if self.reducer is not None else 1.0
            self.opt.step(grad_scale=scale)
            info["stepped"] = True
            return info
        self._pending += 1
        if self._pending < self.accum_steps:
            a = self.arena
            if self._acc is None:
                self._acc = torch.zeros_like(a.grads)
            ops.grad_accumulate(self._acc, a.grads, self.opt.desc(), a.n_chunks, 0 if self._pending == 1 else 1)
            info["stepped"] = False
            return info
        self._apply_window(combine=2)
        info["stepped"] = True
        if self.clip_grad is not None:
            info["grad_norm"] = self.last_clip[0].clone()      # last_clip is overwritten by the next clipped step: infos may be kept
        return info

    def flush(self):
        """Apply a window that is still open (an epoch that ended inside it) with c = the number of micro-steps seen; nothing pending:
        nothing happens.  -> whether an optimiser step was taken."""
        if not self._pending:
            return False
        cur = torch.cuda.current_stream()
        side = self._capture_stream if self._step_on_side else None
        if side is not None:                    # where the calls of this window were issued (_place_beside_process_group)
            side.wait_stream(cur)
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            self._apply_window(combine=0)
        if side is not None:
            cur.wait_stream(side)
        return True

    def _apply_window(self, combine):
        """The optimiser step of a window of c = self._pending micro-steps.  combine = 2: the last gradient is still alone in the gradient
        arena (g = fl(acc + g)); 0: every gradient is in the accumulation arena already (flush: g = acc).  Then exchange, norm, update."""
        a, c = self.arena, self._pending
        desc = self.opt.desc()
        if c > 1:
            if combine == 2:
                ops.grad_accumulate(self._acc, a.grads, desc, a.n_chunks, 2)
            else:
                ops.grad_accumulate(a.grads, self._acc, desc, a.n_chunks, 0)
        world = 1
        if self.reducer is not None:
            self.reducer.finish()
            world = self.reducer.world
        scale = 1.0 / (c * world)
        if self.clip_grad is None:
            self.opt.step(grad_scale=scale)
        else:
            if self.last_clip is None:
                self.last_clip = torch.zeros(2, dtype=torch.float32, device=a.grads.device)
                self._partials = torch.zeros(a.n_chunks, dtype=torch.float32, device=a.grads.device)
                self._norm_sum = torch.zeros((), dtype=torch.float32, device=a.grads.device)
            ops.grad_clip_coef(a.grads, desc, a.n_chunks, scale, self.clip_grad, self._partials, self.last_clip)
            self.opt.step(grad_scale=scale, clip_coef=self.last_clip[1:])
            self._norm_sum.add_(self.last_clip[0])
            self._norm_steps += 1
        self._pending = 0

    def grad_norm_mean(self, reset=True):
        """Mean pre-clip gradient norm over the clipped optimiser steps since the last reset (one device read), or None."""
        if not self._norm_steps:
            return None
        mean = float(self._norm_sum) / self._norm_steps
        if reset:
            self._norm_sum.zero_()
            self._norm_steps = 0
        return mean

    def _forward_backward(self, images, labels, accumulate, next_images=None):
        self.opt.refresh_transposed_weights()
        self.student.train()
        loss, info = self.forward_losses(images, labels, accumulate=accumulate, next_images=next_images)
        self.opt.zero_grad()
        with ops.async_weight_grads():              # wgrad GEMMs trail the dgrad chain on a second stream; joined on exit
            loss.backward()
        self.arena.collect_grads()
        return loss, info

    # ---- the step as a hipGraph ----
    # With a fixed keep count every tensor of the step has a static shape and nothing in it synchronises with the host, so the ~450
    # C-ABI launches + autograd bookkeeping of a step (9.5 ms of Python at 32 images per GPU) can be recorded once
    # and replayed with one call.  What is captured: W^T / bf16 weight refresh, teacher and student forward (their two streams become
    # two branches of the graph), losses, backward (the weight-gradient stream is a third branch).  What stays outside: the gradient
    # exchange (RCCL collectives are issued eagerly after the replay - one flush of the live gradient set instead of buckets that
    # overlap backward), the fused AdamW launch (its per-chunk learning rates and step counters live in device buffers that are
    # updated in place), and the host-side running means of the two loss modules.
    def _use_graph(self, images):
        if self.graph is False or not images.is_cuda:
            return False
        if getattr(self.student, "patch_score_threshold", None) is not None:
            return False                         # dynamic keep ratio: not needed for the fixed-k path this serves; stays eager
        if self.graph is True:
            return True
        # auto: small per-rank batches, where the host cannot issue launches as fast as the GPU retires them (C3 / C4 regime).  With
        # a reducer the eager path's overlap of the exchange with backward is worth more than the launch time at large batches.
        n_tok = getattr(getattr(self.student, "patch_embed", None), "num_patches", 196) + 1
        return images.shape[0] * n_tok <= self.graph_auto_max_rows

    def _graph_key(self, images, labels):
        live = tuple(p.requires_grad for p in self.arena.params_list)
        return (tuple(images.shape), images.dtype, tuple(labels.shape), labels.dtype, self.epoch < self.warmup_steps, hash(live),
                ops.get_gemm_mode(), self._teacher_stream is not None, ops._WGRAD_ENABLED)

    def drop_graphs(self):
        self._graphs.clear()

    def _graph_step(self, images, labels):
        key = self._graph_key(images, labels)
        ent = self._graphs.get(key)
        if ent is None:
            if len(self._graphs) >= 4:           # shapes come and go (a shorter last batch): keep the pool of captured steps small
                self._graphs.pop(next(iter(self._graphs)))
            ent = self._graphs[key] = {"seen": 0, "graph": None}
        if ent["graph"] is None and ent["seen"] < self.GRAPH_WARM_STEPS:
            ent["seen"] += 1
            return self._eager_step(images, labels)
        if ent["graph"] is None:
            self._capture(ent, images, labels)
        ent["images"].copy_(images, non_blocking=True)
        ent["labels"].copy_(labels, non_blocking=True)
        ent["graph"].replay()
        self.last_step_captured = True
        scale = self.reducer.finish() if self.reducer is not None else 1.0
        self.opt.step(grad_scale=scale)
        if self.logits_only:                     # of that route a captured step serves the families whose record names no refusal
            self.tome_loss_fn.accumulate(self.metrics, ent["tome_last"])
        else:
            self.mask_loss_fn.accumulate(self.metrics, ent["mask_last"])
            self.backbone_loss_fn.accumulate(self.metrics, ent["backbone_last"])
        return ent["info"]          # static tensors: overwritten by the next replay of this graph

    def _capture(self, ent, images, labels):
        if self.opt._dirty:
            self.opt._build_desc()               # host -> device copy: before the capture, not inside it
        ent["images"], ent["labels"] = images.clone(), labels.clone()
        # references into the previous step's autograd graph that the model itself holds (they would keep its AccumulateGrad nodes alive)
        for attr in ("pred_logits", "cls_attns", "kept_token_indices", "dropped_token_indices"):
            if isinstance(getattr(self.student, attr, None), list):
                setattr(self.student, attr, [])
        g = torch.cuda.CUDAGraph()
        if self.reducer is not None:
            self.reducer.paused = True
        torch.cuda.synchronize()
        try:
            with torch.cuda.graph(g, stream=self._capture_stream):
                loss, info = self._forward_backward(ent["images"], ent["labels"], accumulate=False)
                info["loss"] = loss.detach()
                info["stepped"] = True
        finally:
            if self.reducer is not None:
                self.reducer.paused = False
        ent["graph"], ent["info"] = g, info
        ent["ws_refs"] = list(ops._ws.values())       # scratch buffers the recorded kernels point at: must outlive the graph even if an
                                                      # eager call with a larger shape replaces them in ops._ws later
        if self.logits_only:
            ent["tome_last"] = self.tome_loss_fn.last
        else:
            ent["mask_last"], ent["backbone_last"] = self.mask_loss_fn.last, self.backbone_loss_fn.last
