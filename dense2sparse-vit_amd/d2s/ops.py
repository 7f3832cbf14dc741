"""Tensor-level wrappers over the C ABI (one Python function per entry point, no arithmetic here).

Conventions: fp32 contiguous device tensors unless a row map says otherwise; 2-D views [rows, features].
"""
import os
import threading

import torch

from . import lib

EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_GELU, EPI_BIAS_RESID = 0, 1, 2, 3, 4
EPI_MUL_GELU_GRAD, EPI_MUL_RELU_MASK, EPI_BIAS_ROWADD, EPI_ACCUM = 5, 6, 7, 8
EPI_BIAS_GELU_Z16, EPI_MUL_GELU_GRAD_Z16 = 9, 10      # d2s_gemm_f32_bf16io only: the saved GELU pre-activation in bf16 (chosen by gemm() from the tensor's dtype)
EPI_BIAS_RESID_ROWSCALE = 11                          # d2s_gemm_f32_rowscale only: rowscale[m / rows_per_group] * (acc + bias) + aux (stochastic depth)
NT, NN, TN = 0, 1, 2

_ws = {}
_WS_NEED = {}       # (layout, M, N, K, mode) -> workspace bytes of d2s_gemm_f32 (a pure function of its arguments)


def workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream): kernels of one stream reuse it in order, kernels of different streams (the
    optional teacher stream, d2s.engine) never share one."""
    key = (device.type, device.index, lib.stream() if device.type == "cuda" else 0)
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


def workspace_on(stream_obj, nbytes, device):
    """The scratch buffer of another stream than the current one (the weight-gradient stream of a composite backward call) - the same
    buffer workspace() hands out inside `with torch.cuda.stream(stream_obj)`.  A (re)allocation happens UNDER that stream: the caching
    allocator ties a block to the stream that was current when it was allocated, and a block tied to the caller's stream would, once a
    larger request replaces it, be handed to the caller's next tensor while launches queued on the other stream still use it (seen as a
    wrong predictor weight gradient in the first step of one run in three, tests/test_graph_gpu.py)."""
    key = (device.type, device.index, stream_obj.cuda_stream)
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        with torch.cuda.stream(stream_obj):
            buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


def _f32(t):
    assert t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.is_contiguous())
    return t


# bf16 data path of the bf16 arithmetic mode: producers (LayerNorm, the attention forward, GEMM epilogues) emit a bf16 copy of what the
# next GEMM multiplies, and that GEMM reads it directly instead of converting its fp32 operand first (d2s_gemm_f32_bf16io).
_BF16_IO = os.environ.get("D2S_BF16_IO", "1") != "0"


def bf16_io():
    return _BF16_IO and get_gemm_mode() == GEMM_BF16


def bf16_buffer(rows, cols, device):
    return torch.empty((rows, cols), dtype=torch.bfloat16, device=device)


# A gradient that leaves one autograd Function and enters the next (a block's dx = the previous block's dy) cannot carry its bf16 copy
# through autograd; the producer parks it here under the fp32 tensor's address and the consumer takes it out again.  An entry is used at
# most once and only if address, element count and the version counter of the fp32 tensor still match (anything that rewrote or replaced
# the gradient in between - an accumulation, a hook, the token scatter at a pruning stage - makes the lookup miss, and the consumer
# converts the fp32 gradient itself).
_SHADOW = {}
shadow_hits = 0                           # diagnostic: how many gradients found their bf16 copy (tests assert the path is taken)


def shadow_put(t, t16):
    _SHADOW.clear()                       # at most one gradient is in flight between two blocks
    # the entry holds the fp32 tensor itself: while it is parked here its address cannot be recycled for another tensor with the same
    # element count and version 0 (a hook that replaces the gradient out of place would otherwise be able to alias it)
    _SHADOW[t.data_ptr()] = (t.numel(), t._version, t16, t)


def shadow_take(t):
    e = _SHADOW.pop(t.data_ptr(), None)
    _SHADOW.clear()
    if e is None or e[0] != t.numel() or e[1] != t._version or e[3].untyped_storage().data_ptr() != t.untyped_storage().data_ptr():
        return None
    global shadow_hits
    shadow_hits += 1
    return e[2]


# bf16 weights.  A weight's bf16 form is made once and reused: for the weights of a parameter arena (the trained model) d2s.engine converts the
# whole arena - and the arena of W^T copies - in one launch each at the start of every step (Bf16Weights.refresh); a weight outside any
# arena that does not require gradients (the frozen teacher) is converted on first use and again only when its version counter moves.
# Anything else (a free-standing trainable tensor) has no safe invalidation signal and is converted inside each GEMM call as before.
_W16 = {}                       # (data_ptr, transposed) -> (weakref to the weight or None for arena entries, epoch, version, shape, bf16 tensor)


def bf16_weight(W, transposed=False):
    """bf16 [N][K] form of the B operand of y = x W^T (transposed=False: W itself) or of dx = dy W (transposed=True: W^T), or None."""
    if not (_BF16_IO and W.is_cuda and W.dim() == 2 and W.shape[0 if transposed else 1] % 32 == 0):
        return None
    ent = _W16.get((W.data_ptr(), transposed))
    shape = tuple(W.shape)
    if ent is not None and ent[2] == W._version and ent[3] == shape:
        if ent[0] is None:
            if ent[1] == weights_epoch:
                return ent[4]                       # arena weight, converted at the start of this step
        elif ent[0]() is W:
            return ent[4]                           # frozen weight, unchanged since its conversion
    if transposed or W.requires_grad or _in_weight_arena(W.data_ptr()):
        return None
    import weakref
    t16 = torch.empty(shape, dtype=torch.bfloat16, device=W.device)
    lib.call("d2s_convert_bf16", lib.ptr(W), lib.ptr(t16), W.numel())
    torch.cuda.current_stream().synchronize()       # once per frozen weight: later calls may read the copy from any stream
    if len(_W16) > 4096:
        _W16.clear()
    _W16[(W.data_ptr(), False)] = (weakref.ref(W), -1, W._version, shape, t16)
    return t16


def invalidate_bf16_weights():
    """Drop every cached bf16 form of a frozen weight.  The cache follows a weight's version counter; writes that bypass it
    (`teacher.weight.data.copy_()`, `dist.broadcast(p.data)`, raw-pointer kernels - `.data` has a version counter of its own) must be
    followed by this call.  vit_models' checkpoint loaders call it; arena weights are refreshed every step and need nothing."""
    _W16.clear()


class Bf16Weights:
    """bf16 mirrors of a parameter arena and of its W^T arena (TransposedArena), each refreshed by ONE launch per step."""

    def __init__(self, arena_params, weights, transposed_arena):
        self.src, self.tsrc = arena_params, transposed_arena.dst
        self.dst = torch.empty(arena_params.numel(), dtype=torch.bfloat16, device=arena_params.device)
        self.tdst = torch.empty(self.tsrc.numel(), dtype=torch.bfloat16, device=arena_params.device)
        self.entries = []
        toff = 0
        for w, off in weights:
            if w.dim() != 2:
                continue
            R, C = w.shape
            self.entries.append((w, self.dst[off:off + R * C].view(R, C), self.tdst[toff:toff + R * C].view(C, R)))
            toff += R * C

    def refresh(self):
        """call after TransposedArena.refresh() of the same step"""
        lib.call("d2s_convert_bf16", lib.ptr(self.src), lib.ptr(self.dst), self.src.numel())
        lib.call("d2s_convert_bf16", lib.ptr(self.tsrc), lib.ptr(self.tdst), self.tsrc.numel())
        for w, w16, wt16 in self.entries:
            shape = tuple(w.shape)
            if w16.data_ptr() % 16 == 0 and wt16.data_ptr() % 16 == 0:
                _W16[(w.data_ptr(), False)] = (None, weights_epoch, w._version, shape, w16)
                _W16[(w.data_ptr(), True)] = (None, weights_epoch, w._version, shape, wt16)


def _gemm_workspace(layout, M, N, K, mode, device):
    """The workspace of a d2s_gemm_f32 / d2s_linear_wgrad_f32 call (layout TN: M = n_out, N = n_in, K = tokens), None where it needs none;
    the size query is made once per problem."""
    qk = (layout, M, N, K, mode)
    need = _WS_NEED.get(qk)
    if need is None:
        need = _WS_NEED[qk] = lib.query("d2s_gemm_f32_workspace_bytes", layout, M, N, K, mode)
    return workspace(need, device) if need else None


def gemm(layout, A, lda, B, ldb, C, ldc, M, N, K, epi=EPI_NONE, bias=None, aux=None, ldaux=0, aux_out=None, aux_rows=0,
         remap_rows=0, remap_skip=0, accumulate=False, a16=None, c16=None, b16=None, rowscale=None, rows_per_group=0):
    mode = get_gemm_mode()
    ws = _gemm_workspace(layout, M, N, K, mode, C.device if C is not None else c16.device)
    if epi == EPI_BIAS_RESID_ROWSCALE:      # stochastic depth: its own entry point, every arithmetic mode (bf16 side channels in mode 2 only)
        assert rowscale is not None and rows_per_group > 0 and aux is not None and not accumulate and remap_rows == 0 and aux_rows == 0
        assert rowscale.dtype == torch.float32 and rowscale.is_contiguous() and rowscale.numel() * rows_per_group >= M
        assert (a16 is None and c16 is None and b16 is None) or mode == GEMM_BF16
        lib.call("d2s_gemm_f32_rowscale", layout, lib.ptr(A), lda, lib.ptr(B), ldb, lib.ptr(C), ldc, M, N, K, lib.ptr(bias), lib.ptr(aux), ldaux,
                 lib.ptr(rowscale), int(rows_per_group), mode, lib.ptr(a16), lib.ptr(b16), lib.ptr(c16), lib.ptr(ws), ws.numel() if ws is not None else 0)
        return C
    assert rowscale is None, "a row scale needs EPI_BIAS_RESID_ROWSCALE"
    z16 = (aux_out if epi == EPI_BIAS_GELU else aux if epi == EPI_MUL_GELU_GRAD else None)
    if z16 is not None and z16.dtype == torch.bfloat16:      # bf16 data path: the GELU pre-activation is kept in bf16 (as under autocast)
        assert a16 is not None or c16 is not None or b16 is not None, "a bf16 pre-activation exists on the bf16 data path only"
        epi = EPI_BIAS_GELU_Z16 if epi == EPI_BIAS_GELU else EPI_MUL_GELU_GRAD_Z16
    if a16 is not None or c16 is not None or b16 is not None:
        assert mode == GEMM_BF16 and not accumulate and remap_rows == 0 and aux_rows == 0
        assert b16 is None or (b16.dtype == torch.bfloat16 and b16.is_contiguous() and tuple(b16.shape) == (N, K)), "b16 must be dense bf16 [N, K]"
        assert a16 is None or (a16.dtype == torch.bfloat16 and a16.is_contiguous() and tuple(a16.shape) == (M, K)), "a16 must be dense bf16 [M, K]"
        assert c16 is None or (c16.dtype == torch.bfloat16 and c16.is_contiguous() and tuple(c16.shape) == (M, N)), "c16 must be dense bf16 [M, N]"
        lib.call("d2s_gemm_f32_bf16io", layout, lib.ptr(A), lda, lib.ptr(B), ldb, lib.ptr(C), ldc, M, N, K, epi, lib.ptr(bias),
                 lib.ptr(aux), ldaux, lib.ptr(aux_out), lib.ptr(a16), lib.ptr(b16), lib.ptr(c16), lib.ptr(ws), ws.numel() if ws is not None else 0)
        return C
    lib.call("d2s_gemm_f32", layout, lib.ptr(A), lda, lib.ptr(B), ldb, lib.ptr(C), ldc, M, N, K, epi, lib.ptr(bias),
             lib.ptr(aux), ldaux, lib.ptr(aux_out), aux_rows, remap_rows, remap_skip, int(accumulate), mode, lib.ptr(ws),
             ws.numel() if ws is not None else 0)
    return C


def linear_fwd(x, W, bias=None, epi=None, aux=None, aux_out=None, out=None, a16=None, c16=None, want_f32=True, rowscale=None, rows_per_group=0):
    """y[M,N] = epi(x[M,K] @ W[N,K]^T + bias).  nn.Linear forward (F.linear).
    rowscale [ceil(M / rows_per_group)] with epi=EPI_BIAS_RESID (stochastic depth): y = rowscale[m // rows_per_group] * (x W^T + bias) + aux.
    bf16 mode only: a16 = bf16 copy of x (x itself may then be None), c16 = bf16 [M, N] buffer that receives a copy of y;
    want_f32=False (needs c16) skips the fp32 result and returns None."""
    _f32(W)
    if x is not None:
        _f32(x)
    M, K = (x if x is not None else a16).shape
    N = W.shape[0]
    if out is None and want_f32:
        out = torch.empty((M, N), dtype=torch.float32, device=W.device)
    if epi is None:
        epi = EPI_BIAS if bias is not None else EPI_NONE
    b16 = bf16_weight(W) if get_gemm_mode() == GEMM_BF16 else None
    if rowscale is not None:
        assert epi in (EPI_BIAS_RESID, EPI_BIAS_RESID_ROWSCALE) and aux_out is None
        epi = EPI_BIAS_RESID_ROWSCALE
    return gemm(NT, x, K, W, K, out, N, M, N, K, epi, bias, aux, N if aux is not None else 0, aux_out, a16=a16, c16=c16, b16=b16,
                rowscale=rowscale, rows_per_group=rows_per_group)


# ---- k-contiguous copies W^T of Linear weights for the input-gradient GEMM ----
# dx = dy W is an NN product (W's reduction index is its row index); with W^T [n_in, n_out] at hand it is an NT product, both operands
# k-contiguous, which the fp32 kernel runs 10-15 % faster on the student's shapes (profiles/r02_e_*).  A weight changes once per
# optimiser step, so its transpose is rebuilt lazily on the first input-gradient call after a change and reused until the next one:
# `weights_epoch` is bumped by everything that writes parameters behind torch's back (the fused AdamW kernel); in-place torch writes
# (load_state_dict, torch optimisers) show up in the tensor's version counter.
# Only weights that live in a registered parameter arena (d2s.engine.ParamArena) take this path: their addresses are stable and unique for
# the arena's lifetime, whereas the address of a free-standing tensor can be recycled for another tensor with the same shape and version.
weights_epoch = 0
_WT = {}                        # data_ptr -> (epoch, version, shape, W^T tensor)
_WT_ARENAS = []                 # (weakref to the arena tensor, first byte, one past the last byte)


def register_weight_arena(arena_tensor):
    import weakref
    _WT_ARENAS[:] = [a for a in _WT_ARENAS if a[0]() is not None]
    lo = arena_tensor.data_ptr()
    hi = lo + arena_tensor.numel() * 4
    for key in [k for k in _WT if lo <= k < hi]:       # an earlier arena's entries at recycled addresses
        del _WT[key]
    _WT_ARENAS.append((weakref.ref(arena_tensor), lo, hi))


def _in_weight_arena(ptr):
    for ref, lo, hi in _WT_ARENAS:
        if lo <= ptr < hi and ref() is not None:
            return True
    return False
_DGRAD_NT_MIN_ROWS = 1024      # arena weights get their W^T copies once per step anyway (TransposedArena); at 3168 rows the NT form is still 5-10 % faster (profiles/r03_d_config3_tile_sweep.txt)


def bump_weights_epoch():
    global weights_epoch
    weights_epoch += 1


def transposed_weight(W):
    key = W.data_ptr()
    ent = _WT.get(key)
    if ent is not None and ent[0] == weights_epoch and ent[1] == W._version and ent[2] == tuple(W.shape):
        return ent[3]
    Wt = ent[3] if (ent is not None and ent[2] == tuple(W.shape)) else torch.empty((W.shape[1], W.shape[0]), dtype=torch.float32, device=W.device)
    lib.call("d2s_transpose_f32", lib.ptr(W), lib.ptr(Wt), W.shape[0], W.shape[1])
    if len(_WT) > 4096:         # models come and go in a test process: do not let stale entries pile up
        _WT.clear()
    _WT[key] = (weights_epoch, W._version, tuple(W.shape), Wt)
    return Wt


class TransposedArena:
    """W^T copies of every 2-D weight of a parameter arena, rebuilt by ONE kernel launch per optimiser step (d2s.engine.FusedAdamW calls
    refresh() right after the update) instead of one small launch per weight on its first input-gradient use."""

    def __init__(self, arena_params, weights):
        """weights: list of (Parameter living in arena_params, its arena offset in floats); only 2-D ones are kept.  The Parameter objects
        (not .data aliases) are held so that refresh() records the version counter the autograd Functions will see."""
        import numpy as np
        self.src = arena_params
        mats = [(w, off) for w, off in weights if w.dim() == 2]
        total = sum(w.numel() for w, _ in mats)
        self.dst = torch.empty(max(total, 1), dtype=torch.float32, device=arena_params.device)
        rows, self.entries, doff = [], [], 0
        for w, off in mats:
            R, C = w.shape
            self.entries.append((w, self.dst[doff:doff + R * C].view(C, R)))
            for r0 in range(0, R, 64):
                for c0 in range(0, C, 64):
                    rows.append((off, doff, R, C, r0, c0))
            doff += R * C
        desc = np.zeros(len(rows), dtype=[("s", "<i8"), ("d", "<i8"), ("R", "<i4"), ("C", "<i4"), ("r0", "<i4"), ("c0", "<i4")])
        for i, r in enumerate(rows):
            desc[i] = r
        self.n_tiles = len(rows)
        self.desc = torch.from_numpy(desc.view(np.uint8).copy()).to(arena_params.device) if rows else None

    def refresh(self):
        if not self.n_tiles:
            return
        lib.call("d2s_transpose_batched_f32", lib.ptr(self.src), lib.ptr(self.dst), lib.ptr(self.desc), self.n_tiles)
        for w, wt in self.entries:
            _WT[w.data_ptr()] = (weights_epoch, w._version, tuple(w.shape), wt)


def linear_dgrad(dy, W, epi=EPI_NONE, aux=None, out=None, a16=None, c16=None, want_f32=True):
    """dx[M,K] = epi(dy[M,N] @ W[N,K]).  bf16 mode only: a16 = bf16 copy of dy (dy may then be None), c16 = bf16 [M, K] buffer receiving a
    copy of dx; want_f32=False (needs c16) skips the fp32 result and returns None."""
    _f32(W)
    if dy is not None:
        _f32(dy)
    M, N = (dy if dy is not None else a16).shape
    K = W.shape[1]
    if out is None and want_f32:
        out = torch.empty((M, K), dtype=torch.float32, device=W.device)
    if get_gemm_mode() == GEMM_BF16:
        wt16 = bf16_weight(W, transposed=True)      # [K][N] = W^T in bf16: the k-contiguous B operand of dx = dy W
        if a16 is not None or c16 is not None or wt16 is not None:
            return gemm(NN, dy, N, W, K, out, K, M, K, N, epi, None, aux, K if aux is not None else 0, a16=a16, c16=c16, b16=wt16)
    if get_gemm_mode() == GEMM_EXACT and M >= _DGRAD_NT_MIN_ROWS and (N % 16 == 0) and (K % 4 == 0) and _in_weight_arena(W.data_ptr()):
        return gemm(NT, dy, N, transposed_weight(W), N, out, K, M, K, N, epi, None, aux, K if aux is not None else 0)
    return gemm(NN, dy, N, W, K, out, K, M, K, N, epi, None, aux, K if aux is not None else 0)


def linear_wgrad(dy, x, dW, accumulate=False, db=None, x16=None, dy16=None):
    """dW[N,K] (+)= dy[M,N]^T @ x[M,K]; with db also db[N] (+)= dy.sum(0), folded into the same pass over dy.
    bf16 mode: x16 = the layer input in bf16 (x may then be None - the bf16 data path saves only that form); dy16 = the gradient in bf16
    where its producer wrote only that (dy may then be None; needs x16)."""
    _f32(dW)
    if dy is not None:
        _f32(dy)
    M, N = (dy if dy is not None else dy16).shape
    K = (x if x is not None else x16).shape[1]
    mode = get_gemm_mode()
    ws = _gemm_workspace(TN, N, K, M, mode, dW.device)      # d2s_linear_wgrad_workspace_bytes(M, N, K, mode) is this query
    if x16 is not None:
        assert mode == GEMM_BF16 and x16.dtype == torch.bfloat16 and x16.is_contiguous() and tuple(x16.shape) == (M, K)
        assert dy16 is None or (dy16.dtype == torch.bfloat16 and dy16.is_contiguous() and tuple(dy16.shape) == (M, N))
        lib.call("d2s_linear_wgrad_f32_bf16x", lib.ptr(dy), lib.ptr(dy16), N, lib.ptr(x16), K, lib.ptr(dW), K, lib.ptr(db), M, N, K,
                 int(accumulate), lib.ptr(ws), ws.numel() if ws is not None else 0)
        return dW
    assert dy16 is None, "a bf16 gradient needs the bf16 layer input as well"
    _f32(x)
    lib.call("d2s_linear_wgrad_f32", lib.ptr(dy), N, lib.ptr(x), K, lib.ptr(dW), K, lib.ptr(db), M, N, K, int(accumulate), mode,
             lib.ptr(ws), ws.numel() if ws is not None else 0)
    return dW


# ---- weight gradients on their own stream ----
# Within a backward pass nothing waits for a weight gradient: dW / db of a Linear are only read by the optimiser (and the gradient
# all-reduce), while the chain that the next layer waits for is dy -> dx.  Inside `async_weight_grads()` (d2s.engine.TrainStep wraps its
# backward in it) the wgrad GEMMs, their slab combines and the bias column sums are issued on a second HIP stream that trails the main
# one, so they fill the CUs that the dgrad / attention kernels of the following layers leave idle in their tails; the caller joins the
# stream before anything reads the gradients (join_weight_grads).  Outside that block - any caller that runs loss.backward() itself and
# then reads .grad on the current stream - everything stays on the current stream.
# HIP multiplexes a process's streams onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4), and two streams that share a queue run
# their kernels strictly one after the other.  Which queue a stream gets depends on what else created streams before it: with an RCCL
# process group alive the teacher stream of d2s.engine landed on the main stream's queue and the teacher / student overlap was gone
# (-5 % on the step, profiles/r03_o_stream_queue_collision.txt).  So a side stream is CHOSEN: candidates from torch's pool are kept only if a
# pair of spin kernels shows that they really run beside every stream they are meant to overlap with.
_STREAM_CHECK = os.environ.get("D2S_STREAM_CHECK", "1") != "0"
stream_picks = []          # diagnostic: (purpose, candidates tried, verified concurrent)


def _streams_overlap(a, b, cycles=3000000):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for st in (a, b):                         # first use of a stream sets things up lazily: keep that out of the measurement
        with torch.cuda.stream(st):
            torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        ev[0].record()
        torch.cuda._sleep(cycles)
        ev[1].record()
    with torch.cuda.stream(b):
        ev[2].record()
        torch.cuda._sleep(cycles)
        ev[3].record()
    torch.cuda.synchronize()
    single = ev[0].elapsed_time(ev[1])
    return ev[0].elapsed_time(ev[3]) < 1.6 * single      # one queue: the second spin starts when the first has ended (2x)


def concurrent_stream(beside, purpose="", tries=12):
    """A torch.cuda.Stream whose kernels run concurrently with those of every stream in `beside` (verified on the device), or - if no
    candidate passes - the last candidate (the step is then correct but loses that overlap; stream_picks records it)."""
    cand = torch.cuda.Stream()
    if not _STREAM_CHECK:
        return cand
    kept = []                  # hold the rejected candidates while searching: the pool hands out its 32 streams round-robin
    for n in range(1, tries + 1):
        if all(_streams_overlap(o, cand) for o in beside):
            stream_picks.append((purpose, n, True))
            return cand
        kept.append(cand)
        cand = torch.cuda.Stream()
    stream_picks.append((purpose, tries, False))
    return cand


def recheck_stream(stream, beside, purpose):
    """`stream` if it still runs beside every stream in `beside`, else a replacement that does.  The queue a stream sits on can end up
    shared AFTER it was picked (an RCCL communicator sets itself up at its first collective): d2s.engine re-checks its side streams once
    the first steps have run."""
    if stream is None or not _STREAM_CHECK or all(_streams_overlap(o, stream) for o in beside):
        return stream
    return concurrent_stream(beside, purpose + " (re-picked)")


def pg_stream_shares_queue(stream, group=None, cycles=20000000):
    """Does the process group's RCCL stream sit on the hardware queue of `stream`?  (torch picks that stream from its pool at the
    group's first collective; nothing lets a caller choose it.)  If it does, every collective - which first waits for the gradient
    streams - holds up whatever `stream` issues after it: measured -17 % on the step.  Probe: a spin on a helper stream, a tiny
    all_reduce issued behind it (RCCL's stream now waits for the spin), then a spin on `stream` - which ends late only if it had to
    queue behind that wait.  The spins are long (~10 ms) so that the host time of the all_reduce call between the two launches cannot be
    mistaken for queueing.  Two collectives per call: every rank of the group must make the same calls."""
    import torch.distributed as dist
    helper = concurrent_stream([stream], "probe helper")
    t = torch.zeros(64, device=torch.device("cuda", torch.cuda.current_device()))
    with torch.cuda.stream(helper):                   # the group's stream exists (and is set up) after its first collective
        dist.all_reduce(t, group=group, async_op=True).wait()
        torch.cuda._sleep(1000)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    with torch.cuda.stream(helper):
        ev[0].record()
        torch.cuda._sleep(cycles)
        ev[1].record()
        w = dist.all_reduce(t, group=group, async_op=True)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        ev[2].record()
    with torch.cuda.stream(helper):
        w.wait()
    torch.cuda.synchronize()
    if os.environ.get("D2S_STREAM_DEBUG") == "1":
        import sys
        print(f"[d2s] rccl-queue probe: helper spin {ev[0].elapsed_time(ev[1]):.2f} ms, start -> end of the probed stream's spin {ev[0].elapsed_time(ev[2]):.2f} ms",
              file=sys.stderr, flush=True)
    return ev[0].elapsed_time(ev[2]) > 1.6 * ev[0].elapsed_time(ev[1])


def ensure_weight_grad_stream(beside):
    """The weight-gradient stream, created now (instead of at the first backward) if it does not exist yet."""
    if _WGRAD["stream"] is None:
        _WGRAD["stream"] = concurrent_stream(list(beside), "weight gradients")
    return _WGRAD["stream"]


def set_weight_grad_stream(stream):
    assert not _WGRAD["on"]
    _WGRAD["stream"] = stream


def recheck_weight_grad_stream(beside):
    if _WGRAD["stream"] is not None and not _WGRAD["on"]:
        _WGRAD["stream"] = recheck_stream(_WGRAD["stream"], beside, "weight gradients")


_WGRAD = {"on": False, "stream": None, "used": False}
_WGRAD_ENABLED = os.environ.get("D2S_WGRAD_STREAM", "1") != "0"


class async_weight_grads:
    def __enter__(self):
        if _WGRAD_ENABLED and torch.cuda.is_available():
            if _WGRAD["stream"] is None:
                _WGRAD["stream"] = concurrent_stream([torch.cuda.current_stream()] + list(_WGRAD.get("beside", [])), "weight gradients")
            _WGRAD["on"], _WGRAD["used"] = True, False
        return self

    def __exit__(self, *exc):
        _WGRAD["on"] = False
        join_weight_grads()
        return False


def weight_grad_stream():
    """The side stream if weight gradients were issued on it since the last join, else None (the reducer of the data-parallel path
    makes its own stream wait on it before it all-reduces a bucket)."""
    return _WGRAD["stream"] if _WGRAD["used"] else None


def join_weight_grads():
    if _WGRAD["used"] and _WGRAD["stream"] is not None:
        torch.cuda.current_stream().wait_stream(_WGRAD["stream"])
    _WGRAD["used"] = False


def linear_param_grads(dy, x, W, b, want_w=True, want_b=True, accumulate=False, x16=None, dy16=None):
    """(dW, db) of a Linear into fresh arena-backed buffers: one fused pass when both are wanted.  x16 / dy16: see linear_wgrad."""
    dW = grad_buffer(W) if want_w else None
    db = grad_buffer(b) if (want_b and b is not None) else None
    if dW is None and db is None:
        return dW, db
    src = dy if dy is not None else dy16
    if dW is None and dy is None:
        dy = dy16.float()            # bias gradient alone from a bf16-only gradient (not on the model's path: weights and biases train together)
    side = _WGRAD["stream"] if (_WGRAD["on"] and src.is_cuda) else None
    if side is None:
        if dW is not None:
            linear_wgrad(dy, x, dW, accumulate=accumulate, db=db, x16=x16, dy16=dy16)
        else:
            colsum(dy, db, accumulate=accumulate)
        return dW, db
    main = torch.cuda.current_stream()
    side.wait_stream(main)                       # dy (and x) were produced on the main stream
    with torch.cuda.stream(side):
        if dW is not None:
            linear_wgrad(dy, x, dW, accumulate=accumulate, db=db, x16=x16, dy16=dy16)
        else:
            colsum(dy, db, accumulate=accumulate)
    for t in (dy, dy16, x, x16, dW, db):                    # autograd may free these on the main stream while the side stream still reads / writes them
        if t is not None:
            t.record_stream(side)
    _WGRAD["used"] = True
    return dW, db


def colsum(x, out, accumulate=False):
    _f32(x)
    M, N = x.shape
    need = lib.query("d2s_colsum_workspace_bytes", M, N)
    ws = workspace(need, x.device)
    lib.call("d2s_colsum_f32", lib.ptr(x), N, M, N, lib.ptr(out), int(accumulate), lib.ptr(ws), ws.numel())
    return out


def contiguous_map(rows, D):
    return (rows, 0, D, 0)


def skip_cls_map(n, D, tail=0):
    """rows of x[:, 1:n - tail] inside a contiguous [B, n, D] buffer."""
    return (n - 1 - tail, n * D, D, D)


def layernorm_fwd(x, rowmap, w, b, rows, D, eps, stats=True):
    """stats=False (forward-only callers: the frozen teacher, eval): the per-row mean / rstd are not written."""
    y = torch.empty((rows, D), dtype=torch.float32, device=x.device)
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device) if stats else None
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device) if stats else None
    lib.call("d2s_layernorm_fwd", lib.ptr(x), *rowmap, lib.ptr(w), lib.ptr(b), lib.ptr(y), lib.ptr(mean), lib.ptr(rstd),
             rows, D, float(eps))
    return y, mean, rstd


def layernorm_fwd_bf16(x, rowmap, w, b, rows, D, eps, stats=True, want_f32=True):
    """LayerNorm forward that also (or only: want_f32=False) writes the bf16 copy a bf16-mode GEMM reads.  -> (y or None, mean, rstd, y16)"""
    y = torch.empty((rows, D), dtype=torch.float32, device=x.device) if want_f32 else None
    y16 = bf16_buffer(rows, D, x.device)
    mean = torch.empty((rows,), dtype=torch.float32, device=x.device) if stats else None
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device) if stats else None
    lib.call("d2s_layernorm_fwd_bf16out", lib.ptr(x), *rowmap, lib.ptr(w), lib.ptr(b), lib.ptr(y), lib.ptr(y16), lib.ptr(mean),
             lib.ptr(rstd), rows, D, float(eps))
    return y, mean, rstd, y16


def layernorm_bwd(x, rowmap, dy, w, mean, rstd, dx, add_src, dw, db, rows, D, accumulate_wb=False, relu_mask=False, dx16=None):
    """dx16 (bf16 mode): dense bf16 [rows, D] buffer that receives a copy of dx."""
    need = lib.query("d2s_layernorm_bwd_workspace_bytes", rows, D)
    ws = workspace(need, dy.device)
    if dx16 is not None:
        assert dx16.dtype == torch.bfloat16 and dx16.is_contiguous() and tuple(dx16.shape) == (rows, D)
        lib.call("d2s_layernorm_bwd_bf16out", lib.ptr(x), *rowmap, lib.ptr(dy), lib.ptr(w), lib.ptr(mean), lib.ptr(rstd), lib.ptr(dx),
                 lib.ptr(dx16), lib.ptr(add_src), lib.ptr(dw), lib.ptr(db), int(accumulate_wb), int(relu_mask), rows, D, lib.ptr(ws), ws.numel())
        return dx
    lib.call("d2s_layernorm_bwd", lib.ptr(x), *rowmap, lib.ptr(dy), lib.ptr(w), lib.ptr(mean), lib.ptr(rstd), lib.ptr(dx),
             lib.ptr(add_src), lib.ptr(dw), lib.ptr(db), int(accumulate_wb), int(relu_mask), rows, D, lib.ptr(ws), ws.numel())
    return dx


def batchnorm_fwd(x, w, b, running_mean, running_var, training, eps=1e-5, momentum=0.1):
    """BatchNorm1d over the rows of x [R, C] (dynamic_vit.py:350-367).  Returns (y, mean, rstd); updates the running estimates in
    place when training."""
    _f32(x)
    R, C = x.shape
    y = torch.empty_like(x)
    mean = torch.empty((C,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((C,), dtype=torch.float32, device=x.device)
    ws = workspace(lib.query("d2s_batchnorm_workspace_bytes", R, C), x.device)
    lib.call("d2s_batchnorm_fwd", lib.ptr(x), lib.ptr(w), lib.ptr(b), lib.ptr(y), lib.ptr(mean), lib.ptr(rstd), lib.ptr(running_mean),
             lib.ptr(running_var), R, C, float(eps), float(momentum), int(bool(training)), lib.ptr(ws), ws.numel())
    return y, mean, rstd


def batchnorm_bwd(x, dy, w, mean, rstd, dw, db, training, relu_mask=False, accumulate=False):
    _f32(x), _f32(dy)
    R, C = x.shape
    dx = torch.empty_like(x)
    ws = workspace(lib.query("d2s_batchnorm_workspace_bytes", R, C), x.device)
    lib.call("d2s_batchnorm_bwd", lib.ptr(x), lib.ptr(dy), lib.ptr(w), lib.ptr(mean), lib.ptr(rstd), lib.ptr(dx), lib.ptr(dw), lib.ptr(db),
             int(relu_mask), int(accumulate), int(bool(training)), R, C, lib.ptr(ws), ws.numel())
    return dx


def softmax_rows(scores):
    _f32(scores)
    R, T = scores.shape
    probs = torch.empty_like(scores)
    lib.call("d2s_softmax_rows", lib.ptr(scores), lib.ptr(probs), R, T)
    return probs


def select_topk(probs, k):
    _f32(probs)
    B, T = probs.shape
    k = min(int(k), T)
    kept = torch.empty((B, k), dtype=torch.int64, device=probs.device)
    dropped = torch.empty((B, T - k), dtype=torch.int64, device=probs.device)
    lib.call("d2s_select_topk", lib.ptr(probs), B, T, k, lib.ptr(kept), lib.ptr(dropped) if T - k > 0 else None)
    return kept, dropped


def select_cls_attn(cls_row, lead, T, k, mean_heads=False):
    """cls_row [B,H,n] (a block's CLS softmax row), tokens in columns lead .. lead + T - 1 -> (probs [B,T], kept [B,k], dropped [B,T-k]):
    max (or mean) over heads, renormalised over the T tokens, and the hard top-k of those probabilities in select_topk's order - one
    launch"""
    _f32(cls_row)
    B, H, n = cls_row.shape
    T, k = int(T), int(k)
    probs = torch.empty((B, T), dtype=torch.float32, device=cls_row.device)
    kept = torch.empty((B, k), dtype=torch.int64, device=cls_row.device)
    dropped = torch.empty((B, T - k), dtype=torch.int64, device=cls_row.device)
    lib.call("d2s_select_cls_attn", lib.ptr(cls_row), B, H, n, int(lead), T, k, 1 if mean_heads else 0, lib.ptr(probs),
             lib.ptr(kept) if k > 0 else None, lib.ptr(dropped) if T - k > 0 else None)
    return probs, kept, dropped


def tome_clip_r(r, n):
    """ToMe's effective merge count of a block with n tokens: at most half of the non-CLS tokens (set A without CLS)."""
    return max(0, min(int(r), (int(n) - 1) // 2))


def _tome_match(entry, qkv, B, n, H, r):
    B, n, H, r = int(B), int(n), int(H), int(r)
    Ta = (n + 1) // 2
    i32 = dict(dtype=torch.int32, device=qkv.device)
    node_max = torch.empty((B, Ta), dtype=torch.float32, device=qkv.device)
    node_idx, unm = torch.empty((B, Ta), **i32), torch.empty((B, max(Ta - r, 0)), **i32)
    src, dst = torch.empty((B, max(r, 0)), **i32), torch.empty((B, max(r, 0)), **i32)
    lib.call(entry, lib.ptr(qkv), B, n, H, r, lib.ptr(node_max), lib.ptr(node_idx), lib.ptr(unm), lib.ptr(src) if r > 0 else None,
             lib.ptr(dst) if r > 0 else None)
    return node_max, node_idx, unm, src, dst


def tome_match(qkv, B, n, H, r):
    """Bipartite soft matching of token merging on the keys of a [B * n, 3 * H * 64] qkv, read in place.  r is the
    effective count (tome_clip_r).  -> (node_max [B,T_a], node_idx [B,T_a], unm_idx [B,T_a-r], src_idx [B,r], dst_idx [B,r]), int32"""
    _f32(qkv)
    return _tome_match("d2s_tome_match", qkv, B, n, H, r)


def tome_match_bf16(qkv16, B, n, H, r):
    """tome_match on a bf16 qkv (the qkv GEMM's c16 on the bf16 data path), read in place: bit for bit tome_match(qkv16.float())."""
    assert qkv16.dtype == torch.bfloat16 and qkv16.is_contiguous(), (qkv16.dtype, qkv16.is_contiguous())
    return _tome_match("d2s_tome_match_bf16", qkv16, B, n, H, r)


def tome_merge(x, size, unm, src, dst, B, n, D, r):
    """x [B * n, D] (or [B, n, D]), size [B, n] or None (all ones), a plan of tome_match -> (x_out [B * (n - r), D], size_out [B, n - r])"""
    _f32(x)
    B, n, D, r = int(B), int(n), int(D), int(r)
    for t in (unm, src, dst):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert tuple(unm.shape) == (B, (n + 1) // 2 - r) and tuple(src.shape) == (B, r) and tuple(dst.shape) == (B, r)
    if size is not None:
        _f32(size)
        assert tuple(size.shape) == (B, n)
    out = torch.empty((B * max(n - r, 0), D), dtype=torch.float32, device=x.device)
    size_out = torch.empty((B, max(n - r, 0)), dtype=torch.float32, device=x.device)
    lib.call("d2s_tome_merge", lib.ptr(x), lib.ptr(size), lib.ptr(unm), lib.ptr(src) if r > 0 else None, lib.ptr(dst) if r > 0 else None,
             B, n, D, r, lib.ptr(out), lib.ptr(size_out))
    return out, size_out


def tome_merge_bwd(dy, size, size_out, unm, src, dst, B, n, D, r, dx16=None):
    """Backward of tome_merge in x: dy [B * (n - r), D], size [B, n] or None and the plan as the forward took them, size_out [B, n - r] as
    it wrote them -> dx [B * n, D].  dx16 (the bf16 data path behind a merge): a bf16 buffer [B * n, D] that receives dx rounded once, in
    the same launch."""
    _f32(dy)
    _f32(size_out)
    B, n, D, r = int(B), int(n), int(D), int(r)
    for t in (unm, src, dst):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert tuple(unm.shape) == (B, (n + 1) // 2 - r) and tuple(src.shape) == (B, r) and tuple(dst.shape) == (B, r)
    assert dy.numel() == B * (n - r) * D and tuple(size_out.shape) == (B, n - r)
    if size is not None:
        _f32(size)
        assert tuple(size.shape) == (B, n)
    dx = torch.empty((B * n, D), dtype=torch.float32, device=dy.device)
    if dx16 is not None:
        assert dx16.dtype == torch.bfloat16 and dx16.is_contiguous() and dx16.numel() == B * n * D and dx16.is_cuda
        lib.call("d2s_tome_merge_bwd_bf16out", lib.ptr(dy), lib.ptr(size), lib.ptr(size_out), lib.ptr(unm), lib.ptr(src) if r > 0 else None,
                 lib.ptr(dst) if r > 0 else None, B, n, D, r, lib.ptr(dx), lib.ptr(dx16))
        return dx
    lib.call("d2s_tome_merge_bwd", lib.ptr(dy), lib.ptr(size), lib.ptr(size_out), lib.ptr(unm), lib.ptr(src) if r > 0 else None,
             lib.ptr(dst) if r > 0 else None, B, n, D, r, lib.ptr(dx))
    return dx


def gather_pack(x, ids):
    _f32(x)
    B, n, D = x.shape
    k = ids.shape[1]
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    out = torch.empty((B, k + 1, D), dtype=torch.float32, device=x.device)
    lib.call("d2s_gather_pack_fwd", lib.ptr(x), lib.ptr(ids), lib.ptr(out), B, n, k, D)
    return out


def scatter_unpack(g, ids, n):
    _f32(g)
    B, k1, D = g.shape
    dx = torch.empty((B, n, D), dtype=torch.float32, device=g.device)
    lib.call("d2s_scatter_unpack_bwd", lib.ptr(g), lib.ptr(ids), lib.ptr(dx), B, n, k1 - 1, D)
    return dx


def _fuse_shapes(x, p, kept, dropped, t):
    B, n, D = x.shape
    T, k = n - 1 - int(t), kept.shape[1]
    assert kept.dtype == torch.int64 and kept.is_contiguous() and dropped.dtype == torch.int64 and dropped.is_contiguous()
    assert p.shape == (B, T) and kept.shape == (B, k) and dropped.shape == (B, T - k), \
        f"x {tuple(x.shape)} with t = {t}: p must be [B, {T}], kept [B, k], dropped [B, {T} - k]"
    return B, n, D, T, k


def gather_fuse_fwd(x, p, kept, dropped, t):
    """x [B,n,D] = [CLS | T scored | t package rows], p [B,T], kept [B,k], dropped [B,T-k] -> (y [B,k+t+2,D], S [B]): the kept-token
    gather, the package rows copied, and the new package row sum_{j in dropped} (p_j / S) x[:, 1 + j] last"""
    _f32(x)
    _f32(p)
    B, n, D, T, k = _fuse_shapes(x, p, kept, dropped, t)
    y = torch.empty((B, k + int(t) + 2, D), dtype=torch.float32, device=x.device)
    S = torch.empty((B,), dtype=torch.float32, device=x.device)
    lib.call("d2s_gather_fuse_fwd", lib.ptr(x), lib.ptr(p), lib.ptr(kept) if k else None, lib.ptr(dropped) if T - k else None,
             lib.ptr(y), lib.ptr(S), B, n, int(t), k, D)
    return y, S


def gather_fuse_bwd(g, x, p, S, y, kept, dropped, t):
    """g [B,k+t+2,D] and what gather_fuse_fwd read and wrote -> (dx [B,n,D], dp [B,T]), every element written by the one launch"""
    _f32(g)
    _f32(x)
    _f32(p)
    _f32(y)
    B, n, D, T, k = _fuse_shapes(x, p, kept, dropped, t)
    assert g.shape == y.shape == (B, k + int(t) + 2, D) and S.shape == (B,)
    dx = torch.empty((B, n, D), dtype=torch.float32, device=g.device)
    dp = torch.empty((B, T), dtype=torch.float32, device=g.device)
    lib.call("d2s_gather_fuse_bwd", lib.ptr(g), lib.ptr(x), lib.ptr(p), lib.ptr(S), lib.ptr(y), lib.ptr(kept) if k else None,
             lib.ptr(dropped) if T - k else None, lib.ptr(dx), lib.ptr(dp), B, n, int(t), k, D)
    return dx, dp


def _squeeze_shapes(x, kept, dropped):
    B, n, D = x.shape
    k = kept.shape[1]
    assert kept.dtype == torch.int64 and kept.is_contiguous() and dropped.dtype == torch.int64 and dropped.is_contiguous()
    assert kept.shape == (B, k) and dropped.shape == (B, n - 1 - k), \
        f"x {tuple(x.shape)}: kept must be [B, k], dropped [B, {n - 1} - k]"
    return B, n, D, k, n - 1 - k


def _squeeze_plan(dst, sim, B, m):
    assert dst.dtype == torch.int32 and dst.is_contiguous() and tuple(dst.shape) == (B, m), "dst must be int32 [B, m]"
    _f32(sim)
    assert tuple(sim.shape) == (B, m), "sim must be [B, m]"


def squeeze_match(x, kept, dropped):
    """x [B,n,D] = [CLS | T scored], kept [B,k], dropped [B,T-k] -> (dst [B,T-k] int32, sim [B,T-k]): for every dropped token the position
    in `kept` of the kept token with the highest cosine (the lowest position on a tie) and that cosine"""
    _f32(x)
    B, n, D, k, m = _squeeze_shapes(x, kept, dropped)
    dst = torch.empty((B, m), dtype=torch.int32, device=x.device)
    sim = torch.empty((B, m), dtype=torch.float32, device=x.device)
    lib.call("d2s_squeeze_match", lib.ptr(x), lib.ptr(kept), lib.ptr(dropped) if m else None, B, n, k, D, lib.ptr(dst) if m else None,
             lib.ptr(sim) if m else None)
    return dst, sim


def gather_squeeze_fwd(x, kept, dropped, dst, sim):
    """x, the id lists and a plan of squeeze_match -> (y [B,k+1,D], Z [B,k]): the kept-token gather with every dropped token folded into
    its destination at weight exp(sim) against the kept token's own exp(1); Z the weight sums"""
    _f32(x)
    B, n, D, k, m = _squeeze_shapes(x, kept, dropped)
    _squeeze_plan(dst, sim, B, m)
    y = torch.empty((B, k + 1, D), dtype=torch.float32, device=x.device)
    Z = torch.empty((B, k), dtype=torch.float32, device=x.device)
    lib.call("d2s_gather_squeeze_fwd", lib.ptr(x), lib.ptr(kept), lib.ptr(dropped) if m else None, lib.ptr(dst) if m else None,
             lib.ptr(sim) if m else None, B, n, k, D, lib.ptr(y), lib.ptr(Z))
    return y, Z


def gather_squeeze_bwd(g, kept, dropped, dst, sim, Z, n):
    """g [B,k+1,D], the id lists, the plan and gather_squeeze_fwd's Z -> dx [B,n,D], every element written by the one launch"""
    _f32(g)
    _f32(Z)
    B, k1, D = g.shape
    k, m = k1 - 1, int(n) - k1
    assert kept.dtype == torch.int64 and kept.is_contiguous() and dropped.dtype == torch.int64 and dropped.is_contiguous()
    assert tuple(kept.shape) == (B, k) and tuple(dropped.shape) == (B, m) and tuple(Z.shape) == (B, k)
    _squeeze_plan(dst, sim, B, m)
    dx = torch.empty((B, int(n), D), dtype=torch.float32, device=g.device)
    lib.call("d2s_gather_squeeze_bwd", lib.ptr(g), lib.ptr(kept), lib.ptr(dropped) if m else None, lib.ptr(dst) if m else None,
             lib.ptr(sim) if m else None, lib.ptr(Z), B, int(n), k, D, lib.ptr(dx))
    return dx


def half_mean_concat(x, B, T, C, relu_mask_src=None):
    out = torch.empty((B * T, C), dtype=torch.float32, device=x.device)
    lib.call("d2s_half_mean_concat", lib.ptr(x), lib.ptr(relu_mask_src), lib.ptr(out), B, T, C)
    return out


def im2col_patch(img, P):
    _f32(img)
    B, Cin, H, W = img.shape
    T = (H // P) * (W // P)
    col = torch.empty((B * T, Cin * P * P), dtype=torch.float32, device=img.device)
    lib.call("d2s_im2col_patch", lib.ptr(img), lib.ptr(col), B, Cin, H, W, P)
    return col


def fill_cls(cls, pos, tokens):
    B, n, D = tokens.shape
    lib.call("d2s_fill_cls", lib.ptr(cls), lib.ptr(pos), lib.ptr(tokens), B, n, D)


def batch_sum(g, out, B, count, image_stride, accumulate=False):
    lib.call("d2s_batch_sum", lib.ptr(g), lib.ptr(out), B, count, image_stride, int(accumulate))
    return out


def copy_rows(src, rowmap, rows, D, dst=None, dst_map=None, accumulate=False):
    if dst is None:
        dst = torch.empty((rows, D), dtype=torch.float32, device=src.device)
    if dst_map is None:
        dst_map = contiguous_map(rows, D)
    lib.call("d2s_copy_rows", lib.ptr(src), *rowmap, lib.ptr(dst), *dst_map, rows, D, int(accumulate))
    return dst


def unfold_fwd(src, strides, B, C, H, W, k, s, p):
    """strides = (sb, sc, sy, sx) of the source seen as [B, C, H, W]; -> [B, Ho*Wo, C*k*k]"""
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    out = torch.empty((B, Ho * Wo, C * k * k), dtype=torch.float32, device=src.device)
    lib.call("d2s_unfold_fwd", lib.ptr(src), *strides, lib.ptr(out), B, C, H, W, k, s, p)
    return out


def unfold_bwd(g, dsrc, strides, B, C, H, W, k, s, p):
    lib.call("d2s_unfold_bwd", lib.ptr(g), lib.ptr(dsrc), *strides, B, C, H, W, k, s, p)
    return dsrc


def performer_attn_fwd(kqv, w, B, T, eps=1e-8):
    dev = kqv.device
    M = B * T
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    y, kp, qp, A, ksum, D = f(M, 64), f(M, 32), f(M, 32), f(B, 64, 32), f(B, 32), f(M)
    ws = workspace(lib.query("d2s_performer_workspace_bytes", B, T), dev)
    lib.call("d2s_performer_attn_fwd", lib.ptr(kqv), lib.ptr(w), lib.ptr(y), lib.ptr(kp), lib.ptr(qp), lib.ptr(A), lib.ptr(ksum),
             lib.ptr(D), B, T, float(eps), lib.ptr(ws), ws.numel())
    return y, kp, qp, A, ksum, D


def performer_attn_bwd(kqv, w, y, kp, qp, A, ksum, D, gy, skip, B, T, eps=1e-8):
    dev = kqv.device
    M = B * T
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    dkqv, dnum, dD, dqp, dkp, dA, dksum = f(M, 192), f(M, 64), f(M), f(M, 32), f(M, 32), f(B, 64, 32), f(B, 32)
    ws = workspace(lib.query("d2s_performer_workspace_bytes", B, T), dev)
    lib.call("d2s_performer_attn_bwd", lib.ptr(kqv), lib.ptr(w), lib.ptr(y), lib.ptr(kp), lib.ptr(qp), lib.ptr(A), lib.ptr(ksum),
             lib.ptr(D), lib.ptr(gy), lib.ptr(skip), lib.ptr(dkqv), lib.ptr(dnum), lib.ptr(dD), lib.ptr(dqp), lib.ptr(dkp), lib.ptr(dA),
             lib.ptr(dksum), B, T, float(eps), lib.ptr(ws), ws.numel())
    return dkqv


def attn_fwd(qkv, B, n, H, scale, want_cls=True):
    out = torch.empty((B * n, H * 64), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    cls_row = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device) if want_cls else None
    # bf16 arithmetic mode: the two matrix products of the forward run on the bf16 matrix cores too (same outputs, fp32 backward)
    entry = "d2s_attn_fwd_bf16" if get_gemm_mode() == GEMM_BF16 else "d2s_attn_fwd_f32"
    lib.call(entry, lib.ptr(qkv), lib.ptr(out), lib.ptr(lse), lib.ptr(cls_row), B, n, H, float(scale))
    return out, lse, cls_row


def attn_keyw_fwd(qkv, key_w, B, n, H, scale, want_lse=False):
    """Attention whose key j counts key_w[b, j] times in every softmax row (token merging).  fp32 kernel only: the
    bf16 arithmetic mode has no weighted attention and is refused.  -> (out [B * n, H * 64], lse [B,H,n] or None)"""
    if get_gemm_mode() == GEMM_BF16:
        raise lib.D2SError("key-weighted attention exists in fp32 only (gemm modes exact and split)")
    _f32(key_w)
    assert tuple(key_w.shape) == (B, n)
    out = torch.empty((B * n, H * 64), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device) if want_lse else None
    lib.call("d2s_attn_keyw_fwd_f32", lib.ptr(qkv), lib.ptr(key_w), lib.ptr(out), lib.ptr(lse), B, n, H, float(scale))
    return out, lse


def attn_keyw_bwd(qkv, key_w, out, dout, lse, B, n, H, scale):
    """Backward of attn_keyw_fwd (out, lse as it returned them with want_lse=True) -> dqkv shaped like qkv; the weights get no gradient."""
    if get_gemm_mode() == GEMM_BF16:
        raise lib.D2SError("key-weighted attention exists in fp32 only (gemm modes exact and split)")
    _f32(key_w)
    assert tuple(key_w.shape) == (B, n) and qkv.dtype == torch.float32
    dqkv = torch.empty(qkv.shape, dtype=torch.float32, device=qkv.device)
    delta = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    lib.call("d2s_attn_keyw_bwd_f32", lib.ptr(qkv), lib.ptr(key_w), lib.ptr(out), lib.ptr(dout), lib.ptr(lse), lib.ptr(dqkv), lib.ptr(delta),
             B, n, H, float(scale))
    return dqkv


def attn_fwd_bf16io(qkv, B, n, H, scale, want_cls=True, want_f32=True):
    """bf16-mode attention forward that also (or only) writes the bf16 copy of its output; qkv fp32 or bf16 (the qkv GEMM's c16).
    -> (out or None, lse, cls_row, out16)"""
    assert qkv.is_contiguous() and qkv.dtype in (torch.float32, torch.bfloat16)
    out = torch.empty((B * n, H * 64), dtype=torch.float32, device=qkv.device) if want_f32 else None
    out16 = bf16_buffer(B * n, H * 64, qkv.device)
    lse = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    cls_row = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device) if want_cls else None
    lib.call("d2s_attn_fwd_bf16_bf16out", lib.ptr(qkv), int(qkv.dtype == torch.bfloat16), lib.ptr(out), lib.ptr(out16), lib.ptr(lse),
             lib.ptr(cls_row), B, n, H, float(scale))
    return out, lse, cls_row, out16


def attn_keyw_fwd_bf16io(qkv, key_w, B, n, H, scale, want_f32=True):
    """Key-weighted attention forward (attn_keyw_fwd's definition) on the bf16 matrix cores and the bf16 data path: qkv fp32 or bf16 (the
    qkv GEMM's c16); always writes the bf16 copy of its output for the projection GEMM.  Its backward: attn_keyw_bwd_bf16io.
    -> (out or None, lse [B,H,n], out16)"""
    assert qkv.is_contiguous() and qkv.dtype in (torch.float32, torch.bfloat16)
    _f32(key_w)
    assert tuple(key_w.shape) == (B, n)
    out = torch.empty((B * n, H * 64), dtype=torch.float32, device=qkv.device) if want_f32 else None
    out16 = bf16_buffer(B * n, H * 64, qkv.device)
    lse = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    lib.call("d2s_attn_keyw_fwd_bf16", lib.ptr(qkv), int(qkv.dtype == torch.bfloat16), lib.ptr(key_w), lib.ptr(out), lib.ptr(out16),
             lib.ptr(lse), B, n, H, float(scale))
    return out, lse, out16


def attn_keyw_bwd_bf16io(qkv, key_w, out, dout, lse, B, n, H, scale, dqkv16=None, want_f32=True):
    """Backward of attn_keyw_fwd_bf16io (out its fp32 output, lse as it returned it) on the bf16 matrix cores, attn_bwd's shape in the bf16
    mode: qkv fp32 or bf16; dqkv16: a bf16 buffer shaped like qkv that receives a copy of dqkv; want_f32=False (needs dqkv16): only that
    form is written and None is returned.  The weights get no gradient."""
    assert qkv.is_contiguous() and qkv.dtype in (torch.float32, torch.bfloat16)
    _f32(key_w)
    assert tuple(key_w.shape) == (B, n)
    dqkv = torch.empty(qkv.shape, dtype=torch.float32, device=qkv.device) if (want_f32 or dqkv16 is None) else None
    if dqkv16 is not None:
        assert dqkv16.dtype == torch.bfloat16 and dqkv16.is_contiguous() and dqkv16.numel() == qkv.numel()
    delta = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    lib.call("d2s_attn_keyw_bwd_bf16", lib.ptr(qkv), int(qkv.dtype == torch.bfloat16), lib.ptr(key_w), lib.ptr(out), lib.ptr(dout),
             lib.ptr(lse), lib.ptr(dqkv), lib.ptr(dqkv16), lib.ptr(delta), B, n, H, float(scale))
    return dqkv


def attn_bwd(qkv, out, dout, lse, B, n, H, scale, dqkv16=None, want_f32=True):
    """dqkv16 (bf16 mode with the bf16 attention kernels): bf16 buffer shaped like qkv that receives a copy of dqkv; want_f32=False
    (needs dqkv16): only that form is written and None is returned."""
    dqkv = torch.empty(qkv.shape, dtype=torch.float32, device=qkv.device) if (want_f32 or dqkv16 is None) else None
    delta = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    bf16 = get_gemm_mode() == GEMM_BF16
    if dqkv16 is not None:
        assert bf16 and dqkv16.dtype == torch.bfloat16 and dqkv16.is_contiguous() and dqkv16.numel() == qkv.numel()
        lib.call("d2s_attn_bwd_bf16_bf16out", lib.ptr(qkv), int(qkv.dtype == torch.bfloat16), lib.ptr(out), lib.ptr(dout), lib.ptr(lse),
                 lib.ptr(dqkv), lib.ptr(dqkv16), lib.ptr(delta), B, n, H, float(scale))
        return dqkv
    assert qkv.dtype == torch.float32
    entry = "d2s_attn_bwd_bf16" if bf16 else "d2s_attn_bwd_f32"
    lib.call(entry, lib.ptr(qkv), lib.ptr(out), lib.ptr(dout), lib.ptr(lse), lib.ptr(dqkv), lib.ptr(delta), B, n, H, float(scale))
    return dqkv


# ---- one transformer block per C-ABI call (csrc/block.hip): the same launches as the per-op wrappers above, issued from C ----
_BLOCK_COMPOSITE = os.environ.get("D2S_BLOCK_COMPOSITE", "1") != "0"
_BLOCK_SIZES = {}       # (B, n, D, H, hidden, mode) -> (saved floats train, saved floats eval, bwd scratch floats, main ws bytes, wgrad ws bytes)
c_abi_calls_saved = 0   # diagnostic: per-op calls that the composite entries replaced


def block_composite_ok(x, heads, hidden):
    """fp32 data path (arithmetic modes 0 / 1) on dense [B, n, H * 64] tokens; the bf16 data path keeps its per-op sequence."""
    return _BLOCK_COMPOSITE and x.is_cuda and x.shape[2] == heads * _DH and get_gemm_mode() in (GEMM_EXACT, GEMM_SPLIT)


_DH = 64


def _block_sizes(B, n, D, H, hidden, mode):
    key = (B, n, D, H, hidden, mode)
    ent = _BLOCK_SIZES.get(key)
    if ent is None:
        ent = _BLOCK_SIZES[key] = (lib.query("d2s_block_saved_floats", B, n, D, H, hidden, 1), lib.query("d2s_block_saved_floats", B, n, D, H, hidden, 0),
                                   lib.query("d2s_block_bwd_scratch_floats", B, n, D, H, hidden), lib.query("d2s_block_workspace_bytes", B, n, D, hidden, mode),
                                   lib.query("d2s_block_wgrad_workspace_bytes", B, n, D, hidden, mode),
                                   lib.query("d2s_block_bwd_dp_scratch_floats", B, n, D, H, hidden))
    return ent


def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _dp_row(s, B):
    if s is not None:
        assert s.dtype == torch.float32 and s.is_contiguous() and s.numel() == B and s.is_cuda, "a drop-path row is [B] fp32 on the device"
    return s


def block_fwd(x, params, B, n, D, H, hidden, eps, scale, want_cls, train, s_attn=None, s_mlp=None):
    """-> (y [B,n,D], cls_row [B,H,n] or None, slab): slab holds what block_bwd needs when train, forward-only scratch otherwise.
    s_attn / s_mlp: [B] rows of the drop_path_scales table (stochastic depth), None = branch not dropped."""
    mode = get_gemm_mode()
    sz = _block_sizes(B, n, D, H, hidden, mode)
    slab = torch.empty((sz[0] if train else sz[1],), dtype=torch.float32, device=x.device)
    y = torch.empty((B, n, D), dtype=torch.float32, device=x.device)
    cls_row = torch.empty((B, H, n), dtype=torch.float32, device=x.device) if want_cls else None
    ws = workspace(sz[3], x.device)
    if s_attn is None and s_mlp is None:
        lib.call("d2s_block_fwd_f32", lib.ptr(x), _ptr_array(params), B, n, D, H, hidden, float(eps), float(scale), lib.ptr(y), lib.ptr(cls_row),
                 lib.ptr(slab), int(train), mode, lib.ptr(ws), ws.numel())
    else:
        lib.call("d2s_block_fwd_f32_dp", lib.ptr(x), _ptr_array(params), lib.ptr(_dp_row(s_attn, B)), lib.ptr(_dp_row(s_mlp, B)), B, n, D, H, hidden,
                 float(eps), float(scale), lib.ptr(y), lib.ptr(cls_row), lib.ptr(slab), int(train), mode, lib.ptr(ws), ws.numel())
    return y, cls_row, slab


def block_bwd(gy, x, slab, params, B, n, D, H, hidden, scale, want_dx, dparams, s_attn=None, s_mlp=None):
    """dparams: 12 gradient buffers (None = not wanted; LayerNorm weight / bias come as a pair).  -> dx [B,n,D] or None
    s_attn / s_mlp: the rows the forward ran with."""
    mode = get_gemm_mode()
    sz = _block_sizes(B, n, D, H, hidden, mode)
    dev = gy.device
    dp = s_attn is not None or s_mlp is not None
    scratch = torch.empty((sz[5] if dp else sz[2],), dtype=torch.float32, device=dev)
    dx = torch.empty((B, n, D), dtype=torch.float32, device=dev) if want_dx else None
    # input gradients through the cached k-contiguous W^T copies (exact mode, arena weights, enough rows: linear_dgrad's rule)
    wt = [None] * 4
    if mode == GEMM_EXACT and B * n >= _DGRAD_NT_MIN_ROWS and D % 16 == 0 and hidden % 16 == 0:
        for i, w in enumerate((params[2], params[4], params[8], params[10])):
            if _in_weight_arena(w.data_ptr()):
                wt[i] = transposed_weight(w)
    side = _WGRAD["stream"] if (_WGRAD["on"] and any(dparams[i] is not None for i in (2, 3, 4, 5, 8, 9, 10, 11))) else None
    ws_side = workspace_on(side, sz[4], dev) if side is not None else None
    ws = workspace(sz[3] if side is not None else max(sz[3], sz[4]), dev)      # in line, the weight gradients use the main scratch too
    tail = (lib.ptr(dx), _ptr_array(dparams), lib.ptr(scratch), mode, lib.ptr(ws), ws.numel(), lib.ptr(ws_side),
            ws_side.numel() if ws_side is not None else 0, side.cuda_stream if side is not None else None)
    if dp:
        lib.call("d2s_block_bwd_f32_dp", lib.ptr(gy), lib.ptr(x), lib.ptr(slab), _ptr_array(params), _ptr_array(wt), lib.ptr(_dp_row(s_attn, B)),
                 lib.ptr(_dp_row(s_mlp, B)), B, n, D, H, hidden, float(scale), *tail)
    else:
        lib.call("d2s_block_bwd_f32", lib.ptr(gy), lib.ptr(x), lib.ptr(slab), _ptr_array(params), _ptr_array(wt), B, n, D, H, hidden, float(scale), *tail)
    if side is not None:       # autograd may free these on the main stream while the side stream still reads / writes them
        for t in (gy, slab, scratch):
            t.record_stream(side)
        for t in dparams:
            if t is not None:
                t.record_stream(side)
        _WGRAD["used"] = True
    return dx


# ---- stochastic depth (csrc/droppath.hip) ----
def drop_path_scales(rates, B, seed, out=None):
    """[R, B] table of 0 / (1 / keep) from rates [R] (fp32, device) and a 64-bit seed: row 2i = block i's attention branch, 2i + 1 its MLP branch."""
    _f32(rates)
    R = rates.numel()
    if out is None:
        out = torch.empty((R, B), dtype=torch.float32, device=rates.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (R, B)
    lib.call("d2s_drop_path_scales", lib.ptr(rates), lib.ptr(out), R, B, int(seed) & 0xFFFFFFFFFFFFFFFF)
    return out


def scale_rows(g, rowscale, rows_per_group, out=None):
    """out[m] = rowscale[m // rows_per_group] * g[m] for g [M, D]."""
    _f32(g)
    _f32(rowscale)
    M, D = g.shape
    assert rowscale.numel() * rows_per_group >= M
    if out is None:
        out = torch.empty_like(g)
    lib.call("d2s_scale_rows", lib.ptr(g), lib.ptr(rowscale), lib.ptr(out), M, D, int(rows_per_group))
    return out


def drop_path_fwd(x, s):
    """x [B, ...] * s[b] (DropPath.forward with the draws given; also its backward)."""
    _f32(x)
    _f32(s)
    B = x.shape[0]
    assert s.numel() == B
    out = torch.empty_like(x)
    lib.call("d2s_drop_path_fwd", lib.ptr(x), lib.ptr(s), lib.ptr(out), B, x.numel() // B)
    return out


KL_LOGIT_TARGET, KL_PROB_TARGET, CE_LABEL, MSE_TARGET, SOFT_CE = 0, 1, 2, 3, 4


def teacher_target(cls_attn):
    B, L, H, n = cls_attn.shape
    out = torch.empty((B, n - 1), dtype=torch.float32, device=cls_attn.device)
    lib.call("d2s_teacher_target", lib.ptr(_f32(cls_attn)), lib.ptr(out), B, L, H, n)
    return out


def gather_renorm(target, ids, normalize=True):
    B, T = target.shape
    k = ids.shape[1]
    out = torch.empty((B, k), dtype=torch.float32, device=target.device)
    lib.call("d2s_gather_renorm", lib.ptr(_f32(target)), lib.ptr(ids), lib.ptr(out), B, T, k, int(normalize))
    return out


def kl_rows(s, s_map, rows, C, mode, t=None, t_map=(1, 0, 0, 0), t_ids=None, labels=None, want_grad=True, row_weight=None):
    """row_weight [rows]: every row's loss and gradient are scaled by it (mask / count restricts a mean to the kept tokens)."""
    loss_row = torch.empty((rows,), dtype=torch.float32, device=s.device)
    grad = torch.empty((rows, C), dtype=torch.float32, device=s.device) if want_grad else None
    lib.call("d2s_kl_rows", lib.ptr(s), *s_map, lib.ptr(t), *t_map, lib.ptr(t_ids), lib.ptr(labels), lib.ptr(loss_row),
             lib.ptr(grad), rows, C, mode, lib.ptr(row_weight))
    return loss_row, grad


# ---- dynamic keep ratio (--patch-score-threshold): vit_models/dynamic_vit.py:880-894, :935-949 ----
def select_threshold(probs, threshold, lead=0):
    """-> (mask [B, lead + T] float 0/1, counts [B] int32): keep the tokens whose ascending cumulative probability exceeds `threshold`;
    the `lead` first columns are 1 (lead=1: the attention policy row [CLS, tokens])."""
    _f32(probs)
    B, T = probs.shape
    mask = torch.empty((B, lead + T), dtype=torch.float32, device=probs.device)
    counts = torch.empty((B,), dtype=torch.int32, device=probs.device)
    lib.call("d2s_select_threshold", lib.ptr(probs), B, T, float(threshold), lib.ptr(mask), lead + T, int(lead), lib.ptr(counts))
    return mask, counts


def gather_rows_i32(src, idx, rows):
    D = src.shape[-1]
    dst = torch.empty((rows, D), dtype=torch.float32, device=src.device)
    lib.call("d2s_gather_rows_i32", lib.ptr(_f32(src)), lib.ptr(idx), lib.ptr(dst), rows, D)
    return dst


def ragged_offsets(counts, extra=1):
    cu = torch.empty((counts.numel() + 1,), dtype=torch.int32, device=counts.device)
    lib.call("d2s_ragged_offsets", lib.ptr(counts), counts.numel(), int(extra), lib.ptr(cu))
    return cu


def ragged_pack(x, mask, cu, total):
    """x [B,n,D], mask [B,n-1], cu [B+1] -> (packed [total,D], row_src [total] int32 = source token of every packed row)."""
    _f32(x), _f32(mask)
    B, n, D = x.shape
    out = torch.empty((total, D), dtype=torch.float32, device=x.device)
    src = torch.empty((total,), dtype=torch.int32, device=x.device)
    lib.call("d2s_ragged_pack", lib.ptr(x), lib.ptr(mask), lib.ptr(cu), lib.ptr(out), lib.ptr(src), B, n, D)
    return out, src


# ---- ragged inference through every threshold stage: a stage after the first, on the packed batch (csrc/ragged.hip) ----
def half_mean_concat_varlen(x, cu, B):
    """x [total, C] packed, cu [B+1] -> [total, C]: the first half copied, the second half the mean over each image's non-CLS rows."""
    _f32(x)
    total, C = x.shape
    out = torch.empty((total, C), dtype=torch.float32, device=x.device)
    lib.call("d2s_half_mean_concat_varlen", lib.ptr(x), lib.ptr(cu), lib.ptr(out), int(B), C)
    return out


def ragged_select_threshold(scores, cu, row_src, threshold, N, B, want_probs=False):
    """scores [total] packed (CLS entries ignored) -> (keep [total] float 0/1 with 1 at the CLS rows, counts [B] int32 kept non-CLS
    rows, dense_mask [B, N] in original patch coordinates, probs [total] or None)."""
    _f32(scores)
    total = scores.numel()
    dev = scores.device
    keep = torch.empty((total,), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    dense = torch.empty((B, N), dtype=torch.float32, device=dev)
    probs = torch.empty((total,), dtype=torch.float32, device=dev) if want_probs else None
    lib.call("d2s_ragged_select_threshold", lib.ptr(scores), lib.ptr(cu), lib.ptr(row_src), float(threshold), int(N), lib.ptr(probs),
             lib.ptr(keep), lib.ptr(counts), lib.ptr(dense), int(B))
    return keep, counts, dense, probs


def ragged_repack(x, keep, cu_old, cu_new, row_src_old, total_new, B):
    """x [total, D] packed, keep [total] -> (packed [total_new, D], row_src [total_new] int32 = original token index of every row)."""
    _f32(x), _f32(keep)
    D = x.shape[1]
    out = torch.empty((total_new, D), dtype=torch.float32, device=x.device)
    src = torch.empty((total_new,), dtype=torch.int32, device=x.device)
    lib.call("d2s_ragged_repack", lib.ptr(x), lib.ptr(keep), lib.ptr(cu_old), lib.ptr(cu_new), lib.ptr(row_src_old), lib.ptr(out),
             lib.ptr(src), int(B), D)
    return out, src


# ---- adaptive token sampling at inference: a stage on the packed batch (csrc/ats.hip) ----
def ats_select(cls_row, qkv, cu, row_src, K, N, B, H, max_n, want_dense=True):
    """cls_row [H, total] fp32 (the varlen attention's CLS softmax rows), qkv [total, 3 * H * 64] fp32 or bf16, read in place
    -> (score [total] with 0 at the CLS rows, keep [total] float 0/1 with 1 at the CLS rows, counts [B] int32 kept non-CLS rows,
    dense_mask [B, N] in original patch coordinates or None)."""
    _f32(cls_row)
    assert qkv.dtype in (torch.float32, torch.bfloat16) and qkv.is_contiguous(), (qkv.dtype, qkv.is_contiguous())
    total = qkv.shape[0]
    assert cls_row.shape == (H, total) and qkv.shape[1] == 3 * H * 64 and row_src.numel() == total and cu.numel() == B + 1
    dev = qkv.device
    score = torch.empty((total,), dtype=torch.float32, device=dev)
    keep = torch.empty((total,), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    dense = torch.empty((B, N), dtype=torch.float32, device=dev) if want_dense else None
    lib.call("d2s_ats_select", lib.ptr(cls_row), lib.ptr(qkv), int(qkv.dtype == torch.bfloat16), lib.ptr(cu), lib.ptr(row_src), int(K), int(N),
             int(B), int(H), int(total), int(max_n), lib.ptr(score), lib.ptr(keep), lib.ptr(counts), lib.ptr(dense))
    return score, keep, counts, dense


def mask_row_weights(mask):
    m = _f32(mask).reshape(-1)
    w = torch.empty_like(m)
    lib.call("d2s_mask_row_weights", lib.ptr(m), m.numel(), lib.ptr(w))
    return w


def dense_mask_agreement(a, b):
    B, T = a.shape
    out = torch.empty((B,), dtype=torch.float32, device=a.device)
    lib.call("d2s_dense_mask_agreement", lib.ptr(_f32(a)), lib.ptr(_f32(b)), B, T, lib.ptr(out))
    return out


def patch_keep_mask(kept, N):
    """visualizations.py:18-26: kept ids [B,k] -> int64 mask [B,N] in token order (1 = kept)."""
    assert kept.dtype == torch.int64 and kept.is_contiguous()
    B, k = kept.shape
    mask = torch.empty((B, N), dtype=torch.int64, device=kept.device)
    lib.call("d2s_patch_keep_mask", lib.ptr(kept) if k else None, B, k, N, lib.ptr(mask))
    return mask


def compose_ids(prev, rel):
    """stage-relative ids -> the coordinates `prev` is expressed in: out[b,j] = prev[b, rel[b,j]]."""
    B, k = rel.shape
    out = torch.empty_like(rel)
    lib.call("d2s_compose_ids", lib.ptr(prev.contiguous()), prev.shape[1], lib.ptr(rel.contiguous()), k, lib.ptr(out), B)
    return out


def attn_policy_fwd(qkv, policy, B, n, H, scale, eps=1e-6, want_cls=False):
    out = torch.empty((B * n, H * 64), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    cinv = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    cls_row = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device) if want_cls else None
    lib.call("d2s_attn_policy_fwd_f32", lib.ptr(qkv), lib.ptr(_f32(policy)), lib.ptr(out), lib.ptr(lse), lib.ptr(cinv), lib.ptr(cls_row),
             B, n, H, float(scale), float(eps))
    return out, lse, cinv, cls_row


def attn_policy_bwd(qkv, policy, out, dout, lse, cinv, B, n, H, scale):
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    lib.call("d2s_attn_policy_bwd_f32", lib.ptr(qkv), lib.ptr(policy), lib.ptr(out), lib.ptr(dout), lib.ptr(lse), lib.ptr(cinv),
             lib.ptr(dqkv), lib.ptr(delta), B, n, H, float(scale))
    return dqkv


def attn_policy_bwd_dpol(qkv, policy, out, dout, lse, cinv, B, n, H, scale):
    """attn_policy_bwd plus the gradient of the policy (DynamicViT baseline).  -> (dqkv, dpolicy [B, n], column 0 = 0)"""
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    part = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    dpolicy = torch.empty((B, n), dtype=torch.float32, device=qkv.device)
    lib.call("d2s_attn_policy_bwd_dpol_f32", lib.ptr(qkv), lib.ptr(policy), lib.ptr(out), lib.ptr(dout), lib.ptr(lse), lib.ptr(cinv),
             lib.ptr(dqkv), lib.ptr(delta), lib.ptr(dpolicy), lib.ptr(part), B, n, H, float(scale))
    return dqkv, dpolicy


def attn_policy_fwd_bf16io(qkv, policy, B, n, H, scale, eps=1e-6, want_cls=False, want_f32=True, want_bf16=True):
    """Policy attention on the bf16 matrix cores (bf16 arithmetic mode): qkv fp32 or bf16 (the qkv GEMM's c16); the fp32 output (the
    backward needs it), its bf16 copy for the projection GEMM, or both.  -> (out or None, lse, cinv, cls_row, out16 or None)"""
    assert qkv.is_contiguous() and qkv.dtype in (torch.float32, torch.bfloat16) and (want_f32 or want_bf16)
    out = torch.empty((B * n, H * 64), dtype=torch.float32, device=qkv.device) if want_f32 else None
    out16 = bf16_buffer(B * n, H * 64, qkv.device) if want_bf16 else None
    lse = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    cinv = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    cls_row = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device) if want_cls else None
    lib.call("d2s_attn_policy_fwd_bf16", lib.ptr(qkv), int(qkv.dtype == torch.bfloat16), lib.ptr(_f32(policy)), lib.ptr(out), lib.ptr(out16),
             lib.ptr(lse), lib.ptr(cinv), lib.ptr(cls_row), B, n, H, float(scale), float(eps))
    return out, lse, cinv, cls_row, out16


def attn_policy_bwd_bf16io(qkv, policy, out, dout, lse, cinv, B, n, H, scale, dqkv16=None, want_f32=True, want_dpolicy=False):
    """Backward of attn_policy_fwd_bf16io.  dqkv16: bf16 buffer shaped like qkv that receives a copy of dqkv; want_f32=False (needs dqkv16):
    only that form is written.  -> (dqkv or None, dpolicy [B, n] with column 0 = 0, or None)"""
    assert qkv.is_contiguous() and qkv.dtype in (torch.float32, torch.bfloat16)
    assert dqkv16 is None or (dqkv16.dtype == torch.bfloat16 and dqkv16.is_contiguous() and dqkv16.numel() == qkv.numel())
    dqkv = torch.empty(qkv.shape, dtype=torch.float32, device=qkv.device) if (want_f32 or dqkv16 is None) else None
    delta = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    part = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device) if want_dpolicy else None
    dpolicy = torch.empty((B, n), dtype=torch.float32, device=qkv.device) if want_dpolicy else None
    lib.call("d2s_attn_policy_bwd_bf16", lib.ptr(qkv), int(qkv.dtype == torch.bfloat16), lib.ptr(_f32(policy)), lib.ptr(out), lib.ptr(dout),
             lib.ptr(lse), lib.ptr(cinv), lib.ptr(dqkv), lib.ptr(dqkv16), lib.ptr(delta), lib.ptr(dpolicy), lib.ptr(part), B, n, H, float(scale))
    return dqkv, dpolicy


def attn_varlen_fwd(qkv, cu, B, total, max_n, H, scale, want_cls=False):
    out = torch.empty((total, H * 64), dtype=torch.float32, device=qkv.device)
    cls_row = torch.empty((H, total), dtype=torch.float32, device=qkv.device) if want_cls else None
    lib.call("d2s_attn_varlen_fwd_f32", lib.ptr(qkv), lib.ptr(cu), lib.ptr(out), lib.ptr(cls_row), B, total, max_n, H, float(scale))
    return out, cls_row


# ---- training through a ragged packed batch (csrc/attention_f32.hip's VARLEN backward, csrc/ragged_train.hip) ----
def attn_varlen_fwd_lse(qkv, cu, B, total, max_n, H, scale, want_cls=False):
    """attn_varlen_fwd that keeps the log-sum-exp for attn_varlen_bwd: the same kernel, out / cls_row bit for bit that call's.
    -> (out [total, H * 64], lse [H, total], cls_row [H, total] or None)"""
    assert qkv.dtype == torch.float32 and qkv.is_contiguous()
    out = torch.empty((total, H * 64), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((H, total), dtype=torch.float32, device=qkv.device)
    cls_row = torch.empty((H, total), dtype=torch.float32, device=qkv.device) if want_cls else None
    lib.call("d2s_attn_varlen_fwd_lse_f32", lib.ptr(qkv), lib.ptr(cu), lib.ptr(out), lib.ptr(lse), lib.ptr(cls_row), int(B), int(total),
             int(max_n), int(H), float(scale))
    return out, lse, cls_row


def attn_varlen_bwd(qkv, cu, out, dout, lse, B, total, max_n, H, scale):
    """Backward of attn_varlen_fwd_lse (out, lse as it returned them) -> dqkv shaped like qkv, every element written once."""
    assert qkv.dtype == torch.float32 and qkv.is_contiguous() and tuple(lse.shape) == (H, total)
    _f32(out), _f32(dout), _f32(lse)
    dqkv = torch.empty(qkv.shape, dtype=torch.float32, device=qkv.device)
    delta = torch.empty((H, total), dtype=torch.float32, device=qkv.device)
    lib.call("d2s_attn_varlen_bwd_f32", lib.ptr(qkv), lib.ptr(cu), lib.ptr(out), lib.ptr(dout), lib.ptr(lse), lib.ptr(dqkv), lib.ptr(delta),
             int(B), int(total), int(max_n), int(H), float(scale))
    return dqkv


def ragged_repack_bwd(g_new, keep, cu_old, cu_new, total_old, B, g16=None):
    """Backward of ragged_repack: g_new [total_new, D] -> g_old [total_old, D], a kept row takes the row it became, a dropped row zeros.
    g16 (the bf16 data path behind a stage): a bf16 buffer [total_old, D] that receives g_old rounded once, in the same launch."""
    _f32(g_new), _f32(keep)
    D = g_new.shape[1]
    g_old = torch.empty((total_old, D), dtype=torch.float32, device=g_new.device)
    if g16 is not None:
        assert g16.dtype == torch.bfloat16 and g16.is_contiguous() and g16.numel() == int(total_old) * D and g16.is_cuda
        assert keep.numel() == int(total_old) and cu_old.numel() == int(B) + 1 and cu_new.numel() == int(B) + 1
        lib.call("d2s_ragged_repack_bwd_bf16out", lib.ptr(g_new), lib.ptr(keep), lib.ptr(cu_old), lib.ptr(cu_new), lib.ptr(g_old),
                 lib.ptr(g16), int(B), D)
        return g_old
    lib.call("d2s_ragged_repack_bwd", lib.ptr(g_new), lib.ptr(keep), lib.ptr(cu_old), lib.ptr(cu_new), lib.ptr(g_old), int(B), D)
    return g_old


def ragged_cls_scatter(g_cls, cu, total):
    """Backward of gather_rows_i32(x, cu, B): g_cls [B, D] -> g [total, D] with row cu[b] = g_cls[b] and zeros elsewhere."""
    _f32(g_cls)
    B, D = g_cls.shape
    g = torch.empty((total, D), dtype=torch.float32, device=g_cls.device)
    lib.call("d2s_ragged_cls_scatter", lib.ptr(g_cls), lib.ptr(cu), lib.ptr(g), int(B), int(total), D)
    return g


# ---- training the dynamic keep ratio on the ragged batch (csrc/ragged_threshold.hip) ----
def half_mean_concat_varlen_bwd(g, cu, B):
    """Backward of half_mean_concat_varlen: g [total, C] -> [total, C]; first half copied, second half (1 / T) * the sum over ALL rows of
    the image at its non-CLS rows and 0 at its CLS row."""
    _f32(g)
    total, C = g.shape
    out = torch.empty((total, C), dtype=torch.float32, device=g.device)
    lib.call("d2s_half_mean_concat_varlen_bwd", lib.ptr(g), lib.ptr(cu), lib.ptr(out), int(B), C)
    return out


def ragged_mask_loss_fwd(scores, target, cu, row_src, mode):
    """scores [total] packed, target [B, N] -> loss_rows [B]: per image KL(q || softmax(scores)) (mode KL_PROB_TARGET) or the sum of
    squared differences (mode MSE_TARGET) over its non-CLS rows, q the target gathered at row_src - 1 and renormalised."""
    _f32(scores), _f32(target)
    B, N = target.shape
    assert cu.numel() == B + 1 and row_src.numel() == scores.numel()
    loss_rows = torch.empty((B,), dtype=torch.float32, device=scores.device)
    lib.call("d2s_ragged_mask_loss_fwd", lib.ptr(scores), lib.ptr(target), lib.ptr(cu), lib.ptr(row_src), lib.ptr(loss_rows), B,
             scores.numel(), N, int(mode))
    return loss_rows


def ragged_mask_loss_bwd(scores, target, cu, row_src, mode, scale=1.0):
    """-> dscores [total] = scale * d loss_rows / d scores, exactly 0 at the CLS rows"""
    _f32(scores), _f32(target)
    B, N = target.shape
    assert cu.numel() == B + 1 and row_src.numel() == scores.numel()
    dscores = torch.empty((scores.numel(),), dtype=torch.float32, device=scores.device)
    lib.call("d2s_ragged_mask_loss_bwd", lib.ptr(scores), lib.ptr(target), lib.ptr(cu), lib.ptr(row_src), lib.ptr(dscores), B,
             scores.numel(), N, int(mode), float(scale))
    return dscores


def ragged_teacher_rows(token_t, cu, row_src):
    """token_t [B, N, D] (dense rows; the image stride may be larger, as in the token view of a [B, N + 1, D] tensor), row_src [total]
    -> (out [total, D]: the teacher token of every packed row, zeros at the CLS rows; w [total]: 1 / (total - B), 0 at the CLS rows)"""
    assert token_t.dtype == torch.float32 and token_t.dim() == 3
    if token_t.stride(2) != 1 or token_t.stride(1) != token_t.shape[2]:
        token_t = token_t.contiguous()
    B, N, D = token_t.shape
    total = row_src.numel()
    out = torch.empty((total, D), dtype=torch.float32, device=token_t.device)
    w = torch.empty((total,), dtype=torch.float32, device=token_t.device)
    lib.call("d2s_ragged_teacher_rows", lib.ptr(token_t), int(token_t.stride(0)) if B > 1 else N * D, lib.ptr(cu), lib.ptr(row_src),
             lib.ptr(out), lib.ptr(w), B, total, N, D)
    return out, w


# ---- the A-ViT baseline: per-token adaptive depth on the ragged batch (csrc/avit.hip) ----
def avit_state(B, N, D, L, device):
    """The cleared state of one forward: c, R [B, N] fp32 and halt_layer [B, N] int32 (0: live), acc and ysave [B, D], part [L, B, 3]."""
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=device)
    return dict(c=z(B, N), R=z(B, N), nh=z(B, N, dtype=torch.int32), acc=z(B, D), ysave=z(B, D), part=z(L, B, 3))


_AVIT_THR = {}


def avit_halt(y, cu, row_src, st, layer, last, gamma, beta, eps_halt, save=True):
    """The halting step of block `layer` (1-based) on y [total, D]: updates st (avit_state) in place.
    -> (keep [total], counts [B] int32, w [B], h [total] or None, ycls [B, D] or None); the last two only with save (a backward follows)."""
    _f32(y)
    total, D = y.shape
    B, N = st["c"].shape
    assert cu.numel() == B + 1 and row_src.numel() == total and cu.dtype == torch.int32 and row_src.dtype == torch.int32
    assert 1 <= layer <= st["part"].shape[0] and st["acc"].shape == (B, D)
    dev = y.device
    keep = torch.empty((total,), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    w = torch.empty((B,), dtype=torch.float32, device=dev)
    h = torch.empty((total,), dtype=torch.float32, device=dev) if save else None
    ycls = torch.empty((B, D), dtype=torch.float32, device=dev) if save else None
    thr = _AVIT_THR.get(eps_halt)
    if thr is None:                       # 1 - eps as the fp32 subtraction gives it: the kernel compares against this value, strictly
        thr = _AVIT_THR[eps_halt] = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(float(eps_halt), dtype=torch.float32))
    lib.call("d2s_avit_halt", lib.ptr(y), lib.ptr(cu), lib.ptr(row_src), lib.ptr(st["c"]), lib.ptr(st["R"]), lib.ptr(st["nh"]), lib.ptr(h),
             lib.ptr(w), lib.ptr(st["acc"]), lib.ptr(ycls), lib.ptr(st["ysave"]) if save else None, lib.ptr(keep), lib.ptr(counts),
             lib.ptr(st["part"][layer - 1]), B, N, D, total, int(layer), int(bool(last)), float(gamma), float(beta), thr)
    return keep, counts, w, h, ycls


def avit_halt_bwd(g, h, cu, row_src, st, w, dacc, ycls, gsc, layer, gamma):
    """Backward of avit_halt for block `layer` after the finished forward.  g [total, D]: the gradient that arrived through the re-pack,
    updated in place - or None (the last layer), then a new tensor is written in full.  -> g"""
    B, N = st["c"].shape
    total = h.numel()
    D = dacc.shape[1]
    L = gsc.numel() - 1
    fresh = g is None
    if fresh:
        g = torch.empty((total, D), dtype=torch.float32, device=h.device)
    assert g.is_contiguous() and g.dtype == torch.float32 and tuple(g.shape) == (total, D)
    _f32(dacc), _f32(ycls), _f32(gsc)
    lib.call("d2s_avit_halt_bwd", lib.ptr(g), lib.ptr(h), lib.ptr(cu), lib.ptr(row_src), lib.ptr(st["nh"]), lib.ptr(w), lib.ptr(dacc),
             lib.ptr(ycls), lib.ptr(st["ysave"]), lib.ptr(gsc), B, N, D, total, int(layer), L, int(fresh), float(gamma))
    return g


def avit_halt_repack_bwd_bf16io(g_new, keep, cu_new, h, cu, row_src, st, w, dacc, ycls, gsc, layer, gamma):
    """The backward of an A-ViT block boundary on the bf16 data path, one launch: ragged_repack_bwd, avit_halt_bwd and the cast.  g_new
    [total_new, D] with the keep / cu_new of the boundary's re-pack, or all three None (the last layer: nothing arrived).
    -> (g [total, D] fp32 - the bits of the two ops chained - and g16, the same values rounded once to bf16)"""
    B, N = st["c"].shape
    total = h.numel()
    D = dacc.shape[1]
    L = gsc.numel() - 1
    _f32(dacc), _f32(ycls), _f32(gsc), _f32(h)
    if g_new is not None:
        _f32(g_new), _f32(keep)
        assert g_new.shape[1] == D and keep.numel() == total and cu_new.numel() == B + 1 and cu_new.dtype == torch.int32
    assert cu.numel() == B + 1 and row_src.numel() == total
    g = torch.empty((total, D), dtype=torch.float32, device=h.device)
    g16 = bf16_buffer(total, D, h.device)
    lib.call("d2s_avit_halt_repack_bwd_bf16out", lib.ptr(g_new), lib.ptr(keep), lib.ptr(cu_new), lib.ptr(h), lib.ptr(cu), lib.ptr(row_src),
             lib.ptr(st["nh"]), lib.ptr(w), lib.ptr(dacc), lib.ptr(ycls), lib.ptr(st["ysave"]), lib.ptr(gsc), lib.ptr(g), lib.ptr(g16),
             B, N, D, total, int(layer), L, float(gamma))
    return g, g16


def avit_penalty_fwd(part, tgt, N):
    """part [L, B, 3], tgt [L] -> (out [2] = {ponder mean, distribution prior}, hbar [L], cnt [L])"""
    L, B, _ = part.shape
    _f32(part), _f32(tgt)
    dev = part.device
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    hbar = torch.empty((L,), dtype=torch.float32, device=dev)
    cnt = torch.empty((L,), dtype=torch.float32, device=dev)
    lib.call("d2s_avit_penalty_fwd", lib.ptr(part), lib.ptr(tgt), lib.ptr(out), lib.ptr(hbar), lib.ptr(cnt), L, B, int(N))
    return out, hbar, cnt


def avit_penalty_bwd(hbar, cnt, tgt, dponder, dprior, B, N):
    """dponder, dprior: device scalars -> gsc [L + 1], the factors avit_halt_bwd applies"""
    L = hbar.numel()
    gsc = torch.empty((L + 1,), dtype=torch.float32, device=hbar.device)
    lib.call("d2s_avit_penalty_bwd", lib.ptr(hbar), lib.ptr(cnt), lib.ptr(_f32(tgt)), lib.ptr(_f32(dponder)), lib.ptr(_f32(dprior)),
             lib.ptr(gsc), L, int(B), int(N))
    return gsc


# ---- the LTP baseline: learned per-block token thresholds (csrc/ltp.hip) ----
def ltp_score(qkv, lse, B, n, H, scale, policy=None, cinv=None, cu=None, total=None):
    """The attention every token receives in one block: qkv [rows, 3 * H * 64] and the lse (and cinv) that block's attention forward wrote.
    Plain: lse [B, H, n]; policy: policy [B, n], cinv [B, H, n] as attn_policy_fwd returned them; varlen: cu [B + 1] int32, lse [H, total],
    n = max_n (any upper bound).  -> score [rows] fp32, each image's entries summing to 1.
    qkv in bf16 (the bf16 data path): lse and cinv as the bf16 attention forward wrote them, the score rebuilt on the bf16 matrix cores
    (csrc/ltp_bf16.hip)."""
    if qkv.dtype == torch.bfloat16:
        return _ltp_score_bf16(qkv, lse, B, n, H, scale, policy, cinv, cu, total)
    assert qkv.dtype == torch.float32 and qkv.is_contiguous()
    _f32(lse)
    rows = int(total) if cu is not None else B * n
    assert qkv.numel() == rows * 3 * H * 64 and lse.numel() == rows * H, (tuple(qkv.shape), tuple(lse.shape), rows, H)
    if policy is not None:
        assert cu is None and cinv is not None and policy.numel() == rows and cinv.numel() == rows * H
        _f32(policy), _f32(cinv)
    if cu is not None:
        assert cu.dtype == torch.int32 and cu.numel() == B + 1 and cu.is_contiguous()
    score = torch.empty((rows,), dtype=torch.float32, device=qkv.device)
    need = lib.query("d2s_ltp_score_workspace_bytes", rows, int(H))
    ws = torch.empty((need // 4,), dtype=torch.float32, device=qkv.device)
    lib.call("d2s_ltp_score_f32", lib.ptr(qkv), lib.ptr(lse), lib.ptr(policy), lib.ptr(cinv), lib.ptr(cu), lib.ptr(score), lib.ptr(ws), need,
             int(B), int(n), rows, int(H), float(scale))
    return score


def _ltp_score_bf16(qkv, lse, B, n, H, scale, policy, cinv, cu, total):
    assert qkv.is_contiguous()
    _f32(lse)
    rows = int(total) if cu is not None else B * n
    assert qkv.numel() == rows * 3 * H * 64 and lse.numel() == rows * H, (tuple(qkv.shape), tuple(lse.shape), rows, H)
    if policy is not None:
        assert cu is None and cinv is not None and policy.numel() == rows and cinv.numel() == rows * H
        _f32(policy), _f32(cinv)
    if cu is not None:
        assert cu.dtype == torch.int32 and cu.numel() == B + 1 and cu.is_contiguous()
    score = torch.empty((rows,), dtype=torch.float32, device=qkv.device)
    need = lib.query("d2s_ltp_score_bf16_workspace_bytes", rows, int(H))
    ws = torch.empty((need // 4,), dtype=torch.float32, device=qkv.device)
    lib.call("d2s_ltp_score_bf16", lib.ptr(qkv), lib.ptr(lse), lib.ptr(policy), lib.ptr(cinv), lib.ptr(cu), lib.ptr(score), lib.ptr(ws), need,
             int(B), int(n), rows, int(H), float(scale))
    return score


def ltp_select(score, cu, theta, B, row_src=None, T=0):
    """score [total] packed, theta: a 1-element fp32 device tensor (a view of the parameter; never read on the host)
    -> (keep [total] float 0/1 with 1 at the CLS rows, counts [B] int32 kept non-CLS rows, dense [B, T] in patch coordinates or None)."""
    _f32(score), _f32(theta)
    assert theta.numel() == 1 and cu.dtype == torch.int32 and cu.numel() == B + 1
    total = score.numel()
    keep = torch.empty((total,), dtype=torch.float32, device=score.device)
    counts = torch.empty((B,), dtype=torch.int32, device=score.device)
    dense = None
    if row_src is not None:
        assert row_src.dtype == torch.int32 and row_src.numel() == total and T > 0
        dense = torch.empty((B, T), dtype=torch.float32, device=score.device)
    lib.call("d2s_ltp_select", lib.ptr(score), lib.ptr(cu), lib.ptr(row_src), lib.ptr(theta), lib.ptr(keep), lib.ptr(counts), lib.ptr(dense),
             int(B), int(T), total)
    return keep, counts, dense


def ltp_soft_mask_fwd(score, m_in, theta, tau):
    """score [B, N], m_in [B, N] or None (all ones), theta a 1-element device tensor -> (M [B, N], m_out = m_in * M, msum [B])"""
    _f32(score), _f32(theta)
    B, N = score.shape
    assert theta.numel() == 1 and (m_in is None or tuple(_f32(m_in).shape) == (B, N))
    M, m_out = torch.empty_like(score), torch.empty_like(score)
    msum = torch.empty((B,), dtype=torch.float32, device=score.device)
    lib.call("d2s_ltp_soft_mask_fwd", lib.ptr(score), lib.ptr(m_in), lib.ptr(theta), lib.ptr(M), lib.ptr(m_out), lib.ptr(msum), B, N,
             1.0 / float(tau))
    return M, m_out, msum


def ltp_soft_mask_bwd(g_out, M, m_in, tau, dtheta, greg=None, gm_in=None, want_gm=True, accumulate_dtheta=False):
    """Backward of ltp_soft_mask_fwd.  greg [B] or None: the gradient of msum; dtheta: the 1-element gradient slot, written (or added
    to); gm_in: a [B, N] tensor to add g_out * M to, or None: a fresh one is written when want_gm.  -> (gM [B, N], gm_in or None)"""
    _f32(g_out), _f32(M), _f32(dtheta)
    B, N = M.shape
    assert dtheta.numel() == 1 and tuple(g_out.shape) == (B, N) and (m_in is None or tuple(_f32(m_in).shape) == (B, N))
    assert greg is None or _f32(greg).numel() == B
    accumulate_gm = gm_in is not None
    if gm_in is None and want_gm:
        gm_in = torch.empty_like(M)
    gM = torch.empty_like(M)
    part = torch.empty((B,), dtype=torch.float32, device=M.device)
    lib.call("d2s_ltp_soft_mask_bwd", lib.ptr(g_out), lib.ptr(M), lib.ptr(m_in), lib.ptr(greg), lib.ptr(gM), lib.ptr(gm_in), lib.ptr(dtheta),
             lib.ptr(part), B, N, 1.0 / float(tau), int(accumulate_gm), int(bool(accumulate_dtheta)))
    return gM, gm_in


# ---- graph ranking: PageRank over a block's attention (csrc/graph_rank.hip) ----
def graph_rank(qkv, lse, B, n, H, scale, iters, w0=None):
    """`iters` steps of s <- s P per image and head, P = exp(scale q k^T - lse) recomputed from the block's fp32 qkv [B * n, 3 * H * 64]
    and the lse [B, H, n] its attention forward wrote; the start is w0 [B, H, n] or 1 / n.  -> rank [B, H, n] fp32, the layout of a CLS
    row; every (image, head) keeps the mass of its start (1 without w0).  The ping-pong buffer of iters >= 2 is allocated here."""
    assert qkv.dtype == torch.float32 and qkv.is_contiguous()
    _f32(lse)
    B, n, H, iters = int(B), int(n), int(H), int(iters)
    assert qkv.numel() == B * n * 3 * H * 64 and lse.numel() == B * n * H, (tuple(qkv.shape), tuple(lse.shape), B, n, H)
    if w0 is not None:
        assert _f32(w0).numel() == B * H * n
    rank = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device)
    ws = torch.empty((B, H, n), dtype=torch.float32, device=qkv.device) if iters >= 2 else None
    lib.call("d2s_graph_rank_f32", lib.ptr(qkv), lib.ptr(lse), lib.ptr(w0), lib.ptr(rank), lib.ptr(ws), B, n, H, float(scale), iters)
    return rank


# ---- the similarity stage after attention ranking (csrc/sim_prune.hip) ----
def key_metric(qkv, B, n, H):
    """The key metric of a block's tokens from its fp32 qkv [B * n, 3 * H * 64], read in place (the K third only): -> metric [B, n, 64],
    row t = the mean of token t's keys over the heads divided by its L2 norm (tome_match's metric; a zero row gives NaN)"""
    assert qkv.dtype == torch.float32 and qkv.is_contiguous()
    B, n, H = int(B), int(n), int(H)
    assert qkv.numel() == B * n * 3 * H * 64, (tuple(qkv.shape), B, n, H)
    metric = torch.empty((B, n, 64), dtype=torch.float32, device=qkv.device)
    lib.call("d2s_key_metric_f32", lib.ptr(qkv), B, n, H, lib.ptr(metric))
    return metric


def sim_prune_clip_r(R, k, T):
    """A stage's own similarity-pruning count: at most k (so that r <= half of the k + r candidates) and at most the T - k tokens that
    the importance ranking would drop anyway"""
    return max(0, min(int(R), int(k), int(T) - int(k)))


def sim_prune(metric, probs, cand, lead, r):
    """metric [B, n, 64] (key_metric), probs [B, T] and cand [B, c] as select_cls_attn returned them for c candidates, r the effective
    count (sim_prune_clip_r, 0 <= r <= c // 2): the c // 2 least important candidates are matched against the others by the cosine of
    their metrics and the r with the closest partner are pruned.
    -> (kept [B, c - r], dropped [B, T - c + r], pruned [B, r], partner [B, r], sim [B, r]); ids int64 ascending, the plan in pruned order"""
    _f32(metric), _f32(probs)
    assert cand.dtype == torch.int64 and cand.is_contiguous()
    B, n, _ = metric.shape
    T, c, r = int(probs.shape[1]), int(cand.shape[1]), int(r)
    assert metric.shape[2] == 64 and tuple(probs.shape) == (B, T) and tuple(cand.shape) == (B, c), (tuple(metric.shape), tuple(probs.shape),
                                                                                                   tuple(cand.shape))
    i64 = dict(dtype=torch.int64, device=metric.device)
    k = max(c - r, 0)
    kept, dropped = torch.empty((B, k), **i64), torch.empty((B, max(T - k, 0)), **i64)
    pruned, partner = torch.empty((B, max(r, 0)), **i64), torch.empty((B, max(r, 0)), **i64)
    sim = torch.empty((B, max(r, 0)), dtype=torch.float32, device=metric.device)
    lib.call("d2s_sim_prune_f32", lib.ptr(metric), lib.ptr(probs), lib.ptr(cand), B, n, int(lead), T, c, r, lib.ptr(kept),
             lib.ptr(dropped) if T - k > 0 else None, *((lib.ptr(pruned), lib.ptr(partner), lib.ptr(sim)) if r > 0 else (None, None, None)))
    return kept, dropped, pruned, partner, sim


# ---- the Evo-ViT baseline: slow-fast token update (csrc/evo.hip) ----
def _evo_shapes(X, kept, dropped):
    B, n, D = X.shape
    T, k = n - 1, kept.shape[1]
    assert kept.dtype == torch.int64 and kept.is_contiguous() and dropped.dtype == torch.int64 and dropped.is_contiguous()
    assert kept.shape == (B, k) and dropped.shape == (B, T - k), f"X {tuple(X.shape)}: kept must be [B, k], dropped [B, {T} - k]"
    return B, T, k, D


def evo_select(cls_row, k, tau=0.0, g=None, kept_prev=None):
    """The score evolution and the re-selection of a slow-fast block in one launch.  Without kept_prev: cls_row [B,H,1+T] starts the score,
    g = mean over heads of its token columns.  With it: cls_row [B,H,k+2] is the row of the block that ran on kept_prev [B,k] and
    g_out = g with g_out[kept_prev_i] = (1 - tau) g[kept_prev_i] + tau mean_h cls_row[:, h, 1+i].  -> (g_out [B,T], kept [B,k],
    dropped [B,T-k]), the lists as select_topk(g_out, k) gives them"""
    _f32(cls_row)
    B, H, n_c = cls_row.shape
    k = int(k)
    if kept_prev is None:
        T = n_c - 1
    else:
        _f32(g)
        T = g.shape[1]
        assert kept_prev.dtype == torch.int64 and kept_prev.is_contiguous() and tuple(kept_prev.shape) == (B, k) and n_c == k + 2 \
            and g.shape[0] == B, (tuple(cls_row.shape), tuple(g.shape), tuple(kept_prev.shape), k)
    dev = cls_row.device
    g_out = torch.empty((B, T), dtype=torch.float32, device=dev)
    kept = torch.empty((B, k), dtype=torch.int64, device=dev)
    dropped = torch.empty((B, max(T - k, 0)), dtype=torch.int64, device=dev)
    lib.call("d2s_evo_select", lib.ptr(g), lib.ptr(kept_prev), lib.ptr(cls_row), lib.ptr(g_out), lib.ptr(kept), lib.ptr(dropped), B, H, T,
             k, float(tau))
    return g_out, kept, dropped


def evo_scatter_fwd(X, yc, xc, kept, dropped):
    """The write-back of a slow-fast block, in place on X [B,1+T,D]: CLS and kept rows from yc [B,k+2,D], every dropped row
    += yc[:, k+1] - xc[:, k+1].  -> X"""
    _f32(X), _f32(yc), _f32(xc)
    B, T, k, D = _evo_shapes(X, kept, dropped)
    assert yc.shape == xc.shape == (B, k + 2, D)
    lib.call("d2s_evo_scatter_fwd", lib.ptr(yc), lib.ptr(xc), lib.ptr(kept), lib.ptr(dropped), lib.ptr(X), B, T, k, D)
    return X


def evo_scatter_bwd(dX, kept, dropped):
    """dX [B,1+T,D], the gradient of the written-back X -> dyc [B,k+2,D]; its last row is delta, the sum of the dropped rows of dX"""
    _f32(dX)
    B, T, k, D = _evo_shapes(dX, kept, dropped)
    dyc = torch.empty((B, k + 2, D), dtype=torch.float32, device=dX.device)
    lib.call("d2s_evo_scatter_bwd", lib.ptr(dX), lib.ptr(kept), lib.ptr(dropped), lib.ptr(dyc), B, T, k, D)
    return dyc


def evo_gather_bwd(dX, dxc, dyc, g, S, kept, dropped):
    """In place on dX [B,1+T,D] (in: the gradient of the written-back X; out: the gradient of X before the block): CLS and kept rows from
    dxc [B,k+2,D], dropped row j += (g_j / S) (dxc[:, k+1] - dyc[:, k+1]).  -> dX"""
    _f32(dX), _f32(dxc), _f32(dyc), _f32(g), _f32(S)
    B, T, k, D = _evo_shapes(dX, kept, dropped)
    assert dxc.shape == dyc.shape == (B, k + 2, D) and g.shape == (B, T) and S.shape == (B,)
    lib.call("d2s_evo_gather_bwd", lib.ptr(dxc), lib.ptr(dyc), lib.ptr(g), lib.ptr(S), lib.ptr(kept), lib.ptr(dropped), lib.ptr(dX), B, T,
             k, D)
    return dX


def attn_varlen_fwd_bf16io(qkv, cu, B, total, max_n, H, scale, want_cls=False, want_f32=True):
    """Ragged attention forward on the bf16 matrix cores (bf16 arithmetic mode): qkv [total, 3*H*64] fp32 or bf16 (the qkv GEMM's c16);
    always writes the bf16 copy of its output for the projection GEMM.  -> (out or None, cls_row [H, total] or None, out16)"""
    assert qkv.is_contiguous() and qkv.dtype in (torch.float32, torch.bfloat16)
    out = torch.empty((total, H * 64), dtype=torch.float32, device=qkv.device) if want_f32 else None
    out16 = bf16_buffer(total, H * 64, qkv.device)
    cls_row = torch.empty((H, total), dtype=torch.float32, device=qkv.device) if want_cls else None
    lib.call("d2s_attn_varlen_fwd_bf16", lib.ptr(qkv), int(qkv.dtype == torch.bfloat16), lib.ptr(cu), lib.ptr(out), lib.ptr(out16),
             lib.ptr(cls_row), B, total, max_n, H, float(scale))
    return out, cls_row, out16


# ---- training on the ragged batch in the bf16 arithmetic mode (csrc/attention_bf16.hip's VLSE forward and VARLEN backward) ----
def attn_varlen_fwd_lse_bf16io(qkv, cu, B, total, max_n, H, scale, want_cls=False, want_f32=True):
    """attn_varlen_fwd_bf16io that keeps the log-sum-exp for attn_varlen_bwd_bf16io: out / out16 / cls_row bit for bit that call's; qkv fp32
    or bf16.  -> (out or None, lse [H, total], cls_row [H, total] or None, out16)"""
    assert qkv.is_contiguous() and qkv.dtype in (torch.float32, torch.bfloat16)
    out = torch.empty((total, H * 64), dtype=torch.float32, device=qkv.device) if want_f32 else None
    out16 = bf16_buffer(total, H * 64, qkv.device)
    lse = torch.empty((H, total), dtype=torch.float32, device=qkv.device)
    cls_row = torch.empty((H, total), dtype=torch.float32, device=qkv.device) if want_cls else None
    lib.call("d2s_attn_varlen_fwd_lse_bf16", lib.ptr(qkv), int(qkv.dtype == torch.bfloat16), lib.ptr(cu), lib.ptr(out), lib.ptr(out16),
             lib.ptr(lse), lib.ptr(cls_row), int(B), int(total), int(max_n), int(H), float(scale))
    return out, lse, cls_row, out16


def attn_varlen_bwd_bf16io(qkv, cu, out, dout, lse, B, total, max_n, H, scale, dqkv16=None, want_f32=True):
    """Backward of attn_varlen_fwd_lse_bf16io (out its fp32 output, lse as it returned them); qkv fp32 or bf16.  dqkv16: bf16 buffer shaped
    like qkv that receives a copy of dqkv; want_f32=False (needs dqkv16): only that form is written and None is returned."""
    assert qkv.is_contiguous() and qkv.dtype in (torch.float32, torch.bfloat16) and tuple(lse.shape) == (H, total)
    _f32(out), _f32(dout), _f32(lse)
    assert out.numel() == dout.numel() == total * H * 64 and qkv.numel() == 3 * total * H * 64
    if dqkv16 is not None:
        assert dqkv16.dtype == torch.bfloat16 and dqkv16.is_contiguous() and dqkv16.numel() == qkv.numel()
    dqkv = torch.empty(qkv.shape, dtype=torch.float32, device=qkv.device) if (want_f32 or dqkv16 is None) else None
    delta = torch.empty((H, total), dtype=torch.float32, device=qkv.device)
    lib.call("d2s_attn_varlen_bwd_bf16", lib.ptr(qkv), int(qkv.dtype == torch.bfloat16), lib.ptr(cu), lib.ptr(out), lib.ptr(dout), lib.ptr(lse),
             lib.ptr(dqkv), lib.ptr(dqkv16), lib.ptr(delta), int(B), int(total), int(max_n), int(H), float(scale))
    return dqkv


def sum_scalar(v, scale=1.0):
    out = torch.empty((), dtype=torch.float32, device=v.device)
    lib.call("d2s_sum_scalar", lib.ptr(v), v.numel(), float(scale), lib.ptr(out))
    return out


def scale_by_scalar(x, gscalar, scale=1.0):
    y = torch.empty_like(x)
    lib.call("d2s_scale_by_scalar", lib.ptr(x), lib.ptr(gscalar), float(scale), lib.ptr(y), x.numel())
    return y


def mask_agreement(ids_a, ids_b, T):
    B, k = ids_a.shape
    out = torch.empty((B,), dtype=torch.float32, device=ids_a.device)
    lib.call("d2s_mask_agreement", lib.ptr(ids_a) if k else None, lib.ptr(ids_b) if k else None, B, T, k, lib.ptr(out))
    return out


def act_grad(g, z, kind):
    """g * act'(z) (kind 'gelu': z = pre-activation; 'relu': z = ReLU output)."""
    out = torch.empty_like(g)
    lib.call("d2s_act_grad", lib.ptr(g), lib.ptr(z), lib.ptr(out), g.numel(), 0 if kind == "gelu" else 1)
    return out


def normal_noise(shape, seed, device):
    """Standard-normal tensor from the library's counter-based stream `seed` (no torch RNG, no host copy)."""
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    lib.call("d2s_normal_noise", lib.ptr(out), out.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF)
    return out


# ---- DynamicViT baseline (vit_models/default_dynamic_vit.py) ----
def gumbel_noise(shape, seed, device):
    """Gumbel(0, 1) tensor from the library's counter-based stream `seed` (the noise of F.gumbel_softmax)."""
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    lib.call("d2s_gumbel_noise", lib.ptr(out), out.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF)
    return out


def gumbel_from_bits(bits):
    """bits: int32 tensor holding 32-bit draws -> the Gumbel numbers gumbel_noise makes of them (the conversion alone)"""
    assert bits.dtype == torch.int32 and bits.is_contiguous()
    out = torch.empty(bits.shape, dtype=torch.float32, device=bits.device)
    lib.call("d2s_gumbel_from_bits", lib.ptr(bits), lib.ptr(out), bits.numel())
    return out


def gumbel_keep_fwd(z, g, prev):
    """z, g [M, 2], prev [M] -> (logp [M, 2], y0, hard, decision [M])"""
    _f32(z), _f32(g), _f32(prev)
    M = z.shape[0]
    logp = torch.empty_like(z)
    y0, hard, dec = (torch.empty((M,), dtype=torch.float32, device=z.device) for _ in range(3))
    lib.call("d2s_gumbel_keep_fwd", lib.ptr(z), lib.ptr(g), lib.ptr(prev), lib.ptr(logp), lib.ptr(y0), lib.ptr(hard), lib.ptr(dec), M)
    return logp, y0, hard, dec


def gumbel_keep_bwd(gd, prev, y0, hard):
    """-> (dz [M, 2] w.r.t. the raw logits, dprev [M])"""
    M = gd.numel()
    dz = torch.empty((M, 2), dtype=torch.float32, device=gd.device)
    dprev = torch.empty((M,), dtype=torch.float32, device=gd.device)
    lib.call("d2s_gumbel_keep_bwd", lib.ptr(_f32(gd)), lib.ptr(prev), lib.ptr(y0), lib.ptr(hard), lib.ptr(dz), lib.ptr(dprev), M)
    return dz, dprev


def policy_pool_fwd(x, p, B, N, C):
    """x [B*N, C], p [B, N] -> (out [B*N, C], psum [B], glob [B, C/2])"""
    _f32(x), _f32(p)
    out = torch.empty_like(x)
    psum = torch.empty((B,), dtype=torch.float32, device=x.device)
    glob = torch.empty((B, C // 2), dtype=torch.float32, device=x.device)
    lib.call("d2s_policy_pool_fwd", lib.ptr(x), lib.ptr(p), lib.ptr(out), lib.ptr(psum), lib.ptr(glob), B, N, C)
    return out, psum, glob


def policy_pool_bwd(gout, x, p, psum, glob, B, N, C):
    """-> (dx [B*N, C], dp [B, N])"""
    dx = torch.empty_like(x)
    dp = torch.empty((B, N), dtype=torch.float32, device=x.device)
    ws = torch.empty((B, C // 2), dtype=torch.float32, device=x.device)
    lib.call("d2s_policy_pool_bwd", lib.ptr(_f32(gout)), lib.ptr(x), lib.ptr(p), lib.ptr(psum), lib.ptr(glob), lib.ptr(dx), lib.ptr(dp),
             lib.ptr(ws), B, N, C)
    return dx, dp


def ratio_rows_fwd(d, rho):
    """d [B, N] keep decisions -> (loss_row [B] = (mean_j d - rho)^2, diff [B] = mean_j d - rho)"""
    B, N = d.shape
    loss_row = torch.empty((B,), dtype=torch.float32, device=d.device)
    diff = torch.empty((B,), dtype=torch.float32, device=d.device)
    lib.call("d2s_ratio_rows_fwd", lib.ptr(_f32(d)), float(rho), lib.ptr(loss_row), lib.ptr(diff), B, N)
    return loss_row, diff


def ratio_rows_bwd(diff, g, scale, N):
    """-> grad [B, N] = g * scale * 2 diff[b] / N (g: 0-d device tensor)"""
    B = diff.numel()
    grad = torch.empty((B, N), dtype=torch.float32, device=diff.device)
    lib.call("d2s_ratio_rows_bwd", lib.ptr(diff), lib.ptr(_f32(g)), float(scale), lib.ptr(grad), B, N)
    return grad


def perturbed_topk_fwd(x, noise, k, sigma):
    b, d = x.shape
    nS = noise.shape[1]
    ind = torch.empty((b, k, d), dtype=torch.float32, device=x.device)
    need = lib.query("d2s_perturbed_topk_workspace_bytes", b, k, d)
    ws = workspace(need, x.device)
    lib.call("d2s_perturbed_topk_fwd", lib.ptr(x), lib.ptr(noise), lib.ptr(ind), b, nS, d, k, float(sigma), lib.ptr(ws), ws.numel())
    return ind


def perturbed_topk_bwd(x, noise, g, k, sigma):
    b, d = x.shape
    nS = noise.shape[1]
    gx = torch.empty((b, d), dtype=torch.float32, device=x.device)
    lib.call("d2s_perturbed_topk_bwd", lib.ptr(x), lib.ptr(noise), lib.ptr(g), lib.ptr(gx), b, nS, d, k, float(sigma))
    return gx


def soft_gather_fwd(x, ind):
    """x [B,n,D], ind [B,k,n-1] -> y [B,k+1,D]: y[:,0] = x[:,0], y[:,1:] = ind @ x[:,1:] (dynamic_vit.py:896-900); always exact fp32"""
    _f32(x)
    _f32(ind)
    B, n, D = x.shape
    k = ind.shape[1]
    assert ind.shape == (B, k, n - 1), f"indicators must be [B, k, n - 1] = [{B}, k, {n - 1}]"
    y = torch.empty((B, k + 1, D), dtype=torch.float32, device=x.device)
    lib.call("d2s_soft_gather_fwd", lib.ptr(x), lib.ptr(ind), lib.ptr(y), B, n, k, D)
    return y


def soft_gather_bwd_x(g, ind, n):
    """g [B,k+1,D], ind [B,k,n-1] -> dx [B,n,D]: dx[:,0] = g[:,0], dx[:,1:] = ind^T @ g[:,1:]"""
    _f32(g)
    _f32(ind)
    B, k1, D = g.shape
    assert ind.shape == (B, k1 - 1, n - 1)
    dx = torch.empty((B, n, D), dtype=torch.float32, device=g.device)
    lib.call("d2s_soft_gather_bwd_x", lib.ptr(g), lib.ptr(ind), lib.ptr(dx), B, n, k1 - 1, D)
    return dx


def soft_gather_bwd_ind(g, x):
    """g [B,k+1,D], x [B,n,D] -> dind [B,k,n-1] = g[:,1:] @ x[:,1:]^T"""
    _f32(g)
    _f32(x)
    B, k1, D = g.shape
    n = x.shape[1]
    assert x.shape == (B, n, D)
    dind = torch.empty((B, k1 - 1, n - 1), dtype=torch.float32, device=g.device)
    lib.call("d2s_soft_gather_bwd_ind", lib.ptr(g), lib.ptr(x), lib.ptr(dind), B, n, k1 - 1, D)
    return dind


def softmax_rows_bwd(probs, gprobs):
    _f32(probs)
    _f32(gprobs)
    R, T = probs.shape
    assert gprobs.shape == probs.shape
    out = torch.empty_like(probs)
    lib.call("d2s_softmax_rows_bwd", lib.ptr(probs), lib.ptr(gprobs), lib.ptr(out), R, T)
    return out


def adamw_step(params, grads, exp_avg, exp_avg_sq, desc, n_chunks, beta1, beta2, eps, step, grad_scale=1.0, chunk_steps=None):
    """chunk_steps: int32 [n_chunks] per-tensor update counters (torch.optim.AdamW's state['step']), advanced in place."""
    assert chunk_steps is None or (chunk_steps.dtype == torch.int32 and chunk_steps.numel() == n_chunks)
    lib.call("d2s_adamw_step", lib.ptr(params), lib.ptr(grads), lib.ptr(exp_avg), lib.ptr(exp_avg_sq), lib.ptr(desc), n_chunks,
             float(beta1), float(beta2), float(eps), int(step), float(grad_scale), lib.ptr(chunk_steps))


def adamw_step_ema(params, grads, exp_avg, exp_avg_sq, desc, n_chunks, beta1, beta2, eps, step, ema, ema_decay, grad_scale=1.0,
                   chunk_steps=None):
    """adamw_step, and in the same launch ema = ema_decay * ema + (1 - ema_decay) * params (every chunk, the inactive ones included)."""
    assert chunk_steps is None or (chunk_steps.dtype == torch.int32 and chunk_steps.numel() == n_chunks)
    assert ema.dtype == torch.float32 and ema.numel() == params.numel() and ema.data_ptr() != params.data_ptr()
    lib.call("d2s_adamw_step_ema", lib.ptr(params), lib.ptr(grads), lib.ptr(exp_avg), lib.ptr(exp_avg_sq), lib.ptr(desc), n_chunks,
             float(beta1), float(beta2), float(eps), int(step), float(grad_scale), lib.ptr(chunk_steps), lib.ptr(ema), float(ema_decay))


def adamw_step_clip(params, grads, exp_avg, exp_avg_sq, desc, n_chunks, beta1, beta2, eps, step, coef, ema=None, ema_decay=0.0,
                    grad_scale=1.0, chunk_steps=None):
    """adamw_step (ema None) or adamw_step_ema with the gradient scale fl(grad_scale * coef[0]); coef: device float (grad_clip_coef)."""
    assert chunk_steps is None or (chunk_steps.dtype == torch.int32 and chunk_steps.numel() == n_chunks)
    assert coef.dtype == torch.float32 and coef.numel() >= 1
    assert ema is None or (ema.dtype == torch.float32 and ema.numel() == params.numel() and ema.data_ptr() != params.data_ptr())
    lib.call("d2s_adamw_step_clip", lib.ptr(params), lib.ptr(grads), lib.ptr(exp_avg), lib.ptr(exp_avg_sq), lib.ptr(desc), n_chunks,
             float(beta1), float(beta2), float(eps), int(step), float(grad_scale), lib.ptr(chunk_steps), lib.ptr(ema), float(ema_decay),
             lib.ptr(coef))


def grad_accumulate(acc, g, desc, n_chunks, mode):
    """Active chunks only.  mode 0: acc = g; 1: acc = fl(acc + g); 2: g = fl(acc + g)."""
    _f32(acc)
    _f32(g)
    chunk = lib.query("d2s_adamw_chunk_elems")
    assert acc.numel() == g.numel() == n_chunks * chunk and acc.is_contiguous() and g.is_contiguous()
    lib.call("d2s_grad_accumulate", lib.ptr(acc), lib.ptr(g), lib.ptr(desc), n_chunks, int(mode))


def grad_clip_coef(g, desc, n_chunks, scale, max_norm, partials, out):
    """out[0] = scale * ||g||_2 over the active chunks, out[1] = min(1, max_norm / (out[0] + 1e-6)); partials: n_chunks floats of scratch."""
    _f32(g)
    assert g.numel() == n_chunks * lib.query("d2s_adamw_chunk_elems") and g.is_contiguous()
    assert partials.dtype == torch.float32 and partials.numel() >= n_chunks and out.dtype == torch.float32 and out.numel() >= 2
    lib.call("d2s_grad_clip_coef", lib.ptr(g), lib.ptr(desc), n_chunks, float(scale), float(max_norm), lib.ptr(partials), lib.ptr(out))


# ---- gradient-arena routing: the slice of a flat gradient arena that the gradient of a parameter is written into.  The record lives
# ON the Parameter object (not in a table keyed by its address), so it dies with the parameter, an arena is freed as soon as its model
# and TrainStep are, and a recycled device address can never alias a stale entry. ----
_GRAD_ATTR = "_d2s_grad_slice"


def register_grad_buffer(param, grad_view):
    """Route the gradient of `param` into `grad_view` (a slice of a flat gradient arena, see d2s.engine.ParamArena)."""
    base = grad_view._base if grad_view._base is not None else grad_view
    setattr(param, _GRAD_ATTR, (base, grad_view.storage_offset(), grad_view.numel(), tuple(grad_view.shape)))


def unregister_grad_buffer(param):
    if hasattr(param, _GRAD_ATTR):
        delattr(param, _GRAD_ATTR)


def grad_buffer(param):
    """Tensor to write the gradient of `param` into: a FRESH view of its arena slice when registered (a fresh tensor
    object lets autograd's AccumulateGrad adopt it without a copy), otherwise a new tensor."""
    ent = getattr(param, _GRAD_ATTR, None)
    if ent is None:
        return torch.empty_like(param)
    base, off, numel, shape = ent
    if shape != tuple(param.shape) or base.device != param.device:
        raise lib.D2SError("parameter was reshaped / moved after its gradient arena was built (rebuild the TrainStep)")
    return base.view(-1)[off:off + numel].view(shape)


GEMM_EXACT, GEMM_SPLIT, GEMM_BF16 = 0, 1, 2

# Arithmetic mode of the GEMM / attention calls.  The C ABI takes it per call (no state in the library); this module keeps the
# process default plus a per-thread override stack so that one module (e.g. the frozen teacher) can run in another mode than the
# rest.  Autograd Functions record the mode of their forward and re-enter it in their backward (d2s.functional.mode_recorded),
# because backward runs on autograd's own thread, outside any `with gemm_mode(...)` block of the caller.
_default_mode = GEMM_EXACT
_tls = threading.local()


def set_gemm_mode(mode):
    """Process default: 0 exact fp32 MFMA (bit-for-bit an fp32 fma chain); 1 bf16x3 split on the bf16 matrix cores (fp32-class
    accuracy); 2 bf16 operands with fp32 accumulation (forward, dgrad and - in this mode only - wgrad GEMMs, bf16 attention)."""
    global _default_mode
    mode = int(mode)
    if mode not in (GEMM_EXACT, GEMM_SPLIT, GEMM_BF16):
        raise ValueError(f"gemm mode {mode}")
    _default_mode = mode


def get_gemm_mode():
    stack = getattr(_tls, "stack", None)
    return stack[-1] if stack else _default_mode


class gemm_mode:
    """with ops.gemm_mode(ops.GEMM_BF16): ...   - overrides the process default for the calls of this thread inside the block."""

    def __init__(self, mode):
        self.mode = int(mode)
        if self.mode not in (GEMM_EXACT, GEMM_SPLIT, GEMM_BF16):
            raise ValueError(f"gemm mode {mode}")

    def __enter__(self):
        if not hasattr(_tls, "stack"):
            _tls.stack = []
        _tls.stack.append(self.mode)
        return self

    def __exit__(self, *exc):
        _tls.stack.pop()
        return False


# ---- input pipeline (csrc/augment.hip; d2s/data.py packs the batch) ------------------------------------------------------------------
AUG_DESC_INTS = 64        # == d2s_augment_desc_ints(), checked by augment_images
RA_MAX_OPS, RA_OP_INTS = 8, 16      # == d2s_randaug_max_ops(), d2s_randaug_op_ints(): the op table is [B, RA_MAX_OPS, RA_OP_INTS] int32


def _check_op_table(table, B):
    if lib.query("d2s_randaug_max_ops") != RA_MAX_OPS or lib.query("d2s_randaug_op_ints") != RA_OP_INTS:
        raise lib.D2SError("op table layout of the library and of d2s.ops disagree")
    assert table.dtype == torch.int32 and table.is_contiguous() and table.shape == (B, RA_MAX_OPS, RA_OP_INTS), table.shape


def augment_images(pix, desc, meta, size, op_table=None):
    """Crop + resize (Pillow-exact) + flip + Normalize + RandomErasing + Mixup / CutMix of a packed batch, on the current stream.
    pix: uint8 device buffer (a multiple of 16 bytes), desc: [B, AUG_DESC_INTS] int32 device descriptors, meta: the host maxima written
    by d2s.data.pack_batch.  op_table: None, or the [B, RA_MAX_OPS, RA_OP_INTS] int32 device table of RandAugment / ColorJitter ops
    (d2s.data.pack_ops), applied to the uint8 image between the flip and ToTensor.  Returns fp32 [B, 3, size, size].  The scratch and
    the output are allocated on the current stream."""
    if lib.query("d2s_augment_desc_ints") != AUG_DESC_INTS:
        raise lib.D2SError("augment descriptor layout of the library and of d2s.ops disagree")
    assert pix.dtype == torch.uint8 and pix.is_contiguous() and desc.dtype == torch.int32 and desc.is_contiguous()
    B = desc.shape[0]
    assert desc.shape == (B, AUG_DESC_INTS), desc.shape
    inter = torch.empty(max(int(meta["total_rows"]) * size * 3, 16), dtype=torch.uint8, device=pix.device)
    out = torch.empty((B, 3, size, size), dtype=torch.float32, device=pix.device)
    args = (B, int(size), int(meta["max_rows"]), int(meta["kmax_h"]), int(meta["kmax_v"]), int(meta["rowbytes"]),
            int(meta["seed"]) & 0xFFFFFFFFFFFFFFFF, lib.ptr(inter))
    if op_table is None:
        name = "d2s_augment_images"
        rc = lib._fn(name)(lib.ptr(pix), pix.numel(), lib.ptr(desc), *args, lib.ptr(out), lib.stream())
    else:
        name = "d2s_augment_images_ops"
        _check_op_table(op_table, B)
        images = torch.empty(lib.query("d2s_augment_ops_scratch_bytes", B, int(size)), dtype=torch.uint8, device=pix.device)
        rc = lib._fn(name)(lib.ptr(pix), pix.numel(), lib.ptr(desc), lib.ptr(op_table), *args, lib.ptr(images), lib.ptr(out), lib.stream())
    if rc != 0:
        raise lib.D2SError(f"{name} failed with code {rc} (a crop more than ~40x the output size does not fit the "
                           "coefficient tables)" if rc == -1 else f"{name} failed with code {rc}")
    return out


def randaug_apply(images, op_table):
    """RandAugment / ColorJitter ops on uint8 [B, S, S, 3] device images, bit-exact with Pillow (csrc/randaug.hip): image b's list
    op_table[b] (d2s.data.pack_ops) applied in order.  Returns a new uint8 [B, S, S, 3]; the input is not written."""
    assert images.dtype == torch.uint8 and images.is_contiguous() and images.dim() == 4 and images.shape[3] == 3, images.shape
    B, S = images.shape[0], images.shape[1]
    assert images.shape[2] == S, images.shape
    _check_op_table(op_table, B)
    scratch = torch.empty(lib.query("d2s_randaug_scratch_bytes", B, S), dtype=torch.uint8, device=images.device)
    out = torch.empty_like(images)
    lib.call("d2s_randaug_apply", lib.ptr(images), lib.ptr(op_table), B, S, lib.ptr(scratch), lib.ptr(out))
    return out


def augment_labels(desc, num_classes, smoothing):
    """timm's mixup_target from the per-sample (label, lam) of the descriptors: fp32 [B, num_classes]."""
    B = desc.shape[0]
    off = smoothing / num_classes                  # in double, then rounded to fp32 by the kernel argument, as torch.full does
    on = 1. - smoothing + off
    out = torch.empty((B, num_classes), dtype=torch.float32, device=desc.device)
    lib.call("d2s_augment_labels", lib.ptr(desc), B, int(num_classes), on, off, lib.ptr(out))
    return out
