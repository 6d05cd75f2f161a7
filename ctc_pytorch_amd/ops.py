"""autograd wrappers around the C ABI of libctcn.so.

Every function here enqueues hand-written gfx950 kernels on torch's current HIP stream; PyTorch is used
for device memory, autograd bookkeeping and nothing else.  Tensors must live on a ROCm device -- a CPU
tensor raises (the product has no CPU path; the CPU restatement lives in oracle/ and is test-only).
"""
import collections
import ctypes
import os
import numpy as np

import torch

from . import _lib
from ._lib import _need_gpu, _ptr

CELL = {"lstm": 0, "gru": 1, "tanh": 2}
GATES = {0: 4, 1: 3, 2: 1}

# process-wide numeric mode of the MFMA GEMMs: 0 = exact f32 MFMA, 1 = bf16x3 split-operand MFMA (f32-class accuracy, the
# default: it is the mode every headline number is measured in).  Environment CTCN_PRECISION=0|1 picks the start value.
# A plain module global on purpose: autograd runs backward() on its own worker threads.
def _precision_from_env():
    v = os.environ.get("CTCN_PRECISION", "1").strip()
    if v not in ("0", "1"):
        raise ValueError("CTCN_PRECISION must be 0 (exact f32 MFMA) or 1 (bf16x3 split-operand MFMA), got %r" % v)
    return int(v)


DEFAULT_PRECISION = _precision_from_env()
_precision = [DEFAULT_PRECISION]


def set_precision(p):
    if int(p) not in (0, 1):
        raise ValueError("precision must be 0 (f32 MFMA) or 1 (bf16x3 split-operand MFMA)")
    _precision[0] = int(p)


def get_precision():
    return _precision[0]


def _f32c(t):
    """float32 + contiguous, materialising strided views with the library's own gather kernel."""
    if t.dtype != torch.float32:
        raise TypeError("ctc_pytorch_amd: expected float32, got %s" % t.dtype)
    return t if t.is_contiguous() else contiguous(t)


def _gview(p):
    """Flat-gradient view registered by optim.FlatAdam (backward kernels accumulate into it, beta=1)."""
    return getattr(p, "_ctcn_grad", None) if p is not None else None


def set_rnn_persistent(flag):
    """1: persistent recurrent kernels (default); 0: one launch per timestep (ctcn_set_option)."""
    _lib.check(_lib.lib().ctcn_set_option(b"rnn_persistent", int(bool(flag))), "set_option")


def set_option(name, value):
    """Raw ctcn_set_option (see include/ctcn.h for the option names)."""
    _lib.check(_lib.lib().ctcn_set_option(name.encode(), int(value)), "set_option")


def get_option(name):
    """Raw ctcn_get_option."""
    return int(_lib.lib().ctcn_get_option(name.encode()))


def option_names():
    """Every name ctcn_set_option knows (ctcn_option_name, include/ctcn.h)."""
    L, out, i = _lib.lib(), [], 0
    while True:
        n = L.ctcn_option_name(i)
        if n is None:
            return out
        out.append(n.decode())
        i += 1


def state_snapshot():
    """Everything process-wide that can change what a later call computes or which kernels it launches -- the library's option table and the
    module-level state of this layer: a dict of plain values, comparable with ==.  tests/conftest.py takes one
    before and after every GPU test, asserts that the configuration part is left as found and puts the learnt part (`fallback_shapes`,
    `drop_counter`) back; tools/soak.py and tools/squat_stress.py print it next to a trajectory."""
    from . import parallel
    return {
        "options": {n: get_option(n) for n in option_names()},
        "precision": get_precision(),
        "fallback_shapes": sorted(_fallback_shapes),
        "drop_counter": _drop_counter[0],
        "chunks_on": _chunks_on[0],
        "fuse_bn_dropout": _fuse_bn_dropout[0],
        "side": {k: _side[k] for k in ("fwd_overlap", "enabled", "min_items", "min_items_bwd")},
        "small_split_max_items": SMALL_SPLIT_MAX_ITEMS,
        "grad_ready_hook": _grad_ready["hook"] is not None,
        "sync_bn": _sync_bn["reduce"] is not None,
        "batch_split": (parallel._batch["global"], parallel._batch["local"]),
        "overlap_pending": len(parallel._overlap["works"]) + len(parallel._overlap["events"]),
    }


LEARNT_STATE = ("fallback_shapes", "drop_counter")


def restore_learnt_state(snap):
    """Put back the part of `state_snapshot` a call may legitimately move (shapes learnt to need batch chunks, the dropout stream position)."""
    _fallback_shapes.clear()
    _fallback_shapes.update(tuple(k) for k in snap["fallback_shapes"])
    _drop_counter[0] = snap["drop_counter"]


def restore_state(snap):
    """Everything `state_snapshot` lists, put back (hooks can only be cleared, not re-created: a snapshot records whether one was set)."""
    from . import parallel
    restore_learnt_state(snap)
    for n, v in snap["options"].items():
        if get_option(n) != v:
            set_option(n, v)
    set_precision(snap["precision"])
    _chunks_on[0], _fuse_bn_dropout[0] = snap["chunks_on"], snap["fuse_bn_dropout"]
    for k, v in snap["side"].items():
        _side[k] = v
    if not snap["grad_ready_hook"]:
        parallel.enable_overlap(False)
    if not snap["sync_bn"]:
        _sync_bn["reduce"] = None
    parallel._batch["global"], parallel._batch["local"] = snap["batch_split"]
    parallel._overlap["works"], parallel._overlap["done"], parallel._overlap["events"] = [], [], []


_kernel_counts = {}
_debug_note = [None]          # development: callable(tag, addresses, tensors) invoked by _RNNLayer.forward (tools/squat_stress.py installs it while tracing)


def kernel_counts(reset=False):
    """How often each recurrence kernel was launched by this process's layer calls since the last reset: {'rnn_fwd_tagged': n, 'rnn_bwd_step': m, ...}
    (what bench.py's ragged-epoch leg reports: a shape that falls off the persistent path shows up as rnn_fwd_step / rnn_bwd_step)."""
    out = dict(_kernel_counts)
    if reset:
        _kernel_counts.clear()
    return out


def _count_kernel(name):
    k = (name or b"?").decode() if isinstance(name, (bytes, bytearray)) or name is None else str(name)
    _kernel_counts[k] = _kernel_counts.get(k, 0) + 1


def rnn_last_kernels():
    """(forward, backward) names of the recurrent kernels the library launched last (ctcn_rnn_last_kernel)."""
    L = _lib.lib()
    return (L.ctcn_rnn_last_kernel(0) or b"").decode(), (L.ctcn_rnn_last_kernel(1) or b"").decode()


def diag_squat(wgs_per_xcd, usec, threads=256, lds_bytes=0, stream=None):
    """Diagnostics: occupy `wgs_per_xcd` workgroups on every XCD for `usec` microseconds on `stream` (default: the current one) --
    the footprint of an RCCL kernel waiting for a slow peer (ctcn_diag_squat)."""
    st = stream.cuda_stream if stream is not None else _lib.stream_ptr()
    _lib.check(_lib.lib().ctcn_diag_squat(int(wgs_per_xcd), int(threads), int(lds_bytes), int(usec), ctypes.c_void_p(st)), "diag_squat")


def check_health(device=None):
    """Synchronising check of the sticky status word written by persistent kernels on a hand-off timeout."""
    _lib.check_status(torch.device("cuda", torch.cuda.current_device()) if device is None else device)


def _ws(t, tag="main"):
    _lib.status_word(t.device)
    w = _lib.workspace(t.device, tag=tag)
    return w, ctypes.c_void_p(w.data_ptr()), w.numel()


# --------------------------------------------------------------------------------------------------
# weight-gradient side stream
# --------------------------------------------------------------------------------------------------
# The weight gradients of a recurrent layer (dW_ih = da^T x, dW_hh = da^T h_prev) have no consumer inside the backward
# pass, while the next layer's persistent recurrence is a latency-bound kernel that occupies only
# dirs * ceil(B/16) of the 8 XCDs.  When the gradients go to a flat buffer (optim.FlatAdam) they are therefore issued on
# a second stream, restricted (ctcn_rnn_bwd_weights' xcd_allow) to the XCDs the recurrence leaves idle, and joined to the
# main stream when autograd finishes the backward pass.
# The side work of a layer is DEFERRED until the next recurrence below it is about to be launched (or until a join): issued
# straight away it competes with the critical-path kernels that sit between two recurrences (the input-gradient GEMMs, the
# BatchNorm / dropout backward), which measured 1.5-10x their stand-alone time in that window; behind the deferral they
# have the chip to themselves and the side work overlaps with nothing but the recurrence, on the XCDs it leaves idle.
# Data parallel overlap: `_grad_ready["hook"]` (parallel.enable_overlap) is called on the side stream right after the weight-gradient
# GEMMs of a recurrent layer were enqueued there, with the flat-buffer views they accumulate into: the all-reduce of that slice
# then runs next to the rest of the backward pass instead of after it.
_grad_ready = {"hook": None}


_XCD_ORDERS = ((0, 1, 2, 3, 4, 5, 6, 7), (0, 2, 4, 6, 1, 3, 5, 7), (0, 1, 4, 5, 2, 3, 6, 7), (0, 3, 4, 7, 1, 2, 5, 6), (0, 2, 5, 7, 1, 3, 4, 6), (0, 4, 1, 5, 2, 6, 3, 7))


def _idle_xcd_mask(nx, groups):
    """Physical XCDs a persistent recurrence of `groups` (direction, batch tile) groups leaves idle: group g runs on logical XCD g, which is
    physical XCD _XCD_ORDERS[option "xcd_interleave"][g] on a device of eight (rnn.hip: persist_role)."""
    if nx == 8:
        order = _XCD_ORDERS[min(max(get_option("xcd_interleave"), 0), 5)]
        return sum(1 << order[g] for g in range(min(groups, nx), nx))
    return ((1 << nx) - 1) & ~((1 << groups) - 1)


def set_grad_ready_hook(fn):
    _grad_ready["hook"] = fn


def _env_on(name):
    return os.environ.get(name, "1") != "0"


SIDE_MIN_ITEMS_FWD, SIDE_MIN_ITEMS_BWD = 1 << 21, 1 << 18
SMALL_SPLIT_MAX_ITEMS = 1 << 23       # T*B*H above which an inline layer's two directions stay on one stream (their GEMMs fill the device one at a time)
# the settings of the side stream (set_side_stream, set_fwd_overlap; the per-device runtime state is _DeviceSide)
_side = {"fwd_overlap": _env_on("CTCN_FWD_OVERLAP"), "enabled": _env_on("CTCN_SIDE_STREAM"),
         "min_items": int(os.environ.get("CTCN_SIDE_MIN_ITEMS", SIDE_MIN_ITEMS_FWD)),
         "min_items_bwd": int(os.environ.get("CTCN_SIDE_MIN_ITEMS_BWD", os.environ.get("CTCN_SIDE_MIN_ITEMS", SIDE_MIN_ITEMS_BWD))),
         "small_split": _env_on("CTCN_SMALL_SPLIT"),
         "capacity_slack": float(os.environ.get("CTCN_SIDE_CAPACITY_SLACK", "1.0"))}      # > 1: the weight-gradient side stream also where the rule says it cannot keep up (experiments)


def set_side_stream(flag, min_items=None, min_items_bwd=None):
    """Enable / disable the side stream (default on; env CTCN_SIDE_STREAM=0 disables).  Two size thresholds on T*B*H of a recurrent layer:
    `min_items` (default 2^21, env CTCN_SIDE_MIN_ITEMS) for the input projection pipelined with the forward recurrence, `min_items_bwd`
    (default 2^18, env CTCN_SIDE_MIN_ITEMS_BWD) for the weight-gradient GEMMs next to the recurrence of the layer below.  Passing
    `min_items` alone sets BOTH (what the tests that force everything onto / off the side stream do).  Round 4: the two used to share
    2^21, which kept the shipped-YAML shape (4 x 384, B = 8, 200 steps: 614 k items) inline -- 110 us of launch-bound weight GEMMs per
    layer in front of a 350-us recurrence that leaves six XCDs idle: 4.69 -> 4.36 ms per step with the lower threshold (cfg1 2.02 -> 1.95),
    while the forward pipeline at that size costs more than it hides (5.74 ms)."""
    _side["enabled"] = bool(flag)
    if min_items is not None:
        _side["min_items"] = int(min_items)
        _side["min_items_bwd"] = int(min_items)
    if min_items_bwd is not None:
        _side["min_items_bwd"] = int(min_items_bwd)


def set_fwd_overlap(flag):
    """Pipeline the input projection of a recurrent layer with its persistent forward recurrence (ctcn_rnn_call.side_stream of ctcn_rnn_fwd_ex); default on
    (environment: CTCN_FWD_OVERLAP=0 turns it off)."""
    _side["fwd_overlap"] = bool(flag)


def _tiles16(n):
    """16-row batch tiles of a batch / 16-unit slices (one workgroup, one CU each) of a hidden size."""
    return (n + 15) // 16


def _recurrence_xcds(B, dirs, nx):
    """(groups, idle): the (direction, 16-row batch tile) groups of a persistent recurrence, one XCD each while XCDs last, and the mask of the
    XCDs it leaves idle (0: none, or a device without XCDs to split)."""
    groups = dirs * _tiles16(B)
    return groups, (_idle_xcd_mask(nx, groups) if nx > 1 else 0)


def side_stream_plan(cell, T, B, I, H, dirs, nx, cus, slack=1.0):
    """Where can the weight-gradient GEMMs (dW_ih, dW_hh) of a layer run while the recurrence of the layer below occupies its XCDs?  Returns
    the XCD mask for ctcn_rnn_bwd_weights' xcd_allow, 0 = nowhere (inline on the main stream).  Pure arithmetic (round 4; every constant from a
    measured loss or gain, ms per training step of cfg2's model with | without the side stream):
    * idle XCDs (groups = dirs x batch tiles < XCDs): the mask of the idle ones, if they can digest the GEMMs within the recurrence -- the
      flops at ~300 TFLOP/s of the whole chip, scaled to the idle share, against 0.9 x T backward steps of 1.2 + H / 400 us (~1.5 / 2.0 / 2.5
      us at H = 128 / 320 / 512): B = 32: 13.2 | 15.0, B = 16: 12.0 | 12.6; with 3 batch tiles (two idle XCDs) the side stream fell further
      behind with every layer and the step waited for it at the end: B = 48: 17.9 | 17.2 -> inline -- and if the recurrence leaves CUs free
      on ITS XCDs: the GEMMs' workgroups dealt to a recurrence XCD must start there to find out that they are on the wrong XCD and leave; with
      every CU taken (H = 512: 32 slices) they wait for the recurrence to end, and the in-order dispatcher with them (B = 32: 41.2 | 40.2);
    * NO idle XCD, but at least eight free CUs next to the recurrence on every XCD (B = 64 with H <= 256: 16 + 2 of 32 CUs taken): all XCDs,
      unfiltered -- the GEMMs share the recurrence's XCDs and L2s -- with the same capacity test on the free CUs' share of the chip:
      B = 64 at H = 256: 14.97 | 16.36, at H = 128: 11.39 | 11.92.  (Unfiltered although XCDs ARE idle -- more CUs, shared L2s -- measured
      worse: cfg2 13.31 | filtered 13.22, the shipped-YAML shape 4.37 | 4.35.)"""
    if nx <= 1:
        return 0
    groups, idle = _recurrence_xcds(B, dirs, nx)
    per = cus // nx
    wpx = ((groups + nx - 1) // nx) * _tiles16(H)
    used = wpx + max(2, wpx // 8)
    if groups < nx:
        if used + 2 > per:
            return 0
        share, allow = (nx - groups) / float(nx), idle
    else:
        if per - used < 8:
            return 0
        share, allow = (per - used) / float(per), (1 << nx) - 1
    side_us = 2.0 * T * B * (dirs * GATES[cell] * H) * (I + H) / (300e6 * share)
    return allow if side_us <= 0.9 * T * (1.2 + H / 400.0) * slack else 0


def side_stream_fits(cell, T, B, I, H, dirs, nx, cus, slack=1.0):
    return side_stream_plan(cell, T, B, I, H, dirs, nx, cus, slack) != 0


def plan_fwd_pipeline(T, B, H, dirs, nx, settings=None):
    """The forward's decision, pure: the XCD mask (ctcn_rnn_call.xcd_allow) for the pipelined input projection -- only the first pair of time
    chunks is projected before the recurrence starts, the rest on the side stream, on the XCDs the persistent kernel leaves idle (group g =
    (direction, 16-row batch tile) runs on XCD g) -- or 0: the whole projection in front of the recurrence, on the main stream."""
    s = _side if settings is None else settings
    idle = _recurrence_xcds(B, dirs, nx)[1]
    return idle if s["enabled"] and s["fwd_overlap"] and dirs == 2 and T * B * H >= s["min_items"] else 0


# where the weight-gradient GEMMs of one layer call run (plan_weight_grads)
WG_INLINE = "inline"                  # dW pointers go into ctcn_rnn_bwd_ex, main stream
WG_DEFERRED = "deferred side"         # one ctcn_rnn_bwd_weights(xcd_allow = mask) on the side stream, parked until the layer below launches its recurrence
WG_SPLIT_END = "split, joined at end of backward"     # direction 1 on the side stream, direction 0 on main; joined by the engine callback
WG_SPLIT_NOW = "split, joined at once"                # the same two calls, the main stream waits straight away


def plan_weight_grads(cell, T, B, I, H, dirs, nx, cus, into_flat, chunk, bottom, above_parked, settings=None):
    """The backward's decision, pure: (mode, xcd_allow) for the weight gradients of one layer call.  into_flat: all of them accumulate into
    optim.FlatAdam's flat buffer; chunk: the call is one of several batch chunks of a layer (rnn_layer); bottom: no recurrence follows in this
    backward pass; above_parked: the layer above has deferred work waiting for this layer's recurrence."""
    s = _side if settings is None else settings
    items = T * B * H
    # one of several batch chunks: every chunk accumulates (beta = 1, read-modify-write) into the SAME gradient views, so all of them write on
    # the main stream, in order -- a chunk whose weight GEMMs were deferred to the side stream would race with a sibling chunk's inline GEMMs
    # on the same buffers (test_rnn_batch_chunks_into_flat_gradients)
    if chunk or not (into_flat and s["enabled"] and T > 1):
        return WG_INLINE, 0
    # very small layers stay off the deferred path (below min_items_bwd = 2^18 (frame, row, unit) items: the test fixtures).  Round 1 measured cfg1
    # slower with the side stream (2.27 ms inline, 2.8-4.5 with it) and set the threshold at 2^21; with the queue-form GEMMs and the deferred issue
    # of rounds 2-3 the picture is the opposite (round 4: cfg1 2.02 -> 1.95 ms, the shipped-YAML shape 4.69 -> 4.36): set_side_stream.
    # Above it: where the GEMMs can run next to the recurrence of the layer below -- idle XCDs, or free CUs on every XCD (side_stream_plan)
    allow = side_stream_plan(cell, T, B, I, H, dirs, nx, cus, s["capacity_slack"]) if nx > 1 and items >= s["min_items_bwd"] else 0
    if allow and not bottom:
        return WG_DEFERRED, allow
    # bottom recurrent layer: no recurrence follows, so its weight GEMMs get the whole device -- one direction per stream
    # (eight small dependent launches per direction that do not fill 256 CUs one at a time: 440 -> ~250 us at cfg2)
    if allow and dirs == 2:
        return WG_SPLIT_END, 0
    # small layers (weight GEMMs not deferred): the two directions' weight gradients are independent chains of small launches that do not
    # fill the device one at a time -- one direction per stream, joined at once (nothing runs next to a recurrence)
    # * not when the layer ABOVE has parked side work: the join waits for the whole side stream, which would then hold that layer's deferred
    #   weight GEMMs -- and its early all-reduce -- in front of the main stream; a mixed large / small stack keeps this layer inline;
    # * not for LARGE layers that stay inline because the capacity rule says the side stream cannot keep up -- cfg4: B = 64, H = 512 --:
    #   their weight GEMMs are full-device queue kernels of 131 KB LDS per workgroup, two of which never share a CU, so the two streams ran
    #   them one after the other anyway; round 5: 52.10 | 51.95 ms per cfg4 step with | without the split, and rocprofv3 charged the wait for
    #   the other stream's GEMM to whatever small kernel came next on this one -- the "650-us split-K reduce" of profiles/r03_cfg4_*
    if s["small_split"] and dirs == 2 and not above_parked and items < SMALL_SPLIT_MAX_ITEMS:
        return WG_SPLIT_NOW, 0
    return WG_INLINE, 0


class _DeviceSide(object):
    """Runtime state of one device's side stream: the stream and the prelaunch event (both created on first use), whether the stream holds
    work the main stream has not joined (`pending`), the weight-gradient work parked until the next recurrence is launched (`deferred`, a
    callable) and the number of recurrent layers whose backward is still to come (`live`: the deferral needs to know whether another
    recurrence will follow in the backward pass)."""

    def __init__(self, dev):
        self.dev, self.stream, self.event, self.pending, self.deferred, self.live = dev, None, None, False, None, 0

    def side_stream(self):
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.dev)
        return self.stream

    def prelaunch_event(self):
        """The event that ctcn_rnn_bwd records right before it launches its recurrence (ctcn_rnn_call.prelaunch_event of ctcn_rnn_bwd_ex)."""
        if self.event is None:
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream(self.dev))        # materialises the hipEvent_t behind ev.cuda_event
        return self.event

    def join(self):
        """Issue the parked weight-gradient work on the side stream, ordered behind everything the main stream holds so far, and make the
        main stream wait for the side stream."""
        fn, self.deferred = self.deferred, None
        if fn is not None:
            fn()
        if self.pending:
            self.pending = False
            torch.cuda.current_stream(self.dev).wait_stream(self.stream)

    def join_at_end(self):
        """End-of-backward callback: join, and forget recurrent layers whose backward never came (a forward pass run with
        gradients enabled but never differentiated would otherwise leave the count of pending recurrences too high)."""
        self.join()
        self.live = 0


_devices = {}


def _device_side(dev):
    key = (dev.type, dev.index)
    d = _devices.get(key)
    if d is None:
        d = _devices[key] = _DeviceSide(dev)
    return d


def join_side_stream(device=None):
    """Make the current stream wait for weight gradients still in flight on the side stream (no-op if none)."""
    for d in (list(_devices.values()) if device is None else [_device_side(device)]):
        d.join()


# --------------------------------------------------------------------------------------------------
# layout
# --------------------------------------------------------------------------------------------------
def _copy_strided(src):
    _need_gpu(src)
    if src.dim() > 4:
        raise NotImplementedError("ctc_pytorch_amd.contiguous: rank %d > 4" % src.dim())
    dims = [1] * (4 - src.dim()) + list(src.shape)
    strides = [0] * (4 - src.dim()) + list(src.stride())
    out = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    if out.numel():
        _lib.check(_lib.lib().ctcn_copy_strided4(_ptr(src), _ptr(out), dims[0], dims[1], dims[2], dims[3], strides[0],
                                                 strides[1], strides[2], strides[3], _lib.stream_ptr()), "copy_strided4")
    return out


class _Contiguous(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _copy_strided(x)

    @staticmethod
    def backward(ctx, g):
        return g


def contiguous(x):
    """x.contiguous() through ctcn_copy_strided4 (model_ctc.py:153,158,175)."""
    if x.is_contiguous():
        return x
    if x.dtype != torch.float32:
        raise TypeError("ctc_pytorch_amd.contiguous: float32 only")
    return _Contiguous.apply(x)


class _BctfToTbcf(torch.autograd.Function):
    """(B,C,T,F) -> (T,B,C*F): transpose(1,2).view(B,T,C*F).transpose(0,1) of model_ctc.py:153-158 in one pass."""

    @staticmethod
    def forward(ctx, x):
        _need_gpu(x)
        x = _f32c(x)
        B, C, T, Fq = x.shape
        ctx.shape = (B, C, T, Fq)
        out = torch.empty((T, B, C * Fq), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().ctcn_bctf_to_tbcf(_ptr(x), _ptr(out), B, C, T, Fq, _lib.stream_ptr()), "bctf_to_tbcf")
        return out

    @staticmethod
    def backward(ctx, g):
        B, C, T, Fq = ctx.shape
        g = _f32c(g)
        out = torch.empty((B, C, T, Fq), dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().ctcn_tbcf_to_bctf(_ptr(g), _ptr(out), B, C, T, Fq, _lib.stream_ptr()), "tbcf_to_bctf")
        return out


def bctf_to_tbcf(x):
    return _BctfToTbcf.apply(x)


# --------------------------------------------------------------------------------------------------
# linear (GEMM)
# --------------------------------------------------------------------------------------------------
def gemm(transA, transB, M, N, K, A, lda, Bm, ldb, C, ldc, beta=0.0, xcd_allow=0):
    """xcd_allow != 0: the side-stream form, workgroups confined to those XCDs (ctcn_diag_gemm_on_xcds; tests)."""
    _need_gpu(A, Bm, C)
    w, wp, wn = _ws(C)
    args = (int(transA), int(transB), M, N, K, _ptr(A), lda, _ptr(Bm), ldb, _ptr(C), ldc, float(beta), get_precision(), wp, wn, _lib.stream_ptr())
    _lib.check(_lib.lib().ctcn_diag_gemm_on_xcds(*args, int(xcd_allow)) if xcd_allow else _lib.lib().ctcn_gemm(*args), "gemm")
    return C


def gemm_shift_b_pair(M, N1, N2, K, A, lda, B1, ldb1, C1, ldc1, A2, B2, ldb2, C2, ldc2, shift, beta=0.0, xcd_allow=0, reuse=False, ws=None):
    """C1 = A^T B1, then C2 = A2^T shift_k(B2) with one plane record, as a recurrent layer's weight gradients run (ctcn_diag_gemm_shift_b_pair;
    tests).  reuse: 1 asks the second product for A's planes of the first, 2 also overwrites A with NaN in between (pass A2 = A).  ws: a uint8
    tensor to use as the workspace instead of the stream's own."""
    _need_gpu(A, B1, C1, A2, B2, C2)
    wp, wn = (_ptr(ws), ws.numel()) if ws is not None else _ws(C1)[1:]
    _lib.check(_lib.lib().ctcn_diag_gemm_shift_b_pair(M, N1, N2, K, _ptr(A), lda, _ptr(B1), ldb1, _ptr(C1), ldc1, _ptr(A2), _ptr(B2), ldb2, _ptr(C2), ldc2,
                                                      float(beta), get_precision(), wp, wn, _lib.stream_ptr(), int(xcd_allow), int(shift), int(reuse)),
               "gemm_shift_b_pair")
    return C1, C2


def gemm_dx(M, N, K, A, lda, Bm, ldb, C, ldc, beta=0.0):
    """C = A B for a row-major A (M x K) and a row-major B (K x N) through ctcn_gemm_dx, the entry of a recurrent layer's dx product (tests)."""
    _need_gpu(A, Bm, C)
    w, wp, wn = _ws(C)
    _lib.check(_lib.lib().ctcn_gemm_dx(M, N, K, _ptr(A), lda, _ptr(Bm), ldb, _ptr(C), ldc, float(beta), get_precision(), wp, wn, _lib.stream_ptr()),
               "gemm_dx")
    return C


class _Linear(torch.autograd.Function):
    """y = x @ W^T, W (N,K), no bias  (nn.Linear(bias=False), model_ctc.py:137,166)."""

    @staticmethod
    def forward(ctx, x, w):
        _need_gpu(x, w)
        ctx.gw_view = _gview(w)
        x, w = _f32c(x), _f32c(w)
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        gemm(0, 1, M, N, K, x, K, w, K, y, N)
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _f32c(gy)
        M, K = x.shape
        N = w.shape[0]
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty((M, K), dtype=torch.float32, device=x.device)
            gemm(0, 0, M, K, N, gy, N, w, K, gx, K)            # dX = dY * W
        if ctx.needs_input_grad[1]:
            if ctx.gw_view is not None:
                gemm(1, 0, N, K, M, gy, N, x, K, ctx.gw_view, K, beta=1.0)   # dW += dY^T * X into the flat grad buffer
            else:
                gw = torch.empty((N, K), dtype=torch.float32, device=x.device)
                gemm(1, 0, N, K, M, gy, N, x, K, gw, K)        # dW = dY^T * X
        return gx, gw


def linear(x2d, w):
    return _Linear.apply(x2d, w)


# --------------------------------------------------------------------------------------------------
# recurrent layer
# --------------------------------------------------------------------------------------------------
_Saved = collections.namedtuple("_Saved", "x y gates aux w_ih0 w_hh0 w_ih1 w_hh1")     # what _RNNLayer keeps for its backward (aux, w_ih1, w_hh1 may be None)


def _new_rnn_call(dev):
    """ctcn_rnn_call with the fields every call sets (everything a call needs beyond its tensors: the library keeps no state between calls), and
    the slot that receives the name of the kernel THIS call launched (the process-wide ctcn_rnn_last_kernel is last-writer-wins across threads)."""
    call, launched = _lib.RnnCall(), ctypes.c_char_p(None)
    call.status = _lib.status_word(dev).data_ptr()
    call.launched = ctypes.pointer(launched)
    return call, launched


def _note_launch(launched, step_kernel, cell, T, B, H, dirs):
    """Count the recurrence kernel a layer call launched, and learn the shapes that need batch chunks: a call that fell back to the per-timestep
    kernel `step_kernel` although rnn_persistent is on (rnn_layer chunks this shape's batch from the next call on)."""
    _count_kernel(launched)
    if T > 1 and B > 16 and (launched or b"") == step_kernel and get_option("rnn_persistent"):
        _fallback_shapes.add((cell, H, dirs, B))


def _note_rnn_fwd(I, s, y_drop, w):
    """Development (tools/squat_stress.py trace): where a forward call's buffers live, what it read and wrote."""
    adr = lambda t: t.data_ptr() if t is not None else 0
    _debug_note[0]("rnn_fwd", dict(I=int(I), x=adr(s.x), gates=adr(s.gates), aux=adr(s.aux), y=adr(s.y), y_drop=adr(y_drop), ws=adr(w), w_ih=adr(s.w_ih0), w_hh=adr(s.w_hh0)),
                   dict(x=s.x, y=s.y, gates=s.gates, aux=s.aux, y_drop=y_drop, w_ih=(s.w_ih0, s.w_ih1)))


def _weight_grads(cell, dims, s, dws, prec, xcd_allow=0, side=None):
    """Enqueue ctcn_rnn_bwd_weights on the current stream for the gradients in `dws` (dW_ih0, dW_hh0, dW_ih1, dW_hh1; None: not in this call),
    accumulating (beta = 1).  side: the current stream is this side stream -- its own workspace, and the caching allocator must not recycle
    the saved tensors under it."""
    w, wp, wn = _ws(s.x, tag="main" if side is None else "side")
    _lib.check(_lib.lib().ctcn_rnn_bwd_weights(cell, *dims, _ptr(s.x), _ptr(s.y), _ptr(s.gates), _ptr(s.aux), *[_ptr(d) for d in dws],
                                               1.0, prec, xcd_allow, wp, wn, _lib.stream_ptr()), "rnn_bwd_weights")
    if side is not None:
        for t in (s.x, s.y, s.gates, s.aux):
            if t is not None:
                t.record_stream(side)


class _RNNLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_ih0, w_hh0, w_ih1, w_hh1, cell, training, drop_p=0.0):
        _need_gpu(x, w_ih0, w_hh0, w_ih1, w_hh1)
        ctx.gviews = [_gview(w) for w in (w_ih0, w_hh0, w_ih1, w_hh1)]
        x = _f32c(x)
        ws = [_f32c(w) if w is not None else None for w in (w_ih0, w_hh0, w_ih1, w_hh1)]
        # W_hh is the one operand the recurrent kernels read with unconditional 16-byte loads (ctcn_rnn_fwd refuses another): a caller's
        # misaligned view is copied (G*H*H floats) -- optim.FlatAdam's parameters never are.  Gradients still go to the caller's view.
        for k in (1, 3):
            if ws[k] is not None and ws[k].data_ptr() % 16:
                ws[k] = ws[k].clone()
        T, B, I = x.shape
        G = GATES[cell]
        H = ws[1].shape[1]
        dirs = 2 if ws[2] is not None else 1
        dev = x.device
        y = torch.empty((T, B, dirs * H), dtype=torch.float32, device=dev)
        gates = torch.empty((T, B, dirs, G * H), dtype=torch.float32, device=dev)
        aux = torch.empty((T, B, dirs, H), dtype=torch.float32, device=dev) if cell != 2 else None
        s = _Saved(x, y, gates, aux, *ws)
        w, wp, wn = _ws(x)
        L = _lib.lib()
        side = _device_side(dev)
        call, launched = _new_rnn_call(dev)
        piped = plan_fwd_pipeline(T, B, H, dirs, L.ctcn_device_xcds())
        if piped:
            st = side.side_stream()
            w2, wp2, wn2 = _ws(x, tag="side")
            call.side_stream, call.side_event, call.side_ws, call.side_ws_bytes, call.xcd_allow = st.cuda_stream, side.prelaunch_event().cuda_event, w2.data_ptr(), wn2, piped
        # the layer's dropout (BatchRNN: rnn -> nn.Dropout) in the same call: the recurrence stores the dropped output itself where its
        # tagged-gather kernel applies; the random stream advances exactly as for a separate dropout of y
        ctx.drop = None
        y_drop = None
        if training and drop_p > 0.0:
            y_drop = torch.empty_like(y)
            seed, off = _next_dropout_stream(y.numel())
            ctx.drop = (float(drop_p), seed, off)
            call.y_drop, call.drop_p, call.drop_seed, call.drop_offset = y_drop.data_ptr(), float(drop_p), seed, off
        _lib.check(L.ctcn_rnn_fwd_ex(cell, T, B, I, H, dirs, _ptr(x), _ptr(ws[0]), _ptr(ws[1]), _ptr(ws[2]), _ptr(ws[3]),
                                     _ptr(y), _ptr(gates), _ptr(aux), get_precision(), wp, wn, _lib.stream_ptr(), ctypes.byref(call)), "rnn_fwd_ex")
        _note_launch(launched.value, b"rnn_fwd_step", cell, T, B, H, dirs)
        if _debug_note[0] is not None:
            _note_rnn_fwd(I, s, y_drop, w)
        if piped:
            # by the time the recurrence ends the side stream's GEMMs have long finished (the kernel waited for their counter); the join
            # only tells the allocator and the following kernels so
            torch.cuda.current_stream(dev).wait_stream(st)
            for t in (x, gates, ws[0], ws[2]):
                if t is not None:
                    t.record_stream(st)
        ctx.cell, ctx.dims = cell, (T, B, I, H, dirs)
        ctx.early_ok = not _chunking[0]        # a batch chunk's weight gradients are partial sums: no early all-reduce of the layer's slice (parallel._slice_ready)
        ctx.consumed = False
        ctx.counted = any(ctx.needs_input_grad)     # a recurrent layer of this device whose backward is still to come (_DeviceSide.live)
        if ctx.counted:
            side.live += 1
        ctx.save_for_backward(*s)
        return y if y_drop is None else y_drop

    @staticmethod
    def backward(ctx, gy):
        if ctx.consumed:
            raise RuntimeError("ctc_pytorch_amd RNN layer: backward ran twice (the gate reserve is overwritten in place)")
        ctx.consumed = True
        dims = T, B, I, H, dirs = ctx.dims
        cell = ctx.cell
        s = _Saved(*ctx.saved_tensors)
        wts = (s.w_ih0, s.w_hh0, s.w_ih1, s.w_hh1)
        gy = _f32c(gy)
        dev = s.x.device
        dx = torch.empty_like(s.x) if ctx.needs_input_grad[0] else None
        # the weight gradients: accumulated (beta = 1) into optim.FlatAdam's views where every matrix of the layer has one, else fresh tensors
        into_flat = all(g is not None for g, w in zip(ctx.gviews, wts) if w is not None)
        dws = [None if w is None else (g if into_flat else torch.empty_like(w)) for g, w in zip(ctx.gviews, wts)]
        L = _lib.lib()
        scratch = torch.empty(L.ctcn_rnn_scratch_bytes(cell, B, H, dirs), dtype=torch.uint8, device=dev)
        w, wp, wn = _ws(s.x)
        side = _device_side(dev)
        if ctx.counted:
            side.live = max(0, side.live - 1)
        mode, allow = plan_weight_grads(cell, T, B, I, H, dirs, L.ctcn_device_xcds(), L.ctcn_device_cus(), into_flat=into_flat, chunk=not ctx.early_ok,
                                        bottom=dx is None or side.live == 0, above_parked=side.deferred is not None)
        # the layer above: its weight GEMMs start together with this layer's recurrence -- the library records `ev` right
        # before that launch, behind its own small preparatory kernels, and the side stream waits for it
        above, side.deferred, ev = side.deferred, None, None
        call, launched = _new_rnn_call(dev)
        if above is not None:
            ev = side.prelaunch_event()
            call.prelaunch_event = ev.cuda_event
        gd = None
        if ctx.drop is not None:    # gy is the gradient of the dropped output: the same mask, applied by the recurrence as it consumes gy (or by
            p_, seed_, off_ = ctx.drop                      # a dropout pass into gd where that kernel does not apply)
            gd = torch.empty_like(gy)
            call.dy_tmp, call.drop_p, call.drop_seed, call.drop_offset = gd.data_ptr(), p_, seed_, off_
        prec = get_precision()
        try:
            _lib.check(L.ctcn_rnn_bwd_ex(cell, T, B, I, H, dirs, _ptr(s.x), *[_ptr(t) for t in wts], _ptr(s.y), _ptr(s.gates), _ptr(s.aux), _ptr(gy), _ptr(dx),
                                         *[_ptr(d) if mode == WG_INLINE else None for d in dws],
                                         1.0 if into_flat else 0.0, prec, _ptr(scratch), wp, wn, _lib.stream_ptr(), ctypes.byref(call)), "rnn_bwd_ex")
        except Exception:
            side.deferred = above                       # keep the parked work for the join
            raise
        _note_launch(launched.value, b"rnn_bwd_step", cell, T, B, H, dirs)
        if above is not None:
            above(ev)
        if mode in (WG_SPLIT_END, WG_SPLIT_NOW):
            # one direction per stream (the variants measured and not kept -- the products dealt by matrix, each direction on half of the XCDs --
            # are in DESIGN_HISTORY.md, "Weight-gradient side stream")
            st, main = side.side_stream(), torch.cuda.current_stream(dev)
            st.wait_stream(main)                        # (behind the layer above's weight GEMMs already queued there)
            with torch.cuda.stream(st):
                _weight_grads(cell, dims, s, [None, None] + dws[2:], prec, side=st)
            _weight_grads(cell, dims, s, dws[:2] + [None, None], prec)
            # (no gradient-ready hook: nothing is left to hide a collective behind; these slices go with the step-end all-reduce)
            if mode == WG_SPLIT_NOW:
                main.wait_stream(st)
            else:
                side.pending = True
                torch.autograd.Variable._execution_engine.queue_callback(side.join_at_end)
        elif mode == WG_DEFERRED:
            st = side.side_stream()

            def weights_on_side_stream(after=None):
                if after is None:
                    st.wait_stream(torch.cuda.current_stream(dev))
                else:
                    st.wait_event(after)
                with torch.cuda.stream(st):
                    _weight_grads(cell, dims, s, dws, prec, allow, side=st)
                    if _grad_ready["hook"] is not None:      # this layer's weight gradients are final once `st` gets here (a batch chunk, whose are not, is never deferred)
                        _grad_ready["hook"]([t for t in dws if t is not None])
                side.pending = True

            side.deferred = weights_on_side_stream      # issued when the recurrence of the layer below is launched
            # one join per layer is harmless and keeps the path safe if an earlier backward pass died before its callback ran
            torch.autograd.Variable._execution_engine.queue_callback(side.join_at_end)
        return (dx,) + ((None,) * 7 if into_flat else tuple(dws) + (None,) * 3)


def persistent_batch_limit(H, dirs, nx, cus):
    """Rows one launch of the persistent recurrences can hold: a (direction, 16-row batch tile) group is ceil(H / 16) workgroups on ONE XCD,
    one workgroup per CU, so an XCD of cus / nx CUs takes floor((cus / nx) / ceil(H / 16)) groups -- bidirectional on 8 x 32 CUs: 64 rows for
    256 < H <= 512, 128 for H <= 256, 256 at H = 128.  0: the shape has no persistent launch at all."""
    nsl = _tiles16(H)
    per_xcd = (cus // max(nx, 1)) // nsl if nsl else 0
    return 16 * ((per_xcd * max(nx, 1)) // dirs) if nx > 1 else 0


def rnn_layer(x, w_ih0, w_hh0, w_ih1, w_hh1, cell, training=True, drop_p=0.0):
    """x (T,B,I) -> y (T,B,dirs*H); cell in {'lstm','gru','tanh'} (nn.LSTM/GRU/RNN, bias=False, model_ctc.py:24-25).
    drop_p > 0 (training only): returns dropout(y, drop_p) instead -- the dropout that follows the layer in BatchRNN (model_ctc.py:34).

    A batch that no persistent launch holds runs as BATCH CHUNKS, one persistent launch each, instead of the per-timestep kernels (round 4):
    the utterances of a batch are independent, a chunk of 64 rows costs ~1.6-1.8 us per timestep and the per-timestep kernels 7-8 us whatever
    B -- cfg2's model at B = 128: 75.7 -> 41.1 ms per step.  WHICH shapes those are is learnt, not computed: the library tries several
    geometries per shape (cfg2's model at B = 96 still runs persistently, on the 256-thread flag kernel), so a shape is chunked from its SECOND
    call on, after its first call was seen to fall back to rnn_fwd_step / rnn_bwd_step (`_fallback_shapes`); the chunk size is
    persistent_batch_limit, which every geometry supports.  The chunks are separate layer calls on the strided x[:, b0:b1] (weight gradients
    accumulate across them as across backward passes); the layer's dropout is then the separate pass over the concatenated output (the same
    mask as layer-then-dropout).  CTCN_BATCH_CHUNKS=0 disables."""
    cellc = CELL[cell] if isinstance(cell, str) else cell
    T, B = int(x.shape[0]), int(x.shape[1])
    H, dirs = int(w_hh0.shape[1]), 2 if w_ih1 is not None else 1
    if x.is_cuda and T > 1 and _chunks_on[0] and (cellc, H, dirs, B) in _fallback_shapes and get_option("rnn_persistent"):
        L = _lib.lib()
        bmax = persistent_batch_limit(H, dirs, L.ctcn_device_xcds(), L.ctcn_device_cus())
        if 0 < bmax < B:
            _chunking[0] = True
            try:
                ys = [_RNNLayer.apply(xc, w_ih0, w_hh0, w_ih1, w_hh1, cellc, training, 0.0) for xc in x.split(bmax, dim=1)]   # (_f32c gathers the strided chunk)
            finally:
                _chunking[0] = False
            return dropout(torch.cat(ys, dim=1), float(drop_p), training)
    return _RNNLayer.apply(x, w_ih0, w_hh0, w_ih1, w_hh1, cellc, training, float(drop_p))


_chunks_on = [os.environ.get("CTCN_BATCH_CHUNKS", "1") != "0"]
_chunking = [False]           # set while rnn_layer issues the chunk calls of one layer (read by _RNNLayer.forward)
_fallback_shapes = set()      # (cell, H, dirs, B) whose unchunked call ran the per-timestep kernels although rnn_persistent was on


def set_batch_chunks(flag):
    _chunks_on[0] = bool(flag)


def mark_batch_chunks(cell, H, dirs, B):
    """Chunk the batch of this layer shape from its FIRST call on (rnn_layer otherwise learns it from the first call's fallback to the
    per-timestep kernels, so a process's first step differs in rounding from its later ones): for runs that must be reproducible step for
    step across restarts.  cell: 'lstm' | 'gru' | 'tanh' or its code."""
    _fallback_shapes.add((CELL[cell] if isinstance(cell, str) else int(cell), int(H), int(dirs), int(B)))


# --------------------------------------------------------------------------------------------------
# batch norm (+ fused ReLU)
# --------------------------------------------------------------------------------------------------
# Synchronised BatchNorm (data parallel): `_sync_bn["reduce"]` is a callable (sums_tensor, local_count) -> global_count
# that all-reduces the (C, 2) float64 per-channel sums in place and returns the global element count per channel;
# parallel.enable_sync_bn() installs the torch.distributed one.  None = per-shard statistics (the fast default).
_sync_bn = {"reduce": None}


def set_sync_bn(reducer):
    _sync_bn["reduce"] = reducer


class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, outer, C, inner, training, momentum, eps, relu, nbt=None, drop_p=0.0):
        _need_gpu(x, gamma, beta)
        ctx.gviews = (_gview(gamma), _gview(beta))
        x = _f32c(x)
        dev = x.device
        y = torch.empty_like(x)
        L = _lib.lib()
        ctx.sync = None
        ctx.drop = None
        if training and drop_p > 0.0:
            # BatchNorm (+ ReLU) + the dropout behind it in one apply pass (LayerCNN, model_ctc.py:62-67); the Philox counters are drawn exactly
            # where the separate dropout would draw them (batch_norm() only fuses when nothing random sits between the two)
            mean = torch.empty(C, dtype=torch.float32, device=dev)
            rstd = torch.empty(C, dtype=torch.float32, device=dev)
            seed, off = _next_dropout_stream(x.numel())
            w, wp, wn = _ws(x)
            _lib.check(L.ctcn_bn_fwd_train_dropout(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), _ptr(mean), _ptr(rstd),
                                                   outer, C, inner, float(eps), float(momentum), int(relu), wp, wn, _lib.stream_ptr(), _ptr(nbt),
                                                   float(drop_p), seed, off), "bn_fwd_train_dropout")
            ctx.save_for_backward(x, None, gamma, mean, rstd, beta)
            ctx.train_mode = True
            ctx.drop = (float(drop_p), seed, off)
            ctx.geom = (outer, C, inner, relu, eps)
            return y
        if training and _sync_bn["reduce"] is not None:
            mean = torch.empty(C, dtype=torch.float32, device=dev)
            rstd = torch.empty(C, dtype=torch.float32, device=dev)
            sums = torch.empty((C, 2), dtype=torch.float64, device=dev)
            w, wp, wn = _ws(x)
            _lib.check(L.ctcn_bn_fwd_sums(_ptr(x), _ptr(sums), outer, C, inner, wp, wn, _lib.stream_ptr()), "bn_fwd_sums")
            total = float(_sync_bn["reduce"](sums, outer * inner))
            _lib.check(L.ctcn_bn_fwd_finish(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), _ptr(mean), _ptr(rstd),
                                            _ptr(sums), total, outer, C, inner, float(eps), float(momentum), int(relu),
                                            _lib.stream_ptr(), _ptr(nbt)), "bn_fwd_finish")
            ctx.save_for_backward(x, y if relu else None, gamma, mean, rstd)
            ctx.train_mode = True
            ctx.sync = (_sync_bn["reduce"], total)
        elif training:
            mean = torch.empty(C, dtype=torch.float32, device=dev)
            rstd = torch.empty(C, dtype=torch.float32, device=dev)
            w, wp, wn = _ws(x)
            _lib.check(L.ctcn_bn_fwd_train(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), _ptr(mean), _ptr(rstd),
                                           outer, C, inner, float(eps), float(momentum), int(relu), wp, wn, _lib.stream_ptr(), _ptr(nbt)),
                       "bn_fwd_train")
            ctx.save_for_backward(x, y if relu else None, gamma, mean, rstd)
            ctx.train_mode = True
        else:
            _lib.check(L.ctcn_bn_fwd_eval(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), outer, C, inner, float(eps),
                                          int(relu), _lib.stream_ptr()), "bn_fwd_eval")
            ctx.save_for_backward(x, y if relu else None, gamma, rm, rv)
            ctx.train_mode = False
        ctx.geom = (outer, C, inner, relu, eps)
        return y

    @staticmethod
    def backward(ctx, gy):
        outer, C, inner, relu, eps = ctx.geom
        if ctx.drop is not None:
            x, _, gamma, a, b, beta = ctx.saved_tensors
            gy = _f32c(gy)
            dx = torch.empty_like(x)
            into_flat = ctx.gviews[0] is not None and ctx.gviews[1] is not None
            dgamma, dbeta = ctx.gviews if into_flat else (torch.empty(C, dtype=torch.float32, device=x.device), torch.empty(C, dtype=torch.float32, device=x.device))
            w, wp, wn = _ws(x)
            p_, seed_, off_ = ctx.drop
            _lib.check(_lib.lib().ctcn_bn_bwd_dropout(_ptr(x), _ptr(gy), _ptr(gamma), _ptr(beta), _ptr(a), _ptr(b), _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                                                      outer, C, inner, int(relu), 1.0 if into_flat else 0.0, wp, wn, _lib.stream_ptr(), p_, seed_, off_),
                       "bn_bwd_dropout")
            if into_flat:
                dgamma = dbeta = None
            return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None, None, None
        x, y, gamma, a, b = ctx.saved_tensors
        gy = _f32c(gy)
        dev = x.device
        if not ctx.train_mode:
            # eval-mode BN is an affine map: dx = dy' * gamma / sqrt(rv + eps); statistics carry no gradient.
            raise NotImplementedError("ctc_pytorch_amd: backward through eval-mode BatchNorm is not part of the hot path")
        dx = torch.empty_like(x)
        into_flat = ctx.gviews[0] is not None and ctx.gviews[1] is not None
        if into_flat:
            dgamma, dbeta = ctx.gviews
        else:
            dgamma = torch.empty(C, dtype=torch.float32, device=dev)
            dbeta = torch.empty(C, dtype=torch.float32, device=dev)
        w, wp, wn = _ws(x)
        if ctx.sync is not None:
            reducer, total = ctx.sync
            L = _lib.lib()
            local = torch.empty((C, 2), dtype=torch.float64, device=dev)
            _lib.check(L.ctcn_bn_bwd_sums(_ptr(x), _ptr(y), _ptr(gy), _ptr(a), _ptr(b), _ptr(local), outer, C, inner, int(relu), wp, wn,
                                          _lib.stream_ptr()), "bn_bwd_sums")
            glob = local.clone()
            reducer(glob, outer * inner)
            _lib.check(L.ctcn_bn_bwd_finish(_ptr(x), _ptr(y), _ptr(gy), _ptr(gamma), _ptr(a), _ptr(b), _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                                            _ptr(local), _ptr(glob), total, outer, C, inner, int(relu), 1.0 if into_flat else 0.0,
                                            wp, wn, _lib.stream_ptr()), "bn_bwd_finish")
        else:
            _lib.check(_lib.lib().ctcn_bn_bwd(_ptr(x), _ptr(y), _ptr(gy), _ptr(gamma), _ptr(a), _ptr(b), _ptr(dx), _ptr(dgamma),
                                              _ptr(dbeta), outer, C, inner, int(relu), 1.0 if into_flat else 0.0, wp, wn,
                                              _lib.stream_ptr()), "bn_bwd")
        if into_flat:
            dgamma = dbeta = None
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None, None, None


def batch_norm(x, gamma, beta, running_mean, running_var, outer, C, inner, training, momentum=0.1, eps=1e-5, relu=False, num_batches_tracked=None,
               drop_p=0.0, lengths=None, frame=None):
    """num_batches_tracked: nn.BatchNorm's int64 counter (device tensor) or None -- in training the statistics kernel adds 1 to it (no launch
    of its own).  drop_p > 0 (training only): returns dropout(batch_norm(x), drop_p) from ONE apply pass -- the same values, the same Philox
    counters as a separate ops.dropout behind it (round 5; per-shard statistics only: with synchronised BatchNorm the two stay separate).
    lengths (see batch_norm_masked): statistics over the real frames only, zeros at the padded ones; None runs the plain kernels."""
    if lengths is not None:
        return batch_norm_masked(x, gamma, beta, running_mean, running_var, outer, C, inner, training, lengths, frame, momentum, eps, relu,
                                 num_batches_tracked, drop_p)
    if training and drop_p > 0.0 and (_sync_bn["reduce"] is not None or not _fuse_bn_dropout[0]):
        y = batch_norm(x, gamma, beta, running_mean, running_var, outer, C, inner, training, momentum, eps, relu, num_batches_tracked)
        return dropout(y, drop_p, training)
    if not training:
        drop_p = 0.0
    if num_batches_tracked is not None and (not training or num_batches_tracked.dtype != torch.int64 or not num_batches_tracked.is_cuda):
        if training:
            num_batches_tracked += 1
        num_batches_tracked = None
    return _BatchNorm.apply(x, gamma, beta, running_mean, running_var, outer, C, inner, training, momentum, eps, relu, num_batches_tracked, float(drop_p))


_fuse_bn_dropout = [os.environ.get("CTCN_FUSE_BN_DROPOUT", "1") != "0"]


def set_fuse_bn_dropout(flag):
    """BatchNorm (+ ReLU) and the dropout behind it in one pass (default on; CTCN_FUSE_BN_DROPOUT=0: two passes, the same values)."""
    _fuse_bn_dropout[0] = bool(flag)


# --------------------------------------------------------------------------------------------------
# length-aware BatchNorm and frame mask
# --------------------------------------------------------------------------------------------------
def frame_lengths(lengths, device, batch=None, tmax=None):
    """`lengths` (int tensor on the host or the device, list or tuple: real frames per utterance) as the int32 device vector the masked
    kernels read.  Host-resident lengths are validated here (ValueError for len < 1, len > tmax or a wrong batch size) and uploaded with one
    copy; a device tensor is taken as it is (the kernels clamp it) -- nothing is ever read back."""
    if torch.is_tensor(lengths):
        if lengths.dim() != 1 or lengths.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8, torch.int8):
            raise ValueError("lengths: expected a 1-D integer tensor, got %s %s" % (lengths.dtype, tuple(lengths.shape)))
        if batch is not None and lengths.numel() != batch:
            raise ValueError("lengths: %d entries for a batch of %d" % (lengths.numel(), batch))
        if lengths.is_cuda:
            return lengths if lengths.dtype == torch.int32 and lengths.is_contiguous() else lengths.to(torch.int32).contiguous()
        host = lengths.detach().numpy().astype(np.int64)
    else:
        host = np.asarray(lengths)
        if host.ndim != 1 or host.dtype.kind not in "iu":
            raise ValueError("lengths: expected a flat sequence of integers")
        host = host.astype(np.int64)
        if batch is not None and host.size != batch:
            raise ValueError("lengths: %d entries for a batch of %d" % (host.size, batch))
    check_frame_lengths(host, tmax)
    return torch.from_numpy(host.astype(np.int32)).to(device, non_blocking=True)


def check_frame_lengths(host, tmax=None):
    if host.size and int(host.min()) < 1:
        raise ValueError("lengths: every utterance needs at least one frame, got %d" % int(host.min()))
    if tmax is not None and host.size and int(host.max()) > tmax:
        raise ValueError("lengths: %d exceeds the %d frames of the batch" % (int(host.max()), tmax))


def _frame_geom(outer, inner, lengths, frame):
    """(batch, frame, tmax) of the C ABI's two layouts (include/ctcn.h): rows (inner == 1) or NCHW planes."""
    nb = int(lengths.numel()) if torch.is_tensor(lengths) else len(lengths)
    if inner == 1:
        if nb < 1 or outer % nb != 0 or frame not in (None, 1):
            raise ValueError("lengths: %d entries do not divide %d rows (time-major layout)" % (nb, outer))
        return nb, 1, outer // nb
    frame = 1 if frame is None else int(frame)
    if nb != outer or frame < 1 or inner % frame != 0:
        raise ValueError("lengths: %d entries / frame %d do not fit %d planes of %d elements" % (nb, frame, outer, inner))
    return nb, frame, inner // frame


class _MaskFrames(torch.autograd.Function):
    """y = x at real frames, 0 at padded ones (by select: whatever the padding holds, NaN included, is not read); its own backward."""
    @staticmethod
    def forward(ctx, x, lens, geom):
        _need_gpu(x, lens)
        x = _f32c(x)
        y = torch.empty_like(x)
        ctx.lens, ctx.geom = lens, geom
        batch, frame, outer, C, inner = geom
        _lib.check(_lib.lib().ctcn_mask_frames(_ptr(x), _ptr(y), _ptr(lens), batch, frame, outer, C, inner, _lib.stream_ptr()), "mask_frames")
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = _f32c(gy)
        dx = torch.empty_like(gy)
        batch, frame, outer, C, inner = ctx.geom
        _lib.check(_lib.lib().ctcn_mask_frames(_ptr(gy), _ptr(dx), _ptr(ctx.lens), batch, frame, outer, C, inner, _lib.stream_ptr()), "mask_frames_bwd")
        return dx, None, None


MASK_LAYOUTS = ("tbc", "btf", "bctf")


def mask_frames(x, lengths, layout):
    """Zero the padded frames of `x`.  layout: "tbc" (T,B,C) time-major rows, "btf" (B,T,F) model input, "bctf" (B,C,T,F) feature maps."""
    if layout == "tbc" and x.dim() == 3:
        T, B, C = x.shape
        dims, frame, tmax = (T * B, C, 1), None, T
    elif layout == "btf" and x.dim() == 3:
        B, T, F = x.shape
        dims, frame, tmax = (B, 1, T * F), F, T
    elif layout == "bctf" and x.dim() == 4:
        B, C, T, F = x.shape
        dims, frame, tmax = (B, C, T * F), F, T
    else:
        raise ValueError("mask_frames: layout %r (one of %s) does not fit a %d-D tensor" % (layout, ", ".join(MASK_LAYOUTS), x.dim()))
    lens = frame_lengths(lengths, x.device, B, tmax)           # (checked before anything touches the device)
    _need_gpu(x)
    batch, frame, _ = _frame_geom(dims[0], dims[2], lens, frame)
    return _MaskFrames.apply(x, lens, (batch, frame) + dims)


class _BatchNormMasked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, lens, geom, training, momentum, eps, relu, nbt):
        _need_gpu(x, gamma, beta, lens)
        ctx.gviews = (_gview(gamma), _gview(beta))
        x = _f32c(x)
        y = torch.empty_like(x)
        L = _lib.lib()
        batch, frame, outer, C, inner = geom
        if training:
            mean = torch.empty(C, dtype=torch.float32, device=x.device)
            rstd = torch.empty(C, dtype=torch.float32, device=x.device)
            w, wp, wn = _ws(x)
            _lib.check(L.ctcn_bn_fwd_train_masked(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), _ptr(mean), _ptr(rstd), _ptr(lens),
                                                  batch, frame, outer, C, inner, float(eps), float(momentum), int(relu), wp, wn, _lib.stream_ptr(),
                                                  _ptr(nbt)), "bn_fwd_train_masked")
            ctx.save_for_backward(x, y if relu else None, gamma, mean, rstd)
        else:
            _lib.check(L.ctcn_bn_fwd_eval_masked(_ptr(x), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), _ptr(lens), batch, frame, outer, C, inner,
                                                 float(eps), int(relu), _lib.stream_ptr()), "bn_fwd_eval_masked")
        ctx.train_mode, ctx.lens, ctx.geom, ctx.relu = training, lens, geom, relu
        return y

    @staticmethod
    def backward(ctx, gy):
        if not ctx.train_mode:
            raise NotImplementedError("ctc_pytorch_amd: backward through eval-mode BatchNorm is not part of the hot path")
        x, y, gamma, mean, rstd = ctx.saved_tensors
        batch, frame, outer, C, inner = ctx.geom
        gy = _f32c(gy)
        dx = torch.empty_like(x)
        into_flat = ctx.gviews[0] is not None and ctx.gviews[1] is not None
        dgamma, dbeta = ctx.gviews if into_flat else (torch.empty(C, dtype=torch.float32, device=x.device), torch.empty(C, dtype=torch.float32, device=x.device))
        w, wp, wn = _ws(x)
        _lib.check(_lib.lib().ctcn_bn_bwd_masked(_ptr(x), _ptr(y), _ptr(gy), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                                                 _ptr(ctx.lens), batch, frame, outer, C, inner, int(ctx.relu), 1.0 if into_flat else 0.0, wp, wn,
                                                 _lib.stream_ptr()), "bn_bwd_masked")
        if into_flat:
            dgamma = dbeta = None
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None


def batch_norm_masked(x, gamma, beta, running_mean, running_var, outer, C, inner, training, lengths, frame=None, momentum=0.1, eps=1e-5, relu=False,
                      num_batches_tracked=None, drop_p=0.0):
    """batch_norm over the real frames of a padded batch: `lengths` = frames per utterance; inner == 1: x is (T * B, C) time-major rows;
    inner > 1: x is (B, C, T' * frame) with `frame` elements per time step.  Statistics, running statistics and gradients use the
    n = sum(lengths) * frame valid elements per channel (counted on the device); the output and dx are 0 at padded frames, which are never
    read.  drop_p > 0: the separate ops.dropout follows (the values and Philox counters of the fused pass of batch_norm)."""
    if training and _sync_bn["reduce"] is not None:
        raise NotImplementedError("ctc_pytorch_amd: synchronised BatchNorm (parallel.enable_sync_bn) does not take lengths -- the count of valid "
                                  "frames would have to be reduced across the ranks; run per-shard statistics or drop the lengths")
    batch, frame, tmax = _frame_geom(outer, inner, lengths, frame)
    lens = frame_lengths(lengths, x.device, batch, tmax)
    _need_gpu(x)
    nbt = num_batches_tracked
    if nbt is not None and (not training or nbt.dtype != torch.int64 or not nbt.is_cuda):
        if training:
            nbt += 1
        nbt = None
    y = _BatchNormMasked.apply(x, gamma, beta, running_mean, running_var, lens, (batch, frame, int(outer), int(C), int(inner)), bool(training),
                               momentum, eps, bool(relu), nbt)
    return dropout(y, drop_p, training) if drop_p > 0.0 else y


class _ReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _need_gpu(x)
        x = _f32c(x)
        y = torch.empty_like(x)
        _lib.check(_lib.lib().ctcn_relu_fwd(_ptr(x), _ptr(y), x.numel(), _lib.stream_ptr()), "relu_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = _f32c(gy)
        dx = torch.empty_like(y)
        _lib.check(_lib.lib().ctcn_relu_bwd(_ptr(y), _ptr(gy), _ptr(dx), y.numel(), _lib.stream_ptr()), "relu_bwd")
        return dx


def relu(x):
    return _ReLU.apply(x)


# --------------------------------------------------------------------------------------------------
# dropout
# --------------------------------------------------------------------------------------------------
_drop_counter = [0]
_drop_lock = __import__("threading").Lock()


def _next_dropout_stream(n):
    """(seed, offset): seed follows torch.manual_seed (+ rank so that DP shards decorrelate); the offset
    advances by the number of Philox groups consumed so that successive calls never reuse counters."""
    seed = (torch.initial_seed() ^ (0x9E3779B97F4A7C15 * (1 + _rank()))) & 0xFFFFFFFFFFFFFFFF
    with _drop_lock:        # (two models stepping in two threads of one process share the stream: no two calls may take the same offsets)
        off = _drop_counter[0]
        _drop_counter[0] += (n + 3) // 4
    return seed, off


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        _need_gpu(x)
        x = _f32c(x)
        y = torch.empty_like(x)
        seed, off = _next_dropout_stream(x.numel())
        ctx.rng = (p, seed, off)
        _lib.check(_lib.lib().ctcn_dropout(_ptr(x), _ptr(y), x.numel(), float(p), seed, off, _lib.stream_ptr()), "dropout")
        return y

    @staticmethod
    def backward(ctx, gy):
        p, seed, off = ctx.rng
        gy = _f32c(gy)
        dx = torch.empty_like(gy)
        _lib.check(_lib.lib().ctcn_dropout(_ptr(gy), _ptr(dx), gy.numel(), float(p), seed, off, _lib.stream_ptr()), "dropout_bwd")
        return dx, None


def dropout(x, p, training):
    if not training or p == 0.0:
        return x
    if p < 0.0 or p > 1.0:
        raise ValueError("dropout probability has to be between 0 and 1, but got %r" % (p,))
    if p == 1.0:                    # torch: everything dropped (a memset), still in the graph: x.grad is zeros, not None
        return _DropAll.apply(x)
    return _Dropout.apply(x, p)


class _DropAll(torch.autograd.Function):
    """dropout(p = 1): zeros forward and backward; no launch (torch keeps the node, so backward() through it works and leaves zero gradients)."""
    @staticmethod
    def forward(ctx, x):
        return torch.zeros_like(x)

    @staticmethod
    def backward(ctx, gy):
        return torch.zeros_like(gy)


# --------------------------------------------------------------------------------------------------
# conv2d
# --------------------------------------------------------------------------------------------------
class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, padding):
        _need_gpu(x, w, b)
        ctx.gviews = (_gview(w), _gview(b))
        x, w = _f32c(x), _f32c(w)
        B, Ci, Hi, Wi = x.shape
        Co, _, kh, kw = w.shape
        sh, sw = stride
        ph, pw = padding
        Ho = (Hi + 2 * ph - kh) // sh + 1
        Wo = (Wi + 2 * pw - kw) // sw + 1
        y = torch.empty((B, Co, Ho, Wo), dtype=torch.float32, device=x.device)
        ctx.geom = (B, Ci, Hi, Wi, Co, kh, kw, sh, sw, ph, pw)
        _lib.check(_lib.lib().ctcn_conv2d_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(y), *ctx.geom, _lib.stream_ptr()), "conv2d_fwd")
        ctx.has_bias = b is not None
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _f32c(gy)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        into_flat = ctx.gviews[0] is not None and (not ctx.has_bias or ctx.gviews[1] is not None)
        if into_flat:
            dw, db = ctx.gviews[0], (ctx.gviews[1] if ctx.has_bias else None)
        else:
            dw = torch.empty_like(w)
            db = torch.empty(w.shape[0], dtype=torch.float32, device=x.device) if ctx.has_bias else None
        ws, wp, wn = _ws(x)
        _lib.check(_lib.lib().ctcn_conv2d_bwd(_ptr(x), _ptr(w), _ptr(gy), _ptr(dx), _ptr(dw), _ptr(db), *ctx.geom,
                                              1.0 if into_flat else 0.0, wp, wn, _lib.stream_ptr()), "conv2d_bwd")
        if into_flat:
            dw = db = None
        return dx, dw, db, None, None


class _MaxPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kh, kw):
        _need_gpu(x)
        x = _f32c(x)
        if x.dim() != 4:
            raise ValueError("ctc_pytorch_amd.max_pool2d: expected (B, C, H, W), got %s" % (tuple(x.shape),))
        B, C, Hi, Wi = x.shape
        y = torch.empty((B, C, Hi // kh, Wi // kw), dtype=torch.float32, device=x.device)
        arg = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
        _lib.check(_lib.lib().ctcn_maxpool2d_fwd(_ptr(x), _ptr(y), _ptr(arg), B * C, Hi, Wi, kh, kw, _lib.stream_ptr()), "maxpool2d_fwd")
        ctx.save_for_backward(arg)
        ctx.geom = (B * C, Hi, Wi, kh, kw)
        ctx.in_shape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        (arg,) = ctx.saved_tensors
        gy = _f32c(gy)
        dx = torch.empty(ctx.in_shape, dtype=torch.float32, device=gy.device)
        _lib.check(_lib.lib().ctcn_maxpool2d_bwd(_ptr(gy), _ptr(arg), _ptr(dx), *ctx.geom, _lib.stream_ptr()), "maxpool2d_bwd")
        return dx, None, None


def max_pool2d(x, kernel_size):
    """nn.MaxPool2d(kernel_size)(x): stride = kernel, no padding, floor (model_ctc.py:52-53)."""
    kh, kw = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
    return _MaxPool2d.apply(x, int(kh), int(kw))


def conv2d(x, w, b, stride, padding):
    return _Conv2d.apply(x, w, b, tuple(stride), tuple(padding))


# --------------------------------------------------------------------------------------------------
# log_softmax / argmax / CTC
# --------------------------------------------------------------------------------------------------
class _LogSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        _need_gpu(z)
        z = _f32c(z)
        V = z.shape[-1]
        rows = z.numel() // V
        lp = torch.empty_like(z)
        _lib.check(_lib.lib().ctcn_log_softmax_fwd(_ptr(z), _ptr(lp), None, rows, V, _lib.stream_ptr()), "log_softmax_fwd")
        ctx.save_for_backward(lp)
        return lp

    @staticmethod
    def backward(ctx, g):
        (lp,) = ctx.saved_tensors
        g = _f32c(g)
        V = lp.shape[-1]
        dz = torch.empty_like(lp)
        _lib.check(_lib.lib().ctcn_log_softmax_bwd(_ptr(lp), _ptr(g), _ptr(dz), lp.numel() // V, V, _lib.stream_ptr()), "log_softmax_bwd")
        return dz


def log_softmax(z):
    return _LogSoftmax.apply(z)


def argmax_last(lp):
    """torch.max(lp, -1)[1] (lowest index on ties) as int32 (train_ctc.py:51, ctcDecoder.py:163)."""
    _need_gpu(lp)
    lp = _f32c(lp.detach())
    V = lp.shape[-1]
    out = torch.empty(lp.shape[:-1], dtype=torch.int32, device=lp.device)
    _lib.check(_lib.lib().ctcn_argmax(_ptr(lp), _ptr(out), lp.numel() // V, V, _lib.stream_ptr()), "argmax")
    return out


_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}           # CTCN_REDUCTION_* of include/ctcn.h (torch's at::Reduction values)

CtcArgs = collections.namedtuple("CtcArgs", "lp targets in_len tgt_len Lmax flat batched")


def _lengths(x):
    """input_lengths / target_lengths as torch.nn.CTCLoss takes them (tensor on the host or the device, list, tuple, int) -> 1-D int64 tensor,
    left where it is."""
    t = x if torch.is_tensor(x) else torch.as_tensor(x, dtype=torch.int64)
    return t.reshape(-1).to(dtype=torch.int64)


def ctc_prepare(log_probs, targets, input_lengths, target_lengths):
    """Host-side normalisation of torch.nn.CTCLoss's arguments -> CtcArgs(lp (T,B,V), targets (B,S) padded or 1-D concatenated, in_len (B),
    tgt_len (B) int64, Lmax = the padded row length the lattice reads, flat, batched).  Pure: no kernel, no device allocation.  Unbatched
    (T,C) log-probs come with 1-element or 0-d lengths and 1-D targets and are treated as a batch of one.  Lengths that are already on the
    host are checked against the tensors here (torch raises for them); device lengths are checked by the kernels (NaN for the utterance),
    except that concatenated targets need Lmax = max(target_lengths): one host read of the lengths, as torch's own CUDA path does."""
    if log_probs.dim() not in (2, 3):
        raise ValueError("ctc_pytorch_amd.CTCLoss: log_probs must be (T, B, C) or unbatched (T, C), got %s" % (tuple(log_probs.shape),))
    batched = log_probs.dim() == 3
    lp = log_probs if batched else log_probs.unsqueeze(1)
    T, B, _ = lp.shape
    targets = targets if torch.is_tensor(targets) else torch.as_tensor(targets, dtype=torch.int64)
    in_len, tgt_len = _lengths(input_lengths), _lengths(target_lengths)
    if targets.dim() not in (1, 2):
        raise ValueError("ctc_pytorch_amd.CTCLoss: targets must be (B, S) padded or 1-D concatenated, got %s" % (tuple(targets.shape),))
    flat = targets.dim() == 1
    if in_len.numel() != B or tgt_len.numel() != B or (not flat and targets.shape[0] != B):
        raise ValueError("ctc_pytorch_amd.CTCLoss: batch size mismatch (log_probs %d, targets %s, input_lengths %d, target_lengths %d)"
                         % (B, tuple(targets.shape), in_len.numel(), tgt_len.numel()))
    if flat:
        tl_host = tgt_len.cpu()
        if int(tl_host.min()) < 0:
            raise ValueError("ctc_pytorch_amd.CTCLoss: target_lengths must be >= 0, got min %d" % int(tl_host.min()))
        if int(tl_host.sum()) > targets.numel():
            raise ValueError("ctc_pytorch_amd.CTCLoss: sum(target_lengths) = %d > %d concatenated targets" % (int(tl_host.sum()), targets.numel()))
        Lmax = int(tl_host.max())
    else:
        Lmax = targets.shape[1]
    # torch.nn.CTCLoss raises on lengths outside the tensors; lengths still on the host are checked here for free, lengths
    # already on the device are checked by the kernels (NaN loss and NaN gradient rows for the offending utterance)
    for name, t, hi in (("input_lengths", in_len, T), ("target_lengths", tgt_len, Lmax)):
        if not t.is_cuda and t.numel() and (int(t.min()) < 0 or int(t.max()) > hi):
            raise ValueError("ctc_pytorch_amd.CTCLoss: %s must lie in [0, %d], got min %d max %d" % (name, hi, int(t.min()), int(t.max())))
    return CtcArgs(lp, targets, in_len, tgt_len, Lmax, flat, batched)


class _CTCLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, targets, in_len, tgt_len, Lmax, flat, blank, reduction, zero_infinity):
        T, B, V = lp.shape
        dev = lp.device
        targets = targets.to(device=dev, dtype=torch.int64).contiguous()
        in_len = in_len.to(device=dev).contiguous()
        tgt_len = tgt_len.to(device=dev).contiguous()
        L = _lib.lib()
        if flat:                    # concatenated -> the padded rows the lattice reads, on the device
            padded = torch.empty((B, Lmax), dtype=torch.int64, device=dev)
            if Lmax > 0:
                _lib.check(L.ctcn_ctc_pack_targets(_ptr(targets), targets.numel(), _ptr(tgt_len), _ptr(padded), B, Lmax, _lib.stream_ptr()),
                           "ctc_pack_targets")
            targets = padded
        alpha = torch.empty((T, B, 2 * Lmax + 1), dtype=torch.float32, device=dev)
        nll = torch.empty(B, dtype=torch.float32, device=dev)
        # a gradient will be wanted: beta now, beside alpha, in the same launch (two independent T-step chains)
        beta = torch.empty_like(alpha) if ctx.needs_input_grad[0] else None
        _lib.check(L.ctcn_ctc_fwd_ex(_ptr(lp), _ptr(targets), _ptr(in_len), _ptr(tgt_len), _ptr(alpha), _ptr(beta), _ptr(nll),
                                     T, B, V, Lmax, blank, _lib.stream_ptr()), "ctc_fwd_ex")
        if beta is not None:
            ctx.save_for_backward(lp, targets, in_len, tgt_len, alpha, beta, nll)
        ctx.dims = (T, B, V, Lmax)
        ctx.mode = (blank, reduction, zero_infinity)
        out = torch.empty(B if reduction == _REDUCTIONS["none"] else (), dtype=torch.float32, device=dev)
        _lib.check(L.ctcn_ctc_reduce(_ptr(nll), _ptr(tgt_len), _ptr(out), B, reduction, int(zero_infinity), _lib.stream_ptr()), "ctc_reduce")
        return out

    @staticmethod
    def backward(ctx, g):
        lp, targets, in_len, tgt_len, alpha, beta, nll = ctx.saved_tensors
        T, B, V, Lmax = ctx.dims
        blank, reduction, zero_infinity = ctx.mode
        g = g.to(dtype=torch.float32)
        if g.dim() == 1 and g.stride(0) in (0, 1):         # 'none': (B,) upstream gradient, or the expanded scalar of nll.sum()
            stride = g.stride(0)
        else:
            g = _f32c(g)
            stride = 0 if g.dim() == 0 else 1
        grad = torch.empty_like(lp)
        _lib.check(_lib.lib().ctcn_ctc_grad_ex(_ptr(lp), _ptr(targets), _ptr(in_len), _ptr(tgt_len), _ptr(alpha), _ptr(beta), _ptr(nll),
                                               _ptr(g), stride, reduction, int(zero_infinity), blank, _ptr(grad), T, B, V, Lmax,
                                               _lib.stream_ptr()), "ctc_grad_ex")
        return grad, None, None, None, None, None, None, None, None


def ctc_loss(lp, targets, in_len, tgt_len, blank=0, reduction="sum", zero_infinity=False):
    """torch.nn.functional.ctc_loss on the HIP kernels, in its argument order: any blank in [0, C), reduction 'none' / 'sum' / 'mean'
    (default 'sum', the reference's, train_ctc.py:144; nn.CTCLoss keeps torch's 'mean'), zero_infinity, padded (B, S) or concatenated 1-D
    targets, unbatched (T, C) log-probs.  float32 log-probs on the device only (no CPU fallback)."""
    if reduction not in _REDUCTIONS:
        raise ValueError("%s is not a valid value for reduction" % (reduction,))
    _need_gpu(lp)
    lp = _f32c(lp)
    a = ctc_prepare(lp, targets, in_len, tgt_len)
    V = a.lp.shape[2]
    if not 0 <= int(blank) < V:
        raise ValueError("ctc_pytorch_amd.CTCLoss: blank must lie in [0, %d), got %d" % (V, int(blank)))
    out = _CTCLoss.apply(a.lp, a.targets, a.in_len, a.tgt_len, a.Lmax, a.flat, int(blank), _REDUCTIONS[reduction], bool(zero_infinity))
    return out if a.batched else out.squeeze(0)


CtcAlignment = collections.namedtuple("CtcAlignment", "paths frame_scores scores ok starts ends")


def ctc_forced_align(log_probs, targets, input_lengths, target_lengths, blank=0):
    """CTC forced alignment (ctcn_ctc_align; the capability of torchaudio.functional.forced_align + merge_tokens): the best path through
    the lattice of the KNOWN transcript.  Takes what ctc_loss takes (padded (B, S) or concatenated 1-D targets, lengths as tensors or lists on
    either side, unbatched (T, C) log-probs, any blank in [0, C)) and raises the same ValueErrors, before it looks at the device.  Returns CtcAlignment of device tensors:
    paths (B, T) int32 class id per frame (-1 past the input), frame_scores (B, T) float32 = log_probs[t, b, paths[b, t]] (0 past the
    input), scores (B) float32 = the path's log-probability (a chain of single float32 adds), ok (B) int32 (0: no alignment exists --
    scores -inf, paths -1, spans -1), starts / ends (B, Lmax) int32 = first and one-past-last frame of every target token (-1 past the
    label).  Ties go to the smallest move (stay, then advance one state, then skip the blank).  Unbatched input drops the batch dimension.
    No autograd (log_probs is detached); float32 on the device only (no CPU fallback)."""
    a = ctc_prepare(log_probs, targets, input_lengths, target_lengths)          # pure: the argument errors come before any device work
    T, B, V = a.lp.shape
    if not 0 <= int(blank) < V:
        raise ValueError("ctc_pytorch_amd.ctc_forced_align: blank must lie in [0, %d), got %d" % (V, int(blank)))
    if T == 0 or B == 0:
        raise ValueError("ctc_pytorch_amd.ctc_forced_align: empty log_probs %s" % (tuple(log_probs.shape),))
    _need_gpu(log_probs)
    lp = _f32c(a.lp.detach())
    dev = lp.device
    L = _lib.lib()
    Lmax = a.Lmax
    tg = a.targets.to(device=dev, dtype=torch.int64).contiguous()
    in_len = a.in_len.to(device=dev).contiguous()
    tgt_len = a.tgt_len.to(device=dev).contiguous()
    if a.flat:
        padded = torch.empty((B, Lmax), dtype=torch.int64, device=dev)
        if Lmax > 0:
            _lib.check(L.ctcn_ctc_pack_targets(_ptr(tg), tg.numel(), _ptr(tgt_len), _ptr(padded), B, Lmax, _lib.stream_ptr()), "ctc_pack_targets")
        tg = padded
    paths = torch.empty((B, T), dtype=torch.int32, device=dev)
    frame_scores = torch.empty((B, T), dtype=torch.float32, device=dev)
    scores = torch.empty(B, dtype=torch.float32, device=dev)
    ok = torch.empty(B, dtype=torch.int32, device=dev)
    starts = torch.empty((B, Lmax), dtype=torch.int32, device=dev)
    ends = torch.empty((B, Lmax), dtype=torch.int32, device=dev)
    need = L.ctcn_ctc_align_ws_bytes(T, B, Lmax)
    # back-pointer rows that do not fit in LDS: a buffer of this call's own (stream-ordered: the caching allocator hands it out again only to later work)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    _lib.check(L.ctcn_ctc_align(_ptr(lp), _ptr(tg), _ptr(in_len), _ptr(tgt_len), _ptr(paths), _ptr(frame_scores), _ptr(scores), _ptr(ok),
                                _ptr(starts), _ptr(ends), T, B, V, Lmax, int(blank), _ptr(ws), need, _lib.stream_ptr()), "ctc_align")
    if not a.batched:
        paths, frame_scores, scores, ok, starts, ends = (x.squeeze(0) for x in (paths, frame_scores, scores, ok, starts, ends))
    return CtcAlignment(paths, frame_scores, scores, ok, starts, ends)


# --------------------------------------------------------------------------------------------------
# decode helpers (no autograd)
# --------------------------------------------------------------------------------------------------
def greedy_collapse(idx, lens, blank=0, batch_major=False):
    """idx int32 on device, (T,B) time-major or (B,T) if batch_major (any strides); lens (B)
    -> (ids (B,T) int32, out_len (B) int32), both on device."""
    _need_gpu(idx)
    if idx.dtype != torch.int32:
        idx = idx.to(torch.int32)
    if batch_major:
        B, T = idx.shape
        st_b, st_t = idx.stride()
    else:
        T, B = idx.shape
        st_t, st_b = idx.stride()
    lens = torch.as_tensor(lens, device=idx.device).to(torch.int32).contiguous()
    ids = torch.empty((B, T), dtype=torch.int32, device=idx.device)
    out_len = torch.empty(B, dtype=torch.int32, device=idx.device)
    _lib.check(_lib.lib().ctcn_greedy_collapse(_ptr(idx), st_t, st_b, _ptr(lens), _ptr(ids), _ptr(out_len), T, B, int(blank),
                                               _lib.stream_ptr()), "greedy_collapse")
    return ids, out_len


PathTokens = collections.namedtuple("PathTokens", "ids lengths starts ends mean_lp min_lp mean_margin path_score")


def path_tokens(path, lens, log_probs, blank=0, batch_major=False):
    """The tokens of a per-frame class path with their frames and scores (ctcn_path_tokens; definition in include/ctcn.h): path int32,
    (T,B) time-major or (B,T) if batch_major (any strides) -- the arg-max path of argmax_last or the `paths` of ctc_forced_align; lens (B);
    log_probs (T,B,V) float32.  Returns PathTokens of device tensors: ids, starts, ends (B,T) int32 (-1 past lengths[b]), lengths (B) int32,
    mean_lp, min_lp, mean_margin (B,T) float32 (0 past lengths[b]): per token the mean and the minimum of its class's log-prob over its
    frames [start, end) and the mean lead over the best other class; path_score (B) float32: the log-probability of the whole path.  ids
    and lengths are greedy_collapse's.  A class id outside [0, V) counts as blank.  Raises ValueError, before it looks at the device, for
    a blank outside [0, V), empty tensors, shapes that do not match and lens of the wrong length.  No autograd; float32 on the device
    only (no CPU fallback)."""
    if log_probs.dim() != 3 or path.dim() != 2:
        raise ValueError("ctc_pytorch_amd.path_tokens: expected log_probs (T, B, V) and a 2-D path, got %s and %s" % (tuple(log_probs.shape), tuple(path.shape)))
    T, B, V = log_probs.shape
    if T == 0 or B == 0 or V == 0:
        raise ValueError("ctc_pytorch_amd.path_tokens: empty log_probs %s" % (tuple(log_probs.shape),))
    if tuple(path.shape) != ((B, T) if batch_major else (T, B)):
        raise ValueError("ctc_pytorch_amd.path_tokens: path %s does not match log_probs %s (batch_major=%s)"
                         % (tuple(path.shape), tuple(log_probs.shape), bool(batch_major)))
    if not 0 <= int(blank) < V:
        raise ValueError("ctc_pytorch_amd.path_tokens: blank must lie in [0, %d), got %d" % (V, int(blank)))
    lens = lens if torch.is_tensor(lens) else torch.as_tensor(lens)
    if lens.numel() != B:
        raise ValueError("ctc_pytorch_amd.path_tokens: %d lengths for a batch of %d" % (lens.numel(), B))
    _need_gpu(path, log_probs)
    lp = _f32c(log_probs.detach())
    dev = lp.device
    if path.dtype != torch.int32:
        path = path.to(torch.int32)
    st_b, st_t = path.stride() if batch_major else path.stride()[::-1]
    lens = lens.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    ints = torch.empty((3, B, T), dtype=torch.int32, device=dev)
    vals = torch.empty((3, B, T), dtype=torch.float32, device=dev)
    out_len = torch.empty(B, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ctcn_path_tokens(_ptr(path), st_t, st_b, _ptr(lp), _ptr(lens), _ptr(ints[0]), _ptr(out_len), _ptr(ints[1]),
                                           _ptr(ints[2]), _ptr(vals[0]), _ptr(vals[1]), _ptr(vals[2]), _ptr(score), T, B, V, int(blank),
                                           _lib.stream_ptr()), "path_tokens")
    return PathTokens(ints[0], out_len, ints[1], ints[2], vals[0], vals[1], vals[2], score)


def edit_distance(ids, ids_len, targets, tgt_len):
    """per-utterance Levenshtein distance (B,) int32 on device (editdistance.eval, model_ctc.py:200)."""
    _need_gpu(ids)
    dev = ids.device
    targets = targets.to(device=dev, dtype=torch.int64).contiguous()
    tgt_len = tgt_len.to(device=dev, dtype=torch.int64).contiguous()
    B = ids.shape[0]
    if targets.dim() != 2 or targets.shape[0] != B or tgt_len.numel() != B or ids_len.numel() != B:
        raise ValueError("ctc_pytorch_amd.edit_distance: expected ids (B,T), ids_len (B), targets (B,Lmax), tgt_len (B)")
    ldb = targets.shape[1]
    out = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().ctcn_edit_distance(_ptr(ids), _ptr(ids_len), _ptr(targets), _ptr(tgt_len), _ptr(out), B, ids.shape[1], ldb,
                                             max(ldb, 1), _lib.stream_ptr()), "edit_distance")
    return out


EditOps = collections.namedtuple("EditOps", "counts ali ali_len")


def edit_ops(ids, ids_len, targets, tgt_len, class_map=None, num_classes=None, confusion=None, alignment=False):
    """The error breakdown behind edit_distance (ctcn_edit_ops; definition and tie rule in include/ctcn.h): per utterance
    counts (B,6) int32 = (sub, del, ins, cor, hyp_len', ref_len') with the lengths taken after the class map, and with alignment=True
    ali (B, T + Lmax, 2) int32 = the (reference id, hypothesis id) pairs in forward order, -1 = none, plus ali_len (B) int32 (both None
    otherwise).  class_map: V int32 entries applied to both sequences (a value in [0, V) replaces the id, -1 removes the symbol; ids outside
    [0, V) pass through); confusion: a caller-owned (V+1, V+1) int64 device tensor that is ACCUMULATED into (row V insertions, column V
    deletions).  V = num_classes, else the length of class_map, else confusion.shape[0] - 1.  Takes what edit_distance takes; everything
    stays on the device, no host sync."""
    _need_gpu(ids)
    dev = ids.device
    if ids.dtype != torch.int32 or not ids.is_contiguous():
        ids = ids.to(torch.int32).contiguous()
    ids_len = ids_len.to(device=dev, dtype=torch.int32).contiguous()
    targets = targets.to(device=dev, dtype=torch.int64).contiguous()
    tgt_len = tgt_len.to(device=dev, dtype=torch.int64).contiguous()
    B = ids.shape[0]
    if ids.dim() != 2 or targets.dim() != 2 or targets.shape[0] != B or tgt_len.numel() != B or ids_len.numel() != B:
        raise ValueError("ctc_pytorch_amd.edit_ops: expected ids (B,T), ids_len (B), targets (B,Lmax), tgt_len (B)")
    V = num_classes
    if class_map is not None:
        class_map = torch.as_tensor(class_map).to(device=dev, dtype=torch.int32).contiguous()
        V = class_map.numel() if V is None else V
        if class_map.dim() != 1 or class_map.numel() != V:
            raise ValueError("ctc_pytorch_amd.edit_ops: class_map must hold num_classes = %s entries, got %s" % (V, tuple(class_map.shape)))
    if confusion is not None:
        V = confusion.shape[0] - 1 if V is None else V
        if confusion.dtype != torch.int64 or confusion.device != dev or not confusion.is_contiguous() or tuple(confusion.shape) != (V + 1, V + 1):
            raise ValueError("ctc_pytorch_amd.edit_ops: confusion must be a contiguous int64 (V+1, V+1) tensor on %s with V = %s" % (dev, V))
    V = 0 if V is None else int(V)
    if (class_map is not None or confusion is not None) and V <= 0:
        raise ValueError("ctc_pytorch_amd.edit_ops: num_classes must be positive, got %d" % V)
    L = _lib.lib()
    lda, ldb = ids.shape[1], targets.shape[1]
    counts = torch.empty((B, 6), dtype=torch.int32, device=dev)
    ali = torch.empty((B, lda + ldb, 2), dtype=torch.int32, device=dev) if alignment else None
    ali_len = torch.empty(B, dtype=torch.int32, device=dev) if alignment else None
    need = L.ctcn_edit_ops_ws_bytes(B, lda, max(ldb, 1))
    # move bits that do not fit in LDS: a buffer of this call's own (stream-ordered, as in ctc_forced_align)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    _lib.check(L.ctcn_edit_ops(_ptr(ids), _ptr(ids_len), _ptr(targets), _ptr(tgt_len), _ptr(class_map), V, _ptr(counts), _ptr(ali),
                               _ptr(ali_len), _ptr(confusion), B, lda, ldb, max(ldb, 1), _ptr(ws), need, _lib.stream_ptr()), "edit_ops")
    return EditOps(counts, ali, ali_len)


def step_stats(loss, dist, tgt_len):
    """(loss, sum(dist), sum(tgt_len), hand-off status word) as a float64 device tensor of 4 -- one launch (ctcn_step_stats)."""
    _need_gpu(loss, dist, tgt_len)
    dev = loss.device
    l32 = loss.detach().reshape(-1)[:1].to(torch.float32).contiguous()
    dist = dist.to(dtype=torch.int32).contiguous()
    tgt_len = tgt_len.to(device=dev, dtype=torch.int64).contiguous()
    out = torch.empty(4, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().ctcn_step_stats(_ptr(l32), _ptr(dist), _ptr(tgt_len), dist.numel(), _ptr(_lib.status_word(dev)), _ptr(out),
                                          _lib.stream_ptr()), "step_stats")
    return out


BEAM_PLAN_FIELDS = ("path", "ok", "npt", "lm_lds", "trie_slots", "lds", "threads", "wcap", "smax", "cand_in_lds", "lm_in_lds", "generic_lds",
                    "generic_fits", "max_nodes", "ht_size")


def beam_plan(T, B, V, W, lds_max=160 * 1024, generic_static_lds=0, lm_order=2):
    """ctcn_diag_beam_plan as a dict: the path ctcn_beam_decode takes under the current options (0 fast, 1 fast occ2, 2 generic), the fast
    kernel's fit (ok, npt, lm_lds, trie_slots, lds), the generic kernel's plan, the two workspace totals and rc (0, or -3 = CTCN_EUNSUPPORTED
    where the decode call answers that).  lm_order = 3: the plan of a search with a (V+1)^3 table (ctcn_diag_beam_plan_lm).  Pure
    arithmetic: no device needed."""
    out = (ctypes.c_int * 19)()
    if lm_order == 2:
        rc = _lib.lib().ctcn_diag_beam_plan(int(T), int(B), int(V), int(W), int(lds_max), int(generic_static_lds), ctypes.cast(out, ctypes.c_void_p))
    else:
        rc = _lib.lib().ctcn_diag_beam_plan_lm(int(T), int(B), int(V), int(W), int(lm_order), int(lds_max), int(generic_static_lds),
                                               ctypes.cast(out, ctypes.c_void_p))
    if rc not in (0, -3):
        _lib.check(rc, "diag_beam_plan")
    d = dict(zip(BEAM_PLAN_FIELDS, out))
    d.update(ws_fast=out[15] | (out[16] << 31), ws_generic=out[17] | (out[18] << 31), rc=rc)
    return d


CTC_LATTICE_PLAN_FIELDS = ("skewed", "waves", "ns", "threads", "lds", "skew")


def ctc_lattice_plan(Lmax):
    """ctcn_diag_ctc_lattice_plan as a dict: the launch of a CTC lattice pass over label rows of Lmax symbols under the current
    `ctc_lattice_skew` (skewed or classic kernel, waves of 64 states that cover the lattice, states per thread, threads, dynamic LDS bytes, and
    the skewed kernel's skew in frames per wave).  Pure arithmetic: no device needed."""
    out = (ctypes.c_int * 6)()
    _lib.check(_lib.lib().ctcn_diag_ctc_lattice_plan(int(Lmax), ctypes.cast(out, ctypes.c_void_p)), "diag_ctc_lattice_plan")
    return dict(zip(CTC_LATTICE_PLAN_FIELDS, out))


def _lm_order(lm_table, V):
    """Order of the search's LM from the rank of its table: 2 for (V+1)^2 (any shape of that many elements, as ever), 3 for a 3-D table,
    which must be (V+1, V+1, V+1).  Looks at the shape alone: a wrong table is a ValueError before anything is uploaded or launched."""
    shape = tuple(lm_table.shape) if hasattr(lm_table, "shape") else np.shape(lm_table)
    if len(shape) != 3:
        return 2
    if shape != (V + 1,) * 3:
        raise ValueError("a 3-D lm table must be (V+1, V+1, V+1) = %s, got %s" % ((V + 1,) * 3, shape))
    return 3


def beam_decode_device(x_tbv, lens, lm_table, alpha, beam_width, blank=0, input_is_prob=False):
    """Enqueue the prefix beam search (ctcn_beam_decode) on the current stream; returns DEVICE tensors
    (out_ids (B,T) int32, out_len (B) int32, score (B) float64, status (B) int32) without synchronising.
    lm_table: (V+1, V+1) = a bigram LM, or (V+1, V+1, V+1) = a trigram LM (ctcn_beam_decode_lm, order 3)."""
    order = _lm_order(lm_table, x_tbv.shape[-1])
    _need_gpu(x_tbv)
    x = _f32c(x_tbv.detach())
    T, B, V = x.shape
    dev = x.device
    if torch.is_tensor(lens) and lens.is_cuda:
        lens_t = lens.to(dtype=torch.int32).contiguous()
    else:       # through pinned memory: a pageable upload would make the host wait for everything queued on this stream before it
        lens_h = torch.as_tensor(lens, dtype=torch.int32).contiguous().pin_memory()
        lens_t = lens_h.to(dev, non_blocking=True)
    lm = torch.as_tensor(lm_table, dtype=torch.float64, device=dev).contiguous()
    if order == 2 and lm.numel() != (V + 1) * (V + 1):
        raise ValueError("lm table must be (V+1)x(V+1)")
    L = _lib.lib()
    nb = L.ctcn_beam_ws_bytes(T, B, V, int(beam_width))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    # one zeroed buffer for the four results (one fill, one copy to the host): score | ids | lengths | status
    out = torch.zeros(B * (8 + 4 * T + 4 + 4), dtype=torch.uint8, device=dev)
    score = out[: 8 * B].view(torch.float64)
    out_ids = out[8 * B: 8 * B + 4 * B * T].view(torch.int32).view(B, T)
    out_len = out[8 * B + 4 * B * T: 8 * B + 4 * B * T + 4 * B].view(torch.int32)
    status = out[8 * B + 4 * B * T + 4 * B:].view(torch.int32)
    if order == 3:
        _lib.check(L.ctcn_beam_decode_lm(_ptr(x), int(bool(input_is_prob)), _ptr(lens_t), _ptr(lm), 3, float(alpha), int(beam_width), int(blank), 1,
                                         _ptr(out_ids), _ptr(out_len), _ptr(score), None, _ptr(status), T, B, V, _ptr(ws), ws.numel(),
                                         _lib.stream_ptr()), "beam_decode_lm")
        return out_ids, out_len, score, status
    _lib.check(L.ctcn_beam_decode(_ptr(x), int(bool(input_is_prob)), _ptr(lens_t), _ptr(lm), float(alpha), int(beam_width), int(blank),
                                  _ptr(out_ids), _ptr(out_len), _ptr(score), _ptr(status), T, B, V, _ptr(ws), ws.numel(),
                                  _lib.stream_ptr()), "beam_decode")
    return out_ids, out_len, score, status


_vocab_cache = {}


def _vocabulary(words):
    """(UTF-8 bytes of the words back to back + 17 pad bytes, int32 byte offsets (V), int32 byte lengths (V; -1 = the vocabulary has no such
    id: ctcn_join_tokens reports it as the KeyError it is in Python), longest word in bytes, V) for a list or an {id: word} mapping.
    Cached per object; a hit is confirmed by CONTENT (a list or dict edited in place -- a replaced phone symbol, a remapped space index --
    must not return the stale blob), which costs one tuple comparison per decoded batch."""
    key = id(words)
    snap = tuple(words.items()) if isinstance(words, dict) else tuple(words)
    hit = _vocab_cache.get(key)
    if hit is not None and hit[0] is words and hit[1] == snap:
        return hit[2]
    if isinstance(words, dict):
        V = (max(words) + 1) if words else 1
        get = words.get
    else:
        n = len(words)
        V = max(n, 1)
        get = lambda k: words[k] if k < n else None
    blob, off, ln, longest = bytearray(), np.zeros(V, dtype=np.int32), np.full(V, -1, dtype=np.int32), 0
    for k in range(V):
        w = get(k)
        off[k] = len(blob)
        if w is None:
            continue
        b = str(w).encode("utf-8")
        blob += b
        ln[k] = len(b)
        longest = max(longest, len(b))
    voc = (bytes(blob) + b"\0" * 17, off, ln, longest, V)       # (ctcn_join_tokens moves 16 bytes per short word)
    if len(_vocab_cache) > 16:
        _vocab_cache.clear()
    _vocab_cache[key] = (words, snap, voc)
    return voc


def join_tokens(ids, lens, words, sep=" "):
    """[sep.join(words[k] for k in ids[b, :lens[b]]) for b in range(B)] in one pass of native host code (ctcn_join_tokens, hostjoin.hip):
    ids (B, T) int32 numpy array (C-contiguous rows), lens (B,) int32, words a list or {id: word} mapping, sep '' or one ASCII character.
    The interpreter's join over a decoded batch (cfg5, flat posteriors: 72 k tokens) is 2.3 ms, this is ~0.15 ms."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    if ids.ndim != 2 or lens.shape != (ids.shape[0],):
        raise ValueError("join_tokens: ids must be (B, T) and lens (B,)")
    if len(sep) > 1 or (sep and ord(sep) > 127):
        raise ValueError("join_tokens: sep must be '' or one ASCII character")
    B, T = ids.shape
    blob, off, ln, longest, V = _vocabulary(words)
    total = int(np.minimum(lens, T).clip(min=0).sum())
    cap = total * (longest + 1) + 32
    out = np.empty(cap, dtype=np.uint8)
    out_off = np.empty(B + 1, dtype=np.int64)
    n = _lib.lib().ctcn_join_tokens(ids.ctypes.data, T, lens.ctypes.data, B, blob, off.ctypes.data, ln.ctypes.data, V, ord(sep) if sep else 0,
                                    out.ctypes.data, cap, out_off.ctypes.data)
    if n <= -16:
        k = -(n + 16)
        if isinstance(words, dict):
            raise KeyError(k)
        raise IndexError("list index out of range")
    if n < 0:
        raise RuntimeError("ctcn_join_tokens failed (%d)" % n)
    o = out_off.tolist()
    buf = out[:n].tobytes()
    if buf.isascii():                        # one decode, then slices (byte offsets = character offsets)
        whole = buf.decode("ascii")
        return [whole[o[b]:o[b + 1]] for b in range(B)]
    return [buf[o[b]:o[b + 1]].decode("utf-8") for b in range(B)]


class BeamResult(object):
    """Handle of a prefix beam search enqueued on the current stream (beam_decode_async): the device results are copied into pinned host
    memory behind the search, `result()` waits for that copy alone -- other streams keep running -- and returns what beam_decode returns."""

    def __init__(self, dev_out):
        out_ids, out_len, score, status = dev_out
        B, T = out_ids.shape
        whole = score._base if score._base is not None else None        # the four are views of one buffer (beam_decode_device)
        if whole is None or whole.numel() != B * (8 + 4 * T + 8):
            whole = torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in (score, out_ids, out_len, status)])
        self._host = torch.empty(whole.shape, dtype=torch.uint8, pin_memory=True)
        self._host.copy_(whole, non_blocking=True)
        self._dims = (B, T)
        self._keep = (whole, dev_out)                # the device tensors stay alive until the copy has run
        self._event = torch.cuda.Event()
        self._event.record(torch.cuda.current_stream(out_ids.device))

    def result(self):
        self._event.synchronize()
        self._keep = None
        B, T = self._dims
        h = self._host.numpy()
        score = h[: 8 * B].view(np.float64)
        ids_c = h[8 * B: 8 * B + 4 * B * T].view(np.int32).reshape(B, T)
        len_c = h[8 * B + 4 * B * T: 8 * B + 4 * B * T + 4 * B].view(np.int32)
        status = h[8 * B + 4 * B * T + 4 * B:].view(np.int32)
        return [ids_c[b, : len_c[b]].tolist() for b in range(B)], score.copy(), status.copy()

    def strings(self, words, sep=" "):
        """(strings, scores, status) with strings[b] = sep.join(words[k] for k in labelling b), assembled by join_tokens straight from the
        pinned result buffer (no per-utterance id lists)."""
        self._event.synchronize()
        self._keep = None
        B, T = self._dims
        h = self._host.numpy()
        score = h[: 8 * B].view(np.float64)
        ids_c = h[8 * B: 8 * B + 4 * B * T].view(np.int32).reshape(B, T)
        len_c = h[8 * B + 4 * B * T: 8 * B + 4 * B * T + 4 * B].view(np.int32)
        status = h[8 * B + 4 * B * T + 4 * B:].view(np.int32)
        if status.any():            # a search that reported an error owes no consistent labelling: its rows join as '' and the caller raises from `status`
            len_c = np.where(status != 0, 0, len_c).astype(np.int32)
        return join_tokens(ids_c, len_c, words, sep), score.copy(), status.copy()


def beam_decode_async(x_tbv, lens, lm_table, alpha, beam_width, blank=0, input_is_prob=False):
    """beam_decode without the host synchronisation: enqueues the search on the CURRENT stream and returns a BeamResult.  Two searches
    enqueued on two streams run side by side (a 128-utterance batch is 128 workgroups, half of the device's CUs); `lm_table` may be a
    device tensor (it is uploaded per call otherwise)."""
    return BeamResult(beam_decode_device(x_tbv, lens, lm_table, alpha, beam_width, blank, input_is_prob))


def beam_decode(x_tbv, lens, lm_table, alpha, beam_width, blank=0, input_is_prob=False):
    """x (T,B,V) float32 device tensor (log-probs, or probabilities if input_is_prob); returns CPU
    (ids list-of-lists, scores (B,) float64, status (B,) int32).  Synchronises (host result)."""
    out_ids, out_len, score, status = beam_decode_device(x_tbv, lens, lm_table, alpha, beam_width, blank, input_is_prob)
    B = out_ids.shape[0]
    ids_c, len_c = out_ids.cpu().numpy(), out_len.cpu().numpy()
    return [list(map(int, ids_c[b, : len_c[b]])) for b in range(B)], score.cpu().numpy(), status.cpu().numpy()


def beam_decode_nbest_device(x_tbv, lens, lm_table, alpha, beam_width, nbest, blank=0, input_is_prob=False):
    """Enqueue the n-best prefix beam search (ctcn_beam_decode_nbest / ctcn_beam_decode_lm) on the current stream; returns DEVICE tensors
    (out_ids (B,nbest,T) int32, out_len (B,nbest) int32, score (B,nbest) float64, count (B) int32, status (B) int32) without synchronising:
    what rescore_nbest takes."""
    order = _lm_order(lm_table, x_tbv.shape[-1])
    _need_gpu(x_tbv)
    x = _f32c(x_tbv.detach())
    T, B, V = x.shape
    dev = x.device
    nbest = int(nbest)
    if not 1 <= nbest <= int(beam_width):
        raise ValueError("nbest must lie in [1, beam_width]")
    lens_t = lens.to(device=dev, dtype=torch.int32).contiguous() if torch.is_tensor(lens) else torch.as_tensor(lens, dtype=torch.int32).to(dev)
    lm = torch.as_tensor(lm_table, dtype=torch.float64, device=dev).contiguous()
    if order == 2 and lm.numel() != (V + 1) * (V + 1):
        raise ValueError("lm table must be (V+1)x(V+1)")
    L = _lib.lib()
    ws = torch.empty(max(L.ctcn_beam_ws_bytes(T, B, V, int(beam_width)), 1), dtype=torch.uint8, device=dev)
    out_ids = torch.zeros((B, nbest, T), dtype=torch.int32, device=dev)
    out_len = torch.zeros((B, nbest), dtype=torch.int32, device=dev)
    score = torch.zeros((B, nbest), dtype=torch.float64, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    if order == 3:
        _lib.check(L.ctcn_beam_decode_lm(_ptr(x), int(bool(input_is_prob)), _ptr(lens_t), _ptr(lm), 3, float(alpha), int(beam_width), int(blank), nbest,
                                         _ptr(out_ids), _ptr(out_len), _ptr(score), _ptr(count), _ptr(status), T, B, V, _ptr(ws), ws.numel(),
                                         _lib.stream_ptr()), "beam_decode_lm")
    else:
        _lib.check(L.ctcn_beam_decode_nbest(_ptr(x), int(bool(input_is_prob)), _ptr(lens_t), _ptr(lm), float(alpha), int(beam_width), int(blank), nbest,
                                            _ptr(out_ids), _ptr(out_len), _ptr(score), _ptr(count), _ptr(status), T, B, V, _ptr(ws), ws.numel(),
                                            _lib.stream_ptr()), "beam_decode_nbest")
    return out_ids, out_len, score, count, status


def beam_decode_nbest(x_tbv, lens, lm_table, alpha, beam_width, nbest, blank=0, input_is_prob=False):
    """The `nbest` best labellings of every utterance (ctcn_beam_decode_nbest: the first nbest entries of the reference's final `last.sort()`,
    BeamSearch.py:150 keeps [0]).  Returns CPU (ids: per utterance a list of up to nbest label lists, best first; scores (B, nbest) float64,
    0 past the labellings returned; status (B,) int32).  Synchronises."""
    out_ids, out_len, score, count, status = beam_decode_nbest_device(x_tbv, lens, lm_table, alpha, beam_width, nbest, blank, input_is_prob)
    B = out_ids.shape[0]
    ids_c, len_c, cnt = out_ids.cpu().numpy(), out_len.cpu().numpy(), count.cpu().numpy()
    ids = [[list(map(int, ids_c[b, k, : len_c[b, k]])) for k in range(cnt[b])] for b in range(B)]
    return ids, score.cpu().numpy(), status.cpu().numpy()


# --------------------------------------------------------------------------------------------------
# RNN language model: embedding, cross-entropy over log-probs, n-best rescoring (lm.hip)
# --------------------------------------------------------------------------------------------------
LM_BAD_ID, LM_BAD_TARGET = 1, 2            # bits of the status word of the kernels of lm.hip
_LM_STATUS = {}


def lm_status(device):
    """Per-device sticky int32 the kernels of lm.hip OR their bits into (0: every id and target was in range)."""
    key = (device.type, device.index)
    t = _LM_STATUS.get(key)
    if t is None:
        t = _LM_STATUS[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return t


def check_lm_status(device, value=None):
    """Raise IndexError if an embedding id or a loss target was out of range since the last check.  Synchronises (one small read) unless
    `value`, the word as the caller has already read it, is given; callers that read results anyway call it there."""
    t = _LM_STATUS.get((device.type, device.index))
    if t is None:
        return
    v = int(t.item()) if value is None else int(value)
    if v:
        t.zero_()
        what = [w for bit, w in ((LM_BAD_ID, "an embedding id outside [0, num_embeddings)"), (LM_BAD_TARGET, "a target outside [0, C)")) if v & bit]
        raise IndexError("ctc_pytorch_amd: %s reached the device (its row was treated as zeros)" % " and ".join(what))


def check_token_ids(host, V, what="ids", also=()):
    """Host-resident ids are validated before they are uploaded, as check_frame_lengths does for lengths: ValueError for an id outside
    [0, V) that is none of `also` (an ignore_index)."""
    if host.size:
        bad = (host < 0) | (host >= V)
        for a in also:
            bad &= host != a
        if bad.any():
            raise ValueError("%s: %d lies outside [0, %d)" % (what, int(host[bad][0]), V))


def token_ids(ids, V, device, what="ids", also=()):
    """`ids` (integer tensor on the host or the device, array or nested list) as the int32 device tensor the kernels read, shape kept.
    Host-resident ids are checked (check_token_ids) and go up in one copy; a device tensor is taken as it is -- the kernels check every id
    themselves and report through lm_status."""
    if torch.is_tensor(ids):
        if ids.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8, torch.int8):
            raise ValueError("%s: expected an integer tensor, got %s" % (what, ids.dtype))
        if ids.is_cuda:
            return ids if ids.dtype == torch.int32 and ids.is_contiguous() else ids.to(torch.int32).contiguous()
        host = ids.detach().numpy().astype(np.int64)
    else:
        host = np.asarray(ids)
        if host.dtype.kind not in "iu":
            raise ValueError("%s: expected integers" % what)
        host = host.astype(np.int64)
    check_token_ids(host, V, what, also)
    return torch.from_numpy(np.ascontiguousarray(host.astype(np.int32))).to(device, non_blocking=True)


class _Embedding(torch.autograd.Function):
    """y = table[ids] (nn.Embedding); the backward is a deterministic scatter-add: per table row the float32 sum of its dy rows in ascending
    position (ctcn_embedding_bwd), into the FlatAdam gradient view with beta = 1 where the table lives in one."""

    @staticmethod
    def forward(ctx, ids, table, padding_idx):
        _need_gpu(ids, table)
        ctx.gw_view = _gview(table)
        table = _f32c(table)
        V, E = table.shape
        N = ids.numel()
        y = torch.empty(tuple(ids.shape) + (E,), dtype=torch.float32, device=table.device)
        if N:
            _lib.check(_lib.lib().ctcn_embedding_fwd(_ptr(ids), _ptr(table), _ptr(y), N, V, E, padding_idx, _ptr(lm_status(table.device)),
                                                     _lib.stream_ptr()), "embedding_fwd")
        ctx.save_for_backward(ids)
        ctx.dims = (N, V, E, padding_idx)
        return y

    @staticmethod
    def backward(ctx, gy):
        (ids,) = ctx.saved_tensors
        N, V, E, padding_idx = ctx.dims
        if not ctx.needs_input_grad[1]:
            return None, None, None
        L = _lib.lib()
        into = ctx.gw_view
        gw = None
        if into is None:
            into = gw = torch.empty((V, E), dtype=torch.float32, device=gy.device)
        if N == 0:
            if gw is not None:
                gw.zero_()
            return None, gw, None
        gy = _f32c(gy)
        ws = torch.empty(max(L.ctcn_embedding_bwd_ws_bytes(N, V), 4), dtype=torch.uint8, device=gy.device)
        _lib.check(L.ctcn_embedding_bwd(_ptr(ids), _ptr(gy), _ptr(into), N, V, E, padding_idx, 0.0 if gw is not None else 1.0, _ptr(ws), ws.numel(),
                                        _lib.stream_ptr()), "embedding_bwd")
        return None, gw, None


def embedding(ids, table, padding_idx=None):
    """torch.nn.functional.embedding(ids, table, padding_idx) on the HIP kernels: ids of any shape (host ids are validated and uploaded, device
    ids are checked by the kernel: a bad id gives a row of zeros and check_lm_status raises), table (V, E) float32 on the device."""
    _need_gpu(table)
    V = table.shape[0]
    if padding_idx is None:
        pad = -1
    else:
        pad = int(padding_idx) + (V if int(padding_idx) < 0 else 0)
        if not 0 <= pad < V:
            raise ValueError("padding_idx must lie within num_embeddings")
    return _Embedding.apply(token_ids(ids, V, table.device, "embedding ids"), table, pad)


_XENT_REDUCTIONS = ("none", "sum", "mean")


def _nll(lp, tgt, T, B, V, ignore_index):
    """ctcn_nll_fwd on (T*B, V) log-probs: (tok (T*B) float32, seq_sum (B) float64, total 0-d float64, count 0-d int32) on the device."""
    dev = lp.device
    tok = torch.empty(T * B, dtype=torch.float32, device=dev)
    sums = torch.empty(B + 1, dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().ctcn_nll_fwd(_ptr(lp), _ptr(tgt), T, B, V, int(ignore_index), _ptr(tok), _ptr(sums), _ptr(sums[B:]), _ptr(count),
                                       _ptr(lm_status(dev)), _lib.stream_ptr()), "nll_fwd")
    return tok, sums[:B], sums[B], count


class _CrossEntropy(torch.autograd.Function):
    """F.cross_entropy over the last axis: ctcn_log_softmax_fwd + ctcn_nll_fwd forward, ctcn_xent_bwd backward (one read of the saved
    log-probs, one write of dz; the upstream gradient and the 'mean' count are read on the device)."""

    @staticmethod
    def forward(ctx, z, tgt, ignore_index, reduction):
        V = z.shape[-1]
        N = z.numel() // V
        lp = torch.empty_like(z)
        _lib.check(_lib.lib().ctcn_log_softmax_fwd(_ptr(z), _ptr(lp), None, N, V, _lib.stream_ptr()), "log_softmax_fwd")
        tok, _, total, count = _nll(lp, tgt, N, 1, V, ignore_index)
        ctx.save_for_backward(lp, tgt, count)
        ctx.conf = (N, V, ignore_index, reduction)
        if reduction == "none":
            return tok.view(tgt.shape)
        if reduction == "sum":
            return total.to(torch.float32)
        return (total / count[0].clamp(min=1)).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        lp, tgt, count = ctx.saved_tensors
        N, V, ignore_index, reduction = ctx.conf
        g = _f32c(g)
        dz = torch.empty_like(lp)
        _lib.check(_lib.lib().ctcn_xent_bwd(_ptr(lp), _ptr(tgt), _ptr(dz), N, V, ignore_index, _ptr(g), 1 if reduction == "none" else 0,
                                            _ptr(count) if reduction == "mean" else None, _lib.stream_ptr()), "xent_bwd")
        return dz, None, None, None


def cross_entropy(logits, target, ignore_index=-100, reduction="mean"):
    """Cross-entropy of `logits` (..., V), classes on the LAST axis, against integer `target` (...): 'none' gives the per-row losses in
    target's shape, 'sum' their float64 sum in ascending row order, 'mean' that sum over the rows not ignored (at least 1), both returned
    as float32 scalars.  Rows whose target is ignore_index cost 0 and get a zero gradient."""
    if reduction not in _XENT_REDUCTIONS:
        raise ValueError("%s is not a valid value for reduction" % (reduction,))
    _need_gpu(logits)
    z = _f32c(logits)
    if z.dim() < 1 or z.shape[-1] < 1 or z.numel() == 0:
        raise ValueError("cross_entropy: logits must be (..., V) with at least one row")
    tgt = token_ids(target, z.shape[-1], z.device, "cross_entropy target", also=(int(ignore_index),))
    if tuple(tgt.shape) != tuple(z.shape[:-1]):
        raise ValueError("cross_entropy: target %s does not match logits %s" % (tuple(tgt.shape), tuple(z.shape)))
    return _CrossEntropy.apply(z, tgt, int(ignore_index), reduction)


def sequence_log_prob(logits_tbv, targets_tb, ignore_index=-100):
    """ln P of every sequence of a time-major batch: (B) float64 = - sum over t (ascending, float64) of the float32 token losses of
    `targets_tb` (T, B) under log_softmax(logits_tbv (T, B, V)); steps whose target is ignore_index add nothing.  No gradient."""
    _need_gpu(logits_tbv)
    z = _f32c(logits_tbv.detach())
    if z.dim() != 3:
        raise ValueError("sequence_log_prob: logits must be (T, B, V)")
    T, B, V = z.shape
    tgt = token_ids(targets_tb, V, z.device, "sequence_log_prob targets", also=(int(ignore_index),))
    if tuple(tgt.shape) != (T, B):
        raise ValueError("sequence_log_prob: targets %s do not match logits %s" % (tuple(tgt.shape), tuple(z.shape)))
    lp = torch.empty_like(z)
    _lib.check(_lib.lib().ctcn_log_softmax_fwd(_ptr(z), _ptr(lp), None, T * B, V, _lib.stream_ptr()), "log_softmax_fwd")
    return -_nll(lp, tgt, T, B, V, ignore_index)[1]


def pack_nbest(out_ids, out_len, count, L, boundary=0, ignore_index=-100):
    """ctcn_lm_pack_nbest: the n-best search's (B,N,T) ids, (B,N) lengths and (B) counts as the LM's time-major batch of B*N sequences of
    L + 1 steps (L: the longest labelling): (in_ids (L+1, B*N), targets (L+1, B*N), lens (B*N)), int32 on the device."""
    _need_gpu(out_ids, out_len, count)
    B, N, T = out_ids.shape
    L = int(L)
    dev = out_ids.device
    in_ids = torch.empty((L + 1, B * N), dtype=torch.int32, device=dev)
    tgt = torch.empty((L + 1, B * N), dtype=torch.int32, device=dev)
    lens = torch.empty(B * N, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().ctcn_lm_pack_nbest(_ptr(out_ids), _ptr(out_len), _ptr(count), B, N, T, L, int(boundary), int(ignore_index), _ptr(in_ids),
                                             _ptr(tgt), _ptr(lens), _lib.stream_ptr()), "lm_pack_nbest")
    return in_ids, tgt, lens


RescoredBest = collections.namedtuple("RescoredBest", "ids lengths score k lm")


def rescore_select(score, lm, out_len, count, out_ids, weight, len_bonus=0.0):
    """ctcn_rescore_select: per utterance the entry k < count[b] with the largest (score + weight * lm) + len_bonus * length (float64,
    lowest k on ties) -> (best_ids (B,T), best_len (B), best_score (B) float64, best_k (B)) on the device."""
    _need_gpu(score, lm, out_len, count, out_ids)
    B, N, T = out_ids.shape
    dev = out_ids.device
    best_ids = torch.empty((B, T), dtype=torch.int32, device=dev)
    best_len = torch.empty(B, dtype=torch.int32, device=dev)
    best_score = torch.empty(B, dtype=torch.float64, device=dev)
    best_k = torch.empty(B, dtype=torch.int32, device=dev)
    lm = lm.to(torch.float64).contiguous()
    _lib.check(_lib.lib().ctcn_rescore_select(_ptr(score), _ptr(lm), _ptr(out_len), _ptr(count), _ptr(out_ids), float(weight), float(len_bonus), B, N, T,
                                              _ptr(best_ids), _ptr(best_len), _ptr(best_score), _ptr(best_k), _lib.stream_ptr()), "rescore_select")
    return best_ids, best_len, best_score, best_k


def rescore_nbest(nbest, scorer, weight, len_bonus=0.0, L=None, boundary=0, ignore_index=-100):
    """N-best rescoring on the device: `nbest` = the five tensors of beam_decode_nbest_device, `scorer(in_ids, targets, lens)` -> (B*N)
    float64 ln P of every packed sequence (RNNLM.score_packed).  L: the longest labelling if the caller has read it already, else it is
    read here (one small read).  Returns RescoredBest(ids (B,T), lengths (B), score (B) float64, k (B), lm (B,N) float64)."""
    out_ids, out_len, score, count, _ = nbest
    B, N, T = out_ids.shape
    if L is None:
        L = int(out_len.max())
    in_ids, tgt, lens = pack_nbest(out_ids, out_len, count, min(int(L), T), boundary, ignore_index)
    lm = scorer(in_ids, tgt, lens).view(B, N)
    return RescoredBest(*rescore_select(score, lm, out_len, count, out_ids, weight, len_bonus), lm)


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    _need_gpu(p, g, m, v)
    _lib.check(_lib.lib().ctcn_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), float(lr), float(beta1), float(beta2),
                                         float(eps), float(weight_decay), int(step), _lib.stream_ptr()), "adam_step")


# --------------------------------------------------------------------------------------------------
# gradient-norm clipping and the non-finite-step guard (ctcn_grad_norm / ctcn_clip_control / ctcn_adam_step_ex, include/ctcn.h)
# --------------------------------------------------------------------------------------------------
# words of a ctcn_clip_ctl held as an int32 tensor of 8 (the float fields are read through .view(torch.float32))
CTL_NORM, CTL_NONFINITE, CTL_COEF, CTL_APPLY, CTL_STEP, CTL_SKIPPED, CTL_STEP_SIZE, CTL_SQRT_BC2 = range(8)


def norm_type_code(norm_type):
    """CTCN_NORM_L2 / CTCN_NORM_INF for the two norms the kernels compute; anything else raises NotImplementedError."""
    try:
        nt = float(norm_type)
    except (TypeError, ValueError):
        nt = None
    if nt == 2.0:
        return 2
    if nt == float("inf"):
        return 0
    raise NotImplementedError("ctc_pytorch_amd: norm_type %r -- the gradient-norm kernels compute norm_type 2 and inf" % (norm_type,))


def new_clip_ctl(device, step=0):
    """A zeroed device control block (ctcn_clip_ctl) with the step count `step`."""
    ctl = torch.zeros(8, dtype=torch.int32, device=device)
    if step:
        ctl[CTL_STEP] = int(step)
    return ctl


def _flat_f32(t, what):
    _need_gpu(t)
    if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
        raise TypeError("ctc_pytorch_amd.%s: expected one contiguous 1-D float32 buffer" % what)
    return t


def grad_norm(flat, norm_type=2.0, segments=None, ctl=None, ws=None, blocks=0):
    """Norm (2 or inf) of the 1-D float32 device buffer `flat` as a 0-d device tensor, without a host sync; a function of the buffer's bits
    alone (ctcn_grad_norm).  `segments`: offsets [o_0, ..., o_k] (list, or an int64 device tensor) -> returns (total, per-segment norms (k)).
    `ctl`: a control block (new_clip_ctl) to write total_norm / nonfinite into -- the result is then a view of it; `ws`: a caller-kept
    workspace (uint8 device tensor); `blocks`: force the grid (tests: the result must not move)."""
    flat = _flat_f32(flat, "grad_norm")
    code, dev, L = norm_type_code(norm_type), flat.device, _lib.lib()
    seg_t = seg_norms = None
    nseg = 0
    if segments is not None:
        seg_t = segments if torch.is_tensor(segments) else torch.tensor([int(o) for o in segments], dtype=torch.int64)
        seg_t = seg_t.to(device=dev, dtype=torch.int64).contiguous()
        nseg = int(seg_t.numel()) - 1
        if nseg < 1:
            raise ValueError("ctc_pytorch_amd.grad_norm: segments needs at least two offsets")
        seg_norms = torch.empty(nseg, dtype=torch.float32, device=dev)
    need = int(L.ctcn_grad_norm_ws_bytes(flat.numel(), nseg))
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    if ctl is None:
        ctl = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.check(L.ctcn_grad_norm(_ptr(flat), flat.numel(), code, _ptr(seg_t), nseg, _ptr(seg_norms), ctypes.c_void_p(ctl.data_ptr()),
                                ctypes.c_void_p(ctl.data_ptr() + 4), int(blocks), _ptr(ws), ws.numel(), _lib.stream_ptr()), "grad_norm")
    total = ctl.view(torch.float32)[CTL_NORM]
    return total if segments is None else (total, seg_norms)


def clip_control(ctl, max_norm, lr=0.0, beta1=0.9, beta2=0.999, skip_nonfinite=False):
    """clip_coef, apply and the step bookkeeping of a control block whose total_norm / nonfinite ctcn_grad_norm has just written (ctcn_clip_control)."""
    _need_gpu(ctl)
    _lib.check(_lib.lib().ctcn_clip_control(_ptr(ctl), float(max_norm), float(lr), float(beta1), float(beta2), int(bool(skip_nonfinite)),
                                            _lib.stream_ptr()), "clip_control")


def clip_grad_norm_(flat, max_norm, norm_type=2.0, error_if_nonfinite=False, ctl=None):
    """torch.nn.utils.clip_grad_norm_ over one flat float32 gradient buffer: returns the pre-clip norm (0-d device tensor) and scales `flat`
    in place by min(1, max_norm / (norm + 1e-6)); a non-finite norm gives a NaN coefficient that poisons the gradients, as in torch, unless
    error_if_nonfinite (which reads the flag back: the only host sync here).  The caller joins the side stream (FlatAdam.clip_grad_norm_ and
    nn.utils.clip_grad_norm_ do).  `ctl`: a scratch control block of the caller's (new_clip_ctl), which then holds the coefficient used."""
    flat = _flat_f32(flat, "clip_grad_norm_")
    if not float(max_norm) > 0.0:
        raise ValueError("ctc_pytorch_amd.clip_grad_norm_: max_norm must be > 0, got %r" % (max_norm,))
    ctl = new_clip_ctl(flat.device) if ctl is None else ctl
    total = grad_norm(flat, norm_type, ctl=ctl)
    if error_if_nonfinite and int(ctl[CTL_NONFINITE].item()):
        raise RuntimeError("The total norm of order %s for gradients from `parameters` is non-finite, so it cannot be clipped. To disable this "
                           "error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`" % (float(norm_type),))
    clip_control(ctl, max_norm)
    _lib.check(_lib.lib().ctcn_scale_by_device_scalar(_ptr(flat), flat.numel(), ctypes.c_void_p(ctl.data_ptr() + 4 * CTL_COEF),
                                                      _lib.stream_ptr()), "scale_by_device_scalar")
    return total


def adam_step_ex(p, g, m, v, beta1, beta2, eps, weight_decay, ctl):
    """adam_step with the clip coefficient, the bias-corrected step size and the apply flag read from the device control block (ctcn_adam_step_ex);
    `g` is not written."""
    _need_gpu(p, g, m, v, ctl)
    _lib.check(_lib.lib().ctcn_adam_step_ex(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), float(beta1), float(beta2), float(eps),
                                            float(weight_decay), _ptr(ctl), _lib.stream_ptr()), "adam_step_ex")


# --------------------------------------------------------------------------------------------------
# feature front-end: the wrappers live in frontend.py; their public names stay importable from here
# --------------------------------------------------------------------------------------------------
from .frontend import (  # noqa: E402,F401
    fbank_frames, FbankPlan, MfccPlan, SpectrogramPlan, fbank, mfcc, spectrogram, LogSpecPlan, log_spectrum, resample_samples, ResamplePlan, resample,
    CONTEXT_OPTIONS, context_frames, delta_scales, frame_context_tile, frame_context, SPEC_AUGMENT_OPTIONS, spec_augment_plan, spec_augment_host,
    spec_augment, REVERB_LIMIT_FIELDS, REVERB_OPTIONS, reverb_limits, ReverbBank, reverb_plan, reverberate_host, reverberate, SLIDING_CMN_OPTIONS,
    cmvn_accumulate, _cmvn_groups, cmvn_accumulate_groups, cmvn_apply, cmvn_sliding_run, cmvn_sliding_window, cmvn_sliding_host, cmvn_norm_host,
    cmvn_sliding, PITCH_OPTIONS, PITCH_PROCESS_OPTIONS, PitchPlan, pitch_frames, pitch, pitch_host, pitch_process, pitch_process_host)
