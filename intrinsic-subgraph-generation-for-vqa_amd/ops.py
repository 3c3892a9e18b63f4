"""Tensor-level operators over the C ABI (include/isg.h): one Python function per kernel.

PyTorch is plumbing here: it owns device memory and the stream; every operator validates its
operands on the host (device, dtype, contiguity, shapes -- a wrong shape must never reach a
kernel) and then hands raw pointers to libisg_hip.so on torch's current stream.  When autograd is
recording through an operand the call is routed through autograd.py; an operator
without a backward refuses such an operand loudly.
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import operator
import os
import sys
import types
import weakref
from dataclasses import dataclass, field
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from . import _ext_curves, _ext_ig, _ext_induced, _ext_instances_train, _ext_maskopt, _ext_rollout, _lib, _lib_instances
from . import _ext_shapley

MAX_NODES_PER_GRAPH = 1024   # LDS strip / sampler row capacity of the kernels


# ---------------------------------------------------------------------------------------------------------------------------------
# Every A/B switch of this module in ONE frozen object.  The functions below read `CFG.<field>`; nothing else in the module is
# mutable configuration.  `ops.SPLIT_FORWARD = False` (tests, tools, bench.py: the historical spelling) is routed by the module's
# __setattr__ to `CFG = dataclasses.replace(CFG, split_forward=False)` -- an atomic swap of the whole object, never a field
# written in place -- and `ops.SPLIT_FORWARD` reads the field; `with ops.configured(split_forward=False): ...` restores it.
@dataclasses.dataclass(frozen=True)
class Switches:
    # graph plan
    plan_fused: bool = True                # isg_graph_plan_build (6 launches) instead of isg_graph_ptr + isg_csr_build + isg_graph_edge_ptr (14)
    bounds_to_host: bool = True            # isg_graph_plan_build writes the batch's true bounds into pinned host memory (hint check without a copy)
    # graphs beyond a tile
    mixed_dispatch: bool = True            # graphs beyond a tile go to the per-graph kernels, the rest of the batch stays on the tile kernels ...
    mixed_max_fraction: float = 0.12       # ... while at most this share of the batch's nodes sits in such graphs ...
    # ... and the batch has at least this many nodes: the big graphs are a chain of ~60 launches of a workgroup or a few each, ~1.8 ms of
    # HOST time per step whatever the batch.  Measured (profiles/r04_az_split_forward.txt), 4096 graphs + 1 / 8 / 64 big ones:
    # 1.84-1.91 / 2.00 / 2.12 ms (run_split, sub-batch on its own stream) against 2.35 / 2.49 / 2.63 ms with the per-graph kernels for
    # everything (1.43 ms without big graphs); 1024 graphs + 1: 1.83 vs 0.89 ms.  Tests and tools lower both to force the mode.
    mixed_min_nodes: int = 60000
    split_stream: bool = True              # run_split's sub-batch on a stream of its own, beside the whole batch's tile kernels
    split_forward: bool = True             # the graphs beyond a tile run as a batch of their own through the WHOLE model (off: every tile
                                           # kernel's wrapper fills their rows with the per-graph kernels, layer by layer)
    # message passing
    mp_kernel: str = "graph"               # "graph": per-graph LDS-resident kernel; "chunk": node-chunk kernel
    fuse_logits: bool = True               # lin_edge folded into the attention logits (isg_gatv2_edge_logits + isg_gatv2_mp_fwd_logits)
    fuse_logits_wide: bool = True          # ... also at head dimensions / edge widths beyond the tile shapes (C = 300, K = 300)
    rows_kernel_min_edges: int = 16384     # below this many edges a wide layer (C = 300 / K = 300) projects its edge rows and runs un-fused
    fuse_tile_conv: bool = True            # message + softmax + aggregation with lin_edge inside as one launch on graph tiles (isg_gatv2_tile_conv)
    fuse_layer_conv: bool = True           # ... and lin_l | lin_r inside as well (isg_gatv2_layer_conv): x_l / x_r never exist in memory
    tile_heavy_first: bool = True          # persistent tile kernels walk the tile list heavy tiles first
    fuse_gate: bool = True                 # the masked layer's node gate from the layer input's planes, node_nn inside
    fuse_dense_tail: bool = True           # x_proj + layer tail + next instruction gate as one kernel on graph-aligned tiles
    sparse_conv_out: bool = True           # a masked layer's convolution writes `out` only where that tail's live-row form reads it
    skip_unread_alpha: bool = True         # MGAT asks isg_gatv2_layer_conv for attention weights only under return_attention
    poison_sparse_out: bool = False        # debug: such a launch starts from NaN-filled `out` / `rowmax` (a read of an unwritten row shows)
    dense_tail_rows: int = 64              # nodes per tile of isg_mgat_dense_tail
    fuse_readout: bool = True              # node_nn + mask + per-graph softmax pooling as one launch on graph-aligned tiles
    fuse_question_mlps: bool = True        # the masked layers' ques_nn and the read-out's ques_nn as one launch ahead of the layers (isg_small_mlps)
    fuse_cat_mul_linear: bool = True       # the answer head's Linear over cat(a, b, a * b) reads a and b (isg_linear_f16x3_catmul): no isg_cat_mul_rowmax
    embedding_sum: bool = True             # sum of a node's token embeddings through isg_gather_add instead of gather + reduce
    # dense projections: which kernel runs a Linear (linear_route)
    gemm_backend: str = "bf16x6"           # "bf16x6": this library's kernels; "torch": hipBLASLt fp32 through torch
    gemm_kernel: str = "auto"              # "auto": per shape (linear_route); "panel": isg_linear_panel; "tile": isg_linear_bf16x6
    panel_min_n: int = 256                 # narrowest Linear the row-panel kernels take
    gemm_f16x3: bool = True                # K <= 128 panel shapes on the fp16 three-product kernel (isg_linear_f16x3) instead of bf16x6
    f16x3_f16_out: bool = True             # half-row results (configs[4]) of K <= 128 panel Linears on isg_linear_f16x3_f16 instead of bf16x6
    f16x3_tile: bool = True                # 128 < K Linears on isg_linear_f16x3_tile where the row maxima come cheap (linear_route)
    skinny: bool = True                    # Linears over at most skinny_max_m rows (and M N K <= skinny_max_work) on isg_linear_skinny
    skinny_max_m: int = 1024               # the latency-bound regime: a handful of questions per forward (csrc/isg_gemm_skinny.hip)
    skinny_max_work: int = 1 << 30         # true fp32 MFMAs run at 1/16 of the fp16 rate: beyond ~1e9 multiply-adds the tile kernels win
    linear_multi: bool = True              # the layers' bias-free projections of shared rows as one launch (isg_linear_panel_multi)
    # the planes32 engine (isg_linear_h3p)
    h3p: bool = True                       # Linears with K >= h3p_min_k over at least h3p_min_m rows on isg_linear_h3p
    h3p_min_k: int = 256                   # shortest reduction the engine takes
    # fewest rows the engine takes from a producer that left planes32.  8192 until round 6; swept with the small-batch kernels in place
    # (tools/time_full_model.py G --set=H3P_MIN_M=...): 2048 is 5-7 % faster at 160-700 graphs
    h3p_min_m: int = 2048
    h3p_min_m_unsplit: int = 8192          # fewest rows for an input without planes32 (the Linear pays a split pass of its own)
    h3p_chain: bool = True                 # Linear -> Linear pairs (the Transformer layers' FFN, mlp) through planes: no fp32 intermediate
    h3p_store_policy: int = -1             # store policy of large engine results: -1 library's / 0 plain / 1 nt / 2 sc0 sc1 nt / "auto" (_h3p_tune)
    linear_multi_h3p: bool = True          # the layers' lin_edge over the shared edge features as one engine launch
    ln_planes: bool = True                 # isg_add_layernorm writes its result as planes32 too where Linears on the engine read it
    mp_planes: bool = True                 # the flat message-passing kernel hands x_proj.0 its operand as segmented planes32
    gather_add_planes: bool = True         # isg_gather_add hands its rows to the Linear behind it as planes32
    mha_rows_planes: bool = True           # attention results as planes32 where the all-heads form fits
    mha_rows_max_tq: int = 16              # ... up to this many query rows per batch item


CFG = Switches()
_SWITCH_FIELDS = {f.name.upper(): f.name for f in dataclasses.fields(Switches)}


@contextlib.contextmanager
def configured(**fields):
    """Run a block under a modified copy of the switches (restored afterwards, exceptions included)."""
    global CFG
    keep = CFG
    CFG = dataclasses.replace(CFG, **fields)
    try:
        yield CFG
    finally:
        CFG = keep


class _OpsModule(types.ModuleType):
    def __getattr__(self, name):
        f = _SWITCH_FIELDS.get(name)
        if f is None:
            raise AttributeError(f"module {self.__name__!r} has no attribute {name!r}")
        return getattr(self.__dict__["CFG"], f)

    def __setattr__(self, name, value):
        f = _SWITCH_FIELDS.get(name)
        if f is None:
            super().__setattr__(name, value)
        else:
            self.__dict__["CFG"] = dataclasses.replace(self.__dict__["CFG"], **{f: value})

    def __delattr__(self, name):              # monkeypatch of a name that "did not exist": nothing to delete
        if name not in _SWITCH_FIELDS:
            super().__delattr__(name)


sys.modules[__name__].__class__ = _OpsModule

# Launches that leave this library's own dense kernels, and extra passes a missing hand-off costs; bench.py prints them
# per step ("no GEMM of the inference path runs on hipBLASLt" is then a number, not a sentence).
COUNTERS = {"torch_linear": 0, "torch_layer_norm": 0, "torch_attention": 0, "row_absmax": 0, "linear_h3p": 0, "h3p_segmented": 0, "linear_skinny": 0,
            "tile_nodes": 0, "oversize_nodes": 0,      # nodes the tile kernels took / nodes of graphs beyond a tile (mixed dispatch)
            "text_train_kernels": 0,                   # question encoder / decoder forwards under autograd on this library's kernels
            "sgenc_train_kernels": 0,                  # scene-graph encoder forwards under autograd without the concatenations (SPLIT_TRAIN)
            "torch_attention_train": 0,                # autograd.mha_small calls beyond the backward kernel's limits (torch's ops)
            "linear_bwd_kernels": 0,                   # autograd._Linear backwards on csrc/isg_linear_bwd.hip (autograd.LINEAR_BWD_KERNELS)
            "simple_bwd_kernel": 0,                    # SIMPLE sampler backwards on csrc/isg_simple_bwd.hip (autograd.SIMPLE_BWD_KERNEL)
            "topk_rows": 0,                            # sampler launches with a k per row (csrc/isg_topk_rows.hip; the budget launch is not one)
            "mp_dropout": 0,                           # message-passing forwards with attention dropout, p > 0 (include/isg_mp_train.h)
            "mp_f16_train": 0,                         # message-passing backwards on saved half rows (include/isg_mp_f16_train.h)
            "linear_rowbias": 0,                       # Linears with a bias row per graph (include/isg_concat.h; concat_instr layers)
            "graph_instances": 0,                      # expansions of a distinct batch into graph instances (include/isg_instances.h)
            "instance_rows_bwd": 0,                    # backwards of the instance-row gather (include/ext/isg_instances_train.h)
            "induced_instances": 0,                    # batches of induced-subgraph instances (include/ext/isg_induced.h)
            "attention_rollout": 0,                    # attention-rollout launches (include/ext/isg_rollout.h)
            "ig_path_rows": 0,                         # path-row launches of integrated gradients (include/ext/isg_ig.h)
            "ig_attribution": 0,                       # gradient rows reduced to attributions (include/ext/isg_ig.h)
            "maskopt_step": 0,                         # mask-optimisation iterations (include/ext/isg_maskopt.h)
            "curve_keep_bits": 0,                      # rankings with their keep rows of all levels (include/ext/isg_curves.h)
            "curve_sums": 0,                           # instance probabilities reduced to curves and areas (include/ext/isg_curves.h)
            "shapley_keep_bits": 0,                    # seeded permutations with the keep rows of their prefixes (include/ext/isg_shapley.h)
            "shapley_values": 0,                       # instance probabilities reduced to Shapley estimates (include/ext/isg_shapley.h)
            "eval_groups": 0,                          # grouped meter / grouped co-occurrence calls (include/isg_eval.h)
            "grounding": 0}                            # grounding scores against object annotations (include/isg_grounding.h)


def reset_counters() -> None:
    for k in COUNTERS:
        COUNTERS[k] = 0


def counters() -> dict:
    return dict(COUNTERS)


def _ver(t: Tensor):
    """Validity stamp of a cached derivative of `t`: the autograd version counter, or -- for tensors made under
    torch.inference_mode(), which have none (reading `._version` raises) -- a constant: an in-place write to an inference
    tensor cannot be seen, the caches then rest on (identity, data_ptr, shape) alone.  The reference evaluates under
    inference_mode (run_token_coo.py:49), so this path has to work there."""
    return -1 if t.is_inference() else t._version


class KernelTimer:
    """Optional HIP-event bracket around every launch of one named kernel (bench.py uses it for the
    message-passing kernel).  Events are recorded on the stream the kernel is launched on."""

    def __init__(self):
        self.pairs = []
        self.meta = []

    def bracket(self, info):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.pairs.append((start, end))
        self.meta.append(info)
        return start, end

    def bracket3(self, info):
        """A bracket around TWO consecutive launches with an event between them (info["mid"]): durations_ms() gives the
        pair, split_ms() the two parts."""
        start, end = self.bracket(info)
        info["mid"] = torch.cuda.Event(enable_timing=True)
        return start, info["mid"], end

    def split_ms(self):
        return [(s.elapsed_time(m["mid"]), m["mid"].elapsed_time(e)) for (s, e), m in zip(self.pairs, self.meta) if "mid" in m]

    def drop_last(self):
        """The bracketed launch did not happen (unsupported shape, the caller takes another path)."""
        self.pairs.pop()
        self.meta.pop()

    def durations_ms(self):
        return [s.elapsed_time(e) for s, e in self.pairs]


MP_TIMER: Optional[KernelTimer] = None   # set by bench.py around its timed region
H3P_TIMER: Optional[KernelTimer] = None  # the same around every isg_linear_h3p launch (bench.py: the full model's dense share)


def _rec(*tensors) -> bool:
    """True when autograd is recording through any of the tensors: the call is then routed through autograd.py, whose
    Function.forward re-enters the same ops.* function with autograd off."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_get_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """The current stream's hipStream_t.  torch.cuda.current_stream() builds a Stream object per call (~20 calls and 0.1-0.2 ms
    of host time per step, which a host-bound step -- small batches, the sub-batch of run_split -- pays in full): the raw
    handle of the current device's current stream instead."""
    if _raw_stream is None or _get_device is None:
        return torch.cuda.current_stream().cuda_stream
    return _raw_stream(_get_device())


class _Ready:
    """When a cached device tensor is safe to read: the stream that built it and an event behind the building launches.  A hit
    from ANOTHER stream (run_split's side pass, a caller's own streams) makes that stream wait for the event -- once; the marker
    is dropped when the event has completed.  A hit from the building stream is ordered by the stream itself and costs one
    integer comparison."""
    __slots__ = ("stream", "event")

    def __init__(self, on_cuda: bool):
        self.stream, self.event = None, None
        if on_cuda and not torch.cuda.is_current_stream_capturing():
            self.stream = _stream()
            self.event = torch.cuda.Event()
            self.event.record()

    def wait(self) -> None:
        ev = self.event
        if ev is None or _stream() == self.stream:
            return
        if ev.query():
            self.event = None           # done for every stream from here on
        else:
            torch.cuda.current_stream().wait_event(ev)


def _chk(t: Optional[Tensor], name: str, dtype, shape=None, optional=False) -> int:
    if t is None:
        if optional:
            return 0
        raise ValueError(f"{name} is required")
    if not t.is_cuda:
        raise _lib.IsgError(f"{name} must live on the GPU (got {t.device}); this path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if torch.is_grad_enabled() and t.requires_grad:
        raise NotImplementedError(
            f"{name} requires grad but this operator has no backward (see autograd.py for the differentiable set); "
            "wrap the call in torch.no_grad() or detach the input")
    return t.data_ptr()


def _chk_rows(t: Tensor, name: str, dtype=torch.float32) -> int:
    """Like _chk for a 2-D fp32 (or fp16) tensor whose rows may be strided (columns contiguous, rows aligned to 4
    elements)."""
    if not t.is_cuda:
        raise _lib.IsgError(f"{name} must live on the GPU (got {t.device}); this path has no CPU fallback")
    align = 15 if dtype == torch.float32 else 7
    if t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1 or (t.stride(0) & 3) or (t.data_ptr() & align):
        raise ValueError(f"{name}: expected {dtype} [rows, cols] with contiguous columns and rows aligned to 4 elements")
    if torch.is_grad_enabled() and t.requires_grad:
        raise NotImplementedError(f"{name} requires grad but this operator has no backward (see autograd.py)")
    return t.data_ptr()


# GraphPlan.build trusts the caller's max_nodes / max_edges hints to stay free of a device->host sync; the true bounds
# are computed on the device anyway, so every hinted build queues an asynchronous copy of them into pinned memory and
# the comparison happens later, on the host, once the copy has landed: at the next build (polled, never waited for) or
# at check_plans().  An understated hint (which would size the LDS tables / sampler rows too small and truncate
# graphs silently) therefore raises -- one step late, but loudly and without stalling the stream.
_PENDING_HINTS = []      # (event, pinned int32[2] = true [max nodes, max edges], hinted max_nodes, hinted max_edges)
_PENDING_SIZES = []      # (event, pinned int64[2 or 3] = graphs beyond a tile / their nodes / their edges counted on the device, the hint's counts)


_CAPTURE_BOUNDS = []     # StepCapture: the (pinned int32[2], device int32[2]) a plan built inside the capture in progress hands its last kernel


def _hint_error(true, hints, of: str) -> Optional[Exception]:
    """The IsgError for true (nodes, edges) beyond the hinted (max_nodes, max_edges or None), else None; `of`: what ran under them."""
    (n_true, e_true), (hn, he) = true, hints
    if n_true <= hn and (he is None or e_true <= he):
        return None
    return _lib.IsgError(f"GraphPlan hints understate the batch: max_nodes={hn} / max_edges={he} given, but a graph has "
                         f"{n_true} nodes / {e_true} edges; results of {of} are invalid")


def check_plans(block: bool = True) -> None:
    """Raise IsgError if a GraphPlan was built with hints smaller than the batch's true per-graph bounds.
    block=False only looks at copies that have already completed."""
    keep, bad = [], None
    for ev, host, hn, he in _PENDING_HINTS:
        if not block and not ev.query():
            keep.append((ev, host, hn, he))
            continue
        ev.synchronize()
        bad = bad or _hint_error((int(host[0]), int(host[1])), (hn, he), "that batch")
    _PENDING_HINTS[:] = keep
    keep_s, bad_s = [], None
    for ev, host, expect in _PENDING_SIZES:       # graph_sizes hints (GraphPlan._oversize_stats): counted on the device as well
        if not block and not ev.query():
            keep_s.append((ev, host, expect))
            continue
        ev.synchronize()
        got = [int(v) for v in host.tolist()]
        if got != expect:
            bad_s = bad_s or (got, expect)
    _PENDING_SIZES[:] = keep_s
    if bad_s is not None:
        raise _lib.IsgError(f"GraphPlan graph_sizes disagree with the batch: graphs beyond a tile / their nodes / their edges "
                            f"counted on the device {bad_s[0]}, from the hint {bad_s[1]}; results of that batch are invalid")
    if bad is not None:
        raise bad


def _f32(t: Tensor) -> Tensor:
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


# ------------------------------------------------------------------------------------------------
# Graph plan
# ------------------------------------------------------------------------------------------------


class OversizeGraphs(NamedTuple):
    """The graphs of a batch that do not fit a graph tile, as a batch of their own (GraphPlan.oversize)."""
    gids: Tensor                 # int64 [G] graph ids
    nodes: Tensor                # int64 [Ns] node ids
    edges: Optional[Tensor]      # int64 [Es] original edge ids (None: the plan has no CSR)
    batch: Tensor                # int64 [Ns] local graph index
    edge_index: Optional[Tensor]  # int64 [2, Es] local node ids
    plan: "GraphPlan"


class TilePlan(NamedTuple):
    """One packing of a batch's graphs into tiles (GraphPlan.tiles): five views of one int32 buffer."""
    tile_ptr: Tensor             # int32 [cap + 1] first graph of every tile
    ntiles: Tensor               # int32 [1], on the device
    cap: int                     # upper bound of the tile count: what the kernels are launched with
    info: Tensor                 # int32 [cap, 4] (first node, nodes, first CSR slot, CSR slots) in tile order
    heavy: Tensor                # int32 [cap, 4] the same entries by descending CSR-slot count (tiles_heavy_first)


class _PlanCache:
    """Everything a GraphPlan builds lazily, each on first use.  One object per plan, shared by the views made of it
    (GraphPlan.with_holes): what one of them builds, all of them find."""
    __slots__ = ("tiles", "edge_planes", "oversize_stats", "oversize", "by_src", "slots", "parent_edge_rows", "nmax_true")

    def __init__(self):
        self.tiles = {}                   # (node_cap, edge_cap) -> TilePlan
        self.edge_planes = None           # _from_tensor(edge_attr, NodePlanes)
        self.oversize_stats = {}          # (node_cap, edge_cap) -> dict or None (GraphPlan._oversize_stats)
        self.oversize = {}                # (node_cap, edge_cap) -> OversizeGraphs or None
        self.by_src = None                # (rowptr_s, eid_s, dst_s)
        self.slots = None                 # int64 [N]
        self.parent_edge_rows = None      # on the plan of a batch's oversize graphs: _from_tensor(the batch's edge_attr, their rows)
        self.nmax_true = None             # int: the longest row of a plan built with max_nodes= (GraphPlan.true_nmax)


def _csr_build(lib, edge_index: Tensor, N: int, E: int, rowptr: Tensor, eid: Tensor, src: Tensor, dst: Optional[Tensor]) -> None:
    """CSR by destination of edge_index into the given int32 arrays (isg_csr_build and its workspace)."""
    ws_bytes = lib.isg_csr_workspace_bytes(N, E)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=edge_index.device)
    _lib.check(lib.isg_csr_build(edge_index.data_ptr(), N, E, rowptr.data_ptr(), eid.data_ptr(), src.data_ptr(),
                                 0 if dst is None else dst.data_ptr(), ws.data_ptr(), ws_bytes, _stream()), "isg_csr_build")


@dataclass(slots=True)
class GraphPlan:
    """What every layer needs to know about one PyG Batch, computed once on the device.

    ptr[B+1] node range per graph, nmax (device scalar + host bound), CSR by destination
    (rowptr[N+1], eid[E] original edge ids, src[E] source ids).  Replaces the reference's per-call
    ``batch[-1].item()+1``, ``to_dense_batch`` counting and PyG's per-layer index handling
    (masking.py:135,162; att_pooling.py:60; mgat_v2_conv.py:215).
    """
    N: int
    E: int
    B: int
    ptr: Tensor
    nmax_dev: Tensor
    nmax: int
    emax: int = 0
    rowptr: Optional[Tensor] = None
    eid: Optional[Tensor] = None
    src: Optional[Tensor] = None
    dst: Optional[Tensor] = None
    eptr: Optional[Tensor] = None
    batch: Optional[Tensor] = None           # kept for the backward restatements (autograd.py)
    edge_index: Optional[Tensor] = None      # kept for the lazily built CSR by source (backward only)
    sizes_host: Optional[Tensor] = None           # HOST int64 [2, B] nodes / in-edges per graph when the caller's collate gave them (a hint
                                                  # like max_nodes / max_edges: lets oversize() count without a device-to-host sync)
    no_tiles: bool = False                        # the plan of a batch's oversize graphs: the tile kernels are not asked again
    graph_ids: Optional[Tensor] = None            # int32 [B]: this plan's graphs are a CUT of a larger batch and these are their numbers
                                                  # there -- the samplers' in-kernel noise is keyed by them (ops._gid_ptr)
    holes: Optional["OversizeGraphs"] = None      # with_holes: the tile kernels pass over these graphs and NOTHING fills their rows
    _memo: dict = field(default_factory=dict)     # answers that depend on the plan and the switches only (tile_mode, a layer's route):
                                                  # asked ~17 times per step by the layers, computed once
    _cache: _PlanCache = field(default_factory=_PlanCache)
    _bounds_dev: Optional[Tensor] = None          # these three: set on a plan built from hints inside a hipGraph capture (build) --
    _bounds_host: Optional[Tensor] = None         # where every replay leaves the true bounds, on the device and in pinned memory,
    _hints: Optional[Tuple[int, Optional[int]]] = None        # and the hinted (max_nodes, max_edges or None) they are held against
    nmax_hinted: bool = False                     # build() was given max_nodes: nmax is the caller's bound, the true longest row is
                                                  # nmax_dev (read back once, for the one sampler that needs it on the host: true_nmax)

    def memo(self) -> dict:
        return self._memo

    def with_holes(self, sub: "OversizeGraphs") -> "GraphPlan":
        """A view of this plan for run_split's tile pass: the same tensors and the same cache, `holes` = sub, and a memo of its
        own (a layer's route depends on `holes`).  This plan is not written to."""
        return dataclasses.replace(self, holes=sub, _memo={})

    def edge_planes(self, edge_attr: Tensor) -> Tuple[Tensor, Tensor]:
        """(planes int16 [E, 2, 128], inv_scale fp32 [E]) of the batch's edge features in CSR slot order (isg_edge_planes): the
        operand of isg_gatv2_tile_conv.  Every layer and head reads the same edge features (mgat.py:144-148), so the split is
        made once per batch and kept on the plan (keyed by the tensor's identity, storage and version)."""
        self.require_csr()
        hit = _if_from_tensor(self._cache.edge_planes, edge_attr)
        if hit is None:
            lib = _lib.load()
            E, K = edge_attr.shape
            hit = _empty_node_planes(E, edge_attr.device)
            _lib.check(lib.isg_edge_planes(_chk_rows(edge_attr, "edge_attr"), edge_attr.stride(0), self.eid.data_ptr(), E, K,
                                           hit.planes.data_ptr(), hit.inv.data_ptr(), _stream()), "isg_edge_planes")
            self._cache.edge_planes = _from_tensor(edge_attr, hit)
        return hit.planes, hit.inv

    def tiles_and_edge_planes(self, edge_attr: Tensor, node_cap: int, edge_cap: int):
        """(tiles(node_cap, edge_cap), edge_planes(edge_attr)); when neither exists yet they are made by ONE launch
        (isg_tile_plan_edge_planes: the one-workgroup tile plan runs beside the row split instead of alone on the chip)."""
        key = (int(node_cap), int(edge_cap))
        if CFG.plan_fused and key not in self._cache.tiles and _if_from_tensor(self._cache.edge_planes, edge_attr) is None \
                and edge_cap > 0 and edge_attr.dim() == 2 and edge_attr.size(1) <= 128 and edge_attr.size(1) % 4 == 0 \
                and edge_attr.dtype == torch.float32:
            lib = _lib.load()
            self.require_csr()
            E, K = edge_attr.shape
            t = self._empty_tile_plan(lib, key)
            ep = _empty_node_planes(E, edge_attr.device)
            rc = lib.isg_tile_plan_edge_planes(self.ptr.data_ptr(), self.eptr.data_ptr(), self.B, key[0], key[1], t.tile_ptr.data_ptr(),
                                               t.ntiles.data_ptr(), t.info.data_ptr(), t.cap, t.heavy.data_ptr(),
                                               _chk_rows(edge_attr, "edge_attr"), edge_attr.stride(0), self.eid.data_ptr(), E, K,
                                               ep.planes.data_ptr(), ep.inv.data_ptr(), _stream())
            if rc != ISG_EUNSUPPORTED:
                _lib.check(rc, "isg_tile_plan_edge_planes")
                self._cache.tiles[key] = t
                self._cache.edge_planes = _from_tensor(edge_attr, ep)
        return self.tiles(node_cap, edge_cap), self.edge_planes(edge_attr)

    def _empty_tile_plan(self, lib, key: Tuple[int, int]) -> TilePlan:
        """The unfilled TilePlan of caps `key`: one allocation, info first (16-byte aligned)."""
        cap = int(lib.isg_tile_plan_capacity(self.N, self.E, self.B, key[0], key[1]))
        buf = torch.empty(9 * cap + 8, dtype=torch.int32, device=self.ptr.device)
        return TilePlan(buf[8 * cap + 4:9 * cap + 5], buf[9 * cap + 5:9 * cap + 6], cap, buf[:4 * cap].view(cap, 4),
                        buf[4 * cap:8 * cap].view(cap, 4))

    def tiles_heavy_first(self, node_cap: int = 64, edge_cap: int = 0) -> Tensor:
        """tile_info of tiles(node_cap, edge_cap) ordered by descending CSR-slot count (32-slot classes, ties in tile order): the list
        the PERSISTENT tile kernels (isg_gatv2_layer_conv / _tile_conv: workgroup w takes entries w, w + G, ...) are handed, so that
        every workgroup gets one tile of each weight class per round -- the slowest workgroup's share of the work is 1.03x the mean
        instead of 1.06x at BASELINE configs[1] (tools/sim_tile_balance.py).  Any order gives the same results."""
        t = self._tile_plan(node_cap, edge_cap)
        return t.heavy if CFG.tile_heavy_first else t.info

    def tiles(self, node_cap: int = 64, edge_cap: int = 0) -> Tuple[Tensor, Tensor, int, Tensor]:
        """(tile_ptr int32[cap + 1], ntiles int32[1] on the device, cap, tile_info int32[cap, 4]): consecutive graphs packed greedily into tiles of
        at most `node_cap` nodes (and `edge_cap` CSR slots when > 0) -- the M-tiles of the fused per-layer kernels
        (csrc/isg_layer_tile.hip).  Tile t owns graphs tile_ptr[t] .. tile_ptr[t + 1] and tile_info[t] = (first node, nodes,
        first CSR slot, CSR slots); the count stays on the device (no sync): kernels are launched with `cap` workgroups, the ones
        beyond *ntiles return at once, or walk the tiles persistently.  Built on first use."""
        return self._tile_plan(node_cap, edge_cap)[:4]

    def _tile_plan(self, node_cap: int, edge_cap: int) -> TilePlan:
        key = (int(node_cap), int(edge_cap))
        t = self._cache.tiles.get(key)
        if t is None:
            lib = _lib.load()
            if edge_cap > 0:
                self.require_csr()
            t = self._empty_tile_plan(lib, key)
            _lib.check(lib.isg_tile_plan(self.ptr.data_ptr(), self.eptr.data_ptr() if edge_cap > 0 else 0, self.B, key[0],
                                         key[1], t.tile_ptr.data_ptr(), t.ntiles.data_ptr(), t.info.data_ptr(), t.cap,
                                         t.heavy.data_ptr(), _stream()), "isg_tile_plan")
            self._cache.tiles[key] = t
        return t

    def tile_mode(self, node_cap: int = 64, edge_cap: int = 256) -> str:
        """How the graph-tile kernels (isg_gatv2_layer_conv / _tile_conv, isg_mgat_dense_tail, isg_readout_tile) can take this
        batch: "tiles" -- every graph fits a tile; "mixed" -- a few do not: the tile kernels pass over them (isg_tile_plan
        gives such a graph an empty tile) and the per-graph kernels run on the list of them (`oversize`), both writing disjoint
        rows of the same outputs; "none" -- tiles do not pay (most nodes sit in oversize graphs) or the list cannot be made
        (inside a hipGraph capture: it takes a device-to-host sync)."""
        ecap = edge_cap if self.rowptr is not None else 0
        if self.B <= 0 or self.nmax <= 0 or self.no_tiles:
            return "none"
        if self.nmax <= node_cap and (ecap == 0 or self.emax <= ecap):
            return "tiles"
        if not CFG.mixed_dispatch or torch.cuda.is_current_stream_capturing():
            return "none"
        if self.N < CFG.mixed_min_nodes:
            return "none"                   # decided before the device-to-host sync below: a small batch never pays for it
        key = ("tile_mode", node_cap, ecap, CFG.mixed_max_fraction)
        hit = self._memo.get(key)
        if hit is None:
            st = self._oversize_stats(node_cap, edge_cap)
            if st is None or st["stats"][0] == 0:
                hit = "tiles"               # the hints overstated the batch
            else:   # (the LIST of such graphs -- ~30 launches -- is only built for a batch that then uses it)
                hit = "mixed" if st["stats"][1] <= CFG.mixed_max_fraction * self.N else "none"
            self._memo[key] = hit
        return hit

    def _oversize_stats(self, node_cap: int, edge_cap: int) -> Optional[dict]:
        """How many graphs of the batch lie beyond a tile, with their node / edge totals and maxima: ONE device-to-host sync, paid
        only by batches whose bounds say there is such a graph; cached per (plan, caps)."""
        ecap = int(edge_cap) if self.rowptr is not None else 0
        key = (int(node_cap), ecap)
        if key in self._cache.oversize_stats:
            return self._cache.oversize_stats[key]
        res = None
        if self.nmax > int(node_cap) or (ecap > 0 and self.emax > ecap):
            ptr = self.ptr.long()
            n = ptr[1:] - ptr[:-1]
            big = n > int(node_cap)
            e = eptr = None
            if ecap > 0:
                eptr = self.eptr.long()
                e = eptr[1:] - eptr[:-1]
                big = big | (e > ecap)
            if self.sizes_host is not None:       # the collate's per-graph counts: no sync (verify_hints checks the bounds they imply)
                nh, eh = self.sizes_host[0], self.sizes_host[1]
                bh = nh > int(node_cap)
                if ecap > 0:
                    bh = bh | (eh > ecap)
                st = [int(bh.sum()), int(nh[bh].sum()), int(nh[bh].max()) if bool(bh.any()) else 0]
                if e is not None:
                    st += [int(eh[bh].sum()), int(eh[bh].max()) if bool(bh.any()) else 0]
                if not torch.cuda.is_current_stream_capturing():
                    # the same counts on the device, copied to pinned memory behind the stream and compared at check_plans():
                    # a wrong hint would size the lists below wrongly without any fault
                    dev_cnt = torch.stack([big, big * n] + ([big * e] if e is not None else [])).sum(1)
                    host = torch.empty(dev_cnt.numel(), dtype=torch.int64, pin_memory=True)
                    host.copy_(dev_cnt, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record()
                    _PENDING_SIZES.append((ev, host, [st[0], st[1]] + ([st[3]] if e is not None else [])))
            else:
                zero = n.new_zeros(())
                nb = torch.where(big, n, zero)
                stats = [big.sum(), nb.sum(), nb.max()]
                if e is not None:
                    eb = torch.where(big, e, zero)
                    stats += [eb.sum(), eb.max()]
                st = [int(v) for v in torch.stack(stats).tolist()]
            res = {"stats": st, "ptr": ptr, "n": n, "big": big, "eptr": eptr, "e": e}
        self._cache.oversize_stats[key] = res
        return res

    def oversize(self, node_cap: int = 64, edge_cap: int = 256) -> Optional["OversizeGraphs"]:
        """The graphs of this batch beyond a tile (more than node_cap nodes or edge_cap in-edges) as a batch of their own: graph
        ids, node ids, original edge ids (all ascending: segment sums keep their order), local batch vector / edge_index and the
        GraphPlan over them.  None when every graph fits.  Built once per (plan, caps); one device-to-host sync, paid only by
        batches that have such graphs.  The reference puts no cap on the objects of a scene graph (datasets/scene_graph.py:199-389)."""
        ecap = int(edge_cap) if self.rowptr is not None else 0
        key = (int(node_cap), ecap)
        if key in self._cache.oversize:
            return self._cache.oversize[key]
        res = None
        st = self._oversize_stats(node_cap, edge_cap)        # ONE device-to-host sync: how many such graphs, their nodes / edges
        if st is not None:
            stats, ptr, n, big, eptr, e = st["stats"], st["ptr"], st["n"], st["big"], st["eptr"], st["e"]
            G = stats[0]
            if G > 0:
                # flags -> compaction: every list comes out ascending (segment sums keep their order) without a sort
                Ns, nmax_s = stats[1], stats[2]
                gids = torch.nonzero_static(big, size=G).squeeze(1)
                node_big = big[self.batch]                                    # [N]: the node sits in such a graph
                nodes = torch.nonzero_static(node_big, size=Ns).squeeze(1)
                seg = (big.cumsum(0) - 1)[self.batch[nodes]]                  # local graph index of those nodes
                edges = sub_ei = None
                emax_s = None
                if e is not None:
                    Es, emax_s = stats[3], stats[4]
                    edges = torch.nonzero_static(node_big[self.edge_index[1]], size=Es).squeeze(1)      # by destination: edges stay
                    newid = node_big.cumsum(0) - 1                                                    # inside their graph
                    sub_ei = newid[self.edge_index[:, edges]].contiguous()
                sub_plan = GraphPlan.build(seg.contiguous(), sub_ei, num_graphs=G, max_nodes=nmax_s, max_edges=emax_s)
                sub_plan.no_tiles = True
                own = self.graph_ids                        # a cut of a cut keeps the ORIGINAL batch's numbers
                sub_plan.graph_ids = (gids if own is None else own.long()[gids]).to(torch.int32).contiguous()
                res = OversizeGraphs(gids, nodes, edges, seg, sub_ei, sub_plan)
        self._cache.oversize[key] = res
        return res

    def source_csr(self) -> Tuple[Tensor, Tensor, Tensor]:
        """(rowptr_s[N+1], eid_s[E], dst_s[E]): out-edges of every node in edge-id order.  Only the backward of the
        message passing needs it (d x_l is a scatter by source), so it is built on first use."""
        self.require_csr()
        if self._cache.by_src is None:
            sizes = (self.N + 1, max(self.E, 1), max(self.E, 1))
            by_src = tuple(torch.empty(n, dtype=torch.int32, device=self.rowptr.device) for n in sizes)
            _csr_build(_lib.load(), self.edge_index.flip(0).contiguous(), self.N, self.E, *by_src, None)
            self._cache.by_src = by_src
        return self._cache.by_src

    @staticmethod
    def build(batch: Tensor, edge_index: Optional[Tensor] = None, num_graphs: Optional[int] = None,
              max_nodes: Optional[int] = None, max_edges: Optional[int] = None,
              graph_sizes: Optional[Tensor] = None) -> "GraphPlan":
        lib = _lib.load()
        _chk(batch, "batch", torch.int64)
        N = batch.numel()
        if num_graphs is None:
            num_graphs = int(batch[-1].item()) + 1 if N > 0 else 0     # the reference's own sync (masking.py:135)
        B = int(num_graphs)
        dev = batch.device
        ptr = torch.empty(B + 1, dtype=torch.int32, device=dev)
        bounds = torch.empty(2, dtype=torch.int32, device=dev)     # [max nodes per graph, max edges per graph]
        nmax_dev = bounds[:1]
        plan = GraphPlan(N=N, E=0, B=B, ptr=ptr, nmax_dev=nmax_dev, nmax=0, batch=batch)
        if graph_sizes is not None:
            if graph_sizes.device.type != "cpu" or graph_sizes.dim() != 2 or tuple(graph_sizes.shape) != (2, B):
                raise ValueError("graph_sizes: a HOST tensor [2, num_graphs] (nodes, in-edges per graph)")
            plan.sizes_host = graph_sizes.long()
        host_bounds = bounds_max = None
        plan.nmax_hinted = max_nodes is not None
        if edge_index is not None:
            _chk(edge_index, "edge_index", torch.int64)
            if edge_index.dim() != 2 or edge_index.size(0) != 2:
                raise ValueError(f"edge_index must be [2,E], got {tuple(edge_index.shape)}")
        if edge_index is None or not CFG.plan_fused:        # (the fused plan kernel below makes ptr and the bounds itself)
            bounds.zero_()
            _lib.check(lib.isg_graph_ptr(batch.data_ptr(), N, B, ptr.data_ptr(), nmax_dev.data_ptr(), _stream()), "isg_graph_ptr")
        if edge_index is not None:
            E = edge_index.size(1)
            plan.E, plan.edge_index = E, edge_index
            # one allocation for the five index arrays (rows 16-byte aligned)
            n1, e1 = (N + 1 + 3) // 4 * 4, (max(E, 1) + 3) // 4 * 4
            idx = torch.empty(n1 + 3 * e1 + B + 1, dtype=torch.int32, device=dev)
            plan.rowptr, plan.eid = idx[:N + 1], idx[n1:n1 + max(E, 1)]
            plan.src, plan.dst = idx[n1 + e1:n1 + e1 + max(E, 1)], idx[n1 + 2 * e1:n1 + 2 * e1 + max(E, 1)]
            plan.eptr = idx[n1 + 3 * e1:n1 + 3 * e1 + B + 1]
            if CFG.plan_fused:
                ws_bytes = lib.isg_csr_workspace_bytes(N, E)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                # hinted and eager: the plan's last kernel stores the bounds into pinned host memory itself (no copy in the stream)
                if max_nodes is not None and max_edges is not None and CFG.bounds_to_host:
                    if not torch.cuda.is_current_stream_capturing():
                        host_bounds = torch.empty(2, dtype=torch.int32, pin_memory=True)
                    elif _CAPTURE_BOUNDS:          # StepCapture: pinned memory allocated BEFORE the capture, and a device int32[2]
                        host_bounds, bounds_max = _CAPTURE_BOUNDS[-1]      # in which the replays keep their running maximum
                _lib.check(lib.isg_graph_plan_build(batch.data_ptr(), edge_index.data_ptr(), N, E, B, ptr.data_ptr(),
                                                    bounds.data_ptr(), 0 if host_bounds is None else host_bounds.data_ptr(),
                                                    0 if bounds_max is None else bounds_max.data_ptr(),
                                                    plan.rowptr.data_ptr(), plan.eid.data_ptr(),
                                                    plan.src.data_ptr(), plan.dst.data_ptr(), plan.eptr.data_ptr(), ws.data_ptr(),
                                                    ws_bytes, _stream()), "isg_graph_plan_build")
            else:
                _csr_build(lib, edge_index, N, E, plan.rowptr, plan.eid, plan.src, plan.dst)
                _lib.check(lib.isg_graph_edge_ptr(ptr.data_ptr(), plan.rowptr.data_ptr(), B, plan.eptr.data_ptr(),
                                                  bounds[1:].data_ptr(), _stream()), "isg_graph_edge_ptr")
        if max_nodes is None or (edge_index is not None and max_edges is None):
            got = bounds.tolist()                   # one D2H sync per batch (to_dense_batch syncs per layer)
            plan._cache.nmax_true = got[0]
            max_nodes = got[0] if max_nodes is None else max(int(max_nodes), got[0])
            max_edges = got[1] if max_edges is None else max(int(max_edges), got[1])
        elif torch.cuda.is_current_stream_capturing():
            # Built inside a hipGraph capture: no pinned allocation, no event to query.  The true bounds stay on the device
            # (every replay rewrites them); the owner of the graph calls plan.verify_hints() after replays -- one sync, outside
            # the captured work -- and gets the same error an eager build would raise one step late.
            plan._bounds_dev = bounds
            plan._bounds_host = host_bounds           # (StepCapture reads it between replays, without a sync)
            plan._hints = (int(max_nodes), None if edge_index is None else int(max_edges))
        else:                                       # hinted: verify later, without a sync (see check_plans)
            if _PENDING_HINTS or _PENDING_SIZES:
                check_plans(block=False)
            if host_bounds is not None:
                host = host_bounds
            else:
                host = torch.empty(2, dtype=torch.int32, pin_memory=True)
                host.copy_(bounds, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            _PENDING_HINTS.append((ev, host, int(max_nodes), None if edge_index is None else int(max_edges)))
            if len(_PENDING_HINTS) > 64:
                check_plans(block=True)
        plan.nmax = int(max_nodes)
        plan.emax = int(max_edges or 0)
        if plan.nmax > MAX_NODES_PER_GRAPH:
            raise _lib.IsgError(f"graphs with more than {MAX_NODES_PER_GRAPH} nodes are unsupported (got {plan.nmax})")
        return plan

    def verify_hints(self) -> None:
        """For a plan built inside a hipGraph capture: compare the hints with the bounds the LAST replay computed (one
        device->host sync).  Raises IsgError like check_plans(); a no-op for plans built eagerly (those are verified there)."""
        err = None if self._bounds_dev is None else _hint_error(self._bounds_dev.tolist(), self._hints, "that replay")
        if err is not None:
            raise err

    @staticmethod
    def edges_only(edge_index: Tensor, num_nodes: int) -> "GraphPlan":
        """CSR by destination without any per-graph structure (for callers that only have edge_index)."""
        lib = _lib.load()
        _chk(edge_index, "edge_index", torch.int64)
        dev, N, E = edge_index.device, int(num_nodes), edge_index.size(1)
        plan = GraphPlan(N=N, E=E, B=0, ptr=torch.zeros(1, dtype=torch.int32, device=dev),
                         nmax_dev=torch.zeros(1, dtype=torch.int32, device=dev), nmax=0, edge_index=edge_index)
        plan.rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
        plan.eid = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        plan.src = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        _csr_build(lib, edge_index, N, E, plan.rowptr, plan.eid, plan.src, None)
        return plan

    def dense_slots(self) -> Tensor:
        """Position of every node in the padded [B * nmax] layout of to_dense_batch (int64 [N])."""
        if self._cache.slots is None:
            b = self.batch
            self._cache.slots = b * self.nmax + (torch.arange(self.N, device=b.device) - self.ptr.long()[b])
        return self._cache.slots

    def true_nmax(self, of: str) -> int:
        """The batch's longest row on the host, for `of` -- an operator whose result depends on it and not only on a bound of it
        (the SIMPLE sampler: the row length decides its circuit and the number of competing zero pads).  nmax itself unless
        build() was given max_nodes; then nmax_dev read back, one device-to-host copy per plan, kept in the cache.  A plan built
        inside a stream capture keeps no such number (every replay rewrites nmax_dev), and during a capture the copy is
        impossible: IsgError, before anything is launched.  A hint below the true length raises as check_plans() would."""
        if not self.nmax_hinted:
            return self.nmax
        if self._cache.nmax_true is None:
            if self._bounds_dev is not None or torch.cuda.is_current_stream_capturing():
                raise _lib.IsgError(f"{of} needs the batch's true longest row on the host; this GraphPlan was built with "
                                    f"max_nodes={self.nmax}, and nmax_dev cannot be copied back during a stream capture, nor kept for a "
                                    "plan built inside one: build the plan without max_nodes, outside the capture")
            self._cache.nmax_true = int(self.nmax_dev.item())
        if self._cache.nmax_true > self.nmax:
            raise _hint_error((self._cache.nmax_true, 0), (self.nmax, None), of)
        return self._cache.nmax_true

    def require_csr(self) -> None:
        if self.rowptr is None:
            raise ValueError("this GraphPlan was built without edge_index")


# ------------------------------------------------------------------------------------------------
# The sampled subgraph as a graph
# ------------------------------------------------------------------------------------------------
SUBGRAPH_BLOCK = 1024      # consecutive elements one workgroup of isg_subgraph_cut ranks (SG_BLOCK in csrc/isg_subgraph.hip)


class SubgraphCut:
    """What isg_subgraph_cut left on the device: the induced subgraph of a node mask, renumbered.  The tensors below have the
    parent's capacity (N / E entries); `.sizes()` copies the two counts to the host -- once, the operator's only device-to-host
    copy -- and the trimmed views go through it.

    node_new int32 [N] / edge_new int32 [E]: new id of every node / edge, -1 where it was cut; ptr int32 [B + 1]: node range per
    graph in the cut (graph numbers are the parent's; a graph may be empty); sel int32 [B, table_k] or None: local indices of
    every graph's first table_k kept nodes, then -1; counts int32 [2] = (N', E') on the device."""

    def __init__(self, parent: "GraphPlan", node_new, edge_new, node_id, edge_id, edge_index, batch, ptr, sel, counts):
        self.parent = parent
        self.node_new, self.edge_new, self.ptr, self.sel, self.counts = node_new, edge_new, ptr, sel, counts
        self._node_id, self._edge_id, self._edge_index, self._batch = node_id, edge_id, edge_index, batch
        self._sizes = None
        self._trim = {}

    def sizes(self) -> Tuple[int, int]:
        """(N', E'): nodes and edges of the cut."""
        if self._sizes is None:
            n, e = self.counts.tolist()
            self._sizes = (int(n), int(e))
        return self._sizes

    def _trimmed(self, name: str) -> Tensor:
        if name not in self._trim:
            n, e = self.sizes()
            self._trim[name] = {"node_id": lambda: self._node_id[:n], "edge_id": lambda: self._edge_id[:e],
                                "edge_index": lambda: self._edge_index[:, :e].contiguous(),
                                "batch": lambda: self._batch[:n]}[name]()
        return self._trim[name]

    @property
    def node_id(self) -> Tensor:
        """int64 [N']: the kept nodes, ascending."""
        return self._trimmed("node_id")

    @property
    def edge_id(self) -> Tensor:
        """int64 [E']: the kept edges, in their original order."""
        return self._trimmed("edge_id")

    @property
    def edge_index(self) -> Tensor:
        """int64 [2, E']: the kept edges between the cut's node numbers."""
        return self._trimmed("edge_index")

    @property
    def batch(self) -> Tensor:
        """int64 [N']: graph of every kept node."""
        return self._trimmed("batch")

    def gather_nodes(self, t: Tensor) -> Tensor:
        """t[node_id] for a tensor with one row per node of the parent batch."""
        return t.index_select(0, self.node_id)

    def gather_edges(self, t: Tensor) -> Tensor:
        """t[edge_id] for a tensor with one row per edge of the parent batch."""
        return t.index_select(0, self.edge_id)

    def remap_edge_positions(self, positions: Tensor) -> Tensor:
        """Positions in the parent's GLOBAL edge list (the scene graphs' added_sym_edge as the encoder applies it, quirk Q6) as
        positions in the cut's edge list; those of cut edges, and those beyond the list, are dropped."""
        E = self.edge_new.numel()
        p = positions.long()
        p = p[(p >= 0) & (p < E)]
        new = self.edge_new.long().index_select(0, p)
        return new[new >= 0]

    def plan(self) -> "GraphPlan":
        """The GraphPlan of the cut.  A subgraph's graphs are no larger than the parent's, so the parent's bounds serve as hints
        and the build costs no device-to-host sync."""
        if "plan" not in self._trim:
            self._trim["plan"] = GraphPlan.build(self.batch, self.edge_index, num_graphs=self.parent.B, max_nodes=self.parent.nmax,
                                                 max_edges=self.parent.emax)
        return self._trim["plan"]


def subgraph_cut(node_mask: Tensor, edge_index: Tensor, plan: "GraphPlan", threshold: float = 0.0, complement: bool = False,
                 table_k: int = 0) -> SubgraphCut:
    """The induced subgraph of the nodes with node_mask > threshold (complement: of the others) as a graph, cut on the device
    (isg_subgraph_cut: three launches, no sync).  node_mask fp32 [N] or [N, 1] (a forward's imle_mask), edge_index int64 [2, E],
    plan the batch's GraphPlan; table_k > 0 also fills SubgraphCut.sel."""
    lib = _lib.load()
    if node_mask.dim() == 2 and node_mask.size(1) == 1:
        node_mask = node_mask.squeeze(1)
    p_mask = _chk(node_mask, "node_mask", torch.float32)
    p_ei = _chk(edge_index, "edge_index", torch.int64)
    N, B, k = plan.N, plan.B, int(table_k)
    if tuple(node_mask.shape) != (N,):
        raise ValueError(f"node_mask: expected [{N}] or [{N}, 1], got {tuple(node_mask.shape)}")
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"edge_index must be [2,E], got {tuple(edge_index.shape)}")
    if plan.batch is None:
        raise ValueError("subgraph_cut needs a GraphPlan built from the batch vector")
    p_batch = _chk(plan.batch, "plan.batch", torch.int64, (N,))
    if k < 0:
        raise ValueError(f"table_k must be >= 0, got {table_k}")
    E = edge_index.size(1)
    dev = node_mask.device
    # one allocation per element width; pointers are taken from the buffers (an EMPTY view's data_ptr() is null)
    ws_bytes = lib.isg_subgraph_workspace_bytes(N, E)
    n32 = N + E + (B + 1) + B * k + 2
    i32 = torch.empty(n32 + (ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    i64 = torch.empty(max(2 * N + 3 * E, 1), dtype=torch.int64, device=dev)
    o_nn, o_en, o_ptr, o_sel, o_cnt = 0, N, N + E, N + E + B + 1, N + E + B + 1 + B * k
    o_nid, o_eid, o_ei, o_b = 0, N, N + E, N + 3 * E
    b32, b64 = i32.data_ptr(), i64.data_ptr()
    _lib.check(lib.isg_subgraph_cut(p_mask, float(threshold), 1 if complement else 0, p_ei, p_batch,
                                    _chk(plan.ptr, "plan.ptr", torch.int32, (B + 1,)), N, E, B, b32 + 4 * o_nn, b32 + 4 * o_en,
                                    b64 + 8 * o_nid, b64 + 8 * o_eid, b64 + 8 * o_ei, b64 + 8 * o_b, b32 + 4 * o_ptr,
                                    b32 + 4 * o_sel if k else 0, k, b32 + 4 * o_cnt, b32 + 4 * n32, ws_bytes, _stream()),
               "isg_subgraph_cut")
    return SubgraphCut(plan, i32[o_nn:o_nn + N], i32[o_en:o_en + E], i64[o_nid:o_nid + N], i64[o_eid:o_eid + E],
                       i64[o_ei:o_ei + 2 * E].view(2, E), i64[o_b:o_b + N], i32[o_ptr:o_ptr + B + 1],
                       i32[o_sel:o_sel + B * k].view(B, k) if k else None, i32[o_cnt:o_cnt + 2])


# ------------------------------------------------------------------------------------------------
# Many questions per scene graph: G distinct graphs, Q instances
# ------------------------------------------------------------------------------------------------
INSTANCES_SCAN_BLOCK = 1024      # instances one step of the size pass's scan takes (INST_SCAN_BLOCK in csrc/isg_instances.hip)
INSTANCES_FLAGS = ("bad_index", "bad_grouping")      # words 2 and 3 of GraphInstances.status


class GraphInstances:
    """What isg_instances_size / isg_instances_fill left on the device: the batch of Q graph instances that Q questions would have
    brought along as copies of the parent batch's graphs index[q] (include/isg_instances.h).

    ptr / eptr int32 [Q + 1]: node / edge range of every instance; batch int64 [N'] (value q on instance q's nodes); edge_index
    int64 [2, E'] between the instance batch's node numbers; node_src int64 [N'] / edge_src int64 [E']: the row of the parent
    batch every instance row is a copy of; status int32 [4] = (N', E', bad_index, bad_grouping) on the device; index int32 [Q] on
    the device.  sizes_host: host int64 [2, Q] (nodes, edges per instance) when the caller knew the parent's on the host.
    erange int32 [G + 1]: the edge range of every graph of the parent batch, as the size pass left it in its workspace (the
    backward of gather_rows reads it); index_host: the index as the caller gave it, when it came from the host."""

    def __init__(self, parent: "GraphPlan", index, ptr, eptr, batch, edge_index, node_src, edge_src, status, sizes_host=None,
                 parent_edges=None, erange=None, index_host=None):
        self.parent, self.index, self.ptr, self.eptr, self.status, self.sizes_host = parent, index, ptr, eptr, status, sizes_host
        self.batch, self.edge_index, self.node_src, self.edge_src = batch, edge_index, node_src, edge_src
        self.parent_edges = parent.E if parent_edges is None else int(parent_edges)      # (a plan may have been built without edges)
        self.erange, self.index_host = erange, index_host
        self._plan = self._by_graph = None

    @property
    def Q(self) -> int:
        return self.ptr.numel() - 1

    def gather_nodes(self, t: Tensor) -> Tensor:
        """t[node_src] for a tensor with one row per node of the parent batch (any dtype)."""
        return t.index_select(0, self.node_src)

    def gather_edges(self, t: Tensor) -> Tensor:
        """t[edge_src] for a tensor with one row per edge of the parent batch (any dtype)."""
        return t.index_select(0, self.edge_src)

    def by_graph(self) -> Tuple[Tensor, Tensor]:
        """(gptr int32 [G + 1], glist int32 [Q]) on the device: glist[gptr[g] : gptr[g + 1]] are the instances of graph g in
        ascending q -- the inverse of `index`, cached.  Made on the host when the index came from the host; otherwise by a stable
        device sort of the [Q] index (the counts read off the sorted keys by a binary search, which unlike bincount does not wait
        for the device).  An index outside [0, G) belongs to no graph: it sorts behind all of them."""
        if self._by_graph is None:
            G, dev = self.parent.B, self.index.device
            idx = (self.index if self.index_host is None else self.index_host).long()
            key = torch.where((idx >= 0) & (idx < G), idx, torch.full_like(idx, G))
            key, order = torch.sort(key, stable=True)
            gptr = torch.searchsorted(key, torch.arange(G + 1, dtype=torch.int64, device=key.device))
            self._by_graph = (gptr.to(device=dev, dtype=torch.int32), order.to(device=dev, dtype=torch.int32))
        return self._by_graph

    def counts(self) -> Tensor:
        """int32 [G] on the device: the number of instances of every graph of the parent batch."""
        gptr = self.by_graph()[0]
        return gptr[1:] - gptr[:-1]

    def gather_rows(self, x: Tensor, e: Tensor) -> Tuple[Tensor, Tensor]:
        """(x[node_src], e[edge_src]) for fp32 rows in ONE launch (isg_instance_rows): x [N, Cx], e [E, Ce], widths and row strides
        multiples of 4, rows 16-byte aligned.  When autograd records through x or e: autograd.instance_rows, whose backward is
        instance_rows_backward."""
        if _rec(x, e):
            from . import autograd
            return autograd.instance_rows(self, x, e)
        lib = _lib_instances.load()
        px, pe = _chk_rows(x, "x"), _chk_rows(e, "e")
        if x.size(0) != self.parent.N or e.size(0) != self.parent_edges:
            raise ValueError(f"gather_rows: expected {self.parent.N} node rows and {self.parent_edges} edge rows, got {x.size(0)} and {e.size(0)}")
        if (x.size(1) & 3) or (e.size(1) & 3):
            raise ValueError(f"gather_rows: row widths must be multiples of 4, got {x.size(1)} and {e.size(1)}")
        n, m = self.node_src.numel(), self.edge_src.numel()
        xo = torch.empty(n, x.size(1), dtype=torch.float32, device=x.device)
        eo = torch.empty(m, e.size(1), dtype=torch.float32, device=e.device)
        # (pointers of EMPTY tensors are null: the entry point does not look at a half without rows)
        _lib.check(lib.isg_instance_rows(px, x.stride(0), x.size(0), self.node_src.data_ptr(), n, xo.data_ptr(), x.size(1), x.size(1),
                                         pe, e.stride(0), e.size(0), self.edge_src.data_ptr(), m, eo.data_ptr(), e.size(1), e.size(1),
                                         _stream()), "isg_instance_rows")
        return xo, eo

    def plan(self) -> "GraphPlan":
        """The GraphPlan of the instance batch (num_graphs = Q).  An instance is a copy of a graph of the parent, so the parent's
        bounds serve as hints; with host sizes the list of graphs beyond a tile is made without a device-to-host sync too."""
        if self._plan is None:
            self._plan = GraphPlan.build(self.batch, self.edge_index, num_graphs=self.Q, max_nodes=self.parent.nmax,
                                         max_edges=self.parent.emax, graph_sizes=self.sizes_host)
        return self._plan

    def verify(self) -> None:
        """Read `status` (one device-to-host copy) and raise IsgError naming the flag that is set, or the sizes where the host's
        disagree with the device's.  The model paths never call it."""
        n, e, *flags = (int(v) for v in self.status.tolist())
        bad = [name for name, f in zip(INSTANCES_FLAGS, flags) if f]
        if bad:
            why = {"bad_index": "an index lies outside [0, G); that instance is empty",
                   "bad_grouping": "the edges of a graph are not contiguous and in graph order, or an edge leaves its graph"}
            raise _lib.IsgError("graph_instances: " + "; ".join(f"{b} ({why[b]})" for b in bad))
        if (n, e) != (self.node_src.numel(), self.edge_src.numel()):
            raise _lib.IsgError(f"graph_instances: the sizes given on the host make {self.node_src.numel()} nodes / "
                                f"{self.edge_src.numel()} edges, the device counted {n} / {e}")


def graph_instances(plan: "GraphPlan", edge_index: Tensor, index: Tensor, sizes: Optional[Tensor] = None) -> GraphInstances:
    """The batch of Q instances of the graphs index[q] of `plan`'s batch, expanded on the device (isg_instances_size: a 16-byte
    clear and two launches; isg_instances_fill: one).  plan: the distinct batch's GraphPlan, built from its batch vector;
    edge_index int64 [2, E], the edges of one graph contiguous and the graphs in order; index: int32 or int64 [Q], on the host or
    on the device.  sizes: HOST int64 [2, G] (nodes, edges per graph, what a collate knows): with it and a host index N' and E' are
    computed on the host; otherwise they come from one 8-byte device-to-host copy between the two passes."""
    lib = _lib_instances.load()
    p_ei = _chk(edge_index, "edge_index", torch.int64)
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"edge_index must be [2,E], got {tuple(edge_index.shape)}")
    if plan.batch is None:
        raise ValueError("graph_instances needs a GraphPlan built from the batch vector")
    N, E, G = plan.N, edge_index.size(1), plan.B
    p_batch = _chk(plan.batch, "plan.batch", torch.int64, (N,))
    p_ptr = _chk(plan.ptr, "plan.ptr", torch.int32, (G + 1,))
    if index.dim() != 1 or index.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"index: expected int32 or int64 [Q], got {index.dtype} {tuple(index.shape)}")
    dev = edge_index.device
    Q = index.numel()
    sizes_host = totals = None
    if sizes is not None:
        if sizes.device.type != "cpu" or tuple(sizes.shape) != (2, G):
            raise ValueError(f"sizes: a HOST tensor [2, {G}] (nodes, edges per graph), got {sizes.device} {tuple(sizes.shape)}")
        if index.device.type == "cpu":
            if Q and (int(index.min()) < 0 or int(index.max()) >= G):
                raise ValueError(f"index: values outside [0, {G})")
            sizes_host = sizes.long().index_select(1, index.long())
            totals = (int(sizes_host[0].sum()), int(sizes_host[1].sum()))
    idx = index.to(device=dev, dtype=torch.int32).contiguous()
    COUNTERS["graph_instances"] += 1
    ws_bytes = lib.isg_instances_workspace_bytes(G)
    n32 = 2 * (Q + 1) + 4
    i32 = torch.empty(n32 + (ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    ptr, eptr, status = i32[:Q + 1], i32[Q + 1:2 * Q + 2], i32[2 * Q + 2:n32]
    if Q == 0:
        i32[:n32].zero_()
        totals = (0, 0)
    b32 = i32.data_ptr()
    _lib.check(lib.isg_instances_size(p_ptr, p_batch, p_ei, idx.data_ptr(), N, E, G, Q, b32, b32 + 4 * (Q + 1), b32 + 8 * (Q + 1),
                                      b32 + 4 * n32, ws_bytes, _stream()), "isg_instances_size")
    if totals is None:
        n, e = status[:2].tolist()                  # the operator's only device-to-host copy
        totals = (int(n), int(e))
    Np, Ep = totals
    i64 = torch.empty(max(2 * Np + 3 * Ep, 1), dtype=torch.int64, device=dev)
    b64 = i64.data_ptr()
    _lib.check(lib.isg_instances_fill(p_ptr, p_ei, idx.data_ptr(), N, E, G, Q, b32, b32 + 4 * (Q + 1), b32 + 4 * n32, ws_bytes, Np, Ep,
                                      b64, b64 + 8 * (2 * Np), b64 + 8 * Np, b64 + 8 * (2 * Np + 2 * Ep), _stream()),
               "isg_instances_fill")
    return GraphInstances(plan, idx, ptr, eptr, i64[:Np], i64[2 * Np:2 * Np + 2 * Ep].view(2, Ep), i64[Np:2 * Np],
                          i64[2 * Np + 2 * Ep:2 * Np + 3 * Ep], status, sizes_host, E, erange=i32[n32:n32 + G + 1] if Q else None,
                          index_host=index if index.device.type == "cpu" else None)


def instance_rows_backward(inst: GraphInstances, g_x: Tensor, g_e: Tensor) -> Tuple[Tensor, Tensor]:
    """The backward of GraphInstances.gather_rows in ONE launch (isg_instance_rows_bwd): g_x fp32 [N', Cx] and g_e fp32 [E', Ce],
    gradients of the instance batch's rows -> (d_x [N, Cx], d_e [E, Ce]) of the parent batch's: per distinct row the sum of its
    copies' rows in ascending instance number, plain fp32 adds, no atomics -- two calls agree bit for bit.  Every row is written;
    the rows of a graph that no instance names are +0."""
    lib = _ext_instances_train.load()
    pgx, pge = _chk_rows(g_x, "g_x"), _chk_rows(g_e, "g_e")
    n, m = inst.node_src.numel(), inst.edge_src.numel()
    if g_x.size(0) != n or g_e.size(0) != m:
        raise ValueError(f"instance_rows_backward: expected {n} node rows and {m} edge rows, got {g_x.size(0)} and {g_e.size(0)}")
    if (g_x.size(1) & 3) or (g_e.size(1) & 3):
        raise ValueError(f"instance_rows_backward: row widths must be multiples of 4, got {g_x.size(1)} and {g_e.size(1)}")
    N, E, G, Q = inst.parent.N, inst.parent_edges, inst.parent.B, inst.Q
    dx = torch.empty(N, g_x.size(1), dtype=torch.float32, device=g_x.device)
    de = torch.empty(E, g_e.size(1), dtype=torch.float32, device=g_e.device)
    if Q == 0 or inst.erange is None:            # nothing was expanded: no copies, every sum is empty
        return dx.zero_(), de.zero_()
    gptr, glist = inst.by_graph()
    COUNTERS["instance_rows_bwd"] += 1
    _lib.check(lib.isg_instance_rows_bwd(pgx, g_x.stride(0), n, dx.data_ptr(), g_x.size(1), N, g_x.size(1),
                                         pge, g_e.stride(0), m, de.data_ptr(), g_e.size(1), E, g_e.size(1),
                                         _chk(inst.parent.ptr, "plan.ptr", torch.int32, (G + 1,)),
                                         _chk(inst.erange, "erange", torch.int32, (G + 1,)),
                                         _chk(inst.ptr, "inst.ptr", torch.int32, (Q + 1,)), _chk(inst.eptr, "inst.eptr", torch.int32, (Q + 1,)),
                                         _chk(gptr, "gptr", torch.int32, (G + 1,)), _chk(glist, "glist", torch.int32, (Q,)), G, Q,
                                         _stream()), "isg_instance_rows_bwd")
    return dx, de


# ------------------------------------------------------------------------------------------------
# Attention rollout: the read-out's weights walked back through the layers' attention weights
# ------------------------------------------------------------------------------------------------
ROLLOUT_MAX_LAYERS = 8      # isg_rollout_max_layers() (ROLL_MAX_LAYERS in csrc/isg_rollout.hip)


def attention_rollout(plan: "GraphPlan", alphas, start: Tensor, masks=None, residual: float = 0.5,
                      want_flow: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """(relevance fp32 [N], flow fp32 [L, E] or None) of isg_attention_rollout (include/ext/isg_rollout.h, where the function is
    stated): one launch, one wave per graph.  plan: the batch's GraphPlan, built with edge_index (its CSR by source is built on
    first use); alphas: L fp32 [E, H] tensors in edge-id order, columns contiguous, the row stride free (a layer kernel's
    `alpha`, or a column slice of a wider tensor); start fp32 [N] or [N, 1]; masks: None, or L entries each None or fp32 [N] /
    [N, 1] (the layer's node mask); residual: the share of a node's relevance that stays on it at every layer, in [0, 1].
    flow[l, e] is what edge e carried at layer l (zero for an edge that was skipped)."""
    lib = _ext_rollout.load()
    plan.require_csr()
    alphas = list(alphas)
    L, N, E, B = len(alphas), plan.N, plan.E, plan.B
    if not 1 <= L <= ROLLOUT_MAX_LAYERS:
        raise _lib.IsgError(f"attention_rollout: {L} layers (1 to {ROLLOUT_MAX_LAYERS})")
    if masks is None:
        masks = [None] * L
    masks = list(masks)
    if len(masks) != L:
        raise ValueError(f"masks: expected None or {L} entries (one per layer, each a tensor or None), got {len(masks)}")
    if not 0.0 <= float(residual) <= 1.0:            # (a NaN compares false)
        raise ValueError(f"residual: expected a share in [0, 1], got {residual}")
    if start.dim() == 2 and start.size(1) == 1:
        start = start.reshape(-1)
    p_start = _chk(start, "start", torch.float32, (N,))
    H = alphas[0].size(1) if alphas[0].dim() == 2 else 0
    if H < 1:
        raise ValueError(f"alphas[0]: expected fp32 [{E}, H] with H >= 1, got {tuple(alphas[0].shape)}")
    fields, keep = [], []
    for l, (al, m) in enumerate(zip(alphas, masks)):
        if not al.is_cuda:
            raise _lib.IsgError(f"alphas[{l}] must live on the GPU (got {al.device}); this path has no CPU fallback")
        if al.dtype != torch.float32 or tuple(al.shape) != (E, H) or (E > 0 and (al.stride(1) != 1 or al.stride(0) < H)):
            raise ValueError(f"alphas[{l}]: expected fp32 [{E}, {H}] with contiguous columns, got {al.dtype} {tuple(al.shape)} "
                             f"with strides {tuple(al.stride())}")
        if _rec(al):
            raise NotImplementedError(f"alphas[{l}] requires grad but this operator has no backward; wrap the call in "
                                      "torch.no_grad() or detach the input")
        if m is not None:
            if m.dim() == 2 and m.size(1) == 1:
                m = m.reshape(-1)
            m = _f32(m)
            keep.append(m)
        fields += [al.data_ptr() if E > 0 else 0, al.stride(0) if E > 1 else H, _chk(m, f"masks[{l}]", torch.float32, (N,), optional=True)]
    dev = start.device
    by_src = plan.source_csr() if N > 0 else (plan.rowptr, plan.eid, plan.dst)
    p_ptr = _chk(plan.ptr, "plan.ptr", torch.int32, (B + 1,))
    COUNTERS["attention_rollout"] += 1
    relevance = torch.empty(N, dtype=torch.float32, device=dev)
    flow = torch.zeros(L, E, dtype=torch.float32, device=dev) if want_flow else None
    import ctypes
    table = (ctypes.c_int64 * len(fields))(*fields)
    _lib.check(lib.isg_attention_rollout(p_ptr, by_src[0].data_ptr(), by_src[1].data_ptr(), by_src[2].data_ptr(),
                                         ctypes.addressof(table), L, H, float(residual), p_start, N, E, B, plan.nmax,
                                         relevance.data_ptr(), 0 if flow is None else flow.data_ptr(), _stream()),
               "isg_attention_rollout")
    return relevance, flow


# ------------------------------------------------------------------------------------------------
# Integrated gradients: the path's rows as one instance batch, its gradient rows reduced to attributions
# ------------------------------------------------------------------------------------------------
class IgAttribution(NamedTuple):
    attr_x: Tensor               # fp32 [N]: the attribution of every node of the parent batch
    attr_e: Optional[Tensor]     # fp32 [E], or None when the edge half was skipped
    avg_x: Optional[Tensor]      # fp32 [N, Cx]: the weighted sum of every node's gradient rows; None unless asked for
    avg_e: Optional[Tensor]      # fp32 [E, Ce]


def _ig_base(base: Optional[Tensor], rows: int, C: int, name: str) -> Tuple[int, int]:
    """(address, row stride) of a baseline: None -> (0, 0); fp32 [C] -> one row, stride 0; fp32 [rows, C] -> its rows."""
    if base is None:
        return 0, 0
    if base.dim() == 1:
        return _chk(base, name, torch.float32, (C,)), 0
    p = _chk_rows(base, name)
    if tuple(base.shape) != (rows, C):
        raise ValueError(f"{name}: expected None, fp32 [{C}] or fp32 [{rows}, {C}], got {tuple(base.shape)}")
    return p, _ld(base)


def _ig_rows(inst: GraphInstances, x: Tensor, e: Tensor, what: str) -> Tuple[int, int]:
    px, pe = _chk_rows(x, "x"), _chk_rows(e, "e")
    if x.size(0) != inst.parent.N or e.size(0) != inst.parent_edges:
        raise ValueError(f"{what}: expected {inst.parent.N} node rows and {inst.parent_edges} edge rows, got {x.size(0)} and {e.size(0)}")
    if (x.size(1) & 3) or (e.size(1) & 3):
        raise ValueError(f"{what}: row widths must be multiples of 4, got {x.size(1)} and {e.size(1)}")
    return px, pe


def _ld(t: Tensor) -> int:
    """The row stride the entry points are told.  A tensor of fewer than two rows may carry any (an expanded [1, C] gradient
    has 0 and still counts as contiguous); its width serves."""
    return t.stride(0) if t.size(0) > 1 else t.size(1)


def ig_path_rows(inst: GraphInstances, x: Tensor, e: Tensor, t: Tensor, base_x: Optional[Tensor] = None,
                 base_e: Optional[Tensor] = None, path_edges: bool = False) -> Tuple[Tensor, Tensor]:
    """(x_inst [N', Cx], e_inst [E', Ce]) of isg_ig_path_rows (include/ext/isg_ig.h, where the function is stated): instance q's
    rows are the point t[q] of the straight path from the baseline to the input, x_inst[i] = t x[node_src[i]] + (1 - t) base, in
    ONE launch.  x fp32 [N, Cx], e fp32 [E, Ce] (strided rows as gather_rows takes them); t fp32 [Q] on the device; a baseline
    is None (zeros), one row [C] or rows [rows, C].  path_edges=False copies the edge rows (they stay at the input; base_e is
    then not looked at).  No backward: a tensor that requires grad raises."""
    lib = _ext_ig.load()
    px, pe = _ig_rows(inst, x, e, "ig_path_rows")
    Q, Cx, Ce = inst.Q, x.size(1), e.size(1)
    pt = _chk(t, "t", torch.float32, (Q,))
    pbx, ldbx = _ig_base(base_x, x.size(0), Cx, "base_x")
    pbe, ldbe = _ig_base(base_e, e.size(0), Ce, "base_e") if path_edges else (0, 0)
    n, m = inst.node_src.numel(), inst.edge_src.numel()
    xo = torch.empty(n, Cx, dtype=torch.float32, device=x.device)
    eo = torch.empty(m, Ce, dtype=torch.float32, device=e.device)
    einst = inst.batch.index_select(0, inst.edge_index[0]) if path_edges and m > 0 else None      # the instance of every edge row
    COUNTERS["ig_path_rows"] += 1
    _lib.check(lib.isg_ig_path_rows(px, _ld(x), x.size(0), pbx, ldbx, inst.node_src.data_ptr(), inst.batch.data_ptr(), n,
                                    xo.data_ptr(), Cx, Cx,
                                    pe, _ld(e), e.size(0), pbe, ldbe, inst.edge_src.data_ptr(),
                                    0 if einst is None else einst.data_ptr(), m, eo.data_ptr(), Ce, Ce,
                                    pt, Q, 1 if path_edges else 0, _stream()), "isg_ig_path_rows")
    return xo, eo


def ig_attribution(inst: GraphInstances, g_x: Tensor, g_e: Optional[Tensor], w: Tensor, x: Tensor, e: Tensor,
                   base_x: Optional[Tensor] = None, base_e: Optional[Tensor] = None, want_rows: bool = False,
                   out: Optional[IgAttribution] = None) -> IgAttribution:
    """isg_ig_attribution (include/ext/isg_ig.h, where the function and its order of operations are stated) in ONE launch: g_x
    fp32 [N', Cx] (and g_e fp32 [E', Ce], or None: the edge half is skipped) are the gradients of the instance batch's rows, w
    fp32 [Q] the quadrature weight of every instance; per row of the parent batch the weighted sum of its copies' gradient rows,
    dotted with (x - base).  want_rows also returns those weighted sums (avg_x, avg_e).  out=: a previous result of the same
    shapes, which this call adds to (a path forwarded in chunks) and returns.  No atomics; two calls agree bit for bit."""
    lib = _ext_ig.load()
    px, pe = _ig_rows(inst, x, e, "ig_attribution")
    N, E, G, Q, Cx, Ce = inst.parent.N, inst.parent_edges, inst.parent.B, inst.Q, x.size(1), e.size(1)
    n, m = inst.node_src.numel(), inst.edge_src.numel()
    edges = g_e is not None
    pgx = _chk_rows(g_x, "g_x")
    pge = _chk_rows(g_e, "g_e") if edges else 0
    if tuple(g_x.shape) != (n, Cx) or (edges and tuple(g_e.shape) != (m, Ce)):
        raise ValueError(f"ig_attribution: expected gradient rows [{n}, {Cx}] and [{m}, {Ce}] (or None), got {tuple(g_x.shape)} and "
                         f"{None if g_e is None else tuple(g_e.shape)}")
    pw = _chk(w, "w", torch.float32, (Q,))
    pbx, ldbx = _ig_base(base_x, N, Cx, "base_x")
    pbe, ldbe = _ig_base(base_e, E, Ce, "base_e") if edges else (0, 0)
    dev = x.device
    if out is None:
        attr_x = torch.empty(N, dtype=torch.float32, device=dev)
        attr_e = torch.empty(E, dtype=torch.float32, device=dev) if edges else None
        avg_x = torch.empty(N, Cx, dtype=torch.float32, device=dev) if want_rows else None
        avg_e = torch.empty(E, Ce, dtype=torch.float32, device=dev) if want_rows and edges else None
    else:
        attr_x, attr_e, avg_x, avg_e = out
        if (attr_e is not None) != edges or (avg_x is not None) != bool(want_rows):
            raise ValueError("ig_attribution: `out` was made with another g_e / want_rows")
        _chk(attr_x, "out.attr_x", torch.float32, (N,))
        if edges:
            _chk(attr_e, "out.attr_e", torch.float32, (E,))
        if want_rows:
            _chk(avg_x, "out.avg_x", torch.float32, (N, Cx))
            if edges:
                _chk(avg_e, "out.avg_e", torch.float32, (E, Ce))
    res = IgAttribution(attr_x, attr_e, avg_x, avg_e)
    if Q == 0 or inst.erange is None:            # nothing was expanded: no copies, every sum is empty
        if out is None:
            for t_ in res:
                if t_ is not None:
                    t_.zero_()
        return res
    gptr, glist = inst.by_graph()
    COUNTERS["ig_attribution"] += 1
    _lib.check(lib.isg_ig_attribution(pgx, _ld(g_x), n, px, _ld(x), pbx, ldbx, attr_x.data_ptr(),
                                      0 if avg_x is None else avg_x.data_ptr(), Cx, N, Cx,
                                      pge, _ld(g_e) if edges else Ce, m if edges else 0, pe, _ld(e), pbe, ldbe,
                                      attr_e.data_ptr() if edges else 0, 0 if avg_e is None else avg_e.data_ptr(), Ce,
                                      E if edges else 0, Ce,
                                      pw, _chk(inst.parent.ptr, "plan.ptr", torch.int32, (G + 1,)),
                                      _chk(inst.erange, "erange", torch.int32, (G + 1,)),
                                      _chk(inst.ptr, "inst.ptr", torch.int32, (Q + 1,)), _chk(inst.eptr, "inst.eptr", torch.int32, (Q + 1,)),
                                      _chk(gptr, "gptr", torch.int32, (G + 1,)), _chk(glist, "glist", torch.int32, (Q,)), G, Q,
                                      0 if out is None else 1, _stream()), "isg_ig_attribution")
    return res


# ------------------------------------------------------------------------------------------------
# Mask optimisation: one iteration's arithmetic of a GNNExplainer run as one launch
# ------------------------------------------------------------------------------------------------
def adam_bias_corrections(step: int, betas=(0.9, 0.999)) -> Tuple[float, float]:
    """(1 - beta1^step, 1 - beta2^step) in double, as isg_mt_adam's prologue forms them (include/isg_optim.h)."""
    if isinstance(step, bool) or int(step) != step or int(step) < 1:
        raise ValueError(f"step must be an integer >= 1, got {step!r}")
    return 1.0 - float(betas[0]) ** int(step), 1.0 - float(betas[1]) ** int(step)


def maskopt_step(x: Tensor, g: Optional[Tensor], seg: Tensor, theta: Tensor, exp_avg: Optional[Tensor],
                 exp_avg_sq: Optional[Tensor], *, step: int, a_size: float = 1.0, a_ent: float = 0.1, lr: float = 0.01,
                 betas=(0.9, 0.999), eps: float = 1e-8, out: Optional[Tensor] = None, want_grad: bool = False
                 ) -> Tuple[Tensor, Optional[Tensor]]:
    """(x_masked [N, C], d_theta [N] or None) of isg_maskopt_step (include/ext/isg_maskopt.h, where the function and its order of
    operations are stated) in ONE launch: x fp32 [N, C] the unmasked rows, g fp32 [N, C] the gradient of the summed loss with
    respect to the masked rows (strided rows as gather_rows takes them), seg int32 [B + 1] the range starts of the rows' segments
    (plan.ptr for node rows), theta / exp_avg / exp_avg_sq fp32 [N] updated IN PLACE by Adam's step number `step` (>= 1).
    g=None is the apply-only form: nothing is updated (the moments may be None), x_masked = sigmoid(theta) * x.
    out=: an fp32 [N, C] tensor to write the masked rows to; want_grad also returns d theta.  No backward: a tensor that requires
    grad raises.  No atomics; two calls agree bit for bit."""
    lib = _ext_maskopt.load()
    px = _chk_rows(x, "x")
    N, C = x.size(0), x.size(1)
    if C & 3:
        raise ValueError(f"maskopt_step: the row width must be a multiple of 4, got {C}")
    pg, ldg = 0, C
    if g is not None:
        pg, ldg = _chk_rows(g, "g"), _ld(g)
        if tuple(g.shape) != (N, C):
            raise ValueError(f"maskopt_step: expected gradient rows [{N}, {C}], got {tuple(g.shape)}")
    if seg.dim() != 1 or seg.numel() < 1:
        raise ValueError(f"maskopt_step: seg is int32 [B + 1], got {tuple(seg.shape)}")
    B = seg.numel() - 1
    pseg = _chk(seg, "seg", torch.int32)
    pth = _chk(theta, "theta", torch.float32, (N,))
    pm = _chk(exp_avg, "exp_avg", torch.float32, (N,), optional=g is None)
    pv = _chk(exp_avg_sq, "exp_avg_sq", torch.float32, (N,), optional=g is None)
    bc1, bc2 = adam_bias_corrections(step, betas)
    if out is None:
        out = torch.empty(N, C, dtype=torch.float32, device=x.device)
    po = _chk_rows(out, "out")
    if tuple(out.shape) != (N, C):
        raise ValueError(f"maskopt_step: expected out [{N}, {C}], got {tuple(out.shape)}")
    d_theta = torch.empty(N, dtype=torch.float32, device=x.device) if want_grad and g is not None else None
    COUNTERS["maskopt_step"] += 1
    _lib.check(lib.isg_maskopt_step(px, _ld(x), pg, ldg, pseg, B, pth, pm, pv, po, _ld(out),
                                    0 if d_theta is None else d_theta.data_ptr(), N, C, float(a_size), float(a_ent), float(lr),
                                    float(betas[0]), float(betas[1]), float(eps), bc1, bc2, _stream()), "isg_maskopt_step")
    return out, d_theta


# ------------------------------------------------------------------------------------------------
# Induced-subgraph instances: every instance a graph of the parent batch minus some of its nodes
# ------------------------------------------------------------------------------------------------
INDUCED_WORDS_MAX = 64      # words of keep bits per instance, one per lane of the instance's wave (IND_WORDS_MAX in csrc/isg_induced.hip)


class InducedInstances(GraphInstances):
    """What isg_induced_size / isg_induced_fill left on the device (include/ext/isg_induced.h): instance q is graph index[q] of
    the parent batch with the nodes its row of `keep` names, and the edges among them.  The fields are GraphInstances'; node_src /
    edge_src name the parent row of every instance row, so gather_nodes / gather_edges / gather_rows (without autograd), plan()
    and verify() work as on the parent class -- an instance is no larger than its graph, the parent's bounds stay valid hints.
    keep uint32 [Q, W] on the device, or None (every node kept).

    These are inference forms: the instance-row backward assumes whole copies of a graph's rows at computable addresses, so
    gather_rows under autograd, by_graph() and counts() raise."""

    def __init__(self, *args, keep=None, **kw):
        super().__init__(*args, **kw)
        self.keep = keep

    def gather_rows(self, x: Tensor, e: Tensor) -> Tuple[Tensor, Tensor]:
        if _rec(x, e):
            raise NotImplementedError("InducedInstances.gather_rows has no backward (the instance-row backward assumes whole copies "
                                      "of a graph); wrap the call in torch.no_grad() or detach the inputs")
        return super().gather_rows(x, e)

    def by_graph(self):
        raise NotImplementedError("InducedInstances.by_graph: the instances of a graph are no copies of it (an inference form)")

    def counts(self):
        raise NotImplementedError("InducedInstances.counts: the instances of a graph are no copies of it (an inference form)")


def induced_instances(plan: "GraphPlan", edge_index: Tensor, index: Tensor, keep: Optional[Tensor],
                      sizes: Optional[Tensor] = None) -> InducedInstances:
    """The batch of Q induced-subgraph instances in one pass on the device (isg_induced_size: a 16-byte clear and three launches;
    isg_induced_fill: one).  plan: the parent batch's GraphPlan, built from its batch vector; edge_index int64 [2, E], the edges
    of one graph contiguous and the graphs in order; index int32 or int64 [Q], on the host or on the device; keep uint32-as-int32
    [Q, W] on the device (bit i & 31 of word i >> 5 of row q: local node i of graph index[q] is in instance q; W <= 64), or None:
    every node is kept and the result is ops.graph_instances'.  N' and E' come from one 16-byte device-to-host copy between the
    passes (E' depends on the bits: it cannot be known on the host).  sizes: HOST int64 [2, G] (nodes, edges per graph); it is
    only checked -- the instances' own sizes are not known on the host, so the plan of the instance batch is built without them."""
    lib = _ext_induced.load()
    p_ei = _chk(edge_index, "edge_index", torch.int64)
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"edge_index must be [2,E], got {tuple(edge_index.shape)}")
    if plan.batch is None:
        raise ValueError("induced_instances needs a GraphPlan built from the batch vector")
    N, E, G = plan.N, edge_index.size(1), plan.B
    p_batch = _chk(plan.batch, "plan.batch", torch.int64, (N,))
    p_ptr = _chk(plan.ptr, "plan.ptr", torch.int32, (G + 1,))
    if index.dim() != 1 or index.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"index: expected int32 or int64 [Q], got {index.dtype} {tuple(index.shape)}")
    if sizes is not None and (sizes.device.type != "cpu" or tuple(sizes.shape) != (2, G)):
        raise ValueError(f"sizes: a HOST tensor [2, {G}] (nodes, edges per graph), got {sizes.device} {tuple(sizes.shape)}")
    dev = edge_index.device
    Q = index.numel()
    W, p_keep = 0, 0
    if keep is not None:
        if keep.dim() != 2 or keep.size(0) != Q or keep.dtype != torch.int32:
            raise ValueError(f"keep: expected int32 words [{Q}, W], got {keep.dtype} {tuple(keep.shape)}")
        W = keep.size(1)
        if not 1 <= W <= INDUCED_WORDS_MAX:
            raise _lib.IsgError(f"keep: {W} words per instance (1 to {INDUCED_WORDS_MAX}: {32 * INDUCED_WORDS_MAX} nodes per graph)")
        p_keep = _chk(keep, "keep", torch.int32) if Q else 0
    idx = index.to(device=dev, dtype=torch.int32).contiguous()
    COUNTERS["induced_instances"] += 1
    ws_bytes = lib.isg_induced_workspace_bytes(G, Q)
    n32 = 2 * (Q + 1) + 4
    i32 = torch.empty(n32 + (ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    ptr, eptr, status = i32[:Q + 1], i32[Q + 1:2 * Q + 2], i32[2 * Q + 2:n32]
    b32 = i32.data_ptr()
    if Q == 0:
        i32[:n32].zero_()
        Np = Ep = 0
    else:
        _lib.check(lib.isg_induced_size(p_ptr, p_batch, p_ei, idx.data_ptr(), p_keep, W, N, E, G, Q, b32, b32 + 4 * (Q + 1),
                                        b32 + 8 * (Q + 1), b32 + 4 * n32, ws_bytes, _stream()), "isg_induced_size")
        Np, Ep = (int(v) for v in status.tolist()[:2])          # the operator's only device-to-host copy: the 16 bytes of status
    i64 = torch.empty(max(2 * Np + 3 * Ep, 1), dtype=torch.int64, device=dev)
    b64 = i64.data_ptr()
    _lib.check(lib.isg_induced_fill(p_ptr, p_ei, idx.data_ptr(), p_keep, W, N, E, G, Q, b32, b32 + 4 * (Q + 1), b32 + 4 * n32,
                                    ws_bytes, Np, Ep, b64, b64 + 8 * (2 * Np), b64 + 8 * Np, b64 + 8 * (2 * Np + 2 * Ep), _stream()),
               "isg_induced_fill")
    return InducedInstances(plan, idx, ptr, eptr, i64[:Np], i64[2 * Np:2 * Np + 2 * Ep].view(2, Ep), i64[Np:2 * Np],
                            i64[2 * Np + 2 * Ep:2 * Np + 3 * Ep], status, None, E, erange=i32[n32:n32 + G + 1] if Q else None,
                            index_host=index if index.device.type == "cpu" else None, keep=keep)


def keep_words(max_nodes: int) -> int:
    """Words of 32 keep bits that hold graphs of up to max_nodes nodes (at least one)."""
    return max(1, (int(max_nodes) + 31) // 32)


def _pack_bits(flags: Tensor, W: int) -> Tensor:
    """bool [R, 32 W] -> int32 [R, W]: bit i & 31 of word i >> 5.  The sum runs in int64 and wraps into the int32 word."""
    shifts = torch.arange(32, dtype=torch.int64, device=flags.device)
    words = (flags.view(flags.size(0), W, 32).long() << shifts).sum(dim=2)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()


def keep_bits_leave_one_out(plan: "GraphPlan", graphs: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(index int32 [Q], keep int32 [Q, W], inst_node int64 [Q]) of the leave-one-out batch, made with torch ops on the plan's
    device (O(Q W) words): graph g gets n_g instances, instance j of them lacks local node j, inst_node is the removed node's row
    in the parent batch; the instances of a graph are consecutive, the graphs in order.  A graph with fewer than 2 nodes gets no
    instance (removing its node would leave an empty graph).  graphs: int64 [B'] -- only these graphs, in this order.
    W = keep_words(plan.nmax).  One device-to-host copy (Q, to size the result)."""
    ptr = plan.ptr.long()
    n = ptr[1:] - ptr[:-1]
    g_all = torch.arange(plan.B, dtype=torch.int64, device=ptr.device) if graphs is None else graphs.to(ptr.device).long()
    reps = n.index_select(0, g_all)
    reps = torch.where(reps >= 2, reps, torch.zeros_like(reps))
    index = torch.repeat_interleave(g_all, reps)                 # (the copy: the output's length)
    Q = index.numel()
    first = torch.cumsum(reps, 0) - reps                         # the first instance of every listed graph
    local = torch.arange(Q, dtype=torch.int64, device=ptr.device) - torch.repeat_interleave(first, reps, output_size=Q)
    W = keep_words(plan.nmax)
    bit = torch.arange(32 * W, dtype=torch.int64, device=ptr.device).view(1, -1)
    flags = (bit < n.index_select(0, index).view(-1, 1)) & (bit != local.view(-1, 1))
    return index.to(torch.int32), _pack_bits(flags, W), ptr.index_select(0, index) + local


def keep_bits_from_mask(mask: Tensor, plan: "GraphPlan", threshold: float = 0.0, complement: bool = False) -> Tensor:
    """keep int32 [B, W] for ops.induced_instances with the identity index: bit i of row g is (mask[ptr[g] + i] > threshold) !=
    complement, ops.subgraph_cut's rule (a NaN compares false).  mask fp32 [N] or [N, 1]; W = keep_words(plan.nmax)."""
    flat = mask.reshape(-1)
    if flat.numel() != plan.N:
        raise ValueError(f"mask: expected {plan.N} entries, got {flat.numel()}")
    if plan.batch is None:
        raise ValueError("keep_bits_from_mask needs a GraphPlan built from the batch vector")
    W = keep_words(plan.nmax)
    batch = plan.batch.long()
    local = torch.arange(plan.N, dtype=torch.int64, device=flat.device) - plan.ptr.long().index_select(0, batch)
    flags = torch.zeros(plan.B, 32 * W, dtype=torch.bool, device=flat.device)
    inside = local < 32 * W
    flags[batch[inside], local[inside]] = ((flat > threshold) != bool(complement))[inside]
    return _pack_bits(flags, W)


# ------------------------------------------------------------------------------------------------
# Fidelity curves: ranked keep bits for every level and side, and the curves' sums
# ------------------------------------------------------------------------------------------------
CURVE_LEVELS_MAX = 64       # levels per call (CV_LEVELS_MAX in csrc/isg_curves.hip)
CURVE_SIDES = ("keep", "remove")


def _curve_sides(sides) -> int:
    names = (sides,) if isinstance(sides, str) else tuple(sides)
    if not names or len(set(names)) != len(names) or any(s not in CURVE_SIDES for s in names):
        raise ValueError(f"sides: one or both of {CURVE_SIDES}, each once, got {sides!r}")
    return sum(1 << CURVE_SIDES.index(s) for s in names)


@dataclass
class CurveBits:
    """What isg_curve_keep_bits left on the device (include/ext/isg_curves.h): row q = (r L + j) S + s is listed graph r at level
    j on side s (the keep side first when both are asked for)."""
    index: Tensor                  # int32 [R L S]: the graph of every row -- ops.induced_instances' index
    keep: Tensor                   # int32 words [R L S, W]: the keep bits of every row -- ops.induced_instances' keep
    rank: Tensor                   # int32 [N]: the rank of every node of a listed graph inside its graph (0 = the best); -1 elsewhere
    level_k: Tensor                # int32 [R, L, S]: the nodes ranked into (keep) or out of (remove) every row
    status: Tensor                 # int32 [4]: a graph beyond 32 W nodes, a listed graph outside the batch, R L S, 0
    graphs: Tensor                 # int32 [R] on the device: the listed graphs
    L: int
    S: int
    sides: int                     # the header's bits: 1 keep, 2 remove

    @property
    def R(self) -> int:
        return self.graphs.numel()

    def verify(self) -> "CurveBits":
        """Checks on the host (copies): both status flags are clear, every row holds exactly the bits its level_k promises and
        none beyond its graph, and the rows of a graph and side are nested along ascending level sizes."""
        st = self.status.tolist() if self.R and self.L else [0, 0, 0, 0]
        if st[0] or st[1]:
            raise _lib.IsgError(f"curve_keep_bits: status {st} (a graph beyond 32 W nodes / a listed graph outside the batch)")
        if not (self.R and self.L):
            return self
        words = self.keep.cpu().long() & 0xFFFFFFFF
        pop = torch.zeros(words.size(0), dtype=torch.int64)
        for b in range(32):
            pop += ((words >> b) & 1).sum(dim=1)
        k = self.level_k.cpu().long().reshape(self.R, self.L, self.S)
        pop = pop.view(self.R, self.L, self.S)
        words = words.view(self.R, self.L, self.S, -1)
        for s in range(self.S):
            removal = s == 1 or not (self.sides & 1)
            n = (pop[:, :, s] + k[:, :, s]) if removal else None
            if removal and not bool((n == n[:, :1]).all()):
                raise _lib.IsgError("curve_keep_bits: a remove row's bits and its level size do not add up to the graph's nodes")
            if not removal and not bool((pop[:, :, s] == k[:, :, s]).all()):
                raise _lib.IsgError("curve_keep_bits: a keep row does not hold exactly level_k bits")
            order = torch.argsort(k[:, :, s], dim=1, stable=True)
            w = torch.gather(words[:, :, s], 1, order.unsqueeze(-1).expand(-1, -1, words.size(-1)))
            small, large = (w[:, 1:], w[:, :-1]) if removal else (w[:, :-1], w[:, 1:])
            if bool((small & ~large).any()):
                raise _lib.IsgError("curve_keep_bits: the rows of a graph are not nested")
        return self


def curve_keep_bits(a: Tensor, plan: "GraphPlan", *, graphs: Optional[Tensor] = None, fractions=None, counts=None,
                    sides=CURVE_SIDES) -> CurveBits:
    """The ranking of every listed graph's nodes by the scores a (fp32 [N], higher = more important; ties to the lower node, NaNs
    last) and the keep rows of all levels and sides in ONE launch (isg_curve_keep_bits, include/ext/isg_curves.h, where the rank
    relation, the level rule and the row layout are stated).  Exactly one of fractions (shares of a graph's nodes:
    ceil(fp32(f) * fp32(n)), one fp32 product) and counts (numbers of nodes), at most 64 levels.  A keep row holds
    min(n, max(1, t)) nodes, a remove row lacks min(n - 1, max(0, t)): no instance is empty.  Rank prefixes hold EXACTLY k
    nodes -- unlike ops.topk_threshold, under which ties at the k-th value keep more.
    graphs: int32 / int64 [R], these graphs in this order; None: the graphs with at least one node, which costs one device-to-host
    copy (R, to size the result), as in keep_bits_leave_one_out.  W = keep_words(plan.nmax)."""
    import ctypes
    lib = _ext_curves.load()
    flat = a.reshape(-1)
    N, G = plan.N, plan.B
    p_a = _chk(flat, "a", torch.float32, (N,))
    p_ptr = _chk(plan.ptr, "plan.ptr", torch.int32, (G + 1,))
    if (fractions is None) == (counts is None):
        raise ValueError("curve_keep_bits: exactly one of fractions and counts")
    bits = _curve_sides(sides)
    S = bin(bits).count("1")
    if fractions is not None:
        vals = [float(f) for f in fractions]
        if any(not v >= 0.0 for v in vals):
            raise ValueError(f"curve_keep_bits: fractions are numbers >= 0, got {vals}")
        host = (ctypes.c_float * max(len(vals), 1))(*vals)
        p_frac, p_count = ctypes.addressof(host), 0
    else:
        vals = [operator.index(c) for c in counts]
        if any(v < 0 or v >= 2 ** 31 for v in vals):
            raise ValueError(f"curve_keep_bits: counts are int32 numbers >= 0, got {vals}")
        host = (ctypes.c_int32 * max(len(vals), 1))(*vals)
        p_frac, p_count = 0, ctypes.addressof(host)
    L = len(vals)
    if L > CURVE_LEVELS_MAX:
        raise _lib.IsgError(f"curve_keep_bits: {L} levels (at most {CURVE_LEVELS_MAX})")
    W = keep_words(plan.nmax)
    if W > INDUCED_WORDS_MAX:
        raise _lib.IsgError(f"curve_keep_bits: {W} words per row (at most {INDUCED_WORDS_MAX}: {32 * INDUCED_WORDS_MAX} nodes per graph)")
    dev = plan.ptr.device
    if graphs is None:
        listed = torch.nonzero(plan.ptr[1:] > plan.ptr[:-1]).reshape(-1).to(torch.int32)      # (the copy: the output's length)
    else:
        if graphs.dim() != 1 or graphs.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"graphs: expected int32 or int64 [R], got {graphs.dtype} {tuple(graphs.shape)}")
        listed = graphs.to(device=dev, dtype=torch.int32).contiguous()
    R = listed.numel()
    Q = R * L * S
    i32 = torch.empty(2 * Q + Q * W + 4, dtype=torch.int32, device=dev)
    level_k, index, keep, status = i32[:Q].view(R, L, S), i32[Q:2 * Q], i32[2 * Q:2 * Q + Q * W].view(Q, W), i32[2 * Q + Q * W:]
    rank = torch.full((N,), -1, dtype=torch.int32, device=dev)
    if not Q:
        status.zero_()
    COUNTERS["curve_keep_bits"] += 1
    _lib.check(lib.isg_curve_keep_bits(p_a, p_ptr, listed.data_ptr() if R else 0, p_frac, p_count, N, G, R, L, bits, W,
                                       rank.data_ptr() if N else 0, level_k.data_ptr(), index.data_ptr(), keep.data_ptr(),
                                       status.data_ptr(), _stream()), "isg_curve_keep_bits")
    return CurveBits(index, keep, rank, level_k, status, listed, L, S, bits)


def curve_sums(p_inst: Tensor, bits: CurveBits, w: Tensor, totals: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(auc fp32 [R, S], totals float64 [S, L + 3]) of isg_curve_sums (include/ext/isg_curves.h) in ONE launch: p_inst fp32
    [R L S], the predicted class's probability on every instance of `bits`, in its row order; w fp32 [L] on the device, the
    quadrature weights over the level axis.  auc[r, s] = the fma chain over ascending levels; totals (ACCUMULATED INTO; None: a
    fresh buffer of zeros) holds per side the L level sums, the sum of auc, the graphs counted and the graphs skipped.  A graph with
    a non-finite probability at any level of a side is skipped for that side and its auc is NaN.  Sums run over the rows in order:
    two calls agree bit for bit."""
    lib = _ext_curves.load()
    R, L, S = bits.R, bits.L, bits.S
    p_p = _chk(p_inst, "p_inst", torch.float32, (R * L * S,))
    p_w = _chk(w, "w", torch.float32, (L,))
    if totals is None:
        totals = torch.zeros(S, L + 3, dtype=torch.float64, device=p_inst.device)
    p_t = _chk(totals, "totals", torch.float64, (S, L + 3))
    auc = torch.empty(R, S, dtype=torch.float32, device=p_inst.device)
    COUNTERS["curve_sums"] += 1
    _lib.check(lib.isg_curve_sums(p_p, p_w, R, L, bits.sides, auc.data_ptr(), p_t, _stream()), "isg_curve_sums")
    return auc, totals


# ------------------------------------------------------------------------------------------------
# Shapley sampling: seeded permutations with the keep rows of their prefixes, and the estimates
# ------------------------------------------------------------------------------------------------
SHAPLEY_PERMUTATIONS_MAX = 1024     # permutations per call (SV_PERMUTATIONS_MAX in csrc/isg_shapley.hip)


@dataclass
class ShapleyBits:
    """What isg_shapley_keep_bits left on the device (include/ext/isg_shapley.h): row row_ptr[r] + m (n - 1) + (k - 1) holds the
    first k nodes of permutation m of listed graph r, for k = 1 .. n - 1."""
    index: Tensor                  # int32 [Q]: the graph of every row -- ops.induced_instances' index
    keep: Tensor                   # int32 words [Q, W]: the keep bits of every row -- ops.induced_instances' keep
    pos: Tensor                    # int32 [M, N]: every node's position in permutation m of its graph; -1 for nodes of unlisted graphs
    row_ptr: Tensor                # int32 [R + 1]: the first row of every listed graph
    status: Tensor                 # int32 [4]: a graph beyond 32 W nodes, a listed graph outside the batch, a bad row_ptr, Q
    graphs: Tensor                 # int32 [R] on the device: the listed graphs
    M: int                         # permutations per graph
    antithetic: bool               # permutation 2 t + 1 is permutation 2 t reversed

    @property
    def R(self) -> int:
        return self.graphs.numel()

    @property
    def Q(self) -> int:
        return self.index.numel()

    @property
    def T(self) -> int:
        """Samples per node: M, or M / 2 antithetic pairs."""
        return self.M // 2 if self.antithetic else self.M

    def verify(self) -> "ShapleyBits":
        """Checks on the host (copies): the three status flags are clear and status[3] is Q; every graph's pos rows are
        permutations, an antithetic twin the reversal; row k of a permutation holds exactly its first k nodes (so the rows of a
        permutation are nested) and no bit beyond its graph."""
        st = self.status.tolist() if self.R else [0, 0, 0, self.Q]
        if st[0] or st[1] or st[2] or st[3] != self.Q:
            raise _lib.IsgError(f"shapley_keep_bits: status {st} (a graph beyond 32 W nodes / a listed graph outside the batch / a bad "
                                f"row_ptr / Q = {self.Q})")
        if not self.R:
            return self
        words = self.keep.cpu().long() & 0xFFFFFFFF
        W = words.size(1) if words.dim() == 2 else 1
        first, index = self.row_ptr.tolist(), self.index.cpu()
        bit = torch.arange(32 * W, dtype=torch.int64)
        for r, g in enumerate(self.graphs.tolist()):
            rows, q0 = first[r + 1] - first[r], first[r]
            if not rows:
                continue
            n = rows // self.M + 1
            if not bool((index[q0:q0 + rows] == g).all()):
                raise _lib.IsgError("shapley_keep_bits: a row's index is not its graph")
            flags = ((words[q0:q0 + rows].view(rows, W, 1) >> torch.arange(32).view(1, 1, 32)) & 1).view(self.M, n - 1, 32 * W)
            if bool(flags[:, :, n:].any()) or not bool((flags.sum(dim=2) == torch.arange(1, n).view(1, -1)).all()):
                raise _lib.IsgError("shapley_keep_bits: row k of a permutation does not hold exactly k nodes of its graph")
            if bool((flags[:, :-1] & ~flags[:, 1:] & 1).any()):
                raise _lib.IsgError("shapley_keep_bits: the rows of a permutation are not nested")
            # the positions the rows imply: node i enters at the first k whose row holds it (n - 1 when no row does)
            implied = (n - 1) - flags[:, :, :n].sum(dim=1)
            if not bool((implied.sort(dim=1).values == bit[:n].view(1, -1)).all()):
                raise _lib.IsgError("shapley_keep_bits: a permutation's rows do not order its nodes")
            if self.antithetic and not bool((implied[1::2] == n - 1 - implied[0::2]).all()):
                raise _lib.IsgError("shapley_keep_bits: an antithetic twin is not the reversal")
        return self


def shapley_keep_bits(plan: "GraphPlan", *, graphs: Optional[Tensor] = None, permutations: int = 16, antithetic: bool = True,
                      seed: int = 0) -> ShapleyBits:
    """`permutations` seeded random permutations of every listed graph's nodes and the keep rows of all their proper prefixes in
    ONE launch (isg_shapley_keep_bits, include/ext/isg_shapley.h, where the keys, the position relation and the row layout are
    stated): graph r of n nodes gets permutations * (n - 1) rows, a graph of fewer than 2 nodes none.  antithetic: permutation
    2 t + 1 is permutation 2 t reversed (permutations is even).  A graph's permutations depend on seed and on its number in the
    batch alone, not on what is listed beside it.
    graphs: int32 / int64 [R], these graphs in this order; None: every graph of the batch.  row_ptr is formed with torch ops on
    the device; Q, its last entry, is the one small device-to-host copy (to size the result), as in keep_bits_leave_one_out.
    W = keep_words(plan.nmax)."""
    lib = _ext_shapley.load()
    N, G = plan.N, plan.B
    M = operator.index(permutations)
    anti = bool(antithetic)
    if not 1 <= M <= SHAPLEY_PERMUTATIONS_MAX:
        raise _lib.IsgError(f"shapley_keep_bits: {M} permutations (1 to {SHAPLEY_PERMUTATIONS_MAX})")
    if anti and M & 1:
        raise ValueError(f"shapley_keep_bits: antithetic permutations come in pairs, got permutations={M}")
    seed = operator.index(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"shapley_keep_bits: seed is a 64-bit number >= 0, got {seed}")
    p_ptr = _chk(plan.ptr, "plan.ptr", torch.int32, (G + 1,))
    W = keep_words(plan.nmax)
    if W > INDUCED_WORDS_MAX:
        raise _lib.IsgError(f"shapley_keep_bits: {W} words per row (at most {INDUCED_WORDS_MAX}: {32 * INDUCED_WORDS_MAX} nodes per graph)")
    dev = plan.ptr.device
    if graphs is None:
        listed = torch.arange(G, dtype=torch.int32, device=dev)
    else:
        if graphs.dim() != 1 or graphs.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"graphs: expected int32 or int64 [R], got {graphs.dtype} {tuple(graphs.shape)}")
        listed = graphs.to(device=dev, dtype=torch.int32).contiguous()
    R = listed.numel()
    row_ptr = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    if R and G:
        inside = (listed >= 0) & (listed < G)
        gl = listed.long().clamp(0, G - 1)
        ptr = plan.ptr.long().clamp(0, N)
        n = (torch.maximum(ptr[1:], ptr[:-1]) - ptr[:-1]).clamp(max=32 * W).index_select(0, gl)
        row_ptr[1:] = torch.cumsum(torch.where(inside, M * (n - 1).clamp(min=0), torch.zeros_like(n)), 0)
    Q = int(row_ptr[-1]) if R else 0                              # (the copy: the output's length)
    if Q >= 2 ** 31 - 1024:
        raise _lib.IsgError(f"shapley_keep_bits: {Q} rows (fewer than 2^31 - 1024): list fewer graphs per call or lower permutations")
    row_ptr = row_ptr.to(torch.int32)
    i32 = torch.empty(Q + Q * W + 4, dtype=torch.int32, device=dev)
    index, keep, status = i32[:Q], i32[Q:Q + Q * W].view(Q, W), i32[Q + Q * W:]
    pos = torch.full((M, N), -1, dtype=torch.int32, device=dev)
    if not R:
        status.zero_()
    COUNTERS["shapley_keep_bits"] += 1
    _lib.check(lib.isg_shapley_keep_bits(p_ptr, listed.data_ptr() if R else 0, row_ptr.data_ptr(), N, G, R, M, Q, int(anti), seed, W,
                                         pos.data_ptr() if N else 0, index.data_ptr() if Q else 0, keep.data_ptr() if Q else 0,
                                         status.data_ptr(), _stream()), "isg_shapley_keep_bits")
    return ShapleyBits(index, keep, pos, row_ptr, status, listed, M, anti)


def shapley_values(p_inst: Tensor, p: Tensor, bits: ShapleyBits, plan: "GraphPlan", v_empty: float = 0.0,
                   want_m2: bool = True) -> Tuple[Tensor, Optional[Tensor], Tensor, Tensor]:
    """(phi fp32 [N], m2 fp32 [N] or None, gap fp32 [R], flag int32 [R]) of isg_shapley_values (include/ext/isg_shapley.h, where
    the estimator and its arithmetic order are stated) in ONE launch: p_inst fp32 [Q], the predicted class's probability on every
    instance of `bits`, in its row order; p fp32 [B], that class's probability on the whole graph; v_empty: the value of the empty
    set (a finite float).  phi is the mean marginal contribution over the bits' permutations, m2 the sum of the squared samples,
    gap[r] = sum_i phi_i - (p[g] - v_empty); flag[r]: 0 fine, 1 a non-finite probability (phi, m2 and gap NaN), 2 a bad graphs or
    row_ptr entry (nothing written).  phi and m2 are 0 on the nodes of unlisted graphs.  Two calls agree bit for bit."""
    lib = _ext_shapley.load()
    N, G, R, M, Q = plan.N, plan.B, bits.R, bits.M, bits.Q
    p_pi = _chk(p_inst, "p_inst", torch.float32, (Q,))
    p_p = _chk(p, "p", torch.float32, (G,))
    p_ptr = _chk(plan.ptr, "plan.ptr", torch.int32, (G + 1,))
    p_pos = _chk(bits.pos, "bits.pos", torch.int32, (M, N))
    p_rp = _chk(bits.row_ptr, "bits.row_ptr", torch.int32, (R + 1,))
    v = float(v_empty)
    if not math.isfinite(v):
        raise ValueError(f"shapley_values: v_empty is a finite number, got {v_empty}")
    W = bits.keep.size(1) if bits.keep.dim() == 2 and bits.keep.size(1) else keep_words(plan.nmax)
    dev = p.device
    f32 = torch.zeros((2 if want_m2 else 1) * N + R, dtype=torch.float32, device=dev)
    phi, m2, gap = f32[:N], (f32[N:2 * N] if want_m2 else None), f32[(2 if want_m2 else 1) * N:]
    flag = torch.zeros(R, dtype=torch.int32, device=dev)
    COUNTERS["shapley_values"] += 1
    _lib.check(lib.isg_shapley_values(p_pi if Q else 0, p_p if G else 0, p_pos if N else 0, p_ptr, bits.graphs.data_ptr() if R else 0, p_rp,
                                      N, G, R, M, Q, int(bits.antithetic), v, W, phi.data_ptr() if N else 0,
                                      m2.data_ptr() if want_m2 and N else 0, gap.data_ptr() if R else 0, flag.data_ptr() if R else 0,
                                      _stream()), "isg_shapley_values")
    return phi, m2, gap, flag


# ------------------------------------------------------------------------------------------------
# Scoring the explanations: token co-occurrence
# ------------------------------------------------------------------------------------------------
COO_TOKENS_MAX = 128       # question words / text tokens per question (ISG_COO_TOKENS_MAX in include/isg.h)
COO_TOTALS = 16 + 4 * (COO_TOKENS_MAX + 1)      # int64 entries of the running totals (ISG_COO_TOTALS)
COO_NODE_CHUNK = 256       # nodes of a graph isg_token_coo stages in LDS per pass (COO_NODE_CHUNK in csrc/isg_token_coo.hip)


class TokenCoo(NamedTuple):
    table: Tensor                # int32 [B, 8]: the row of every question (include/isg.h, isg_token_coo)
    totals: Optional[Tensor]     # int64 [COO_TOTALS]: the caller's running totals with this batch added, or None


def token_coo(names: Tensor, node_mask: Tensor, plan: "GraphPlan", pred: Tensor, label: Tensor, ans_sg: Tensor,
              qtok: Optional[Tensor] = None, qflags: Optional[Tensor] = None, ttok: Optional[Tensor] = None,
              tkeep: Optional[Tensor] = None, threshold: float = 0.0, totals: Optional[Tensor] = None) -> TokenCoo:
    """Token co-occurrence of a batch on the device (isg_token_coo: two launches, one without totals; no sync, no copy).
    names int64 [N], possibly a strided column such as x[:, 0]; node_mask fp32 [N] or [N, 1] (a forward's imle_mask); pred, label
    int64 [B]; ans_sg int32 [A]; qtok int32 [B, T], qflags int32 [B], ttok int32 [B, T2] with tkeep fp32 [B, T2] (both or neither).
    `totals` (int64 [COO_TOTALS], zeroed by the caller once per evaluation) has this batch ADDED to it."""
    lib = _lib.load()
    if (ttok is None) != (tkeep is None):
        raise ValueError("ttok and tkeep come together")
    if node_mask.dim() == 2 and node_mask.size(1) == 1:
        node_mask = node_mask.squeeze(1)
    N, B = plan.N, plan.B
    p_mask = _chk(node_mask, "node_mask", torch.float32, (N,))
    if names.dim() != 1 or names.numel() != N or names.dtype != torch.int64:
        raise ValueError(f"names: expected int64 [{N}] (a strided column is fine), got {names.dtype} {tuple(names.shape)}")
    if not names.is_cuda:
        raise _lib.IsgError(f"names must live on the GPU (got {names.device}); this path has no CPU fallback")
    stride = names.stride(0) if N > 1 else 1
    if stride < 1:
        raise ValueError(f"names: stride {stride}")
    T = 0 if qtok is None else (qtok.size(1) if qtok.dim() == 2 else -1)
    T2 = 0 if ttok is None else (ttok.size(1) if ttok.dim() == 2 else -1)
    if T < 0 or T2 < 0:
        raise ValueError("qtok / ttok must be [B, T]")
    p_qtok = _chk(qtok, "qtok", torch.int32, (B, T), optional=True)
    p_ttok = _chk(ttok, "ttok", torch.int32, (B, T2), optional=True)
    p_tkeep = _chk(tkeep, "tkeep", torch.float32, (B, T2), optional=True)
    table = torch.empty(B, 8, dtype=torch.int32, device=node_mask.device)
    _lib.check(lib.isg_token_coo(names.data_ptr(), stride, p_mask, float(threshold), _chk(plan.ptr, "plan.ptr", torch.int32, (B + 1,)),
                                 _chk(pred, "pred", torch.int64, (B,)), _chk(label, "label", torch.int64, (B,)),
                                 _chk(ans_sg, "ans_sg", torch.int32, (ans_sg.numel(),)), p_qtok,
                                 _chk(qflags, "qflags", torch.int32, (B,), optional=True), p_ttok, p_tkeep, N, B, ans_sg.numel(),
                                 T, T2, table.data_ptr(), _chk(totals, "totals", torch.int64, (COO_TOTALS,), optional=True),
                                 _stream()), "isg_token_coo")
    return TokenCoo(table, totals)


# ------------------------------------------------------------------------------------------------
# Message passing
# ------------------------------------------------------------------------------------------------
def instr_gate(x: Tensor, instr: Tensor, batch: Tensor, plan: Optional["GraphPlan"] = None) -> Tensor:
    """gelu(x * instr[batch])   (mgat_v2_conv.py:156-157).  ``plan`` selects the HIP backward (else torch recompute)."""
    if _rec(x, instr):
        from . import autograd
        return autograd.instr_gate(x, instr, batch, plan)
    lib = _lib.load()
    N, C = x.shape
    out = torch.empty_like(x)
    _lib.check(lib.isg_instr_gate(_chk(x, "x", torch.float32), _chk(instr, "instr", torch.float32, (instr.size(0), C)),
                                  _chk(batch, "batch", torch.int64, (N,)), out.data_ptr(), N, C, _stream()),
               "isg_instr_gate")
    return out


def node_to_edge_mask(mask: Tensor, edge_index: Tensor, plan: Optional[GraphPlan] = None) -> Tensor:
    """mask[src] * mask[dst]   (sampling/node_edge_masks.py:7-10).  mask [N,1] or [N] -> [E,1] / [E].
    ``plan`` (CSR by destination) is only needed when the mask requires grad."""
    if _rec(mask):
        from . import autograd
        if plan is None:
            raise ValueError("node_to_edge_mask needs the GraphPlan to differentiate (its backward walks the CSR)")
        return autograd.node_to_edge_mask(mask, edge_index, plan)
    lib = _lib.load()
    E = edge_index.size(1)
    flat = mask.reshape(-1)
    out = torch.empty(E, dtype=torch.float32, device=mask.device)
    _lib.check(lib.isg_node_to_edge_mask(_chk(flat, "mask", torch.float32), _chk(edge_index, "edge_index", torch.int64),
                                         E, out.data_ptr(), _stream()), "isg_node_to_edge_mask")
    return out.view(E, 1) if mask.dim() == 2 else out


def _mp_operands(att: Tensor, bias: Optional[Tensor], node_mask: Optional[Tensor], edge_mask: Optional[Tensor], N: int, E: int,
                 HC: int) -> Tuple[int, int, int, int]:
    """(att, bias, node_mask, edge_mask) as every kernel of the message-passing family takes them: flattened and checked, once per
    call of a wrapper however many entry points it tries; an optional one that is absent is a null pointer."""
    return (_chk(att.reshape(-1), "att", torch.float32, (HC,)),
            _chk(None if bias is None else bias.reshape(-1), "bias", torch.float32, (HC,), optional=True),
            _chk(None if node_mask is None else node_mask.reshape(-1), "node_mask", torch.float32, (N,), optional=True),
            _chk(None if edge_mask is None else edge_mask.reshape(-1), "edge_mask", torch.float32, (E,), optional=True))


def _launched(rc: int, what: str, timer: Optional[KernelTimer], event) -> bool:
    """The status of a launch inside an MP_TIMER bracket.  ISG_EUNSUPPORTED: the kernel has no launch for this shape and the
    caller takes another path (False, the bracket dropped).  Any other status is checked, and `event` recorded behind the launch."""
    if rc == ISG_EUNSUPPORTED:
        if timer is not None:
            timer.drop_last()
        return False
    _lib.check(rc, what)
    if timer is not None:
        event.record()
    return True


def _segmented_planes32(N: int, H: int, C: int, device):
    """The unwritten SEGMENTED Planes32 result [N, H*C] of the flat per-graph kernel (H = 4: two segments of 2 * C columns, each
    under its own row scale), and the two pointers the kernel writes through: the planes, the inverse scales [2, N]."""
    seg = 2 * C
    pl = torch.empty(N * 2 * ((seg + 31) // 32) * 64, dtype=torch.int16, device=device)
    pinv = torch.empty(2, N, dtype=torch.float32, device=device)
    return Planes32(pl, pinv[1], N, H * C, pinv[0], seg), pl.data_ptr(), pinv.data_ptr()


def gatv2_mp(x_l: Tensor, x_r: Tensor, e_proj: Tensor, att: Tensor, plan: GraphPlan, heads: int,
             bias: Optional[Tensor] = None, node_mask: Optional[Tensor] = None, edge_mask: Optional[Tensor] = None,
             negative_slope: float = 0.2, kernel: Optional[str] = None, want_rowmax: bool = False,
             want_planes: bool = False, dropout_p: float = 0.0, dropout_seed: int = 0) -> Tuple[Tensor, Tensor]:
    """MaskingGATv2Conv.message + aggregate (mgat_v2_conv.py:243-279).  Returns (out[N,H*C], alpha[E,H]).
    dropout_p > 0 (training, fp32 rows): attention dropout on the aggregation's weights, keep or drop a pure function of
    (dropout_seed, original edge id, head) (include/isg_mp_train.h); alpha is the softmax before it, as the reference's
    ``self._alpha``.  The row-maxima and planes forms are inference forms and are not asked for then.
    want_rowmax (inference, fp32 rows): the kernel also writes max |out| per (node, head) and `out` carries it as
    ``out._isg_rowmax`` [N, H] -- the row scales of the fp16 three-product GEMM that reads `out` next (x_proj).
    want_planes (inference, fp32 rows, H = 4): where the flat per-graph kernel runs (the reference's C = 300), `out` comes back
    as a SEGMENTED Planes32 -- the operand of x_proj.0 on isg_linear_h3p with no fp32 copy and no split pass; anywhere else the
    fp32 rows as always."""
    dropout_p, dropout_seed = _drop_args(dropout_p, dropout_seed)
    if _rec(x_l, x_r, e_proj, att, bias, node_mask, edge_mask):
        from . import autograd
        return autograd.gatv2_mp(x_l, x_r, e_proj, att, plan, heads, bias, node_mask, edge_mask, negative_slope, kernel,
                                 dropout_p, dropout_seed)
    lib = _lib.load()
    plan.require_csr()
    N, HC = x_l.shape
    H = int(heads)
    C = HC // H
    E = plan.E
    if N != plan.N or H * C != HC:
        raise ValueError(f"x_l {tuple(x_l.shape)} does not match plan N={plan.N} / heads={H}")
    # x_l / x_r may be column slices of one fused [N, 2*H*C] projection: rows strided, columns contiguous
    ld_l, ld_r, ld_e = x_l.stride(0), x_r.stride(0), (e_proj.stride(0) if E > 0 else HC)
    if x_l.stride(1) != 1 or x_r.stride(1) != 1 or tuple(x_r.shape) != (N, HC) or tuple(e_proj.shape) != (E, HC):
        raise ValueError("x_l / x_r must be [N, H*C] and e_proj [E, H*C], columns contiguous")
    fdt = x_l.dtype                # feature rows: fp32, or fp16 (BASELINE configs[4]; fp32 arithmetic, per-graph kernel)
    if fdt not in (torch.float32, torch.float16) or x_r.dtype != fdt or (E > 0 and e_proj.dtype != fdt):
        raise TypeError(f"x_l / x_r / e_proj must share one dtype (fp32 or fp16), got {x_l.dtype}/{x_r.dtype}/{e_proj.dtype}")
    out = torch.empty(N, HC, dtype=fdt, device=x_l.device)
    alpha = torch.empty(E, H, dtype=torch.float32, device=x_l.device)
    use_graph = (kernel or CFG.mp_kernel) == "graph" and plan.B > 0 and plan.nmax > 0
    if fdt == torch.float16 and not use_graph:
        raise _lib.IsgError("fp16 feature rows need the per-graph kernel (a GraphPlan built with edge_index)")
    # every entry point takes `ins`, its results, `dims`; the per-graph arrays are handed over only where that kernel may run
    attp, biasp, nm, em = _mp_operands(att, bias, node_mask, edge_mask, N, E, HC)
    ins = (_chk_rows(x_l, "x_l", fdt), _chk_rows(x_r, "x_r", fdt), _chk_rows(e_proj, "e_proj", fdt) if E > 0 else 0, attp, biasp,
           plan.rowptr.data_ptr(), plan.eid.data_ptr(), plan.src.data_ptr(), nm, em)
    dims = (N, E, H, C, float(negative_slope), plan.ptr.data_ptr() if use_graph else 0, plan.eptr.data_ptr() if use_graph else 0,
            plan.dst.data_ptr() if use_graph else 0, plan.B, plan.nmax if use_graph else 0, plan.emax if use_graph else 0,
            ld_l, ld_r, ld_e, _stream())
    timer = MP_TIMER
    if timer is not None:
        ev0, ev1 = timer.bracket({"N": N, "E": E, "H": H, "C": C, "masked": node_mask is not None or edge_mask is not None,
                                  "feat_bytes": 2 if fdt == torch.float16 else 4})
        ev0.record()
    if dropout_p > 0.0:
        if fdt != torch.float32:
            raise _lib.IsgError("attention dropout exists on fp32 feature rows only (fp16 rows are an inference form)")
        from . import _lib_mp_train
        COUNTERS["mp_dropout"] += 1
        _lib.check(_lib_mp_train.load().isg_gatv2_mp_fwd_dropout(*ins, out.data_ptr(), alpha.data_ptr(), *dims[:-1], dropout_p,
                                                                 dropout_seed, dims[-1]), "isg_gatv2_mp_fwd_dropout")
        if timer is not None:
            ev1.record()
        return out, alpha
    # the richer result first; ISG_EUNSUPPORTED = this batch / width takes another kernel: the next form, inside the same bracket
    if want_planes and CFG.mp_planes and use_graph and fdt == torch.float32 and E > 0 and H == 4 and C % 4 == 0:
        planes, pl, pinv = _segmented_planes32(N, H, C, x_l.device)
        rc = lib.isg_gatv2_mp_fwd_planes(*ins, pl, pinv, alpha.data_ptr(), *dims)
        if rc != ISG_EUNSUPPORTED:
            _lib.check(rc, "isg_gatv2_mp_fwd_planes")
            if timer is not None:
                ev1.record()
            return planes, alpha
    if want_rowmax and use_graph and fdt == torch.float32 and E > 0:
        rowmax = torch.empty(N, H, dtype=torch.float32, device=x_l.device)
        rc = lib.isg_gatv2_mp_fwd_rowmax(*ins, out.data_ptr(), alpha.data_ptr(), rowmax.data_ptr(), *dims)
        if rc != ISG_EUNSUPPORTED:
            _lib.check(rc, "isg_gatv2_mp_fwd_rowmax")
            if timer is not None:
                ev1.record()
            attach_row_maxima(out, rowmax)
            return out, alpha
    entry = lib.isg_gatv2_mp_fwd if fdt == torch.float32 else lib.isg_gatv2_mp_fwd_f16
    _lib.check(entry(*ins, out.data_ptr(), alpha.data_ptr(), *dims), "isg_gatv2_mp_fwd")
    if timer is not None:
        ev1.record()
    return out, alpha


# lin_edge folded into the attention logits (csrc/isg_mp_logits.hip): e_proj [E, H*C] is never written or read
GK_NCAP_L, GK_ECAP_L = 256, 1024      # the per-graph message-passing kernel's largest tables (csrc/isg_mp_graph.hip)


def _fused_logits_ok(heads: int, channels: int, edge_dim: int, B: int, E: int, nmax: int, has_csr: bool, cfg: Switches) -> bool:
    """fused_logits_supported over plain values (conv_route)."""
    cp = (channels + 31) // 32 * 32       # round 5: heads padded to whole 32-channel tiles (the reference's C = 300 -> 320), K <= 304
    wide = channels % 32 != 0 or edge_dim > 128
    if wide and E < cfg.rows_kernel_min_edges:
        # the rows kernel streams all of lin_edge's tiles through its three-slot ring whatever the number of slots: ~94 us for 400
        # edges as for 50 000 (40 tiles x one DMA round trip each).  A small batch projects its few edge rows (isg_linear_skinny, ~5 us)
        # and runs the flat kernel on e_proj instead
        return False
    return (cfg.fuse_logits and (cfg.fuse_logits_wide or not wide) and cfg.gemm_backend == "bf16x6" and cfg.gemm_f16x3 and
            cfg.mp_kernel == "graph" and channels % 4 == 0 and heads * cp <= 2048 and 0 < edge_dim <= 304 and edge_dim % 4 == 0 and
            B > 0 and nmax > 0 and has_csr and E > 0)


def fused_logits_supported(plan: "GraphPlan", heads: int, channels: int, edge_dim: int) -> bool:
    """Shape test of isg_gatv2_edge_logits + isg_gatv2_mp_fwd_logits (inference, fp32 rows, per-graph kernel)."""
    return _fused_logits_ok(heads, channels, edge_dim, plan.B, plan.E, plan.nmax, plan.rowptr is not None, CFG)


def _edge_logits_weight(w_edge: Tensor, heads: int):
    """lin_edge.weight [H*C, K] as the fragment planes isg_gatv2_edge_logits reads: the weight itself when 32 | C and K <= 128; else
    with zero rows behind every head's C-th up to the next multiple of 32 (C = 300 -> 320: a channel tile never straddles heads)
    and, for K > 128 (the rows kernel: 19 k steps), zero columns up to 304."""
    HC, K = w_edge.shape
    C = HC // heads
    cp = (C + 31) // 32 * 32
    kp = K if K <= 128 else 304
    if cp == C and kp == K:
        return _weight_planes(w_edge, True, "f16x3")

    def build():
        w = torch.zeros(heads, cp, kp, dtype=torch.float32, device=w_edge.device)
        w[:, :C, :K] = w_edge.detach().view(heads, C, K)
        return w.view(heads * cp, kp)
    return _weight_planes(derived_weight(f"edge_logits_pad{heads}", (w_edge,), build), True, "f16x3")


def _edge_logits(lib, x_l: Tensor, x_r: Tensor, edge_attr: Tensor, w_planes, attp: int, nm: int, em: int, plan: "GraphPlan", H: int,
                 C: int, negative_slope: float, timer: Optional[KernelTimer] = None, event=None) -> Optional[Tensor]:
    """isg_gatv2_edge_logits (fp32 rows) or its _f16 twin (half rows: BASELINE configs[4]'s storage, K >= 128) on checked
    operands: logits fp32 [E, H] in CSR SLOT order (slot t = edge plan.eid[t]), or None when the kernel has no launch."""
    E, K = edge_attr.shape
    fdt = x_l.dtype
    logits = torch.empty(E, H, dtype=torch.float32, device=x_l.device)
    entry, what = (lib.isg_gatv2_edge_logits, "isg_gatv2_edge_logits") if fdt == torch.float32 else \
        (lib.isg_gatv2_edge_logits_f16, "isg_gatv2_edge_logits_f16")
    rc = entry(_chk_rows(edge_attr, "edge_attr"), edge_attr.stride(0), w_planes[0].data_ptr(), w_planes[1].data_ptr(),
               _chk_rows(x_l, "x_l", fdt), x_l.stride(0), 0, _chk_rows(x_r, "x_r", fdt), x_r.stride(0), 0, attp,
               plan.eid.data_ptr(), plan.src.data_ptr(), plan.dst.data_ptr(), em, nm, logits.data_ptr(), E, H, C, K,
               float(negative_slope), _stream())
    return logits if _launched(rc, what, timer, event) else None


def gatv2_edge_logits(x_l: Tensor, x_r: Tensor, edge_attr: Tensor, w_edge: Tensor, att: Tensor, plan: "GraphPlan", heads: int,
                      node_mask: Optional[Tensor] = None, edge_mask: Optional[Tensor] = None,
                      negative_slope: float = 0.2) -> Optional[Tensor]:
    """isg_gatv2_edge_logits alone: logits fp32 [E, H] in CSR SLOT order (slot t = edge plan.eid[t]); None if unsupported."""
    lib = _lib.load()
    plan.require_csr()
    N, HC = x_l.shape
    H = int(heads)
    attp, _, nm, em = _mp_operands(att, None, node_mask, edge_mask, N, edge_attr.size(0), HC)
    return _edge_logits(lib, x_l, x_r, edge_attr, _edge_logits_weight(w_edge, H), attp, nm, em, plan, H, HC // H, negative_slope)


def gatv2_mp_edge_logits(x_l: Tensor, x_r: Tensor, edge_attr: Tensor, w_edge: Tensor, att: Tensor, plan: "GraphPlan",
                         heads: int, bias: Optional[Tensor] = None, node_mask: Optional[Tensor] = None,
                         edge_mask: Optional[Tensor] = None, negative_slope: float = 0.2, want_rowmax: bool = False,
                         want_planes: bool = False):
    """gatv2_mp(x_l, x_r, lin_edge(edge_attr), ...) as two launches that never materialise lin_edge's output
    (mgat_v2_conv.py:243-279 with :259-261 inside): isg_gatv2_edge_logits forms the logits [E, H] in the epilogue of the
    edge GEMM, isg_gatv2_mp_fwd_logits does softmax + aggregation.  Returns (out, alpha), or None when the per-graph kernel
    has no instantiation for this batch / width (the caller then runs the un-fused pair)."""
    lib = _lib.load()
    plan.require_csr()
    N, HC = x_l.shape
    H = int(heads)
    C = HC // H
    E, K = edge_attr.shape
    if N != plan.N or E != plan.E or tuple(w_edge.shape) != (HC, K):
        raise ValueError("gatv2_mp_edge_logits: operand shapes do not match the plan")
    if x_l.dtype not in (torch.float32, torch.float16) or edge_attr.dtype != torch.float32:
        raise TypeError("gatv2_mp_edge_logits: x_l / x_r as fp32 or fp16 rows, fp32 edge rows")
    if tuple(x_r.shape) != (N, HC) or x_r.dtype != x_l.dtype:
        raise ValueError("gatv2_mp_edge_logits: x_r must be [N, H*C] of x_l's type")
    w_planes = _edge_logits_weight(w_edge, H)
    # BASELINE configs[4]'s storage (fp16 feature rows, fp32 arithmetic): the rows kernel gathers half rows and rounds the edge
    # projection to half as the un-fused path stores it; the result row leaves as half.  K >= 128 (the rows kernel only).
    half = x_l.dtype == torch.float16
    if half and K < 128:
        return None
    alpha = torch.empty(E, H, dtype=torch.float32, device=x_l.device)
    # the result as the segmented planes32 operand of x_proj.0 (the flat kernel, H = 4: the reference's C = 300) -- or rows
    as_planes = bool(not half and want_planes and CFG.mp_planes and H == 4 and C % 32 != 0)
    out = None if as_planes else torch.empty(N, HC, dtype=x_l.dtype, device=x_l.device)
    rowmax = None
    if not half and want_rowmax and not as_planes and C % 32 == 0:
        rowmax = torch.empty(N, H, dtype=torch.float32, device=x_l.device)
    attp, biasp, nm, em = _mp_operands(att, bias, node_mask, edge_mask, N, E, HC)
    timer, evm, ev1 = MP_TIMER, None, None
    if timer is not None:   # bench.py: ONE bracket around both launches -- together they are the reference's message +
        # aggregate (plus lin_edge); the roofline keeps the un-fused algorithmic bytes of SURVEY 8(d)
        ev0, evm, ev1 = timer.bracket3({"N": N, "E": E, "H": H, "C": C, "K": K,
                                        "masked": node_mask is not None or edge_mask is not None,
                                        "feat_bytes": 2 if half else 4, "fused_logits": True})
        ev0.record()
    logits = _edge_logits(lib, x_l, x_r, edge_attr, w_planes, attp, nm, em, plan, H, C, negative_slope, timer, evm)
    if logits is None:
        return None
    # the three softmax + aggregation entry points take `ins`, their results, `dims` (x_l: checked by _edge_logits)
    ins = (x_l.data_ptr(), logits.data_ptr(), attp, biasp, plan.rowptr.data_ptr(), plan.eid.data_ptr(), plan.src.data_ptr(), nm, em)
    dims = (N, E, H, C, float(negative_slope), plan.ptr.data_ptr(), plan.eptr.data_ptr(), plan.dst.data_ptr(), plan.B, plan.nmax,
            plan.emax, x_l.stride(0), _stream())
    if as_planes:
        planes, pl, pinv = _segmented_planes32(N, H, C, x_l.device)
        rc = lib.isg_gatv2_mp_fwd_logits_planes(*ins, pl, pinv, alpha.data_ptr(), *dims)
        if rc != ISG_EUNSUPPORTED:
            _lib.check(rc, "isg_gatv2_mp_fwd_logits_planes")
            if timer is not None:
                ev1.record()
            return planes, alpha
        out = torch.empty(N, HC, dtype=torch.float32, device=x_l.device)
    if half:
        rc, what = lib.isg_gatv2_mp_fwd_logits_f16(*ins, out.data_ptr(), alpha.data_ptr(), *dims), "isg_gatv2_mp_fwd_logits_f16"
    else:
        rc, what = lib.isg_gatv2_mp_fwd_logits(*ins, out.data_ptr(), alpha.data_ptr(), 0 if rowmax is None else rowmax.data_ptr(),
                                               *dims), "isg_gatv2_mp_fwd_logits"
    if not _launched(rc, what, timer, ev1):
        return None
    if rowmax is not None:
        attach_row_maxima(out, rowmax)
    return out, alpha


class StepCapture:
    """Product-path hipGraph execution (opt-in: `AnswerModel.forward(..., capture=True)`, `ISubGVQA.forward(..., capture=True)`).
    A forward over fixed-shape inputs is ~25-110 launches; below ~1000 graphs per step the step is launch-bound (1 024
    graphs 0.641 ms eager vs 0.542 ms replayed, 256 graphs 0.652 vs 0.332).  `run(fn, tensors, key)` keeps one captured hipGraph
    per KEY = (shape / dtype / device of every input, the caller's hints and options, the module's switches): the first call of a key
    runs `fn` eagerly on private static copies of the inputs (kernel attributes, derived weights, allocator pools; the plan's hints
    are checked), captures it once, and every call replays it after copying the caller's tensors into the static ones (a tensor
    that already IS the static one is not copied).  A capture bakes in the tensors derived_weight() made from the weights at capture
    time, so the caller hands over `stamp=WeightsWatch(module).stamp()`: an entry whose stamp differs from the call's (a weight or buffer
    written in place, replaced or loaded; invalidate_weight_cache()) is retired and captured again in its place -- a replay never
    runs on derived weights older than the live ones.  `fn(*tensors) -> (outputs, plan)`: the GraphPlan must be built INSIDE fn
    from host-side bounds (no device-to-host read is possible in a capture); the plan's own last kernel hands the largest true
    bounds of ALL the entry's replays (kept on the device) to pinned host memory, compared with the hints at the next call that finds the last replay
    finished, when the entry is retired or evicted, and in verify() -- a batch whose graphs exceed the hints raises IsgError at one
    of those, however far the host runs ahead of the device in between.  Outputs are the graph's static tensors: valid
    until the next call with the same key.  Nothing here is a fallback: a forward that cannot be captured raises."""

    def __init__(self, max_entries: int = 8):
        import collections
        self.entries = collections.OrderedDict()
        self.max_entries = int(max_entries)
        self.replays = 0
        self.captures = 0

    @staticmethod
    def _sig(t):
        return None if t is None else (tuple(t.shape), t.dtype, t.device.index)

    def _check_bounds(self, ent) -> None:
        plan, host = ent["plan"], ent["host"]
        if plan is None or host is None or not ent["event"].query():
            return                                      # the last replay has not finished: its bounds stay in the running maximum
        # `host` holds the largest of every replay since the capture (or the last raise)
        err = _hint_error(host.tolist(), plan._hints, f"a recent replay (the capture of {ent['what']!r})")
        if err is not None:
            ent["max"].zero_()                          # reported once: the running maximum starts over (in stream order; no
            host.zero_()                                # replay is in flight: the event has completed)
            raise err

    def _retire(self, key) -> None:
        """Drop an entry (its hipGraph and private allocator pool); its replays' bounds are compared first, none is lost: this
        waits for the entry's last replay (an eviction or a stale stamp is followed by a capture, which synchronises anyway)."""
        ent = self.entries.pop(key)
        ent["event"].synchronize()
        self._check_bounds(ent)

    def run(self, fn, tensors, key_extra=(), warm: int = 2, stamp=None):
        if torch.is_grad_enabled():
            raise RuntimeError("StepCapture: inference only (wrap the call in torch.no_grad() / inference_mode())")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("StepCapture: already inside a capture")
        key = (tuple(self._sig(t) for t in tensors), key_extra, CFG)
        ent = self.entries.get(key)
        if ent is not None and ent["stamp"] != stamp:
            self._retire(key)                          # captured from other weights: freed before its successor is captured
            ent = None
        if ent is None:
            while len(self.entries) >= self.max_entries > 0:     # room first: an evicted entry's bounds are compared (and may raise)
                self._retire(next(iter(self.entries)))           # before anything new is captured
            static = [None if t is None else t.clone() for t in tensors]
            for _ in range(max(1, warm)):
                fn(*static)
            check_plans()                              # the eager runs' hints: a wrong one raises HERE, before anything is captured
            torch.cuda.synchronize()
            # outside the capture: memory of the graph's own pool would be zeroed again by every replay
            host = torch.zeros(2, dtype=torch.int32, pin_memory=True)
            running = torch.zeros(2, dtype=torch.int32, device=torch.cuda.current_device())
            graph = torch.cuda.CUDAGraph()
            _CAPTURE_BOUNDS.append((host, running))
            try:
                with torch.cuda.graph(graph):
                    outs, plan = fn(*static)
            finally:
                _CAPTURE_BOUNDS.pop()
            if plan is not None and plan._bounds_host is None:
                host = None                            # (a plan without an edge list / without both hints keeps its bounds on the device)
            ent = {"graph": graph, "static": static, "outs": outs, "plan": plan, "host": host, "max": running, "event": torch.cuda.Event(),
                   "stamp": stamp, "what": key_extra}
            self.entries[key] = ent
            self.captures += 1
        else:
            self.entries.move_to_end(key)
            self._check_bounds(ent)
            for st, t in zip(ent["static"], tensors):
                if t is not None and st.data_ptr() != t.data_ptr():
                    st.copy_(t, non_blocking=True)
        ent["graph"].replay()
        ent["event"].record()
        self.replays += 1
        return ent["outs"]

    def verify(self) -> None:
        """Synchronise and check every entry's replays (tests; the end of an evaluation loop)."""
        torch.cuda.synchronize()
        for ent in self.entries.values():
            self._check_bounds(ent)
            if ent["plan"] is not None and ent["host"] is None:
                ent["plan"].verify_hints()


ISG_EUNSUPPORTED = -2      # include/isg.h
ISG_LC_SPARSE_OUT = 1      # include/isg_sparse_out.h

# message + softmax + aggregation with lin_edge inside as ONE launch on graph-aligned tiles (csrc/isg_layer_tile.hip): the
# head's x_l slice of a tile is staged once in LDS and serves the logit epilogue's row gathers and the aggregation
TILE_CONV_NODES, TILE_CONV_EDGES = 64, 256


def _tile_conv_ok(heads: int, channels: int, edge_dim: int, B: int, E: int, has_csr: bool, tile_mode: str, cfg: Switches) -> bool:
    """tile_conv_supported over plain values (conv_route); tile_mode is GraphPlan.tile_mode(TILE_CONV_NODES, TILE_CONV_EDGES)."""
    return (cfg.fuse_tile_conv and cfg.fuse_logits and cfg.gemm_backend == "bf16x6" and cfg.gemm_f16x3 and cfg.mp_kernel == "graph" and
            channels == 128 and 0 < edge_dim <= 128 and edge_dim % 4 == 0 and heads <= 64 and B > 0 and has_csr and E > 0 and
            tile_mode != "none")


def _layer_conv_ok(heads: int, channels: int, in_channels: int, edge_dim: int, B: int, E: int, has_csr: bool, tile_mode: str,
                   cfg: Switches) -> bool:
    """layer_conv_supported over plain values (conv_route)."""
    return (cfg.fuse_layer_conv and in_channels == 128 and heads <= 16 and
            _tile_conv_ok(heads, channels, edge_dim, B, E, has_csr, tile_mode, cfg))


# the plan-taking forms ask GraphPlan.tile_mode LAST, only when everything cheaper has passed: it can cost a device-to-host sync
def tile_conv_supported(plan: "GraphPlan", heads: int, channels: int, edge_dim: int) -> bool:
    """Shape test of isg_gatv2_tile_conv (inference, fp32 rows): C = 128, edge features <= 128 wide, every graph within one
    64-node / 256-slot tile -- or all but a few (GraphPlan.tile_mode: those go to the per-graph kernels)."""
    return (_tile_conv_ok(heads, channels, edge_dim, plan.B, plan.E, plan.rowptr is not None, "tiles", CFG) and
            plan.tile_mode(TILE_CONV_NODES, TILE_CONV_EDGES) != "none")


def layer_conv_supported(plan: "GraphPlan", heads: int, channels: int, in_channels: int, edge_dim: int) -> bool:
    """Shape test of isg_gatv2_layer_conv: isg_gatv2_tile_conv's, and a 128-wide layer input."""
    return (_layer_conv_ok(heads, channels, in_channels, edge_dim, plan.B, plan.E, plan.rowptr is not None, "tiles", CFG) and
            plan.tile_mode(TILE_CONV_NODES, TILE_CONV_EDGES) != "none")


class NodePlanes(NamedTuple):
    """Node rows as isg_gatv2_layer_conv reads them: per-row power-of-two scale, (hi, mid) fp16 planes int16 [N, 2, 128] and the
    inverse scales fp32 [N] (the staging of the exact-split Linears, made once per row by the kernel that produces the rows)."""
    planes: Tensor
    inv: Tensor


def _empty_node_planes(rows: int, device) -> NodePlanes:
    """Unwritten planes for the kernel that fills them (edge rows take the same form); one row at least, so that an empty batch
    still hands its kernel a pointer."""
    return NodePlanes(torch.empty(max(rows, 1), 2, 128, dtype=torch.int16, device=device),
                      torch.empty(max(rows, 1), dtype=torch.float32, device=device))


def node_planes(x: Tensor) -> NodePlanes:
    """fp32 rows [N, 128] -> NodePlanes (isg_edge_planes in row order): for callers that hold the gated rows only as fp32."""
    lib = _lib.load()
    N, K = x.shape
    out = _empty_node_planes(N, x.device)
    _lib.check(lib.isg_edge_planes(_chk_rows(x, "x"), x.stride(0), 0, N, K, out.planes.data_ptr(), out.inv.data_ptr(), _stream()),
               "isg_edge_planes")
    return out


def instr_gate_planes(x: Tensor, instr: Tensor, batch: Tensor, want_rows: bool = False) -> Tuple[Optional[Tensor], NodePlanes]:
    """gelu(x * instr[batch]) (mgat_v2_conv.py:156-157) as NodePlanes for gatv2_layer_conv, plus the fp32 rows when a masked
    layer's node gate needs them: isg_instr_gate_planes.  Inference only (C = 128)."""
    lib = _lib.load()
    N, C = x.shape
    rows = torch.empty_like(x) if want_rows else None
    out = _empty_node_planes(N, x.device)
    _lib.check(lib.isg_instr_gate_planes(_chk(x, "x", torch.float32), _chk(instr, "instr", torch.float32, (instr.size(0), C)),
                                         _chk(batch, "batch", torch.int64, (N,)), 0 if rows is None else rows.data_ptr(),
                                         out.planes.data_ptr(), out.inv.data_ptr(), N, C, _stream()), "isg_instr_gate_planes")
    return rows, out


def _count_tile_nodes(plan: "GraphPlan", sub: Optional["OversizeGraphs"]) -> None:
    COUNTERS["tile_nodes"] += plan.N - (0 if sub is None else sub.nodes.numel())
    COUNTERS["oversize_nodes"] += 0 if sub is None else sub.nodes.numel()


def _mixed_sub(plan: "GraphPlan") -> Optional["OversizeGraphs"]:
    """The oversize graphs of a batch the tile kernels take in "mixed" mode (None in "tiles" mode) -- and None when they run as a
    batch of their own through the whole model (run_split: plan.holes), so that nobody fills their rows layer by layer."""
    if plan.holes is not None:
        _count_tile_nodes(plan, plan.holes)
        return None
    sub = plan.oversize(TILE_CONV_NODES, TILE_CONV_EDGES) if plan.tile_mode(TILE_CONV_NODES, TILE_CONV_EDGES) == "mixed" else None
    _count_tile_nodes(plan, sub)
    return sub


_side_streams: dict = {}


def _side_stream(device) -> "torch.cuda.Stream":
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=device)
    return _side_streams[key]


def oversize_split(plan: "GraphPlan") -> Optional["OversizeGraphs"]:
    """The graphs a model running on the graph-tile kernels should send through run_split (None: none, or not worth it)."""
    if not CFG.split_forward or plan.holes is not None or plan.rowptr is None:
        return None
    if plan.tile_mode(TILE_CONV_NODES, TILE_CONV_EDGES) != "mixed":
        return None
    return plan.oversize(TILE_CONV_NODES, TILE_CONV_EDGES)


def run_split(plan: "GraphPlan", sub: "OversizeGraphs", core, x: Tensor, edge_index: Tensor, edge_attr: Tensor, batch: Tensor,
              instr: Tensor, glf: Tensor, noises=None, seed=None, kinds: str = "gnn"):
    """core(x, edge_index, edge_attr, batch, instr, glf, plan, noises, seed, gate_feats) -> tuple of tensors / lists / None, one per
    letter of `kinds` ("g": a row per graph, "n": a row per node, "e": a row per edge, merged through sub.edges), run TWICE: on the whole batch with the tile kernels passing
    over the graphs beyond a tile (their rows stay unwritten: plan.holes), and on those graphs as a batch of their own (per-graph
    kernels; instr is [L, B, C]); the second result is then copied over the rows of the first.  Every op of the path is local to
    a graph (or a row), so nothing of a hole reaches another graph -- with ONE exception that the reference itself makes: a masked
    layer's node gate reads the question row batch[batch[n]] (masking.py:151-155, quirk Q3), i.e. for graph g the row of the graph
    that holds NODE number g; the sub-batch is handed exactly those rows (gate_feats, to MGAT.forward).  A real GQA batch has a few such graphs (the reference caps
    nothing: datasets/scene_graph.py:199-389); filling their rows after every tile kernel instead cost ~200 small launches per step
    (profiles/r04_az_split_forward.txt).  Dense [B, nmax] noise is cut to the sub-batch; under a seed every graph of the sub-batch draws the stream of its number in the WHOLE batch (plan.graph_ids), so a seeded mask does not depend on the dispatch."""
    nmax_s = sub.plan.nmax

    def run_side():
        xs, es = x.index_select(0, sub.nodes), edge_attr.index_select(0, sub.edges)
        instr_s, glf_s = instr.index_select(1, sub.gids), glf.index_select(0, sub.gids)
        gate_s = glf.index_select(0, batch.index_select(0, sub.gids.clamp(max=max(plan.N - 1, 0))))
        nz_s = None
        if noises is not None:
            nz_s = {}
            for k, v in noises.items():
                v = v.index_select(0, sub.gids)
                nz_s[k] = (v[:, :nmax_s] if v.dim() == 2 else v[:, :, :nmax_s]).contiguous()
        return core(xs, sub.edge_index, es, sub.batch, instr_s, glf_s, sub.plan, nz_s, seed, gate_s)

    def run_main():
        # a view with its own `holes`: the caller's plan is not written to, and a second run_split on it (another thread, a
        # re-entrant core) sees none; what the pass builds lazily lands in the cache both share, where the caller's plan finds it
        return core(x, edge_index, edge_attr, batch, instr, glf, plan.with_holes(sub), noises, seed, None)

    if CFG.split_stream and x.is_cuda and not torch.cuda.is_current_stream_capturing():
        # The sub-batch is a chain of ~60 launches of one or a few workgroups each (0.65 ms of GPU time for ONE 100-node graph):
        # on a stream of its own it runs beside the tile kernels instead of behind them.  The main pass is issued FIRST (the GPU
        # starts on it while the host is still issuing the sub-batch).
        cur = torch.cuda.current_stream()
        side_stream = _side_stream(x.device)
        side_stream.wait_stream(cur)                 # inputs and the lists of `sub` are complete
        main = run_main()                            # (weight caches the two passes share: every entry carries its _Ready marker)
        with torch.cuda.stream(side_stream):
            side = run_side()
        cur.wait_stream(side_stream)

        def keep(t):                                 # results made on the side stream, read on this one
            if isinstance(t, Tensor):
                t.record_stream(cur)
            elif isinstance(t, (list, tuple)):
                for u in t:
                    keep(u)
        keep(side)
    else:
        main = run_main()
        side = run_side()
    if len(main) != len(kinds) or len(side) != len(kinds):
        raise ValueError("run_split: one letter of `kinds` per result")

    def merge(m, s_, kind):
        if m is None:
            return None
        if isinstance(m, (list, tuple)):
            return type(m)(merge(a, b, kind) for a, b in zip(m, s_))
        idx, rows = {"g": (sub.gids, plan.B), "n": (sub.nodes, plan.N), "e": (sub.edges, plan.E)}[kind]
        if m.size(0) != rows or s_.size(0) != idx.numel():
            raise ValueError(f"run_split: a '{kind}' result of {tuple(m.shape)} / {tuple(s_.shape)} rows")
        if m.dim() == 2 and kind in ("n", "e") and s_.dim() == 2 and m.size(1) != s_.size(1):
            raise ValueError("run_split: per-node results of different widths" if kind == "n" else
                             "run_split: per-edge results of different widths")
        return m.index_copy_(0, idx, s_.to(m.dtype))
    return tuple(merge(m, s_, k) for m, s_, k in zip(main, side, kinds))


def _oversize_conv(sub: "OversizeGraphs", x_l: Tensor, x_r: Tensor, edge_attr: Tensor, w_edge: Tensor, att: Tensor, heads: int,
                   bias, node_mask, edge_mask, negative_slope: float, out: Tensor, alpha: Tensor, rowmax: Optional[Tensor]) -> None:
    """Message passing of the graphs the tile kernels passed over (mgat_v2_conv.py:215-279 on the sub-batch): lin_edge +
    the per-graph kernel (256-node / 1024-edge tables, or node chunks beyond), written into the rows / edges of `out` /
    `alpha` / `rowmax` that belong to those graphs."""
    cache = sub.plan._cache
    rows = _if_from_tensor(cache.parent_edge_rows, edge_attr)      # every layer reads the same edge features
    if rows is None:
        rows = edge_attr.index_select(0, sub.edges)
        cache.parent_edge_rows = _from_tensor(edge_attr, rows)
    e_proj = linear(rows, w_edge)
    nm = None if node_mask is None else node_mask.reshape(-1).index_select(0, sub.nodes)
    em = None if edge_mask is None else edge_mask.reshape(-1).index_select(0, sub.edges)
    o, a = gatv2_mp(x_l, x_r, e_proj, att, sub.plan, heads, bias=bias, node_mask=nm, edge_mask=em,
                    negative_slope=negative_slope, want_rowmax=rowmax is not None)
    out.index_copy_(0, sub.nodes, o)
    if alpha is not None:
        alpha.index_copy_(0, sub.edges, a)
    if rowmax is not None:
        rm = row_maxima(o)
        if rm is None:                                  # the node-chunk kernel leaves none: one pass over the few rows
            rm = o.view(o.size(0), heads, -1).abs().amax(dim=2)
        rowmax.index_copy_(0, sub.nodes, rm)


def _tile_conv_operands(plan: "GraphPlan", ntiles: Tensor, cap: int, att: Tensor, bias, node_mask, edge_mask, H: int, HC: int,
                        want_rowmax: bool, device, want_alpha: bool = True, poison: bool = False):
    """What isg_gatv2_layer_conv and isg_gatv2_tile_conv take alike, in the order both take it -- att, bias, the CSR, the tile list,
    the masks, out, its row stride, alpha, rowmax -- and the three result tensors (rowmax: None unless wanted; alpha: None and a
    null pointer when not wanted, which isg_gatv2_layer_conv alone takes).  poison: out / rowmax start NaN-filled."""
    N, E = plan.N, plan.E
    tile_info = plan.tiles_heavy_first(TILE_CONV_NODES, TILE_CONV_EDGES)        # a persistent kernel: balanced rounds
    new = (lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=device)) if poison else \
        (lambda *shape: torch.empty(*shape, dtype=torch.float32, device=device))
    out = new(N, HC)
    alpha = torch.empty(E, H, dtype=torch.float32, device=device) if want_alpha else None
    rowmax = new(N, H) if want_rowmax else None
    attp, biasp, nm, em = _mp_operands(att, bias, node_mask, edge_mask, N, E, HC)
    shared = (attp, biasp, plan.rowptr.data_ptr(), plan.eid.data_ptr(), plan.src.data_ptr(), plan.dst.data_ptr(), tile_info.data_ptr(),
              ntiles.data_ptr(), cap, nm, em, out.data_ptr(), HC, 0 if alpha is None else alpha.data_ptr(),
              0 if rowmax is None else rowmax.data_ptr())
    return shared, out, alpha, rowmax


def gatv2_layer_conv(x, lin_l, lin_r, edge_attr: Tensor, w_edge: Tensor, att: Tensor, plan: "GraphPlan", heads: int,
                     bias: Optional[Tensor] = None, node_mask: Optional[Tensor] = None, edge_mask: Optional[Tensor] = None,
                     negative_slope: float = 0.2, want_rowmax: bool = False, want_alpha: bool = True, sparse_out: bool = False):
    """lin_l(x), lin_r(x), lin_edge(edge_attr), message, softmax and aggregation of one MaskingGATv2Conv as ONE launch
    (mgat_v2_conv.py:177-181, :215-232, :243-279): isg_gatv2_layer_conv.  x = the gated layer input [N, 128], as NodePlanes (from
    instr_gate_planes / mgat_dense_tail) or as fp32 rows (split here, one more launch).  Bit-identical to linear_fused +
    gatv2_tile_conv.  Returns (out, alpha), or None when the kernel has no launch for this shape.
    want_alpha=False: the attention weights are not stored and alpha is None (out keeps its bits).
    sparse_out=True (a masked launch with want_rowmax, on groups of tiles): a row that no live slot has as
    destination -- flagged dead in every head, `+0 + bias` -- is written in `out` and its maxima for the first such row of every
    tile only; `out` then carries a marker, mgat_dense_tail's live-row form reads it as it is, and EVERY other reader goes through
    dense_conv_out(out)."""
    lib = _lib.load()
    plan.require_csr()
    if not isinstance(x, NodePlanes):
        if x.dtype != torch.float32 or x.dim() != 2 or x.size(1) != 128:
            raise TypeError("gatv2_layer_conv: fp32 rows [N, 128] or NodePlanes")
        x = node_planes(x)
    N, K_in = plan.N, 128
    if x.planes.size(0) < N or x.inv.size(0) < N:
        raise ValueError("gatv2_layer_conv: node planes shorter than the plan's node count")
    dev = x.planes.device
    H = int(heads)
    HC = lin_l.weight.size(0)
    C = HC // H
    E, K = edge_attr.shape
    if N != plan.N or E != plan.E or tuple(w_edge.shape) != (HC, K) or tuple(lin_r.weight.shape) != (HC, K_in) or \
            lin_l.weight.size(1) != K_in:
        raise ValueError("gatv2_layer_conv: operand shapes do not match the plan")
    if edge_attr.dtype != torch.float32:
        raise TypeError("gatv2_layer_conv: fp32 edge rows")
    cat_w = derived_weight("layer_conv_w", (lin_l.weight, lin_r.weight),
                           lambda: torch.cat([lin_l.weight.detach(), lin_r.weight.detach()], 0).contiguous())
    zeros = lambda m: torch.zeros(HC, dtype=torch.float32, device=dev) if m.bias is None else m.bias.detach()
    srcs = tuple(t for t in (lin_l.weight, lin_l.bias, lin_r.bias) if t is not None)
    cat_b = derived_weight("layer_conv_b", srcs, lambda: torch.cat([zeros(lin_l), zeros(lin_r)]).float().contiguous())
    wn, wn_inv = _weight_planes(cat_w, True, "f16x3")
    we, we_inv = _weight_planes(w_edge, True, "f16x3")
    (_, ntiles, cap, _), (ep, ep_inv) = plan.tiles_and_edge_planes(edge_attr, TILE_CONV_NODES, TILE_CONV_EDGES)
    # a sparse launch: masked, with flags for its readers, on groups of tiles (the library's rule for this shape)
    masked = node_mask is not None or edge_mask is not None
    mlib, group = None, 1
    if masked and cap > 0:
        from . import _lib_masked
        mlib = _lib_masked.load()
        group = mlib.isg_gatv2_layer_conv_group(N, E, H, cap)
    sparse = bool(sparse_out and CFG.sparse_conv_out and masked and want_rowmax and group > 1 and
                  CFG.dense_tail_rows == TILE_CONV_NODES)      # the tail's tiles are the convolution's
    shared, out, alpha, rowmax = _tile_conv_operands(plan, ntiles, cap, att, bias, node_mask, edge_mask, H, HC, want_rowmax, dev,
                                                     want_alpha=want_alpha, poison=sparse and CFG.poison_sparse_out)
    # a masked launch also says which (row, head) kept all-zero accumulators: those rows of `out` are +0 + bias, all alike, and
    # mgat_dense_tail runs x_proj once for them.  Rows of a mixed plan's oversize graphs are written elsewhere: never flagged.
    row_dead = None
    if rowmax is not None and (node_mask is not None or edge_mask is not None):
        whole = plan.tile_mode(TILE_CONV_NODES, TILE_CONV_EDGES) == "tiles"
        row_dead = (torch.empty if whole else torch.zeros)(N, H, dtype=torch.uint8, device=dev)
    # a masked launch on groups of tiles reads every tile's live tables from memory: one pre-pass builds them for all heads
    # (include/isg_masked.h).  Rebuilt on every call -- the mask is the step's -- in a buffer of this call, on the launch stream.
    tables = None
    if mlib is not None and mlib.isg_layer_conv_live_tables_enabled() and group > 1:
        tables = torch.empty(mlib.isg_layer_conv_live_tables_bytes(cap), dtype=torch.uint8, device=dev)
    timer, ev1 = MP_TIMER, None
    if timer is not None:
        ev0, ev1 = timer.bracket({"N": N, "E": E, "H": H, "C": C, "K": K, "masked": node_mask is not None or edge_mask is not None,
                                  "feat_bytes": 4, "tile_conv": True, "layer_conv": True, "K_in": K_in})
        ev0.record()
    front = (x.planes.data_ptr(), x.inv.data_ptr(), wn.data_ptr(), wn_inv.data_ptr(), cat_b.data_ptr(), ep.data_ptr(), ep_inv.data_ptr(),
             we.data_ptr(), we_inv.data_ptr(), *shared, 0 if row_dead is None else row_dead.data_ptr())
    if tables is not None:
        _, _, rowptr_p, eid_p, src_p, dst_p, tile_info_p, ntiles_p, _, nm_p, em_p = shared[:11]
        _lib.check(mlib.isg_layer_conv_live_tables(rowptr_p, eid_p, src_p, dst_p, ep_inv.data_ptr(), tile_info_p, ntiles_p, cap,
                                                   nm_p, em_p, tables.data_ptr(), N, E, _stream()), "isg_layer_conv_live_tables")
    if sparse:
        from . import _lib_sparse_out
        rc = _lib_sparse_out.load().isg_gatv2_layer_conv_sparse(*front, 0 if tables is None else tables.data_ptr(), ISG_LC_SPARSE_OUT, N, E, H, C, K_in, K,
                                              float(negative_slope), _stream())
    elif tables is None:
        rc = lib.isg_gatv2_layer_conv(*front, N, E, H, C, K_in, K, float(negative_slope), _stream())
    else:
        rc = mlib.isg_gatv2_layer_conv_tables(*front, tables.data_ptr(), N, E, H, C, K_in, K, float(negative_slope), _stream())
    if not _launched(rc, "isg_gatv2_layer_conv", timer, ev1):
        return None
    sub = _mixed_sub(plan)
    if sub is not None:
        # the gated rows of those graphs out of the SAME planes the tile kernel read (hi + mid, exact), projected per node
        pl = x.planes.view(torch.float16).index_select(0, sub.nodes).float()
        xs = ((pl[:, 0] + pl[:, 1]) * x.inv.index_select(0, sub.nodes)[:, None]).contiguous()
        y = linear(xs, cat_w, cat_b)
        _oversize_conv(sub, y[:, :HC], y[:, HC:], edge_attr, w_edge, att, H, bias, node_mask, edge_mask, negative_slope,
                       out, alpha, rowmax)
    if rowmax is not None:
        attach_row_maxima(out, rowmax)
    if row_dead is not None:
        attach_dead_rows(out, row_dead)
    if sparse:
        _attach(out, "_isg_sparse_out", None if bias is None else bias.detach())
    return out, alpha


def gatv2_tile_conv(x_l: Tensor, x_r: Tensor, edge_attr: Tensor, w_edge: Tensor, att: Tensor, plan: "GraphPlan", heads: int,
                    bias: Optional[Tensor] = None, node_mask: Optional[Tensor] = None, edge_mask: Optional[Tensor] = None,
                    negative_slope: float = 0.2, want_rowmax: bool = False):
    """gatv2_mp(x_l, x_r, lin_edge(edge_attr), ...) as ONE launch per layer (mgat_v2_conv.py:243-279 with :259-261 inside):
    isg_gatv2_tile_conv.  Bit-identical to gatv2_mp_edge_logits (the two-launch pair it replaces).  Returns (out, alpha), or
    None when the kernel has no launch for this shape (the caller then runs the pair)."""
    lib = _lib.load()
    plan.require_csr()
    N, HC = x_l.shape
    H = int(heads)
    C = HC // H
    E, K = edge_attr.shape
    if N != plan.N or E != plan.E or tuple(w_edge.shape) != (HC, K) or tuple(x_r.shape) != (N, HC):
        raise ValueError("gatv2_tile_conv: operand shapes do not match the plan")
    if x_l.dtype != torch.float32 or x_r.dtype != torch.float32 or edge_attr.dtype != torch.float32:
        raise TypeError("gatv2_tile_conv: fp32 rows")
    we, we_inv = _weight_planes(w_edge, True, "f16x3")
    ep, ep_inv = plan.edge_planes(edge_attr)
    _, ntiles, cap, _ = plan.tiles(TILE_CONV_NODES, TILE_CONV_EDGES)
    shared, out, alpha, rowmax = _tile_conv_operands(plan, ntiles, cap, att, bias, node_mask, edge_mask, H, HC, want_rowmax,
                                                     x_l.device)
    xlp, xrp = _chk_rows(x_l, "x_l"), _chk_rows(x_r, "x_r")
    timer, ev1 = MP_TIMER, None
    if timer is not None:
        ev0, ev1 = timer.bracket({"N": N, "E": E, "H": H, "C": C, "K": K, "masked": node_mask is not None or edge_mask is not None,
                                  "feat_bytes": 4, "tile_conv": True})
        ev0.record()
    rc = lib.isg_gatv2_tile_conv(xlp, x_l.stride(0), xrp, x_r.stride(0), ep.data_ptr(), ep_inv.data_ptr(), we.data_ptr(),
                                 we_inv.data_ptr(), *shared, N, E, H, C, K, float(negative_slope), _stream())
    if not _launched(rc, "isg_gatv2_tile_conv", timer, ev1):
        return None
    sub = _mixed_sub(plan)
    if sub is not None:
        _oversize_conv(sub, x_l.index_select(0, sub.nodes), x_r.index_select(0, sub.nodes), edge_attr, w_edge, att, H, bias,
                       node_mask, edge_mask, negative_slope, out, alpha, rowmax)
    if rowmax is not None:
        attach_row_maxima(out, rowmax)
    return out, alpha


def _mp_rows_f32(x_l: Tensor, x_r: Tensor, e_proj: Tensor, plan: GraphPlan, H: int):
    """fp32 feature rows of the message-passing backward, dense: (x_l, x_r, e_proj as read, their three addresses)."""
    N, HC = x_l.shape
    E = plan.E
    x_l, x_r, e_proj = x_l.contiguous(), x_r.contiguous(), e_proj.contiguous()
    return (x_l, x_r, e_proj, _chk(x_l, "x_l", torch.float32, (N, HC)), _chk(x_r, "x_r", torch.float32, (N, HC)),
            _chk(e_proj, "e_proj", torch.float32, (E, HC)) if E > 0 else 0)


def _mp_rows_f16(x_l: Tensor, x_r: Tensor, e_proj: Tensor, plan: GraphPlan, H: int):
    """Half feature rows, read where they lie (rows strided by a multiple of 4 halves, columns contiguous)."""
    N, HC = x_l.shape
    E = plan.E
    if N != plan.N or H * (HC // H) != HC or tuple(x_r.shape) != (N, HC) or tuple(e_proj.shape) != (E, HC):
        raise ValueError(f"x_l / x_r must be [N, H*C] and e_proj [E, H*C] of plan N={plan.N}, E={E}, heads={H}")
    return (x_l, x_r, e_proj, _chk_rows(x_l, "x_l", torch.float16) if N > 0 else 0, _chk_rows(x_r, "x_r", torch.float16) if N > 0 else 0,
            _chk_rows(e_proj, "e_proj", torch.float16) if E > 0 else 0)


def _mp_pitches(x_l: Tensor, x_r: Tensor, e_proj: Tensor, d_x_l: Tensor, d_x_r: Tensor):
    """isg_gatv2_mp_bwd_f16's ld_l, ld_r, ld_e (halves), ld_dl, ld_dr (floats)."""
    HC = x_l.size(1)
    ld = lambda t: int(t.stride(0)) if t.size(0) > 1 else HC         # a single row has no pitch to speak of
    return ld(x_l), ld(x_r), ld(e_proj) if e_proj.size(0) > 0 else 0, ld(d_x_l), ld(d_x_r)


def _mp_backward(entry, name: str, rows, tail, x_l: Tensor, x_r: Tensor, e_proj: Tensor, att: Tensor, alpha: Tensor, grad_out: Tensor,
                 plan: GraphPlan, heads: int, node_mask: Optional[Tensor], edge_mask: Optional[Tensor], negative_slope: float,
                 want_mask_grad: bool, d_x_lr: Optional[Tensor] = None):
    """The message-passing backward marshalled once for its three entry points (isg_gatv2_mp_bwd, isg_gatv2_mp_bwd_dropout,
    isg_gatv2_mp_bwd_f16), which share their operand list up to the slope.  rows: _mp_rows_f32 or _mp_rows_f16, the feature rows
    checked; tail(x_l, x_r, e_proj, d_x_l, d_x_r): the entry point's arguments between the slope and the stream.  d_x_lr: see
    gatv2_mp_backward_f16.  Every tensor whose address is passed is a local here, held until the launch is queued."""
    plan.require_csr()
    N, HC = x_l.shape
    H = int(heads)
    C = HC // H
    E = plan.E
    dev = x_l.device
    x_l, x_r, e_proj, p_l, p_r, p_e = rows(x_l, x_r, e_proj, plan, H)
    grad_out = grad_out.contiguous()
    rowptr_s, eid_s, dst_s = plan.source_csr()
    if d_x_lr is None:
        d_x_l = torch.empty(N, HC, dtype=torch.float32, device=dev)
        d_x_r = torch.empty(N, HC, dtype=torch.float32, device=dev)
    else:
        if d_x_lr.dtype != torch.float32 or tuple(d_x_lr.shape) != (N, 2 * HC) or not d_x_lr.is_contiguous() or d_x_lr.device != dev:
            raise ValueError(f"d_x_lr: expected a contiguous fp32 [{N}, {2 * HC}] buffer on {dev}")
        d_x_l, d_x_r = d_x_lr[:, :HC], d_x_lr[:, HC:]
    d_e = torch.empty(E, HC, dtype=torch.float32, device=dev)
    part = torch.empty((N + 15) // 16, HC, dtype=torch.float32, device=dev)
    d_m = torch.empty(E, dtype=torch.float32, device=dev) if want_mask_grad else None
    att_flat = att.reshape(-1)
    node_flat = None if node_mask is None else node_mask.reshape(-1)
    edge_flat = None if edge_mask is None else edge_mask.reshape(-1)
    _lib.check(entry(
        p_l, p_r, p_e,
        _chk(att_flat, "att", torch.float32, (HC,)), _chk(alpha, "alpha", torch.float32, (E, H)) if E > 0 else 0,
        _chk(grad_out, "grad_out", torch.float32, (N, HC)),
        plan.rowptr.data_ptr(), plan.eid.data_ptr(), plan.src.data_ptr(),
        rowptr_s.data_ptr(), eid_s.data_ptr(), dst_s.data_ptr(),
        _chk(node_flat, "node_mask", torch.float32, (N,), optional=True),
        _chk(edge_flat, "edge_mask", torch.float32, (E,), optional=True),
        d_x_l.data_ptr(), d_x_r.data_ptr(), d_e.data_ptr(), part.data_ptr(), 0 if d_m is None else d_m.data_ptr(),
        N, E, H, C, float(negative_slope), *tail(x_l, x_r, e_proj, d_x_l, d_x_r), _stream()), name)
    return d_x_l, d_x_r, d_e, part.sum(0), grad_out.sum(0), d_m


def gatv2_mp_backward(x_l: Tensor, x_r: Tensor, e_proj: Tensor, att: Tensor, alpha: Tensor, grad_out: Tensor,
                      plan: GraphPlan, heads: int, node_mask: Optional[Tensor] = None,
                      edge_mask: Optional[Tensor] = None, negative_slope: float = 0.2, want_mask_grad: bool = False,
                      dropout_p: float = 0.0, dropout_seed: int = 0):
    """Backward of gatv2_mp: (d_x_l, d_x_r, d_e_proj, d_att[H*C], d_bias[H*C], d_edge_mask[E] or None).
    dropout_p / dropout_seed: those of the forward; the kernels draw its mask again (include/isg_mp_train.h).

    No reference counterpart file: the reference relies on autograd through PyG's propagate
    (mgat_v2_conv.py:215-279); the formulas are derived in csrc/isg_mp_bwd.hip.
    """
    drop = _drop_args(dropout_p, dropout_seed)
    if drop[0] > 0.0:
        from . import _lib_mp_train
        entry, name = _lib_mp_train.load().isg_gatv2_mp_bwd_dropout, "isg_gatv2_mp_bwd_dropout"
    else:
        entry, name, drop = _lib.load().isg_gatv2_mp_bwd, "isg_gatv2_mp_bwd", ()
    return _mp_backward(entry, name, _mp_rows_f32, lambda *_: drop, x_l, x_r, e_proj, att, alpha, grad_out, plan, heads, node_mask,
                        edge_mask, negative_slope, want_mask_grad)


def gatv2_mp_backward_f16(x_l: Tensor, x_r: Tensor, e_proj: Tensor, att: Tensor, alpha: Tensor, grad_out: Tensor,
                          plan: GraphPlan, heads: int, node_mask: Optional[Tensor] = None,
                          edge_mask: Optional[Tensor] = None, negative_slope: float = 0.2, want_mask_grad: bool = False,
                          dropout_p: float = 0.0, dropout_seed: int = 0, d_x_lr: Optional[Tensor] = None):
    """gatv2_mp_backward on saved rows stored as IEEE half (include/isg_mp_f16_train.h): the same tuple, every gradient fp32,
    the bits of gatv2_mp_backward on the same rows upcast.  x_l / x_r / e_proj may be column slices (rows strided by a multiple
    of 4 halves, columns contiguous): the halves of the fused [N, 2*H*C] projection are read where they lie.
    d_x_lr: a caller-owned fp32 [N, 2*H*C] buffer; d_x_l and d_x_r are then written into its column halves and returned as
    views of it -- the upstream gradient of the fused lin_l | lin_r Linear, with no torch.cat.  Its other contents are kept.
    Attention dropout has no half-row form (dropout_p > 0 raises)."""
    if _drop_args(dropout_p, dropout_seed)[0] > 0.0:
        raise _lib.IsgError("attention dropout exists on fp32 feature rows only (the half-row backward has no dropout form)")
    from . import _lib_mp_f16_train
    res = _mp_backward(_lib_mp_f16_train.load().isg_gatv2_mp_bwd_f16, "isg_gatv2_mp_bwd_f16", _mp_rows_f16, _mp_pitches, x_l, x_r,
                       e_proj, att, alpha, grad_out, plan, heads, node_mask, edge_mask, negative_slope, want_mask_grad, d_x_lr)
    COUNTERS["mp_f16_train"] += 1
    return res


def node_to_edge_mask_backward(d_edge_mask: Tensor, plan: GraphPlan) -> Tensor:
    """NodeMaskToEdgeMask.backward (sampling/node_edge_masks.py:13-19): scatter to the destination only."""
    lib = _lib.load()
    plan.require_csr()
    out = torch.empty(plan.N, dtype=torch.float32, device=d_edge_mask.device)
    _lib.check(lib.isg_node_to_edge_mask_bwd(_chk(d_edge_mask.reshape(-1), "d_edge_mask", torch.float32, (plan.E,)),
                                             plan.rowptr.data_ptr(), plan.eid.data_ptr(), out.data_ptr(), plan.N,
                                             _stream()), "isg_node_to_edge_mask_bwd")
    return out


def layer_tail_backward(ins, c, h, plan: GraphPlan, weight, bias, mean_scale, eps, node_mask, grad_out, want_mask: bool):
    """(d_ins, d_c, d_h, d_weight, d_bias, d_mean_scale, d_mask|None) of mgat_layer_tail."""
    lib = _lib.load()
    N, C = c.shape
    dev = c.device
    d_ins = torch.empty(plan.B, C, dtype=torch.float32, device=dev)
    d_c, d_h = torch.empty(N, C, dtype=torch.float32, device=dev), torch.empty(N, C, dtype=torch.float32, device=dev)
    d_mask = torch.empty(N, dtype=torch.float32, device=dev) if want_mask else None
    part = torch.empty(plan.B, 3, C, dtype=torch.float32, device=dev)
    _lib.check(lib.isg_instr_attn_graphnorm_residual_bwd(
        _chk(ins, "ins", torch.float32, (plan.B, C)), _chk(c, "c", torch.float32, (plan.N, C)),
        _chk(h, "h", torch.float32, (plan.N, C)), plan.ptr.data_ptr(), _chk(weight, "weight", torch.float32, (C,)),
        _chk(bias, "bias", torch.float32, (C,)), _chk(mean_scale, "mean_scale", torch.float32, (C,)), float(eps),
        _chk(None if node_mask is None else node_mask.reshape(-1), "node_mask", torch.float32, (N,), optional=True),
        _chk(grad_out, "grad_out", torch.float32, (N, C)), d_ins.data_ptr(), d_c.data_ptr(), d_h.data_ptr(),
        0 if d_mask is None else d_mask.data_ptr(), part.data_ptr(), plan.B, C, _stream()),
        "isg_instr_attn_graphnorm_residual_bwd")
    sums = part.sum(0)
    return d_ins, d_c, d_h, sums[0], sums[1], sums[2], d_mask


def global_attn_pool_backward(xn, q, plan: GraphPlan, node_mask, grad_out, grad_gate, want_mask: bool):
    """(d_xn, d_q, d_mask|None) of global_attn_pool."""
    lib = _lib.load()
    N, C = xn.shape
    d_xn = torch.empty(N, C, dtype=torch.float32, device=xn.device)
    d_q = torch.empty(plan.B, C, dtype=torch.float32, device=xn.device)
    d_mask = torch.empty(N, dtype=torch.float32, device=xn.device) if want_mask else None
    _lib.check(lib.isg_global_attn_pool_bwd(
        _chk(xn, "xn", torch.float32, (plan.N, C)), _chk(q, "q", torch.float32, (plan.B, C)), plan.ptr.data_ptr(),
        _chk(None if node_mask is None else node_mask.reshape(-1), "node_mask", torch.float32, (N,), optional=True),
        _chk(grad_out, "grad_out", torch.float32, (plan.B, C)),
        _chk(None if grad_gate is None else grad_gate.reshape(-1), "grad_gate", torch.float32, (N,), optional=True),
        d_xn.data_ptr(), d_q.data_ptr(), 0 if d_mask is None else d_mask.data_ptr(), plan.B, C, _stream()),
        "isg_global_attn_pool_bwd")
    return d_xn, d_q, d_mask


def instr_gate_backward(x, instr, plan: GraphPlan, grad_out):
    lib = _lib.load()
    N, C = x.shape
    d_x = torch.empty_like(x)
    d_instr = torch.empty(plan.B, C, dtype=torch.float32, device=x.device)
    _lib.check(lib.isg_instr_gate_bwd(_chk(x, "x", torch.float32, (plan.N, C)),
                                      _chk(instr, "instr", torch.float32, (plan.B, C)), plan.ptr.data_ptr(),
                                      _chk(grad_out, "grad_out", torch.float32, (N, C)), d_x.data_ptr(),
                                      d_instr.data_ptr(), plan.B, C, _stream()), "isg_instr_gate_bwd")
    return d_x, d_instr


def node_gate_backward(xn, q, batch, double_index: bool, plan: GraphPlan, grad_gate):
    """(d_xn, d_q): the per-graph partial rows are scattered into d_q here (several graphs may share a row of q)."""
    lib = _lib.load()
    N, C = xn.shape
    d_xn = torch.empty_like(xn)
    part = torch.empty(plan.B, C, dtype=torch.float32, device=xn.device)
    _lib.check(lib.isg_node_gate_bwd(_chk(xn, "xn", torch.float32, (plan.N, C)), _chk(q, "q", torch.float32, (q.size(0), C)),
                                     _chk(batch, "batch", torch.int64, (N,)), 1 if double_index else 0,
                                     plan.ptr.data_ptr(), _chk(grad_gate.reshape(-1), "grad_gate", torch.float32, (N,)),
                                     d_xn.data_ptr(), part.data_ptr(), N, plan.B, C, _stream()), "isg_node_gate_bwd")
    g = torch.arange(plan.B, device=xn.device)
    rows = batch[g.clamp(max=max(N - 1, 0))] if double_index else g
    return d_xn, torch.zeros_like(q).index_add_(0, rows, part)


def mp_algorithmic_bytes(N: int, E: int, H: int, C: int, masked: bool, feat_bytes: int = 4) -> int:
    """bytes_mp = s*(3*N*HC + E*HC) + 4*E*H + 16*E (+4*E if edge-masked)."""
    HC = H * C
    return feat_bytes * (3 * N * HC + E * HC) + 4 * E * H + 16 * E + (4 * E if masked else 0)


def edge_logits_algorithmic_bytes(N: int, E: int, H: int, C: int, K: int, masked: bool, K2: int = 0, feat_bytes: int = 4) -> int:
    """isg_gatv2_edge_logits' OWN minimum traffic: edge_attr rows (4*E*K), every x_l and x_r row once (2 * 4*N*HC), the
    logits (4*E*H), eid / src / dst (12*E), the edge mask if any (4*E).  The W planes (4*HC*K) stay in L2.  K2 > 0: the
    form that computes x_r itself reads every layer-input row once (4*N*K2) instead of x_r (4*N*HC)."""
    xr = 4 * N * K2 if K2 else feat_bytes * N * H * C
    return 4 * E * K + feat_bytes * N * H * C + xr + 4 * E * H + 12 * E + (4 * E if masked else 0)


def mp_logits_algorithmic_bytes(N: int, E: int, H: int, C: int, masked: bool, feat_bytes: int = 4) -> int:
    """isg_gatv2_mp_fwd_logits' OWN minimum traffic: x_l in and out back (2 * 4*N*HC), logits in and alpha out (8*E*H),
    the CSR (16*E as in bytes_mp), the edge mask if any (4*E)."""
    return 2 * feat_bytes * N * H * C + 8 * E * H + 16 * E + (4 * E if masked else 0)


def scatter_mean(msg: Tensor, plan: GraphPlan) -> Tensor:
    """scatter_mean(msg, dst, dim_size=N)   (scene_graph_encoder.py:141)"""
    if _rec(msg):
        from . import autograd
        return autograd.scatter_mean(msg, plan)
    lib = _lib.load()
    plan.require_csr()
    E, C = msg.shape
    if E != plan.E:
        raise ValueError(f"msg has {E} rows, plan has {plan.E} edges")
    out = torch.empty(plan.N, C, dtype=torch.float32, device=msg.device)
    _lib.check(lib.isg_scatter_mean(_chk(msg, "msg", torch.float32), plan.rowptr.data_ptr(), plan.eid.data_ptr(),
                                    out.data_ptr(), plan.N, C, _stream()), "isg_scatter_mean")
    return out


# ------------------------------------------------------------------------------------------------
# Node gate + samplers
# ------------------------------------------------------------------------------------------------
def node_gate(xn: Tensor, q: Tensor, batch: Tensor, double_index: bool, plan: Optional["GraphPlan"] = None) -> Tensor:
    """gelu(<xn_n, q[r(n)]>/sqrt(C)) -> [N,1]   (masking.py:151-155).  ``plan`` selects the HIP backward."""
    if _rec(xn, q):
        from . import autograd
        return autograd.node_gate(xn, q, batch, double_index, plan)
    lib = _lib.load()
    N, C = xn.shape
    gate = torch.empty(N, 1, dtype=torch.float32, device=xn.device)
    _lib.check(lib.isg_node_gate(_chk(xn, "xn", torch.float32), _chk(q, "q", torch.float32, (q.size(0), C)),
                                 _chk(batch, "batch", torch.int64, (N,)), 1 if double_index else 0, gate.data_ptr(),
                                 N, C, _stream()), "isg_node_gate")
    return gate


def node_gate_planes_supported(node_nn: torch.nn.Sequential, q: Tensor) -> bool:
    """Shape test of isg_node_gate_planes: inference, node_nn = Linear(128 -> 128) + exact GELU, 128-wide question rows."""
    if not (CFG.fuse_gate and CFG.gemm_backend == "bf16x6" and CFG.gemm_f16x3) or torch.is_grad_enabled():
        return False
    mods = list(node_nn)
    if len(mods) != 2 or not isinstance(mods[0], torch.nn.Linear) or not isinstance(mods[1], torch.nn.GELU) \
            or mods[1].approximate != "none" or mods[0].bias is None:
        return False
    return tuple(mods[0].weight.shape) == (128, 128) and q.dim() == 2 and q.size(1) == 128 and q.dtype == torch.float32


def node_gate_planes(x: "NodePlanes", node_nn: torch.nn.Sequential, q: Tensor, batch: Tensor, double_index: bool) -> Tensor:
    """gelu(<gelu(node_nn(x))_n, q[r(n)]>/sqrt(C)) -> [N,1] (masking.py:137, 151-155) from the layer input as NodePlanes:
    isg_node_gate_planes.  The caller checks node_gate_planes_supported() first."""
    lib = _lib.load()
    N = batch.numel()
    l0 = node_nn[0]
    wp, w_inv = _weight_planes(l0.weight, True, "f16x3")
    gate = torch.empty(N, 1, dtype=torch.float32, device=q.device)
    _lib.check(lib.isg_node_gate_planes(x.planes.data_ptr(), x.inv.data_ptr(), wp.data_ptr(), w_inv.data_ptr(),
                                        _chk(l0.bias.detach(), "node_nn.0.bias", torch.float32, (128,)),
                                        _chk(q, "q", torch.float32, (q.size(0), 128)), _chk(batch, "batch", torch.int64, (N,)),
                                        1 if double_index else 0, gate.data_ptr(), N, 128, _stream()), "isg_node_gate_planes")
    return gate


def _rows(scores: Tensor, plan: Optional[GraphPlan]):
    """(ptr, B, nmax_host, nmax_dev, out) for the ragged (plan) or dense ([B,Nmax]) row layout."""
    if plan is not None:
        flat = scores.reshape(-1)
        if flat.numel() != plan.N:
            raise ValueError(f"scores has {flat.numel()} entries, plan has {plan.N} nodes")
        return flat, plan.ptr.data_ptr(), plan.B, plan.nmax, plan.nmax_dev.data_ptr()
    if scores.dim() != 2:
        raise ValueError("dense scores must be [B, Nmax]")
    if scores.size(1) > MAX_NODES_PER_GRAPH:
        raise _lib.IsgError(f"rows longer than {MAX_NODES_PER_GRAPH} slots are unsupported")
    return scores, 0, scores.size(0), scores.size(1), 0


def _gid_ptr(plan: Optional["GraphPlan"]) -> int:
    """The graph-id table of a plan that is a CUT of a larger batch (run_split's sub-batch: plan.graph_ids = int32 [B], the graphs'
    numbers in the batch they came from): row b of a sampler then draws the Philox stream of graph graph_ids[b], i.e. the noise
    that graph gets when the batch is not split (seeded masks do not depend on the dispatch).  0: row b draws stream b."""
    g = None if plan is None else plan.graph_ids
    if g is None:
        return 0
    if g.dtype != torch.int32 or g.numel() != plan.B or not g.is_contiguous():
        raise ValueError("plan.graph_ids must be a contiguous int32 [B] tensor")
    return g.data_ptr()


def _noise_ptr(noise: Optional[Tensor], B: int, nmax: int) -> int:
    if noise is None:
        return 0
    if noise.numel() != B * nmax:
        raise ValueError(f"noise must hold B*Nmax = {B}*{nmax} values, got {tuple(noise.shape)}")
    return _chk(noise.reshape(B, nmax), "noise", torch.float32)


def topk_budget(plan: GraphPlan, ratio: float, k_min: int, k_cap: int) -> Tensor:
    """The per-graph node budget k_rows int32 [B]: k_rows[b] = min(k_cap, max(k_min, ceil(ratio * n_b))), n_b the graph's node
    count -- torch.ceil(torch.tensor(ratio, dtype=torch.float32) * n.float()), clamped (isg_topk_budget).  One launch,
    nothing is read back (usable inside a capture), kept in plan.memo() under its arguments: a batch's layers share one tensor."""
    ratio, k_min, k_cap = float(ratio), int(k_min), int(k_cap)
    if not ratio > 0.0 or k_min < 1 or k_cap < k_min:
        raise ValueError(f"topk_budget needs 0 < ratio and 1 <= k_min <= k_cap, got ratio={ratio}, k_min={k_min}, k_cap={k_cap}")
    key = ("topk_budget", ratio, k_min, k_cap)
    hit = plan.memo().get(key)
    if hit is None:
        from . import _lib_topk_rows
        lib = _lib_topk_rows.load()
        hit = torch.empty(plan.B, dtype=torch.int32, device=plan.ptr.device)
        _lib.check(lib.isg_topk_budget(plan.ptr.data_ptr(), plan.B, ratio, k_min, k_cap, hit.data_ptr(), _stream()),
                   "isg_topk_budget")
        plan.memo()[key] = hit
    return hit


def _k_rows(k, k_cap: Optional[int], B: int, device) -> Optional[Tuple[int, int]]:
    """None for an int k (the scalar entry points).  For a tensor k -- a k per row, int32 [B] on the rows' device, entries in
    [1, k_cap] -- (its address, k_cap); the caller holds the tensor until the launch is queued."""
    if not isinstance(k, Tensor):
        if k_cap is not None:
            raise ValueError("k_cap goes with a tensor k (a k per row); an int k is its own bound")
        return None
    if k_cap is None:
        raise ValueError("a tensor k (a k per row) needs k_cap, the bound of its entries")
    if k.dtype != torch.int32 or k.device != device or k.dim() != 1 or k.numel() != B or not k.is_contiguous():
        raise ValueError(f"a k per row must be a contiguous int32 [{B}] tensor on {device}, got {k.dtype} {tuple(k.shape)} on {k.device}")
    if int(k_cap) < 1:
        raise ValueError(f"k_cap must be at least 1, got {k_cap}")
    return k.data_ptr(), int(k_cap)


def topk_gumbel(scores: Tensor, k, tau: float = 0.1, plan: Optional[GraphPlan] = None,
                noise: Optional[Tensor] = None, seed: int = 0, return_khot: bool = False, k_cap: Optional[int] = None):
    """Relaxed Gumbel top-k + straight-through hard mask (gumbel_scheme.py:55-104).

    Ragged (plan given): scores [N] / [N,1] -> mask of the same shape (the dense-pad and the `[mask]`
    un-pad of masking.py:162,176 are fused).  Dense: scores [B,Nmax] -> [B,Nmax].
    ``k``: an int, or a k per row as an int32 [B] device tensor with ``k_cap`` the bound of its entries (isg_topk_gumbel_rows).
    """
    if _rec(scores):
        from . import autograd
        if return_khot:
            raise ValueError("return_khot is an inspection output and is not differentiable")
        return autograd.topk_gumbel(scores, k, tau, plan, noise, seed, k_cap)
    flat, ptr, B, nmax, nmax_dev = _rows(scores, plan)
    rows = _k_rows(k, k_cap, B, scores.device)
    out = torch.empty_like(flat)
    khot = torch.empty(B, nmax, dtype=torch.float32, device=scores.device) if return_khot else None
    if rows is None:
        lib = _lib.load()
        _lib.check(lib.isg_topk_gumbel(_chk(flat, "scores", torch.float32), ptr, B, nmax, nmax_dev,
                                       _noise_ptr(noise, B, nmax), int(seed) & (2 ** 64 - 1), _gid_ptr(plan), int(k), float(tau),
                                       out.data_ptr(), 0 if khot is None else khot.data_ptr(), _stream()),
                   "isg_topk_gumbel")
    else:
        from . import _lib_topk_rows
        _lib.check(_lib_topk_rows.load().isg_topk_gumbel_rows(
            _chk(flat, "scores", torch.float32), ptr, B, nmax, nmax_dev, _noise_ptr(noise, B, nmax), int(seed) & (2 ** 64 - 1),
            _gid_ptr(plan), rows[0], rows[1], float(tau), out.data_ptr(), 0 if khot is None else khot.data_ptr(), _stream()),
            "isg_topk_gumbel_rows")
        COUNTERS["topk_rows"] += 1
    out = out.view(scores.shape)
    return (out, khot) if return_khot else out


def topk_threshold(scores: Tensor, k, plan: Optional[GraphPlan] = None, noise: Optional[Tensor] = None,
                   noise_scale: float = 0.0, seed: int = 0, return_dense: bool = False, k_cap: Optional[int] = None):
    """(scores + noise*noise_scale) >= k-th largest, per row (deterministic_scheme.py:36-43).  Not differentiable by
    itself: the I-MLE / AIMLE estimators around it are autograd.imle_topk / aimle_topk.  ``return_dense`` also returns
    the selection over the padded [B, Nmax] rows (pads included).  ``k``: an int, or a k per row as an int32 [B] device tensor
    with ``k_cap`` the bound of its entries (isg_topk_threshold_rows)."""
    scores = scores.detach()
    flat, ptr, B, nmax, nmax_dev = _rows(scores, plan)
    rows = _k_rows(k, k_cap, B, scores.device)
    out = torch.empty_like(flat)
    dense = torch.empty(B, nmax, dtype=torch.float32, device=scores.device) if return_dense else None
    if rows is None:
        lib = _lib.load()
        _lib.check(lib.isg_topk_threshold(_chk(flat, "scores", torch.float32), ptr, B, nmax, nmax_dev,
                                          _noise_ptr(noise, B, nmax), float(noise_scale), int(seed) & (2 ** 64 - 1), _gid_ptr(plan),
                                          int(k), out.data_ptr(), 0 if dense is None else dense.data_ptr(), _stream()),
                   "isg_topk_threshold")
    else:
        from . import _lib_topk_rows
        _lib.check(_lib_topk_rows.load().isg_topk_threshold_rows(
            _chk(flat, "scores", torch.float32), ptr, B, nmax, nmax_dev, _noise_ptr(noise, B, nmax), float(noise_scale),
            int(seed) & (2 ** 64 - 1), _gid_ptr(plan), rows[0], rows[1], out.data_ptr(),
            0 if dense is None else dense.data_ptr(), _stream()), "isg_topk_threshold_rows")
        COUNTERS["topk_rows"] += 1
    out = out.view(scores.shape)
    return (out, dense) if return_dense else out


def _simple_n(nmax: int) -> int:
    """Variables of the SIMPLE circuit over rows of nmax slots: nmax rounded up to a power of two (simple_scheme.py:88)."""
    return 1 << max(nmax - 1, 0).bit_length() if nmax > 0 else 0


def _simple_rows(scores: Tensor, plan: Optional[GraphPlan]):
    """_rows for the SIMPLE sampler's forward and backward, (flat, ptr, B, nmax): nmax is the true longest row under a max_nodes
    hint too (GraphPlan.true_nmax), so that a backward follows the row length of the forward it differentiates."""
    flat, ptr, B, nmax, _ = _rows(scores, plan)
    return flat, ptr, B, (nmax if plan is None else plan.true_nmax("the SIMPLE sampler"))


def simple_topk(scores: Tensor, k: int, plan: Optional[GraphPlan] = None, uniform: Optional[Tensor] = None,
                seed: int = 0, return_marginals: bool = False):
    """SIMPLE sampler (simple_scheme.py:44-162): mask = (Gumbel top-k sample - marginals) + marginals, marginals exact
    through the exactly-k circuit.  Ragged (plan given): scores [N] / [N,1]; dense: scores [B,Nmax].  ``uniform``: the [B, n]
    torch.rand draw (n = Nmax rounded up to a power of two).  ``k`` is an int: the circuit and its tables are built per (n, k)
    for the launch, a k per row is not implemented.

    Nmax is the batch's TRUE longest row, never a bound of it: the number of zero pads and of -1e10 pads behind a row decides
    its marginals, so a plan built with ``max_nodes=`` (plan.nmax is then the hint) gives the un-hinted plan's bits.  The
    length is read from plan.nmax_dev -- one device-to-host copy per hinted plan (GraphPlan.true_nmax), none on other plans;
    during a stream capture, where that copy is impossible, IsgError is raised before any launch.  The marginals are
    [B, true Nmax].  On a hinted plan ``uniform`` may also be [B, n(hint)], the draw of a caller who knows the hint alone: its
    first n(true) columns are the draw, the rule Gumbel noise follows under a hint."""
    if isinstance(k, Tensor):
        raise NotImplementedError("simple_topk takes one k for the batch: the SIMPLE sampler's circuit and tables are built per "
                                  "(n, k) for the launch, so a per-graph budget (a k per row) is out of its scope")
    if _rec(scores):
        from . import autograd
        return autograd.simple_topk(scores, k, plan, uniform, seed, return_marginals)
    lib = _lib.load()
    flat, ptr, B, nmax = _simple_rows(scores, plan)
    out = torch.empty_like(flat)
    n = _simple_n(nmax)
    if uniform is not None:
        n_hint = n if plan is None else _simple_n(plan.nmax)
        if uniform.numel() == B * n:
            uniform = uniform.reshape(B, n)
        elif uniform.numel() == B * n_hint:
            uniform = uniform.reshape(B, n_hint)[:, :n].contiguous()     # the kernel strides the draw by n
        else:
            raise ValueError(f"uniform must hold B*n = {B}*{n} values" + (f" (or {B}*{n_hint}, by the plan's max_nodes hint)"
                                                                          if n_hint != n else "") + f", got {tuple(uniform.shape)}")
    marg = torch.empty(B, nmax, dtype=torch.float32, device=scores.device) if return_marginals else None
    _lib.check(lib.isg_simple_topk(_chk(flat, "scores", torch.float32), ptr, B, nmax,
                                   0 if uniform is None else _chk(uniform, "uniform", torch.float32),
                                   int(seed) & (2 ** 64 - 1), _gid_ptr(plan), int(k), out.data_ptr(),
                                   0 if marg is None else marg.data_ptr(), _stream()), "isg_simple_topk")
    out = out.view(scores.shape)
    return (out, marg) if return_marginals else out


def simple_topk_backward(scores: Tensor, k: int, plan: Optional[GraphPlan] = None, g_out: Optional[Tensor] = None,
                         g_marg: Optional[Tensor] = None) -> Optional[Tensor]:
    """d scores of simple_topk for d out = g_out (the layout of scores) and d marginals = g_marg ([B, Nmax]); either may be None
    (= 0).  One launch of isg_simple_topk_bwd, which rebuilds the circuit's trees from the scores alone: the sample carries no
    gradient, so neither ``uniform`` nor ``seed`` is an argument.  None when the library refuses the shape (a row whose four trees
    exceed the LDS rule of isg_simple_topk_bwd_row_bytes): the caller differentiates the torch restatement instead.
    Nmax is the forward's: the batch's true longest row, on a plan built with ``max_nodes=`` too (see simple_topk)."""
    from . import _lib_sampler_train
    lib = _lib_sampler_train.load()
    scores = scores.detach()
    flat, ptr, B, nmax = _simple_rows(scores, plan)
    go = None if g_out is None else g_out.detach().reshape(flat.shape)          # held until the launch is queued
    gm = None if g_marg is None else g_marg.detach().reshape(B, nmax)
    d = torch.empty_like(flat)
    status = lib.isg_simple_topk_bwd(_chk(flat, "scores", torch.float32), ptr, B, nmax, int(k),
                                     _chk(go, "g_out", torch.float32, optional=True), _chk(gm, "g_marg", torch.float32, optional=True),
                                     d.data_ptr(), _stream())
    if status == ISG_EUNSUPPORTED:
        return None
    _lib.check(status, "isg_simple_topk_bwd")
    COUNTERS["simple_bwd_kernel"] += 1
    return d.view(scores.shape)


def topk_gumbel_backward(scores: Tensor, grad_out: Tensor, k, tau: float = 0.1, plan: Optional[GraphPlan] = None,
                         noise: Optional[Tensor] = None, seed: int = 0, k_cap: Optional[int] = None) -> Tensor:
    """d scores of topk_gumbel for d out = grad_out (straight-through, gumbel_scheme.py:83-90); same arguments as the
    forward (the relaxation is replayed from scores + noise/seed).  With a k per row, ``k_cap`` sizes the kernel's LDS history."""
    flat, ptr, B, nmax, nmax_dev = _rows(scores, plan)
    rows = _k_rows(k, k_cap, B, scores.device)
    g = grad_out.reshape(flat.shape).contiguous()
    out = torch.empty_like(flat)
    if rows is None:
        lib = _lib.load()
        _lib.check(lib.isg_topk_gumbel_bwd(_chk(flat, "scores", torch.float32), ptr, B, nmax, nmax_dev,
                                           _noise_ptr(noise, B, nmax), int(seed) & (2 ** 64 - 1), _gid_ptr(plan), int(k), float(tau),
                                           _chk(g, "grad_out", torch.float32), out.data_ptr(), _stream()),
                   "isg_topk_gumbel_bwd")
    else:
        from . import _lib_topk_rows
        _lib.check(_lib_topk_rows.load().isg_topk_gumbel_rows_bwd(
            _chk(flat, "scores", torch.float32), ptr, B, nmax, nmax_dev, _noise_ptr(noise, B, nmax), int(seed) & (2 ** 64 - 1),
            _gid_ptr(plan), rows[0], rows[1], float(tau), _chk(g, "grad_out", torch.float32), out.data_ptr(), _stream()),
            "isg_topk_gumbel_rows_bwd")
        COUNTERS["topk_rows"] += 1
    return out.view(scores.shape)


# ------------------------------------------------------------------------------------------------
# Per-graph attention / norm / pooling
# ------------------------------------------------------------------------------------------------
def scatter_attention(query: Tensor, key: Tensor, plan: GraphPlan, value: Optional[Tensor] = None) -> Tensor:
    """softmax_g(<query_g, key_n>/sqrt(C)) * value_n   (utils/scatter_scaled_dot_product.py:6-15)"""
    if value is None:
        value = key
    if _rec(query, key, value):
        from . import autograd
        return autograd.scatter_attention(query, key, plan, value)
    lib = _lib.load()
    N, C = key.shape
    out = torch.empty_like(value)
    _lib.check(lib.isg_scatter_attention(_chk(query, "query", torch.float32, (plan.B, C)),
                                         _chk(key, "key", torch.float32, (plan.N, C)),
                                         _chk(value, "value", torch.float32, (plan.N, C)),
                                         plan.ptr.data_ptr(), out.data_ptr(), plan.B, C, _stream()),
               "isg_scatter_attention")
    return out


def graph_norm(x: Tensor, plan: GraphPlan, weight: Tensor, bias: Tensor, mean_scale: Tensor, eps: float = 1e-5,
               fp64: bool = False) -> Tensor:
    """PyG GraphNorm forward (mgat.py:171); fp64=True mirrors scene_graph_encoder.py:99-102."""
    if _rec(x, weight, bias, mean_scale):
        from . import autograd
        return autograd.graph_norm(x, plan, weight, bias, mean_scale, eps, fp64)
    lib = _lib.load()
    N, C = x.shape
    out = torch.empty_like(x)
    _lib.check(lib.isg_graph_norm(_chk(x, "x", torch.float32, (plan.N, C)), plan.ptr.data_ptr(),
                                  _chk(weight, "weight", torch.float32, (C,)), _chk(bias, "bias", torch.float32, (C,)),
                                  _chk(mean_scale, "mean_scale", torch.float32, (C,)), float(eps), 1 if fp64 else 0,
                                  out.data_ptr(), plan.B, C, _stream()), "isg_graph_norm")
    return out


def mgat_layer_tail(ins: Tensor, c: Tensor, h: Tensor, plan: GraphPlan, weight: Tensor, bias: Tensor,
                    mean_scale: Tensor, eps: float = 1e-5, node_mask: Optional[Tensor] = None) -> Tensor:
    """scatter attention -> GraphNorm -> + h [-> * mask], fused (mgat.py:168-177)."""
    if _rec(ins, c, h, weight, bias, mean_scale, node_mask):
        from . import autograd
        return autograd.mgat_layer_tail(ins, c, h, plan, weight, bias, mean_scale, eps, node_mask)
    lib = _lib.load()
    N, C = c.shape
    out = torch.empty_like(h)
    _lib.check(lib.isg_instr_attn_graphnorm_residual(
        _chk(ins, "ins", torch.float32, (plan.B, C)), _chk(c, "c", torch.float32, (plan.N, C)),
        _chk(h, "h", torch.float32, (plan.N, C)), plan.ptr.data_ptr(), _chk(weight, "weight", torch.float32, (C,)),
        _chk(bias, "bias", torch.float32, (C,)), _chk(mean_scale, "mean_scale", torch.float32, (C,)), float(eps),
        _chk(None if node_mask is None else node_mask.reshape(-1), "node_mask", torch.float32, (N,), optional=True),
        out.data_ptr(), plan.B, C, _stream()), "isg_instr_attn_graphnorm_residual")
    return out


def dense_tail_supported(plan: GraphPlan, x_proj: torch.nn.Sequential, width_in: int, channels: int) -> bool:
    """Shape test of isg_mgat_dense_tail (csrc/isg_layer_tile.hip): inference, fp32, Linear(512 -> 256) GELU Linear(256 ->
    128) GELU (MGAT at C = 128, H = 4: BASELINE configs[1]), every graph within one 64-node tile."""
    if not (CFG.fuse_dense_tail and CFG.gemm_backend == "bf16x6" and CFG.gemm_f16x3) or torch.is_grad_enabled():
        return False
    mods = list(x_proj)
    if len(mods) != 4 or not all(isinstance(m, torch.nn.GELU) and m.approximate == "none" for m in (mods[1], mods[3])):
        return False
    l0, l2 = mods[0], mods[2]
    if not (isinstance(l0, torch.nn.Linear) and isinstance(l2, torch.nn.Linear)) or l0.bias is None or l2.bias is None:
        return False
    return (width_in == 512 and channels == 128 and tuple(l0.weight.shape) == (256, 512) and
            tuple(l2.weight.shape) == (128, 256) and plan.B > 0 and plan.batch is not None and
            plan.tile_mode(CFG.dense_tail_rows, TILE_CONV_EDGES) != "none")


def mgat_dense_tail(conv_out: Tensor, x_proj: torch.nn.Sequential, ins: Tensor, h: Tensor, plan: GraphPlan, weight: Tensor,
                    bias: Tensor, mean_scale: Tensor, eps: float = 1e-5, node_mask: Optional[Tensor] = None,
                    ins_next: Optional[Tensor] = None, want_rows: bool = True, want_planes: bool = False,
                    group: Optional[int] = None) -> Optional[Tuple[Tensor, Optional[Tensor], Optional["NodePlanes"]]]:
    """mgat.py:156-177 after the convolution, plus the next layer's instruction gate (mgat_v2_conv.py:156-157), as one launch:
    x_proj (Linear GELU Linear GELU) -> scatter attention -> GraphNorm -> + h [-> * mask] -> (h', xg, xg planes) with
    xg = gelu(h' * ins_next[batch]) as fp32 rows (want_rows) and / or as NodePlanes for gatv2_layer_conv (want_planes).
    conv_out must carry its row maxima (the message-passing kernels leave them); returns None when it does not (the caller
    runs the un-fused chain).  The caller checks dense_tail_supported() first.
    When conv_out also carries the dead-row flags of a masked gatv2_layer_conv launch, the kernel's live-row form runs x_proj once
    per `group` tiles, on their live rows plus one dead row; group = None: dense_tail_group's rule."""
    lib = _lib.load()
    N, K1 = conv_out.shape
    dead = dead_rows(conv_out)
    if dead is not None and (tuple(dead.shape) != (N, 4) or dead.dtype != torch.uint8 or not dead.is_contiguous()):
        dead = None
    if dead is None or dense_tail_dense_rows():
        conv_out = dense_conv_out(conv_out)       # the form that reads every row (identity unless a sparse launch left conv_out)
    rm = row_maxima(conv_out)
    if rm is None or rm.dim() != 2 or rm.size(0) != N or rm.stride(1) != 1 or rm.dtype != torch.float32:
        return None
    l0, l2 = x_proj[0], x_proj[2]
    C = l2.weight.size(0)
    p1, inv1 = _weight_planes(l0.weight, True, "f16x3")
    p2, inv2 = _weight_planes(l2.weight, True, "f16x3")
    ybound = derived_weight("dense_tail_bound", (l0.weight, l0.bias), lambda: torch.stack(
        [l0.weight.detach().abs().sum(dim=1).max(), l0.bias.detach().abs().max()]).float().contiguous())
    # one tile plan per batch: the convolution's (64 nodes / 256 slots) serves this kernel too when it exists
    # one tile plan per batch, the convolution's (64 nodes / 256 slots): the same graphs are "oversize" for every tile kernel
    tile_ptr, ntiles, cap, tile_info = plan.tiles(CFG.dense_tail_rows, TILE_CONV_EDGES if plan.rowptr is not None else 0)
    if dead is not None and group is None:
        group = dense_tail_group(N, plan.E if plan.rowptr is not None else 0, h.device)
    h_out = torch.empty_like(h)
    xg = torch.empty_like(h) if ins_next is not None and want_rows else None
    xp = _empty_node_planes(N, h.device) if ins_next is not None and want_planes else None
    rc = lib.isg_mgat_dense_tail(
        _chk_rows(conv_out, "conv_out"), conv_out.stride(0), rm.data_ptr(), rm.size(1), rm.stride(0),
        p1.data_ptr(), inv1.data_ptr(), _chk(l0.bias.detach(), "x_proj.0.bias", torch.float32, (l0.weight.size(0),)),
        ybound.data_ptr(), p2.data_ptr(), inv2.data_ptr(), _chk(l2.bias.detach(), "x_proj.2.bias", torch.float32, (C,)),
        _chk(ins, "ins", torch.float32, (plan.B, C)), _chk(h, "h", torch.float32, (plan.N, C)),
        _chk(weight.detach(), "weight", torch.float32, (C,)), _chk(bias.detach(), "bias", torch.float32, (C,)),
        _chk(mean_scale.detach(), "mean_scale", torch.float32, (C,)), float(eps),
        _chk(None if node_mask is None else node_mask.reshape(-1), "node_mask", torch.float32, (N,), optional=True),
        _chk(ins_next, "ins_next", torch.float32, (plan.B, C), optional=True), h_out.data_ptr(),
        0 if xg is None else xg.data_ptr(), 0 if xp is None else xp.planes.data_ptr(), 0 if xp is None else xp.inv.data_ptr(),
        plan.ptr.data_ptr(), _chk(plan.batch, "batch", torch.int64, (N,)),
        tile_ptr.data_ptr(), tile_info.data_ptr(), ntiles.data_ptr(), cap, 0 if dead is None else dead.data_ptr(),
        1 if dead is None else int(group), N, K1, l0.weight.size(0), C, _stream())
    if rc == ISG_EUNSUPPORTED:
        return None
    _lib.check(rc, "isg_mgat_dense_tail")
    sub = _mixed_sub(plan)
    if sub is not None:
        # mgat.py:156-177 on the graphs the tile kernel passed over: x_proj, the per-graph layer tail, the next gate
        cs = mlp(x_proj, dense_conv_out(conv_out).index_select(0, sub.nodes))
        nm = None if node_mask is None else node_mask.reshape(-1).index_select(0, sub.nodes).view(-1, 1)
        hs = mgat_layer_tail(ins.index_select(0, sub.gids), cs.contiguous(), h.index_select(0, sub.nodes), sub.plan, weight, bias,
                             mean_scale, eps, node_mask=nm)
        h_out.index_copy_(0, sub.nodes, hs)
        if ins_next is not None and (xg is not None or xp is not None):
            rows, pl = instr_gate_planes(hs, ins_next.index_select(0, sub.gids), sub.batch, want_rows=xg is not None)
            if xg is not None:
                xg.index_copy_(0, sub.nodes, rows)
            if xp is not None:
                xp.planes.index_copy_(0, sub.nodes, pl.planes[:sub.nodes.numel()])
                xp.inv.index_copy_(0, sub.nodes, pl.inv[:sub.nodes.numel()])
    return h_out, xg, xp


def readout_tile_supported(plan: GraphPlan, node_nn: torch.nn.Sequential, width_in: int) -> bool:
    """Shape test of isg_readout_tile: inference, fp32, node_nn = Linear(128 -> 128) GELU Linear(128 -> 128), tiles of 64 nodes."""
    if not (CFG.fuse_readout and CFG.gemm_backend == "bf16x6" and CFG.gemm_f16x3) or torch.is_grad_enabled():
        return False
    mods = list(node_nn)
    if len(mods) != 3 or not isinstance(mods[1], torch.nn.GELU) or mods[1].approximate != "none":
        return False
    l0, l2 = mods[0], mods[2]
    if not (isinstance(l0, torch.nn.Linear) and isinstance(l2, torch.nn.Linear)) or l0.bias is None or l2.bias is None:
        return False
    return (width_in == 128 and tuple(l0.weight.shape) == (128, 128) and tuple(l2.weight.shape) == (128, 128) and plan.B > 0 and
            plan.batch is not None and plan.tile_mode(CFG.dense_tail_rows, TILE_CONV_EDGES) != "none")


def readout_tile(x: Tensor, node_nn: torch.nn.Sequential, q: Tensor, plan: GraphPlan, node_mask: Optional[Tensor] = None):
    """GlobalAttention.forward's device work as ONE launch (att_pooling.py:57-77): node_nn(x) * mask, per-graph softmax of
    <xn, q>/sqrt(C), pooled sum.  Returns (out [B,C], gate [N,1]) or None when the kernel has no launch for this shape."""
    lib = _lib.load()
    N, C = x.shape
    l0, l2 = node_nn[0], node_nn[2]
    p1, inv1 = _weight_planes(l0.weight, True, "f16x3")
    p2, inv2 = _weight_planes(l2.weight, True, "f16x3")
    ybound = derived_weight("dense_tail_bound", (l0.weight, l0.bias), lambda: torch.stack(
        [l0.weight.detach().abs().sum(dim=1).max(), l0.bias.detach().abs().max()]).float().contiguous())
    tile_ptr, ntiles, cap, tile_info = plan.tiles(CFG.dense_tail_rows, TILE_CONV_EDGES if plan.rowptr is not None else 0)
    out = torch.empty(plan.B, C, dtype=torch.float32, device=x.device)
    gate = torch.empty(N, 1, dtype=torch.float32, device=x.device)
    rc = lib.isg_readout_tile(
        _chk_rows(x, "x"), x.stride(0), p1.data_ptr(), inv1.data_ptr(), _chk(l0.bias.detach(), "node_nn.0.bias", torch.float32, (C,)),
        ybound.data_ptr(), p2.data_ptr(), inv2.data_ptr(), _chk(l2.bias.detach(), "node_nn.2.bias", torch.float32, (C,)),
        _chk(q, "q", torch.float32, (plan.B, C)),
        _chk(None if node_mask is None else node_mask.reshape(-1), "node_mask", torch.float32, (N,), optional=True),
        out.data_ptr(), gate.data_ptr(), plan.ptr.data_ptr(), _chk(plan.batch, "batch", torch.int64, (N,)), tile_ptr.data_ptr(),
        tile_info.data_ptr(), ntiles.data_ptr(), cap, N, C, _stream())
    if rc == ISG_EUNSUPPORTED:
        return None
    _lib.check(rc, "isg_readout_tile")
    sub = _mixed_sub(plan)
    if sub is not None:
        # att_pooling.py:62-73 on the graphs the tile kernel passed over (it zeroed their rows of `out`)
        xn = mlp(node_nn, x.index_select(0, sub.nodes))
        nm = None if node_mask is None else node_mask.reshape(-1).index_select(0, sub.nodes).view(-1, 1)
        o, g = global_attn_pool(xn.contiguous(), q.index_select(0, sub.gids), sub.plan, nm)
        out.index_copy_(0, sub.gids, o)
        gate.index_copy_(0, sub.nodes, g)
    return out, gate


def global_attn_pool(xn: Tensor, q: Tensor, plan: GraphPlan, node_mask: Optional[Tensor] = None):
    """GlobalAttention soft-max pooling (att_pooling.py:63-73).  Returns (out[B,C], gate[N,1])."""
    if _rec(xn, q, node_mask):
        from . import autograd
        return autograd.global_attn_pool(xn, q, plan, node_mask)
    lib = _lib.load()
    N, C = xn.shape
    out = torch.empty(plan.B, C, dtype=torch.float32, device=xn.device)
    gate = torch.empty(N, 1, dtype=torch.float32, device=xn.device)
    _lib.check(lib.isg_global_attn_pool(
        _chk(xn, "xn", torch.float32, (plan.N, C)), _chk(q, "q", torch.float32, (plan.B, C)), plan.ptr.data_ptr(),
        _chk(None if node_mask is None else node_mask.reshape(-1), "node_mask", torch.float32, (N,), optional=True),
        out.data_ptr(), gate.data_ptr(), plan.B, C, _stream()), "isg_global_attn_pool")
    return out, gate


# ------------------------------------------------------------------------------------------------
# Dense projections: fp32 accuracy on the bf16 matrix cores (csrc/isg_gemm.hip)
# ------------------------------------------------------------------------------------------------
_DERIVED = {}   # (tag, ids of the source tensors) -> ((weakref, version, data_ptr) per source, value, _Ready): tensors derived from parameters


def derived_weight(tag, sources, build):
    """Cache of tensors computed from static weights (kernel operand layouts, slices, concatenations): rebuilt when a source
    was updated in place (tensor._version / data_ptr) or replaced; invalidate_weight_cache() drops it."""
    key = (tag, id(sources[0])) if len(sources) == 1 else (tag, *map(id, sources))
    hit = _DERIVED.get(key)
    if hit is not None:
        # the weak references pin the identities: a freed weight's id (and even its address) can be reused by another model
        for (r, v, p), t in zip(hit[0], sources):
            if r() is not t or v != _ver(t) or p != t.data_ptr():
                break
        else:
            hit[2].wait()           # built on another stream a moment ago (run_split's two passes share this cache)?
            return hit[1]
    stamps = tuple((weakref.ref(t), _ver(t), t.data_ptr()) for t in sources)
    with torch.no_grad():
        value = build()
    if len(_DERIVED) > 256:
        for k in [k for k, v in _DERIVED.items() if any(r() is None for r, _, _ in v[0])]:
            del _DERIVED[k]
    _DERIVED[key] = (stamps, value, _Ready(any(t.is_cuda for t in sources)))
    return value


def gather_add(A: Tensor, ia: Tensor, B: Optional[Tensor] = None, ib: Optional[Tensor] = None, T: Optional[Tensor] = None,
               it: Optional[Tensor] = None, sign: Optional[Tensor] = None, D: Optional[Tensor] = None,
               bias: Optional[Tensor] = None, gelu: bool = False, planes_out: bool = False, csr_a=None, csr_b=None, csr_t=None,
               T2: Optional[Tensor] = None, sign2: Optional[Tensor] = None):
    """act(A[ia] + B[ib] + sign * T[it] + D + bias) -> [E, C]: the per-edge remainder of a Linear over
    cat([x[row], x[col], emb]) once its node parts are projected per node (scene_graph_encoder.py:119-120,139-140;
    csrc/isg_sgenc.hip).  A / B / T / D may be column slices of wider tensors (row stride a multiple of 4).
    planes_out: the rows as Planes32 only (the operand of the Linear that follows, no split pass, no fp32 rows).
    Under autograd through A, B, T, D or bias the call goes to autograd.gather_add (fp32 rows only: planes have no backward);
    csr_a / csr_b / csr_t: (rowptr, eid) of ia / ib / it where the caller has them (a plan's CSRs), else token_csr builds them.
    T2 / sign2 (autograd only): a second tensor with T's values that is only differentiated, under the factor sign2."""
    if T2 is not None and not _rec(T2):
        raise ValueError("gather_add: T2 is a tensor to differentiate; it takes no part in the value")
    if _rec(A, B, T, D, bias, T2):
        if planes_out:
            raise NotImplementedError("gather_add(planes_out=True) has no backward: an operand requires grad; ask for fp32 rows "
                                      "(planes_out=False), wrap the call in torch.no_grad() or detach the operands")
        if any(t is not None and t.requires_grad for t in (sign, sign2)):
            raise NotImplementedError("gather_add: sign has no gradient here; detach it")
        from . import autograd
        return autograd.gather_add(A, ia, B, ib, T, it, sign, D, bias, gelu, csr_a, csr_b, csr_t, T2, sign2)
    lib = _lib.load()
    E, C = ia.numel(), A.size(1)
    out = None if planes_out else torch.empty(E, C, dtype=torch.float32, device=A.device)
    pl = torch.empty(int(lib.isg_planes32_elems(E, C)), dtype=torch.int16, device=A.device) if planes_out else None
    pinv = torch.empty(E, dtype=torch.float32, device=A.device) if planes_out else None

    def rows(t, name):
        if t is None:
            return 0, 0
        if tuple(t.shape[1:]) != (C,):
            raise ValueError(f"{name}: expected [*, {C}], got {tuple(t.shape)}")
        return _chk_rows(t, name), t.stride(0)

    def idx(t, name, n):
        if t is None:
            return 0
        if t.numel() != n:
            raise ValueError(f"{name}: expected {n} indices, got {t.numel()}")
        return _chk(t.reshape(-1), name, torch.int64)

    pa, la = rows(A, "A")
    pb, lb = rows(B, "B")
    pt, lt = rows(T, "T")
    pd, ld = rows(D, "D")
    if D is not None and D.size(0) != E:
        raise ValueError(f"D: expected {E} rows, got {D.size(0)}")
    _lib.check(lib.isg_gather_add(pa, idx(ia, "ia", E), la, pb, idx(ib, "ib", E), lb, pt, idx(it, "it", E),
                                  _chk(None if sign is None else sign.reshape(-1), "sign", torch.float32, (E,), optional=True),
                                  lt, pd, ld, _chk(bias, "bias", torch.float32, (C,), optional=True),
                                  0 if out is None else out.data_ptr(), E, C, 1 if gelu else 0,
                                  0 if pl is None else pl.data_ptr(), 0 if pinv is None else pinv.data_ptr(), _stream()),
               "isg_gather_add")
    return Planes32(pl, pinv, E, C) if planes_out else out


def embedding_sum(weight: Tensor, idx: Tensor, padding_idx: Optional[int] = None) -> Tensor:
    """sum_t weight[idx[:, t]] -> [N, C]: torch.sum(embedding(idx), dim=-2) (scene_graph_encoder.py:63-70) without the [N, T, C]
    intermediate -- isg_gather_add adds up to three gathered rows (and a dense term) per launch, so four tokens are two launches
    over a table that sits in L2 (1.5 MB) instead of a 79 us gather x 2 and a 116 us reduction at 82 k nodes.  fp32, 4 | C;
    anything else: the torch ops.  (The sum runs ((t0 + t1) + t2) then + t3: equal to torch's to rounding.)
    padding_idx: the row that gets no gradient, as nn.Embedding(padding_idx=...) has it -- under autograd the call goes to
    autograd.embedding_sum (a segment sum over the tokens' CSR that skips that row), and the torch ops are told of it too."""
    if (not CFG.embedding_sum or weight.dtype != torch.float32 or idx.dim() != 2 or idx.size(1) < 2 or
            weight.size(1) % 4 != 0 or not weight.is_cuda or idx.dtype != torch.int64):
        return torch.sum(torch.nn.functional.embedding(idx, weight, padding_idx=padding_idx), dim=-2)
    if _rec(weight):
        from . import autograd
        return autograd.embedding_sum(weight, idx, padding_idx)
    w = weight.detach()
    cols = [idx[:, t].contiguous() for t in range(idx.size(1))]
    out, t = None, 0
    while t < len(cols):
        take = cols[t:t + 3] if out is None else cols[t:t + 2]
        args = [w, take[0]]
        args += [w, take[1]] if len(take) > 1 else [None, None]
        args += [w, take[2]] if len(take) > 2 else [None, None]
        out = gather_add(*args, None, out)
        t += len(take)
    return out


# ------------------------------------------------------------------------------------------------
# Training of the scene-graph encoder (include/isg_sgenc_train.h, csrc/isg_sgenc_bwd.hip)
# ------------------------------------------------------------------------------------------------
def token_csr(idx: Tensor, V: int) -> Tuple[Tensor, Tensor]:
    """(rowptr int32[V+1], eid int32[M]): for every token v in [0, V) the positions of `idx` (flattened) that hold it, in
    ascending position.  A stable sort and a bisection of the sorted values, no host read -- and NOT isg_csr_build, whose rank
    kernel compares every slot with its whole segment: fine for in-degrees bounded by a graph's size, 10^10 comparisons for a token
    that owns 10^5 entries.  Values outside [0, V) are the caller's error (their entries land in no segment's range)."""
    flat = idx.reshape(-1)
    if flat.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"token_csr: integer indices, got {flat.dtype}")
    if flat.numel() >= (1 << 31) - 1024 or V >= (1 << 31) - 1024:
        raise ValueError("token_csr: int32 positions")
    vals, order = torch.sort(flat, stable=True)
    rowptr = torch.searchsorted(vals, torch.arange(V + 1, dtype=vals.dtype, device=vals.device)).to(torch.int32)
    return rowptr, order.to(torch.int32)


def segment_rows_chunk() -> int:
    """Slots per piece of isg_segment_rows_sum."""
    from . import _lib_sgenc_train
    return int(_lib_sgenc_train.load().isg_segment_rows_chunk())


def segment_rows_sum(rowptr: Tensor, eid: Tensor, G: Tensor, w: Optional[Tensor] = None, gdiv: int = 1, skip: Optional[int] = None,
                     out: Optional[Tensor] = None, M: Optional[int] = None) -> Tensor:
    """out[s] = sum over t in [rowptr[s], rowptr[s+1]) of w[eid[t]] * G[eid[t] // gdiv]  -> [S, C]  (isg_segment_rows_sum: no
    atomics, the order of every sum a function of the CSR alone).  M: the number of entries where eid is longer than that (a
    plan's eid has one element for an edgeless batch).  out: fp32 [S, C] rows to write, e.g. a column slice of a wider tensor.
    skip: a segment written as zeros (padding_idx).  The entry ids are trusted like every index the forward kernels take."""
    from . import _lib_sgenc_train
    lib = _lib_sgenc_train.load()
    S = rowptr.numel() - 1
    M = eid.numel() if M is None else int(M)
    if S < 0 or M > eid.numel() or gdiv < 1:
        raise ValueError(f"segment_rows_sum: rowptr of {rowptr.numel()} entries, eid of {eid.numel()}, M = {M}, gdiv = {gdiv}")
    if G.dim() != 2:
        raise ValueError(f"segment_rows_sum: G is [rows, C], got {tuple(G.shape)}")
    C = G.size(1)
    if w is not None and w.numel() < M:
        raise ValueError(f"segment_rows_sum: w has {w.numel()} factors for {M} entries")
    if out is None:
        out = torch.empty(S, C, dtype=torch.float32, device=G.device)
    elif tuple(out.shape) != (S, C):
        raise ValueError(f"segment_rows_sum: out {tuple(out.shape)}, expected {(S, C)}")
    if S == 0:
        return out
    sk = -1 if skip is None else int(skip)
    if sk < -1:
        raise ValueError(f"segment_rows_sum: skip = {skip}")
    ws_bytes = int(lib.isg_segment_rows_ws_bytes(M, C))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=G.device)
    _lib.check(lib.isg_segment_rows_sum(_chk(rowptr, "rowptr", torch.int32), _chk(eid, "eid", torch.int32),
                                        _chk(None if w is None else w.reshape(-1), "w", torch.float32, optional=True),
                                        _chk_rows(G, "G"), G.stride(0), int(gdiv), _chk_rows(out, "out"), out.stride(0), S, M, C, sk,
                                        ws.data_ptr(), ws_bytes, _stream()), "isg_segment_rows_sum")
    return out


def gather_add_bwd(A: Tensor, ia: Tensor, B: Optional[Tensor], ib: Optional[Tensor], T: Optional[Tensor], it: Optional[Tensor],
                   sign: Optional[Tensor], D: Optional[Tensor], bias: Optional[Tensor], gelu: bool, grad_out: Tensor,
                   want_bias: bool = True):
    """(dz [E, C], d_bias [C] or None) of gather_add: the pre-activation is evaluated again from the operands (isg_gather_add_bwd);
    dz is the gradient of D, and segment_rows_sum of it over the CSRs of ia / ib / it gives those of A / B / T."""
    from . import _lib_sgenc_train
    lib = _lib_sgenc_train.load()
    E, C = ia.numel(), A.size(1)

    def rows(t, name, n=None):
        if t is None:
            return 0, 0
        if tuple(t.shape[1:]) != (C,) or (n is not None and t.size(0) != n):
            raise ValueError(f"{name}: expected [{'*' if n is None else n}, {C}], got {tuple(t.shape)}")
        return _chk_rows(t, name), t.stride(0)

    def idx(t, name):
        if t is None:
            return 0
        if t.numel() != E:
            raise ValueError(f"{name}: expected {E} indices, got {t.numel()}")
        return _chk(t.reshape(-1), name, torch.int64)

    pa, la = rows(A, "A")
    pb, lb = rows(B, "B")
    pt, lt = rows(T, "T")
    pd, ld = rows(D, "D", E)
    pg, lg = rows(grad_out, "grad_out", E)
    dz = torch.empty(E, C, dtype=torch.float32, device=A.device)
    parts = max(int(lib.isg_gather_add_bwd_parts(E)), 1)
    part = torch.zeros(parts, C, dtype=torch.float32, device=A.device) if want_bias else None
    _lib.check(lib.isg_gather_add_bwd(pa, idx(ia, "ia"), la, pb, idx(ib, "ib"), lb, pt, idx(it, "it"),
                                      _chk(None if sign is None else sign.reshape(-1), "sign", torch.float32, (E,), optional=True),
                                      lt, pd, ld, _chk(bias, "bias", torch.float32, (C,), optional=True), pg, lg, dz.data_ptr(), C,
                                      0 if part is None else part.data_ptr(), E, C, 1 if gelu else 0, _stream()),
               "isg_gather_add_bwd")
    return dz, (part.sum(0) if want_bias else None)


def scatter_mean_bwd(grad_out: Tensor, plan: GraphPlan) -> Tensor:
    """d_msg[e] = grad_out[dst[e]] / max(deg(dst[e]), 1) -> [E, C]: the backward of scatter_mean over the same plan."""
    from . import _lib_sgenc_train
    plan.require_csr()
    N, C = grad_out.shape
    if N != plan.N:
        raise ValueError(f"grad_out has {N} rows, plan has {plan.N} nodes")
    d_msg = torch.empty(plan.E, C, dtype=torch.float32, device=grad_out.device)
    _lib.check(_lib_sgenc_train.load().isg_scatter_mean_bwd(
        _chk_rows(grad_out, "grad_out"), grad_out.stride(0), _chk(plan.edge_index[1], "dst", torch.int64, (plan.E,)),
        plan.rowptr.data_ptr(), d_msg.data_ptr(), C, plan.N, plan.E, C, _stream()), "isg_scatter_mean_bwd")
    return d_msg


def graph_norm_bwd(x: Tensor, plan: GraphPlan, weight: Tensor, mean_scale: Tensor, eps: float, fp64: bool, grad_out: Tensor):
    """(d_x, d_weight, d_bias, d_mean_scale) of graph_norm in the same mode (isg_graph_norm_bwd): the per-graph partial rows of the
    three parameter gradients -- doubles with fp64 -- are summed here in graph order and rounded once."""
    from . import _lib_sgenc_train
    N, C = x.shape
    d_x = torch.empty(N, C, dtype=torch.float32, device=x.device)
    part = torch.zeros(max(plan.B, 1), 3, C, dtype=torch.float64 if fp64 else torch.float32, device=x.device)
    _lib.check(_lib_sgenc_train.load().isg_graph_norm_bwd(
        _chk(x, "x", torch.float32, (plan.N, C)), plan.ptr.data_ptr(), _chk(weight, "weight", torch.float32, (C,)),
        _chk(mean_scale, "mean_scale", torch.float32, (C,)), float(eps), 1 if fp64 else 0,
        _chk(grad_out, "grad_out", torch.float32, (N, C)), d_x.data_ptr(), part.data_ptr(), plan.B, C, _stream()),
        "isg_graph_norm_bwd")
    sums = part.sum(0).float()
    return d_x, sums[0], sums[1], sums[2]


_WEIGHTS_GENERATION = 0      # invalidate_weight_cache() counts up: part of every weights_stamp()


def invalidate_weight_cache() -> None:
    """Drop every cached derivative of a weight (split planes, fused weights) and make every StepCapture entry stale (each holds
    such derivatives inside its hipGraph; it is captured again at its next call).  The cache is validated by (object identity,
    tensor._version, data_ptr); a write THROUGH `.data` (weight.data.copy_/mul_, as init / EMA / weight-surgery code does) bumps
    neither, so such code must call this (Module.load_state_dict goes through copy_ on the Parameter and is safe)."""
    global _WEIGHTS_GENERATION
    _WEIGHTS_GENERATION += 1
    _DERIVED.clear()


class WeightsWatch:
    """Stamp of the weights of one or more modules, cheap enough to take before every captured call (StepCapture.run's `stamp`):
    two stamps are equal when nothing in between could have changed what a forward computes from the parameters and buffers.
    stamp() = (walk number, every tensor's _version, every tensor's data_ptr) -- what derived_weight() validates its cache by,
    so a captured and an eager forward notice the same events: an in-place write (optimizer.step(), p.add_(), load_state_dict's
    copy_, BatchNorm's running statistics) changes a version; `p.data = other` (Module.to(dtype) / .half(), weight swaps) an
    address; a Parameter or buffer OBJECT that was replaced is noticed by identity (the modules' own `_parameters` / `_buffers`
    dicts are read at every call) and invalidate_weight_cache() by its generation: both walk the module tree again, which starts
    a new walk number.  Host work only; the tree itself is walked once.  Timed with perf_counter loops on a CPU-only build host
    (not on the GPU host): 27-37 us per stamp() over the 147 tensors of ISubGVQA's question side before data_ptr was added
    (~0.2 us per tensor and attribute), against 330 us for list(Module.modules()) of the 251-module ISubGVQA alone.
    Blind spots, each answered by invalidate_weight_cache(): a WRITE through `.data` (p.data.mul_(): neither version, address nor
    identity moves -- derived_weight() cannot see it either), a submodule exchanged for another, a tensor registered on a
    module that had none when the tree was walked.  Tensors made under torch.inference_mode() have no version (_ver): identity
    and address stand for them."""
    _WALKS = 0

    def __init__(self, *modules):
        self.modules = modules
        self._generation = None

    def _walk(self) -> None:
        WeightsWatch._WALKS += 1
        self._generation, self._number = _WEIGHTS_GENERATION, WeightsWatch._WALKS
        seen, dicts = set(), []
        for root in self.modules:
            for m in root.modules():
                if id(m) not in seen:
                    seen.add(id(m))
                    dicts += [d for d in (m._parameters, m._buffers) if d]
        self._dicts = dicts
        self._tensors = [t for d in dicts for t in d.values()]          # (None for an absent bias: compared by identity too)
        self._present = [t for t in self._tensors if t is not None]
        self._versioned = [t for t in self._present if not t.is_inference()]

    def stamp(self):
        if self._generation != _WEIGHTS_GENERATION:
            self._walk()
        now = [t for d in self._dicts for t in d.values()]
        if len(now) != len(self._tensors) or not all(map(operator.is_, now, self._tensors)):
            self._walk()
        return (self._number, *map(_VERSION_OF, self._versioned), *map(_DATA_PTR_OF, self._present))


_VERSION_OF, _DATA_PTR_OF = operator.attrgetter("_version"), operator.methodcaller("data_ptr")


def _weight_planes(weight: Tensor, cache: bool = True, layout: str = "tile") -> Tensor:
    """The weight split into the operand layout of one GEMM kernel ("tile": isg_linear_bf16x6, "panel", "f16x3", "f16x3_rows"),
    once per weight version; cache=False (a weight being trained, or a temporary): split per call."""
    return derived_weight(("planes", layout), (weight,), lambda: _split_weight(weight, layout)) if cache else \
        _split_weight(weight, layout)


def _split_weight(weight: Tensor, layout: str):
    lib = _lib.load()
    N, K = weight.shape
    w = weight.detach()
    if layout == "f16x3_rows":  # row-major scaled fp16 planes of isg_linear_f16x3_tile
        Kp = (K + 31) // 32 * 32
        planes = torch.empty(2 * N * Kp, dtype=torch.int16, device=weight.device)
        inv = torch.empty(N, dtype=torch.float32, device=weight.device)
        _lib.check(lib.isg_split_f16x2_rows(_chk(w.contiguous(), "weight", torch.float32), N, K, planes.data_ptr(),
                                            inv.data_ptr(), _stream()), "isg_split_f16x2_rows")
        planes = (planes, inv)
    elif layout == "f16x3":      # two scaled fp16 planes + the inverse row scales of isg_linear_f16x3
        planes = torch.empty(int(lib.isg_split_f16x2_frag_elems(N, K)), dtype=torch.int16, device=weight.device)
        inv = torch.empty((N + 31) // 32 * 32, dtype=torch.float32, device=weight.device)
        _lib.check(lib.isg_split_f16x2_frag(_chk(w.contiguous(), "weight", torch.float32), N, K, planes.data_ptr(),
                                            inv.data_ptr(), _stream()), "isg_split_f16x2_frag")
        planes = (planes, inv)
    elif layout == "panel":      # fragment-major planes of isg_linear_panel
        planes = torch.empty(int(lib.isg_split_bf16x3_frag_elems(N, K)), dtype=torch.int16, device=weight.device)
        _lib.check(lib.isg_split_bf16x3_frag(_chk(w.contiguous(), "weight", torch.float32), N, K, planes.data_ptr(),
                                             _stream()), "isg_split_bf16x3_frag")
    else:
        Kp = (K + 31) // 32 * 32
        planes = torch.empty(3 * N * Kp, dtype=torch.int16, device=weight.device)
        _lib.check(lib.isg_split_bf16x3(_chk(w.contiguous(), "weight", torch.float32), N, K, planes.data_ptr(), _stream()),
                   "isg_split_bf16x3")
    return planes


def _stamp(x: Tensor):
    """What a value attached to an activation is valid for: x's version, storage and shape (an in-place write invalidates it)."""
    return (_ver(x), x.data_ptr(), tuple(x.shape))


def _from_tensor(t: Tensor, value) -> tuple:
    """A cache entry for a value made from this very tensor (a plan's edge planes, the edge rows of its oversize graphs): valid
    while `t` is the same object -- a weak reference, since the id of a freed tensor can be reused -- with the same version,
    storage and shape."""
    return (weakref.ref(t), _stamp(t), value)


def _if_from_tensor(entry: Optional[tuple], t: Tensor):
    """The value of a _make_from entry if it was made from `t` as it is now, else None."""
    return entry[2] if entry is not None and entry[0]() is t and entry[1] == _stamp(t) else None


def _attach(x: Tensor, name: str, value) -> None:
    setattr(x, name, (_stamp(x), value))


def _attached(x: Tensor, name: str):
    hit = getattr(x, name, None)
    return hit[1] if hit is not None and hit[0] == _stamp(x) else None


def attach_row_maxima(x: Tensor, rowmax: Tensor) -> Tensor:
    """Leave partial row maxima [M, P] (max |x| over P equal column blocks of every row) on `x` for the fp16 three-product
    Linears that read it.  They are tied to x's version counter: an in-place write to x afterwards invalidates them
    (`row_maxima` then returns None and the Linear makes its own pass) -- a stale maximum would mis-scale the fp16 planes."""
    _attach(x, "_isg_rowmax", rowmax)
    return x


def row_maxima(x: Tensor) -> Optional[Tensor]:
    return _attached(x, "_isg_rowmax")


def attach_dead_rows(x: Tensor, row_dead: Tensor) -> Tensor:
    """Leave on `x` (the output of a masked gatv2_layer_conv launch) the uint8 flags [N, H] of the (row, head) pairs whose
    accumulators stayed all-zero bits: rows with every flag set are `+0 + bias`, one and the same vector.  Tied to x's version
    like the row maxima."""
    _attach(x, "_isg_row_dead", row_dead)
    return x


def dead_rows(x: Tensor) -> Optional[Tensor]:
    return _attached(x, "_isg_row_dead")


def is_sparse_conv_out(x: Tensor) -> bool:
    """Did a sparse gatv2_layer_conv launch leave `x`?  (The marker is tied to x's version like the flags it goes with.)"""
    hit = getattr(x, "_isg_sparse_out", None)
    return hit is not None and hit[0] == _stamp(x) and dead_rows(x) is not None


def dense_conv_out(x: Tensor) -> Tensor:
    """`x` itself unless a sparse gatv2_layer_conv launch left it (sparse_out=True); then a tensor with every row: the rows whose
    flags are set in every head -- of which the launch wrote one per tile -- are `0 + bias`, their maxima that vector's per head,
    which is what a dense launch writes there bit for bit.  The result carries its maxima and flags and no marker."""
    if not is_sparse_conv_out(x):
        return x
    bias, dead, rm = x._isg_sparse_out[1], dead_rows(x), row_maxima(x)
    H = dead.size(1)
    const = torch.zeros(x.size(1), dtype=x.dtype, device=x.device)
    if bias is not None:
        const = const + bias.reshape(-1).to(x.dtype)         # an addition, as in the kernel: +0 + -0 = +0
    flagged = (dead != 0).all(dim=1, keepdim=True)
    full = torch.where(flagged, const.unsqueeze(0), x)
    if rm is not None:
        attach_row_maxima(full, torch.where(flagged, const.view(H, -1).abs().amax(dim=1).unsqueeze(0), rm))
    return attach_dead_rows(full, dead)


_CUS = {}


_DT_DENSE_ROWS = None


def dense_tail_dense_rows() -> bool:
    """ISG_DT_DENSE_ROWS=1 as isg_mgat_dense_tail reads it (once per process): x_proj over every row whatever the flags say."""
    global _DT_DENSE_ROWS
    if _DT_DENSE_ROWS is None:
        e = os.environ.get("ISG_DT_DENSE_ROWS", "")
        try:
            _DT_DENSE_ROWS = int(e.strip() or 0) != 0
        except ValueError:
            _DT_DENSE_ROWS = False                   # atoi of a word is 0
    return _DT_DENSE_ROWS


def sparse_conv_out_rule(masked: bool, tail_supported: bool, explainer: bool, dense_rows: bool, conv: str) -> bool:
    """May a layer's convolution leave the rows without a live in-slot unwritten (gatv2_layer_conv sparse_out)?  Only when the one
    reader of its result is mgat_dense_tail's live-row form: a masked layer whose fused tail will run, outside the explainer,
    without ISG_DT_DENSE_ROWS, on the layer_conv route.  Pure: MGAT.forward asks it once per layer."""
    return bool(masked and tail_supported and not explainer and not dense_rows and conv == "layer_conv")


def dense_tail_group(N: int, E: int, device) -> int:
    """Tiles per workgroup of the dense tail's live-row form: as many as make the launch ONE round of workgroups at two per CU,
    at most 4.  The tile count stays on the device; N / 64 and E / 256 (what fills a tile) bound it from below and are within
    a fifth of it on the batches the tile kernels take (BASELINE configs[1]: 1 286 against 1 514 tiles -> 3)."""
    idx = torch.device(device).index or 0
    if idx not in _CUS:
        _CUS[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    est = max(-(-N // TILE_CONV_NODES), -(-E // TILE_CONV_EDGES), 1)
    return max(1, min(4, -(-est // (2 * _CUS[idx]))))


def carry_row_maxima(dst: Tensor, src: Tensor) -> Tensor:
    """`dst` is a row-order-preserving view / reshape of `src` (same rows, same values): it keeps src's maxima, and src's
    planes32 (what a Linear on the engine would otherwise split again)."""
    rm = row_maxima(src)
    if rm is not None and dst.dim() >= 1:
        attach_row_maxima(dst, rm)
    pl = _attached(src, "_isg_planes32")
    if pl is not None and dst.data_ptr() == src.data_ptr() and dst.numel() == src.numel():
        _attach(dst, "_isg_planes32", pl)
    return dst


def add_layernorm(x: Tensor, residual: Optional[Tensor], norm: torch.nn.LayerNorm, want_rowmax: bool = True) -> Tensor:
    """LayerNorm(x + residual) over the last dimension in one launch (csrc/isg_attn.hip::add_layernorm_kernel), the
    result carrying its row maxima for the next Linear.  x / residual: fp32 [M, D] rows."""
    lib = _lib.load()
    M, D = x.shape
    if residual is not None and tuple(residual.shape) != (M, D):
        raise ValueError(f"add_layernorm: x {tuple(x.shape)} vs residual {tuple(residual.shape)}")
    if tuple(norm.normalized_shape) != (D,) or norm.weight is None:
        raise ValueError("add_layernorm: an affine LayerNorm over the last dimension")
    out = torch.empty(M, D, dtype=torch.float32, device=x.device)
    rm = torch.empty(M, 1, dtype=torch.float32, device=x.device) if want_rowmax else None
    # the consumers of a LayerNorm result are Linears: where they run on the planes32 engine the kernel writes the planes too
    pl = None
    if CFG.ln_planes and CFG.h3p and D % 32 == 0 and D >= CFG.h3p_min_k and M >= CFG.h3p_min_m:
        pl = Planes32(torch.empty(M * D * 2, dtype=torch.int16, device=x.device),
                      torch.empty(M, dtype=torch.float32, device=x.device), M, D)
    rc = lib.isg_add_layernorm(_chk_rows(x, "x"), x.stride(0), 0 if residual is None else _chk_rows(residual, "residual"),
                               0 if residual is None else residual.stride(0),
                               _chk(norm.weight.detach(), "weight", torch.float32, (D,)),
                               _chk(None if norm.bias is None else norm.bias.detach(), "bias", torch.float32, (D,), optional=True),
                               float(norm.eps), out.data_ptr(), D, 0 if rm is None else rm.data_ptr(), M, D,
                               0 if pl is None else pl.planes.data_ptr(), 0 if pl is None else pl.inv.data_ptr(), _stream())
    if rc == ISG_EUNSUPPORTED:
        COUNTERS["torch_layer_norm"] += 1
        y = x if residual is None else x + residual
        return torch.nn.functional.layer_norm(y, norm.normalized_shape, norm.weight, norm.bias, norm.eps)
    _lib.check(rc, "isg_add_layernorm")
    if rm is not None:
        attach_row_maxima(out, rm)
    if pl is not None:
        _attach(out, "_isg_planes32", pl)       # what split_planes32(out) would make
    return out


def _linear_torch(x: Tensor, weight: Tensor, bias: Optional[Tensor], gelu: bool, relu: bool) -> Tensor:
    COUNTERS["torch_linear"] += 1
    y = torch.nn.functional.linear(x, weight, bias)
    return torch.relu(y) if relu else (torch.nn.functional.gelu(y) if gelu else y)


def reads_planes32(M: int, N: int, K: int, cfg: Optional[Switches] = None) -> bool:
    """Does a Linear of shape (M, N, K) read a planes32 operand on the engine (isg_linear_h3p)?  A producer that can write its
    result as planes32 (the attention and gate kernels, gather_add, a chained Linear) asks this before it does."""
    cfg = CFG if cfg is None else cfg
    return (cfg.h3p and cfg.gemm_backend == "bf16x6" and cfg.gemm_kernel == "auto" and cfg.gemm_f16x3 and K >= cfg.h3p_min_k and
            (K & 3) == 0 and (N & 3) == 0 and M >= cfg.h3p_min_m and M * ((K + 31) // 32) * 128 < (1 << 31) and
            N * ((K + 31) // 32) * 128 < (1 << 31)
            and M * ((N + 31) // 32 * 32) * 4 < (1 << 32) - 16)       # the result through a buffer descriptor: 32-bit byte offsets


def _k_chunks(K: int):
    """isg_linear_f16x3_tile's reduction as chains of at most 640 (2.75x an fp32 GEMM's error at 1024-long chains, < 2x here):
    (number of chunks, columns per chunk)."""
    nchunk = (K + 639) // 640
    return nchunk, ((K + nchunk - 1) // nchunk + 31) // 32 * 32


def _usable_rowmax(x: Tensor, M: int) -> Optional[Tensor]:
    rm = row_maxima(x)
    return None if rm is None or rm.dim() != 2 or rm.size(0) != M or rm.size(1) > 64 or rm.stride(1) != 1 else rm


def _rowmax_slices(K: int, P: int) -> bool:
    """Do the producer's maxima over P column blocks of a row serve every K-chunk (each covers whole columns of ONE chunk)?"""
    nchunk, step = _k_chunks(K)
    per = K // P if P > 0 and K % P == 0 else 0
    return P > 0 and (nchunk == 1 or (per > 0 and step % per == 0))       # one chunk: any partition of the row serves


def _use_panel(M: int, N: int, K: int, cfg: Optional[Switches] = None) -> bool:
    """linear_route's panel rule: an A panel split once serves many columns (K <= 128: lin_edge 182 vs 212 us, lin_l|lin_r 153
    vs 166 us) with enough 64-row panels to fill the chip; the tile kernels elsewhere (profiles/r02_a_gemm_structures.md)."""
    cfg = CFG if cfg is None else cfg
    if cfg.gemm_kernel != "auto":
        return cfg.gemm_kernel == "panel"
    return K <= 128 and N >= cfg.panel_min_n and M >= 32768


def linear_route(M: int, N: int, K: int, x_dtype=torch.float32, out_dtype=torch.float32, relu: bool = False,
                 recording: bool = False, planes32: bool = False, carries_planes: bool = False, rowmax_slices: bool = False,
                 aligned: bool = True, skinny_layout: bool = True, cfg: Optional[Switches] = None) -> str:
    """The kernel ops.linear runs act(x @ W^T + b) on for x [M, K], W [N, K]: a pure function of plain values.

    recording: autograd records through x, W or b; planes32: x IS a Planes32; carries_planes: x's producer left its planes32 on
    it; rowmax_slices: x carries partial row maxima that serve every K-chunk of isg_linear_f16x3_tile; aligned: x has contiguous
    columns, a row stride of 4 | ld and 16-byte alignment; skinny_layout=False: isg_linear_skinny refused the operands' layout.
    Under the default switches, fp32 rows, inference, the first match of:
      M == 0                                                         "empty"
      K % 4 != 0                                                     "torch" (hipBLASLt)
      M <= 1024, M N K <= 2^30                                       "skinny"
      K >= 256, 4 | N, M >= 8192 (2048 if the producer left planes32) "h3p"
      K > 128, the producer's row maxima slice the row, or N >= 256 and M >= 4096
                                                                     "f16x3_tile"
      K <= 128, N >= 256, M >= 32768, no ReLU                        "f16x3" ("f16x3_f16": fp16 result)
      anything else                                                  "bf16x6" ("bf16x6_f16": fp16 rows in or out)
    A Planes32 meets "h3p"; ReLU under autograd "torch", anything else under autograd "autograd"."""
    cfg = CFG if cfg is None else cfg
    if planes32:
        return "h3p"
    f16_io = x_dtype == torch.float16 or out_dtype == torch.float16
    ours = cfg.gemm_backend == "bf16x6" and (K & 3) == 0
    if relu and (recording or not ours or M == 0):
        return "torch"
    if not ours or M == 0:
        return "empty" if M == 0 else "torch"
    if recording:
        return "autograd"
    if (skinny_layout and cfg.skinny and cfg.gemm_kernel == "auto" and M <= cfg.skinny_max_m and M * N * K <= cfg.skinny_max_work
            and not f16_io and x_dtype == torch.float32):
        return "skinny"      # the latency-bound regime: the HOST's time per call is what the forward costs
    if not f16_io and aligned and (M >= cfg.h3p_min_m_unsplit or carries_planes) and reads_planes32(M, N, K, cfg):
        # below h3p_min_m_unsplit rows only an input whose PRODUCER left its planes (isg_add_layernorm, the attention kernels,
        # the gates): an isolated Linear there would pay a split pass of its own and loses to the tile kernels
        return "h3p"
    if (cfg.gemm_f16x3 and cfg.f16x3_tile and cfg.gemm_kernel == "auto" and K > 128 and not f16_io and M < (1 << 23) and
            (rowmax_slices or (N >= 256 and M >= 4096))):   # a pass over x for the row maxima only pays for wide Linears over many rows
        return "f16x3_tile"
    if not relu and _use_panel(M, N, K, cfg):
        if cfg.gemm_f16x3 and K <= 128 and cfg.f16x3_f16_out and x_dtype == torch.float32 and out_dtype == torch.float16:
            return "f16x3_f16"
        return "f16x3" if cfg.gemm_f16x3 and K <= 128 and not f16_io else "panel"
    return "bf16x6_f16" if f16_io else "bf16x6"


class ConvRoute(NamedTuple):
    """How one MaskingGATv2Conv layer runs (conv_route)."""
    conv: str          # "layer_conv" | "tile_conv" | "pair" | "unfused": the kernels of the message passing
    gate: str          # "planes" | "planes32" | "rows" | "none": what gelu(x * instruction[batch]) is written as when the layer gates itself
    gate_rows: bool    # the layer reads fp32 ROWS of its gated input (beside, or instead of, the planes)
    e_proj: bool       # lin_edge runs as a Linear: the kernel reads e_proj [E, H*C] from memory


def conv_route(*, heads: int, channels: int, in_channels: int, edge_dim: Optional[int], N: int, B: int, E: int, nmax: int,
               has_csr: bool, tile_mode: str, rows_dtype=torch.float32, share_weights: bool = False,
               use_instr: bool = True, masked: bool = False, gate_on_planes: bool = False, grad: bool = False,
               e_proj_given: bool = False, has_edge_lin: bool = True, cfg: Optional[Switches] = None,
               attn_dropout: bool = False, concat_instr: bool = False) -> ConvRoute:
    """How a MaskingGATv2Conv layer (in_channels -> heads x channels, edge features edge_dim wide) runs on a batch of B graphs, N
    nodes (at most nmax per graph) and E edges: a pure function of plain values, the ONE place that decides.

    edge_dim: None without 2-D edge features; has_csr: the plan holds the CSR by destination; tile_mode: GraphPlan.tile_mode of the
    64-node / 256-slot tiles; rows_dtype: MaskingGATv2Conv.rows_dtype(plan); masked: the layer has a node gate (masking_threshold
    != 1), gate_on_planes: which can run on the input's planes (MaskingModel.planes_ready); grad: autograd is recording;
    e_proj_given: the caller hands e_proj in; has_edge_lin: the layer has a lin_edge; attn_dropout: the layer drops attention
    weights on this call (self.training and self.dropout > 0, under no_grad too) -- only the un-fused message-passing kernels
    have a dropout form (include/isg_mp_train.h), so it selects "unfused" as autograd does and a fused kernel never skips it.
    conv, the first match of (under the default switches):
      e_proj given, no edge features or lin_edge, autograd, attn_dropout     "unfused"  lin_edge as a Linear + the message-passing kernel
      4 !| C, H ceil32(C) > 2048, K = 0, K > 304, 4 !| K, nothing to do (B, E, nmax = 0), no CSR,
        or a wide layer (32 !| C or K > 128) under 16 384 edges              "unfused"
      fp16 rows                                                              "pair" when K >= 128, else "unfused"
      other half rows                                                        "unfused"
      the next rule's shape, lin_l and lin_r distinct, in_channels = 128,    "layer_conv"  lin_l | lin_r, lin_edge, logits, softmax and
        H <= 16                                                                            aggregation as one persistent launch on tiles
      C = 128, K <= 128, H <= 64, tile_mode not "none"                       "tile_conv"   the same with x_l / x_r projected before it
      anything else                                                          "pair"        lin_edge folded into the logits, softmax +
                                                                                           aggregation from them (per-graph kernel)
    gate, the first match of:
      no instruction gate                                                    "none"
      conv is "layer_conv"                                                   "planes"    ops.NodePlanes (+ fp32 rows if gate_rows)
      inference, fp32 rows, the lin_l | lin_r projection reads planes32      "planes32"  its operand (+ fp32 rows for a node gate)
      anything else                                                          "rows"
    gate_rows: everything but "layer_conv" reads rows, and so does a node gate that cannot run on the planes.  e_proj: conv is
    "unfused" (a stack of layers then projects every layer's edge rows in one launch).
    concat_instr: the layer reads cat(x, instruction[batch]) instead of the gated rows (in_channels is then its TRUE input
    width, 2 x the node rows' -- at C = 64 that is 128 and still no layer_conv shape).  It never gates ("none"), projects lin_l |
    lin_r ahead of the message passing on the row-biased Linear (ops.linear_rowbias) and so reads rows; the graph-tile kernels
    have no such projection: conv is "unfused" by the first two rules, on half rows as above, and "pair" otherwise."""
    cfg = CFG if cfg is None else cfg
    if concat_instr:
        if e_proj_given or edge_dim is None or not has_edge_lin or grad or attn_dropout:
            conv = "unfused"
        elif not _fused_logits_ok(heads, channels, edge_dim, B, E, nmax, has_csr, cfg):
            conv = "unfused"
        elif rows_dtype != torch.float32:
            conv = "pair" if rows_dtype == torch.float16 and edge_dim >= 128 else "unfused"
        else:
            conv = "pair"
        return ConvRoute(conv, "none", True, conv == "unfused")
    if e_proj_given or edge_dim is None or not has_edge_lin or grad or attn_dropout:
        conv = "unfused"
    elif not _fused_logits_ok(heads, channels, edge_dim, B, E, nmax, has_csr, cfg):
        conv = "unfused"
    elif rows_dtype != torch.float32:
        # fp16 feature rows (BASELINE configs[4]): the pair exists on the rows kernel (K >= 128), the tile kernels do not
        conv = "pair" if rows_dtype == torch.float16 and edge_dim >= 128 else "unfused"
    elif not share_weights and _layer_conv_ok(heads, channels, in_channels, edge_dim, B, E, has_csr, tile_mode, cfg):
        conv = "layer_conv"
    elif _tile_conv_ok(heads, channels, edge_dim, B, E, has_csr, tile_mode, cfg):
        conv = "tile_conv"
    else:
        conv = "pair"
    if not use_instr:
        gate = "none"
    elif conv == "layer_conv":
        gate = "planes"
    elif (not grad and rows_dtype == torch.float32 and
          reads_planes32(N, (1 if share_weights else 2) * heads * channels, in_channels, cfg)):
        gate = "planes32"
    else:
        gate = "rows"
    return ConvRoute(conv, gate, conv != "layer_conv" or (masked and not gate_on_planes), conv == "unfused")


_ROUTES = {}   # facts of an ops.linear call -> (the CFG they were decided under, route or None, which input facts decide it)
_INPUT_FACTS = [(c, s, a) for c in (False, True) for s in (False, True) for a in (False, True)]


def _route(x: Tensor, M: int, N: int, K: int, out_dtype, relu: bool, rec: bool, skinny_layout: bool = True) -> str:
    """linear_route, memoised.  Of x's attachments and layout (planes32, row maxima, alignment) only the facts the shape's route
    depends on are looked at (host time: a one-question forward is ~75 Linears)."""
    cfg = CFG
    key = (M, N, K, x.dtype, out_dtype, relu, rec, skinny_layout)
    hit = _ROUTES.get(key)
    if hit is None or hit[0] is not cfg:
        if len(_ROUTES) > 4096:
            _ROUTES.clear()
        r = {f: linear_route(M, N, K, x.dtype, out_dtype, relu, rec, False, *f, skinny_layout, cfg) for f in _INPUT_FACTS}
        need = tuple(any(r[f] != r[f[:i] + (not f[i],) + f[i + 1:]] for f in _INPUT_FACTS) for i in range(3))
        hit = _ROUTES[key] = (cfg, None if any(need) else r[_INPUT_FACTS[0]], need)
    if hit[1] is not None:
        return hit[1]
    need, rm = hit[2], (_usable_rowmax(x, M) if hit[2][1] else None)       # a fact no route depends on keeps any value
    key += (need[0] and has_planes32(x), rm is not None and _rowmax_slices(K, rm.size(1)),
            need[2] and x.stride(1) == 1 and (x.stride(0) & 3) == 0 and (x.data_ptr() & 15) == 0)
    hit = _ROUTES.get(key)
    if hit is None or hit[0] is not cfg:
        hit = _ROUTES[key] = (cfg, linear_route(M, N, K, x.dtype, out_dtype, relu, rec, False, *key[8:], skinny_layout, cfg))
    return hit[1]


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, gelu: bool = False,
           cache_planes: bool = True, out_dtype=torch.float32, relu: bool = False, want_rowmax: bool = False) -> Tensor:
    """act(x @ weight^T + bias), x [M,K] fp32 (fp16 rows, a Planes32), weight [N,K] (torch Linear layout), on the kernel
    linear_route chooses.  ``cache_planes=False``: the weight is being trained (or is a temporary), so its planes are split per
    call instead of cached.  ``want_rowmax``: isg_linear_f16x3_tile leaves the result's row maxima on it."""
    if relu and gelu:
        raise ValueError("relu excludes gelu")
    if isinstance(x, Planes32):                    # the producer handed the rows over pre-split (a Linear's planes output)
        route = linear_route(x.rows, weight.size(0), x.cols, planes32=True)
    else:
        M, K = x.shape
        rec = torch.is_grad_enabled() and _rec(x, weight, bias)
        if x.dtype == torch.float16 or out_dtype == torch.float16:
            if CFG.gemm_backend != "bf16x6" or (K & 3) != 0 or rec:
                raise _lib.IsgError("fp16 feature rows are an inference feature of the bf16x6 kernel (K % 4 == 0, no autograd)")
            if relu:
                raise ValueError("relu excludes fp16 rows")
        N = weight.size(0)
        hit = _ROUTES.get((M, N, K, x.dtype, out_dtype, relu, rec, True))      # _route's common case inline (host time)
        route = hit[1] if hit is not None and hit[0] is CFG and hit[1] is not None else _route(x, M, N, K, out_dtype, relu, rec)
        if route == "skinny":
            y = linear_skinny(x, weight, bias, gelu=gelu, relu=relu)
            if y is not None:
                return y
            route = _route(x, M, N, K, out_dtype, relu, rec, skinny_layout=False)      # a layout it cannot take
    return _launch(route, x, weight, bias, gelu, relu, cache_planes, out_dtype, want_rowmax)


def _launch(route: str, x, weight: Tensor, bias: Optional[Tensor], gelu: bool, relu: bool, cache_planes: bool, out_dtype,
            want_rowmax: bool):
    """One launcher per route but "skinny" (ops.linear runs isg_linear_skinny itself, and takes the route without it where the
    kernel refuses the operands' layout).  A shape a kernel has no launch for (more than 65535 row tiles) goes to hipBLASLt."""
    if route == "h3p":
        return linear_h3p(x, weight, bias, gelu=gelu, relu=relu, cache_planes=cache_planes)
    if route == "torch":
        return _linear_torch(x, weight, bias, gelu, relu)
    if route == "empty":
        return x.new_empty(0, weight.size(0))
    if route == "autograd":
        from . import autograd
        return autograd.linear(x, weight, bias, gelu)
    lib, (M, K), N = _lib.load(), x.shape, weight.size(0)
    out = torch.empty(M, N, dtype=out_dtype, device=x.device)
    if route == "f16x3_tile":
        return _linear_f16x3_tile(lib, x, weight, bias, gelu, relu, cache_planes, out, want_rowmax, M, N, K)
    if route in ("f16x3", "f16x3_f16"):        # fp32 rows in; fp32 out, or half rows (configs[4]'s x_l | x_r) rounded once
        planes, inv = _weight_planes(weight, cache_planes, "f16x3")
        name = "isg_linear_" + route
        _lib.check(getattr(lib, name)(_chk(x, "x", torch.float32), planes.data_ptr(), inv.data_ptr(), _bias_ptr(bias, N),
                                      out.data_ptr(), M, N, K, K, N, 1 if gelu else 0, N, 0, _stream()), name)
        return out
    planes = _weight_planes(weight, cache_planes, "panel" if route == "panel" else "tile")
    if route == "bf16x6":
        rc = lib.isg_linear_bf16x6(_chk(x, "x", torch.float32), planes.data_ptr(), _bias_ptr(bias, N), out.data_ptr(), M, N, K,
                                   K, N, 2 if relu else (1 if gelu else 0), _stream())
        if rc == ISG_EUNSUPPORTED:
            return _linear_torch(x, weight, bias, gelu, relu)
        _lib.check(rc, "isg_linear_bf16x6")
        return out
    name = "isg_linear_panel" if route == "panel" else "isg_linear_bf16x6_f16"
    _lib.check(getattr(lib, name)(_chk(x, "x", x.dtype), 1 if x.dtype == torch.float16 else 0, planes.data_ptr(), _bias_ptr(bias, N),
                                  out.data_ptr(), 1 if out_dtype == torch.float16 else 0, M, N, K, K, N, 1 if gelu else 0,
                                  _stream()), name)
    return out


def _bias_ptr(bias: Optional[Tensor], N: int) -> int:
    return _chk(None if bias is None else bias.detach(), "bias", torch.float32, (N,), optional=True)


def _linear_f16x3_tile(lib, x: Tensor, weight: Tensor, bias, gelu: bool, relu: bool, cache_planes: bool, out: Tensor,
                       want_rowmax: bool, M: int, N: int, K: int) -> Tensor:
    """fp16 three-product tile kernel.  Row scales: the producer's partial maxima (a chunk takes the slice that covers its
    columns), or one pass over x which is then left on x for its other consumers; reductions longer than 640 run as K-chunks
    that accumulate into `out` (every chunk its own fp32 chain and its own row scales)."""
    a_rowmax = _usable_rowmax(x, M)
    P = a_rowmax.size(1) if a_rowmax is not None else 0
    nchunk, step = _k_chunks(K)
    sliced = _rowmax_slices(K, P)
    per = K // P if sliced and K % P == 0 else 0
    planes, inv = _weight_planes(weight, cache_planes, "f16x3_rows")
    act = 2 if relu else (1 if gelu else 0)
    bptr = _bias_ptr(bias, N)
    d_rowmax = torch.empty(M, (N + 31) // 32, dtype=torch.float32, device=x.device) if want_rowmax else None
    xp = _chk(x, "x", torch.float32)
    k0, c = 0, 0
    while k0 < K:
        kc = min(step, K - k0)
        last = k0 + kc >= K
        if sliced and nchunk == 1:
            rm_ptr, rm_p, rm_ld = a_rowmax.data_ptr(), P, a_rowmax.stride(0)
        elif sliced:
            rm_ptr, rm_p, rm_ld = a_rowmax.data_ptr() + 4 * (k0 // per), (kc + per - 1) // per, a_rowmax.stride(0)
        else:
            rm = torch.empty(M, 1, dtype=torch.float32, device=x.device)
            _lib.check(lib.isg_row_absmax(xp + 4 * k0, M, kc, K, rm.data_ptr(), _stream()), "isg_row_absmax")
            COUNTERS["row_absmax"] += 1
            if nchunk == 1:
                attach_row_maxima(x, rm)          # the next Linear over the same rows does not repeat the pass
            rm_ptr, rm_p, rm_ld = rm.data_ptr(), 1, 1
        rc = lib.isg_linear_f16x3_tile(
            xp + 4 * k0, rm_ptr, rm_p, rm_ld, planes.data_ptr(), inv.data_ptr(), bptr if last else 0,
            out.data_ptr(), d_rowmax.data_ptr() if (last and d_rowmax is not None) else 0, M, N, kc, K, N,
            act if last else 0, K, k0, 1 if c > 0 else 0, _stream())
        if rc == ISG_EUNSUPPORTED and c == 0:       # a shape the kernel has no launch for (> 65535 row tiles): hipBLASLt
            return _linear_torch(x, weight, bias, gelu, relu)
        _lib.check(rc, "isg_linear_f16x3_tile")
        k0 += kc
        c += 1
    if d_rowmax is not None:
        attach_row_maxima(out, d_rowmax)
    return out


# ------------------------------------------------------------------------------------------------
# The K >= 256 engine (csrc/isg_gemm_h3p.hip): both operands pre-split ("planes32"), LDS-DMA operand path
# ------------------------------------------------------------------------------------------------
class Planes32(NamedTuple):
    """An activation as the fp16 three-product GEMM reads it: planes [rows * ceil(cols / 32) * 64] int16 (row r, k-tile kt =
    one 128-byte line [hi 32 | mid 32] of the row scaled by its own power of two), inv [rows] = 1 / scale."""
    planes: Tensor
    inv: Tensor
    rows: int
    cols: int
    # SEGMENTED (isg_gatv2_mp_fwd_planes): columns [0, seg_cols) of a row under inv_first, the rest under inv; each segment padded
    # to whole 32-column lines, so the planes hold 2 * ceil(seg_cols / 32) lines per row and the weight is laid out to match
    inv_first: Optional[Tensor] = None
    seg_cols: int = 0


def has_planes32(x: Tensor) -> bool:
    """Did x's producer leave its planes32 (still valid for x's current version)?"""
    return _attached(x, "_isg_planes32") is not None


def split_planes32(x: Tensor) -> Planes32:
    """fp32 rows [M, K] -> planes32 (exact row maxima).  The planes stay attached to `x` (tied to its version counter, like
    the row maxima): a second Linear over the same rows (the decoder layers' cross-attention over the encoder memory) does
    not repeat the pass."""
    hit = _attached(x, "_isg_planes32")
    if hit is not None:
        return hit
    lib = _lib.load()
    M, K = x.shape
    planes = torch.empty(int(lib.isg_planes32_elems(M, K)), dtype=torch.int16, device=x.device)
    inv = torch.empty(M, dtype=torch.float32, device=x.device)
    _lib.check(lib.isg_split_planes32(_chk_rows(x, "x"), M, K, x.stride(0), planes.data_ptr(), inv.data_ptr(), _stream()),
               "isg_split_planes32")
    out = Planes32(planes, inv, M, K)
    _attach(x, "_isg_planes32", out)
    return out


def instr_gate_planes32(x: Tensor, instr: Tensor, batch: Tensor, want_rows: bool = False):
    """gelu(x * instr[batch]) (mgat_v2_conv.py:156-157) as Planes32 for the lin_l | lin_r projection on the engine, plus the fp32
    rows when a masked layer's node gate needs them (they then carry the planes: a Linear over them splits nothing).
    Returns (rows or None, Planes32).  Inference only."""
    lib = _lib.load()
    N, C = x.shape
    rows = torch.empty_like(x) if want_rows else None
    planes = torch.empty(max(int(lib.isg_planes32_elems(N, C)), 1), dtype=torch.int16, device=x.device)
    inv = torch.empty(max(N, 1), dtype=torch.float32, device=x.device)
    _lib.check(lib.isg_instr_gate_planes32(_chk(x, "x", torch.float32), _chk(instr, "instr", torch.float32, (instr.size(0), C)),
                                           _chk(batch, "batch", torch.int64, (N,)), 0 if rows is None else rows.data_ptr(),
                                           planes.data_ptr(), inv.data_ptr(), N, C, _stream()), "isg_instr_gate_planes32")
    pl = Planes32(planes, inv, N, C)
    if rows is not None:
        _attach(rows, "_isg_planes32", pl)
    return rows, pl


def _h3p_weight(weight: Tensor, bias: Optional[Tensor], cache: bool = True, seg_cols: int = 0):
    """planes32 of a weight [N, K], its inverse row scales and the output bound {2^14 * max_n ||w_n||_1, max |b|} (device).
    seg_cols: the layout of a SEGMENTED activation -- columns [0, seg_cols) and [seg_cols, K) each padded with zero columns to a
    multiple of 32."""
    def build():
        w = weight.detach()
        if seg_cols:
            sp = (seg_cols + 31) // 32 * 32
            wl = torch.zeros(w.size(0), 2 * sp, dtype=w.dtype, device=w.device)
            wl[:, :seg_cols] = w[:, :seg_cols]
            wl[:, sp:sp + w.size(1) - seg_cols] = w[:, seg_cols:]
            p = split_planes32(wl)
        else:
            p = split_planes32(w.contiguous().clone())       # a private copy: nothing stays attached to the parameter
        l1 = w.abs().sum(dim=1).max() * 16384.0
        bm = bias.detach().abs().max() if bias is not None else torch.zeros((), device=w.device)
        return p.planes, p.inv, torch.stack([l1, bm]).to(torch.float32).contiguous()
    if not cache:
        with torch.no_grad():
            return build()
    return derived_weight(f"h3p{seg_cols or ''}", (weight,) if bias is None else (weight, bias), build)


def linear_skinny(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, gelu: bool = False, relu: bool = False) -> Optional[Tensor]:
    """act(x @ weight^T + bias) on isg_linear_skinny (small M: the reduction split over a workgroup's waves, true fp32 MFMAs, the
    weight read as it is).  None when the operands' layout is not the kernel's (the caller takes the tile kernels)."""
    # (host time matters here -- a forward at this size is ~70 of these calls and the GPU needs ~10 us for each: every tensor
    # property is read once, nothing is detached or viewed)
    if relu and gelu:
        raise ValueError("relu excludes gelu")
    if x.dim() != 2 or weight.dim() != 2:
        return None
    M, K = x.shape
    N, Kw = weight.shape
    lda, ldw, xp, wp = x.stride(0), weight.stride(0), x.data_ptr(), weight.data_ptr()
    if (x.stride(1) != 1 or weight.stride(1) != 1 or ((lda | ldw) & 3) or ((xp | wp) & 15) or x.dtype != torch.float32
            or weight.dtype != torch.float32 or weight.device != x.device):
        return None
    if not x.is_cuda:
        raise _lib.IsgError(f"x must live on the GPU (got {x.device}); this path has no CPU fallback")
    if Kw != K:
        raise ValueError(f"linear_skinny: x has {K} columns, weight {tuple(weight.shape)}")
    if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
        raise NotImplementedError("linear_skinny has no backward (autograd.linear is the differentiable Linear)")
    bp = 0
    if bias is not None:
        if bias.dtype != torch.float32 or bias.numel() != N or not bias.is_contiguous() or bias.device != x.device:
            raise ValueError(f"linear_skinny: bias must be a contiguous fp32 [{N}] tensor on {x.device}")
        bp = bias.data_ptr()
    lib = _lib.load()
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    rc = lib.isg_linear_skinny(xp, lda, wp, ldw, bp, out.data_ptr(), N, M, N, K, 2 if relu else (1 if gelu else 0), _stream())
    if rc == ISG_EUNSUPPORTED:
        return None
    _lib.check(rc, "isg_linear_skinny")
    COUNTERS["linear_skinny"] += 1
    return out


# The cache policy of a large (>= 128 MB) fp32 result's stores in isg_linear_h3p: -1 (the library's choice: nt at K >= 512, plain
# below) / 0 plain / 1 nt / 2 sc0 sc1 nt, or "auto" = measured once per process on the box (_h3p_tune).  Results do not depend on
# it.  In ISOLATION 2 runs the K = 300 projections 15-32 % faster than plain stores on some MI355X boxes and 21 % slower on others
# (the same way in every process on a box); in the full model, on a box where it wins in isolation, every policy gives the same
# step (20.09-20.29 ms: profiles/r04_ag_h3p_store_policy.txt) -- what the producer gains by not leaving its result in L2 / the
# Infinity Cache its consumer loses.  So the default is the library's choice and "auto" stays an experiment.
_h3p_policy_state = {"chosen": None, "us": None}


def h3p_store_policy():
    """What _h3p_tune chose in this process (None before the first large Linear), with the times it measured."""
    return dict(_h3p_policy_state)


def _h3p_tune(dev) -> None:
    """One-time choice of the store policy for large results: the K = 300 projection of 65 536 rows onto 1 200 columns (a 315 MB
    result), the library's own choice against write-through streaming stores, median of three launches each.  ~3 ms, once per
    process; skipped (library's choice) while a stream is being captured."""
    lib = _lib.load()
    if CFG.h3p_store_policy != "auto":
        _lib.check(lib.isg_linear_h3p_store_policy(int(CFG.h3p_store_policy)), "isg_linear_h3p_store_policy")
        _h3p_policy_state.update(chosen=int(CFG.h3p_store_policy), us=None)
        return
    if torch.cuda.is_current_stream_capturing():
        return
    M, N, K = 65536, 1200, 300
    KT = (K + 31) // 32
    ap = torch.zeros(M * KT * 64, dtype=torch.int16, device=dev)
    ainv = torch.ones(M, dtype=torch.float32, device=dev)
    wp = torch.zeros(N * KT * 64, dtype=torch.int16, device=dev)
    winv = torch.ones(N, dtype=torch.float32, device=dev)
    out = torch.empty(M, N, dtype=torch.float32, device=dev)
    ap.random_(0, 15000)          # fp16 bit patterns of finite values in [0, 0.8): the kernel's speed does not depend on the
    wp.random_(0, 15000)          # values, but the chip's clocks do on all-zero operands
    us = {}
    for pol in (-1, 2, -1, 2):
        _lib.check(lib.isg_linear_h3p_store_policy(pol), "isg_linear_h3p_store_policy")
        ts = []
        for _ in range(4):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            _lib.check(lib.isg_linear_h3p(ap.data_ptr(), ainv.data_ptr(), wp.data_ptr(), winv.data_ptr(), 0, out.data_ptr(), 0, 0, 0,
                                          M, N, K, N, 0, 0, 0, _stream()), "isg_linear_h3p")
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e) * 1e3)
        us.setdefault(pol, []).extend(ts[1:])
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    chosen = 2 if med[2] < 0.95 * med[-1] else -1
    _lib.check(lib.isg_linear_h3p_store_policy(chosen), "isg_linear_h3p_store_policy")
    _h3p_policy_state.update(chosen=chosen, us={str(k): round(v, 1) for k, v in med.items()})


def linear_h3p(x, weight: Tensor, bias: Optional[Tensor] = None, gelu: bool = False, relu: bool = False,
               planes_out: bool = False, cache_planes: bool = True):
    """act(x @ weight^T + bias) on the planes32 engine.  x: Planes32 or fp32 rows (split here, once per tensor version).
    planes_out: the result as Planes32 (its columns padded with zeros to a multiple of 32), scaled by the bound known before the
    product -- the input of the next Linear with no pass over it; otherwise fp32 [M, N]."""
    if relu and gelu:
        raise ValueError("relu excludes gelu")
    lib = _lib.load()
    xp = x if isinstance(x, Planes32) else split_planes32(x)
    M, K = xp.rows, xp.cols
    N = weight.size(0)
    if weight.size(1) != K:
        raise ValueError(f"linear_h3p: x has {K} columns, weight {tuple(weight.shape)}")
    seg = xp.seg_cols
    if seg and (not gelu or relu or 2 * seg != K):
        raise ValueError("linear_h3p: a segmented operand (isg_gatv2_mp_fwd_planes) feeds a Linear + GELU over two equal halves")
    wp, winv, bound = _h3p_weight(weight, bias, cache_planes, seg)
    bptr = _bias_ptr(bias, N)
    act = 2 if relu else (1 if gelu else 0)
    dev = xp.planes.device
    ksplit = (seg + 31) // 32 * 32
    Kc = 2 * ksplit if seg else K                    # the k extent the kernel walks: both segments with their padding
    seg_args = (xp.inv_first.data_ptr(), ksplit) if seg else (0, 0)
    timer = H3P_TIMER
    COUNTERS["linear_h3p"] += 1                      # launches of the engine / of them, those fed a segmented message-passing result
    COUNTERS["h3p_segmented"] += 1 if seg else 0
    if timer is not None:
        ev0, ev1 = timer.bracket({"M": M, "N": N, "K": Kc, "planes_out": bool(planes_out)})
    if planes_out:
        dp = torch.empty(int(lib.isg_planes32_elems(M, N)), dtype=torch.int16, device=dev)
        dinv = torch.empty(M, dtype=torch.float32, device=dev)
        if timer is not None:
            ev0.record()
        _lib.check(lib.isg_linear_h3p(xp.planes.data_ptr(), xp.inv.data_ptr(), wp.data_ptr(), winv.data_ptr(), bptr, 0,
                                      dp.data_ptr(), dinv.data_ptr(), bound.data_ptr(), M, N, Kc, 0, act, *seg_args, _stream()),
                   "isg_linear_h3p")
        if timer is not None:
            ev1.record()
        return Planes32(dp, dinv, M, N)
    if _h3p_policy_state["chosen"] is None and M * N * 4 >= 128_000_000:
        _h3p_tune(dev)
    out = torch.empty(M, N, dtype=torch.float32, device=dev)
    if timer is not None:
        ev0.record()
    _lib.check(lib.isg_linear_h3p(xp.planes.data_ptr(), xp.inv.data_ptr(), wp.data_ptr(), winv.data_ptr(), bptr,
                                  out.data_ptr(), 0, 0, 0, M, N, Kc, N, act, *seg_args, _stream()), "isg_linear_h3p")
    if timer is not None:
        ev1.record()
    return out


def planes32_to_rows(p: Planes32) -> Tensor:
    """fp32 rows of a Planes32 (hi + mid) * inv: tests and diagnostics only."""
    if p.seg_cols:
        st = (p.seg_cols + 31) // 32
        v = p.planes.view(torch.float16).view(p.rows, 2 * st, 2, 32).float()
        full = (v[:, :, 0] + v[:, :, 1]).reshape(p.rows, 2, st * 32)
        return torch.cat([full[:, 0, :p.seg_cols] * p.inv_first[:, None], full[:, 1, :p.cols - p.seg_cols] * p.inv[:, None]],
                         dim=1).contiguous()
    KT = (p.cols + 31) // 32
    v = p.planes.view(torch.float16).view(p.rows, KT, 2, 32).float()
    return ((v[:, :, 0] + v[:, :, 1]).reshape(p.rows, KT * 32)[:, :p.cols] * p.inv[:, None]).contiguous()


def linear_multi(x: Tensor, weights, out_dtype=torch.float32):
    """x @ W_i^T for several bias-free Linears of one shape over the same rows, as ONE launch of the row-panel kernel
    (isg_linear_panel_multi): a tuple of dense [M, n] tensors, or None when the shape is not the panel kernel's (the caller
    then projects layer by layer).  MGAT's per-layer lin_edge projections of the shared edge features use it."""
    if not CFG.linear_multi or CFG.gemm_backend != "bf16x6" or _rec(x, *weights) or len(weights) < 2:
        return None
    M, K = x.shape
    n = weights[0].size(0)
    if any(tuple(w.shape) != (n, K) for w in weights):
        return None
    if (CFG.linear_multi_h3p and x.dtype == torch.float32 and out_dtype == torch.float32 and (n & 3) == 0 and
            reads_planes32(M, len(weights) * n, K) and x.stride(1) == 1 and (x.stride(0) & 3) == 0 and (x.data_ptr() & 15) == 0):
        # K >= 256 (the reference's default width): ONE launch of the planes32 engine over the concatenated weights -- the shared
        # rows are read once instead of once per layer (262 MB per layer at 205 k edges); the layers' results are column slices
        cat = derived_weight("linear_multi", tuple(weights), lambda: torch.cat([w.detach() for w in weights], 0).contiguous())
        y = linear_h3p(x, cat, None)
        return tuple(y[:, i * n:(i + 1) * n] for i in range(len(weights)))
    if (n & 31) or (K & 3):
        return None
    route = linear_route(M, len(weights) * n, K, x.dtype, out_dtype)
    if route not in ("f16x3", "f16x3_f16", "panel"):      # the row-panel kernels' shapes only
        return None
    lib = _lib.load()
    cat = derived_weight("linear_multi", tuple(weights), lambda: torch.cat([w.detach() for w in weights], 0).contiguous())
    L = len(weights)
    out = torch.empty(L, M, n, dtype=out_dtype, device=x.device)
    if route != "panel":
        planes, inv = _weight_planes(cat, True, "f16x3")
        fn = lib.isg_linear_f16x3 if route == "f16x3" else lib.isg_linear_f16x3_f16
        _lib.check(fn(_chk(x, "x", torch.float32), planes.data_ptr(), inv.data_ptr(), 0, out.data_ptr(),
                      M, L * n, K, K, n, 0, n, M * n, _stream()), "isg_linear_f16x3")
        return tuple(out[i] for i in range(L))
    planes = _weight_planes(cat, True, "panel")
    _lib.check(lib.isg_linear_panel_multi(
        _chk(x, "x", x.dtype), 1 if x.dtype == torch.float16 else 0, planes.data_ptr(), 0, out.data_ptr(),
        1 if out_dtype == torch.float16 else 0, M, L * n, K, K, n, 0, n, M * n, _stream()), "isg_linear_panel_multi")
    return tuple(out[i] for i in range(L))


def mha_small_supported(t_kv: int, head_dim: int) -> bool:
    """isg_mha_small's launch limits (csrc/isg_attn.hip): head_dim <= 64 and a multiple of 4, <= 128 keys, and a head's Q / K /
    V rows (as many queries as keys at most: the callers pass the longer of the two) + score strips within 64 KB of LDS -- at
    head_dim 64 that is 80 keys (CLIP questions: 77).  Callers ask BEFORE choosing the kernel path."""
    return head_dim <= 64 and head_dim % 4 == 0 and t_kv <= 128 and (t_kv * (3 * head_dim + 4) + 4 * 128) * 4 <= 64 * 1024


def mha_rows_supported(t_q: int, t_kv: int, heads: int, head_dim: int) -> bool:
    """The all-heads form of isg_mha_small (one workgroup per batch item, the result rows assembled in LDS and written as
    planes32): a head's Q / K / V, the score strips and t_q whole rows within 64 KB -- 12-token questions and the decoder's 4
    queries at d = 512, not CLIP's 77 tokens."""
    return (CFG.mha_rows_planes and t_q <= CFG.mha_rows_max_tq and mha_small_supported(max(t_q, t_kv), head_dim) and
            (t_kv * (2 * head_dim + 4) + t_q * head_dim + (4 if t_q <= 4 else 8 if t_q <= 8 else 12) * 128 +
             t_q * heads * head_dim) * 4 <= 64 * 1024)


def mha_small(q: Tensor, k: Tensor, v: Tensor, batch_size: int, heads: int, key_bias: Optional[Tensor] = None,
              want_rowmax: bool = False, planes_out: bool = False):
    """softmax(Q K^T / sqrt(hd) + key_bias) V per (batch item, head) for short sequences (csrc/isg_attn.hip).
    q [Tq*B, D], k / v [Tk*B, D] in torch's [T, B, D] row order (row t*B + b; column slices of a fused projection are
    fine), key_bias fp32 [B, Tk] additive (question_encoder.py:35-37) -> [Tq*B, D].
    planes_out (callers ask mha_rows_supported first): the result as Planes32 only -- out_proj's operand, no split pass."""
    lib = _lib.load()
    B, H, D = int(batch_size), int(heads), q.size(1)
    hd = D // H
    Tq, Tk = q.size(0) // B, k.size(0) // B
    if H * hd != D or Tq * B != q.size(0) or Tk * B != k.size(0) or tuple(v.shape) != tuple(k.shape):
        raise ValueError(f"mha_small: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} vs B={B}, H={H}")
    kb = _chk(key_bias, "key_bias", torch.float32, (B, Tk), optional=True)
    if planes_out:
        pl = torch.empty(int(lib.isg_planes32_elems(Tq * B, D)), dtype=torch.int16, device=q.device)
        pinv = torch.empty(Tq * B, dtype=torch.float32, device=q.device)
        _lib.check(lib.isg_mha_small(_chk_rows(q, "q"), q.stride(0), _chk_rows(k, "k"), k.stride(0), _chk_rows(v, "v"),
                                     v.stride(0), kb, 0, D, 0, B, H, hd, Tq, Tk, pl.data_ptr(), pinv.data_ptr(), _stream()),
                   "isg_mha_small")
        return Planes32(pl, pinv, Tq * B, D)
    out = torch.empty(Tq * B, D, dtype=torch.float32, device=q.device)
    rm = torch.empty(Tq * B, H, dtype=torch.float32, device=q.device) if want_rowmax else None
    _lib.check(lib.isg_mha_small(_chk_rows(q, "q"), q.stride(0), _chk_rows(k, "k"), k.stride(0), _chk_rows(v, "v"),
                                 v.stride(0), kb, out.data_ptr(), D, 0 if rm is None else rm.data_ptr(), B, H, hd, Tq, Tk, 0, 0,
                                 _stream()), "isg_mha_small")
    if rm is not None:
        attach_row_maxima(out, rm)
    return out


def linear_wgrad(grad_out: Tensor, x: Tensor) -> Tensor:
    """dW[N,K] = grad_out^T x for y = x W^T: split-M GEMM on the fp32 matrix cores (csrc/isg_wgrad.hip)."""
    lib = _lib.load()
    M, N = grad_out.shape
    K = x.size(1)
    if M == 0:
        return torch.zeros(N, K, dtype=torch.float32, device=x.device)
    splits = int(lib.isg_linear_wgrad_splits(M, N, K))
    part = torch.empty(splits, N, K, dtype=torch.float32, device=x.device)
    _lib.check(lib.isg_linear_wgrad(_chk(grad_out, "grad_out", torch.float32, (M, N)), _chk(x, "x", torch.float32, (M, K)),
                                    part.data_ptr(), M, N, K, N, K, splits, _stream()), "isg_linear_wgrad")
    return part.sum(0) if splits > 1 else part[0]


# ------------------------------------------------------------------------------------------------
# A Linear's backward (include/isg_linear_train.h, csrc/isg_linear_bwd.hip); autograd._Linear wires these
# ------------------------------------------------------------------------------------------------
def _chk_rows4(t: Tensor, name: str) -> int:
    """_chk for a 2-D fp32 tensor whose rows may be strided and are aligned to 4 bytes only (a column slice of a wider tensor)."""
    if not t.is_cuda:
        raise _lib.IsgError(f"{name} must live on the GPU (got {t.device}); this path has no CPU fallback")
    if t.dtype != torch.float32 or t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1) or (t.size(0) > 1 and t.stride(0) < t.size(1)):
        raise ValueError(f"{name}: expected fp32 [rows, cols] with contiguous columns and a row pitch of at least cols")
    if torch.is_grad_enabled() and t.requires_grad:
        raise NotImplementedError(f"{name} requires grad but this operator has no backward (see autograd.py)")
    return t.data_ptr()


def _pitch(t: Tensor) -> int:
    return max(int(t.stride(0)), int(t.size(1))) if t.size(0) > 1 else int(t.size(1))


LINEAR_BWD_MODES = {"identity": 0, "gelu": 1, "relu": 2}


def linear_bwd_prep(g: Tensor, saved: Optional[Tensor], mode: int, want_dz: bool = True, want_db: bool = True):
    """(dz | None, db | None) of a Linear's upstream gradient g [M, N] in one pass (isg_linear_bwd_prep): mode 0 dz = g (asked for
    db alone, g is not copied), 1 dz = g * GELU'(saved = the pre-activation), 2 dz = g * (saved = the ReLU's result > 0); db = the
    column sums of dz, from the kernel's partial rows."""
    from . import _lib_linear_train
    lib = _lib_linear_train.load()
    if not (want_dz or want_db):
        raise ValueError("linear_bwd_prep: nothing asked for")
    if mode not in (0, 1, 2):
        raise ValueError(f"linear_bwd_prep: mode {mode} (0 identity, 1 GELU, 2 ReLU)")
    if mode != 0 and (saved is None or saved.shape != g.shape):
        raise ValueError("linear_bwd_prep: modes 1 and 2 need the saved tensor, of the gradient's shape")
    gp = _chk_rows4(g, "g")
    sp = 0 if mode == 0 else _chk_rows4(saved, "saved")
    M, N = g.shape
    dz = torch.empty(M, N, dtype=torch.float32, device=g.device) if want_dz else None
    if M == 0 or N == 0:
        return dz, (torch.zeros(N, dtype=torch.float32, device=g.device) if want_db else None)
    P = int(lib.isg_linear_bwd_prep_parts(M, N))
    part = torch.empty(P, N, dtype=torch.float32, device=g.device) if want_db else None
    _lib.check(lib.isg_linear_bwd_prep(gp, _pitch(g), sp, 0 if mode == 0 else _pitch(saved), mode,
                                       0 if dz is None else dz.data_ptr(), N, 0 if part is None else part.data_ptr(), M, N,
                                       _stream()), "isg_linear_bwd_prep")
    db = None if part is None else (part.sum(0) if P > 1 else part[0])
    return dz, db


def linear_wgrad_bf16x6(grad_out: Tensor, x: Tensor, splits: Optional[int] = None) -> Tensor:
    """dW[N,K] = grad_out^T x for y = x W^T: split-M GEMM on the bf16 matrix cores, six products per pair of fp32 values
    (csrc/isg_linear_bwd.hip).  Rows of both operands may be strided (column slices)."""
    from . import _lib_linear_train
    lib = _lib_linear_train.load()
    M, N = grad_out.shape
    K = x.size(1)
    if x.size(0) != M:
        raise ValueError(f"linear_wgrad_bf16x6: grad_out has {M} rows, x {x.size(0)}")
    if M == 0 or N == 0 or K == 0:
        return torch.zeros(N, K, dtype=torch.float32, device=x.device)
    gp, xp = _chk_rows4(grad_out, "grad_out"), _chk_rows4(x, "x")
    if splits is None:
        splits = int(lib.isg_linear_wgrad_bf16x6_splits(M, N, K))
    part = torch.empty(splits, N, K, dtype=torch.float32, device=x.device)
    _lib.check(lib.isg_linear_wgrad_bf16x6(gp, xp, part.data_ptr(), M, N, K, _pitch(grad_out), _pitch(x), splits, _stream()),
               "isg_linear_wgrad_bf16x6")
    return part.sum(0) if splits > 1 else part[0]


# ------------------------------------------------------------------------------------------------
# Training of the question side (include/isg_train.h, csrc/isg_text_bwd.hip); autograd.py wires these
# ------------------------------------------------------------------------------------------------
MHA_BWD_LDS_MAX = 160 * 1024     # isg_mha_small_bwd: Q, K, V, dO and the two [Tq][Tk] strips in the LDS of one CU


def mha_small_bwd_lds_bytes(head_dim: int, t_q: int, t_kv: int) -> int:
    """isg_mha_small_bwd's LDS (restated from csrc/isg_text_bwd.hip): K and V rows padded by a float4, Q, dO, P~ and dS strips."""
    return 4 * (2 * t_kv * (head_dim + 4) + 2 * t_q * head_dim + 2 * t_q * t_kv)


def mha_small_train_supported(t_q: int, t_kv: int, head_dim: int) -> bool:
    """Do isg_mha_small / isg_mha_small_train (the forward's 64 KB) and isg_mha_small_bwd (160 KB) both take the shape?"""
    return (head_dim <= 64 and head_dim % 4 == 0 and 1 <= t_kv <= 128 and
            (t_kv * (2 * head_dim + 4) + t_q * head_dim + 4 * 128) * 4 <= 64 * 1024 and
            mha_small_bwd_lds_bytes(head_dim, t_q, t_kv) <= MHA_BWD_LDS_MAX)


def _drop_args(p: float, seed: int):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability {p}: 0 <= p < 1")
    return p, int(seed) & 0xFFFFFFFFFFFFFFFF


def dropout(x: Tensor, p: float, seed: int) -> Tensor:
    """x * keep / (1 - p) under the keep rule of include/isg_train.h (element (i, j): Philox block (i, j >> 2), word j & 3).  Its
    backward is the same call on the gradient."""
    from . import _lib_train
    p, seed = _drop_args(p, seed)
    M, D = x.shape
    out = torch.empty(M, D, dtype=torch.float32, device=x.device)
    _lib.check(_lib_train.load().isg_dropout(_chk_rows(x, "x"), x.stride(0), out.data_ptr(), D, M, D, p, seed, _stream()), "isg_dropout")
    return out


def mha_small_train(q: Tensor, k: Tensor, v: Tensor, batch_size: int, heads: int, key_bias: Optional[Tensor], p: float,
                    seed: int) -> Tensor:
    """ops.mha_small's heads form with dropout on the attention probabilities (isg_mha_small_train)."""
    from . import _lib_train
    p, seed = _drop_args(p, seed)
    B, H, D = int(batch_size), int(heads), q.size(1)
    hd = D // H
    Tq, Tk = q.size(0) // B, k.size(0) // B
    if H * hd != D or Tq * B != q.size(0) or Tk * B != k.size(0) or tuple(v.shape) != tuple(k.shape):
        raise ValueError(f"mha_small_train: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} vs B={B}, H={H}")
    out = torch.empty(Tq * B, D, dtype=torch.float32, device=q.device)
    _lib.check(_lib_train.load().isg_mha_small_train(
        _chk_rows(q, "q"), q.stride(0), _chk_rows(k, "k"), k.stride(0), _chk_rows(v, "v"), v.stride(0),
        _chk(key_bias, "key_bias", torch.float32, (B, Tk), optional=True), out.data_ptr(), D, B, H, hd, Tq, Tk, p, seed, _stream()),
        "isg_mha_small_train")
    return out


def mha_small_backward(q: Tensor, k: Tensor, v: Tensor, batch_size: int, heads: int, key_bias: Optional[Tensor], grad_out: Tensor,
                       d_q: Tensor, d_k: Tensor, d_v: Tensor, p: float, seed: int) -> bool:
    """isg_mha_small_bwd into the caller's d_q / d_k / d_v (column slices of one gradient are fine).  False: the kernel does not
    take the shape (ISG_EUNSUPPORTED), nothing was written."""
    from . import _lib_train
    p, seed = _drop_args(p, seed)
    B, H, D = int(batch_size), int(heads), q.size(1)
    hd = D // H
    Tq, Tk = q.size(0) // B, k.size(0) // B
    if tuple(grad_out.shape) != tuple(q.shape) or tuple(d_q.shape) != tuple(q.shape) or tuple(d_k.shape) != tuple(k.shape) or \
            tuple(d_v.shape) != tuple(v.shape):
        raise ValueError("mha_small_backward: a gradient's shape differs from its operand's")
    rc = _lib_train.load().isg_mha_small_bwd(
        _chk_rows(q, "q"), q.stride(0), _chk_rows(k, "k"), k.stride(0), _chk_rows(v, "v"), v.stride(0),
        _chk(key_bias, "key_bias", torch.float32, (B, Tk), optional=True), _chk_rows(grad_out, "grad_out"), grad_out.stride(0),
        _chk_rows(d_q, "d_q"), d_q.stride(0), _chk_rows(d_k, "d_k"), d_k.stride(0), _chk_rows(d_v, "d_v"), d_v.stride(0),
        B, H, hd, Tq, Tk, p, seed, _stream())
    if rc == ISG_EUNSUPPORTED:
        return False
    _lib.check(rc, "isg_mha_small_bwd")
    return True


def _ln_operands(x: Tensor, residual: Optional[Tensor], norm: torch.nn.LayerNorm):
    M, D = x.shape
    if residual is not None and tuple(residual.shape) != (M, D):
        raise ValueError(f"add_layernorm: x {tuple(x.shape)} vs residual {tuple(residual.shape)}")
    if tuple(norm.normalized_shape) != (D,) or norm.weight is None:
        raise ValueError("add_layernorm: an affine LayerNorm over the last dimension")
    return (M, D, _chk_rows(x, "x"), x.stride(0), 0 if residual is None else _chk_rows(residual, "residual"),
            0 if residual is None else residual.stride(0), _chk(norm.weight.detach(), "weight", torch.float32, (D,)))


def dropout_add_layernorm(x: Tensor, residual: Optional[Tensor], norm: torch.nn.LayerNorm, p: float, seed: int) -> Optional[Tensor]:
    """LayerNorm(residual + dropout(x)) in one launch (isg_dropout_add_layernorm).  None: a shape the kernel does not take."""
    from . import _lib_train
    p, seed = _drop_args(p, seed)
    M, D, xp, ldx, rp, ldr, gp = _ln_operands(x, residual, norm)
    out = torch.empty(M, D, dtype=torch.float32, device=x.device)
    rc = _lib_train.load().isg_dropout_add_layernorm(
        xp, ldx, rp, ldr, gp, _chk(None if norm.bias is None else norm.bias.detach(), "bias", torch.float32, (D,), optional=True),
        float(norm.eps), out.data_ptr(), D, M, D, p, seed, _stream())
    if rc == ISG_EUNSUPPORTED:
        return None
    _lib.check(rc, "isg_dropout_add_layernorm")
    return out


def add_layernorm_backward(x: Tensor, residual: Optional[Tensor], norm: torch.nn.LayerNorm, grad_out: Tensor, p: float, seed: int,
                           want_residual: bool = True):
    """isg_add_layernorm_bwd: (d_x, d_residual or None, d_gamma, d_beta or None); the partial rows of d_gamma / d_beta (one per
    workgroup) are summed here, in one fixed order."""
    from . import _lib_train
    lib = _lib_train.load()
    p, seed = _drop_args(p, seed)
    M, D, xp, ldx, rp, ldr, gp = _ln_operands(x, residual, norm)
    parts = max(int(lib.isg_add_layernorm_bwd_parts(M)), 1)
    d_x = torch.empty(M, D, dtype=torch.float32, device=x.device)
    d_r = torch.empty(M, D, dtype=torch.float32, device=x.device) if residual is not None and want_residual else None
    dg = torch.zeros(parts, D, dtype=torch.float32, device=x.device)
    db = torch.zeros(parts, D, dtype=torch.float32, device=x.device) if norm.bias is not None else None
    _lib.check(lib.isg_add_layernorm_bwd(xp, ldx, rp, ldr, gp, float(norm.eps), _chk_rows(grad_out, "grad_out"), grad_out.stride(0),
                                         d_x.data_ptr(), D, 0 if d_r is None else d_r.data_ptr(), D, dg.data_ptr(),
                                         0 if db is None else db.data_ptr(), M, D, p, seed, _stream()), "isg_add_layernorm_bwd")
    return d_x, d_r, dg.sum(0), None if db is None else db.sum(0)


# ------------------------------------------------------------------------------------------------
# The step's tail: loss, accuracy (include/isg_optim.h; the optimizer half is optim.py)
# ------------------------------------------------------------------------------------------------
class CrossEntropy(NamedTuple):
    """What ops.cross_entropy returns.  Everything stays on the device: `stats` is the kernel's double [4] = (mean_loss, n_counted,
    n_correct, n_rows), `loss` its first entry rounded to fp32 (the scalar to call .backward() on)."""
    loss: Tensor        # 0-dim fp32
    pred: Tensor        # [B] int32, the lowest index among a row's maxima
    row_loss: Tensor    # [B] fp32; 0 on ignored rows, NaN where a label is outside [0, A)
    stats: Tensor       # [4] float64
    lse: Tensor         # [B] float64, what the backward recomputes the probabilities from


def _xent_operands(logits: Tensor, labels: Tensor):
    if not logits.is_cuda or not labels.is_cuda:
        raise _lib.IsgError(f"cross_entropy: logits and labels must live on the GPU (got {logits.device}, {labels.device}); "
                            "this path has no CPU fallback")
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.size(1) < 1 or (logits.size(0) > 1 and logits.stride(0) < logits.size(1)) \
            or (logits.size(1) > 1 and logits.stride(1) != 1):
        raise ValueError("cross_entropy: logits are fp32 [B, A] with contiguous columns (a column slice of a wider matrix is fine)")
    B, A = logits.shape
    if labels.dtype != torch.int64 or tuple(labels.shape) != (B,) or not labels.is_contiguous():
        raise ValueError(f"cross_entropy: labels are a contiguous int64 [{B}], got {labels.dtype} {tuple(labels.shape)}")
    return B, A, max(logits.stride(0), A) if B > 1 else A


def cross_entropy(logits: Tensor, labels: Tensor, ignore_index: int = -100, totals: Optional[Tensor] = None) -> CrossEntropy:
    """Mean softmax cross-entropy over the rows whose label is not `ignore_index`, with top-1 (isg_xent_fwd): F.cross_entropy's
    value, the reference's accuracy() count and, when `totals` (train.Meters.totals: a device float64 [8]) is given, the running
    meters advanced in the same launch.  Nothing returns to the host.  Under autograd the call goes through
    autograd.cross_entropy, whose backward is isg_xent_bwd."""
    if _rec(logits):
        from . import autograd
        return autograd.cross_entropy(logits, labels, ignore_index, totals)
    from . import _lib_optim
    B, A, ld = _xent_operands(logits, labels)
    dev = logits.device
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    lse = torch.empty(B, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    row_loss = torch.empty(B, dtype=torch.float32, device=dev)
    pred = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib_optim.load().isg_xent_fwd(logits.data_ptr(), ld, labels.data_ptr(), int(ignore_index), row_loss.data_ptr(),
                                              lse.data_ptr(), pred.data_ptr(), stats.data_ptr(), loss.data_ptr(),
                                              _chk(totals, "totals", torch.float64, (8,), optional=True), B, A, _stream()),
               "isg_xent_fwd")
    return CrossEntropy(loss, pred, row_loss, stats, lse)


def cross_entropy_backward(logits: Tensor, labels: Tensor, lse: Tensor, stats: Tensor, grad: Optional[Tensor],
                           ignore_index: int = -100) -> Tensor:
    """d loss / d logits times the upstream gradient `grad` (a device fp32 scalar, or None for 1): isg_xent_bwd, one pass."""
    from . import _lib_optim
    B, A, ld = _xent_operands(logits, labels)
    if grad is not None and (not grad.is_cuda or grad.dtype != torch.float32 or grad.numel() != 1):
        raise ValueError("cross_entropy_backward: the upstream gradient is one fp32 value on the GPU")
    d = torch.empty(B, A, dtype=torch.float32, device=logits.device)
    _lib.check(_lib_optim.load().isg_xent_bwd(logits.data_ptr(), ld, labels.data_ptr(), int(ignore_index),
                                              _chk(lse, "lse", torch.float64, (B,)), _chk(stats, "stats", torch.float64, (4,)),
                                              0 if grad is None else grad.data_ptr(), d.data_ptr(), A, B, A, _stream()),
               "isg_xent_bwd")
    return d


# ------------------------------------------------------------------------------------------------
# Evaluation by question type (include/isg_eval.h): the answer's rank, grouped meters, grouped co-occurrence totals
# ------------------------------------------------------------------------------------------------
EVAL_TOPK_MAX, EVAL_FACETS_MAX, EVAL_GROUPS_MAX, GROUP_SLOTS = 8, 4, 256, 8      # ISG_EVAL_*_MAX, ISG_GRP_SLOTS


class AnswerRank(NamedTuple):
    """What ops.answer_rank returns, all on the device."""
    rank: Tensor                 # [B] int32: classes that beat the label; -1 ignored row; A for a bad label or a NaN row
    top_ids: Optional[Tensor]    # [B, k] int64: the k best classes, value descending, index ascending among equals; -1 beyond A
    top_prob: Optional[Tensor]   # [B, k] fp32: their softmax probabilities (needs `lse`), 0 where the id is -1


def answer_rank(logits: Tensor, labels: Tensor, k: int = 5, ignore_index: int = -100, lse: Optional[Tensor] = None,
                want_top: bool = False) -> AnswerRank:
    """The rank of every row's label among its logits (isg_answer_rank: one launch, a wave per row, no sync): the reference's
    accuracy(output, target, topk) counts a row as a hit at k exactly where 0 <= rank < k.  With want_top the k best classes come
    along (1 <= k <= 8), and their probabilities when `lse` (ops.cross_entropy(...).lse) is given."""
    from . import _lib_eval
    B, A, ld = _xent_operands(logits, labels)
    k = int(k)
    if want_top and not 1 <= k <= EVAL_TOPK_MAX:
        raise ValueError(f"answer_rank: the {k} best classes were asked for; the kernel lists 1 to {EVAL_TOPK_MAX}")
    dev = logits.device
    rank = torch.empty(B, dtype=torch.int32, device=dev)
    top_ids = torch.empty(B, k, dtype=torch.int64, device=dev) if want_top else None
    top_prob = torch.empty(B, k, dtype=torch.float32, device=dev) if want_top and lse is not None else None
    _lib.check(_lib_eval.load().isg_answer_rank(logits.data_ptr(), ld, labels.data_ptr(), int(ignore_index),
                                                _chk(lse, "lse", torch.float64, (B,), optional=True), rank.data_ptr(),
                                                0 if top_ids is None else top_ids.data_ptr(),
                                                0 if top_prob is None else top_prob.data_ptr(), k if want_top else 0, B, A, _stream()),
               "isg_answer_rank")
    return AnswerRank(rank, top_ids, top_prob)


def _groups_operand(groups: Tensor, B: int, what: str) -> int:
    if groups.dim() != 2 or groups.size(0) != B or not 1 <= groups.size(1) <= EVAL_FACETS_MAX:
        raise ValueError(f"{what}: groups are int32 [{B}, F] with 1 <= F <= {EVAL_FACETS_MAX}, got {tuple(groups.shape)}")
    return groups.size(1)


def _group_totals(totals: Tensor, slots: int, dtype, what: str) -> int:
    if totals.dim() != 2 or totals.size(1) != slots or not 1 <= totals.size(0) <= EVAL_GROUPS_MAX:
        raise ValueError(f"{what}: totals are {dtype} [G, {slots}] with 1 <= G <= {EVAL_GROUPS_MAX}, got {tuple(totals.shape)}")
    return totals.size(0)


def group_meters_parts(B: int, G: int) -> int:
    """Doubles of the workspace isg_group_meters needs for B rows and G groups (a host-only call)."""
    from . import _lib_eval
    return int(_lib_eval.load().isg_group_meters_parts(int(B), int(G)))


def group_meters(row_loss: Tensor, rank: Tensor, groups: Tensor, totals: Tensor, k: int = 5, status: Optional[Tensor] = None,
                 overall: Optional[Tensor] = None) -> Tensor:
    """Running meters per group of questions (isg_group_meters: two launches, no sync): `totals` (float64 [G, 8], slots ISG_GRP_*
    of include/isg_eval.h: rows, loss sum, nonfinite losses, hits at 1, hits at k) has this batch ADDED to it.  row_loss fp32 [B]
    and rank int32 [B] are ops.cross_entropy's and ops.answer_rank's; groups int32 [B, F] holds ids in [0, G), -1 for none.
    `status` (int32 [2], zeroed once per evaluation): bad ids seen and the first row that held one.  `overall` (float64 [8]): the
    same slots over all rows, each counted once whatever its groups.  Returns totals."""
    from . import _lib_eval
    B = row_loss.numel()
    G = _group_totals(totals, GROUP_SLOTS, torch.float64, "group_meters")
    F = _groups_operand(groups, B, "group_meters")
    if int(k) < 1:
        raise ValueError(f"group_meters: k = {k}")
    n = group_meters_parts(B, G)
    parts = torch.empty(n, dtype=torch.float64, device=totals.device)
    _lib.check(_lib_eval.load().isg_group_meters(_chk(row_loss, "row_loss", torch.float32, (B,)),
                                                 _chk(rank, "rank", torch.int32, (B,)),
                                                 _chk(groups, "groups", torch.int32), F, G, int(k),
                                                 _chk(totals, "totals", torch.float64),
                                                 _chk(overall, "overall", torch.float64, (GROUP_SLOTS,), optional=True),
                                                 parts.data_ptr(), n, _chk(status, "status", torch.int32, (2,), optional=True), B,
                                                 _stream()), "isg_group_meters")
    COUNTERS["eval_groups"] += 1
    return totals


def token_coo_groups(table: Tensor, qflags: Optional[Tensor], groups: Tensor, totals: Tensor, status: Optional[Tensor] = None) -> Tensor:
    """Token co-occurrence totals per group of questions (isg_token_coo_groups: one launch, no sync): row g of `totals` (int64
    [G, COO_TOTALS]) has added to it exactly what ops.token_coo adds to its totals for the questions of group g alone.  `table`
    is ops.token_coo(...).table; groups and status as ops.group_meters takes them.  Returns totals."""
    from . import _lib_eval
    B = table.size(0)
    G = _group_totals(totals, COO_TOTALS, torch.int64, "token_coo_groups")
    F = _groups_operand(groups, B, "token_coo_groups")
    _lib.check(_lib_eval.load().isg_token_coo_groups(_chk(table, "table", torch.int32, (B, 8)),
                                                     _chk(qflags, "qflags", torch.int32, (B,), optional=True),
                                                     _chk(groups, "groups", torch.int32), F, G, _chk(totals, "totals", torch.int64),
                                                     _chk(status, "status", torch.int32, (2,), optional=True), B, _stream()),
               "isg_token_coo_groups")
    COUNTERS["eval_groups"] += 1
    return totals


# ------------------------------------------------------------------------------------------------
# Grounding of the sampled subgraph in GQA's object annotations (include/isg_grounding.h)
# ------------------------------------------------------------------------------------------------
from ._lib_grounding import CONSTANTS as _GROUND      # noqa: E402 -- the header's numbers; reading them loads no library

GROUND_COLS, GROUND_TOTALS, GROUND_GOLD_MAX = _GROUND["ISG_GROUND_COLS"], _GROUND["ISG_GROUND_TOTALS"], _GROUND["ISG_GROUND_GOLD_MAX"]
GROUND_FACETS, GROUND_SETS, GROUND_HEAD = _GROUND["ISG_GROUND_FACETS"], _GROUND["ISG_GROUND_SETS"], _GROUND["ISG_GROUND_HEAD"]
GROUND_BLOCK, GROUND_HIST = _GROUND["ISG_GROUND_BLOCK"], _GROUND["ISG_GROUND_HIST"]


class Grounding(NamedTuple):
    table: Tensor                # int32 [B, GROUND_COLS]: the row of every question (include/isg_grounding.h)
    totals: Optional[Tensor]     # int64 [1 + G, GROUND_TOTALS]: the caller's running totals with this batch added, or None


def grounding(mask: Tensor, plan: "GraphPlan", gold: Tensor, pred: Optional[Tensor] = None, label: Optional[Tensor] = None,
              groups: Optional[Tensor] = None, num_groups: int = 0, threshold: float = 0.0, totals: Optional[Tensor] = None,
              status: Optional[Tensor] = None) -> Grounding:
    """How many of the annotated objects are among the kept nodes (isg_grounding: two launches, one without totals; no sync, no
    copy).  mask fp32 [N] or [N, 1] (a forward's imle_mask); gold int32 [B, F, M] of LOCAL node indices, -1 pad, -2 annotated but
    not in the graph (datasets.gqa.ObjectAnnotations.encode); pred, label int64 [B], both or neither; groups int32 [B, Fg] with
    num_groups = G as ops.group_meters takes them.  `totals` (int64 [1 + G, GROUND_TOTALS], zeroed by the caller once per
    evaluation; a plain [GROUND_TOTALS] without groups) has this batch ADDED to it; `status` as ops.group_meters."""
    from . import _lib_grounding
    lib = _lib_grounding.load()
    if (pred is None) != (label is None):
        raise ValueError("pred and label come together")
    if mask.dim() == 2 and mask.size(1) == 1:
        mask = mask.squeeze(1)
    N, B = plan.N, plan.B
    if gold.dim() != 3 or gold.size(0) != B or not 1 <= gold.size(1) <= GROUND_FACETS or not 1 <= gold.size(2) <= GROUND_GOLD_MAX:
        raise ValueError(f"gold: expected int32 [{B}, F, M] with 1 <= F <= {GROUND_FACETS} and 1 <= M <= {GROUND_GOLD_MAX}, "
                         f"got {tuple(gold.shape)}")
    G = int(num_groups)
    Fg = 0
    if groups is None:
        if G != 0:
            raise ValueError(f"grounding: num_groups = {G} without groups")
    else:
        if not 1 <= G <= EVAL_GROUPS_MAX:
            raise ValueError(f"grounding: num_groups = {G} (1 to {EVAL_GROUPS_MAX})")
        Fg = _groups_operand(groups, B, "grounding")
    if totals is not None and tuple(totals.shape) not in ((1 + G, GROUND_TOTALS),) + (((GROUND_TOTALS,),) if G == 0 else ()):
        raise ValueError(f"totals: expected int64 [{1 + G}, {GROUND_TOTALS}], got {tuple(totals.shape)}")
    table = torch.empty(B, GROUND_COLS, dtype=torch.int32, device=mask.device)
    _lib.check(lib.isg_grounding(_chk(mask, "mask", torch.float32, (N,)), float(threshold),
                                 _chk(plan.ptr, "plan.ptr", torch.int32, (B + 1,)), _chk(gold, "gold", torch.int32),
                                 gold.size(1), gold.size(2), _chk(pred, "pred", torch.int64, (B,), optional=True),
                                 _chk(label, "label", torch.int64, (B,), optional=True),
                                 _chk(groups, "groups", torch.int32, optional=True), Fg, G, _chk(table, "table", torch.int32),
                                 _chk(totals, "totals", torch.int64, optional=True),
                                 _chk(status, "status", torch.int32, (2,), optional=True), N, B, _stream()), "isg_grounding")
    COUNTERS["grounding"] += 1
    return Grounding(table, totals)


def cat_mul(a: Tensor, b: Tensor) -> Tensor:
    """cat((a, b, a * b), dim=1) (isubgvqa.py:288-291).  Inference on fp32 rows: one launch that also leaves the result's row
    maxima on it for the Linear that follows (isg_cat_mul_rowmax); otherwise the torch ops."""
    if (_rec(a, b) or a.dtype != torch.float32 or b.dtype != torch.float32 or a.dim() != 2 or a.shape != b.shape
            or a.size(1) % 4 != 0 or not a.is_cuda):
        return torch.cat((a, b, a * b), dim=1)
    lib = _lib.load()
    M, C = a.shape
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty(M, 3 * C, dtype=torch.float32, device=a.device)
    rm = torch.empty(M, 1, dtype=torch.float32, device=a.device)
    rc = lib.isg_cat_mul_rowmax(a.data_ptr(), b.data_ptr(), out.data_ptr(), rm.data_ptr(), M, C, _stream())
    if rc == ISG_EUNSUPPORTED:
        return torch.cat((a, b, a * b), dim=1)
    _lib.check(rc, "isg_cat_mul_rowmax")
    return attach_row_maxima(out, rm)


CAT_MUL_MAX_C = 128       # ISG_CATMUL_MAX_C of include/isg_fused.h


def cat_mul_linear_supported(M: int, N: int, C: int, x_dtype=torch.float32, grad: bool = False, cfg: Optional[Switches] = None) -> bool:
    """May isg_linear_f16x3_catmul run act(cat(a, b, a * b) @ W^T + bias) for a, b [M, C], W [N, 3C]?  A pure function of plain
    values.  Yes when: the switch is on; inference on fp32 rows; 32 | C <= 128 and 32 | N; and the two launches it stands for
    would be isg_cat_mul_rowmax + isg_linear_f16x3_tile in ONE K-chunk -- ops.linear_route's answer for rows that carry their
    row maxima -- whose bits it reproduces.  Everywhere else those two launches run."""
    cfg = CFG if cfg is None else cfg
    if not cfg.fuse_cat_mul_linear or grad or x_dtype != torch.float32 or M <= 0:
        return False
    if C <= 0 or C % 32 or C > CAT_MUL_MAX_C or N <= 0 or N % 32 or (M + 31) // 32 > 65535:
        return False
    return _k_chunks(3 * C)[0] == 1 and linear_route(M, N, 3 * C, rowmax_slices=True, cfg=cfg) == "f16x3_tile"


def cat_mul_linear(a: Tensor, b: Tensor, weight: Tensor, bias: Optional[Tensor] = None, gelu: bool = False,
                   want_rowmax: bool = False) -> Tensor:
    """ops.linear(ops.cat_mul(a, b), weight, bias, gelu=gelu, want_rowmax=want_rowmax), bit for bit (the result and the row
    maxima left on it), as ONE launch that reads a and b (isg_linear_f16x3_catmul) where cat_mul_linear_supported says so;
    those two launches everywhere else, also where the library declines (ISG_F16X3_MFMA=32)."""
    ok = (a.dim() == 2 and a.shape == b.shape and a.is_cuda and a.dtype == b.dtype and weight.dim() == 2 and
          weight.size(1) == 3 * a.size(1) and weight.dtype == torch.float32 and
          cat_mul_linear_supported(a.size(0), weight.size(0), a.size(1), a.dtype, torch.is_grad_enabled()))
    if ok:
        from . import _lib_fused
        lib = _lib_fused.load()
        (M, C), N = a.shape, weight.size(0)
        a, b = a.contiguous(), b.contiguous()
        planes, inv = _weight_planes(weight, True, "f16x3_rows")
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
        rm = torch.empty(M, N // 32, dtype=torch.float32, device=a.device) if want_rowmax else None
        rc = lib.isg_linear_f16x3_catmul(_chk(a, "a", torch.float32), _chk(b, "b", torch.float32), planes.data_ptr(), inv.data_ptr(),
                                         _bias_ptr(bias, N), out.data_ptr(), 0 if rm is None else rm.data_ptr(), M, N, C, N,
                                         1 if gelu else 0, _stream())
        if rc != ISG_EUNSUPPORTED:
            _lib.check(rc, "isg_linear_f16x3_catmul")
            return out if rm is None else attach_row_maxima(out, rm)
    return linear(cat_mul(a, b), weight, bias, gelu=gelu, want_rowmax=want_rowmax)


def cat_mul_mlp(seq: torch.nn.Sequential, a: Tensor, b: Tensor, want_rowmax: bool = False) -> Tensor:
    """ops.mlp(seq, ops.cat_mul(a, b), want_rowmax) for the answer heads: a Sequential that is ONE Linear (+ exact GELU, eval
    Dropout) goes through cat_mul_linear, anything else through the two calls."""
    steps = _mlp_steps(seq)
    if steps is not None and len(steps) == 1:
        return cat_mul_linear(a, b, steps[0][0].weight, steps[0][0].bias, gelu=steps[0][1], want_rowmax=want_rowmax)
    return mlp(seq, cat_mul(a, b), want_rowmax=want_rowmax)


def mlp(seq: torch.nn.Sequential, x: Tensor, want_rowmax: bool = False) -> Tensor:   # x may be fp16 feature rows; the output is fp32
    """Run an nn.Sequential of Linear / GELU / Dropout(eval) modules with every Linear(+GELU) pair as one launch (or a plain list
    of its modules, some replaced by callables: the scene-graph encoder's weighted BatchNorm; what is no Linear is simply called).
    ``want_rowmax``: the caller feeds the result to another Linear (the last launch's epilogue leaves its row maxima on it)."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, torch.nn.Linear) or (hasattr(m, "weight") and hasattr(m, "bias") and m.weight.dim() == 2):
            fuse = i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.GELU) and mods[i + 1].approximate == "none"
            nxt = i + (2 if fuse else 1)
            more = nxt < len(mods) and hasattr(mods[nxt], "weight") and getattr(mods[nxt].weight, "dim", lambda: 0)() == 2
            if not isinstance(x, Planes32):
                rm = row_maxima(x)
                x = x.contiguous()
                if rm is not None:
                    attach_row_maxima(x, rm)
            tail = want_rowmax and not any(hasattr(t, "weight") and getattr(t.weight, "dim", lambda: 0)() == 2 for t in mods[nxt:]) \
                and all(isinstance(t, torch.nn.Dropout) and not t.training for t in mods[nxt:])   # only identities follow
            rows_in = x.rows if isinstance(x, Planes32) else x.size(0)
            chain = (more and CFG.h3p_chain and not _rec(m.weight, mods[nxt].weight) and not torch.is_grad_enabled() and
                     (isinstance(x, Planes32) or x.dtype == torch.float32) and
                     reads_planes32(rows_in, *m.weight.shape) and reads_planes32(rows_in, *mods[nxt].weight.shape))
            if chain:      # this Linear's result as the planes the next Linear reads: no fp32 intermediate, no split pass
                x = linear_h3p(x, m.weight, m.bias, gelu=fuse, planes_out=True)
            else:
                x = linear(x, m.weight, m.bias, gelu=fuse, want_rowmax=more or tail)      # the epilogue's maxima cost next to nothing
            i = nxt
        else:
            x = m(x)
            i += 1
    return x


SMALL_MLPS_MAX_CHAINS, SMALL_MLPS_MAX_WIDTH = 4, 128       # ISG_SMALL_MLPS_MAX_CHAINS / _MAX_WIDTH of include/isg_fused.h


def small_mlps_supported(M: int, chains, x_dtype=torch.float32, grad: bool = False, cfg: Optional[Switches] = None) -> bool:
    """May isg_small_mlps run these chains over M rows each?  A pure function of plain values.  chains: per chain the (N, K)
    of its one or two Linears, in order.  Yes when: the switch is on; inference on fp32 rows; one to four chains; every width a
    multiple of 32 of at most 128; a second Linear reads what the first wrote; and every Linear is one ops.linear_route sends to
    "bf16x6" at this M -- the kernel whose bits the launch reproduces.  So at M <= 1024 (isg_linear_skinny's regime) and at
    C = 300 nothing changes, and no row's bits depend on this switch."""
    cfg = CFG if cfg is None else cfg
    if not cfg.fuse_question_mlps or grad or x_dtype != torch.float32 or M <= 0:
        return False
    if not 1 <= len(chains) <= SMALL_MLPS_MAX_CHAINS:
        return False
    for chain in chains:
        if not 1 <= len(chain) <= 2 or (len(chain) == 2 and chain[1][1] != chain[0][0]):
            return False
        for N, K in chain:
            if N % 32 or K % 32 or not (32 <= N <= SMALL_MLPS_MAX_WIDTH and 32 <= K <= SMALL_MLPS_MAX_WIDTH):
                return False
            if linear_route(M, N, K, cfg=cfg) != "bf16x6":
                return False
    return True


def _mlp_steps(seq) -> Optional[list]:
    """An nn.Sequential as [(Linear, followed by an exact GELU)], or None when it holds anything but Linear / exact GELU (after a
    Linear) / Dropout in eval mode."""
    steps = []
    for m in seq:
        if isinstance(m, torch.nn.Linear):
            steps.append([m, False])
        elif isinstance(m, torch.nn.GELU) and m.approximate == "none" and steps and not steps[-1][1]:
            steps[-1][1] = True
        elif not (isinstance(m, torch.nn.Dropout) and not m.training):
            return None
    return steps


def _small_mlps_plan(chains):
    """[(nn.Sequential, x)] -> (M, the chains' [(Linear, gelu)] steps) when isg_small_mlps takes them, else None: the tensors'
    facts, then the pure rule."""
    if not chains or not isinstance(chains[0][1], Tensor) or chains[0][1].dim() != 2:
        return None
    x0, grad = chains[0][1], torch.is_grad_enabled()
    M, plan, shapes = x0.size(0), [], []
    for seq, x in chains:
        steps = _mlp_steps(seq)
        if (not steps or not isinstance(x, Tensor) or x.dim() != 2 or not x.is_cuda or x.dtype != torch.float32 or x.size(0) != M
                or x.size(1) != steps[0][0].weight.size(1)
                or any(m.weight.dtype != torch.float32 or m.weight.device != x.device for m, _ in steps)):
            return None
        plan.append(steps)
        shapes.append([tuple(m.weight.shape) for m, _ in steps])
    return (M, plan) if small_mlps_supported(M, shapes, torch.float32, grad) else None


def small_mlps(chains, strict: bool = True) -> Optional[list]:
    """[ops.mlp(seq, x) for seq, x in chains], bit for bit, as ONE launch (isg_small_mlps): up to four narrow MLPs over the same
    number of rows.  Chains that ops.small_mlps_supported refuses raise; with ``strict=False`` the answer is None instead (the
    caller lets every module run its own MLP, as it always did) -- also when the library declines the launch because
    ISG_GEMM_KROT / ISG_GEMM_DUAL_K give isg_linear_bf16x6 another accumulation order."""
    import ctypes
    plan = _small_mlps_plan(chains)
    if plan is None:
        if strict:
            raise ValueError("small_mlps: chains that ops.small_mlps_supported refuses (run them through ops.mlp)")
        return None
    from . import _lib_fused
    lib = _lib_fused.load()
    M, plan = plan
    fields, outs, keep = [], [], []
    for (seq, x), steps in zip(chains, plan):
        x = x.contiguous()
        out = torch.empty(M, steps[-1][0].weight.size(0), dtype=torch.float32, device=x.device)
        row = [_chk(x, "x", torch.float32), x.stride(0), out.data_ptr(), out.stride(0), len(steps)]
        for m, gelu in (steps + steps[:1])[:2]:        # one Linear: the second slot repeats the first (the kernel ignores it)
            N, K = m.weight.shape
            planes = _weight_planes(m.weight, True, "tile")
            row += [planes.data_ptr(), _bias_ptr(m.bias, N), N, K, 1 if gelu else 0]
            keep.append(planes)
        fields += row
        keep.append(x)
        outs.append(out)
    arr = (ctypes.c_int64 * len(fields))(*fields)
    rc = lib.isg_small_mlps(ctypes.addressof(arr), len(chains), M, _stream())
    if rc == ISG_EUNSUPPORTED and not strict:
        return None
    _lib.check(rc, "isg_small_mlps")
    return outs


def fused_weight(weights, biases):
    """(weight, bias) of Linears that share their input, as ONE projection: the weights stacked along the output dim, and the
    biases in a row with zeros for a layer that has none -- None when no layer has one."""
    w = torch.cat(list(weights), dim=0)
    if all(b is None for b in biases):
        return w, None
    return w, torch.cat([torch.zeros(m.size(0), device=w.device) if b is None else b for m, b in zip(weights, biases)])


def linear_fused(x: Tensor, layers, out_dtype=torch.float32) -> Tuple[Tensor, ...]:
    """Several Linear layers that share their input as ONE projection (fused_weight, a derived weight); returns one column-slice
    view of the fused output per layer (row stride = total width)."""
    biases = [m.bias for m in layers if m.bias is not None]
    cat = lambda: fused_weight([m.weight for m in layers], [m.bias for m in layers])
    if _rec(*([] if isinstance(x, Planes32) else [x]), *[m.weight for m in layers]):      # training: differentiable, nothing cached
        y = linear(x, *cat())
    else:
        y = linear(x, *derived_weight("linear_fused", [m.weight for m in layers] + biases, cat), out_dtype=out_dtype)
    outs, o = [], 0
    for m in layers:
        n = m.weight.size(0)
        outs.append(y[:, o:o + n])
        o += n
    return tuple(outs)


# ------------------------------------------------------------------------------------------------
# concat_instr (include/isg_concat.h): cat(x, u[batch]) W^T + b = x W[:, :C]^T + (u W[:, C:]^T + b)[batch]
# ------------------------------------------------------------------------------------------------
def _rowbias_planes(weight: Tensor) -> Tensor:
    """The bf16x6 planes of a weight that is a column slice W[:, :C] of a parameter (or a tensor of its own), cached on the
    tensor the slice is a view of: a slice is a new object at every call, its base is not."""
    base = weight._base if weight._base is not None else weight
    tag = ("rowbias_planes", weight.storage_offset(), tuple(weight.shape), tuple(weight.stride()))
    return derived_weight(tag, (base,), lambda: _split_weight(weight, "tile"))


def segment_rowptr(seg: Tensor, S: int) -> Tensor:
    """int32 [S + 1]: where each segment's rows begin in a non-decreasing seg [M] (a batch vector) -- GraphPlan.ptr of it."""
    return torch.searchsorted(seg, torch.arange(S + 1, dtype=seg.dtype, device=seg.device)).int()


def segment_range_sum(rowptr: Tensor, G: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """out[s] = the sum of G's rows [rowptr[s], rowptr[s + 1]) in row order -> [S, C]  (isg_segment_range_sum: one workgroup per
    segment and block of columns, no atomics).  rowptr: int32 [S + 1], non-decreasing within [0, rows of G] -- a plan's ptr.  G,
    out: fp32 rows with contiguous columns (column slices of wider tensors are fine)."""
    from . import _lib_concat
    S = rowptr.numel() - 1
    if S < 0 or G.dim() != 2:
        raise ValueError(f"segment_range_sum: rowptr of {rowptr.numel()} entries, G {tuple(G.shape)}")
    M, C = G.shape
    if out is None:
        out = torch.empty(S, C, dtype=torch.float32, device=G.device)
    elif tuple(out.shape) != (S, C):
        raise ValueError(f"segment_range_sum: out {tuple(out.shape)}, expected {(S, C)}")
    if S == 0 or C == 0:
        return out
    _lib.check(_lib_concat.load().isg_segment_range_sum(_chk(rowptr, "rowptr", torch.int32), _chk_rows4(G, "G"), _pitch(G),
                                                        _chk_rows4(out, "out"), _pitch(out), S, M, C, _stream()),
               "isg_segment_range_sum")
    return out


def linear_rowbias(x: Tensor, weight: Tensor, P: Tensor, seg: Tensor, gelu: bool = False, relu: bool = False,
                   out_dtype=torch.float32, out: Optional[Tensor] = None, rowptr: Optional[Tensor] = None,
                   cache_planes: bool = True) -> Tensor:
    """act(x @ weight^T + P[seg]): x [M, K] fp32 rows, weight [N, K] (a column slice W[:, :K] of a parameter, or a tensor of its
    own), P [S, N] fp32 with contiguous columns (a column slice of a wider tensor is fine), seg int32 [M] with values in [0, S) --
    one launch of isg_linear_bf16x6_rowbias, whose epilogue adds the row P[seg[m]] where isg_linear_bf16x6 adds the bias.
    out_dtype = torch.float16: the result rounded once to half rows.  out: [M, N] rows of out_dtype to write (a column slice of a
    wider tensor).  Under autograd it is autograd.linear_rowbias (fp32 only; seg non-decreasing; rowptr: int32 [S + 1], where
    each segment's rows begin -- a plan's ptr -- derived from seg when it is not given)."""
    if relu and gelu:
        raise ValueError("relu excludes gelu")
    if x.dim() != 2 or weight.dim() != 2 or P.dim() != 2 or weight.size(1) != x.size(1) or P.size(1) != weight.size(0):
        raise ValueError(f"linear_rowbias: x {tuple(x.shape)}, weight {tuple(weight.shape)}, P {tuple(P.shape)}")
    M, K = x.shape
    N, S = weight.size(0), P.size(0)
    if seg.dtype != torch.int32 or seg.dim() != 1 or seg.numel() != M:
        raise ValueError(f"linear_rowbias: seg is int32 [{M}], got {seg.dtype} {tuple(seg.shape)}")
    if torch.is_grad_enabled() and _rec(x, weight, P):
        if out_dtype != torch.float32 or out is not None:
            raise _lib.IsgError("linear_rowbias: training a concat_instr layer on half rows (or into a caller's rows) is not "
                                "supported; the row-biased Linear differentiates fp32 rows only")
        from . import autograd
        return autograd.linear_rowbias(x, weight, P, seg, gelu, relu, rowptr)
    if CFG.gemm_backend != "bf16x6":
        raise _lib.IsgError("linear_rowbias exists on the bf16x6 kernel only (gemm_backend)")
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=x.device)
    elif out.dtype != out_dtype or tuple(out.shape) != (M, N) or (N > 1 and out.stride(1) != 1) or (M > 1 and out.stride(0) < N):
        raise ValueError(f"linear_rowbias: out is {out_dtype} [{M}, {N}] with contiguous columns, got {out.dtype} {tuple(out.shape)}")
    if M == 0:
        return out
    if S < 1:
        raise ValueError("linear_rowbias: P has no rows")
    from . import _lib_concat
    lib = _lib_concat.load()
    planes = _rowbias_planes(weight) if cache_planes else _split_weight(weight, "tile")
    if not x.is_cuda or not out.is_cuda:
        raise _lib.IsgError(f"x must live on the GPU (got {x.device}); this path has no CPU fallback")
    if x.dtype != torch.float32 or (K > 1 and x.stride(1) != 1):
        raise ValueError("linear_rowbias: x is fp32 rows with contiguous columns")
    COUNTERS["linear_rowbias"] += 1
    _lib.check(lib.isg_linear_bf16x6_rowbias(x.data_ptr(), planes.data_ptr(), _chk_rows4(P.detach(), "P"), _pitch(P), _chk(seg, "seg", torch.int32),
                                             S, out.data_ptr(), 1 if out_dtype == torch.float16 else 0, M, N, K,
                                             max(int(x.stride(0)), K) if M > 1 else K, _pitch(out), 2 if relu else (1 if gelu else 0),
                                             _stream()), "isg_linear_bf16x6_rowbias")
    return out
