"""Training mode of the MPN: the graph operators of PyG / torch_scatter as atomic-free HIP kernels with
hand-written backwards (``csrc/train.hip``), composed by torch autograd with the module's own dense layers.

``train_forward`` is ``NodeClassificationMPNSimple.py:62-97`` with ``layers.py:63-86`` (MPLayer) and
``layers.py:207-274`` (TypeAwareMPNLayer) written with the ``nn`` layers of ``mpn/model.py``: BatchNorm runs on
batch statistics and updates its running statistics, and every parameter keeps its ``state_dict`` key. The three
operators stock torch would run on float atomics are

* ``seg_aggregate``: softmax attention / sum / mean / max per (target node, source type) segment;
* ``gather_pair``: ``(x[dst], x[src])``, whose backward is one per-node sum over both edge lists;
* ``permute_rows``: the per-type bucketing of ``TypeAwareNodeUpdate``, a permutation both ways (pure gathers).

With ``model.fused_edge_update = True`` the edge update ``mlp_edge(cat([x[dst], x[src], ef]))`` runs as one fused
fp32-MFMA operator with a hand-written backward (``edge_update``, ``csrc/train_edge.hip``) next to ``gather_dst``,
in place of ``gather_pair``, the concatenation and the two torch GEMMs. Off by default.

They consume a ``SegmentPlan`` (sorted edge lists + offsets) built once per graph with torch ops and cached on
the model. Results are bitwise reproducible from call to call.
"""
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .. import _lib

KINDS = {"attn": 0, "add": 1, "sum": 1, "mean": 2, "max": 3}     # pemp.h PEMP_AGGR_*
N_TYPE_MLPS = 17                                                 # layers.py:264-271 hard-codes 17 message MLPs


@dataclass
class SegmentPlan:
    """Inverted indices of one graph (int32 on the graph's device; ``src`` / ``dst`` / ``type_src`` int64)."""
    N: int
    E: int
    T: int
    perm_dst: torch.Tensor        # [E] edge ids sorted by (dst, type[src], edge id)
    seg_off: torch.Tensor         # [N T + 1] offsets into perm_dst
    dst_off: torch.Tensor         # [N + 1] seg_off[::T]: the edges into each node
    perm_src: torch.Tensor        # [E] edge ids sorted by (src, edge id)
    src_off: torch.Tensor         # [N + 1]
    src: torch.Tensor             # [E] edge_index[0]
    dst: torch.Tensor             # [E] edge_index[1]
    type_src: torch.Tensor        # [E] type of the source node (zeros for T = 1)
    bucket_perm: Optional[torch.Tensor] = None    # [E] edge ids sorted by (type[src], edge id)   (T > 1)
    bucket_inv: Optional[torch.Tensor] = None     # [E] its inverse
    bucket_sizes: Optional[list] = None           # 17 host ints: edges per source type
    src32: Optional[torch.Tensor] = None          # [E] src as int32 (the fused edge update's ids)
    dst32: Optional[torch.Tensor] = None          # [E] dst as int32


def _offsets(keys, n):
    off = torch.zeros(n + 1, dtype=torch.int64, device=keys.device)
    if keys.numel():
        off[1:] = torch.bincount(keys, minlength=n).cumsum(0)
    return off.to(torch.int32)


def build_plan(edge_index, node_types, N, T):
    """The SegmentPlan of ``edge_index`` [2, E] (row 0 the source, row 1 the target) and the (already summarised)
    ``node_types`` [N]. One stable sort per key, ``bincount`` and ``cumsum``: deterministic. With T > 1 the
    per-type edge buckets of ``TypeAwareNodeUpdate`` are part of the plan; their sizes are the one host read."""
    N, T = int(N), int(T)
    if T < 1:
        raise ValueError(f"build_plan: T = {T} < 1")
    src, dst = edge_index[0].long(), edge_index[1].long()
    E = src.numel()
    if E >= 2 ** 31 or N * T >= 2 ** 31 - 1:
        raise ValueError(f"build_plan: E = {E}, N T = {N * T} exceed the kernels' int32 indices")
    dev = src.device
    type_src = node_types.long().reshape(-1)[src] if T > 1 else torch.zeros(E, dtype=torch.int64, device=dev)
    plan = SegmentPlan(N, E, T, None, None, None, None, None, src, dst, type_src)
    # the one host read per graph: the index ranges (a plan is never built over ids it cannot hold) and, for the
    # type-aware layer, the edges per source type
    nb = max(T, N_TYPE_MLPS)
    if E:
        counts = torch.bincount(type_src.clamp(0, nb), minlength=nb + 1)
        host = torch.cat([torch.stack([src.min(), src.max(), dst.min(), dst.max(), type_src.min()]), counts]).tolist()
    else:
        host = [0] * (5 + nb + 1)
    lo, hi, sizes = min(host[0], host[2]), max(host[1], host[3]), host[5:]
    if E and (lo < 0 or hi >= N):
        raise ValueError(f"build_plan: edge_index holds node ids outside [0, {N})")
    if host[4] < 0 or any(sizes[T:]):
        raise ValueError(f"build_plan: node types outside [0, {T})")
    if T > 1:
        order = torch.sort(type_src, stable=True).indices
        plan.bucket_sizes = sizes[:N_TYPE_MLPS]
        plan.bucket_perm = order
        plan.bucket_inv = torch.empty_like(order)
        plan.bucket_inv[order] = torch.arange(E, device=dev)
    key = dst * T + type_src
    plan.perm_dst = torch.sort(key, stable=True).indices.to(torch.int32)
    plan.seg_off = _offsets(key, N * T)
    plan.dst_off = plan.seg_off[::T].contiguous()
    plan.perm_src = torch.sort(src, stable=True).indices.to(torch.int32)
    plan.src_off = _offsets(src, N)
    plan.src32, plan.dst32 = src.to(torch.int32), dst.to(torch.int32)
    return plan


def cached_plan(model, edge_index, node_types, N, T):
    """The model's plan of this graph: rebuilt when edge_index / node_types are other tensors (or other views) or
    were written since (``_version``), like the ``_sym_graph`` / ``_knn_graph`` tags. One plan per model. The node
    types are summarised (NODE_TYPE_SUMMARY) only when a plan is built."""
    def ident(t):
        return (t.data_ptr(), tuple(t.shape), t.stride(), t.dtype, t.device, t._version)
    key = (ident(edge_index), ident(node_types), N, T)
    hit = getattr(model, "_train_plan", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    types = node_types
    if T > 1 and model.node_summary != "not":
        from .model import TYPE_LUTS
        types = torch.tensor(TYPE_LUTS[model.node_summary], device=node_types.device)[node_types.long()]
    plan = build_plan(edge_index, types, N, T)
    model._train_plan = (key, plan, edge_index, node_types)      # the tensors are held: their storage is not reused
    return plan


def _device_f32(name, t):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{name}: expected a float32 tensor (got {getattr(t, 'dtype', type(t))})")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: pemp_amd runs on the HIP device only (no CPU fallback)")
    return t if t.is_contiguous() else t.contiguous()


def _same_device(name, plan, t):
    if plan.perm_dst.device != t.device:      # the kernels would follow host pointers
        raise RuntimeError(f"{name}: the plan lies on {plan.perm_dst.device}, the rows on {t.device}")


class _SegAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, msgs, scores, plan, kind):
        L = _lib.lib()
        msgs = _device_f32("seg_aggregate msgs", msgs)
        _same_device("seg_aggregate", plan, msgs)
        if msgs.dim() != 2 or msgs.shape != (plan.E, 64):
            raise ValueError(f"seg_aggregate: msgs {tuple(msgs.shape)}, expected ({plan.E}, 64)")
        if kind == 0:
            if scores is None:
                raise ValueError("seg_aggregate: attention needs scores")
            scores = _device_f32("seg_aggregate scores", scores)
            if scores.shape != (plan.E,) or scores.device != msgs.device:
                raise ValueError(f"seg_aggregate: scores {tuple(scores.shape)}, expected ({plan.E},)")
        elif kind not in (1, 2, 3):
            raise ValueError(f"seg_aggregate: unknown kind {kind}")
        else:
            scores = None
        dev = msgs.device
        out = torch.empty(plan.N * plan.T, 64, dtype=torch.float32, device=dev)
        alpha = torch.empty(plan.E, dtype=torch.float32, device=dev) if kind == 0 else None
        arg = torch.empty(plan.N * plan.T, 64, dtype=torch.int32, device=dev) if kind == 3 else None
        _lib.check(L.pemp_seg_aggr_fwd(kind, plan.T, plan.N, plan.E, _lib.ptr(msgs), _lib.ptr(scores),
                                       plan.perm_dst.data_ptr(), plan.seg_off.data_ptr(), out.data_ptr(),
                                       _lib.ptr(alpha), _lib.ptr(arg), _lib.stream(dev)))
        ctx.plan, ctx.kind = plan, kind
        ctx.save_for_backward(*(t for t in ((msgs, alpha) if kind == 0 else (arg,) if kind == 3 else ())))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        L = _lib.lib()
        plan, kind = ctx.plan, ctx.kind
        g = _device_f32("seg_aggregate grad", grad_out)
        msgs = alpha = arg = None
        if kind == 0:
            msgs, alpha = ctx.saved_tensors
        elif kind == 3:
            arg, = ctx.saved_tensors
        gm = torch.empty(plan.E, 64, dtype=torch.float32, device=g.device)
        gs = torch.empty(plan.E, dtype=torch.float32, device=g.device) if kind == 0 else None
        _lib.check(L.pemp_seg_aggr_bwd(kind, plan.T, plan.N, plan.E, g.data_ptr(), _lib.ptr(msgs), _lib.ptr(alpha),
                                       None, _lib.ptr(arg), plan.perm_dst.data_ptr(),
                                       plan.seg_off.data_ptr(), gm.data_ptr(), _lib.ptr(gs), _lib.stream(g.device)))
        return gm, gs, None, None


class _GatherPair(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan):
        _lib.lib()
        x = _device_f32("gather_pair x", x)
        _same_device("gather_pair", plan, x)
        if x.dim() != 2 or x.shape[0] != plan.N or x.shape[1] not in (64, 128):
            raise ValueError(f"gather_pair: x {tuple(x.shape)}, expected ({plan.N}, 64 or 128)")
        ctx.plan, ctx.W = plan, x.shape[1]
        return x.index_select(0, plan.dst), x.index_select(0, plan.src)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_i, grad_j):
        L = _lib.lib()
        plan = ctx.plan
        gi = _device_f32("gather_pair grad", grad_i)
        gj = _device_f32("gather_pair grad", grad_j)
        out = torch.empty(plan.N, ctx.W, dtype=torch.float32, device=gi.device)
        _lib.check(L.pemp_seg_rows_sum(plan.N, plan.E, ctx.W, gi.data_ptr(), plan.perm_dst.data_ptr(),
                                       plan.dst_off.data_ptr(), gj.data_ptr(), plan.perm_src.data_ptr(),
                                       plan.src_off.data_ptr(), out.data_ptr(), _lib.stream(gi.device)))
        return out, None


class _GatherDst(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan):
        _lib.lib()
        x = _device_f32("gather_dst x", x)
        _same_device("gather_dst", plan, x)
        if x.dim() != 2 or x.shape[0] != plan.N or x.shape[1] not in (64, 128):
            raise ValueError(f"gather_dst: x {tuple(x.shape)}, expected ({plan.N}, 64 or 128)")
        ctx.plan, ctx.W = plan, x.shape[1]
        return x.index_select(0, plan.dst)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return _rows_sum(ctx.plan, _device_f32("gather_dst grad", grad), ctx.W, by_dst=True), None


def _rows_sum(plan, rows, W, by_dst):
    """[N, W]: the rows [E, W] summed per target (by_dst) or per source node, in list order."""
    out = torch.empty(plan.N, W, dtype=torch.float32, device=rows.device)
    perm, off = (plan.perm_dst, plan.dst_off) if by_dst else (plan.perm_src, plan.src_off)
    _lib.check(_lib.lib().pemp_seg_rows_sum(plan.N, plan.E, W, rows.data_ptr(), perm.data_ptr(), off.data_ptr(), None,
                                            None, None, out.data_ptr(), _lib.stream(rows.device)))
    return out


_EDGE_WS = _lib.Workspace()      # the weight-gradient partials of pemp_edge_mlp_bwd (per device and stream)


class _EdgeMlp(torch.autograd.Function):
    """e_new = relu(relu(P[dst] + Q[src] + ef C^T) W2^T + b2) (pemp.h pemp_edge_mlp_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, P, Q, ef, C, W2, b2, plan):
        L = _lib.lib()
        P, Q, ef = _device_f32("edge_update P", P), _device_f32("edge_update Q", Q), _device_f32("edge_update ef", ef)
        C, W2, b2 = _device_f32("edge_update C", C), _device_f32("edge_update W2", W2), _device_f32("edge_update b2", b2)
        _same_device("edge_update", plan, ef)
        if plan.src32 is None or plan.dst32 is None:
            raise ValueError("edge_update: the plan carries no src32 / dst32 (build it with build_plan)")
        We = ef.shape[1] if ef.dim() == 2 else -1
        if ef.dim() != 2 or ef.shape[0] != plan.E or We not in (64, 128):
            raise ValueError(f"edge_update: ef {tuple(ef.shape)}, expected ({plan.E}, 64 or 128)")
        if P.shape != (plan.N, 64) or Q.shape != (plan.N, 64):
            raise ValueError(f"edge_update: P {tuple(P.shape)}, Q {tuple(Q.shape)}, expected ({plan.N}, 64)")
        if C.shape != (64, We) or W2.shape != (64, 64) or b2.shape != (64,):
            raise ValueError(f"edge_update: C {tuple(C.shape)}, W2 {tuple(W2.shape)}, b2 {tuple(b2.shape)}, expected "
                             f"(64, {We}), (64, 64), (64,)")
        for name, t in (("P", P), ("Q", Q), ("C", C), ("W2", W2), ("b2", b2)):
            if t.device != ef.device:
                raise RuntimeError(f"edge_update: {name} lies on {t.device}, ef on {ef.device}")
        h = torch.empty(plan.E, 64, dtype=torch.float32, device=ef.device)
        e_new = torch.empty(plan.E, 64, dtype=torch.float32, device=ef.device)
        _lib.check(L.pemp_edge_mlp_fwd(plan.N, plan.E, We, P.data_ptr(), Q.data_ptr(), ef.data_ptr(),
                                       plan.src32.data_ptr(), plan.dst32.data_ptr(), C.data_ptr(), W2.data_ptr(),
                                       b2.data_ptr(), h.data_ptr(), e_new.data_ptr(), _lib.stream(ef.device)))
        ctx.plan, ctx.We = plan, We
        ctx.save_for_backward(ef, h, e_new, C, W2)
        return e_new

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        L = _lib.lib()
        plan, We = ctx.plan, ctx.We
        ef, h, e_new, C, W2 = ctx.saved_tensors
        g = _device_f32("edge_update grad", grad)
        dev = g.device
        g1 = torch.empty(plan.E, 64, dtype=torch.float32, device=dev)
        g_ef = torch.empty(plan.E, We, dtype=torch.float32, device=dev)
        dC = torch.empty(64, We, dtype=torch.float32, device=dev)
        dW2 = torch.empty(64, 64, dtype=torch.float32, device=dev)
        db2 = torch.empty(64, dtype=torch.float32, device=dev)
        nbytes = L.pemp_edge_mlp_workspace_size(plan.E, We)
        ws = _EDGE_WS.get(nbytes, dev)
        _lib.check(L.pemp_edge_mlp_bwd(plan.N, plan.E, We, g.data_ptr(), ef.data_ptr(), h.data_ptr(), e_new.data_ptr(),
                                       C.data_ptr(), W2.data_ptr(), g1.data_ptr(), g_ef.data_ptr(), dC.data_ptr(),
                                       dW2.data_ptr(), db2.data_ptr(), ws.data_ptr(), nbytes, _lib.stream(dev)))
        need = ctx.needs_input_grad
        dP = _rows_sum(plan, g1, 64, by_dst=True) if need[0] else None
        dQ = _rows_sum(plan, g1, 64, by_dst=False) if need[1] else None
        return dP, dQ, g_ef if need[2] else None, dC if need[3] else None, dW2 if need[4] else None, \
            db2 if need[5] else None, None


class _PermuteRows(torch.autograd.Function):
    """rows[perm] whose backward is grad[inv] (perm a permutation, inv its inverse): a gather both ways."""

    @staticmethod
    def forward(ctx, rows, perm, inv):
        ctx.inv = inv
        return rows.index_select(0, perm)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return grad.index_select(0, ctx.inv), None, None


def seg_aggregate(msgs, scores, plan, kind):
    """[N T, 64]: the ``kind`` ("attn" | "add" | "mean" | "max" or a PEMP_AGGR_* code) aggregate of the message rows
    ``msgs`` [E, 64] per (target, source type) segment of ``plan``; ``scores`` [E] are the attention logits
    ("attn" only). fp32 HIP tensors; differentiable in msgs and scores."""
    return _SegAggregate.apply(msgs, scores, plan, KINDS[kind] if isinstance(kind, str) else int(kind))


def gather_pair(x, plan):
    """(x[dst], x[src]) for node rows x [N, 64 | 128]; the backward sums both gradients per node in one kernel."""
    return _GatherPair.apply(x, plan)


def gather_dst(x, plan):
    """x[dst] for node rows x [N, 64 | 128]; the backward sums the gradient rows per target node."""
    return _GatherDst.apply(x, plan)


def edge_update(nf, ef, plan, mlp_edge):
    """``mlp_edge(cat([nf[dst], nf[src], ef]))`` [E, 64] without the gathers and the concatenation, for the agnostic
    ``mlp_edge`` = Linear(2 Wn + We -> 64), ReLU, Linear(64 -> 64), ReLU; nf [N, Wn], ef [E, We], We in (64, 128).
    The first layer's weight is split by columns, W1 = [A | B | C]: the node tables P = nf A^T + b1 and Q = nf B^T
    are torch ops (autograd gives the gradients of A, B, b1 and nf), the per-edge rest is one fused kernel each way.
    fp32 HIP tensors; differentiable in nf, ef and the four parameters."""
    lin1, lin2 = mlp_edge[0], mlp_edge[2]
    Wn = nf.shape[1] if nf.dim() == 2 else -1
    if ef.dim() != 2 or lin1.in_features != 2 * Wn + ef.shape[1] or lin1.out_features != 64 or \
            (lin2.in_features, lin2.out_features) != (64, 64):
        raise ValueError(f"edge_update: mlp_edge {lin1.in_features} -> {lin1.out_features} -> {lin2.out_features} "
                         f"does not fit nf {tuple(nf.shape)}, ef {tuple(ef.shape)}")
    nf = _device_f32("edge_update nf", nf)
    W1 = lin1.weight
    P = F.linear(nf, W1[:, :Wn], lin1.bias)
    Q = F.linear(nf, W1[:, Wn:2 * Wn])
    return _EdgeMlp.apply(P, Q, ef, W1[:, 2 * Wn:], lin2.weight, lin2.bias, plan)


def permute_rows(rows, perm, inv):
    return _PermuteRows.apply(rows, perm, inv)


# ------------------------------------------------------------------------------------------------------------
def refuse_unsupported(model):
    """Options that run in eval only."""
    from .model import LateFusionEdgeMLP
    layer = model.mpn_node_cls
    if getattr(layer, "edge_mlp", "agnostic") == "per_type":
        raise NotImplementedError("pemp_amd MPN training: EDGE_MLP per_type is not built (eval only)")
    if getattr(layer, "update_type", "mlp") != "mlp":
        raise NotImplementedError(f"pemp_amd MPN training: UPDATE_TYPE {layer.update_type} is not built (eval only)")
    if isinstance(model.edge_embedding, LateFusionEdgeMLP):
        raise NotImplementedError("pemp_amd MPN training: LATE_FUSION_POS is not built (eval only)")


def _type_aware_messages(mlp_node, xi_e, plan):
    """TypeAwareNodeUpdate.forward (layers.py:268-274) over the plan's per-type buckets: no mask, no host sync."""
    rows = permute_rows(xi_e, plan.bucket_perm, plan.bucket_inv)
    outs = [mlp_node.mlp[t](chunk) for t, chunk in enumerate(rows.split(plan.bucket_sizes)) if chunk.shape[0]]
    if not outs:
        return xi_e.new_zeros(0, mlp_node.output_dim)
    return permute_rows(torch.cat(outs, 0), plan.bucket_inv, plan.bucket_perm)


def _layer(model, layer, plan, nf, ef):
    if getattr(model, "fused_edge_update", False):                    # x[src] is never materialised
        x_i = gather_dst(nf, plan)
        e_new = edge_update(nf, ef, plan, layer.mlp_edge)
    else:
        x_i, x_j = gather_pair(nf, plan)
        e_new = layer.mlp_edge(torch.cat([x_i, x_j, ef], dim=1))
    xi_e = torch.cat([x_i, e_new], dim=1)
    if plan.T == 1:                                                   # MPLayer (layers.py:63-86)
        agg = seg_aggregate(layer.mlp_node(xi_e), None, plan, model.aggr_code)
        if layer.update_mlp is not None:
            agg = layer.update_mlp(agg)
        return agg, e_new
    msgs = _type_aware_messages(layer.mlp_node, xi_e, plan)          # TypeAwareMPNLayer (layers.py:207-258)
    scores = None
    if model.aggr_code == 0:
        scores = layer.attn_net(e_new)
        if layer.aggr_sub == "node_edge_attn_per_type":               # score column type[src] (layers.py:245-249)
            scores = scores.gather(1, plan.type_src[:, None])
        scores = scores.reshape(-1)
    agg = seg_aggregate(msgs, scores, plan, model.aggr_code)
    return layer.update_mlp(agg.reshape(plan.N, -1)), e_new


def train_forward(model, x, edge_attr, edge_index, node_types):
    """``NodeClassificationMPNSimple.forward`` in training mode; the tuple and list lengths of the eval path."""
    from .model import _rows
    refuse_unsupported(model)
    if x.device.type != "cuda":
        raise RuntimeError("pemp_amd MPN runs on the HIP device only (no CPU fallback)")
    if x.dtype != torch.float32 or edge_attr.dtype != torch.float32:
        raise TypeError(f"pemp_amd MPN training: x / edge_attr must be float32 (got {x.dtype}, {edge_attr.dtype})")
    _lib.lib()
    for name, t in (("edge_attr", edge_attr), ("edge_index", edge_index), ("node_types", node_types)):
        if t.device != x.device:
            raise RuntimeError(f"pemp_amd MPN training: {name} lies on {t.device}, x on {x.device}")
    N = x.shape[0]
    plan = cached_plan(model, edge_index, node_types, N, model.num_types)
    nf = model.node_embedding(x)
    ef = model.edge_embedding(edge_attr)
    nf0, ef0 = nf, ef
    steps, aux = model.edge_steps, model.aux_loss_steps
    edge_cols, node_cols, preds_class = [], [], []
    for i in range(steps):
        if model.use_skip_connections:
            nf = torch.cat([nf0, nf], dim=1)
            ef = torch.cat([ef0, ef], dim=1)
        nf, ef = _layer(model, model.mpn_node_cls, plan, nf, ef)
        if i >= steps - aux - 1:
            node_cols.append(model.node_classification(nf))
            preds_class.append(model.classification(nf))
            edge_cols.append(model.edge_classification(ef))
    node_cols.append(model.node_classification(nf))
    preds_class.append(model.classification(nf))
    preds_edge = _rows(torch.stack([c.reshape(-1) for c in edge_cols]), len(edge_cols)) if edge_cols else []
    preds_node = _rows(torch.stack([c.reshape(-1) for c in node_cols]), len(node_cols))
    return preds_edge, preds_node, preds_class, [None]
