"""The node features as a differentiable read of the maps they come from (``csrc/node_grad.hip``, ``pemp.h``
pemp_node_*): the reference's ``x = features[:, joint_y, joint_x].T`` (``ConstructGraph.py:262-269``) carries the MPN's
gradient for ``x`` back into ``feature_gather`` and the backbone (``PoseEstimation.py:76-93``, ``train.py:232``).

* ``gather_nodes(features, joint_det, batch_index)``: ``x[n] = features[b_n, :, y_n, x_n]`` for dense features
  ``[B, C, H, W]``; the backward scatters ``g`` into a zero map, the nodes of one pixel added in ascending node index.
* ``gather_nodes_conv(raw, conv, joint_det, batch_index)``: ``x[n] = conv(raw)[b_n, :, y_n, x_n]`` with the conv
  evaluated under the nodes only, forward (``pemp_gather_projected_conv``) and backward (``pemp_node_conv_bwd``):
  gradients for ``raw``, ``conv.weight`` and ``conv.bias``, each computed only when asked for.
* ``PixelPlan``: the sorted pixel keys of a node set, made once per graph with torch ops on the device (no host read).

``construct_graph`` attaches the same two functions to the ``x`` it has filled already (``graph_constructor._finish``)
whenever the features require a gradient. Both backwards are atomic-free and bitwise reproducible; ``joint_det``,
``batch_index``, ``raw`` and the weight go through ``save_for_backward``, so an in-place edit before the backward is
caught.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib


class PixelPlan:
    """For the nodes ``joint_det [N, 3]`` (x, y, type) / ``batch_index [N]`` on maps ``[B, ., h, w]`` and a k x k
    window with padding ``pad`` under each: the entry ``(n, dy, dx)`` lands on pixel ``(b, y - pad + dy, x - pad + dx)``
    and gets the key ``(b h + yy) w + xx``, or the sentinel ``B h w`` outside the map. ``keys`` are the keys in
    ascending order, ``perm`` the entry of every sorted position; the sort is stable, so the entries of one pixel stay
    in ascending ``(n, dy, dx)``."""

    def __init__(self, joint_det, batch_index, B, h, w, k=1, pad=0):
        dev = joint_det.device
        d = torch.arange(k, device=dev, dtype=torch.int64) - pad
        yy = joint_det[:, 1].view(-1, 1, 1) + d.view(1, k, 1)
        xx = joint_det[:, 0].view(-1, 1, 1) + d.view(1, 1, k)
        b = batch_index.view(-1, 1, 1)
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w) & (b >= 0) & (b < B)
        key = torch.where(ok, (b * h + yy) * w + xx, B * h * w).reshape(-1)
        self.keys, self.perm = torch.sort(key, stable=True)
        self.args = (B, h, w, k, pad, joint_det.shape[0])


def _nodes(joint_det, batch_index, dev):
    for name, t, shape in (("joint_det", joint_det, (-1, 3)), ("batch_index", batch_index, (-1,))):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
            raise TypeError(f"{name}: expected an int64 tensor (got {getattr(t, 'dtype', type(t))})")
        if t.device != dev:
            raise RuntimeError(f"{name} lies on {t.device}, the maps on {dev}")
        if t.dim() != len(shape) or (len(shape) == 2 and t.shape[1] != 3):
            raise ValueError(f"{name}: shape {tuple(t.shape)}")
    if joint_det.shape[0] != batch_index.shape[0]:
        raise ValueError(f"joint_det has {joint_det.shape[0]} rows, batch_index {batch_index.shape[0]}")
    return joint_det.contiguous(), batch_index.contiguous()


def _maps(name, t):
    """[B, C, h, w] on the HIP device as fp32 contiguous, by ordinary torch ops (the gradient flows through them)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise TypeError(f"{name}: expected a [B, C, h, w] tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name}: pemp_amd runs on the HIP device only (no CPU fallback)")
    return t.float().contiguous()


def _one_map(t):
    vp = ctypes.c_void_p
    return (ctypes.cast((vp * 1)(t.data_ptr()), vp), ctypes.cast((ctypes.c_int32 * 1)(t.shape[2]), vp),
            ctypes.cast((ctypes.c_int32 * 1)(t.shape[3]), vp))


class _GatherNodes(torch.autograd.Function):
    """x_filled: the x a build has written already (returned as it is), or None (pemp_gather_projected reads it)."""

    @staticmethod
    def forward(ctx, features, joint_det, batch_index, x_filled, plan):
        B, C, H, W = features.shape
        N = joint_det.shape[0]
        if x_filled is None:
            x = torch.empty(N, C, dtype=torch.float32, device=features.device)
            _lib.check(_lib.lib().pemp_gather_projected(*_one_map(features), 1, C, H, W, 1.0, _lib.ptr(joint_det),
                                                        _lib.ptr(batch_index), N, _lib.ptr(x),
                                                        _lib.stream(features.device)))
        else:
            x = x_filled.detach()
        ctx.save_for_backward(joint_det, batch_index)
        ctx.shape, ctx.plan = (B, C, H, W), plan
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        joint_det, batch_index = ctx.saved_tensors
        B, C, H, W = ctx.shape
        N = joint_det.shape[0]
        plan = ctx.plan or PixelPlan(joint_det, batch_index, B, H, W)
        g = g.float().contiguous()
        dfeat = torch.empty(B, C, H, W, dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().pemp_node_grad_pixels(_lib.ptr(g), N, C, _lib.ptr(plan.keys), _lib.ptr(plan.perm), B, H, W,
                                                    _lib.ptr(dfeat), _lib.stream(g.device)))
        return dfeat, None, None, None, None


class _GatherNodesConv(torch.autograd.Function):
    """weight_t: the weight as the forward's [Cin, k, k, Cout] (or None: made here); x_filled as in _GatherNodes."""

    @staticmethod
    def forward(ctx, raw, weight, bias, joint_det, batch_index, pad, x_filled, weight_t, plan):
        B, Cin, h, w = raw.shape
        Cout, k = weight.shape[0], weight.shape[2]
        N = joint_det.shape[0]
        if x_filled is None:
            if weight_t is None:
                weight_t = weight.detach().permute(1, 2, 3, 0).contiguous()
            x = torch.empty(N, Cout, dtype=torch.float32, device=raw.device)
            _lib.check(_lib.lib().pemp_gather_projected_conv(
                *_one_map(raw), 1, Cin, _lib.ptr(weight_t), _lib.ptr(bias), Cout, k, pad, h + 2 * pad - k + 1,
                w + 2 * pad - k + 1, 1.0, _lib.ptr(joint_det), _lib.ptr(batch_index), N, _lib.ptr(x),
                _lib.stream(raw.device)))
        else:
            x = x_filled.detach()
        ctx.save_for_backward(raw, weight, joint_det, batch_index)
        ctx.pad, ctx.has_bias, ctx.plan = pad, bias is not None, plan
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        raw, weight, joint_det, batch_index = ctx.saved_tensors
        B, Cin, h, w = raw.shape
        Cout, k, pad = weight.shape[0], weight.shape[2], ctx.pad
        N, dev = joint_det.shape[0], raw.device
        need_raw, need_w, need_b = ctx.needs_input_grad[:3]
        need_b = need_b and ctx.has_bias
        L = _lib.lib()
        g = g.float().contiguous()
        draw = torch.empty_like(raw) if need_raw else None
        dW = torch.empty(Cout, Cin, k, k, dtype=torch.float32, device=dev) if need_w else None
        db = torch.empty(Cout, dtype=torch.float32, device=dev) if need_b else None
        plan = w2 = None
        if need_raw:
            plan = ctx.plan or PixelPlan(joint_det, batch_index, B, h, w, k, pad)
            w2 = weight.permute(0, 2, 3, 1).contiguous()       # [Cout, k, k, Cin]: D's rows are [k k][Cin]
        ws = torch.empty(max(int(L.pemp_node_conv_workspace_size(N, Cin, Cout, k)), 256), dtype=torch.uint8, device=dev)
        _lib.check(L.pemp_node_conv_bwd(_lib.ptr(g), _lib.ptr(raw), _lib.ptr(w2), _lib.ptr(joint_det),
                                        _lib.ptr(batch_index), N, B, Cin, h, w, Cout, k, pad,
                                        None if plan is None else _lib.ptr(plan.keys),
                                        None if plan is None else _lib.ptr(plan.perm), _lib.ptr(draw), _lib.ptr(dW),
                                        _lib.ptr(db), _lib.ptr(ws), ws.numel(), _lib.stream(dev)))
        return draw, dW, db, None, None, None, None, None, None


def conv_geometry(conv):
    """(k, pad) of a Conv2d the sparse path takes (the forward's conditions, frontend.ProjectedMaps), else raises."""
    if not isinstance(conv, torch.nn.Conv2d):
        raise TypeError("gather_nodes_conv: conv must be an nn.Conv2d (the model's feature_gather)")
    k, pad = conv.kernel_size, conv.padding
    if (isinstance(pad, str) or k[0] != k[1] or pad[0] != pad[1] or tuple(conv.stride) != (1, 1)
            or tuple(conv.dilation) != (1, 1) or conv.groups != 1 or conv.padding_mode != "zeros"
            or not 1 <= k[0] <= 7 or not 0 <= pad[0] < k[0]):
        raise NotImplementedError("gather_nodes_conv: the conv must be stride 1, dilation 1, groups 1, square kernel "
                                  "<= 7 with symmetric zero padding < kernel")
    if conv.out_channels > 512:
        raise NotImplementedError("gather_nodes_conv: more than 512 output channels")
    return k[0], pad[0]


def _check_plan(plan, B, h, w, k, pad, N):
    if plan is not None and plan.args != (B, h, w, k, pad, N):
        raise ValueError(f"PixelPlan was made for (B, h, w, k, pad, N) = {plan.args}, the call has {(B, h, w, k, pad, N)}")


def gather_nodes(features, joint_det, batch_index, plan=None):
    """x [N, C] = features[batch_index, :, joint_det[:, 1], joint_det[:, 0]], differentiable in ``features``."""
    features = _maps("features", features)
    joint_det, batch_index = _nodes(joint_det, batch_index, features.device)
    B, _, H, W = features.shape
    _check_plan(plan, B, H, W, 1, 0, joint_det.shape[0])
    return _GatherNodes.apply(features, joint_det, batch_index, None, plan)


def gather_nodes_conv(raw, conv, joint_det, batch_index, plan=None):
    """x [N, Cout] = conv(raw)[batch_index, :, joint_det[:, 1], joint_det[:, 0]] with the conv evaluated under the
    nodes only; differentiable in ``raw``, ``conv.weight`` and ``conv.bias``."""
    k, pad = conv_geometry(conv)
    raw = _maps("raw", raw)
    if raw.shape[1] != conv.in_channels:
        raise ValueError(f"gather_nodes_conv: conv expects {conv.in_channels} channels, raw has {raw.shape[1]}")
    joint_det, batch_index = _nodes(joint_det, batch_index, raw.device)
    weight = conv.weight.float().contiguous()
    bias = None if conv.bias is None else conv.bias.float().contiguous()
    B, _, h, w = raw.shape
    _check_plan(plan, B, h, w, k, pad, joint_det.shape[0])
    return _GatherNodesConv.apply(raw, weight, bias, joint_det, batch_index, pad, None, None, plan)
