"""The MPN training loss on the device: the node, edge and class terms of the reference's ``ClassMPNLossFactory``
(``Utils/loss.py:785-862``) and the same part of ``ClassMultiLossFactory`` (``:606-621, 668-689``), with the graph
reduction ``train.py:104-112, 140-154`` prepares for them, as one fused HIP pass each way (``csrc/loss.hip``,
``pemp.h`` pemp_loss_*).

* ``mpn_loss(...)``: the functional form, ``(total, terms)``; one ``torch.autograd.Function``.
* ``MPNLoss(config)``: an ``nn.Module`` over ``construct_graph``'s 15-tuple and the model's output tuple.
* ``ClassMPNLossFactory(config)``: the reference's ``forward(outputs, labels, masks) -> (loss, logging)``; the
  per-prediction masks arrive in ``masks["edge"]``.
* ``mask_node_connections(...)``: the reference's function, for callers that keep their own loop.

The forward is two launches (the pass and a one-block fixed-order reduction in fp64), the backward one; neither
synchronises the host. ``terms`` = (node, edge, class, total) stays on the device: a caller that logs reads it once.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .mpn.train import _device_f32

TERM_NAMES = {"node": _lib.LOSS_TERM_NODE, "edge": _lib.LOSS_TERM_EDGE, "class": _lib.LOSS_TERM_CLASS}
DEFAULTS = dict(USE_FOCAL=True, EDGE_WITH_LOGITS=True, NODE_USE_FOCAL=True, FOCAL_ALPHA=1.0, FOCAL_GAMMA=2.0,
                NODE_BCE_POS_WEIGHT=1.0, EDGE_BCE_POS_WEIGHT=1.0, INCLUDE_BORDERING_NODES=False, NODE_WEIGHT=1.0,
                EDGE_WEIGHT=1.0, CLASS_WEIGHT=1.0, NODE_THRESHOLD=1.0, TERMS=("node", "edge", "class"))
_WS = _lib.Workspace()      # the forward's block partials (per device and stream)


def loss_options(cfg_or_kwargs=None, **over):
    """The loss's options as a plain dict (``DEFAULTS`` keys) from a config (``MODEL.LOSS.*`` +
    ``MODEL.MPN.NODE_THRESHOLD``; ``LOSS.LOSS_WEIGHTS`` of length 2 or 3, when set, gives the weights as
    ``ClassMPNLossFactory`` reads them, ``:857-859``), a ``MODEL.LOSS`` node, or keyword options."""
    opt = dict(DEFAULTS)
    src = cfg_or_kwargs
    if src is not None:
        if "MODEL" in src:
            th = src["MODEL"].get("MPN", {}).get("NODE_THRESHOLD")
            if th is not None:
                opt["NODE_THRESHOLD"] = th
            src = src["MODEL"].get("LOSS", {})
        for k, v in src.items():
            if k in opt:
                opt[k] = v
        lw = src.get("LOSS_WEIGHTS")
        if lw is not None:
            if len(lw) not in (2, 3):
                raise ValueError(f"LOSS.LOSS_WEIGHTS has {len(lw)} entries (2 or 3)")
            opt["NODE_WEIGHT"], opt["EDGE_WEIGHT"] = lw[0], lw[1]
            opt["CLASS_WEIGHT"] = lw[2] if len(lw) == 3 else 1.0
    for k, v in over.items():
        if k not in opt:
            raise TypeError(f"mpn_loss: unknown option {k}")
        opt[k] = v
    return opt


def _refusals(opt, K_e, K_n, J):
    """The limits and the variants that are not built; raised before the library is touched."""
    if not opt["USE_FOCAL"] and not opt["EDGE_WITH_LOGITS"]:
        raise NotImplementedError("pemp_amd loss: EDGE_WITH_LOGITS False (BCELoss on probabilities) is not built")
    if K_e == 0:
        raise ValueError("pemp_amd loss: preds_edge is empty (the reference divides by zero)")
    if K_n == 0:
        raise ValueError("pemp_amd loss: preds_node is empty")
    if K_e > _lib.LOSS_MAXKE or K_n > _lib.LOSS_MAXKN:
        raise NotImplementedError(f"pemp_amd loss: {K_e} edge / {K_n} node predictions (limits: K_e <= "
                                  f"{_lib.LOSS_MAXKE}, K_n <= {_lib.LOSS_MAXKN})")
    if J is not None and J > _lib.LOSS_MAXJ:
        raise NotImplementedError(f"pemp_amd loss: J = {J} classes (limit: J <= {_lib.LOSS_MAXJ})")
    bad = [t for t in opt["TERMS"] if t not in TERM_NAMES]
    if bad:
        raise ValueError(f"pemp_amd loss: unknown terms {bad}")


def _f32_on(name, t, dev, shape):
    t = _device_f32(name, t)
    if t.device != dev:
        raise RuntimeError(f"{name} lies on {t.device}, the edge logits on {dev}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _i64_on(name, t, dev, shape):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
        raise TypeError(f"{name}: expected an int64 tensor (got {getattr(t, 'dtype', type(t))})")
    if t.device != dev:
        raise RuntimeError(f"{name} lies on {t.device}, the edge logits on {dev}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.contiguous()


def _ptrs(n, tensors):
    arr = (_lib.c_p * n)()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def build_record(opt, pe, pn, pc, edge_index, edge_labels, label_mask, node_labels, label_mask_node, node_classes,
                 edge_masks=None):
    """``(rec, held)``: the ``pemp_loss_rec`` of one call (``_lib.PempLossRec``) after the input checks, and the
    tensors its raw pointers point into (``held[:3]`` the contiguous edge / node / class logit lists): whoever keeps
    ``rec`` keeps ``held``. ``pc`` empty: no class term. Touches no library."""
    K_e, K_n, has_class = len(pe), len(pn), bool(pc)
    J = pc[0].shape[1] if has_class and pc[0].dim() == 2 else None
    _refusals(opt, K_e, K_n, J)
    flat = lambda t: t if t.dim() == 1 else t.reshape(-1)      # no view of a tensor that is flat already
    pe = [_device_f32(f"preds_edge[{k}]", flat(t)) for k, t in enumerate(pe)]
    dev, E = pe[0].device, pe[0].numel()
    pe = [_f32_on(f"preds_edge[{k}]", t, dev, (E,)) for k, t in enumerate(pe)]
    N = pn[0].numel()
    pn = [_f32_on(f"preds_node[{k}]", flat(t), dev, (N,)) for k, t in enumerate(pn)]
    if has_class and len(pc) != K_n:
        raise ValueError(f"mpn_loss: {len(pc)} class predictions for {K_n} node predictions")
    pc = [_f32_on(f"preds_class[{k}]", t, dev, (N, J)) for k, t in enumerate(pc)]
    edge_labels = _f32_on("edge_labels", edge_labels, dev, (E,))
    label_mask = _f32_on("label_mask", label_mask, dev, (E,))
    node_labels = _f32_on("node_labels", node_labels, dev, (N,))
    label_mask_node = _f32_on("label_mask_node", label_mask_node, dev, (N,))
    node_classes = _i64_on("node_classes", node_classes, dev, (N,)) if has_class else None
    if edge_masks is not None:
        if len(edge_masks) != K_e:
            raise ValueError(f"mpn_loss: {len(edge_masks)} edge masks for {K_e} edge predictions")
        edge_masks = [_f32_on(f"edge_mask[{k}]", t, dev, (E,)) for k, t in enumerate(edge_masks)]
        edge_index = None
    else:
        if K_n < K_e:
            raise ValueError(f"mpn_loss: mask_k needs node prediction k ({K_n} node, {K_e} edge predictions)")
        edge_index = _i64_on("edge_index", edge_index, dev, (2, E))
    terms = 0
    for t in opt["TERMS"]:
        terms |= TERM_NAMES[t]
    rec = _lib.PempLossRec(N=N, E=E, J=J or 0, K_e=K_e, K_n=K_n,
                           edge_kind=_lib.LOSS_FOCAL if opt["USE_FOCAL"] else _lib.LOSS_BCE,
                           node_kind=_lib.LOSS_FOCAL if opt["NODE_USE_FOCAL"] else _lib.LOSS_BCE,
                           include_bordering=int(bool(opt["INCLUDE_BORDERING_NODES"])), terms=terms,
                           alpha=opt["FOCAL_ALPHA"], gamma=opt["FOCAL_GAMMA"],
                           edge_pos_weight=opt["EDGE_BCE_POS_WEIGHT"], node_pos_weight=opt["NODE_BCE_POS_WEIGHT"],
                           node_threshold=opt["NODE_THRESHOLD"], node_weight=opt["NODE_WEIGHT"],
                           edge_weight=opt["EDGE_WEIGHT"], class_weight=opt["CLASS_WEIGHT"])
    rec.pe, rec.pn, rec.pc = _ptrs(_lib.LOSS_MAXKE, pe), _ptrs(_lib.LOSS_MAXKN, pn), _ptrs(_lib.LOSS_MAXKN, pc)
    rec.edge_mask = _ptrs(_lib.LOSS_MAXKE, edge_masks or ())
    rec.edge_index = _lib.ptr(edge_index)
    rec.edge_labels, rec.label_mask = edge_labels.data_ptr(), label_mask.data_ptr()
    rec.node_labels, rec.label_mask_node = node_labels.data_ptr(), label_mask_node.data_ptr()
    rec.node_classes = _lib.ptr(node_classes)
    return rec, (pe, pn, pc, edge_index, edge_labels, label_mask, node_labels, label_mask_node, node_classes, edge_masks)


class _MpnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opt, K_e, K_n, has_class, edge_index, edge_labels, label_mask, node_labels, label_mask_node,
                node_classes, edge_masks, *logits):
        pe, pn = logits[:K_e], logits[K_e:K_e + K_n]
        pc = logits[K_e + K_n:] if has_class else ()
        rec, held = build_record(opt, pe, pn, pc, edge_index, edge_labels, label_mask, node_labels, label_mask_node,
                                 node_classes, edge_masks)
        pe, pn, pc = held[:3]
        dev, N, E = pe[0].device, rec.N, rec.E
        L = _lib.lib()
        nbytes = L.pemp_loss_workspace_size(N, E, K_e, K_n)
        ws = _WS.get(nbytes, dev)
        out = torch.empty(_lib.LOSS_OUT, dtype=torch.float32, device=dev)
        _lib.check(L.pemp_loss_fwd(ctypes.byref(rec), ws.data_ptr(), ws.numel(), out.data_ptr(), _lib.stream(dev)))
        # the record holds raw pointers into `held`; the tensors go through save_for_backward, so that a logit
        # written in place before the backward (which recomputes from the logits) is caught by autograd's version check
        flat = [*pe, *pn, *pc, *held[3:9], *(held[9] or ())]
        ctx.save_for_backward(*flat)
        ctx.rec, ctx.shapes = rec, [t.shape for t in logits]
        ctx.out = out
        ctx.counts = (K_e, K_n, len(pc), held[9] is not None)
        total, terms_t = out[3], out[:4]
        ctx.mark_non_differentiable(terms_t)
        return total, terms_t

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_total, _grad_terms):
        L = _lib.lib()
        K_e, K_n, K_c, own_masks = ctx.counts
        saved = ctx.saved_tensors
        pe, pn, pc = saved[:K_e], saved[K_e:K_e + K_n], saved[K_e + K_n:K_e + K_n + K_c]
        rest = saved[K_e + K_n + K_c:]
        rec = ctx.rec
        rec.pe, rec.pn, rec.pc = _ptrs(_lib.LOSS_MAXKE, pe), _ptrs(_lib.LOSS_MAXKN, pn), _ptrs(_lib.LOSS_MAXKN, pc)
        rec.edge_index, rec.edge_labels, rec.label_mask = (_lib.ptr(t) for t in rest[:3])
        rec.node_labels, rec.label_mask_node, rec.node_classes = (_lib.ptr(t) for t in rest[3:6])
        rec.edge_mask = _ptrs(_lib.LOSS_MAXKE, rest[6:] if own_masks else ())
        dev = ctx.out.device
        need = ctx.needs_input_grad[11:]
        gt = grad_total.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        g_pe = [torch.empty_like(t) if need[k] else None for k, t in enumerate(pe)]
        g_pn = [torch.empty_like(t) if need[K_e + k] else None for k, t in enumerate(pn)]
        g_pc = [torch.empty_like(t) if need[K_e + K_n + k] else None for k, t in enumerate(pc)]
        arrs = (_ptrs(_lib.LOSS_MAXKE, g_pe), _ptrs(_lib.LOSS_MAXKN, g_pn), _ptrs(_lib.LOSS_MAXKN, g_pc))
        _lib.check(L.pemp_loss_bwd(ctypes.byref(rec), ctx.out.data_ptr(), gt.data_ptr(),
                                   *(ctypes.cast(a, _lib.c_p) for a in arrs), _lib.stream(dev)))
        grads = [None if g is None else g.view(shape) for g, shape in zip(g_pe + g_pn + g_pc, ctx.shapes)]
        return (None,) * 11 + tuple(grads)


def mpn_loss(preds_edge, preds_node, preds_class, edge_index, edge_labels, label_mask, node_labels, label_mask_node,
             node_classes, cfg_or_kwargs=None, edge_masks=None, **options):
    """``(total, terms)`` of the MPN loss. ``preds_edge``: K_e <= 8 logit tensors [E]; ``preds_node``: K_n <= 9
    [N]; ``preds_class``: K_n [N, J <= 32] or None; ``node_classes`` None (EDGE_LABEL_METHOD 4): no class term.
    ``cfg_or_kwargs``: a config, a ``MODEL.LOSS`` node or a dict of ``DEFAULTS`` keys; keyword options override it.
    ``edge_masks``: K_e caller-made masks [E] used in place of ``label_mask * mask_node_connections(...)``.
    fp32 HIP tensors. ``total`` is differentiable in every logit tensor; ``terms`` = (node, edge, class, total) [4]
    carries no gradient."""
    opt = loss_options(cfg_or_kwargs, **options)
    preds_edge, preds_node = list(preds_edge), list(preds_node)
    has_class = preds_class is not None and node_classes is not None and "class" in opt["TERMS"]
    pc = list(preds_class) if has_class else []
    K_e, K_n = len(preds_edge), len(preds_node)
    _refusals(opt, K_e, K_n, pc[0].shape[-1] if pc and pc[0].dim() == 2 else None)
    for name, ts in (("preds_edge", preds_edge), ("preds_node", preds_node), ("preds_class", pc)):
        for k, t in enumerate(ts):      # before the library is loaded
            _device_f32(f"{name}[{k}]", t)
    return _MpnLoss.apply(opt, K_e, K_n, has_class, edge_index, edge_labels, label_mask, node_labels, label_mask_node,
                          node_classes if has_class else None, edge_masks, *preds_edge, *preds_node, *pc)


def _terms_of(config):
    """LOSS.NAME's entries among node / edge / class ("edge_loss", the reference's default spelling, counts)."""
    names = config["MODEL"]["LOSS"].get("NAME")
    if names is None:
        return DEFAULTS["TERMS"]
    if isinstance(names, str):
        raise NotImplementedError("MODEL.LOSS.NAME must be a list of the losses to use (Utils/loss.py:544-547)")
    alias = {"edge_loss": "edge", "node_loss": "node", "class_loss": "class"}
    return tuple(t for t in ("node", "edge", "class") if any(alias.get(n, n) == t for n in names))


class MPNLoss(torch.nn.Module):
    """The loss of one training step from ``construct_graph``'s 15-tuple and the model's outputs. Reads
    ``MODEL.LOSS.*``, ``MODEL.MPN.NODE_THRESHOLD`` and ``MODEL.LOSS.NAME`` (terms it does not list are skipped)."""

    def __init__(self, config):
        super().__init__()
        self.options = loss_options(config, TERMS=_terms_of(config))
        _refusals(self.options, 1, 1, None)

    def forward(self, out15, preds):
        """``out15``: the constructor's tuple with the label slots filled; ``preds``: the model's (preds_edge,
        preds_node, preds_class, ...). Returns ``(total, terms)``."""
        if out15[3] is None:
            raise ValueError("MPNLoss: the graph carries no labels (construct_graph ran without ground truth)")
        return mpn_loss(preds[0], preds[1], preds[2], out15[2], out15[3], out15[8], out15[4], out15[9], out15[5],
                        self.options)


class ClassMPNLossFactory(torch.nn.Module):
    """``Utils/loss.py:785-862`` for outputs without a ``refine`` entry: ``forward(outputs, labels, masks)`` over the
    reference's dicts returns ``(loss, logging)``. ``masks["edge"]`` and ``labels["edge"]`` are the lists the loop of
    train.py:144-151 builds, one entry per NODE prediction; like the reference's ``for i in range(len(preds_edges))``
    the first ``len(outputs["edge"])`` masks are used, and the label tensor is the same one in every entry. The
    reference's train.py:154 calls its factories with a fourth argument (``output["graph"]``), which its own
    ``ClassMPNLossFactory.forward`` does not take; here it is accepted and ignored, so that call site stays as it is.
    The logging floats come from one read of ``terms``."""

    def __init__(self, config):
        super().__init__()
        over = {}
        if not config["MODEL"]["LOSS"].get("USE_FOCAL", True):
            over["EDGE_BCE_POS_WEIGHT"] = 1.0      # :798 fixes the edge pos_weight
        self.options = loss_options(config, **over)
        _refusals(self.options, 1, 1, None)

    def forward(self, outputs, labels, masks, graph=None):
        if "refine" in outputs:
            raise NotImplementedError("pemp_amd loss: the refine regression term is not built")
        pe = outputs["edge"]
        el = labels["edge"]
        el = list(el) if isinstance(el, (list, tuple)) else [el] * len(pe)
        edge_masks = list(masks["edge"])
        if len(el) < len(pe) or len(edge_masks) < len(pe):
            raise ValueError(f"pemp_amd loss: {len(el)} edge labels / {len(edge_masks)} edge masks for {len(pe)} edge "
                             "predictions")
        if any(t is not el[0] and (t.data_ptr() != el[0].data_ptr() or t.shape != el[0].shape) for t in el):
            raise NotImplementedError("pemp_amd loss: one edge label tensor for every prediction (train.py:149)")
        if any(p is None for p in pe):
            raise NotImplementedError("pemp_amd loss: a None entry in outputs['edge']")
        pc, classes = outputs.get("class"), labels.get("class")
        total, terms = mpn_loss(pe, outputs["node"], pc, None, el[0] if el else None, edge_masks[0] if pe else None,
                                labels["node"], masks["node"], classes if pc is not None else None, self.options,
                                edge_masks=edge_masks[:len(pe)])
        node, edge, cls, loss = terms.tolist()
        return total, {"edge": edge, "node": node, "class_loss": cls, "reg": 0.0, "loss": loss}


def mask_node_connections(preds_nodes, edge_index, th, node_labels=None, include_bordering_nodes=False):
    """train.py:104-112: the bool mask [E] of the edges whose ends (both, or either with
    ``include_bordering_nodes``) are selected: ``preds_nodes > th`` or ``node_labels == 1``."""
    sel = preds_nodes > th
    if node_labels is not None:
        sel = sel | (node_labels == 1.0)
    a, b = sel[edge_index[0]], sel[edge_index[1]]
    return (a | b) if include_bordering_nodes else (a & b)
