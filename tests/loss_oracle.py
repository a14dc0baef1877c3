"""Plain-torch, dtype-generic, differentiable restatement of the MPN training loss (test infrastructure).

The node, edge and class terms of ``ClassMPNLossFactory`` (``Utils/loss.py:785-862``) / ``ClassMultiLossFactory``
(``:606-621, 668-689``) with the graph reduction of ``train.py:104-112, 140-154``; in fp32 the same torch ops as the
reference, in the same order. Runs in any dtype on any device (those of the logits).
``tools/gen_golden_loss.py`` checks it against the reference in fp64.

``ClassMultiLossFactory.forward:687`` hands ``CrossEntropyLossWithLogits.forward`` one argument too many and raises
``TypeError`` as shipped; the class term here has the four-argument meaning ``ClassMPNLossFactory:850`` uses.
"""
import numpy as np
import torch
import torch.nn.functional as F

OPTIONS = dict(USE_FOCAL=True, EDGE_WITH_LOGITS=True, NODE_USE_FOCAL=True, FOCAL_ALPHA=1.0, FOCAL_GAMMA=2.0,
               NODE_BCE_POS_WEIGHT=1.0, EDGE_BCE_POS_WEIGHT=1.0, INCLUDE_BORDERING_NODES=False, NODE_WEIGHT=1.0,
               EDGE_WEIGHT=1.0, CLASS_WEIGHT=1.0, NODE_THRESHOLD=1.0, TERMS=("node", "edge", "class"))


def mask_node_connections(preds_nodes, edge_index, th, node_labels=None, include_bordering_nodes=False):
    """train.py:104-112."""
    sel = preds_nodes > th
    if node_labels is not None:
        sel = sel | (node_labels == 1.0)
    a, b = sel[edge_index[0]], sel[edge_index[1]]
    return (a | b) if include_bordering_nodes else (a & b)


def focal(x, t, mask, alpha, gamma):
    """FocalLoss.forward with logits, reduction "mean" and a mask (:872-887)."""
    bce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    pt = torch.exp(-bce)
    f = alpha * (1 - pt) ** gamma * bce
    f = f * mask
    return torch.sum(f) / mask.sum()


def bce_logits(x, t, mask, pos_weight):
    """BCELossWtihLogits.forward (:899-905)."""
    bce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    bce = bce * mask
    if pos_weight is not None:
        bce = torch.where(t == 1.0, bce * pos_weight, bce)
    return bce.mean()


def class_ce(logits, classes, node_labels):
    """CrossEntropyLossWithLogits.forward (:928-933): the mean over all nodes of CE * mask."""
    return (F.cross_entropy(logits, classes, reduction="none") * node_labels).mean()


def edge_masks(preds_node, edge_index, label_mask, node_labels, opt):
    """train.py:144-150: one mask per node prediction, from the detached prediction."""
    return [label_mask * mask_node_connections(p.detach().sigmoid(), edge_index, opt["NODE_THRESHOLD"], node_labels,
                                               opt["INCLUDE_BORDERING_NODES"]).to(label_mask.dtype)
            for p in preds_node]


def mpn_loss(preds_edge, preds_node, preds_class, edge_index, edge_labels, label_mask, node_labels, label_mask_node,
             node_classes, options=None, masks=None):
    """(total, terms [4] = node, edge, class, total); ``masks``: per-prediction edge masks in place of the computed
    ones. The labels and masks are cast to the logits' dtype."""
    opt = dict(OPTIONS, **(options or {}))
    if not preds_edge:
        raise ValueError("empty preds_edge")
    dt, dev = preds_node[0].dtype, preds_node[0].device
    edge_labels, label_mask, node_labels, label_mask_node = (
        t.to(device=dev, dtype=dt) for t in (edge_labels, label_mask, node_labels, label_mask_node))
    zero = torch.zeros((), dtype=dt, device=dev)
    node = edge = cls = zero
    if "node" in opt["TERMS"]:
        for p in preds_node:
            if opt["NODE_USE_FOCAL"]:
                node = node + focal(p, node_labels, label_mask_node, opt["FOCAL_ALPHA"], opt["FOCAL_GAMMA"])
            else:
                node = node + bce_logits(p, node_labels, label_mask_node, opt["NODE_BCE_POS_WEIGHT"])
        node = node / len(preds_node)
    if "edge" in opt["TERMS"]:
        if masks is None:
            masks = edge_masks(preds_node, edge_index.to(dev), label_mask, node_labels, opt)
        for p, m in zip(preds_edge, masks):
            m = m.to(device=dev, dtype=dt)
            if opt["USE_FOCAL"]:
                edge = edge + focal(p, edge_labels, m, opt["FOCAL_ALPHA"], opt["FOCAL_GAMMA"])
            elif opt["EDGE_WITH_LOGITS"]:
                edge = edge + bce_logits(p, edge_labels, m, opt["EDGE_BCE_POS_WEIGHT"])
            else:
                raise NotImplementedError("EDGE_WITH_LOGITS False")
        edge = edge / len(preds_edge)
        if torch.isnan(edge):
            edge = zero
    if "class" in opt["TERMS"] and preds_class is not None and node_classes is not None:
        for p in preds_class:
            cls = cls + class_ce(p, node_classes.to(dev), node_labels)
        cls = cls / len(preds_class)
    total = opt["NODE_WEIGHT"] * node + opt["EDGE_WEIGHT"] * edge + opt["CLASS_WEIGHT"] * cls
    return total, torch.stack([node.detach(), edge.detach(), cls.detach(), total.detach()])


def run(arrays, options, dtype=torch.float64, device="cpu", masks=False):
    """Forward + backward from numpy inputs (``pe<k>``, ``pn<k>``, ``pc<k>``, ``edge_index``, ``edge_labels``,
    ``label_mask``, ``node_labels``, ``label_mask_node``, optional ``node_classes``): {"terms", "g_pe<k>", ...} as
    float64 arrays. ``masks``: go through explicit per-prediction masks (the factories' path)."""
    def logits(prefix):
        out, k = [], 0
        while f"{prefix}{k}" in arrays:
            out.append(torch.as_tensor(np.asarray(arrays[f"{prefix}{k}"])).to(device=device, dtype=dtype)
                       .requires_grad_(True))
            k += 1
        return out

    pe, pn, pc = logits("pe"), logits("pn"), logits("pc")
    t = {k: torch.as_tensor(np.asarray(arrays[k])).to(device) for k in
         ("edge_index", "edge_labels", "label_mask", "node_labels", "label_mask_node")}
    classes = torch.as_tensor(np.asarray(arrays["node_classes"])).to(device) if "node_classes" in arrays else None
    opt = dict(OPTIONS, **(options or {}))
    ms = None
    if masks:
        ms = edge_masks(pn, t["edge_index"], t["label_mask"].to(dtype), t["node_labels"].to(dtype), opt)
    total, terms = mpn_loss(pe, pn, pc or None, t["edge_index"], t["edge_labels"], t["label_mask"], t["node_labels"],
                            t["label_mask_node"], classes, opt, ms)
    if total.requires_grad:
        total.backward()
    out = {"terms": terms.detach().cpu().double().numpy()}
    for prefix, ts in (("pe", pe), ("pn", pn), ("pc", pc)):
        for k, x in enumerate(ts):
            g = x.grad if x.grad is not None else torch.zeros_like(x)
            out[f"g_{prefix}{k}"] = g.detach().cpu().double().numpy()
    return out
