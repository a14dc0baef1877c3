"""Generate ``tests/golden/loss_*.npz``: the REFERENCE's loss factories on the CPU, forward + backward.

Test infrastructure (needs the reference tree, see oracle/ref_shims.py, which is imported only when the tool runs).
    PYTHONDONTWRITEBYTECODE=1 python -B tools/gen_golden_loss.py [name ...]
The reference's ``Utils/loss.py`` is loaded by path behind ``oracle.ref_shims.install_stubs()`` (plus a
``torch_scatter.scatter_mean`` entry, which that file imports and the stub lacks) and ``mask_node_connections`` is
taken out of ``train.py`` with ``ref_shims._extract_functions``. Per case and variant the per-prediction edge masks
are built as train.py:144-150 builds them and handed to

* ``mpn``:   ``ClassMPNLossFactory`` (node + edge + class, ``LOSS_WEIGHTS``);
* ``multi``: ``ClassMultiLossFactory`` with ``LOSS.NAME = ["edge", "node"]`` (its class branch raises ``TypeError`` as
  shipped, ``:687``), ``NODE_WEIGHT`` / ``EDGE_WEIGHT``;

each in fp64 and in fp32. Stored: the inputs, per variant the fp64 terms (node, edge, class, total, unweighted as
``pemp_amd.loss`` reports them) and logit gradients, and in ``meta`` the options and the reference's own
fp32-vs-fp64 error per tensor. Before a fixture is written ``tests/loss_oracle`` in fp64 must agree with the
reference in fp64 within ``1e-9 * max|.|`` per tensor.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

OUT = os.path.join(ROOT, "tests", "golden")
AGREE = 1e-9
PLANTED = (40.0, -40.0, 90.0, -90.0)

# name: J, K_e, labels with classes, variant options ("mpn" / "multi": DEFAULTS keys of pemp_amd.loss)
CASES = {
    "loss_j17_focal": dict(J=17, K_e=3, classes=True, seed=1,
                           mpn=dict(NODE_THRESHOLD=1.0, NODE_WEIGHT=1.0, EDGE_WEIGHT=2.0, CLASS_WEIGHT=0.5),
                           multi=dict(NODE_THRESHOLD=1.0, NODE_WEIGHT=0.7, EDGE_WEIGHT=1.3)),
    "loss_j14_border": dict(J=14, K_e=2, classes=True, seed=2,
                            mpn=dict(NODE_THRESHOLD=0.5, INCLUDE_BORDERING_NODES=True, EDGE_WEIGHT=1.5),
                            multi=dict(NODE_THRESHOLD=0.5, INCLUDE_BORDERING_NODES=True, FOCAL_ALPHA=0.25,
                                       FOCAL_GAMMA=1.5)),
    "loss_method4": dict(J=17, K_e=3, classes=False, seed=3,
                         mpn=dict(NODE_THRESHOLD=0.5), multi=dict(NODE_THRESHOLD=0.5, EDGE_WEIGHT=0.5)),
    "loss_bce": dict(J=17, K_e=3, classes=True, seed=4,
                     mpn=dict(NODE_THRESHOLD=0.5, USE_FOCAL=False, NODE_USE_FOCAL=False, NODE_BCE_POS_WEIGHT=2.0),
                     multi=dict(NODE_THRESHOLD=0.5, USE_FOCAL=False, EDGE_BCE_POS_WEIGHT=3.0)),
    "loss_zero_mask": dict(J=17, K_e=3, classes=True, seed=5, zero_mask=1,
                           mpn=dict(NODE_THRESHOLD=0.5), multi=dict(NODE_THRESHOLD=0.5)),
}


def make_inputs(case, N=40):
    """N nodes, the fully connected graph (E = N (N - 1)); logits over about +-8 with +-40 and +-90 planted in every
    prediction; no node logit within 0.05 of 0 (sigmoid stays 1e-2 away from the 0.5 threshold). ``zero_mask``: that
    node prediction is all negative and one node alone is labelled, so its mask_k is all zero."""
    g = torch.Generator().manual_seed(1000 + case["seed"])
    J, K_e = case["J"], case["K_e"]
    K_n = K_e + 1
    idx = torch.arange(N)
    src, dst = torch.meshgrid(idx, idx, indexing="ij")
    keep = src != dst
    ei = torch.stack([src[keep], dst[keep]])
    E = ei.shape[1]

    def logits(shape):
        x = (torch.rand(shape, generator=g) * 2 - 1) * 8
        x = torch.where(x.abs() < 0.05, torch.full_like(x, 0.3), x)
        flat = x.view(-1)
        pos = torch.randperm(flat.numel(), generator=g)[:len(PLANTED)]
        flat[pos] = torch.tensor(PLANTED)
        return x

    a = {"edge_index": ei.numpy()}
    for k in range(K_e):
        a[f"pe{k}"] = logits((E,)).numpy()
    for k in range(K_n):
        a[f"pn{k}"] = logits((N,)).numpy()
        if case["classes"]:
            a[f"pc{k}"] = logits((N, J)).numpy()
    persons = torch.randint(0, 5, (N,), generator=g)
    node_labels = (torch.rand(N, generator=g) < 0.6).float()
    if "zero_mask" in case:
        node_labels = torch.zeros(N)
        node_labels[7] = 1.0
        k = case["zero_mask"]
        a[f"pn{k}"] = -np.abs(a[f"pn{k}"])
    matched = node_labels == 1
    a["edge_labels"] = (matched[ei[0]] & matched[ei[1]] & (persons[ei[0]] == persons[ei[1]])).float().numpy()
    a["label_mask"] = (torch.rand(E, generator=g) < 0.9).float().numpy()
    a["node_labels"] = node_labels.numpy()
    a["label_mask_node"] = (torch.rand(N, generator=g) < 0.9).float().numpy()
    if case["classes"]:
        a["node_classes"] = torch.randint(0, J, (N,), generator=g).numpy()
    return a


def reference_config(variant, opt, J):
    from pemp_amd import config as pcfg
    from pemp_amd.loss import DEFAULTS
    o = dict(DEFAULTS, **opt)
    cfg = pcfg.get_config()
    loss = {k: o[k] for k in ("USE_FOCAL", "EDGE_WITH_LOGITS", "NODE_USE_FOCAL", "FOCAL_ALPHA", "FOCAL_GAMMA",
                              "NODE_BCE_POS_WEIGHT", "EDGE_BCE_POS_WEIGHT", "INCLUDE_BORDERING_NODES", "NODE_WEIGHT",
                              "EDGE_WEIGHT", "CLASS_WEIGHT")}
    if variant == "mpn":
        loss["LOSS_WEIGHTS"] = [o["NODE_WEIGHT"], o["EDGE_WEIGHT"], o["CLASS_WEIGHT"]]
    else:
        loss["NAME"] = ["edge", "node"]
    cfg.merge({"MODEL": {"LOSS": loss, "MPN": {"NODE_THRESHOLD": o["NODE_THRESHOLD"]},
                         "HRNET": {"NUM_JOINTS": J, "LOSS": {"NUM_STAGES": 2}}}})
    return cfg, o


def run_reference(ref_loss, mask_fn, variant, opt, arrays, J, dtype):
    cfg, o = reference_config(variant, opt, J)

    def logits(prefix):
        out, k = [], 0
        while f"{prefix}{k}" in arrays:
            out.append(torch.from_numpy(arrays[f"{prefix}{k}"]).to(dtype).requires_grad_(True))
            k += 1
        return out

    pe, pn, pc = logits("pe"), logits("pn"), logits("pc")
    ei = torch.from_numpy(arrays["edge_index"])
    f = {k: torch.from_numpy(arrays[k]).to(dtype) for k in ("edge_labels", "label_mask", "node_labels", "label_mask_node")}
    classes = torch.from_numpy(arrays["node_classes"]) if "node_classes" in arrays else None
    # the graph reduction of train.py:144-150
    masks = [f["label_mask"] * mask_fn(p.sigmoid().detach(), ei, cfg.MODEL.MPN.NODE_THRESHOLD, f["node_labels"],
                                       include_bordering_nodes=cfg.MODEL.LOSS.INCLUDE_BORDERING_NODES).float()
             for p in pn]
    outputs = {"edge": pe, "node": pn, "class": pc or None, "heatmap": None, "tag": None}
    labels = {"edge": [f["edge_labels"]] * len(pn), "node": f["node_labels"], "class": classes, "heatmap": None,
              "tag": None, "batch_index": None, "person": None, "keypoints": None}
    ms = {"edge": masks, "node": f["label_mask_node"], "class": None, "heatmap": None}
    if variant == "mpn":
        loss, log = ref_loss.ClassMPNLossFactory(cfg)(outputs, labels, ms)
        terms = [log["node"], log["edge"], log["class_loss"], log["loss"]]
    else:
        loss, log = ref_loss.ClassMultiLossFactory(cfg)(outputs, labels, ms, {"nodes": torch.zeros(1, 3)})
        terms = [log["node"] / o["NODE_WEIGHT"], log["edge"] / o["EDGE_WEIGHT"], 0.0, log["loss"]]
    loss.backward()
    res = {"terms": np.asarray(terms, np.float64)}
    for prefix, ts in (("pe", pe), ("pn", pn), ("pc", pc)):
        for k, x in enumerate(ts):
            g = x.grad if x.grad is not None else torch.zeros_like(x)
            res[f"g_{prefix}{k}"] = g.detach().double().numpy()
    return res


def oracle_options(variant, opt):
    return dict(opt, TERMS=("node", "edge", "class") if variant == "mpn" else ("node", "edge"))


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max() if b.size else 0.0
    err = np.abs(a - b).max() if b.size else 0.0
    return float(err / scale) if scale > 0 else float(err)


def main(only=()):
    from oracle import ref_shims
    from tests import loss_oracle as lo
    ref_shims.install_stubs()
    sys.modules["torch_scatter"].scatter_mean = ref_shims.scatter_mean
    ref_loss = ref_shims._load("ref_loss", os.path.join(ref_shims.REF_SRC, "Utils", "loss.py"))
    mask_fn = ref_shims._extract_functions(os.path.join(ref_shims.REF_SRC, "train.py"),
                                           ["mask_node_connections"])["mask_node_connections"]
    for name, case in CASES.items():
        if only and name not in only:
            continue
        arrays = make_inputs(case)
        stored = dict(arrays)
        meta = dict(J=case["J"], K_e=case["K_e"], K_n=case["K_e"] + 1, N=int(arrays["node_labels"].shape[0]),
                    E=int(arrays["edge_index"].shape[1]), classes=case["classes"], variants={}, reference_fp32_rel_err={},
                    oracle_vs_reference={})
        for variant in ("mpn", "multi"):
            opt = case[variant]
            r64 = run_reference(ref_loss, mask_fn, variant, opt, arrays, case["J"], torch.float64)
            r32 = run_reference(ref_loss, mask_fn, variant, opt, arrays, case["J"], torch.float32)
            mine = lo.run(arrays, oracle_options(variant, opt), torch.float64, masks=True)
            worst = 0.0
            for k, v in r64.items():
                err = rel_err(mine[k], v)
                worst = max(worst, err)
                assert err <= AGREE, (name, variant, k, err)
            meta["variants"][variant] = oracle_options(variant, opt)
            meta["oracle_vs_reference"][variant] = worst
            meta["reference_fp32_rel_err"][variant] = {k: rel_err(r32[k], v) for k, v in r64.items()}
            for k, v in r64.items():
                stored[f"{variant}.{k}"] = v
        if "zero_mask" in case:
            assert stored["mpn.terms"][1] == 0.0 and not any(np.any(stored[f"mpn.g_pe{k}"]) for k in range(case["K_e"]))
        path = os.path.join(OUT, f"{name}.npz")
        np.savez_compressed(path, meta=json.dumps(meta), **stored)
        print(f"{name}: N={meta['N']} E={meta['E']} oracle_vs_reference={meta['oracle_vs_reference']} "
              f"ref_fp32_err(max)={ {v: max(d.values()) for v, d in meta['reference_fp32_rel_err'].items()} } "
              f"bytes={os.path.getsize(path)}")
        assert os.path.getsize(path) < 1_000_000, path


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
