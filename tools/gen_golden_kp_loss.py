"""Generate ``tests/golden/kp_loss_*.npz``: the REFERENCE's keypoint losses on the CPU, forward + backward.

Test infrastructure (needs the reference tree, see oracle/ref_shims.py, which is imported only when the tool runs).
    PYTHONDONTWRITEBYTECODE=1 python -B tools/gen_golden_kp_loss.py [name ...]
The reference's ``Utils/loss.py`` is loaded as ``tools/gen_golden_loss.py`` loads it. Per case, in fp64 and in fp32:

* ``HeatmapLoss`` on every stage and ``AELoss`` on stage 0, on their own: the per-image values [B] and the gradient
  of their sum (``hm<s>``, ``push``, ``pull``, ``g_hm<s>``, ``g_ae``);
* ``ClassMultiLossFactory`` with ``LOSS.NAME = ["edge", "node", "heatmap", "tagmap"]`` over a small graph of
  ``gen_golden_loss.make_inputs``: the logging dict and the gradients of every prediction (``multi.*``).

Stored: the inputs, the fp64 results, and in ``meta`` the options and the reference's own fp32-vs-fp64 error per
tensor. Before a fixture is written ``tests/kp_loss_oracle`` in fp64 must agree with the reference in fp64 within
``1e-9 * max|.|`` per tensor. Every image has at least two persons: ``AELoss``'s branches for none and for one call
``.cuda()`` (``Utils/loss.py:29-34, 60-65``) and cannot run on the CPU; those images are held to the oracle alone.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from tools import gen_golden_loss as ggl  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
AGREE = 1e-9
B, J, P = 2, 5, 4
SIZES = ((2 * J, 16, 16), (J, 32, 32))          # (C, H, W) per stage; stage 0 carries the tag planes
LOG_KEYS = ("heatmap", "tag_loss", "edge", "node", "class_loss", "loss")
MPN_CASE = dict(J=J, K_e=2, classes=False, seed=11)
MPN_OPT = dict(NODE_THRESHOLD=0.5, NODE_WEIGHT=0.7, EDGE_WEIGHT=1.3)

CASES = {
    "kp_loss_exp": dict(seed=1, kind="exp", heat=(1.0, 0.5), push=(0.001, 0.001), pull=(0.002, 0.001)),
    "kp_loss_max": dict(seed=2, kind="max", heat=(0.7, 1.0), push=(0.5, 0.5), pull=(0.25, 0.25)),
}
CENTRES = (0.0, 0.45, 1.7, 2.3)                   # person tag centres: no two at distance 1


def make_inputs(case):
    """Stage 0 [B, 2J, 16, 16] with tags, stage 1 [B, J, 32, 32]; masks with values other than 0 / 1. Image 0 has four
    persons (all J joints; one joint; visible entries that are not packed to the front; two joints), image 1 two."""
    g = torch.Generator().manual_seed(2000 + case["seed"])
    a = {}
    for s, (C, H, W) in enumerate(SIZES):
        a[f"pred{s}"] = (torch.rand((B, C, H, W), generator=g) * 0.6 - 0.1).numpy()
        gt = torch.rand((B, J, H, W), generator=g)
        a[f"gt{s}"] = torch.where(gt > 0.9, gt, torch.zeros_like(gt)).numpy()
        m = (torch.rand((B, H, W), generator=g) > 0.2).float()
        m[:, 0, :] = 0.5
        a[f"mask{s}"] = m.numpy()
    C, H, W = SIZES[0]
    tag = np.zeros((B, P, J, 2), np.int32)
    visible = {(0, 0): range(J), (0, 1): (2,), (0, 2): (1, 3, 4), (0, 3): (0, 4), (1, 0): (0, 1, 2), (1, 2): (3, 4)}
    pred0 = a["pred0"]
    for (b, p), joints in visible.items():
        for j in range(J):
            pix = int(torch.randint(0, H * W, (1,), generator=g))
            tag[b, p, j] = (j * H * W + pix, 1 if j in joints else 0)
            if j in joints:
                pred0[b, J + j, pix // W, pix % W] = CENTRES[p] + 0.05 * float(torch.rand((), generator=g))
    tag[0, 1, 0] = (7, 0)                          # an index on an entry that is not visible is never read
    a["tag0"] = tag
    return a


def reference_config(case):
    cfg, _ = ggl.reference_config("multi", MPN_OPT, J)
    cfg.merge({"MODEL": {"KP": "hrnet", "LOSS": {"NAME": ["edge", "node", "heatmap", "tagmap"]},
                         "HRNET": {"NUM_JOINTS": J,
                                   "LOSS": {"NUM_STAGES": 2, "WITH_HEATMAPS_LOSS": (True, True),
                                            "HEATMAPS_LOSS_FACTOR": case["heat"], "AE_LOSS_TYPE": case["kind"],
                                            "PUSH_LOSS_FACTOR": case["push"], "PULL_LOSS_FACTOR": case["pull"]}}},
               "TRAIN": {"WITH_AE_LOSS": [True, False]}})
    return cfg


def oracle_options(case):
    return dict(NUM_JOINTS=J, WITH_HEATMAPS_LOSS=(True, True), HEATMAPS_LOSS_FACTOR=case["heat"],
                WITH_AE_LOSS=(True, False), AE_LOSS_TYPE=case["kind"], PUSH_LOSS_FACTOR=case["push"],
                PULL_LOSS_FACTOR=case["pull"])


def run_parts(mod, case, a, dtype):
    """(reference results, the same from ``mod`` given as the oracle): HeatmapLoss / AELoss on their own."""
    res = {}
    for s in range(len(SIZES)):
        p = torch.from_numpy(a[f"pred{s}"]).to(dtype).requires_grad_(True)
        v = mod["heatmap"](p[:, :J], torch.from_numpy(a[f"gt{s}"]).to(dtype), torch.from_numpy(a[f"mask{s}"]).to(dtype))
        v.sum().backward()
        res[f"hm{s}"], res[f"g_hm{s}"] = v.detach().double().numpy(), p.grad.double().numpy()
    p = torch.from_numpy(a["pred0"]).to(dtype).requires_grad_(True)
    push, pull = mod["ae"](case["kind"])(p[:, J:].contiguous().view(B, -1, 1), torch.from_numpy(a["tag0"]))
    (push.sum() + pull.sum()).backward()
    res["push"], res["pull"] = push.detach().double().numpy().reshape(B), pull.detach().double().numpy().reshape(B)
    res["g_ae"] = p.grad.double().numpy()
    return res


def run_factory(ref_loss, mask_fn, case, a, mpn, dtype):
    cfg = reference_config(case)
    lg = lambda prefix: [torch.from_numpy(mpn[k]).to(dtype).requires_grad_(True)
                         for k in sorted(mpn) if k.startswith(prefix) and k[len(prefix):].isdigit()]
    pe, pn = lg("pe"), lg("pn")
    preds = [torch.from_numpy(a[f"pred{s}"]).to(dtype).requires_grad_(True) for s in range(len(SIZES))]
    ei = torch.from_numpy(mpn["edge_index"])
    f = {k: torch.from_numpy(mpn[k]).to(dtype) for k in ("edge_labels", "label_mask", "node_labels", "label_mask_node")}
    masks = [f["label_mask"] * mask_fn(p.sigmoid().detach(), ei, cfg.MODEL.MPN.NODE_THRESHOLD, f["node_labels"],
                                       include_bordering_nodes=cfg.MODEL.LOSS.INCLUDE_BORDERING_NODES).float()
             for p in pn]
    outputs = {"edge": pe, "node": pn, "class": None, "heatmap": preds, "tag": None}
    labels = {"edge": [f["edge_labels"]] * len(pn), "node": f["node_labels"], "class": None,
              "heatmap": [torch.from_numpy(a[f"gt{s}"]).to(dtype) for s in range(len(SIZES))],
              "tag": [torch.from_numpy(a["tag0"]), None], "batch_index": None, "person": None, "keypoints": None}
    ms = {"edge": masks, "node": f["label_mask_node"], "class": None,
          "heatmap": [torch.from_numpy(a[f"mask{s}"]).to(dtype) for s in range(len(SIZES))]}
    loss, log = ref_loss.ClassMultiLossFactory(cfg)(outputs, labels, ms, {"nodes": torch.zeros(1, 3)})
    loss.backward()
    res = {"multi.log": np.asarray([log[k] for k in LOG_KEYS], np.float64),
           "multi.terms": np.asarray([log["heatmap"], log["tag_loss"], log["heatmap"] + log["tag_loss"]], np.float64)}
    for name, ts in (("pe", pe), ("pn", pn), ("pred", preds)):
        for k, x in enumerate(ts):
            res[f"multi.g_{name}{k}"] = x.grad.double().numpy()
    return res


def main(only=()):
    from oracle import ref_shims
    from tests import kp_loss_oracle as ko, loss_oracle as lo
    ref_shims.install_stubs()
    sys.modules["torch_scatter"].scatter_mean = ref_shims.scatter_mean
    ref_loss = ref_shims._load("ref_loss", os.path.join(ref_shims.REF_SRC, "Utils", "loss.py"))
    mask_fn = ref_shims._extract_functions(os.path.join(ref_shims.REF_SRC, "train.py"),
                                           ["mask_node_connections"])["mask_node_connections"]
    ref_mod = {"heatmap": ref_loss.HeatmapLoss(), "ae": ref_loss.AELoss}
    mine_mod = {"heatmap": ko.heatmap_loss, "ae": lambda kind: (lambda tags, joints: ko.ae_loss(tags, joints, kind))}
    for name, case in CASES.items():
        if only and name not in only:
            continue
        a = make_inputs(case)
        assert ko.max_kinks_clear(a, 0, J), name
        mpn = ggl.make_inputs(MPN_CASE, N=12)
        r64 = dict(run_parts(ref_mod, case, a, torch.float64), **run_factory(ref_loss, mask_fn, case, a, mpn, torch.float64))
        r32 = dict(run_parts(ref_mod, case, a, torch.float32), **run_factory(ref_loss, mask_fn, case, a, mpn, torch.float32))
        # the oracle in fp64: the parts, the two terms, and the node / edge part through loss_oracle
        mine = run_parts(mine_mod, case, a, torch.float64)
        kp = ko.run(a, oracle_options(case), torch.float64)
        mo = lo.run(mpn, dict(MPN_OPT, TERMS=("node", "edge")), torch.float64, masks=True)
        mine["multi.terms"] = kp["terms"]
        node, edge = mo["terms"][0] * MPN_OPT["NODE_WEIGHT"], mo["terms"][1] * MPN_OPT["EDGE_WEIGHT"]
        mine["multi.log"] = np.asarray([kp["terms"][0], kp["terms"][1], edge, node, 0.0, kp["terms"][2] + node + edge])
        for k in r64:
            if k.startswith("multi.g_pred"):
                mine[k] = kp[k[len("multi."):]]
            elif k.startswith("multi.g_"):
                mine[k] = mo[k[len("multi."):]]
        worst = 0.0
        for k, v in r64.items():
            err = ggl.rel_err(mine[k], v)
            worst = max(worst, err)
            assert err <= AGREE, (name, k, err)
        meta = dict(B=B, J=J, P=P, sizes=SIZES, options=oracle_options(case), mpn_options=MPN_OPT, log_keys=LOG_KEYS,
                    K_e=MPN_CASE["K_e"], K_n=MPN_CASE["K_e"] + 1, oracle_vs_reference=worst,
                    reference_fp32_rel_err={k: ggl.rel_err(r32[k], v) for k, v in r64.items()})
        stored = dict(a, **{f"mpn.{k}": v for k, v in mpn.items()}, **r64)
        path = os.path.join(OUT, f"{name}.npz")
        np.savez_compressed(path, meta=json.dumps(meta), **stored)
        print(f"{name}: oracle_vs_reference={worst:.3g} ref_fp32_err(max)={max(meta['reference_fp32_rel_err'].values()):.3g} "
              f"bytes={os.path.getsize(path)}")
        assert os.path.getsize(path) < 1_000_000, path


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
