"""Generate ``tests/golden/labels_*.npz`` by running the REFERENCE's NaiveGraphConstructor with ground truth on the CPU.

Test infrastructure (needs the reference tree, see oracle/ref_shims.py, and scipy). Run:
    PYTHONDONTWRITEBYTECODE=1 python -B tools/gen_golden_labels.py
Each fixture holds the inputs (scoremaps, joints_gt, factors) and the seven label outputs of the reference's
``construct_graph`` (slots 3, 4, 5, 8, 9, 10, 13). A draw is rejected and re-drawn when the labels could depend on
rounding or on an unspecified choice:
  * a similarity within relative 1e-4 of MATCHING_RADIUS or INCLUSION_RADIUS;
  * an assignment whose optimum is not unique (removing any matched pair and re-solving must cost more than 1e-6);
  * more visible ground-truth joints than detections in an image;
  * a detection matched by two rows;
  * float32 and float64 factors giving different labels.
Every stored fixture has a positive edge label, an ambiguous detection when USE_NEIGHBOURS is on and a different-type
fill-in for method 6 (the counts are printed). ``labels_lsap_*.npz`` keep a few of the cost matrices with scipy's
solution for the solver test. The restatement tests/labels_oracle.py is checked against every fixture before it is
written.
"""
import json
import os
import sys

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.ref_shims import load_reference      # noqa: E402
import pemp_amd.config as pcfg                   # noqa: E402
from pemp_amd import synthetic as syn             # noqa: E402
from tests import labels_oracle as lo             # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SLOTS = (3, 4, 5, 8, 9, 10, 13)
B, J, H, W, PERSONS, C = 2, 17, 96, 104, 3, 8
MR, IR = 0.5, 0.75                               # model_58_4_4.yaml

CASES = {
    # name: (method, USE_NEIGHBOURS, WITH_BACKGROUND, graph)
    "labels_m4_fully": (4, False, False, "fully"),
    "labels_m4_nb_fully": (4, True, False, "fully"),
    "labels_m6_fully": (6, False, False, "fully"),
    "labels_m6_bg_fully": (6, False, True, "fully"),
    "labels_m6_nb_fully": (6, True, False, "fully"),
    "labels_m6_nb_bg_fully": (6, True, True, "fully"),
    "labels_m6_nb_knn": (6, True, False, "knn"),
}


def label_config(method, nb, bg, graph):
    g = pcfg.inference_gc_config(graph, 5, False)
    g.merge({"EDGE_LABEL_METHOD": method, "USE_NEIGHBOURS": nb, "WITH_BACKGROUND": bg, "MATCHING_RADIUS": MR,
             "INCLUSION_RADIUS": IR})
    return g


def run_reference(cg, cfg, hm, gt, fac):
    feats = torch.from_numpy(syn.closed_form((B, C, H, W), 0.25))
    tags = torch.from_numpy(syn.closed_form((B, J, H, W, 1), 0.75))
    gcn = cg.NaiveGraphConstructor(torch.from_numpy(hm), tags, feats, torch.from_numpy(gt), torch.from_numpy(fac),
                                   None, torch.device("cpu"), cfg, True, None, J)
    return gcn.construct_graph()


def unique_optimum(w):
    """scipy's (rows, cols) of nonzero weight, or None when removing a matched pair does not cost > 1e-6."""
    r, c = linear_sum_assignment(w, maximize=True)
    keep = w[r, c] != 0
    r, c = r[keep], c[keep]
    total = w[r, c].sum()
    for i, j in zip(r, c):
        w2 = w.copy()
        w2[i, j] = 0
        r2, c2 = linear_sum_assignment(w2, maximize=True)
        if not total - w2[r2, c2].sum() > 1e-6:
            return None
    return r, c


def check_draw(det, bidx, gt, fac, method):
    """None when the draw must be rejected, else (fill-ins, the cost matrices with scipy's solutions)."""
    fills, mats = 0, []
    for b in range(B):
        for f in (fac[b].astype(np.float32), fac[b]):   # (the float64 matrix is the one solved below)
            pi, ji, sim, same = lo.similarity(det[bidx == b], gt[b], f, H, W)
            if sim.shape[0] > sim.shape[1]:
                return None
            for rad in (MR, IR):
                if (np.abs(sim - rad) <= 1e-4 * rad).any():
                    return None
        cols = []
        for k, sel in enumerate((same, ~same)[:2 if method == 6 else 1]):
            w = np.where(sel & (sim >= MR), sim, 0).astype(np.float64)
            sol = unique_optimum(w)
            if sol is None:
                return None
            mats.append((w, sol))
            cols.append(dict(zip(*sol)))
        final = dict(cols[0])
        if method == 6:
            for g, n in cols[1].items():
                if g not in final:
                    final[g] = n
                    fills += 1
        if len(set(final.values())) != len(final):
            return None
    return fills, mats


def main():
    cg = load_reference()[0]
    os.makedirs(OUT, exist_ok=True)
    lsap = []
    for name, (method, nb, bg, graph) in CASES.items():
        cfg = label_config(method, nb, bg, graph)
        seed = 100 + 7 * len(name)
        for attempt in range(200):
            seed += 1
            hm, gt, fac = syn.make_labelled_heatmaps(seed, B, J, H, W, PERSONS)
            try:
                ref = run_reference(cg, cfg, hm, gt, fac)
                ref32 = run_reference(cg, cfg, hm, gt, fac.astype(np.float32))
            except AssertionError:                      # (method 4's own assert on an unmatched neighbour row)
                continue
            det, bidx, ei = ref[7].numpy(), ref[12].numpy(), ref[2].numpy()
            got = {i: None if ref[i] is None else ref[i].numpy() for i in SLOTS}
            if any((got[i] is None) != (ref32[i] is None) or
                   (got[i] is not None and not np.array_equal(got[i], ref32[i].numpy())) for i in SLOTS):
                continue
            chk = check_draw(det, bidx, gt, fac, method)
            if chk is None:
                continue
            fills, mats = chk
            mine = lo.construct_labels(det, bidx, ei, gt, fac, H, W, B, J, method, nb, bg, MR, IR)
            n_pos = int(got[3].sum())
            n_amb = int((got[8][got[3] == got[3]] == 0).sum()) if nb else 0
            amb_nodes = int(np.concatenate([lo.node_labels(det[bidx == b], gt[b], fac[b], H, W, method, nb, bg, MR, IR,
                                                           J)["ambiguous"] for b in range(B)]).sum())
            if n_pos == 0 or (nb and amb_nodes == 0) or (method == 6 and fills == 0):
                continue
            for i in SLOTS:
                assert (mine[i] is None) == (got[i] is None), (name, i)
                if got[i] is not None:
                    assert mine[i].dtype == got[i].dtype and np.array_equal(mine[i], got[i]), (name, i)
            break
        else:
            raise RuntimeError(f"{name}: no acceptable draw")
        meta = dict(seed=seed, B=B, J=J, H=H, W=W, C=C, persons=PERSONS, method=method, use_neighbours=nb,
                    with_background=bg, graph=graph, matching_radius=MR, inclusion_radius=IR, N=int(det.shape[0]),
                    E=int(ei.shape[1]), positive_edges=n_pos, ambiguous_nodes=amb_nodes, fill_ins=fills)
        arrays = {f"slot{i}": got[i] for i in SLOTS if got[i] is not None}
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), meta=json.dumps(meta), scoremaps=hm, joints_gt=gt,
                            factors=fac, **arrays)
        print(f"{name}: seed={seed} N={meta['N']} E={meta['E']} positive_edges={n_pos} "
              f"ambiguous_nodes={amb_nodes} fill_ins={fills} masked_edges={n_amb}")
        for m in mats:                                  # distinct matrices, same-type and different-type ones
            if len(m[1][0]) >= 3 and all(m[0].shape != o[0].shape or not np.array_equal(m[0], o[0]) for o in lsap):
                lsap.append(m)
    lsap = lsap[:3] + lsap[-1:]
    for k, (w, (r, c)) in enumerate(lsap[:4]):
        np.savez_compressed(os.path.join(OUT, f"labels_lsap_{k}.npz"), cost=w, rows=r.astype(np.int64),
                            cols=c.astype(np.int64))
        print(f"labels_lsap_{k}: {w.shape} matched={len(r)} total={w[r, c].sum():.6f}")


if __name__ == "__main__":
    main()
