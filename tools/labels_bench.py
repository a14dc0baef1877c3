"""Timing of the training-label construction (EDGE_LABEL_METHOD 6, USE_NEIGHBOURS) on the GPU.

    python tools/labels_bench.py [--out FILE.json]

1. The edge label pass (pemp_label_edges) with HIP events, on the c3 graph (8 images, 640 x 640, the benchmark's
   heatmaps) and on a fully connected batch of 8 x 432 nodes (1.49 M edges), against the same labels by plain torch
   ops on the same device. 20 calls per event pair, median of 15 pairs after a warm-up.
2. construct_graph at the 15-tuple level with and without ground truth (host clock around a device synchronise,
   median of 30 after 5 warm-ups), against the same labels by the restated rules as torch ops on the device with
   scipy's solves on the host (the reference's form), given the graph.
Bytes are the algorithm's: 16 B read and 8 B written per edge. The share of HBM bandwidth is that over 8 TB/s.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pemp_amd                                   # noqa: E402
from pemp_amd import _lib, config as pcfg, synthetic as syn   # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12
MR, IR = 0.5, 0.75


def events_ms(fn, inner=20, outer=15, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(outer):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return statistics.median(times), min(times), max(times)


def host_ms(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def torch_edge_pass(ei, bidx, persons, amb, B):
    ps, pd = persons[ei[0]], persons[ei[1]]
    lab = ((ps >= 0) & (ps == pd)).float()
    mask = (~(amb[ei[0]] | amb[ei[1]])).float()
    img = bidx[ei[0]]
    pos = torch.zeros(B, device=ei.device).index_reduce_(0, img, lab, "amax", include_self=True)
    return lab, mask * pos[img]


def edge_pass_case(name, ei, node_off, bidx, persons, amb, B):
    L = _lib.lib()
    E, N = ei.shape[1], persons.shape[0]
    lab, mask = torch.empty(E, device=DEV), torch.empty(E, device=DEV)
    ws = torch.empty(L.pemp_label_edges_scratch_size(B), dtype=torch.uint8, device=DEV)
    st = _lib.stream(DEV)
    amb8 = amb.to(torch.uint8)

    def hip():
        _lib.check(L.pemp_label_edges(ei.data_ptr(), E, node_off.data_ptr(), B, N, persons.data_ptr(),
                                      amb8.data_ptr(), lab.data_ptr(), mask.data_ptr(), ws.data_ptr(), ws.numel(), st))

    hip()
    tl, tm = torch_edge_pass(ei, bidx, persons, amb, B)
    assert torch.equal(lab, tl) and torch.equal(mask, tm), name
    h, t = events_ms(hip), events_ms(lambda: torch_edge_pass(ei, bidx, persons, amb, B))
    byt = 24 * E
    return dict(case=name, E=E, N=N, positives=int(lab.sum()), hip_ms=h, torch_ms=t, bytes=byt,
                hip_gbs=byt / (h[0] * 1e-3) / 1e9, hbm_share=byt / (h[0] * 1e-3) / HBM_PEAK)


def torch_labels(out, gt, fac, H, W, B, J):
    """Method 6 with neighbours as the reference computes it, on the constructor's graph: dense torch ops on the
    device, scipy's two solves per image on the host."""
    from scipy.optimize import linear_sum_assignment as lsa
    det, ei, bidx = out[7], out[2], out[12]
    N = det.shape[0]
    persons = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    classes = torch.zeros(N, dtype=torch.int64, device=DEV)
    labels = torch.zeros(N, device=DEV)
    amb_all = torch.zeros(N, dtype=torch.bool, device=DEV)
    start = 0
    for b in range(B):
        d = det[bidx == b]
        n = d.shape[0]
        pi, ji = gt[b, :, :, 2].nonzero(as_tuple=True)
        pos = gt[b, pi, ji, :2].round().clamp(0, max(H, W))
        d2 = (pos[:, None, :] - d[None, :, :2].float()).pow(2).sum(2)
        sim = torch.exp(-d2 / fac[b, pi, ji][:, None])
        same = ji[:, None] == d[None, :, 2]
        ws_ = torch.where(same & (sim >= MR), sim, torch.zeros_like(sim)).cpu().numpy()
        wd_ = torch.where(~same & (sim >= MR), sim, torch.zeros_like(sim)).cpu().numpy()
        G = ws_.shape[0]
        col = np.full(G, -1, np.int64)
        if G:
            r, c = lsa(ws_, maximize=True)
            k = ws_[r, c] != 0
            col[r[k]] = c[k]
            r, c = lsa(wd_, maximize=True)
            k = (wd_[r, c] != 0) & (col[r] < 0)
            col[r[k]] = c[k]
        w2 = sim.cpu().numpy()
        w2[w2 < IR] = 0
        rows = np.nonzero(col >= 0)[0]
        w2[:, col[rows]] = 0
        amb = (w2 != 0).sum(0) > 1
        w2[:, amb] = 0
        w2[col < 0] = 0
        r2, c2 = np.nonzero(w2)
        gs = torch.from_numpy(np.concatenate([rows, r2])).to(DEV)
        ns = torch.from_numpy(np.concatenate([col[rows], c2])).to(DEV) + start
        labels[ns] = 1.0
        persons[ns] = pi[gs]
        classes[ns] = ji[gs]
        amb_all[start:start + n] = torch.from_numpy(amb).to(DEV)
        start += n
    mask_node = (~amb_all).float()
    lab, mask = torch_edge_pass(ei, bidx, persons, amb_all, B)
    return lab, labels, classes, mask, mask_node, labels * mask_node, persons


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--edge-only", action="store_true", help="part 1 only (for a kernel trace of the edge pass)")
    args = ap.parse_args()
    res = {"edge_pass": [], "device": torch.cuda.get_device_name(0)}
    B, J, H, W = 8, 17, 640, 640
    hm_b = torch.from_numpy(syn.make_heatmaps(1000, B, J, H, W, 9)).to(DEV)      # bench.py's c3 heatmaps
    feats = torch.from_numpy(syn.closed_form((B, 128, H, W), 0.25)).to(DEV)
    tags = torch.from_numpy(syn.closed_form((B, J, H, W, 1), 0.75)).to(DEV)
    cfg = pcfg.inference_gc_config("fully", 5, False)
    cfg.merge({"EDGE_LABEL_METHOD": 6, "USE_NEIGHBOURS": True, "MATCHING_RADIUS": MR, "INCLUSION_RADIUS": IR})

    def gc(hm, gt, fac):
        return pemp_amd.get_graph_constructor(cfg, scoremaps=hm, features=feats, tagmaps=tags, joints_gt=gt,
                                              factor_list=fac, masks=None, device=DEV, testing=True, heatmaps=None,
                                              num_joints=J).construct_graph()

    # ---- 1. the edge pass ----
    out = gc(hm_b, None, None)
    det, ei, bidx = out[7], out[2], out[12]
    N = det.shape[0]
    node_off = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    node_off[1:] = torch.bincount(bidx, minlength=B).cumsum(0)
    g = torch.Generator(device="cpu").manual_seed(0)
    local = torch.arange(N, device=DEV) - node_off[bidx]
    persons = torch.where(torch.rand(N, generator=g).to(DEV) < 0.8, local % 9, torch.full_like(local, -1))
    amb = torch.rand(N, generator=g).to(DEV) < 0.02
    res["edge_pass"].append(edge_pass_case("c3", ei, node_off, bidx, persons, amb, B))
    n = 432
    idx = torch.arange(n, device=DEV)
    s, d = torch.meshgrid(idx, idx, indexing="ij")
    keep = s != d
    one = torch.stack([s[keep], d[keep]])
    ei2 = torch.cat([one + b * n for b in range(B)], 1).contiguous()
    bidx2 = torch.arange(B, device=DEV).repeat_interleave(n)
    off2 = torch.arange(B + 1, device=DEV) * n
    local2 = torch.arange(B * n, device=DEV) % n
    persons2 = torch.where(torch.rand(B * n, generator=g).to(DEV) < 0.8, local2 % 9, torch.full_like(local2, -1))
    amb2 = torch.rand(B * n, generator=g).to(DEV) < 0.02
    res["edge_pass"].append(edge_pass_case("8x432 fully", ei2, off2, bidx2, persons2, amb2, B))

    if args.edge_only:
        print(json.dumps(res, indent=1))
        return
    # ---- 2. the whole label construction ----
    hm_l, gt, fac = syn.make_labelled_heatmaps(1000, B, J, H, W, 9)
    hm_l, gt, fac = torch.from_numpy(hm_l).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(fac).to(DEV)
    lab_out = gc(hm_l, gt, fac)
    res["construct"] = dict(N=int(lab_out[7].shape[0]), E=int(lab_out[2].shape[1]),
                            gt_joints=int((gt[..., 2] != 0).sum()), matched=int(lab_out[4].sum()),
                            positive_edges=int(lab_out[3].sum()),
                            with_gt_ms=host_ms(lambda: gc(hm_l, gt, fac)),
                            without_gt_ms=host_ms(lambda: gc(hm_l, None, None)))
    try:
        ref = torch_labels(lab_out, gt, fac, H, W, B, J)
        slots = (3, 4, 5, 8, 9, 10, 13)
        res["construct"]["torch_labels_mismatches"] = {i: int((a != lab_out[i]).sum()) for i, a in zip(slots, ref)}
        from tests import labels_oracle as lo
        mine = lo.construct_labels(lab_out[7].cpu().numpy(), lab_out[12].cpu().numpy(), lab_out[2].cpu().numpy(),
                                   gt.cpu().numpy(), fac.cpu().numpy(), H, W, B, J, 6, True, False, MR, IR)
        res["construct"]["oracle_mismatches"] = {i: int((mine[i] != lab_out[i].cpu().numpy()).sum()) for i in slots}
        res["construct"]["torch_labels_ms"] = host_ms(lambda: torch_labels(lab_out, gt, fac, H, W, B, J))
    except ImportError:
        res["construct"]["torch_labels_ms"] = None
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
