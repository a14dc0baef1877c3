"""Generate ``tests/golden/*.npz`` by running the REFERENCE's own hot-path code on CPU.

TEST INFRASTRUCTURE, container-only (needs ``/root/reference``). Run:
    PYTHONDONTWRITEBYTECODE=1 python -B oracle/gen_golden.py [case names: only these are written]
The reference's ``NaiveGraphConstructor.construct_graph`` (ConstructGraph.py:46-249) and
``NodeClassificationMPNSimple.forward`` (NodeClassificationMPNSimple.py:62-97) are executed from
``/root/reference`` under ``oracle/ref_shims.py``. Each fixture stores the inputs that are not
closed-form (heatmaps, masks) and the reference outputs. Before a fixture is written, the
oracle restatement (``oracle/restate.py``) is checked against it; a draw whose top-k boundary
ties would make the reference's (unspecified) tie order matter is re-drawn, never stored.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import restate                       # noqa: E402
from oracle.ref_shims import load_reference      # noqa: E402
import pemp_amd.config as pcfg                   # noqa: E402  (plain config data, no HIP)
from pemp_amd import synthetic as syn             # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FEATURE_SALT, TAG_SALT = 0.25, 0.75


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def gc_inputs(meta):
    B, J, H, W = meta["B"], meta["J"], meta["H"], meta["W"]
    hm = syn.make_heatmaps(meta["seed"], B, J, H, W, meta["persons"], variant=meta["variant"])
    feats = syn.closed_form((B, meta["C"], H, W), FEATURE_SALT)
    tags = syn.closed_form((B, J, H, W, meta["F"]), TAG_SALT)
    masks = None
    if meta["mask_crowds"]:
        rng = np.random.default_rng(meta["seed"] + 99)
        masks = (rng.random((B, H, W)) > 0.05).astype(np.float32)
    return hm, feats, tags, masks


def gc_config(meta):
    g = pcfg.inference_gc_config(meta["graph"], meta["pool"], meta["mask_crowds"])
    g.DETECT_THRESHOLD = meta["thr"]
    if "features" in meta:
        g.EDGE_FEATURES_TO_USE = list(meta["features"])
    if "hybrid_k" in meta:
        g.HYBRID_K = meta["hybrid_k"]
    if "norm" in meta:
        g.NORM_NODE_DISTANCE = bool(meta["norm"])
    return g


def run_reference_gc(cg, meta, hm, feats, tags, masks):
    g = gc_config(meta)
    gcn = cg.NaiveGraphConstructor(torch.from_numpy(hm), torch.from_numpy(tags), torch.from_numpy(feats),
                                   None, None, None if masks is None else torch.from_numpy(masks),
                                   torch.device("cpu"), g, True, None, meta["J"])
    return gcn.construct_graph()


def make_gc_case(cg, name, meta, store_full):
    for attempt in range(20):
        hm, feats, tags, masks = gc_inputs(meta)
        ref = run_reference_gc(cg, meta, hm, feats, tags, masks)
        mine = restate.construct_graph(torch.from_numpy(hm), torch.from_numpy(feats), torch.from_numpy(tags),
                                       None if masks is None else torch.from_numpy(masks), gc_config(meta), meta["J"])
        ok = all(torch.equal(ref[i], mine[i]) for i in (0, 1, 2, 7, 11, 12, 14))
        if ok:
            break
        meta["seed"] += 1000                 # boundary tie -> re-draw (never stored)
    else:
        raise RuntimeError(f"{name}: restatement disagrees with the reference on every draw")
    x, ea, ei, det, sc, bi, tg = ref[0], ref[1], ref[2], ref[7], ref[11], ref[12], ref[14]
    arrays = {"scoremaps": hm}
    if masks is not None:
        arrays["masks"] = masks
    arrays.update(joint_det=det.numpy(), joint_scores=sc.numpy(), batch_index=bi.numpy(),
                  joint_tags=tg.numpy())
    meta.update(N=int(det.shape[0]), E=int(ei.shape[1]), sha_x=sha(x), sha_edge_attr=sha(ea),
                sha_edge_index=sha(ei), sha_joint_tags=sha(tg))
    if store_full:
        arrays.update(x=x.numpy(), edge_attr=ea.numpy(), edge_index=ei.numpy())
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), meta=json.dumps(meta), **arrays)
    print(f"{name}: N={meta['N']} E={meta['E']} seed={meta['seed']}")
    return ref


def mpn_cfg(meta):
    c = pcfg.published_mpn_config(meta["J"], meta["steps"], meta["variant"])
    if meta.get("aggr_sub") is not None:
        c.AGGR_SUB = meta["aggr_sub"]
        c.AGGR = meta["aggr"]
    if meta.get("update_mlp"):
        c.USE_NODE_UPDATE_MLP = True
    if meta.get("edge_in"):
        c.EDGE_INPUT_DIM = meta["edge_in"]
    if meta.get("update_type"):
        c.UPDATE_TYPE = meta["update_type"]
    if meta.get("edge_mlp"):
        c.EDGE_MLP = meta["edge_mlp"]
    if meta.get("late_fusion"):
        c.LATE_FUSION_POS = True
        c.EDGE_EMB.BN = True
    if meta.get("node_summary"):
        c.NODE_TYPE_SUMMARY = meta["node_summary"]
    return c


def make_mpn_case(MPN, name, meta, graph):
    torch.manual_seed(0)
    cfg = mpn_cfg(meta)
    model = MPN(cfg)
    sd = syn.closed_form_state_dict(model, meta["salt"], meta.get("attn_gain", 1.0), meta.get("weight_gain", 1.0))
    model.load_state_dict(sd)
    model.eval()
    x, ea, ei, det = graph[0], graph[1], graph[2], graph[7]
    with torch.no_grad():
        pe, pn, pc, _ = model(x, ea, ei, node_types=det[:, 2])
        mine = restate.mpn_forward(sd, cfg, x, ea, ei, det[:, 2])
    err = max((a - b).abs().max().item() for a, b in zip(pe + pn + pc, mine[0] + mine[1] + mine[2]))
    assert err < 1e-4, f"{name}: restatement vs reference max err {err}"
    meta.update(N=int(x.shape[0]), E=int(ei.shape[1]), restate_err=err,
                n_params=sum(v.numel() for v in sd.values()))
    arrays = dict(x=x.numpy(), edge_attr=ea.numpy(), edge_index=ei.numpy(), node_types=det[:, 2].numpy(),
                  edge_logits=pe[-1].numpy(), node_logits=pn[-1].numpy(), class_logits=pc[-1].numpy(),
                  n_edge_preds=np.int64(len(pe)), n_node_preds=np.int64(len(pn)))
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), meta=json.dumps(meta), **arrays)
    print(f"{name}: N={meta['N']} E={meta['E']} restate_err={err:.2e}")


GC_CASES = {
    # name: (meta, store_full)
    "gc_small_fully": (dict(seed=1, B=2, J=17, H=96, W=96, C=128, F=1, persons=2, variant="clean",
                            graph="fully", pool=5, thr=0.1, mask_crowds=False), True),
    "gc_realistic_knn": (dict(seed=2, B=1, J=17, H=128, W=128, C=128, F=2, persons=1, variant="realistic",
                              graph="knn", pool=5, thr=0.1, mask_crowds=False), True),
    "gc_noisy_masked_j14": (dict(seed=3, B=1, J=14, H=96, W=112, C=128, F=1, persons=4, variant="noisy",
                                 graph="fully", pool=3, thr=0.1, mask_crowds=True), True),
    "gc_c1_512": (dict(seed=4, B=1, J=17, H=512, W=512, C=128, F=1, persons=2, variant="clean",
                       graph="fully", pool=5, thr=0.1, mask_crowds=False), True),
    "gc_c2_like": (dict(seed=5, B=1, J=17, H=160, W=160, C=128, F=1, persons=9, variant="clean",
                        graph="fully", pool=5, thr=0.1, mask_crowds=False), False),
    "gc_knn_large": (dict(seed=6, B=1, J=17, H=192, W=192, C=128, F=1, persons=6, variant="clean",
                          graph="knn", pool=3, thr=0.1, mask_crowds=False), False),
    "gc_no_threshold": (dict(seed=7, B=1, J=17, H=64, W=80, C=128, F=1, persons=2, variant="noisy",
                             graph="fully", pool=3, thr=2.0, mask_crowds=False), False),
    "gc_ae_pos_conn_f2": (dict(seed=10, B=2, J=17, H=96, W=96, C=128, F=2, persons=2, variant="clean",
                               graph="fully", pool=5, thr=0.1, mask_crowds=False,
                               features=["ae_normed", "position", "connection_type"]), True),
    "gc_ae_pos_conn_f1": (dict(seed=11, B=1, J=17, H=96, W=96, C=128, F=1, persons=3, variant="clean",
                               graph="knn", pool=5, thr=0.1, mask_crowds=False,
                               features=["ae_normed", "position", "connection_type"]), False),
    "gc_ae": (dict(seed=12, B=1, J=14, H=80, W=96, C=128, F=1, persons=2, variant="noisy",
                   graph="fully", pool=3, thr=0.1, mask_crowds=False, features=["ae"]), False),
    "gc_ae_normed_f2": (dict(seed=13, B=1, J=14, H=80, W=96, C=128, F=2, persons=2, variant="clean",
                             graph="fully", pool=5, thr=0.1, mask_crowds=False, features=["ae_normed"]), False),
    "gc_ae_tracking_f2": (dict(seed=14, B=2, J=17, H=64, W=64, C=128, F=2, persons=2, variant="clean",
                               graph="fully", pool=5, thr=0.1, mask_crowds=False, features=["ae_tracking_1"]), False),
    # feature_knn_mpn_graph (ConstructGraph.py:370-374): knn over the 128-d node features
    "gc_feature_knn": (dict(seed=15, B=2, J=17, H=128, W=128, C=128, F=1, persons=6, variant="clean",
                            graph="feature_knn", pool=5, thr=0.1, mask_crowds=False), False),
    "gc_feature_knn_small": (dict(seed=16, B=2, J=14, H=64, W=80, C=32, F=2, persons=2, variant="noisy",
                                  graph="feature_knn", pool=3, thr=0.1, mask_crowds=False,
                                  features=["position", "connection_type", "ae_normed"]), True),
    "gc_score_based": (dict(seed=8, B=2, J=17, H=128, W=128, C=128, F=1, persons=6, variant="clean",
                            graph="score_based", pool=5, thr=0.1, mask_crowds=False), False),
    "gc_score_based_nothr": (dict(seed=9, B=1, J=17, H=64, W=80, C=128, F=1, persons=2, variant="noisy",
                                  graph="score_based", pool=3, thr=2.0, mask_crowds=False), False),
    # the edge-feature modes without tags (ConstructGraph.py:326-335); the angle cases keep edge_attr in full and
    # flag its theta column, which the tests compare within 2 ulp (acos differs between libraries at the last ulp)
    "gc_conn_only_j14": (dict(seed=20, B=2, J=14, H=80, W=96, C=16, F=1, persons=2, variant="clean",
                              graph="fully", pool=5, thr=0.1, mask_crowds=False, features=["connection_type"]), False),
    "gc_nothing": (dict(seed=21, B=2, J=17, H=96, W=80, C=16, F=1, persons=2, variant="clean",
                        graph="fully", pool=5, thr=0.1, mask_crowds=False, features=["nothing"]), False),
    "gc_position": (dict(seed=22, B=2, J=17, H=96, W=80, C=16, F=1, persons=2, variant="clean",
                         graph="fully", pool=3, thr=0.1, mask_crowds=False, features=["position"]), False),
    "gc_angle_fully": (dict(seed=23, B=2, J=17, H=80, W=96, C=16, F=1, persons=2, variant="clean",
                            graph="fully", pool=5, thr=0.1, mask_crowds=False, theta_col=2,
                            features=["position", "angle", "connection_type"]), True),
    "gc_angle_knn": (dict(seed=24, B=1, J=17, H=96, W=96, C=16, F=1, persons=5, variant="clean",
                          graph="knn", pool=5, thr=0.1, mask_crowds=False, theta_col=2,
                          features=["position", "angle", "connection_type"]), True),
    # HYBRID_K other than 5 with the threshold set, NORM_NODE_DISTANCE False (the reference's default config)
    "gc_k1": (dict(seed=25, B=1, J=17, H=64, W=96, C=16, F=1, persons=2, variant="noisy",
                   graph="fully", pool=3, thr=0.1, mask_crowds=False, hybrid_k=1), False),
    "gc_k9": (dict(seed=26, B=1, J=14, H=64, W=80, C=16, F=1, persons=2, variant="noisy",
                   graph="fully", pool=3, thr=0.1, mask_crowds=True, hybrid_k=9), False),
    "gc_k32": (dict(seed=27, B=1, J=14, H=96, W=64, C=16, F=1, persons=1, variant="noisy",
                    graph="fully", pool=3, thr=0.1, mask_crowds=False, hybrid_k=32), False),
    "gc_norm_off": (dict(seed=28, B=2, J=17, H=96, W=80, C=16, F=1, persons=2, variant="clean",
                         graph="fully", pool=5, thr=0.1, mask_crowds=False, norm=False), False),
}

MPN_CASES = {
    # name: (meta, source gc case)
    "mpn_attn_t1": (dict(J=17, steps=1, variant="attn", salt=0.5), "gc_small_fully"),
    "mpn_attn_t3": (dict(J=17, steps=3, variant="attn", salt=1.5), "gc_realistic_knn"),
    "mpn_attn_t10": (dict(J=17, steps=10, variant="attn", salt=2.5), "gc_small_fully"),
    "mpn_attn_j14": (dict(J=14, steps=3, variant="attn", salt=3.5), "gc_noisy_masked_j14"),
    "mpn_max_t3": (dict(J=17, steps=3, variant="max", salt=4.5), "gc_realistic_knn"),
    "mpn_mean_t2": (dict(J=17, steps=2, variant="mean", salt=5.5, update_mlp=True), "gc_small_fully"),
    "mpn_add_t2": (dict(J=17, steps=2, variant="add", salt=6.5), "gc_c1_512"),
    "mpn_pertype_sum_t2": (dict(J=17, steps=2, variant="attn", salt=7.5, aggr_sub="None", aggr="add"),
                           "gc_realistic_knn"),
    "mpn_pertype_max_t2": (dict(J=17, steps=2, variant="attn", salt=8.5, aggr_sub="None", aggr="max"),
                           "gc_small_fully"),
    "mpn_attn_c2_t3": (dict(J=17, steps=3, variant="attn", salt=9.5), "gc_c2_like"),
    "mpn_attn_ae_t2": (dict(J=17, steps=2, variant="attn", salt=11.5, edge_in=20), "gc_ae_pos_conn_f2"),
    "mpn_attn_hmlp_t2": (dict(J=17, steps=2, variant="attn", salt=12.5, update_type="hierarch_mlp"),
                         "gc_small_fully"),
    "mpn_max_hmlp_j14_t2": (dict(J=14, steps=2, variant="attn", salt=13.5, update_type="hierarch_mlp",
                                 aggr_sub="None", aggr="max"), "gc_noisy_masked_j14"),
    "mpn_attn_hcnn_t3": (dict(J=17, steps=3, variant="attn", salt=14.5, update_type="hierarch_cnn"),
                         "gc_realistic_knn"),
    "mpn_attn_ept_t2": (dict(J=17, steps=2, variant="attn", salt=15.5, edge_mlp="per_type"), "gc_realistic_knn"),
    "mpn_attn_ept_pt_t3": (dict(J=17, steps=3, variant="attn", salt=16.5, edge_mlp="per_type",
                                aggr_sub="node_edge_attn_per_type", aggr="add", attn_gain=16.0), "gc_small_fully"),
    "mpn_max_latefusion_t3": (dict(J=17, steps=3, variant="max", salt=17.5, late_fusion=True), "gc_realistic_knn"),
    "mpn_attn_latefusion_t2": (dict(J=17, steps=2, variant="attn", salt=18.5, late_fusion=True), "gc_small_fully"),
    "mpn_attn_pertype_t2": (dict(J=17, steps=2, variant="attn", salt=10.5, aggr_sub="node_edge_attn_per_type",
                                 aggr="add", attn_gain=16.0), "gc_realistic_knn"),
    # NODE_TYPE_SUMMARY type LUTs (src/Models/MessagePassingNetwork/utils.py:11-19): 9 / 6 merged types
    "mpn_attn_lr_t3": (dict(J=17, steps=3, variant="attn", salt=19.5, node_summary="left_right"), "gc_realistic_knn"),
    "mpn_attn_pbp_t2": (dict(J=17, steps=2, variant="attn", salt=20.5, node_summary="per_body_part"),
                        "gc_small_fully"),
    "mpn_pertype_max_lr_t2": (dict(J=17, steps=2, variant="attn", salt=21.5, aggr_sub="None", aggr="max",
                                   node_summary="left_right"), "gc_small_fully"),
    "mpn_pertype_max_pbp_t3": (dict(J=17, steps=3, variant="attn", salt=22.5, aggr_sub="None", aggr="max",
                                    node_summary="per_body_part"), "gc_realistic_knn"),
    # trained-checkpoint logit magnitudes (every Linear weight x2: |logit| up to ~50)
    "mpn_attn_gain2_t3": (dict(J=17, steps=3, variant="attn", salt=9.5, weight_gain=2.0), "gc_c2_like"),
}


def main(only=()):
    """Regenerate every case, or only the cases named in `only` (every other fixture stays as it is): a named
    graph case is rewritten alone; for a named MPN case its source graph is rebuilt in memory."""
    os.makedirs(OUT, exist_ok=True)
    cg, MPN, _ = load_reference()
    graphs = {}
    mpn_names = [n for n in MPN_CASES if not only or n in only]
    need = {MPN_CASES[n][1] for n in mpn_names}
    for name, (meta, full) in GC_CASES.items():
        if only and name not in only and name not in need:
            continue
        if only and name not in only:    # re-run the reference on the stored case's (final) seed
            stored = json.loads(str(np.load(os.path.join(OUT, f"{name}.npz"))["meta"]))
            m = dict(meta, seed=stored["seed"])
            hm, feats, tags, masks = gc_inputs(m)
            graphs[name] = run_reference_gc(cg, m, hm, feats, tags, masks)
            assert sha(graphs[name][2]) == stored["sha_edge_index"], f"{name}: stored fixture not reproduced"
        else:
            graphs[name] = make_gc_case(cg, name, dict(meta), full)
    for name in mpn_names:
        meta, src = MPN_CASES[name]
        make_mpn_case(MPN, name, dict(meta), graphs[src])


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
