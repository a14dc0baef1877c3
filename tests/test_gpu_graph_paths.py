"""The launches one construct_graph() call queues (graph_constructor.py: the step entry, the capacity build for
projected features, the exact build), pinned per path: the library profiler's whole report of the call,
label -> launches, equals a table.

Every case is a B, J, H, W = 2, 17, 96, 104 batch with 128 closed-form feature channels and the published `attn`
T=3 model in f16x3 bound (bind_mpn). A case starts without capacity hints or step plans and with the detection
capacity at 512; where it pins a repeated batch shape, an unprofiled 3-person call sets the hint first. The tables
were recorded from the driver before it was split into a call record and three stages, and must hold unchanged."""
import pytest
import torch

import pemp_amd
from pemp_amd import _lib, config as pcfg, synthetic as syn
from pemp_amd.frontend import ProjectedMaps
from pemp_amd.graph_constructor import NaiveGraphConstructor
from pemp_amd.mpn import model as mm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, J, H, W = 2, 17, 96, 104

DETECT = {"detect_nms": 1, "detect_select_emit": 1}
# the step entry: detection, capacity build and the bound model's capacity-mode forward
STEP = {**DETECT, "graph_build": 1, "mpn_prepare_fully": 1, "node_embed": 1, "node_table": 1, "edge_embed": 1,
        "edge_step": 2, "node_update_table": 2, "edge_step_head": 1, "node_update": 1}
# name: (graph type, features, tagmaps, persons of the priming call or None, (seed, persons) of the profiled call,
#        the following model call takes the queued result, expected report)
CASES = {
    "fully_first": ("fully", "dense", False, None, (1, 3), False, {**DETECT, "graph_build": 1}),
    "fully_step": ("fully", "dense", False, 3, (2, 2), True, STEP),
    "fully_step_overflow": ("fully", "dense", False, 3, (4, 6), False, {**STEP, "graph_build": 2}),
    "fully_projected_cap": ("fully", "projected", False, 3, (2, 2), False,
                            {**DETECT, "graph_build": 1, "gather_projected": 1}),
    "knn": ("knn", "dense", False, None, (5, 5), False, {**DETECT, "pack_nodes": 1, "knn_build": 1}),
    "fully_tags_step": ("fully", "dense", True, 3, (2, 2), True, STEP),
}


def construct(gtype, feats, tags, seed, persons):
    hm = torch.from_numpy(syn.make_heatmaps(seed, B, J, H, W, persons, margin=4)).to(DEV)
    gc = pcfg.inference_gc_config(gtype, 5, False)
    return pemp_amd.get_graph_constructor(gc, scoremaps=hm, features=feats, tagmaps=tags, joints_gt=None,
                                          factor_list=None, masks=None, device=DEV, testing=True, heatmaps=None,
                                          num_joints=J).construct_graph()


@pytest.mark.parametrize("name", list(CASES))
def test_construct_launches(name, monkeypatch):
    gtype, fkind, with_tags, prime, (seed, persons), takes, expected = CASES[name]
    with NaiveGraphConstructor._mu:
        NaiveGraphConstructor._graph_hint.clear()
        NaiveGraphConstructor._plans.clear()
        NaiveGraphConstructor._cap = 512
    model = pemp_amd.get_mpn_model(pcfg.published_mpn_config(J, 3, "attn"))
    model.load_state_dict(syn.closed_form_state_dict(model, 1.25, 1.0, 1.0))
    model.precision = "f16x3"
    model = model.eval().to(DEV)
    if fkind == "projected":
        feats = ProjectedMaps([torch.from_numpy(syn.closed_form((B, 128, H // 2, W // 2), 0.25)).to(DEV)], (H, W))
    else:
        feats = torch.from_numpy(syn.closed_form((B, 128, H, W), 0.25)).to(DEV)
    tags = torch.from_numpy(syn.closed_form((B, J, H, W, 1), 0.75)).to(DEV) if with_tags else None
    taken = []
    orig_take = mm.NodeClassificationMPNSimple._take_cap

    def take(self, *a):
        r = orig_take(self, *a)
        taken.append(r is not None)
        return r

    monkeypatch.setattr(mm.NodeClassificationMPNSimple, "_take_cap", take)
    pemp_amd.bind_mpn(model)
    try:
        if prime is not None:
            construct(gtype, feats, tags, 1, prime)
            torch.cuda.synchronize()
        _lib.prof_enable("*")
        try:
            _lib.prof_report()
            out = construct(gtype, feats, tags, seed, persons)
            rep = _lib.prof_report()
        finally:
            _lib.prof_enable(None)
        counts = {label: n for label, (n, _) in rep.items()}
        print(f"graph_launches {name}: {counts}")
        with torch.no_grad():
            model(out[0], out[1], out[2], node_types=out[7][:, 2])
        torch.cuda.synchronize()
        assert taken == [takes]
        assert (out[14] is not None) == with_tags
        assert counts == expected
    finally:
        pemp_amd.bind_mpn(None)
