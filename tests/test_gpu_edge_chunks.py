"""The edge passes' per-edge segment positions (mpn.hip: edge_ranges_kernel packs each edge's distance to the first
and last edge of its (target, type) segment, clamped to 15, into the high byte of its sorted-target entry; every
tile of every pass rebuilds its chunk structure from them). Hand-built graphs at the sizes where that table can go
wrong, through the model's forward as tests/test_gpu_mpn.py runs it: logits against the CPU oracle at the suite's
bar (1e-4, as test_vs_oracle applies it) and a second forward bit-identical to the first."""
import functools

import pytest
import torch

import pemp_amd
from oracle import restate
from pemp_amd import config as pcfg, synthetic as syn
from tests.test_gpu_mpn import DEV, TOL, graph, make_model, max_err, run

pytestmark = pytest.mark.gpu
J = 17
N_NODES = 128
# Segment lengths in sorted order (one segment per target, targets ascending). With well under 65536 edges every
# workgroup's nominal share is one 16-edge tile, moved forward to the next segment start, so:
#   16 then 560: the first workgroup's range is both segments, 36 tiles over 16 waves (2 or 3 each). Wave 0's
#     first tile is the 16-edge segment exactly: it ends at the tile end and the next tile starts another target (no
#     carry). Every other wave lies inside the 560-edge segment: it is cut by wave-range boundaries, a wave's middle
#     tile takes a carry in and hands one out, and the next 35 nominal workgroup boundaries fall inside the segment
#     (moved to its end: workgroups without a range);
#   1, 2, 15, 16, 17, 31, 32, 33, 100: the clamp at 15 on both sides, segments that start at a tile origin and ones
#     that do not (the origins follow the moved range starts), tiles holding several segments;
#   the tail: a seeded mix of short and medium segments.
LENGTHS = [16, 560, 1, 2, 15, 16, 17, 31, 32, 33, 100, 16, 16, 1, 1, 1, 30, 2, 47, 3, 16, 5, 64, 1, 15, 17, 48, 7, 9, 33]
EMPTY_TARGETS = (0, 5, 6, 50)          # targets without edges (their segments are empty)
ATTN_GAIN = 4.0                        # sharpened attention: a wrong segment maximum or normaliser moves the logits


def build_graph(type_values, lengths_per_type, seed):
    """Nodes of the given types (type_values[k] for a share of the nodes); for each type the listed segment lengths,
    one per target in ascending order (skipping EMPTY_TARGETS), the sources cycling through that type's nodes -- a
    segment longer than the type has nodes repeats (source, target) pairs, which the model sums like any edges."""
    g = torch.Generator().manual_seed(seed)
    shares = [N_NODES - 24 * (len(type_values) - 1)] + [24] * (len(type_values) - 1)
    types = torch.cat([torch.full((n,), t, dtype=torch.long) for t, n in zip(type_values, shares)])
    types = types[torch.randperm(N_NODES, generator=g)]
    targets = [d for d in range(N_NODES) if d not in EMPTY_TARGETS]
    src, dst = [], []
    for t, lengths in zip(type_values, lengths_per_type):
        nodes = (types == t).nonzero().flatten()
        assert len(lengths) <= len(targets)
        for d, n in zip(targets, lengths):
            off = int(torch.randint(0, len(nodes), (1,), generator=g))
            src.append(nodes[(torch.arange(n) + off) % len(nodes)])
            dst.append(torch.full((n,), d, dtype=torch.long))
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    perm = torch.randperm(ei.shape[1], generator=g)              # the order of the list is free
    ei = ei[:, perm].contiguous()
    x = torch.rand(N_NODES, 128, generator=g) * 2 - 1
    ea = torch.rand(ei.shape[1], J + 2, generator=g) * 2 - 1
    return x, ea, ei, types


@functools.lru_cache(maxsize=None)
def segments_graph(n_types):
    if n_types == 1:                   # one source type (the agnostic aggregations ignore the types anyway)
        return build_graph([4], [LENGTHS], 1)
    # three source types with edges (14 of the 17 without): the long list on the first, rotated lists on the others
    return build_graph([2, 7, 16], [LENGTHS, LENGTHS[2:11] + [1, 16, 16, 17], [33, 1, 32, 15, 2]], 3)


@functools.lru_cache(maxsize=None)
def oracle_logits(variant, n_types, aux):
    """(cfg, oracle logits) of one graph and model: computed once, shared by the precisions."""
    cfg = pcfg.published_mpn_config(J, 3, variant)
    cfg.AUX_LOSS_STEPS = aux
    m = pemp_amd.get_mpn_model(cfg)
    sd = syn.closed_form_state_dict(m, 0.375 + J, ATTN_GAIN, 1.0)
    x, ea, ei, types = segments_graph(n_types)
    ref = restate.mpn_forward(sd, cfg, x, ea, ei, types)
    return cfg, ref


def check(model, inputs, ref):
    pe, pn, pc, _ = run(model, *inputs)
    rpe, rpn, rpc = ref[:3]
    assert len(pe) == len(rpe) and len(pn) == len(rpn) and len(pc) == len(rpc)
    for a, b in zip(pe + pn + pc, rpe + rpn + rpc):
        assert a.shape == b.shape
        assert max_err(a, b) < TOL
    again = run(model, *inputs)
    for a, b in zip(pe + pn + pc, again[0] + again[1] + again[2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("variant,n_types", [("attn", 3), ("attn", 1), ("max", 1), ("mean", 1)])
def test_segment_shapes(variant, n_types, prec):
    cfg, ref = oracle_logits(variant, n_types, 0)
    model, _ = make_model(cfg, 0.375 + J, prec, ATTN_GAIN)
    check(model, segments_graph(n_types), ref)


def test_recorded_middle_pass():
    """AUX_LOSS_STEPS 1: the second of three passes records the edge head while it still writes the next r (the
    12-wave range table, other tile origins over the same packed positions)."""
    cfg, ref = oracle_logits("attn", 3, 1)
    assert len(ref[0]) == 2
    model, _ = make_model(cfg, 0.375 + J, "f16x3", ATTN_GAIN)
    check(model, segments_graph(3), ref)


@pytest.mark.parametrize("variant", ["attn", "max"])
def test_tiny_edge_counts(variant):
    """E = 1, 15, 16, 17 (a last tile of 1, 15, 16 lanes and a second tile of one lane), as one segment and as
    one-edge segments."""
    cfg = pcfg.published_mpn_config(J, 3, variant)
    model, sd = make_model(cfg, 1.625, "f16x3")
    g = torch.Generator().manual_seed(5)
    n = 20
    x = torch.rand(n, 128, generator=g) * 2 - 1
    types = torch.full((n,), 3, dtype=torch.long)
    for E in (1, 15, 16, 17):
        for one_segment in (True, False):
            src = torch.arange(E) % n
            dst = torch.full((E,), 19) if one_segment else (torch.arange(E) + 1) % n
            ei = torch.stack([src, dst])
            ea = torch.rand(E, J + 2, generator=g) * 2 - 1
            check(model, (x, ea, ei, types), restate.mpn_forward(sd, cfg, x, ea, ei, types))


def test_knn_graph():
    g = graph(2, J, 160, 160, 9, "knn")
    cfg = pcfg.published_mpn_config(J, 3, "attn")
    model, sd = make_model(cfg, 0.875, "f16x3")
    x, ea, ei, types = g[0], g[1], g[2], g[7][:, 2]
    check(model, (x, ea, ei, types), restate.mpn_forward(sd, cfg, x, ea, ei, types))


def test_capacity_mode_refreshes_positions():
    """Capacity mode (bind_mpn, as test_capacity_mode_mpn): the device-side edge count lies below the capacity, so
    padded positions follow the last real edge, and the next batch -- another graph in the same capacity -- must
    get its own positions, not the previous batch's. Each queued result equals the exact forward on copies of the
    same graph bit for bit and the oracle within the bar."""
    from pemp_amd.graph_constructor import NaiveGraphConstructor
    from pemp_amd.mpn import model as mm
    B, H, W = 2, 96, 104
    NaiveGraphConstructor._graph_hint.clear()
    NaiveGraphConstructor._cap = 512
    gc = pcfg.inference_gc_config("fully", 5, False)
    cfg = pcfg.published_mpn_config(J, 3, "attn")
    model, sd = make_model(cfg, 1.25, "f16x3")
    feats = torch.from_numpy(syn.closed_form((B, 128, H, W), 0.25))
    taken = []
    orig_take = mm.NodeClassificationMPNSimple._take_cap

    def take(self, *a):
        r = orig_take(self, *a)
        taken.append(r is not None)
        return r

    mm.NodeClassificationMPNSimple._take_cap = take
    pemp_amd.bind_mpn(model)
    try:
        used, edges = [], []
        for seed, persons in ((1, 3), (2, 2), (3, 3), (4, 1)):   # the first call sets the capacities (exact build)
            hm = torch.from_numpy(syn.make_heatmaps(seed, B, J, H, W, persons, margin=4))
            out = pemp_amd.get_graph_constructor(gc, scoremaps=hm.to(DEV), features=feats.to(DEV), tagmaps=None,
                                                 joints_gt=None, factor_list=None, masks=None, device=DEV,
                                                 testing=True, heatmaps=None, num_joints=J).construct_graph()
            x, ea, ei, types = out[0], out[1], out[2], out[7][:, 2]
            taken.clear()
            got = run(model, x, ea, ei, types)
            used.append(bool(taken and taken[0]))
            edges.append(ei.shape[1])
            exact = run(model, x.clone(), ea.clone(), ei.clone(), types.clone())
            ref = restate.mpn_forward(sd, cfg, x.cpu(), ea.cpu(), ei.cpu(), types.cpu())
            for a, b, r in zip(got[0] + got[1] + got[2], exact[0] + exact[1] + exact[2], ref[0] + ref[1] + ref[2]):
                assert a.shape == b.shape and torch.equal(a, b), (seed, persons)
                assert max_err(a, r) < TOL
        assert used == [False, True, True, True], used
        # batches of 2 and 1 persons lie below the capacities the 3-person batch set; every batch is another graph
        assert edges[1] < edges[0] and edges[3] < edges[0] and len(set(edges)) == 4, edges
    finally:
        pemp_amd.bind_mpn(None)
        mm.NodeClassificationMPNSimple._take_cap = orig_take
