"""Model shapes other than the published one: the case table shared by tests/test_mpn_shapes_cpu.py and
tests/test_gpu_mpn_shapes.py, with the config and graph builders both use.

Every case changes only the listed keys of ``published_mpn_config``; ``plan_forward`` (csrc/mpn.hip) picks its
kernels from exactly these shapes, so each case names the launch site it reaches (``label``: the library
profiler's label of that site, None where the shape stays on the published kernels)."""
import functools

import torch

import pemp_amd
from oracle import restate
from pemp_amd import config as pcfg, synthetic as syn

J = 17
SALT, GAINS = 2.5, (4.0, 1.5)      # closed_form_state_dict(model, 2.5, attn_gain=4.0, weight_gain=1.5): |logit| ~ 1-5
# The unnormalised sum (AGGR add) grows with the in-degree: at (4.0, 1.5) its logits reach 1e4 on `small` and the fp32
# oracle is 2e-3 from fp64, at weight gain 1.0 still 7e-5 (|logit| up to 280) -- no fp32 arithmetic reaches the bar
# there. At weight gain 0.7 the node / class logits are 3 to 17 and the fp32 oracle is 3e-6 from fp64, the room the
# other aggregations have (tests/test_mpn_shapes_cpu.py checks both for every case)
GAINS_ADD = (4.0, 0.7)
FALLBACK_LABELS = ("edge_embed_wide", "edge_embed_generic", "edge_step_head_generic", "heads")

# name -> (per-image node counts, seed). 16 rows per node workgroup, 16 edges per wave tile, 64 edges per
# edge_embed_wide_kernel block: small cuts all three (N = 36, E = 662), tile fills them exactly (N = 16, E = 240),
# tiny is one tile that is almost all padding (N = 2, E = 2)
GRAPHS = {"small": ((23, 13), 1), "tile": ((16,), 2), "tiny": ((2,), 3)}


class Case:
    def __init__(self, over, label=None, lengths=(1, 2, 2), more=(), steps=None):
        self.over, self.label, self.lengths, self.more, self.steps = over, label, lengths, tuple(more), steps


CASES = {
    # node embedding (node_rows_kernel, ROWS_EMBED)
    "node32": Case({"NODE_INPUT_DIM": 32, "NODE_EMB.OUTPUT_SIZES": [32, 64, 64]}),
    "node50": Case({"NODE_INPUT_DIM": 50}),                                   # K0 % 16 != 0, K0 % 4 != 0
    "node_emb4": Case({"NODE_EMB.OUTPUT_SIZES": [128, 64, 64, 64], "NODE_EMB.BN": False}),
    "node_emb_relu": Case({"NODE_EMB.END_WITH_RELU": True, "NODE_EMB.BN": False}),
    "node_emb_relu_bn": Case({"NODE_EMB.END_WITH_RELU": True, "NODE_EMB.BN": True}),   # trailing BN: a diagonal layer
    "node_emb_128": Case({"NODE_EMB.OUTPUT_SIZES": [128, 128, 64]}),          # node_emb_whole false: per-layer staging
    # edge embedding
    "edge_in2": Case({"EDGE_INPUT_DIM": 2}),
    "edge_in17": Case({"EDGE_INPUT_DIM": 17}),
    "edge_in20": Case({"EDGE_INPUT_DIM": 20}),
    "edge_in33": Case({"EDGE_INPUT_DIM": 33}, "edge_embed_generic"),          # two k-blocks in layer 0
    "edge_in100": Case({"EDGE_INPUT_DIM": 100}, "edge_embed_wide"),
    "edge_emb_relu": Case({"EDGE_EMB.END_WITH_RELU": True, "EDGE_EMB.BN": False}, "edge_embed_generic"),
    "edge_emb_odd": Case({"EDGE_EMB.OUTPUT_SIZES": [19, 40, 64]}, "edge_embed_generic", more=("attn_per_type",)),
    "edge_emb_wide": Case({"EDGE_EMB.OUTPUT_SIZES": [128, 64]}, "edge_embed_wide"),
    # edge head (edge_step_kernel<AGG, 2, ...>, one instantiation per aggregation and precision)
    "edge_head1": Case({"EDGE_CLASS.OUTPUT_SIZES": [1]}, "edge_step_head_generic", more=("mean", "add")),
    "edge_head_40_20": Case({"EDGE_CLASS.OUTPUT_SIZES": [40, 20, 1]}, "edge_step_head_generic",
                            more=("mean", "add", "attn_per_type")),
    "edge_head_32_32": Case({"EDGE_CLASS.OUTPUT_SIZES": [32, 32, 1]}, "edge_step_head_generic", more=("mean", "add")),
    # node and class heads
    "heads_32": Case({"NODE_CLASS.OUTPUT_SIZES": [32, 32, 1], "CLASS.OUTPUT_SIZES": [32, 17]}),
    "heads_wide": Case({"NODE_CLASS.OUTPUT_SIZES": [128, 1], "CLASS.OUTPUT_SIZES": [128, 17]}, "heads"),
    "class18": Case({"CLASS.OUTPUT_SIZES": [64, 32, 18]}),                    # class width != num_types
    "bn_heads": Case({"BN": True}),                                           # MODEL.MPN.BN: all three heads
    # recorded passes
    "steps0": Case({}, lengths=(0, 1, 1), steps=0),
    "aux_gt_steps": Case({"AUX_LOSS_STEPS": 4}, lengths=(2, 3, 3), steps=2),
}
BF16_CASES = ("edge_in33", "edge_emb_relu", "edge_emb_odd", "edge_emb_wide", "edge_head1", "edge_head_40_20",
              "edge_head_32_32")


def variants(case):
    """attn and max (the agnostic layer, T = 1) for every case, plus the case's own."""
    return ("attn", "max") + CASES[case].more


def config(case, variant, steps=3):
    c = CASES[case]
    cfg = pcfg.published_mpn_config(J, steps if c.steps is None else c.steps, variant)
    for key, val in c.over.items():
        node = cfg
        *path, leaf = key.split(".")
        for p in path:
            node = node[p]
        assert leaf in node, key
        node[leaf] = val
    return cfg


def graph(sizes, J, A, C, seed):
    """(x [N, C], edge_attr [E, A], edge_index [2, E], node_types [N]): every image fully connected without self
    loops, edge_index sorted by (src, dst), features uniform in [-1, 1), types uniform in [0, J). Plain tensors
    (no graph-constructor tags): the generic sorting prepare orders the edges."""
    g = torch.Generator().manual_seed(seed)
    parts, off = [], 0
    for n in sizes:
        src, dst = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
        keep = src != dst
        parts.append(torch.stack([src[keep], dst[keep]]) + off)
        off += n
    ei = torch.cat(parts, 1).contiguous()
    x = torch.rand(off, C, generator=g) * 2 - 1
    ea = torch.rand(ei.shape[1], A, generator=g) * 2 - 1
    types = torch.randint(0, J, (off,), generator=g)
    return x, ea, ei, types


def case_graph(cfg, gname):
    sizes, seed = GRAPHS[gname]
    return graph(sizes, J, cfg.EDGE_INPUT_DIM, cfg.NODE_INPUT_DIM, seed)


def gains_for(variant):
    return GAINS_ADD if variant == "add" else GAINS


def state_dict(cfg, gains):
    model = pemp_amd.get_mpn_model(cfg)
    sd = syn.closed_form_state_dict(model, SALT, attn_gain=gains[0], weight_gain=gains[1])
    model.load_state_dict(sd)
    return model, sd


@functools.lru_cache(maxsize=None)
def oracle(case, variant, gname, gains=None, double=False):
    """restate.mpn_forward of the case on the graph, computed once per test session: (pe, pn, pc). Read only."""
    cfg = config(case, variant)
    gains = gains or gains_for(variant)
    _, sd = state_dict(cfg, gains)
    x, ea, ei, types = case_graph(cfg, gname)
    if double:
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        x, ea = x.double(), ea.double()
    return restate.mpn_forward(sd, cfg, x, ea, ei, types)[:3]


def node_emb_whole(in_dim, sizes):
    """csrc/mpn.hip node_emb_whole: the whole node embedding's LDS image fits beside node_rows_kernel's three
    16-row buffers (160 KiB); otherwise the kernel stages one layer at a time."""
    stride = lambda k: (k - 8 + 63) // 64 * 64 + 8
    pad = lambda n: (n + 15) // 16 * 16
    floats, k = 0, in_dim
    for out in sizes:
        floats += pad(out) * stride(pad(k)) + pad(out)
        k = out
    return (3 * 16 * 136 + floats) * 4 <= 160 * 1024
