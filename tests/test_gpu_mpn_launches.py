"""The launch sequence of one inference forward (csrc/mpn.hip: plan_forward decides it, Forward::run queues it), pinned
per model variant: the library profiler's whole report of one forward, label -> launches, equals a table.

Every case is the published shape in f16x3 on the 36-node / 662-edge `small` graph of tests/mpn_shapes.py (plain
tensors: the sorting prepare, one `mpn_prepare`). A profiled forward runs serially on the launch stream and, unless
the model asks otherwise, keeps the embedding launch apart from the first pass. The tables follow from the driver:

* prelude: `node_embed` (node_rows_kernel with the embedding), the first `node_table` when there are steps, the edge
  order, and `edge_embed` when there are steps (`edge_first` instead where the fused first pass runs: it is pass 0 too);
* per step the edge pass -- `edge_step`, or `edge_step_head` on the last AUX_LOSS_STEPS + 1 steps, which record
  logits -- and then the node step: where the update block rides in the edge pass (attention) an unrecorded middle
  step is one `node_update_table` launch; every other middle step is `node_update` + `node_table`, and the last step
  a `node_update` with the heads. EDGE_MLP per_type keeps the two launches (its table needs the per-type columns),
  and a hierarchical update runs its MLP as a `node_update` of its own: two on the last step, where the heads follow."""
import functools

import pytest
import torch

import pemp_amd
from pemp_amd import _lib, config as pcfg, synthetic as syn
from tests import mpn_shapes as ms

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

PRELUDE = {"mpn_prepare": 1, "node_embed": 1, "node_table": 1, "edge_embed": 1}
# two launches per middle step, three steps (max, mean, EDGE_MLP per_type)
UNFUSED = {**PRELUDE, "node_table": 3, "edge_step": 2, "node_update": 3, "edge_step_head": 1}
# name: (variant, steps, AUX_LOSS_STEPS, other config keys, fuse_first_pass, expected report)
CASES = {
    "attn": ("attn", 3, 0, {}, None,
             {**PRELUDE, "edge_step": 2, "node_update_table": 2, "edge_step_head": 1, "node_update": 1}),
    "attn_aux1": ("attn", 3, 1, {}, None,
                  {**PRELUDE, "node_table": 2, "edge_step": 1, "node_update_table": 1, "edge_step_head": 2,
                   "node_update": 2}),
    "attn_steps1": ("attn", 1, 0, {}, None, {**PRELUDE, "edge_step_head": 1, "node_update": 1}),
    "steps0": ("attn", 0, 0, {}, None, {"mpn_prepare": 1, "node_embed": 1}),
    "max": ("max", 3, 0, {}, None, UNFUSED),
    "mean": ("mean", 3, 0, {}, None, UNFUSED),
    "edge_mlp_per_type": ("attn", 3, 0, {"EDGE_MLP": "per_type"}, None, UNFUSED),
    "hierarch_mlp": ("attn", 3, 0, {"UPDATE_TYPE": "hierarch_mlp"}, None, {**UNFUSED, "node_update": 4}),
    "attn_fused_first": ("attn", 3, 0, {}, True,
                         {"mpn_prepare": 1, "node_embed": 1, "node_table": 1, "edge_first": 1, "edge_step": 1,
                          "node_update_table": 2, "edge_step_head": 1, "node_update": 1}),
}


@functools.lru_cache(maxsize=None)
def graph():
    return tuple(t.to(DEV) for t in ms.case_graph(pcfg.published_mpn_config(ms.J, 3, "attn"), "small"))


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence(name):
    variant, steps, aux, over, fuse, expected = CASES[name]
    cfg = pcfg.published_mpn_config(ms.J, steps, variant)
    cfg.AUX_LOSS_STEPS = aux
    for key, val in over.items():
        assert key in cfg, key
        cfg[key] = val
    model = pemp_amd.get_mpn_model(cfg)
    model.load_state_dict(syn.closed_form_state_dict(model, ms.SALT, attn_gain=ms.GAINS[0], weight_gain=ms.GAINS[1]))
    model.precision = "f16x3"
    model.fuse_first_pass = fuse
    model = model.eval().to(DEV)
    x, ea, ei, types = graph()
    _lib.prof_enable("*")
    try:
        _lib.prof_report()
        with torch.no_grad():
            out = model(x, ea, ei, node_types=types)
        rep = _lib.prof_report()
    finally:
        _lib.prof_enable(None)
    counts = {label: n for label, (n, _) in rep.items()}
    print(f"mpn_launches {name}: {counts}")
    assert model.precision == "f16x3"
    assert [len(o) for o in out[:3]] == [min(steps, aux + 1), min(steps, aux + 1) + 1, min(steps, aux + 1) + 1]
    assert counts == expected
