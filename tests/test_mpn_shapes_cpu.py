"""Preconditions of tests/test_gpu_mpn_shapes.py, checked without a GPU: for every case of tests/mpn_shapes.py the
model constructs and loads its weights, the reference arithmetic alone reaches a tenth of the GPU test's bar (the
fp32 oracle against the same oracle in fp64), and the logits are large enough for a defect to show. These are
conditions on the inputs, not measurements of the code under test."""
import pytest

from tests import mpn_shapes as ms

TOL = 1e-4           # the GPU test's bar (tests/test_gpu_mpn.py)
REL_SUM = 2e-6       # plus this relative part for the unnormalised sum (AGGR add), as in test_vs_oracle
PAIRS = [(c, v) for c in ms.CASES for v in ms.variants(c)]


@pytest.mark.parametrize("case,variant", PAIRS, ids=[f"{c}-{v}" for c, v in PAIRS])
def test_reference_reaches_the_bar(case, variant):
    cfg = ms.config(case, variant)
    model, sd = ms.state_dict(cfg, ms.gains_for(variant))          # constructs; load_state_dict (strict) inside
    assert list(model.state_dict().keys()) == list(sd.keys())
    r32 = ms.oracle(case, variant, "small")
    r64 = ms.oracle(case, variant, "small", double=True)
    assert tuple(len(r) for r in r64) == ms.CASES[case].lengths
    rel = REL_SUM if variant == "add" else 0.0
    err = max(((a.double() - b).abs() - rel * b.abs()).max().item() for a, b in zip(sum(r32, []), sum(r64, [])))
    top = max(b.abs().max().item() for b in sum(r64, []))
    print(f"{case}-{variant}: fp32 oracle vs fp64 {err:.2e}, largest |logit| {top:.2f}")
    assert err < TOL / 10
    assert top >= 0.5


def test_node_emb_whole_is_false_for_a_case():
    """The table reaches both forms of node_rows_kernel's embedding: the published shape's image fits the LDS whole,
    the cases with a fourth 64-wide layer or a second 128-wide one do not (one layer staged at a time)."""
    staged = set()
    for case in ms.CASES:
        cfg = ms.config(case, "attn")
        diag = [64] if case == "node_emb_relu_bn" else []           # the trailing BatchNorm's diagonal layer
        if not ms.node_emb_whole(cfg.NODE_INPUT_DIM, cfg.NODE_EMB.OUTPUT_SIZES + diag):
            staged.add(case)
    assert staged == {"node_emb4", "node_emb_relu_bn", "node_emb_128"}


def test_graphs_cut_the_tiles():
    shapes = {}
    for name, (sizes, seed) in ms.GRAPHS.items():
        x, ea, ei, types = ms.graph(sizes, ms.J, 19, 128, seed)
        N, E = x.shape[0], ei.shape[1]
        shapes[name] = (N, E)
        assert ea.shape == (E, 19) and types.shape == (N,) and int(types.min()) >= 0 and int(types.max()) < ms.J
        assert -1 <= float(x.min()) and float(x.max()) < 1 and -1 <= float(ea.min()) and float(ea.max()) < 1
        key = ei[0] * N + ei[1]
        assert bool((key[1:] > key[:-1]).all()) and bool((ei[0] != ei[1]).all())      # sorted by (src, dst), no loops
    assert shapes == {"small": (36, 662), "tile": (16, 240), "tiny": (2, 2)}
    N, E = shapes["small"]
    assert (N % 16, E % 16, E % 64) == (4, 6, 22)
