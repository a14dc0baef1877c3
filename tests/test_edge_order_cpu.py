"""CPU checks of the edge-order helpers (tests/edge_order.py) and of pemp_mpn_order_layout: the numpy reference
against a brute-force loop, the planted heatmaps against the oracle's detection, the layout query as host
arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import restate
from pemp_amd import _lib, config as pcfg
from tests import edge_order as eo


@pytest.mark.parametrize("T", [5, 1])
def test_expected_order_against_brute_force(T):
    """A 30-node multigraph with duplicate edges, self loops and invalid entries (source or target outside
    [0, N), a source of a type outside [0, T)): every (type, target) segment lists its edges in edge-id order."""
    rng = np.random.default_rng(3)
    N, E = 30, 400
    ei = rng.integers(0, N, (2, E))
    ei[:, 50:60] = ei[:, 40:50]                                  # duplicates
    ei[0, [7, 100]] = (N, -1)
    ei[1, [9, 200]] = (-1, N + 5)
    types = rng.integers(0, 5, N)
    types[[4, 11]] = (5, -1)                                     # invalid for T = 5, ignored for T = 1
    seg, s_src, s_dst, s_orig = eo.expected_order(ei, types, N, T)
    want_seg, want = [0], []
    for t in range(T):
        for d in range(N):
            for e in range(E):
                s = ei[0, e]
                if 0 <= s < N and ei[1, e] == d and (types[s] if T != 1 else 0) == t:
                    want.append(e)
            want_seg.append(len(want))
    assert seg.tolist() == want_seg
    assert s_orig.tolist() == want
    assert s_src.tolist() == ei[0, want].tolist() and s_dst.tolist() == ei[1, want].tolist()
    assert E - 4 - (0 if T == 1 else int(np.isin(ei[0], [4, 11]).sum())) <= seg[-1] <= E - 4


def test_planted_heatmaps_are_detected_exactly():
    """The oracle's detection finds counts[b][j] nodes of type j in image b: at the knn prepare's image limit and
    one past it (512, 513: one type alone needs 96 x 96 planes), in an empty image, a one-node image, and an image
    past a 64-node word with an absent type."""
    J = 17
    counts = [eo.spread(512, J, absent=(5,)), [0] * J, eo.spread(1, J, absent=(5,), shift=3),
              eo.spread(68, J, absent=(5,), shift=7), eo.spread(513, J), [0] * 9 + [512] + [0] * 7]
    hm = eo.planted_heatmaps(counts, 96, 96, seed=1)
    assert [sum(c) for c in counts] == [512, 0, 1, 68, 513, 512]
    gc = pcfg.inference_gc_config("knn", 3, False)
    feats = torch.zeros(len(counts), 1, 96, 96)
    out = restate.construct_graph(hm, feats, torch.zeros_like(hm), None, gc, J)
    det, bi = out[7], out[12]
    got = torch.zeros(len(counts), J, dtype=torch.long)
    got.index_put_((bi, det[:, 2]), torch.ones_like(bi), accumulate=True)
    assert got.tolist() == counts
    with pytest.raises(ValueError):
        eo.planted_heatmaps([[257]], 64, 64)                     # 64 x 64 planes hold 256 sites


def test_order_layout_is_host_only():
    """pemp_mpn_order_layout: the five arrays at ascending 4-byte aligned offsets inside the workspace, without
    overlap; no device call (the offsets precede everything sized by the device's CU count); NULL is an error."""
    L = _lib.load_cdll()
    for T, N, E in ((17, 4080, 230_000), (1, 20_000, 250_000), (17, 1, 0), (17, 0, 0), (3, 7, 5)):
        desc = _lib.PempMpnDesc(T, 17, 1, 0, 3, 64, 19, 128, 2, 1, 0)
        offs = (ctypes.c_size_t * 5)()
        assert L.pemp_mpn_order_layout(ctypes.byref(desc), N, E, offs) == 0
        size = L.pemp_mpn_workspace_size(ctypes.byref(desc), N, E)
        lens = (T * N + 1, eo.MAXT + 2, E, E, E)
        o = list(offs)
        assert all(v % 4 == 0 for v in o)
        assert all(a + 4 * n <= b for a, n, b in zip(o, lens, o[1:] + [size])), (T, N, E, o, size)
        assert o[0] >= 4 * (64 + T * N + 1)                      # behind the flags and the counts
    assert L.pemp_mpn_order_layout(None, 10, 10, offs) != 0
    assert L.pemp_mpn_order_layout(ctypes.byref(desc), 10, 10, None) != 0
    assert L.pemp_mpn_order_layout(ctypes.byref(desc), -1, 10, offs) != 0
