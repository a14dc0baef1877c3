"""The type-major edge order every MPN forward starts from (csrc/mpn_order.hip: seg, wg_start, s_src, s_dst, s_orig),
as tests/test_edge_order_cpu.py and tests/test_gpu_edge_order.py check it: a numpy reference of the order, heatmaps
that make the graph constructor detect exactly a given number of nodes per image and type, and the read-back of
the order from a model's workspace (pemp_mpn_order_layout). Helpers only, no tests."""
import ctypes

import numpy as np
import torch

MAXT = 17                    # csrc/mpn_internal.h: wg_start holds MAXT + 2 words
SDST_ID_MASK = 0xFFFFFF      # after a forward s_dst carries the passes' segment positions above the target id


def expected_order(ei, types, N, T):
    """(seg [T N + 1], s_src, s_dst, s_orig) of the edge list ei [2, E] over N nodes of the given types: the edges
    sorted by (type of source, target, edge id). An edge with an end outside [0, N), or a source type outside
    [0, T), is dropped; one message type (T == 1) ignores the types."""
    ei, types = np.asarray(ei, np.int64), np.asarray(types, np.int64)
    src, dst = ei[0], ei[1]
    ok = (src >= 0) & (src < N) & (dst >= 0) & (dst < N)
    t = np.zeros(src.shape, np.int64)
    if T != 1:
        t[ok] = types[src[ok]]
        ok &= (t >= 0) & (t < T)
    ids = np.nonzero(ok)[0]
    key = t[ids] * N + dst[ids]
    order = ids[np.argsort(key, kind="stable")]          # stable: edge-id order inside a segment
    seg = np.zeros(T * N + 1, np.int64)
    seg[1:] = np.cumsum(np.bincount(key, minlength=T * N))
    return seg, src[order], dst[order], order


def spread(n, J, absent=(), shift=0):
    """n nodes spread evenly over the J types except `absent`; the remainder goes to the present types from
    position `shift` on (so that it does not always land on the same types)."""
    present = [j for j in range(J) if j not in absent]
    out = [0] * J
    for i, j in enumerate(present):
        out[j] = n // len(present) + (1 if (i - shift) % len(present) < n % len(present) else 0)
    return out


def planted_heatmaps(counts, H, W, seed=0):
    """[B, J, H, W] float32 planes, zero except counts[b][j] isolated peaks in plane (b, j): sites of the 4-spaced
    grid (4 r + 2, 4 c + 2) drawn at random (seeded), with distinct values in [0.2, 0.9]. A peak is the only
    nonzero value of its 3 x 3 (and 5 x 5) window and lies over DETECT_THRESHOLD 0.1, so the detection of
    inference_gc_config(graph, 3, False) finds exactly counts[b][j] nodes of type j in image b."""
    rng = np.random.default_rng(seed)
    B, J = len(counts), len(counts[0])
    gh, gw = H // 4, W // 4
    hm = np.zeros((B, J, H, W), np.float32)
    for b in range(B):
        for j in range(J):
            n = counts[b][j]
            if n > gh * gw:
                raise ValueError(f"{n} peaks do not fit the {gh * gw} sites of a {H} x {W} plane")
            sites = rng.choice(gh * gw, n, replace=False)
            vals = rng.permutation(np.linspace(0.2, 0.9, max(n, 1), dtype=np.float64))[:n]
            hm[b, j, 4 * (sites // gw) + 2, 4 * (sites % gw) + 2] = vals.astype(np.float32)
    return torch.from_numpy(hm)


def read_order(model, N, E):
    """(seg, wg_start, s_src, s_dst, s_orig) as numpy int32 arrays, full words, from the workspace of the model's
    last forward over N nodes and E edges on the current stream (read after a device synchronise)."""
    from pemp_amd import _lib
    L = _lib.lib()
    desc, ws = model._order_workspace(N, E)
    torch.cuda.synchronize()
    offs = (ctypes.c_size_t * 5)()
    _lib.check(L.pemp_mpn_order_layout(desc, N, E, offs))
    lens = (model.num_types * N + 1, MAXT + 2, E, E, E)
    return tuple(ws[o:o + 4 * n].view(torch.int32).cpu().numpy() for o, n in zip(offs, lens))
