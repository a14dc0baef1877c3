"""The type-major edge order of the four prepares of csrc/mpn_order.hip (the sorting prepare, and the closed forms for the
constructor's fully graph, for symmetric sorted lists and for the knn build's bit rows), checked exactly -- integer
arrays against the numpy reference of tests/edge_order.py -- at the sizes where each prepare takes another path or
hands over to the next one. No tolerance anywhere in this file.

A forward is "checked" when
 (a) seg, s_src, s_dst & 0xFFFFFF and s_orig equal edge_order.expected_order,
 (b) all five arrays, full words, equal those of the same forward with the fast prepare switched off,
 (c) the logits of the two forwards are bit-identical,
 (d) pemp_mpn_status is clear (validate=True),
 (e) one more forward under the library profiler reports the expected prepare label.
Graphs come from the graph constructor on planted heatmaps (edge_order.planted_heatmaps), so the tags and bit rows
are the product's own; models are the published shapes with STEPS = 1 (T = 17 "attn", T = 1 "max") in f16x3."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pemp_amd
from oracle import restate
from pemp_amd import _lib, config as pcfg, synthetic as syn
from tests import edge_order as eo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
J = 17
ABSENT = 5                  # a type no node of a batch has: its type range is empty
ARRAYS = ("seg", "wg_start", "s_src", "s_dst", "s_orig")
VARIANTS = ["attn", "max"]


@pytest.fixture(autouse=True)
def constructor_state(monkeypatch):
    """The constructor's class-wide capacity hints (grown by the 2048-node images here) go back after each test."""
    from pemp_amd.graph_constructor import NaiveGraphConstructor as G
    monkeypatch.setattr(G, "_cap", G._cap)
    monkeypatch.setattr(G, "_graph_hint", dict(G._graph_hint))


def make_model(variant):
    m = pemp_amd.get_mpn_model(pcfg.published_mpn_config(J, 1, variant))
    m.load_state_dict(syn.closed_form_state_dict(m, 3.75))
    m.precision = "f16x3"
    return m.eval().to(DEV)


shared_model = functools.lru_cache(maxsize=None)(make_model)


def forward(model, x, ea, ei, types):
    with torch.no_grad():
        pe, pn, pc, _ = model(x, ea, ei, node_types=types, validate=True)      # (d)
    torch.cuda.synchronize()
    return pe + pn + pc


def same(name, got, want):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, f"{name}: {got.shape} entries, expected {want.shape}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{name}: {bad.size} of {got.size} entries differ, the first at {bad[0]}: "
                           f"got {got[bad[0]]}, expected {want[bad[0]]}")


def same_order(got, want):
    """(a): got = read_order's five arrays, want = expected_order's four."""
    same("seg", got[0], want[0])
    same("s_src", got[2], want[1])
    same("s_dst & 0xFFFFFF", got[3] & eo.SDST_ID_MASK, want[2])
    same("s_orig", got[4], want[3])


def checked(model, g, label, off, monkeypatch):
    """Checks (a) to (e) on the graph g = (x, edge_attr, edge_index, node_types); off: the switches of
    mpn/model.py that take the fast prepare away, one tuple per comparison forward. Returns E."""
    from pemp_amd.mpn import model as mm
    x, ea, ei, types = g
    N, E = x.shape[0], ei.shape[1]
    want = eo.expected_order(ei.cpu().numpy(), types.cpu().numpy(), N, model.num_types)
    assert want[0][-1] == E                                    # every edge of these graphs is valid
    fast = forward(model, *g)
    got = eo.read_order(model, N, E)
    same_order(got, want)                                                       # (a)
    for names in off:
        for n in names:
            monkeypatch.setattr(mm, n, True)
        slow = forward(model, *g)
        ref = eo.read_order(model, N, E)
        for n in names:
            monkeypatch.setattr(mm, n, False)
        for name, a, b in zip(ARRAYS, got, ref):
            same(f"{name} (against {'/'.join(names)})", a, b)                   # (b)
        assert len(fast) == len(slow)
        for a, b in zip(fast, slow):
            assert torch.equal(a, b)                                            # (c)
    _lib.prof_enable("mpn_prepare")
    try:
        forward(model, *g)
        rep = _lib.prof_report()
    finally:
        _lib.prof_enable(None)
    assert {k: v[0] for k, v in rep.items()} == {label: 1}                      # (e)
    return E


def construct(counts, H, W, gtype, seed, oracle):
    """construct_graph's tuple for planted heatmaps with counts[b][j] nodes of type j in image b; with `oracle`, its
    outputs 0, 1, 2, 7, 11 and 12 bit-exact against restate.construct_graph."""
    B = len(counts)
    hm = eo.planted_heatmaps(counts, H, W, seed)
    feats = torch.rand(B, 128, H, W, generator=torch.Generator().manual_seed(seed)) * 2 - 1
    gc = pcfg.inference_gc_config(gtype, 3, False)
    out = pemp_amd.get_graph_constructor(gc, scoremaps=hm.to(DEV), features=feats.to(DEV), tagmaps=None,
                                         joints_gt=None, factor_list=None, masks=None, device=DEV, testing=True,
                                         heatmaps=None, num_joints=J).construct_graph()
    got = torch.bincount(out[12] * J + out[7][:, 2], minlength=B * J).view(B, J).cpu()
    assert got.tolist() == [list(c) for c in counts]            # the planted counts, per image and type
    if oracle:
        ref = restate.construct_graph(hm, feats, torch.zeros(B, J, H, W), None, gc, J)
        for i in (0, 1, 2, 7, 11, 12):
            assert torch.equal(out[i].cpu(), ref[i]), f"construct_graph output {i} differs from the oracle"
    return out


def graph_of(out):
    return out[0], out[1], out[2], out[7][:, 2]


def spread_counts(sizes):
    return [eo.spread(n, J, absent=(ABSENT,), shift=b) for b, n in enumerate(sizes)]


# ---- knn rows (knn_prepare_kernel: B <= 64, N <= 4096, images <= 512 nodes) ---------------------------------
SIZES_16 = [0, 1, 2, 50, 51, 52, 63, 64, 65, 127, 128, 129, 191, 192, 193, 17]
ONE_TYPE = [512 if j == 9 else 0 for j in range(J)]             # an image of a single type


def knn_counts(name):
    if name == "B64-N4080":     # rows 2048 and 3072 crossed, images at the 64-node word boundaries, k + 1 = 51 nodes,
        return spread_counts(SIZES_16 * 3 + list(range(15)) + [0]), 64     # empty first and last images
    full = spread_counts([512] * 8)
    full[3] = ONE_TYPE
    if name == "B8-N4096":      # both limits exactly
        return full, 96
    if name == "B9-N4097":      # one node past N = 4096
        return full + [eo.spread(1, J, absent=(ABSENT,), shift=2)], 96
    if name == "B65":           # one image past B = 64
        return spread_counts([(3, 0, 17, 1, 52, 2, 64)[b % 7] for b in range(65)]), 64
    if name == "n513":          # one node past the 512-node image (the knn build's other kernel, no bit rows)
        return spread_counts([513, 20]), 96
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def knn_graph(name):
    counts, hw = knn_counts(name)
    return construct(counts, hw, hw, "knn", 11, oracle=True)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["B64-N4080", "B8-N4096"])
def test_knn_rows_prepare(name, variant, monkeypatch):
    """knn_prepare_kernel at its limits: 64 images, rows past 2048 and 3072 (the third load loop, the re-read of R
    in the placement), 512-node images, N = 4096; the list placement and the row-by-row one (PEMP_KNN_LIST_CAP=0);
    against the symmetric and the sorting prepare. The knn build itself (graph.hip) against the oracle."""
    from pemp_amd.mpn import model as mm
    g = graph_of(knn_graph(name))
    N = g[0].shape[0]
    assert N == (4080 if name == "B64-N4080" else 4096)
    assert mm._knn_graph(g[2], N) is not None
    off = [("_KNN_OFF",), ("_KNN_OFF", "_SYM_OFF")]
    E = checked(shared_model(variant), g, "mpn_prepare_knn", off, monkeypatch)
    monkeypatch.setenv("PEMP_KNN_LIST_CAP", "0")
    checked(shared_model(variant), g, "mpn_prepare_knn", off, monkeypatch)
    monkeypatch.delenv("PEMP_KNN_LIST_CAP")
    print(f"knn {name} {variant}: N={N} E={E} mpn_prepare_knn")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["B9-N4097", "B65", "n513"])
def test_knn_graph_past_the_rows_limits(name, variant, monkeypatch):
    """One step past each limit of the knn prepare (N = 4097, 65 images, a 513-node image): no bit rows are handed
    over and the symmetric prepare orders the edges."""
    from pemp_amd.mpn import model as mm
    g = graph_of(knn_graph(name))
    N = g[0].shape[0]
    assert mm._knn_graph(g[2], N) is None and mm._sym_graph(g[2])
    E = checked(shared_model(variant), g, "mpn_prepare_sym", [("_SYM_OFF",)], monkeypatch)
    print(f"knn {name} {variant}: N={N} E={E} mpn_prepare_sym")


# ---- symmetric prepare (sym_rows_kernel, sym_scan_kernel, sym_place_kernel: N < 2^24) ---------------------------
SYM_N, SYM_HUB = 20_000, 3_333
SYM_ROWS = {40: 1, 41: 63, 42: 64, 43: 65, 44: 128, 45: 129}    # node -> entries of its row (node 0: none)


@functools.lru_cache(maxsize=None)
def sym_graph():
    """A sorted symmetric list over 20,000 nodes (the second pass of sym_scan_kernel's scan needs N > 16384): about
    10 entries per row at random, rows of exactly 0, 1, 63, 64, 65, 128 and 129 entries (the 64-entry rounds of the
    row and placement kernels), a hub joined to every node but node 0 and to itself (a row of N - 1), self loops,
    node 0 isolated, node N - 1 with edges, random types."""
    rng = np.random.default_rng(5)
    N, hub = SYM_N, SYM_HUB
    special = np.array([0, hub] + list(SYM_ROWS))
    ordinary = np.setdiff1d(np.arange(N), special)
    a, b = rng.choice(ordinary, (2, 5 * N))
    pairs = [np.stack([a, b]), np.stack([ordinary[::7], ordinary[::7]]),        # random pairs, self loops
             np.stack([np.full(N - 1, hub), np.arange(1, N)])]                  # the hub (its own row included)
    for node, n in SYM_ROWS.items():                                            # the hub + n - 1 partners
        pairs.append(np.stack([np.full(n - 1, node), rng.choice(ordinary, n - 1, replace=False)]))
    p = np.concatenate(pairs, 1)
    key = np.unique(np.concatenate([p[0] * N + p[1], p[1] * N + p[0]]))         # symmetric, sorted by (src, dst)
    ei = np.stack([key // N, key % N])
    rows = np.bincount(ei[0], minlength=N)
    assert rows[0] == 0 and rows[N - 1] > 0 and rows[hub] == N - 1 and (ei[0] == ei[1]).sum() > 1000
    assert all(rows[node] == n for node, n in SYM_ROWS.items())
    E = ei.shape[1]
    gen = torch.Generator().manual_seed(5)
    eid = torch.from_numpy(ei).to(DEV)
    eid._pemp_sym = eid._version
    return (torch.randn(N, 128, generator=gen).to(DEV), torch.randn(E, J + 2, generator=gen).to(DEV), eid,
            torch.from_numpy(rng.integers(0, J, N)).to(DEV))


@pytest.mark.parametrize("variant", VARIANTS)
def test_symmetric_prepare_large(variant, monkeypatch):
    from pemp_amd.mpn import model as mm
    g = sym_graph()
    assert mm._sym_graph(g[2])
    E = checked(shared_model(variant), g, "mpn_prepare_sym", [("_SYM_OFF",)], monkeypatch)
    print(f"sym {variant}: N={SYM_N} E={E} mpn_prepare_sym")


# ---- fully graph (fully_prepare_kernel: B <= 64, images <= 2048 nodes) ---------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B", [64, 65])
def test_fully_prepare_batch_limit(B, variant, monkeypatch):
    """64 images take the closed form; with 65, mpn/model.py::_fully_graph refuses and the sorting prepare runs."""
    from pemp_amd.mpn import model as mm
    out = construct(spread_counts([(0, 1, 2, 3, 17, 40)[b % 6] for b in range(B)]), 64, 64, "fully", 13, oracle=False)
    g = graph_of(out)
    assert (mm._fully_graph(g[2], g[3], g[0].shape[0]) is not None) == (B == 64)
    label = "mpn_prepare_fully" if B == 64 else "mpn_prepare"
    E = checked(shared_model(variant), g, label, [("_FULLY_OFF",)], monkeypatch)
    print(f"fully B={B} {variant}: N={g[0].shape[0]} E={E} {label}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", [2048, 2049])
def test_fully_prepare_image_limit(n, variant, monkeypatch):
    """Two images, 40 and n nodes; in the large one a type of 1 node, one of 600 and an absent one. 2048 nodes are
    the closed form's limit (its per-image lists live in LDS); with 2049 the library falls back to the sorting
    prepare. E is about 4.2 million and the workspace several GB, so the model is the test's own and freed."""
    from pemp_amd.mpn import model as mm
    big = [0] * J
    big[2], big[11] = 1, 600
    rest = [j for j in range(J) if j not in (2, 11, ABSENT)]
    for i, j in enumerate(rest):
        big[j] = (n - 601) // len(rest) + (1 if i < (n - 601) % len(rest) else 0)
    assert sum(big) == n
    out = construct([eo.spread(40, J, absent=(ABSENT,)), big], 128, 128, "fully", 17, oracle=False)
    g = graph_of(out)
    assert g[2].shape[1] == 40 * 39 + n * (n - 1)
    assert mm._fully_graph(g[2], g[3], g[0].shape[0]) is not None
    model = make_model(variant)
    label = "mpn_prepare_fully" if n == 2048 else "mpn_prepare"
    try:
        E = checked(model, g, label, [("_FULLY_OFF",)], monkeypatch)
    finally:
        del model, out, g
        torch.cuda.empty_cache()
    print(f"fully n={n} {variant}: E={E} {label}")


# ---- the sorting prepare alone (pemp_mpn_prepare) and the PREPARED flag ----------------------------------------
MG_N, MG_E = 1_300, 50_000       # K = 17 x 1,300 counts cross one 16,384-count pass of mpn_scan_kernel


@functools.lru_cache(maxsize=None)
def multigraph():
    """A shuffled random multigraph with duplicate edges and self loops; no edge starts at its last two nodes."""
    rng = np.random.default_rng(9)
    ei = np.stack([rng.integers(0, MG_N - 2, MG_E), rng.integers(0, MG_N, MG_E)])
    ei[:, 10_000:15_000] = ei[:, :5_000]                        # duplicates
    ei = np.ascontiguousarray(ei[:, rng.permutation(MG_E)])
    return ei, rng.integers(0, J, MG_N)


def prepare_alone(T, ei, types, N):
    """pemp_mpn_prepare on a workspace of the test's own (filled with -1): the five arrays before any pass packs
    s_dst, and pemp_mpn_status's return code."""
    L = _lib.lib()
    E = ei.shape[1]
    desc = ctypes.byref(_lib.PempMpnDesc(T, J, 1, 0, 3, 64, J + 2, 128, 2, 1, 0))
    ws = torch.full((L.pemp_mpn_workspace_size(desc, N, E),), 0xFF, dtype=torch.uint8, device=DEV)
    eid, td = torch.from_numpy(np.ascontiguousarray(ei)).to(DEV), torch.from_numpy(types).to(DEV)
    _lib.check(L.pemp_mpn_prepare(desc, eid.data_ptr(), td.data_ptr(), N, E, ws.data_ptr(), ws.numel(),
                                  _lib.stream(DEV)))
    torch.cuda.synchronize()
    offs = (ctypes.c_size_t * 5)()
    _lib.check(L.pemp_mpn_order_layout(desc, N, E, offs))
    lens = (T * N + 1, eo.MAXT + 2, E, E, E)
    arrays = tuple(ws[o:o + 4 * n].view(torch.int32).cpu().numpy() for o, n in zip(offs, lens))
    return arrays, L.pemp_mpn_status(desc, N, E, ws.data_ptr(), _lib.stream(DEV))


@pytest.mark.parametrize("T", [17, 1])
def test_sorting_prepare_multigraph(T):
    """mpn_count / mpn_scan / mpn_scatter / mpn_segsort: mpn_scatter places by atomics and mpn_segsort must undo
    their order, so two runs give identical arrays."""
    ei, types = multigraph()
    want = eo.expected_order(ei, types, MG_N, T)
    runs = [prepare_alone(T, ei, types, MG_N) for _ in range(2)]
    for got, rc in runs:
        assert rc == 0
        same_order(got, want)
    for name, a, b in zip(ARRAYS, *[r[0] for r in runs]):
        same(f"{name} (second run)", a, b)


def test_sorting_prepare_skips_and_flags_invalid_entries():
    """200 invalid entries (a source of N, a target of -1, a source whose type is T or -1): the valid edges are
    placed exactly as the reference says, seg[T N] is their count, nothing is written behind them, and
    pemp_mpn_status reports the list. Prepare only: no forward runs on this list."""
    T = J
    ei, types = (a.copy() for a in multigraph())
    pos = np.random.default_rng(2).choice(MG_E, 200, replace=False)
    ei[0, pos[:70]] = MG_N
    ei[1, pos[70:140]] = -1
    ei[0, pos[140:170]], ei[0, pos[170:]] = MG_N - 2, MG_N - 1
    types[MG_N - 2], types[MG_N - 1] = T, -1
    want = eo.expected_order(ei, types, MG_N, T)
    assert want[0][-1] == MG_E - 200
    got, rc = prepare_alone(T, ei, types, MG_N)
    valid = MG_E - 200
    same("seg", got[0], want[0])
    assert got[0][T * MG_N] == valid
    for name, a, b in zip(ARRAYS[2:], got[2:], want[1:]):
        same(name, a[:valid], b)
        assert (a[valid:] == -1).all(), f"{name}: written behind the valid edges"
    assert rc == _lib.ERR_INVALID_ARG
    assert b"edge_index" in _lib.lib().pemp_last_error()
    # types alone
    ei2, _ = multigraph()
    got, rc = prepare_alone(T, np.concatenate([ei2, [[MG_N - 1], [0]]], 1), types, MG_N)
    assert got[0][T * MG_N] == MG_E and rc == _lib.ERR_INVALID_ARG
    assert b"node_types" in _lib.lib().pemp_last_error()


@pytest.mark.parametrize("variant", VARIANTS)
def test_prepared_flag(variant):
    """pemp_mpn_prepare, then pemp_mpn_forward with PEMP_MPN_PREPARED on the same workspace and stream: logits
    bit-identical to the plain forward, and no prepare launched by that forward."""
    L = _lib.lib()
    model = shared_model(variant)
    ei, types = multigraph()
    gen = torch.Generator().manual_seed(4)
    g = (torch.randn(MG_N, 128, generator=gen).to(DEV), torch.randn(MG_E, J + 2, generator=gen).to(DEV),
         torch.from_numpy(ei).to(DEV), torch.from_numpy(types).to(DEV))
    plain = forward(model, *g)
    assert len(plain) == 1 + 2 + 2                              # STEPS = 1: one edge record, two node / class ones
    d = model._desc
    desc = ctypes.byref(_lib.PempMpnDesc(d.num_types, d.num_joints, d.steps, d.aux_loss_steps, d.aggr, d.hidden,
                                         d.edge_attr_dim, d.node_in_dim, d.precision, d.types_stride,
                                         _lib.MPN_PREPARED))
    fw = model._weights(DEV)
    ws = torch.empty(L.pemp_mpn_workspace_size(desc, MG_N, MG_E), dtype=torch.uint8, device=DEV)
    el = torch.empty(1, MG_E, device=DEV)
    nl = torch.empty(2, MG_N, device=DEV)
    cl = torch.empty(2, MG_N, J, device=DEV)
    st = _lib.stream(DEV)
    _lib.check(L.pemp_mpn_prepare(desc, g[2].data_ptr(), g[3].data_ptr(), MG_N, MG_E, ws.data_ptr(), ws.numel(), st))
    _lib.prof_enable("mpn_prepare")
    try:
        _lib.check(L.pemp_mpn_forward(desc, fw.struct_ref, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(),
                                      g[3].data_ptr(), MG_N, MG_E, el.data_ptr(), nl.data_ptr(), cl.data_ptr(),
                                      ws.data_ptr(), ws.numel(), st))
        rep = _lib.prof_report()
    finally:
        _lib.prof_enable(None)
    torch.cuda.synchronize()
    assert rep == {}
    _lib.check(L.pemp_mpn_status(desc, MG_N, MG_E, ws.data_ptr(), st))
    for a, b in zip(plain, [el[0], nl[0], nl[1], cl[0], cl[1]]):
        assert torch.equal(a.reshape(-1), b.reshape(-1))
