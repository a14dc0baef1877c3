"""The differentiable node features without a GPU: the derived bound of tests/node_grad_ref.py is attainable (torch's
own fp32 CPU conv backward stays inside it on every planted case), the pixel plan's order, the argument checks of the
new entry points (they come before any HIP call) and the constructor's refusals."""
import ctypes

import numpy as np
import pytest
import torch

from pemp_amd import _lib, node_gather as ng
from pemp_amd.frontend import ProjectedMaps
from pemp_amd.graph_constructor import NaiveGraphConstructor
from tests import node_grad_ref as nr

CASES = [(c, s) for c in nr.CONVS for s in nr.NODE_SETS]
IDS = [f"{c[0]}-{c[1]}-k{c[2]}p{c[3]}-{s}" for c, s in CASES]


@pytest.mark.parametrize("case,set_name", CASES, ids=IDS)
def test_torch_fp32_is_inside_the_derived_bound(case, set_name):
    """The bound is attainable: torch's fp32 CPU forward and backward of the dense conv + indexing against fp64."""
    d = nr.conv_inputs(case, set_name)
    ref = nr.conv_reference(d)
    got = nr.conv_autograd(d["raw"], d["weight"], d["bias"], d["g"], d["jd"], d["bi"], d["pad"], torch.float32)
    for i, name in enumerate(("x", "draw", "dW", "db")):
        r = nr.ratio(got[i], *ref[name])
        print(f"node_grad cpu {case} {set_name}: {name} error/bound {r:.3f}")
        assert r <= 1.0, (name, r)


def test_planted_sets_hold_what_they_promise():
    jd, bi = nr.nodes("base")
    pix = [tuple(r) for r in np.column_stack([bi, jd[:, 1], jd[:, 0]])]
    assert pix.count((0, 5, 7)) == 3 and len({t for t in jd[:3, 2]}) == 3           # three types on one pixel
    for corner in ((0, 0), (0, nr.W - 1), (nr.H - 1, 0), (nr.H - 1, nr.W - 1)):
        assert (0,) + corner in pix
    assert (0, 6, 10) in pix and (0, 6, 11) in pix                                  # one pixel apart
    assert 1 not in bi and np.all(np.diff(bi) >= 0)                                 # the middle image is empty
    assert [nr.nodes(s)[0].shape[0] for s in nr.NODE_SETS] == [14, 1, 0, 257, 513]


@pytest.mark.parametrize("k,pad", [(1, 0), (3, 1), (3, 0), (5, 2)])
def test_pixel_plan_orders_entries_by_pixel_then_entry(k, pad):
    jd, bi = nr.nodes("n257")
    h, w = nr.H + k - 1 - 2 * pad, nr.W + k - 1 - 2 * pad
    plan = ng.PixelPlan(torch.from_numpy(jd), torch.from_numpy(bi), nr.B, h, w, k, pad)
    want = []
    for n in range(jd.shape[0]):
        for dy in range(k):
            for dx in range(k):
                yy, xx = jd[n, 1] - pad + dy, jd[n, 0] - pad + dx
                ok = 0 <= yy < h and 0 <= xx < w
                want.append((bi[n] * h + yy) * w + xx if ok else nr.B * h * w)
    want = np.array(want, np.int64)
    order = np.argsort(want, kind="stable")
    assert np.array_equal(plan.keys.numpy(), want[order]) and np.array_equal(plan.perm.numpy(), order)
    assert plan.args == (nr.B, h, w, k, pad, 257)
    if pad:
        assert (want == nr.B * h * w).any()          # windows at the corners leave the map


def test_entry_points_check_arguments_before_any_hip_call():
    L = _lib.load_cdll()
    p = ctypes.c_void_p(4096)                        # never followed: every call below fails its checks first
    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED
    pix = L.pemp_node_grad_pixels
    assert pix(p, -1, 8, p, p, 1, 4, 4, p, None) == INV
    assert pix(p, 4, 0, p, p, 1, 4, 4, p, None) == INV
    assert pix(p, 4, 8, p, p, 1, 4, 4, None, None) == INV and b"dfeat" in L.pemp_last_error()
    assert pix(None, 4, 8, p, p, 1, 4, 4, p, None) == INV
    assert pix(p, 4, 8, None, p, 1, 4, 4, p, None) == INV
    assert pix(p, 2 ** 31, 8, p, p, 1, 4, 4, p, None) == UNS
    bwd = L.pemp_node_conv_bwd

    def conv(N=4, B=1, Cin=8, h=6, w=6, Cout=16, k=3, pad=1, g=p, raw=p, wk=p, keys=p, ws=p, ws_bytes=1 << 30):
        return bwd(g, raw, wk, p, p, N, B, Cin, h, w, Cout, k, pad, keys, p, p, p, p, ws, ws_bytes, None)

    assert conv(N=-1) == INV and conv(Cin=0) == INV and conv(pad=3) == INV and conv(pad=-1) == INV
    assert conv(Cout=513) == UNS and conv(k=8, pad=0, h=9, w=9) == UNS
    assert conv(Cin=4096, k=3) == INV and b"LDS" in L.pemp_last_error()
    assert conv(h=2, w=2, k=5, pad=0) == INV and b"empty" in L.pemp_last_error()
    assert conv(g=None) == INV and conv(raw=None) == INV and conv(wk=None) == INV and conv(keys=None) == INV
    assert conv(ws=None) == INV and conv(ws_bytes=16) == INV and b"workspace" in L.pemp_last_error()
    assert conv(ws=ctypes.c_void_p(4100)) == INV and b"aligned" in L.pemp_last_error()
    assert conv(N=2 ** 31) == UNS


def test_workspace_size_is_host_arithmetic():
    L = _lib.load_cdll()
    size = L.pemp_node_conv_workspace_size
    assert size(0, 48, 128, 3) == 0 and size(-5, 48, 128, 3) == 0
    assert size(10, 48, 513, 3) == 0 and size(10, 48, 128, 8) == 0 and size(10, 0, 128, 3) == 0
    part = 128 * 48 * 9 + 128
    for N, chunks in ((1, 1), (256, 1), (257, 2), (513, 3), (256 * 33, 33)):
        d = (N * 9 * 48 * 4 + 255) // 256 * 256
        assert size(N, 48, 128, 3) == d + (chunks + (chunks + 31) // 32) * part * 4, N
    assert all(size(n + 1, 5, 24, 3) >= size(n, 5, 24, 3) for n in range(1, 600))


def _constructor(features):
    gc = object.__new__(NaiveGraphConstructor)       # (the constructor itself needs the HIP device)
    gc.features = features
    return gc


def test_grad_kind_and_refusals():
    """Which backward a construct takes, and the refusals of a required gradient, before the library is touched."""
    conv = torch.nn.Conv2d(4, 6, 3, padding=1)
    raw = torch.zeros(1, 4, 8, 10)
    assert _constructor(torch.zeros(1, 4, 8, 10))._grad_kind() is None
    assert _constructor(torch.zeros(1, 4, 8, 10, requires_grad=True))._grad_kind() == "dense"
    assert _constructor(ProjectedMaps(raw, (8, 10), gather=conv))._grad_kind() == "conv"
    assert _constructor(ProjectedMaps(raw.clone().requires_grad_(True), (8, 10)))._grad_kind() == "maps"
    assert _constructor(ProjectedMaps(raw, (8, 10)))._grad_kind() is None
    with torch.no_grad():
        assert _constructor(torch.zeros(1, 4, 8, 10, requires_grad=True))._grad_kind() is None
        assert _constructor(ProjectedMaps([raw, raw], (16, 20), gather=conv))._grad_kind() is None
    live = raw.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="2 maps"):
        _constructor(ProjectedMaps([live, raw], (8, 10), gather=conv))._grad_kind()
    with pytest.raises(NotImplementedError, match="does not project"):
        _constructor(ProjectedMaps(live, (16, 20), gather=conv))._grad_kind()
    with pytest.raises(NotImplementedError, match="does not project"):
        _constructor(ProjectedMaps(live, (8, 10), gather=torch.nn.Conv2d(4, 6, 3)))._grad_kind()
    with pytest.raises(NotImplementedError, match="divisor"):
        _constructor(ProjectedMaps(live, (8, 10), divisor=2.0, gather=conv))._grad_kind()
    with pytest.raises(NotImplementedError, match="does not project"):
        _constructor(ProjectedMaps(live, (16, 20)))._grad_kind()
    # only the conv's parameters require a gradient (every nn.Conv2d starts so): the projecting call runs as it
    # always has, without a gradient, and says so once per process
    NaiveGraphConstructor._warned_projection = False
    with pytest.warns(UserWarning, match="x will carry none"):
        assert _constructor(ProjectedMaps([raw, raw], (16, 20), gather=conv))._grad_kind() is None
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert _constructor(ProjectedMaps(raw, (16, 20), gather=conv))._grad_kind() is None
    for p in conv.parameters():
        p.requires_grad_(False)
    assert _constructor(ProjectedMaps([raw, raw], (16, 20), gather=conv))._grad_kind() is None   # as today
    w, b = ProjectedMaps(raw, (8, 10), gather=conv).live_params()
    assert w is conv.weight and b is conv.bias      # the optimizer's own tensors, not copies
    assert not ProjectedMaps(raw, (8, 10), gather=conv).conv_params()[0].requires_grad


def test_functional_forms_refuse_what_the_kernels_do_not_take():
    jd, bi = (torch.from_numpy(a) for a in nr.nodes("base"))
    with pytest.raises(RuntimeError, match="HIP device only"):
        ng.gather_nodes(torch.zeros(3, 4, nr.H, nr.W), jd, bi)
    with pytest.raises(NotImplementedError, match="stride 1"):
        ng.gather_nodes_conv(torch.zeros(3, 4, nr.H, nr.W), torch.nn.Conv2d(4, 8, 3, stride=2), jd, bi)
    with pytest.raises(NotImplementedError, match="512"):
        ng.gather_nodes_conv(torch.zeros(3, 4, nr.H, nr.W), torch.nn.Conv2d(4, 513, 1), jd, bi)
    with pytest.raises(TypeError, match="Conv2d"):
        ng.gather_nodes_conv(torch.zeros(3, 4, nr.H, nr.W), torch.nn.Linear(4, 4), jd, bi)
