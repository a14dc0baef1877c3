"""CPU-side checks of the fused edge update (csrc/train_edge.hip): the three entry points are exported and declared
alike in include/pemp.h and the binding table, argument errors come back before any HIP call, the workspace size is
host arithmetic, and the segment plan carries the int32 node ids the kernels read."""
import os
import re

import pytest
import torch

from pemp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pemp_edge_mlp_workspace_size", "pemp_edge_mlp_fwd", "pemp_edge_mlp_bwd")
P = 0x1000   # never dereferenced: every call that carries it fails its argument checks first


def fwd_args(N=4, E=8, We=128, **null):
    names = ("P", "Q", "ef", "src32", "dst32", "C", "W2", "b2", "h", "e_new")
    return [N, E, We] + [None if n in null else P for n in names] + [None]


def bwd_args(N=4, E=8, We=128, ws=P, ws_bytes=None, **null):
    names = ("g", "ef", "h", "e_new", "C", "W2", "g1", "g_ef", "dC", "dW2", "db2")
    if ws_bytes is None:
        ws_bytes = _lib.load_cdll().pemp_edge_mlp_workspace_size(E, We)
    return [N, E, We] + [None if n in null else P for n in names] + [ws, ws_bytes, None]


def test_exports_header_and_binding_agree():
    L = _lib.load_cdll()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pemp.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SIGNATURES
        decl = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert decl, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(decl.group(2).split(",")), name
        assert (decl.group(1) == "size_t") == (res is _lib.c_sz), name
    assert L.pemp_abi_version() == 24 == _lib.ABI_VERSION         # an additive change


def test_argument_errors_need_no_gpu():
    L = _lib.load_cdll()
    fwd, bwd = L.pemp_edge_mlp_fwd, L.pemp_edge_mlp_bwd
    bad = [("We", fwd(*fwd_args(We=32))), ("We", fwd(*fwd_args(We=96))), ("We", fwd(*fwd_args(We=256))),
           ("We", bwd(*bwd_args(We=0, ws_bytes=1 << 30))), ("We", bwd(*bwd_args(We=192, ws_bytes=1 << 30))),
           ("size", fwd(*fwd_args(N=-1))), ("size", fwd(*fwd_args(E=-8))),
           ("size", bwd(*bwd_args(N=-1, ws_bytes=1 << 30))), ("size", bwd(*bwd_args(E=-8, ws_bytes=1 << 30))),
           ("size", fwd(*fwd_args(E=2 ** 31))), ("size", bwd(*bwd_args(E=2 ** 31, ws_bytes=1 << 62)))]
    for name in ("P", "Q", "ef", "src32", "dst32", "C", "W2", "b2", "h", "e_new"):
        bad.append(("NULL " + name, fwd(*fwd_args(**{name: True}))))
    for name in ("g", "ef", "h", "e_new", "C", "W2", "g1", "g_ef", "dC", "dW2", "db2"):
        bad.append(("NULL " + name, bwd(*bwd_args(**{name: True}))))
    for We in (64, 128):
        for E in (1, 256, 257, 40_003):
            need = L.pemp_edge_mlp_workspace_size(E, We)
            bad.append(("workspace", bwd(*bwd_args(E=E, We=We, ws_bytes=need - 1))))
            bad.append(("workspace", bwd(*bwd_args(E=E, We=We, ws_bytes=0))))
            bad.append(("workspace", bwd(*bwd_args(E=E, We=We, ws=None))))
    for what, rc in bad:
        assert rc == _lib.ERR_INVALID_ARG, what
    assert fwd(*fwd_args(We=32)) == _lib.ERR_INVALID_ARG
    assert b"We = 32" in L.pemp_last_error()
    assert bwd(*bwd_args(ws_bytes=16)) == _lib.ERR_INVALID_ARG
    assert b"workspace" in L.pemp_last_error()


def test_no_edge_returns_ok_without_a_gpu():
    L = _lib.load_cdll()
    for We in (64, 128):
        assert L.pemp_edge_mlp_fwd(5, 0, We, *([None] * 11)) == 0
        assert L.pemp_edge_mlp_fwd(0, 0, We, *([None] * 11)) == 0
        assert L.pemp_edge_mlp_fwd(*fwd_args(N=5, E=0, We=We)) == 0
        assert L.pemp_edge_mlp_bwd(5, 0, We, *([None] * 12), 0, None) == 0


def test_workspace_size_is_host_arithmetic():
    L = _lib.load_cdll()
    size = L.pemp_edge_mlp_workspace_size
    for We in (64, 128):
        part = 4 * (64 * We + 64 * 64 + 64)              # one partial: dC, dW2, db2
        assert size(0, We) == 0
        prev = 0
        for E in (1, 2, 255, 256, 257, 512, 513, 3000, 8192, 8193, 40_003, 186_048, 2 ** 31 - 1):
            n = size(E, We)
            assert n >= prev and n >= -(-E // 256) * part and n % part == 0, (E, We)
            prev = n
    assert size(1000, 128) > size(1000, 64)
    assert size(1000, 96) == 0 and size(-5, 64) == 0      # nothing to size (the entries refuse these)


@pytest.mark.parametrize("T", [1, 17])
@pytest.mark.parametrize("E", [0, 1, 700])
def test_build_plan_fills_the_int32_ids(T, E):
    from pemp_amd.mpn.train import build_plan
    N = 23
    g = torch.Generator().manual_seed(3 * T + E)
    ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)])
    plan = build_plan(ei, torch.randint(0, 17, (N,), generator=g), N, T)
    assert plan.src32.dtype == torch.int32 and plan.dst32.dtype == torch.int32
    assert plan.src32.shape == (E,) and plan.dst32.shape == (E,)
    assert plan.src32.is_contiguous() and plan.dst32.is_contiguous()
    assert torch.equal(plan.src32.long(), ei[0]) and torch.equal(plan.dst32.long(), ei[1])
