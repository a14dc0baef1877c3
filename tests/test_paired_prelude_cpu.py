"""The paired prelude (csrc/mpn.hip prelude_a_kernel / prelude_b_kernel), host side: how the two launches' blocks are
split between their roles (pemp_mpn_prelude_grids, the arithmetic Forward::prelude launches with), and the descriptor
flag that keeps the four separate launches."""
import ctypes
import pathlib
import re

import pytest

from pemp_amd import _lib

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "pemp.h"
T = 17
G = 192            # workgroups of an edge pass (256 CUs less the reserved 64)
CUS = 256
PREP_GX, A_GX, ROWS, A_SPLIT, RANGES_RB, RANGES, TABLE, B_SPLIT = range(8)


def grids(N, E, B, nmax, T=T, G=G, cus=CUS):
    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.load_cdll().pemp_mpn_prelude_grids(N, E, B, T, nmax, G, cus, out))
    return list(out)


def images(N, B):
    """per-image node counts of N nodes in B images, as even as they come"""
    return [N // B + (1 if b < N % B else 0) for b in range(B)]


def check_partition(g, N, E, B, nmax, T=T, cus=CUS):
    """Each launch's blocks are the first role's grid followed by the second role's: disjoint, no block left over,
    the first role (the edge order in A, the wave ranges in B: the roles whose blocks run longest) from block 0."""
    groups = ((128 + 64 * T) // 16 + 3) // 4
    # the four role grids, from the kernels' own mappings
    gx = max(1, min(64, (T * nmax * 4 + 511) // 512))                 # 4 threads per (type, target) segment
    assert g[PREP_GX] == gx
    # launch A holds one block per CU (the embedding's LDS): the order gets the CUs the embedding leaves, at least
    # one block per image and no more than its own launch has
    gx = g[A_GX]
    assert 1 <= gx <= g[PREP_GX] and g[A_SPLIT] == gx * B
    if B > 0 and gx < g[PREP_GX]:
        assert gx == 1 or gx * B + g[ROWS] <= cus < (gx + 1) * B + g[ROWS]
    assert g[ROWS] == (N + 15) // 16                                  # 16-node tiles
    assert g[TABLE] == (N + 31) // 32 * groups                        # 32-node chunks x 64-column groups
    if E == 0:
        assert g[RANGES] == g[RANGES_RB] == 0
    else:
        assert g[RANGES_RB] == min(64, (G * 28 + 255) // 256)         # 16 + 12 waves per edge-pass workgroup
        assert g[RANGES] == g[RANGES_RB] + min(1024, (E + 255) // 256)
    for split, first, second in ((g[A_SPLIT], gx * B, g[ROWS]), (g[B_SPLIT], g[RANGES], g[TABLE])):
        total = first + second                                        # the launch's grid
        role0, role1 = range(0, split), range(split, total)
        assert len(role0) == first and len(role1) == second
        assert not set(role0) & set(role1) and sorted([*role0, *role1]) == list(range(total))
    # every (x, y) block of the order's 2-D grid is decoded from exactly one block of launch A
    assert [(bx % gx, bx // gx) for bx in range(g[A_SPLIT])] == [(x, y) for y in range(B) for x in range(gx)]
    # rows and table cover every node
    assert 16 * g[ROWS] >= N > 16 * (g[ROWS] - 1) or N == 0


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("N", [1, 2, 15, 16, 17, 1550])
def test_roles_partition_both_launches(N, B):
    per = images(N, B)
    E = sum(n * (n - 1) for n in per)
    g = grids(N, E, B, max(per))
    check_partition(g, N, E, B, max(per))
    if N == 1550 and B == 8:     # bench.py's c3 (exact forward): 19 x 8 + 97 blocks in launch A, 21 + 931 in launch B
        assert (g[PREP_GX], g[A_GX], g[ROWS], g[RANGES_RB], g[TABLE]) == (26, 19, 97, 21, 931)
        # ... and as capacity mode launches it (512 detections per image at most): still one block per CU
        gc = grids(N, E, B, 512)
        check_partition(gc, N, E, B, 512)
        assert gc[PREP_GX] == 64 and gc[A_SPLIT] + gc[ROWS] <= CUS
        # a device the embedding's tiles fill: the order keeps one block per image
        gs = grids(N, E, B, max(per), cus=64)
        check_partition(gs, N, E, B, max(per), cus=64)
        assert gs[A_GX] == 1


def test_empty_image_and_no_edges():
    # a batch whose second image has no node
    per = [9, 0, 14]
    N, E = sum(per), sum(n * (n - 1) for n in per)
    check_partition(grids(N, E, len(per), max(per)), N, E, len(per), max(per))
    # a batch of nothing but empty images (the forward launches nothing; the arithmetic still holds)
    g = grids(0, 0, 2, 0)
    check_partition(g, 0, 0, 2, 0)
    assert g[ROWS] == g[TABLE] == g[RANGES] == 0
    # nodes without edges: one node per image; launch B is the node table alone
    for N in (1, 5):
        g = grids(N, 0, N, 1)
        check_partition(g, N, 0, N, 1)
        assert g[B_SPLIT] == 0 and g[TABLE] > 0


def test_one_type_model_and_bad_args():
    check_partition(grids(36, 662, 2, 23, T=1), 36, 662, 2, 23, T=1)
    L = _lib.load_cdll()
    out = (ctypes.c_int32 * 8)()
    assert L.pemp_mpn_prelude_grids(16, 240, 1, 0, 16, G, CUS, out) == _lib.ERR_INVALID_ARG     # T = 0
    assert L.pemp_mpn_prelude_grids(16, 240, 65, T, 16, G, CUS, out) == _lib.ERR_INVALID_ARG    # past 64 images
    assert L.pemp_mpn_prelude_grids(16, 240, 1, T, 16, G, CUS, None) == _lib.ERR_INVALID_ARG


def test_flag_is_a_new_bit_and_the_abi_stays():
    text = HEADER.read_text()
    defs = {k: int(v) for k, v in re.findall(r"#define (PEMP_MPN_[A-Z_]+) (\d+)", text)}
    flag = defs["PEMP_MPN_SEPARATE_PRELUDE"]
    assert flag == _lib.MPN_SEPARATE_PRELUDE == 16
    others = [v for k, v in defs.items() if k != "PEMP_MPN_SEPARATE_PRELUDE"]
    assert len(others) >= 3 and all(v & (v - 1) == 0 for v in [flag, *others])     # single bits
    assert not any(flag & v for v in others) and len(set(others)) == len(others)
    L = _lib.load_cdll()
    assert int(re.search(r"#define PEMP_ABI_VERSION (\d+)", text).group(1)) == L.pemp_abi_version() == _lib.ABI_VERSION
    sizes = set()
    for flags in (0, flag):
        desc = _lib.PempMpnDesc(17, 17, 3, 0, 3, 64, 19, 128, 2, 1, flags)
        sizes.add(L.pemp_mpn_workspace_size(ctypes.byref(desc), 1546, 232_846))
    assert len(sizes) == 1 and sizes.pop() > 0


def test_model_attribute_maps_to_the_flag():
    import pemp_amd
    from pemp_amd import config as pcfg
    m = pemp_amd.get_mpn_model(pcfg.published_mpn_config(17, 3, "attn"))
    assert m.paired_prelude is True and m._first_flag() == 0
    m.paired_prelude = False
    assert m._first_flag() == _lib.MPN_SEPARATE_PRELUDE
    m.fuse_first_pass = False
    assert m._first_flag() == _lib.MPN_SEPARATE_PRELUDE | _lib.MPN_TWO_LAUNCH_FIRST
