"""The case table of the projected detection (tests/projected_cases.py), checked without a GPU: every case takes the
loader its row says (pemp_detect_projected_path, host arithmetic of csrc/detect.hip, against the table and against
an independent numpy restatement), the table covers every (loader, pool, flipped pass, masks) body of the strip
kernel and both sides of the separable loader's 16-row limit, and the oracle alone finds what each case is for:
detections on all four borders, inside the plateau, and negative scores where the reference can emit any."""
import ctypes
import itertools

import numpy as np
import pytest

from pemp_amd import _lib
from tests import projected_cases as pc


def library_path(hs, ws, H, W, pool):
    L = _lib.load_cdll()
    S = len(hs)
    x2 = ctypes.c_int32(-1)
    rc = L.pemp_detect_projected_path((ctypes.c_int * S)(*hs), (ctypes.c_int * S)(*ws), S, H, W, pool,
                                      ctypes.byref(x2))
    return rc, x2.value


def test_table_row_counts():
    """The staged-row counts and 2x bands written next to each row ratio are what the restatement computes."""
    for name, (h, H, nx2, staged) in pc.ROWS.items():
        if staged is not None:
            assert tuple(pc.staged_rows(h, H, p) for p in pc.POOLS) == staged, name
        if h * 2 == H:
            assert {pc.x2_bands(h, H, p) for p in pc.POOLS} == {nx2}, name
        else:
            assert nx2 == 0, name


@pytest.mark.parametrize("name", pc.NAMES)
def test_loader_intent(name):
    c = pc.BY_NAME[name]
    hs, ws = [h for h, _ in c.sizes], [w for _, w in c.sizes]
    want = (1, 0) if c.loader == "gen" else (2, c.x2)
    assert (c.loader == "x2") == (c.x2 > 0), name
    assert library_path(hs, ws, c.size[0], c.size[1], c.pool) == want, name
    assert pc.loader_path(hs, c.size[0], c.pool) == want, name


def test_restatement_agrees_with_library_sweep():
    """Every (H, h, pool) for H, h <= 128: the library's host arithmetic and the numpy restatement choose the same
    loader and count the same 2x bands; optional output pointer, argument errors."""
    L = _lib.load_cdll()
    one = ctypes.c_int * 1
    x2 = ctypes.c_int32(0)
    w = one(40)
    for H in range(1, 129):
        for h in range(1, 129):
            for pool in pc.POOLS:
                rc = L.pemp_detect_projected_path(one(h), w, 1, H, 80, pool, ctypes.byref(x2))
                assert (rc, x2.value) == pc.loader_path([h], H, pool), (H, h, pool)
    assert L.pemp_detect_projected_path(one(24), w, 1, 48, 80, 5, None) == 2
    for bad in ((0, 48, 80, 5), (5, 48, 80, 5), (1, 0, 80, 5), (1, 48, 0, 5), (1, 48, 80, 4), (1, 48, 80, 11)):
        assert L.pemp_detect_projected_path(one(24), w, *bad, None) == _lib.ERR_INVALID_ARG, bad
    assert L.pemp_detect_projected_path(None, w, 1, 48, 80, 5, None) == _lib.ERR_INVALID_ARG
    assert L.pemp_detect_projected_path(one(0), w, 1, 48, 80, 5, None) == _lib.ERR_INVALID_ARG


def test_matrix_coverage():
    """The table is the coverage: every body of the strip kernel's projected loads is run by at least one case."""
    hit = set().union(*(pc.cells(c) for c in pc.CASES))
    for loader in ("x2", "sep"):      # template bodies per pool, flipped pass and masks
        for cell in itertools.product([loader], pc.POOLS, (False, True), (False, True)):
            assert cell in hit, cell
    for pool, masked in itertools.product(pc.POOLS, (False, True)):      # (the generic loader tests the pass at run time)
        assert any((("gen", pool, flip, masked) in hit) for flip in (False, True)), (pool, masked)
    assert {c.flip for c in pc.CASES if c.loader == "gen"} == {False, True}
    # both sides of the 16-row limit, on the same pair of maps
    staged = {(c.sizes[0][0], c.size[0], c.pool): pc.staged_rows(c.sizes[0][0], c.size[0], c.pool)
              for c in pc.CASES if len(c.sizes) == 1}
    assert staged[(34, 50, 5)] == 16 and staged[(34, 50, 7)] == 17
    assert staged[(45, 80, 9)] == 16 and staged[(46, 80, 9)] == 17
    assert staged[(31, 48, 5)] == staged[(31, 48, 7)] == 16 and staged[(31, 48, 9)] == 18
    # the four threshold forms on a separable and a generic case; masks with MODE_ALL and with the two-compare test
    for loader in ("sep", "gen"):
        assert {c.thr for c in pc.CASES if c.loader == loader} >= {0.1, 0.0, pc.NEG_THR, 2.0}, loader
    assert any(c.thr > 1.5 and c.mask != "off" for c in pc.CASES)
    assert any(c.thr <= 0 and c.mask != "off" for c in pc.CASES)
    assert any(c.mask == "half" for c in pc.CASES)
    # the scales: a non-power-of-two divisor with and without the flipped pass, 2x + separable, a generic second scale
    assert {c.flip for c in pc.CASES if len(c.sizes) == 3} == {False, True}
    assert any(len(c.sizes) == 2 and c.loader == "x2" for c in pc.CASES)
    assert any(len(c.sizes) == 2 and c.loader == "gen" and c.sizes[0][0] * 2 == c.size[0] for c in pc.CASES)
    assert any(c.divisor == 2.0 and len(c.sizes) == 1 for c in pc.CASES)
    # the columns: one full strip, one column into the second, narrower than a wave, a last strip past the plane
    shapes = {(c.size[1], c.pool) for c in pc.CASES}
    assert {(56, 9), (57, 9), (62, 3)} <= shapes and any(W == 8 for W, _ in shapes)
    assert {pool for W, pool in shapes if W == 130} >= {3, 5, 7, 9}
    assert any(c.sizes[0][0] * 2 == c.size[0] and c.sizes[0][1] * 2 != c.size[1] for c in pc.CASES)
    # the two-kernel selection, with the 2x path in its interior bands; both joint sets; B = 1, 2, 3
    big = pc.BY_NAME["large"]
    units = -(-big.size[0] // pc.SR) * -(-big.size[1] // (64 - 2 * (big.pool // 2)))
    assert units > pc.SEL_UNITS and big.x2 > 0 and big.flip
    assert all(-(-c.size[0] // pc.SR) * -(-c.size[1] // (64 - 2 * (c.pool // 2))) <= pc.SEL_UNITS
               for c in pc.CASES if c.name != "large")
    assert {c.J for c in pc.CASES} == {14, 17} and {c.B for c in pc.CASES} == {1, 2, 3}
    assert sum(c.feats == "projected" for c in pc.CASES) >= 6


@pytest.mark.parametrize("name", pc.NAMES)
def test_oracle_sanity(name):
    """What the case is for exists in the oracle's own answer. A negative score needs a negative value among a
    plane's top-k or over the threshold: the reference zeroes every pixel that is not a maximum or is masked out, and
    those zeros outrank negatives, so only pool 1 without masks (every pixel its own maximum) or a negative threshold
    can yield one; there it is required."""
    c = pc.BY_NAME[name]
    ref = pc.reference(name)[3]
    det, sc, bi = ref[7].numpy(), ref[11].numpy(), ref[12].numpy()
    H, W = c.size
    per_image = np.bincount(bi, minlength=c.B)
    print(f"projected case {name}: detections per image {per_image.tolist()}, edges {ref[2].shape[1]}")
    assert per_image.max() <= 700, name       # the fully graph of the oracle stays cheap
    for what, n in (("x = 0", (det[:, 0] == 0).sum()), ("x = W - 1", (det[:, 0] == W - 1).sum()),
                    ("y = 0", (det[:, 1] == 0).sum()), ("y = H - 1", (det[:, 1] == H - 1).sum())):
        assert n >= 1, (name, what)
    y0, y1, x1 = pc.plateau_box(c)
    inside = ((bi == 0) & np.isin(det[:, 2], pc.PLATEAU_PLANES) & (det[:, 1] >= y0) & (det[:, 1] < y1)
              & (det[:, 0] < x1))
    assert inside.sum() >= 1, name
    if c.B > 1 and ((c.pool == 1 and c.mask == "off") or c.thr < 0):
        assert ((bi == 1) & (sc < 0)).sum() >= 1, name
    if c.mask == "half":                     # some emitted scores are value x 0.5
        masks = pc.make_inputs(name)[2].numpy()
        assert (masks[bi, det[:, 1], det[:, 0]] == 0.5).sum() >= 1, name
