"""Cases and inputs of the projected detection (pemp_detect_projected: the three loaders of the NMS strip kernel and
the emission's proj_pixel, csrc/detect.hip) at every pool radius, with and without masks and the flipped pass, on
both sides of the separable loader's 16-row limit and on the plane's four borders (tests/test_projected_cases_cpu.py,
tests/test_gpu_detect_projected.py). Host only; the loader a case takes is stated in the table and restated here in
numpy from csrc/detect.hip (proj_sep_ok, PROJ_X2_BAND). No pytest hooks."""
import collections
import functools

import numpy as np
import torch

from oracle import restate
from pemp_amd import config as pcfg, synthetic as syn

f32 = np.float32
COCO_FLIP = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
CROWD_FLIP = [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 12, 13]
SR, PROJ_LR, SEL_UNITS = 16, 16, 1024      # csrc/detect.hip: rows of a band, staged rows, units of the fused selection
POOLS = (1, 3, 5, 7, 9)
NEG_THR = -0.05


# ---- the loader choice, restated -----------------------------------------------------------------------------------
def tap0(dst, out_size, in_size):
    """First source index of output index dst (proj_taps: torch's source index in fp32, one rounding per operation)."""
    scale = f32(in_size) / f32(out_size)
    src = scale * (f32(dst) + f32(0.5)) - f32(0.5)
    return int(max(src, f32(0)))


def staged_rows(h, H, pool):
    """Low-resolution rows the separable loader stages for its worst band: the band's rows with the halo, clamped to
    the plane, from the first tap of the top row to the second tap of the bottom row, and the one past it."""
    p, worst = pool // 2, 0
    for y0 in range(0, H, SR):
        ya, yb = min(max(y0 - p, 0), H - 1), min(max(y0 + SR + p - 1, 0), H - 1)
        lo, hi = tap0(ya, H, h), tap0(yb, H, h)
        hi += 1 if hi < h - 1 else 0
        worst = max(worst, hi - lo + 2)
    return worst


def x2_bands(h0, H, pool):
    """Bands in which the first scale takes the exact-2x register path (no clamped row in the band's halo)."""
    p = pool // 2
    return sum(1 for y0 in range(0, H, SR) if h0 * 2 == H and y0 - p >= 1 and y0 + SR - 1 + p <= H - 3)


def loader_path(hs, H, pool):
    """(1 generic | 2 separable, bands of the exact-2x path) for scales of hs rows projected to H rows."""
    sep = all(staged_rows(h, H, pool) <= PROJ_LR for h in hs)
    return (2, x2_bands(hs[0], H, pool)) if sep else (1, 0)


# ---- the case table ------------------------------------------------------------------------------------------------
# source rows -> plane rows: (h, H, bands of the 2x path while separable, worst staged rows at pools 1/3/5/7/9)
ROWS = {
    "x2a": (24, 48, 1, (11, 11, 13, 13, 15)),     # 2x in 1 of 3 bands, separable at every pool
    "x2b": (35, 70, 3, (11, 11, 13, 13, 15)),     # 2x in 3 of 5 bands, last band 6 rows
    "b31": (31, 48, 0, (12, 14, 16, 16, 18)),     # exactly 16 at pools 5 and 7, generic at 9
    "b34": (34, 50, 0, (13, 15, 16, 17, 18)),     # 16 at pool 5, 17 (generic) at pool 7, last band 2 rows
    "b45": (45, 80, 0, (12, 12, 14, 14, 16)),     # at the limit at pool 9
    "b46": (46, 80, 0, (12, 13, 14, 15, 17)),     # just past it at pool 9
    "up13": (13, 37, 0, None),                    # strong up-sampling, odd sizes
    "id48": (48, 48, 0, None),                    # identity: generic
    "dn50": (50, 33, 0, None),                    # down-sampling: generic
    "half": (96, 48, 0, None),                    # exact 1/2: generic
    "big": (264, 528, 31, None),                  # 33 bands, the 2x path in all but the first and the last
}
# source columns -> plane columns (unrelated to the row ratios); strips are 64 - 2 (pool // 2) columns wide
COLS = {
    "w57": (23, 57),       # one column into a second strip at pool 9
    "w56": (25, 56),       # exactly one strip at pool 9
    "w62": (27, 62),       # exactly one strip at pool 3
    "w8": (5, 8),          # narrower than a wave
    "w130": (61, 130),     # the last strip ends past the plane
    "w64": (32, 64),       # exactly 2x, one strip at pool 1
    "w40": (40, 40),       # identity
    "big": (900, 1800),
}

Case = collections.namedtuple("Case", "name sizes size pool flip mask loader x2 thr B J divisor feats seed")


def _case(name, rows, cols, pool, flip, mask="off", loader="sep", thr=0.1, B=2, J=17, divisor=None, feats="dense",
          more=()):
    """rows / cols: keys of ROWS / COLS for scale 0; more: further scales as (rows key or h, w); loader: the loader
    the case is for (x2: separable with the 2x bands of ROWS; sep: separable without; gen: generic)."""
    h, H, nx2, _ = ROWS[rows]
    w, W = COLS[cols]
    sizes = [(h, w)] + [(ROWS[r][0] if isinstance(r, str) else r, ww) for r, ww in more]
    assert all(isinstance(r, int) or ROWS[r][1] == H for r, _ in more), name
    return Case(name, tuple(sizes), (H, W), pool, flip, mask, loader, nx2 if loader == "x2" else 0, thr, B, J,
                divisor, feats, 1000 + 7 * len(name) + pool + sum(map(ord, name)))


def _table():
    t = []
    # the 2x and separable loaders: every pool x flipped pass x masks (the bands at the top and bottom of a 2x plane
    # take the separable staging, so a 2x case runs both bodies); the columns walk through COLS
    cols = ["w57", "w130", "w56", "w8", "w62", "w64"]
    n = 0
    for pool in POOLS:
        for flip in (False, True):
            for mask in ("off", "rand"):
                col = cols[n % len(cols)]
                if pool == 9 and col == "w8":      # a 9 x 9 window spans all 8 columns: no maximum left for a border
                    col = "w57"
                if pool == 1 and col == "w130":    # pool 1 emits every pixel above the threshold: keep the plane small
                    col = "w64"
                t.append(_case(f"x2-p{pool}-f{int(flip)}-m{mask}", "x2b" if n % 2 else "x2a", col, pool, flip, mask,
                               "x2", feats="projected" if n % 5 == 0 else "dense"))
                n += 1
    t += [
        # the generic loader: every pool x masks, on the ratios that never fit and just past the 16-row limit
        _case("gen-p1-id", "id48", "w40", 1, True, "off", "gen"),
        _case("gen-p1-down", "dn50", "w57", 1, False, "rand", "gen"),
        _case("gen-p3-half", "half", "w62", 3, False, "off", "gen", feats="projected"),
        _case("gen-p3-id", "id48", "w130", 3, True, "rand", "gen"),
        _case("gen-p5-down", "dn50", "w130", 5, True, "off", "gen", feats="projected"),
        _case("gen-p5-half", "half", "w8", 5, False, "half", "gen"),
        _case("gen-p7-17rows", "b34", "w57", 7, True, "off", "gen"),
        _case("gen-p7-17rows-m", "b34", "w130", 7, False, "rand", "gen"),
        _case("gen-p9-18rows", "b31", "w56", 9, False, "off", "gen"),
        _case("gen-p9-17rows", "b46", "w57", 9, True, "rand", "gen", J=14),
        # the separable loader at its limit and on other ratios
        _case("sep-p5-16rows", "b31", "w57", 5, True, "off", "sep"),
        _case("sep-p7-16rows", "b31", "w130", 7, False, "half", "sep"),
        _case("sep-p5-16rows-cut", "b34", "w57", 5, False, "off", "sep", B=3),
        _case("sep-p9-16rows", "b45", "w56", 9, True, "off", "sep", feats="projected"),
        _case("sep-p1-b45", "b45", "w64", 1, False, "off", "sep"),
        _case("sep-p3-up13", "up13", "w8", 3, True, "rand", "sep", feats="projected"),
        _case("sep-p9-up13", "up13", "w57", 9, False, "off", "sep", J=14),
        # the thresholds: MODE_POS with the one-compare test (0.1), with the two-compare test (0, negative), MODE_ALL
        _case("sep-thr0", "b31", "w57", 5, True, "rand", "sep", thr=0.0),
        _case("sep-thrneg", "b31", "w57", 5, True, "off", "sep", thr=NEG_THR),
        _case("sep-thr2", "b31", "w57", 5, True, "off", "sep", thr=2.0),
        _case("gen-thr0", "b34", "w57", 7, True, "off", "gen", thr=0.0),
        _case("gen-thrneg", "b34", "w57", 7, True, "rand", "gen", thr=NEG_THR),
        _case("gen-thr2", "b34", "w57", 7, True, "rand", "gen", thr=2.0),
        _case("x2-thr2-m", "x2b", "w130", 3, False, "rand", "x2", thr=2.0),
        _case("x2-thrneg", "x2a", "w57", 9, True, "off", "x2", thr=NEG_THR),
        # the scales: 2x + separable; three scales (divisor 3: the IEEE division) with and without the flipped pass;
        # an explicit divisor on one scale; a second scale that alone sends the whole call to the generic loader
        _case("s2-x2-sep", "x2a", "w57", 5, True, "off", "x2", more=[("b31", 40)]),
        _case("s3-flip", "x2a", "w130", 7, True, "rand", "x2", more=[("b31", 40), (13, 19)]),
        _case("s3-noflip", "x2a", "w56", 3, False, "off", "x2", more=[("b31", 40), (13, 19)], feats="projected"),
        _case("s1-div2", "b31", "w62", 3, True, "off", "sep", divisor=2.0),
        _case("s1-div3", "x2b", "w57", 5, False, "rand", "x2", divisor=3.0),
        _case("s2-second-generic", "x2a", "w57", 5, True, "off", "gen", more=[("id48", 57)]),
        # more than 1024 units per plane: the two-kernel selection and emission on projected maps
        _case("large", "big", "big", 9, True, "off", "x2", B=1),
    ]
    assert len({c.name for c in t}) == len(t)
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def cells(c):
    """The (loader, pool, flipped pass, masked) bodies of the strip kernel that the case runs."""
    masked = c.mask != "off"
    kinds = {"x2": ("x2", "sep"), "sep": ("sep",), "gen": ("gen",)}[c.loader]
    return {(k, c.pool, c.flip, masked) for k in kinds}


# ---- the inputs ----------------------------------------------------------------------------------------------------
PLATEAU_PLANES = (0, 1)
PLATEAU = 0.5


def plateau_rows(h):
    r0 = max(2, int(round(0.25 * h)))
    return r0, r0 + 3


def plateau_box(c):
    """The plateau of scale 0 in plane coordinates: y0, y1, x1 (exclusive), generous by one source pixel."""
    (h, w), (H, W) = c.sizes[0], c.size
    r0, r1 = plateau_rows(h)
    return int(r0 * H / h) - 1, int(np.ceil(r1 * H / h)) + 1, int(np.ceil(min(4, w - 1) * W / w)) + 1


def _plant(plane, y, x, v):
    plane[y, x] = max(plane[y, x], v)


def _pass(rng, c, h, w, layout, heights, gain, floor):
    """One pass of one scale in the forward orientation, [B, J, h, w]: the floor, per plane the planted peaks (four
    corners, one on each edge, three interior) of distinct heights, the plateau on image 0 and the negative image."""
    B, J = c.B, c.J
    lo, hi = floor
    hm = (lo + (hi - lo) * rng.random((B, J, h, w))).astype(f32)
    for b in range(B):
        if b == 1:      # negative but for a few values (far below every threshold of the table)
            hm[b] = (-0.9 + 0.4 * rng.random((J, h, w))).astype(f32)
            cy, cx = h // 2, max(w // 2 - 1, 0)
            hm[b, :4, cy:cy + 3, cx:cx + 3] = -0.02                     # ties of negative maxima above NEG_THR
            hm[b, :2, h - 3:h - 1, 0:2] = 0.0
            hm[b, 2, 1:3, w - 3:w - 1] = 0.7
            continue
        for j in range(J if c.pool > 1 else min(J, 4)):                  # (pool 1 emits a peak's whole footprint)
            fy, fx = layout[b, j, :, 0], layout[b, j, :, 1]
            v = heights[b, j] * gain[b, j]
            ey, ex = 1 + int(fy[0] * (h - 3)), 1 + int(fx[0] * (w - 3))
            pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1),
                   (0, ex), (h - 1, 1 + int(fx[1] * (w - 3))), (h - 1 - ey // 3, 0), (ey, w - 1)]
            pts += [(1 + int(fy[k] * (h - 3)), 1 + int(fx[k] * (w - 3))) for k in (2, 3, 4)]
            for k, (y, x) in enumerate(pts):
                _plant(hm[b, j], y, x, f32(v[k]))
        if b == 0:
            r0, r1 = plateau_rows(h)
            hm[0, PLATEAU_PLANES, r0:r1, 0:min(4, w - 1)] = PLATEAU
    return hm


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """(outs, flips or None, masks or None, low-resolution feature map or None) of case `name`: network outputs
    [B, 2J, h, w] per scale (heatmaps, per-joint tags) as float32 torch tensors on the host; the flipped pass as the
    network would produce it (mirrored, its channels in the flipped order) with heights and floor of its own."""
    c = BY_NAME[name]
    rng = np.random.default_rng(c.seed)
    B, J, (H, W) = c.B, c.J, c.size
    fi = np.array(COCO_FLIP if J == 17 else CROWD_FLIP)
    layout = rng.random((B, J, 5, 2))
    heights = (0.6 + 0.6 * rng.permutation(B * J * 11).reshape(B, J, 11) / (B * J * 11)).astype(f32)
    floor = (-0.9, -0.5) if c.thr <= 0 else (0.0, 0.0) if c.pool == 1 else (0.0, 0.04)
    outs, flips = [], []
    for k, (h, w) in enumerate(c.sizes):
        ones = np.ones((B, J, 11), f32)
        hm = _pass(rng, c, h, w, layout, heights, ones, floor)
        outs.append(torch.from_numpy(np.concatenate([hm, syn.closed_form((B, J, h, w), 0.5 + 0.1 * k)], 1)))
        if c.flip:
            g = _pass(rng, c, h, w, layout, heights, (0.8 + 0.4 * rng.random((B, J, 11))).astype(f32), floor)
            fl = np.empty_like(g)
            fl[:, fi] = g[..., ::-1]          # what the oracle's flip and re-index turn back into g
            flips.append(torch.from_numpy(np.concatenate([fl, syn.closed_form((B, J, h, w), 0.7 + 0.1 * k)], 1)))
    masks = None
    if c.mask != "off":
        u = rng.random((B, H, W))
        m = (u > 0.2).astype(f32)
        if c.mask == "half":
            m[u > 0.9] = 0.5
        masks = torch.from_numpy(m)
    low = None
    if c.feats == "projected":
        low = torch.from_numpy(syn.closed_form((B, 16, c.sizes[0][0], c.sizes[0][1]), 0.25))
    return outs, (flips if c.flip else None), masks, low


def flip_index(c):
    return None if not c.flip else COCO_FLIP if c.J == 17 else CROWD_FLIP


def gc_config(c):
    gc = pcfg.inference_gc_config("fully", c.pool, c.mask != "off")
    gc.DETECT_THRESHOLD = c.thr
    return gc


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle on case `name`: (projected scoremaps, projected tags, dense features, construct_graph's tuple)."""
    c = BY_NAME[name]
    outs, flips, masks, low = make_inputs(name)
    s, t = restate.project_frontend(outs, flips, c.size, c.J, flip_index(c), divisor=c.divisor)
    if low is None:
        feats = torch.from_numpy(syn.closed_form((c.B, 16) + c.size, 0.25))
    else:
        feats = torch.from_numpy(restate.upsample_bilinear(low.numpy(), c.size))
    return s, t, feats, restate.construct_graph(s, feats, t, masks, gc_config(c), c.J)


def dense_inputs(thr):
    """A small dense case for pemp_detect's four threshold forms: the heatmaps of the input maker at the plane's own
    size (no projection), masks on."""
    c = _case(f"dense-thr{thr}", "up13", "w130", 3, False, "rand", "sep", thr=thr, B=3)
    H, W = c.size
    c = c._replace(sizes=((H, W),))
    rng = np.random.default_rng(77)
    layout = rng.random((c.B, c.J, 5, 2))
    heights = (0.6 + 0.6 * rng.permutation(c.B * c.J * 11).reshape(c.B, c.J, 11) / (c.B * c.J * 11)).astype(f32)
    floor = (-0.9, -0.5) if thr <= 0 else (0.0, 0.04)
    hm = _pass(rng, c, H, W, layout, heights, np.ones((c.B, c.J, 11), f32), floor)
    masks = (rng.random((c.B, H, W)) > 0.2).astype(f32)
    return c, torch.from_numpy(hm), torch.from_numpy(masks)
