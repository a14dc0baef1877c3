"""Cases and references for the differentiable node features (pemp_amd/node_gather.py, csrc/node_grad.hip;
tests/test_node_grad_cpu.py, tests/test_gpu_node_grad.py). No pytest hooks.

Dense backward: a numpy loop that adds the rows of g in ascending node index in fp32; the device must give its bits.
Conv backward: torch autograd of F.conv2d(raw, W, b, padding=pad)[batch_index, :, y, x] in fp64 on the CPU from the
same fp32-exact inputs, under a derived bound: an fp32 dot product of K products in any order, with or without FMA,
errs by at most gamma_K sum|terms|, gamma_K = K 2^-24 / (1 - K 2^-24); sum|terms| is the same expression on absolute
values in fp64, K the element's product count plus 4 (Cout x entries on the pixel for draw, N for dW and db)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32
B, H, W = 3, 12, 20                    # the middle image stays empty
# (Cin, Cout, k, pad): FMA body with odd channel counts; the published conv (MFMA); k = 1 (MFMA, one column tile);
# no padding (raw is [B, 7, 14, 22]); Cout past 128 and not a multiple of 16, k = 5
CONVS = [(5, 24, 3, 1), (48, 128, 3, 1), (16, 128, 1, 0), (7, 128, 3, 0), (4, 130, 5, 2)]
DENSE_C = [128, 24]
NODE_SETS = ["base", "one", "none", "n257", "n513"]     # 257 and 513: one past a chunk of 256 nodes and two past


def gamma(K):
    u = K * 2.0 ** -24
    return u / (1.0 - u)


@functools.lru_cache(maxsize=None)
def nodes(name):
    """(joint_det [N, 3] int64 (x, y, type), batch_index [N] int64), sorted by image, images 0 and 2 only.
    base: three nodes of different types on one pixel, the four corners, two nodes one pixel apart (their windows
    overlap), one pixel used in both images. The large sets repeat base and add pseudo-random pixels (with repeats)."""
    base = [(7, 5, 0, 0), (7, 5, 3, 0), (7, 5, 9, 0),                                # one pixel, three types
            (0, 0, 1, 0), (W - 1, 0, 2, 0), (0, H - 1, 4, 0), (W - 1, H - 1, 5, 0),  # the corners
            (10, 6, 6, 0), (11, 6, 7, 0), (10, 7, 8, 0),                             # neighbours
            (7, 5, 0, 2), (W - 1, H - 1, 1, 2), (3, 2, 2, 2), (4, 2, 2, 2)]
    if name == "base":
        rows = base
    elif name == "one":
        rows = [(W - 1, 0, 3, 2)]
    elif name == "none":
        rows = []
    else:
        n = int(name[1:])
        rng = np.random.default_rng(n)
        extra = [(int(rng.integers(W)), int(rng.integers(H)), int(rng.integers(17)), int(rng.choice([0, 2])))
                 for _ in range(n - len(base))]
        rows = base + extra
        assert len(rows) == n
    rows = sorted(rows, key=lambda r: r[3])                  # stable: by image, as the constructor lists nodes
    a = np.array(rows, np.int64).reshape(-1, 4)
    return a[:, :3].copy(), a[:, 3].copy()


def values(shape, salt):
    """fp32 values in (-1, 1) from a seeded generator (the same on every machine)."""
    rng = np.random.default_rng(1000 + salt)
    return (rng.random(shape, dtype=np.float64) * 2 - 1).astype(f32)


def dense_backward(g, joint_det, batch_index, shape):
    """dfeat [B, C, H, W]: zeros, then g[n] added at (b_n, :, y_n, x_n) in ascending n, in fp32."""
    out = np.zeros(shape, f32)
    g = np.asarray(g, f32)
    for n in range(joint_det.shape[0]):
        x, y = int(joint_det[n, 0]), int(joint_det[n, 1])
        out[int(batch_index[n]), :, y, x] = out[int(batch_index[n]), :, y, x] + g[n]
    return out


def dense_forward(feats, joint_det, batch_index):
    return np.ascontiguousarray(feats[batch_index, :, joint_det[:, 1], joint_det[:, 0]])


def conv_inputs(case, set_name):
    """raw, weight, bias, g as fp32 numpy, and the node arrays, of one planted case."""
    Cin, Cout, k, pad = case
    jd, bi = nodes(set_name)
    h, w = H + k - 1 - 2 * pad, W + k - 1 - 2 * pad          # the conv output is H x W
    salt = 7 * CONVS.index(case) + NODE_SETS.index(set_name)
    return dict(raw=values((B, Cin, h, w), salt), weight=values((Cout, Cin, k, k), salt + 100) * f32(0.25),
                bias=values((Cout,), salt + 200), g=values((jd.shape[0], Cout), salt + 300), jd=jd, bi=bi, k=k, pad=pad)


def conv_autograd(raw, weight, bias, g, jd, bi, pad, dtype):
    """(x, draw, dW, db) of x = conv2d(raw, W, b, padding=pad)[bi, :, y, x] and its backward from g, by torch on the
    CPU in `dtype` (inputs numpy, converted exactly)."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True)
    r, wt, b = t(raw), t(weight), t(bias)
    jd, bi = torch.from_numpy(jd), torch.from_numpy(bi)
    x = F.conv2d(r, wt, b, padding=pad)[bi, :, jd[:, 1], jd[:, 0]]
    x.backward(torch.from_numpy(np.asarray(g)).to(dtype))
    return tuple(v.detach().numpy() for v in (x, r.grad, wt.grad, b.grad))


def entries_on_pixel(jd, bi, shape, k, pad):
    """[B, h, w]: how many in-bounds (n, dy, dx) land on each pixel of raw."""
    cnt = np.zeros((shape[0], shape[2], shape[3]), np.int64)
    for n in range(jd.shape[0]):
        for dy in range(k):
            for dx in range(k):
                yy, xx = int(jd[n, 1]) - pad + dy, int(jd[n, 0]) - pad + dx
                if 0 <= yy < shape[2] and 0 <= xx < shape[3]:
                    cnt[int(bi[n]), yy, xx] += 1
    return cnt


def conv_reference(d):
    """The fp64 results and the derived bounds of one case: {"x" | "draw" | "dW" | "db": (want fp64, bound fp64)}."""
    raw, weight, bias, g, jd, bi, k, pad = (d[n] for n in ("raw", "weight", "bias", "g", "jd", "bi", "k", "pad"))
    Cout, Cin = weight.shape[:2]
    N = jd.shape[0]
    want = conv_autograd(raw, weight, bias, g, jd, bi, pad, torch.float64)
    mag = conv_autograd(np.abs(raw), np.abs(weight), np.abs(bias), np.abs(g), jd, bi, pad, torch.float64)
    cnt = entries_on_pixel(jd, bi, raw.shape, k, pad)
    K = dict(x=Cin * k * k + 1 + 4, draw=(Cout * cnt + 4)[:, None, :, :], dW=N + 4, db=N + 4)
    return {name: (want[i], gamma(np.asarray(K[name], np.float64)) * mag[i])
            for i, name in enumerate(("x", "draw", "dW", "db"))}


def ratio(got, want, bound):
    """The largest error-to-bound ratio; an element with a zero bound must be exact."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - want)
    assert np.all(err[bound == 0] == 0), "an element with no term is not zero"
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
