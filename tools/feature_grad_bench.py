"""Forward + backward of the feature path of a training step on the GPU (not part of bench.py): from the raw
backbone features to x and back to feature_gather's weight, bias and (end-to-end) the raw features.

usage: python tools/feature_grad_bench.py [--rounds 30] [--warmup 5] [--out profiles/feature_grad.md]
  The published training shape: B = 4, feature_gather 48 -> 128 channels, 3 x 3, padding 1, H = W = 256, about 150
  detections per image (the constructor's own detections on planted peaks). Three forms, alternating round by round:
    (a) the reference's: torch conv2d over the whole map, x = features[b, :, y, x], torch autograd;
    (b) the dense conv with the node-order scatter backward (pemp_amd.gather_nodes);
    (c) the sparse path: the conv under the detections only, both ways (pemp_amd.gather_nodes_conv).
  torch.cuda.Event time around forward + backward of each form, medians with min and max, and the peak device
  memory a form adds. Then the library's kernels alone (its event profiler) against the bytes each must move.
  Twice: end to end (raw requires a gradient) and with the backbone frozen (only the conv's parameters do).
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3        # achievable HBM rate of the MI355X (float4 copy), TB/s
B, CIN, COUT, K, PAD, H, W, J, PERSONS = 4, 48, 128, 3, 1, 256, 256, 17, 9


def spread(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def detections(dev):
    """joint_det, batch_index of the constructor on planted peaks (9 people x 17 joints per image)."""
    import pemp_amd
    from pemp_amd import config as pcfg, synthetic as syn
    hm = torch.from_numpy(syn.make_heatmaps(3, B, J, H, W, PERSONS)).to(dev)
    out = pemp_amd.get_graph_constructor(pcfg.inference_gc_config("fully", 5, False), scoremaps=hm,
                                         features=torch.zeros(B, 1, H, W, device=dev), tagmaps=None, joints_gt=None,
                                         factor_list=None, masks=None, device=dev, testing=True, heatmaps=None,
                                         num_joints=J).construct_graph()
    return out[7].clone(), out[12].clone()


def make_forms(dev, jd, bi, raw_grad):
    import pemp_amd
    from pemp_amd import synthetic as syn
    conv = torch.nn.Conv2d(CIN, COUT, K, padding=PAD).to(dev)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(syn.closed_form((COUT, CIN, K, K), 0.1) * np.float32(0.1)))
        conv.bias.copy_(torch.from_numpy(syn.closed_form((COUT,), 0.2)))
    raw = torch.from_numpy(syn.closed_form((B, CIN, H, W), 0.3)).to(dev).requires_grad_(raw_grad)
    g = torch.from_numpy(syn.closed_form((jd.shape[0], COUT), 0.4)).to(dev)
    ys, xs = jd[:, 1], jd[:, 0]

    def clear():
        raw.grad = conv.weight.grad = conv.bias.grad = None

    def form_a():
        clear()
        conv(raw)[bi, :, ys, xs].backward(g)

    def form_b():
        clear()
        pemp_amd.gather_nodes(conv(raw), jd, bi).backward(g)

    def form_c():
        clear()
        pemp_amd.gather_nodes_conv(raw, conv, jd, bi).backward(g)

    grads = lambda: [t.grad.clone() for t in (conv.weight, conv.bias) + ((raw,) if raw_grad else ())]
    return dict(a=form_a, b=form_b, c=form_c), grads, clear


def measure(forms, clear, rounds, warmup):
    """{form: (times in ms, peak bytes added)}: the forms alternate round by round."""
    peak, ts = {}, {k: [] for k in forms}
    for k, fn in forms.items():
        for _ in range(warmup):
            fn()
        clear()                               # (the gradients of the last call are part of what a call adds)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
    for _ in range(rounds):
        for k, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: (ts[k], peak[k]) for k in forms}


def kernel_rows(fn, reps, N, raw_grad):
    """[(label, launches per call, us per call, MB the kernels must move per call)] of one form."""
    from pemp_amd import _lib
    KC, M = CIN * K * K, N * K * K
    chunks = (N + 255) // 256
    part = COUT * KC + COUT
    f = 4
    need = {   # bytes per call, from the shapes
        "gather_projected_conv": f * (N * CIN * (K + 1) ** 2 + KC * COUT + COUT + N * COUT) + 32 * N,
        # D = g W2 (read g and W2, write D) when raw takes a gradient; the chunk partials (read g, the windows, write)
        "node_conv_bwd": (f * (N * COUT + COUT * KC + N * KC) if raw_grad else 0)
        + f * (2 * N * COUT + N * KC + chunks * part) + 32 * N,
        "node_conv_tree": f * (chunks * part + part),
        # the ordered per-pixel sum: rows, keys and entries in, the touched pixels out (upper bound: every row its own)
        "node_grad_pixels": f * 2 * M * CIN + 16 * M,
        "gather_projected": f * 2 * N * COUT + 32 * N,
    }
    dense_pixels = f * 2 * N * COUT + 16 * N
    _lib.prof_enable("*")
    try:
        _lib.prof_report()
        for _ in range(reps):
            fn()
        rep = _lib.prof_report()
    finally:
        _lib.prof_enable(None)
    rows = []
    for label, (n, ms) in sorted(rep.items()):
        nbytes = need.get(label, 0)
        if label == "node_grad_pixels" and "node_conv_bwd" not in rep:
            nbytes = dense_pixels
        rows.append((label, n / reps, 1e3 * ms / reps, nbytes / 1e6))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_grad_bench: no HIP device (the measurement has no CPU form)")
    dev = torch.device("cuda:0")
    jd, bi = detections(dev)
    N = jd.shape[0]
    per_image = np.bincount(bi.cpu().numpy(), minlength=B).tolist()
    out = [f"# Feature path of a training step: dense conv + autograd against the sparse path\n",
           f"`python tools/feature_grad_bench.py --rounds {args.rounds} --warmup {args.warmup}` on "
           f"{torch.cuda.get_device_name(0)}; B = {B}, feature_gather {CIN} -> {COUT}, {K} x {K}, padding {PAD}, "
           f"H = W = {H}; N = {N} detections ({per_image} per image). Forward + backward of the feature path, "
           "torch.cuda.Event time around each call, the three forms alternating round by round; median (min .. max) "
           "in ms; peak = the device memory a call adds to what is allocated before it.\n"]
    for raw_grad in (True, False):
        forms, grads, clear = make_forms(dev, jd, bi, raw_grad)
        res = measure(forms, clear, args.rounds, args.warmup)
        forms["a"]()
        ga = grads()
        forms["c"]()
        gc = grads()
        torch.cuda.synchronize()
        dev_max = [float((x - y).abs().max() / x.abs().max()) for x, y in zip(ga, gc)]
        title = "End to end (raw requires a gradient)" if raw_grad else "Backbone frozen (only feature_gather trains)"
        out += [f"## {title}\n", "| form | ms | peak MB |", "|---|---|---|"]
        names = dict(a="(a) torch conv2d + indexing + autograd", b="(b) dense conv + `gather_nodes`",
                     c="(c) sparse `gather_nodes_conv`")
        for k in "abc":
            out.append(f"| {names[k]} | {spread(res[k][0])} | {res[k][1] / 1e6:.1f} |")
        med_c, min_a = statistics.median(res["c"][0]), min(res["a"][0])
        out += ["", f"(a) median / (c) median: {statistics.median(res['a'][0]) / med_c:.2f}. Acceptance ((c)'s median "
                f"below (a)'s minimum, {med_c:.3f} against {min_a:.3f} ms): {'met' if med_c < min_a else 'NOT met'}. "
                f"Largest |(a) - (c)| over the largest |(a)| of " +
                ", ".join(f"{n} {d:.1e}" for n, d in zip(("dW", "db", "draw"), dev_max)) + ".\n"]
        out += ["Kernels of the library alone (its event profiler around each launch; the event records' overhead is "
                "inside the figure), per call, against the bytes they must move at the achievable HBM rate "
                f"({HBM_TBS} TB/s):\n",
                "| form | label | launches | us | bytes (MB) | bytes at the HBM rate (us) | time / that |",
                "|---|---|---|---|---|---|---|"]
        for k in "bc":
            for label, n, us, mb in kernel_rows(forms[k], 20, N, raw_grad):
                floor = mb / HBM_TBS
                out.append(f"| ({k}) | {label} | {n:g} | {us:.1f} | {mb:.2f} | {floor:.2f} | "
                           f"{us / floor:.0f}x |" if floor else f"| ({k}) | {label} | {n:g} | {us:.1f} | | | |")
        out.append("")
    text = "\n".join(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
