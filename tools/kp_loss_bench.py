"""Forward + backward of the keypoint losses of a training step on the GPU (not part of bench.py).

usage: python tools/kp_loss_bench.py [--rounds 30] [--warmup 5] [--out profiles/kp_loss.md]
  The published training shape: B = 4, J = 17, stage 0 [4, 34, 128, 128] with the associative-embedding term, stage 1
  [4, 17, 256, 256], P = 30 person slots with 9 people per image (about four joints in five visible).
  Whole loss, and the heatmap term alone, the forms alternating round by round:
    (f) the fused loss (pemp_amd.keypoint_loss);
    (a) the oracle's torch form (tests/kp_loss_oracle.py) in fp32 on the same device.
  The associative-embedding term alone: (f), (a), and (b) the reference-style loop, one indexing op per visible joint
  and a torch.stack per person behind joints.cpu() (Utils/loss.py:42-98).
  torch.cuda.Event time around forward + backward of each form, medians with min and max. Then the library's kernels
  alone (its event profiler) against the bytes each pass must move, with the inputs resident in the Infinity Cache
  (calls back to back) and evicted (512 MB written between calls).
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_TBS = 3.7       # what the memory-bound NMS pass reaches inside a step, TB/s
B, J, P, PERSONS = 4, 17, 30, 9
SIZES = ((2 * J, 128, 128), (J, 256, 256))


def spread(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def make_inputs(dev):
    g = torch.Generator().manual_seed(7)
    preds, gts, masks = [], [], []
    for C, H, W in SIZES:
        preds.append((torch.rand((B, C, H, W), generator=g) * 0.5).to(dev).requires_grad_(True))
        gt = torch.rand((B, J, H, W), generator=g)
        gts.append(torch.where(gt > 0.98, gt, torch.zeros_like(gt)).to(dev))
        masks.append((torch.rand((B, H, W), generator=g) > 0.1).float().to(dev))
    H, W = SIZES[0][1:]
    tag = torch.zeros((B, P, J, 2), dtype=torch.int32)
    tag[:, :PERSONS, :, 0] = (torch.arange(J) * H * W).view(1, 1, J).int() + \
        torch.randint(0, H * W, (B, PERSONS, J), generator=g).int()
    tag[:, :PERSONS, :, 1] = (torch.rand((B, PERSONS, J), generator=g) < 0.8).int()
    return preds, gts, masks, [tag, None]


def reference_style_ae(tags_pred, joints, kind):
    """AELoss.forward with its per-joint indexing (Utils/loss.py:42-98); an image without people gives zeros."""
    joints = joints.cpu().data.numpy()
    pushes, pulls = [], []
    for i in range(tags_pred.size(0)):
        pred_tag, tags, pull = tags_pred[i], [], 0
        for person in joints[i]:
            tmp = [pred_tag[j[0]] for j in person if j[1] > 0]
            if not tmp:
                continue
            tmp = torch.stack(tmp)
            tags.append(torch.mean(tmp, dim=0))
            pull = pull + torch.mean((tmp - tags[-1].expand_as(tmp)) ** 2)
        n = len(tags)
        tags = torch.stack(tags)
        diff = tags.expand(n, n) - tags.expand(n, n).permute(1, 0)
        push = torch.sum(torch.exp(-torch.pow(diff, 2))) - n if kind == "exp" else \
            torch.clamp(1 - torch.abs(diff), min=0).sum() - n
        pushes.append(push / ((n - 1) * n) * 0.5)
        pulls.append(pull / n)
    return torch.stack(pushes), torch.stack(pulls)


def make_forms(dev, mode):
    import pemp_amd
    from tests import kp_loss_oracle as ko
    preds, gts, masks, tags = make_inputs(dev)
    ae_only = mode == "ae"
    opt = dict(NUM_JOINTS=J, WITH_HEATMAPS_LOSS=() if ae_only else (True, True), HEATMAPS_LOSS_FACTOR=(1.0, 1.0),
               WITH_AE_LOSS=() if mode == "heat" else (True, False), AE_LOSS_TYPE="exp", PUSH_LOSS_FACTOR=(0.001, 0.001),
               PULL_LOSS_FACTOR=(0.001, 0.001))
    dev_tags = [tags[0].to(dev), None]
    if ae_only:
        preds, gts, masks = preds[:1], [None], [None]
        tags, dev_tags = tags[:1], dev_tags[:1]

    def clear():
        for p in preds:
            p.grad = None

    def fused():
        clear()
        pemp_amd.keypoint_loss(preds, gts, masks, dev_tags, opt, validate=False)[0].backward()

    def oracle():
        clear()
        ko.keypoint_loss(preds, gts, masks, tags, opt)[0].backward()

    def loop():
        clear()
        t = preds[0][:, J:].contiguous().view(B, -1, 1)
        push, pull = reference_style_ae(t, dev_tags[0], "exp")
        ((push * 0.001).mean() + (pull * 0.001).mean()).backward()

    forms = dict(f=fused, a=oracle)
    if ae_only:
        forms["b"] = loop
    return forms, lambda: [p.grad.clone() for p in preds]


def measure(forms, rounds, warmup):
    ts = {k: [] for k in forms}
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return ts


def kernel_us(fn, reps, evict):
    """{label: us per call} from the library's event profiler; ``evict``: write 512 MB before every call."""
    from pemp_amd import _lib
    big = torch.empty(512 << 20, dtype=torch.uint8, device="cuda:0") if evict else None
    _lib.prof_enable("kp_loss")
    try:
        _lib.prof_report()
        for _ in range(reps):
            if evict:
                big.fill_(1)
            fn()
        rep = _lib.prof_report()
    finally:
        _lib.prof_enable(None)
    return {label: 1e3 * ms / reps for label, (n, ms) in rep.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kp_loss_bench: no HIP device (the measurement has no CPU form)")
    dev = torch.device("cuda:0")
    vis = int(make_inputs("cpu")[3][0][..., 1].sum())
    out = ["# Keypoint losses of a training step: the fused pass against torch\n",
           f"`python tools/kp_loss_bench.py --rounds {args.rounds} --warmup {args.warmup}` on "
           f"{torch.cuda.get_device_name(0)}; B = {B}, J = {J}, stage 0 {[B, *SIZES[0]]} with the associative-embedding "
           f"term, stage 1 {[B, *SIZES[1]]}, P = {P} slots with {PERSONS} people per image ({vis} visible joints in all). "
           "Forward + backward, torch.cuda.Event time around each call (host work of the call included), the forms "
           "alternating round by round after the warm-up; median (min .. max) in ms. The yardsticks are torch on the "
           "same device in the same process.\n"]
    names = dict(f="(f) fused `keypoint_loss`", a="(a) the oracle's torch form, fp32",
                 b="(b) reference-style loop, one indexing op per visible joint")
    fused = None
    titles = dict(both="Both terms, both stages", heat="The heatmap term alone, both stages",
                  ae="The associative-embedding term alone")
    for mode in ("both", "heat", "ae"):
        forms, grads = make_forms(dev, mode)
        ts = measure(forms, args.rounds, args.warmup)
        forms["f"]()
        gf = grads()
        forms["a"]()
        ga = grads()
        torch.cuda.synchronize()
        dev_max = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(gf, ga))
        out += [f"## {titles[mode]}\n", "| form | ms |",
                "|---|---|"] + [f"| {names[k]} | {spread(ts[k])} |" for k in forms]
        med = statistics.median(ts["f"])
        out += ["", ", ".join(f"({k}) median / (f) median: {statistics.median(ts[k]) / med:.1f}" for k in forms if k != "f")
                + f". Largest |(f) - (a)| over the largest |(a)| of the gradients: {dev_max:.1e}.\n"]
        if mode == "both":
            fused = forms["f"]
    mb_f = sum(B * J * H * W * 8 + B * H * W * 4 for C, H, W in SIZES) / 1e6
    mb_b = mb_f + sum(B * C * H * W * 4 for C, H, W in SIZES) / 1e6
    out += ["## The library's kernels against the bytes they must move\n",
            f"Both terms, both stages. Forward: pred's heatmap planes, gt and the masks, {mb_f:.1f} MB; backward: the "
            f"same reads and the full-size gradients, {mb_b:.1f} MB. The library's event profiler around each launch "
            "(the event records' overhead is inside the figure), 20 calls. Warm: calls back to back, so the inputs "
            "(under the 256 MB of the Infinity Cache) can be served from it; cold: 512 MB written between the calls. "
            f"The yardstick rate is the {STEP_TBS} TB/s the memory-bound NMS pass reaches inside a step (DESIGN 8).\n",
            "| cache | label | us | bytes (MB) | achieved TB/s | us at the yardstick rate | share of it reached |",
            "|---|---|---|---|---|---|---|"]
    for evict in (False, True):
        rep = kernel_us(fused, 20, evict)
        for label in ("kp_loss_fwd", "kp_loss_reduce", "kp_loss_bwd", "kp_loss_bwd_tags"):
            us = rep.get(label)
            if us is None:
                continue
            mb = {"kp_loss_fwd": mb_f, "kp_loss_bwd": mb_b}.get(label)
            cache = "cold" if evict else "warm"
            if mb:
                out.append(f"| {cache} | {label} | {us:.1f} | {mb:.1f} | {mb / us:.2f} | {mb / STEP_TBS:.1f} | "
                           f"{100 * mb / us / STEP_TBS:.0f} % |")
            else:
                out.append(f"| {cache} | {label} | {us:.1f} | | | | |")
    out.append("")
    text = "\n".join(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
