"""Training-step timing of the MPN on the GPU (not part of bench.py).

usage: python tools/train_bench.py [--iters 30] [--warmup 5] [--out profiles/train_step.md]
  * forward + backward of the published attention model (T = 17, STEPS 3) on bench.py's c3 graph (E = 186,048):
    the HIP operators (model.train()) against the same forward with tests/train_oracle's torch operators
    (index_add_ / scatter_reduce, float atomics), same GPU, same process, alternating;
  * the same step with model.fused_edge_update = True against the unfused one (the default), alternating pairs;
  * the operators alone, forward + backward, against their torch forms at that shape, with the bytes each
    kernel has to move over the time it took, as a share of the achievable HBM rate; the fused edge update
    (tr.edge_update) against the torch concatenation form of the same block.
torch.cuda.Event timing around each call after a warm-up, medians. The operators' torch forms are the oracle's.

       python tools/train_bench.py --leg loss [--out profiles/train_loss.md]
  * the MPN loss (pemp_amd.loss.mpn_loss, csrc/loss.hip) forward + backward on the c3 graph's logits (STEPS 3,
    AUX_LOSS_STEPS 2: 3 edge, 4 node and 4 class predictions) against tests/loss_oracle's fp32 torch form, alternating;
    the library's launches (its event profiler) and torch's kernel count (torch.profiler);
  * the whole step, construct labels -> forward -> loss -> backward, on a labelled batch of c3's shape with either loss.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3        # achievable HBM rate of the MI355X (float4 copy), TB/s


def spread(ts):
    return statistics.median(ts), min(ts), max(ts)


def timed(fn, iters, warmup):
    """Median and spread (min, max) of fn's device time in ms."""
    return spread(samples(fn, iters, warmup))


def samples(fn, iters, warmup):
    """fn's device time in ms, call by call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def loss_leg(args):
    import bench
    from pemp_amd import _lib, config as pcfg, loss as pl, synthetic as syn
    import pemp_amd
    from tests import loss_oracle as lo
    from tests.test_labels_cpu import label_config

    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["c3"]
    J = wl["J"]
    mcfg = pcfg.published_mpn_config(J, 3, "attn")
    mcfg.AUX_LOSS_STEPS = 2
    model = pemp_amd.get_mpn_model(mcfg)
    model.load_state_dict(syn.closed_form_state_dict(model, 0.5))
    model.to(dev).train()
    opt = dict(NODE_THRESHOLD=0.5)

    # ---- the loss alone: c3's graph, the training forward's logits, synthetic labels
    gc = pcfg.inference_gc_config(wl["graph"], 5, False)
    hm, feats, tags = bench.make_inputs(wl, 0, dev)
    out = bench.run_step(wl, gc, bench.make_model(wl, dev)[0], hm, feats, tags, dev)[0]
    x, ea, ei, types = out[0].clone(), out[1].clone(), out[2].clone(), out[7][:, 2].clone()
    N, E = x.shape[0], ei.shape[1]
    with torch.no_grad():
        pe, pn, pc, _ = model(x, ea, ei, node_types=types)
    pe, pn, pc = ([t.detach().clone() for t in ts] for ts in (pe, pn, pc))
    g = torch.Generator(device=dev).manual_seed(9)
    persons = torch.randint(0, 9, (N,), generator=g, device=dev)
    node_labels = (torch.rand(N, generator=g, device=dev) < 0.6).float()
    on = node_labels == 1
    edge_labels = (on[ei[0]] & on[ei[1]] & (persons[ei[0]] == persons[ei[1]])).float()
    label_mask = (torch.rand(E, generator=g, device=dev) < 0.9).float()
    mask_node = (torch.rand(N, generator=g, device=dev) < 0.9).float()
    classes = torch.randint(0, J, (N,), generator=g, device=dev)
    rest = (ei, edge_labels, label_mask, node_labels, mask_node, classes)

    def leaves():
        return ([t.detach().requires_grad_(True) for t in ts] for ts in (pe, pn, pc))

    def loss_hip():
        a, b, c = leaves()
        pl.mpn_loss(a, b, c, *rest, opt)[0].backward()

    def loss_torch():
        a, b, c = leaves()
        lo.mpn_loss(a, b, c, *rest, opt)[0].backward()

    alone = {"hip": [], "torch": []}
    for _ in range(3):
        alone["hip"] += samples(loss_hip, args.iters, args.warmup)
        alone["torch"] += samples(loss_torch, args.iters, args.warmup)
    alone = {k: spread(v) for k, v in alone.items()}
    _lib.prof_enable("loss_")
    for _ in range(args.iters):
        loss_hip()
    torch.cuda.synchronize()
    launches = {k: (n // args.iters, ms / n * 1e3) for k, (n, ms) in _lib.prof_report().items()}
    _lib.prof_enable(None)
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            loss_torch()
            torch.cuda.synchronize()
        torch_kernels = sum(1 for ev in prof.events() if str(ev.device_type).endswith("CUDA"))
    except Exception as exc:           # no tracer on this host: the count is left out, the timings stand
        torch_kernels = f"not counted ({type(exc).__name__})"

    # ---- the whole step on a labelled batch of c3's shape
    hm_l, gt, fac = syn.make_labelled_heatmaps(7, wl["B"], J, wl["H"], wl["W"], 7)
    lcfg = label_config(dict(graph="fully", method=6, use_neighbours=True, with_background=False,
                             matching_radius=0.5, inclusion_radius=0.75))
    hm_l, gt, fac = torch.from_numpy(hm_l).to(dev), torch.from_numpy(gt), torch.from_numpy(fac)
    cfg = pcfg.get_config()
    cfg.MODEL.MPN = mcfg
    cfg.merge({"MODEL": {"LOSS": {"NAME": ["edge", "node", "class"]}, "MPN": {"NODE_THRESHOLD": 0.5}}})
    loss_fn = pemp_amd.MPNLoss(cfg)
    shape = {}

    def whole(hip):
        model.zero_grad(set_to_none=True)
        o = pemp_amd.get_graph_constructor(lcfg, scoremaps=hm_l, features=feats, tagmaps=tags, joints_gt=gt,
                                           factor_list=fac, masks=None, device=dev, testing=True, heatmaps=None,
                                           num_joints=J).construct_graph()
        shape["N"], shape["E"] = o[0].shape[0], o[2].shape[1]
        preds = model(o[0], o[1], o[2], node_types=o[7][:, 2])
        if hip:
            total = loss_fn(o, preds)[0]
        else:
            total = lo.mpn_loss(preds[0], preds[1], preds[2], o[2], o[3], o[8], o[4], o[9], o[5], opt)[0]
        total.backward()

    step = {"hip": [], "torch": []}
    for _ in range(3):
        step["hip"] += samples(lambda: whole(True), args.iters, args.warmup)
        step["torch"] += samples(lambda: whole(False), args.iters, args.warmup)
    step = {k: spread(v) for k, v in step.items()}
    load = os.getloadavg()
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    ok = alone["hip"][0] < alone["torch"][0]
    inside = step["hip"][0] >= step["torch"][1] and step["hip"][0] <= step["torch"][2]
    lines = ["# The MPN loss: one fused HIP pass each way against its torch form", "",
             f"`python tools/train_bench.py --leg loss --iters {args.iters} --warmup {args.warmup}` on "
             f"{torch.cuda.get_device_name(0)}; host load average {load[0]:.1f} / {load[1]:.1f} / {load[2]:.1f} on "
             f"{os.cpu_count()} CPUs. torch.cuda.Event time around each call, 3 alternating rounds of {args.iters} calls "
             f"after {args.warmup} warm-ups each, pooled: median (min .. max) in ms.", "",
             "## The loss alone, forward + backward", "",
             f"bench.py's c3 graph: N = {N}, E = {E}; the published attention model's training logits (STEPS 3, "
             f"AUX_LOSS_STEPS 2: {len(pe)} edge, {len(pn)} node, {len(pc)} class predictions), focal terms, threshold 0.5.", "",
             "| form | ms |", "|---|---|",
             f"| HIP (`pemp_amd.mpn_loss`) | {fmt(alone['hip'])} |",
             f"| torch (`tests/loss_oracle.mpn_loss`, fp32) | {fmt(alone['torch'])} |", "",
             f"Ratio torch / HIP: {alone['torch'][0] / alone['hip'][0]:.2f}. Acceptance (the HIP form faster than its "
             f"torch form at this shape): {'met' if ok else 'NOT met'}.", "",
             "Launches per forward + backward, HIP form (the library's event profiler, us per launch with the event "
             "records' overhead inside): " + ", ".join(f"{k} x{n} ({us:.1f} us)" for k, (n, us) in sorted(launches.items()))
             + f". torch form: {torch_kernels} kernels (torch.profiler, one forward + backward).", "",
             "## The whole step: construct labels -> forward -> loss -> backward", "",
             f"A labelled batch of c3's shape (B = {wl['B']}, {wl['H']} x {wl['W']}, synthetic ground truth, "
             f"EDGE_LABEL_METHOD 6): N = {shape['N']}, E = {shape['E']}.", "",
             "| loss | ms |", "|---|---|",
             f"| HIP (`MPNLoss`) | {fmt(step['hip'])} |",
             f"| torch (`tests/loss_oracle.mpn_loss`) | {fmt(step['torch'])} |", "",
             f"Difference of the medians: {step['torch'][0] - step['hip'][0]:.3f} ms of {step['torch'][0]:.3f} ms. "
             + ("The HIP median lies inside the torch form's own min .. max: at the whole step the difference is inside "
                "the run-to-run spread." if inside else
                "The HIP median lies outside the torch form's own min .. max.")]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="step", choices=["step", "loss"], help="loss: the MPN loss leg alone")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5, help="alternations of the unfused and the fused model step")
    ap.add_argument("--out", default=None, help="profiles/train_step.md, or profiles/train_loss.md for --leg loss")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "train_loss.md" if args.leg == "loss" else "train_step.md")
    if not torch.cuda.is_available():
        raise SystemExit("train_bench: no HIP device (timings are taken on the GPU only)")
    if args.leg == "loss":
        return loss_leg(args)
    import bench
    from pemp_amd.mpn import train as tr
    from tests import train_oracle as to

    dev = torch.device("cuda", 0)
    wl = bench.WORKLOADS["c3"]
    gc = bench.pcfg.inference_gc_config(wl["graph"], 5, False)
    hm, feats, tags = bench.make_inputs(wl, 0, dev)
    model, cfg = bench.make_model(wl, dev)
    out = bench.run_step(wl, gc, model, hm, feats, tags, dev)[0]
    x, ea, ei, types = out[0].clone(), out[1].clone(), out[2].clone(), out[7][:, 2].clone()
    N, E, T = x.shape[0], ei.shape[1], model.num_types
    model.train()
    sd = {k: (v.detach().clone().requires_grad_(v.is_floating_point() and not k.endswith(("running_mean", "running_var"))))
          for k, v in model.state_dict().items()}

    def step_hip():
        model.zero_grad(set_to_none=True)
        pe, pn, pc, _ = model(x, ea, ei, node_types=types)
        to.fixture_loss(pe, pn, pc).backward()

    def step_torch():
        for v in sd.values():
            v.grad = None
        pe, pn, pc, _ = to.train_forward(sd, cfg, x, ea, ei, types)
        to.fixture_loss(pe, pn, pc).backward()

    # alternate the two forms (other people's work shares the host): two rounds each, the better median kept
    res = {"hip": [], "torch": []}
    for _ in range(2):
        res["hip"].append(timed(step_hip, args.iters, args.warmup))
        res["torch"].append(timed(step_torch, args.iters, args.warmup))
    step = {k: min(v) for k, v in res.items()}

    # the fused edge update against the unfused step (the default, the code above), alternating
    def step_fused():
        model.fused_edge_update = True
        try:
            step_hip()
        finally:
            model.fused_edge_update = False

    pair = {"unfused": [], "fused": []}
    for _ in range(args.pairs):
        pair["unfused"] += samples(step_hip, args.iters, args.warmup)
        pair["fused"] += samples(step_fused, args.iters, args.warmup)
    fused = {k: spread(v) for k, v in pair.items()}

    plan = tr.build_plan(ei, types, N, T)
    src, dst, tsrc = plan.src, plan.dst, plan.type_src
    g = torch.Generator(device=dev).manual_seed(5)
    msgs0 = torch.rand(E, 64, generator=g, device=dev)
    sc0 = torch.rand(E, generator=g, device=dev) * 4 - 2
    w_out = torch.rand(N * T, 64, generator=g, device=dev) - 0.5
    from pemp_amd import _lib

    def kernel_us(fn, filt="seg_"):
        """{label: us per launch} of the library's own kernels under fn (its event profiler, one event pair per
        launch: the figure includes the event records' overhead)."""
        _lib.prof_enable(filt)
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        st = _lib.prof_report()
        _lib.prof_enable(None)
        return {k: ms / n * 1e3 for k, (n, ms) in st.items()}

    ops = []
    for kind in ("attn", "add", "mean", "max"):
        def run(hip, kind=kind):
            m = msgs0.detach().requires_grad_(True)
            s = sc0.detach().requires_grad_(True) if kind == "attn" else None
            o = tr.seg_aggregate(m, s, plan, kind) if hip else to.seg_aggregate(m, s, dst, tsrc, N, T, kind)
            o.backward(w_out)
        # bytes the kernels must move: forward rows + indices + out (ATTN: scores read twice cached, alpha written),
        # backward grad_out + (ATTN: rows and alpha again) + grad rows (+ grad_scores)
        fwd = E * (256 + 4) + N * T * 256 + (E * 8 if kind == "attn" else 0) + (N * T * 256 if kind == "max" else 0)
        bwd = N * T * 256 + E * (256 + 4) + (E * (256 + 8) if kind == "attn" else 0) + (N * T * 256 if kind == "max" else 0)
        ops.append((f"seg_aggregate {kind}", timed(lambda: run(True), args.iters, args.warmup),
                    timed(lambda: run(False), args.iters, args.warmup), fwd + bwd, kernel_us(lambda: run(True)),
                    {"seg_aggr_fwd": fwd, "seg_aggr_bwd": bwd}))
    for W in (64, 128):
        x0 = torch.rand(N, W, generator=g, device=dev)
        gi, gj = torch.rand(E, W, generator=g, device=dev), torch.rand(E, W, generator=g, device=dev)

        def run(hip, x0=x0, gi=gi, gj=gj):
            xx = x0.detach().requires_grad_(True)
            a, b = tr.gather_pair(xx, plan) if hip else to.gather_pair(xx, src, dst)
            torch.autograd.backward([a, b], [gi, gj])
        nbytes = 2 * E * W * 4 * 2 + 2 * E * 4 + N * W * 4       # gather: 2 E rows written; backward: 2 E rows read
        ops.append((f"gather_pair W={W}", timed(lambda: run(True), args.iters, args.warmup),
                    timed(lambda: run(False), args.iters, args.warmup), nbytes, kernel_us(lambda: run(True)),
                    {"seg_rows_sum": 2 * E * W * 4 + 2 * E * 4 + N * W * 4}))

    # the edge update mlp_edge(cat([x[dst], x[src], ef])) at the model's widths (SKIP: Wn = We = 128)
    mlp = model.mpn_node_cls.mlp_edge
    Wn = (mlp[0].in_features) // 3
    nf0 = torch.rand(N, Wn, generator=g, device=dev) - 0.3
    ef0 = torch.rand(E, Wn, generator=g, device=dev) - 0.3
    ge = torch.rand(E, 64, generator=g, device=dev) - 0.5

    def run_edge(form):
        for p in mlp.parameters():
            p.grad = None
        nf, ef = nf0.detach().requires_grad_(True), ef0.detach().requires_grad_(True)
        if form == "fused":
            o = tr.edge_update(nf, ef, plan, mlp)
        elif form == "unfused":                                  # the model's default path
            o = mlp(torch.cat([*tr.gather_pair(nf, plan), ef], dim=1))
        else:                                                    # plain torch (index_add_ backward, float atomics)
            o = mlp(torch.cat([nf[dst], nf[src], ef], dim=1))
        o.backward(ge)
    nchunk = (E + 255) // 256
    part = 4 * (64 * Wn + 64 * 64 + 64)
    # forward: ef and the ids read, h and e_new written (the P / Q rows come from L2); backward: g, ef, h, e_new read,
    # g1 and g_ef written, one partial per 256 edges written (and read again by the tree)
    e_fwd = E * (Wn * 4 + 8 + 512)
    e_bwd = E * (3 * 256 + Wn * 4 + 256 + Wn * 4) + nchunk * part
    e_tree = (nchunk + (nchunk + 31) // 32 * 2 + 1) * part
    e_rows = 2 * (E * (256 + 4) + N * 256)
    edge_t = {f: timed(lambda f=f: run_edge(f), args.iters, args.warmup) for f in ("fused", "torch", "unfused")}
    edge_k = kernel_us(lambda: run_edge("fused"), "edge_mlp")
    edge_k.update({"seg_rows_sum (dP, dQ; each)": v for k, v in kernel_us(lambda: run_edge("fused")).items()})
    ops.append((f"edge_update We={Wn}", edge_t["fused"], edge_t["torch"], e_fwd + e_bwd + e_tree + e_rows, edge_k,
                {"edge_mlp_fwd": e_fwd, "edge_mlp_bwd": e_bwd, "edge_mlp_tree": e_tree,
                 "seg_rows_sum (dP, dQ; each)": e_rows // 2}))
    ok_model = fused["fused"][0] < fused["unfused"][1]
    ok_op = edge_t["fused"][0] < edge_t["torch"][0]

    lines = ["# Training step of the MPN: HIP graph operators against their torch forms", "",
             f"`python tools/train_bench.py --iters {args.iters} --warmup {args.warmup}` on {torch.cuda.get_device_name(0)}; "
             f"bench.py's c3 graph: N = {N}, E = {E}, T = {T}, STEPS {cfg.STEPS}, attention model. "
             "torch.cuda.Event time around each call, medians (min .. max) in ms.", "",
             "## Forward + backward of the model", "",
             "| form | ms |", "|---|---|",
             f"| HIP operators (`model.train()`) | {step['hip'][0]:.3f} ({step['hip'][1]:.3f} .. {step['hip'][2]:.3f}) |",
             f"| torch operators (`tests/train_oracle`, float atomics) | {step['torch'][0]:.3f} "
             f"({step['torch'][1]:.3f} .. {step['torch'][2]:.3f}) |", "",
             f"Ratio torch / HIP: {step['torch'][0] / step['hip'][0]:.2f}. Both forms run the same dense layers "
             "through torch autograd; they differ in the graph operators (and in the per-type message MLPs' "
             "bucketing, a permutation here and boolean masks there).", "",
             "## The fused edge update (`model.fused_edge_update = True`) against the default", "",
             f"{args.pairs} alternating pairs of {args.iters} steps (after {args.warmup} warm-up steps each), all "
             "steps of a form pooled: median (min .. max) in ms.", "",
             "| form | ms |", "|---|---|",
             f"| unfused (default; gather_pair, concatenation, torch GEMMs) | {fused['unfused'][0]:.3f} "
             f"({fused['unfused'][1]:.3f} .. {fused['unfused'][2]:.3f}) |",
             f"| fused (`tr.gather_dst` + `tr.edge_update`) | {fused['fused'][0]:.3f} "
             f"({fused['fused'][1]:.3f} .. {fused['fused'][2]:.3f}) |", "",
             f"Unfused median / fused median: {fused['unfused'][0] / fused['fused'][0]:.3f}. Condition 1 (the fused "
             f"median below the unfused minimum): {'met' if ok_model else 'NOT met'}. Condition 2 (`edge_update` "
             f"faster than its torch concatenation form, table below): {'met' if ok_op else 'NOT met'} "
             f"({edge_t['fused'][0]:.3f} ms against {edge_t['torch'][0]:.3f} ms; the model's own unfused form of the "
             f"block, `gather_pair` + concatenation + `mlp_edge`: {edge_t['unfused'][0]:.3f} "
             f"({edge_t['unfused'][1]:.3f} .. {edge_t['unfused'][2]:.3f}) ms).", "",
             "## Operators alone, forward + backward", "",
             "| operator | HIP ms | torch ms | torch / HIP | bytes (MB) | bytes / HIP time (TB/s) | share of 6.3 TB/s |",
             "|---|---|---|---|---|---|---|"]
    for name, h, t, nbytes, _, _ in ops:
        rate = nbytes / (h[0] * 1e-3) / 1e12
        lines.append(f"| {name} | {h[0]:.3f} ({h[1]:.3f} .. {h[2]:.3f}) | {t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f}) | "
                     f"{t[0] / h[0]:.2f} | {nbytes / 1e6:.1f} | {rate:.2f} | {100 * rate / HBM_TBS:.0f}% |")
    lines += ["", "The HIP time of an operator includes the autograd call, its output allocations and two kernel "
              "launches (three for gather_pair with its two index_select gathers); the byte count is what the "
              "kernels must move (rows, indices, outputs), so the last column is a whole-call rate, not a kernel's "
              "share of peak."]
    lines += ["", "## The HIP kernels alone", "",
              "The library's event profiler around each launch (`pemp_prof_enable`; the event records' overhead is "
              "inside the figure), against the bytes the kernel must move at the achievable HBM rate "
              f"({HBM_TBS} TB/s).", "",
              "| operator | kernel | us | bytes (MB) | bytes at the HBM rate (us) | time / that | TB/s |", "|---|---|---|---|---|---|---|"]
    for name, _, _, _, kus, kbytes in ops:
        for label, nb in kbytes.items():
            if label in kus:
                floor_us = nb / (HBM_TBS * 1e12) * 1e6
                lines.append(f"| {name} | {label} | {kus[label]:.1f} | {nb / 1e6:.1f} | {floor_us:.1f} | "
                             f"{kus[label] / floor_us:.1f}x | {nb / (kus[label] * 1e-6) / 1e12:.2f} |")
    slower = [f"{name} (torch / HIP {t[0] / h[0]:.2f}: its kernels take {sum(kus.values()):.0f} us of the "
              f"{h[0] * 1e3:.0f} us call, the rest is the host side of the autograd Function, two library calls and "
              f"the output allocations, against a single torch op each way)"
              for name, h, t, _, kus, _ in ops if t[0] <= h[0]]
    lines += ["", "Acceptance (each operator faster than its torch form at this shape): " +
              ("met for every operator." if not slower else "NOT met for " + ", ".join(slower) + ".")]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
