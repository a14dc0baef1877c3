"""GPU tests of the fused edge update of the training mode (mpn/train.py edge_update / gather_dst,
csrc/train_edge.hip): the operator against the torch concatenation form in fp64, one training step of every model
case of tests/test_gpu_train.py with model.fused_edge_update = True, bitwise reproducibility, the peak memory of a
step, and that a model with the attribute off (and the eval path) did not move.

Error bound per tensor, as tests/test_gpu_train.py: 4 * max|torch form fp32 - fp64| + 2^-22 * max|fp64|
(test_gpu_train.bound_ratio); the operator's fp32 yardstick is the torch form on the CPU, as for the other
operators. Each test prints its largest error / bound ratio (DESIGN 7e records them).

No test here feeds node ids outside [0, N): build_plan refuses them, and that the kernels never follow such an id is
a property of their code (the ids are compared with N before any row address is formed), not something to provoke."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from pemp_amd.mpn import train as tr
from tests import test_gpu_train as tg, train_oracle as to

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_OPS = 41
MARGIN = 1e-4     # |pre-activation| of every kept edge: far above fp32's error (~1e-6), so no ReLU mask depends on
                  # the number format and the fp32 yardstick, the fp64 one and the kernel differentiate one function
OP_CASES = [(E, W) for W in (64, 128) for E in (1, 63, 64, 65, 255, 256, 257, 3000)] + [(40_003, 128), (140_001, 64)]
NAMES = ("e_new", "grad_nf", "grad_ef", "grad_W1", "grad_b1", "grad_W2", "grad_b2")


@functools.lru_cache(maxsize=None)
def op_case(E, W):
    """A random multigraph on N = 41 nodes with E edges (node 10 has no incoming edge, node 11 no outgoing one), node
    and edge rows of W floats and the weights of mlp_edge. The biases put about a third of both pre-activations
    below zero; candidate edges with a pre-activation within MARGIN of zero (about 1 in 100) are not kept, so none
    is exactly zero in any precision."""
    g = torch.Generator().manual_seed(1000 * W + E)
    N, K = N_OPS, 3 * W
    nf = torch.randn(N, W, generator=g, dtype=torch.float64)
    W1 = torch.randn(64, K, generator=g, dtype=torch.float64) / K ** 0.5
    b1 = 0.43 + 0.1 * torch.randn(64, generator=g, dtype=torch.float64)
    W2 = torch.randn(64, 64, generator=g, dtype=torch.float64) / 8.0
    b2 = 0.42 + 0.1 * torch.randn(64, generator=g, dtype=torch.float64)
    M = E + E // 8 + 16                                          # candidates
    src = torch.tensor([n for n in range(N) if n != 11])[torch.randint(0, N - 1, (M,), generator=g)]
    dst = torch.tensor([n for n in range(N) if n != 10])[torch.randint(0, N - 1, (M,), generator=g)]
    ef = torch.randn(M, W, generator=g, dtype=torch.float64)
    # the masks are decided on the values the fp32 runs see
    f32 = [t.float().double() for t in (nf, ef, W1, b1, W2, b2)]
    z1 = F.linear(torch.cat([f32[0][dst], f32[0][src], f32[1]], 1), f32[2], f32[3])
    z2 = F.linear(torch.relu(z1), f32[4], f32[5])
    keep = ((z1.abs().min(1).values > MARGIN) & (z2.abs().min(1).values > MARGIN)).nonzero().reshape(-1)[:E]
    assert len(keep) == E
    src, dst, ef, z1, z2 = src[keep], dst[keep], ef[keep], z1[keep], z2[keep]
    assert not (dst == 10).any() and not (src == 11).any()
    if E >= 255:
        assert 0.25 < float((z1 < 0).double().mean()) < 0.42 and 0.25 < float((z2 < 0).double().mean()) < 0.42
    w_out = torch.randn(E, 64, generator=g, dtype=torch.float64)
    return dict(N=N, E=E, W=W, ei=torch.stack([src, dst]), nf=nf.float(), ef=ef.float(), W1=W1.float(), b1=b1.float(),
                W2=W2.float(), b2=b2.float(), w_out=w_out.float())


def cat_form(G, dtype):
    """The torch form of the block (mpn/train.py _layer, layers.py:207-258) on the CPU."""
    nf, ef, W1, b1, W2, b2 = (G[k].clone().to(dtype).requires_grad_(True) for k in ("nf", "ef", "W1", "b1", "W2", "b2"))
    src, dst = G["ei"][0], G["ei"][1]
    h = torch.relu(F.linear(torch.cat([nf[dst], nf[src], ef], dim=1), W1, b1))
    e_new = torch.relu(F.linear(h, W2, b2))
    (e_new * G["w_out"].to(dtype)).sum().backward()
    return [e_new.detach(), nf.grad, ef.grad, W1.grad, b1.grad, W2.grad, b2.grad]


def mlp_of(G, W):
    mlp = nn.Sequential(nn.Linear(3 * W, 64), nn.ReLU(inplace=True), nn.Linear(64, 64), nn.ReLU(inplace=True))
    with torch.no_grad():
        for p, k in zip(mlp.parameters(), ("W1", "b1", "W2", "b2")):
            p.copy_(G[k])
    return mlp.to(DEV)


def device_form(G):
    W = G["W"]
    plan = tr.build_plan(G["ei"].to(DEV), torch.zeros(G["N"], dtype=torch.int64, device=DEV), G["N"], 1)
    mlp = mlp_of(G, W)
    nf, ef = G["nf"].to(DEV).requires_grad_(True), G["ef"].to(DEV).requires_grad_(True)
    e_new = tr.edge_update(nf, ef, plan, mlp)
    (e_new * G["w_out"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return [t.detach().cpu() for t in [e_new, nf.grad, ef.grad] + [p.grad for p in mlp.parameters()]]


@pytest.mark.parametrize("E,W", OP_CASES)
def test_edge_update_against_fp64(E, W):
    """E = 1 .. 257 around the 64-edge tile and the 256-edge chunk of the weight-gradient sums; E = 3000 with twelve
    partials; E = 40,003 (We = 128): 626 tiles over the persistent workgroups, 157 partials (two tree passes, the
    second over 5 of its 32 leaves) and a last tile of 3 edges; E = 140,001 (We = 64): 547 partials, more than the
    backward's 2 x 256 persistent workgroups, so some of them take a second chunk."""
    G = op_case(E, W)
    got = device_form(G)
    o32, o64 = cat_form(G, torch.float32), cat_form(G, torch.float64)
    ratios = {}
    for name, a, b, c in zip(NAMES, got, o32, o64):
        assert a.shape == c.shape and a.dtype == torch.float32, name
        ratios[name] = tg.bound_ratio(a, b, c)
    print(f"edge_update E={E} We={W} error/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


def test_gather_dst_and_input_checks():
    G = op_case(3000, 128)
    N, E = G["N"], G["E"]
    plan = tr.build_plan(G["ei"].to(DEV), torch.zeros(N, dtype=torch.int64, device=DEV), N, 1)
    w = torch.randn(E, 128, generator=torch.Generator().manual_seed(1))
    res = {}
    for dtype in (torch.float32, torch.float64):
        x = G["nf"].clone().to(dtype).requires_grad_(True)
        xi = x[G["ei"][1]]
        (xi * w.to(dtype)).sum().backward()
        res[dtype] = (xi.detach(), x.grad)
    xd = G["nf"].to(DEV).requires_grad_(True)
    xi = tr.gather_dst(xd, plan)
    (xi * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(xi.detach().cpu(), res[torch.float32][0])
    ratio = tg.bound_ratio(xd.grad.cpu(), res[torch.float32][1], res[torch.float64][1])
    print(f"gather_dst W=128 error/bound: grad_x {ratio:.3f}")
    assert ratio <= 1.0 and not xd.grad[10].any()                # node 10 is no target
    mlp = mlp_of(G, 128)
    nf, ef = G["nf"].to(DEV), G["ef"].to(DEV)
    with pytest.raises(RuntimeError):
        tr.edge_update(G["nf"], ef, plan, mlp)                   # CPU rows
    with pytest.raises(RuntimeError):
        tr.edge_update(nf, G["ef"], plan, mlp)
    with pytest.raises(TypeError):
        tr.edge_update(nf.double(), ef, plan, mlp)
    with pytest.raises(TypeError):
        tr.edge_update(nf, ef.half(), plan, mlp)
    with pytest.raises(ValueError):
        tr.edge_update(nf, ef[:, :64].contiguous(), plan, mlp)   # mlp_edge does not fit the rows
    with pytest.raises(ValueError):
        tr.edge_update(nf, ef[:-1].contiguous(), plan, mlp)      # E of the plan
    with pytest.raises(ValueError):
        tr.edge_update(nf[:-1].contiguous(), ef, plan, mlp)      # N of the plan
    with pytest.raises(TypeError):
        tr.gather_dst(nf.half(), plan)
    with pytest.raises(RuntimeError):
        tr.gather_dst(G["nf"], plan)
    # no edge: empty rows forward, zero gradients backward
    plan0 = tr.build_plan(torch.zeros(2, 0, dtype=torch.int64, device=DEV), torch.zeros(N, dtype=torch.int64, device=DEV), N, 1)
    nf0 = nf.clone().requires_grad_(True)
    out = tr.edge_update(nf0, torch.zeros(0, 128, device=DEV), plan0, mlp)
    assert out.shape == (0, 64)
    mlp.zero_grad(set_to_none=True)
    (out.sum() + tr.gather_dst(nf0, plan0).sum()).backward()
    torch.cuda.synchronize()
    assert not nf0.grad.any() and all(p.grad is not None and not p.grad.any() for p in mlp.parameters())


# ---- model -----------------------------------------------------------------------------------------------------
def fused_model(cfg, meta):
    model, sd = tg.fresh_model(cfg, meta)
    model.to(DEV).train()
    model.fused_edge_update = True
    return model, sd


@functools.lru_cache(maxsize=None)
def cpu_step(name):
    """The torch-operator form of the step in fp32 on the CPU, on one thread: the same number on every run."""
    meta, a, cfg = tg.case_inputs(name)
    _, sd = tg.fresh_model(cfg, meta)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return to.step(sd, cfg, a["x"], a["edge_attr"], a["edge_index"], a["node_types"], dtype=torch.float32, device="cpu")
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("name", tg.MODEL_CASES)
def test_fused_model_step_against_fp64(name, monkeypatch):
    """test_gpu_train.test_model_step_against_fp64 with model.fused_edge_update = True: the same bound per tensor and
    the same special cases (ORDER_DEPENDENT, attn_net.0.bias); tr.edge_update must have run once per layer iteration.

    The fp32 yardstick of every logit, statistic and gradient is that test's: the torch-operator form on this GPU.
    It runs on float atomics and differs from evaluation to evaluation, which two kinds of tensor cannot bear, so
    these also get a yardstick that is the same number on every run and does not pass through this library: the same
    torch form in fp32 on the CPU, on one thread (cpu_step; with more threads the CPU sums are split by the thread
    count; between two hosts' CPUs it moved by up to 1.5x).
    * `loss` is one fp32 number of cancelling terms (|loss| 1.5e-3 .. 3e-2 from terms of order one): any form is a few
      of the loss's own ulps from fp64, and 4 |o32 - o64| of the GPU yardstick moved 10x between eight draws
      (train_attn_lr_t3: 1.3e-09 .. 1.1e-08 against a fused error of 3.2e-09). Its bound is taken from the CPU form
      alone: 4 |cpu32 - o64| + 2^-22 |o64|. Fused error / that bound on the MI355X host: train_add_t2 0.19,
      train_attn_j14 0.09, train_attn_lr_t3 0.09, train_attn_pertype_t2 0.21, train_attn_t3 0.04, train_max_t3 0.04,
      train_mean_t2 0.00, train_pertype_max_t2 0.05, train_pertype_sum_t2 0.04, mpn_attn_c2_t3 0.02.
    * the two ORDER_DEPENDENT gradients keep that test's handling, the larger of the two GPU evaluations of the torch
      form, and the CPU form joins them as a third. With mpn_attn_c2_t3 the GPU evaluations land on 7.38e-08 / 4.56e-08
      (bias / weight) or on 3.2e-10 / 1.7e-09 depending on the draw, and this model lands on the larger pair in every
      run, fused or not; when both evaluations drew the smaller one the case read 33. The CPU form is 4.4e-06 / 3.2e-06
      from fp64 there: a loose yardstick for two sums whose rows cancel behind a BatchNorm, but a fixed one."""
    meta, a, cfg = tg.case_inputs(name)
    model, sd = fused_model(cfg, meta)
    keys = list(model.state_dict().keys())
    calls = []
    inner = tr.edge_update

    def counted(*args, **kw):
        calls.append(1)
        return inner(*args, **kw)
    monkeypatch.setattr(tr, "edge_update", counted)
    got, (pe, pn, pc) = tg.device_step(model, a)
    assert len(calls) == cfg.STEPS
    o64 = tg.oracle_step(name, torch.float64, "cpu")
    o32 = tg.oracle_step(name, torch.float32, "cuda:0")
    m32 = tg.module_form_step(cfg, meta, a, monkeypatch)          # (undoes the counter's patch too)
    c32 = cpu_step(name)
    assert list(model.state_dict().keys()) == keys == list(sd.keys())
    n_rec = sum(1 for i in range(cfg.STEPS) if i >= cfg.STEPS - cfg.AUX_LOSS_STEPS - 1)
    assert (len(pe), len(pn), len(pc)) == (n_rec, n_rec + 1, n_rec + 1)
    worst = ("", 0.0)
    for k, want in o64.items():
        if k.startswith("aux."):
            continue
        if k.endswith("num_batches_tracked"):
            assert np.array_equal(got[k], want), k
            continue
        have = got.get(k)
        if have is None:          # a parameter the forward never reaches: None here, zeros in the oracle
            assert k.startswith("grad.") and not np.any(want), k
            continue
        assert have.shape == want.shape, k
        err = float(np.abs(have - want).max()) if want.size else 0.0
        if k == to.ATTN_BIAS:
            bound = to.residue_bound(o64, 2.0 ** -24)
            print(f"fused model step {name}: |grad attn_net.0.bias| {err:.2e} (torch form {np.abs(o32[k]).max():.2e}, "
                  f"fp64 {np.abs(want).max():.2e}), residue bound {bound:.2e}")
        else:
            bound = to.error_bound(c32 if k == "loss" else o32, o64, k)
            if k in tg.ORDER_DEPENDENT:
                print(f"fused model step {name}: {k} error {err:.2e}; torch form {np.abs(o32[k] - want).max():.2e} "
                      f"(functional), {np.abs(m32[k] - want).max():.2e} (through the modules), "
                      f"{np.abs(c32[k] - want).max():.2e} (CPU, one thread)")
                bound = max(bound, to.error_bound(m32, o64, k), to.error_bound(c32, o64, k))
        r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        if k == "loss":
            print(f"fused model step {name}: loss error {err:.2e}, torch form on the CPU {np.abs(c32[k] - want).max():.2e} "
                  f"(on this GPU {np.abs(o32[k] - want).max():.2e}), floor {2.0 ** -22 * np.abs(want).max():.2e}: ratio {r:.3f}")
        if r > worst[1]:
            worst = (k, r)
    print(f"fused model step {name}: largest error/bound {worst[1]:.3f} ({worst[0]})")
    assert worst[1] <= 1.0, worst
    for k in got:
        assert k in o64, k


@pytest.mark.parametrize("name", ["train_attn_t3", "train_mean_t2"])
def test_fused_step_is_reproducible(name):
    meta, a, cfg = tg.case_inputs(name)
    model, _ = fused_model(cfg, meta)
    runs = [tg.device_step(model, a)[0] for _ in range(3)]
    for k, v in runs[0].items():
        if k.startswith(("logit.", "grad.", "loss")):
            assert all(np.array_equal(v, r[k]) for r in runs[1:]), k
    assert int(runs[2]["bn.node_embedding.2.num_batches_tracked"]) == 3


def test_fused_step_needs_less_memory():
    """The fused path keeps neither x[src] nor the [E, 384] concatenation alive until backward."""
    meta, a, cfg = tg.case_inputs("mpn_attn_c2_t3")
    model, _ = tg.fresh_model(cfg, meta)
    model.to(DEV).train()
    x = torch.from_numpy(a["x"]).to(DEV).requires_grad_(True)
    ea = torch.from_numpy(a["edge_attr"]).to(DEV).requires_grad_(True)
    peak = {}
    for fused in (False, True):
        model.fused_edge_update = fused
        for measured in (False, True):                            # the first step of a form warms its caches
            x.grad = ea.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(DEV)
            base = torch.cuda.memory_allocated(DEV)
            tg.device_step(model, a, x, ea)
            peak[fused] = torch.cuda.max_memory_allocated(DEV) - base
    E = a["edge_index"].shape[1]
    print(f"peak memory of one step above its start, E = {E}: unfused {peak[False] / 2**20:.1f} MiB, "
          f"fused {peak[True] / 2**20:.1f} MiB")
    assert torch.cuda.max_memory_allocated(DEV) > 0 and peak[True] < peak[False], peak


def test_attribute_off_and_eval_are_left_alone():
    """With the attribute False a step is bit-identical to one of an instance that never had the attribute. Eval
    never reads it: after a fused and after an unfused training step the eval logits agree bit for bit. (The two
    steps update the BatchNorm running statistics of the heads from rows that differ in their last bits, so the
    statistics are levelled by loading the unfused model's state_dict before the comparison; those the edge update
    does not feed are compared as they are.)"""
    meta, a, cfg = tg.case_inputs("train_attn_t3")
    plain, _ = tg.fresh_model(cfg, meta)
    plain.to(DEV).train()
    del plain.fused_edge_update
    assert not hasattr(plain, "fused_edge_update")
    off, _ = tg.fresh_model(cfg, meta)
    off.to(DEV).train()
    assert off.fused_edge_update is False
    r0, r1 = tg.device_step(plain, a)[0], tg.device_step(off, a)[0]
    assert set(r0) == set(r1)
    for k, v in r0.items():
        assert np.array_equal(v, r1[k]), k
    on, _ = fused_model(cfg, meta)
    r2 = tg.device_step(on, a)[0]
    assert any(not np.array_equal(r2[k], r1[k]) for k in r1 if k.startswith("grad."))   # the fused path did run
    for k in r1:
        if k.startswith(("bn.node_embedding", "bn.edge_embedding")):
            assert np.array_equal(r2[k], r1[k]), k
    on.load_state_dict(off.state_dict())
    ins = [torch.from_numpy(a[k]).to(DEV) for k in ("x", "edge_attr", "edge_index")]
    types = torch.from_numpy(a["node_types"]).to(DEV)
    outs = []
    for m in (off, on):
        m.eval()
        with torch.no_grad():
            outs.append(m(*ins, node_types=types))
    torch.cuda.synchronize()
    assert on.fused_edge_update is True
    for p, q in zip(outs[0][0] + outs[0][1] + outs[0][2], outs[1][0] + outs[1][1] + outs[1][2]):
        assert torch.equal(p, q)
