"""Generate ``tests/golden/train_*.npz``: one training forward + backward of the REFERENCE's MPN on the CPU.

Test infrastructure (needs the reference tree, see oracle/ref_shims.py, which is imported only when the tool runs).
    PYTHONDONTWRITEBYTECODE=1 python -B tools/gen_golden_train.py [name ...]
Per case: the reference's ``NodeClassificationMPNSimple`` is loaded through ``oracle.ref_shims.load_reference()``,
given ``synthetic.closed_form_state_dict`` weights (the salt of the source fixture), put in ``.train()`` and run on
the inputs stored in the source ``tests/golden/mpn_*.npz``, in fp64 and in fp32. The loss is
``tests/train_oracle.fixture_loss``. Stored: the fp64 logits and loss, the BatchNorm buffers after the forward, the
fp64 gradients (``train_oracle.pack``: in full for x, edge_attr and, while the byte budget lasts, the parameters of at
most 16,384 elements; L2 norm + closed-form probe for the others, ``meta`` lists the small ones among them: the 17
per-type message weights alone are 1.6 MB in fp64, above the size limit of a committed file) and, in ``meta``, the
reference's own fp32-vs-fp64 error per tensor.

The reference allocates its per-type message and aggregate buffers as ``torch.zeros(..., dtype=torch.float32)``
(layers.py:236, 244, 270), which would round an fp64 run to fp32 at those points; for the fp64 run the layers
module sees a ``torch`` whose ``zeros`` follows the run's dtype. Nothing else of the reference is altered.

Before a fixture is written, ``tests/train_oracle`` in fp64 must agree with the reference in fp64 within
``1e-9 * max|.|`` per tensor (the two differ only in operation order); the analytically zero gradient of
``attn_net.0.bias`` within twice ``train_oracle.residue_bound`` at fp64's roundoff.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

OUT = os.path.join(ROOT, "tests", "golden")
CASES = ["mpn_attn_t3", "mpn_attn_pertype_t2", "mpn_attn_j14", "mpn_attn_lr_t3", "mpn_pertype_sum_t2",
         "mpn_pertype_max_t2", "mpn_max_t3", "mpn_mean_t2", "mpn_add_t2"]
BUDGET = 900_000          # bytes of arrays stored in full per fixture (a committed file stays below 1 MiB)
AGREE = 1e-9


class _TorchWithDtype:
    """``torch`` as the reference's layers module sees it in a non-fp32 run: zeros(dtype=float32) -> the run's dtype."""

    def __init__(self, dtype):
        self._dtype = dtype

    def __getattr__(self, name):
        return getattr(torch, name)

    def zeros(self, *args, **kwargs):
        if kwargs.get("dtype") is torch.float32:
            kwargs["dtype"] = self._dtype
        return torch.zeros(*args, **kwargs)


def run_reference(MPN, layers, cfg, meta, arrays, dtype):
    from pemp_amd import synthetic as syn
    from tests import train_oracle as to
    torch.manual_seed(0)
    model = MPN(cfg)
    model.load_state_dict(syn.closed_form_state_dict(model, meta["salt"], meta.get("attn_gain", 1.0),
                                                     meta.get("weight_gain", 1.0)))
    model.to(dtype).train()
    x = torch.from_numpy(arrays["x"]).to(dtype).requires_grad_(True)
    ea = torch.from_numpy(arrays["edge_attr"]).to(dtype).requires_grad_(True)
    saved = layers.torch
    layers.torch = _TorchWithDtype(dtype)
    try:
        pe, pn, pc, _ = model(x, ea, torch.from_numpy(arrays["edge_index"]),
                              node_types=torch.from_numpy(arrays["node_types"]))
        loss = to.fixture_loss(pe, pn, pc)
        loss.backward()
    finally:
        layers.torch = saved
    stats = {k: v for k, v in model.state_dict().items()
             if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    grads = {"x": x.grad, "edge_attr": ea.grad}
    grads.update({k: p.grad for k, p in model.named_parameters()})
    return to.collect(pe, pn, pc, loss, stats, grads), model


def rel_err(a, b, scale):
    """max|a - b| over `scale` (train_oracle.scale_of: max|b|)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(scale, 1e-300)) if b.size else 0.0


def main(only=()):
    from oracle.ref_shims import load_reference          # lazily: importing this tool needs no reference tree
    from pemp_amd import synthetic as syn
    from tests import golden_util as gu, train_oracle as to
    _, MPN, layers = load_reference()
    for src in CASES:
        if only and src not in only:
            continue
        meta, arrays = gu.load(src)
        cfg = gu.mpn_config(meta)
        ref64, model = run_reference(MPN, layers, cfg, meta, arrays, torch.float64)
        ref32, _ = run_reference(MPN, layers, cfg, meta, arrays, torch.float32)
        sd = syn.closed_form_state_dict(MPN(cfg), meta["salt"], meta.get("attn_gain", 1.0), meta.get("weight_gain", 1.0))
        mine = to.step(sd, cfg, arrays["x"], arrays["edge_attr"], arrays["edge_index"], arrays["node_types"])
        worst = 0.0
        for k, v in ref64.items():
            if k.endswith("num_batches_tracked"):
                assert np.array_equal(v, mine[k]), (src, k)
                continue
            got = mine.get(k)
            assert got is not None, (src, k, "missing in the restatement")
            if k == to.ATTN_BIAS:          # analytically zero: an absolute bound from its terms, not 1e-9 of itself
                assert np.abs(got - v).max() <= 2 * to.residue_bound(mine, 2.0 ** -53), (src, k)
                continue
            err = rel_err(got, v, to.scale_of(ref64, k))
            worst = max(worst, err)
            assert err <= AGREE, (src, k, err)
        for k in mine:     # a gradient the restatement has and the reference leaves at None must be zero
            assert k in ref64 or k.startswith("aux.") or not np.any(mine[k]), (src, k)
        ref_fp32_err = {k: rel_err(ref32[k], v, to.scale_of(ref64, k)) for k, v in ref64.items()
                        if k in ref32 and not k.endswith("num_batches_tracked") and k != to.ATTN_BIAS}
        packed = to.pack(ref64, BUDGET)
        out_meta = dict(meta, source=src, oracle_vs_reference=worst, reference_fp32_rel_err=ref_fp32_err,
                        full_gradients=sorted(k[5:] for k in packed if k.startswith("grad.")),
                        demoted_small_gradients=sorted(k[6:] for k in packed if k.startswith("gnorm.")
                                                       and ref64["grad." + k[6:]].size <= to.FULL_GRAD_LIMIT))
        name = "train_" + src[4:]
        path = os.path.join(OUT, f"{name}.npz")
        np.savez_compressed(path, meta=json.dumps(out_meta), **packed)
        print(f"{name}: N={meta['N']} E={meta['E']} oracle_vs_reference={worst:.2e} "
              f"ref_fp32_err(max)={max(ref_fp32_err.values()):.2e} bytes={os.path.getsize(path)}")
        assert os.path.getsize(path) < 1_000_000, path


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
