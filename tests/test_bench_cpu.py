"""bench.py's command line and --dump-outputs writer, CPU side (no step runs here)."""
import os
import sys

import numpy as np
import pytest
import torch

import bench


def _step(N=7, E=30):
    """A step's results shaped as run_steps returns them: construct_graph's 15-tuple and the MPN's three lists."""
    g = torch.Generator().manual_seed(3)
    out = [None] * 15
    out[0] = torch.rand(N, 128, generator=g)
    out[1] = torch.rand(E, 8, generator=g)
    out[2] = torch.randint(0, N, (2, E), generator=g)
    out[7] = torch.randint(0, 640, (N, 3), generator=g)
    out[11] = torch.rand(N, generator=g)
    out[12] = torch.zeros(N, dtype=torch.int64)
    out[14] = torch.rand(N, 1, generator=g)
    pe, pn, pc = [torch.rand(E, generator=g)], [torch.rand(N, generator=g)] * 2, [torch.rand(N, 17, generator=g)] * 2
    return tuple(out), pe, pn, pc


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_every_returned_tensor(tmp_path):
    last = _step()
    bench.dump_outputs(str(tmp_path / "d"), last, 0)
    got = _load(tmp_path / "d")
    assert sorted(got) == sorted(["x", "edge_attr", "edge_index", "joint_det", "joint_scores", "batch_index",
                                  "joint_tags", "edge_logits_0", "node_logits_0", "node_logits_1", "class_logits_0",
                                  "class_logits_1"])
    out, pe, pn, pc = last
    for name, t in (("x", out[0]), ("edge_attr", out[1]), ("edge_index", out[2]), ("joint_det", out[7]),
                    ("batch_index", out[12]), ("edge_logits_0", pe[0]), ("class_logits_1", pc[1])):
        a = got[name]
        assert a.dtype == (np.float32 if t.dtype == torch.float32 else np.float64), name
        assert a.shape == tuple(t.shape) and np.array_equal(a, t.numpy().astype(a.dtype)), name


def test_dump_outputs_rank_directory(tmp_path):
    bench.dump_outputs(str(tmp_path), _step(), 1)
    assert "x.npy" in os.listdir(tmp_path / "rank1")


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    """Over the budget: small arrays stay whole, the large ones become the same seeded sample in every run, and the
    payload stays within the budget."""
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4096)
    last = _step()
    bench.dump_outputs(str(tmp_path / "a"), last, 0)
    bench.dump_outputs(str(tmp_path / "b"), last, 0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(v.nbytes for v in a.values()) <= 4096
    assert all(np.array_equal(a[k], b[k]) for k in a) and sorted(a) == sorted(b)
    assert a["joint_scores"].shape == (7,) and np.array_equal(a["joint_scores"], last[0][11].numpy())
    x = last[0][0].numpy().reshape(-1)
    assert a["x"].ndim == 1 and 0 < a["x"].size < x.size and np.isin(a["x"], x).all()


def test_command_line(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    args = bench.parse()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (5, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "somewhere"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
