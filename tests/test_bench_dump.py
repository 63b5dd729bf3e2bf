"""bench.py --dump-outputs and --full without a GPU: the dumped sample is a fixed function of the batch's descriptors,
the files hold exactly the sampled windows' slices of x / y (float64, within the byte budget), and a line built
without the copy-ceiling measurement (a plain run) keeps the roofline's other figures."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from dervet_hip.packed import PackedBatch  # noqa: E402


def _batch(count=37, seed=5):
    rng = np.random.default_rng(seed)
    n = rng.integers(3, 40, count)
    m = rng.integers(1, 30, count)
    desc = np.zeros((count, 8), np.int64)
    desc[:, 0], desc[:, 1] = n, m
    desc[:, 6], desc[:, 7] = np.cumsum(n) - n, np.cumsum(m) - m
    x, y = rng.standard_normal(int(n.sum())), rng.standard_normal(int(m.sum()))
    z = torch.zeros(0)
    dev = PackedBatch(desc=desc, indptr=z, indices=z, data=z, c=z, c0=z, q=z, l=z, u=z,
                      x=torch.as_tensor(x), y=torch.as_tensor(y))
    stats = rng.standard_normal((count, 4))
    istats = rng.integers(0, 5000, (count, 2)).astype(np.int32)
    return desc, dev, x, y, stats, istats


def test_segments():
    off, n = np.array([10, 0, 4], np.int64), np.array([2, 3, 1], np.int64)
    assert bench._segments(off, n).tolist() == [10, 11, 0, 1, 2, 4]


def test_sample_is_fixed_sorted_and_within_budget():
    desc = _batch()[0]
    a, b = bench.dump_sample(desc), bench.dump_sample(desc.copy())
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0)
    assert len(a) == len(desc)  # (the whole batch fits the default budget)
    budget = 8 * 300
    s = bench.dump_sample(desc, budget=budget)
    assert 0 < len(s) < len(desc) and 8 * int((desc[s, 0] + desc[s, 1]).sum()) <= budget
    assert len(bench.dump_sample(desc, budget=0)) == 1  # never empty


def test_dump_outputs_writes_the_sampled_slices(tmp_path):
    desc, dev, x, y, stats, istats = _batch()
    out = str(tmp_path / "dump")
    gathered = torch.arange(len(desc) * 5, dtype=torch.float64).reshape(len(desc), 5)
    bench.dump_outputs(out, dev, desc, stats, istats, gathered, budget=8 * 400)
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["gathered_sample", "istats", "sample_windows", "stats", "x_sample", "y_sample"]
    assert all(a.dtype == np.float64 for a in got.values())
    win = got["sample_windows"].astype(np.int64)
    assert np.array_equal(win, bench.dump_sample(desc, 8 * 400)) and 0 < len(win) < len(desc)
    assert np.array_equal(got["stats"], stats) and np.array_equal(got["istats"], istats.astype(np.float64))
    assert np.array_equal(got["x_sample"], np.concatenate([x[desc[k, 6]:desc[k, 6] + desc[k, 0]] for k in win]))
    assert np.array_equal(got["y_sample"], np.concatenate([y[desc[k, 7]:desc[k, 7] + desc[k, 1]] for k in win]))
    assert np.array_equal(got["gathered_sample"], gathered.numpy()[win])
    assert sum(a.nbytes for a in got.values()) <= 64e6
    # the same batch again: the same files
    bench.dump_outputs(out, dev, desc, stats, istats, budget=8 * 400)
    assert np.array_equal(np.load(os.path.join(out, "x_sample.npy")), got["x_sample"])


def test_roofline_without_the_copy_ceiling():
    prof = {"pdhg_traffic": {"hbm_bytes_per_step": 4.0e10},
            "pdhg_valu": {"counters_per_step": {"SQ_INSTS_VALU_FMA_F64": 1e9, "SQ_INSTS_VALU": 4e9}}}
    plain = bench.roofline_object(1e12, 0.4, prof, "k", 2, None)
    full = bench.roofline_object(1e12, 0.4, prof, "k", 2, 5000.0)
    assert plain["hbm"]["stream_copy"] is None and plain["hbm"]["frac_of_stream_copy"] is None
    assert full["hbm"]["stream_copy"] == 5000.0 and full["hbm"]["frac_of_stream_copy"] == round(100.0 / 5000.0, 5)
    for k in ("achieved", "frac", "traffic", "issue", "effective"):
        assert plain[k] == full[k]
    assert plain["hbm"]["achieved"] == full["hbm"]["achieved"] == 100.0
