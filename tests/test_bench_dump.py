"""bench.py --dump-outputs on the CPU: file names, dtypes (integer slots as float64), the [n, envs] layout, the total-size budget with
the .npy headers counted, and the seeded sample of the envs (env_index) when the full state would not fit.  A stand-in simulator
carries the slots dump_outputs reads; no GPU, no libsmj.so."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

ROWS = {"qpos": 27, "qvel": 26, "qacc_warmstart": 26, "actuator_length": 10, "actuator_velocity": 10, "base_pose": 3, "xpose": 240, "info": 4}


def _sim(B):
    g = torch.Generator().manual_seed(7)
    s = types.SimpleNamespace(device=torch.device("cpu"))
    for k, n in ROWS.items():
        setattr(s, k, torch.randint(-3, 1 << 20, (n, B), generator=g, dtype=torch.int32) if k == "info" else torch.randn(n, B, generator=g))
    s.nstep = torch.full((B,), 625, dtype=torch.int32)
    return s, torch.randn(B, generator=g)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_writes_every_slot_in_its_layout_and_dtype(tmp_path):
    B = 64
    sim, ret = _sim(B)
    bench.dump_outputs(str(tmp_path), sim, ret)
    out = _load(str(tmp_path))
    assert set(out) == set(ROWS) | {"nstep", "returns"}
    for k, n in ROWS.items():
        assert out[k].shape == (n, B), k
        assert out[k].dtype == (np.float64 if k == "info" else np.float32), k
        np.testing.assert_array_equal(out[k], getattr(sim, k).numpy())   # integers exactly, floats bit for bit
    assert out["nstep"].dtype == np.float64 and out["nstep"].shape == (B,) and (out["nstep"] == 625).all()
    np.testing.assert_array_equal(out["returns"], ret.numpy())


def test_dump_over_the_budget_is_a_fixed_seeded_sample_within_it(tmp_path, monkeypatch):
    B = 4096
    sim, ret = _sim(B)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1_000_000)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), sim, ret)
    bench.dump_outputs(str(b), sim, ret)
    assert _size(str(a)) <= 1_000_000
    oa, ob = _load(str(a)), _load(str(b))
    keep = oa["env_index"].astype(np.int64)
    assert oa["env_index"].dtype == np.float64 and 0 < len(keep) < B
    assert (np.diff(keep) > 0).all() and keep[0] >= 0 and keep[-1] < B
    np.testing.assert_array_equal(keep, ob["env_index"])                # the same sample every run
    for k, n in ROWS.items():
        assert oa[k].shape == (n, len(keep)), k
        np.testing.assert_array_equal(oa[k], getattr(sim, k).numpy()[:, keep])
    np.testing.assert_array_equal(oa["returns"], ret.numpy()[keep])


def test_default_budget_holds_with_headers_at_a_large_batch(tmp_path):
    B = 60000   # ~1.35 kB per env: the full state would be ~81 MB
    sim, ret = _sim(B)
    bench.dump_outputs(str(tmp_path), sim, ret)
    assert "env_index" in _load(str(tmp_path)) and _size(str(tmp_path)) <= 64 * 10**6
