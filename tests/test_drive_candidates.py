"""utils.arc_candidates, the table of pull_base_command(): against the closed form in fp64, against a midpoint integration of the
unicycle, at w = 0, |w| = 1e-9 and v < 0, with a footprint, and at the entry's limits.  CPU only."""
import numpy as np
import pytest
import torch

from stretch_mujoco_amd.utils import BaseCandidates, arc_candidates, unicycle_pose

F32 = 2.0 ** -24      # half an ulp of a value below 1: what storing a coordinate < 1 m as fp32 may change


def _integrate(v, w, t, steps=10_000):
    """Midpoint rule on x' = v cos(th), y' = v sin(th), th' = w.  For constant (v, w) a step of the rule is a chord at the mid heading:
    its error per step is v h (w h)^2 / 24, in all v t (w t)^2 / (24 steps^2) < 1e-8 m here."""
    x = y = th = 0.0
    h = t / steps
    for _ in range(steps):
        mid = th + 0.5 * h * w
        x += h * v * np.cos(mid)
        y += h * v * np.sin(mid)
        th += h * w
    return x, y, th


def test_default_set():
    c = arc_candidates(device="cpu")
    assert isinstance(c, BaseCandidates) and c.bias is None
    assert tuple(c.command.shape) == (35, 2) and tuple(c.points.shape) == (35, 13, 2) and c.command.dtype == c.points.dtype == torch.float32
    cmd = c.command.numpy()
    assert sorted(set(np.round(cmd[:, 0].astype(np.float64), 6))) == [0.0, 0.08, 0.16, 0.25]
    assert sorted(set(cmd[:, 1].tolist())) == np.linspace(-1, 1, 9).tolist() and not ((cmd[:, 0] == 0) & (cmd[:, 1] == 0)).any()
    assert len({tuple(r) for r in cmd.tolist()}) == 35 and (np.diff(cmd[:, 0]) <= 0).all()      # the fastest first
    turn = c.points.numpy()[(cmd[:, 0] == 0)]
    assert (turn[:, :12] == 0).all() and np.allclose(np.hypot(turn[:, 12, 0], turn[:, 12, 1]), 0.3)      # turning in place sweeps the own cell only


def test_against_the_closed_form_and_the_integration():
    v = np.array([0.25, 0.25, 0.16, -0.2, 0.08, 0.25, 0.3, 0.25, 0.25])
    w = np.array([1.0, -0.7, 0.3, 0.5, -1.0, 0.0, 1e-9, -1e-9, 2.0])
    H, N, LA = 1.5, 12, 0.3
    c = arc_candidates(v, w, horizon=H, samples=N, lookahead=LA, device="cpu")
    pts = c.points.numpy().astype(np.float64)
    assert pts.shape == (9, N + 1, 2) and np.array_equal(c.command.numpy(), np.stack((v, w), 1).astype(np.float32))
    for k in range(9):
        for i in range(N):
            t = H * (i + 1) / N
            x, y, th = unicycle_pose(v[k], w[k], t)
            if abs(w[k]) > 1e-6:      # the closed form as it is usually written
                assert abs(x - v[k] / w[k] * np.sin(w[k] * t)) < 1e-15 and abs(y - v[k] / w[k] * (1 - np.cos(w[k] * t))) < 1e-15 and th == w[k] * t
            else:                     # the limit: a straight line, bent by v w t^2 / 2
                assert abs(x - v[k] * t) < 1e-15 and abs(y - 0.5 * v[k] * w[k] * t * t) < 1e-15
            assert abs(pts[k, i, 0] - x) <= F32 and abs(pts[k, i, 1] - y) <= F32
            if i in (0, N // 2, N - 1):
                ix, iy, ith = _integrate(v[k], w[k], t)
                assert np.hypot(ix - x, iy - y) < 1e-6 and abs(ith - th) < 1e-9, (k, i)
        x, y, th = unicycle_pose(v[k], w[k], H)
        assert abs(pts[k, N, 0] - (x + LA * np.cos(th))) <= F32 and abs(pts[k, N, 1] - (y + LA * np.sin(th))) <= F32
    assert (pts[5, :, 1] == 0).all() and np.allclose(pts[5, :N, 0], 0.25 * H * (np.arange(N) + 1) / N, atol=F32)      # w = 0: straight ahead
    assert np.abs(pts[6] - arc_candidates([0.3], [0.0], device="cpu").points.numpy()[0]).max() < 1e-9 and np.isfinite(pts).all()      # no blow-up at 1e-9
    assert (pts[3, :N, 0] < 0).all() and (pts[3, :N, 1] < 0).all()      # backwards while turning left: behind and to the right
    big = unicycle_pose(1.0, np.array([1e-300, -1e-12, 1e-5]), 2.0)
    assert np.isfinite(big[0]).all() and np.allclose(big[0], 2.0, atol=1e-9) and np.allclose(big[1], [0, -2e-12, 2e-5], atol=1e-12)


def test_footprint_points():
    fp = [(0.17, 0.17), (0.17, -0.17), (-0.17, 0.0)]
    v, w = np.array([0.25, 0.1]), np.array([0.5, -1.0])
    c = arc_candidates(v, w, horizon=2.0, samples=4, lookahead=0.2, footprint=fp, device="cpu")
    pts = c.points.numpy().astype(np.float64)
    assert pts.shape == (2, 4 * 3 + 1, 2)
    for k in range(2):
        for i in range(4):
            x, y, th = unicycle_pose(v[k], w[k], 2.0 * (i + 1) / 4)
            for j, (fx, fy) in enumerate(fp):
                want = (x + np.cos(th) * fx - np.sin(th) * fy, y + np.sin(th) * fx + np.cos(th) * fy)
                assert np.abs(pts[k, 3 * i + j] - want).max() <= F32
        x, y, th = unicycle_pose(v[k], w[k], 2.0)
        assert np.abs(pts[k, 12] - (x + 0.2 * np.cos(th), y + 0.2 * np.sin(th))).max() <= F32
    one = arc_candidates(v, w, horizon=2.0, samples=4, lookahead=0.2, footprint=[(0.0, 0.0)], device="cpu")
    assert torch.equal(one.points, arc_candidates(v, w, horizon=2.0, samples=4, lookahead=0.2, device="cpu").points)


def test_bias_and_limits():
    c = arc_candidates([0.1, 0.2], [0.0, 0.0], bias=[5, -3], device="cpu")
    assert c.bias.dtype == torch.int32 and c.bias.tolist() == [5, -3]
    t = arc_candidates([0.1, 0.0, 0.0], [0.0, 0.5, -0.5], bias=[5, -3, 0], turn_bias=1500, device="cpu")
    assert t.bias.tolist() == [5, 1497, 1500] and arc_candidates(turn_bias=7, device="cpu").bias.tolist() == [0] * 27 + [7] * 8
    ok = arc_candidates(np.full(1024, 0.1), np.linspace(-1, 1, 1024), samples=31, device="cpu")      # K P = 32768 exactly
    assert tuple(ok.points.shape) == (1024, 32, 2)
    assert tuple(arc_candidates([0.1], [0.0], samples=255, device="cpu").points.shape) == (1, 256, 2)
    assert tuple(arc_candidates([0.1], [0.0], samples=51, footprint=[(0.1, 0.0)] * 5, device="cpu").points.shape) == (1, 256, 2)
    for kw in (dict(v=np.full(1025, 0.1), w=np.zeros(1025), samples=1), dict(v=[0.1], w=[0.0], samples=256), dict(v=np.full(1024, 0.1), w=np.zeros(1024), samples=32),
               dict(v=np.full(129, 0.1), w=np.zeros(129), samples=255), dict(v=[0.1], w=[0.0], samples=52, footprint=[(0.1, 0.0)] * 5), dict(v=[0.1], w=None),
               dict(v=[0.1, 0.2], w=[0.0]), dict(v=[], w=[]), dict(v=[float("nan")], w=[0.0]), dict(v=[0.1], w=[0.0], samples=0), dict(v=[0.1], w=[0.0], horizon=0.0),
               dict(v=[0.1], w=[0.0], lookahead=float("inf")), dict(v=[0.1], w=[0.0], footprint=[(0.1,)]), dict(v=[0.1], w=[0.0], footprint=[]),
               dict(v=[0.1], w=[0.0], bias=[1, 2]), dict(v=[0.1], w=[0.0], bias=[0.5]), dict(v=[0.1], w=[0.0], bias=[1 << 31])):
        with pytest.raises(ValueError):
            arc_candidates(device="cpu", **kw)
