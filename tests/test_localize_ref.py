"""The numpy reference of smj_scan_to_particles (tests/localize_ref.py) on the CPU: the properties of its exact stage (thresholds,
ancestors, copies, the extremes of the draw, one particle, the largest total), its weights against a long-hand loop, the cap on
unsure (particle, point) pairs for the float-stage cases the GPU tests use, and the closed loop -- a robot found from a spread of
+-1 m and +-30 degrees that the scan matcher alone cannot bridge."""
import functools

import numpy as np
import pytest

import localize_ref as ref
import scanmatch_ref
from stretch_mujoco_amd.utils import scan_angles
from test_scanmatch_ref import _model_rays


def _random_S(rng, P, kind):
    if kind == "sparse":
        return np.where(rng.random(P) < 0.5, 0, rng.integers(0, 91801, P))
    if kind == "near":
        return 90000 + rng.integers(0, 1800, P)
    if kind == "equal":
        return np.full(P, 777)
    return rng.integers(0, 1 << 18, P)


@pytest.mark.parametrize("P", [1, 2, 7, 64, 257, 1000, 4096])
@pytest.mark.parametrize("kind", ["sparse", "near", "equal", "any"])
def test_properties_of_the_resampling(P, kind):
    rng = np.random.default_rng(P + len(kind))
    S = _random_S(rng, P, kind)
    if S.max() == 0:
        S[P // 2] = 5
    for span in (1, 4096, 1 << 18):
        for draw in (0, 1, 0x80000000, 0xFFFFFFFF, int(rng.integers(0, 1 << 32))):      # both ends of the draw are valid
            r = ref.resample(S, draw, span, 30, 360, 1)
            assert r.status == ref.OK and r.stat[3] == ref.OK and r.stat[2] == 360
            a, w, total = np.array(r.ancestors), np.array(r.w), r.total
            assert total == w.sum() >= 1 and r.stat[4] == total and r.stat[6] == max(int(S.max()) - span, 0) and r.stat[1] == S.max()
            o = (draw * total) >> 32
            assert 0 <= o < total and all(ref.threshold(k, total, o, P) < total for k in (0, P - 1))      # u_k < total, monotone in k
            assert (np.diff(a) >= 0).all() and a.min() >= 0 and a.max() < P                                  # ancestors are monotone in k
            assert (w[a] > 0).all()                                                                          # a weight-0 particle is never chosen
            copies = np.bincount(a, minlength=P)
            assert (np.abs(copies - P * w / total) < 1 + 1e-9).all()                                         # within one of its expected copies
            assert r.stat[7] == len(set(a.tolist())) and r.stat[0] == int(np.argmax(S)) and 1 <= r.stat[5] <= P
            assert r.stat[5] == total * total // int((w.astype(object) ** 2).sum())
            if kind == "equal":
                assert a.tolist() == list(range(P)) and r.stat[0] == 0 and r.stat[5] == P                    # all S equal: the identity, best particle 0


def test_status_and_what_does_not_run():
    S = [0, 5, 9, 9, 0]
    few = ref.resample(S, 7, 4096, 30, 29, 1)
    assert few.stat == [-1, 9, 29, ref.FEW, 0, 0, 0, 0] and few.ancestors == [0, 1, 2, 3, 4]
    lost = ref.resample([0] * 5, 7, 4096, 30, 30, 1)
    assert lost.stat == [-1, 0, 30, ref.LOST, 0, 0, 0, 0] and lost.ancestors == [0, 1, 2, 3, 4]
    assert ref.resample([0] * 5, 7, 4096, 30, 3, 1).status == ref.FEW      # too few returns comes first
    off = ref.resample(S, 7, 4, 30, 30, 0)
    assert off.stat == [2, 9, 30, ref.OK, 8, 2, 5, 0] and off.ancestors == [0, 1, 2, 3, 4]      # w = 0 0 4 4 0
    on = ref.resample(S, 0, 4, 30, 30, 1)
    assert on.stat == [2, 9, 30, ref.OK, 8, 2, 5, 2] and on.ancestors == [2, 2, 2, 3, 3]        # u = 0 1 3 4 6 on C = 0 0 4 8 8
    one = ref.resample([3], 0xFFFFFFFF, 1, 1, 1, 1)
    assert one.stat == [0, 3, 1, ref.OK, 1, 1, 2, 1] and one.ancestors == [0]
    parts = np.array([[1, 2, 3, 4, 5], [0, 0, 0, 0, 0], [9, 8, 7, 6, 5]], np.float32)
    assert np.array_equal(ref.move(parts, on.ancestors)[0], [3, 3, 3, 4, 4])
    assert ref.pose_bits(parts, on.stat).view(np.float32).tolist() == [3, 0, 7] and (ref.pose_bits(parts, lost.stat) == 0x7FC00000).all()


def test_the_largest_total():
    """4096 particles of 360 points of 255, the span at its cap: total = 376012800 <= 2^30, the squares fit uint64 with room."""
    P, S = 4096, 360 * 255
    r = ref.resample([S] * P, 0xFFFFFFFF, 1 << 18, 30, 360, 1)
    assert r.total == 4096 * 360 * 255 <= 1 << 30 and r.stat[4] == r.total and r.stat[5] == P and r.stat[7] == P and r.ancestors == list(range(P))
    assert P * S * S < 1 << 64 and ref.threshold(P - 1, r.total, r.total - 1, P) == r.total - 1
    top = ref.resample([S] + [0] * (P - 1), 0xFFFFFFFF, 1 << 18, 30, 360, 1)
    assert top.ancestors == [0] * P and top.stat[5] == 1 and top.stat[7] == 1


def _longhand_weight(points, particle, field, x0, y0, cell):
    """S of one particle, a point at a time in fp64 (no margins: the mid value)."""
    ny, nx = field.shape
    x, y, th = (float(v) for v in particle)
    if not np.isfinite([x, y, th]).all():
        return 0
    S = 0
    for px, py in points:
        if not (np.isfinite(px) and np.isfinite(py)):
            continue
        gx, gy = x + np.cos(th) * px - np.sin(th) * py, y + np.sin(th) * px + np.cos(th) * py
        ix, iy = int(np.floor((gx - x0) / cell)), int(np.floor((gy - y0) / cell))
        if 0 <= ix < nx and 0 <= iy < ny:
            S += int(field[iy, ix])
    return S


def test_weights_equal_a_long_hand_loop_and_bracket_it():
    geom = _model_rays()
    _, pts, mar = scanmatch_ref.float_stage_inputs([geom] * 3)
    fs = scanmatch_ref.FLOAT_STAGE
    nx, ny, (x0, y0) = fs.grids[1]
    rng = np.random.default_rng(2)
    field = rng.integers(0, 256, (ny, nx)).astype(np.uint8)
    parts = ref.float_stage_particles(64)
    x0f, y0f, cf = (float(np.float32(v)) for v in (x0, y0, fs.cell))
    for e in range(3):
        w = ref.weights(pts[e], mar[e], parts[:, e], field, x0, y0, fs.cell)
        assert w.n == int(np.isfinite(pts[e]).all(-1).sum()) >= 200
        assert (w.lo <= w.mid).all() and (w.mid <= w.hi).all() and ((w.lo == w.hi) | w.unsure.any(1)).all()
        for j in range(64):
            assert w.mid[j] == _longhand_weight(pts[e], parts[:, e, j].astype(np.float64), field, x0f, y0f, cf), (e, j)
        dead = ~np.isfinite(parts[:, e]).all(0)
        assert dead.sum() >= 4 and (w.hi[dead] == 0).all() and (w.hi[~dead] > 0).sum() > 40


def test_unsure_pairs_of_the_float_stage_cases_stay_under_the_cap():
    """A condition on the inputs of tests/test_gpu_localize.py's float stage, met by the reference alone: per env at most 2 % of the
    (particle, point) pairs are unsure, for every P and both grids; on a constant field a particle without unsure points has
    S = 200 x its on-grid count."""
    fs = scanmatch_ref.FLOAT_STAGE
    geom = _model_rays()
    _, pts, mar = scanmatch_ref.float_stage_inputs([geom] * 3)
    for nx, ny, (x0, y0) in fs.grids:
        field = np.full((ny, nx), 200, np.uint8)
        for P in ref.SHAPES:
            parts = ref.float_stage_particles(P)
            for e in range(3):
                w = ref.weights(pts[e], mar[e], parts[:, e], field, x0, y0, fs.cell)
                share = ref.unsure_share(w)
                print(f"{nx} x {ny} P {P} env {e}: unsure share {share:.5f}, S in [{int(w.lo.min())}, {int(w.hi.max())}]")
                assert share <= ref.MAX_AMBIGUOUS, (nx, ny, P, e, share)
                assert (w.lo % 200 == 0).all() and (w.hi % 200 == 0).all() and w.hi.max() > 0


@functools.lru_cache(maxsize=None)
def _loop():
    return ref.closed_loop()


def test_the_filter_finds_the_robots_in_a_synthetic_room():
    """From a spread of +-1 m and +-30 degrees round a centre 0.63 m and 17 degrees (or more) off: after LOOP.updates updates, and for
    LOOP.extra more, the best particle lies within half a cell and 1 degree of the truth in all three envs."""
    errors, statuses, ess = _loop()
    L = ref.LOOP
    for i in range(len(errors)):
        print(f"update {i:2d}: " + "  ".join(f"({m:.3f} m, {np.rad2deg(a):.2f} deg)" for m, a in errors[i]) + f"  ess {ess[i].tolist()}")
    assert (statuses == ref.OK).all() and errors.shape == (L.updates + L.extra, 3, 2)
    off = np.array([ref.pose_error(c, t) for c, t in zip(ref.loop_inputs().center, ref.loop_inputs().truth)])
    assert (off[:, 0] >= 0.6).all() and (off[:, 1] >= np.deg2rad(15.0)).all()                        # the centre is far off
    assert (np.abs(L.offset) <= np.array(L.half_extent)).all() and L.half_extent[0] >= 1.0 and L.half_extent[2] >= np.deg2rad(30.0)      # and the truth inside the spread
    tail = errors[L.updates - 1:]
    assert len(tail) == L.extra + 1
    assert (tail[..., 0] <= 0.5 * L.bound[0]).all() and (tail[..., 1] <= 0.5 * L.bound[1]).all(), tail.tolist()
    assert (ess[0] < 50).all() and (ess[-1] > 200).all()      # the weights start on a few particles and end spread over many


def test_the_matcher_alone_does_not_bridge_the_spread():
    """scanmatch_ref.decide from the spread's centre with the default window (+-0.5 m, +-5 degrees) misses the bound: the case the
    particle filter exists for."""
    g = scanmatch_ref.ROOM_GRID
    o, d, So, Sd = scanmatch_ref.unit_rays()
    field = ref.loop_field()
    inp = ref.loop_inputs()
    angles = scan_angles().angles.numpy()
    W = int(round(0.5 / g.cell))
    for e in range(3):
        scan = scanmatch_ref.room_scan(inp.truth[e], o, d).astype(np.float32).astype(np.float64)
        pts, mar, _ = scanmatch_ref.frame_points(o, d, So, Sd, scan, *ref.LOOP.limits)
        prior = inp.center[e].astype(np.float32)[:, None]
        pl = scanmatch_ref.place(pts[None], mar[None], prior, angles, *g.origin, g.cell, g.nx, g.ny)
        dec = scanmatch_ref.decide(pl.cell, field[None], prior, angles, g.cell, pl.n, wx=W, wy=W, min_points=30)
        err = ref.pose_error(dec.pose[:, 0], inp.truth[e])
        print(f"env {e}: the matcher from the centre ends ({err[0]:.3f} m, {np.rad2deg(err[1]):.2f} deg) off")
        assert dec.status[0] == scanmatch_ref.OK and (err[0] > ref.LOOP.bound[0] or err[1] > ref.LOOP.bound[1]), err
