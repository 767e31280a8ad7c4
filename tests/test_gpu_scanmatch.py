"""Correlative scan matching on the HIP path: smj_scan_to_pose through the C-ABI and StretchBatchSimulator.pull_scan_match.

One simulator for the module, the rig of tests/test_gpu_occupancy.py: stretch_scene, three envs driven apart, 200 steps, the lidar on.
The scans fed to the entry are synthetic: ranges cast in fp64 in the room of tests/scanmatch_ref.py along the rays the rig's XPOSE
gives in the robot's frame, with NaN, -1, ranges below r_min, above r_max and +inf among them.  The kernel is compared in the two
stages of the reference: the cells of every ray and rotation against place() (sure points equal, unsure ones among their candidates,
at most 2 % unsure per env), and score, best and pose against decide() on the device's own cells, bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import perception_rig
import scanmatch_ref as ref
from conftest import ROOT
from perception_rig import B, DEV, Guarded, bare, dev as _dev, f32, stream as _stream  # noqa: F401 (bare: the module's fixture)
from point_cloud_ref import body_pose

pytestmark = pytest.mark.gpu

K = 360
CELL = 0.05
FILL = -7
INF = float("inf")
NaN = float("nan")
LIMITS = ref.FLOAT_STAGE.limits


@pytest.fixture(scope="module")
def rig():
    r = perception_rig.scan_rig(K)
    r.prior = np.ascontiguousarray(ref.FLOAT_STAGE.prior.T)
    yield r
    r.sim.stop()


def _outputs(T, wx, wy):
    return [torch.full((3, B), float(FILL), dtype=torch.float32, device=DEV), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV),
            torch.full((B, T, 2 * wy + 1, 2 * wx + 1), FILL, dtype=torch.int32, device=DEV), torch.full((B, T, K, 2), FILL, dtype=torch.int32, device=DEV)]


def _match(r, scan, field, prior, angles, *, origin, wx, wy, bias=None, sw=0, mp=30, limits=LIMITS, cell=CELL, out=None, score=True, cells=True, rc=0, ctx=None,
           frame=None, ld=None):
    """The C call on device tensors; returns [pose, best, score, cell] (sentinels where nothing is written)."""
    ny, nx = field.shape[1:]
    T = angles.shape[0]
    if out is None:
        out = _outputs(T, wx, wy)
    ptr = perception_rig.ptr
    got = r.L.smj_scan_to_pose(ctx or r.sim._ctx, ptr(scan), scan.stride(0) if ld is None else ld, r.base if frame is None else frame, limits[0], limits[1],
                               ptr(field), nx, ny, origin[0], origin[1], cell, ptr(prior), ptr(angles), ptr(bias), T, wx, wy, sw, mp, ptr(out[0]), ptr(out[1]),
                               ptr(out[2]) if score else None, ptr(out[3]) if cells else None, _stream())
    assert got == rc, (got, r.L.smj_last_error(ctx or r.sim._ctx))
    return out


def _field(nx, ny, seed, flavour="mixed"):
    """uint8 [B, ny, nx] from a small set of values, so that equal sums are the rule; "full": 255 everywhere."""
    if flavour == "full":
        return np.full((B, ny, nx), 255, np.uint8)
    rng = np.random.default_rng(seed)
    return np.array([0, 0, 255, 200, 13], np.uint8)[rng.integers(0, 5, (B, ny, nx))]


def _angles(T):
    k = np.array([0] + [s * j for j in range(1, T // 2 + 1) for s in (-1, 1)][:T - 1])
    return (k * 0.0123).astype(np.float32)


def _equal_decide(tag, got, field, prior, angles, cell, **kw):
    """score, best and pose of the device equal decide() on the device's own cells and n, bit for bit."""
    torch.cuda.synchronize()
    pose, best, score, cells = (t.cpu().numpy() for t in got)
    want = ref.decide(cells, field, prior, angles, cell, best[:, 2], **kw)
    assert np.array_equal(score, want.score), (tag, int((score != want.score).sum()), np.argwhere(score != want.score)[:5].tolist())
    assert np.array_equal(best, want.best), (tag, best.tolist(), want.best.tolist())
    assert pose.tobytes() == want.pose.tobytes(), (tag, pose.tolist(), want.pose.tolist())
    return want


@pytest.mark.parametrize("nx,ny,origin", ref.FLOAT_STAGE.grids)
def test_float_stage_cells_against_the_reference_with_a_cap(rig, nx, ny, origin):
    r, fs = rig, ref.FLOAT_STAGE
    field = _field(nx, ny, 1)
    got = _match(r, r.scan, _dev(field), _dev(r.prior), _dev(fs.angles), origin=origin, wx=2, wy=1)
    torch.cuda.synchronize()
    pl = ref.place(r.pts, r.mar, r.prior, fs.angles, origin[0], origin[1], CELL, nx, ny)
    share = ref.unsure_share(pl)
    cells = got[3].cpu().numpy()
    print(f"{nx} x {ny}: counting rays {pl.n.tolist()}, unsure share {share.tolist()}, with a cell {int((cells[..., 0] != ref.NO_CELL).sum())}")
    assert (share <= ref.MAX_AMBIGUOUS).all(), share
    bad = ref.check_cells(cells, pl)
    assert not bad, (len(bad), bad[:5])
    assert got[1][:, 2].tolist() == pl.n.tolist() and (pl.n >= 200).all()
    assert ((cells[..., 0] == ref.NO_CELL) == (cells[..., 1] == ref.NO_CELL)).all()
    assert (cells[..., 0] != ref.NO_CELL).sum() > 300      # not about empty tables
    dropped = ~np.isfinite(r.pts).all(-1)                  # rays that are no return have no cell under any rotation
    assert dropped.sum() > 60 and (cells[np.broadcast_to(dropped[:, None, :], cells.shape[:3])] == ref.NO_CELL).all()
    _equal_decide("float stage", got, field, r.prior, fs.angles, CELL, wx=2, wy=1)


# (nx, ny, origin, cell, T, wx, wy, field, bias, shift_weight): both builds of the kernel (up to 16384 cells, above), the sizes on
# either side of that threshold, one rotation and one candidate, 64 rotations, the widest window, a grid of one cell
INTEGER_STAGE = [(128, 96, (-3.187, -2.379), CELL, 1, 0, 0, "mixed", False, 0),
                 (128, 96, (-3.187, -2.379), CELL, 5, 3, 2, "mixed", True, 3),
                 (128, 96, (-3.187, -2.379), CELL, 5, 3, 2, "full", False, 0),
                 (37, 29, (-0.913, -0.707), CELL, 5, 3, 2, "mixed", False, 1024),
                 (37, 29, (-0.913, -0.707), CELL, 64, 1, 1, "mixed", True, 0),
                 (37, 29, (-0.913, -0.707), CELL, 64, 1, 1, "full", True, 1),
                 (61, 83, (-1.513, -2.079), CELL, 3, 32, 32, "mixed", True, 1),
                 (128, 128, (-3.2, -3.2), CELL, 5, 3, 2, "mixed", False, 0),
                 (129, 128, (-3.2, -3.2), CELL, 5, 3, 2, "mixed", True, 3),
                 (256, 256, (-6.4, -6.4), CELL, 5, 3, 2, "mixed", True, 3),
                 (4096, 16, (-102.4, -0.4), CELL, 2, 1, 32, "mixed", False, 0),
                 (1, 1, (-2.0, -2.0), 4.0, 5, 3, 2, "mixed", True, 0),
                 (1, 1, (-2.0, -2.0), 4.0, 1, 0, 0, "full", False, 0)]


@pytest.mark.parametrize("nx,ny,origin,cell,T,wx,wy,flavour,with_bias,sw", INTEGER_STAGE)
def test_integer_stage_equals_the_reference(rig, nx, ny, origin, cell, T, wx, wy, flavour, with_bias, sw):
    r = rig
    field, angles = _field(nx, ny, nx + T, flavour), _angles(T)
    bias = np.array([0, 7, -5, 255, 1 << 21, 3, 1 << 20, 40], np.int32)[np.arange(T) % 8] if with_bias else None
    got = _match(r, r.scan, _dev(field), _dev(r.prior), _dev(angles), origin=origin, cell=cell, wx=wx, wy=wy, bias=_dev(bias) if with_bias else None, sw=sw)
    want = _equal_decide((nx, ny, T, wx, wy), got, field, r.prior, angles, cell, wx=wx, wy=wy, bias=bias, shift_weight=sw)
    assert (want.status == ref.OK).all()
    cells = got[3].cpu().numpy()
    tied = [int((want.score[e] == want.best[e, 1]).sum()) for e in range(B)]
    print(f"{nx} x {ny} T {T} window {wx} x {wy} {flavour}: rays with a cell {int((cells[..., 0] != ref.NO_CELL).sum())} of {B * T * K}, best {want.best.tolist()}, "
          f"candidates at the maximum {tied}")
    assert (cells[..., 0] != ref.NO_CELL).sum() > 100 * T
    if flavour == "full" and nx > 1 and not with_bias and sw == 0:
        assert min(tied) > 100      # massive ties: the smallest index among them won (decide() takes the first maximum)


def test_statuses(rig):
    """A prior that is not finite; fewer returns than min_points; a scan without a single return."""
    r = rig
    nx, ny, origin, T = 61, 83, (-1.513, -2.079), 3
    field, angles = _field(nx, ny, 9), _angles(T)
    bias = np.array([5, 0, 2], np.int32)
    prior = r.prior.copy()
    prior[0, 0] = NaN
    prior[2, 1] = INF
    got = _match(r, r.scan, _dev(field), _dev(prior), _dev(angles), origin=origin, wx=2, wy=2, bias=_dev(bias), sw=2)
    want = _equal_decide("not finite", got, field, prior, angles, CELL, wx=2, wy=2, bias=bias, shift_weight=2)
    assert want.best[:, 3].tolist() == [ref.OFF, ref.OFF, ref.OK] and want.best[:2, :2].tolist() == [[-1, 0]] * 2
    cells = got[3].cpu().numpy()
    assert (cells[:2] == ref.NO_CELL).all() and (cells[2, ..., 0] != ref.NO_CELL).any()
    # the scores of a pose that is not finite are evaluated all the same: no point is placed, so J = -bias - shift_weight r^2
    dy, dx = np.mgrid[-2:3, -2:3]
    assert np.array_equal(got[2][0].cpu().numpy(), -bias[:, None, None] - 2 * (dx * dx + dy * dy)[None])
    # few: env 0 keeps 12 returns, env 1 none at all (every kind of dropped ray), env 2 all of its own
    scan = r.scan_host.copy()
    keep = np.nonzero(np.isfinite(r.pts[0]).all(-1))[0][:12]
    col = np.full(K, -1.0, np.float32)
    col[keep] = scan[keep, 0]
    scan[:, 0] = col
    scan[:, 1] = np.array([NaN, -1.0, 0.1, 7.0, INF, -INF], np.float32)[np.arange(K) % 6]
    for mp, statuses in ((30, [ref.FEW, ref.FEW, ref.OK]), (12, [ref.OK, ref.FEW, ref.OK]), (13, [ref.FEW, ref.FEW, ref.OK]), (1, [ref.OK, ref.FEW, ref.OK])):
        got = _match(r, _dev(scan), _dev(field), _dev(r.prior), _dev(angles), origin=origin, wx=2, wy=2, mp=mp)
        want = _equal_decide(("few", mp), got, field, r.prior, angles, CELL, wx=2, wy=2, min_points=mp)
        assert want.best[:, 3].tolist() == statuses and want.best[:2, 2].tolist() == [12, 0]
        assert (got[3][1] == ref.NO_CELL).all() and int(got[2][1].abs().max()) == 0


def test_two_calls_agree_and_envs_do_not_see_each_other(rig):
    r = rig
    nx, ny, origin, T = 128, 96, (-3.187, -2.379), 5
    field, angles = _field(nx, ny, 4), _angles(T)
    args = dict(origin=origin, wx=3, wy=2, sw=1)
    a = _match(r, r.scan, _dev(field), _dev(r.prior), _dev(angles), **args)
    b = _match(r, r.scan, _dev(field), _dev(r.prior), _dev(angles), **args)
    torch.cuda.synchronize()
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    # another scan, field and prior for env 1 alone: envs 0 and 2 give what they gave
    scan, f2, p2 = r.scan_host.copy(), field.copy(), r.prior.copy()
    scan[:, 1] = np.roll(scan[:, 1], 17)
    f2[1] = f2[1, ::-1, ::-1]
    p2[:, 1] += np.array([0.3, -0.2, 0.4], np.float32)
    c = _match(r, _dev(scan), _dev(f2), _dev(p2), _dev(angles), **args)
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(a, c)):
        x, y = (x.t(), y.t()) if k == 0 else (x, y)      # the pose is [3, B]
        assert torch.equal(x[0], y[0]) and torch.equal(x[2], y[2]) and not torch.equal(x[1], y[1])


def test_null_score_and_cell_are_left_untouched(rig):
    r = rig
    nx, ny, origin, T = 37, 29, (-0.913, -0.707), 5
    field, angles = _dev(_field(nx, ny, 2)), _dev(_angles(T))
    full = _match(r, r.scan, field, _dev(r.prior), angles, origin=origin, wx=3, wy=2)
    for score, cells in ((False, True), (True, False), (False, False)):
        got = _match(r, r.scan, field, _dev(r.prior), angles, origin=origin, wx=3, wy=2, score=score, cells=cells)
        torch.cuda.synchronize()
        assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1])
        assert torch.equal(got[2], full[2]) if score else int((got[2] != FILL).sum()) == 0
        assert torch.equal(got[3], full[3]) if cells else int((got[3] != FILL).sum()) == 0


def _shifted(t, fill, by):
    big = torch.full((t.numel() + by + 21,), fill, dtype=t.dtype, device=DEV)
    view = big[by:by + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (by * t.element_size()) % 16
    return big, view


@pytest.mark.parametrize("nx,ny,origin", [(61, 83, (-1.513, -2.079)), (129, 128, (-3.2, -3.2)), (5, 3, (-0.113, -0.107))])
def test_nothing_outside_the_outputs_is_written_and_alignment_does_not_matter(rig, nx, ny, origin):
    """The outputs as views 4, 8 or 12 bytes past a 16-byte boundary inside buffers of sentinels: the guards stay untouched and the
    values are those of the aligned call; the same with the field 1 .. 15 bytes past a 16-byte boundary (its copy into LDS has a path
    for the bytes before the first boundary, one for whole groups of 16 and one for the rest) and every other input 4 bytes past one."""
    r = rig
    T, wx, wy = 3, 2, 1
    field, angles, bias, prior = _dev(_field(nx, ny, 6)), _dev(_angles(T)), _dev(np.array([3, 0, 9], np.int32)), _dev(r.prior)
    aligned = _match(r, r.scan, field, prior, angles, origin=origin, wx=wx, wy=wy, bias=bias, sw=1)
    assert all(t.data_ptr() % 16 == 0 for t in aligned) and field.data_ptr() % 16 == 0
    ins = [_shifted(t, f, 1) for t, f in ((r.scan, 55.0), (prior, 55.0), (angles, 55.0), (bias, 55))]
    results, fields = [], []
    for moved, by, pads in ((False, 1, (1, 1, 1, 1)), (True, 2, (1, 1, 1, 1)), (False, 3, (2, 3, 2, 3)), (True, 7, (3, 2, 3, 2)), (False, 8, (2, 1, 3, 1)), (True, 13, (1, 3, 1, 2)),
                            (False, 15, (3, 3, 2, 1)), (True, 16, (2, 2, 2, 2))):
        outs = [Guarded.of(32 + pads[0], torch.float32, 3, B), Guarded.of(32 + pads[1], torch.int32, B, 4), Guarded.of(32 + pads[2], torch.int32, B, T, 2 * wy + 1, 2 * wx + 1),
                Guarded.of(32 + pads[3], torch.int32, B, T, K, 2)]
        fbig, fview = _shifted(field, 99, by)
        scan, pr, an, bi = [v for _, v in ins] if moved else (r.scan, prior, angles, bias)
        _match(r, scan, fview, pr, an, origin=origin, wx=wx, wy=wy, bias=bi, sw=1, out=[o.view for o in outs])
        results.append(outs)
        fields.append((fbig, fview, by))
    torch.cuda.synchronize()
    _equal_decide("aligned", aligned, field.cpu().numpy(), r.prior, angles.cpu().numpy(), CELL, wx=wx, wy=wy, bias=bias.cpu().numpy(), shift_weight=1)
    for outs in results:
        for o, w in zip(outs, aligned):
            o.check(w)
    for (big, view), t in zip(ins, (r.scan, prior, angles, bias)):
        fill = big[0].item()
        assert (big[1 + t.numel():] == fill).all() and view.cpu().numpy().tobytes() == t.cpu().numpy().tobytes()      # the inputs and what lies round them are unchanged
    for fbig, fview, by in fields:
        assert (fbig[:by] == 99).all() and (fbig[by + field.numel():] == 99).all() and torch.equal(fview, field)


def test_error_codes_and_a_refused_call_writes_nothing(rig, bare):
    r = rig
    L, sim = r.L, r.sim
    nx = ny = 32
    T, wx, wy = 4, 2, 1
    C = (2 * wx + 1) * (2 * wy + 1)
    cells = B * nx * ny
    nbody = sim.xpose.shape[0] // 12
    sizes = dict(scan=K * B, field=cells // 4, pose=3 * B, angle=T, bias=T, pose_out=3 * B, best=4 * B, score=B * T * C, cell=B * T * K * 2)
    pool = torch.zeros(sum(sizes.values()) + 64, dtype=torch.int32, device=DEV)      # one allocation, so that ranges can be made to overlap
    at, p = {}, pool.data_ptr()
    for name, words in sizes.items():
        at[name] = p
        p += 4 * ((words + 3) // 4 * 4)      # every range starts on a 16-byte boundary
    good = dict(ld=B, frame=r.base, r_min=0.2, r_max=5.0, nx=nx, ny=ny, x0=-0.81, y0=-0.81, cell=0.05, T=T, wx=wx, wy=wy, sw=0, mp=30)

    def call(a, ctx=None, **ptrs):
        q = dict(at, **ptrs)
        vp = lambda v: ctypes.c_void_p(v) if v else None
        return L.smj_scan_to_pose(ctx or sim._ctx, vp(q["scan"]), a["ld"], a["frame"], a["r_min"], a["r_max"], vp(q["field"]), a["nx"], a["ny"], a["x0"], a["y0"], a["cell"],
                                  vp(q["pose"]), vp(q["angle"]), vp(q["bias"]), a["T"], a["wx"], a["wy"], a["sw"], a["mp"], vp(q["pose_out"]), vp(q["best"]),
                                  vp(q["score"]), vp(q["cell"]), _stream())

    bad = [dict(ld=B - 1), dict(ld=0), dict(ld=-5), dict(nx=0), dict(ny=0), dict(nx=-4), dict(ny=-1), dict(nx=4097, ny=1), dict(nx=1, ny=4097), dict(nx=8192, ny=8),
           dict(nx=257, ny=256), dict(nx=256, ny=257), dict(cell=0.0), dict(cell=-0.05), dict(cell=NaN), dict(cell=INF), dict(x0=NaN), dict(x0=INF), dict(y0=-INF), dict(y0=NaN),
           dict(r_min=NaN), dict(r_max=NaN), dict(r_max=INF), dict(r_min=-0.1), dict(r_min=-INF), dict(r_min=5.5), dict(r_max=0.1), dict(cell=0.0005, r_max=4.2),
           dict(cell=1e-3, r_max=8.5), dict(frame=r.lib.FRAME_WORLD), dict(frame=r.lib.FRAME_CAMERA), dict(frame=-3), dict(frame=10 ** 6), dict(frame=nbody),
           dict(T=0), dict(T=-1), dict(T=65), dict(wx=-1), dict(wx=33), dict(wy=-1), dict(wy=33), dict(wx=2 ** 16, wy=2 ** 16), dict(sw=-1), dict(sw=1025), dict(mp=0),
           dict(mp=-7), dict(mp=1025)]
    for change in bad:
        rc = call(dict(good, **change))
        assert rc == -1 and L.smj_last_error(sim._ctx), (change, rc)
    for name in ("scan", "field", "pose", "angle", "pose_out", "best"):      # null required pointers
        assert call(good, **{name: None}) == -1, name
    for name, by in (("scan", 2), ("pose", 1), ("angle", 3), ("bias", 2), ("pose_out", 1), ("best", 2), ("score", 2), ("cell", 1)):
        assert call(good, **{name: at[name] + by}) == -1 and b"aligned" in L.smj_last_error(sim._ctx), (name, by)
    # overlap: an output on an input, on another output, on the bound XPOSE array, by a whole range and by one word at either end
    last = lambda name: 4 * (sizes[name] - 1)
    for kw in (dict(pose_out=at["pose"]), dict(best=at["scan"]), dict(score=at["field"]), dict(cell=at["angle"]), dict(pose_out=at["bias"]), dict(best=at["pose_out"]),
               dict(score=at["pose_out"]), dict(cell=at["best"]), dict(cell=at["score"]), dict(score=at["best"]), dict(pose_out=at["pose"] + last("pose")),
               dict(pose_out=at["pose"] - last("pose_out")), dict(field=at["pose_out"] + last("pose_out") + 3), dict(field=at["cell"] - 4 * sizes["field"] + 1),
               dict(best=at["pose_out"] + last("pose_out")), dict(best=at["pose_out"] - last("best")), dict(cell=at["score"] + last("score")),
               dict(cell=at["scan"] - last("cell")), dict(bias=at["cell"] + last("cell")), dict(angle=at["best"] - last("angle")), dict(scan=at["score"] - last("scan")),
               dict(pose_out=sim.xpose.data_ptr()), dict(best=sim.xpose.data_ptr() + 4 * (sim.xpose.numel() - 1))):
        assert call(good, **kw) == -1 and b"overlap" in L.smj_last_error(sim._ctx), kw
    xpose_before = sim.xpose.clone()
    torch.cuda.synchronize()
    assert int(pool.abs().max()) == 0      # a refused call writes nothing
    # a bare context (nothing bound): -5, after every -1
    assert call(good, ctx=bare.ctx) == -5 and b"XPOSE" in L.smj_last_error(bare.ctx)
    assert call(dict(good, T=0), ctx=bare.ctx) == -1 and call(dict(good, frame=nbody), ctx=bare.ctx) == -1
    # models without a lidar: no ray-casting tables at all, and tables with no rangefinder
    from stretch_mujoco_amd import model_blob

    no_tables = {k: v for k, v in sim.model.items() if k != "sensor_lidar_static"}
    no_rays = dict(sim.model, sensor_lidar_site=np.zeros(0, np.int32), sensor_lidar_static=np.zeros(0, np.float64))
    for model in (no_tables, no_rays):
        blob = model_blob.dumps(model)
        ctx = ctypes.c_void_p()
        assert L.smj_create(blob, len(blob), B, 0, ctypes.byref(ctx)) == 0, L.smj_last_error(ctx)
        try:
            assert call(good, ctx=ctx) == -6 and b"lidar" in L.smj_last_error(ctx)
            assert call(dict(good, T=0), ctx=ctx) == -6      # -6 comes first
        finally:
            L.smj_destroy(ctx)
    torch.cuda.synchronize()
    assert int(pool.abs().max()) == 0 and torch.equal(sim.xpose, xpose_before)
    # accepted: the extremes of every argument, null optional pointers, adjacent ranges, a misaligned field, the last body as the frame
    for change, ptrs in ((dict(sw=1024, mp=1024), {}), (dict(mp=1, r_min=0.0, r_max=0.0), {}), (dict(cell=0.0009765625, r_max=8.0), dict(field=at["field"] + 1)),
                         (dict(cell=1e-30, x0=-3e38, y0=3e38, r_min=0.0, r_max=1e-27), dict(bias=None, score=None, cell=None)), (dict(frame=nbody - 1), {}),
                         (dict(T=1, wx=0, wy=0), {}), ({}, {})):
        assert call(dict(good, **change), **ptrs) == 0, (change, L.smj_last_error(sim._ctx))
    torch.cuda.synchronize()
    words = lambda name: pool[(at[name] - pool.data_ptr()) // 4:][:sizes[name]]
    # all-zero inputs: every range 0 is below r_min, so no ray counts: too few points, the prior (0, 0, 0) comes back, no cell, J = 0
    assert words("best").view(B, 4).tolist() == [[-1, 0, 0, ref.FEW]] * B and int(words("pose_out").abs().max()) == 0
    assert all(int(words(name).abs().max()) == 0 for name in ("scan", "field", "pose", "angle", "bias"))      # the inputs are unchanged
    assert (words("cell") == ref.NO_CELL).all() and int(words("score").abs().max()) == 0


def test_consistent_with_the_occupancy_entry(rig):
    """The simulator's own scan, mapped by smj_lidar_to_occupancy in the world frame, and matched from the planar pose of the same
    body (the host copy of XPOSE), one rotation, no shift: the field is 255 on the hit cells and their 8 neighbours, the two passes
    place a point at most one cell apart, so every counted return collects 255: S = 255 n exactly."""
    r = rig
    sim = r.sim
    nx = ny = 128
    origin = (-3.2 + 0.0137, -3.2 - 0.0071)
    scan = sim.lidar[:K].clone()
    hit = torch.zeros(B, ny, nx, dtype=torch.int32, device=DEV)
    limits = (0.2, 9.5)      # the bounds tests/test_gpu_occupancy.py counts the rig's returns in
    rc = r.L.smj_lidar_to_occupancy(sim._ctx, perception_rig.ptr(scan), B, r.lib.FRAME_WORLD, origin[0], origin[1], CELL, nx, ny, limits[0], limits[1], 0, 0,
                                    perception_rig.ptr(hit), None, _stream())
    assert rc == 0, r.L.smj_last_error(sim._ctx)
    near = torch.nn.functional.max_pool2d((hit > 0).float().unsqueeze(1), 3, 1, 1).squeeze(1)
    field = (near * 255).to(torch.uint8).contiguous()
    bp, bm = body_pose(r.xpose, r.base)
    prior = np.stack((bp[:, 0], bp[:, 1], np.arctan2(bm[:, 1, 0], bm[:, 0, 0]))).astype(np.float32)
    got = _match(r, scan, field, _dev(prior), _dev(np.zeros(1, np.float32)), origin=origin, wx=0, wy=0, mp=1, limits=limits)
    torch.cuda.synchronize()
    best = got[1].cpu().numpy()
    print("consistency: best", best.tolist(), "hit cells", (hit > 0).sum((1, 2)).tolist())
    assert (best[:, 3] == ref.OK).all() and (best[:, 2] >= 50).all() and (best[:, 0] == 0).all()
    assert (best[:, 1] == 255 * best[:, 2]).all()
    assert got[0].cpu().numpy().tobytes() == prior.tobytes()      # no shift, no rotation: x + 0 cell and theta + 0


def test_end_to_end_through_pull_scan_match(rig):
    """The simulator's own scan against a map made of it at the true pose; priors off by whole lattice steps.  The device equals the
    reference on the scan copied to the host (decide() on the device's cells, those within place()'s margins), and the winner lies
    within one lattice step of the truth -- asserted after the reference itself, on its own fp64 cells, meets that bound."""
    from stretch_mujoco_amd.datamodels import StatusStretchScanMatch
    from stretch_mujoco_amd.utils import scan_angles

    r = rig
    sim = r.sim
    og = sim.pull_occupancy_grid(frame="world")
    df = sim.pull_distance_field(og)
    bp, bm = body_pose(r.xpose, r.base)
    truth = np.stack((bp[:, 0], bp[:, 1], np.arctan2(bm[:, 1, 0], bm[:, 0, 0])))
    step = 0.008727
    offsets = np.array([(3, -2, 4), (-7, 5, -6), (10, -10, 10)])
    prior = (truth + offsets.T * np.array([[CELL], [CELL], [step]])).astype(np.float32)
    m = sim.pull_scan_match(df, _dev(prior), sigma=0.10, scores=True, cells=True)
    assert isinstance(m, StatusStretchScanMatch) and m.frame == "world" and m.window == (10, 10) and m.origin == (-3.2, -3.2) and m.cell == CELL
    assert tuple(m.pose.shape) == (3, B) and tuple(m.best.shape) == (B, 4) and tuple(m.score.shape) == (B, 21, 21, 21) and tuple(m.cells.shape) == (B, 21, K, 2)
    torch.cuda.synchronize()
    field = df.likelihood(0.10).cpu().numpy()
    angles = scan_angles().angles.numpy()
    assert torch.equal(m.angles.cpu(), scan_angles().angles)
    scan = sim.lidar[:K].cpu().numpy()
    want = _equal_decide("pull_scan_match", [m.pose, m.best, m.score, m.cells], field, prior, angles, CELL, wx=10, wy=10)
    per = [ref.frame_points(*g, scan[:, e].astype(np.float64), 0.2, 5.0) for e, g in enumerate(r.geoms)]
    pl = ref.place(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]), prior, angles, -3.2, -3.2, CELL, 128, 128)
    assert (ref.unsure_share(pl) <= ref.MAX_AMBIGUOUS).all() and not ref.check_cells(m.cells.cpu().numpy(), pl)
    assert m.best[:, 2].tolist() == pl.n.tolist() and m.ok().all()
    own = ref.decide(pl.cell, field, prior, angles, CELL, pl.n, wx=10, wy=10)      # the reference alone, on its own cells
    k_of_row = np.round(angles / step).astype(int)

    def errors(best):
        out = []
        for e in range(B):
            t, dy, dx = ref.unindex(int(best[e, 0]), 10, 10)
            out.append((dx + offsets[e, 0], dy + offsets[e, 1], int(k_of_row[t]) + offsets[e, 2]))
        return out

    print("lattice errors of the reference", errors(own.best), "of the device", errors(want.best), "fit", m.fit().tolist())
    assert max(abs(v) for err in errors(own.best) for v in err) <= 1      # the reference meets the bound on these three poses
    assert max(abs(v) for err in errors(want.best) for v in err) <= 1
    fine = m.refined()
    assert tuple(fine.shape) == (3, B) and bool(((fine - m.pose).abs() <= torch.tensor([[CELL], [CELL], [step]], device=DEV)).all())
    # the occupancy grid itself and a bare field give the same match; the pose feeds pull_base_command as it is
    first = [t.clone() for t in (m.pose, m.best)]
    again = sim.pull_scan_match(og, _dev(prior))
    assert again.score is None and again.cells is None and torch.equal(again.pose, first[0]) and torch.equal(again.best, first[1])
    bare_field = sim.pull_scan_match(df.likelihood(0.10), _dev(prior), origin=(-3.2, -3.2), cell=CELL)
    assert bare_field.frame == "grid" and torch.equal(bare_field.pose, first[0])
    nf = sim.pull_navigation_field((0.5, 0.0), df)
    cmd = sim.pull_base_command(nf, pose=again.pose)
    assert tuple(cmd.cmd.shape) == (2, B)
    # prior=None is the simulator's own pose: the match stays within a step of it
    home = sim.pull_scan_match(df)
    torch.cuda.synchronize()
    assert home.ok().all() and bool(((home.pose - sim.base_pose).abs() <= torch.tensor([[CELL], [CELL], [step]], device=DEV) * 1.001).all())


def test_value_errors_are_raised_before_any_launch(rig):
    from stretch_mujoco_amd.datamodels import StatusStretchDistanceField, StatusStretchOccupancyGrid
    from stretch_mujoco_amd.utils import ScanAngles, scan_angles

    sim = rig.sim
    dev = sim.device
    og = sim.pull_occupancy_grid(frame="world")
    df = sim.pull_distance_field(og)
    keep = sim.pull_scan_match(df, scores=True, cells=True)
    torch.cuda.synchronize()
    tensors = (og.hit, df.dist2, keep.pose, keep.best, keep.score, keep.cells, sim.base_pose)
    snap = [t.clone() for t in tensors]
    a = scan_angles(device=dev)
    u8 = df.likelihood()
    odd = lambda **kw: StatusStretchDistanceField(**dict(dict(time=0, dist2=df.dist2, nearest=None, origin=df.origin, cell=df.cell, frame="world"), **kw))
    base_og = StatusStretchOccupancyGrid(time=0, hit=og.hit, miss=og.miss, origin=og.origin, cell=og.cell, frame="base")
    for field, kw in (("field", {}), (df.dist2, {}), (u8, {}), (u8, dict(origin=(0.0, 0.0))), (u8, dict(cell=0.05)), (u8[0], dict(origin=(0.0, 0.0), cell=0.05)),
                      (u8[:2], dict(origin=(0.0, 0.0), cell=0.05)), (u8, dict(origin=(0.0, NaN), cell=0.05)), (u8, dict(origin=(0.0, 0.0), cell=0.0)),
                      (odd(frame="base"), {}), (base_og, {}), (odd(frame="odom"), {}), (odd(dist2=df.dist2.to(torch.int64)), {}), (odd(dist2=df.dist2[:2]), {}),
                      (odd(dist2=df.dist2.cpu()), {}), (odd(cell=0.0), {}), (odd(cell=NaN), {}), (df, dict(cell=0.05)), (df, dict(origin=(0.0, 0.0))),
                      (df, dict(sigma=0.0)), (df, dict(sigma=-0.1)), (df, dict(sigma=NaN)), (df, dict(sigma=INF)), (og, dict(sigma=0.0)),
                      (df, dict(window=(1.7, 0.5))), (df, dict(window=(0.5, -0.1))), (df, dict(window=0.5)), (df, dict(window=(0.5, NaN))), (df, dict(window=(0.5, 0.5, 0.5))),
                      (df, dict(range_limits=(0.2,))), (df, dict(range_limits=(-0.1, 5.0))), (df, dict(range_limits=(5.0, 0.2))), (df, dict(range_limits=(0.2, INF))),
                      (df, dict(range_limits=(0.2, 500.0))), (df, dict(min_points=0)), (df, dict(min_points=1025)), (df, dict(shift_weight=-1)), (df, dict(shift_weight=1025)),
                      (df, dict(angles="table")), (df, dict(angles=(a.angles, a.bias))), (df, dict(angles=ScanAngles(a.angles.double(), a.bias))),
                      (df, dict(angles=ScanAngles(a.angles, a.bias[:3]))), (df, dict(angles=ScanAngles(a.angles, a.bias.float()))),
                      (df, dict(angles=ScanAngles(torch.zeros(65, device=dev), None))), (df, dict(angles=ScanAngles(torch.zeros(0, device=dev), None))),
                      (df, dict(angles=ScanAngles(torch.zeros(3, 1, device=dev), None))),
                      (df, dict(prior=torch.zeros(3, device=dev))), (df, dict(prior=torch.zeros(2, B, device=dev))), (df, dict(prior=torch.zeros(3, B, dtype=torch.int32, device=dev))),
                      (df, dict(prior=[0.0, 0.0, 0.0]))):
        with pytest.raises(ValueError):
            sim.pull_scan_match(field, **kw)
            print("accepted:", type(field).__name__, sorted(kw))      # reached only when nothing was raised
    torch.cuda.synchronize()
    assert all(torch.equal(x, t) for x, t in zip(snap, tensors))      # nothing ran
    assert sim.pull_scan_match(df, angles=ScanAngles(a.angles[:1], None), window=(0.0, 0.0)).window == (0, 0)      # the smallest search


def test_the_example_runs():
    """examples/localize_batch.py 2 3: map, spoil the pose, localise, in a process of its own."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "localize_batch.py"), "2", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    assert "error of the prior" in out.stdout and "error of the match" in out.stdout and "status [0, 0]" in out.stdout
