"""Mapping at a pose handed in, on the HIP path: smj_scan_to_map through the C-ABI and StretchBatchSimulator.pull_map_update.

One simulator for the module, the rig of tests/test_gpu_scanmatch.py: stretch_scene, three envs driven apart, 200 steps, the lidar on.
The scans fed to the entry are synthetic: ranges cast in fp64 in the room of tests/scanmatch_ref.py along the rays the rig's XPOSE
gives in the robot's frame, with NaN, -1, ranges below r_min, above r_max and +inf among them.  The kernel is compared in the two
stages of the reference (tests/mapping_ref.py): the cells of every ray against place_rays() (sure rays equal, unsure ones among their
candidates, at most 2 % unsure per env), and hit, miss and info against integrate() on the device's own cells, bit for bit.  The
closed loop -- smj_scan_to_pose, smj_scan_to_map gated by its status, pull_distance_field, likelihood -- runs on the device with the
asserts of tests/test_mapping_ref.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mapping_ref as ref
import occupancy_ref
import perception_rig
import scanmatch_ref
from conftest import ROOT
from perception_rig import B, DEV, Guarded, bare, dev as _dev, rig_scans as _rig_scans, stream as _stream  # noqa: F401 (bare: the module's fixture)

pytestmark = pytest.mark.gpu

K = 360
CELL = 0.05
FILL = -7
NaN, INF = float("nan"), float("inf")
FS = scanmatch_ref.FLOAT_STAGE
LIMITS = FS.limits
# (nx, ny, origin, cell): both float-stage grids (three bands; an odd per-env stride, so the 16-byte store groups start misaligned),
# one cell, and sixteen bands of one row each
GRIDS = [(128, 96, (-3.187, -2.379), CELL), (37, 29, (-0.913, -0.707), CELL), (1, 1, (-2.0, -2.0), 4.0), (4096, 16, (-102.4, -0.4), CELL)]


@pytest.fixture(scope="module")
def rig():
    r = perception_rig.scan_rig(K)
    r.prior = np.ascontiguousarray(FS.prior.T)                            # [3, B] fp32
    r.truth = np.ascontiguousarray(FS.truth.T.astype(np.float32))
    yield r
    r.sim.stop()


def _outputs(nx, ny, fill=FILL):
    return [torch.full((B, ny, nx), fill, dtype=torch.int32, device=DEV), torch.full((B, ny, nx), fill, dtype=torch.int32, device=DEV),
            torch.full((B, 4), fill, dtype=torch.int32, device=DEV), torch.full((B, K, 4), fill, dtype=torch.int32, device=DEV)]


def _map(r, scan, pose, nx, ny, origin, cell=CELL, *, gate=None, gate_ld=1, nrc=1, acc=0, out=None, miss=True, cells=True, limits=LIMITS, rc=0, ctx=None, frame=None,
         ld=None):
    """The C call on device tensors; returns [hit, miss, info, cells] (what they held where nothing is written).  gate: a tensor or a
    ctypes pointer."""
    if out is None:
        out = _outputs(nx, ny)
    ptr = perception_rig.ptr
    g = gate if gate is None or isinstance(gate, ctypes.c_void_p) else ptr(gate)
    got = r.L.smj_scan_to_map(ctx or r.sim._ctx, ptr(scan), scan.stride(0) if ld is None else ld, r.base if frame is None else frame, limits[0], limits[1], ptr(pose), g,
                              gate_ld, origin[0], origin[1], cell, nx, ny, nrc, acc, ptr(out[0]), ptr(out[1]) if miss else None, ptr(out[2]),
                              ptr(out[3]) if cells else None, _stream())
    assert got == rc, (got, r.L.smj_last_error(ctx or r.sim._ctx))
    return out


def _kinds(scan_host, limits, nrc):
    return np.stack([occupancy_ref.classify(scan_host[:, e].astype(np.float64), perception_rig.f32(limits[0]), perception_rig.f32(limits[1]), nrc)[0] for e in range(B)])


def _equal_integrate(tag, got, scan_host, pose, nx, ny, *, cells=None, gate=None, nrc=1, acc=0, before=None, miss=True, limits=LIMITS):
    """hit, miss and info of the device equal integrate() on the device's own cells (`cells` when the call wrote none), bit for bit."""
    torch.cuda.synchronize()
    hit, mis, info, own = (t.cpu().numpy() for t in got)
    cells = own if cells is None else cells
    status = ref.status_of(pose, gate)
    wh, wm, winfo = ref.integrate(cells, _kinds(scan_host, limits, nrc), status, nx, ny, None if before is None else before[0], None if before is None else before[1], bool(acc))
    assert np.array_equal(info, winfo), (tag, info.tolist(), winfo.tolist())
    assert np.array_equal(hit, wh), (tag, "hit", int((hit != wh).sum()), np.argwhere(hit != wh)[:5].tolist())
    if miss:
        assert np.array_equal(mis, wm), (tag, "miss", int((mis != wm).sum()), np.argwhere(mis != wm)[:5].tolist())
    return winfo


@pytest.mark.parametrize("which", ["prior", "truth"])
@pytest.mark.parametrize("nx,ny,origin", FS.grids)
def test_float_stage_cells_against_the_reference_with_a_cap(rig, nx, ny, origin, which):
    r = rig
    pose = getattr(r, which)
    got = _map(r, r.scan, _dev(pose), nx, ny, origin)
    torch.cuda.synchronize()
    cells = got[3].cpu().numpy()
    for e in range(B):
        pl = ref.place_rays(*r.geoms[e], r.scan_host[:, e].astype(np.float64), pose[:, e], origin[0], origin[1], CELL, *LIMITS, 1)
        share = ref.unsure_share(pl)
        print(f"{nx} x {ny} {which} env {e}: kept {int(pl.kept.sum())}, returns {int((pl.kind == ref.RETURN).sum())}, unsure share {share}")
        assert pl.origin_sure.all() and share <= ref.MAX_AMBIGUOUS, (e, share)
        bad = ref.check_cells(cells[e], pl)
        assert not bad, (e, len(bad), bad[:5])
        assert (pl.kind == ref.RETURN).sum() >= 200 and (pl.kind == ref.CLEAR).sum() > 10 and (pl.kind == ref.DROP).sum() > 5
    winfo = _equal_integrate("float stage", got, r.scan_host, pose, nx, ny)
    assert (winfo[:, 0] == ref.OK).all() and (winfo[:, 1] >= 200).all() and (winfo[:, 2] > 10).all() and (winfo[:, 3] == 0).all()


@pytest.mark.parametrize("miss,cells,acc,nrc", [(True, True, 0, 1), (False, True, 1, 0), (True, False, 1, 1), (False, False, 0, 0)])
@pytest.mark.parametrize("nx,ny,origin,cell", GRIDS)
def test_integer_stage_equals_the_reference(rig, nx, ny, origin, cell, miss, cells, acc, nrc):
    r = rig
    pose = _dev(r.prior)
    full = _map(r, r.scan, pose, nx, ny, origin, cell, nrc=nrc)      # the device's cells, for the calls that write none
    torch.cuda.synchronize()
    own = full[3].cpu().numpy()
    rng = np.random.default_rng(nx + acc)
    before = [rng.integers(0, 1000, (B, ny, nx)).astype(np.int32) for _ in range(2)] if acc else [np.full((B, ny, nx), FILL, np.int32)] * 2
    out = [_dev(before[0]), _dev(before[1]), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV), torch.full((B, K, 4), FILL, dtype=torch.int32, device=DEV)]
    got = _map(r, r.scan, pose, nx, ny, origin, cell, nrc=nrc, acc=acc, out=out, miss=miss, cells=cells)
    winfo = _equal_integrate((nx, ny, miss, cells, acc, nrc), got, r.scan_host, r.prior, nx, ny, cells=own, nrc=nrc, acc=acc, before=before, miss=miss)
    if not miss:
        assert np.array_equal(got[1].cpu().numpy(), before[1])      # a null miss layer is left untouched
    assert torch.equal(got[3], full[3]) if cells else int((got[3] != FILL).sum()) == 0
    print(f"{nx} x {ny} miss {miss} cells {cells} accumulate {acc} clears {nrc}: info {winfo.tolist()}, hits {int(got[0].sum()) - (int(before[0].sum()) if acc else 0)}")
    assert (winfo[:, 0] == ref.OK).all() and (winfo[:, 1] >= 200).all() and ((winfo[:, 2] > 10).all() if nrc else (winfo[:, 2] == 0).all())


def test_a_pose_far_off_the_grid_touches_no_cell_and_nothing_out_of_bounds(rig):
    """3 km off: every ray is kept (the origin's index stays within 2^20) and every cell skipped; with the origin beyond 2^20 cells
    every ray is dropped by the guard.  The outputs sit in guarded buffers, 4 bytes past a 16-byte boundary."""
    r = rig
    nx, ny, origin = 37, 29, (-0.913, -0.707)
    far = r.prior.copy()
    far[0] += 3000.0
    far[1] -= 3000.0
    beyond = r.prior.copy()
    beyond[0, :] = 60000.0      # 1.2 million cells
    for pose, kept in ((far, True), (beyond, False)):
        hit, miss = Guarded(37, ny, nx), Guarded(37, ny, nx)
        info, cells = torch.full((B, 4), FILL, dtype=torch.int32, device=DEV), torch.full((B, K, 4), FILL, dtype=torch.int32, device=DEV)
        got = _map(r, r.scan, _dev(pose), nx, ny, origin, out=[hit.view, miss.view, info, cells])
        winfo = _equal_integrate(("far", kept), got, r.scan_host, pose, nx, ny)
        zero = torch.zeros(B, ny, nx, dtype=torch.int32, device=DEV)
        hit.check(zero)
        miss.check(zero)
        assert (winfo[:, 0] == ref.OK).all()
        if kept:
            assert (winfo[:, 1] >= 200).all() and (winfo[:, 3] == 0).all() and int((cells == ref.NO_CELL).sum()) == 4 * int((_kinds(r.scan_host, LIMITS, 1) == ref.DROP).sum())
        else:
            assert (winfo[:, 1:3] == 0).all() and (winfo[:, 3] >= 210).all() and bool((cells == ref.NO_CELL).all())


def test_gate_and_status(rig):
    """A gate of [0, 1, 0] and a theta that is not finite in env 2: env 0 alone is integrated.  The others keep their bits under
    accumulate and are zero without it; their info is (status, 0, 0, 0) and their cells NO_CELL."""
    r = rig
    nx, ny, origin = 128, 96, (-3.187, -2.379)
    pose = r.prior.copy()
    pose[2, 2] = INF
    gate = np.array([0, 1, 0], np.int32)
    rng = np.random.default_rng(3)
    before = [rng.integers(0, 1000, (B, ny, nx)).astype(np.int32) for _ in range(2)]
    for acc in (1, 0):
        out = [_dev(before[0]), _dev(before[1]), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV), torch.full((B, K, 4), FILL, dtype=torch.int32, device=DEV)]
        got = _map(r, r.scan, _dev(pose), nx, ny, origin, gate=_dev(gate), acc=acc, out=out)
        winfo = _equal_integrate(("gate", acc), got, r.scan_host, pose, nx, ny, gate=gate, acc=acc, before=before)
        assert winfo[:, 0].tolist() == [ref.OK, ref.GATED, ref.OFF] and winfo[1:, 1:].tolist() == [[0, 0, 0]] * 2 and winfo[0, 1] >= 200
        for e in (1, 2):
            want = before if acc else [np.zeros_like(before[0])] * 2
            assert np.array_equal(got[0][e].cpu().numpy(), want[0][e]) and np.array_equal(got[1][e].cpu().numpy(), want[1][e])
        assert bool((got[3][1:] == ref.NO_CELL).all()) and bool((got[3][0] != ref.NO_CELL).any())
        assert int(got[0][0].sum()) > int(before[0][0].sum()) * acc
    # a pose that is not finite comes before the gate, whatever the gate's word; any word but 0 gates
    got = _map(r, r.scan, _dev(pose), nx, ny, origin, gate=_dev(np.array([-1, 1 << 30, 5], np.int32)))
    torch.cuda.synchronize()
    assert got[2][:, 0].tolist() == [ref.GATED, ref.GATED, ref.OFF] and int(got[0].abs().max()) == 0 and int(got[1].abs().max()) == 0


def test_the_matchers_status_gates_where_it_lies(rig):
    """best + 3 with gate_ld = 4 from a real smj_scan_to_pose call (env 1 has too few returns for its min_points, env 2 a prior that
    is not finite) equals the status column copied to a contiguous tensor."""
    r = rig
    nx, ny, origin = 128, 96, (-3.187, -2.379)
    scan = r.scan_host.copy()
    scan[20:, 1] = -1.0
    prior = r.prior.copy()
    prior[0, 2] = NaN
    field = _dev(np.full((B, ny, nx), 200, np.uint8))
    pose_out, best = torch.zeros(3, B, device=DEV), torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    ptr = perception_rig.ptr
    scan_d, prior_d, angles_d = _dev(scan), _dev(prior), _dev(np.zeros(1, np.float32))      # held: a temporary's memory may be handed out again before the launch
    rc = r.L.smj_scan_to_pose(r.sim._ctx, ptr(scan_d), B, r.base, LIMITS[0], LIMITS[1], ptr(field), nx, ny, origin[0], origin[1], CELL, ptr(prior_d),
                              ptr(angles_d), None, 1, 1, 1, 0, 30, ptr(pose_out), ptr(best), None, None, _stream())
    assert rc == 0, r.L.smj_last_error(r.sim._ctx)
    torch.cuda.synchronize()
    assert best[:, 3].tolist() == [scanmatch_ref.OK, scanmatch_ref.FEW, scanmatch_ref.OFF]
    in_place = _map(r, scan_d, pose_out, nx, ny, origin, gate=ctypes.c_void_p(best.data_ptr() + 12), gate_ld=4)
    copied = _map(r, scan_d, pose_out, nx, ny, origin, gate=best[:, 3].contiguous())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(in_place, copied))
    assert in_place[2][:, 0].tolist() == [ref.OK, ref.GATED, ref.OFF] and int(in_place[0][0].sum()) >= 200 and int(in_place[0][1:].abs().max()) == 0
    assert best[:, 3].tolist() == [scanmatch_ref.OK, scanmatch_ref.FEW, scanmatch_ref.OFF]      # the gate is an input


def test_a_padded_scan_gives_the_packed_calls_bits(rig):
    """lidar_ld > num_envs, odd: the scan inside a store of canaries, which stay as they are."""
    r = rig
    nx, ny, origin = 37, 29, (-0.913, -0.707)
    packed = _map(r, r.scan, _dev(r.prior), nx, ny, origin)
    canary = torch.tensor([0x7FC0BEEF], dtype=torch.int32).view(torch.float32).item()
    ld = B + 4
    store = torch.full((K + 2, ld), canary, dtype=torch.float32, device=DEV)
    store[1:K + 1, :B] = r.scan
    padded = _map(r, store[1:K + 1], _dev(r.prior), nx, ny, origin, ld=ld)
    torch.cuda.synchronize()
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(packed, padded))
    bits = store.view(torch.int32)
    assert bool((bits[0] == 0x7FC0BEEF).all()) and bool((bits[K + 1] == 0x7FC0BEEF).all()) and bool((bits[:, B:] == 0x7FC0BEEF).all())
    assert store[1:K + 1, :B].cpu().numpy().tobytes() == r.scan.cpu().numpy().tobytes()


def test_end_cells_agree_with_the_matcher(rig):
    """smj_scan_to_pose with the rotation table [0]: for every ray that scanmatch_ref.place calls sure and placed, (bx, by) equals
    the matcher's cell.  The two kernels may contract the transform differently, so unsure points are exempt."""
    r = rig
    ptr = perception_rig.ptr
    for nx, ny, origin in FS.grids:
        field = _dev(np.zeros((B, ny, nx), np.uint8))
        angles = np.zeros(1, np.float32)
        pose_out, best = torch.zeros(3, B, device=DEV), torch.zeros(B, 4, dtype=torch.int32, device=DEV)
        mcells = torch.full((B, 1, K, 2), FILL, dtype=torch.int32, device=DEV)
        prior_d, angles_d = _dev(r.prior), _dev(angles)      # held: a temporary's memory may be handed out again before the launch
        rc = r.L.smj_scan_to_pose(r.sim._ctx, ptr(r.scan), B, r.base, LIMITS[0], LIMITS[1], ptr(field), nx, ny, origin[0], origin[1], CELL, ptr(prior_d),
                                  ptr(angles_d), None, 1, 0, 0, 0, 1, ptr(pose_out), ptr(best), None, ptr(mcells), _stream())
        assert rc == 0, r.L.smj_last_error(r.sim._ctx)
        got = _map(r, r.scan, prior_d, nx, ny, origin, nrc=0)
        torch.cuda.synchronize()
        pl = scanmatch_ref.place(r.pts, r.mar, r.prior, angles, origin[0], origin[1], CELL, nx, ny)
        judged = pl.sure[:, 0] & (pl.cell[:, 0, :, 0] != scanmatch_ref.NO_CELL)
        ends, theirs = got[3].cpu().numpy()[:, :, 2:], mcells.cpu().numpy()[:, 0]
        print(f"{nx} x {ny}: sure and placed {judged.sum(1).tolist()} of {K}")
        assert (judged.sum(1) >= 150).all()
        assert np.array_equal(ends[judged], theirs[judged]), np.argwhere((ends != theirs).any(-1) & judged)[:5].tolist()
        assert np.array_equal(ends[judged], pl.cell[:, 0][judged])


def test_two_calls_give_identical_bytes(rig):
    r = rig
    nx, ny, origin = 128, 96, (-3.187, -2.379)
    rng = np.random.default_rng(8)
    before = [rng.integers(0, 50, (B, ny, nx)).astype(np.int32) for _ in range(2)]
    runs = []
    for _ in range(2):
        out = [_dev(before[0]), _dev(before[1]), torch.full((B, 4), FILL, dtype=torch.int32, device=DEV), torch.full((B, K, 4), FILL, dtype=torch.int32, device=DEV)]
        runs.append(_map(r, r.scan, _dev(r.prior), nx, ny, origin, acc=1, out=out, gate=_dev(np.array([0, 0, 3], np.int32))))
    torch.cuda.synchronize()
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(*runs))
    assert int(runs[0][0].sum()) > int(before[0].sum())


def test_error_codes_and_a_refused_call_writes_nothing(rig, bare):
    r = rig
    L, sim = r.L, r.sim
    nx = ny = 32
    nbody = sim.xpose.shape[0] // 12
    cells = B * nx * ny
    sizes = dict(scan=K * B, pose=3 * B, gate=4 * B, hit=cells, miss=cells, info=4 * B, cell=B * K * 4)
    pool = torch.zeros(sum(sizes.values()) + 64, dtype=torch.int32, device=DEV)      # one allocation, so that ranges can be made to overlap
    at, p = {}, pool.data_ptr()
    for name, words in sizes.items():
        at[name] = p
        p += 4 * ((words + 3) // 4 * 4)      # every range starts on a 16-byte boundary
    good = dict(ld=B, frame=r.base, r_min=0.2, r_max=5.0, gate_ld=4, x0=-0.81, y0=-0.81, cell=0.05, nx=nx, ny=ny, nrc=1, acc=0)
    sent = perception_rig.sentinels(ny, nx)      # the rig's sentinel pair: outputs of calls that are refused for another reason

    def call(a, ctx=None, **ptrs):
        q = dict(at, **ptrs)
        vp = lambda v: ctypes.c_void_p(v) if v else None
        return L.smj_scan_to_map(ctx or sim._ctx, vp(q["scan"]), a["ld"], a["frame"], a["r_min"], a["r_max"], vp(q["pose"]), vp(q["gate"]), a["gate_ld"], a["x0"], a["y0"],
                                 a["cell"], a["nx"], a["ny"], a["nrc"], a["acc"], vp(q["hit"]), vp(q["miss"]), vp(q["info"]), vp(q["cell"]), _stream())

    bad = [dict(ld=B - 1), dict(ld=0), dict(ld=-5), dict(gate_ld=0), dict(gate_ld=-4), dict(nx=0), dict(ny=0), dict(nx=-4), dict(ny=-1), dict(nx=257, ny=256), dict(nx=256, ny=257),
           dict(nx=65537, ny=1), dict(nx=1 << 20, ny=1 << 20), dict(cell=0.0), dict(cell=-0.05), dict(cell=NaN), dict(cell=INF), dict(x0=NaN), dict(x0=INF), dict(y0=-INF),
           dict(y0=NaN), dict(r_min=NaN), dict(r_max=NaN), dict(r_max=INF), dict(r_min=-0.1), dict(r_min=-INF), dict(r_min=5.5), dict(r_max=0.1), dict(cell=0.0005, r_max=4.2),
           dict(cell=1e-3, r_max=8.5), dict(frame=r.lib.FRAME_WORLD), dict(frame=r.lib.FRAME_CAMERA), dict(frame=-3), dict(frame=10 ** 6), dict(frame=nbody)]
    for change in bad:
        for outs in ({}, dict(hit=sent[0].data_ptr(), miss=sent[1].data_ptr())):
            rc = call(dict(good, **change), **outs)
            assert rc == -1 and L.smj_last_error(sim._ctx), (change, rc)
    for name in ("scan", "pose", "hit", "info"):      # null required pointers
        assert call(good, **{name: None}) == -1, name
    for name, by in (("scan", 2), ("pose", 1), ("gate", 3), ("hit", 2), ("miss", 1), ("info", 2), ("cell", 3)):
        assert call(good, **{name: at[name] + by}) == -1 and b"aligned" in L.smj_last_error(sim._ctx), (name, by)
    # overlap: an output on an input, on another output, on the bound XPOSE array, by a whole range and by one word at either end
    last = lambda name: 4 * (sizes[name] - 1)
    gate_last = 4 * (4 * (B - 1))      # the gate's range ends with the word of the last env
    for kw in (dict(hit=at["scan"]), dict(hit=at["pose"]), dict(hit=at["gate"]), dict(miss=at["scan"]), dict(info=at["pose"]), dict(cell=at["gate"]), dict(miss=at["hit"]),
               dict(info=at["hit"]), dict(cell=at["miss"]), dict(cell=at["info"]), dict(hit=at["scan"] + last("scan")), dict(hit=at["pose"] - last("hit")),
               dict(hit=at["gate"] + gate_last), dict(info=at["gate"] + gate_last), dict(info=at["gate"] - last("info")), dict(miss=at["hit"] + last("hit")),
               dict(cell=at["hit"] - last("cell")), dict(pose=at["cell"] + last("cell")), dict(gate=at["info"] - gate_last), dict(scan=at["miss"] - last("scan")),
               dict(hit=sim.xpose.data_ptr()), dict(info=sim.xpose.data_ptr() + 4 * (sim.xpose.numel() - 1))):
        assert call(good, **kw) == -1 and b"overlap" in L.smj_last_error(sim._ctx), kw
    xpose_before = sim.xpose.clone()
    torch.cuda.synchronize()
    assert int(pool.abs().max()) == 0 and bool((sent[0] == FILL).all()) and bool((sent[1] == FILL).all())      # a refused call writes nothing
    # a bare context (nothing bound): -5, after every -1
    assert call(good, ctx=bare.ctx) == -5 and b"XPOSE" in L.smj_last_error(bare.ctx)
    assert call(dict(good, gate_ld=0), ctx=bare.ctx) == -1 and call(dict(good, frame=nbody), ctx=bare.ctx) == -1
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
            assert call(dict(good, gate_ld=0), ctx=ctx) == -6      # -6 comes first
        finally:
            L.smj_destroy(ctx)
    torch.cuda.synchronize()
    assert int(pool.abs().max()) == 0 and torch.equal(sim.xpose, xpose_before)
    # accepted: the extremes of every argument, null optional pointers, adjacent ranges, a gate as best_dev + 3 of the matcher lies (the
    # word of its last env is the last word before the hit layer), the last body as the frame
    for change, ptrs in ((dict(r_min=0.0, r_max=0.0), {}), (dict(cell=0.0009765625, r_max=8.0), {}), (dict(cell=1e-30, x0=-3e38, y0=3e38, r_min=0.0, r_max=1e-27), dict(gate=None, miss=None, cell=None)),
                         (dict(frame=nbody - 1), {}), (dict(gate_ld=4), dict(gate=at["gate"] + 12)), (dict(gate_ld=1), {}), (dict(nx=1, ny=1), {}), ({}, {})):
        assert call(dict(good, **change), **ptrs) == 0, (change, L.smj_last_error(sim._ctx))
    torch.cuda.synchronize()
    words = lambda name: pool[(at[name] - pool.data_ptr()) // 4:][:sizes[name]]
    # all-zero inputs: every range 0 is below r_min (or a return of length 0 with r_min = 0), the pose (0, 0, 0), the gate open
    assert words("info").view(B, 4)[:, 0].tolist() == [ref.OK] * B
    assert all(int(words(name).abs().max()) == 0 for name in ("scan", "pose", "gate"))      # the inputs are unchanged


def test_the_loop_closes_on_the_device(rig):
    """The closed loop of tests/test_mapping_ref.py through the C-ABI, three envs with a bias each: smj_scan_to_pose, smj_scan_to_map
    gated by `best`, pull_distance_field of the map, likelihood(0.10), again.  Nothing is read back inside the loop but for the
    asserts' bookkeeping after it."""
    from stretch_mujoco_amd.datamodels import StatusStretchOccupancyGrid
    from stretch_mujoco_amd.utils import scan_angles

    r = rig
    sim, L, ptr = r.sim, r.L, perception_rig.ptr
    g, W, step = scanmatch_ref.ROOM_GRID, scanmatch_ref.ROOM_WINDOW, scanmatch_ref.ROOM_STEP
    nx, ny, origin = g.nx, g.ny, g.origin
    angles = scan_angles(window=2 * W * step, step=step).angles.to(DEV)
    assert angles.shape == (21,)
    sign = np.array([(1, 1, 1), (-1, -1, -1), (-1, 1, -1)], np.float64)      # per env its own bias
    bias = sign * ref.LOOP_BIAS
    truth = ref.LOOP_POSES
    scans = [_dev(_rig_scans(r, np.repeat(truth[i][None], B, 0))) for i in range(len(truth))]
    new_maps = lambda: [torch.zeros(B, ny, nx, dtype=torch.int32, device=DEV) for _ in range(2)]
    info = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    loop, dead, true_map = new_maps(), new_maps(), new_maps()

    def add(maps, scan, pose, gate=None):
        _map(r, scan, pose, nx, ny, origin, gate=gate, gate_ld=4, acc=1, out=[maps[0], maps[1], info, None], cells=False)

    start = _dev(np.repeat(truth[0][:, None], B, 1).astype(np.float32))
    for maps in (loop, dead, true_map):
        add(maps, scans[0], start)
    est, dr = start.clone(), np.repeat(truth[0][:, None], B, 1)
    pose_out, best = torch.zeros(3, B, device=DEV), torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    estimates, statuses, infos = [], [], []
    for i in range(1, len(truth)):
        inc = (truth[i] - truth[i - 1])[:, None] + bias.T                      # [3, B]
        prior = (est.double() + _dev(inc)).float().contiguous()
        dr = dr + inc
        df = sim.pull_distance_field(StatusStretchOccupancyGrid(time=None, hit=loop[0], miss=loop[1], origin=origin, cell=g.cell, frame="world"))
        field = df.likelihood(ref.LOOP_SIGMA).contiguous()
        rc = L.smj_scan_to_pose(sim._ctx, ptr(scans[i]), B, r.base, ref.LOOP_LIMITS[0], ref.LOOP_LIMITS[1], ptr(field), nx, ny, origin[0], origin[1], g.cell, ptr(prior),
                                ptr(angles), None, 21, W, W, 0, 30, ptr(pose_out), ptr(best), None, None, _stream())
        assert rc == 0, L.smj_last_error(sim._ctx)
        add(loop, scans[i], pose_out, gate=ctypes.c_void_p(best.data_ptr() + 12))
        est = pose_out.clone()
        estimates.append(est)
        statuses.append(best[:, 3].clone())
        infos.append(info.clone())
        add(dead, scans[i], _dev(dr.astype(np.float32)))
        add(true_map, scans[i], _dev(np.repeat(truth[i][:, None], B, 1).astype(np.float32)))
    torch.cuda.synchronize()
    assert all(s.tolist() == [scanmatch_ref.OK] * B for s in statuses)
    assert all(v[:, 0].tolist() == [ref.OK] * B and bool((v[:, 1] >= 200).all()) for v in infos)
    errors = np.array([[ref.lattice_error(estimates[i - 1][:, e].cpu().numpy(), truth[i], g.cell, step) for e in range(B)] for i in range(1, len(truth))])
    dr_errors = [np.round(ref.lattice_error(dr[:, e], truth[-1], g.cell, step), 1).tolist() for e in range(B)]
    worst = []
    for e in range(B):
        truth_dist2 = scanmatch_ref.dist2_of(true_map[0][e].cpu().numpy() > 0)
        worst.append((ref.worst_dist2(loop[0][e].cpu().numpy(), truth_dist2), ref.worst_dist2(dead[0][e].cpu().numpy(), truth_dist2)))
    print(f"worst error per env in lattice steps {np.abs(errors).max((0, 2)).tolist()} (dead reckoning ends {dr_errors} off); worst squared distance to the "
          f"truth-pose map (loop, dead reckoning) per env {worst}")
    assert ref.within_one_step(errors), np.round(errors, 3).tolist()
    assert all(w[0] <= ref.LOOP_MAX_DIST2 for w in worst), worst
    assert all(w[1] > ref.LOOP_DEAD_RECKONING for w in worst), worst


def test_pull_map_update(rig):
    """pull_map_update equals the C call at the same arguments; its grid goes through pull_distance_field and pull_scan_match
    unchanged; gate=match equals gate=match.status."""
    from stretch_mujoco_amd.datamodels import StatusStretchMapUpdate, StatusStretchOccupancyGrid

    r = rig
    sim = r.sim
    scan = sim.lidar[:K].clone()
    pose = sim.base_pose.clone()
    up = sim.pull_map_update(pose, shape=(96, 128), origin=(-3.187, -2.379), accumulate=False, cells=True)
    assert isinstance(up, StatusStretchMapUpdate) and isinstance(up.grid, StatusStretchOccupancyGrid) and up.grid.frame == "world"
    assert up.grid.origin == (-3.187, -2.379) and up.grid.cell == CELL and tuple(up.grid.hit.shape) == (B, 96, 128) and tuple(up.cells.shape) == (B, K, 4)
    want = _map(r, scan, pose, 128, 96, (-3.187, -2.379))
    torch.cuda.synchronize()
    assert torch.equal(up.grid.hit, want[0]) and torch.equal(up.grid.miss, want[1]) and torch.equal(up.info, want[2]) and torch.equal(up.cells, want[3])
    assert up.integrated().tolist() == [True] * B and up.gated().tolist() == [False] * B and up.status.tolist() == [0] * B and bool((up.returns() >= 50).all())
    assert int(up.grid.hit.sum()) > 100
    # accumulate is the default: the same scan again doubles the map; the simulator's own buffers are those of the first call
    twice = sim.pull_map_update(pose, shape=(96, 128), origin=(-3.187, -2.379))
    assert twice.cells is None and twice.grid.hit.data_ptr() == up.grid.hit.data_ptr() and torch.equal(twice.grid.hit, 2 * want[0])
    # the map goes into the pulls after it as it is, and a match gates where it lies
    df = sim.pull_distance_field(twice.grid)
    match = sim.pull_scan_match(twice.grid, pose)
    assert df.frame == "world" and match.frame == "world" and match.ok().all()
    og = sim.pull_occupancy_grid(frame="world", shape=(64, 64), origin=(-1.6, -1.6))      # the first scan mapped by the simulator's own pose
    keep = [og.hit.clone(), og.miss.clone()]
    match.best[1, 3] = 1      # as if env 1 had too few returns
    a = sim.pull_map_update(match.pose, og, gate=match, cells=True)
    got = [t.clone() for t in (a.grid.hit, a.grid.miss, a.info, a.cells)]
    assert a.grid.hit.data_ptr() == og.hit.data_ptr() and a.grid.origin == og.origin and a.grid.frame == "world" and a.status.tolist() == [0, 1, 0]
    og.hit.copy_(keep[0])
    og.miss.copy_(keep[1])
    b = sim.pull_map_update(match.pose, og, gate=match.status.contiguous(), cells=True)
    assert all(torch.equal(x, y) for x, y in zip(got, (b.grid.hit, b.grid.miss, b.info, b.cells)))
    assert torch.equal(b.grid.hit[1], keep[0][1]) and int(b.grid.hit[0].sum()) > int(keep[0][0].sum()) and b.gated().tolist() == [False, True, False]
    assert sim.pull_frontiers(b.grid) is not None and sim.pull_navigation_field((0.5, 0.0), sim.pull_distance_field(b.grid)) is not None


def test_value_errors_are_raised_before_any_launch(rig):
    from stretch_mujoco_amd.datamodels import StatusStretchOccupancyGrid, StatusStretchScanMatch

    sim = rig.sim
    dev = sim.device
    pose = sim.base_pose.clone()
    keep = sim.pull_map_update(pose, cells=True)
    og = sim.pull_occupancy_grid(frame="world")
    torch.cuda.synchronize()
    tensors = (keep.grid.hit, keep.grid.miss, keep.info, keep.cells, og.hit, og.miss)
    snap = [t.clone() for t in tensors]
    odd = lambda **kw: StatusStretchOccupancyGrid(**dict(dict(time=0, hit=og.hit, miss=og.miss, origin=og.origin, cell=og.cell, frame="world"), **kw))
    match = lambda best: StatusStretchScanMatch(time=0, pose=pose, best=best, score=None, cells=None, angles=None, window=(0, 0), origin=(0, 0), cell=CELL, frame="world")
    for p, kw in (("pose", {}), (pose[:2], {}), (pose.reshape(B, 3)[:, :2], {}), (pose.to(torch.int32), {}), (pose.cpu(), {}), ([0.0, 0.0, 0.0], {}),
                  (pose, dict(grid=og.hit)), (pose, dict(grid=odd(frame="base"))), (pose, dict(grid=odd(frame="odom"))), (pose, dict(grid=odd(hit=og.hit.to(torch.int64)))),
                  (pose, dict(grid=odd(hit=og.hit[:2]))), (pose, dict(grid=odd(miss=og.miss[:, :5]))), (pose, dict(grid=odd(hit=og.hit.cpu()))), (pose, dict(grid=odd(hit=None))),
                  (pose, dict(grid=odd(cell=0.0))), (pose, dict(grid=odd(cell=NaN))), (pose, dict(grid=odd(hit=og.hit.transpose(1, 2)))),
                  (pose, dict(shape=(0, 4))), (pose, dict(shape=(300, 300))), (pose, dict(shape=5)), (pose, dict(cell=0.0)), (pose, dict(cell=-1.0)), (pose, dict(origin=(0.0, NaN))),
                  (pose, dict(origin=(0.0,))), (pose, dict(range_limits=(0.2,))), (pose, dict(range_limits=(-0.1, 5.0))), (pose, dict(range_limits=(5.0, 0.2))),
                  (pose, dict(range_limits=(0.2, INF))), (pose, dict(range_limits=(0.2, 500.0))),
                  (pose, dict(gate="ok")), (pose, dict(gate=[0, 0, 0])), (pose, dict(gate=torch.zeros(B, device=dev))), (pose, dict(gate=torch.zeros(B + 1, dtype=torch.int32, device=dev))),
                  (pose, dict(gate=torch.zeros(B, dtype=torch.int32))), (pose, dict(gate=torch.zeros(B, 1, dtype=torch.int32, device=dev))),
                  (pose, dict(gate=match(torch.zeros(B, 3, dtype=torch.int32, device=dev)))), (pose, dict(gate=match(torch.zeros(B, 4, dtype=torch.int64, device=dev)))),
                  (pose, dict(gate=match(torch.zeros(B, 8, dtype=torch.int32, device=dev)[:, ::2]))), (pose, dict(gate=match(None)))):
        with pytest.raises(ValueError):
            sim.pull_map_update(p, **kw)
            print("accepted:", type(p).__name__, sorted(kw))      # reached only when nothing was raised
    torch.cuda.synchronize()
    assert all(torch.equal(x, t) for x, t in zip(snap, tensors))      # nothing ran
    # accepted: fp64 poses (converted), a gate that is a strided view, no miss layer in the grid
    up = sim.pull_map_update(pose.double(), odd(miss=None), gate=torch.zeros(B, 2, dtype=torch.int32, device=dev)[:, 0])
    assert up.grid.miss is None and up.integrated().all()


def test_the_example_runs():
    """examples/slam_batch.py 2 6: map and localise at once, in a process of its own; the loop ends nearer the simulator's pose than
    dead reckoning does, in position and in heading."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "slam_batch.py"), "2", "6"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    assert "status of the last match [0, 0]" in out.stdout and "legs gated [0, 0]" in out.stdout
    rows = {name: [tuple(float(v) for v in m) for m in re.findall(r"\(([\d.]+) cm, ([\d.]+) cm, ([\d.]+) deg\)", line)]
            for name, line in re.findall(r"^error of (dead reckoning|the loop)\s+(.*)$", out.stdout, flags=re.M)}
    assert len(rows["dead reckoning"]) == len(rows["the loop"]) == 2
    for dead, loop in zip(rows["dead reckoning"], rows["the loop"]):
        assert np.hypot(loop[0], loop[1]) < np.hypot(dead[0], dead[1]) and loop[2] < dead[2], (dead, loop)
