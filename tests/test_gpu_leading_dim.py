"""The leading dimension of the C-ABI's batch-major slots on the device (include/smj.h: "[dim][ld], ld >= num_envs").  Every test runs
the same calls on two contexts of one blob through tests/capi_rig.py -- a packed one (ld = B) and a padded one (ld = B + pad, every slot
inside a canary-filled store with guard rows) -- with identical inputs.  `ld` changes addresses and no arithmetic, so after EVERY call the
padded context holds the packed one's bits in every slot (same_bits) and not one padding or guard word of either has been written
(assert_padding_untouched).  The packed results themselves are held to the fp64 oracle by the rest of the suite.  Every comparison is
bit equality.  pollers = 0 throughout: with pollers the rounding of a handed-over env depends on timing (tests/test_gpu_parity.py).
The CPU leg is tests/test_emul_leading_dim.py; the comparators prove that they can fail in tests/test_capi_rig.py."""
import contextlib
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import stretch_mujoco_amd.model_blob as mb
from capi_rig import CANARY_F32_BITS, CapiRig, envs_all_differ, same_bits
from conftest import MIX_CTRL, MODELS, home_qpos
from perception_rig import POSES, ptr
from stretch_mujoco_amd import lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(3, 1), (65, 3), (130, 62)]   # odd 4-byte row offsets | two 64-env staging tiles + a tail env, odd stride | three tiles, ld = the packed stride of another batch
SENSORS = ("GYRO", "ACCEL", "LIDAR", "XPOSE", "BASECTL")
READ_ALL = lib.READ_IMU | lib.READ_LIDAR | lib.READ_POSES
NEWTON, PGS = 2, 0
DROP_CTRL = [0, 0, 0.0, 0.3, 0, -1.57, 0, 0, 0, 0]   # tests/test_gpu_parity.py: lift to the floor, wrist pitched down, from qpos0
# the library is built with fp32 division that is not correctly rounded: x / c for a constant c is x * fl(1 / c)
WHEEL_RADIUS, WHEEL_SEPARATION, BASE_X_VEL, BASE_R_VEL = np.float32(0.0508), np.float32(0.3153), np.float32(0.3), np.float32(1.0)   # csrc/smj_model.h


@functools.lru_cache(None)
def _model(name):
    with open(os.path.join(MODELS, name + ".smjb"), "rb") as f:
        m = mb.loads(f.read())
    names = json.loads(mb.get_str(m, "names_json"))
    adr = np.asarray(m["jnt_qposadr"]).reshape(-1)
    return m, {n: int(adr[i]) for i, n in enumerate(names["joint"])}, {n: i for i, n in enumerate(names["actuator"])}, names


def _inputs(model, B):
    """Per env another base x, y, yaw, lift, arm, wrist pitch, head pan / tilt, ctrl and base move (BASECTL modes 0 .. 3): no two envs
    share a column.  Returns numpy fp32 (qpos [nq, B], ctrl [nu, B], bctl [8, B])."""
    m, jq, act, _ = _model(model)
    e = np.arange(B, dtype=np.float64)
    q = np.repeat(home_qpos(m["qpos0"])[:, None], B, 1)
    if model.startswith("stretch_scene"):   # the free poses of tests/perception_rig.py
        assert B == len(POSES)
        x, y, yaw = (np.array([p[k] for p in POSES]) for k in range(3))
    else:
        x, y, yaw = 0.05 * e, -0.03 * e, 0.02 * e - 1.0
    q[0], q[1], q[3], q[4], q[5], q[6] = x, y, np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)
    q[jq["joint_lift"]] = 0.3 + 0.003 * e
    for k in range(4):
        q[jq[f"joint_arm_l{k}"]] = 0.01 + 0.0001 * e
    q[jq["joint_wrist_pitch"]] = -0.8 + 0.003 * e
    q[jq["joint_head_pan"]] = -0.5 + 0.01 * e
    q[jq["joint_head_tilt"]] = -0.6 + 0.002 * e
    s = 0.4 + 0.6 * e / B
    u = np.asarray(MIX_CTRL, np.float64)[:, None] * s
    u[act["lift"]] = q[jq["joint_lift"]] + 0.05
    u[act["arm"]] = 4 * q[jq["joint_arm_l0"]] + 0.02
    u[act["wrist_pitch"]], u[act["head_pan"]], u[act["head_tilt"]] = q[jq["joint_wrist_pitch"]], q[jq["joint_head_pan"]], q[jq["joint_head_tilt"]]
    bc = np.zeros((8, B))
    bc[0] = np.arange(B) % 4
    bc[1], bc[2], bc[3] = x, y, yaw
    bc[4] = np.where(np.arange(B) % 8 < 4, 0.3, -0.4)
    bc[5], bc[6] = 0.05 + 0.001 * e, 0.1 - 0.002 * e
    return q.astype(np.float32), u.astype(np.float32), bc.astype(np.float32)


def _upload(r, model, q=None, u=None, bc=None):
    q0, u0, bc0 = _inputs(model, r.B)
    r["QPOS"][:] = torch.tensor(q0 if q is None else q, device=DEV)
    r["CTRL"][:] = torch.tensor(u0 if u is None else u, device=DEV)
    if "BASECTL" in r.stores:
        r["BASECTL"][:] = torch.tensor(bc0 if bc is None else bc, device=DEV)


@contextlib.contextmanager
def _rigs(model, B, pads, optional=SENSORS, options=(), upload=True, **inputs):
    """One context per entry of `pads` on `model`, reset, with the same options and inputs; pollers = 0."""
    rigs = []
    try:
        for pad in pads:
            r = CapiRig(model, B, pad, optional, DEV)
            rigs.append(r)
            for name, v in (("pollers", 0),) + tuple(options):
                assert r.set_option(name, v) == 0, (name, r.error())
            assert r.reset() == 0, r.error()
            if upload:
                _upload(r, model, **inputs)
        yield rigs
    finally:
        for r in rigs:
            r.close()


def _check(rigs):
    """After a call: padding and guard rows of every context, and every context's slots equal the first one's.  Returns its snapshot."""
    for r in rigs:
        r.assert_padding_untouched()
    first = rigs[0].snapshot()
    for r in rigs[1:]:
        same_bits(first, r.snapshot())
    return first


def _call(rigs, fn, want=0):
    for r in rigs:
        rc = fn(r)
        assert rc == want, (rc, r.error(), r.pad)
    return _check(rigs)


def _plain(snap, nsteps, names=("QPOS", "QVEL", "ACT_LENGTH")):
    """The packed run is a plain one and tells the envs apart: no flag, `nsteps` everywhere, no two envs alike in `names`."""
    assert (snap["INFO"][3] == 0).all(), np.flatnonzero(snap["INFO"][3])
    assert (snap["NSTEP"] == nsteps).all()
    envs_all_differ(snap, names)


# ---------------------------------------------------------------------------------------------- 1, 2: the step call
@pytest.mark.parametrize("debug", [False, True], ids=["lean", "general"])
@pytest.mark.parametrize("B,pad", SHAPES)
def test_step_newton_lean_and_general_build(B, pad, debug):
    """12 steps (5 + 7) of stretch_empty with IMU, lidar and pose readout.  Without the debug slot the call runs the lean build through
    the staging transposes alone; with it the general build, whose debug dump is stored straight into the slot with ld."""
    opt = SENSORS + (("DEBUG",) if debug else ())
    with _rigs("stretch_empty", B, (0, pad), opt, (("solver", NEWTON),)) as rigs:
        _check(rigs)
        for n in (5, 7):
            snap = _call(rigs, lambda r: r.step(n, READ_ALL))
            assert [r.last_build() for r in rigs] == ["step" if debug else "lean"] * 2
        _plain(snap, 12, ("QPOS", "QVEL", "ACT_LENGTH", "BASE_POSE", "GYRO", "ACCEL", "XPOSE") + (("DEBUG",) if debug else ()))
        assert (snap["LIDAR"] != CANARY_F32_BITS).all() and (snap["INFO"][0] > 0).all()


@pytest.mark.parametrize("B,pad", SHAPES)
def test_step_pgs_build(B, pad):
    with _rigs("stretch_empty", B, (0, pad), SENSORS + ("DEBUG",), (("solver", PGS),)) as rigs:
        for n in (5, 7):
            snap = _call(rigs, lambda r: r.step(n, READ_ALL))
            assert [r.last_build() for r in rigs] == ["pgs"] * 2
        _plain(snap, 12, ("QPOS", "QVEL", "ACT_LENGTH", "DEBUG"))


# ---------------------------------------------------------------------------------------------- 3: pipelined chunks
def test_step_pipelined_chunks():
    """65 envs, pipeline_min_envs = 1, pipeline = 5: the 12 steps of one call run as chunks of 5 / 5 / 2 (smj_step_plan.h: more envs
    than pipeline_min_envs, a call longer than a chunk, no debug or profiling slot), one workgroup per (chunk, env), each importing and
    exporting the env's staging row.  Packed = padded = the padded context with pipeline = 0."""
    B, pad = 65, 3
    chunked = (("solver", NEWTON), ("pipeline_min_envs", 1), ("pipeline", 5))
    with _rigs("stretch_empty", B, (0, pad), SENSORS, chunked) as rigs, _rigs("stretch_empty", B, (pad,), SENSORS, (("solver", NEWTON), ("pipeline", 0))) as plain:
        snap = _call(rigs + plain, lambda r: r.step(12, READ_ALL))
        assert [r.last_build() for r in rigs + plain] == ["lean"] * 3
        _plain(snap, 12)    # every env went through all three chunks


# ---------------------------------------------------------------------------------------------- 4: hand-over to the larger build
def test_step_hand_over_to_the_tall_build():
    """primary_rows = 46 on 65 envs: the envs at the home pose never need more than 42 rows in these 12 steps; envs 2, 31 and 64 (one
    per staging tile, the tail env among them) start from qpos0 under the drop script of test_capacity_escalation..., 5 cm inside the
    base hull with 56 rows at the first step (the figures of the lane emulator), so the standard build parks them and the tall build
    finishes them: it writes their staging rows, INFO and contact records.  An env whose INFO reports more rows than the limit without
    the overflow flag was handed over."""
    B, pad, limit, dropped = 65, 3, 46, [2, 31, 64]
    m, _, _, _ = _model("stretch_empty")
    q, u, bc = _inputs("stretch_empty", B)
    bc[0] = 0
    for k, e in enumerate(dropped):
        q[7:, e] = np.asarray(m["qpos0"], np.float32)[7:]
        u[:, e] = np.asarray(DROP_CTRL, np.float32) * (1 - 0.05 * k)
    opts = (("solver", NEWTON), ("primary_rows", limit), ("pipeline", 0))
    with _rigs("stretch_empty", B, (0, pad), SENSORS + ("CONTACTS",), opts, q=q, u=u, bc=bc) as rigs:
        snap = _call(rigs, lambda r: r.step(1, READ_ALL | lib.READ_CONTACTS))
        over = snap["INFO"][0] > limit
        print("rows after the first step:", snap["INFO"][0][dropped].tolist(), "elsewhere at most", int(snap["INFO"][0][~over].max()))
        assert over[dropped].all() and over.sum() == len(dropped) and (snap["INFO"][3] == 0).all()    # handed over, finished unflagged
        ncon = snap["INFO"][1]
        assert (ncon[dropped] >= 6).all()
        for e in dropped:
            assert (snap["CONTACTS"][e, :ncon[e]] != CANARY_F32_BITS).any(axis=1).all()    # the tall build's records
        handed = 0
        for n in (7, 4):
            snap = _call(rigs, lambda r: r.step(n, READ_ALL | lib.READ_CONTACTS))
            handed += int((snap["INFO"][0] > limit).sum())
        _plain(snap, 12)
        print("envs beyond the limit at the end of the two later calls:", handed)
    # without the hand-over the same first step is flagged: the limit is what parks the envs
    with _rigs("stretch_empty", B, (pad,), SENSORS + ("CONTACTS",), opts + (("escalate", 0),), q=q, u=u, bc=bc) as (r,):
        snap = _call([r], lambda r: r.step(1, READ_ALL | lib.READ_CONTACTS))
        assert np.flatnonzero(snap["INFO"][3] & 1).tolist() == dropped


# ---------------------------------------------------------------------------------------------- 5: the satellite builds
@pytest.mark.parametrize("two_waves,tag", [(0, "sat"), (1, "sat2")])
def test_step_satellite_build(two_waves, tag):
    """stretch_scene_sat: the free objects are satellites (csrc/smj_sat.h), their state rows, debug dump and contact records included."""
    opts = (("solver", NEWTON), ("newton_two_waves", two_waves))
    with _rigs("stretch_scene_sat", 3, (0, 1), SENSORS + ("DEBUG", "CONTACTS"), opts) as rigs:
        assert rigs[0].dims["NSAT_MAX"] > 0
        for n in (5, 7):
            snap = _call(rigs, lambda r: r.step(n, READ_ALL | lib.READ_CONTACTS))
            assert [r.last_build() for r in rigs] == [tag] * 2
        _plain(snap, 12, ("QPOS", "QVEL", "ACT_LENGTH", "DEBUG", "CONTACTS"))
        assert (snap["INFO"][1] >= 1).all()


# ---------------------------------------------------------------------------------------------- 6: smj_reset
@pytest.mark.parametrize("B,pad", SHAPES)
def test_reset_masked_and_unmasked_on_dirty_state(B, pad):
    m, _, _, _ = _model("stretch_empty")
    q0 = np.asarray(m["qpos0"], np.float64).astype(np.float32).view(np.int32)
    zeroed = ("QVEL", "WARMSTART", "CTRL", "BASECTL", "NSTEP", "INFO")
    with _rigs("stretch_empty", B, (0, pad), SENSORS, (("solver", NEWTON),)) as rigs:
        before = _call(rigs, lambda r: r.step(12, READ_ALL))
        _plain(before, 12)
        for name in zeroed:    # dirty: a reset has something to clear in every slot it owns
            a = before[name].reshape(-1, B)
            assert (a != 0).any(axis=0).all(), name
        mask = torch.zeros(B, dtype=torch.uint8, device=DEV)
        mask[0::2] = 1
        after = _call(rigs, lambda r: r.reset(mask))
        hit, kept = np.arange(B) % 2 == 0, np.arange(B) % 2 == 1
        assert (after["QPOS"][:, hit] == q0[:, None]).all()
        for name in zeroed:
            assert (after[name][..., hit] == 0).all(), name
        for name in before:    # every slot, the ones a reset does not own included
            assert np.array_equal(after[name][..., kept], before[name][..., kept]), name
            if name not in zeroed + ("QPOS",):
                assert np.array_equal(after[name], before[name]), name
        final = _call(rigs, lambda r: r.reset(None))
        assert (final["QPOS"] == q0[:, None]).all()
        for name in zeroed:
            assert (final[name] == 0).all(), name


# ---------------------------------------------------------------------------------------------- 7: smj_base_controller_tick
def _tick_closed_form(base, bc, ctrl):
    """smj_base_tick_kernel in numpy fp32, op for op (csrc/smj_kernels.hip)."""
    f = np.float32
    ctrl, bc = ctrl.copy(), bc.copy()
    for e in range(base.shape[1]):
        mode = int(bc[0, e])
        if mode == 0:
            continue
        x, y, th = base[:, e]
        inc = bc[4, e]
        sign = f(1) if inc > 0 else f(-1)
        v, w, nxt = f(0), f(0), mode
        if mode == 1:
            dx, dy = f(x - bc[1, e]), f(y - bc[2, e])
            if not np.sqrt(f(f(dx * dx) + f(dy * dy))) <= abs(inc):
                nxt = 0
            else:
                v = f(BASE_X_VEL * sign)
        elif mode == 2:
            if not abs(f(bc[3, e] - th)) <= abs(inc):
                nxt = 0
            else:
                w = f(BASE_R_VEL * sign)
        else:
            v, w = bc[5, e], bc[6, e]
        half = f(f(w * WHEEL_SEPARATION) / f(2))
        rcp = f(f(1) / WHEEL_RADIUS)
        ctrl[0, e] = f(f(v - half) * rcp)
        ctrl[1, e] = f(f(v + half) * rcp)
        bc[0, e] = f(nxt)
    return ctrl, bc


@pytest.mark.parametrize("B,pad", SHAPES)
def test_base_controller_tick(B, pad):
    """Hand-written BASECTL rows, modes 0 / 1 / 2 / 3 spread over the envs, moves still under way and moves that have arrived (far from
    the threshold either way), BASE_POSE per env; the wheel rows of CTRL and the mode row against the packed context and against the
    closed form; the other rows of CTRL untouched."""
    e = np.arange(B)
    base = np.stack([0.05 * e, -0.03 * e, 0.02 * e - 1.0]).astype(np.float32)
    bc = np.zeros((8, B), np.float32)
    bc[0] = e % 4
    arrived = (e // 4) % 2 == 1    # every other group of four has travelled 1.5 x its increment
    bc[4] = np.where(e % 8 < 4, 0.3, -0.4)
    travelled = np.where(arrived, 1.5, 0.25) * np.abs(bc[4])
    bc[1], bc[2], bc[3] = base[0] - travelled, base[1], base[2] + travelled
    bc[5], bc[6] = 0.05 + 0.001 * e, 0.1 - 0.002 * e
    u = _inputs("stretch_empty", B)[1]
    with _rigs("stretch_empty", B, (0, pad), SENSORS, upload=False) as rigs:
        for r in rigs:
            r["CTRL"][:] = torch.tensor(u, device=DEV)
            r["BASECTL"][:] = torch.tensor(bc, device=DEV)
            r["BASE_POSE"][:] = torch.tensor(base, device=DEV)
        before = _check(rigs)
        after = _call(rigs, lambda r: r.tick())
        envs_all_differ(after, ("CTRL", "BASECTL", "BASE_POSE"))
        want_ctrl, want_bc = _tick_closed_form(base, bc, u)
        assert np.array_equal(after["CTRL"], want_ctrl.view(np.int32)), np.argwhere(after["CTRL"] != want_ctrl.view(np.int32))[:5]
        assert np.array_equal(after["BASECTL"], want_bc.view(np.int32))
        assert np.array_equal(after["CTRL"][2:], before["CTRL"][2:])
        modes = after["BASECTL"][0].view(np.float32)
        for mode, there, nxt in ((1, True, 0.0), (1, False, 1.0), (2, True, 0.0), (2, False, 2.0), (3, True, 3.0), (3, False, 3.0)):
            assert (modes[(e % 4 == mode) & (arrived == there)] == nxt).all(), (mode, there)    # a move that has arrived ends, the others go on
        moving = (e % 4 != 0)
        assert (after["CTRL"][:2, moving] != before["CTRL"][:2, moving]).all() and np.array_equal(after["CTRL"][:2, ~moving], before["CTRL"][:2, ~moving])
        for name in before:
            if name not in ("CTRL", "BASECTL"):
                assert np.array_equal(after[name], before[name]), name


# ---------------------------------------------------------------------------------------------- 8, 9: renderers and perception entries
SCENES = [("stretch_scene", 3, 1), ("stretch_empty", 65, 3)]


def _bits(t):
    t = t.contiguous()
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu().numpy()


def _same_outputs(tag, outs, distinct=True):
    """outs: per context one device tensor [B, ...] (or [..., B] with batch_last): equal bits, and (distinct) no two envs alike."""
    a = _bits(outs[0])
    for o in outs[1:]:
        b = _bits(o)
        assert np.array_equal(a, b), (tag, int((a != b).sum()))
    if distinct:
        assert len({a[e].tobytes() for e in range(a.shape[0])}) == a.shape[0], (tag, "two envs hold the same output")
    return a


@pytest.mark.parametrize("model,B,pad", SCENES)
def test_renderers_read_a_padded_xpose(model, B, pad):
    W, H = 64, 48
    with _rigs(model, B, (0, pad), SENSORS, (("solver", NEWTON),)) as rigs:
        snap = _call(rigs, lambda r: r.step(1, lib.READ_POSES))
        _plain(snap, 1, ("QPOS", "XPOSE"))
        ncam = rigs[0].dims["NCAM"]
        assert ncam >= 4
        for raster in (1, 0):
            for r in rigs:
                assert r.set_option("depth_raster", raster) == 0
            for cam, fovy in ((1, 58.0), (3, 42.0)):    # d405_depth, d435i_camera_depth
                outs = []
                for r in rigs:
                    rc, img = r.render_depth(cam, W, H, fovy, 10.0)
                    assert rc == 0, r.error()
                    outs.append(img)
                _check(rigs)
                a = _same_outputs(("depth", raster, cam), outs).view(np.float32)
                assert np.isfinite(a).all() and (a > 0).any(axis=(1, 2)).all() and (a != -3.0).all()
        outs = [r.render_rgb(2, W, H, 42.0) for r in rigs]    # d435i_camera_rgb
        assert all(o[0] == 0 for o in outs)
        _check(rigs)
        _same_outputs("rgb", [o[1] for o in outs], distinct=False)
        gid = _same_outputs("gid", [o[2] for o in outs], distinct=False)
        assert (gid != -9).all() and (gid >= 0).any(axis=(1, 2)).all() and len({gid[e].tobytes() for e in range(B)}) > 1


@pytest.mark.parametrize("model,B,pad", SCENES)
def test_perception_entries_read_a_padded_xpose(model, B, pad):
    """One small call of each entry that reads XPOSE: the point cloud (world frame), the height map and the occupancy grid (base frame),
    the scan match; the scan is handed over with an ODD leading dimension of its own."""
    W, H, N = 64, 48, 32
    base_body = 1    # base_link is the first body after the world (csrc/smj_step_impl.h)
    x0, y0, cell = -1.6, -1.6, 0.1
    with _rigs(model, B, (0, pad), SENSORS, (("solver", NEWTON),)) as rigs:
        snap = _call(rigs, lambda r: r.step(1, READ_ALL))
        _plain(snap, 1, ("QPOS", "XPOSE"))
        nl = rigs[0].dims["NLIDAR"]
        lidar_ld = B + 4 if B % 2 else B + 5    # odd
        assert lidar_ld % 2 == 1 and nl == 360
        g = torch.Generator().manual_seed(11)
        field = torch.randint(0, 256, (B, N, N), generator=g, dtype=torch.uint8).to(DEV)
        angles = torch.tensor([-0.05, 0.0, 0.05], dtype=torch.float32, device=DEV)
        res = {k: [] for k in ("points", "zmax", "count", "hit", "miss", "pose", "best", "score", "cell")}
        for r in rigs:
            L, s = r.L, r.stream()
            rc, img = r.render_depth(3, W, H, 42.0, 10.0)
            assert rc == 0, r.error()
            pts = torch.full((B, H, W, 3), -5.0, dtype=torch.float32, device=DEV)
            assert L.smj_depth_to_points(r.ctx, 3, W, H, 42.0, ptr(img), 1, lib.FRAME_WORLD, ptr(pts), s) == 0, r.error()
            zmax = torch.full((B, N, N), -5.0, dtype=torch.float32, device=DEV)
            count = torch.full((B, N, N), -5, dtype=torch.int32, device=DEV)
            assert L.smj_depth_to_heightmap(r.ctx, 3, W, H, 42.0, ptr(img), 1, base_body, x0, y0, cell, N, N, -1.0, 3.0, 0, ptr(zmax), ptr(count), s) == 0, r.error()
            scan = torch.full((nl, lidar_ld), float("nan"), dtype=torch.float32, device=DEV)
            scan[:, :B] = r["LIDAR"]
            hit = torch.full((B, N, N), -5, dtype=torch.int32, device=DEV)
            miss = torch.full((B, N, N), -5, dtype=torch.int32, device=DEV)
            assert L.smj_lidar_to_occupancy(r.ctx, ptr(scan), lidar_ld, base_body, x0, y0, cell, N, N, 0.05, 5.0, 1, 0, ptr(hit), ptr(miss), s) == 0, r.error()
            prior = r["BASE_POSE"].contiguous()
            pose = torch.full((3, B), -5.0, dtype=torch.float32, device=DEV)
            best = torch.full((B, 4), -5, dtype=torch.int32, device=DEV)
            score = torch.full((B, 3, 5, 5), -5, dtype=torch.int32, device=DEV)
            cells = torch.full((B, 3, nl, 2), -5, dtype=torch.int32, device=DEV)
            assert L.smj_scan_to_pose(r.ctx, ptr(scan), lidar_ld, base_body, 0.05, 5.0, ptr(field), N, N, x0, y0, cell, ptr(prior), ptr(angles), None, 3, 2, 2, 0, 5,
                                      ptr(pose), ptr(best), ptr(score), ptr(cells), s) == 0, r.error()
            for k, t in zip(res, (pts, zmax, count, hit, miss, pose.t(), best, score, cells)):
                res[k].append(t)
            assert torch.isnan(scan[:, B:]).all()
        _check(rigs)
        scene = model == "stretch_scene"    # in the empty scene a robot sees itself alone: its base-frame products are the same in every env
        pts = _same_outputs("points", res["points"]).view(np.float32)
        assert np.isfinite(pts).any(axis=(1, 2, 3)).all() and (pts != -5.0).all()
        _same_outputs("zmax", res["zmax"], distinct=scene)
        cnt = _same_outputs("count", res["count"], distinct=scene)
        assert (cnt >= 0).all() and (cnt > 0).any(axis=(1, 2)).all()
        hit = _same_outputs("hit", res["hit"], distinct=scene)
        _same_outputs("miss", res["miss"], distinct=scene)
        assert (hit >= 0).all() and (hit > 0).any(axis=(1, 2)).all()
        _same_outputs("pose", res["pose"])
        _same_outputs("best", res["best"], distinct=False)
        sc = _same_outputs("score", res["score"], distinct=scene)
        assert (sc != -5).all()
        _same_outputs("cell", res["cell"], distinct=False)


def test_scan_to_pose_takes_outputs_in_the_padding_of_xpose():
    """The columns of a slot beyond num_envs are the caller's: an output of smj_scan_to_pose that lives in the padding columns of the
    XPOSE store's last row shares no word with what the entry reads, and the call is not refused as an overlap.  (An output on the
    slot's own words is: -1.)"""
    B, pad, N = 3, 13, 32
    with _rigs("stretch_scene", B, (0, pad), SENSORS, (("solver", NEWTON),)) as rigs:
        _call(rigs, lambda r: r.step(1, READ_ALL))
        field = torch.randint(0, 256, (B, N, N), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).to(DEV)
        angles = torch.tensor([-0.05, 0.0, 0.05], dtype=torch.float32, device=DEV)
        best, poses = [], []
        for r in rigs:
            prior = r["BASE_POSE"].contiguous()
            b = torch.full((B, 4), -5, dtype=torch.int32, device=DEV)
            xs = r.stores["XPOSE"]
            rows = xs.bits.shape[0] - 2
            last_pad = xs.bits.view(torch.float32)[rows, B:B + 3 * B]    # 9 words of the last bound row's padding (none in the packed context)
            own = torch.full((3, B), -5.0, dtype=torch.float32, device=DEV)
            out = last_pad if r.pad else own
            args = lambda pose_out: (r.ctx, ptr(r["LIDAR"].contiguous()), B, 1, 0.1, 5.0, ptr(field), N, N, -1.6, -1.6, 0.1, ptr(prior), ptr(angles), None, 3, 2, 2, 0, 5,
                                     ctypes.c_void_p(pose_out.data_ptr()), ptr(b), None, None, r.stream())
            assert r.L.smj_scan_to_pose(*args(xs.view[rows - 1])) == -1 and "overlap" in r.error()    # the slot's own last row
            assert r.L.smj_scan_to_pose(*args(out)) == 0, r.error()
            r.sync()
            poses.append(out.clone().reshape(3, B).t())
            best.append(b)
            if r.pad:
                assert (last_pad.view(torch.int32) != CANARY_F32_BITS).all()
                last_pad.view(torch.int32)[:] = CANARY_F32_BITS    # hand the padding back as it was
        _check(rigs)
        _same_outputs("pose", poses)
        _same_outputs("best", best, distinct=False)


# ---------------------------------------------------------------------------------------------- 10: lidar without XPOSE
def test_lidar_without_xpose_uses_the_library_workspace_at_ld_equal_B_only():
    B = 65
    with _rigs("stretch_empty", B, (0,), SENSORS, (("solver", NEWTON),)) as (bound,), \
            _rigs("stretch_empty", B, (0, 3), ("GYRO", "ACCEL", "LIDAR", "BASECTL"), (("solver", NEWTON),)) as (packed, padded):
        want = _call([bound], lambda r: r.step(3, lib.READ_LIDAR))
        got = _call([packed], lambda r: r.step(3, lib.READ_LIDAR))
        _plain(want, 3)
        assert (want["LIDAR"] != CANARY_F32_BITS).all() and len({want["LIDAR"][:, e].tobytes() for e in range(B)}) > 1
        same_bits({k: v for k, v in want.items() if k != "XPOSE"}, got)    # the ranges among them
        before = _check([padded])
        after = _call([padded], lambda r: r.step(3, lib.READ_LIDAR), want=-5)
        assert "bind SMJ_SLOT_XPOSE when the leading dimension differs from num_envs" in padded.error()
        same_bits(before, after)
        # the refusal is the lidar's alone: the same context steps without it
        _call([padded], lambda r: r.step(3, 0))


# ---------------------------------------------------------------------------------------------- 11: binding rules
def test_binding_rules():
    B, pad = 65, 3
    with _rigs("stretch_empty", B, (pad,), SENSORS, (("solver", NEWTON),)) as (r,):
        before = _check([r])
        for name in ("QVEL", "INFO", "LIDAR", "XPOSE", "BASECTL"):    # required and optional slots alike
            other = r.make_stores(pad + 2)[name]
            assert r.bind(name, other) == 0
            for what, fn in (("step", lambda r: r.step(2, READ_ALL)), ("reset", lambda r: r.reset(None)), ("tick", lambda r: r.tick())):
                assert fn(r) == -5, (name, what)
                assert "leading dimension" in r.error(), (name, what, r.error())
            other.assert_padding_untouched(name)
            assert (other.snapshot() == other.canary).all()
            assert r.bind(name, r.stores[name]) == 0
            same_bits(before, _check([r]))
        for name in ("QPOS", "NSTEP", "XPOSE", "CONTACTS"):
            assert r.bind(name, r.stores.get(name, r.stores["QPOS"]), ld=B - 1) == -1 and "num_envs" in r.error(), name
        same_bits(before, _check([r]))
        # NSTEP is one row: it may carry any ld
        assert r.bind("NSTEP", r.stores["NSTEP"], ld=B + 40) == 0
        with _rigs("stretch_empty", B, (0,), SENSORS, (("solver", NEWTON),)) as (p,):
            snap = _call([p, r], lambda r: r.step(3, READ_ALL))
            _plain(snap, 3)


# ---------------------------------------------------------------------------------------------- 12: re-binding between calls
def test_rebinding_every_slot_between_calls():
    """6 steps, then every slot is bound to a fresh store with ANOTHER pad that holds a copy of the state, 6 more: the packed context's
    6 + 6, and the first set of stores is left as it was."""
    B = 65
    with _rigs("stretch_empty", B, (0, 1), SENSORS + ("CONTACTS",), (("solver", NEWTON),)) as rigs:
        p, q = rigs
        flags = READ_ALL | lib.READ_CONTACTS
        _call(rigs, lambda r: r.step(6, flags))
        first, left = q.stores, q.snapshot()
        fresh = q.make_stores(4)
        for name, s in fresh.items():
            s.view.copy_(first[name].view)
        q.bind_stores(fresh)
        assert q.stores is fresh and fresh["QPOS"].ld == B + 4
        _check(rigs)
        snap = _call(rigs, lambda r: r.step(6, flags))
        _plain(snap, 12)
        q.assert_padding_untouched(first)
        same_bits(left, q.snapshot(first))
        assert not np.array_equal(left["QPOS"], snap["QPOS"])
