"""Organised point clouds on the HIP path: smj_depth_to_points through the C-ABI and StretchBatchSimulator.pull_point_cloud.

One simulator for the module: scene.xml, three envs driven apart (base pose, lift, wrist pitch and head pan differ, then 200
steps), both depth cameras.  The kernel is compared with the fp64 restatement (tests/point_cloud_ref.py) fed the kernel's own
inputs -- the same fp32 depth image, the XPOSE array, the blob's camera offsets.

Tolerance per component, derived, not measured: 32 * 2^-24 * S, S = the sum of the absolute values of every term that enters the
component: |x_body|_1 + |x_cambody|_1 + |cam_pos|_1 + d (|xn| + |yn| + 1).  The longest rounding chain is two 3x3 compositions, the
pixel direction (one 2.5-ulp division included), the scale by d, a three-term dot product and the add: under 16 roundings of at
most 2^-24 S each, doubled.  About 5e-5 m at 10 m.  Every finite point must pass."""
import ctypes
import json

import numpy as np
import pytest
import torch

import perception_rig
from perception_rig import B
from point_cloud_ref import body_pose, camera_pose, deproject, pixel_dirs

pytestmark = pytest.mark.gpu

SMALL = (37, 23)
STRIDES = (1, 2, 3, 5)
EPS = 32 * 2.0 ** -24


@pytest.fixture(scope="module")
def rig():
    from stretch_mujoco_amd.enums import StretchCameras

    r = perception_rig.build(cameras=StretchCameras.depth() + [StretchCameras.cam_d405_rgb], pose_arm_and_head=True)
    sim = r.sim
    # the three transforms differ
    for cam in StretchCameras.depth():
        cp, _, _ = camera_pose(r.xpose, r.cam_bodyid, r.cam_pos, r.cam_mat, r.cam_names.index(cam.camera_name_in_mjcf))
        assert min(np.abs(cp[a] - cp[b]).max() for a in range(B) for b in range(a)) > 0.05
    yield r
    sim.stop()


def _points(r, ci, W, H, fovy, depth, stride, frame, out=None):
    hp, wp = -(-H // stride), -(-W // stride)
    if out is None:
        out = torch.full((B, hp, wp, 3), 7.0, dtype=torch.float32, device=r.sim.device)
    rc = r.L.smj_depth_to_points(r.sim._ctx, ci, W, H, float(fovy), ctypes.c_void_p(depth.data_ptr()), stride, frame,
                                 ctypes.c_void_p(out.data_ptr()), r.sim._stream())
    assert rc == 0, r.L.smj_last_error(r.sim._ctx)
    return out


def _render(r, ci, W, H, fovy, limit):
    return perception_rig.render(r, ci, W, H, fovy, limit)[0]


def _scale(r, ci, W, H, fovy, stride, depth, frame):
    """S of the module docstring, [B, H', W'] (the same for the three components)."""
    xn, yn = pixel_dirs(W, H, fovy, stride)
    S = np.abs(depth[:, ::stride, ::stride]) * (np.abs(xn) + np.abs(yn) + 1)
    if frame != "camera":
        _, _, cbp = camera_pose(r.xpose, r.cam_bodyid, r.cam_pos, r.cam_mat, ci)
        S = S + (np.abs(cbp).sum(1) + np.abs(r.cam_pos[ci]).sum())[:, None, None]
    if frame == "body":
        S = S + np.abs(body_pose(r.xpose, r.base)[0]).sum(1)[:, None, None]
    return S


@pytest.mark.parametrize("which", ["cam_d405_depth", "cam_d435i_depth"])
def test_kernel_against_fp64_on_its_own_inputs(rig, which):
    r = rig
    cam = r.cams[which]
    st = cam.initial_camera_settings
    ci = r.cam_names.index(cam.camera_name_in_mjcf)
    fovy = float(st.field_of_view_vertical_in_degrees)
    cp, cm, _ = camera_pose(r.xpose, r.cam_bodyid, r.cam_pos, r.cam_mat, ci)
    bp, bm = body_pose(r.xpose, r.base)
    worst = 0.0
    # the small image raw (far plane where nothing is hit: depths up to 40 m), the camera's own size limited (zeros -> NaN rows)
    for (W, H), limit in ((SMALL, 0.0), ((st.width, st.height), cam.depth_limit)):
        img = _render(r, ci, W, H, fovy, limit)
        torch.cuda.synchronize()
        depth = img.cpu().numpy()
        assert np.isfinite(depth).all() and (depth > 0).any()
        if limit > 0:
            assert (depth == 0).any()
        for stride in STRIDES:
            keep = depth[:, ::stride, ::stride]
            invalid = ~(np.isfinite(keep) & (keep > 0))
            for frame, fid in (("camera", r.lib.FRAME_CAMERA), ("world", r.lib.FRAME_WORLD), ("body", r.base)):
                got = _points(r, ci, W, H, fovy, img, stride, fid)
                torch.cuda.synchronize()
                got = got.cpu().numpy()
                want = deproject(depth, W, H, fovy, stride, cp, cm, frame, bp, bm)
                assert got.shape == want.shape == (B, -(-H // stride), -(-W // stride), 3)
                nan = np.isnan(got)
                assert np.array_equal(nan.all(-1), invalid) and np.array_equal(nan.any(-1), invalid), (which, W, H, stride, frame)
                tol = EPS * _scale(r, ci, W, H, fovy, stride, depth, frame)
                err = np.abs(got.astype(np.float64) - want).max(-1)
                ratio = np.where(invalid, 0.0, err / tol)
                worst = max(worst, float(ratio.max()))
                print(which, (W, H), "stride", stride, frame, "worst error / tolerance %.3f" % ratio.max(), "finite points", int((~invalid).sum()))
                assert (ratio <= 1.0).all(), (which, W, H, stride, frame, float(ratio.max()))
    print(which, "worst error / tolerance overall %.3f" % worst)


def test_nothing_outside_the_output_is_written_and_alignment_does_not_matter(rig):
    """37 x 23 at stride 1, three envs: 2553 points, N mod 4 = 1.  The output as a view 4 bytes past a 16-byte boundary inside a larger
    buffer of sentinels: the guards on both sides stay untouched and the values are those of the aligned call, bit for bit; the same
    with the depth image 4 bytes past a 16-byte boundary."""
    r = rig
    cam = r.cams.cam_d435i_depth
    ci = r.cam_names.index(cam.camera_name_in_mjcf)
    W, H = SMALL
    n = B * H * W
    assert n == 2553 and n % 4 == 1
    img = _render(r, ci, W, H, 42.0, 10.0)
    assert img.data_ptr() % 16 == 0
    for frame in (r.lib.FRAME_WORLD, r.lib.FRAME_CAMERA):
        ref = _points(r, ci, W, H, 42.0, img, 1, frame)
        assert ref.data_ptr() % 16 == 0
        sentinel, pad = -12345.678, 37      # 37 floats = 148 bytes = 4 mod 16
        big = torch.full((pad + 3 * n + pad,), sentinel, dtype=torch.float32, device=r.sim.device)
        view = big[pad: pad + 3 * n].view(B, H, W, 3)
        assert view.data_ptr() % 16 == 4
        _points(r, ci, W, H, 42.0, img, 1, frame, out=view)
        dbig = torch.full((1 + n + 3,), sentinel, dtype=torch.float32, device=r.sim.device)
        dview = dbig[1: 1 + n].view(B, H, W)
        dview.copy_(img)
        assert dview.data_ptr() % 16 == 4
        shifted = _points(r, ci, W, H, 42.0, dview, 1, frame)
        big2 = torch.full((pad + 3 * n + pad,), sentinel, dtype=torch.float32, device=r.sim.device)
        view2 = big2[pad: pad + 3 * n].view(B, H, W, 3)
        _points(r, ci, W, H, 42.0, dview, 1, frame, out=view2)      # both only 4-byte aligned
        torch.cuda.synchronize()
        guard = torch.full((pad,), sentinel, dtype=torch.float32, device=r.sim.device)
        for b in (big, big2):
            assert torch.equal(b[:pad], guard) and torch.equal(b[pad + 3 * n:], guard)
        bits = ref.view(torch.int32)
        assert not torch.equal(bits, torch.full_like(ref, 7.0).view(torch.int32))
        assert torch.equal(view.contiguous().view(torch.int32), bits)
        assert torch.equal(shifted.view(torch.int32), bits)
        assert torch.equal(view2.contiguous().view(torch.int32), bits)
        assert torch.isnan(ref).any() and torch.isfinite(ref).any()


def test_floor_pixels_land_on_the_world_plane_through_the_python_api(rig):
    """Pixels whose first geom is the plane (geom ids of the depth camera through smj_render_rgb) and that have a depth: their
    world-frame points from pull_point_cloud have |z| <= 1e-4 + 1e-4 d, the per-pixel bound of tests/test_gpu_depth.py, with that
    file's cap of 0.5 % left out (silhouette pixels of the rasteriser); at least 200 of them per env for the d405 at its own size."""
    r = rig
    sim = r.sim
    planes = torch.tensor(np.where(np.asarray(sim.model["geom_type"]) == 0)[0], device=sim.device)
    for cam in r.cams.depth():
        st = cam.initial_camera_settings
        ci = r.cam_names.index(cam.camera_name_in_mjcf)
        gid = torch.full((B, st.height, st.width), -7, dtype=torch.int32, device=sim.device)
        rgb = torch.zeros(B, st.height, st.width, 3, dtype=torch.uint8, device=sim.device)
        assert r.L.smj_render_rgb(sim._ctx, ci, st.width, st.height, float(st.field_of_view_vertical_in_degrees),
                                  ctypes.c_void_p(rgb.data_ptr()), ctypes.c_void_p(gid.data_ptr()), sim._stream()) == 0
        pts = sim.pull_point_cloud(cam, "world")
        depth = sim._depth[cam]
        torch.cuda.synchronize()
        floor = torch.isin(gid, planes) & (depth > 0)
        assert torch.equal(torch.isnan(pts).all(-1), depth == 0)
        for e in range(B):
            z, d = pts[e][floor[e]][:, 2], depth[e][floor[e]]
            n = int(floor[e].sum())
            bad = float((z.abs() > 1e-4 + 1e-4 * d).float().mean()) if n else 0.0
            print(cam.name, "env", e, "floor pixels", n, "left out", bad, "worst |z|", float(z.abs().max()) if n else None)
            assert n >= 200, (cam, e, n)
            assert bad <= 5e-3, (cam, e, bad)


def test_api_behaviour(rig):
    r = rig
    sim = r.sim
    d405, d435 = r.cams.cam_d405_depth, r.cams.cam_d435i_depth
    for cam in (d405, d435):
        st = cam.initial_camera_settings
        for s in (1, 4, 7):
            p = sim.pull_point_cloud(cam, stride=s)
            assert tuple(p.shape) == (B, -(-st.height // s), -(-st.width // s), 3) and p.dtype == torch.float32
    plain = sim.pull_point_cloud(d435, "world", stride=3).clone()
    turned = sim.pull_point_cloud(d435, "world", stride=3, auto_rotate=True)
    assert turned.shape == (B, plain.shape[2], plain.shape[1], 3)
    assert torch.equal(turned.view(torch.int32), torch.rot90(plain, -1, (1, 2)).view(torch.int32))
    same = sim.pull_point_cloud(d405, "world", stride=3, auto_rotate=True)      # only the d435i is mounted sideways
    assert same.shape == sim.pull_point_cloud(d405, "world", stride=3).shape
    # render=False after pull_camera_data() == render=True, bit for bit, no step in between
    a = sim.pull_point_cloud(d435, "world", stride=2, render=True).clone()
    sim._depth[d435].fill_(123.0)
    sim.pull_camera_data()
    b = sim.pull_point_cloud(d435, "world", stride=2, render=False)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(ValueError):
        sim.pull_point_cloud(r.cams.cam_d405_rgb)        # in cameras_to_use, but a colour camera
    with pytest.raises(ValueError):
        sim.pull_point_cloud(r.cams.cam_nav_rgb)         # not in cameras_to_use
    with pytest.raises(ValueError):
        sim.pull_point_cloud(d405, frame="odom")
    # "base" == the world cloud carried through get_link_pose("base_link", simulated=True)
    for cam in (d405, d435):
        st = cam.initial_camera_settings
        ci = r.cam_names.index(cam.camera_name_in_mjcf)
        w = sim.pull_point_cloud(cam, "world", stride=4).clone()
        bcl = sim.pull_point_cloud(cam, "base", stride=4)
        T = sim.get_link_pose("base_link", simulated=True).double()
        torch.cuda.synchronize()
        want = torch.einsum("bji,bhwj->bhwi", T[:, :3, :3], w.double() - T[:, None, None, :3, 3]).cpu().numpy()
        depth = sim._depth[cam].cpu().numpy()
        tol = EPS * _scale(r, ci, st.width, st.height, st.field_of_view_vertical_in_degrees, 4, depth, "body")
        err = np.abs(bcl.cpu().numpy().astype(np.float64) - want).max(-1)
        ok = np.isnan(want).all(-1)
        assert np.array_equal(ok, np.isnan(err)) and (~ok).any()
        assert (np.where(ok, 0.0, err) <= tol).all(), float(np.nanmax(err / tol))
    # base_link welded into its fused body at a fixed offset (no shipped model has one: the model's entry is changed for the
    # length of this check): the constant pose is carried along exactly -- the same comparison, |offset|_1 more in S
    i = sim.names["body"].index("base_link")
    keep = sim.model["link_relpos"][i].copy(), sim.model["link_relquat"][i].copy()
    try:
        sim.model["link_relpos"][i] = [0.3, -0.2, 0.1]
        sim.model["link_relquat"][i] = [np.cos(0.35), 0.0, np.sin(0.35) * 0.6, np.sin(0.35) * 0.8]
        w = sim.pull_point_cloud(d435, "world", stride=4).clone()
        bcl = sim.pull_point_cloud(d435, "base", stride=4)
        T = sim.get_link_pose("base_link", simulated=True).double()
        torch.cuda.synchronize()
        want = torch.einsum("bji,bhwj->bhwi", T[:, :3, :3], w.double() - T[:, None, None, :3, 3]).cpu().numpy()
        st = d435.initial_camera_settings
        tol = EPS * (_scale(r, r.cam_names.index(d435.camera_name_in_mjcf), st.width, st.height, st.field_of_view_vertical_in_degrees, 4,
                            sim._depth[d435].cpu().numpy(), "body") + 0.6)
        err = np.abs(bcl.cpu().numpy().astype(np.float64) - want).max(-1)
        assert np.isfinite(err).any() and (np.where(np.isnan(want).all(-1), 0.0, err) <= tol).all(), float(np.nanmax(err / tol))
    finally:
        sim.model["link_relpos"][i], sim.model["link_relquat"][i] = keep
    # error codes of the entry
    L, ctx = r.L, sim._ctx
    img = sim._depth[d405]
    st = d405.initial_camera_settings
    out = torch.zeros(B, st.height, st.width, 3, dtype=torch.float32, device=sim.device)
    dp, op, fovy = ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(out.data_ptr()), float(st.field_of_view_vertical_in_degrees)
    assert L.smj_depth_to_points(ctx, 99, st.width, st.height, fovy, dp, 1, -1, op, sim._stream()) < 0
    assert b"camera id" in L.smj_last_error(ctx)
    assert L.smj_depth_to_points(ctx, 1, st.width, st.height, fovy, dp, 0, -1, op, sim._stream()) < 0
    assert L.smj_depth_to_points(ctx, 1, st.width, st.height, fovy, dp, 1, -1, None, sim._stream()) < 0
    assert L.smj_depth_to_points(ctx, 1, st.width, st.height, fovy, None, 1, -1, op, sim._stream()) < 0
    assert L.smj_depth_to_points(ctx, 1, 0, st.height, fovy, dp, 1, -1, op, sim._stream()) < 0
    assert L.smj_depth_to_points(ctx, 1, st.width, st.height, fovy, dp, 1, 10 ** 6, op, sim._stream()) < 0       # body id >= nbody
    assert L.smj_depth_to_points(ctx, 1, st.width, st.height, fovy, dp, 1, -3, op, sim._stream()) < 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0        # a refused call writes nothing
    # a bare context (nothing bound): the world frame needs XPOSE (-5), the camera frame needs no slot
    bare = ctypes.c_void_p()
    assert L.smj_create(sim._blob, len(sim._blob), 1, 0, ctypes.byref(bare)) == 0
    try:
        one = img[:1].contiguous()
        o1 = torch.zeros(1, st.height, st.width, 3, dtype=torch.float32, device=sim.device)
        args = (1, st.width, st.height, fovy, ctypes.c_void_p(one.data_ptr()), 1)
        assert L.smj_depth_to_points(bare, *args, -2, ctypes.c_void_p(o1.data_ptr()), sim._stream()) == -5
        assert b"XPOSE" in L.smj_last_error(bare)
        assert L.smj_depth_to_points(bare, *args, 0, ctypes.c_void_p(o1.data_ptr()), sim._stream()) == -5
        assert L.smj_depth_to_points(bare, *args, -1, ctypes.c_void_p(o1.data_ptr()), sim._stream()) == 0
        torch.cuda.synchronize()
        valid = one > 0
        assert valid.any() and torch.equal(o1[..., 2][valid], one[valid]) and torch.isnan(o1[~valid]).all()
    finally:
        L.smj_destroy(bare)
