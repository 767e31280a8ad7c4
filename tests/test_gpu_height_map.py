"""Egocentric height maps on the HIP path: smj_depth_to_heightmap through the C-ABI and StretchBatchSimulator.pull_height_map.

One simulator for the module, the rig of tests/test_gpu_point_cloud.py: stretch_scene, three envs driven apart, 200 steps, both
depth cameras.  The kernel is compared with the fp64 reference (tests/height_map_ref.py) fed the kernel's own inputs -- the same fp32
depth image, the XPOSE array, the blob's camera offsets, and the fp32 values of origin and cell -- by that file's comparison rule:
every cell, n_lo <= count <= n_hi, NaN iff count == 0, z_lo - m_z <= height <= z_hi + m_z, with the share of ambiguous points
asserted <= 1 % per env and case (and printed).  Everything else is exact: bit-for-bit equalities and integer counts.

Two places where the issue's wording needed care, both about points within rounding of a cell edge:
* the exact case replicates smj_points_dir in np.float32, but the library is built with 2.5-ulp fp32 division, so (u + 0.5f) / width
  is not a single rounding on the device.  The test therefore also requires of its INPUT (origin searched on a 2^-10 lattice) that
  no replicated pixel lies within 2e-5 cells of an edge -- ten times what 2.5 ulp of the quotient and one ulp of tanf can move it --
  and then asks exactly what the issue asks: equal counts, height == 1.0f in every hit cell, NaN elsewhere.
* a grid cut in two by a shifted y0 rounds y - y0 differently in the two calls, so a point within 2^-22 m of a row edge can change
  rows.  The origin (a multiple of the cell first, then of cell / 16) is taken so that the REFERENCE has no point that close, margin
  included; then the equality is bit for bit over all cells."""
import ctypes
import math

import numpy as np
import pytest
import torch

import height_map_ref as ref
import perception_rig
from perception_rig import B, f32
from perception_rig import frame_id as _fid
from perception_rig import render as _render
from point_cloud_ref import body_pose, camera_pose, deproject, pixel_dirs

pytestmark = pytest.mark.gpu

SMALL = (37, 23)
X0, Y0 = -1.613, -1.587
INF = float("inf")


@pytest.fixture(scope="module")
def rig():
    from stretch_mujoco_amd.enums import StretchCameras

    r = perception_rig.build(cameras=StretchCameras.depth() + [StretchCameras.cam_d405_rgb], pose_arm_and_head=True)
    yield r
    r.sim.stop()


def _cam(r, which):
    cam = r.cams[which]
    st = cam.initial_camera_settings
    return cam, st, r.cam_names.index(cam.camera_name_in_mjcf), float(st.field_of_view_vertical_in_degrees)


def _hmap(r, ci, W, H, fovy, depth, stride, frame, x0, y0, cell, nx, ny, zl, zh, acc=0, out=None, count=True, ctx=None, rc=0):
    dev = r.sim.device
    if out is None:
        out = (torch.full((depth.shape[0], ny, nx), 7.0, dtype=torch.float32, device=dev), torch.full((depth.shape[0], ny, nx), 7, dtype=torch.int32, device=dev))
    got = r.L.smj_depth_to_heightmap(ctx or r.sim._ctx, ci, W, H, float(fovy), ctypes.c_void_p(depth.data_ptr()) if depth is not None else None,
                                     stride, frame, x0, y0, cell, nx, ny, zl, zh, acc, ctypes.c_void_p(out[0].data_ptr()) if out[0] is not None else None,
                                     ctypes.c_void_p(out[1].data_ptr()) if count else None, r.sim._stream())
    assert got == rc, (got, r.L.smj_last_error(ctx or r.sim._ctx))
    return out


def _points_and_scale(r, ci, W, H, fovy, depth, stride, frame):
    """fp64 points [B, H', W', 3] from the kernel's own inputs and the scale S of tests/test_gpu_point_cloud.py."""
    key = ("pts", ci, W, H, stride, frame, depth.ctypes.data)
    if key not in r.cache:
        cp, cm, cbp = camera_pose(r.xpose, r.cam_bodyid, r.cam_pos, r.cam_mat, ci)
        bp, bm = body_pose(r.xpose, r.base)
        pts = deproject(depth, W, H, fovy, stride, cp, cm, frame, bp, bm)
        xn, yn = pixel_dirs(W, H, fovy, stride)
        S = np.abs(depth[:, ::stride, ::stride].astype(np.float64)) * (np.abs(xn) + np.abs(yn) + 1)
        if frame != "camera":
            S = S + (np.abs(cbp).sum(1) + np.abs(r.cam_pos[ci]).sum())[:, None, None]
        if frame == "body":
            S = S + np.abs(bp).sum(1)[:, None, None]
        r.cache[key] = (pts, S)
    return r.cache[key]


def _bounds(r, ci, W, H, fovy, depth, stride, frame, x0, y0, cell, nx, ny, zl, zh):
    pts, S = _points_and_scale(r, ci, W, H, fovy, depth, stride, frame)
    return [ref.bounds(pts[e], S[e], f32(x0), f32(y0), f32(cell), nx, ny, f32(zl), f32(zh)) for e in range(B)]


def _compare(tag, height, count, bds):
    torch.cuda.synchronize()
    h, n = height.cpu().numpy(), count.cpu().numpy()
    for e, bd in enumerate(bds):
        share = ref.ambiguous_share(bd)
        print(tag, "env", e, "valid", bd.valid, "sure", bd.sure, "ambiguous", bd.ambiguous, "share %.4f %%" % (100 * share), "occupied", int((n[e] > 0).sum()))
        assert share <= ref.MAX_AMBIGUOUS, (tag, e, share)
        bad = ref.check_map(h[e], n[e], bd)
        assert not bad, (tag, e, len(bad), bad[:5])
    return h, n


def _origin_around(pts, nx, ny, cell):
    """Origin of a grid centred on something the camera sees, so that the grid is not empty: the point (inside the z band of the
    reference test if there is one) nearest to the median of the cloud.  Not a round number."""
    p = pts.reshape(-1, 3)
    p = p[~np.isnan(p[:, 0])]
    band = p[(p[:, 2] > 0.0) & (p[:, 2] < 1.9)]
    p = band if len(band) else p
    c = p[np.argmin(np.abs(p[:, :2] - np.median(p[:, :2], 0)).sum(1))]
    return f32(c[0] - nx * cell / 2 + 0.0137), f32(c[1] - ny * cell / 2 + 0.0113)


@pytest.mark.parametrize("which", ["cam_d405_depth", "cam_d435i_depth"])
def test_kernel_against_the_reference_on_its_own_inputs(rig, which):
    r = rig
    cam, st, ci, fovy = _cam(r, which)
    sure = 0
    for (W, H), limit in ((SMALL, 0.0), ((st.width, st.height), cam.depth_limit)):
        img, depth = _render(r, ci, W, H, fovy, limit)
        assert np.isfinite(depth).all() and (depth > 0).any()
        for stride in (1, 3):
            for frame in ("world", "body"):
                pts, _ = _points_and_scale(r, ci, W, H, fovy, depth, stride, frame)
                # the robot-centred origin of the issue's example, and grids centred on what the camera sees (the head camera looks
                # past a 3.2 m window around the robot)
                for (nx, ny), (x0, y0) in (((16, 12), _origin_around(pts, 16, 12, 0.05)), ((64, 64), (X0, Y0)), ((64, 64), _origin_around(pts, 64, 64, 0.05))):
                    args = (f32(x0), f32(y0), f32(0.05), nx, ny, -0.05, 2.0)
                    height, count = _hmap(r, ci, W, H, fovy, img, stride, _fid(r, frame), *args)
                    bds = _bounds(r, ci, W, H, fovy, depth, stride, frame, *args)
                    _compare(f"{which} {W}x{H} stride {stride} {frame} grid {nx}x{ny}", height, count, bds)
                    sure += sum(bd.sure for bd in bds)
                    if (W, H) != SMALL and (nx, ny) == (64, 64) and (x0, y0) != (X0, Y0):
                        assert sum(bd.sure for bd in bds) > 0.05 * sum(bd.valid for bd in bds), [bd.sure for bd in bds]      # not about empty maps
    assert sure > 1000


@pytest.mark.parametrize("size", [SMALL, "own"])
def test_exact_case_constant_depth_in_the_camera_frame(rig, size):
    """Depth 1.0 everywhere, camera frame, cell 0.0625 (inv_cell = 16 exactly): the point is (xn, -yn, 1) exactly as smj_points_dir
    gives xn and yn, and the cell index is floor((x - x0) * 16).  Replicated in np.float32 (module docstring: the input is chosen so
    that no pixel is near a cell edge); counts equal, height == 1.0f in every hit cell, NaN elsewhere."""
    r = rig
    cam, st, ci, fovy = _cam(r, "cam_d435i_depth")
    W, H = (st.width, st.height) if size == "own" else size
    one, half, two = np.float32(1), np.float32(0.5), np.float32(2)
    th = np.float32(math.tan(float(np.float32(np.float32(fovy) * np.float32(3.14159265358979323846) / np.float32(360)))))
    aspect = np.float32(W) / np.float32(H)
    u, v = np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32)
    xn = ((u + half) / np.float32(W) * two - one) * th * aspect
    yn = (one - (v + half) / np.float32(H) * two) * th
    x, y = xn * one, -(yn * one)
    nx, ny, cell = 40, 24, np.float32(0.0625)
    for j in range(64):      # origin on a 2^-10 lattice: the first one that keeps every pixel 2e-5 cells away from an edge
        x0, y0 = np.float32(-1.25 - j / 1024), np.float32(-0.75 - j / 1024)
        fx, fy = (x - x0) * np.float32(16), (y - y0) * np.float32(16)
        if min(np.abs(fx - np.round(fx)).min(), np.abs(fy - np.round(fy)).min()) > 2e-5:
            break
    else:
        pytest.fail("no origin keeps the pixels off the cell edges")
    ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    want = np.zeros((ny, nx), np.int64)
    keep = ((iy >= 0) & (iy < ny))[:, None] & ((ix >= 0) & (ix < nx))[None, :]
    np.add.at(want, (np.broadcast_to(iy[:, None], keep.shape)[keep], np.broadcast_to(ix[None, :], keep.shape)[keep]), 1)
    assert 0 < want.sum() and (want == 0).any()
    img = torch.ones(B, H, W, dtype=torch.float32, device=r.sim.device)
    for stride in (1,):
        height, count = _hmap(r, ci, W, H, fovy, img, stride, r.lib.FRAME_CAMERA, float(x0), float(y0), float(cell), nx, ny, 0.5, 1.5)
        torch.cuda.synchronize()
        h, n = height.cpu().numpy(), count.cpu().numpy()
        print("exact case", (W, H), "origin", float(x0), float(y0), "pixels in the grid", int(want.sum()), "of", W * H)
        for e in range(B):
            assert np.array_equal(n[e], want), (e, np.argwhere(n[e] != want)[:5])
            assert (h[e][want > 0] == np.float32(1)).all() and np.isnan(h[e][want == 0]).all()


def test_one_cell_takes_every_valid_pixel(rig):
    """nx = ny = 1, a huge cell, an infinite band: every lane of every wavefront hits the same address."""
    r = rig
    for which in ("cam_d405_depth", "cam_d435i_depth"):
        cam, st, ci, fovy = _cam(r, which)
        for (W, H), limit in ((SMALL, 0.0), ((st.width, st.height), cam.depth_limit)):
            img, depth = _render(r, ci, W, H, fovy, limit)
            for stride in (1, 3):
                args = (-5e5, -5e5, 1e6, 1, 1, -INF, INF)
                height, count = _hmap(r, ci, W, H, fovy, img, stride, r.lib.FRAME_WORLD, *args)
                bds = _bounds(r, ci, W, H, fovy, depth, stride, "world", *args)
                pts, S = _points_and_scale(r, ci, W, H, fovy, depth, stride, "world")
                h, n = _compare(f"one cell {which} {W}x{H} stride {stride}", height, count, bds)
                keep = depth[:, ::stride, ::stride]
                for e in range(B):
                    assert bds[e].ambiguous == 0 and int(n[e, 0, 0]) == int((keep[e] > 0).sum()) == bds[e].valid > 0
                    # the margin of the POINT alone (EPS * S): the cell-edge term of m is 0.24 m for this cell and does not apply to z
                    assert abs(float(h[e, 0, 0]) - np.nanmax(pts[e][..., 2])) <= ref.EPS * np.nanmax(np.where(np.isnan(pts[e][..., 2]), 0, S[e]))


def test_bands_equal_the_two_half_grids(rig):
    """64 x 96 cells at 0.0625 m are two bands.  The grid equals, bit for bit, its two halves of 48 rows computed by two calls
    with y0 and y0 + 3 (module docstring: y0 is taken so that the reference has no point within its margin + 2^-22 m of a row edge)."""
    r = rig
    cam, st, ci, fovy = _cam(r, "cam_d435i_depth")
    nx, ny, cell = 64, 96, 0.0625
    checked = 0
    for (W, H), limit, stride in ((SMALL, 0.0, 1), ((st.width, st.height), cam.depth_limit, 5)):
        img, depth = _render(r, ci, W, H, fovy, limit)
        pts, S = _points_and_scale(r, ci, W, H, fovy, depth, stride, "body")
        x0 = -2.0
        ok = ~np.isnan(pts[..., 1])
        xv, yv, zv = pts[..., 0][ok], pts[..., 1][ok], pts[..., 2][ok]
        m = ref.EPS * S[ok] + 2.0 ** -22 * (np.abs(pts[..., 0][ok] - x0) + np.abs(yv + 3.0)) + 2.0 ** -22
        for j in range(16):
            y0 = -3.0 - j / 256
            inside = (yv > y0 - 1) & (yv < y0 + ny * cell + 1) & (xv > x0 - 1) & (xv < x0 + nx * cell + 1) & (zv > -1) & (zv < 3)   # who can be kept at all
            if (np.floor((yv - m - y0) / cell) == np.floor((yv + m - y0) / cell))[inside].all():
                break
        else:
            pytest.fail("every candidate origin has a point within rounding of a row edge")
        args = (stride, r.base, x0)
        full = _hmap(r, ci, W, H, fovy, img, *args, y0, cell, nx, ny, -0.05, 2.0)
        lo = _hmap(r, ci, W, H, fovy, img, *args, y0, cell, nx, 48, -0.05, 2.0)
        hi = _hmap(r, ci, W, H, fovy, img, *args, y0 + 48 * cell, cell, nx, 48, -0.05, 2.0)
        torch.cuda.synchronize()
        print("bands", (W, H), "y0", y0, "occupied", int((full[1] > 0).sum()), int((lo[1] > 0).sum()), int((hi[1] > 0).sum()))
        for k in (0, 1):
            assert torch.equal(full[k][:, :48].contiguous().view(torch.int32), lo[k].view(torch.int32))
            assert torch.equal(full[k][:, 48:].contiguous().view(torch.int32), hi[k].view(torch.int32))
        assert int((lo[1] > 0).sum()) > 0 and int((hi[1] > 0).sum()) > 0
        checked += 1
        # and against the reference, as every other grid
        _compare(f"bands {W}x{H}", *full, _bounds(r, ci, W, H, fovy, depth, stride, "body", x0, y0, cell, nx, ny, -0.05, 2.0))
    assert checked == 2


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_order_independence_and_accumulate(rig):
    r = rig
    imgs = {}
    for which in ("cam_d405_depth", "cam_d435i_depth"):
        cam, st, ci, fovy = _cam(r, which)
        imgs[which] = (ci, st.width, st.height, fovy, _render(r, ci, st.width, st.height, fovy, cam.depth_limit)[0])
    for nx, ny in ((64, 64), (96, 80)):
        grid = (f32(2 * X0), f32(2 * Y0), f32(0.1), nx, ny, -0.05, 2.0)      # 10 cm cells: the head camera looks past a 3.2 m window

        def call(which, acc=0, out=None):
            ci, W, H, fovy, img = imgs[which]
            return _hmap(r, ci, W, H, fovy, img, 1, r.base, *grid, acc=acc, out=out)

        a, a2, b = call("cam_d435i_depth"), call("cam_d435i_depth"), call("cam_d405_depth")
        assert torch.equal(_bits(a[0]), _bits(a2[0])) and torch.equal(a[1], a2[1])      # two calls, identical arrays
        ab = call("cam_d405_depth", 1, call("cam_d435i_depth"))
        ba = call("cam_d435i_depth", 1, call("cam_d405_depth"))
        torch.cuda.synchronize()
        want_h = torch.where(torch.isnan(a[0]), b[0], torch.where(torch.isnan(b[0]), a[0], torch.maximum(a[0], b[0])))
        assert torch.equal(_bits(ab[0]), _bits(want_h)) and torch.equal(ab[1], a[1] + b[1])
        assert torch.equal(_bits(ab[0]), _bits(ba[0])) and torch.equal(ab[1], ba[1])
        both = ((a[1] > 0) & (b[1] > 0)).sum()
        print("accumulate", (nx, ny), "occupied", int((a[1] > 0).sum()), int((b[1] > 0).sum()), "by both", int(both))
        assert int((a[1] > 0).sum()) > 50 and int((b[1] > 0).sum()) > 10
        # without a count buffer the heights are the same and nothing else is touched
        h_only = torch.full((B, ny, nx), 7.0, dtype=torch.float32, device=r.sim.device)
        ci, W, H, fovy, img = imgs["cam_d435i_depth"]
        _hmap(r, ci, W, H, fovy, img, 1, r.base, *grid, out=(h_only, None), count=False)
        assert torch.equal(_bits(h_only), _bits(a[0]))


def test_nothing_outside_the_outputs_is_written_and_alignment_does_not_matter(rig):
    """37 x 23, three envs (851 pixels per env: the envs' images start at every alignment), grids of one and two bands.  The outputs as
    views 4 bytes past a 16-byte boundary inside buffers of sentinels: the guards stay untouched and the values are those of the
    aligned call, bit for bit; the same with the depth image 4 bytes past a 16-byte boundary, and with both."""
    r = rig
    cam, st, ci, fovy = _cam(r, "cam_d435i_depth")
    W, H = SMALL
    img, _ = _render(r, ci, W, H, fovy, 0.0)
    assert img.data_ptr() % 16 == 0
    dev = r.sim.device
    n = B * H * W
    dbig = torch.full((1 + n + 3,), -1.0, dtype=torch.float32, device=dev)
    dview = dbig[1: 1 + n].view(B, H, W)
    dview.copy_(img)
    assert dview.data_ptr() % 16 == 4
    _, depth_host = _render(r, ci, W, H, fovy, 0.0)
    for nx, ny, stride in ((16, 12, 1), (64, 64, 1), (61, 83, 1), (61, 83, 3)):
        pts, _ = _points_and_scale(r, ci, W, H, fovy, depth_host, stride, "body")
        grid = (*_origin_around(pts, nx, ny, 0.0625), f32(0.0625), nx, ny, -INF, INF)
        want = _hmap(r, ci, W, H, fovy, img, stride, r.base, *grid)
        assert want[0].data_ptr() % 16 == 0 and want[1].data_ptr() % 16 == 0
        cells, pad = B * nx * ny, 37      # 37 words = 148 bytes = 4 mod 16
        results = []
        for depth in (img, dview):
            hbig = torch.full((pad + cells + pad,), -12345.678, dtype=torch.float32, device=dev)
            cbig = torch.full((pad + cells + pad,), -12345, dtype=torch.int32, device=dev)
            hv, cv = hbig[pad: pad + cells].view(B, ny, nx), cbig[pad: pad + cells].view(B, ny, nx)
            assert hv.data_ptr() % 16 == 4 and cv.data_ptr() % 16 == 4
            _hmap(r, ci, W, H, fovy, depth, stride, r.base, *grid, out=(hv, cv))
            results.append((hbig, cbig, hv, cv))
        # heights misaligned, counts aligned: the two outputs take different paths
        hbig = torch.full((pad + cells + pad,), -12345.678, dtype=torch.float32, device=dev)
        calign = torch.full((B, ny, nx), 7, dtype=torch.int32, device=dev)
        _hmap(r, ci, W, H, fovy, img, stride, r.base, *grid, out=(hbig[pad: pad + cells].view(B, ny, nx), calign))
        results.append((hbig, None, hbig[pad: pad + cells].view(B, ny, nx), calign))
        shifted = _hmap(r, ci, W, H, fovy, dview, stride, r.base, *grid)
        torch.cuda.synchronize()
        assert int((want[1] > 0).sum()) > 0
        assert torch.equal(_bits(shifted[0]), _bits(want[0])) and torch.equal(shifted[1], want[1])
        for hbig, cbig, hv, cv in results:
            assert (hbig[:pad] == -12345.678).all() and (hbig[pad + cells:] == -12345.678).all()
            if cbig is not None:
                assert (cbig[:pad] == -12345).all() and (cbig[pad + cells:] == -12345).all()
            assert torch.equal(_bits(hv), _bits(want[0])) and torch.equal(cv.contiguous(), want[1])
        assert (dbig[0] == -1.0) and (dbig[1 + n:] == -1.0).all()


def test_error_codes_and_a_refused_call_writes_nothing(rig):
    r = rig
    L, sim = r.L, r.sim
    cam, st, ci, fovy = _cam(r, "cam_d405_depth")
    W, H = st.width, st.height
    img, _ = _render(r, ci, W, H, fovy, cam.depth_limit)
    nx = ny = 64
    out = (torch.zeros(B, ny, nx, dtype=torch.float32, device=sim.device), torch.zeros(B, ny, nx, dtype=torch.int32, device=sim.device))
    nan = float("nan")
    good = dict(ci=ci, W=W, H=H, fovy=fovy, stride=1, frame=r.lib.FRAME_WORLD, x0=X0, y0=Y0, cell=0.05, nx=nx, ny=ny, zl=-0.05, zh=2.0)
    bad = [dict(ci=99), dict(ci=-1), dict(W=0), dict(H=0), dict(stride=0), dict(nx=0), dict(ny=0), dict(nx=257, ny=256), dict(nx=65537, ny=1),
           dict(cell=0.0), dict(cell=-0.05), dict(cell=INF), dict(cell=nan), dict(x0=INF), dict(x0=nan), dict(y0=-INF), dict(y0=nan),
           dict(zl=nan), dict(zh=nan), dict(zl=1.0, zh=0.5), dict(frame=10 ** 6), dict(frame=-3)]
    for change in bad:
        a = dict(good, **change)
        rc = L.smj_depth_to_heightmap(sim._ctx, a["ci"], a["W"], a["H"], a["fovy"], ctypes.c_void_p(img.data_ptr()), a["stride"], a["frame"],
                                      a["x0"], a["y0"], a["cell"], a["nx"], a["ny"], a["zl"], a["zh"], 0, ctypes.c_void_p(out[0].data_ptr()),
                                      ctypes.c_void_p(out[1].data_ptr()), sim._stream())
        assert rc == -1, (change, rc)
        assert L.smj_last_error(sim._ctx)
    g = (good["x0"], good["y0"], good["cell"], nx, ny, good["zl"], good["zh"])
    dp, hp, cp = img.data_ptr(), out[0].data_ptr(), out[1].data_ptr()
    for d, h, c in ((None, hp, cp), (dp, None, cp), (dp + 2, hp, cp), (dp, hp + 1, cp), (dp, hp, cp + 2)):      # null / misaligned pointers
        rc = L.smj_depth_to_heightmap(sim._ctx, ci, W, H, fovy, ctypes.c_void_p(d) if d else None, 1, r.lib.FRAME_WORLD, *g, 0,
                                      ctypes.c_void_p(h) if h else None, ctypes.c_void_p(c), sim._stream())
        assert rc == -1, (d, h, c, rc)
    torch.cuda.synchronize()
    assert float(out[0].abs().max()) == 0.0 and int(out[1].abs().max()) == 0        # a refused call writes nothing
    # the largest grid is taken; a null count buffer is allowed (test_order_independence_and_accumulate)
    _hmap(r, ci, W, H, fovy, img, 1, r.lib.FRAME_WORLD, X0, Y0, 0.05, 256, 256, -0.05, 2.0)
    # a bare context (nothing bound): world and body frames need XPOSE (-5), the camera frame needs no slot
    bare = ctypes.c_void_p()
    assert L.smj_create(sim._blob, len(sim._blob), 1, 0, ctypes.byref(bare)) == 0
    try:
        one = img[:1].contiguous()
        o1 = (torch.zeros(1, ny, nx, dtype=torch.float32, device=sim.device), torch.zeros(1, ny, nx, dtype=torch.int32, device=sim.device))
        _hmap(r, ci, W, H, fovy, one, 1, r.lib.FRAME_WORLD, *g, out=o1, ctx=bare, rc=-5)
        assert b"XPOSE" in L.smj_last_error(bare)
        _hmap(r, ci, W, H, fovy, one, 1, 0, *g, out=o1, ctx=bare, rc=-5)
        torch.cuda.synchronize()
        assert float(o1[0].abs().max()) == 0.0 and int(o1[1].max()) == 0
        _hmap(r, ci, W, H, fovy, one, 1, r.lib.FRAME_CAMERA, -0.8, -0.8, 0.025, nx, ny, 0.0, INF, out=o1, ctx=bare, rc=0)
        torch.cuda.synchronize()
        assert int(o1[1].sum()) > 0 and torch.equal(torch.isnan(o1[0]), o1[1] == 0)
    finally:
        L.smj_destroy(bare)


def test_python_api(rig):
    r = rig
    sim = r.sim
    d405, d435 = r.cams.cam_d405_depth, r.cams.cam_d435i_depth
    from stretch_mujoco_amd.datamodels import StatusStretchHeightMap

    hm = sim.pull_height_map(origin=(X0, Y0), cell=0.05, shape=(48, 64), z_range=(-0.05, 2.0))
    assert isinstance(hm, StatusStretchHeightMap) and hm.frame == "base" and hm.cell == 0.05 and hm.origin == (X0, Y0)
    assert tuple(hm.height.shape) == tuple(hm.count.shape) == (B, 48, 64) and hm.height.dtype == torch.float32 and hm.count.dtype == torch.int32
    assert tuple(hm.time.shape) == (B,)
    again = sim.pull_height_map(origin=(X0, Y0), cell=0.05, shape=(48, 64), z_range=(-0.05, 2.0))
    assert again.height.data_ptr() == hm.height.data_ptr()      # simulator-owned, keyed by (frame, shape)
    assert sim.pull_height_map(frame="world", shape=(48, 64)).height.data_ptr() != hm.height.data_ptr()
    # both cameras == the two C-ABI calls on the images the simulator rendered, bit for bit
    got = sim.pull_height_map(origin=(X0, Y0), cell=0.05, shape=(64, 64), z_range=(-0.05, 2.0))
    gh, gc = got.height.clone(), got.count.clone()
    out = None
    for k, cam in enumerate(c for c in sim._cameras if c.is_depth):
        _, st, ci, fovy = _cam(r, cam.name)
        out = _hmap(r, ci, st.width, st.height, fovy, sim._depth[cam], 1, r.base, X0, Y0, 0.05, 64, 64, -0.05, 2.0, acc=int(k > 0), out=out)
    torch.cuda.synchronize()
    assert k == 1 and torch.equal(_bits(gh), _bits(out[0])) and torch.equal(gc, out[1]) and int((gc > 0).sum()) > 100
    one = sim.pull_height_map(cameras=[d435], origin=(X0, Y0), shape=(64, 64), z_range=(-0.05, 2.0))
    assert int(one.count.sum()) < int(gc.sum()) and int(one.count.sum()) > 0
    # render=False after pull_camera_data() == render=True, no step in between
    for cam in (d405, d435):
        sim._depth[cam].fill_(123.0)
    sim.pull_camera_data()
    again = sim.pull_height_map(origin=(X0, Y0), cell=0.05, shape=(64, 64), z_range=(-0.05, 2.0), render=False)
    assert torch.equal(_bits(again.height), _bits(gh)) and torch.equal(again.count, gc)
    s3 = sim.pull_height_map(origin=(X0, Y0), shape=(64, 64), z_range=(-0.05, 2.0), stride=3, render=False)
    assert 0 < int(s3.count.sum()) < int(gc.sum())
    for kw in (dict(cameras=[r.cams.cam_d405_rgb]), dict(cameras=[r.cams.cam_nav_rgb]), dict(frame="odom"), dict(shape=(0, 4)), dict(shape=(257, 256)),
               dict(shape=(4,)), dict(cell=0.0), dict(cell=float("nan")), dict(z_range=(1.0, 0.5)), dict(z_range=(float("nan"), 1.0)), dict(stride=0),
               dict(origin=(INF, 0.0)), dict(cameras=[])):
        with pytest.raises(ValueError):
            sim.pull_height_map(**kw)
    # base_link at a fixed pose inside its fused body (no shipped model: the entry is changed for the length of this check)
    i = sim.names["body"].index("base_link")
    keep = sim.model["link_relpos"][i].copy()
    try:
        sim.model["link_relpos"][i] = [0.3, -0.2, 0.1]
        with pytest.raises(ValueError, match="base_link"):
            sim.pull_height_map()
        sim.pull_height_map(frame="world")
    finally:
        sim.model["link_relpos"][i] = keep


def test_floor_cells_lie_on_the_world_plane(rig):
    """World-frame map of the band [-0.05, 0.05]: every occupied cell whose pixels are all floor (first geom the plane, by the geom ids
    of smj_render_rgb) has |height| <= 1e-4 + 1e-4 d_max, d_max the largest depth among the cell's pixels: the per-pixel bound of
    tests/test_gpu_depth.py.  A cell's pixels are all pixels that can have been binned into it: the candidates of the reference.  At
    least 50 such cells per env for the d405 at its own size."""
    r = rig
    sim = r.sim
    planes = torch.tensor(np.where(np.asarray(sim.model["geom_type"]) == 0)[0], device=sim.device)
    nx = ny = 64
    for cam in r.cams.depth():
        _, st, ci, fovy = _cam(r, cam.name)
        W, H = st.width, st.height
        gid = torch.full((B, H, W), -7, dtype=torch.int32, device=sim.device)
        rgb = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=sim.device)
        assert r.L.smj_render_rgb(sim._ctx, ci, W, H, fovy, ctypes.c_void_p(rgb.data_ptr()), ctypes.c_void_p(gid.data_ptr()), sim._stream()) == 0
        hm = sim.pull_height_map(cameras=[cam], frame="world", origin=(X0, Y0), cell=0.05, shape=(ny, nx), z_range=(-0.05, 0.05))
        torch.cuda.synchronize()
        depth = sim._depth[cam].cpu().numpy()
        floor = (torch.isin(gid, planes).cpu().numpy()) & (depth > 0)
        pts, S = _points_and_scale(r, ci, W, H, fovy, depth, 1, "world")
        h, n = hm.height.cpu().numpy(), hm.count.cpu().numpy()
        x0, y0, cell = f32(X0), f32(Y0), f32(0.05)
        for e in range(B):
            p, s = pts[e].reshape(-1, 3), S[e].reshape(-1)
            ok = ~np.isnan(p[:, 0])
            m = ref.EPS * s + 2.0 ** -22 * (np.abs(p[:, 0] - x0) + np.abs(p[:, 1] - y0))
            cand = ok & (p[:, 2] + m >= f32(-0.05)) & (p[:, 2] - m <= f32(0.05))
            other = np.zeros((ny, nx), bool)              # cells that a non-floor pixel may have entered
            dmax = np.zeros((ny, nx))
            fl, d = floor[e].reshape(-1), depth[e].reshape(-1).astype(np.float64)
            for sx in (-1, 1):
                for sy in (-1, 1):      # a box smaller than a cell meets exactly the cells of its corners
                    ix = np.floor((p[:, 0] + sx * m - x0) / cell)
                    iy = np.floor((p[:, 1] + sy * m - y0) / cell)
                    inside = cand & (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
                    ii, jj = iy[inside].astype(np.int64), ix[inside].astype(np.int64)
                    other[ii[~fl[inside]], jj[~fl[inside]]] = True
                    np.maximum.at(dmax, (ii, jj), d[inside])
            cells = (n[e] > 0) & ~other
            worst = float((np.abs(h[e][cells]) / (1e-4 + 1e-4 * dmax[cells])).max()) if cells.any() else 0.0
            print(cam.name, "env", e, "floor-only cells", int(cells.sum()), "of", int((n[e] > 0).sum()), "occupied; worst |height| / bound %.3f" % worst)
            assert (np.abs(h[e][cells]) <= 1e-4 + 1e-4 * dmax[cells]).all(), (cam.name, e, worst)
            if cam == r.cams.cam_d405_depth:
                assert int(cells.sum()) >= 50, (e, int(cells.sum()))
