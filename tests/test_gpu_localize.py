"""Monte Carlo localisation on the HIP path: smj_scan_to_particles through the C-ABI and StretchBatchSimulator.pull_particle_update.

One simulator for the module, the rig of tests/test_gpu_mapping.py: stretch_scene, three envs driven apart, 200 steps, the lidar on.
The scans fed to the entry are synthetic: ranges cast in fp64 in the room of tests/scanmatch_ref.py along the rays the rig's XPOSE
gives in the robot's frame, with NaN, -1, ranges below r_min, above r_max and +inf among them.  The kernel is compared in the two
stages of the reference (tests/localize_ref.py): every S_j within [S_lo, S_hi] of cells_of() / sums() (at most 2 % of an env's
(particle, point) pairs unsure), and stat, ancestors, particle_out and pose_out against resample() on the device's own weights, bit
for bit.  The closed loop -- weigh, resample, add noise, again -- runs on the device with the inputs of tests/test_localize_ref.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import localize_ref as ref
import mapping_ref
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
# (nx, ny, origin, cell): both float-stage grids (the second has an odd per-env stride, so the field's 16-byte copy starts
# misaligned), one cell, and the widest grid the entry takes
GRIDS = [(128, 96, (-3.187, -2.379), CELL), (37, 29, (-0.913, -0.707), CELL), (1, 1, (-2.0, -2.0), 4.0), (4096, 16, (-102.4, -0.4), CELL)]
DRAWS = (0, 1, 0x80000000, 0xFFFFFFFF, None)      # None: random words
SPANS = (1, 4096, 1 << 18)


@pytest.fixture(scope="module")
def rig():
    r = perception_rig.scan_rig(K)
    r.n = [int(np.isfinite(r.pts[e]).all(-1).sum()) for e in range(B)]      # the counting rays
    yield r
    r.sim.stop()


def _field(nx, ny, seed=1):
    """uint8 [B, ny, nx]: a third of the cells 0, the rest anything."""
    rng = np.random.default_rng(seed + nx)
    return np.where(rng.random((B, ny, nx)) < 0.33, 0, rng.integers(0, 256, (B, ny, nx))).astype(np.uint8)


def _noise(P, seed=4):
    return (np.array([0.02, 0.02, 0.01])[:, None, None] * np.random.default_rng(seed + P).standard_normal((3, B, P))).astype(np.float32)


def _draws(draw, seed=6):
    return np.random.default_rng(seed).integers(0, 1 << 32, B, dtype=np.uint64).astype(np.uint32) if draw is None else np.full(B, draw, np.uint32)


def _outputs(P):
    return dict(out=torch.full((3, B, P), float(FILL), device=DEV), weight=torch.full((B, P), FILL, dtype=torch.int32, device=DEV),
                anc=torch.full((B, P), FILL, dtype=torch.int32, device=DEV), stat=torch.full((B, 8), FILL, dtype=torch.int32, device=DEV),
                pose=torch.full((3, B), float(FILL), device=DEV))


def _mcl(r, scan, field, parts, nx, ny, origin, cell=CELL, *, noise=None, draw=None, span=4096, min_points=30, resample=1, out=None, anc=True, pose=True,
         limits=LIMITS, rc=0, ld=None):
    """The C call on device tensors; returns the dict of outputs (what they held where nothing is written).  draw: a uint32 array."""
    P = parts.shape[2]
    if out is None:
        out = _outputs(P)
    ptr = perception_rig.ptr
    draw_d = None if draw is None else _dev(np.asarray(draw, np.uint32).view(np.int32))
    got = r.L.smj_scan_to_particles(r.sim._ctx, ptr(scan), scan.stride(0) if ld is None else ld, r.base, limits[0], limits[1], ptr(field), nx, ny, origin[0], origin[1], cell,
                                    ptr(parts), P, ptr(noise), ptr(draw_d), span, min_points, resample, ptr(out["out"]), ptr(out["weight"]), ptr(out["anc"]) if anc else None,
                                    ptr(out["stat"]), ptr(out["pose"]) if pose else None, _stream())
    assert got == rc, (got, r.L.smj_last_error(r.sim._ctx))
    torch.cuda.synchronize()      # draw_d is a temporary: held until the kernel has run
    return out


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _equal_resample(tag, r, got, parts, noise, draw, span, min_points, resample, n=None):
    """stat, ancestors, particle_out and pose_out of the device equal ref.resample() fed the device's own weights, bit for bit."""
    torch.cuda.synchronize()
    weight, stat, anc = got["weight"].cpu().numpy(), got["stat"].cpu().numpy(), got["anc"].cpu().numpy()
    out, pose = got["out"].cpu().numpy(), got["pose"].cpu().numpy()
    results = []
    for e in range(B):
        res = ref.resample(weight[e], draw[e] if draw is not None else 0, span, min_points, (r.n if n is None else n)[e], resample)
        assert stat[e].tolist() == res.stat, (tag, e, stat[e].tolist(), res.stat)
        assert anc[e].tolist() == res.ancestors, (tag, e, "ancestors", np.argwhere(anc[e] != np.array(res.ancestors))[:5].tolist())
        ran = res.status == ref.OK and resample
        want = ref.move(parts[:, e], res.ancestors, noise[:, e] if noise is not None and ran else None)
        assert np.array_equal(_bits(out[:, e]), _bits(want)), (tag, e, "particle_out", np.argwhere(_bits(out[:, e]) != _bits(want))[:5].tolist())
        assert np.array_equal(_bits(pose[:, e]), ref.pose_bits(parts[:, e], res.stat)), (tag, e, "pose_out", pose[:, e].tolist())
        results.append(res)
    return results


@pytest.mark.parametrize("P", ref.SHAPES)
@pytest.mark.parametrize("nx,ny,origin", FS.grids)
def test_float_stage_weights_lie_within_the_references_interval(rig, nx, ny, origin, P):
    """Every device S_j lies in [S_lo, S_hi] on a random field; on a constant field of 200 a particle without unsure points has
    exactly 200 x its on-grid count.  One placement per env serves both fields."""
    r = rig
    parts = ref.float_stage_particles(P)
    fields = (_field(nx, ny), np.full((B, ny, nx), 200, np.uint8))
    got = [_mcl(r, r.scan, _dev(f), _dev(parts), nx, ny, origin, resample=0)["weight"].cpu().numpy() for f in fields]
    for e in range(B):
        cells = ref.cells_of(r.pts[e], r.mar[e], parts[:, e], origin[0], origin[1], CELL, nx, ny)
        share = float(cells.unsure.mean())
        assert cells.n == r.n[e] >= 200 and share <= ref.MAX_AMBIGUOUS, (e, share)
        for f, g in zip(fields, got):
            w = ref.sums(cells, f[e])
            bad = np.nonzero((g[e] < w.lo) | (g[e] > w.hi))[0]
            assert len(bad) == 0, (e, len(bad), [(int(j), int(g[e, j]), int(w.lo[j]), int(w.hi[j])) for j in bad[:5]])
        sure = ~cells.unsure.any(1)
        on = ((cells.mid[..., 0] >= 0) & (cells.mid[..., 0] < nx) & (cells.mid[..., 1] >= 0) & (cells.mid[..., 1] < ny)).sum(1)
        assert np.array_equal(got[1][e][sure], 200 * on[sure])
        dead = ~np.isfinite(parts[:, e]).all(0)
        assert (got[0][e][dead] == 0).all() and (got[1][e][dead] == 0).all()
        print(f"{nx} x {ny} P {P} env {e}: unsure share {share:.5f}, particles without an unsure point {int(sure.sum())}, S up to {int(got[0][e].max())}")
        assert P < 64 or (sure.sum() >= 1 and (got[1][e] > 0).sum() >= P // 2)


@pytest.mark.parametrize("P", ref.SHAPES)
@pytest.mark.parametrize("nx,ny,origin,cell", GRIDS)
def test_integer_stage_equals_the_reference(rig, nx, ny, origin, cell, P):
    r = rig
    parts = ref.float_stage_particles(P)
    field = _dev(_field(nx, ny) if nx > 1 else np.full((B, 1, 1), 200, np.uint8))
    parts_d, noise = _dev(parts), _noise(P)
    noise_d = _dev(noise)
    seen = set()
    combos = [(d, s, (i % 2 == 0), 1) for i, (d, s) in enumerate((d, s) for d in DRAWS for s in SPANS)] + [(None, 4096, True, 0), (1, 1, False, 0)]
    for draw, span, with_noise, resample in combos:
        words = _draws(draw)
        got = _mcl(r, r.scan, field, parts_d, nx, ny, origin, cell, noise=noise_d if with_noise else None, draw=words, span=span, resample=resample)
        res = _equal_resample((nx, ny, P, draw, span, with_noise, resample), r, got, parts, noise if with_noise else None, words, span, 30, resample)
        seen |= {x.status for x in res}
        if resample:
            assert all(x.stat[7] >= 1 for x in res if x.status == ref.OK)
    w = got["weight"].cpu().numpy()
    print(f"{nx} x {ny} P {P}: S up to {w.max(1).tolist()}, statuses {sorted(seen)}")
    assert ref.OK in seen or P < 7      # a single particle may lie off a small grid


def test_corner_cases(rig):
    r = rig
    nx, ny, origin = 128, 96, (-3.187, -2.379)
    P = 257
    field = _dev(np.full((B, ny, nx), 200, np.uint8))
    words = _draws(None)
    prior = np.repeat(np.ascontiguousarray(FS.prior.T)[:, :, None], P, 2)                                   # [3, B, P], every particle the prior
    # all particles off the grid: LOST, the identity, NaN bits in pose_out
    far = prior.copy()
    far[0] += 1000.0
    got = _mcl(r, r.scan, field, _dev(far), nx, ny, origin, noise=_dev(_noise(P)), draw=words)
    res = _equal_resample("off the grid", r, got, far, _noise(P), words, 4096, 30, 1)
    assert all(x.status == ref.LOST and x.ancestors == list(range(P)) for x in res) and int(got["weight"].abs().max()) == 0
    assert bool((got["pose"].view(torch.int32) == 0x7FC00000).all()) and np.array_equal(_bits(got["out"].cpu().numpy()), _bits(far))
    # one particle on the grid: every ancestor is that particle
    one = far.copy()
    one[:, :, 100] = prior[:, :, 100]
    got = _mcl(r, r.scan, field, _dev(one), nx, ny, origin, draw=words)
    res = _equal_resample("one on the grid", r, got, one, None, words, 4096, 30, 1)
    assert all(x.status == ref.OK and x.ancestors == [100] * P and x.stat[0] == 100 and x.stat[5] == 1 and x.stat[7] == 1 for x in res)
    assert np.array_equal(_bits(got["pose"].cpu().numpy()), _bits(prior[:, :, 100]))
    # all S equal: the best is particle 0 and every slot keeps its own particle
    got = _mcl(r, r.scan, field, _dev(prior), nx, ny, origin, draw=words, span=1)
    res = _equal_resample("all equal", r, got, prior, None, words, 1, 30, 1)
    assert all(x.status == ref.OK and x.stat[0] == 0 and x.ancestors == list(range(P)) and x.stat[5] == P and x.stat[7] == P for x in res)
    # FEW, through min_points: one more than any env has
    got = _mcl(r, r.scan, field, _dev(prior), nx, ny, origin, draw=words, min_points=max(r.n) + 1)
    res = _equal_resample("few", r, got, prior, None, words, 4096, max(r.n) + 1, 1)
    assert all(x.status == ref.FEW and x.stat[0] == -1 and x.stat[1] > 0 for x in res) and bool((got["pose"].view(torch.int32) == 0x7FC00000).all())
    # a particle that is not finite weighs nothing and dies out
    mixed = ref.float_stage_particles(P)
    got = _mcl(r, r.scan, field, _dev(mixed), nx, ny, origin, draw=words, span=1 << 18)
    res = _equal_resample("not finite", r, got, mixed, None, words, 1 << 18, 30, 1)
    for e in range(B):
        dead = np.nonzero(~np.isfinite(mixed[:, e]).all(0))[0]
        assert len(dead) >= 20 and (got["weight"][e].cpu().numpy()[dead] == 0).all() and not set(dead.tolist()) & set(res[e].ancestors)
        assert np.isfinite(got["out"][:, e].cpu().numpy()).all()


def test_guarded_outputs_and_a_padded_scan(rig):
    """The outputs 4 bytes past a 16-byte boundary inside guard words, and the scan with lidar_ld > num_envs inside canaries: the
    packed call's bits, guards and canaries as they were."""
    r = rig
    nx, ny, origin = 37, 29, (-0.913, -0.707)
    P = 257
    parts, noise, words = ref.float_stage_particles(P), _noise(P), _draws(None)
    field, parts_d, noise_d = _dev(_field(nx, ny)), _dev(parts), _dev(noise)
    plain = _mcl(r, r.scan, field, parts_d, nx, ny, origin, noise=noise_d, draw=words)
    g = dict(out=Guarded(37, P, 3), weight=Guarded(37, P, 1), anc=Guarded(37, P, 1), stat=Guarded(37, 8, 1), pose=Guarded(37, 3, 1))
    views = dict(out=g["out"].view.view(-1).view(torch.float32).view(3, B, P), weight=g["weight"].view.view(B, P), anc=g["anc"].view.view(B, P),
                 stat=g["stat"].view.view(B, 8), pose=g["pose"].view.view(-1).view(torch.float32).view(3, B))
    assert all(v.data_ptr() % 16 == 4 for v in views.values())
    canary = torch.tensor([0x7FC0BEEF], dtype=torch.int32).view(torch.float32).item()
    ld = B + 4
    store = torch.full((K + 2, ld), canary, dtype=torch.float32, device=DEV)
    store[1:K + 1, :B] = r.scan
    _mcl(r, store[1:K + 1], field, parts_d, nx, ny, origin, noise=noise_d, draw=words, out=views, ld=ld)
    for name, guard in g.items():
        guard.check(plain[name].view(torch.int32).reshape(guard.view.shape))
    bits = store.view(torch.int32)
    assert bool((bits[0] == 0x7FC0BEEF).all()) and bool((bits[K + 1] == 0x7FC0BEEF).all()) and bool((bits[:, B:] == 0x7FC0BEEF).all())
    assert store[1:K + 1, :B].cpu().numpy().tobytes() == r.scan.cpu().numpy().tobytes()
    assert plain["stat"][:, 3].tolist() == [ref.OK] * B
    # null optional outputs are left untouched
    part = _mcl(r, r.scan, field, parts_d, nx, ny, origin, noise=noise_d, draw=words, anc=False, pose=False)
    assert int((part["anc"] != FILL).sum()) == 0 and int((part["pose"] != FILL).sum()) == 0
    assert all(torch.equal(part[k], plain[k]) for k in ("out", "weight", "stat"))


def test_two_calls_give_identical_bytes(rig):
    r = rig
    nx, ny, origin = 128, 96, (-3.187, -2.379)
    P = 4096
    parts, noise, words = ref.float_stage_particles(P), _noise(P), _draws(None)
    field, parts_d, noise_d = _dev(_field(nx, ny)), _dev(parts), _dev(noise)
    runs = [_mcl(r, r.scan, field, parts_d, nx, ny, origin, noise=noise_d, draw=words) for _ in range(2)]
    assert all(runs[0][k].cpu().numpy().tobytes() == runs[1][k].cpu().numpy().tobytes() for k in runs[0])
    assert runs[0]["stat"][:, 3].tolist() == [ref.OK] * B and bool((runs[0]["stat"][:, 7] > 1).all())
    assert parts_d.cpu().numpy().tobytes() == parts.tobytes() and noise_d.cpu().numpy().tobytes() == noise.tobytes()      # the inputs are unchanged


def test_error_codes_and_a_refused_call_writes_nothing(rig, bare):
    r = rig
    L, sim = r.L, r.sim
    nx = ny = 32
    P = 8
    nbody = sim.xpose.shape[0] // 12
    sizes = dict(scan=K * B, field=B * nx * ny // 4, particle=3 * B * P, noise=3 * B * P, draw=B, out=3 * B * P, weight=B * P, anc=B * P, stat=8 * B, pose=3 * B)
    pool = torch.zeros(sum(sizes.values()) + 64, dtype=torch.int32, device=DEV)      # one allocation, so that ranges can be made to overlap
    at, p = {}, pool.data_ptr()
    for name, words in sizes.items():
        at[name] = p
        p += 4 * ((words + 3) // 4 * 4)      # every range starts on a 16-byte boundary
    good = dict(ld=B, frame=r.base, r_min=0.2, r_max=5.0, nx=nx, ny=ny, x0=-0.81, y0=-0.81, cell=0.05, P=P, span=4096, min_points=30, resample=1)

    def call(a, ctx=None, **ptrs):
        q = dict(at, **ptrs)
        vp = lambda v: ctypes.c_void_p(v) if v else None
        return L.smj_scan_to_particles(ctx or sim._ctx, vp(q["scan"]), a["ld"], a["frame"], a["r_min"], a["r_max"], vp(q["field"]), a["nx"], a["ny"], a["x0"], a["y0"], a["cell"],
                                       vp(q["particle"]), a["P"], vp(q["noise"]), vp(q["draw"]), a["span"], a["min_points"], a["resample"], vp(q["out"]), vp(q["weight"]),
                                       vp(q["anc"]), vp(q["stat"]), vp(q["pose"]), _stream())

    bad = [dict(ld=B - 1), dict(ld=0), dict(ld=-5), dict(nx=0), dict(ny=0), dict(nx=-4), dict(ny=-1), dict(nx=257, ny=256), dict(nx=256, ny=257), dict(nx=65537, ny=1),
           dict(nx=4097, ny=1), dict(nx=1, ny=4097), dict(nx=1 << 20, ny=1 << 20), dict(cell=0.0), dict(cell=-0.05), dict(cell=NaN), dict(cell=INF), dict(x0=NaN), dict(x0=INF),
           dict(y0=-INF), dict(y0=NaN), dict(r_min=NaN), dict(r_max=NaN), dict(r_max=INF), dict(r_min=-0.1), dict(r_min=-INF), dict(r_min=5.5), dict(r_max=0.1),
           dict(cell=0.0005, r_max=4.2), dict(cell=1e-3, r_max=8.5), dict(frame=r.lib.FRAME_WORLD), dict(frame=r.lib.FRAME_CAMERA), dict(frame=-3), dict(frame=10 ** 6),
           dict(frame=nbody), dict(P=0), dict(P=-1), dict(P=4097), dict(span=0), dict(span=-3), dict(span=(1 << 18) + 1), dict(min_points=0), dict(min_points=1025),
           dict(resample=2), dict(resample=-1)]
    for change in bad:
        rc = call(dict(good, **change))
        assert rc == -1 and L.smj_last_error(sim._ctx), (change, rc)
    for name in ("scan", "field", "particle", "out", "weight", "stat", "draw"):      # null required pointers; the draw is required with resample = 1
        assert call(good, **{name: None}) == -1, name
    for name, by in (("scan", 2), ("particle", 1), ("noise", 3), ("draw", 2), ("out", 1), ("weight", 2), ("anc", 3), ("stat", 1), ("pose", 2)):
        assert call(good, **{name: at[name] + by}) == -1 and b"aligned" in L.smj_last_error(sim._ctx), (name, by)
    # overlap: an output on an input, on another output, on the bound XPOSE array, by a whole range and by one word at either end
    last = lambda name: 4 * (sizes[name] - 1)
    for kw in (dict(out=at["scan"]), dict(out=at["particle"]), dict(out=at["noise"]), dict(weight=at["field"]), dict(anc=at["draw"]), dict(stat=at["particle"]),
               dict(pose=at["noise"]), dict(weight=at["out"]), dict(anc=at["weight"]), dict(stat=at["anc"]), dict(pose=at["stat"]), dict(pose=at["out"]),
               dict(out=at["particle"] + last("particle")), dict(out=at["particle"] - last("out")), dict(weight=at["draw"] + last("draw")), dict(stat=at["draw"] - last("stat")),
               dict(pose=at["field"] + 4 * (sizes["field"] - 1)), dict(anc=at["weight"] + last("weight")), dict(stat=at["pose"] - last("stat")),
               dict(particle=at["stat"] + last("stat")), dict(noise=at["weight"] - last("noise")), dict(scan=at["anc"] - last("scan")),
               dict(out=sim.xpose.data_ptr()), dict(stat=sim.xpose.data_ptr() + 4 * (sim.xpose.numel() - 1))):
        assert call(good, **kw) == -1 and b"overlap" in L.smj_last_error(sim._ctx), kw
    xpose_before = sim.xpose.clone()
    torch.cuda.synchronize()
    assert int(pool.abs().max()) == 0      # a refused call writes nothing
    # a bare context (nothing bound): -5, after every -1
    assert call(good, ctx=bare.ctx) == -5 and b"XPOSE" in L.smj_last_error(bare.ctx)
    assert call(dict(good, P=0), ctx=bare.ctx) == -1 and call(dict(good, frame=nbody), ctx=bare.ctx) == -1
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
            assert call(dict(good, span=0), ctx=ctx) == -6      # -6 comes first
        finally:
            L.smj_destroy(ctx)
    torch.cuda.synchronize()
    assert int(pool.abs().max()) == 0 and torch.equal(sim.xpose, xpose_before)
    # accepted: the extremes of every argument, null optional pointers (the draw too without resampling), adjacent ranges, the last body
    for change, ptrs in ((dict(r_min=0.0, r_max=0.0), {}), (dict(cell=0.0009765625, r_max=8.0), {}), (dict(cell=1e-30, x0=-3e38, y0=3e38, r_min=0.0, r_max=1e-27), dict(noise=None, anc=None, pose=None)),
                         (dict(frame=nbody - 1), {}), (dict(resample=0), dict(draw=None)), (dict(span=1, min_points=1), {}), (dict(span=1 << 18, min_points=1024), {}),
                         (dict(P=1), {}), (dict(nx=1, ny=1), {}), ({}, {})):
        assert call(dict(good, **change), **ptrs) == 0, (change, L.smj_last_error(sim._ctx))
    torch.cuda.synchronize()
    words = lambda name: pool[(at[name] - pool.data_ptr()) // 4:][:sizes[name]]
    # all-zero inputs: every range 0 is below r_min, so no ray counts: FEW, the particles as they went in, NaN in pose_out
    assert words("stat").view(B, 8).tolist() == [[-1, 0, 0, ref.FEW, 0, 0, 0, 0]] * B and bool((words("pose") == 0x7FC00000).all())
    assert words("anc").view(B, P).tolist() == [list(range(P))] * B
    assert all(int(words(name).abs().max()) == 0 for name in ("scan", "field", "particle", "noise", "draw", "out", "weight"))      # the inputs are unchanged


def test_the_status_gates_the_mapping_entry_where_it_lies(rig):
    """smj_scan_to_map(gate = stat + 3, gate_ld = 8) equals the status column copied out; pose_out of a LOST env gives SMJ_MAP_OFF."""
    r = rig
    ptr = perception_rig.ptr
    nx, ny, origin = 128, 96, (-3.187, -2.379)
    P = 64
    scan = r.scan_host.copy()
    scan[20:, 1] = -1.0                                       # env 1: too few returns
    parts = np.repeat(np.ascontiguousarray(FS.prior.T)[:, :, None], P, 2).copy()
    parts[0, 2] += 1000.0                                     # env 2: every particle off the grid
    scan_d, field = _dev(scan), _dev(np.full((B, ny, nx), 200, np.uint8))
    got = _mcl(r, scan_d, field, _dev(parts), nx, ny, origin, draw=_draws(None))
    assert got["stat"][:, 3].tolist() == [ref.OK, ref.FEW, ref.LOST]

    def to_map(pose, gate, gate_ld):
        out = [torch.zeros(B, ny, nx, dtype=torch.int32, device=DEV), torch.zeros(B, ny, nx, dtype=torch.int32, device=DEV), torch.zeros(B, 4, dtype=torch.int32, device=DEV)]
        rc = r.L.smj_scan_to_map(r.sim._ctx, ptr(scan_d), B, r.base, LIMITS[0], LIMITS[1], ptr(pose), gate, gate_ld, origin[0], origin[1], CELL, nx, ny, 1, 0, ptr(out[0]),
                                 ptr(out[1]), ptr(out[2]), None, _stream())
        assert rc == 0, r.L.smj_last_error(r.sim._ctx)
        torch.cuda.synchronize()
        return out

    finite = _dev(np.ascontiguousarray(FS.prior.T))
    copied_gate = got["stat"][:, 3].contiguous()
    in_place = to_map(finite, ctypes.c_void_p(got["stat"].data_ptr() + 12), 8)
    copied = to_map(finite, ptr(copied_gate), 1)
    assert all(torch.equal(a, b) for a, b in zip(in_place, copied))
    assert in_place[2][:, 0].tolist() == [mapping_ref.OK, mapping_ref.GATED, mapping_ref.GATED] and int(in_place[0][0].sum()) >= 200 and int(in_place[0][1:].abs().max()) == 0
    # pose_out as the pose, no gate: the envs that are not OK hold NaN, which the mapping entry turns away by itself
    by_pose = to_map(got["pose"], None, 1)
    assert by_pose[2][:, 0].tolist() == [mapping_ref.OK, mapping_ref.OFF, mapping_ref.OFF] and int(by_pose[0][0].sum()) >= 200
    assert got["stat"][:, 3].tolist() == [ref.OK, ref.FEW, ref.LOST]      # the gate is an input


def test_pull_particle_update_and_the_views(rig):
    """pull_particle_update equals the C call at the same arguments; update.particles goes into the next call as it is; mean() and
    spread() against fp64 numpy."""
    from stretch_mujoco_amd import utils
    from stretch_mujoco_amd.datamodels import StatusStretchParticles

    r = rig
    sim = r.sim
    nx, ny, origin = 128, 96, (-3.187, -2.379)
    P = 1000
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    parts = utils.spread_particles(sim.base_pose, (0.5, 0.5, 0.3), P, generator=gen)
    noise = utils.particle_noise(0.02, 0.01, (3, B, P), generator=gen)
    assert parts.shape == (3, B, P) and parts.dtype == torch.float32 and noise.shape == (3, B, P) and noise.device == parts.device
    assert bool(((parts - sim.base_pose.unsqueeze(2)).abs().amax(2) <= torch.tensor([0.5, 0.5, 0.3], device=DEV).unsqueeze(1) + 1e-6).all())
    assert 0.015 < float(noise[:2].std()) < 0.025 and 0.007 < float(noise[2].std()) < 0.013
    og = sim.pull_occupancy_grid(frame="world", shape=(ny, nx), origin=origin)
    df = sim.pull_distance_field(og)
    field = df.likelihood(0.10).contiguous()
    draw = _draws(None)
    draw_d = _dev(draw.astype(np.int64))
    up = sim.pull_particle_update(df, parts, noise, draw_d, span=2000, min_points=20, ancestors=True)
    assert isinstance(up, StatusStretchParticles) and up.frame == "world" and up.origin == origin and up.cell == CELL
    scan = sim.lidar[:K].clone()
    want = _mcl(r, scan, field, parts, nx, ny, origin, noise=noise, draw=draw, span=2000, min_points=20)
    assert torch.equal(up.weights, want["weight"]) and torch.equal(up.stat, want["stat"]) and torch.equal(up.ancestors, want["anc"])
    assert up.particles.cpu().numpy().tobytes() == want["out"].cpu().numpy().tobytes() and up.pose.cpu().numpy().tobytes() == want["pose"].cpu().numpy().tobytes()
    assert up.ok().tolist() == [True] * B and up.few().tolist() == [False] * B and up.lost().tolist() == [False] * B and up.status.tolist() == [0] * B
    assert torch.equal(up.best(), up.stat[:, 0]) and torch.equal(up.ess(), up.stat[:, 5]) and torch.equal(up.total(), up.stat[:, 4]) and bool((up.ess() >= 1).all())
    assert torch.equal(up.w().sum(1).to(torch.int32), up.total())
    # mean() against fp64 numpy.  The issue's bound: an fp32 sum of P terms is off by at most P ulp of its largest partial sum, the
    # weighted sum and the sum of weights each, and their quotient by the two relative errors added and two more roundings: below
    # 4 P ulp of the largest coordinate.  (mean() sums in fp64, so it meets the bound with room.)
    w = up.w().cpu().numpy().astype(np.float64)
    x = parts.cpu().numpy().astype(np.float64)
    tot = w.sum(1)
    mean = np.stack(((w * x[0]).sum(1) / tot, (w * x[1]).sum(1) / tot, np.arctan2((w * np.sin(x[2])).sum(1), (w * np.cos(x[2])).sum(1))))
    bound = 4 * P * np.spacing(np.float32(np.abs(x).max()))
    got = up.mean().cpu().numpy().astype(np.float64)
    print(f"mean() off the fp64 mean by {np.abs(got - mean).max():.3e}, bound {bound:.3e}")
    assert up.mean().dtype == torch.float32 and np.abs(got - mean).max() <= bound
    sd = np.sqrt(np.stack(((w * (x[0] - mean[0][:, None]) ** 2).sum(1) / tot, (w * (x[1] - mean[1][:, None]) ** 2).sum(1) / tot)))
    assert np.allclose(up.spread().cpu().numpy()[:2], sd, rtol=1e-4, atol=1e-6) and bool((up.spread()[2] >= 0).all()) and bool((up.spread()[2] < 0.4).all())
    # the next call takes update.particles as it is (the two simulator-owned sets take turns), a bare field, and its own draws
    first = up.particles.clone()
    nxt = sim.pull_particle_update(field, up.particles, origin=origin, cell=CELL)
    assert nxt.particles.data_ptr() != up.particles.data_ptr() and torch.equal(up.particles, first) and nxt.frame == "grid" and nxt.ancestors is None
    assert nxt.prior.data_ptr() == up.particles.data_ptr() and nxt.ok().all()
    again = sim.pull_particle_update(field, nxt.particles, origin=origin, cell=CELL, resample=False)
    assert again.particles.data_ptr() == up.particles.data_ptr() and torch.equal(again.particles, nxt.particles) and int(again.stat[:, 7].abs().max()) == 0
    # predict(): the robot's own frame
    moved = again.predict((0.1, 0.0, 0.2))
    th = again.particles[2]
    assert torch.allclose(moved[0], again.particles[0] + 0.1 * torch.cos(th)) and torch.allclose(moved[1], again.particles[1] + 0.1 * torch.sin(th))
    assert torch.allclose(moved[2], th + 0.2) and moved.data_ptr() != again.particles.data_ptr()
    per_env = again.predict(torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.0]], device=DEV).t().contiguous(), noise=noise)
    assert torch.allclose(per_env[1, 1], again.particles[1, 1] + 0.5 * torch.cos(th[1]) + noise[1, 1]) and torch.allclose(per_env[:, 0], again.particles[:, 0] + noise[:, 0])
    # an occupancy grid goes through the distance field by itself; the best particle is a prior the matcher takes
    via_grid = sim.pull_particle_update(og, parts, noise, draw_d, span=2000, min_points=20)
    assert torch.equal(via_grid.weights, want["weight"]) and torch.equal(via_grid.stat, want["stat"])
    match = sim.pull_scan_match(df, via_grid.pose)
    assert match.ok().all()


def test_value_errors_are_raised_before_any_launch(rig):
    from stretch_mujoco_amd.datamodels import StatusStretchDistanceField

    sim = rig.sim
    dev = sim.device
    P = 16
    parts = sim.base_pose.unsqueeze(2).repeat(1, 1, P).contiguous()
    og = sim.pull_occupancy_grid(frame="world")
    df = sim.pull_distance_field(og)
    keep = sim.pull_particle_update(df, parts, ancestors=True)
    torch.cuda.synchronize()
    tensors = (keep.particles, keep.weights, keep.ancestors, keep.stat, keep.pose, df.dist2)
    snap = [t.clone() for t in tensors]
    odd = lambda **kw: StatusStretchDistanceField(**dict(dict(time=0, dist2=df.dist2, nearest=None, origin=df.origin, cell=df.cell, frame="world"), **kw))
    u8 = torch.zeros(B, 8, 8, dtype=torch.uint8, device=dev)
    for f, p, kw in ((df, "particles", {}), (df, parts[:2], {}), (df, parts[:, :2], {}), (df, parts.to(torch.int32), {}), (df, parts.cpu(), {}), (df, parts[:, :, :0], {}),
                     (df, torch.zeros(3, B, 4097, device=dev), {}), (df, parts.reshape(3, B * P), {}),
                     (df, parts, dict(noise=parts[:, :, :5])), (df, parts, dict(noise=parts.cpu())), (df, parts, dict(noise=parts.to(torch.int32))), (df, parts, dict(noise="no")),
                     (df, parts, dict(draw=torch.zeros(B, device=dev))), (df, parts, dict(draw=torch.zeros(B + 1, dtype=torch.int32, device=dev))),
                     (df, parts, dict(draw=torch.zeros(B, dtype=torch.int32))), (df, parts, dict(draw=[0, 0, 0])), (df, parts, dict(draw=torch.zeros(B, dtype=torch.bool, device=dev))),
                     (df, parts, dict(span=0)), (df, parts, dict(span=(1 << 18) + 1)), (df, parts, dict(min_points=0)), (df, parts, dict(min_points=1025)),
                     (df, parts, dict(range_limits=(0.2,))), (df, parts, dict(range_limits=(-0.1, 5.0))), (df, parts, dict(range_limits=(5.0, 0.2))),
                     (df, parts, dict(range_limits=(0.2, INF))), (df, parts, dict(range_limits=(0.2, 500.0))), (df, parts, dict(sigma=0.0)), (df, parts, dict(sigma=NaN)),
                     (odd(frame="base"), parts, {}), (odd(dist2=df.dist2.to(torch.int64)), parts, {}), (odd(dist2=df.dist2[:2]), parts, {}), (odd(dist2=df.dist2.cpu()), parts, {}),
                     (odd(cell=0.0), parts, {}), (u8, parts, {}), (u8, parts, dict(origin=(0.0, 0.0))), (u8, parts, dict(cell=0.05)), (u8.to(torch.int32), parts, dict(origin=(0.0, 0.0), cell=0.05)),
                     (u8[:2], parts, dict(origin=(0.0, 0.0), cell=0.05)), (torch.zeros(B, 300, 300, dtype=torch.uint8, device=dev), parts, dict(origin=(0.0, 0.0), cell=0.05)),
                     ("field", parts, {})):
        with pytest.raises(ValueError):
            sim.pull_particle_update(f, p, **kw)
            print("accepted:", type(f).__name__, type(p).__name__, sorted(kw))      # reached only when nothing was raised
    torch.cuda.synchronize()
    assert all(torch.equal(x, t) for x, t in zip(snap, tensors))      # nothing ran
    # accepted: fp64 particles and noise (converted), uint8 fields with origin and cell, int64 draws
    up = sim.pull_particle_update(u8, parts.double(), parts.double() * 0, torch.full((B,), (1 << 32) - 1, dtype=torch.int64, device=dev), origin=(-0.2, -0.2), cell=0.05)
    assert up.lost().all() and torch.equal(up.particles, parts)


def test_the_loop_finds_the_robots_on_the_device(rig):
    """The closed loop of tests/test_localize_ref.py through the C-ABI, with its seeded particles, noise and draws and the rig's own
    rays: after LOOP.updates updates and for LOOP.extra more the best particle lies within one cell and 2 degrees of the truth -- the
    reference's own result (half of that, tests/localize_ref.py) with a factor of two, since the device may break an unsure cell the
    other way and so take another branch of the resampling.  scanmatch_ref.decide from the spread's centre with the default window
    does not get there.  Nothing is read back inside the loop."""
    from stretch_mujoco_amd.utils import scan_angles

    r = rig
    L, g = ref.LOOP, scanmatch_ref.ROOM_GRID
    inp = ref.loop_inputs()
    field_host = ref.loop_field()
    field = _dev(np.repeat(field_host[None], B, 0))
    scan_host = _rig_scans(r, inp.truth)
    scan = _dev(scan_host)
    ptr = perception_rig.ptr
    sets = [_dev(inp.first), torch.empty(3, B, L.particles, device=DEV)]
    noise = [_dev(v) for v in inp.noise]
    draws = [_dev(v.view(np.int32)) for v in inp.draws]
    weight, stat = torch.empty(B, L.particles, dtype=torch.int32, device=DEV), torch.empty(B, 8, dtype=torch.int32, device=DEV)
    poses, stats = [], []
    for i in range(inp.steps):
        pose = torch.empty(3, B, device=DEV)
        rc = r.L.smj_scan_to_particles(r.sim._ctx, ptr(scan), B, r.base, L.limits[0], L.limits[1], ptr(field), g.nx, g.ny, g.origin[0], g.origin[1], g.cell, ptr(sets[i % 2]),
                                       L.particles, ptr(noise[i]), ptr(draws[i]), L.span, L.min_points, 1, ptr(sets[(i + 1) % 2]), ptr(weight), None, ptr(stat), ptr(pose),
                                       _stream())
        assert rc == 0, r.L.smj_last_error(r.sim._ctx)
        poses.append(pose)
        stats.append(stat.clone())
    torch.cuda.synchronize()
    errors = np.array([[ref.pose_error(p.cpu().numpy()[:, e], inp.truth[e]) for e in range(B)] for p in poses])
    for i in range(inp.steps):
        print(f"update {i:2d}: " + "  ".join(f"({m:.3f} m, {np.rad2deg(a):.2f} deg)" for m, a in errors[i]) + f"  ess {stats[i][:, 5].tolist()}")
    assert all(s[:, 3].tolist() == [ref.OK] * B for s in stats)
    tail = errors[L.updates - 1:]
    assert len(tail) == L.extra + 1 and (tail[..., 0] <= L.bound[0]).all() and (tail[..., 1] <= L.bound[1]).all(), tail.tolist()
    # the matcher alone, from the spread's centre
    angles = scan_angles().angles.numpy()
    W = int(round(0.5 / g.cell))
    for e in range(B):
        pts, mar, _ = scanmatch_ref.frame_points(*r.geoms[e], scan_host[:, e].astype(np.float64), *L.limits)
        prior = inp.center[e].astype(np.float32)[:, None]
        pl = scanmatch_ref.place(pts[None], mar[None], prior, angles, *g.origin, g.cell, g.nx, g.ny)
        dec = scanmatch_ref.decide(pl.cell, field_host[None], prior, angles, g.cell, pl.n, wx=W, wy=W, min_points=30)
        err = ref.pose_error(dec.pose[:, 0], inp.truth[e])
        print(f"env {e}: the matcher from the centre ends ({err[0]:.3f} m, {np.rad2deg(err[1]):.2f} deg) off")
        assert err[0] > L.bound[0] or err[1] > L.bound[1], err


def test_the_example_runs():
    """examples/relocalize_batch.py 2: map, move the robots, localise from a spread of +-1 m and +-30 degrees, in a process of its
    own; the filter followed by the matcher ends within 10 cm and 3 degrees where the matcher alone does not."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "relocalize_batch.py"), "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    rows = {name: [tuple(float(v) for v in m) for m in re.findall(r"\(([\d.]+) cm, ([\d.]+) deg\)", line)]
            for name, line in re.findall(r"^error of (the matcher alone|the filter, then the matcher)\s+(.*)$", out.stdout, flags=re.M)}
    assert len(rows["the matcher alone"]) == len(rows["the filter, then the matcher"]) == 2
    for alone, both in zip(rows["the matcher alone"], rows["the filter, then the matcher"]):
        assert both[0] < 10.0 and both[1] < 3.0 and (alone[0] > both[0] or alone[1] > both[1]), (alone, both)
