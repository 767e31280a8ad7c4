"""Exact distance fields of occupancy grids on the HIP path: smj_occupancy_to_distance through the C-ABI and
StretchBatchSimulator.pull_distance_field.

Most tests run on a bare context -- smj_create on the stretch_scene blob, three envs, NOTHING bound: the entry needs no slot and
no lidar.  Every comparison of dist2 and nearest is integer equality with tests/distance_ref.py (the minimum of (d^2, index) over all
obstacle cells) on every cell; there is no tolerance anywhere.  The reference of a shape is computed once, for R = 0, and shared;
R = 3 applies the reference's own bound rule to it.

Shapes (nx, ny): the smallest at which the kernel can go wrong -- single cells and single rows / columns, 16 x 12, the odd 61 x 83
(no 16-byte row alignment), 64 x 64, 131 x 127 (two strips of 66 and 65 columns), 4096 x 16 and 16 x 4096 (four strips each, the
extremes of the cut), and 256 x 256 (four strips) once."""
import ctypes

import numpy as np
import pytest
import torch

import distance_ref as ref
import perception_rig
from perception_rig import B, DEV, Guarded, ptr as _ptr, same as _same, stream as _stream

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 1), (1, 7), (16, 12), (61, 83), (64, 64), (131, 127), (4096, 16), (16, 4096)]
NONE = 1 << 30


@pytest.fixture(scope="module")
def bare():
    yield from perception_rig.bare_context()


def _edt(b, hit, miss=None, min_hits=1, unknown=0, R=0, nearest=True, out=None, rc=0):
    """One call on [B, ny, nx] int32 device tensors; the outputs start as sentinels."""
    _, ny, nx = hit.shape
    if out is None:
        out = perception_rig.sentinels(ny, nx)
    got = b.L.smj_occupancy_to_distance(b.ctx, _ptr(hit), _ptr(miss), nx, ny, min_hits, unknown, R, _ptr(out[0]), _ptr(out[1]) if nearest else None, _stream())
    assert got == rc, (got, b.L.smj_last_error(b.ctx))
    return out


def _last_strip_c0(nx, ny):
    """First column of the last strip, by the cut smj_edt.h describes: the fewest strips of at most 16384 // ny columns, of equal width."""
    wmax = 16384 // ny
    n = -(-nx // wmax)
    w = -(-nx // n)
    return (-(-nx // w) - 1) * w, -(-nx // w)


def _contents(nx, ny):
    """The twelve grids of a shape, as bool [12, ny, nx]."""
    rng = np.random.default_rng(1000 * nx + ny)
    g = np.zeros((12, ny, nx), bool)
    g[1] = True                                                    # 0 empty, 1 full
    for k, (j, i) in enumerate(((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1))):
        g[2 + k, j, i] = True                                      # 2 .. 5 one obstacle in each corner
    g[6] = rng.random((ny, nx)) < 0.01
    g[7] = rng.random((ny, nx)) < 0.30
    g[8] = np.indices((ny, nx)).sum(0) % 2 == 1                    # checkerboard: ties everywhere
    g[9] = ref.tie_grid(ny, nx)
    c0, _ = _last_strip_c0(nx, ny)
    ys = np.arange(0, ny, 3)
    g[10, ys, c0 + ys % (nx - c0)] = True                          # obstacles in the last strip alone
    g[11] = g[6] | g[9]
    return g


def _reference(b, nx, ny):
    key = (nx, ny)
    if key not in b.cache:
        g = _contents(nx, ny)
        out = [ref.field_of_mask(m) for m in g]
        b.cache[key] = (g, np.stack([o[0] for o in out]), np.stack([o[1] for o in out]))
    return b.cache[key]


def test_strip_cut_of_the_shapes():
    assert _last_strip_c0(64, 64)[1] == 1 and _last_strip_c0(61, 83)[1] == 1 and _last_strip_c0(131, 127) == (66, 2)
    assert _last_strip_c0(4096, 16) == (3072, 4) and _last_strip_c0(16, 4096) == (12, 4) and _last_strip_c0(256, 256) == (192, 4)


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_every_cell_equals_the_reference(bare, nx, ny):
    b = bare
    g, d2, near = _reference(b, nx, ny)
    assert (d2[0] == NONE).all() and (near[0] == -1).all() and (d2[1] == 0).all()
    results = []
    for k in range(0, 12, B):      # a different content per env
        hit = torch.tensor(g[k:k + B].astype(np.int32), device=DEV)
        for R in (0, 3):
            both = _edt(b, hit, R=R)
            only = _edt(b, hit, R=R, nearest=False)
            results.append((k, R, hit, both, only))
    torch.cuda.synchronize()
    for k, R, hit, both, only in results:
        wd, wn = ref.apply_bound(d2[k:k + B], near[k:k + B], R)
        _same(("dist2", nx, ny, k, R), both[0], wd)
        _same(("nearest", nx, ny, k, R), both[1], wn)
        _same(("dist2 alone", nx, ny, k, R), only[0], wd)
        assert int((only[1] != -7).sum()) == 0      # a null nearest_dev: that buffer is not touched
        assert np.array_equal(hit.cpu().numpy(), g[k:k + B].astype(np.int32))


def test_256_x_256_once(bare):
    b = bare
    nx = ny = 256
    rng = np.random.default_rng(256)
    g = np.zeros((B, ny, nx), bool)
    g[0] = rng.random((ny, nx)) < 0.005
    g[1, 255, 255] = True
    g[2] = ref.tie_grid(ny, nx) | (rng.random((ny, nx)) < 0.001)
    assert g.mean() <= 0.02
    want = [ref.field_of_mask(m) for m in g]
    hit = torch.tensor(g.astype(np.int32), device=DEV)
    got0, got20 = _edt(b, hit), _edt(b, hit, R=20)
    torch.cuda.synchronize()
    for e in range(B):
        _same(("dist2", e), got0[0][e], want[e][0])
        _same(("nearest", e), got0[1][e], want[e][1])
        wd, wn = ref.apply_bound(*want[e], 20)
        _same(("dist2 R 20", e), got20[0][e], wd)
        _same(("nearest R 20", e), got20[1][e], wn)


@pytest.mark.parametrize("nx,ny", [(61, 83), (131, 127)])
def test_min_hits_and_unknown_cells(bare, nx, ny):
    b = bare
    rng = np.random.default_rng(nx)
    hit = rng.integers(0, 6, (B, ny, nx)).astype(np.int32) * (rng.random((B, ny, nx)) < 0.1)
    miss = (rng.integers(0, 4, (B, ny, nx)) * (rng.random((B, ny, nx)) < 0.97)).astype(np.int32)
    hit = hit.astype(np.int32)
    h, m = torch.tensor(hit, device=DEV), torch.tensor(miss, device=DEV)
    seen = []
    for min_hits in (1, 3):
        for unknown in (0, 1):
            for R in (0, 3):
                got = _edt(b, h, m, min_hits=min_hits, unknown=unknown, R=R)
                want = ref.field(hit, miss, min_hits, bool(unknown), R)
                _same((min_hits, unknown, R, "dist2"), got[0], want[0])
                _same((min_hits, unknown, R, "nearest"), got[1], want[1])
                if R == 0:
                    seen.append(int((want[0] == 0).sum()))
    assert len(set(seen)) == 4      # the four predicates differ on this input
    # without unknown_is_obstacle the miss layer is not looked at, present or not
    a, c = _edt(b, h, m, min_hits=3), _edt(b, h, None, min_hits=3)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_two_calls_agree_and_envs_do_not_see_each_other(bare):
    b = bare
    for nx, ny in ((61, 83), (131, 127)):
        g, d2, near = _reference(b, nx, ny)
        first = torch.tensor(g[[7, 6, 9]].astype(np.int32), device=DEV)
        second = torch.tensor(g[[1, 0, 7]].astype(np.int32), device=DEV)      # grid 7 in env 2, beside other neighbours
        a, a2, c = _edt(b, first, R=0), _edt(b, first, R=0), _edt(b, second, R=0)
        torch.cuda.synchronize()
        assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])
        assert torch.equal(a[0][0], c[0][2]) and torch.equal(a[1][0], c[1][2])
        _same("env 2", c[0][2], d2[7])


@pytest.mark.parametrize("nx,ny", [(61, 83), (131, 127)])
def test_nothing_outside_the_outputs_is_written_and_alignment_does_not_matter(bare, nx, ny):
    """A one-strip and a two-strip grid.  The outputs as views 4 bytes past a 16-byte boundary inside buffers of sentinels: the guards
    stay untouched and the values are those of the aligned call; the same with the inputs 4 bytes past a 16-byte boundary, with
    both, and with only one of the two outputs misaligned."""
    b = bare
    rng = np.random.default_rng(ny)
    cells, pad = B * nx * ny, 37      # 37 words = 148 bytes = 4 mod 16
    hit = torch.tensor((rng.random((B, ny, nx)) < 0.03).astype(np.int32) * 2, device=DEV)
    miss = torch.tensor((rng.random((B, ny, nx)) < 0.9).astype(np.int32), device=DEV)
    assert hit.data_ptr() % 16 == 0 and miss.data_ptr() % 16 == 0
    hbig = torch.full((1 + cells + 3,), -77, dtype=torch.int32, device=DEV)
    mbig = torch.full((1 + cells + 3,), -77, dtype=torch.int32, device=DEV)
    hv, mv = hbig[1:1 + cells].view(B, ny, nx), mbig[1:1 + cells].view(B, ny, nx)
    hv.copy_(hit)
    mv.copy_(miss)
    assert hv.data_ptr() % 16 == 4 and mv.data_ptr() % 16 == 4
    for R, unknown in ((0, 1), (3, 0)):
        want = _edt(b, hit, miss, unknown=unknown, R=R)
        assert want[0].data_ptr() % 16 == 0 and want[1].data_ptr() % 16 == 0
        results = []
        for (h, m), dpad, npad in (((hit, miss), pad, pad), ((hv, mv), pad, pad), ((hit, miss), pad, 36), ((hit, miss), 36, pad), ((hv, mv), 36, 36)):
            dg, ng = Guarded(dpad, ny, nx), Guarded(npad, ny, nx)
            _edt(b, h, m, unknown=unknown, R=R, out=(dg.view, ng.view))
            results.append((dg, ng))
        torch.cuda.synchronize()
        wd, wn = ref.field(hit.cpu().numpy(), miss.cpu().numpy(), 1, bool(unknown), R)
        _same("aligned dist2", want[0], wd)
        _same("aligned nearest", want[1], wn)
        for dg, ng in results:
            dg.check(want[0])
            ng.check(want[1])
    assert hbig[0] == -77 and (hbig[1 + cells:] == -77).all() and mbig[0] == -77 and (mbig[1 + cells:] == -77).all()
    assert torch.equal(hv, hit) and torch.equal(mv, miss)      # the inputs are unchanged


def test_error_codes_and_a_refused_call_writes_nothing(bare):
    b = bare
    L = b.L
    nx = ny = 64
    cells = B * nx * ny
    pool = torch.zeros(4 * cells + 64, dtype=torch.int32, device=DEV)      # one allocation, so that ranges can be made to overlap
    hp, mp, dp, npp = (pool.data_ptr() + 4 * k * cells for k in range(4))
    good = dict(nx=nx, ny=ny, min_hits=1, unknown=0, R=0)

    def call(a, h=hp, m=mp, d=dp, n=npp):
        vp = lambda v: ctypes.c_void_p(v) if v else None
        return L.smj_occupancy_to_distance(b.ctx, vp(h), vp(m), a["nx"], a["ny"], a["min_hits"], a["unknown"], a["R"], vp(d), vp(n), _stream())

    bad = [dict(nx=0), dict(ny=0), dict(nx=-4), dict(ny=-1), dict(nx=4097, ny=1), dict(nx=1, ny=4097), dict(nx=8192, ny=8), dict(nx=257, ny=256),
           dict(nx=256, ny=257), dict(min_hits=0), dict(min_hits=-2), dict(R=-1), dict(R=-2 ** 31)]
    for change in bad:
        rc = call(dict(good, **change))
        assert rc == -1 and L.smj_last_error(b.ctx), (change, rc)
    assert call(dict(good, unknown=1), m=None) == -1 and b"miss" in L.smj_last_error(b.ctx)
    for h, m, d, n in ((None, mp, dp, npp), (hp, mp, None, npp), (hp + 2, mp, dp, npp), (hp, mp + 1, dp, npp), (hp, mp, dp + 2, npp), (hp, mp, dp, npp + 3)):
        assert call(good, h, m, d, n) == -1, (h, m, d, n)      # null / misaligned pointers
    # overlap: an output on an input, on the other output, by a whole range and by one word at either end
    last = 4 * (cells - 1)
    for h, m, d, n in ((hp, mp, hp, npp), (hp, mp, mp, npp), (hp, mp, dp, hp), (hp, mp, dp, mp), (hp, mp, dp, dp), (hp, mp, hp + last, npp),
                       (hp, mp, dp, mp - last), (hp, None, dp, dp + last), (hp, mp, dp, dp - last), (dp + last, mp, dp, npp), (hp, mp, mp + last, None)):
        assert call(good, h, m, d, n) == -1 and b"overlap" in L.smj_last_error(b.ctx), (h, m, d, n)
    torch.cuda.synchronize()
    assert int(pool.abs().max()) == 0      # a refused call writes nothing
    # accepted: the extremes of the cut, the largest grid, a null nearest_dev and a null miss_dev, adjacent ranges, a huge R
    for gx, gy in ((4096, 16), (16, 4096), (256, 256)):
        n = B * gx * gy
        buf = torch.zeros(3 * n, dtype=torch.int32, device=DEV)
        base = buf.data_ptr()
        assert call(dict(good, nx=gx, ny=gy), base, None, base + 4 * n, None) == 0
        assert call(dict(good, nx=gx, ny=gy, R=2 ** 31 - 1), base, None, base + 4 * n, base + 8 * n) == 0
        torch.cuda.synchronize()
        assert (buf[n:2 * n] == NONE).all() and (buf[2 * n:] == -1).all() and (buf[:n] == 0).all()


# ------------------------------------------------------------------ the simulator

@pytest.fixture(scope="module")
def rig():
    """The rig of tests/test_gpu_occupancy.py: stretch_scene, three envs driven apart, 200 steps, the lidar on."""
    r = perception_rig.lidar_rig()
    yield r
    r.sim.stop()


def test_end_to_end_from_the_lidar_scan(rig):
    from stretch_mujoco_amd.datamodels import StatusStretchDistanceField

    sim = rig.sim
    og = sim.pull_occupancy_grid()
    df = sim.pull_distance_field(nearest=True)
    assert isinstance(df, StatusStretchDistanceField) and df.frame == og.frame == "base" and df.cell == og.cell and df.origin == og.origin
    assert tuple(df.dist2.shape) == tuple(df.nearest.shape) == (B, 128, 128) and df.dist2.dtype == df.nearest.dtype == torch.int32
    torch.cuda.synchronize()
    hit, miss = og.hit.cpu().numpy(), og.miss.cpu().numpy()
    assert (hit > 0).any((1, 2)).all()
    want = ref.field(hit, miss)
    _same("dist2", df.dist2, want[0])
    _same("nearest", df.nearest, want[1])
    iy, ix = int(np.floor((0.0 - og.origin[1]) / og.cell)), int(np.floor((0.0 - og.origin[0]) / og.cell))      # the base's own cell
    d = df.distance()[:, iy, ix]
    print("clearance of the base per env [m]:", d.tolist())
    assert bool(torch.isfinite(d).all())
    # a StatusStretchOccupancyGrid handed in, with the other predicate and a bound
    df2 = sim.pull_distance_field(og, min_hits=2, unknown_is_obstacle=True, max_distance=0.49, nearest=True)      # R = ceil(9.8) = 10
    want2 = ref.field(hit, miss, 2, True, R=10)
    _same("dist2, grid handed in", df2.dist2, want2[0])
    _same("nearest, grid handed in", df2.nearest, want2[1])
    assert df2.dist2.data_ptr() == df.dist2.data_ptr() and df2.nearest.data_ptr() == df.nearest.data_ptr()      # keyed by shape, reused
    # occupancy keywords pass through for grid=None
    df3 = sim.pull_distance_field(shape=(48, 64), frame="world", origin=(-1.7, -1.1))
    assert tuple(df3.dist2.shape) == (B, 48, 64) and df3.nearest is None and df3.frame == "world" and df3.origin == (-1.7, -1.1)
    assert df3.dist2.data_ptr() != df.dist2.data_ptr() and sim.pull_distance_field(shape=(48, 64), frame="world", origin=(-1.7, -1.1)).dist2.data_ptr() == df3.dist2.data_ptr()


def test_mask_path_and_helpers(rig):
    sim = rig.sim
    rng = np.random.default_rng(48)
    mask = rng.random((B, 48, 64)) < 0.02
    mask[1] = False      # an env without obstacles
    df = sim.pull_distance_field(torch.tensor(mask, device=sim.device), cell=0.05, origin=(-1.6, -1.2), nearest=True)
    assert df.frame == "grid" and df.cell == 0.05 and df.origin == (-1.6, -1.2)
    torch.cuda.synchronize()
    wd, wn = ref.field(mask.astype(np.int32))
    _same("dist2", df.dist2, wd)
    _same("nearest", df.nearest, wn)
    for other in (torch.tensor(mask.astype(np.int64) * 5, device=sim.device), torch.tensor(mask.astype(np.uint8), device=sim.device)):
        _same("integer mask", sim.pull_distance_field(other).dist2, wd)
    df = sim.pull_distance_field(torch.tensor(mask, device=sim.device), cell=0.05, origin=(-1.6, -1.2), nearest=True)
    # distance(): sqrt(dist2) cell in fp32, inf where none
    dist = df.distance()
    assert dist.dtype == torch.float32
    want = np.where(wd == NONE, np.inf, np.sqrt(wd.astype(np.float32)) * np.float32(0.05)).astype(np.float32)
    got = dist.cpu().numpy()
    assert np.array_equal(np.isinf(got), wd == NONE) and np.isinf(got[1]).all()
    fin = wd != NONE
    assert np.abs(got[fin] - want[fin]).max() <= 2 * np.spacing(np.float32(want[fin].max()))      # one rounding each of sqrt and the product
    # nearest_offset(): (dy, dx), zeros where none; it points at an obstacle and its length is dist2
    no = df.nearest_offset()
    assert no.dtype == torch.int32 and tuple(no.shape) == (B, 48, 64, 2)
    no = no.cpu().numpy()
    yy, xx = np.mgrid[0:48, 0:64]
    assert np.array_equal(no[..., 0], np.where(wn >= 0, wn // 64 - yy, 0)) and np.array_equal(no[..., 1], np.where(wn >= 0, wn % 64 - xx, 0))
    assert np.array_equal((no.astype(np.int64) ** 2).sum(-1)[fin], wd[fin]) and (no[1] == 0).all()
    # inflated_cost(): the same formula in numpy, to one count of cost
    r_ins, r_inf, k = 0.17, 0.56, 10.0      # no sqrt(integer) * 0.05 comes within 1e-3 of either radius
    cost = df.inflated_cost(r_ins, r_inf, k)
    assert cost.dtype == torch.uint8
    d64 = np.where(fin, np.sqrt(wd.astype(np.float64)) * 0.05, np.inf)
    with np.errstate(over="ignore"):
        wc = np.floor(252.0 * np.exp(-k * (d64 - r_ins)))
    wc = np.where(d64 <= r_ins, 253, wc)
    wc = np.where(wd == 0, 254, wc)
    wc = np.where(d64 > r_inf, 0, wc)
    edge = (np.abs(d64 - r_ins) < 1e-6) | (np.abs(d64 - r_inf) < 1e-6)      # fp32 and fp64 would disagree about a distance within rounding of a radius
    assert not edge.any()
    gc = cost.cpu().numpy().astype(np.int64)
    assert np.abs(gc - wc).max() <= 1, np.abs(gc - wc).max()
    assert np.array_equal(gc == 254, wd == 0) and (gc[1] == 0).all() and ((gc == 253) == ((d64 <= r_ins) & (wd > 0))).all() and (gc[d64 > r_inf] == 0).all()
    assert set(np.unique(gc)) - {0, 253, 254} and gc[(gc > 0) & (gc < 253)].max() <= 252
    with pytest.raises(ValueError):
        sim.pull_distance_field(torch.tensor(mask, device=sim.device)).nearest_offset()


def test_value_errors_are_raised_before_any_launch(rig):
    sim = rig.sim
    dev = sim.device
    ok = torch.zeros(B, 8, 8, dtype=torch.bool, device=dev)
    og = sim.pull_occupancy_grid(shape=(32, 32))
    keep = sim.pull_distance_field(og, nearest=True)
    d0, n0 = keep.dist2.clone(), keep.nearest.clone()
    for grid, kw in ((ok, dict(min_hits=0)), (og, dict(min_hits=0)), (og, dict(min_hits=-1)), (og, dict(max_distance=0.0)), (og, dict(max_distance=-1.0)),
                     (og, dict(max_distance=float("nan"))), (og, dict(max_distance=float("inf"))), (ok, dict(unknown_is_obstacle=True)), (ok, dict(min_hits=2)),
                     (ok, dict(cell=0.0)), (ok, dict(cell=float("nan"))), (ok, dict(origin=(0.0,))), (ok, dict(origin=(float("inf"), 0.0))),
                     (ok.float(), dict()), (ok[0], dict()), (ok[:2], dict()), (torch.zeros(B, 4097, 1, dtype=torch.bool, device=dev), dict()),
                     (torch.zeros(B, 1, 4097, dtype=torch.bool, device=dev), dict()), (torch.zeros(B, 257, 256, dtype=torch.bool, device=dev), dict()),
                     (torch.zeros(B, 0, 4, dtype=torch.bool, device=dev), dict()), ("grid", dict()), (ok, dict(shape=(8, 8))), (og, dict(frame="world")),
                     (og, dict(cell=0.05)), (og, dict(origin=(0.0, 0.0))), (None, dict(shape=(0, 4))), (None, dict(frame="odom"))):
        with pytest.raises(ValueError):
            sim.pull_distance_field(grid, **kw)
    torch.cuda.synchronize()
    assert torch.equal(keep.dist2, d0) and torch.equal(keep.nearest, n0)      # nothing ran
