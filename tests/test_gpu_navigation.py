"""Exact cost-to-goal fields of costmaps on the HIP path: smj_costmap_to_navigation through the C-ABI and
StretchBatchSimulator.pull_navigation_field.

Most tests run on a bare context -- smj_create on the stretch_scene blob, three envs, NOTHING bound: the entry needs no slot and no
model tables.  Every comparison of potential and next is integer equality with tests/navigation_ref.py (a heap Dijkstra, next by its
definition) on every cell; there is no tolerance anywhere.  The references of a shape are computed once and shared.

Shapes (nx, ny): the smallest at which the kernel can go wrong -- a single cell, single rows / columns, 16 x 12, the odd 61 x 83 (no
16-byte row alignment), 128 x 128 (SMJ_NAV_LDS_CELLS = 16384 cells: the largest grid whose potential lives in LDS), 129 x 128 (the
smallest one relaxed in potential_dev itself), 4096 x 4 and 4 x 4096 (16 lines per thread one way, the longest lines cut into 32 runs the other), and 256 x 256 once."""
import ctypes

import numpy as np
import pytest
import torch

import navigation_ref as ref
import perception_rig
from perception_rig import B, DEV, Guarded, ptr as _ptr, same as _same, stream as _stream

pytestmark = pytest.mark.gpu

G = 3
SHAPES = [(1, 1), (7, 1), (1, 7), (16, 12), (61, 83), (128, 128), (129, 128), (4096, 4), (4, 4096)]
NONE = 1 << 30


@pytest.fixture(scope="module")
def bare():
    yield from perception_rig.bare_context()


def _nav(b, cost, goal, lethal=253, neutral=50, shape=None, nxt=True, out=None, rc=0):
    """One call: cost uint8 [B, ny, nx] on the device or None (then shape = (ny, nx)), goal int32 [B, g]; the outputs start as
    sentinels."""
    ny, nx = shape if cost is None else cost.shape[1:]
    if out is None:
        out = perception_rig.sentinels(ny, nx)
    got = b.L.smj_costmap_to_navigation(b.ctx, _ptr(cost), _ptr(goal), goal.shape[1], nx, ny, lethal, neutral, _ptr(out[0]), _ptr(out[1]) if nxt else None,
                                        _stream())
    assert got == rc, (got, b.L.smj_last_error(b.ctx))
    return out


def _pick(passable, k, rng):
    """k passable cells (linear indices), spread over the grid; fewer cells are repeated."""
    free = np.flatnonzero(passable.ravel())
    return [int(v) for v in free[np.linspace(0, len(free) - 1, k).astype(int)]] if len(free) else [0] * k


def _cases(nx, ny):
    """The maps of a shape: a list of (tag, cost uint8 [ny, nx] or None, goals [G], lethal, neutral), three per call."""
    rng = np.random.default_rng(1000 * nx + ny)
    n = nx * ny
    yy, xx = np.mgrid[0:ny, 0:nx]
    free = np.zeros((ny, nx), np.uint8)
    costs = rng.integers(0, 253, (ny, nx)).astype(np.uint8)                                    # no lethal cell
    r30 = np.where(rng.random((ny, nx)) < 0.3, rng.integers(253, 256, (ny, nx)), rng.integers(0, 253, (ny, nx))).astype(np.uint8)
    r30g = _pick(r30 < 253, G, rng)
    wall = free.copy()
    wall[:, nx // 2] = 254
    wall[max(ny - 2, 0), nx // 2] = 7                                                          # the gap
    pocket = costs.copy()
    if nx >= 7 and ny >= 7:
        ring = (np.maximum(np.abs(yy - 3), np.abs(xx - 3)) == 2)
        pocket[ring] = 253                                                                     # the cells (2 .. 4, 2 .. 4) inside are cut off
    checker = np.where((yy + xx) % 2 == 1, 254, 0).astype(np.uint8)
    full = np.where(rng.random((ny, nx)) < 0.3, 255, rng.integers(0, 255, (ny, nx))).astype(np.uint8)
    full.ravel()[n - 1] = 255
    centre = (ny // 2) * nx + nx // 2
    corners = [0, nx - 1, (ny - 1) * nx, n - 1]
    lethal_goal = costs.copy()
    lethal_goal.ravel()[centre] = 253
    A = dict(lethal=253, neutral=50)
    cases = [("all free", free, [centre, -1, -1], A), ("all lethal", np.full((ny, nx), 253, np.uint8), [centre, 0, n - 1], A),
             ("goal on a lethal cell", lethal_goal, [-1, centre, -1], A)]
    cases += [(f"goal in corner {k}", costs, [-1, -1, c], A) for k, c in enumerate(corners)]
    cases += [("no goal", costs, [-1, -1, -1], A), ("goal out of range", costs, [n, -2, 2 ** 31 - 1], A),
              ("three goals", costs, [corners[1], centre, corners[2]], A), ("wall with one gap", wall, [0, -1, -1], A),
              ("serpentine", ref.serpentine(ny, nx), [0, -1, -1], A), ("closed pocket", pocket, [n - 1, -1, 0], A),
              ("30 % lethal", r30, r30g, A), ("checkerboard", checker, [0, -1, -1], A)]
    C = dict(lethal=256, neutral=50)
    cases += [("lethal 256, cost 255 present", full, [0, -1, n - 1], C), ("lethal 256, 30 % map", r30, r30g, C),
              ("lethal 256, serpentine", ref.serpentine(ny, nx, 255), [0, -1, -1], C)]
    for neutral in (1, 255):
        D = dict(lethal=253, neutral=neutral)
        cases += [(f"neutral {neutral}, 30 % lethal", r30, r30g, D), (f"neutral {neutral}, costs", costs, [centre, -1, corners[3]], D),
                  (f"neutral {neutral}, free", free, [corners[0], corners[3], -1], D)]
    E = dict(lethal=256, neutral=255)
    cases += [("largest weights", np.full((ny, nx), 255, np.uint8), [0, -1, -1], E), ("largest weights, serpentine", ref.serpentine(ny, nx, 255), [0, -1, -1], E),
              ("largest weights, 30 % map", full, [centre, -1, -1], E)]
    F = dict(lethal=1, neutral=50)
    cases += [("null cost", None, [centre, -1, -1], F), ("null cost, three goals", None, corners[:3], F), ("null cost, no goal", None, [-1, n, -1], F)]
    assert len(cases) % B == 0
    return cases


def _reference(b, nx, ny):
    key = (nx, ny)
    if key not in b.cache:
        cases, want = _cases(nx, ny), []
        for tag, cost, goals, kw in cases:
            c = np.zeros((ny, nx), np.uint8) if cost is None else cost
            p = ref.potential(c, goals, **kw)
            want.append((p, ref.next_of(c, p, **kw)))
        b.cache[key] = (cases, want)
    return b.cache[key]


def _device_inputs(cases):
    cost = None if cases[0][1] is None else torch.tensor(np.stack([c[1] for c in cases]), device=DEV)
    goal = torch.tensor(np.array([c[2] for c in cases], np.int64).astype(np.int32), device=DEV)      # 2^31 - 1 stays, -2 stays
    return cost, goal


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_every_cell_equals_the_reference(bare, nx, ny):
    b = bare
    cases, want = _reference(b, nx, ny)
    by_tag = {c[0]: w for c, w in zip(cases, want)}
    n = nx * ny
    # what the reference says about the cases themselves, so that none is vacuous
    assert (by_tag["all lethal"][0] == NONE).all() and (by_tag["goal on a lethal cell"][0] == NONE).all() and (by_tag["no goal"][0] == NONE).all()
    assert (by_tag["goal out of range"][0] == NONE).all() and (by_tag["null cost, no goal"][1] == -1).all()
    assert (by_tag["all free"][0] < NONE).all() and (by_tag["three goals"][0] == 0).sum() == len({nx - 1, (ny // 2) * nx + nx // 2, (ny - 1) * nx})
    assert (by_tag["checkerboard"][0] < NONE).sum() == 1
    if min(nx, ny) >= 12:      # in a strip a few cells wide a 30 % map is cut with near certainty: the share is asserted on the 2-D shapes
        assert (by_tag["30 % lethal"][0] < NONE).mean() >= 0.5
        assert (by_tag["closed pocket"][0][2:5, 2:5] == NONE).all() and (by_tag["closed pocket"][0] < NONE).sum() == n - 16 - 9
    if nx > 2 and ny > 2:
        assert (by_tag["wall with one gap"][0][:, nx // 2 + 1:] < NONE).all() and (by_tag["wall with one gap"][0][:, nx // 2] < NONE).sum() == 1
        assert (by_tag["serpentine"][0] < NONE).sum() == ((ny + 1) // 2) * nx + ny // 2
    results = []
    for k in range(0, len(cases), B):
        cost, goal = _device_inputs(cases[k:k + B])
        kw = cases[k][3]
        assert all(c[3] == kw for c in cases[k:k + B])
        both = _nav(b, cost, goal, shape=(ny, nx), **kw)
        only = _nav(b, cost, goal, shape=(ny, nx), nxt=False, **kw) if k == 0 else None
        results.append((k, cost, goal, both, only))
    torch.cuda.synchronize()
    for k, cost, goal, both, only in results:
        for e in range(B):
            tag, c, g, _ = cases[k + e]
            _same(("potential", nx, ny, tag), both[0][e], want[k + e][0])
            _same(("next", nx, ny, tag), both[1][e], want[k + e][1])
            if c is not None:
                assert np.array_equal(cost[e].cpu().numpy(), c)      # the inputs are unchanged
        assert np.array_equal(goal.cpu().numpy().astype(np.int64), np.array([c[2] for c in cases[k:k + B]], np.int64))
        if only is not None:
            assert torch.equal(only[0], both[0]) and int((only[1] != -7).sum()) == 0      # a null next_dev: that buffer is not touched


def test_256_x_256_once(bare):
    b = bare
    nx = ny = 256
    rng = np.random.default_rng(256)
    cost = np.zeros((B, ny, nx), np.uint8)
    cost[0] = np.where(rng.random((ny, nx)) < 0.3, 254, rng.integers(0, 253, (ny, nx)))
    cost[1] = rng.integers(0, 20, (ny, nx))
    cost[2] = ref.serpentine(ny, nx)
    goals = np.array([_pick(cost[0] < 253, G, rng), [ny * nx - 1, -1, -1], [0, -1, -1]])
    want = ref.field(cost, goals)
    assert (want[0][0] < NONE).mean() >= 0.5 and (want[0][2] < NONE).sum() == 128 * 256 + 128
    got = _nav(b, torch.tensor(cost, device=DEV), torch.tensor(goals.astype(np.int32), device=DEV))
    torch.cuda.synchronize()
    _same("potential", got[0], want[0])
    _same("next", got[1], want[1])


def test_two_calls_agree_and_envs_do_not_see_each_other(bare):
    b = bare
    for nx, ny in ((61, 83), (129, 128)):
        cases, want = _reference(b, nx, ny)
        idx = {c[0]: k for k, c in enumerate(cases)}
        first = [cases[idx[t]] for t in ("30 % lethal", "three goals", "serpentine")]
        second = [cases[idx[t]] for t in ("all lethal", "closed pocket", "30 % lethal")]      # the 30 % map in env 2, beside other neighbours
        c1, g1 = _device_inputs(first)
        c2, g2 = _device_inputs(second)
        a, a2, c = _nav(b, c1, g1), _nav(b, c1, g1), _nav(b, c2, g2)
        torch.cuda.synchronize()
        assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])
        assert torch.equal(a[0][0], c[0][2]) and torch.equal(a[1][0], c[1][2])
        _same("env 2", c[0][2], want[idx["30 % lethal"]][0])


@pytest.mark.parametrize("nx,ny", [(61, 83), (129, 128)])
def test_nothing_outside_the_outputs_is_written_and_alignment_does_not_matter(bare, nx, ny):
    """An LDS grid and one relaxed in place.  The outputs as views 4 bytes past a 16-byte boundary inside buffers of sentinels: the
    guards stay untouched and the values are those of the aligned call; the same with the goals 4 bytes and the cost 1 byte past a
    16-byte boundary, with both, and with only one of the two outputs misaligned."""
    b = bare
    cases, want = _reference(b, nx, ny)
    idx = {c[0]: k for k, c in enumerate(cases)}
    pick = [cases[idx[t]] for t in ("30 % lethal", "three goals", "closed pocket")]
    cost, goal = _device_inputs(pick)
    cells, pad = B * nx * ny, 37      # 37 words = 148 bytes = 4 mod 16
    assert cost.data_ptr() % 16 == 0 and goal.data_ptr() % 16 == 0
    cbig = torch.full((1 + cells + 5,), 99, dtype=torch.uint8, device=DEV)
    gbig = torch.full((1 + B * G + 3,), -77, dtype=torch.int32, device=DEV)
    cv, gv = cbig[1:1 + cells].view(B, ny, nx), gbig[1:1 + B * G].view(B, G)
    cv.copy_(cost)
    gv.copy_(goal)
    assert cv.data_ptr() % 16 == 1 and gv.data_ptr() % 16 == 4
    aligned = _nav(b, cost, goal)
    assert aligned[0].data_ptr() % 16 == 0 and aligned[1].data_ptr() % 16 == 0
    results = []
    for (c, g), ppad, npad in (((cost, goal), pad, pad), ((cv, gv), pad, pad), ((cost, goal), pad, 36), ((cost, goal), 36, pad), ((cv, gv), 36, 36),
                               ((cv, gv), 38, 39)):
        pg, ng = Guarded(ppad, ny, nx), Guarded(npad, ny, nx)
        _nav(b, c, g, out=(pg.view, ng.view))
        results.append((pg, ng))
    torch.cuda.synchronize()
    for e in range(B):
        _same("aligned potential", aligned[0][e], want[idx[pick[e][0]]][0])
        _same("aligned next", aligned[1][e], want[idx[pick[e][0]]][1])
    for pg, ng in results:
        pg.check(aligned[0])
        ng.check(aligned[1])
    assert cbig[0] == 99 and (cbig[1 + cells:] == 99).all() and gbig[0] == -77 and (gbig[1 + B * G:] == -77).all()
    assert torch.equal(cv, cost) and torch.equal(gv, goal)      # the inputs are unchanged


def test_error_codes_and_a_refused_call_writes_nothing(bare):
    b = bare
    L = b.L
    nx = ny = 64
    cells = B * nx * ny
    pool = torch.zeros(4 * cells + 64, dtype=torch.int32, device=DEV)      # one allocation, so that ranges can be made to overlap
    cp, gp, pp, npp = (pool.data_ptr() + 4 * k * cells for k in range(4))      # the cost takes the first quarter of its slot
    good = dict(g=G, nx=nx, ny=ny, lethal=253, neutral=50)

    def call(a, c=cp, g=gp, p=pp, n=npp):
        vp = lambda v: ctypes.c_void_p(v) if v else None
        return L.smj_costmap_to_navigation(b.ctx, vp(c), vp(g), a["g"], a["nx"], a["ny"], a["lethal"], a["neutral"], vp(p), vp(n), _stream())

    bad = [dict(nx=0), dict(ny=0), dict(nx=-4), dict(ny=-1), dict(nx=4097, ny=1), dict(nx=1, ny=4097), dict(nx=8192, ny=8), dict(nx=257, ny=256),
           dict(nx=256, ny=257), dict(g=0), dict(g=-1), dict(g=65), dict(lethal=0), dict(lethal=-3), dict(lethal=257), dict(neutral=0), dict(neutral=-1),
           dict(neutral=256), dict(neutral=2 ** 31 - 1)]
    for change in bad:
        rc = call(dict(good, **change))
        assert rc == -1 and L.smj_last_error(b.ctx), (change, rc)
    for c, g, p, n in ((cp, None, pp, npp), (cp, gp, None, npp), (cp, gp + 2, pp, npp), (cp, gp, pp + 1, npp), (cp, gp, pp, npp + 2), (None, gp + 3, pp, npp)):
        assert call(good, c, g, p, n) == -1, (c, g, p, n)      # null / misaligned pointers
    # overlap: an output on an input, on the other output, by a whole range and by one word (or byte) at either end
    last, glast = 4 * (cells - 1), 4 * (B * G - 1)
    for c, g, p, n in ((cp, gp, cp, npp), (cp, gp, gp, npp), (cp, gp, pp, cp), (cp, gp, pp, gp), (cp, gp, pp, pp), (cp, gp, cp + cells - 4, npp),
                       (pp + 4 * cells - 1, gp, pp, npp), (cp, gp, pp, gp - last), (cp, gp, gp + glast, npp), (None, gp, pp, pp + last), (cp, gp, pp, pp - last),
                       (cp, pp + last, pp, None)):
        assert call(good, c, g, p, n) == -1 and b"overlap" in L.smj_last_error(b.ctx), (c, g, p, n)
    torch.cuda.synchronize()
    assert int(pool.abs().max()) == 0      # a refused call writes nothing
    # accepted: the extremes, the largest grid, a null next_dev and a null cost_dev, adjacent ranges, 64 goals, a misaligned cost
    for gx, gy in ((4096, 16), (16, 4096), (256, 256)):
        n = B * gx * gy
        buf = torch.zeros(3 * n + 64 * B, dtype=torch.int32, device=DEV)
        base = buf.data_ptr()
        goals = base + 12 * n      # zeros: 64 times cell 0
        assert call(dict(good, nx=gx, ny=gy, g=64), None, goals, base + 4 * n, None) == 0
        assert call(dict(good, nx=gx, ny=gy, g=64, lethal=1), base + 1, goals, base + 4 * n, base + 8 * n) == 0      # cost 0 < lethal 1: as free as the null map
        torch.cuda.synchronize()
        want = 50 * ref.free_closed_form(gy, gx, 0, 0, 1)
        assert np.array_equal(buf[n:2 * n].view(B, gy, gx)[B - 1].cpu().numpy(), want) and int(buf[2 * n]) == 0 and (buf[:n] == 0).all() and (buf[3 * n:] == 0).all()


# ------------------------------------------------------------------ the simulator

@pytest.fixture(scope="module")
def rig():
    """The rig of tests/test_gpu_occupancy.py: stretch_scene, three envs driven apart, 200 steps, the lidar on."""
    r = perception_rig.lidar_rig()
    yield r
    r.sim.stop()


def test_end_to_end_from_the_lidar_scan(rig):
    from stretch_mujoco_amd.datamodels import StatusStretchNavigationField

    sim = rig.sim
    df = sim.pull_distance_field(max_distance=0.56)
    cost = df.inflated_cost(0.17, 0.56, 10.0)      # handed as it is to the reference: the fp32 exponential is not re-derived
    torch.cuda.synchronize()
    c = cost.cpu().numpy()
    assert (c >= 253).any((1, 2)).all() and ((c > 0) & (c < 253)).any((1, 2)).all()
    # per env a goal a good metre from the robot: the zero-cost cell nearest to (1.0, 0.5), handed over in metres at its centre
    yy, xx = np.mgrid[0:128, 0:128]
    away = (yy - 74) ** 2 + (xx - 84) ** 2
    cells = [int(np.argmin(np.where(c[e] == 0, away, 1 << 40))) for e in range(B)]
    goal = torch.tensor([[-3.2 + (k % 128 + 0.5) * 0.05, -3.2 + (k // 128 + 0.5) * 0.05] for k in cells], dtype=torch.float32, device=sim.device)
    nf = sim.pull_navigation_field(goal, next=True)
    assert isinstance(nf, StatusStretchNavigationField) and nf.frame == df.frame == "base" and nf.cell == df.cell and nf.origin == df.origin and nf.neutral == 50
    assert tuple(nf.potential.shape) == tuple(nf.next.shape) == (B, 128, 128) and nf.potential.dtype == nf.next.dtype == torch.int32
    torch.cuda.synchronize()
    assert nf.goal.dtype == torch.int32 and nf.goal.cpu().tolist() == [[k] for k in cells]
    assert np.array_equal(df.inflated_cost(0.17, 0.56, 10.0).cpu().numpy(), c)      # the same scan, the same costmap
    want = ref.field(c, nf.goal.cpu().numpy())
    _same("potential", nf.potential, want[0])
    _same("next", nf.next, want[1])
    print("reachable cells per env:", (want[0] < NONE).sum((1, 2)).tolist())
    assert ((want[0] < NONE).sum((1, 2)) > 1000).all()
    # a StatusStretchDistanceField handed in, other parameters, no next
    nf2 = sim.pull_navigation_field(goal, df, lethal=254, neutral=1, inscribed_radius=0.1, inflation_radius=0.4, cost_scaling_factor=5.0)
    c2 = df.inflated_cost(0.1, 0.4, 5.0).cpu().numpy()
    _same("potential, field handed in", nf2.potential, ref.field(c2, nf.goal.cpu().numpy(), 254, 1)[0])
    assert nf2.next is None and nf2.neutral == 1 and nf2.potential.data_ptr() == nf.potential.data_ptr()      # keyed by shape, reused
    # distance keywords pass through for cost=None
    nf3 = sim.pull_navigation_field(goal, shape=(48, 64), frame="world", origin=(-1.7, -1.1))
    assert tuple(nf3.potential.shape) == (B, 48, 64) and nf3.frame == "world" and nf3.origin == (-1.7, -1.1) and nf3.potential.data_ptr() != nf.potential.data_ptr()


def test_uint8_path_goal_forms_and_helpers(rig):
    sim = rig.sim
    dev = sim.device
    rng = np.random.default_rng(48)
    ny, nx, cell, origin = 48, 64, 0.05, (-1.6, -1.2)
    cost = np.where(rng.random((B, ny, nx)) < 0.2, 254, rng.integers(0, 253, (B, ny, nx))).astype(np.uint8)
    cost[1] = 254      # an env where nothing is passable
    free = np.flatnonzero(cost[0].ravel() < 253)
    cells = np.array([[free[5], free[-7]], [3, 4], [np.flatnonzero(cost[2].ravel() < 253)[40], -1]], np.int64)
    ct = torch.tensor(cost, device=dev)
    want = ref.field(cost, cells)
    # int tensor [B, G]
    nf = sim.pull_navigation_field(torch.tensor(cells, device=dev), ct, cell=cell, origin=origin, next=True)
    assert nf.frame == "grid" and nf.cell == cell and nf.origin == origin
    _same("potential", nf.potential, want[0])
    _same("next", nf.next, want[1])
    assert np.array_equal(nf.goal.cpu().numpy(), cells)
    # int tensor [B]; out-of-range indices become -1
    one = sim.pull_navigation_field(torch.tensor([int(cells[0, 0]), ny * nx, int(cells[2, 0])], device=dev), ct)
    assert one.goal.cpu().tolist() == [[int(cells[0, 0])], [-1], [int(cells[2, 0])]] and one.cell == 1.0 and one.origin == (0.0, 0.0)
    _same("potential, [B]", one.potential, ref.field(cost, cells[:, :1])[0])
    # metres: [B, G, 2] at the cells' centres, with one goal outside and one NaN; [B, 2]; (x, y)
    centre = lambda k: [origin[0] + (k % nx + 0.5) * cell, origin[1] + (k // nx + 0.5) * cell]
    metres = torch.tensor([[centre(cells[0, 0]), centre(cells[0, 1])], [centre(3), [origin[0] - 0.01, 0.0]], [centre(cells[2, 0]), [float("nan"), 0.0]]],
                          dtype=torch.float32, device=dev)
    m = sim.pull_navigation_field(metres, ct, cell=cell, origin=origin)
    assert m.goal.cpu().tolist() == [[int(cells[0, 0]), int(cells[0, 1])], [3, -1], [int(cells[2, 0]), -1]]
    _same("potential, metres", m.potential, want[0])
    m2 = sim.pull_navigation_field(metres[:, 0], ct, cell=cell, origin=origin)
    assert m2.goal.cpu().tolist() == [[int(cells[0, 0])], [3], [int(cells[2, 0])]]
    x, y = centre(cells[0, 0])
    m3 = sim.pull_navigation_field((x, y), ct, cell=cell, origin=origin)
    assert m3.goal.cpu().tolist() == [[int(cells[0, 0])]] * B
    # the helpers against numpy on the reference arrays
    nf = sim.pull_navigation_field(torch.tensor(cells, device=dev), ct, cell=cell, origin=origin, next=True, neutral=7)
    wp, wn = ref.field(cost, cells, 253, 7)
    fin = wp < NONE
    dist = nf.distance()
    assert dist.dtype == torch.float32
    got = dist.cpu().numpy()
    wd = wp.astype(np.float64) * cell / 70.0
    assert np.array_equal(np.isinf(got), ~fin) and np.isinf(got[1]).all()
    assert np.abs(got[fin] - wd[fin]).max() <= 3 * np.spacing(np.float32(wd[fin].max()))      # int -> fp32, the fp32 factor, the product
    off = nf.next_offset()
    assert off.dtype == torch.int32 and tuple(off.shape) == (B, ny, nx, 2)
    off = off.cpu().numpy()
    yy, xx = np.mgrid[0:ny, 0:nx]
    assert np.array_equal(off[..., 0], np.where(wn >= 0, wn // nx - yy, 0)) and np.array_equal(off[..., 1], np.where(wn >= 0, wn % nx - xx, 0))
    assert np.abs(off).max() == 1 and (off[wp == 0] == 0).all() and (off[1] == 0).all()
    head = nf.heading().cpu().numpy()
    moving = fin & (wp > 0)
    assert head.dtype == np.float32 and np.array_equal(np.isnan(head), ~moving)
    assert np.abs(head[moving] - np.arctan2(off[..., 0], off[..., 1])[moving]).max() <= 1e-6
    reach = np.flatnonzero(fin[0].ravel())
    assert len(reach) > ny * nx // 2
    starts = np.array([reach[len(reach) // 2], 5, -1], np.int64)      # env 1 has no path, env 2 starts outside
    steps = 40
    path = nf.path(torch.tensor(starts, device=dev), steps)
    assert path.dtype == torch.int64 and tuple(path.shape) == (B, steps + 1)
    path = path.cpu().numpy()
    walk = ref.follow(wn[0], starts[0], steps)
    assert (path[1:] == -1).all() and path[0].tolist() == walk + [walk[-1]] * (steps + 1 - len(walk))
    full = nf.path(torch.tensor(starts, device=dev), ny * nx).cpu().numpy()[0]
    assert full[-1] in cells[0] and (np.diff(wp[0].ravel()[full]) <= 0).all()
    sx, sy = centre(starts[0])
    assert np.array_equal(nf.path((sx, sy), steps).cpu().numpy()[0], path[0])
    assert np.array_equal(nf.path(torch.tensor([[sx, sy]] * B, dtype=torch.float32, device=dev), steps).cpu().numpy()[0], path[0])
    with pytest.raises(ValueError):
        sim.pull_navigation_field((x, y), ct).next_offset()
    with pytest.raises(ValueError):
        sim.pull_navigation_field((x, y), ct).path((x, y), 3)


def test_value_errors_are_raised_before_any_launch(rig):
    sim = rig.sim
    dev = sim.device
    ok = torch.zeros(B, 8, 8, dtype=torch.uint8, device=dev)
    goal = (2.0, 2.0)
    df = sim.pull_distance_field(shape=(32, 32), nearest=True)
    keep = sim.pull_navigation_field((0.5, 0.5), df, next=True)
    d0, n0, p0, x0 = df.dist2.clone(), df.nearest.clone(), keep.potential.clone(), keep.next.clone()
    f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
    i = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device=dev)
    for g, cost, kw in ((goal, ok, dict(lethal=0)), (goal, ok, dict(lethal=257)), (goal, df, dict(neutral=0)), (goal, None, dict(neutral=256)),
                        (goal, None, dict(lethal=-1)), ((1.0,), ok, dict()), ("goal", ok, dict()), (None, ok, dict()), (f(B, 3), ok, dict()),
                        (f(B - 1, 2), ok, dict()), (f(B, 65, 2), ok, dict()), (f(B, 0, 2), ok, dict()), (f(B, 2, 2, 2), ok, dict()), (i(B + 1), ok, dict()),
                        (i(B, 65), ok, dict()), (i(B, 0), ok, dict()), (i(B, 2, 2), ok, dict()), (torch.zeros(B, dtype=torch.bool, device=dev), ok, dict()),
                        (goal, ok.float(), dict()), (goal, ok[0], dict()), (goal, ok[:2], dict()), (goal, ok.to(torch.int32), dict()), (goal, "cost", dict()),
                        (goal, torch.zeros(B, 4097, 1, dtype=torch.uint8, device=dev), dict()), (goal, torch.zeros(B, 257, 256, dtype=torch.uint8, device=dev), dict()),
                        (goal, torch.zeros(B, 0, 4, dtype=torch.uint8, device=dev), dict()), (goal, ok, dict(cell=0.0)), (goal, ok, dict(cell=float("nan"))),
                        (goal, ok, dict(origin=(0.0,))), (goal, ok, dict(origin=(float("inf"), 0.0))), (goal, ok, dict(shape=(8, 8))), (goal, ok, dict(min_hits=2)),
                        (goal, df, dict(cell=0.05)), (goal, df, dict(origin=(0.0, 0.0))), (goal, df, dict(frame="world")), (goal, df, dict(inscribed_radius=-0.1)),
                        (goal, df, dict(inscribed_radius=0.6)), (goal, df, dict(inflation_radius=float("inf"))), (goal, None, dict(inflation_radius=0.0, inscribed_radius=0.0)),
                        (goal, None, dict(cost_scaling_factor=-1.0)), (goal, None, dict(cost_scaling_factor=float("nan"))), (goal, None, dict(max_distance=1.0)),
                        (goal, None, dict(min_hits=0)), (goal, None, dict(shape=(0, 4))), (goal, None, dict(frame="odom"))):
        with pytest.raises(ValueError):
            sim.pull_navigation_field(g, cost, **kw)
    torch.cuda.synchronize()
    assert torch.equal(df.dist2, d0) and torch.equal(df.nearest, n0) and torch.equal(keep.potential, p0) and torch.equal(keep.next, x0)      # nothing ran
