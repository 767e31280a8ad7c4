"""Frontier regions of occupancy grids on the HIP path: smj_occupancy_to_frontiers through the C-ABI and
StretchBatchSimulator.pull_frontiers.

Most tests run on a bare context -- smj_create on the stretch_scene blob, three envs, NOTHING bound: the entry needs no slot and no
model tables.  Every comparison of label, goal, region and count is integer equality with tests/frontier_ref.py (numpy states, a
flood fill, Python integers for the representative's key); there is no tolerance anywhere.  The references of a shape are computed
once and shared.

Shapes (nx, ny): the smallest at which the kernel can go wrong -- a single cell, single rows / columns, 16 x 12, the odd 61 x 83 (no
16-byte row alignment), the largest grid whose labels live in LDS and the smallest one labelled in label_dev itself (both read from
SMJ_FRONT_LDS_CELLS: 128 x 128 and 145 x 113 = 16385 cells), 4096 x 4 and 4 x 4096 (the longest rows / columns), and 256 x 256 once."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import capi_check
import frontier_ref as ref
import perception_rig
from conftest import ROOT
from perception_rig import B, DEV, Guarded, ptr as _ptr, same as _same, stream as _stream

pytestmark = pytest.mark.gpu

LDS_CELLS = int(re.search(r"SMJ_FRONT_LDS_CELLS\s*=\s*(\d+)", capi_check.kernel_header("smj_front.h")).group(1))


def _rectangle(cells):
    """(nx, ny) with nx ny == cells, the squarest one within the side limit."""
    ny = max(d for d in range(1, int(cells ** 0.5) + 1) if cells % d == 0)
    assert cells // ny <= 4096
    return cells // ny, ny


LAST_LDS, FIRST_GLOBAL = _rectangle(LDS_CELLS), _rectangle(LDS_CELLS + 1)
SHAPES = [(1, 1), (7, 1), (1, 7), (16, 12), (61, 83), LAST_LDS, FIRST_GLOBAL, (4096, 4), (4, 4096)]
FILL = -7


@pytest.fixture(scope="module")
def bare():
    yield from perception_rig.bare_context()


def _outputs(ny, nx, G):
    new = lambda *shape: torch.full((B, *shape), FILL, dtype=torch.int32, device=DEV)
    return [new(ny, nx), new(G), new(G, 4), new(2)]


def _front(b, hit, miss, cost=None, min_hits=1, lethal=253, min_size=1, max_regions=16, out=None, region=True, count=True, rc=0):
    """One call: hit, miss int32 [B, ny, nx] and cost uint8 [B, ny, nx] or None, on the device; the outputs start as sentinels."""
    ny, nx = hit.shape[1:]
    if out is None:
        out = _outputs(ny, nx, max_regions)
    got = b.L.smj_occupancy_to_frontiers(b.ctx, _ptr(hit), _ptr(miss), _ptr(cost), nx, ny, min_hits, lethal, min_size, max_regions, _ptr(out[0]), _ptr(out[1]),
                                         _ptr(out[2]) if region else None, _ptr(out[3]) if count else None, _stream())
    assert got == rc, (got, b.L.smj_last_error(b.ctx))
    return out


def _cases(nx, ny):
    """The maps of a shape: a list of (tag, hit, miss, cost or None, keywords), three per call."""
    rng = np.random.default_rng(1000 * nx + ny)
    n = nx * ny
    fill = lambda v: np.full((ny, nx), v, np.int8)
    thirds, thirds2 = rng.integers(0, 3, (ny, nx)) - 1, rng.integers(0, 3, (ny, nx)) - 1
    holes = np.where(rng.random((ny, nx)) < 0.02, -1, 0)      # long rings around a few unknown cells
    maps = dict(thirds=thirds, thirds2=thirds2, holes=holes, disc=ref.disc(ny, nx), serpentine=ref.serpentine(ny, nx), spiral=ref.spiral(ny, nx),
                isolated=ref.isolated(ny, nx), rooms=ref.rooms(ny, nx))
    pair = {k: ref.counts_of(v) for k, v in maps.items()}
    cases = []

    def group(tags, cost=None, **kw):
        for k, t in enumerate(tags):
            h, m = pair[t] if isinstance(t, str) else t
            cases.append((f"{t if isinstance(t, str) else 'counts'} {kw}" + (" cost" if cost is not None else ""), h, m, None if cost is None else cost[k], kw))

    A = dict(min_hits=1, lethal=253, min_size=1, max_regions=16)
    group([ref.counts_of(fill(-1)), ref.counts_of(fill(0)), ref.counts_of(fill(1))], **A)
    group(["thirds", "disc", "serpentine"], **A)
    group(["spiral", "rooms", "thirds2"], **A)
    group(["isolated", "thirds", "holes"], **dict(A, max_regions=64))
    group(["thirds", "rooms", "disc"], **dict(A, max_regions=1))
    group(["thirds", "holes", "spiral"], **dict(A, min_size=4))
    group([(rng.integers(0, 4, (ny, nx)).astype(np.int32), rng.integers(0, 4, (ny, nx)).astype(np.int32)) for _ in range(3)], **dict(A, min_hits=2, min_size=2))
    cost = np.where(rng.random((3, ny, nx)) < 0.3, rng.integers(253, 256, (3, ny, nx)), rng.integers(0, 253, (3, ny, nx))).astype(np.uint8)
    group(["thirds", "serpentine", "disc"], cost, **A)
    group(["thirds", "serpentine", "disc"], cost, **dict(A, lethal=256))
    group(["thirds", "serpentine", "rooms"], **dict(A, min_size=n + 1))
    assert len(cases) % B == 0
    return cases


def _reference(b, nx, ny):
    key = (nx, ny)
    if key not in b.cache:
        cases = _cases(nx, ny)
        b.cache[key] = (cases, [ref.frontiers(h, m, c, **kw) for _, h, m, c, kw in cases])
    return b.cache[key]


def _device_inputs(cases):
    hit = torch.tensor(np.stack([c[1] for c in cases]), dtype=torch.int32, device=DEV)
    miss = torch.tensor(np.stack([c[2] for c in cases]), dtype=torch.int32, device=DEV)
    cost = None if cases[0][3] is None else torch.tensor(np.stack([c[3] for c in cases]), device=DEV)
    return hit, miss, cost


def _check(tag, got, want, e=None):
    for name, g, w in zip(("label", "goal", "region", "count"), got, want):
        _same((name, tag), g if e is None else g[e], w)


def _ties(want, nx):
    """How many cells of the first kept region share the smallest representative's key."""
    lab, goal, region, count = want
    r, s, sx, sy = (int(v) for v in region[0])
    cells = np.flatnonzero(lab.ravel() == r)
    keys = [(s * (int(c) % nx) - sx) ** 2 + (s * (int(c) // nx) - sy) ** 2 for c in cells]
    return keys.count(min(keys))


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_every_output_equals_the_reference(bare, nx, ny):
    b = bare
    cases, want = _reference(b, nx, ny)
    n = nx * ny
    idx = lambda k, e: want[3 * k + e]
    # what the reference says about the cases themselves, so that none is vacuous
    for e in range(3):      # all unknown / free / occupied: no frontier
        assert (idx(0, e)[0] == -1).all() and (idx(0, e)[1] == -1).all() and idx(0, e)[3].tolist() == [0, 0]
    iso = idx(3, 0)
    assert iso[3].tolist() == [-(-ny // 2) * -(-nx // 2) if n > 1 else 0] * 2 and (iso[2][:, 1] <= 1).all()      # a lone cell has no neighbour
    firsts = np.flatnonzero(ref.isolated(ny, nx).ravel() == 0)[:64 if n > 1 else 0]
    assert iso[1][:len(firsts)].tolist() == firsts.tolist() and (len(firsts) < 2 or firsts[1] == 2 or nx == 1)
    if n >= 61 * 83:      # the cap and the label tie-break decide the output
        capped = idx(3, 1)
        assert capped[3][0] > 64 and len(set(capped[2][:, 1].tolist())) < 64 and (capped[1] >= 0).all()
        assert idx(4, 0)[3][0] > 1 and idx(1, 0)[3][0] > 16
    if min(nx, ny) >= 12:
        d = idx(1, 1)
        assert d[3][0] == 1 and _ties(d, nx) == 8      # the disc's ring: eight cells equally near the centre
        s = idx(1, 2)
        free = int((ref.serpentine(ny, nx) == 0).sum())      # all of the corridor but the cell above the first gap (and, for odd ny, the one below the last)
        assert s[3].tolist() == [1, free - 1 - ny % 2] and ((nx, ny) != (128, 128) or free - 1 == 8255)
        assert idx(2, 0)[3][0] == 1 and idx(2, 1)[3][0] == 2
        assert idx(2, 1)[2][0, 1] > idx(2, 1)[2][1, 1] > 0      # two rooms of different size
        assert idx(5, 0)[3][0] < idx(1, 0)[3][0]      # min_size 4 drops regions
        assert idx(7, 0)[3][1] < idx(8, 0)[3][1] == idx(1, 0)[3][1]      # lethal cells leave the frontier; lethal 256 keeps all
        assert not np.array_equal(idx(6, 0)[0], ref.frontiers(cases[18][1], cases[18][2], min_hits=1, min_size=2)[0])      # min_hits 2 matters
    for e in range(3):      # nothing kept: no goal, but every label
        none = idx(9, e)
        assert (none[1] == -1).all() and none[3][0] == 0 and (none[2] == [-1, 0, 0, 0]).all()
    assert np.array_equal(idx(9, 0)[0], idx(1, 0)[0]) and (n < 100 or idx(9, 0)[3][1] > 0)
    results = []
    for k in range(0, len(cases), B):
        hit, miss, cost = _device_inputs(cases[k:k + B])
        kw = cases[k][4]
        assert all(c[4] == kw for c in cases[k:k + B])
        results.append((k, hit, miss, cost, _front(b, hit, miss, cost, **kw)))
    torch.cuda.synchronize()
    for k, hit, miss, cost, got in results:
        for e in range(B):
            _check((nx, ny, cases[k + e][0]), got, want[k + e], e)
            assert np.array_equal(hit[e].cpu().numpy(), cases[k + e][1]) and np.array_equal(miss[e].cpu().numpy(), cases[k + e][2])      # the inputs are unchanged
            if cost is not None:
                assert np.array_equal(cost[e].cpu().numpy(), cases[k + e][3])


def test_256_x_256_once(bare):
    b = bare
    nx = ny = 256
    rng = np.random.default_rng(256)
    states = np.stack([rng.integers(0, 3, (ny, nx)) - 1, ref.serpentine(ny, nx), ref.spiral(ny, nx)])
    hit, miss = ref.counts_of(states)
    want = ref.batch(hit, miss, min_size=1, max_regions=64)
    assert want[3][0][0] > 64 and len(set(want[2][0][:, 1].tolist())) < 64 and want[3][1].tolist() == [1, 32895] and want[3][2][0] == 1
    got = _front(b, torch.tensor(hit, device=DEV), torch.tensor(miss, device=DEV), max_regions=64)
    torch.cuda.synchronize()
    _check("256 x 256", got, want)


def test_two_calls_agree_and_envs_do_not_see_each_other(bare):
    b = bare
    for nx, ny in ((61, 83), FIRST_GLOBAL):
        cases, want = _reference(b, nx, ny)
        first, second = [cases[k] for k in (3, 4, 5)], [cases[k] for k in (0, 6, 3)]      # thirds in env 0, then in env 2 beside other neighbours
        a, a2, c = _front(b, *_device_inputs(first)), _front(b, *_device_inputs(first)), _front(b, *_device_inputs(second))
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(a, a2))
        assert all(torch.equal(x[0], y[2]) for x, y in zip(a, c))
        _check("env 2", c, want[3], 2)


def test_null_region_and_count_are_left_untouched(bare):
    b = bare
    for nx, ny in ((16, 12), FIRST_GLOBAL):
        cases, want = _reference(b, nx, ny)
        hit, miss, cost = _device_inputs(cases[3:6])
        full = _front(b, hit, miss)
        for region, count in ((False, True), (True, False), (False, False)):
            got = _front(b, hit, miss, region=region, count=count)
            torch.cuda.synchronize()
            assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1])
            assert torch.equal(got[2], full[2]) if region else int((got[2] != FILL).sum()) == 0
            assert torch.equal(got[3], full[3]) if count else int((got[3] != FILL).sum()) == 0


class _Words:
    """A small int32 output of `shape` per env as .view, `pad` words into a buffer of -12345 with 9 more behind it."""

    def __init__(self, pad, *shape):
        self.pad, self.words = pad, B * int(np.prod(shape))
        self.big = torch.full((pad + self.words + 9,), -12345, dtype=torch.int32, device=DEV)
        self.view = self.big[pad:pad + self.words].view(B, *shape)

    def check(self, want):
        assert (self.big[:self.pad] == -12345).all() and (self.big[self.pad + self.words:] == -12345).all()
        assert torch.equal(self.view, want)


@pytest.mark.parametrize("nx,ny", [(61, 83), FIRST_GLOBAL])
def test_nothing_outside_the_outputs_is_written_and_alignment_does_not_matter(bare, nx, ny):
    """An LDS grid and one labelled in place.  The outputs as views 4, 8 or 12 bytes past a 16-byte boundary inside buffers of
    sentinels: the guards stay untouched and the values are those of the aligned call; the same with hit and miss 4 bytes and the
    cost 1 byte past a 16-byte boundary."""
    b = bare
    cases, want = _reference(b, nx, ny)
    pick = cases[21:24]      # thirds, serpentine, disc with a cost
    hit, miss, cost = _device_inputs(pick)
    cells, G = B * nx * ny, 16
    hbig, mbig = (torch.full((1 + cells + 3,), 55, dtype=torch.int32, device=DEV) for _ in range(2))
    cbig = torch.full((1 + cells + 5,), 99, dtype=torch.uint8, device=DEV)
    hv, mv, cv = hbig[1:1 + cells].view(B, ny, nx), mbig[1:1 + cells].view(B, ny, nx), cbig[1:1 + cells].view(B, ny, nx)
    hv.copy_(hit)
    mv.copy_(miss)
    cv.copy_(cost)
    assert hv.data_ptr() % 16 == 4 and mv.data_ptr() % 16 == 4 and cv.data_ptr() % 16 == 1
    aligned = _front(b, hit, miss, cost)
    assert all(t.data_ptr() % 16 == 0 for t in aligned)
    results = []
    for (h, m, c), pads in (((hit, miss, cost), (37, 37, 37, 37)), ((hv, mv, cv), (37, 37, 37, 37)), ((hit, miss, cost), (36, 37, 36, 38)),
                            ((hv, mv, cv), (38, 36, 39, 36)), ((hit, miss, cost), (39, 38, 37, 39))):
        outs = [Guarded(pads[0], ny, nx), _Words(pads[1], G), _Words(pads[2], G, 4), _Words(pads[3], 2)]
        _front(b, h, m, c, out=[o.view for o in outs])
        results.append(outs)
    torch.cuda.synchronize()
    for e in range(B):
        _check(("aligned", pick[e][0]), aligned, want[21 + e], e)
    for outs in results:
        for o, w in zip(outs, aligned):
            o.check(w)
    assert hbig[0] == 55 and (hbig[1 + cells:] == 55).all() and mbig[0] == 55 and (mbig[1 + cells:] == 55).all() and cbig[0] == 99 and (cbig[1 + cells:] == 99).all()
    assert torch.equal(hv, hit) and torch.equal(mv, miss) and torch.equal(cv, cost)      # the inputs are unchanged


def test_error_codes_and_a_refused_call_writes_nothing(bare):
    b = bare
    L = b.L
    nx = ny = 64
    cells = B * nx * ny
    pool = torch.zeros(6 * cells + 64, dtype=torch.int32, device=DEV)      # one allocation, so that ranges can be made to overlap
    hp, mp, cp, lp, gp, rp = (pool.data_ptr() + 4 * k * cells for k in range(6))      # the cost takes the first quarter of its slot
    kp = rp + 4 * B * 64 * 4      # count, behind the largest region table
    good = dict(nx=nx, ny=ny, min_hits=1, lethal=253, min_size=4, g=16)

    def call(a, h=hp, m=mp, c=cp, l=lp, g=gp, r=rp, k=kp):
        vp = lambda v: ctypes.c_void_p(v) if v else None
        return L.smj_occupancy_to_frontiers(b.ctx, vp(h), vp(m), vp(c), a["nx"], a["ny"], a["min_hits"], a["lethal"], a["min_size"], a["g"], vp(l), vp(g), vp(r),
                                            vp(k), _stream())

    bad = [dict(nx=0), dict(ny=0), dict(nx=-4), dict(ny=-1), dict(nx=4097, ny=1), dict(nx=1, ny=4097), dict(nx=8192, ny=8), dict(nx=257, ny=256),
           dict(nx=256, ny=257), dict(min_hits=0), dict(min_hits=-1), dict(lethal=0), dict(lethal=-3), dict(lethal=257), dict(min_size=0), dict(min_size=-5),
           dict(g=0), dict(g=-1), dict(g=65), dict(g=2 ** 31 - 1)]
    for change in bad:
        rc = call(dict(good, **change))
        assert rc == -1 and L.smj_last_error(b.ctx), (change, rc)
    for kw in (dict(h=None), dict(m=None), dict(l=None), dict(g=None), dict(h=hp + 2), dict(m=mp + 1), dict(l=lp + 3), dict(g=gp + 2), dict(r=rp + 1), dict(k=kp + 2)):
        assert call(good, **kw) == -1, kw      # null / misaligned pointers
    # overlap: an output on an input, on another output, by a whole range and by one word (or byte) at either end
    last, glast, rlast = 4 * (cells - 1), 4 * (B * 16 - 1), 4 * (B * 16 * 4 - 1)
    for kw in (dict(l=hp), dict(l=mp), dict(l=cp), dict(g=hp), dict(r=mp), dict(k=cp), dict(g=lp), dict(r=lp), dict(k=lp), dict(r=gp), dict(k=gp), dict(k=rp),
               dict(l=hp + last), dict(l=mp - last), dict(c=lp + 4 * cells - 1), dict(l=cp + cells - 4), dict(g=lp + last), dict(g=lp - glast), dict(r=gp + glast),
               dict(r=gp - rlast), dict(k=rp + rlast), dict(k=gp - 4), dict(g=hp + last), dict(c=gp + glast + 3)):
        assert call(good, **kw) == -1 and b"overlap" in L.smj_last_error(b.ctx), kw
    torch.cuda.synchronize()
    assert int(pool.abs().max()) == 0      # a refused call writes nothing
    # accepted: the extremes, the largest grids, null optional pointers, adjacent ranges, 64 regions, a misaligned cost
    for gx, gy in ((4096, 16), (16, 4096), (256, 256)):
        n = B * gx * gy
        buf = torch.zeros(4 * n + B * 64 * 6, dtype=torch.int32, device=DEV)      # hit = 0, miss: one unknown cell per env at the far corner
        base = buf.data_ptr()
        buf[n:2 * n] = 1
        buf[n:2 * n].view(B, gy * gx)[:, -1] = 0
        goal, region, count = base + 16 * n, base + 16 * n + 4 * B * 64, base + 16 * n + 4 * B * 64 * 5
        assert call(dict(good, nx=gx, ny=gy, g=64, min_size=1), base, base + 4 * n, None, base + 12 * n, goal, None, None) == 0
        torch.cuda.synchronize()
        assert (buf[16 * n // 4 + B * 64:] == 0).all()      # neither region nor count
        assert call(dict(good, nx=gx, ny=gy, g=64, min_size=2 ** 31 - 1, min_hits=2 ** 31 - 1, lethal=256), base, base + 4 * n, base + 8 * n + 1, base + 12 * n, goal,
                    region, count) == 0
        assert call(dict(good, nx=gx, ny=gy, g=64, min_size=1, lethal=1), base, base + 4 * n, base + 8 * n + 1, base + 12 * n, goal, region, count) == 0
        torch.cuda.synchronize()
        # cost 0 < lethal 1: the two cells beside the unknown corner, which touch diagonally: one region
        a, c = gy * gx - 2, (gy - 1) * gx - 1
        lab = buf[3 * n:4 * n].view(B, gy * gx)[B - 1].cpu().numpy()
        assert (lab[[c, a]] == c).all() and (lab >= 0).sum() == 2
        out = buf[4 * n:].cpu().numpy()
        assert out[:B * 64].reshape(B, 64)[:, 0].tolist() == [c] * B and (out[:B * 64].reshape(B, 64)[:, 1:] == -1).all()
        assert out[B * 64:B * 64 * 5].reshape(B, 64, 4)[B - 1, 0].tolist() == [c, 2, 2 * gx - 3, 2 * gy - 3] and out[B * 64 * 5:B * 64 * 5 + 2 * B].tolist() == [1, 2] * B
        assert (buf[:n] == 0).all() and int(buf[n:2 * n].sum()) == n - B      # the inputs are unchanged


# ------------------------------------------------------------------ the simulator

@pytest.fixture(scope="module")
def rig():
    """The rig of tests/test_gpu_occupancy.py: stretch_scene, three envs driven apart, 200 steps, the lidar on."""
    r = perception_rig.lidar_rig()
    yield r
    r.sim.stop()


def test_end_to_end_from_the_lidar_scan(rig):
    from stretch_mujoco_amd.datamodels import StatusStretchFrontiers

    sim = rig.sim
    fr = sim.pull_frontiers(range_limits=(0.2, 2.0))      # the free disc of 2 m ends inside the 6.4 m grid: its rim is frontier
    assert isinstance(fr, StatusStretchFrontiers) and fr.frame == "base" and fr.cell == 0.05 and fr.origin == (-3.2, -3.2)
    assert tuple(fr.label.shape) == (B, 128, 128) and tuple(fr.goal.shape) == (B, 16) and tuple(fr.region.shape) == (B, 16, 4) and tuple(fr.count.shape) == (B, 2)
    assert all(t.dtype == torch.int32 for t in (fr.label, fr.goal, fr.region, fr.count))
    og = sim.pull_occupancy_grid(range_limits=(0.2, 2.0))      # the same scan, the same buffers
    torch.cuda.synchronize()
    hit, miss = og.hit.cpu().numpy(), og.miss.cpu().numpy()
    want = ref.batch(hit, miss, min_hits=1, min_size=4, max_regions=16)
    print("regions kept and frontier cells per env:", want[3].tolist())
    assert (want[3][:, 0] >= 1).all() and (want[1][:, 0] >= 0).all()      # every env keeps a region
    _check("from the scan", (fr.label, fr.goal, fr.region, fr.count), want)
    # the mask against occupancy(): kept cells are free and have an unknown 4-neighbour
    occ = og.occupancy().cpu().numpy()
    mask = fr.mask().cpu().numpy()
    unknown = np.pad(occ == -1, ((0, 0), (1, 1), (1, 1)))
    near = unknown[:, :-2, 1:-1] | unknown[:, 2:, 1:-1] | unknown[:, 1:-1, :-2] | unknown[:, 1:-1, 2:]
    assert mask.any((1, 2)).all() and (occ[mask] == 0).all() and near[mask].all()
    assert np.array_equal((occ == 0) & near, fr.label.cpu().numpy() >= 0)
    # with the costmap: goals are passable, and the navigation field takes them as they are
    df = sim.pull_distance_field(og, max_distance=0.56)
    cost = df.inflated_cost(0.17, 0.56, 10.0)
    fr2 = sim.pull_frontiers(og, cost=cost, min_size=2, max_regions=8)
    assert fr2.label.data_ptr() != fr.label.data_ptr() and fr2.frame == og.frame and fr2.origin == og.origin      # keyed by (shape, max_regions)
    torch.cuda.synchronize()
    c = cost.cpu().numpy()
    want2 = ref.batch(hit, miss, c, min_hits=1, lethal=253, min_size=2, max_regions=8)
    _check("with the costmap", (fr2.label, fr2.goal, fr2.region, fr2.count), want2)
    assert (want2[3][:, 0] >= 1).all() and (want2[3][:, 1] <= want[3][:, 1]).all() and (want2[3][:, 1] < want[3][:, 1]).any()      # lethal cells left the frontier
    goal = fr2.goal.clone()
    nf = sim.pull_navigation_field(fr2.goal, cost)
    torch.cuda.synchronize()
    pot = nf.potential.cpu().numpy().reshape(B, -1)
    for e in range(B):
        used = sorted(int(g) for g in want2[1][e] if g >= 0)
        assert np.flatnonzero(pot[e] == 0).tolist() == used and len(used) >= 1
    assert torch.equal(fr2.goal, goal) and np.array_equal(nf.goal.cpu().numpy(), want2[1])


def test_int8_path_and_helpers(rig):
    sim = rig.sim
    dev = sim.device
    rng = np.random.default_rng(77)
    ny, nx, cell, origin = 48, 64, 0.05, (-1.6, -1.2)
    states = (rng.integers(0, 3, (B, ny, nx)) - 1).astype(np.int8)
    states[1] = ref.rooms(ny, nx)
    states[2] = 0      # no frontier at all
    grid = torch.tensor(np.where(states > 0, 100, states).astype(np.int8), device=dev)      # the occupancy() convention
    hit, miss = ref.counts_of(states)
    want = ref.batch(hit, miss, min_size=3, max_regions=5)
    fr = sim.pull_frontiers(grid, min_size=3, max_regions=5, cell=cell, origin=origin)
    assert fr.frame == "grid" and fr.cell == cell and fr.origin == origin
    torch.cuda.synchronize()
    _check("int8", (fr.label, fr.goal, fr.region, fr.count), want)
    assert want[3][0, 0] > 5 and want[3][1, 0] == 2 and want[3][2].tolist() == [0, 0]
    bare = sim.pull_frontiers(grid, min_size=3, max_regions=5)
    assert bare.cell == 1.0 and bare.origin == (0.0, 0.0) and bare.label.data_ptr() == fr.label.data_ptr()
    # the helpers against numpy
    lab, goal, region, count = want
    assert np.array_equal(fr.size().cpu().numpy(), region[..., 1])
    used = region[..., 1] > 0
    cen = fr.centroid().cpu().numpy()
    assert cen.dtype == np.float32 and cen.shape == (B, 5, 2) and np.array_equal(np.isnan(cen).any(-1), ~used) and np.isnan(cen[2]).all()
    wc = np.stack((origin[0] + (region[..., 2] / np.maximum(region[..., 1], 1) + 0.5) * cell, origin[1] + (region[..., 3] / np.maximum(region[..., 1], 1) + 0.5) * cell), -1)
    assert np.abs(cen[used] - wc[used]).max() <= 4 * np.spacing(np.float32(3.2))      # the fp32 quotient, sum, product and offset
    gxy = fr.goal_xy().cpu().numpy()
    wg = np.stack((origin[0] + (goal % nx + 0.5) * cell, origin[1] + (goal // nx + 0.5) * cell), -1)
    assert np.array_equal(np.isnan(gxy).any(-1), goal < 0) and np.abs(gxy[goal >= 0] - wg[goal >= 0]).max() <= 4 * np.spacing(np.float32(3.2))
    mask = fr.mask().cpu().numpy()
    wm = np.zeros((B, ny, nx), bool)
    for e in range(B):
        for r in region[e, :, 0]:
            if r >= 0:
                wm[e] |= lab[e] == r
    assert mask.dtype == bool and np.array_equal(mask, wm) and wm[0].sum() < (lab[0] >= 0).sum()


def test_value_errors_are_raised_before_any_launch(rig):
    from stretch_mujoco_amd.datamodels import StatusStretchOccupancyGrid

    sim = rig.sim
    dev = sim.device
    ok = torch.zeros(B, 8, 8, dtype=torch.int8, device=dev)
    cost = torch.zeros(B, 8, 8, dtype=torch.uint8, device=dev)
    og = sim.pull_occupancy_grid(shape=(32, 32))
    df = sim.pull_distance_field(og, nearest=True)
    keep = sim.pull_frontiers(og)
    nav = sim.pull_navigation_field(keep.goal, df, next=True)
    torch.cuda.synchronize()
    snap = [t.clone() for t in (og.hit, og.miss, df.dist2, df.nearest, keep.label, keep.goal, keep.region, keep.count, nav.potential, nav.next)]
    bad_og = StatusStretchOccupancyGrid(time=0, hit=og.hit, miss=og.miss[:, :16], origin=og.origin, cell=og.cell, frame=og.frame)
    for grid, kw in ((ok, dict(min_hits=0)), (og, dict(min_hits=0)), (ok, dict(min_hits=2)), (ok, dict(min_size=0)), (og, dict(min_size=-1)), (og, dict(max_regions=0)),
                     (og, dict(max_regions=65)), (ok, dict(lethal=0)), (og, dict(lethal=257)), (ok.float(), dict()), (ok.to(torch.int32), dict()), (ok[0], dict()),
                     (ok[:2], dict()), ("grid", dict()), (torch.zeros(B, 4097, 1, dtype=torch.int8, device=dev), dict()),
                     (torch.zeros(B, 257, 256, dtype=torch.int8, device=dev), dict()), (torch.zeros(B, 0, 4, dtype=torch.int8, device=dev), dict()),
                     (ok, dict(cost=cost.float())), (ok, dict(cost=cost[0])), (ok, dict(cost=cost[:, :4])), (ok, dict(cost="cost")), (og, dict(cost=cost)),
                     (ok, dict(cell=0.0)), (ok, dict(cell=float("nan"))), (ok, dict(origin=(0.0,))), (ok, dict(origin=(float("inf"), 0.0))), (ok, dict(shape=(8, 8))),
                     (ok, dict(range_limits=(0.2, 2.0))), (og, dict(cell=0.05)), (og, dict(origin=(0.0, 0.0))), (og, dict(frame="world")), (bad_og, dict()),
                     (None, dict(shape=(0, 4))), (None, dict(frame="odom")), (None, dict(range_limits=(2.0, 1.0))), (None, dict(min_size=0))):
        with pytest.raises(ValueError):
            sim.pull_frontiers(grid, **kw)
    torch.cuda.synchronize()
    now = (og.hit, og.miss, df.dist2, df.nearest, keep.label, keep.goal, keep.region, keep.count, nav.potential, nav.next)
    assert all(torch.equal(a, b) for a, b in zip(snap, now))      # nothing ran


def test_the_example_runs():
    """examples/explore_batch.py 2 2: the whole chain, scan to base velocity, in a process of its own."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "explore_batch.py"), "2", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [line for line in out.stdout.splitlines() if "regions" in line]
    print(out.stdout)
    assert len(lines) >= 2 and all("cells seen" in line for line in lines)
