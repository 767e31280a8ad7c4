"""Every build of the step kernel against the fp64 oracle on the device, row by row of tests/build_matrix.py: a primary row runs the bench
workload state-synchronised (the oracle's state uploaded before every step) and must report its own tag from smj_last_build after EVERY
step; a sweep row forces the PGS hand-over into the build and holds the forced run to the unforced one beside it.  Bounds: the project's
existing one-step bounds of each solver and family (tests/test_rollout_parity.py, tests/test_satellites.py, tests/test_collision_fuzz.py),
nothing new.  TEST INFRASTRUCTURE (imports oracle/)."""
import numpy as np
import pytest

import build_matrix as bm
import rollout_common as rc
import stretch_mujoco_amd.model_blob as mb
from oracle.oracle import Oracle
from test_rollout_parity import _check_contacts, _check_events, _check_pgs, _keeps_manifolds

pytestmark = pytest.mark.gpu

def _check_newton_satellites(rel, events, flags):
    """The assertions of test_satellites.test_gpu_satellite_build_state_synchronised, its run with the manifold cache on (the default)."""
    S = rc.state_synchronised
    c, clean, cr, ob = S.contacts, S.clean, S.clean_robot, S.rel_obj
    print(f"\n{len(rel)} env-steps: rel qacc p50 {np.percentile(rel, 50):.1e} p99 {np.percentile(rel, 99):.1e} max {rel.max():.1e}; satellite dofs on their own scale p50 "
          f"{np.percentile(ob, 50):.1e} p99 {np.percentile(ob, 99):.1e} max {ob.max():.1e}; on steps with agreeing contact lists: robot p99 {np.percentile(cr, 99):.1e}; "
          f"events {len(events)}; contacts {c['n']}, steps with differing pair lists {c['mismatched_steps']}")
    assert flags == 0
    assert len(clean) > 0.9 * len(rel) and np.percentile(cr, 99) < rc.TYPICAL_TOL
    rc.assert_object_dofs()
    assert all(ev["explained"] and ev["flags"] == 0 for ev in events) and len(rc.gross_events(events)) <= 0.005 * len(rel) + 2
    assert c["mismatched_steps"] <= 0.005 * len(rel) + 1 and np.percentile(np.array(c["depth"]), 99) < 5e-5


@pytest.mark.parametrize("row", bm.rows("primary", pile=False), ids=bm.row_id)
def test_gpu_primary_build_state_synchronised(row):
    """4 envs x `windows` x 50 steps of the bench workload on the row's build, the oracle's state uploaded before every step.  Asserted in this
    order: the row's tag after every step, no flag, then the solver's and family's bounds -- Newton on the dense builds: _check_events and
    _check_contacts of test_rollout_parity.py; Newton on the satellite builds: _check_newton_satellites; PGS on either: _check_pgs.
    Measured on the device, relative one-step qacc error (0 differing pair lists and flags 0 in every row):

      row            robot p50 / p99      objects p99: own narrowphase / kernel's contact list    contacts compared, events
      step-newton    1.3e-4 / 5.1e-4      --                                                       960, 0
      prof-newton    1.3e-4 / 5.1e-4      --                                                       960, 0
      mid-newton     1.3e-4 / 5.1e-4      6.7e-5 / 5.3e-5                                          1360, 0
      big38-newton   1.1e-4 / 4.8e-4      1.2e-3 / 1.4e-5                                          4517, 0
      big50-newton   1.2e-4 / 5.3e-4      1.3e-4 / 1.4e-5                                          8160, 0
      sat-newton     1.1e-4 / 4.8e-4      1.2e-3 / 1.4e-5                                          4517, 0
      sat2-newton    1.1e-4 / 4.8e-4      1.2e-3 / 1.4e-5                                          4517, 0

      row (PGS)      robot p50 / p90 / p99         objects p99: own / kernel's list (p50 on the kernel's list)   sweeps per step, events
      pgs-pgs        1.3e-4 / 3.7e-4 / 2.6e-3      --                                                             48.9, 0
      prof-pgs       1.3e-4 / 3.7e-4 / 2.6e-3      --                                                             48.9, 0
      midp-pgs       1.4e-4 / 3.5e-4 / 2.8e-3      6.7e-5 / 5.3e-5 (5.3e-5)                                       48.5, 0
      big38p-pgs     9.1e-5 / 1.9e-4 / 5.8e-4      2.6e-3 / 7.0e-5 (2.5e-5)                                       100, 1 (explained at 1e-7: robot 9.2e-2, gone on the kernel's contact list)
      big50p-pgs     1.3e-4 / 3.8e-4 / 2.8e-3      2.3e-3 / 5.5e-5 (3.0e-5)                                       100, 0
      sat1-pgs       1.3e-4 / 4.0e-4 / 2.7e-3      2.3e-3 / 4.9e-5 (2.6e-5)                                       100, 0
      satp-pgs       1.3e-4 / 4.0e-4 / 2.7e-3      2.3e-3 / 4.8e-5 (2.5e-5)                                       100, 0"""
    blob = bm.blob_of(row)
    model = mb.loads(blob)
    B, solver = 4, row["solver"]
    be = rc.HipBackend(row["scene"], B, solver=solver, counters="PROF" in row["slots"])
    for name, v in row["options"].items():
        be.sim.set_option(name, v)
    if solver == bm.PGS:
        be.sim.set_option("qcqp_exact", 1)   # MuJoCo's own QCQP iteration on both sides; MuJoCo's warm start on both sides is the backend's setting
    nsat = be.sim.nsat_max
    rel, events = rc.state_synchronised(be, blob, model, B, row["windows"], seed=row["seed"], solver=solver, twin=_keeps_manifolds(model))
    flags, seen = int(be.sim.info[3].max()), set(be.builds_seen)
    be.close()
    assert seen == {row["tag"]}, seen      # every one of the steps, not most of them
    assert flags == 0
    if solver == bm.PGS:
        _check_pgs(rel, events, f"{bm.row_id(row)}, ")
    elif nsat:
        _check_newton_satellites(rel, events, flags)
    else:
        _check_events(rel, events)
        _check_contacts()


@pytest.mark.parametrize("row", bm.rows("primary", pile=True), ids=bm.row_id)
def test_gpu_big_build_piles_state_synchronised(row):
    """The 64-column build as the model's own kernel: two piles of nine free primitives (54 dofs), 100 steps each, the protocol and the
    bounds of test_collision_fuzz.test_gpu_piles_of_primitives_state_synchronised -- the oracle's state uploaded before every step, contact
    and row counts equal on >= 99 % of the steps, one-step velocities p90 < 1e-4 relative on the steps that agree, no flag -- and `big` after
    every step.  The compared steps start after build_matrix.PILE_SETTLE oracle steps, with all nine bodies resting on each other.
    Measured on the device (the emulator's figures are the same): Newton 200 of 200 steps agree, rel dqvel p50 1.1e-7 / p90 1.8e-5 / max 7.0e-5,
    25 and 17 contacts (75 and 51 rows); PGS 200 of 200, 2.5e-7 / 2.5e-5 / 9.2e-5, 23 and 17 contacts."""
    import torch
    from stretch_mujoco_amd import StretchBatchSimulator

    pgs = row["solver"] == bm.PGS
    agree, total, errs = 0, 0, []
    for pile, blob in enumerate(bm.pile_blobs()):
        o = Oracle(blob); o.set_option("solver", row["solver"])
        sim = StretchBatchSimulator(num_envs=1, device="cuda:0", model_blob_bytes=blob, solver="pgs" if pgs else "newton")
        sim.start(home=False)
        assert sim.nv == 54 and sim.nv_max == 64 and sim.nefc_max == 224
        if pgs:
            sim.set_option("qcqp_exact", 1)   # MuJoCo's own QCQP iteration on both sides
            o.set_option("pgs_dual_warmstart", 1)   # the kernels' default: a second start from the previous step's forces, on both sides
        o.step(bm.PILE_SETTLE)
        for step in range(100):
            for name, t in (("qpos", sim.qpos), ("qvel", sim.qvel), ("qacc_warmstart", sim.qacc_warmstart)):
                t[:, 0] = torch.tensor(o.arr(name), dtype=torch.float32, device=sim.device)
            o.step(1); sim.step(1)
            torch.cuda.synchronize()
            assert sim._L.smj_last_build(sim._ctx) == b"big", (pile, step)
            total += 1
            if int(sim.info[1, 0]) == o.ncon and int(sim.info[0, 0]) == o.nefc:
                agree += 1
                v = o.arr("qvel")
                errs.append(np.abs(sim.qvel[:, 0].cpu().numpy() - v).max() / max(1.0, np.abs(v).max()))
        assert int(sim.info[3, 0]) == 0, (pile, hex(int(sim.info[3, 0])))
        print(f"\npile {pile}: the last step has {o.ncon} contacts, {o.nefc} rows")
        sim.stop()
        o.close()
    print(f"piles of 9 [{bm.row_id(row)}]: {agree} of {total} steps with equal contact / row counts; rel dqvel p50 {np.percentile(errs, 50):.1e} p90 {np.percentile(errs, 90):.1e} max {max(errs):.1e}")
    assert agree >= 0.99 * total and np.percentile(errs, 90) < 1e-4


def _hand_over_stat(sim, o):
    return np.abs(sim.qvel[:, 0].cpu().numpy() - o.arr("qvel")).max() / max(1.0, np.abs(o.arr("qvel")).max())


@pytest.mark.parametrize("row", bm.rows("sweep"), ids=bm.row_id)
def test_gpu_pgs_hand_over_into_the_build(row):
    """The shape of test_gpu_kitchen.test_three_envs_per_cu_build_hands_over_to_the_160_row_build under PGS: 3 envs x 40 steps, the oracle's
    state uploaded before every step, `primary_rows` a few rows under the oracle's settled count so that the row's build finishes the
    step; a second simulator without the limit runs beside it on the same uploads.  Exact on the forced run: no flag, the oracle's row and
    contact counts on the compared steps, the hand-over on at least 30 of the 40 steps, the three envs bit-equal, and without escalation the
    same step is flagged.  Accuracy: |dqvel|.max() / max(1, |qvel_o|.max()) of both runs against the oracle -- the forced run's median and
    0.8 quantile at most TWICE the unforced run's (two roundings of an unconverged 100-sweep iteration, as in
    test_satellites.test_gpu_pgs_two_wavefronts_per_env_agree_with_one); the unforced primary is held to the oracle by its own primary row.
    Measured on the device, 40 of 40 steps beyond the limit and 40 compared steps in every row, median / 0.8 quantile / max:

      row               rows, limit    forced                          unforced
      tall-from-midp    46 .. 52, 42   2.74e-6 / 2.03e-5 / 5.40e-5     2.59e-6 / 1.95e-5 / 5.71e-5
      big-from-big38p   69 .. 72, 66   1.58e-5 / 1.86e-5 / 2.10e-5     1.65e-5 / 1.85e-5 / 2.29e-5
      big-from-big50p   96, 90         4.61e-4 / 4.97e-4 / 1.01e-3     4.61e-4 / 4.97e-4 / 1.01e-3
      sat32-from-satp   96, 90         4.61e-4 / 4.97e-4 / 1.01e-3     4.61e-4 / 4.97e-4 / 1.01e-3

    (the two kitchen4 rows: the same scene on the dense and on the satellite builds; forced and unforced differ beyond the digits printed)"""
    import torch
    from stretch_mujoco_amd import StretchBatchSimulator

    ctrl, settle, under = row["script"]
    blob = bm.blob_of(row)
    sims = []
    for _ in range(2):
        sim = StretchBatchSimulator(num_envs=3, device="cuda:0", scene=row["scene"], solver="pgs")
        sim.start(home=False)
        sim.set_option("qcqp_exact", 1)           # MuJoCo's own QCQP iteration and warm start, as the unmodified oracle's
        sim.set_option("pgs_dual_warmstart", 0)
        sim.ctrl[:] = torch.tensor(ctrl, dtype=torch.float32, device=sim.device).unsqueeze(1)
        sims.append(sim)
    forced, free = sims
    o = Oracle(blob); o.set_option("solver", 0)
    o.arr("ctrl")[:10] = ctrl
    o.step(settle)
    limit = max(30, o.nefc - under)
    forced.set_option("primary_rows", limit)
    over, stat = 0, {"forced": [], "free": []}
    for k in range(40):
        state = {name: torch.tensor(o.arr(name), dtype=torch.float32, device=forced.device).unsqueeze(1) for name in ("qpos", "qvel", "qacc_warmstart")}
        for sim in sims:
            sim.qpos[:] = state["qpos"]; sim.qvel[:] = state["qvel"]; sim.qacc_warmstart[:] = state["qacc_warmstart"]
        o.step(1)
        for sim in sims:
            sim.step(1)
        torch.cuda.synchronize()
        assert forced._L.smj_last_build(forced._ctx).decode() == row["via"] == free._L.smj_last_build(free._ctx).decode(), k
        assert int(forced.info[3].max()) == 0 and int(free.info[3].max()) == 0, k
        assert torch.equal(forced.qpos[:, 0], forced.qpos[:, 1]) and torch.equal(forced.qpos[:, 0], forced.qpos[:, 2]), k
        assert torch.equal(forced.qvel[:, 0], forced.qvel[:, 1]) and torch.equal(forced.qvel[:, 0], forced.qvel[:, 2]), k
        over += int(forced.info[0, 0]) > limit
        counts = (o.nefc, o.ncon)
        if (int(forced.info[0, 0]), int(forced.info[1, 0])) == counts == (int(free.info[0, 0]), int(free.info[1, 0])):
            stat["forced"].append(_hand_over_stat(forced, o))
            stat["free"].append(_hand_over_stat(free, o))
    assert over >= 30, over     # the hand-over was exercised on nearly every step
    f, u = np.array(stat["forced"]), np.array(stat["free"])
    q = lambda a: f"median {np.median(a):.2e}, 0.8 quantile {np.quantile(a, 0.8):.2e}, max {a.max():.2e}"
    print(f"\n[{bm.row_id(row)}] rows beyond {limit} on {over} of 40 steps; {len(f)} compared steps; forced: {q(f)}; unforced: {q(u)}")
    assert len(f) >= 30     # the oracle's row / contact counts
    assert np.isfinite(f).all() and np.isfinite(u).all()
    assert np.median(f) <= 2 * np.median(u) and np.quantile(f, 0.8) <= 2 * np.quantile(u, 0.8), (q(f), q(u))
    forced.set_option("escalate", 0)
    forced.step(1)
    torch.cuda.synchronize()
    assert int(forced.info[3].max()) & 1   # without the hand-over the same step is flagged
    for sim in sims:
        sim.stop()
    o.close()
