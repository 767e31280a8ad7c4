"""Contact readout (SMJ_SLOT_CONTACTS / StretchBatchSimulator.pull_contact_data) on the CPU: the ABI constants, the decoding of
hand-made records and the helpers, and the kernel's writer through the lane emulator (tests/emul, Emul.bind_contacts)
against the debug dump and the fp64 oracle on identical contacts.  The `-m gpu` twin is
tests/test_gpu_contacts.py."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import MIX_CTRL, MODELS, ROOT, home_qpos
from emul.emul import Emul
from oracle.oracle import Oracle
from stretch_mujoco_amd import StretchBatchSimulator, lib
from stretch_mujoco_amd.datamodels import StatusStretchContacts

W = lib.CONTACT_WORDS


# ---------------------------------------------------------------------------------------------- ABI
def _header_enum():
    src = open(os.path.join(ROOT, "include", "smj.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {k: int(v) for k, v in re.findall(r"\b(SMJ_[A-Z0-9_]+)\s*=\s*(\d+)", src)}


def test_abi_constants_match_header():
    h = _header_enum()
    assert h["SMJ_SLOT_CONTACTS"] == lib.SLOT["CONTACTS"] == 16 and h["SMJ_SLOT_COUNT"] == 17
    assert h["SMJ_READ_CONTACTS"] == lib.READ_CONTACTS == 8
    assert h["SMJ_DIM_CONTACT_CAP"] == lib.DIM["CONTACT_CAP"] == 13 and h["SMJ_DIM_COUNT"] == 14
    assert h["SMJ_CONTACT_WORDS"] == W == 24
    names = dict(DIST="SMJ_CON_DIST", POS="SMJ_CON_POS", FRAME="SMJ_CON_FRAME", FORCE="SMJ_CON_FORCE", GEOM1="SMJ_CON_GEOM1",
                 GEOM2="SMJ_CON_GEOM2", CONDIM="SMJ_CON_CONDIM", EFC_ADR="SMJ_CON_EFC_ADR")
    assert {k: h[v] for k, v in names.items()} == lib.CON
    assert "smj_bind" in lib.EXPORTS and len(lib.EXPORTS) == 15   # no new entry point: the slot and the flag are the interface


def test_cpu_device_still_refused():
    sim = StretchBatchSimulator(num_envs=2, device="cpu", contacts=True)
    with pytest.raises(lib.SmjError):
        sim.start()


# ---------------------------------------------------------------------------------------------- decoding
def _records(B, C, rows):
    """rows: {(env, c): dict(dist, pos, frame, force, g1, g2, dim, efc)} -> float32 records [B, C, 24]."""
    rec = np.zeros((B, C, W), np.float32)
    iv = rec.view(np.int32)
    for (b, c), r in rows.items():
        rec[b, c, 0] = r["dist"]; rec[b, c, 1:4] = r["pos"]; rec[b, c, 4:13] = np.asarray(r["frame"]).ravel()
        rec[b, c, 13:19] = r["force"]
        iv[b, c, 19], iv[b, c, 20], iv[b, c, 21], iv[b, c, 22] = r["g1"], r["g2"], r["dim"], r["efc"]
    return torch.from_numpy(rec)


def _rot(ax, ang):
    c, s = np.cos(ang), np.sin(ang)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[ax]


def test_decoding_and_helpers():
    F1 = _rot("x", 0.4) @ _rot("z", 1.1)          # a contact frame (rows: normal, tangents)
    f1 = np.array([7.0, 1.5, -0.5, 0.01, 0, 0])
    F2 = np.eye(3)
    f2 = np.array([3.0, 0.0, 0.0, 0, 0, 0])
    rows = {(0, 0): dict(dist=-1e-3, pos=[0.1, 0.2, 0.3], frame=F1, force=f1, g1=2, g2=5, dim=3, efc=4),
            (0, 1): dict(dist=-2e-3, pos=[0, 0, 0], frame=F2, force=f2, g1=5, g2=3, dim=1, efc=7),
            (0, 2): dict(dist=5.0, pos=[9, 9, 9], frame=F2, force=[99, 99, 99, 0, 0, 0], g1=1, g2=2, dim=3, efc=0),   # past count: stale
            (1, 0): dict(dist=-1e-4, pos=[1, 1, 1], frame=F2, force=f2, g1=3, g2=2, dim=3, efc=-1)}                  # entered no rows
    rec = _records(2, 4, rows)
    count = torch.tensor([2, 1], dtype=torch.int32)
    # geom -> MJCF body through geom_origbody: geoms 0..5 belong to bodies 0, 0, 4, 6, 6, 9
    gob = torch.tensor([0, 0, 4, 6, 6, 9])
    st = StatusStretchContacts.from_records(rec, count, gob, time=torch.zeros(2))
    assert st.valid.tolist() == [[True, True, False, False], [True, False, False, False]]
    assert st.geom.dtype == torch.int32 and st.geom[0, 0].tolist() == [2, 5] and st.geom[0, 1].tolist() == [5, 3]
    assert st.body[0, 0].tolist() == [4, 9] and st.body[0, 1].tolist() == [9, 6] and st.body[1, 0].tolist() == [6, 4]
    assert st.efc_adr.tolist() == [[4, 7, -1, -1], [-1, -1, -1, -1]] and st.condim[0].tolist() == [3, 1, 0, 0]
    assert float(st.dist[0, 2]) == 0 and float(st.force[0, 2].abs().sum()) == 0 and float(st.pos[0, 2].abs().sum()) == 0   # masked
    np.testing.assert_allclose(st.frame[0, 0].numpy(), F1, atol=1e-6)
    np.testing.assert_allclose(st.force_world[0, 0].numpy(), F1.T @ f1[:3], atol=1e-5)
    np.testing.assert_allclose(st.force_world[0, 1].numpy(), f2[:3], atol=1e-6)
    # sign: + on geom2's body, - on geom1's
    fw0 = F1.T @ f1[:3]
    np.testing.assert_allclose(st.net_force([9], [4])[0].numpy(), fw0, atol=1e-5)          # body 9 is geom2 of contact 0
    np.testing.assert_allclose(st.net_force([4])[0].numpy(), -fw0, atol=1e-5)              # body 4 is geom1 of contact 0
    np.testing.assert_allclose(st.net_force([9])[0].numpy(), fw0 - f2[:3], atol=1e-5)      # geom2 of contact 0, geom1 of contact 1
    np.testing.assert_allclose(st.net_force([4, 9, 6])[0].numpy(), 0 * fw0, atol=1e-5)     # every contact inside the set cancels
    assert st.net_force([4], [6])[0].abs().max() == 0 and st.net_force([9], [9])[0].abs().max() == 0
    assert st.touching([4]).tolist() == [True, False]              # env 1: its only contact entered no rows
    assert st.touching([9], [6]).tolist() == [True, False] and st.touching([4], [6]).tolist() == [False, False]
    assert st.touching([6], [4]).tolist() == [False, False]        # (env 1's contact between 6 and 4 has efc -1)


def test_body_names_through_geom_origbody():
    """The simulator's geom -> body map on a fused blob (the robot's geoms keep the MJCF body they were declared in, though bodies were
    fused) and on a satellite blob (static kitchen geometry: the world body or its fixture body)."""
    from stretch_mujoco_amd import model_blob

    for scene in ("stretch_empty", "stretch_scene_sat"):
        m = model_blob.loads(open(os.path.join(MODELS, scene + ".smjb"), "rb").read())
        import json

        names = json.loads(model_blob.get_str(m, "names_json"))
        gob = np.asarray(m["geom_origbody"]).reshape(-1)
        gbf = np.asarray(m["geom_bodyid"]).reshape(-1)
        assert len(gob) == len(gbf) and gob.max() < len(names["body"])
        # every geom's MJCF body sits on the fused body that carries it
        assert np.array_equal(np.asarray(m["link_fused"]).reshape(-1)[gob], gbf)
        assert (gob == 0).any()                                      # the floor
        fingers = [names["body"].index(n) for n in names["body"] if "finger" in n]
        assert fingers and np.isin(fingers, gob).all()
        if m.get("k_nsat") is not None and int(np.asarray(m["k_nsat"]).ravel()[0]) > 0:
            static = gbf == 0
            assert static.any() and set(np.unique(gob[static])) <= {0} | set(np.nonzero(np.asarray(m["link_fused"]).reshape(-1) == 0)[0])


# ---------------------------------------------------------------------------------------------- kernel logic on the emulator
def _settled(blob, solver, steps=300):
    o = Oracle(blob)
    o.set_option("solver", solver)
    o.arr("ctrl")[:] = np.asarray(MIX_CTRL, np.float64)[: o.dim("nu")] if o.dim("nu") else 0
    o.arr("qpos")[:] = home_qpos(o.arr("qpos"))
    o.step(steps)
    return o


def _oracle_contacts(o):
    n = o.ncon
    co = o.arr("contact").reshape(n, -1)
    ints = np.ascontiguousarray(co[:, 27:29]).view(np.int32).reshape(n, 4)   # dim, geom1, geom2, efc_address
    return co, ints


@pytest.mark.parametrize("scene,variant", [("stretch_empty", "standard"), ("stretch_scene_sat", "sat")])
@pytest.mark.parametrize("solver", [2, 0])
def test_emulated_records_match_dump_and_oracle(scene, variant, solver):
    blob = open(os.path.join(MODELS, scene + ".smjb"), "rb").read()
    o = _settled(blob, solver)
    e = Emul(blob, dict(nq=o.dim("nq"), nv=o.dim("nv"), nu=o.dim("nu"), nlidar=360), num_envs=1, variant=variant)
    e.bind_contacts(64)   # never-written words stay NaN
    try:
        e.buf["qpos"][:, 0] = o.arr("qpos"); e.buf["qvel"][:, 0] = o.arr("qvel"); e.buf["warm"][:, 0] = o.arr("qacc_warmstart")
        e.buf["ctrl"][: o.dim("nu"), 0] = o.arr("ctrl")
        L = e.L
        L.emul_set_option(e.c, b"solver", float(solver))
        # without the flag nothing is written
        e.step(1, 0)
        assert np.isnan(e.rec).all()
        e.buf["qpos"][:, 0] = o.arr("qpos"); e.buf["qvel"][:, 0] = o.arr("qvel"); e.buf["warm"][:, 0] = o.arr("qacc_warmstart")
        state = (o.arr("qpos").copy(), o.arr("qvel").copy(), o.arr("qacc_warmstart").copy())
        e.step(1, lib.READ_CONTACTS)
        n = int(e.buf["info"][1, 0])
        assert 4 <= n <= e.ncon_max
        rec = e.rec[0, :n]
        ri = rec.view(np.int32)
        assert np.isnan(e.rec[0, n:]).all()                                     # past the count: untouched
        # geometry: the debug dump's contact list, bit for bit
        lay = lib.debug_layout(L.emul_nvp(), e.ncon_max, 16 if variant == "sat" else 0)
        dump = e.buf["debug"][lay["con"]:lay["con"] + 8 * n, 0].reshape(n, 8)
        np.testing.assert_array_equal(rec[:, 0:7], dump[:, 0:7])
        code = dump[:, 7].astype(np.int64)
        assert np.array_equal(ri[:, 19], (code >> 4) & 1023) and np.array_equal(ri[:, 20], code >> 14)
        assert np.array_equal(ri[:, 21], code & 15) and (ri[:, 23] == 0).all()
        # forces: the solver's own final row forces -- the debug dump's efc_force (its first 64 rows), bit for bit
        efd = e.buf["debug"][lay["efc_force"]:lay["efc_force"] + 64, 0]
        for c in range(n):
            dim, adr = int(ri[c, 21]), int(ri[c, 22])
            if 0 <= adr and adr + dim <= 64:
                np.testing.assert_array_equal(rec[c, 13:13 + dim], efd[adr:adr + dim])
        # frame: row 0 the normal, orthonormal
        Fr = rec[:, 4:13].reshape(n, 3, 3).astype(np.float64)
        assert np.abs(Fr @ Fr.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5
        # forces: the oracle on the kernel's contact list at the same state, row by row of each contact
        sh = Oracle(blob)
        sh.set_option("solver", solver)
        sh.arr("qpos")[:] = state[0]; sh.arr("qvel")[:] = state[1]; sh.arr("qacc_warmstart")[:] = state[2]
        sh.arr("ctrl")[:] = o.arr("ctrl")
        sh.set_contacts(np.concatenate([rec[:, 0:7].astype(np.float64), ri[:, 19:21].astype(np.float64)], 1))
        sh.forward()
        assert sh.ncon == n
        co, oi = _oracle_contacts(sh)
        ef = sh.arr("efc_force")
        fmax = max(float(np.abs(rec[:, 13]).max()), 1e-9)
        worst = 0.0
        for c in range(n):
            dim, adr = int(ri[c, 21]), int(ri[c, 22])
            assert dim == oi[c, 0] and adr >= 0 and oi[c, 3] >= 0
            want = np.zeros(6); want[:dim] = ef[oi[c, 3]:oi[c, 3] + dim]
            worst = max(worst, float(np.abs(rec[c, 13:19] - want).max()) / fmax)
            assert (rec[c, 13 + dim:19] == 0).all()
            np.testing.assert_allclose(Fr[c, 0], co[c, 4:7], atol=1e-6)      # the oracle keeps the handed normal
        print(f"{scene} solver {solver}: {n} contacts, max |f - oracle| / max normal force = {worst:.2e}")
        # Newton: 1e-4, the bound test_single_step_stages holds efc_force to.  PGS: the fp32 sweeps and the fp64 ones part at 1.7e-4 (empty
        # scene) / 1.0e-4 (16-satellite scene) of the largest normal force (2.0e-4 with 200 fixed sweeps on both sides, so not where they
        # stop; the debug dump's efc_force shows the same gap, checked bit for bit above): held to 5e-4 (contact readout)
        assert worst < (1e-4 if solver == 2 else 5e-4), worst
        assert (rec[:, 13] >= 0).all()                                          # normal forces push apart
        sh.close()
    finally:
        e.close()
        o.close()


# ---------------------------------------------------------------------------------------------- closed-form statics on the oracle
def incline_scene(theta, mu):
    """A robot-less blob: a static box incline of angle theta (about y) and a 2 kg box resting on it, both with sliding friction mu."""
    import math

    from stretch_mujoco_amd import mjcf_compiler as C
    from stretch_mujoco_amd import model_blob as MB
    from stretch_mujoco_amd import model_fuse as F

    n = np.array([math.sin(theta), 0.0, math.cos(theta)])
    d = 0.05 + 0.05 - 0.0002
    xml = ('<mujoco><compiler angle="radian"/><option integrator="implicitfast" cone="elliptic" impratio="20" timestep="0.002"/><worldbody>'
           f'<geom name="incline" type="box" size="1 1 0.05" euler="0 {theta} 0" friction="{mu} 0.005 0.0001"/>'
           f'<body name="box" pos="{n[0] * d} 0 {n[2] * d}" euler="0 {theta} 0"><freejoint/>'
           f'<geom type="box" size=".1 .1 .05" mass="2" friction="{mu} 0.005 0.0001"/></body></worldbody></mujoco>')
    return MB.dumps(F.prepare_for_kernels(C.compile_string(xml))), n


INCLINE = dict(theta=0.3, mu_stick=1.0, mu_slide=0.2, mass=2.0, g=9.81)
# bounds the device is held to (tests/test_gpu_contacts.py); the oracle meets them by orders of magnitude (asserted below)
INCLINE_STICK_TOL = 1e-3   # |F - m g z| / (m g)
INCLINE_RATIO_TOL = 2e-3   # | |F_t| / F_n - mu | / mu
INCLINE_COS_TOL = -0.999   # cos(F_t, sliding velocity) at most


def incline_figures(F, v, n):
    """Total contact force F on the box and its velocity v, incline normal n -> (|F_t| / F_n, cos(F_t, v_t))."""
    fn = float(F @ n)
    ft = F - fn * n
    vt = v - float(v @ n) * n
    return float(np.linalg.norm(ft)) / fn, float(ft @ vt) / (float(np.linalg.norm(ft) * np.linalg.norm(vt)) + 1e-30)


def _oracle_box_force(o, box_geom):
    n = o.ncon
    co = o.arr("contact").reshape(n, -1)
    ii = np.ascontiguousarray(co[:, 27:29]).view(np.int32).reshape(n, 4)
    ef = o.arr("efc_force")
    tot = np.zeros(3)
    for c in range(n):
        f = np.zeros(3)
        k = min(3, int(ii[c, 0]))
        f[:k] = ef[ii[c, 3]:ii[c, 3] + k]
        fw = co[c, 4:13].reshape(3, 3).T @ f
        tot += fw if ii[c, 2] == box_geom else -fw   # + on geom2's body
    return tot


def test_incline_statics_on_the_oracle():
    """The bounds of the device's incline test, set on the fp64 oracle: mu > tan(theta) -- the box sticks and the contacts carry m g z;
    mu < tan(theta) -- it slides, |F_t| / F_n = mu with F_t against the sliding velocity (every 50 steps while it slides)."""
    from stretch_mujoco_amd import model_blob as MB

    P = INCLINE
    mg = P["mass"] * P["g"]
    blob, n = incline_scene(P["theta"], P["mu_stick"])
    box_geom = int(np.nonzero(np.asarray(MB.loads(blob)["geom_bodyid"]).ravel() == 1)[0][0])
    o = Oracle(blob); o.set_option("solver", 2)
    o.step(500); o.forward()
    assert np.linalg.norm(_oracle_box_force(o, box_geom) - [0, 0, mg]) / mg < 1e-3 * INCLINE_STICK_TOL
    o.close()
    blob, n = incline_scene(P["theta"], P["mu_slide"])
    o = Oracle(blob); o.set_option("solver", 2)
    for _ in range(5):
        o.step(50); o.forward()
        ratio, cos = incline_figures(_oracle_box_force(o, box_geom), o.arr("qvel")[0:3].copy(), n)
        assert abs(ratio - P["mu_slide"]) / P["mu_slide"] < 1e-3 * INCLINE_RATIO_TOL and cos < INCLINE_COS_TOL, (ratio, cos)
    o.close()
