"""The leading dimension of the batch-major slots on the CPU: the step kernel's direct batch-major indexing (no staging rows in the
emulator: the load / store blocks of smj_step_impl.h, the debug dumps, the IMU readout, smj_sat.h, the contact writer) run through the
lane emulator with ld = B + pad.  `ld` changes addresses and no arithmetic: every slot equals the packed run's bit for bit and the
padding columns keep their canary.  The device leg is tests/test_gpu_leading_dim.py."""
import os

import numpy as np
import pytest

import stretch_mujoco_amd.model_blob as mb
from capi_rig import CANARY_F32_BITS, CANARY_I32, envs_all_differ, same_bits
from conftest import HOME_CTRL, MIX_CTRL, MODELS, home_qpos
from emul.emul import CANARY_BITS, Emul
from stretch_mujoco_amd import lib

B, STEPS = 3, 20
SPIN_CTRL = [-3, 3, 0.2, 0.3, 2, -1, -1, 0.03, -2, 0.5]
NEWTON, PGS = 2, 0
CONFIGS = [("stretch_empty", "standard", NEWTON), ("stretch_empty", "standard", PGS), ("stretch_scene_sat", "sat", NEWTON)]
IDS = ["empty-standard-newton", "empty-standard-pgs", "scene_sat-sat-newton"]
INPUTS = ("qpos", "qvel", "ctrl", "warm", "bctl", "nstep", "info")   # what a step reads
_packed = {}


def test_the_emulator_and_the_rig_share_one_canary():
    assert CANARY_BITS[np.dtype(np.float32)] == CANARY_F32_BITS and CANARY_BITS[np.dtype(np.int32)] == CANARY_I32


def _run(scene, variant, solver, ld, ignore_ld=False):
    """20 steps from the home pose, another ctrl in every env, IMU and contact readout, the debug slot bound.  Returns (snapshot of the
    [:, :B] views as int32 bit patterns, the stores).  ignore_ld: the stores are bound with ld = B and the inputs are laid out where such
    a kernel reads them (stride B from the store's first word; the input stores are zero elsewhere), so it steps the same states."""
    with open(os.path.join(MODELS, scene + ".smjb"), "rb") as f:
        blob = f.read()
    m = mb.loads(blob)
    nq, nv, nu = (int(x) for x in m["dims"][:3])
    e = Emul(blob, dict(nq=nq, nv=nv, nu=nu, nlidar=360), num_envs=B, debug=True, variant=variant, ld=ld)
    try:
        e.set_option("solver", solver)
        e.bind_contacts(64)
        q = np.repeat(home_qpos(m["qpos0"]).astype(np.float32)[:, None], B, 1)
        u = np.asarray([HOME_CTRL, MIX_CTRL, SPIN_CTRL], np.float32).T[:nu]
        if ignore_ld:
            e.bind(B)
            for k in INPUTS:
                e.store[k][...] = 0
            e.store["qpos"].reshape(-1)[:q.size] = q.reshape(-1)
            e.store["ctrl"].reshape(-1)[:u.size] = u.reshape(-1)
        else:
            e.qpos[:] = q
            e.ctrl[:] = u
        e.step(STEPS, lib.READ_IMU | lib.READ_CONTACTS)
        snap = {k: np.ascontiguousarray(a).view(np.int32).copy() for k, a in e.buf.items()}
        snap["CONTACTS"] = np.ascontiguousarray(e.rec).view(np.int32).copy()
        stores = {k: a.view(np.int32).copy() for k, a in e.store.items()}
        stores["CONTACTS"] = e.rec_store.view(np.int32).copy()
    finally:
        e.close()
    return snap, stores


def _packed_run(cfg):
    if cfg not in _packed:   # computed once per configuration and left unchanged
        _packed[cfg] = _run(*cfg, ld=B)[0]
    return _packed[cfg]


def _assert_padding(stores, only=None):
    for k, full in stores.items():
        if only is not None and k not in only:
            continue
        pad = full[B:] if k == "CONTACTS" else full[..., B:]
        assert pad.size > 0 and (pad == (CANARY_I32 if k in ("info", "nstep") else CANARY_F32_BITS)).all(), (k, "padding written")


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_packed_run_tells_the_envs_apart(cfg):
    """Without this a column mix-up would be invisible: no two envs of the packed run agree in qpos, qvel, act_len or the debug dump; the
    run is a plain one (20 steps everywhere, no flag, contacts in every env)."""
    p = _packed_run(cfg)
    envs_all_differ(p, ["qpos", "qvel", "act_len", "debug", "gyro", "accel", "CONTACTS"])
    assert (p["nstep"] == STEPS).all() and (p["info"][3] == 0).all() and (p["info"][1] >= 1).all() and (p["info"][0] > 0).all()
    n = int(p["info"][1].min())
    assert (p["CONTACTS"][:, :n] != CANARY_F32_BITS).any(axis=(1, 2)).all()    # every env wrote records


@pytest.mark.parametrize("pad", [1, 5])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_padded_run_equals_the_packed_run_bit_for_bit(cfg, pad):
    snap, stores = _run(*cfg, ld=B + pad)
    same_bits(_packed_run(cfg), snap)
    _assert_padding(stores)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_a_kernel_that_ignores_ld_is_noticed(cfg):
    """The negative control: the padded stores bound with ld = B, which is what a kernel indexing with B in place of ld does.  Every access
    stays inside the stores (B < ld).  It steps the packed run's states (its flat [rows][B] image equals the packed run), and both checks
    object: the [:, :B] views differ from the packed run's, and the padding of the output slots has been written."""
    snap, stores = _run(*cfg, ld=B + 5, ignore_ld=True)
    p = _packed_run(cfg)
    for k in ("qpos", "qvel", "act_len"):
        rows = p[k].shape[0]
        assert np.array_equal(stores[k].reshape(-1)[:rows * B].reshape(rows, B), p[k]), k    # the same arithmetic, other addresses
    with pytest.raises(AssertionError):
        same_bits(p, snap)
    for k in ("act_len", "act_vel", "base", "gyro", "accel", "debug"):
        with pytest.raises(AssertionError):
            same_bits({k: p[k]}, {k: snap[k]})
        with pytest.raises(AssertionError):
            _assert_padding(stores, only=(k,))
