"""The lean build on two wavefronts per env (smj_step_impl.h SMJ_W2_COLLISION: the second wavefront runs the collision stage beside the
first one's tree stages and the contact-free head of make_constraint) against the lean build on one wavefront and against the general
build, on the device: option lean_build 1 / 2 / 0 (csrc/smj_builds.h: `lean`, its twin `lean2`, `step`).  One wavefront alone builds
the contact list, in table order, so on the same inputs the three must leave the same bits -- everything tests/test_gpu_lean.py
compares, plus the IMU readout -- and each simulator must have launched the kernel it was asked for (smj_last_build).

Every case runs once (cached) and is looked at by two tests: its own, which asserts the builds launched and everything
test_gpu_lean._assert_equal compares, and test_gpu_imu_readout_of_the_three_builds_bit_for_bit, which asserts the gyro / accelerometer
readouts of all four cases."""
import functools

import numpy as np
import pytest

from test_gpu_lean import _assert_equal as _assert_equal_state

BUILDS = ((1, b"lean"), (2, b"lean2"), (0, b"step"))   # option lean_build -> the tag smj_last_build must report


def _sim(B, lean):
    from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors

    sim = StretchBatchSimulator(num_envs=B, device="cuda:0", contacts=True, sensors_to_use=[StretchSensors.base_gyro, StretchSensors.base_accel])
    sim.start(home=False)
    sim.set_option("lean_build", lean)
    return sim


def _sims(B):
    return [_sim(B, lean) for lean, _ in BUILDS]


def _assert_equal(sims, what, imu):
    """Builds launched and states asserted here; IMU readouts that differ are appended to `imu` with their figures."""
    import torch

    for sim, (lean, tag) in zip(sims, BUILDS):
        assert sim._L.smj_last_build(sim._ctx) == tag, f"{what}: lean_build = {lean}"
    ref = sims[0]
    assert bool((ref.accel != 0).any()), f"{what}: no IMU readout"   # (gravity: never zero; the gyro of a robot at rest is)
    for sim, (lean, _) in list(zip(sims, BUILDS))[1:]:
        w = f"{what}, lean_build {lean} against {BUILDS[0][0]}"
        _assert_equal_state(sim, ref, w)
        for name in ("gyro", "accel"):
            x, y = getattr(sim, name), getattr(ref, name)
            if not torch.equal(x, y):   # the figures: how many envs, which axes, how far
                d = (x - y).abs()
                ulp = (x.view(torch.int32) - y.view(torch.int32)).abs()
                imu.append(f"{w}: {name} differs in {int((d > 0).any(0).sum())} of {x.shape[1]} envs, per axis {(d > 0).sum(1).tolist()}, max |diff| {float(d.max()):.3e}, "
                           f"at most {int(ulp.max())} representable values apart, largest |value| {float(y.abs().max()):.3e}")
                print("\n" + imu[-1])


def _random_action(sims, g):
    import torch

    a = sims[0]
    cr = torch.tensor(np.asarray(a.model["actuator_ctrlrange"]), dtype=torch.float32, device=a.device)
    a.ctrl[:] = cr[:, :1] + (cr[:, 1:] - cr[:, :1]) * torch.rand(a.nu, a.num_envs, generator=g, device=a.device)
    for b in sims[1:]:
        b.ctrl[:] = a.ctrl


def _generator(sim, seed):
    import torch

    g = torch.Generator(device=sim.device)
    g.manual_seed(seed)
    return g


@functools.lru_cache(maxsize=None)
def _three_launches():
    import torch

    sims, imu = _sims(64), []
    g = _generator(sims[0], 21)
    ncon = []
    for w, n in enumerate((50, 50, 10)):
        _random_action(sims, g)
        for sim in sims:
            sim.step(n)
        torch.cuda.synchronize()
        _assert_equal(sims, f"launch {w}", imu)
        ncon.append(float(sims[0].info[1].float().mean()))
    a = sims[0]
    assert int(a.nstep.min()) == int(a.nstep.max()) == 110 and bool(torch.isfinite(a.qpos).all())
    print(f"\nmean contacts per env after the three launches: {ncon}")
    assert np.mean(ncon) >= 1   # the comparison went through the contact list the second wavefront built
    for sim in sims:
        sim.stop()
    return imu


@functools.lru_cache(maxsize=None)
def _pipelined_chunks():
    import torch

    sims, imu = _sims(512), []
    _random_action(sims, _generator(sims[0], 22))
    for sim in sims:
        sim.step(20)
    torch.cuda.synchronize()
    _assert_equal(sims, "512 envs", imu)
    a = sims[0]
    assert int(a.nstep.min()) == int(a.nstep.max()) == 20 and bool(torch.isfinite(a.qpos).all())
    for sim in sims:
        sim.stop()
    return imu


@functools.lru_cache(maxsize=None)
def _mid_step_hand_over():
    import torch

    B, n = 64, 20
    sims, imu = _sims(B), []
    dry = _sim(B, 2)   # the one-wavefront lean build
    g = _generator(dry, 23)
    _random_action([dry], g)
    dry.step(50)
    _random_action([dry], g)
    torch.cuda.synchronize()
    for sim in sims:   # the whole state of an env is in its bound slots
        for name in ("qpos", "qvel", "qacc_warmstart", "ctrl", "nstep"):
            getattr(sim, name).copy_(getattr(dry, name))
    rows = []
    for _ in range(n):
        dry.step(1)
        rows.append(dry.info[0].clone())
    torch.cuda.synchronize()
    assert dry._L.smj_last_build(dry._ctx) == b"lean2" and int(dry.info[3].max()) == 0
    most = torch.stack(rows).max(0).values   # per env: the most rows any of its 20 steps needs
    lo, hi = int(most.min()), int(most.max())
    assert lo < hi, (lo, hi)
    limit = (lo + hi) // 2
    parks = most > limit
    print(f"\nrows needed per env over the {n} steps: {lo} .. {hi}; primary_rows = {limit}: {int(parks.sum())} envs park, {int((~parks).sum())} do not")
    assert bool(parks.any()) and bool((~parks).any())
    for sim in sims:
        sim.set_option("primary_rows", limit)
        sim.step(n)
    torch.cuda.synchronize()
    _assert_equal(sims, f"primary_rows {limit}", imu)
    a = sims[0]
    assert int(a.info[3].max()) == 0   # handed over and finished unflagged
    assert int(a.nstep.min()) == int(a.nstep.max()) == 50 + n and bool(torch.isfinite(a.qpos).all())
    for sim in sims + [dry]:
        sim.stop()
    return imu


@functools.lru_cache(maxsize=None)
def _one_step_launches():
    import torch

    sims, imu = _sims(64), []
    _random_action(sims, _generator(sims[0], 24))
    for k in range(7):
        for sim in sims:
            sim.step(1)
        torch.cuda.synchronize()
        _assert_equal(sims, f"one-step launch {k}", imu)
    a = sims[0]
    assert int(a.nstep.min()) == int(a.nstep.max()) == 7 and bool(torch.isfinite(a.qpos).all())
    for sim in sims:
        sim.stop()
    return imu


@pytest.mark.gpu
def test_gpu_two_wavefront_lean_build_bit_for_bit_over_three_launches():
    """(a) 64 envs x 110 steps in launches of 50 / 50 / 10, a new random action per launch; at least one contact per env on average."""
    _three_launches()


@pytest.mark.gpu
def test_gpu_two_wavefront_lean_build_on_the_pipelined_chunk_path():
    """(b) 512 envs x 20 steps: the smallest batch whose launch goes out as pipelined chunks (option pipeline_min_envs = 511) -- four
    workgroups per env, each with a second wavefront of its own."""
    _pipelined_chunks()


@pytest.mark.gpu
def test_gpu_two_wavefront_lean_build_hands_steps_over_in_mid_step():
    """(c) 64 envs x 20 steps with option primary_rows between the smallest and the largest row count a dry run of the same states and
    actions shows on the one-wavefront build: an env whose step needs more rows parks in mid-step -- the first wavefront leaves the step
    after make_constraint while the second one waits for its next job -- and is finished by `tall`; the others run through.  64 envs:
    the plan is sweep-only (no pipelined chunks, no pollers), so the run is reproducible.  The states the 20 steps start from come from
    50 random-action steps of the dry simulator, so that the envs differ."""
    _mid_step_hand_over()


@pytest.mark.gpu
def test_gpu_two_wavefront_lean_build_in_one_step_launches():
    """(d) step(1) x 7 on 64 envs: every launch is one fork and one join, readouts and contact records with every step."""
    _one_step_launches()


@pytest.mark.gpu
def test_gpu_imu_readout_of_the_three_builds_bit_for_bit():
    """The gyro / accelerometer readouts of the cases (a) .. (d) above, all three builds against each other.

    imu() ends in some sixty wave-uniform fp32 operations.  While the compiler was free to fuse them, every translation unit fused them
    its own way and the three builds disagreed in the last bits (measured: `step` against the one-wavefront lean build in up to 45 of 64
    envs, gyro 1 and accelerometer up to 32 representable values apart; two waves against one in the accelerometer's x axis of up to 37
    of 64 envs).  imu() is now compiled with contraction off (csrc/smj_step_impl.h SMJ_NO_CONTRACT): one rounding per operation, in
    source order, in every build."""
    imu = _three_launches() + _pipelined_chunks() + _mid_step_hand_over() + _one_step_launches()
    assert not imu, "\n".join(imu)
