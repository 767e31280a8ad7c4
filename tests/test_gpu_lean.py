"""The lean twin of the standard Newton build (stretch_mujoco_amd/csrc/smj_kernels_lean.hip) against the general build (option
lean_build = 0) on the device: the lean build only leaves out code its launches can never execute (smj_step_impl.h SMJ_LEAN), so on
the same inputs the two must leave the same bits -- states, warm starts, row / contact / iteration counts, flags, step counters, the
readouts and the contact records -- and each simulator must have launched the kernel it was asked for (smj_last_build)."""
import numpy as np
import pytest


def _pair(B):
    from stretch_mujoco_amd import StretchBatchSimulator

    sims = []
    for lean in (1, 0):
        sim = StretchBatchSimulator(num_envs=B, device="cuda:0", contacts=True)   # the default model, default options, Newton
        sim.start(home=False)
        sim.set_option("lean_build", lean)
        sims.append(sim)
    return sims


def _assert_equal(a, b, what):
    import torch

    for name in ("qpos", "qvel", "qacc_warmstart", "ctrl", "actuator_length", "actuator_velocity", "base_pose", "xpose"):
        assert torch.equal(getattr(a, name), getattr(b, name)), f"{what}: {name}"
    assert torch.equal(a.info[:3], b.info[:3]), f"{what}: nefc / ncon / niter"
    assert torch.equal(a.info[3], b.info[3]), f"{what}: flags"
    assert torch.equal(a.nstep, b.nstep), f"{what}: nstep"
    # contact records of the last step: the words of the contacts each env has (the rest of the slot is never written)
    n = a.info[1].long()
    live = torch.arange(a.contact_cap, device=a.device)[None, :] < n[:, None]
    ra, rb = a.contact_records.view(torch.int32), b.contact_records.view(torch.int32)
    assert torch.equal(ra[live], rb[live]), f"{what}: contact records"


def _builds(a, b):
    return a._L.smj_last_build(a._ctx), b._L.smj_last_build(b._ctx)


@pytest.mark.gpu
def test_gpu_lean_build_equals_general_build_bit_for_bit_over_three_launches():
    """64 envs x 110 steps in launches of 50 / 50 / 10, a new random action per launch."""
    import torch

    B = 64
    a, b = _pair(B)
    cr = torch.tensor(np.asarray(a.model["actuator_ctrlrange"]), dtype=torch.float32, device=a.device)
    g = torch.Generator(device=a.device); g.manual_seed(11)
    ncon = []
    for w, n in enumerate((50, 50, 10)):
        a.ctrl[:] = cr[:, :1] + (cr[:, 1:] - cr[:, :1]) * torch.rand(a.nu, B, generator=g, device=a.device)
        b.ctrl[:] = a.ctrl
        a.step(n); b.step(n)
        torch.cuda.synchronize()
        assert _builds(a, b) == (b"lean", b"step"), f"launch {w}"
        _assert_equal(a, b, f"launch {w}")
        ncon.append(float(a.info[1].float().mean()))
    assert int(a.nstep.min()) == int(a.nstep.max()) == 110
    # the comparison went through the contact rows of the solver: a robot that rests on the plane touches it somewhere (random actions can
    # lift a wheel or the caster, so no more than one contact per env is asked on average)
    assert bool(torch.isfinite(a.qpos).all()) and np.mean(ncon) >= 1
    for sim in (a, b):
        sim.stop()


@pytest.mark.gpu
def test_gpu_lean_build_equals_general_build_on_the_pipelined_chunk_path():
    """512 envs x 20 steps: the smallest batch whose launch goes out as pipelined chunks (option pipeline_min_envs = 511)."""
    import torch

    B = 512
    a, b = _pair(B)
    cr = torch.tensor(np.asarray(a.model["actuator_ctrlrange"]), dtype=torch.float32, device=a.device)
    g = torch.Generator(device=a.device); g.manual_seed(12)
    a.ctrl[:] = cr[:, :1] + (cr[:, 1:] - cr[:, :1]) * torch.rand(a.nu, B, generator=g, device=a.device)
    b.ctrl[:] = a.ctrl
    a.step(20); b.step(20)
    torch.cuda.synchronize()
    assert _builds(a, b) == (b"lean", b"step")
    _assert_equal(a, b, "512 envs")
    assert int(a.nstep.min()) == int(a.nstep.max()) == 20 and bool(torch.isfinite(a.qpos).all())
    for sim in (a, b):
        sim.stop()
