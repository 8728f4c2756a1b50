"""The grouped early-out march (rm_kernels.h, `march`: trips of two steps and a look up to RM_EARLY_DENSE_STEPS = 8, then
trips of four steps and one look) against what defines it:

1. frames with the early-out against the same frames without it, where the stepwise loop takes no look at all: every bit
   equal, for step counts on both sides of the head (8), of the group boundary, of the 16-step knowledge drop and of the
   priority step (32), with and without a stepwise remainder, through the specialised kernels and the LDS interpreter;
2. nexec, the recorded trajectory and the final points of rm_march_forward against a host replay of the documented rule
   (fixed point or equality with the snapshot; looks after steps 2, 4, 6, 8, 12, 16, ...; snapshot refreshed at 2, 4, 8, 16, ...)
   on the trajectory of the run without the early-out;
3. the gradients of a recording frame with the early-out against those without it.
"""
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEP_COUNTS = (1, 2, 3, 7, 8, 9, 11, 12, 13, 16, 17, 31, 32, 33, 36, 64)
FRAMES = {"scene2_outside": ("scene2", -3.0), "scene2_inside": ("scene2", 1.0), "closed1": ("closed", -1.0)}


def scene_module(name):
    from ray_marching_amd.scene import scene_registry as R
    return {"scene2": R.make_test_scene2, "closed": R.make_closed_test_scene}[name]()


@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("path", ["specialised", "interpreter"])
def test_frames_equal_the_loop_without_looks(path, frame, monkeypatch):
    """20 x 28 (partial 8x8 tiles on both edges), modes 0 and 4, every step count of STEP_COUNTS: torch.equal."""
    monkeypatch.setenv("RM_SPECIALIZE", "off" if path == "interpreter" else "auto")
    scene, z = FRAMES[frame]
    h, w = 20, 28
    early = H.make_loop(scene_module(scene), h, w, early_out=True)
    plain = H.make_loop(scene_module(scene), h, w, early_out=False)
    q, t = H._pose(z)
    with torch.no_grad():
        for mode in (0, 4):
            for steps in STEP_COUNTS:
                got, want = early(q, t, mode, 1, steps), plain(q, t, mode, 1, steps)
                assert got.shape == (1, h, w, 3)
                assert H._same(got, want), (path, frame, mode, steps, (got - want).abs().max().item())


def bits(x):
    return x.contiguous().view(torch.int32)


def same_bits(a, b):
    """[rays, 3] x [rays, 3] -> [rays]: the three components equal bit for bit (the kernel's same_bits)."""
    return (bits(a) == bits(b)).all(dim=-1)


def replay(traj, final, steps):
    """The documented early-out rule on the full trajectory of 64 rays.  traj [steps, 64, 3] (row i = the iterate before step
    i), final [64, 3] (the iterate after the last step).  -> (nexec, final points [64, 3])."""
    def iterate(i):
        return final if i == steps else traj[i]
    lam = torch.zeros(64, dtype=torch.int64)
    snap, snap_step, next_snap = traj[0], 0, 2
    looks = [d for d in (2, 4, 6, 8) if d <= steps] + list(range(12, steps + 1, 4))
    for done in looks:
        p, prev = iterate(done), iterate(done - 1)
        found = torch.where(same_bits(p, prev), 1, torch.where(same_bits(p, snap), done - snap_step, 0))
        lam = torch.where(lam == 0, found, lam)
        if bool((lam > 0).all()):
            at = done + (steps - done) % lam
            return done, torch.stack([iterate(int(at[k]))[k] for k in range(64)])
        if done == next_snap:
            snap, snap_step, next_snap = p, done, next_snap * 2
    return steps, final


def recorded_march(cs, pos, dirs, steps, early):
    """ops.March on rays that ask for a gradient -> (final points, trajectory [steps, rays, 3], nexec [rays]) on the CPU."""
    from ray_marching_amd import ops
    pos = pos.clone().requires_grad_(True)
    out = ops.March.apply(None, pos, dirs, cs, steps, ops.default_flags(early))
    _, _, traj, nexec = out.grad_fn.saved_tensors
    torch.cuda.synchronize()
    return out.detach().cpu(), traj.cpu(), nexec.cpu()


def test_bookkeeping_against_a_host_replay():
    """256 rays (a 16 x 16 camera at (0, 0, -3), 64 consecutive rays per wave) of scene 2 through rm_march_forward at 12, 32 and
    128 steps: with the early-out, nexec is the look step of the replay for every ray, the trajectory rows below nexec are the
    full run's and the final points those of the replay (which are the full run's: asserted too).  Some wave must have left
    early and some wave must have walked every step, or the test proves nothing."""
    from ray_marching_amd import ops
    from ray_marching_amd.compiler import compiled_for
    h = w = 16
    loop = H.make_loop(scene_module("scene2"), h, w)
    cs = compiled_for(loop.marcher.sdf_scene)
    q, t = H._pose(-3.0)
    with torch.no_grad():
        pos, _, dirs = ops.camera_forward(loop.camera.ray_positions, loop.camera.ray_directions, q, t)
    pos, dirs = pos.reshape(-1, 3).contiguous(), dirs.reshape(-1, 3).contiguous()
    assert pos.shape == (256, 3)
    left_early = walked_all = 0
    for steps in (12, 32, 128):
        full_out, full_traj, full_nexec = recorded_march(cs, pos, dirs, steps, early=False)
        out, traj, nexec = recorded_march(cs, pos, dirs, steps, early=True)
        assert bool((full_nexec == steps).all())
        for g in range(4):
            rays = slice(64 * g, 64 * g + 64)
            want_nexec, want_final = replay(full_traj[:, rays], full_out[rays], steps)
            print(f"march groups: {steps} steps, rays {rays.start}..{rays.stop - 1}: nexec {nexec[rays].unique().tolist()}, "
                  f"replay {want_nexec}")
            assert bool((nexec[rays] == want_nexec).all()), (steps, g, nexec[rays], want_nexec)
            assert bool(same_bits(traj[:want_nexec, rays].reshape(-1, 3), full_traj[:want_nexec, rays].reshape(-1, 3)).all()), (steps, g)
            assert bool(same_bits(out[rays], want_final).all()), (steps, g)
            assert bool(same_bits(out[rays], full_out[rays]).all()), (steps, g)
            left_early += want_nexec < steps
            walked_all += want_nexec == steps
    assert left_early > 0 and walked_all > 0, (left_early, walked_all)


def test_recording_frame_gradients(monkeypatch):
    """The 32 x 32 x 16 training step of the closed scene: its gradients with the early-out against those without it, within
    the bounds tests/test_deferred_backward.py holds a frame's gradients to (matches_cpu: parameters 1e-4, pose
    1e-4 max(1, scale)) -- with a trajectory recorded, the steps from nexec on read p_final, an ulp or two off inside a cycle."""
    from tests.test_deferred_backward import matches_cpu, run_backward
    pose = (((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, -1.0)),)
    got = run_backward(monkeypatch, "closed", 32, 32, pose, 0, 16, early_out=True)
    want = run_backward(monkeypatch, "closed", 32, 32, pose, 0, 16, early_out=False)
    worst = matches_cpu(got, want, 0, "march groups: closed 32x32x16, early-out against none")
    print(f"march groups: recording frame, largest gradient difference {worst:.3g}")
