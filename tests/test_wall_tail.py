"""The wall tail of the plain inference frame kernel (rm_kernels.h, `march`) on the GPU:

1. frames with the early-out (and with it the tail) against the same frames without it: every bit equal;
2. the switch really happens: tiles that the restated rule (tests/test_wall_tail_rule.py, here on the GPU's own trajectory)
   switches report the look at which they switched as their cost, tiles it refuses report the stepwise nexec;
3. scenes that must not switch do not;
4. the recording kernels keep the bookkeeping of tests/test_march_groups.py.
"""
import functools

import pytest
import torch

from tests import helpers as H
from tests.test_wall_tail_rule import looks_of, same_bits, tiles_of, wall_program, wall_rule

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEP_COUNTS = (31, 32, 33, 36, 64, 128)
IDENT = [1.0, 0.0, 0.0, 0.0]


def scene_module(name):
    from ray_marching_amd.scene import scene_registry as R
    return {"scene2": R.make_test_scene2, "closed": R.make_closed_test_scene, "many32": lambda: R.make_many_primitive_scene(32)}[name]()


def moved_room_scene():
    """Scene 2 with its room under an affine node: the room's box is no longer evaluated in the outermost frame."""
    from oracle import sdf_oracle as O
    s2 = O.scene_test2()
    room = ("affine", {"translation": torch.tensor([0.05, 0.0, 0.0]), "orientation": torch.tensor(IDENT)}, s2[2][0])
    return H.spec_to_module(("union", {}, [room, s2[2][1]]))


def gpu_test_programs():
    """The compiled program whose specialised library the GPU tests of this module load besides those of the default scenes
    and of tests/test_user_leaf.py (__graft_entry__.build() makes it)."""
    from ray_marching_amd.compiler import compile_scene
    return [compile_scene(moved_room_scene())]


def specialised(loop):
    """The loop's scene runs through a per-scene library (the wall tail exists nowhere else)."""
    from ray_marching_amd import _abi
    from ray_marching_amd.compiler import compiled_for
    assert compiled_for(loop.scene).lib(False, loop.precision) is not _abi.lib, "specialised library missing: __graft_entry__.build() makes it"
    return loop


def poses(n, z):
    q = torch.tensor([IDENT, [0.97, 0.05, 0.22, -0.03]][:n], device=DEV)
    t = torch.tensor([[0.0, 0.0, z], [0.4, -0.3, z + 0.5]][:n], device=DEV)
    return torch.nn.functional.normalize(q, dim=-1), t


# ----------------------------------------------------------------------------------------------------------------------
# 1. frames
# ----------------------------------------------------------------------------------------------------------------------
FRAME_CASES = [("scene2", 72, 128, -3.0, "exact"), ("scene2", 40, 64, -3.0, "exact"), ("closed", 72, 128, -1.0, "exact"),
               ("closed", 40, 64, -1.0, "exact"), ("many32", 40, 64, -3.0, "exact"), ("scene2", 72, 128, -3.0, "fast"),
               ("scene2", 40, 64, -3.0, "fast"), ("closed", 72, 128, -1.0, "fast"), ("closed", 40, 64, -1.0, "fast")]


@pytest.mark.parametrize("scene,h,w,z,precision", FRAME_CASES)
def test_frames_equal_the_loop_without_looks(scene, h, w, z, precision):
    """Modes 0 and 4, every step count of STEP_COUNTS: torch.equal with the frame of early_out=False."""
    early = specialised(H.make_loop(scene_module(scene), h, w, early_out=True, precision=precision))
    plain = H.make_loop(scene_module(scene), h, w, early_out=False, precision=precision)
    q, t = poses(1, z)
    with torch.no_grad():
        for mode in (0, 4):
            for steps in STEP_COUNTS:
                got, want = early(q, t, mode, 1, steps), plain(q, t, mode, 1, steps)
                assert got.shape == (1, h, w, 3)
                assert H._same(got, want), (scene, precision, mode, steps, (got - want).abs().max().item())


@pytest.mark.parametrize("variant", ["fp16_module", "row_band", "two_cameras"])
def test_frame_variants_equal_the_loop_without_looks(variant):
    """Scene 2, 72 x 128: an fp16 module, a row band that cuts through tiles, two cameras in one launch."""
    h, w, n = 72, 128, 2 if variant == "two_cameras" else 1
    early = specialised(H.make_loop(scene_module("scene2"), h, w, n=n, early_out=True))
    plain = H.make_loop(scene_module("scene2"), h, w, n=n, early_out=False)
    q, t = poses(n, -3.0)
    rows = (12, 52) if variant == "row_band" else None
    if variant == "fp16_module":
        early, plain, q, t = early.to(torch.float16), plain.to(torch.float16), q.half(), t.half()
    with torch.no_grad():
        for mode in (0, 4):
            for steps in (33, 128):
                got, want = early(q, t, mode, 1, steps, rows=rows), plain(q, t, mode, 1, steps, rows=rows)
                assert H._same(got, want), (variant, mode, steps)


# ----------------------------------------------------------------------------------------------------------------------
# 2. / 3. what the tiles cost
# ----------------------------------------------------------------------------------------------------------------------
def tile_costs(loop, q, t, steps, tiles):
    cost = torch.full((tiles,), -1, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        image = loop(q, t, 0, 1, steps, tile_cost=cost)
    torch.cuda.synchronize()
    return image, cost.cpu()


def restated(loop, h, w, z, steps):
    """The restated rule on the GPU's own trajectory of the frame's rays (rm_march_forward without the early-out, f from
    rm_sdf_forward), tile by tile -> [(stepwise nexec, look of the switch or None)]."""
    from ray_marching_amd import ops
    from ray_marching_amd.compiler import compiled_for
    from tests.test_march_groups import recorded_march
    cs = compiled_for(loop.scene)
    q, t = poses(1, z)
    with torch.no_grad():
        pos, _, dirs = ops.camera_forward(loop.camera.ray_positions, loop.camera.ray_directions, q, t)
        pos, dirs = tiles_of(pos[0], h, w).reshape(-1, 3).contiguous(), tiles_of(dirs[0], h, w).reshape(-1, 3).contiguous()
    out, traj, _ = recorded_march(cs, pos, dirs, steps, early=False)
    with torch.no_grad():
        f = ops.SDFEval.apply(None, traj.to(DEV).reshape(-1, 3), cs).reshape(steps, -1).cpu()
    traj = torch.cat([traj, out[None]]).reshape(steps + 1, -1, 64, 3)
    f, v = f.reshape(steps, -1, 64), dirs.cpu().reshape(-1, 64, 3)
    room = wall_program(cs)
    result = []
    for k in range(traj.shape[1]):
        if room is None:
            nexec, done, _ = stepwise(traj[:, k], steps)
        else:
            nexec, done, end = wall_rule(traj[:, k], lambda i: f[i, k], v[k], room[0], room[1], steps)
            if done is not None:
                assert bool(same_bits(end, traj[steps, k]).all()), ("the rule's tail on the GPU trajectory", k, done)
        result.append((nexec, done))
    return result


def stepwise(traj, steps):
    """The documented early-out alone (tests/test_march_groups.py, replay) -> (nexec, None, None)."""
    lam = torch.zeros(64, dtype=torch.int64)
    snap, snap_step, next_snap = traj[0], 0, 2
    for done in looks_of(steps):
        p, prev = traj[done], traj[done - 1]
        found = torch.where(same_bits(p, prev), 1, torch.where(same_bits(p, snap), done - snap_step, 0))
        lam = torch.where(lam == 0, found, lam)
        if bool((lam > 0).all()):
            return done, None, None
        if done == next_snap:
            snap, snap_step, next_snap = p, done, next_snap * 2
    return steps, None, None


@functools.lru_cache(maxsize=None)
def scene2_restated(steps=128):
    h, w = 72, 128
    return restated(H.make_loop(scene_module("scene2"), h, w), h, w, -3.0, steps)


def test_the_switch_happens():
    """Scene 2, 72 x 128 x 128 at (0, 0, -3): at least half as many tiles as the restated rule switches report a cost below
    `steps` where the stepwise rule gives `steps`; every tile the rule refuses reports the stepwise nexec; the image is the
    one of early_out=False."""
    h, w, steps = 72, 128, 128
    rule = scene2_restated(steps)
    loop = specialised(H.make_loop(scene_module("scene2"), h, w))
    q, t = poses(1, -3.0)
    image, cost = tile_costs(loop, q, t, steps, len(rule))
    with torch.no_grad():
        assert H._same(image, H.make_loop(scene_module("scene2"), h, w, early_out=False)(q, t, 0, 1, steps))
    predicted = [k for k, (nexec, done) in enumerate(rule) if done is not None]
    switched = [k for k, (nexec, done) in enumerate(rule) if nexec == steps and int(cost[k]) < steps]
    print(f"wall tail: {len(switched)} of {len(rule)} tiles switched (rule: {len(predicted)}); "
          f"kernel looks {sorted(set(int(cost[k]) for k in switched))}, rule looks {sorted(set(rule[k][1] for k in predicted))}")
    assert len(predicted) >= 27 and 2 * len(switched) >= len(predicted), (len(switched), len(predicted))
    for k, (nexec, done) in enumerate(rule):
        if done is None:
            assert int(cost[k]) == nexec, (k, int(cost[k]), nexec)
        else:
            assert int(cost[k]) in looks_of(steps) and int(cost[k]) >= 12, (k, int(cost[k]))


def user_sphere_scene():
    from tests.test_user_leaf import USphere, _register, scene2_with
    _register()
    return scene2_with(USphere)


def nan_halfside_scene():
    m = scene_module("scene2")
    with torch.no_grad():
        box = [p for name, p in m.named_parameters() if p.numel() == 3 and bool((p == 5.0).all())][0]
        box[1] = float("nan")
    return m


@pytest.mark.parametrize("name", ["room_under_affine", "user_sphere", "nan_halfside"])
def test_scenes_that_must_not_switch(name):
    """The room under an affine node, scene 2 with its sphere as an unbounded user leaf (no cull site), a NaN half-side: the
    frames are those of early_out=False and every tile costs what the stepwise rule gives it."""
    h, w, steps = 40, 64, 64
    make = {"room_under_affine": moved_room_scene, "user_sphere": user_sphere_scene, "nan_halfside": nan_halfside_scene}[name]
    loop = specialised(H.make_loop(make(), h, w))
    from ray_marching_amd.compiler import compiled_for
    assert (wall_program(compiled_for(loop.scene)) is None) == (name != "nan_halfside")
    q, t = poses(1, -3.0)
    rule = restated(loop, h, w, -3.0, steps)
    image, cost = tile_costs(loop, q, t, steps, len(rule))
    with torch.no_grad():
        assert H._same(image, H.make_loop(make(), h, w, early_out=False)(q, t, 0, 1, steps)), name
    assert all(done is None for _, done in rule), name
    assert [int(c) for c in cost] == [nexec for nexec, _ in rule], name


def test_a_live_edit_that_stretches_the_capsule_through_the_walls():
    """Two frames of one loop: scene 2 as it is (tiles switch), then with its capsule stretched from corner to corner and
    through the walls by an in-place edit, which makes the bounding sphere of the guarded contents cover the room: no tile
    may switch any more."""
    h, w, steps = 40, 64, 64
    loop = specialised(H.make_loop(scene_module("scene2"), h, w))
    q, t = poses(1, -3.0)
    _, before = tile_costs(loop, q, t, steps, (h // 8) * (w // 8))
    rule = restated(loop, h, w, -3.0, steps)
    assert any(int(c) < steps and nexec == steps for c, (nexec, _) in zip(before, rule)), "no tile switched before the edit"
    start, end = [(name, p) for name, p in loop.scene.named_parameters() if name.endswith("start") or name.endswith("end")]
    with torch.no_grad():
        start[1].copy_(torch.tensor([-6.0, -6.0, -6.0]))
        end[1].copy_(torch.tensor([6.0, 6.0, 6.0]))
    image, cost = tile_costs(loop, q, t, steps, len(rule))
    rule = restated(loop, h, w, -3.0, steps)
    plain = H.make_loop(scene_module("scene2"), h, w, early_out=False)
    plain.scene.load_state_dict(loop.scene.state_dict())
    with torch.no_grad():
        assert H._same(image, plain(q, t, 0, 1, steps))
    assert all(done is None for _, done in rule)
    assert [int(c) for c in cost] == [nexec for nexec, _ in rule]


# ----------------------------------------------------------------------------------------------------------------------
# 4. the recording kernels
# ----------------------------------------------------------------------------------------------------------------------
def test_recording_paths_keep_the_stepwise_bookkeeping():
    """Scene 2, 72 x 128 x 128: rm_march_forward with the early-out and a training frame (p_final, trajectory and nexec
    recorded) give, for every tile, the nexec of the stepwise rule -- `steps` on every tile the plain kernel switches."""
    from ray_marching_amd import ops
    from ray_marching_amd.compiler import compiled_for
    from tests.test_march_groups import recorded_march
    h, w, steps = 72, 128, 128
    rule = scene2_restated(steps)
    want = torch.tensor([nexec for nexec, _ in rule], dtype=torch.int32)
    assert int((want == steps).sum()) >= 27
    loop = specialised(H.make_loop(scene_module("scene2"), h, w))
    cs = compiled_for(loop.scene)
    q, t = poses(1, -3.0)
    with torch.no_grad():
        pos, _, dirs = ops.camera_forward(loop.camera.ray_positions, loop.camera.ray_directions, q, t)
        pos, dirs = tiles_of(pos[0], h, w).reshape(-1, 3).contiguous(), tiles_of(dirs[0], h, w).reshape(-1, 3).contiguous()
    _, _, nexec = recorded_march(cs, pos, dirs, steps, early=True)
    assert torch.equal(nexec.reshape(-1, 64), want[:, None].expand(-1, 64))
    image = loop(q, t, 0, 1, steps)                    # the scene's parameters ask for a gradient: a recording frame
    saved = image.grad_fn.saved_tensors
    frame_nexec = [s for s in saved if s is not None and s.dtype == torch.int32][0].cpu().reshape(h, w)
    per_tile = frame_nexec.reshape(h // 8, 8, w // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64)
    assert torch.equal(per_tile, want[:, None].expand(-1, 64))
