"""The deferred-ray backward kernels (DeferToList in k_render_bwd, then k_bwd_hard_n / _a / _b) at the shapes,
modes and list sizes the rest of the suite runs with the list switched off or never checks for a deferred ray.

Every case runs ONE backward of a frame through `run_backward()` and holds it against two references:

1. the in-place walk -- the same frame with ``ops.bwd_hard_capacity = 0`` -- to summation order: |a - b| <= 2e-6 max(1, max|a|)
   with identical NaN patterns (the bound of test_deferred_rays_give_the_same_gradients);
2. CPU autograd on the oracle (oracle.render, with cpu_eval / the link's composition for user-defined nodes): scene parameters
   <= 1e-4, pose <= 1e-4 max(1, scale); modes 1, 2, 5 the NaN pattern element for element and finite components
   <= 2e-4 max(1, scale) (test_fused_vjp_of_the_globally_normalised_shaders).

and asserts ``work[32] == 0`` without the list and ``work[32] > 0`` with it: a case that defers nothing tests nothing here.
The loss of every case is sum(image * weights) / (number of elements of the whole frame): the mean for a whole frame, and
additive over row bands.  CPU references are computed once per (scene, frame, pose, mode, steps, band) and shared.
"""
import functools

import pytest
import torch

from oracle import sdf_oracle as O
from tests import helpers as H
from tests.test_user_leaf import _link_scene_cpu
from tests.test_user_warp import cpu_parameters, cpu_render, spec_of

pytestmark = pytest.mark.gpu

DEV = "cuda"

# poses known to defer: the closed scene seen from inside, close to a wall (test_deferred_rays_give_the_same_gradients), and the
# reference's default position inside the torus of scene 2 (inside_the_torus of tests/test_user_shader.py)
CLOSED_POSE = ((0.98, 0.05, -0.12, 0.03), (0.15, -0.1, -1.2))
CLOSED_POSE_B = ((0.97, -0.1, 0.15, 0.05), (-0.2, 0.1, -1.0))
# a camera of the closed scene whose nearest and farthest surface points (0.79, 8.77) enclose those of CLOSED_POSE_B (1.01, 8.71):
# in a mode 1 batch of the two, the minimum and the maximum -- the two NaN rays -- are both this camera's
CLOSED_POSE_C = ((0.95, 0.2, 0.1, -0.1), (0.3, 0.2, -0.8))
TORUS_POSE = ((0.99, 0.06, -0.08, 0.03), (0.0, 0.0, 1.0))
NORMALISED = (1, 2, 5)


# --------------------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------------------
def perturbed_warped_scene():
    """contrib.make_warped_scene() with the perturbation of test_training_step_moves_a_perturbed_warped_scene_back."""
    from ray_marching_amd.contrib import make_warped_scene
    scene = make_warped_scene()
    mirror = scene.sdfs[1].sdf
    placed = mirror.sdf.sdfs[0]
    with torch.no_grad():
        mirror.origin += 0.05
        placed.sdf.scale += 0.05
        placed.translation += torch.tensor([0.04, -0.03, 0.03])
    return scene


def scene_factories():
    from ray_marching_amd import contrib
    from ray_marching_amd.scene import scene_registry as R
    return {"closed": R.make_closed_test_scene, "scene2": R.make_test_scene2, "open": R.make_test_scene,
            "link": contrib.make_link_scene, "bounded_link": lambda: contrib.make_link_scene(bounded=True),
            "carved": contrib.make_carved_scene, "warped": contrib.make_warped_scene,
            "bounded_warped": lambda: contrib.make_warped_scene(bounded=True), "perturbed_warped": perturbed_warped_scene}


ORACLE_SPECS = {"closed": O.scene_test1_closed, "scene2": O.scene_test2, "open": O.scene_test1}
# the parameters of the user-defined nodes of each scene (suffixes of named_parameters()): case 5 wants a real gradient in each
USER_PARAMETERS = {"link": ("length", "radius1", "radius2"), "bounded_link": ("length", "radius1", "radius2"), "carved": ("blend",),
                   "warped": ("scale", "origin", "period", "halfsides"), "bounded_warped": ("scale", "origin", "period", "halfsides")}


def pose_tensors(poses):
    q = torch.nn.functional.normalize(torch.tensor([p[0] for p in poses], dtype=torch.float32), dim=-1)
    return q, torch.tensor([p[1] for p in poses], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def frame_weights(n, h, w):
    return torch.rand(n, h, w, 3, generator=torch.Generator().manual_seed(3 + 7 * n + h + 131 * w))


@functools.lru_cache(maxsize=None)
def colormap():
    return torch.from_numpy(H.gold("cmap.npz")["cyclic_cmap"])


def loss_of(image, n, h, w, rows):
    r0, r1 = rows if rows is not None else (0, h)
    weights = frame_weights(n, h, w)[:, r0:r1].to(image.device)
    return (image * weights).sum() / (n * h * w * 3)


# --------------------------------------------------------------------------------------------------------------
# the two references and the frame under test
# --------------------------------------------------------------------------------------------------------------
class Gradients:
    """Parameter gradients by name, dL/dq and dL/dt [cameras, 4 | 3], and the two counters of the launch."""

    def __init__(self, params, gq, gt, offered=0, pairs=0):
        self.params, self.gq, self.gt, self.offered, self.pairs = params, gq, gt, offered, pairs

    def items(self):
        return list(self.params.items()) + [("orientation", self.gq), ("translation", self.gt)]

    def __add__(self, other):
        return Gradients({k: v + other.params[k] for k, v in self.params.items()}, self.gq + other.gq, self.gt + other.gt,
                         self.offered + other.offered, self.pairs + other.pairs)


@functools.lru_cache(maxsize=None)
def cpu_reference(scene, h, w, poses, mode, steps, rows=None):
    """CPU autograd through the oracle's render of the same frame (band), fp32.  Cached: callers must not modify it."""
    module = scene_factories()[scene]()
    names = [name for name, _ in module.named_parameters()]
    n = len(poses)
    r0, r1 = rows if rows is not None else (0, h)
    bufs = tuple(b[:, r0:r1] for b in O.camera_buffers(n, w, h, H.PX * h, H.PX * w, H.PX * h))
    q, t = pose_tensors(poses)
    q.requires_grad_(True), t.requires_grad_(True)
    cmap = colormap() if mode in (6, 7) else None
    with pytest.MonkeyPatch.context() as patch:
        if scene in ORACLE_SPECS:
            spec = O.map_spec(ORACLE_SPECS[scene](), lambda x: x.clone().requires_grad_(True))
            params = [x for _, x in O.spec_parameters(spec)]
            image = O.render(spec, bufs, q, t, mode, 1, steps, H.EPS, cmap=cmap)
        elif scene in ("link", "bounded_link"):        # the user LEAF: oracle.sdf_eval of the built-in part, min with the link
            spec, link, lt, lq = _link_scene_cpu()
            spec = O.map_spec(spec, lambda x: x.clone().requires_grad_(True))
            lt.requires_grad_(True), lq.requires_grad_(True)
            params = [x for _, x in O.spec_parameters(spec)] + [lt, lq] + list(link.parameters())
            # (tests/test_user_leaf.py's composition() for the root, which cannot stand in for the sdf_eval it calls itself;
            # sdf_eval's own recursion into the children goes through the same name and stays the oracle's)
            builtin_eval = O.sdf_eval
            patch.setattr(O, "sdf_eval", lambda s, p: builtin_eval(s, p) if s is not spec else torch.minimum(
                builtin_eval(s, p), link.forward(O.quat_rotate(p - lt, O.quat_conj(lq)))))
            image = O.render(spec, bufs, q, t, mode, 1, steps, H.EPS, cmap=cmap)
        else:                                             # user combinators and warps: cpu_eval in the oracle's render
            spec = spec_of(module)
            params = cpu_parameters(spec)
            image = cpu_render(spec, patch, bufs, q, t, mode, 1, steps, H.EPS, cmap=cmap)
    assert len(params) == len(names), (scene, len(params), names)
    loss_of(image, n, h, w, rows).backward()
    grads = {name: (torch.zeros_like(x) if x.grad is None else x.grad).detach().float() for name, x in zip(names, params)}
    return Gradients(grads, q.grad.detach(), t.grad.detach())


def run_backward(monkeypatch, scene, h, w, poses, mode, steps, rows=None, capacity=None, tile8x8=True, early_out=True):
    """One backward of the frame (band) on the GPU with a deferred-ray list of ``capacity`` rays (None: default sizing, 0: every
    ray walked in place).  -> Gradients with work[32] (rays offered to the list) and work[33] ((ray, step) pairs)."""
    from ray_marching_amd import ops
    module = scene_factories()[scene]().to(DEV)
    n = len(poses)
    r0, r1 = rows if rows is not None else (0, h)
    loop = H.make_loop(module, h, w, n=n, tile8x8=tile8x8, early_out=early_out)
    if mode in (6, 7):
        loop.shader.cyclic_cmap = colormap().to(DEV)
    q, t = (x.to(DEV).requires_grad_(True) for x in pose_tensors(poses))
    tiles = int(ops._lib.rm_wave_tiles(n, r1 - r0, w, ops.default_flags(early_out, tile8x8, True)))
    with monkeypatch.context() as knobs:
        knobs.setattr(ops, "bwd_hard_capacity", capacity)
        knobs.setattr(ops, "bwd_tile_cost_sink", torch.zeros(tiles, dtype=torch.int32, device=DEV))      # keeps the workspace
        loss_of(loop(q, t, mode, 1, steps, rows=rows), n, h, w, rows).backward()
        work = ops.bwd_last_work.cpu()
    grads = {name: x.grad.detach().cpu() for name, x in module.named_parameters()}
    return Gradients(grads, q.grad.cpu(), t.grad.cpu(), int(work[32]), int(work[33]))


@functools.lru_cache(maxsize=None)
def in_place_walk(scene, h, w, poses, mode, steps, rows=None, tile8x8=True):
    """The frame with the list switched off: bitwise reproducible, so computed once.  Callers must not modify it."""
    with pytest.MonkeyPatch.context() as patch:
        ref = run_backward(patch, scene, h, w, poses, mode, steps, rows, capacity=0, tile8x8=tile8x8)
    assert ref.offered == 0 and ref.pairs == 0, (ref.offered, ref.pairs)
    return ref


FIGURES = {}      # group -> [cases, least work[32], most work[32], largest list-vs-in-place difference, largest error vs the CPU]


def note(group, offered=None, in_place=None, cpu=None):
    f = FIGURES.setdefault(group, [0, None, None, 0.0, 0.0])
    if offered is not None:
        f[0] += 1
        f[1] = offered if f[1] is None else min(f[1], offered)
        f[2] = offered if f[2] is None else max(f[2], offered)
    f[3] = max(f[3], in_place or 0.0)
    f[4] = max(f[4], cpu or 0.0)
    print(f"deferred backward [{group}]: cases {f[0]}, work[32] {f[1]}..{f[2]}, list vs in place {f[3]:.3g}, vs CPU {f[4]:.3g}")


def same_to_summation_order(got, ref, what):
    """|a - b| <= 2e-6 max(1, max|a|) per tensor, identical NaN patterns.  -> the largest difference."""
    worst = 0.0
    for (name, b), (_, a) in zip(got.items(), ref.items()):
        assert torch.equal(a.isnan(), b.isnan()), (what, name, a, b)
        fin = ~a.isnan()
        if fin.any():
            diff = (a[fin] - b[fin]).abs().max().item()
            bound = 2e-6 * max(1.0, a[fin].abs().max().item())
            print(f"{what}: {name} list vs in place {diff:.3g} (bound {bound:.3g})")
            assert diff <= bound, (what, name, diff, bound)
            worst = max(worst, diff)
    return worst


def matches_cpu(got, want, mode, what):
    """The project's contract against CPU autograd.  -> the largest error."""
    worst = 0.0
    for (name, g), (_, c) in zip(got.items(), want.items()):
        assert g.shape == c.shape, (what, name)
        pose = name in ("orientation", "translation")
        assert torch.equal(c.isnan(), g.isnan()), (what, name, c, g)
        fin = ~c.isnan()
        if not fin.any():
            continue
        err = (g[fin] - c[fin]).abs().max().item()
        scale = c[fin].abs().max().item()
        if mode in NORMALISED:
            bound = 2e-4 * max(1.0, scale)
        else:
            bound = 1e-4 * max(1.0, scale) if pose else 1e-4
        print(f"{what}: {name} vs CPU {err:.3g} (|g| {scale:.3g})")
        assert err <= bound, (what, name, err, bound)
        worst = max(worst, err)
    return worst


def check_case(monkeypatch, group, scene, h, w, poses, mode, steps, rows=None, capacity=None, tile8x8=True, cpu=True):
    """List against the in-place walk and against the CPU; the list took rays, the in-place walk none.  -> the list's Gradients."""
    what = f"{scene} {h}x{w}x{steps} mode {mode}" + (f" rows {rows}" if rows else "") + ("" if tile8x8 else " row-major")
    ref = in_place_walk(scene, h, w, poses, mode, steps, rows, tile8x8)
    got = run_backward(monkeypatch, scene, h, w, poses, mode, steps, rows, capacity, tile8x8)
    print(f"{what}: {got.offered} rays offered to the list, {got.pairs} (ray, step) pairs")
    assert got.offered > 0, f"{what}: no ray was deferred"
    d = same_to_summation_order(got, ref, what)
    e = None
    if cpu:
        want = cpu_reference(scene, h, w, poses, mode, steps, rows)
        e = max(matches_cpu(got, want, mode, what), matches_cpu(ref, want, mode, what + " in place"))
    note(group, got.offered, d, e)
    return got


# --------------------------------------------------------------------------------------------------------------
# 1. every fused mode that marches
# --------------------------------------------------------------------------------------------------------------
# (mode 2's upstream is zero where scene(p) < 1e-2, i.e. on every ray that has arrived: from inside the torus scene 2 defers no
# ray at any step count, so that case looks at the scene from z = -3 and stops after 12 steps, most rays still on their way)
SCENE2_FRONT = ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, -3.0))
MODE_CASES = [("closed", m, 32, CLOSED_POSE) for m in (0, 4, 6, 7, 1, 2, 5)] + [
    ("scene2", 1, 32, TORUS_POSE), ("scene2", 2, 12, SCENE2_FRONT), ("scene2", 5, 32, TORUS_POSE)]


@pytest.mark.parametrize("scene,mode,steps,pose", MODE_CASES, ids=[f"{c[0]}-mode{c[1]}" for c in MODE_CASES])
def test_every_marching_mode_through_the_list(scene, mode, steps, pose, monkeypatch):
    """Modes 0, 4, 6, 7 (per pixel) and 1, 2, 5 (k_render_bwd kinds 3, 2, 1) with deferred rays.  (The pose gradient of a
    one-camera frame of modes 1 and 2 is NaN in the reference -- the rays of the minimum and the maximum reach it -- so mode 1's
    finite dL/dt, which deferred rays get through the `direct` branch of k_bwd_hard_a, is checked in
    test_two_cameras_with_different_poses.)"""
    h, w = 40, 56
    check_case(monkeypatch, "modes", scene, h, w, (pose,), mode, steps)


# --------------------------------------------------------------------------------------------------------------
# 2. frame geometry
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile8x8", [True, False])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("h,w", [(13, 21), (27, 45), (17, 130)])
def test_ragged_frames(h, w, mode, tile8x8, monkeypatch):
    """Frames that are no multiple of the 8x8 tile nor of 64 pixels: wave tiles with lanes that have no pixel."""
    check_case(monkeypatch, "ragged", "closed", h, w, (CLOSED_POSE,), mode, 24, tile8x8=tile8x8)


@pytest.mark.parametrize("mode", [0, 1])
def test_two_cameras_with_different_poses(mode, monkeypatch):
    """k_bwd_hard_a decodes the camera from the band index of the ray: each pose alone defers, the batch defers, and both rows
    of dL/dq and dL/dt are those of the in-place walk and of the CPU.  Mode 1: the batch is normalised as a whole, both NaN
    rays are the first camera's, and the second camera's dL/dt is finite.  For its deferred rays the shader's direct dependence on
    the ray origin arrives only through the `direct` read-modify-write of grad_pos in k_bwd_hard_a: it is there and matches."""
    h, w, steps = 24, 40, 40
    poses = (CLOSED_POSE_C, CLOSED_POSE_B)
    for pose in poses:
        check_case(monkeypatch, "cameras", "closed", h, w, (pose,), mode, steps)
    got = check_case(monkeypatch, "cameras", "closed", h, w, poses, mode, steps)
    assert got.gq.shape == (2, 4) and got.gt.shape == (2, 3)
    want = cpu_reference("closed", h, w, poses, mode, steps)
    if mode == 0:       # the two rows are different numbers: a camera index stuck at 0 cannot give both
        assert (want.gt[0] - want.gt[1]).abs().max().item() > 1e-3
    else:
        assert want.gt[0].isnan().all() and not want.gt[1].isnan().any() and want.gt[1].abs().max().item() > 1e-3, want.gt
        assert (got.gt[1] - want.gt[1]).abs().max().item() <= 2e-4 * max(1.0, want.gt[1].abs().max().item())


BANDS = ((0, 5), (5, 29), (29, 40))


@pytest.mark.parametrize("mode", [0, 1])
def test_row_bands(mode, monkeypatch):
    """A 40-row frame rendered as three bands: k_bwd_hard_a adds row_begin back into the index of the camera buffers.  Each
    band against its own in-place walk and the CPU's band; the middle band defers; the bands' gradients add up to the whole
    frame's in-place gradients (mode 0: mode 1 is normalised per band, so its bands are no parts of the whole frame's)."""
    from ray_marching_amd import ops
    h, w, steps = 40, 56, 40
    total = None
    for rows in BANDS:
        if rows == BANDS[1]:
            got = check_case(monkeypatch, "bands", "closed", h, w, (CLOSED_POSE,), mode, steps, rows=rows)
        else:           # (a band of five rows next to the ceiling may have no ray to defer: same checks without that assertion)
            what = f"closed {h}x{w}x{steps} mode {mode} rows {rows}"
            got = run_backward(monkeypatch, "closed", h, w, (CLOSED_POSE,), mode, steps, rows)
            d = same_to_summation_order(got, in_place_walk("closed", h, w, (CLOSED_POSE,), mode, steps, rows), what)
            e = matches_cpu(got, cpu_reference("closed", h, w, (CLOSED_POSE,), mode, steps, rows), mode, what)
            print(f"{what}: {got.offered} rays offered to the list")
            note("bands", None, d, e)
        total = got if total is None else total + got
    if mode == 0:
        d = same_to_summation_order(total, in_place_walk("closed", h, w, (CLOSED_POSE,), mode, steps), "bands summed")
        note("bands", None, d)
    assert ops.bwd_hard_capacity is None and ops.bwd_tile_cost_sink is None


@pytest.mark.parametrize("tile8x8", [True, False])
@pytest.mark.parametrize("mode", [0, 1])
def test_ragged_frame_of_the_open_scene(mode, tile8x8, monkeypatch):
    """make_test_scene() is open: rays leave it and their iterates become NaN.  The list gives the NaN pattern of the in-place
    walk in every gradient, and the list holds every ray at most once: k_render_bwd runs the lanes of a ragged tile that have
    no pixel as ray 0, and such a lane must not put ray 0 on the list a second time."""
    h, w, steps = 27, 45, 40
    pose = ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, -1.0))
    what = f"open {h}x{w}x{steps} mode {mode}" + ("" if tile8x8 else " row-major")
    ref = in_place_walk("open", h, w, (pose,), mode, steps, None, tile8x8)
    got = run_backward(monkeypatch, "open", h, w, (pose,), mode, steps, tile8x8=tile8x8)
    print(f"{what}: {got.offered} of {h * w} rays offered to the list; NaN in "
          f"{[name for name, g in got.items() if g.isnan().any()]}")
    assert got.offered > 0, f"{what}: no ray was deferred"
    assert got.offered <= h * w, f"{what}: {got.offered} list entries for {h * w} rays"
    d = same_to_summation_order(got, ref, what)
    e = matches_cpu(got, cpu_reference("open", h, w, (pose,), mode, steps), mode, what)
    note("open", got.offered, d, e)


# --------------------------------------------------------------------------------------------------------------
# 3. step counts
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [5, 13, 30, 33, 40])
def test_step_counts(steps, monkeypatch):
    """k_bwd_hard_a fetches eight n_s at once (guarded by s - k >= 0) and k_render_bwd defers from RM_BWD_INLINE_STEPS + 1
    remaining steps on: step counts below, at and off a multiple of eight.  The pose gradients carry step 0's n_0."""
    check_case(monkeypatch, "steps", "closed", 24, 40, (CLOSED_POSE,), 0, steps)


def test_no_list_without_the_early_out(monkeypatch):
    """early_out=False: the reverse sweep walks every step of every ray in place, whatever the capacity."""
    h, w, steps = 24, 40, 13
    got = run_backward(monkeypatch, "closed", h, w, (CLOSED_POSE,), 0, steps, early_out=False)
    assert got.offered == 0 and got.pairs == 0
    e = matches_cpu(got, cpu_reference("closed", h, w, (CLOSED_POSE,), 0, steps), 0, "no early out")
    note("no early out", None, None, e)


# --------------------------------------------------------------------------------------------------------------
# 4. list boundaries
# --------------------------------------------------------------------------------------------------------------
def test_list_boundaries(monkeypatch):
    """Lists that overflow, that end on a partial wave, that are exactly full and that are not a multiple of 4 (the ABI rounds
    the capacity down): the frame of test_deferred_rays_give_the_same_gradients.  N, the number of rays the default list
    takes, is the same every run; only the slot order varies.  work[32] counts offers (an overflowing wave still adds its
    rays), so it may exceed the capacity, but the waves that were refused walk in place and never offer again: never N.
    Against the in-place walk only: CPU autograd through 12 288 rays x 64 steps takes minutes, and the same pose is held against
    the CPU at 40 x 56 in test_every_marching_mode_through_the_list."""
    h, w, steps = 96, 128, 64
    args = ("closed", h, w, (CLOSED_POSE,), 0, steps)
    n_def = check_case(monkeypatch, "capacities", *args, cpu=False).offered
    assert n_def == run_backward(monkeypatch, *args).offered
    assert 64 < n_def < 4096, n_def          # (the default list, max(4096, h w / 8) rays, did not overflow)
    capacities = [4, 64, n_def & ~3, (n_def & ~3) - 4, (n_def + 63) // 64 * 64] + ([n_def + 1] if (n_def + 1) % 4 else [])
    print(f"list boundaries: N = {n_def}, capacities {capacities}")
    for cap in capacities:
        got = check_case(monkeypatch, "capacities", *args, capacity=cap, cpu=False)
        assert got.offered <= n_def, (cap, got.offered, n_def)
        if cap >= n_def:
            assert got.offered == n_def, (cap, got.offered, n_def)


@pytest.mark.parametrize("capacity", [1, 2, 3])
def test_capacities_below_four_are_refused(capacity, monkeypatch):
    """rm_bwd_hard_floats sizes the workspace for any capacity > 0, rm_render_backward rounds the capacity down to a multiple
    of 4 and refuses 0 ("capacity >= 4") before it launches anything: an error, not a k_bwd_hard_a launch of zero blocks and
    not a silent in-place walk.  ops.py passes the capacity through unchanged."""
    from ray_marching_amd import _abi, ops
    assert int(ops._lib.rm_bwd_hard_floats(capacity, 16)) == capacity * (11 + 10 * 16)
    with pytest.raises(_abi.RmError, match="capacity >= 4"):
        run_backward(monkeypatch, "closed", 16, 16, (CLOSED_POSE,), 0, 16, capacity=capacity)
    assert ops.bwd_hard_capacity is None
    got = run_backward(monkeypatch, "closed", 16, 16, (CLOSED_POSE,), 0, 16, capacity=0)      # the launch path is not left broken
    assert got.offered == 0


# --------------------------------------------------------------------------------------------------------------
# 5. user-defined nodes
# --------------------------------------------------------------------------------------------------------------
USER_POSES = {"link": ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, -1.5)), "bounded_link": ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, -1.5)),
              "carved": ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, -1.5)),
              "warped": ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, -3.0)), "bounded_warped": ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, -3.0))}


@pytest.mark.parametrize("mode", [0, 4])
@pytest.mark.parametrize("scene", sorted(USER_POSES))
def test_user_defined_nodes_through_the_list(scene, mode, monkeypatch):
    """A user leaf, the CSG combinators and the four warps (and the variants that sign a bound, so that cull tests sit in the
    program) through k_bwd_hard_n / _b: the other tests of these scenes switch the list off.  Every parameter of a user node
    has a CPU gradient of at least 1e-3 in some component, so that the absolute 1e-4 means something."""
    h, w, steps = 48, 64, 32
    pose = USER_POSES[scene]
    want = cpu_reference(scene, h, w, (pose,), mode, steps)
    for name, g in want.params.items():
        if name.rsplit(".", 1)[-1] in USER_PARAMETERS[scene]:
            print(f"{scene} mode {mode}: CPU gradient of {name}: {g.abs().max().item():.3g}")
            assert g.abs().max().item() >= 1e-3, (scene, mode, name, g)
    check_case(monkeypatch, "user nodes", scene, h, w, (pose,), mode, steps)


# --------------------------------------------------------------------------------------------------------------
# 6. repeatability
# --------------------------------------------------------------------------------------------------------------
def test_eight_runs_of_the_perturbed_warped_frame(monkeypatch):
    """The frame of test_training_step_moves_a_perturbed_warped_scene_back's first step (64 x 96 x 32, mode 4, z = -3), eight
    times through the list: the slot order of the list differs from run to run, each run is within the summation-order bound
    of the in-place walk.  The spread per parameter is printed."""
    h, w, steps = 64, 96, 32
    pose = ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, -3.0))
    args = ("perturbed_warped", h, w, (pose,), 4, steps)
    runs = [check_case(monkeypatch, "repeat", *args) for _ in range(8)]
    assert len({r.offered for r in runs}) == 1, [r.offered for r in runs]
    ref = in_place_walk(*args)
    for (name, a), *others in zip(ref.items(), *[r.items() for r in runs]):
        stack = torch.stack([g for _, g in others])
        spread = (stack.max(dim=0).values - stack.min(dim=0).values).max().item()
        off = (stack - a).abs().max().item()
        print(f"repeatability: {name} |g| {a.abs().max().item():.3g}, spread over 8 runs {spread:.3g}, furthest from in place {off:.3g}")
