"""The opt-in precision="fast" build (every line under RM_FAST_MATH in csrc/rm_device.h, compiled with FMA contraction:
librm_hip_fast.so and the specialised fast libraries of scene 2 and closed scene 1) against the CPU oracle in float64.

The fast build is bit-exact with nothing, so one rule is used throughout (tests/helpers.py, fast_*_rule):

    E_fast = |fast - o64|  <=  max(4 E_ref, a floor of float32 resolution),     E_ref = |o32 - o64|

where o32 and o64 are the oracle's own float32 and float64 results on the same inputs, computed here on the CPU next to the
device call.  E_ref is the reference alone: neither the code under test nor the exact device build enters it.  The factor 4
is derived from the documented accuracy of the operations the fast build swaps in (helpers.FAST_FACTOR), not fitted.

A  every node through the fast interpreter's stand-alone kernels (rm_sdf_forward / rm_sdf_backward, march, normals),
B  frames of all eight shader modes on the three prebuilt fast libraries (+ regeneration kernels, fp16 storage, two
   cameras, ragged tiles),
C  frame gradients (k_render_bwd kinds 0-3, the deferred-ray kernels, the reduction tail),
D  CULL_MIN on against off inside the fast interpreter, bit for bit (the one exact assertion the fast build gets: culling
   only skips children, the handlers that still run are the same code).

No test compiles anything: all of it runs on what __graft_entry__.build() left behind, and every test asserts which of the
libraries it ran on.
"""
import functools

import pytest
import torch

from oracle import sdf_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda"

SPECS = {"scene2": O.scene_test2, "scene1c": O.scene_test1_closed, "many8": lambda: O.scene_many(8)}
IDENTITY = ((1.0, 0.0, 0.0, 0.0),)
_PREBUILT = []


# --------------------------------------------------------------------------
# choosing the library
# --------------------------------------------------------------------------
@pytest.fixture
def library(monkeypatch):
    """library("auto"): the prebuilt specialised fast libraries (scene 2, closed scene 1); library("off"): the fast interpreter."""
    from ray_marching_amd import specialize

    def choose(policy):
        assert policy in ("auto", "off")
        monkeypatch.setenv("RM_SPECIALIZE", policy)
        specialize._loaded.clear()
        if policy == "auto" and not _PREBUILT:
            specialize.prebuild_default_scenes()      # no-op when __graft_entry__.build() already made them
            _PREBUILT.append(True)

    yield choose
    specialize._loaded.clear()


@pytest.fixture
def fast_standalone(monkeypatch):
    """module(points), SDFMarcher and SDFNormals take CompiledScene.lib() -- the exact library; here it forwards
    precision="fast", so the stand-alone kernels of the fast build run."""
    from ray_marching_amd.compiler import CompiledScene
    plain = CompiledScene.lib

    def lib(self, backward=False, precision="exact"):
        return plain(self, backward, "fast")

    monkeypatch.setattr(CompiledScene, "lib", lib)


def ran_on(module, specialised, backward=False):
    """Assert the fast library a frame (or, ``backward``, its gradient) of ``module`` takes: a specialised one, or the interpreter."""
    from ray_marching_amd import _abi
    from ray_marching_amd.compiler import compiled_for
    lib = compiled_for(module).lib(backward, "fast")
    assert lib is not _abi.lib
    if specialised:
        assert lib is not _abi.fast_lib(), "specialised fast library missing: __graft_entry__.build() makes it"
    else:
        assert lib is _abi.fast_lib()


def f64(spec):
    return O.map_spec(spec, lambda x: x.detach().double())


# --------------------------------------------------------------------------
# A. every node, in the fast interpreter
# --------------------------------------------------------------------------
NODES = ["sphere", "box", "plane", "line", "disk", "torus", "affine", "rounding", "onion", "union",
         "smooth_union", "scene1", "scene2", "scene1_closed", "scene_many8"]
# Every smooth union above has blend_k = 22, and d = -logsumexp(-k d_i) / k divides whatever rm_exp / rm_log got wrong by k:
# a relative error of 4e-6 in either (a mistyped constant) then moves d by 2e-7 at most, less than d's own rounding.  One
# soft blend (k = 1, the children of the smooth_union node) lets their error through undivided.
SOFT = "smooth_union_soft"


def node_spec(name):
    if name == SOFT:
        return ("smooth_union", {"blend_k": O._t(1.0)}, H.node_specs()["smooth_union"][2])
    return H.node_specs()[name]


@functools.lru_cache(maxsize=None)
def node_points():
    seeded = torch.rand(4096, 3, generator=torch.Generator().manual_seed(7)) * 6 - 3
    return {"seeded": seeded, "f1": torch.from_numpy(H.gold("f1_nodes.npz")["points"])}


@pytest.mark.parametrize("name", NODES + [SOFT])
def test_node_values(name, library, fast_standalone):
    library("off")
    spec = node_spec(name)
    module = H.spec_to_module(spec).to(DEV)
    ran_on(module, specialised=False)
    for which, pts in node_points().items():
        with torch.no_grad():
            got = module(pts.to(DEV))
            o32, o64 = O.sdf_eval(spec, pts), O.sdf_eval(f64(spec), pts.double())
        assert got.shape == (pts.shape[0], 1) and got.dtype == torch.float32
        H.fast_value_rule("A values", f"{name} [{which}]", got, o32, o64)


@pytest.mark.parametrize("name", ["scene1_closed", "scene2", "scene_many8", "disk", "rounding", "line", "torus", "affine",
                                  "onion", "smooth_union", "union", SOFT])
def test_node_gradients(name, library, fast_standalone):
    """Point gradient and every parameter gradient of (d w).sum() against float64 autograd on the oracle, with the tolerances
    test_sdf_backward_vs_oracle_autograd has for the exact build (VJPs use the 1-ulp forms there too: the fast build only
    adds contraction and the hardware exp / log of the forward half)."""
    library("off")
    spec = O.map_spec(node_spec(name), lambda x: x.double().clone().requires_grad_(True))
    module = H.spec_to_module(spec).to(DEV)
    ran_on(module, specialised=False, backward=True)
    gen = torch.Generator().manual_seed(7)
    pts = torch.rand(3000, 3, generator=gen) * 6 - 3
    w = torch.randn(3000, 1, generator=gen)
    p_cpu = pts.double().requires_grad_(True)
    (O.sdf_eval(spec, p_cpu) * w.double()).sum().backward()
    p_gpu = pts.to(DEV).requires_grad_(True)
    (module(p_gpu) * w.to(DEV)).sum().backward()
    err = H.report("grad_points", p_gpu.grad, p_cpu.grad)[0]
    print(f"{name} grad_points: {err:.3g}")
    assert err <= 1e-5
    wants, gots = O.spec_parameters(spec), list(module.named_parameters())
    assert len(wants) == len(gots)
    for (pname, want), (_, got) in zip(wants, gots):
        scale = max(1.0, want.grad.abs().max().item())
        err = (got.grad.cpu().double() - want.grad).abs().max().item()
        print(f"{name} {pname}: {err:.3g} (scale {scale:.3g})")
        assert err <= 1e-4 * scale, (pname, err, scale)


def test_tie_subgradients(library, fast_standalone):
    """The six tie cases of f6_ties.npz with the tolerances of test_tie_subgradients_vs_golden: both children of a tie run
    the same handler code, so a tie survives the fast arithmetic."""
    library("off")
    g = H.gold("f6_ties.npz")
    cases = {
        "union_tie": ("union", {}, [O.scene_sphere(0.5), O.scene_sphere(0.5)]),
        "box_face": ("box", {"halfsides": O._t((0.5, 0.5, 0.5))}),
        "line_clamp": ("line", {"start": O._t((0.0, 0.0, 0.0)), "end": O._t((1.0, 0.0, 0.0)), "radius": O._t(0.1)}),
        "onion_zero": ("onion", {"radius": O._t(0.1)}, O.scene_sphere(1.0)),
        "smooth_tie": ("smooth_union", {"blend_k": O._t(22.0)}, [O.scene_sphere(0.5), O.scene_sphere(0.5)]),
        "disk_edge": ("disk", {"radius": O._t(0.8)}),
    }
    for name, spec in cases.items():
        module = H.spec_to_module(spec).to(DEV)
        ran_on(module, specialised=False, backward=True)
        p = torch.from_numpy(g[name + "_points"]).to(DEV).requires_grad_(True)
        d = module(p)
        d.sum().backward()
        figures = [H.report(name + " d", d, g[name + "_d"])[0], H.report(name + " grad_p", p.grad, g[name + "_grad_p"])[0]]
        figures += [H.report(f"{name} {pname}", prm.grad, g[f"{name}_grad:{pname}"])[0] for pname, prm in module.named_parameters()]
        print(f"tie {name}: |d| {figures[0]:.3g}, |grad_p| {figures[1]:.3g}, parameters {[f'{x:.3g}' for x in figures[2:]]}")
        assert figures[0] <= 1e-6 and figures[1] <= 1e-6, (name, figures)
        assert all(x <= 2e-6 for x in figures[2:]), (name, figures)


def test_march_and_normals(library, fast_standalone):
    """SDFMarcher (12 steps) and SDFNormals of the fast interpreter on closed scene 1, the 256 rays of
    test_random_scene_trees_vs_oracle's set-up: the value rule on p, on n and on lap / lap_scale."""
    from ray_marching_amd.rendering.ray_marching import SDFMarcher, SDFNormals
    library("off")
    spec = O.scene_test1_closed()
    module = H.spec_to_module(spec).to(DEV)
    ran_on(module, specialised=False)
    gen = torch.Generator().manual_seed(1000)
    o = torch.tensor([[0.0, 0.0, -4.0]]).expand(256, 3).contiguous()
    v = torch.nn.functional.normalize(torch.rand(256, 3, generator=gen) - torch.tensor([0.5, 0.5, -0.5]), dim=-1)
    scale = 6 / H.EPS ** 2
    with torch.no_grad():
        p32 = O.march(spec, o, v, 12)
        n32, lap32 = O.normals(spec, p32, H.EPS)
        p64 = O.march(f64(spec), o.double(), v.double(), 12)
        n64, lap64 = O.normals(f64(spec), p64, H.EPS)
        p = SDFMarcher(module)(o.to(DEV), v.to(DEV), 12)
        n, lap = SDFNormals(module, H.EPS).to(DEV)(p)
    H.fast_value_rule("A march", "march p", p, p32, p64)
    H.fast_value_rule("A march", "normals n", n, n32, n64)
    H.fast_value_rule("A march", "laplacian / lap_scale", lap / scale, lap32 / scale, lap64 / scale)


# --------------------------------------------------------------------------
# B. frames
# --------------------------------------------------------------------------
def two_camera_poses():
    """The perturbed poses of test_fp16_io_equals_fp32_arithmetic_on_fp16_storage (n = 2)."""
    gen = torch.Generator().manual_seed(5)
    q = torch.nn.functional.normalize(torch.tensor([[1.0, 0.0, 0.0, 0.0]]) + 0.1 * torch.randn(2, 4, generator=gen), dim=-1).half()
    t = (torch.tensor([[0.0, 0.0, -3.0]]) + 0.2 * torch.randn(2, 3, generator=gen)).half()
    return tuple(map(tuple, q.float().tolist())), tuple(map(tuple, t.float().tolist()))


#            scene      library  (h, w, steps)  q                      t                     modes
FRAMES = {
    "scene2_front": ("scene2", "auto", (48, 64, 64), IDENTITY, ((0.0, 0.0, -3.0),), (0, 1, 2, 3, 4, 6, 7)),
    "scene2_inside": ("scene2", "auto", (48, 64, 64), IDENTITY, ((0.0, 0.0, 1.0),), (0, 1, 4, 5, 6, 7)),
    "scene1c": ("scene1c", "auto", (48, 64, 64), IDENTITY, ((0.1, 0.0, -1.0),), (0, 1, 2, 3, 4, 5, 6, 7)),
    "scene1c_ragged": ("scene1c", "auto", (27, 45, 40), IDENTITY, ((0.1, 0.0, -1.0),), (0, 4)),
    "many8_interpreter": ("many8", "off", (48, 64, 64), IDENTITY, ((0.0, 0.0, -3.0),), (0, 1, 4, 5, 6, 7)),
    "scene2_interpreter": ("scene2", "off", (48, 64, 64), IDENTITY, ((0.0, 0.0, -3.0),), (0, 4)),
    "scene2_two_cameras": ("scene2", "auto", (24, 40, 32)) + two_camera_poses() + ((0, 4),),
}
FRAME_PARAMS = [pytest.param(case, mode, id=f"{case}-mode{mode}") for case, row in FRAMES.items() for mode in row[5]]


@functools.lru_cache(maxsize=None)
def frame_reference(case, mode):
    """(o32, o64) of one frame: computed once, shared, never modified."""
    scene, _, (h, w, steps), q, t, _ = FRAMES[case]
    q, t = torch.tensor(q), torch.tensor(t)
    spec = SPECS[scene]()
    bufs = O.camera_buffers(len(q), w, h, H.PX * h, H.PX * w, H.PX * h)
    cmap = O.synthetic_cmap()
    with torch.no_grad():
        o32 = O.render(spec, bufs, q, t, mode, 1, steps, H.EPS, cmap=cmap)
        o64 = O.render(f64(spec), tuple(b.double() for b in bufs), q.double(), t.double(), mode, 1, steps, H.EPS, cmap=cmap)
    return o32, o64


def fast_loop(case, library, **options):
    scene, policy, (h, w, _), q, t, _ = FRAMES[case]
    library(policy)
    module = H.spec_to_module(SPECS[scene]())
    loop = H.make_loop(module, h, w, n=len(q), precision="fast", **options)
    loop.shader.cyclic_cmap = O.synthetic_cmap().to(DEV)
    ran_on(module, specialised=policy == "auto")
    return loop, torch.tensor(q, device=DEV), torch.tensor(t, device=DEV)


@pytest.mark.parametrize("case,mode", FRAME_PARAMS)
def test_frames(case, mode, library):
    loop, q, t = fast_loop(case, library)
    (h, w, steps) = FRAMES[case][2]
    with torch.no_grad():
        got = loop(q, t, mode, 1, steps)
    assert got.shape == (len(q), h, w, 3)
    H.fast_frame_rule("B frames", f"{case} mode {mode}", got, *frame_reference(case, mode))


def differing_pixels(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return int(((H.ulp_distance(a, b) > 0) | (a.isnan() != b.isnan())).any(dim=-1).sum())


@pytest.mark.parametrize("mode", [0, 4])
def test_regeneration_kernels_and_full_march(mode, library):
    """k_march_regen + k_render_finish (regen=True), and the march without its early-out, of the specialised fast scene-2
    library under the frame rule.  The fast build contracts per kernel, so how many pixels differ in a bit from the tile
    kernel's is printed, not asserted."""
    from ray_marching_amd import ops
    case = "scene2_front"
    steps = FRAMES[case][2][2]
    flags = ops.default_flags(True, True, True, True)
    assert ops.regen_applies(flags, steps, False)
    frames = {}
    for name, options in (("tile", {}), ("pools", {"regen": True}), ("full march", {"early_out": False})):
        loop, q, t = fast_loop(case, library, **options)
        with torch.no_grad():
            frames[name] = loop(q, t, mode, 1, steps)
        H.fast_frame_rule("B frames", f"{case} mode {mode} [{name}]", frames[name], *frame_reference(case, mode))
    print(f"fast build, {case} mode {mode}: {differing_pixels(frames['pools'], frames['tile'])} pixels differ in a bit between "
          f"the pool and tile kernels, {differing_pixels(frames['full march'], frames['tile'])} between the full march and "
          f"the early-out, of {frames['tile'].numel() // 3}")


def fp16_ulp(x):
    """One unit in the last place of the fp16 value x (float64 tensor)."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -14))       # |x| = m 2^e, m in [0.5, 1): 11 significant bits
    return torch.ldexp(torch.ones_like(x), e - 11)


@pytest.mark.parametrize("mode", [0, 4])
def test_fp16_module(mode, library):
    """A scene-2 module cast .to(float16): fp16 storage, fast fp32 arithmetic, one rounding to fp16 -- against o64 on the
    fp16-rounded inputs, rounded once to fp16.  At most 1 % of the values differ, none by more than one fp16 ulp of the value
    (the float32 oracle alone: 0 and 12 of 9216 differ, the largest by one ulp)."""
    from tests.test_gpu_fullsize import _fp16_oracle_inputs
    library("auto")
    h, w, steps = 48, 64, 32
    spec = O.scene_test2()
    module = H.spec_to_module(spec)
    loop = H.make_loop(module, h, w, precision="fast").to(torch.float16)
    assert loop.camera.ray_positions.dtype == torch.float16 and loop.scene.sdfs[0].radius.dtype == torch.float16
    ran_on(module, specialised=True)
    spec16, bufs, tetra = _fp16_oracle_inputs(spec, 1, w, h)
    q, t = torch.tensor(IDENTITY), torch.tensor([[0.0, 0.0, -3.0]])
    with torch.no_grad():
        o32 = O.render(spec16, bufs, q, t, mode, 1, steps, H.EPS, tetra=tetra).half()
        o64 = O.render(f64(spec16), tuple(b.double() for b in bufs), q.double(), t.double(), mode, 1, steps, H.EPS,
                       tetra=tuple(c.double() for c in tetra)).half()
        got = loop(q.to(DEV).half(), t.to(DEV).half(), mode, 1, steps)
    assert got.dtype == torch.float16 and got.shape == (1, h, w, 3)
    got, o32, o64 = got.cpu().double(), o32.double(), o64.double()
    assert torch.equal(got.isnan(), o64.isnan())
    ulps = torch.nan_to_num((got - o64).abs() / fp16_ulp(o64))
    ref = torch.nan_to_num((o32 - o64).abs() / fp16_ulp(o64))
    print(f"fp16 mode {mode}: {int((ulps > 0).sum())} of {ulps.numel()} values differ from o64, the largest by {float(ulps.max()):.3g} "
          f"fp16 ulp (o32: {int((ref > 0).sum())}, {float(ref.max()):.3g})")
    assert float((ulps > 0).double().mean()) <= 0.01
    assert float(ulps.max()) <= 1.0


# --------------------------------------------------------------------------
# C. frame gradients
# --------------------------------------------------------------------------
GRAD_SHAPE = (24, 32, 32)
GRAD_POSE = {"scene2": (0.0, 0.0, -3.0), "scene1c": (0.1, 0.0, -1.0), "many8": (0.0, 0.0, -3.0)}
GRAD_PARAMS = [pytest.param(scene, mode, True, id=f"{scene}-mode{mode}") for scene in SPECS for mode in (0, 3, 4, 6, 7, 5)] \
    + [pytest.param("scene2", 2, True, id="scene2-mode2")] \
    + [pytest.param(scene, 0, False, id=f"{scene}-mode0-no-list") for scene in SPECS]


def grad_weights():
    h, w, _ = GRAD_SHAPE
    return torch.randn(1, h, w, 3, generator=torch.Generator().manual_seed(13))


@functools.lru_cache(maxsize=None)
def gradient_reference(scene, mode):
    """{name: (g32, g64)} of the loss (image W).sum() / (H W): scene parameters, then the pose.  Computed once, never modified."""
    h, w, steps = GRAD_SHAPE
    bufs = O.camera_buffers(1, w, h, H.PX * h, H.PX * w, H.PX * h)
    cmap = O.synthetic_cmap()
    out = []
    for dtype in (torch.float32, torch.float64):
        spec = O.map_spec(SPECS[scene](), lambda x: x.to(dtype).clone().requires_grad_(True))
        q = torch.tensor(IDENTITY, dtype=dtype, requires_grad=True)
        t = torch.tensor([GRAD_POSE[scene]], dtype=dtype, requires_grad=True)
        image = O.render(spec, tuple(b.to(dtype) for b in bufs), q, t, mode, 1, steps, H.EPS, cmap=cmap)
        ((image * grad_weights().to(dtype)).sum() / (h * w)).backward()
        named = O.spec_parameters(spec) + [("orientation", q), ("translation", t)]
        out.append({name: (torch.zeros_like(x) if x.grad is None else x.grad).detach() for name, x in named})
    return {name: (out[0][name], out[1][name]) for name in out[0]}


@pytest.mark.parametrize("scene,mode,listed", GRAD_PARAMS)
def test_frame_gradients(scene, mode, listed, library, monkeypatch):
    """Scene parameters and the pose, with the deferred-ray list at its default size and (``listed`` False) switched off."""
    from ray_marching_amd import ops
    h, w, steps = GRAD_SHAPE
    policy = "off" if scene == "many8" else "auto"
    library(policy)
    module = H.spec_to_module(SPECS[scene]())
    loop = H.make_loop(module, h, w, precision="fast")
    loop.shader.cyclic_cmap = O.synthetic_cmap().to(DEV)
    ran_on(module, specialised=policy == "auto")
    ran_on(module, specialised=policy == "auto", backward=True)
    q = torch.tensor(IDENTITY, device=DEV, requires_grad=True)
    t = torch.tensor([GRAD_POSE[scene]], device=DEV, requires_grad=True)
    tiles = int(ops._lib.rm_wave_tiles(1, h, w, ops.default_flags(True, True, True)))
    monkeypatch.setattr(ops, "bwd_hard_capacity", None if listed else 0)
    monkeypatch.setattr(ops, "bwd_tile_cost_sink", torch.zeros(tiles, dtype=torch.int32, device=DEV))      # keeps the workspace
    image = loop(q, t, mode, 1, steps)
    ((image * grad_weights().to(DEV)).sum() / (h * w)).backward()
    offered = int(ops.bwd_last_work.cpu()[32])
    print(f"{scene} mode {mode}: {offered} rays offered to the deferred-ray list")
    if not listed:
        assert offered == 0
    elif mode != 3:                 # (the vignette reaches no scene parameter: nothing to walk, nothing deferred)
        assert offered > 0, "this frame is expected to defer rays: the deferred-ray kernels of the fast build are under test"
    gots = [(name, p.grad) for name, p in module.named_parameters()] + [("orientation", q.grad), ("translation", t.grad)]
    wants = gradient_reference(scene, mode)
    assert len(gots) == len(wants)
    for (_, got), (wname, (g32, g64)) in zip(gots, wants.items()):
        got = torch.zeros_like(g32) if got is None else got.reshape(g64.shape)
        H.fast_gradient_rule("C gradients", f"{scene} mode {mode}{'' if listed else ' no list'} {wname}", got, g32, g64)


# --------------------------------------------------------------------------
# D. culling stays exact inside the fast interpreter
# --------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["scene2", "many32", "tree4", "tree13"])
def test_union_culling_changes_no_bit(case, library, fast_standalone, monkeypatch):
    """The body of tests/test_gpu_parity.py's test of the same name through the fast interpreter: RM_CULL=0 against RM_CULL=1,
    values, gradients and frames bit for bit.  This pins the cull margins (cull_min_test, the by-children test) against
    the 1-ulp square root inside them."""
    from ray_marching_amd import _abi, ops
    from ray_marching_amd.compiler import compiled_for
    from ray_marching_amd.scene.scene_registry import make_many_primitive_scene, make_test_scene2
    library("off")                                       # same (interpreter) kernels on both sides
    # bitwise comparison of parameter gradients: keep every ray in its own wave (the deferred-ray list is filled
    # through an atomic counter, so its order -- and with it the grouping of partial sums -- varies run to run)
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)
    gen = torch.Generator().manual_seed(77)
    pts = torch.cat([torch.rand(4096, 3, generator=gen) * 8 - 4,          # far from the objects: culls fire
                     torch.rand(4096, 3, generator=gen) * 2 - 1]).to(DEV)   # among them: they do not
    wts = torch.randn(8192, 1, generator=gen).to(DEV)

    def make():
        if case == "scene2":
            return make_test_scene2()
        if case == "many32":
            return make_many_primitive_scene(32)
        g = torch.Generator().manual_seed(1000 + int(case[4:]))
        return H.spec_to_module(O.map_spec(H.random_spec(g), lambda x: x.clone().float()))

    res, n_cull = {}, {}
    monkeypatch.setenv("RM_CULL_MIN_COST", "40" if not case.startswith("tree") else "0")   # trees: cull everything boundable
    for cull in ("0", "1"):
        monkeypatch.setenv("RM_CULL", cull)
        module = make().to(DEV)
        cs = compiled_for(module)
        ran_on(module, specialised=False)
        ran_on(module, specialised=False, backward=True)
        n_cull[cull] = int((cs.program.reshape(-1, 4)[:, 0] == _abi.OP_CULL_MIN).sum())
        p = pts.clone().requires_grad_(True)
        d = module(p)
        (d * wts).sum().backward()
        loop = H.make_loop(module, 40, 72, precision="fast")
        q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV); t = torch.tensor([[0.0, 0.0, -3.0]], device=DEV)
        with torch.no_grad():
            frames = [loop(q, t, m, 1, 48) for m in (0, 4, 5)]
        for prm in module.parameters():
            prm.grad = None
        loop(q, t, 0, 1, 24).pow(2).mean().backward()
        res[cull] = dict(d=d.detach(), gp=p.grad, frames=frames,
                         gw=[None if x.grad is None else x.grad.clone() for x in module.parameters()])
    assert n_cull["0"] == 0
    assert n_cull["1"] > 0, "every case here is expected to carry CULL_MIN instructions"
    a, b = res["0"], res["1"]
    assert H._same(a["d"], b["d"]) and H._same(a["gp"], b["gp"])
    for x, y in zip(a["frames"], b["frames"]):
        assert H._same(x, y)
    for x, y in zip(a["gw"], b["gw"]):
        assert (x is None) == (y is None)
        if x is not None:
            assert H._same(x, y)
