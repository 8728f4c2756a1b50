"""User-defined leaves, combinators, warps, shaders and material nodes in the two storage regimes no other user-extension test
reaches (StaticCfg, csrc/rm_kernels.h): the LDS tape (HybridStore, n_slots >= RM_LDS_TAPE_MIN_SLOTS = 17) and the gradient
accumulator rows (RowAccStore, n_params + n_grad_derived > 96, built and run under RM_STATIC_BACKWARD_ACC).

Hand-built scenes inside make_room(), each held to its regime on the CPU (test_every_program_is_in_its_regime):

    wide                  LDS tape, register accumulators     every user opcode, SDFLink, four contrib warps / combinators
    wide_rows             LDS tape, accumulator rows          wide + three placed boxes
    narrow_rows           register tape, accumulator rows     a smooth union of warped and placed nodes, smoothly carved
    twin_builtin / _user  LDS tape, register accumulators     built-in nodes / restated with UAffine, USphere, UMin (RM_CULL=0)
    twin_*_rows           LDS tape, accumulator rows          the twins with four more affine frames
    wide_material, wide_rows_material                         SDFMaterial around three subtrees of wide / wide_rows

The CPU side of every comparison is tests/test_user_warp.py's cpu_eval over spec_of (with one more kind here, ("leaf", instance),
evaluated by the instance's own forward), tests/test_materials.py's ref_eval for the material legs and the shader files' own
cpu_frame; every tolerance is the one the project already uses for the same quantity and is named where it is applied.  Every
float32 reference is asserted to lie within a quarter of the tolerance the GPU is held to of the float64 one (the test_*_admitted
tests: gradients of every leg, values, normals, colours, the material frames), with two exceptions the references name
themselves: the one ray of 65 whose float32 and float64 marches part (resolved_rays) and the three pixels of 1120 and one of the
two shader frames (admitted_pixels).  Libraries come from __graft_entry__.build() through gpu_test_programs() and
build_row_libraries().

Mutation evidence (libraries of wide, wide_rows and narrow_rows built from a scratch copy of csrc/rm_device.h with one value-only
edit of user_end_bwd each, never committed; MI355X):

1. the gd[i] it stores scaled by 1.001: test_stand_alone_kernels_on_the_lds_tape fails for both scenes at the first count (point
   gradient of scene(points), n = 1: 8.3e-5 from both references under a bound of 1e-5) and all six two-camera cases of
   test_frame_gradients_against_cpu_autograd fail (1.1e-4 to 2.9e-4 under 1e-4: a sphere's radius, the mirrored torus's
   translation, the camera's orientation);
2. theta.flush skipped: the same eight tests fail on the smooth subtraction's ``blend``, whose whole gradient is missing
   (scene(points), n = 63: 0.123 under 1e-4; frames: 0.0287, 8.2e-4, 0.0223 and 2.2e-3 under 1e-4).

The wall pose sees neither (no ray of it ends on the carved body), and scene(points) on the cube of
tests/test_standalone_backward.py alone does not see the second: hence standalone_points().
"""
import contextlib
import copy
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import sdf_oracle as O
from tests import helpers as H
from tests import test_user_warp as W
from tests.helpers import environment
from tests.test_deferred_backward import Gradients, matches_cpu, same_to_summation_order
from tests.test_user_combinator import UMin
from tests.test_user_leaf import USphere
from tests.test_user_warp import UAffine

DEV = "cuda"
IDENT, Q_ROT = [1.0, 0.0, 0.0, 0.0], [0.9014, 0.25, 0.25, 0.25]
ROWS_ENV = dict(RM_STATIC_BACKWARD_ACC="400")
MISSING = "specialised library missing: __graft_entry__.build() makes it"


def _register():
    from tests import test_user_combinator, test_user_leaf
    test_user_leaf._register()
    test_user_combinator._register()
    W._register()


# --------------------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------------------
def wide(extra=0, material=False):
    """Room, a smoothly carved intersection of a six-child smooth union (one child a scaled, mirrored, placed torus) with a box, a
    placed SDFLink and an elongated torus; ``extra`` placed boxes more; ``material``: SDFMaterial around the body and the cutter
    of the smooth subtraction and around the link."""
    from ray_marching_amd.contrib import (SDFElongate, SDFIntersection, SDFLink, SDFMaterial, SDFMirror, SDFScale,
                                          SDFSmoothSubtraction)
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFSmoothUnion, SDFUnion
    paint = (lambda sdf, albedo: SDFMaterial(sdf, albedo=albedo)) if material else (lambda sdf, albedo: sdf)
    blob = [A(SDFSphere(0.2 + 0.02 * i), orientation=IDENT, translation=[-0.8 + 0.35 * i, 0.1 * i, 0.0]) for i in range(5)]
    blob.append(SDFScale(SDFMirror(A(SDFTorus(0.3, 0.08), orientation=IDENT, translation=[0.5, 0.0, 0.3]), origin=0.1), scale=1.3))
    body = SDFIntersection([SDFSmoothUnion(blob, blend_k=22.0), SDFBox(BODY_BOX)])
    cutter = A(SDFSphere(0.4), orientation=IDENT, translation=[0.0, 0.6, -0.3])
    carved = SDFSmoothSubtraction([paint(body, (0.9, 0.2, 0.1)), paint(cutter, (0.1, 0.3, 0.9))], blend=0.1)
    link = paint(A(SDFLink(0.3, 0.2, 0.06), orientation=IDENT, translation=[-1.2, -0.8, 0.5]), (0.2, 0.8, 0.3))
    more = [A(SDFBox(EXTRA_BOX), orientation=EXTRA_Q, translation=[EXTRA_AT[0], EXTRA_AT[1] + 0.5 * i, EXTRA_AT[2]]) for i in range(extra)]
    return SDFUnion([make_room(), carved, link, SDFElongate(SDFTorus(0.3, 0.08), halfsides=(0.05, 0.02, 0.2))] + more)


# (with half-sides of 1.6 the box of the intersection cuts nothing and its float64 gradient is exactly zero)
BODY_BOX = (0.9, 0.9, 0.9)
EXTRA_BOX, EXTRA_Q, EXTRA_AT = (0.12, 0.12, 0.12), Q_ROT, (1.7, -0.9, 0.8)


def narrow_rows():
    """Register tape, accumulator rows: fewer than 17 slots -- a root union of two, the room's onion, a smooth union of seven and
    its value, the scale's value slot, the smooth subtraction's 2 x 2 -- and more than 96 accumulators, most of them in nested
    affine frames, which cost parameters and no slot.  The combinator has a parameter of its own (``blend``), so that
    UserTheta::flush adds into an accumulator row here as well."""
    from ray_marching_amd.contrib import SDFElongate, SDFLink, SDFMirror, SDFScale, SDFSmoothSubtraction
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFSmoothUnion, SDFUnion
    twice = lambda sdf, t: A(A(sdf, orientation=Q_ROT, translation=[0.05, -0.05, 0.1]), orientation=IDENT, translation=t)
    kids = [A(SDFScale(SDFSphere(0.25), scale=1.6), orientation=IDENT, translation=[-0.7, 0.3, 0.0]),
            A(SDFLink(0.3, 0.25, 0.08), orientation=Q_ROT, translation=[0.5, -0.3, 0.2]),
            A(SDFElongate(SDFTorus(0.3, 0.1), halfsides=(0.2, 0.05, 0.1)), orientation=IDENT, translation=[0.0, 0.6, -0.2]),
            SDFMirror(A(SDFSphere(0.3), orientation=IDENT, translation=[0.9, -0.6, 0.1]), origin=0.05),
            twice(SDFBox((0.25, 0.2, 0.3)), [-0.3, -0.5, 0.2]),
            twice(SDFTorus(0.3, 0.1), [0.2, 0.1, 0.5]),
            twice(SDFBox((0.2, 0.3, 0.15)), [-0.9, -0.3, -0.2])]
    cutter = A(SDFSphere(0.35), orientation=IDENT, translation=NARROW_CUTTER)
    return SDFUnion([make_room(), SDFSmoothSubtraction([SDFSmoothUnion(kids, blend_k=10.0), cutter], blend=0.1)])


NARROW_CUTTER = [-0.5, 0.1, -0.35]


def twin_builtin(pad=0):
    """Room, a smooth union of seven placed primitives (two of them onion shells: seven bare primitives give the scene 15 slots,
    the shells make it 17) and a hard union of three; ``pad`` of the seven get one more affine frame around them."""
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFOnion, SDFSmoothUnion, SDFUnion
    from ray_marching_amd.scene.scene_registry import make_room
    prims = [SDFSphere(0.3), SDFOnion(SDFSphere(0.35), radius=0.05), SDFBox((0.2, 0.3, 0.25)), SDFSphere(0.25),
             SDFOnion(SDFBox((0.3, 0.2, 0.2)), radius=0.04), SDFTorus(0.3, 0.1), SDFSphere(0.2)]
    placed = [A(p, orientation=Q_ROT if i % 2 else IDENT, translation=[-0.9 + 0.33 * i, 0.25 * ((i % 3) - 1), 0.1 * i])
              for i, p in enumerate(prims)]
    placed = [A(p, orientation=Q_ROT, translation=[0.02 * i, 0.03, -0.02]) if i < pad else p for i, p in enumerate(placed)]
    three = SDFUnion([A(SDFSphere(0.4), orientation=IDENT, translation=[-1.3, -0.9, 0.6]), SDFTorus(1.6, 0.1),
                      A(SDFBox((0.2, 0.2, 0.2)), orientation=Q_ROT, translation=[1.2, 0.9, 0.4])])
    return SDFUnion([make_room(), SDFSmoothUnion(placed, blend_k=14.0), three])


def restated(module):
    """A deep copy of a scene of built-in nodes with every SDFAffineTransformation replaced by UAffine, every SDFSphere by USphere
    and every SDFUnion by UMin (parameter names and order are kept)."""
    from ray_marching_amd.scene.primitives import SDFSphere
    from ray_marching_amd.scene.transformations import SDFAffineTransformation, SDFUnion

    def swap(m):
        for name, child in list(m._modules.items()):
            m._modules[name] = swap(child)
        if isinstance(m, SDFAffineTransformation):
            return UAffine(m.sdf, m.orientation.detach().tolist(), m.translation.detach().tolist())
        if isinstance(m, SDFSphere):
            return USphere(float(m.radius.detach()))
        if isinstance(m, SDFUnion):
            return UMin(list(m.sdfs))
        return m

    return swap(copy.deepcopy(module))


TWIN_PAD = 4
CULL_OFF = dict(RM_CULL="0")


def _ao():
    from tests.test_user_shader_probes import ambient_occlusion
    return ambient_occlusion()


def _marched():
    from tests.test_user_shader_chained_probes import marched_shadow
    return marched_shadow()


def _lambert():
    from tests.test_materials import lambert
    return lambert()


# name -> (scene, shader or None, environment of compile_scene and of every launch, LDS tape, accumulator rows)
PROGRAMS = {
    "wide": (wide, None, {}, True, False),
    "wide_rows": (lambda: wide(3), None, ROWS_ENV, True, True),
    "narrow_rows": (narrow_rows, None, ROWS_ENV, False, True),
    "twin_builtin": (twin_builtin, None, CULL_OFF, True, False),
    "twin_user": (lambda: restated(twin_builtin()), None, CULL_OFF, True, False),
    "twin_builtin_rows": (lambda: twin_builtin(TWIN_PAD), None, {**CULL_OFF, **ROWS_ENV}, True, True),
    "twin_user_rows": (lambda: restated(twin_builtin(TWIN_PAD)), None, {**CULL_OFF, **ROWS_ENV}, True, True),
    "wide_ao": (wide, _ao, {}, True, False),
    "wide_marched": (wide, _marched, {}, True, False),
    "wide_material": (lambda: wide(material=True), None, {}, True, False),
    "wide_material_lambert": (lambda: wide(material=True), _lambert, {}, True, False),
    "wide_rows_material": (lambda: wide(3, material=True), None, ROWS_ENV, True, True),
    "wide_rows_material_lambert": (lambda: wide(3, material=True), _lambert, ROWS_ENV, True, True),
}


def scene_of(name):
    _register()
    return PROGRAMS[name][0]()


def env_of(name):
    return PROGRAMS[name][2]


@functools.lru_cache(maxsize=None)
def compiled(name):
    from ray_marching_amd.compiler import compile_scene
    make, shader, env = PROGRAMS[name][:3]
    _register()
    with environment(**env):
        return compile_scene(make(), shader()) if shader is not None else compile_scene(make())


def rows_programs():
    return [name for name in PROGRAMS if PROGRAMS[name][4]]


def gpu_test_programs():
    """The programs of the GPU legs whose libraries do not depend on the environment at build time: build() compiles them in its
    pool.  The accumulator-row ones are build_row_libraries()'s."""
    from ray_marching_amd import specialize
    out = [compiled(name) for name in PROGRAMS if name not in rows_programs()]
    return list({specialize.scene_hash(cs): cs for cs in out}.values())


def build_row_libraries():
    """hipcc the libraries of the accumulator-row programs (at once where they exist).  specialize.build reads
    RM_STATIC_BACKWARD_ACC when it runs -- the "|bwd" of the library key and the backward kernels themselves depend on it -- so
    they are built here, under that environment, and not in a pool that runs without it.  -> their paths."""
    from concurrent.futures import ThreadPoolExecutor
    from ray_marching_amd import specialize
    with environment(**ROWS_ENV), ThreadPoolExecutor(max_workers=4) as ex:
        return list(ex.map(specialize.build, [compiled(name) for name in rows_programs()]))


def library_path(name):
    from ray_marching_amd import specialize
    with environment(**env_of(name)):
        return specialize.lib_path(compiled(name))


# --------------------------------------------------------------------------------------------------------------
# the CPU side
# --------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def with_user_leaves():
    """tests/test_user_warp.py's spec_of / cpu_eval / cpu_parameters know warps and combinators and assert on a user leaf: inside
    this context they know one more kind, ("leaf", a copy of the instance with fresh parameters), evaluated by the instance's
    own forward.  Their recursion goes through that module's own names, so a leaf deep in a tree is reached only by putting the
    three wrappers there for the length of the context (restored on the way out; the references are built in one thread); the
    alternative is a second copy of cpu_eval's eleven kinds here."""
    from ray_marching_amd.extensions import leaf_spec
    spec_of, cpu_eval, cpu_parameters = W.spec_of, W.cpu_eval, W.cpu_parameters

    def spec_of_(module, dtype=torch.float32):
        if leaf_spec(module) is None:
            return spec_of(module, dtype)
        inst = copy.copy(module)
        inst._parameters = {k: nn.Parameter(v.detach().clone().to(dtype)) for k, v in module._parameters.items()}
        return ("leaf", inst)

    W.spec_of = spec_of_
    W.cpu_eval = lambda spec, p: spec[1].forward(p) if spec[0] == "leaf" else cpu_eval(spec, p)
    W.cpu_parameters = lambda spec: list(spec[1].parameters()) if spec[0] == "leaf" else cpu_parameters(spec)
    try:
        yield
    finally:
        W.spec_of, W.cpu_eval, W.cpu_parameters = spec_of, cpu_eval, cpu_parameters


H_, W_, STEPS = 20, 28, 24            # partial 8 x 8 tiles on both edges
FRONT = ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, -3.0))
NEAR = ((0.98, 0.05, -0.12, 0.03), (0.3, -0.2, -2.2))
POSES = (FRONT, NEAR)
# The shader and the material legs look from elsewhere: the pose gradients of the probing shaders are sums over a few silhouette
# pixels that float32 and float64 resolve differently, and from POSES the two references are 4.6e-5 apart where a quarter of the
# tolerance is 2.5e-5; the material legs want at least 40 pixels on which two materials blend (27 from POSES) and a float32 frame
# within 0.25e-5 of the float64 one (9.4e-6 from NEAR: one silhouette pixel).
SHADER_POSES = (((0.995, 0.03, -0.08, 0.02), (0.2, -0.1, -2.6)), ((0.995, 0.03, -0.08, 0.02), (0.15, -0.05, -2.9)))
MATERIAL_POSES = (((1.0, 0.0, 0.0, 0.0), (0.2, 0.2, -1.8)), ((1.0, -0.055, -0.101, -0.018), (0.01, -0.08, -1.82)))
PARAM_TOL = 1e-4                      # matches_cpu (tests/test_deferred_backward.py): scene parameters 1e-4, pose 1e-4 max(1, scale)


def pose_tensors(poses, dtype=torch.float32):
    from tests.test_deferred_backward import pose_tensors as fp32
    q, t = fp32(poses)
    return q.to(dtype), t.to(dtype)


def frame_loss(image, n):
    """loss_of of tests/test_deferred_backward.py for the whole frame, in the image's dtype."""
    from tests.test_deferred_backward import frame_weights
    return (image * frame_weights(n, H_, W_).to(device=image.device, dtype=image.dtype)).sum() / (n * H_ * W_ * 3)


@functools.lru_cache(maxsize=None)
def frame_reference(name, poses, mode, dtype=torch.float32):
    """CPU autograd through the oracle's render (cpu_eval as its distance function) of the 20 x 28 x 24 frame of ``poses``.
    -> (image, Gradients), cached: callers must not modify it."""
    module = scene_of(name)
    names = [k for k, _ in module.named_parameters()]
    n = len(poses)
    bufs = tuple(b.to(dtype) for b in O.camera_buffers(n, W_, H_, H.PX * H_, H.PX * W_, H.PX * H_))
    q, t = (x.requires_grad_(True) for x in pose_tensors(poses, dtype))
    with with_user_leaves(), pytest.MonkeyPatch.context() as patch:
        spec = W.spec_of(module, dtype)
        params = W.cpu_parameters(spec)
        image = W.cpu_render(spec, patch, bufs, q, t, mode, 1, STEPS, H.EPS)
    assert len(params) == len(names), (name, len(params), names)
    frame_loss(image, n).backward()
    grads = {k: (torch.zeros_like(x) if x.grad is None else x.grad).detach() for k, x in zip(names, params)}
    return image.detach(), Gradients(grads, q.grad.detach(), t.grad.detach())


def user_parameter_names(module):
    """named_parameters() of the user-defined nodes of a scene (leaves, combinators, warps) and of its material nodes."""
    from ray_marching_amd.extensions import user_spec
    out = []
    for path, node in module.named_modules():
        if user_spec(node) is not None or getattr(node, "_rm_kind", None) == "material":
            out += [f"{path}.{k}" if path else k for k, _ in node.named_parameters(recurse=False)]
    return out


# one camera 0.3 above the floor (CLOSED_POSE's orientation): rays that creep along it and never settle; 101 (mode 0) and 7
# (mode 4) of its 560 rays are offered to the deferred-ray list, 183 to 461 of the 1120 of POSES
WALL = (((0.98, 0.05, -0.12, 0.03), (0.2, -4.6, -2.5)),)


@functools.lru_cache(maxsize=None)
def shader_reference(which, dtype=torch.float32):
    """``wide`` under AmbientOcclusionShader ("wide_ao", 5 probes) or MarchedShadowShader ("wide_marched", chained, 8 probes): the
    shader files' cpu_frame, loss and weights at this file's frame and SHADER_POSES.  -> (image, shader gradients by name, Gradients)."""
    from tests import test_user_shader_probes as P
    module, shader = scene_of(which), PROGRAMS[which][1]().to(dtype)
    names = [k for k, _ in module.named_parameters()]
    n = len(SHADER_POSES)
    q, t = (x.requires_grad_(True) for x in pose_tensors(SHADER_POSES, dtype))
    mp = pytest.MonkeyPatch()
    try:
        with with_user_leaves():
            spec = W.spec_of(module, dtype)
            params = W.cpu_parameters(spec)
            image = P.cpu_frame(spec, shader, mp, tuple(b.to(dtype) for b in P._bufs(n, H_, W_)), q, t, STEPS, sdf_eval=W.cpu_eval)
    finally:
        mp.undo()
    P._loss(image, P._weights(n, H_, W_, 7).to(dtype)).backward()
    grads = {k: (torch.zeros_like(x) if x.grad is None else x.grad).detach() for k, x in zip(names, params)}
    own = {k: p.grad.detach().clone() for k, p in P._trainable(shader)}
    return image.detach(), own, Gradients(grads, q.grad.detach(), t.grad.detach())


@functools.lru_cache(maxsize=None)
def material_reference(which, dtype=torch.float32):
    """tests/test_materials.py's frame_reference for ``wide_material_lambert`` / ``wide_rows_material_lambert`` at this file's frame
    and MATERIAL_POSES.  -> (image, blend weights [N, H, W, J], gradients by name: the scene's parameters, "shader.ambient", "orientation",
    "translation")."""
    from tests import test_materials as M
    from tests.test_user_shader import _bufs, _weights, cpu_frame
    scene, shader = scene_of(which).to(dtype), PROGRAMS[which][1]().to(dtype)
    q, t = (x.requires_grad_(True) for x in pose_tensors(MATERIAL_POSES, dtype))
    n = len(MATERIAL_POSES)
    wrapped = M._WithMaterial(scene, shader)
    mp = pytest.MonkeyPatch()
    try:
        image = cpu_frame(scene, wrapped, mp, tuple(b.to(dtype) for b in _bufs(n, H_, W_)), q, t, STEPS,
                          sdf_eval=lambda s, p: M.ref_eval(s, p, []))
    finally:
        mp.undo()
    M._frame_loss(image, _weights(n, H_, W_, 7).to(dtype)).backward()
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad).detach() for k, p in scene.named_parameters()}
    grads["shader.ambient"] = shader.ambient.grad.detach()
    grads["orientation"], grads["translation"] = q.grad.detach(), t.grad.detach()
    return image.detach(), wrapped.weights, grads


ALBEDO_COUNTS = (65, 257)


@functools.lru_cache(maxsize=None)
def albedo_reference(which):
    """tests/test_materials.py's point_reference for this file's material scenes, at the 257 points every count takes its first n
    of: 200 of the usual cube and 57 in a shell of 0.3 to 0.5 around the centre of the cutter (radius 0.4), where its weight and the
    body's blend."""
    from tests import test_materials as M
    scene = scene_of(which)
    shell = torch.nn.functional.normalize(H._points(57, seed=12, lo=-1.0, hi=1.0), dim=-1) * (0.3 + 0.2 * torch.rand(57, 1, generator=torch.Generator().manual_seed(14)))
    pts = torch.cat([H._points(200, seed=11), shell + torch.tensor([0.0, 0.6, -0.3])])[torch.randperm(257, generator=torch.Generator().manual_seed(13))]
    w = torch.rand(257, 3, generator=torch.Generator().manual_seed(5)) + 0.5
    out = {}
    for dtype in (torch.float32, torch.float64):
        a, albedos = M.ref_weights(copy.deepcopy(scene).to(dtype), pts.to(dtype))
        out[dtype] = (a, albedos, M.ref_colour(a, albedos).detach())
    return scene, pts, w, out


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
USER_OPS = ("OP_USER", "OP_USER_FOLD", "OP_USER_END", "OP_USER_PUSH", "OP_USER_POP")


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_every_program_is_in_its_regime(name):
    """The storage each library is compiled with (StaticCfg): the tape by n_slots against RM_LDS_TAPE_MIN_SLOTS = 17, the
    accumulators by n_params + n_grad_derived against 96 -- and, above it, a backward at all only under the environment
    variable.  Every user opcode is in the program (the built-in twins: none), a USER_POP with a value slot wherever a warp
    with an `out` was put (UAffine, the twins' only warp, has none), RM_OP_MATERIAL in the material scenes; and
    rm_validate_program accepts it."""
    from ray_marching_amd import _abi, specialize
    cs = compiled(name)
    lds_tape, rows = PROGRAMS[name][3:]
    acc = cs.n_params + cs.n_grad_derived
    print(f"{name}: {cs.n_instr} instructions, {cs.n_params} parameters, {acc} accumulators, {cs.n_slots} slots")
    assert (cs.n_slots >= 17) == lds_tape and cs.n_slots < 64
    assert (acc > specialize.MAX_STATIC_BACKWARD_ACC) == rows
    assert specialize.static_backward(cs) == (not rows)
    with environment(**env_of(name)):
        assert specialize.static_backward(cs)
    ops = cs.program[:, 0].tolist()
    for op in USER_OPS:
        assert (getattr(_abi, op) in ops) == (not name.startswith("twin_builtin")), (name, op)
    pops = cs.program[cs.program[:, 0] == _abi.OP_USER_POP]
    assert bool(((pops[:, 3] & 65535) > 0).any()) == (not name.startswith("twin")), name
    assert (_abi.OP_MATERIAL in ops) == ("material" in name)
    if name.startswith("twin"):
        assert _abi.OP_CULL_MIN not in ops and _abi.OP_CULL_LSE not in ops
    assert cs.n_instr <= 80
    prog = np.ascontiguousarray(cs.program)
    assert _abi.lib.rm_validate_program(prog.ctypes.data, prog.shape[0], cs.n_params, cs.n_derived, cs.stack_floats, cs.n_slots) == 0, \
        _abi.lib.rm_last_error().decode()


def test_the_twins_are_restatements():
    """twin_user is twin_builtin with 7 -> 22, 8 -> 23 (UAffine), 1 -> 19 (USphere) and the hard unions as UMin: the same parameter
    names in the same order with the same values, no built-in union, affine frame or sphere left."""
    from ray_marching_amd import _abi
    for a, b in (("twin_builtin", "twin_user"), ("twin_builtin_rows", "twin_user_rows")):
        builtin, user = scene_of(a), scene_of(b)
        assert [k for k, _ in builtin.named_parameters()] == [k for k, _ in user.named_parameters()]
        assert all(torch.equal(x, y) for x, y in zip(builtin.parameters(), user.parameters()))
        ops = compiled(b).program[:, 0].tolist()
        for op in (_abi.OP_SPHERE, _abi.OP_AFFINE_PUSH, _abi.OP_AFFINE_POP, _abi.OP_FOLD_MIN):
            assert op not in ops, (b, op)
        assert compiled(a).n_params == compiled(b).n_params and compiled(a).leaf_names == compiled(b).leaf_names


def test_the_stripped_material_scenes_are_wide_and_wide_rows():
    """contrib.strip_materials of the two material scenes compiles to the programs of ``wide`` and ``wide_rows``: the library a
    built-in mode's frame of the material scene is compared with, bit for bit, is one of this file's own."""
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.contrib import strip_materials
    for painted, bare in (("wide_material", "wide"), ("wide_rows_material", "wide_rows")):
        assert compile_scene(strip_materials(scene_of(painted))).signature == compiled(bare).signature
        assert compiled(painted).n_params == compiled(bare).n_params + 9


def test_every_library_was_built():
    """build() leaves every library of this file behind (gpu_test_programs, build_row_libraries), the accumulator-row ones under
    their "|bwd" key."""
    from ray_marching_amd import specialize
    assert len(PROGRAMS) == 13
    paths = {name: library_path(name) for name in PROGRAMS}
    assert len(set(paths.values())) == len(PROGRAMS)
    for name in rows_programs():
        assert paths[name] != specialize.lib_path(compiled(name)), name       # the forward-only key is another one
    for name, path in paths.items():
        assert os.path.isfile(path), f"{name}: {MISSING}"


def frame_cases():
    return [(name, poses, mode) for name in ("wide", "wide_rows", "narrow_rows") for poses in (POSES, WALL) for mode in (0, 4)]


def admitted_pixels(i32, i64, tol=1e-5):
    """[N, H, W] bool: the pixels of a float32 reference frame that lie within a quarter of ``tol`` of the float64 frame in every
    channel.  The reference names the pixels it cannot vouch for (DESIGN.md 10 does the same for the config-5 fixture)."""
    return (i32.double() - i64.double()).abs().amax(dim=-1) <= 0.25 * tol


def admit(what, g32, g64, tol, relative):
    """|g32 - g64| <= tol / 4 (``relative``: of max(1, max|g64|)) and equal NaN patterns.  -> the share of the quarter used."""
    a, b = g32.double(), g64.double()
    assert torch.equal(a.isnan(), b.isnan()), what
    fin = ~b.isnan()
    if not bool(fin.any()):
        return 0.0
    bound = 0.25 * tol * (max(1.0, float(b[fin].abs().max())) if relative else 1.0)
    err = float((a - b)[fin].abs().max())
    print(f"{what}: |g32 - g64| {err:.3g}, a quarter of the tolerance {bound:.3g}")
    assert err <= bound, (what, err, bound)
    return err / bound


@pytest.mark.parametrize("name,poses,mode", frame_cases(), ids=[f"{c[0]}-{'wall' if c[1] is WALL else 'two'}-mode{c[2]}" for c in frame_cases()])
def test_references_are_admitted(name, poses, mode):
    """Every (scene, pose, mode) of the frame leg: no NaN pixel in the float32 frame, and the float32 gradients -- the reference
    matches_cpu holds the GPU to -- within a quarter of matches_cpu's bounds of the float64 ones."""
    i32, g32 = frame_reference(name, poses, mode, torch.float32)
    i64, g64 = frame_reference(name, poses, mode, torch.float64)
    assert not bool(i32.isnan().any()) and not bool(i64.isnan().any())
    for (k, a), (_, b) in zip(g32.items(), g64.items()):
        admit(f"{name} mode {mode} {k}", a, b, PARAM_TOL, relative=k in ("orientation", "translation"))


@pytest.mark.parametrize("which", ["wide_ao", "wide_marched"])
def test_shader_references_are_admitted(which):
    """The shader legs hold every gradient to 1e-4 (tests/test_user_shader_probes.py) or max(1e-4, 4 E_ref)
    (tests/test_user_shader_chained_probes.py): E_ref = |g32 - g64| is at most a quarter of 1e-4 for every tensor, so both
    bounds are 1e-4 here.  The frame, held to 1e-5: no NaN pixel, and the pixels whose float32 value is further than a quarter of
    that from the float64 one (admitted_pixels: three of 1120 and one, on silhouettes) are at most 1 % of the frame -- the share
    H.fast_frame_rule allows beyond its threshold.  None of 70 poses tried brought both shaders' whole frames within 0.25e-5."""
    i32, s32, g32 = shader_reference(which, torch.float32)
    i64, s64, g64 = shader_reference(which, torch.float64)
    ok = admitted_pixels(i32, i64)
    print(f"{which}: fp32 vs fp64 frame diff {float((i32.double() - i64).abs().max()):.3g}, {int((~ok).sum())} of {ok.numel()} pixels not admitted")
    assert not bool(i32.isnan().any()) and float((~ok).double().mean()) <= 0.01
    for k in s32:
        admit(f"{which} shader.{k}", s32[k], s64[k], 1e-4, relative=False)
    for (k, a), (_, b) in zip(g32.items(), g64.items()):
        admit(f"{which} {k}", a, b, 1e-4, relative=False)


@pytest.mark.parametrize("which", ["wide_material_lambert", "wide_rows_material_lambert"])
def test_material_references_are_admitted(which):
    """H.gradient_contract takes the nearer of the float32 and the float64 reference under 1e-4 max(1, max|g64|): the two are
    within a quarter of that of each other; no NaN pixel; the float32 frame within a quarter of the 1e-5 the GPU's is held to of
    the float64 frame, at every pixel; and at least 40 pixels blend two materials with weights above 0.02 (the condition of
    test_the_frame_reference_alone of tests/test_materials.py)."""
    i32, a32, g32 = material_reference(which, torch.float32)
    i64, a64, g64 = material_reference(which, torch.float64)
    share = a64 / a64.sum(dim=-1, keepdim=True)
    blended = int(((share > 0.02).sum(dim=-1) >= 2).sum())
    diff = float((i32.double() - i64).abs().max())
    print(f"{which}: fp32 vs fp64 colour diff {diff:.3g}, blended pixels {blended}")
    assert not bool(i32.isnan().any()) and diff <= 0.25e-5 and blended >= 40
    for k in g32:
        admit(f"{which} {k}", g32[k], g64[k], 1e-4, relative=True)


@pytest.mark.parametrize("which", ["wide_material", "wide_rows_material"])
def test_albedo_references_are_admitted(which):
    """The points of the surface_albedo leg: at least 10 of the 257 (and one of the first 65) blend two materials with weights
    above 0.02; the float32 colours within a quarter of the 1e-5 they hold the GPU to of the float64 ones; the albedo gradients
    of the two within a quarter of H.gradient_contract's 1e-4 max(1, max|g64|)."""
    from tests import test_materials as M
    _, pts, w, ref = albedo_reference(which)
    (a32, albedos, c32), (a64, _, c64) = ref[torch.float32], ref[torch.float64]
    share = a64 / a64.sum(dim=-1, keepdim=True).clamp(min=1e-30)
    blended = (share > 0.02).sum(dim=-1) >= 2
    diff = float((c32.double() - c64).abs().max())
    print(f"{which}: {int(blended.sum())} blended points ({int(blended[:65].sum())} among the first 65), colour diff {diff:.3g}")
    assert int(blended.sum()) >= 10 and int(blended[:65].sum()) >= 1 and diff <= 0.25e-5
    assert sum(c is not None for c in albedos) == 3
    for n in ALBEDO_COUNTS:
        for j, (a, b) in enumerate(zip(M.albedo_gradients(a32[:n], albedos, w[:n]), M.albedo_gradients(a64[:n], albedos, w[:n]))):
            admit(f"{which} n={n} albedo {j}", a, b, 1e-4, relative=True)
            assert float(b.abs().max()) >= 1e-3, (which, n, j)


def test_every_user_parameter_is_visible():
    """Every parameter of a user node, of a user shader and every albedo has a float64 gradient of at least ten times the absolute
    tolerance it is held to (1e-4) in at least one case of its scene: a dropped term shows."""
    best = {}
    for name, poses, mode in frame_cases():
        _, g = frame_reference(name, poses, mode, torch.float64)
        for k in user_parameter_names(scene_of(name)):
            best[name, k] = max(best.get((name, k), 0.0), float(g.params[k].abs().max()))
    for which in ("wide_ao", "wide_marched"):
        for k, g in shader_reference(which, torch.float64)[1].items():
            best[which, "shader." + k] = float(g.abs().max())
    for which in ("wide_material_lambert", "wide_rows_material_lambert"):
        g = material_reference(which, torch.float64)[2]
        for k in user_parameter_names(scene_of(which)) + ["shader.ambient"]:
            best[which, k] = float(g[k].abs().max())
    for key, value in best.items():
        print(f"largest float64 gradient of {key[0]} {key[1]}: {value:.3g}")
    assert len(best) > 30
    small = {key: value for key, value in best.items() if value < 1e-3}
    assert not small, small


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
FIGURES = {}      # leg -> [largest error, the rule it was held to (the legs assert it, per comparison), what]


def note(leg, err, rule, what):
    if leg not in FIGURES or err > FIGURES[leg][0]:
        FIGURES[leg] = [err, rule, what]


@contextlib.contextmanager
def launching(name):
    """The environment the program was compiled under -- the library key depends on it -- and no compiler at run time: a library
    that build() did not leave behind is an error, not a build."""
    with environment(RM_SPECIALIZE="prebuilt", **env_of(name)):
        yield


def device_scene(name):
    """-> (a fresh scene on the device, its shader or None); both kinds of kernels come from the program's own library."""
    from ray_marching_amd import _abi
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    scene = scene_of(name).to(DEV)
    shader = PROGRAMS[name][1]().to(DEV) if PROGRAMS[name][1] is not None else None
    cs = compiled_for(scene) if shader is None else compiled_with_shader(scene, shader)
    assert os.path.isfile(library_path(name)), f"{name}: {MISSING}"
    for backward in (False, True):
        assert cs.lib(backward) is not _abi.lib, f"{name}: {MISSING}"
    return scene, shader


def clear_grads(*modules):
    for m in modules:
        for p in m.parameters():
            p.grad = None


def run_backward(name, poses, mode, capacity, shader_loss=None):
    """run_backward of tests/test_deferred_backward.py for this file's programs: one backward of the 20 x 28 x 24 frame with a
    deferred-ray list of ``capacity`` rays (None: default sizing, 0: every ray walked in place).  -> Gradients with work[32]."""
    from ray_marching_amd import ops
    from tests.test_deferred_backward import colormap
    n = len(poses)
    with launching(name), pytest.MonkeyPatch.context() as knobs:
        scene, _ = device_scene(name)
        loop = H.make_loop(scene, H_, W_, n=n)
        if mode in (6, 7):
            loop.shader.cyclic_cmap = colormap().to(DEV)
        q, t = (x.to(DEV).requires_grad_(True) for x in pose_tensors(poses))
        tiles = int(ops._lib.rm_wave_tiles(n, H_, W_, ops.default_flags(True, True, True)))
        knobs.setattr(ops, "bwd_hard_capacity", capacity)
        knobs.setattr(ops, "bwd_tile_cost_sink", torch.zeros(tiles, dtype=torch.int32, device=DEV))      # keeps the workspace
        frame_loss(loop(q, t, mode, 1, STEPS), n).backward()
        work = ops.bwd_last_work.cpu()
    grads = {k: x.grad.detach().float().cpu() for k, x in scene.named_parameters()}
    return Gradients(grads, q.grad.float().cpu(), t.grad.float().cpu(), int(work[32]), int(work[33]))


# ---- 1. exact twins
@pytest.mark.gpu
@pytest.mark.parametrize("rows", [False, True], ids=["register_accumulators", "accumulator_rows"])
def test_restated_twin_is_bit_identical_with_the_builtin(rows):
    """Zero tolerance on everything that is a function of the program: twin_user restates twin_builtin's nodes (UAffine, USphere,
    UMin), on an LDS tape of 23 slots against one of 17, so scene(points) at 257 points and its gradients, the frames of all
    eight modes through the tile kernel, without the early-out and through the ray pools, a rows=(5, 17) band and a float16
    module agree in every bit.  The frame gradients of modes 0, 4 and 6 run with the deferred-ray list at its default size and
    follow same_to_summation_order's rule (2e-6 max(1, max|g|), equal NaN patterns)."""
    user, builtin = ("twin_user_rows", "twin_builtin_rows") if rows else ("twin_user", "twin_builtin")
    pts = H._points(257, seed=11)
    q, t = (x.to(DEV) for x in pose_tensors(POSES))

    def everything(name):
        out = dict(frames=[], grads={})
        with launching(name):
            scene, _ = device_scene(name)
            p = pts.to(DEV).requires_grad_(True)
            d = scene(p)
            d.sum().backward()
            out.update(d=d.detach(), gp=p.grad, gw=[x.grad.clone() for x in scene.parameters()])
            for kw in (dict(), dict(early_out=False), dict(regen=True)):
                loop = H.make_loop(scene, H_, W_, n=2, **kw)
                with torch.no_grad():
                    out["frames"] += [loop(q, t, mode, 2, STEPS) for mode in range(8)]
            with torch.no_grad():
                out["frames"] += [H.make_loop(scene, H_, W_, n=2)(q, t, mode, 1, STEPS, rows=(5, 17)) for mode in (0, 4)]
        for mode in (0, 4, 6):
            out["grads"][mode] = run_backward(name, POSES, mode, None)
        with launching(name), torch.no_grad():
            half = H.make_loop(scene, H_, W_, n=2).to(torch.float16)
            out["half"] = [half(q.half(), t.half(), mode, 1, STEPS) for mode in (0, 4)]
        return out

    got, want = everything(user), everything(builtin)
    assert H._same(got["d"], want["d"]) and H._same(got["gp"], want["gp"])
    assert float(want["gp"].abs().max()) > 0.5
    for i, (a, b) in enumerate(zip(got["gw"], want["gw"])):
        assert H._same(a, b), ("scene(points) parameter gradient", i)
    assert len(got["frames"]) == 26
    for i, (a, b) in enumerate(zip(got["frames"], want["frames"])):
        assert a.shape == b.shape and H._same(a, b), ("frame", i)
    for i, (a, b) in enumerate(zip(got["half"], want["half"])):
        assert a.dtype == torch.float16 and H._same(a, b), ("float16 frame", i)
    assert float(want["frames"][0].max()) > 0.1
    for mode in (0, 4, 6):
        a, b = got["grads"][mode], want["grads"][mode]
        assert list(a.params) == list(b.params)            # (the restatement keeps names and order)
        worst = same_to_summation_order(a, b, f"{user} vs {builtin} mode {mode}")
        note(f"1. twins ({'rows' if rows else 'registers'}): frame gradients", worst, "2e-6 max(1, max|g|) per tensor", f"mode {mode}")


# ---- 2. stand-alone kernels
POINT_COUNTS = (1, 63, 64, 65, 255, 256, 257)


def cpu_both(name, inputs, forward, upstreams):
    """both_references of tests/test_standalone_backward.py over this file's scenes: autograd through ``forward(spec, *inputs)``
    with cpu_eval as the oracle's sdf_eval, in float32 and float64.  -> ((outputs, input gradients, [(name, gradient)]), ...)"""
    out = []
    for dtype in (torch.float32, torch.float64):
        module = scene_of(name)
        names = [k for k, _ in module.named_parameters()]
        xs = [x.detach().to(dtype).clone().requires_grad_(True) for x in inputs]
        with with_user_leaves(), pytest.MonkeyPatch.context() as patch:
            spec = W.spec_of(module, dtype)
            params = W.cpu_parameters(spec)
            patch.setattr(O, "sdf_eval", W.cpu_eval)
            outs = forward(spec, *xs)
        sum((o * u.to(dtype)).sum() for o, u in zip(outs, upstreams) if u is not None).backward()
        grad = lambda x: x.grad if x.grad is not None else torch.zeros_like(x)
        out.append(([o.detach() for o in outs], [grad(x) for x in xs], [(k, grad(p)) for k, p in zip(names, params)]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def standalone_points():
    """seeded_points() of tests/test_standalone_backward.py (the cube [-3, 3]^3 and its upstream weights), every fourth point moved
    into a shell of 0.3 to 0.5 around the centre of the cutter of ``wide`` (radius 0.4): in the cube alone the smooth
    subtraction's ``blend`` takes no gradient, and a combinator that dropped its own parameters' gradients would pass."""
    from tests import test_standalone_backward as S
    pts, w = (x[:257].clone() for x in S.seeded_points())
    gen = torch.Generator().manual_seed(14)
    shell = torch.nn.functional.normalize(torch.randn(65, 3, generator=gen), dim=-1) * (0.3 + 0.2 * torch.rand(65, 1, generator=gen))
    pts[::4] = shell + torch.tensor([0.0, 0.6, -0.3])
    return pts, w


def standalone_cases():
    return [("points", n) for n in POINT_COUNTS] + [("march", 65), ("normals", 65)]


@functools.lru_cache(maxsize=None)
def standalone_case(name, kind, n):
    """One case of the stand-alone leg, computed once: (inputs, upstreams, both references of cpu_both).  "points": the first n of
    standalone_points(); "march": the 65 rays of a 5 x 13 camera at FRONT, STEPS steps; "normals": the float32 CPU march's final
    points with the jitter and the upstreams of surface_points() of tests/test_standalone_backward.py."""
    import math
    from tests import test_standalone_backward as S
    if kind == "points":
        inputs, ups = [standalone_points()[0][:n]], [standalone_points()[1][:n]]
        forward = lambda s, p: (O.sdf_eval(s, p),)
    elif kind == "march":
        pos, dirs = S.camera_rays(5, 13, FRONT[1])
        assert pos.shape == (n, 3)
        inputs, ups = [pos, dirs], [S.march_weights(n)]
        forward = lambda s, p, v: (O.march(s, p, v, STEPS),)
    else:
        hit = standalone_case(name, "march", n)[2][0][0][0]
        assert bool(torch.isfinite(hit).all())
        gen = torch.Generator().manual_seed(13)
        shrink = min(1.0, 2.0 ** math.floor(math.log2(4.0 / math.sqrt(n))))
        inputs = [hit + 1e-2 * torch.randn(n, 3, generator=gen)]
        ups = [shrink * torch.randn(n, 3, generator=gen), shrink * 1e-3 * torch.randn(n, 1, generator=gen)]
        forward = lambda s, p: O.normals(s, p, H.EPS)
    return inputs, ups, cpu_both(name, inputs, forward, ups)


def resolved_rays(refs):
    """The rays whose float32 CPU march ends within a quarter of 1e-5 of the float64 one: the others' final points are the
    reference's own disagreement (a ray grazing a blend crease takes another turn), as in
    test_carved_scene_against_cpu_autograd_and_the_stand_alone_modules."""
    return (refs[0][0][0].double() - refs[1][0][0]).abs().max(dim=-1).values <= 0.25e-5


@pytest.mark.parametrize("kind,n", standalone_cases(), ids=[f"{k}-{n}" for k, n in standalone_cases()])
@pytest.mark.parametrize("name", ["wide", "wide_rows"])
def test_stand_alone_references_are_admitted(name, kind, n):
    """The references of the stand-alone leg: float32 values and normals within a quarter of the 1e-5 the GPU's are held to of the
    float64 ones (final positions: on the resolved rays, all but a few); every gradient within a quarter of
    H.gradient_contract's bound -- 1e-5 absolute for the point gradients of scene(points), 1e-4 max(1, max|g64|) otherwise."""
    _, _, ((o32, i32, p32), (o64, i64, p64)) = standalone_case(name, kind, n)
    if kind == "march":
        ok = resolved_rays(((o32,), (o64,)))
        print(f"{name} march: {int(ok.sum())} of {n} rays resolved")
        assert int((~ok).sum()) <= 3
    else:
        admit(f"{name} {kind} n={n} values", o32[0], o64[0], 1e-5, relative=False)
    for a, b in zip(i32, i64):
        admit(f"{name} {kind} n={n} input gradient", a, b, 1e-5 if kind == "points" else 1e-4, relative=kind != "points")
    for (k, a), (_, b) in zip(p32, p64):
        admit(f"{name} {kind} n={n} {k}", a, b, 1e-4, relative=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wide", "wide_rows"])
def test_stand_alone_kernels_on_the_lds_tape(name):
    """scene(points) forward and backward at counts around every wave and block edge, then SDFMarcher (early-out on and off) and
    SDFNormals backward at 65 rays / points, against cpu_eval in float32 and float64: the contract of
    tests/test_standalone_backward.py (H.gradient_contract: the nearer reference, 1e-4 max(1, max|g64|); point gradients of
    scene(points) 1e-5 absolute).  Values, final positions and normals within 1e-5 of the float32 reference (the bound of
    test_carved_scene_against_cpu_autograd_and_the_stand_alone_modules; positions: on the resolved rays)."""
    from ray_marching_amd.rendering.ray_marching import SDFNormals
    from tests import test_standalone_backward as S
    group = f"wide storage {name}"
    with launching(name):
        scene, _ = device_scene(name)
        for n in POINT_COUNTS:
            (pts,), (w,), refs = standalone_case(name, "points", n)
            dev = S.dev_grads(scene, [pts], lambda p: (scene(p),), [w])
            err = float((dev[0][0].detach().cpu() - refs[0][0][0]).abs().max())
            print(f"{name} n={n}: values max|err| {err:.3g}")
            assert dev[0][0].shape == (n, 1) and err <= 1e-5
            note(f"2. stand-alone ({name}): values", err, "1e-5", f"n={n}")
            S.check_gradients(group, f"{name} scene(points) n={n}", dev, refs, ["grad_points"], tol_inputs=1e-5, absolute_inputs=True)
        (pos, dirs), (w,), refs = standalone_case(name, "march", 65)
        resolved = resolved_rays(refs)
        for early in (True, False):
            out, gp, gv, gpar, nexec = S.dev_march(scene, pos, dirs, STEPS, w, early)
            err = float((out.detach().cpu() - refs[0][0][0])[resolved].abs().max())
            print(f"{name} march early_out={early}: positions max|err| {err:.3g} on {int(resolved.sum())} of 65 rays")
            assert out.shape == (65, 3) and err <= 1e-5
            note(f"2. stand-alone ({name}): values", err, "1e-5", f"march early_out={early}")
            S.check_gradients(group, f"{name} march early_out={early}", ([out], [gp, gv], gpar), refs, ["grad_pos", "grad_dirs"])
        (pts,), (wn, wl), refs = standalone_case(name, "normals", 65)
        normals = SDFNormals(scene, H.EPS).to(DEV)
        dev = S.dev_grads(scene, [pts], lambda p: normals(p), [wn, wl])
        err = float((dev[0][0].detach().cpu() - refs[0][0][0]).abs().max())
        print(f"{name} normals: max|err| {err:.3g}")
        assert err <= 1e-5
        note(f"2. stand-alone ({name}): values", err, "1e-5", "normals")
        S.check_gradients(group, f"{name} normals", dev, refs, ["grad_points"])
    for kind in ("inputs", "parameters"):
        (e32, w32), (e64, w64), _ = H.STANDALONE_WORST[f"{group} {kind}"]
        print(f"wide storage [2. stand-alone ({name}): gradients, {kind}]: worst |got - g32| {e32:.3g} ({w32}), worst |got - g64| "
              f"{e64:.3g} ({w64}); per tensor the nearer reference is held to 1e-4 max(1, max|g64|) (point gradients of scene(points): 1e-5)")


# ---- 3. frames
@pytest.mark.gpu
@pytest.mark.parametrize("name,poses,mode", frame_cases(), ids=[f"{c[0]}-{'wall' if c[1] is WALL else 'two'}-mode{c[2]}" for c in frame_cases()])
def test_frame_gradients_against_cpu_autograd(name, poses, mode):
    """The fused backward (k_render_bwd and, with the list, the deferred-ray kernels behind it) of the 20 x 28 x 24 frame: once with
    the deferred-ray list at its default size, once with every ray walked in place.  The two agree by same_to_summation_order
    and each satisfies matches_cpu (parameters 1e-4, pose 1e-4 max(1, scale)) against CPU autograd; every case offers rays to
    the list (work[32] > 0), the in-place walk none."""
    what = f"{name} {'wall' if poses is WALL else 'two cameras'} mode {mode}"
    want = frame_reference(name, poses, mode)[1]
    listed = run_backward(name, poses, mode, None)
    in_place = run_backward(name, poses, mode, 0)
    print(f"{what}: {listed.offered} rays offered to the list, {listed.pairs} (ray, step) pairs")
    assert in_place.offered == 0 and in_place.pairs == 0
    assert listed.offered > 0, f"{what}: no ray was deferred"
    d = same_to_summation_order(listed, in_place, what)
    e = max(matches_cpu(listed, want, mode, what), matches_cpu(in_place, want, mode, what + " in place"))
    note(f"3. frames ({name}): list vs in place", d, "2e-6 max(1, max|g|) per tensor", what)
    note(f"3. frames ({name}): vs CPU autograd", e, "parameters 1e-4, pose 1e-4 max(1, max|g|)", what)


# ---- 4. user shaders
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["wide_ao", "wide_marched"])
def test_probing_shaders_on_the_lds_tape(which, monkeypatch):
    """AmbientOcclusionShader (5 probes: five more scene evaluations per pixel) and MarchedShadowShader (8 chained probes: two
    sliding windows) over the 21-slot tape of ``wide``: the frame within 1e-5 of the CPU's (restated math mode: host
    independent; on the admitted pixels, which is what counts, and -- as the sibling files ask -- on every other one too) and the ray pools' frame equal to the tile kernel's in every bit; the gradients of the shader's parameters,
    the scene's and the pose within 1e-4 (tests/test_user_shader_probes.py), the marched shadow's within max(1e-4, 4 E_ref)
    (tests/test_user_shader_chained_probes.py)."""
    from ray_marching_amd import ops
    from tests import test_user_shader_probes as P
    _, s32, g32 = shader_reference(which, torch.float32)
    _, s64, g64 = shader_reference(which, torch.float64)
    q, t = pose_tensors(SHADER_POSES)
    with with_user_leaves(), torch.no_grad(), O.math_mode("restated"):
        want = P.cpu_frame(W.spec_of(scene_of(which)), PROGRAMS[which][1](), monkeypatch, P._bufs(2, H_, W_), q, t, STEPS, sdf_eval=W.cpu_eval)
    with launching(which):
        scene, shader = device_scene(which)
        with torch.no_grad():
            tile = H.make_loop(scene, H_, W_, n=2)(q.to(DEV), t.to(DEV), shader, 1, STEPS)
            pools = H.make_loop(scene, H_, W_, n=2, regen=True)(q.to(DEV), t.to(DEV), shader, 1, STEPS)
        err, frac = H.report(f"{which} frame", tile.cpu(), want)
        ok = admitted_pixels(shader_reference(which, torch.float32)[0], shader_reference(which, torch.float64)[0])
        err_ok = float((tile.cpu() - want)[ok].abs().max())
        print(f"{which}: frame max|err| {err:.3g} ({err_ok:.3g} on the {int(ok.sum())} admitted pixels), {frac:.3g} of the values beyond 1e-5")
        assert tile.shape == (2, H_, W_, 3) and err_ok <= 1e-5 and err <= 1e-5
        assert H._same(pools, tile)
        note(f"4. shaders ({which}): frame", err, "1e-5", which)
        qg, tg = q.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
        sink = torch.zeros(int(ops._lib.rm_wave_tiles(2, H_, W_, 2)), dtype=torch.int32, device=DEV)
        monkeypatch.setattr(ops, "bwd_tile_cost_sink", sink)          # (measurement hook: keeps the backward's workspace)
        P._loss(H.make_loop(scene, H_, W_, n=2)(qg, tg, shader, 1, STEPS), P._weights(2, H_, W_, 7).to(DEV)).backward()
        torch.cuda.synchronize()
        print(f"{which}: {int(ops.bwd_last_work[32])} rays deferred")
        monkeypatch.setattr(ops, "bwd_tile_cost_sink", None)
    got = [(f"shader.{k}", p.grad.cpu(), s32[k], s64[k]) for k, p in P._trainable(shader)]
    got += [(k, p.grad.cpu(), g32.params[k], g64.params[k]) for k, p in scene.named_parameters()]
    got += [("orientations", qg.grad.cpu(), g32.gq, g64.gq), ("translations", tg.grad.cpu(), g32.gt, g64.gt)]
    bad = []
    for k, g, c32, c64 in got:
        assert bool(torch.isfinite(g).all()), k
        e_ref = float((c32.double() - c64).abs().max())
        bound = 1e-4 if which == "wide_ao" else max(1e-4, 4 * e_ref)
        e = float((g - c32).abs().max())
        print(f"{which}: grad {k} max|err| {e:.3g}, E_ref {e_ref:.3g}, bound {bound:.3g} (|g| {float(c32.abs().max()):.3g})")
        note(f"4. shaders ({which}): gradients", e, "1e-4" if which == "wide_ao" else "max(1e-4, 4 E_ref)", k)
        if not e <= bound:
            bad.append(k)
    assert not bad, (which, bad)


# ---- 5. materials
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["wide_material", "wide_rows_material"])
def test_materials_on_the_lds_tape(which, monkeypatch):
    """The material colour's two sweeps over one tape (kMatColour, kMatGrad) where the tape is in LDS, and -- wide_rows_material --
    where the sweep's albedo gradients go through the accumulator rows; one of the three materials is the body of the
    SDFSmoothSubtraction, so that combinator's VJP feeds the blend weights.  contrib.surface_albedo at 65 and 257 points and
    MaterialLambertShader frames and gradients against tests/test_materials.py's reference, with its bounds (colours and frames
    1e-5, gradients H.gradient_contract); two backwards of one frame with the list off give every gradient the same bits; modes
    0 and 4 render the stripped scene -- ``wide`` / ``wide_rows`` -- bit for bit and leave the albedos a zero gradient."""
    from ray_marching_amd import ops
    from ray_marching_amd.compiler import compiled_for
    from ray_marching_amd.contrib import SDFMaterial, surface_albedo
    from tests import test_materials as M
    from tests.test_user_shader import _weights
    group = f"wide storage {which}"
    # ---- surface_albedo at points
    _, pts, w, ref = albedo_reference(which)
    a32, albedos, c32 = ref[torch.float32]
    a64, _, c64 = ref[torch.float64]
    share = a64 / a64.sum(dim=-1, keepdim=True).clamp(min=1e-30)
    assert int(((share > 0.02).sum(dim=-1) >= 2).sum()) >= 10          # points where two materials blend
    with launching(which):
        scene, _ = device_scene(which)
        for n in ALBEDO_COUNTS:
            clear_grads(scene)
            got = surface_albedo(scene, pts[:n].to(DEV))
            err = float((got.detach().cpu() - c32[:n]).abs().max())
            print(f"{which} n={n}: max |colour - float32 reference| {err:.3g}")
            assert got.shape == (n, 3) and got.dtype == torch.float32 and err <= 1e-5
            note(f"5. materials ({which}): colours", err, "1e-5", f"n={n}")
            (got * w[:n].to(DEV)).sum().backward()
            cs = compiled_for(scene)
            order = [cs.leaves[i] for i, _ in cs.albedo_leaves]
            g32, g64 = M.albedo_gradients(a32[:n], albedos, w[:n]), M.albedo_gradients(a64[:n], albedos, w[:n])
            assert len(order) == len(g32) == 3 == sum(isinstance(m, SDFMaterial) for m in scene.modules())
            for j, (p, a, b) in enumerate(zip(order, g32, g64)):
                H.gradient_contract(group, f"{which} n={n} albedo {j}", p.grad, a, b)
            ids = {id(p) for p in order}
            assert all(p.grad is None for p in scene.parameters() if id(p) not in ids)
    # ---- frames under MaterialLambertShader
    lambert = which + "_lambert"
    want, _, g32 = material_reference(lambert, torch.float32)
    _, _, g64 = material_reference(lambert, torch.float64)
    q, t = pose_tensors(MATERIAL_POSES)

    def backward(scene, shader, capacity):
        clear_grads(scene, shader)
        qg, tg = q.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
        sink = torch.zeros(int(ops._lib.rm_wave_tiles(2, H_, W_, 2)), dtype=torch.int32, device=DEV)
        with monkeypatch.context() as knobs:
            knobs.setattr(ops, "bwd_hard_capacity", capacity)
            knobs.setattr(ops, "bwd_tile_cost_sink", sink)          # (measurement hook: keeps the backward's workspace)
            M._frame_loss(H.make_loop(scene, H_, W_, n=2)(qg, tg, shader, 1, STEPS), _weights(2, H_, W_, 7).to(DEV)).backward()
            torch.cuda.synchronize()
            deferred = int(ops.bwd_last_work[32])
        return qg.grad, tg.grad, deferred

    with launching(lambert):
        scene, shader = device_scene(lambert)
        with torch.no_grad():
            for kw in (dict(), dict(regen=True)):
                got = H.make_loop(scene, H_, W_, n=2, **kw)(q.to(DEV), t.to(DEV), shader, 1, STEPS).cpu()
                err = float((got - want).abs().max())
                print(f"{lambert} {kw}: frame max|err| {err:.3g}")
                assert got.shape == (2, H_, W_, 3) and err <= 1e-5
                note(f"5. materials ({which}): frames", err, "1e-5", str(kw))
        gq, gt, deferred = backward(scene, shader, None)
        print(f"{lambert}: {deferred} rays deferred")
        for k, p in scene.named_parameters():
            H.gradient_contract(group, f"{lambert} {k}", p.grad, g32[k], g64[k])
        H.gradient_contract(group, f"{lambert} ambient", shader.ambient.grad, g32["shader.ambient"], g64["shader.ambient"])
        H.gradient_contract(group, f"{lambert} orientation", gq, g32["orientation"], g64["orientation"])
        H.gradient_contract(group, f"{lambert} translation", gt, g32["translation"], g64["translation"])
        runs = []
        for _ in range(2):
            gq, gt, deferred = backward(scene, shader, 0)
            assert deferred == 0
            runs.append({**{k: p.grad.clone() for k, p in scene.named_parameters()}, "ambient": shader.ambient.grad.clone(), "q": gq, "t": gt})
        differ = [k for k in runs[0] if not H._same(runs[0][k], runs[1][k])]
        print(f"{lambert}: gradients whose bits differ between two backwards with the list off: {differ or 'none'}")
        assert not differ, differ
    (e32, w32), (e64, w64), _ = H.STANDALONE_WORST[group]
    print(f"wide storage [5. materials ({which}): gradients]: worst |got - g32| {e32:.3g} ({w32}), worst |got - g64| {e64:.3g} ({w64}); "
          f"per tensor the nearer reference is held to 1e-4 max(1, max|g64|)")
    # ---- built-in modes: the stripped scene, bit for bit
    stripped = "wide_rows" if "rows" in which else "wide"
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)
    for mode in (0, 4):
        out = []
        for name in (which, stripped):
            with launching(name):
                s, _ = device_scene(name)
                qg, tg = q.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
                image = H.make_loop(s, H_, W_, n=2)(qg, tg, mode, 1, STEPS)
                M._frame_loss(image, _weights(2, H_, W_, 7).to(DEV)).backward()
                out.append((image.detach(), qg.grad, tg.grad, s))
        for a, b in zip(out[0][:3], out[1][:3]):
            assert H._same(a, b), (which, mode)
        kept = [p for k, p in out[0][3].named_parameters() if not k.endswith("albedo")]
        bare = list(out[1][3].named_parameters())
        assert len(kept) == len(bare) and float(out[0][1].abs().max()) > 0
        for p, (k, b) in zip(kept, bare):
            assert H._same(p.grad, b.grad), (which, mode, k)
        for k, p in out[0][3].named_parameters():
            if k.endswith("albedo"):
                assert torch.equal(p.grad, torch.zeros(3, device=DEV)), k


# ---- 6. summary
@pytest.mark.gpu
def test_zz_worst_figures():
    """Per leg, the largest error seen and the rule its comparisons were held to.  Printed only: each leg has asserted its own
    bounds, per tensor, and several of them scale with the gradient."""
    for leg in sorted(FIGURES):
        err, rule, what = FIGURES[leg]
        print(f"wide storage [{leg}]: largest error {err:.3g}, held to {rule} ({what})")
    assert FIGURES, "run the whole file: the legs fill the table"
