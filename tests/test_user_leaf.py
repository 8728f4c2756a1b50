"""User-defined SDF leaves (ray_marching_amd/extensions.py): registration, the RM_OP_USER program, the specialised
libraries that carry the leaves' HIP source, and -- on the GPU -- parity of such scenes with built-in twins, with
culling on and off, with CPU autograd through the leaf's own PyTorch forward, and through a captured training loop.

The CPU side of every GPU comparison is `composition()` below: torch.minimum of the oracle's evaluation of the
built-in part and the leaf's own forward at the affine-transformed point.  test_link_in_the_reference_combinators
pins that composition, bit for bit, to the same SDFLink instance inside the reference's own SDFUnion /
SDFAffineTransformation.
"""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import ref_bridge, sdf_oracle as O
from tests import helpers as H
from tests.helpers import _points, _pose, _same, environment

DEV = "cuda"


# --------------------------------------------------------------------------------------------------------------
# test-defined leaves
# --------------------------------------------------------------------------------------------------------------
class USphere(nn.Module):
    """SDFSphere restated as a user leaf: the op stream of the built-in handler, so everything must agree bit for bit."""

    def __init__(self, radius: float):
        super().__init__()
        self.radius = nn.Parameter(torch.tensor(radius, dtype=torch.float32))

    def forward(self, query_positions):
        return torch.linalg.vector_norm(query_positions, dim=-1, keepdim=True) - self.radius


USPHERE_HIP = """
template <bool Fast> RM_DEV float usphere_fwd(rm::V3 p, const float* theta) { return norm3_t<Fast>(p) - theta[0]; }
template <bool Fast> RM_DEV void usphere_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) {
  const float n = norm3_t<Fast>(p);
  const float s = (n == 0.0f) ? 0.0f : div_t<Fast>(g, n);
  gp = gp + mk3(p.x * s, p.y * s, p.z * s);
  gtheta[0] = -g;
}
"""


class UPill(nn.Module):
    """A capsule along y (half height, radius): the leaf type that is only ever compiled at test time."""

    def __init__(self, half_height: float, radius: float):
        super().__init__()
        self.half_height = nn.Parameter(torch.tensor(half_height, dtype=torch.float32))
        self.radius = nn.Parameter(torch.tensor(radius, dtype=torch.float32))

    def forward(self, query_positions):
        y = query_positions[..., [1]]
        q = torch.cat([query_positions[..., [0]], y - torch.clamp(y, min=-self.half_height, max=self.half_height),
                       query_positions[..., [2]]], dim=-1)
        return torch.linalg.vector_norm(q, dim=-1, keepdim=True) - self.radius


UPILL_HIP = """
template <bool Fast> RM_DEV float upill_fwd(rm::V3 p, const float* theta) {
  return norm3_t<Fast>(mk3(p.x, p.y - t_clamp(p.y, -theta[0], theta[0]), p.z)) - theta[1];
}
template <bool Fast> RM_DEV void upill_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) {
  const float qy = p.y - t_clamp(p.y, -theta[0], theta[0]);
  const float n = norm3_t<Fast>(mk3(p.x, qy, p.z));
  const float s = (n == 0.0f) ? 0.0f : div_t<Fast>(g, n);
  const float side = (p.y > theta[0]) ? 1.0f : ((p.y < -theta[0]) ? -1.0f : 0.0f);
  gp = gp + mk3(p.x * s, (side != 0.0f) ? qy * s : 0.0f, p.z * s);
  gtheta[0] = -qy * s * side;
  gtheta[1] = -g;
}
"""


def _register():
    from ray_marching_amd.extensions import register_leaf
    register_leaf(USphere, params=("radius",), hip=USPHERE_HIP, cost=13)
    register_leaf(UPill, params=("half_height", "radius"), hip=UPILL_HIP, cost=20)


# --------------------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------------------
LINK = dict(length=0.35, radius1=0.3, radius2=0.08)
LINK_T, LINK_Q = [-0.6, 0.1, 0.2], [0.9014, 0.25, 0.25, 0.25]


def builtin_part_spec(dtype=torch.float32):
    """The built-in part of contrib.make_link_scene(): the room and the sphere of 0.5 moved to x = 0.9."""
    sphere = ("affine", {"translation": O._t((0.9, 0.0, 0.0), dtype), "orientation": O._t((1.0, 0.0, 0.0, 0.0), dtype)},
              ("sphere", {"radius": O._t(0.5, dtype)}))
    return ("union", {}, [O.scene_room(dtype), sphere])


def composition(spec, link, t, q, p):
    """min(built-in part, link at the affine-transformed point): what the GPU tests compare the link scene against."""
    return torch.minimum(O.sdf_eval(spec, p), link.forward(O.quat_rotate(p - t, O.quat_conj(q))))


def scene2_with(sphere_cls):
    from ray_marching_amd.scene.primitives import SDFLine, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFUnion
    return SDFUnion([make_room(), SDFUnion(sdfs=[sphere_cls(0.5), SDFTorus(radius1=1.0, radius2=0.25),
                                                 SDFLine(start=(1.0, 0.0, 0.0), end=(-1.0, 0.0, 0.0), radius=0.1)])])


def closed_scene_with(sphere_cls):
    from ray_marching_amd.scene.primitives import SDFBox, SDFLine, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFOnion, SDFSmoothUnion, SDFUnion
    inner = SDFSmoothUnion(sdfs=[
        A(SDFOnion(SDFBox(halfsides=(0.1, 0.2, 0.05)), radius=0.1), orientation=[0.9014, 0.25, 0.25, 0.25], translation=[0.0, 0.25, 0.25]),
        A(sphere_cls(0.5), orientation=[1.0, 0.0, 0.0, 0.0], translation=[0.0, 0.0, 1.0]),
        SDFLine(start=(-1.0, 1.0, 2.0), end=(1.0, 1.0, 0.0), radius=0.1),
        A(SDFTorus(radius1=0.5, radius2=0.1), orientation=[0.0, 0.5 ** 0.5, 0.5 ** 0.5, 0.0], translation=[0.0, 0.5, 1.0]),
    ], blend_k=22.0)
    return SDFUnion([inner, make_room()])


def link_among_cullable_siblings():
    """Culling leg 1: the link as a sibling of children that get a CULL_MIN each under RM_CULL_MIN_COST=0."""
    from ray_marching_amd.contrib import SDFLink
    from ray_marching_amd.scene.primitives import SDFLine, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    return SDFUnion([
        make_room(),
        A(SDFTorus(radius1=0.5, radius2=0.12), orientation=[0.0, 0.5 ** 0.5, 0.5 ** 0.5, 0.0], translation=[1.1, 0.4, 0.5]),
        A(SDFLink(**LINK), orientation=LINK_Q, translation=LINK_T),
        A(SDFSphere(0.4), orientation=[1.0, 0.0, 0.0, 0.0], translation=[0.2, -0.9, 0.8]),
        SDFLine(start=(-1.5, 1.0, 1.0), end=(-0.5, 1.2, 0.4), radius=0.1),
    ])


def link_inside_a_blob():
    """Culling leg 2: the link as one of 8 children of a smooth union that sits under a min-union next to the room."""
    from ray_marching_amd.contrib import SDFLink
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFSmoothUnion, SDFUnion
    g = torch.Generator().manual_seed(77)
    t = (torch.rand(8, 3, generator=g) * 5.0 - 2.5).tolist()
    q = torch.nn.functional.normalize(torch.randn(8, 4, generator=g), dim=-1).tolist()
    # (the link shares its child with a much smaller sphere walked before it: a bound left over from that sphere would
    # be far too tight for the child)
    pair = SDFUnion([SDFSphere(0.1), A(SDFLink(**LINK), orientation=LINK_Q, translation=[0.3, 0.0, 0.0])])
    prims = [SDFSphere(0.3), SDFBox((0.2, 0.3, 0.15)), SDFTorus(0.4, 0.1), pair,
             SDFSphere(0.25), SDFBox((0.3, 0.1, 0.2)), SDFTorus(0.35, 0.08), SDFSphere(0.35)]
    return SDFUnion([make_room(), SDFSmoothUnion([A(p, orientation=q[i], translation=t[i]) for i, p in enumerate(prims)], blend_k=22.0)])


TIGHT_END = (0.9, 1.18, 0.0)      # the far end of the long link of link_with_a_tight_neighbour(), on its surface


def link_with_a_tight_neighbour():
    """Culling leg 3, built so that a wrong bound for the link SHOWS: a stiff smooth union (k = 300: a child is skipped
    from 0.35 behind the nearest one) in which the link shares its child with a tiny sphere walked before it, and a
    second tiny sphere sits 0.12 off the link's far end.  A bound table entry that repeated the tiny sphere's bound for
    the link (0.5 around (0.45, 0, 0) for the pair; the link reaches 1.26 from there) would skip the pair for waves at that
    end, where the link is the surface: the value would jump from ~0 to the neighbour's 0.07."""
    from ray_marching_amd.contrib import SDFLink
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFSmoothUnion, SDFUnion
    ident = [1.0, 0.0, 0.0, 0.0]
    pair = SDFUnion([SDFSphere(0.05), A(SDFLink(0.8, 0.3, 0.08), orientation=ident, translation=[0.9, 0.0, 0.0])])
    far = [A(SDFSphere(0.3), orientation=ident, translation=[-2.0, -1.5, 1.0]), A(SDFBox((0.2, 0.3, 0.15)), orientation=LINK_Q, translation=[2.0, -1.0, 0.5]),
           A(SDFTorus(0.4, 0.1), orientation=LINK_Q, translation=[-1.5, 1.5, -1.0]), A(SDFSphere(0.25), orientation=ident, translation=[0.0, -2.0, -1.5]),
           A(SDFBox((0.3, 0.1, 0.2)), orientation=ident, translation=[2.2, 1.8, 1.5]), A(SDFTorus(0.35, 0.08), orientation=ident, translation=[-2.2, 0.0, 2.0])]
    neighbour = A(SDFSphere(0.05), orientation=ident, translation=[TIGHT_END[0], TIGHT_END[1] + 0.12, TIGHT_END[2]])
    return SDFUnion([make_room(), SDFSmoothUnion([pair, neighbour] + far, blend_k=300.0)])


def two_links_and_a_usphere():
    """CPU leg: two instances of one leaf type and a second, test-defined type."""
    from ray_marching_amd.contrib import SDFLink
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFOnion, SDFRounding, SDFUnion
    return SDFUnion([make_room(),
                     A(SDFLink(**LINK), orientation=LINK_Q, translation=LINK_T),
                     SDFRounding(USphere(0.4), 0.05),
                     SDFOnion(A(SDFLink(0.2, 0.25, 0.05), orientation=[1.0, 0.0, 0.0, 0.0], translation=[0.5, 0.5, 0.0]), 0.02)])


CULL_ENVS = {"siblings": [dict(RM_CULL_MIN_COST="0", RM_CULL="0"), dict(RM_CULL_MIN_COST="0")],
             "blob": [dict(RM_CULL="0"), dict(), dict(RM_CULL_LSE="1", RM_CULL_LSE_MIN="2")],
             "tight_neighbour": [dict(RM_CULL="0"), dict(), dict(RM_CULL_LSE="1", RM_CULL_LSE_MIN="2")]}
CULL_SCENES = {"siblings": link_among_cullable_siblings, "blob": link_inside_a_blob, "tight_neighbour": link_with_a_tight_neighbour}


def gpu_test_programs():
    """Every test-defined program the GPU legs launch (the JIT leg's excepted): the CPU suite builds their libraries,
    so that a GPU run of the same tree finds them; where they are missing the library builds itself on first use."""
    from ray_marching_amd.compiler import compile_scene
    _register()
    out = [compile_scene(scene2_with(USphere)), compile_scene(closed_scene_with(USphere))]
    for name, envs in CULL_ENVS.items():
        for env in envs:
            with environment(**env):
                out.append(compile_scene(CULL_SCENES[name]()))
    from ray_marching_amd import specialize
    return list({specialize.scene_hash(cs): cs for cs in out}.values())      # (the blob's default program is its RM_CULL=0 one)


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
def test_registration_errors():
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.extensions import leaf_spec, register_leaf
    _register()
    assert leaf_spec(USphere(0.3)).name == "usphere" and leaf_spec(nn.Linear(2, 2)) is None
    register_leaf(USphere, params=("radius",), hip=USPHERE_HIP, cost=13)                 # the same again: fine
    with pytest.raises(ValueError, match="already registered"):
        register_leaf(USphere, params=("radius",), hip=USPHERE_HIP.replace("- theta[0]", "- theta[0] - 0.0f"), cost=13)

    class Lone(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = nn.Parameter(torch.tensor(1.0)); self.b = nn.Parameter(torch.tensor(2.0)); self.c = nn.Parameter(torch.tensor(3.0))

        def forward(self, p):
            return p[..., :1]

    src = ("template <bool Fast> RM_DEV float NAME_fwd(rm::V3 p, const float* theta) { return p.x; }\n"
           "template <bool Fast> RM_DEV void NAME_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) { gp.x += g; }\n")
    with pytest.raises(ValueError, match="exactly two device functions"):
        register_leaf(Lone, params=(), hip=src.replace("NAME_vjp", "other_vjp").replace("NAME", "lone"), cost=1)
    with pytest.raises(ValueError, match="inline assembly"):
        register_leaf(Lone, params=(), hip=src.replace("NAME", "lone").replace("gp.x += g;", 'asm volatile(""); gp.x += g;'), cost=1)
    with pytest.raises(ValueError, match="already used"):
        register_leaf(Lone, params=(), hip=src.replace("NAME", "usphere"), cost=1)
    with pytest.raises(TypeError):
        register_leaf(dict, params=(), hip=src.replace("NAME", "lone"), cost=1)

    class Unknown(Lone):
        pass

    register_leaf(Unknown, params=("a", "nope"), hip=src.replace("NAME", "unknown_attr"), cost=1)
    with pytest.raises(ValueError, match="nope"):
        compile_scene(Unknown())

    class Gap(Lone):
        pass

    register_leaf(Gap, params=("a", "c"), hip=src.replace("NAME", "gap"), cost=1)          # b lies between them
    with pytest.raises(ValueError, match="not contiguous"):
        compile_scene(Gap())

    class Free(nn.Module):                                                                 # a leaf without parameters
        def forward(self, p):
            return p[..., :1]

    register_leaf(Free, params=(), hip=src.replace("NAME", "free_plane"), cost=1)
    cs = compile_scene(Free())
    assert cs.program.tolist() == [[19, 0, 0, 0]] and cs.user_leaves[0][:2] == ("free_plane", 0)
    # an unregistered foreign module keeps the closed-vocabulary error
    with pytest.raises(TypeError, match="is not a ray_marching_amd SDF node"):
        compile_scene(nn.Linear(3, 1))


def test_program_of_a_scene_with_two_leaf_types():
    import copy
    import hashlib
    import pickle
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import compile_scene
    _register()
    scene = two_links_and_a_usphere()
    cs = compile_scene(scene)
    rows = cs.program.reshape(-1, 4)
    user = rows[rows[:, 0] == _abi.OP_USER]
    offs = dict(zip(cs.leaf_names, cs.leaf_offsets))
    assert _abi.OP_USER == 19 and user.tolist() == [[19, offs["sdfs.1.sdf.length"], 0, 3],
                                                    [19, offs["sdfs.2.sdf.radius"], 1, 1],
                                                    [19, offs["sdfs.3.sdf.sdf.length"], 0, 3]]
    assert cs.user_leaves == (("link", 3, hashlib.sha1(contrib._LINK_HIP.encode()).hexdigest()),
                              ("usphere", 1, hashlib.sha1(USPHERE_HIP.encode()).hexdigest()))
    assert cs.signature[-1] == cs.user_leaves
    # never boundable: no cull test in front of a child that holds a user leaf, even when every child is asked for one
    with environment(RM_CULL_MIN_COST="0"):
        eager = compile_scene(two_links_and_a_usphere()).program.reshape(-1, 4)
    sites = np.flatnonzero(eager[:, 0] == _abi.OP_CULL_MIN)
    assert len(sites) == 1                                     # (the room: the only child without a user leaf)
    for i in sites:
        assert not (eager[i + 1:i + (eager[i, 3] >> 8), 0] == _abi.OP_USER).any()
    ok = lambda prog: _abi.lib.rm_validate_program(prog.ctypes.data, prog.shape[0], cs.n_params, cs.n_derived, cs.stack_floats, cs.n_slots)
    assert ok(cs.program) == 0
    bad = cs.program.copy()
    at = int(np.flatnonzero(bad[:, 0] == _abi.OP_USER)[-1])
    bad[at, 3] = cs.n_params                                   # aux1: more parameter floats than the block holds
    assert ok(bad) == -2 and b"user leaf" in _abi.lib.rm_last_error()
    bad[at, 3] = -1
    assert ok(bad) == -2
    # the source is part of the library key; pickle / deepcopy keep the scene whole
    hdr = specialize.code_header(cs)
    assert "#define RM_USER_LEAVES 2" in hdr and "link_fwd<Fast>" in hdr and "usphere_vjp<Fast>" in hdr
    cs2 = pickle.loads(pickle.dumps(cs))
    assert cs2.user_leaves == cs.user_leaves and specialize.code_header(cs2) == hdr and specialize.scene_hash(cs2) == specialize.scene_hash(cs)
    twin = compile_scene(copy.deepcopy(scene))
    assert twin.signature == cs.signature
    # CPU points run the class's own PyTorch forward (also as a child of a built-in node there is no CPU kernel path)
    p = _points(64)
    link = scene.sdfs[1].sdf
    assert torch.equal(link(p), contrib.SDFLink._rm_torch_forward(link, p)) and link(p).shape == (64, 1)


def test_specialised_library_cross_compiles_and_reports_its_leaves(monkeypatch, tmp_path):
    from concurrent.futures import ThreadPoolExecutor
    from ray_marching_amd import _abi, specialize
    from ray_marching_amd.compiler import compile_scene
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    _register()
    cs = compile_scene(two_links_and_a_usphere())
    # (one pool for this library and for those of the GPU legs: hipcc takes 15-40 s each)
    with ThreadPoolExecutor(max_workers=4) as ex:
        paths = list(ex.map(specialize.build, [cs] + gpu_test_programs()))
    assert all(os.path.isfile(p) for p in paths)
    monkeypatch.setenv("RM_SPECIALIZE", "prebuilt")
    specialize._loaded.clear()
    lib = cs.lib()
    assert lib is not _abi.lib and lib.rm_user_leaves() == 2 and lib.rm_abi_version() == 14 == _abi.ABI_VERSION
    assert cs.lib(True) is lib and cs.specialised
    assert _abi.lib.rm_user_leaves() == 0 and _abi.fast_lib().rm_user_leaves() == 0
    from ray_marching_amd.scene.scene_registry import make_test_scene2
    assert compile_scene(make_test_scene2()).lib().rm_user_leaves() == 0          # a specialised library of built-in nodes
    # the interpreter is never an option
    monkeypatch.setenv("RM_SPECIALIZE", "off")
    fresh = compile_scene(two_links_and_a_usphere())
    with pytest.raises(_abi.RmError, match="user-defined leaves"):
        fresh.lib()
    monkeypatch.setattr(specialize, "SPEC_DIR", str(tmp_path))
    monkeypatch.setenv("RM_SPECIALIZE", "prebuilt")
    specialize._loaded.clear()
    with pytest.raises(_abi.RmError, match="librm_spec_"):
        compile_scene(two_links_and_a_usphere()).lib()
    monkeypatch.setenv("RM_STATIC_BACKWARD_ACC", "8")
    with pytest.raises(_abi.RmError, match="RM_STATIC_BACKWARD_ACC"):
        compile_scene(two_links_and_a_usphere()).lib(True)
    monkeypatch.delenv("RM_STATIC_BACKWARD_ACC")
    # a leaf that does not compile: hipcc's own words reach the caller
    from ray_marching_amd.extensions import register_leaf

    class Broken(nn.Module):
        def forward(self, p):
            return p[..., :1]

    register_leaf(Broken, params=(), cost=1, hip=(
        "template <bool Fast> RM_DEV float broken_fwd(rm::V3 p, const float* theta) { return no_such_helper(p); }\n"
        "template <bool Fast> RM_DEV void broken_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) {}\n"))
    monkeypatch.setenv("RM_SPECIALIZE", "jit")
    with pytest.raises(_abi.RmError, match="no_such_helper"):
        compile_scene(Broken()).lib()
    specialize._loaded.clear()


@pytest.mark.skipif(not ref_bridge.reference_available(), reason="reference tree not present")
def test_link_in_the_reference_combinators():
    """The reference's combinators take any nn.Module: the same SDFLink instance, placed by ITS SDFAffineTransformation
    inside ITS SDFUnion, equals `composition()` bit for bit -- which is what the GPU legs compare the kernels with."""
    from ray_marching_amd.contrib import SDFLink
    ref = ref_bridge.load_reference()
    link = SDFLink(**LINK)
    spec = builtin_part_spec()
    scene = ref.tf.SDFUnion([ref_bridge.spec_to_reference(ref, spec),
                             ref.tf.SDFAffineTransformation(link, orientation=LINK_Q, translation=LINK_T)])
    p = _points(4096, seed=3)
    with torch.no_grad():
        want = scene(p)
        got = composition(spec, link, O._t(LINK_T), O._t(LINK_Q), p)
    assert want.shape == got.shape == (4096, 1) and torch.equal(want, got)
    with torch.no_grad():
        inside = int((link(O.quat_rotate(p - O._t(LINK_T), O.quat_conj(O._t(LINK_Q)))) == got).sum())
    assert 400 < inside < 3600, "the link decides the minimum on too few points for this test to mean anything"


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scene2", "closed_scene1"])
def test_restated_sphere_is_bit_identical_with_the_builtin(which, monkeypatch):
    """Zero tolerance: USphere restates SDFSphere's op stream, so a scene with it and its built-in twin agree in every
    bit of every value, point gradient and frame; parameter and pose gradients to summation order."""
    from ray_marching_amd.compiler import compiled_for
    from ray_marching_amd.scene.primitives import SDFSphere
    _register()
    make = scene2_with if which == "scene2" else closed_scene_with
    user, twin = make(USphere).to(DEV), make(SDFSphere).to(DEV)
    assert compiled_for(user).lib().rm_user_leaves() == 1 and compiled_for(twin).specialised
    assert [n for n, _ in user.named_parameters()] == [n for n, _ in twin.named_parameters()]
    pts = _points(4096, seed=11).to(DEV)
    res = {}
    for name, scene in (("user", user), ("twin", twin)):
        p = pts.clone().requires_grad_(True)
        d = scene(p)
        d.sum().backward()
        res[name] = (d.detach(), p.grad, [x.grad.clone() for x in scene.parameters()])
    assert torch.equal(res["user"][0], res["twin"][0]) and torch.equal(res["user"][1], res["twin"][1])
    for a, b in zip(res["user"][2], res["twin"][2]):
        assert (a - b).abs().max().item() <= 1e-5 * max(1.0, b.abs().max().item())
    h, w, steps = 40, 56, 24
    cams = [_pose(-3.0), (torch.nn.functional.normalize(torch.tensor([[1.0, 0.05, -0.1, 0.02]]), dim=-1).to(DEV),
                          torch.tensor([[0.3, -0.2, -2.0]], device=DEV))]
    for kw in (dict(), dict(early_out=False), dict(regen=True)):
        lu, lt = H.make_loop(user, h, w, **kw), H.make_loop(twin, h, w, **kw)
        for q, t in cams:
            for mode in range(8):
                with torch.no_grad():
                    assert _same(lu(q, t, mode, 2, steps), lt(q, t, mode, 2, steps)), (kw, mode)
    # two cameras in one batch
    lu, lt = H.make_loop(user, h, w, n=2), H.make_loop(twin, h, w, n=2)
    q2, t2 = torch.cat([c[0] for c in cams]), torch.cat([c[1] for c in cams])
    for mode in (0, 1, 4):
        with torch.no_grad():
            assert _same(lu(q2, t2, mode, 1, steps), lt(q2, t2, mode, 1, steps)), mode
    # Lambertian MSE step: parameter and pose gradients
    grads = {}
    for name, scene in (("user", user), ("twin", twin)):
        for x in scene.parameters():
            x.grad = None
        loop = H.make_loop(scene, 32, 32)
        q, t = _pose(-1.0 if which == "closed_scene1" else -3.0)
        q.requires_grad_(True); t.requires_grad_(True)
        loop(q, t, 0, 1, 16).pow(2).mean().backward()
        grads[name] = [x.grad.clone() for x in scene.parameters()] + [q.grad, t.grad]
    for a, b in zip(grads["user"], grads["twin"]):
        assert (a - b).abs().max().item() <= 1e-5 * max(1.0, b.abs().max().item())
    # one fp16 module (fp16 storage of buffers and parameters, fp32 arithmetic): cast last, it converts the scenes in place
    lu, lt = H.make_loop(user, h, w).to(torch.float16), H.make_loop(twin, h, w).to(torch.float16)
    q, t = cams[0][0].half(), cams[0][1].half()
    for mode in (0, 4):
        with torch.no_grad():
            a, b = lu(q, t, mode, 1, steps), lt(q, t, mode, 1, steps)
        assert a.dtype == torch.float16 and _same(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["siblings", "blob", "tight_neighbour"])
def test_culling_around_a_user_leaf_changes_no_bit(case, monkeypatch):
    """A user leaf has no bounding sphere.  Compiled without cull tests (RM_CULL=0) and with them -- `siblings`: a test in
    front of every boundable sibling of the link; `blob`: the link inside a smooth union of 8, by default and with the
    exact logsumexp culling, whose bound table has an entry per child: the link's must say "unbounded", not repeat the
    bound of the leaf walked before it (`tight_neighbour`: a scene in which that mistake changes values by 0.07: it is
    the case that fails when subtree_bound has no case for RM_OP_USER) -- values, gradients and frames are the same bits."""
    from ray_marching_amd import _abi, ops
    from ray_marching_amd.compiler import compiled_for
    _register()
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)      # bitwise parameter gradients: no atomically ordered deferred-ray list
    gen = torch.Generator().manual_seed(5)
    centres = (torch.rand(64, 1, 3, generator=gen) * 2 - 1) * 2.5
    if case == "tight_neighbour":      # half of the waves at the far end of the long link
        centres[:32] = torch.tensor(TIGHT_END) + 0.05 * (torch.rand(32, 1, 3, generator=gen) * 2 - 1)
    pts = (centres + (0.01 if case == "tight_neighbour" else 0.05) * torch.randn(64, 64, 3, generator=gen)).reshape(-1, 3).to(DEV)      # coherent waves: culls fire
    wts = torch.randn(pts.shape[0], 1, generator=gen).to(DEV)
    res = []
    for env in CULL_ENVS[case]:
        for k in ("RM_CULL", "RM_CULL_MIN_COST", "RM_CULL_LSE", "RM_CULL_LSE_MIN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        scene = CULL_SCENES[case]().to(DEV)
        cs = compiled_for(scene)
        ops_ = cs.program.reshape(-1, 4)[:, 0]
        n_cull = int(((ops_ == _abi.OP_CULL_MIN) | (ops_ == _abi.OP_CULL_LSE)).sum())
        assert cs.lib().rm_user_leaves() == 1
        p = pts.clone().requires_grad_(True)
        d = scene(p)
        (d * wts).sum().backward()
        gw = [x.grad.clone() for x in scene.parameters()]
        loop = H.make_loop(scene, 40, 72)
        q, t = _pose(-3.5)
        if case == "tight_neighbour":      # close to the link's far end, looking at it
            t = torch.tensor([[TIGHT_END[0], TIGHT_END[1], -1.0]], device=DEV)
        with torch.no_grad():
            frames = [loop(q, t, m, 1, 48) for m in (0, 4, 2, 5)]
        for x in scene.parameters():
            x.grad = None
        loop(q, t, 0, 1, 24).pow(2).mean().backward()
        res.append(dict(env=env, n_cull=n_cull, d=d.detach(), gp=p.grad, frames=frames, gw=gw,
                        gf=[x.grad.clone() for x in scene.parameters()]))
    assert res[0]["n_cull"] == 0
    if case == "siblings":
        assert res[1]["n_cull"] >= 3, "RM_CULL_MIN_COST=0 did not put a cull test in front of the link's siblings"
    else:
        assert res[2]["n_cull"] >= 8, "RM_CULL_LSE=1 did not put a cull test in front of the blob's children"
    print(f"culling leg {case}: cull instructions per variant {[r['n_cull'] for r in res]}")
    ref = res[0]
    for got in res[1:]:
        assert _same(ref["d"], got["d"]) and _same(ref["gp"], got["gp"]), got["env"]
        for x, y in zip(ref["frames"], got["frames"]):
            assert _same(x, y), got["env"]
        for name in ("gw", "gf"):
            for x, y in zip(ref[name], got[name]):
                assert _same(x, y), (got["env"], name)


def _link_scene_cpu(dtype=torch.float32):
    from ray_marching_amd.contrib import SDFLink
    link = SDFLink(**LINK).to(dtype)
    return builtin_part_spec(dtype), link, O._t(LINK_T, dtype), O._t(LINK_Q, dtype)


@pytest.mark.gpu
def test_link_scene_against_cpu_autograd_and_the_stand_alone_modules():
    """New geometry: contrib.make_link_scene() (library prebuilt by build()) against the CPU composition.  Values <= 1e-5,
    gradients <= 1e-4 (the contracts of smoke()); march positions <= 1e-5 or on a ray the CPU's own fp32 and fp64
    marches split by more than that (at most 5 % of the frame may be excused); RenderLoop == the stand-alone chain."""
    from ray_marching_amd.compiler import compiled_for
    from ray_marching_amd.contrib import make_link_scene
    scene = make_link_scene().to(DEV)
    assert compiled_for(scene).lib().rm_user_leaves() == 1
    spec, link, lt, lq = _link_scene_cpu()
    spec = O.map_spec(spec, lambda x: x.clone().requires_grad_(True))
    lt.requires_grad_(True); lq.requires_grad_(True)
    pts = _points(4096, seed=21)
    wts = torch.randn(4096, 1, generator=torch.Generator().manual_seed(22))
    pc = pts.clone().requires_grad_(True)
    want = composition(spec, link, lt, lq, pc)
    (want * wts).sum().backward()
    pg = pts.to(DEV).requires_grad_(True)
    got = scene(pg)
    (got * wts.to(DEV)).sum().backward()
    err = (got.detach().cpu() - want.detach()).abs().max().item()
    n_diff = int((got.detach().cpu() != want.detach()).sum())
    print(f"link scene: scene(points) max|err| {err:.3g}; {n_diff} of 4096 values not bit-identical with the CPU composition")
    assert err <= 1e-5
    gerr = (pg.grad.cpu() - pc.grad).abs().max().item()
    print(f"link scene: point gradient max|err| {gerr:.3g}")
    assert gerr <= 1e-4
    # named_parameters() order of make_link_scene(): room, sphere's affine + sphere, link's affine + link
    cpu_params = [v for _, v in O.spec_parameters(spec)] + [lt, lq] + list(link.parameters())
    names = [n for n, _ in scene.named_parameters()]
    assert len(cpu_params) == len(names) and names[-3:] == ["sdfs.1.sdfs.1.sdf.length", "sdfs.1.sdfs.1.sdf.radius1", "sdfs.1.sdfs.1.sdf.radius2"]
    for (name, g), c in zip(scene.named_parameters(), cpu_params):
        e = (g.grad.cpu() - c.grad).abs().max().item()
        print(f"link scene: grad {name} max|err| {e:.3g} (|g| {c.grad.abs().max().item():.3g})")
        assert e <= 1e-4, name
    # march, 64 x 96 rays, 32 steps from (0, 0, -1.5)
    h, w, steps = 64, 96, 32
    loop = H.make_loop(scene, h, w)
    q, t = _pose(-1.5)
    bufs = O.camera_buffers(1, w, h, H.PX * h, H.PX * w, H.PX * h)
    marches = {}
    for dtype in (torch.float32, torch.float64):
        s, l, tt, qq = _link_scene_cpu(dtype)
        pos, _, dirs = O.camera_forward(bufs[0].to(dtype), bufs[1].to(dtype), q.cpu().to(dtype), t.cpu().to(dtype))
        with torch.no_grad():
            for _ in range(steps):
                pos = composition(s, l, tt, qq, pos) * dirs + pos
        marches[dtype] = pos.double()
    from ray_marching_amd.rendering.ray_marching import SDFMarcher
    with torch.no_grad():
        pos, frames, _, dirs = loop.camera(q, t)
        p_gpu = SDFMarcher(scene)(pos, dirs, steps)
    e = (p_gpu.cpu().double() - marches[torch.float32]).abs()
    ill = ((marches[torch.float32] - marches[torch.float64]).abs().max(dim=-1, keepdim=True).values > 1e-5)
    off = e > 1e-5
    n_exc = int(ill.sum())
    print(f"link scene march: max|err| {e.max().item():.3g}; {int(off.sum())} coordinates beyond 1e-5, "
          f"{int((off & ~ill).sum())} of them on rays the CPU resolves; CPU fp32-vs-fp64 spread > 1e-5 on {n_exc} of {h * w} rays")
    assert not (off & ~ill).any() and n_exc <= 0.05 * h * w
    # RenderLoop == camera -> SDFMarcher -> scene / SDFNormals -> Shader, the package's own stand-alone modules
    for mode in (0, 4):
        with torch.no_grad():
            frame = loop(q, t, mode, 1, steps)
            p = loop.marcher(pos, dirs, steps)
            n, lap = loop.normals(p)
            img = loop.shader(pos, q, frames, dirs, p, n, lap, loop.scene(p), mode=mode, degree=1)
        assert _same(frame, img.expand(frame.shape)), mode
    # capture and display_frame go through the same launch
    with torch.no_grad():
        frame = loop(q, t, 0, 1, steps)
        assert _same(loop.capture(mode=0, marching_steps=steps)(q, t), frame)
        rgba = loop.display_frame(q, t, 0, 1, steps)
    assert rgba.shape == (h, w, 4) and _same(rgba[..., :3], frame[0].float()) and bool((rgba[..., 3] == 1).all())


@pytest.mark.gpu
def test_training_step_moves_a_perturbed_link_back():
    """20 Adam steps on the link's three parameters and its affine pose, towards a frame of the unperturbed scene: each
    replayed step of the captured graph gives the loss of the eager step taken from the same parameters (tolerance of
    test_training_step_helper_matches_the_eager_loop), and the last loss is below the first.  The loss is the MSE of the
    normal-shader image (mode 4): the exact gradient of the Lambertian one is dominated by a few crease pixels
    (examples/optimize_scene.py, "Note on conditioning") and twenty Adam steps on it go nowhere, for built-in scenes too."""
    from ray_marching_amd.contrib import make_link_scene
    h, w, steps = 64, 96, 32
    q, t = _pose(-1.5)
    with torch.no_grad():
        target = H.make_loop(make_link_scene(), h, w)(q, t, 4, 1, steps).clone()
    loss_fn = lambda image: (image - target).pow(2).mean()

    def perturbed():
        scene = make_link_scene().to(DEV)
        holder = scene.sdfs[1].sdfs[1]                      # the affine node that places the link
        with torch.no_grad():
            holder.sdf.length += 0.04; holder.sdf.radius1 -= 0.03; holder.sdf.radius2 += 0.015
            holder.translation += torch.tensor([0.04, -0.03, 0.03], device=DEV)
        return scene, list(holder.parameters())

    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*AccumulateGrad node's stream does not match.*")
        scene, moving = perturbed()
        loop = H.make_loop(scene, h, w)
        opt = torch.optim.Adam(moving, lr=2e-3, capturable=True)
        step = loop.training_step(loss_fn, mode=4, marching_steps=steps, optimizer=opt)
        twin, _ = perturbed()
        twin_loop = H.make_loop(twin, h, w)
        with torch.no_grad():
            first = float(loss_fn(loop(q, t, 4, 1, steps)))
        losses = []
        for it in range(20):
            if it == 0:
                step(q, t)                                   # warm-up iterations, the capture, one replay
            with torch.no_grad():
                for a, b in zip(twin.parameters(), scene.parameters()):
                    a.copy_(b)
            got = float(step(q, t))
            want = loss_fn(twin_loop(q, t, 4, 1, steps))
            want.backward()                                  # the eager step's own backward (its gradients are not applied:
            for x in twin.parameters():                      # the twin takes the captured loop's parameters every iteration)
                x.grad = None
            assert abs(got - float(want.detach())) <= 1e-6 * max(1.0, abs(float(want.detach()))), (it, got, float(want.detach()))
            losses.append(got)
    print(f"training leg: loss before {first:.6g}, per step {[round(x, 6) for x in losses]}")
    assert losses[-1] < first and losses[-1] < losses[0]


@pytest.mark.gpu
def test_leaf_type_compiled_at_test_time(monkeypatch, tmp_path):
    """The JIT path on the box: a leaf type nobody prebuilt, its library built by hipcc on first use (RM_SPECIALIZE=auto),
    against its own PyTorch forward on the CPU -- as the root, and under SDFRounding / SDFOnion / SDFSmoothUnion."""
    from ray_marching_amd import specialize
    from ray_marching_amd.compiler import compiled_for
    from ray_marching_amd.scene.primitives import SDFSphere
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFOnion, SDFRounding, SDFSmoothUnion
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    _register()
    monkeypatch.setattr(specialize, "SPEC_DIR", str(tmp_path))
    monkeypatch.setenv("RM_SPECIALIZE", "auto")
    specialize._loaded.clear()
    pill = UPill(0.4, 0.15)
    pts = _points(4096, seed=31, lo=-1.5, hi=1.5)
    pc = pts.clone().requires_grad_(True)
    want = pill(pc)
    want.sum().backward()
    cpu_grads = [x.grad.clone() for x in pill.parameters()]
    for x in pill.parameters():
        x.grad = None
    pill.to(DEV)
    pg = pts.to(DEV).requires_grad_(True)
    got = pill(pg)                                           # the leaf as the root: CUDA points go to the HIP evaluator
    assert compiled_for(pill).lib().rm_user_leaves() == 1 and len(os.listdir(tmp_path)) >= 1
    got.sum().backward()
    assert (got.detach().cpu() - want.detach()).abs().max().item() <= 1e-5
    assert (pg.grad.cpu() - pc.grad).abs().max().item() <= 1e-4
    for a, b in zip(pill.parameters(), cpu_grads):
        assert (a.grad.cpu() - b).abs().max().item() <= 1e-4 * max(1.0, b.abs().max().item())
    # under the built-in wrappers, against the same wrappers written out on the CPU
    k = 12.0
    scene = SDFSmoothUnion([SDFOnion(SDFRounding(A(UPill(0.4, 0.15), orientation=LINK_Q, translation=[0.2, 0.0, 0.1]), 0.03), 0.02),
                            SDFSphere(0.3)], blend_k=k).to(DEV)
    with torch.no_grad():
        got = scene(pts.to(DEV)).cpu()
        local = O.quat_rotate(pts - O._t([0.2, 0.0, 0.1]), O.quat_conj(O._t(LINK_Q)))
        a = (UPill(0.4, 0.15)(local) - 0.03).abs() - 0.02
        b = torch.linalg.vector_norm(pts, dim=-1, keepdim=True) - 0.3
        want = O.t_logsumexp(torch.stack([a, b], dim=-2) * (-k), -2) / (-k)
    assert (got - want).abs().max().item() <= 1e-5
    specialize._loaded.clear()
