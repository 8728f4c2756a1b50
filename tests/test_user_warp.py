"""User-defined domain operators (ray_marching_amd/extensions.py: register_warp): registration, the RM_OP_USER_PUSH /
RM_OP_USER_POP program, the specialised libraries that carry the operators' HIP source, and -- on the GPU -- parity of such
scenes with built-in twins (UAffine restates SDFAffineTransformation), with CPU autograd through the operators' own ``warp`` /
``out``, nested and through the replayed tail of the reverse march, with culling on and off around and inside them, and
through a captured training loop.

The CPU side of every GPU comparison is `cpu_eval()` below over a spec that `spec_of()` reads off the scene's own module
tree: the oracle's functions (oracle.sdf_oracle) for the built-in nodes, ``warp`` / ``out`` / ``combine`` of the instance for
the user-defined ones.  Helpers, the restated-math mode of the oracle and every tolerance are those of
tests/test_user_combinator.py.
"""
import copy
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import sdf_oracle as O
from tests import helpers as H
from tests.helpers import _points, _pose, _same, environment

DEV = "cuda"


# --------------------------------------------------------------------------------------------------------------
# test-defined warps
# --------------------------------------------------------------------------------------------------------------
class _Unary(nn.Module):
    def __init__(self, sdf):
        super().__init__()
        self.sdf = sdf

    def forward(self, query_coords):
        values = self.sdf(self.warp(query_coords))
        return self.out(values, query_coords) if hasattr(self, "out") else values


class UAffine(_Unary):
    """SDFAffineTransformation restated as a user warp: the map and the VJP of RM_OP_AFFINE_PUSH, so a scene built with it
    must agree with the built-in one bit for bit."""

    def __init__(self, sdf, orientation, translation):
        super().__init__(sdf)
        self.translation = nn.Parameter(torch.tensor(translation, dtype=torch.float32))
        self.orientation = nn.Parameter(torch.tensor(orientation, dtype=torch.float32))

    def warp(self, points):
        return O.quat_rotate(points - self.translation, O.quat_conj(self.orientation))


UAFFINE_HIP = """
template <bool Fast> RM_DEV rm::V3 uaffine_fwd(rm::V3 p, const float* theta) {
  return qrot(p - mk3(theta[0], theta[1], theta[2]), theta[3], neg(mk3(theta[4], theta[5], theta[6])));
}
template <bool Fast> RM_DEV void uaffine_vjp(rm::V3 p, const float* theta, rm::V3 gl, rm::V3& gp, float* gtheta) {
  float w = theta[3];
  V3 u = neg(mk3(theta[4], theta[5], theta[6]));
  V3 v = p - mk3(theta[0], theta[1], theta[2]);
  V3 t = 2.0f * cross(u, v);
  V3 ugl = cross(u, gl);
  V3 gv = (gl + 2.0f * cross(u, ugl)) - (2.0f * w) * ugl;
  float gw = (gl.x * t.x + gl.y * t.y) + gl.z * t.z;
  V3 gt = w * gl + cross(gl, u);
  V3 gu = cross(t, gl) + 2.0f * cross(v, gt);
  gtheta[0] = -gv.x; gtheta[1] = -gv.y; gtheta[2] = -gv.z;
  gtheta[3] = gw;
  gtheta[4] = -gu.x; gtheta[5] = -gu.y; gtheta[6] = -gu.z;
  gp = gp + gv;
}
"""


class UShear(_Unary):
    """A warp with an ``out`` and parameters in both: child(p + a * (p.y, 0, 0)) * b + c * p.z -- not a distance, only a
    function whose every partial derivative (gd, the direct gp, gtheta of both halves) is non-trivial.  On the node's
    surface the CHILD's value is -c p.z / b, not 0: d(out)/db = g * d reads the value slot where it matters."""

    def __init__(self, sdf, a, bc):
        super().__init__(sdf)
        self.a = nn.Parameter(torch.tensor(a, dtype=torch.float32))
        self.bc = nn.Parameter(torch.tensor(bc, dtype=torch.float32))

    def warp(self, points):
        return torch.cat([points[..., :1] + self.a * points[..., 1:2], points[..., 1:]], dim=-1)

    def out(self, values, points):
        return values * self.bc[0] + self.bc[1] * points[..., 2:]


USHEAR_HIP = """
template <bool Fast> RM_DEV rm::V3 ushear_fwd(rm::V3 p, const float* theta) { return mk3(p.x + theta[0] * p.y, p.y, p.z); }
template <bool Fast> RM_DEV void ushear_vjp(rm::V3 p, const float* theta, rm::V3 gq, rm::V3& gp, float* gtheta) {
  gp.x += gq.x; gp.y += gq.y + theta[0] * gq.x; gp.z += gq.z;
  gtheta[0] = gq.x * p.y;
}
template <bool Fast> RM_DEV float ushear_out_fwd(float d, rm::V3 p, const float* theta) { return d * theta[1] + theta[2] * p.z; }
template <bool Fast> RM_DEV void ushear_out_vjp(float d, rm::V3 p, const float* theta, float g, float& gd, rm::V3& gp, float* gtheta) {
  gd = g * theta[1];
  gp.z += g * theta[2];
  gtheta[1] = g * d;
  gtheta[2] = g * p.z;
}
"""


def _register():
    from ray_marching_amd.extensions import register_warp
    register_warp(UAffine, params=("translation", "orientation"), hip=UAFFINE_HIP, cost=25)
    register_warp(UShear, params=("a", "bc"), hip=USHEAR_HIP, cost=8)


# --------------------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------------------
Q_ROT, IDENT = [0.9014, 0.25, 0.25, 0.25], [1.0, 0.0, 0.0, 0.0]


def scene2_placed():
    """make_test_scene2() with its sphere and torus placed by affine nodes (scene 2 itself has none to substitute)."""
    from ray_marching_amd.scene.primitives import SDFLine, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    return SDFUnion([make_room(), SDFUnion([A(SDFSphere(radius=0.5), orientation=IDENT, translation=[0.9, 0.0, 0.0]),
                                            A(SDFTorus(radius1=1.0, radius2=0.25), orientation=Q_ROT, translation=[0.0, 0.1, 0.2]),
                                            SDFLine(start=(1.0, 0.0, 0.0), end=(-1.0, 0.0, 0.0), radius=0.1)])])


def _twin_factories():
    from ray_marching_amd.scene.scene_registry import make_closed_test_scene, make_test_scene2
    return {"scene2": make_test_scene2, "closed_scene1": make_closed_test_scene, "scene2_placed": scene2_placed}


def with_uaffine(module):
    """A deep copy of the scene with every SDFAffineTransformation replaced by a UAffine of the same pose."""
    from ray_marching_amd.scene.transformations import SDFAffineTransformation

    def swap(m):
        for name, child in list(m._modules.items()):
            m._modules[name] = swap(child)
        if isinstance(m, SDFAffineTransformation):
            return UAffine(m.sdf, m.orientation.detach().tolist(), m.translation.detach().tolist())
        return m

    return swap(copy.deepcopy(module))


TWIN_ENVS = [dict(RM_CULL="0"), dict()]


def operator_scenes():
    """One scene per shipped operator, and the shipped scene that nests all four."""
    from ray_marching_amd.contrib import SDFElongate, SDFMirror, SDFRepeat, SDFScale, make_warped_scene
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A
    return {"scale": lambda: SDFScale(A(SDFTorus(0.5, 0.12), orientation=Q_ROT, translation=[0.1, 0.0, 0.2]), scale=0.7),
            "mirror": lambda: SDFMirror(A(SDFBox((0.3, 0.2, 0.4)), orientation=Q_ROT, translation=[0.6, 0.1, 0.2]), origin=0.15),
            "repeat": lambda: SDFRepeat(SDFSphere(0.2), period=(0.9, 1.1, 1.3)),
            "elongate": lambda: SDFElongate(SDFTorus(0.4, 0.1), halfsides=(0.3, 0.05, 0.2)),
            "warped": make_warped_scene}


REPEAT_PERIODS = {"repeat": (0.9, 1.1, 1.3), "warped": (0.5, 0.5, 0.5)}
POINT_RANGE = {"scale": 1.5, "mirror": 1.5, "repeat": 2.5, "elongate": 1.5, "warped": 2.5}


def operator_points(which, n=4096):
    """n random points; for the scenes with an SDFRepeat those within 1e-4 of a cell border (where round() jumps) are left
    out.  Returns (points, number left out)."""
    r = POINT_RANGE[which]
    pts = _points(n, seed=31 + sorted(POINT_RANGE).index(which), lo=-r, hi=r)
    if which not in REPEAT_PERIODS:
        return pts, 0
    period = torch.tensor(REPEAT_PERIODS[which])
    cell = pts / period
    to_border = ((cell - cell.floor() - 0.5).abs() * period).min(dim=-1).values      # borders lie at (k + 1/2) period
    keep = to_border >= 1e-4
    return pts[keep], int((~keep).sum())


def nesting_scene():
    """A warp inside a warp (with and without an ``out``, in both orders) inside a smooth union inside a combinator."""
    from ray_marching_amd.contrib import SDFElongate, SDFIntersection, SDFMirror, SDFScale
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFSmoothUnion, SDFUnion
    one = SDFScale(SDFMirror(A(SDFSphere(0.3), orientation=IDENT, translation=[0.5, 0.0, 0.0]), origin=0.1), scale=1.4)
    two = A(SDFMirror(UShear(SDFElongate(SDFTorus(0.3, 0.08), halfsides=(0.05, 0.02, 0.2)), a=0.2, bc=[0.9, 0.3]), origin=-0.2),
            orientation=Q_ROT, translation=[0.0, 0.9, 0.2])
    blob = SDFSmoothUnion([one, two], blend_k=22.0)
    return SDFUnion([make_room(), SDFIntersection([blob, SDFBox((1.6, 1.6, 1.6))])])


def cull_nested_scene():
    """Culling leg 1: a mirrored min-union whose torus is expensive enough for a CULL_MIN of its own (inside the warp's
    frame), under an affine node, next to the room and a bounded built-in sibling that gets the CULL_MIN of the root."""
    from ray_marching_amd.contrib import SDFMirror
    from ray_marching_amd.scene.primitives import SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    inner = SDFUnion([SDFSphere(0.25), A(SDFTorus(0.5, 0.12), orientation=IDENT, translation=[0.9, 0.3, 0.2])])
    return SDFUnion([make_room(), A(SDFMirror(inner, origin=0.0), orientation=Q_ROT, translation=[-0.3, 0.1, 0.2]),
                     A(SDFTorus(radius1=0.5, radius2=0.12), orientation=[0.0, 0.5 ** 0.5, 0.5 ** 0.5, 0.0], translation=[1.1, 0.4, 1.5])])


TIGHT_END = (0.9, 0.8, 0.0)       # a point on the scaled sphere of scaled_with_a_tight_neighbour()


def scaled_with_a_tight_neighbour():
    """Culling leg 2, built so that a wrong bound for a warped node SHOWS: a stiff smooth union (k = 300: a child is skipped
    from 0.35 behind the nearest one) that holds a sphere of 0.1 scaled by 8 and a tiny sphere 0.12 off its surface.  The
    bound table has an entry per child; were subtree_bound to fall through at USER_POP, the scaled node's entry would be its
    CHILD's sphere -- radius 0.1, in the child's frame -- and waves at TIGHT_END, 0.7 outside that sphere and 0.07 from the
    neighbour, would skip the node whose surface they are on."""
    from ray_marching_amd.contrib import SDFScale
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFSmoothUnion, SDFUnion
    big = A(SDFScale(SDFSphere(0.1), scale=8.0), orientation=IDENT, translation=[TIGHT_END[0], 0.0, 0.0])
    neighbour = A(SDFSphere(0.05), orientation=IDENT, translation=[TIGHT_END[0], TIGHT_END[1] + 0.12, TIGHT_END[2]])
    far = [A(SDFSphere(0.3), orientation=IDENT, translation=[-2.0, -1.5, 1.0]), A(SDFBox((0.2, 0.3, 0.15)), orientation=Q_ROT, translation=[2.4, -1.0, 0.5]),
           A(SDFTorus(0.4, 0.1), orientation=Q_ROT, translation=[-1.5, 1.5, -1.0]), A(SDFSphere(0.25), orientation=IDENT, translation=[0.0, -2.0, -1.5]),
           A(SDFBox((0.3, 0.1, 0.2)), orientation=IDENT, translation=[2.2, 1.8, 1.5]), A(SDFTorus(0.35, 0.08), orientation=IDENT, translation=[-2.2, 0.0, 2.0])]
    return SDFUnion([make_room(), SDFSmoothUnion([big, neighbour] + far, blend_k=300.0)])


CULL_ENVS = {"nested": [dict(RM_CULL="0"), dict()],
             "tight_neighbour": [dict(RM_CULL="0"), dict(), dict(RM_CULL_LSE="1", RM_CULL_LSE_MIN="2")]}
CULL_SCENES = {"nested": cull_nested_scene, "tight_neighbour": scaled_with_a_tight_neighbour}


# --------------------------------------------------------------------------------------------------------------
# the CPU side
# --------------------------------------------------------------------------------------------------------------
def spec_of(module, dtype=torch.float32):
    """The scene's module tree as a cpu_eval() spec: (kind, {own parameters as fresh leaf tensors}, children) for the built-in
    nodes (oracle layout), ("warp" | "comb", a copy of the instance without its children, children) for the user-defined."""
    from ray_marching_amd.extensions import combinator_spec, warp_spec

    def stand_in(node, attr):
        inst = copy.copy(node)
        inst._parameters = {k: nn.Parameter(v.detach().clone().to(dtype)) for k, v in node._parameters.items()}
        inst._modules = {attr: nn.Identity()}
        return inst

    kind = getattr(module, "_rm_kind", None)
    if kind is None and warp_spec(module) is not None:
        return ("warp", stand_in(module, warp_spec(module).child), spec_of(getattr(module, warp_spec(module).child), dtype))
    if kind is None and combinator_spec(module) is not None:
        return ("comb", stand_in(module, combinator_spec(module).children), [spec_of(c, dtype) for c in module.sdfs])
    prm = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in module._parameters.items()}
    if kind in ("affine", "rounding", "onion"):
        return (kind, prm, spec_of(module.sdf, dtype))
    if kind in ("union", "smooth_union"):
        return (kind, prm, [spec_of(c, dtype) for c in module.sdfs])
    assert kind in ("sphere", "box", "plane", "line", "disk", "torus"), kind
    return (kind, prm)


def cpu_eval(spec, p):
    """oracle.sdf_eval with user-defined nodes anywhere in the tree: the inner nodes restate its one-liners around cpu_eval of
    their children, the leaves are the oracle's."""
    kind = spec[0]
    if kind == "warp":
        values = cpu_eval(spec[2], spec[1].warp(p))
        return spec[1].out(values, p) if hasattr(spec[1], "out") else values
    if kind == "comb":
        return spec[1].combine(torch.cat([cpu_eval(c, p) for c in spec[2]], dim=-1))
    if kind == "affine":
        return cpu_eval(spec[2], O.quat_rotate(p - spec[1]["translation"], O.quat_conj(spec[1]["orientation"])))
    if kind == "union":
        return torch.stack([cpu_eval(c, p) for c in spec[2]], dim=-2).min(dim=-2).values
    if kind == "smooth_union":
        k = spec[1]["blend_k"]
        return O.t_logsumexp(torch.stack([cpu_eval(c, p) for c in spec[2]], dim=-2) * (-k), -2) / (-k)
    if kind == "rounding":
        return cpu_eval(spec[2], p) - spec[1]["rounding"]
    if kind == "onion":
        return cpu_eval(spec[2], p).abs() - spec[1]["radius"]
    return _ORACLE_SDF_EVAL(spec, p)


_ORACLE_SDF_EVAL = O.sdf_eval      # (cpu_render() puts cpu_eval in its place for the length of one render)


def cpu_render(spec, monkeypatch, *args, **kwargs):
    """oracle.render -- camera, march, normals, shader, all on the CPU -- over a spec with user-defined nodes: the oracle's
    own code with cpu_eval where it calls sdf_eval."""
    with monkeypatch.context() as m:
        m.setattr(O, "sdf_eval", cpu_eval)
        return O.render(spec, *args, **kwargs)


def cpu_parameters(spec):
    """Parameter tensors of a spec in the scene's named_parameters() order (own first, then the children)."""
    own = list(spec[1].parameters()) if spec[0] in ("warp", "comb") else list(spec[1].values())
    kids = spec[2] if len(spec) > 2 else []
    return own + [x for c in (kids if isinstance(kids, list) else [kids]) for x in cpu_parameters(c)]


def compiled_under(scene, env):
    """The scene compiled under ``env`` (compiler.compiled_for keeps the program with the module)."""
    from ray_marching_amd.compiler import compiled_for
    with environment(**env):
        compiled_for(scene)
    return scene


def gpu_test_programs():
    """Every test-defined program the GPU legs launch: the CPU suite and build() compile their libraries, so that a GPU run of
    the same tree finds them; where they are missing the library builds itself on first use."""
    from ray_marching_amd import specialize
    from ray_marching_amd.compiler import compile_scene
    _register()
    out = [compile_scene(with_uaffine(make())) for name, make in _twin_factories().items() if name != "scene2"]
    for env in TWIN_ENVS:                         # the built-in twins, with and without cull tests
        with environment(**env):
            out += [compile_scene(make()) for make in _twin_factories().values()]
    out += [compile_scene(make()) for make in operator_scenes().values()]
    out.append(compile_scene(nesting_scene()))
    for case, envs in CULL_ENVS.items():
        for env in envs:
            with environment(**env):
                out.append(compile_scene(CULL_SCENES[case]()))
    return list({specialize.scene_hash(cs): cs for cs in out}.values())


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
UNARY = ("template <bool Fast> RM_DEV rm::V3 NAME_fwd(rm::V3 p, const float* theta) { return p; }\n"
         "template <bool Fast> RM_DEV void NAME_vjp(rm::V3 p, const float* theta, rm::V3 gq, rm::V3& gp, float* gtheta) { gp = gp + gq; }\n")
UNARY_OUT = ("template <bool Fast> RM_DEV float NAME_out_fwd(float d, rm::V3 p, const float* theta) { return d; }\n"
             "template <bool Fast> RM_DEV void NAME_out_vjp(float d, rm::V3 p, const float* theta, float g, float& gd, rm::V3& gp, "
             "float* gtheta) { gd = g; }\n")


def test_registration_errors():
    from ray_marching_amd import contrib
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.extensions import combinator_spec, leaf_spec, register_combinator, register_leaf, register_warp, warp_spec
    from ray_marching_amd.scene.primitives import SDFSphere
    from ray_marching_amd.scene.transformations import SDFUnion
    _register()
    node = UAffine(SDFSphere(0.3), IDENT, [0.0, 0.0, 0.0])
    spec = warp_spec(node)
    assert (spec.name, spec.child, spec.has_out, spec.params) == ("uaffine", "sdf", False, ("translation", "orientation"))
    assert leaf_spec(node) is None and combinator_spec(node) is None
    assert warp_spec(SDFSphere(0.3)) is None and warp_spec(nn.Linear(2, 2)) is None and warp_spec(contrib.SDFLink(0.3, 0.3, 0.1)) is None
    scale = warp_spec(contrib.SDFScale(SDFSphere(0.3), 0.5))
    assert (scale.name, scale.has_out, scale.params, scale.cost) == ("sdf_scale", True, ("scale",), 36)
    assert [warp_spec(c(SDFSphere(0.3), v)).has_out for c, v in ((contrib.SDFMirror, 0.0), (contrib.SDFRepeat, (1.0, 1.0, 1.0)),
                                                                  (contrib.SDFElongate, (0.1, 0.1, 0.1)))] == [False] * 3
    register_warp(UAffine, params=("translation", "orientation"), hip=UAFFINE_HIP, cost=25)          # the same again: fine
    with pytest.raises(ValueError, match="already registered"):
        register_warp(UAffine, params=("translation", "orientation"), hip=UAFFINE_HIP.replace("gp = gp + gv", "gp = gv + gp"), cost=25)
    with pytest.raises(ValueError, match="already registered"):
        register_warp(UAffine, params=("translation", "orientation"), hip=UAFFINE_HIP, cost=26)
    with pytest.raises(ValueError, match="already registered"):
        register_warp(UAffine, params=("orientation", "translation"), hip=UAFFINE_HIP, cost=25)
    with pytest.raises(ValueError, match="already registered"):
        register_warp(UAffine, params=("translation", "orientation"), hip=UAFFINE_HIP, cost=25, child="inner")

    class Same(_Unary):
        def warp(self, points):
            return points

    with pytest.raises(TypeError, match="not an nn.Module"):
        register_warp(dict, hip=UNARY.replace("NAME", "same"))
    with pytest.raises(TypeError, match="already a ray_marching_amd node"):
        register_warp(SDFUnion, hip=UNARY.replace("NAME", "same"))
    with pytest.raises(TypeError, match="already registered as a leaf"):
        register_warp(contrib.SDFLink, hip=UNARY.replace("NAME", "same"))
    with pytest.raises(TypeError, match="already registered as a combinator"):
        register_warp(contrib.SDFIntersection, hip=UNARY.replace("NAME", "same"))
    with pytest.raises(TypeError, match="already registered as a warp"):
        register_leaf(contrib.SDFMirror, params=(), cost=1, hip=(
            "template <bool Fast> RM_DEV float flat_fwd(rm::V3 p, const float* theta) { return p.x; }\n"
            "template <bool Fast> RM_DEV void flat_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) { gp.x += g; }\n"))

    class NoWarp(nn.Module):
        def __init__(self, sdf):
            super().__init__()
            self.sdf = sdf

        def forward(self, query_coords):
            return self.sdf(query_coords)

    with pytest.raises(TypeError, match="has no warp"):
        register_warp(NoWarp, hip=UNARY.replace("NAME", "no_warp"))

    class WithOut(Same):
        def out(self, values, points):
            return values

    with pytest.raises(TypeError, match="has an out"):                                # `out` in Python, none in HIP
        register_warp(WithOut, hip=UNARY.replace("NAME", "with_out"))
    with pytest.raises(TypeError, match="has no out"):                                # ... and the reverse
        register_warp(Same, hip=(UNARY + UNARY_OUT).replace("NAME", "same"))
    for half in UNARY_OUT.splitlines(keepends=True)[:1], UNARY_OUT.splitlines(keepends=True)[1:]:
        with pytest.raises(ValueError, match="both or neither"):                      # only one of the two `out` functions
            register_warp(WithOut, hip=(UNARY + "".join(half)).replace("NAME", "with_out"))
    with pytest.raises(TypeError, match="has an out"):                                # the pair under another NAME is not this warp's
        register_warp(WithOut, hip=UNARY.replace("NAME", "with_out") + UNARY_OUT.replace("NAME", "other"))
    with pytest.raises(ValueError, match="with one NAME"):
        register_warp(Same, hip=UNARY.replace("NAME_vjp", "other_vjp").replace("NAME", "same"))
    with pytest.raises(ValueError, match="with one NAME"):                            # a leaf's signature is not a warp's
        register_warp(Same, hip=contrib._LINK_HIP.replace("link_", "same_"))
    # identifiers are unique across leaves, combinators and warps, in every direction
    with pytest.raises(ValueError, match="already used by SDFLink"):
        register_warp(Same, hip=UNARY.replace("NAME", "link"))
    with pytest.raises(ValueError, match="already used by SDFIntersection"):
        register_warp(Same, hip=UNARY.replace("NAME", "sdf_intersection"))
    with pytest.raises(ValueError, match="already used by SDFMirror"):
        register_warp(Same, hip=UNARY.replace("NAME", "sdf_mirror"))
    with pytest.raises(ValueError, match="already used by UAffine"):
        class Flat(nn.Module):
            def forward(self, p):
                return p[..., :1]
        register_leaf(Flat, params=(), cost=1, hip=(
            "template <bool Fast> RM_DEV float uaffine_fwd(rm::V3 p, const float* theta) { return p.x; }\n"
            "template <bool Fast> RM_DEV void uaffine_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) { gp.x += g; }\n"))
    with pytest.raises(ValueError, match="already used by SDFScale"):
        class First(nn.Module):
            def __init__(self, sdfs):
                super().__init__()
                self.sdfs = nn.ModuleList(sdfs)

            def combine(self, values):
                return values[..., :1]

            def forward(self, query_coords):
                return self.sdfs[0](query_coords)
        register_combinator(First, hip=(
            "template <bool Fast, int N> RM_DEV float sdf_scale_fwd(const float (&d)[N], const float* theta) { return d[0]; }\n"
            "template <bool Fast, int N> RM_DEV void sdf_scale_vjp(const float (&d)[N], const float* theta, float g, float (&gd)[N], "
            "float* gtheta) { gd[0] = g; }\n"))
    with pytest.raises(ValueError, match="inline assembly"):
        register_warp(Same, hip=UNARY.replace("NAME", "same").replace("return p;", 'asm volatile(""); return p;'))
    assert warp_spec(Same(SDFSphere(0.3))) is None and warp_spec(WithOut(SDFSphere(0.3))) is None      # no failure registered anything

    # the child attribute: missing on the instance, or not a module
    class Elsewhere(Same):
        pass

    register_warp(Elsewhere, hip=UNARY.replace("NAME", "warp_elsewhere"), child="inner")
    with pytest.raises(ValueError, match="inner"):
        compile_scene(Elsewhere(SDFSphere(0.3)))
    register_warp(Same, hip=UNARY.replace("NAME", "same"))
    cs = compile_scene(Same(SDFSphere(0.3)))
    assert cs.program.tolist() == [[22, 0, 0, 0], [1, 0, 0, 0], [23, 0, 0, 0]] and cs.user_warps[0][:3] == ("same", 0, False)
    assert cs.n_slots == 0 and cs.stack_floats == 6
    register_warp(WithOut, hip=(UNARY + UNARY_OUT).replace("NAME", "with_out"))       # a subclass of a warp, registered on its own
    cs = compile_scene(WithOut(Same(SDFSphere(0.3))))
    assert cs.program.tolist() == [[22, 0, 0, 0], [22, 0, 1, 0], [1, 0, 0, 0], [23, 0, 1, 0], [23, 0, 0, 1]] and cs.n_slots == 1
    assert [w[:3] for w in cs.user_warps] == [("with_out", 0, True), ("same", 0, False)]

    class Gap(Same):
        def __init__(self, sdf):
            super().__init__(sdf)
            self.a = nn.Parameter(torch.tensor(1.0)); self.b = nn.Parameter(torch.tensor(2.0)); self.c = nn.Parameter(torch.tensor(3.0))

    register_warp(Gap, params=("a", "c"), hip=UNARY.replace("NAME", "warp_gap"))      # b lies between them
    with pytest.raises(ValueError, match="not contiguous"):
        compile_scene(Gap(SDFSphere(0.3)))

    class Sized(Same):
        def __init__(self, sdf, n):
            super().__init__(sdf)
            self.v = nn.Parameter(torch.zeros(n))

    register_warp(Sized, params=("v",), hip=UNARY.replace("NAME", "warp_sized"))
    with pytest.raises(ValueError, match="same number of parameter floats"):
        compile_scene(Sized(Sized(SDFSphere(0.3), 2), 3))
    # CPU points run the class's own PyTorch forward
    link = contrib.SDFLink(0.35, 0.3, 0.08)
    p = _points(64)
    scaled = contrib.SDFScale(link, 0.5)
    assert torch.equal(scaled(p), link(p / 0.5) * 0.5) and scaled(p).shape == (64, 1)
    assert torch.equal(scaled(p), contrib.SDFScale._rm_torch_forward(scaled, p))
    mirrored = contrib.SDFMirror(link, 0.25)
    assert torch.equal(mirrored(p), link(torch.cat([(p[:, :1] - 0.25).abs(), p[:, 1:]], dim=-1)))
    assert [n for n, _ in scaled.named_parameters()][0] == "scale"


# sha1(repr(signature)) of the scenes that compiled before this extension point existed, computed at the parent commit
PARENT_SIGNATURES = {
    "make_room": "cc8d9a3fc5b8ce19a05a7ce39a79e9e05533d7cb",
    "make_test_scene": "850dec081c7649c71eb44f8a82b355df051f7cae",
    "make_test_scene2": "663383d9a93e783b836a2cfdf8291c3546ab9718",
    "make_closed_test_scene": "2c397b0264226da8c3d4e5a5f8636ae1c01493cb",
    "make_many_primitive_scene": "84a871043254241a0b2c979e67ecdd1fd2fe1389",
    "make_link_scene": "f5ae69c9410708b5fa9fdde29a2741ef2161e09a",
    "make_bounded_link_scene": "b98ea11fc1b81b63dd7acd21f56c7b6acf73c88b",
    "make_carved_scene": "398bb2a2152f807d0b5c7662cb7c24871a402e49",
}


def test_program_of_scenes_with_warps():
    import hashlib
    import pickle
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.scene import scene_registry as R
    from ray_marching_amd.scene.primitives import SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    _register()
    assert (_abi.OP_USER_PUSH, _abi.OP_USER_POP) == (22, 23) and _abi.ABI_VERSION == 14
    sha = lambda text: hashlib.sha1(text.encode()).hexdigest()
    # ---- the shipped scene: PUSH / POP nest around the child's rows with the same offset and type
    scene = contrib.make_warped_scene()
    cs = compile_scene(scene)
    rows = cs.program.reshape(-1, 4)
    offs = dict(zip(cs.leaf_names, cs.leaf_offsets))
    pushes = np.flatnonzero(rows[:, 0] == _abi.OP_USER_PUSH)
    pops = np.flatnonzero(rows[:, 0] == _abi.OP_USER_POP)
    assert cs.user_warps == (("sdf_mirror", 1, False, sha(contrib._MIRROR_HIP)), ("sdf_scale", 1, True, sha(contrib._SCALE_HIP)),
                             ("sdf_elongate", 3, False, sha(contrib._ELONGATE_HIP)), ("sdf_repeat", 3, False, sha(contrib._REPEAT_HIP)))
    assert cs.user_warp_sources == (contrib._MIRROR_HIP, contrib._SCALE_HIP, contrib._ELONGATE_HIP, contrib._REPEAT_HIP)
    assert rows[pushes].tolist() == [[22, offs["sdfs.1.sdf.origin"], 0, 1], [22, offs["sdfs.1.sdf.sdf.sdfs.0.sdf.scale"], 1, 1],
                                     [22, offs["sdfs.1.sdf.sdf.sdfs.1.sdf.halfsides"], 2, 3], [22, offs["sdfs.2.sdfs.0.period"], 3, 3]]
    stack = []
    for i, (op, off, a0, a1) in enumerate(rows.tolist()):
        if op in (_abi.OP_USER_PUSH, _abi.OP_AFFINE_PUSH):
            stack.append((op, off, a0, a1))
        if op == _abi.OP_AFFINE_POP:
            assert stack.pop()[:2] == (_abi.OP_AFFINE_PUSH, off)
        if op == _abi.OP_USER_POP:
            assert stack.pop() == (_abi.OP_USER_PUSH, off, a0, a1 >> 16), i
    assert not stack and len(pops) == 4
    # the value slot: present only for the type with an `out` (slots: root union 0-2, the room's onion 3, the mirrored union
    # 4-5, the scale's 6, the intersection 7-8 + 9-10)
    assert [(int(r[2]), int(r[3]) & 65535) for r in rows[pops]] == [(1, 7), (2, 0), (0, 0), (3, 0)] and cs.n_slots == 11
    assert cs.signature[-1] == cs.user_warps and cs.signature[-3] == () and cs.signature[-2] == cs.user_combinators and len(cs.signature) == 9
    assert not (rows[:, 0] == _abi.OP_CULL_MIN).any()          # both solids hold a warp: nothing to cull in this scene
    # ---- a frame costs what an affine frame costs
    plain = compile_scene(A(SDFSphere(0.3), orientation=IDENT, translation=[0.1, 0.0, 0.0]))
    for warp in (contrib.SDFMirror(SDFSphere(0.3), 0.1), contrib.SDFScale(SDFSphere(0.3), 0.5), UAffine(SDFSphere(0.3), IDENT, [0.1, 0.0, 0.0])):
        assert compile_scene(warp).stack_floats == plain.stack_floats == 6
    assert compile_scene(contrib.SDFMirror(A(SDFSphere(0.3), orientation=IDENT, translation=[0.1, 0.0, 0.0]), 0.0)).stack_floats == 12
    # ---- a min-union that holds an expensive warped child gets no CULL_MIN for it; the one inside the child stays
    cs = compile_scene(cull_nested_scene())
    rows = cs.program.reshape(-1, 4)
    sites = np.flatnonzero(rows[:, 0] == _abi.OP_CULL_MIN)
    push, pop = int(np.flatnonzero(rows[:, 0] == _abi.OP_USER_PUSH)[0]), int(np.flatnonzero(rows[:, 0] == _abi.OP_USER_POP)[0])
    assert len(sites) == 2
    for i in sites:
        inside = rows[i + 1:i + (rows[i, 3] >> 8), 0]
        assert not ((inside == _abi.OP_USER_PUSH) | (inside == _abi.OP_USER_POP)).any()
    assert push < sites[0] < pop < sites[1] and rows[sites[0] + 2, 0] == _abi.OP_TORUS and rows[sites[1] + 2, 0] == _abi.OP_TORUS
    with environment(RM_CULL_MIN_COST="0"):                    # ... even when every boundable child is asked for one
        eager = compile_scene(cull_nested_scene()).program.reshape(-1, 4)
    for i in np.flatnonzero(eager[:, 0] == _abi.OP_CULL_MIN):
        inside = eager[i + 1:i + (eager[i, 3] >> 8), 0]
        assert not ((inside == _abi.OP_USER_PUSH) | (inside == _abi.OP_USER_POP)).any()
    with environment(RM_CULL="0"):
        assert not (compile_scene(cull_nested_scene()).program[:, 0] == _abi.OP_CULL_MIN).any()
    # the smooth union of the tight-neighbour scene: a bound table entry per child under RM_CULL_LSE=1, the warped one included
    with environment(RM_CULL_LSE="1", RM_CULL_LSE_MIN="2"):
        tight = compile_scene(scaled_with_a_tight_neighbour()).program.reshape(-1, 4)
    assert int((tight[:, 0] == _abi.OP_CULL_LSE).sum()) == 8
    # ---- every scene that compiled before keeps its signature
    scenes = {"make_room": R.make_room(), "make_test_scene": R.make_test_scene(), "make_test_scene2": R.make_test_scene2(),
              "make_closed_test_scene": R.make_closed_test_scene(), "make_many_primitive_scene": R.make_many_primitive_scene(),
              "make_link_scene": contrib.make_link_scene(), "make_bounded_link_scene": contrib.make_link_scene(bounded=True),
              "make_carved_scene": contrib.make_carved_scene()}
    assert {k: sha(repr(compile_scene(m).signature)) for k, m in scenes.items()} == PARENT_SIGNATURES
    # ---- the sources are part of the library key; pickle / deepcopy keep the scene whole
    cs = compile_scene(scene)
    hdr = specialize.code_header(cs)
    assert "#define RM_USER_WARPS 4" in hdr and "#define RM_USER_WARP_MAX_PARAMS 3" in hdr and "#define RM_USER_COMBINATORS 1" in hdr
    assert "RM_USER_LEAVES" not in hdr and hdr.count("sdf_scale_out_fwd<Fast>") == 1 and "sdf_mirror_out" not in hdr
    for fn in ("user_warp_fwd", "user_warp_vjp", "user_warp_out_fwd", "user_warp_out_vjp"):
        assert fn + "(int type" in hdr
    for other in (R.make_test_scene2(), contrib.make_link_scene(), contrib.make_carved_scene()):
        assert "RM_USER_WARP" not in specialize.code_header(compile_scene(other))
    cs2 = pickle.loads(pickle.dumps(cs))
    assert cs2.user_warps == cs.user_warps and cs2.user_warp_sources == cs.user_warp_sources
    assert specialize.code_header(cs2) == hdr and specialize.scene_hash(cs2) == specialize.scene_hash(cs)
    cs3 = copy.deepcopy(cs)
    assert cs3.user_warps == cs.user_warps and specialize.code_header(cs3) == hdr
    assert compile_scene(copy.deepcopy(scene)).signature == cs.signature
    assert compile_scene(pickle.loads(pickle.dumps(scene))).signature == cs.signature
    other = contrib.make_warped_scene()
    other.sdfs[1].sdf.origin.data += 0.5                       # parameter values are not part of the key
    assert specialize.scene_hash(compile_scene(other)) == specialize.scene_hash(cs)
    # ---- the UAffine twins: the built-in program with 7 -> 22, 8 -> 23 and no cull tests
    for name, make in _twin_factories().items():
        with environment(RM_CULL="0"):
            twin = compile_scene(make())
            user = compile_scene(with_uaffine(make()))         # (scene 2 has no affine node: its twin is itself, cull test included)
        if name != "scene2":
            assert user.signature == compile_scene(with_uaffine(make())).signature      # nothing left to cull
        want = twin.program.copy()
        is_push, is_pop = want[:, 0] == _abi.OP_AFFINE_PUSH, want[:, 0] == _abi.OP_AFFINE_POP
        want[is_push, 0], want[is_push, 3] = _abi.OP_USER_PUSH, 7
        want[is_pop, 0], want[is_pop, 3] = _abi.OP_USER_POP, 7 << 16
        assert user.program.tolist() == want.tolist() and user.leaf_names == twin.leaf_names, name
        assert len(user.user_warps) == (0 if name == "scene2" else 1) and (user.n_slots, user.stack_floats) == (twin.n_slots, twin.stack_floats)


def test_validator_rejects_broken_warp_frames():
    from ray_marching_amd import _abi, contrib
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.scene.primitives import SDFSphere
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A
    cs = compile_scene(contrib.SDFScale(A(contrib.SDFMirror(SDFSphere(0.3), 0.1), orientation=IDENT, translation=[0.1, 0.0, 0.0]), 0.5))
    assert cs.program.tolist() == [[22, 0, 0, 1], [7, 1, 0, 0], [22, 8, 1, 1], [1, 9, 0, 0], [23, 8, 1, 1 << 16], [8, 1, 0, 0],
                                   [23, 0, 0, (1 << 16) | 1]]
    assert (cs.n_params, cs.n_slots, cs.stack_floats) == (10, 1, 18)
    ok = lambda prog, slots=cs.n_slots, stack=cs.stack_floats: _abi.lib.rm_validate_program(
        prog.ctypes.data, prog.shape[0], cs.n_params, cs.n_derived, stack, slots)
    err = lambda: _abi.lib.rm_last_error().decode()
    assert ok(cs.program) == 0
    bad = np.delete(cs.program, 6, axis=0)                     # an unmatched PUSH
    assert ok(bad) == -2 and "unbalanced" in err()
    bad = np.delete(cs.program, 0, axis=0)                     # ... and an unmatched POP
    assert ok(bad) == -2 and "USER_POP without a USER_PUSH" in err()
    bad = cs.program.copy(); bad[[4, 5]] = bad[[5, 4]]         # frames that cross: the affine node closes inside the warp
    assert ok(bad) == -2 and "USER_POP without a USER_PUSH" in err()
    bad = cs.program.copy(); bad[4, 1] = 7                     # mismatched offsets
    assert ok(bad) == -2 and "does not match its USER_PUSH at instr 2" in err()
    bad = cs.program.copy(); bad[4, 2] = 0                     # ... and types
    assert ok(bad) == -2 and "does not match its USER_PUSH" in err()
    bad = cs.program.copy(); bad[6, 3] = (2 << 16) | 1         # ... and parameter counts
    assert ok(bad) == -2 and "does not match its USER_PUSH" in err()
    bad = cs.program.copy(); bad[2, 1] = bad[4, 1] = cs.n_params      # theta outside the block
    assert ok(bad) == -2 and "user warp params out of range" in err()
    bad = cs.program.copy(); bad[2, 3], bad[4, 3] = 3, 3 << 16        # 8 + 3 > 10
    assert ok(bad) == -2 and "user warp params out of range" in err()
    bad = cs.program.copy(); bad[6, 3] = (1 << 16) | 2         # a value slot >= n_slots
    assert ok(bad) == -2 and "USER_POP value slot 1 out of range" in err()
    assert ok(cs.program, slots=0) == -2 and "value slot" in err()
    assert ok(cs.program, stack=17) == -2 and "stack_floats" in err()      # a warp frame costs 6 floats, like an affine one


def test_repeat_points_leave_out_at_most_one_percent():
    for which in REPEAT_PERIODS:
        pts, left_out = operator_points(which)
        print(f"{which}: {left_out} of 4096 points lie within 1e-4 of a cell border and are left out")
        assert left_out <= 40 and pts.shape[0] == 4096 - left_out
        period = torch.tensor(REPEAT_PERIODS[which])
        cell = (pts / period).round()
        assert ((pts - (cell - 0.5) * period).abs().min() >= 1e-4) and ((pts - (cell + 0.5) * period).abs().min() >= 1e-4)


def test_specialised_library_cross_compiles_and_reports_its_warps(monkeypatch, tmp_path):
    from concurrent.futures import ThreadPoolExecutor
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.scene.scene_registry import make_test_scene2
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    _register()
    programs = gpu_test_programs()
    # (one pool for every library of the GPU legs: hipcc takes 15-40 s each)
    with ThreadPoolExecutor(max_workers=4) as ex:
        paths = list(ex.map(specialize.build, programs + [compile_scene(contrib.make_warped_scene()), compile_scene(contrib.make_carved_scene()),
                                                          compile_scene(contrib.make_link_scene()), compile_scene(make_test_scene2())]))
    assert all(os.path.isfile(p) for p in paths)
    monkeypatch.setenv("RM_SPECIALIZE", "prebuilt")
    specialize._loaded.clear()
    for cs in programs:
        lib = cs.lib()
        assert lib.rm_user_warps() == len(cs.user_warps) and lib.rm_user_combinators() == len(cs.user_combinators)
        assert lib.rm_user_leaves() == 0 and lib.rm_abi_version() == _abi.ABI_VERSION
    assert sorted({len(cs.user_warps) for cs in programs}) == [0, 1, 4]
    cs = compile_scene(contrib.make_warped_scene())
    lib = cs.lib()
    assert lib is not _abi.lib and (lib.rm_user_warps(), lib.rm_user_combinators(), lib.rm_user_leaves()) == (4, 1, 0)
    assert cs.lib(True) is lib and cs.specialised
    assert _abi.lib.rm_user_warps() == 0 and _abi.fast_lib().rm_user_warps() == 0
    plain = compile_scene(make_test_scene2())
    assert plain.specialised and plain.lib().rm_user_warps() == 0                 # a specialised library of built-in nodes
    assert compile_scene(contrib.make_link_scene()).lib().rm_user_warps() == 0
    assert compile_scene(contrib.make_carved_scene()).lib().rm_user_warps() == 0
    assert "rm_user_warps" in _abi.EXPORTED_SYMBOLS
    # the interpreter is never an option
    monkeypatch.setenv("RM_SPECIALIZE", "off")
    with pytest.raises(_abi.RmError, match=r"combinators: sdf_intersection; warps: sdf_mirror, sdf_scale, sdf_elongate, sdf_repeat"):
        compile_scene(contrib.make_warped_scene()).lib()
    from ray_marching_amd.scene.primitives import SDFSphere
    with pytest.raises(_abi.RmError, match=r"user-defined warps \(sdf_mirror\)"):
        compile_scene(contrib.SDFMirror(SDFSphere(0.3), 0.0)).lib()
    with pytest.raises(_abi.RmError, match=r"user-defined leaves \(link\)"):      # leaf-only scenes read as they did
        compile_scene(contrib.make_link_scene()).lib()
    monkeypatch.setattr(specialize, "SPEC_DIR", str(tmp_path))
    monkeypatch.setenv("RM_SPECIALIZE", "prebuilt")
    specialize._loaded.clear()
    with pytest.raises(_abi.RmError, match="librm_spec_"):
        compile_scene(contrib.make_warped_scene()).lib()
    monkeypatch.setenv("RM_STATIC_BACKWARD_ACC", "8")
    with pytest.raises(_abi.RmError, match="RM_STATIC_BACKWARD_ACC"):
        compile_scene(contrib.make_warped_scene()).lib(True)
    monkeypatch.delenv("RM_STATIC_BACKWARD_ACC")
    # a warp that does not compile: hipcc's own words reach the caller
    from ray_marching_amd.extensions import register_warp

    class Broken(_Unary):
        def warp(self, points):
            return points

    register_warp(Broken, hip=UNARY.replace("NAME", "broken_warp").replace("return p;", "return no_such_helper(p);"))
    monkeypatch.setenv("RM_SPECIALIZE", "jit")
    with pytest.raises(_abi.RmError, match="no_such_helper"):
        compile_scene(Broken(SDFSphere(0.3))).lib()
    specialize._loaded.clear()


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scene2", "closed_scene1", "scene2_placed"])
def test_restated_affine_is_bit_identical_with_the_builtin(which, monkeypatch):
    """Zero tolerance: UAffine restates RM_OP_AFFINE_PUSH's map and VJP, so a scene with it in place of every
    SDFAffineTransformation and the built-in scene -- compiled without cull tests and by default: culling changes no bit, and
    the twin has lost its cull tests -- agree in every bit of scene(points), its gradients, the frames of all eight modes,
    p_final and the parameter and pose gradients of a Lambertian MSE step.  Every ray is walked in place (no deferred-ray
    list, whose atomically ordered partial sums are the one thing here that is not a function of the program), so the
    gradients are compared with torch.equal as well.  make_test_scene2() has no affine node: its twin is the scene itself
    and the case only pins that down; `scene2_placed` is scene 2 with its sphere and torus placed by affine nodes."""
    from ray_marching_amd import ops
    from ray_marching_amd.compiler import compiled_for
    from ray_marching_amd.rendering.ray_marching import SDFMarcher
    _register()
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)
    make = _twin_factories()[which]
    user = with_uaffine(make()).to(DEV)
    lib = compiled_for(user).lib()
    assert lib.rm_user_warps() == (0 if which == "scene2" else 1) and lib.rm_user_leaves() == 0 and lib.rm_user_combinators() == 0
    assert not (compiled_for(user).program[:, 0] == 17).any() or which == "scene2"
    pts = _points(4096, seed=11).to(DEV)
    h, w, steps = 40, 56, 24
    cams = [_pose(-3.0), (torch.nn.functional.normalize(torch.tensor([[1.0, 0.05, -0.1, 0.02]]), dim=-1).to(DEV),
                          torch.tensor([[0.3, -0.2, -2.0]], device=DEV))]

    def everything(scene):
        p = pts.clone().requires_grad_(True)
        d = scene(p)
        d.sum().backward()
        out = dict(d=d.detach(), gp=p.grad, gw=[x.grad.clone() for x in scene.parameters()], frames=[], final=[])
        for kw in (dict(), dict(early_out=False), dict(regen=True)):
            loop = H.make_loop(scene, h, w, **kw)
            for q, t in cams:
                with torch.no_grad():
                    out["frames"] += [loop(q, t, mode, 2, steps) for mode in range(8)]
        loop = H.make_loop(scene, h, w)
        for q, t in cams:
            with torch.no_grad():
                pos, _, _, dirs = loop.camera(q, t)
                out["final"].append(SDFMarcher(scene)(pos, dirs, steps))
        for x in scene.parameters():
            x.grad = None
        loop = H.make_loop(scene, 32, 32)
        q, t = _pose(-1.0 if which == "closed_scene1" else -3.0)
        q.requires_grad_(True); t.requires_grad_(True)
        loop(q, t, 0, 1, 16).pow(2).mean().backward()
        out["gf"] = [x.grad.clone() for x in scene.parameters()] + [q.grad, t.grad]
        return out

    got = everything(user)
    for env in TWIN_ENVS:
        twin = compiled_under(make(), env).to(DEV)
        assert compiled_for(twin).specialised and [n for n, _ in user.named_parameters()] == [n for n, _ in twin.named_parameters()]
        want = everything(twin)
        assert torch.equal(got["d"], want["d"]) and torch.equal(got["gp"], want["gp"]), env
        for key in ("frames", "final"):
            for i, (a, b) in enumerate(zip(got[key], want[key])):
                assert _same(a, b), (env, key, i)
        for key in ("gw", "gf"):
            for i, (a, b) in enumerate(zip(got[key], want[key])):
                print(f"{which} {env} {key}[{i}]: max|diff| {(a - b).abs().max().item():.3g} (|g| {b.abs().max().item():.3g})")
            for i, (a, b) in enumerate(zip(got[key], want[key])):
                assert _same(a, b), (env, key, i)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scale", "mirror", "repeat", "elongate", "warped"])
def test_operator_against_cpu_autograd_and_the_stand_alone_modules(which, monkeypatch):
    """Each shipped operator over a placed primitive, and contrib.make_warped_scene() (library prebuilt by build()), against
    cpu_eval(): every bit of the values at 4096 random points (restated math mode of the oracle: host independent); point and
    parameter gradients <= 1e-4 against CPU autograd (the contract of smoke()); every bit of the march's final positions and
    of the frame (modes 0 and 4) against the oracle's own render on the CPU, restated mode, with cpu_eval as its distance
    function; RenderLoop == the stand-alone chain in every bit; capture == the frame.  For the scenes with an SDFRepeat the
    points within 1e-4 of a cell border are left out (test_repeat_points_leave_out_at_most_one_percent: 2 of 4096 for
    `repeat`, 4 for `warped`)."""
    from ray_marching_amd.compiler import compiled_for
    scene = operator_scenes()[which]()
    spec = spec_of(scene)
    scene = scene.to(DEV)
    cs = compiled_for(scene)
    assert cs.lib().rm_user_warps() == len(cs.user_warps) == (4 if which == "warped" else 1)
    pts, left_out = operator_points(which)
    assert left_out <= 40
    with torch.no_grad(), O.math_mode("restated"):
        exact = cpu_eval(spec, pts)
    wts = torch.randn(pts.shape[0], 1, generator=torch.Generator().manual_seed(22))
    pc = pts.clone().requires_grad_(True)
    want = cpu_eval(spec, pc)
    (want * wts).sum().backward()
    pg = pts.to(DEV).requires_grad_(True)
    got = scene(pg)
    (got * wts.to(DEV)).sum().backward()
    n_diff = int((got.detach().cpu() != exact).sum())
    print(f"{which}: {n_diff} of {pts.shape[0]} values not bit-identical with the CPU composition (max|err| "
          f"{(got.detach().cpu() - exact).abs().max().item():.3g}); {left_out} points left out")
    assert _same(got.detach().cpu(), exact)
    gerr = (pg.grad.cpu() - pc.grad).abs().max().item()
    print(f"{which}: point gradient max|err| {gerr:.3g}")
    assert gerr <= 1e-4
    cpu_params = cpu_parameters(spec)
    names = [n for n, _ in scene.named_parameters()]
    assert len(cpu_params) == len(names)
    own = 0.0
    for (name, g), c in zip(scene.named_parameters(), cpu_params):
        assert g.shape == c.shape, name
        cg = c.grad if c.grad is not None else torch.zeros_like(c)
        e = (g.grad.cpu() - cg).abs().max().item()
        print(f"{which}: grad {name} max|err| {e:.3g} (|g| {cg.abs().max().item():.3g})")
        assert e <= 1e-4, name
        if name.rsplit(".", 1)[-1] in ("scale", "origin", "period", "halfsides"):
            own = max(own, cg.abs().max().item())
    assert own > 1e-3, "the operator's own parameters take part on too few points for this test to mean anything"
    # RenderLoop == camera -> SDFMarcher -> scene / SDFNormals -> Shader, the package's own stand-alone modules
    h, w, steps = 64, 96, 32
    loop = H.make_loop(scene, h, w)
    q, t = _pose(-3.0)
    with torch.no_grad():
        pos, frames, _, dirs = loop.camera(q, t)
    for mode in (0, 4):
        with torch.no_grad():
            frame = loop(q, t, mode, 1, steps)
            p = loop.marcher(pos, dirs, steps)
            n, lap = loop.normals(p)
            img = loop.shader(pos, q, frames, dirs, p, n, lap, loop.scene(p), mode=mode, degree=1)
        assert _same(frame, img.expand(frame.shape)), mode
    with torch.no_grad():
        frame = loop(q, t, 0, 1, steps)
        assert _same(loop.capture(mode=0, marching_steps=steps)(q, t), frame)
    # ... and against the CPU: the oracle's camera, march, normals and shader around cpu_eval, every bit
    bufs = O.camera_buffers(1, w, h, H.PX * h, H.PX * w, H.PX * h)
    for mode in (0, 4):
        with torch.no_grad(), O.math_mode("restated"):
            img, aux = cpu_render(spec, monkeypatch, bufs, q.cpu(), t.cpu(), mode, 1, steps, H.EPS, return_aux=True)
        with torch.no_grad():
            frame = loop(q, t, mode, 1, steps).cpu()
            p_gpu = loop.marcher(pos, dirs, steps).cpu()
        p_cpu = aux["p"].reshape(p_gpu.shape)
        n_p = int((torch.nan_to_num(p_gpu, nan=-7.0) != torch.nan_to_num(p_cpu, nan=-7.0)).sum())
        n_f = int((torch.nan_to_num(frame, nan=-7.0) != torch.nan_to_num(img, nan=-7.0)).sum())
        print(f"{which} mode {mode}: {n_p} of {p_gpu.numel()} final coordinates and {n_f} of {frame.numel()} frame values not "
              f"bit-identical with the CPU render")
        assert _same(p_gpu, p_cpu), mode
        assert _same(frame, img), mode


@pytest.mark.gpu
def test_nested_warps_through_the_replayed_tail(monkeypatch):
    """A warp inside a warp (Scale over Mirror, Mirror over a test-local warp with an ``out`` and three parameters over
    Elongate) inside a smooth union inside an SDFIntersection.  Values <= 1e-5 and gradients <= 1e-4 against CPU autograd, as
    for the carved scene.  Then the reverse march of a frame twice: with the converged tail (one point-gradient pass at the
    anchor, then vjp_replay over the tape it left -- the `out` slot is read a second time) and without it (early_out=False: a
    full VJP at every step).  The tile costs show which path ran.  Bit equality cannot hold between the two (the tail evaluates
    the VJP at an anchor at most 1e-6 max(1, |p|) away and sums the upstream first), so each parameter's gradient is held to
    1e-5 max(1, |g|), the bound tests/test_user_combinator.py puts on two paths that differ in summation order; the loss is a
    sum over the pixels, so that the bound is a relative one.  A value slot that the first reverse pass had clobbered, or that
    was never recorded, shows in the parameters of the two `out`s, whose gradients are g times the slot's content."""
    from ray_marching_amd import ops
    from ray_marching_amd.compiler import compiled_for
    _register()
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)
    scene = nesting_scene()
    spec = spec_of(scene)
    scene = scene.to(DEV)
    assert compiled_for(scene).lib().rm_user_warps() == 4 and compiled_for(scene).lib().rm_user_combinators() == 1
    pts = _points(4096, seed=51, lo=-2.0, hi=2.0)
    wts = torch.randn(4096, 1, generator=torch.Generator().manual_seed(52))
    pc = pts.clone().requires_grad_(True)
    want = cpu_eval(spec, pc)
    (want * wts).sum().backward()
    pg = pts.to(DEV).requires_grad_(True)
    got = scene(pg)
    (got * wts.to(DEV)).sum().backward()
    err = (got.detach().cpu() - want.detach()).abs().max().item()
    gerr = (pg.grad.cpu() - pc.grad).abs().max().item()
    print(f"nested warps: values max|err| {err:.3g}, point gradient max|err| {gerr:.3g}")
    assert err <= 1e-5 and gerr <= 1e-4
    for (name, g), c in zip(scene.named_parameters(), cpu_parameters(spec)):
        cg = c.grad if c.grad is not None else torch.zeros_like(c)
        e = (g.grad.cpu() - cg).abs().max().item()
        print(f"nested warps: grad {name} max|err| {e:.3g} (|g| {cg.abs().max().item():.3g})")
        assert e <= 1e-4, name
    h, w, steps = 64, 64, 48
    q, t = _pose(-3.0)
    target = torch.rand(1, h, w, 1, generator=torch.Generator().manual_seed(5)).to(DEV)
    grads, cost = {}, {}
    for early in (True, False):
        loop = H.make_loop(scene, h, w, early_out=early)
        sink = torch.zeros(int(ops._lib.rm_wave_tiles(1, h, w, 2)), dtype=torch.int32, device=DEV)
        monkeypatch.setattr(ops, "bwd_tile_cost_sink", sink)
        for x in scene.parameters():
            x.grad = None
        (loop(q, t, 0, 1, steps)[..., :1] - target).pow(2).sum().backward()      # (a sum: gradients of order 1 and above)
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "bwd_tile_cost_sink", None)
        grads[early] = {name: x.grad.clone() for name, x in scene.named_parameters()}
        cost[early] = float(sink.float().sum())
    print(f"nested warps: reverse-march tile cost with the tail {cost[True]:.0f}, without {cost[False]:.0f}")
    assert 0 < cost[True] < 0.5 * cost[False], "the converged tail (vjp_replay) was not taken"
    # the parameters of the two `out`s must get a real gradient through the replayed path: d(out)/d(scale) and d(out)/d(bc[0])
    # are g times the child's value, which the replay reads from the value slot the point-gradient pass left (UShear's child is
    # not 0 on the surface, see the class)
    outs = [n for n in grads[True] if n.endswith(".scale") or n.endswith(".bc")]
    assert len(outs) == 2, outs
    bad = []
    for name in grads[True]:
        a, b = grads[True][name], grads[False][name]
        e, g = (a - b).abs().max().item(), b.abs().max().item()
        print(f"nested warps: replayed vs per-step grad {name} max|diff| {e:.3g} (|g| {g:.3g}, bound {1e-5 * max(1.0, g):.3g})")
        if not (bool(torch.isfinite(a).all()) and e <= 1e-5 * max(1.0, g)):
            bad.append(name)
        if name in outs and not a.abs().min().item() > 1e-2:
            bad.append(name + ": no gradient through the `out`")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nested", "tight_neighbour"])
def test_culling_around_and_inside_a_warp_changes_no_bit(case, monkeypatch):
    """`nested`: a CULL_MIN in front of a built-in sibling of a warped subtree and one INSIDE the warp's frame, none over the
    warp.  `tight_neighbour`: a stiff smooth union whose bound table (RM_CULL_LSE=1) has an entry per child; the scaled
    sphere's must say "unbounded" -- it is the case that fails when subtree_bound has no case for RM_OP_USER_POP.  Compiled
    without cull tests and with them, values, gradients and frames are the same bits."""
    from ray_marching_amd import _abi, ops
    from ray_marching_amd.compiler import compiled_for
    _register()
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)      # bitwise parameter gradients: no atomically ordered deferred-ray list
    gen = torch.Generator().manual_seed(5)
    centres = (torch.rand(64, 1, 3, generator=gen) * 2 - 1) * 2.5
    if case == "tight_neighbour":      # half of the waves on the scaled sphere, next to the neighbour
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
        assert cs.lib().rm_user_warps() == 1
        p = pts.clone().requires_grad_(True)
        d = scene(p)
        (d * wts).sum().backward()
        gw = [x.grad.clone() for x in scene.parameters()]
        loop = H.make_loop(scene, 40, 72)
        q, t = _pose(-3.5)
        if case == "tight_neighbour":      # close to the scaled sphere's top, looking at it
            t = torch.tensor([[TIGHT_END[0], TIGHT_END[1], -1.5]], device=DEV)
        with torch.no_grad():
            frames = [loop(q, t, m, 1, 48) for m in (0, 4, 2, 5)]
        for x in scene.parameters():
            x.grad = None
        loop(q, t, 0, 1, 24).pow(2).mean().backward()
        res.append(dict(env=env, n_cull=n_cull, d=d.detach(), gp=p.grad, frames=frames, gw=gw,
                        gf=[x.grad.clone() for x in scene.parameters()]))
    print(f"culling leg {case}: cull instructions per variant {[r['n_cull'] for r in res]}")
    assert res[0]["n_cull"] == 0
    if case == "nested":
        assert res[1]["n_cull"] == 2
    else:
        assert res[2]["n_cull"] >= 8, "RM_CULL_LSE=1 did not put a cull test in front of the blob's children"
        near = (pts.cpu() - torch.tensor(TIGHT_END)).norm(dim=-1) < 0.1
        assert int(near.sum()) > 1000 and res[0]["d"].cpu()[near].abs().max().item() < 0.12      # those waves ARE at the surface
    ref = res[0]
    for got in res[1:]:
        assert _same(ref["d"], got["d"]) and _same(ref["gp"], got["gp"]), got["env"]
        for x, y in zip(ref["frames"], got["frames"]):
            assert _same(x, y), got["env"]
        for name in ("gw", "gf"):
            for x, y in zip(ref[name], got[name]):
                assert _same(x, y), (got["env"], name)


@pytest.mark.gpu
def test_training_step_moves_a_perturbed_warped_scene_back():
    """20 Adam steps on SDFMirror.origin, SDFScale.scale and the pose of the scaled torus, towards a frame of the unperturbed
    scene: each replayed step of the captured graph gives the loss of the eager step taken from the same parameters
    (tolerance of test_training_step_helper_matches_the_eager_loop), and the last loss is below the first.  The loss is the
    MSE of the normal-shader image (mode 4), as in the carved scene's training leg.

    Adam's eps is 1e-3, not its default 1e-8: with the default every coordinate moves by the full learning rate whatever the size
    of its gradient, the loss zigzags around 0.020 for a dozen steps, and from step 8 on the summation order of the deferred-ray
    list -- 4.8e-7 in the first step's gradients, tests/test_deferred_backward.py -- decided whether it had come down by step 20
    (in place: 0.0176; through the list: 0.0201, above the first replayed step's 0.0199).  With 1e-3 the coordinates whose gradient
    is below that stay put, the loss falls steadily from 0.0201 to 0.0141, and the in-place walk and the list give the same
    twenty losses to six digits."""
    from ray_marching_amd.contrib import make_warped_scene
    h, w, steps = 64, 96, 32
    q, t = _pose(-3.0)
    with torch.no_grad():
        target = H.make_loop(make_warped_scene(), h, w)(q, t, 4, 1, steps).clone()
    loss_fn = lambda image: (image - target).pow(2).mean()

    def perturbed():
        scene = make_warped_scene().to(DEV)
        mirror = scene.sdfs[1].sdf
        placed = mirror.sdf.sdfs[0]
        with torch.no_grad():
            mirror.origin += 0.05
            placed.sdf.scale += 0.05
            placed.translation += torch.tensor([0.04, -0.03, 0.03], device=DEV)
        return scene, [mirror.origin, placed.sdf.scale, placed.translation, placed.orientation]

    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*AccumulateGrad node's stream does not match.*")
        scene, moving = perturbed()
        loop = H.make_loop(scene, h, w)
        opt = torch.optim.Adam(moving, lr=2e-3, eps=1e-3, capturable=True)
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
