"""Bounds of user-defined domain operators (`RM_DEV void NAME_bound(const float* theta, rm::LeafBound& b)` in a warp's HIP
source: the child's bound in, the node's bound out; ray_marching_amd/extensions.py): registration, the programs the compiler
emits once a warped subtree is boundable, the generated `user_warp_bound` dispatch and its guard RM_USER_WARP_BOUNDS, the
shipped bounds against the operators' own PyTorch forward, and -- on the GPU -- bit identity with a built-in twin (UBAffine
restates SDFAffineTransformation AND the arithmetic of RM_OP_AFFINE_POP's bound), hand-computed bounds, that the cull tests
which now cover a warped subtree change no bit, that the bound follows the live parameters, and that it is really consumed
(a warp that lies about its sphere is skipped where it should not be, and `extensions.check_bound` says where).

Zero tolerance wherever two programs of one scene are compared: a correct bound changes no bit.

The GPU legs launch nine libraries of their own (the two UBAffine twins, four variants of cull_scene(), chain(), the lying
warp alone and in its union) and the two built-in twins that tests/test_user_warp.py builds as well.
"""
import copy
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import helpers as H
from tests.helpers import _points, _pose, _same
from tests.test_user_leaf_bounds import CULL_OFF, _compile, _on_device
from tests.test_user_warp import IDENT, Q_ROT, TIGHT_END, UAFFINE_HIP, UAffine, _Unary, scene2_placed

DEV = "cuda"


# --------------------------------------------------------------------------------------------------------------
# test-defined nodes
# --------------------------------------------------------------------------------------------------------------
class UBAffine(UAffine):
    """tests/test_user_warp.py's UAffine plus the bound of the built-in affine node: ubaffine_bound restates the case
    RM_OP_AFFINE_POP of subtree_bound (csrc/rm_device.h) operation for operation, so every derived constant of a scene built
    with it -- and with them every cull decision -- is the built-in scene's."""


UBAFFINE_HIP = UAFFINE_HIP.replace("uaffine_", "ubaffine_") + """
RM_DEV void ubaffine_bound(const float* theta, rm::LeafBound& b) {
  const float inf = __builtin_inff();
  const float* a = theta;
  float w4 = a[3];
  V3 qv = mk3(a[4], a[5], a[6]);
  float s2 = ((w4 * w4 + qv.x * qv.x) + qv.y * qv.y) + qv.z * qv.z;
  float sigma = fminf(1.0f, 2.0f * s2 - 1.0f) - 1e-5f;
  if (!(sigma > 0.5f) || !(s2 < 4.0f)) { b.R = b.Ru = inf; return; }
  V3 c0 = mk3(b.c.x, b.c.y, b.c.z);
  V3 c1 = qrot(c0, w4, qv);
  V3 back = qrot(c1, w4, neg(qv)) - c0;
  float e = sqrtf((back.x * back.x + back.y * back.y) + back.z * back.z);
  b.c.x = c1.x + a[0]; b.c.y = c1.y + a[1]; b.c.z = c1.z + a[2];
  b.R = (b.R + e) * 1.0001f + 1e-4f * (fabsf(b.c.x) + fabsf(b.c.y) + fabsf(b.c.z));
  b.slope = b.slope * sigma;
  b.Ru = (b.Ru + b.uslope * e) * 1.0001f + 1e-4f * (fabsf(b.c.x) + fabsf(b.c.y) + fabsf(b.c.z));
  b.uslope = b.uslope * (fmaxf(1.0f, 2.0f * s2 - 1.0f) + 1e-5f);
}
"""


class Same(_Unary):
    """The identity map; the base of the test-local warps below."""

    def warp(self, points):
        return points


class Plain(Same):
    """... without a bound."""


class LiarWarp(Same):
    """The identity map that signs a sphere of 0.1 around (40, 0, 0), whatever its child's was: a wrong bound, on purpose.
    Wrong numbers only: evaluation only, every access in range."""


SAME_HIP = ("template <bool Fast> RM_DEV rm::V3 NAME_fwd(rm::V3 p, const float* theta) { return p; }\n"
            "template <bool Fast> RM_DEV void NAME_vjp(rm::V3 p, const float* theta, rm::V3 gq, rm::V3& gp, float* gtheta) { gp = gp + gq; }\n")
BOUND_KEEP = "RM_DEV void NAME_bound(const float* theta, rm::LeafBound& b) {}\n"          # the identity map: the child's bound as it is
LIAR_HIP = SAME_HIP.replace("NAME", "liarwarp") + """
RM_DEV void liarwarp_bound(const float* theta, rm::LeafBound& b) { b.c = mk3(40.0f, 0.0f, 0.0f); b.R = b.Ru = 0.1f; b.slope = b.uslope = 1.0f; }
"""


class WBall(nn.Module):
    """A ball of ``radius`` around ``centre``: the bounded leaf whose known sphere the shipped operators' bounds are applied to
    on the CPU."""

    def __init__(self, centre, radius):
        super().__init__()
        self.centre = nn.Parameter(torch.tensor(centre, dtype=torch.float32))
        self.radius = nn.Parameter(torch.tensor(radius, dtype=torch.float32))

    def forward(self, query_positions):
        return torch.linalg.vector_norm(query_positions - self.centre, dim=-1, keepdim=True) - self.radius


WBALL_HIP = """
template <bool Fast> RM_DEV float wball_fwd(rm::V3 p, const float* theta) { return norm3_t<Fast>(p - mk3(theta[0], theta[1], theta[2])) - theta[3]; }
template <bool Fast> RM_DEV void wball_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) {
  const rm::V3 v = p - mk3(theta[0], theta[1], theta[2]);
  const float n = norm3_t<Fast>(v);
  const float s = (n == 0.0f) ? 0.0f : div_t<Fast>(g, n);
  gp = gp + mk3(v.x * s, v.y * s, v.z * s);
  gtheta[0] = -v.x * s; gtheta[1] = -v.y * s; gtheta[2] = -v.z * s; gtheta[3] = -g;
}
RM_DEV void wball_bound(const float* theta, rm::LeafBound& b) {
  if (theta[3] >= 0.0f) { b.c = mk3(theta[0], theta[1], theta[2]); b.R = b.Ru = theta[3]; }
}
"""


def _register():
    from ray_marching_amd.extensions import register_leaf, register_warp
    register_warp(UBAffine, params=("translation", "orientation"), hip=UBAFFINE_HIP, cost=25)      # the affine node's cost: the twins' programs must agree
    register_warp(Same, hip=SAME_HIP.replace("NAME", "wb_same") + BOUND_KEEP.replace("NAME", "wb_same"), cost=40)
    register_warp(Plain, hip=SAME_HIP.replace("NAME", "wb_plain"), cost=40)
    register_warp(LiarWarp, hip=LIAR_HIP, cost=40)                  # (compiler._CULL_MIN_CHILD_COST: gets a site of its own)
    register_leaf(WBall, params=("centre", "radius"), hip=WBALL_HIP, cost=16)


# --------------------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------------------
def with_ubaffine(module):
    """A deep copy of the scene with every SDFAffineTransformation replaced by a UBAffine of the same pose."""
    from ray_marching_amd.scene.transformations import SDFAffineTransformation

    def swap(m):
        for name, child in list(m._modules.items()):
            m._modules[name] = swap(child)
        if isinstance(m, SDFAffineTransformation):
            return UBAffine(m.sdf, m.orientation.detach().tolist(), m.translation.detach().tolist())
        return m

    return swap(copy.deepcopy(module))


def _twin_factories():
    from ray_marching_amd.scene.scene_registry import make_closed_test_scene
    return {"scene2_placed": scene2_placed, "closed_scene1": make_closed_test_scene}


def scaled_torus_scene(scale_cls):
    """The room, a bounded built-in sibling and an affine-placed scaled torus."""
    from ray_marching_amd.scene.primitives import SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    return SDFUnion([make_room(), A(SDFTorus(radius1=0.5, radius2=0.12), orientation=[0.0, 0.5 ** 0.5, 0.5 ** 0.5, 0.0], translation=[1.1, 0.4, 1.5]),
                     A(scale_cls(SDFTorus(0.5, 0.12), scale=0.7), orientation=Q_ROT, translation=[-0.6, 0.1, 0.2])])


def cull_scene():
    """The scene of the culling and live-parameter legs.  `nested`: a mirrored min-union (a placed scaled torus, a sphere, an
    elongated sphere) under an affine node, next to the room and a bounded built-in sibling (the smooth union) -- cull tests
    over the mirror and, inside its frame, over the scaled torus (by default) or the elongated sphere (with a test in front
    of every child).  93 parameter floats: the backward stays specialised (specialize.MAX_STATIC_BACKWARD_ACC = 96; the
    interpreter has no handler for user warps).  `tight_neighbour`: the stiff smooth union of
    tests/test_user_warp.py's scaled_with_a_tight_neighbour() with the bounded scale (k = 300: a child is skipped from 0.35
    behind the nearest one); its bound table has a finite entry for the scaled sphere -- radius 0.8, not the child's 0.1 --
    and waves at TIGHT_END, on that sphere and 0.07 from the neighbour, show an entry that is too small."""
    from ray_marching_amd.contrib import SDFBoundedElongate, SDFBoundedMirror, SDFBoundedScale
    from ray_marching_amd.scene.primitives import SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFSmoothUnion, SDFUnion
    inner = SDFUnion([A(SDFBoundedScale(SDFTorus(0.5, 0.12), scale=0.8), orientation=IDENT, translation=[0.9, 0.3, 0.2]), SDFSphere(0.25),
                      SDFBoundedElongate(SDFSphere(0.2), halfsides=(0.05, 0.3, 0.1))])
    big = A(SDFBoundedScale(SDFSphere(0.1), scale=8.0), orientation=IDENT, translation=[TIGHT_END[0], 0.0, 0.0])
    neighbour = A(SDFSphere(0.05), orientation=IDENT, translation=[TIGHT_END[0], TIGHT_END[1] + 0.12, TIGHT_END[2]])
    far = [A(SDFSphere(r), orientation=q, translation=t) for r, q, t in (
        (0.3, IDENT, [-2.0, -1.5, 1.0]), (0.25, Q_ROT, [2.4, -1.0, 0.5]), (0.35, Q_ROT, [-1.5, 1.5, -1.0]), (0.25, IDENT, [0.0, -2.0, -1.5]),
        (0.3, IDENT, [2.2, 1.8, 1.5]), (0.2, IDENT, [-2.2, 0.0, 2.0]))]
    return SDFUnion([make_room(), A(SDFBoundedMirror(inner, origin=0.0), orientation=Q_ROT, translation=[-0.3, 0.1, -1.2]),
                     SDFSmoothUnion([big, neighbour] + far, blend_k=300.0)])


def cull_scene_warps(scene):
    """(the mirror, [the torus's scale, the big sphere's scale], the elongation) of a cull_scene()."""
    mirror = scene.sdfs[1].sdf
    return mirror, [mirror.sdf.sdfs[0].sdf, scene.sdfs[2].sdfs[0].sdf], mirror.sdf.sdfs[2]


LSE = dict(RM_CULL_LSE="1", RM_CULL_LSE_MIN="2")
CULL_LEGS = {"nested": [CULL_OFF, dict(), dict(RM_CULL_MIN_COST="0")], "tight_neighbour": [CULL_OFF, LSE]}


def chain(scale=1.7, t2=(0.2, -0.3, 0.5), origin=0.15, halfsides=(0.05, 0.3, 0.1), t1=(0.4, 0.1, -0.2), radius=0.3):
    """Every shipped bounded operator in one node, nested in each other and in an affine node, over a placed sphere:
    scale(affine(mirror(elongate(affine(sphere))))).  Identity quaternions: the affine rule of the walk is then centre + t,
    R -> 1.0001 R + 1e-4 |centre|_1, slopes times (1 -+ 1e-5), which chain_bound() restates."""
    from ray_marching_amd.contrib import SDFBoundedElongate, SDFBoundedMirror, SDFBoundedScale
    from ray_marching_amd.scene.primitives import SDFSphere
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A
    inner = SDFBoundedMirror(SDFBoundedElongate(A(SDFSphere(radius), orientation=IDENT, translation=list(t1)), halfsides=halfsides), origin=origin)
    return SDFBoundedScale(A(inner, orientation=IDENT, translation=list(t2)), scale=scale)


def chain_bound(scale=1.7, t2=(0.2, -0.3, 0.5), origin=0.15, halfsides=(0.05, 0.3, 0.1), t1=(0.4, 0.1, -0.2), radius=0.3):
    """(centre, R, slope, Ru, uslope) of chain() by hand: the operators' rules (contrib.py) between the factors the walk itself
    applies at an affine node (csrc/rm_device.h: RM_OP_AFFINE_POP, unit quaternion) and to |halfsides| (1.00001)."""
    l1 = lambda c: sum(abs(x) for x in c)
    c, slope, uslope = list(t1), 1.0 - 1e-5, 1.0 + 1e-5                       # affine over the sphere
    R = Ru = radius * 1.0001 + 1e-4 * l1(c)
    h = math.sqrt(sum(x * x for x in halfsides)) * 1.00001                    # elongate
    R, Ru = R + h, Ru + uslope * h
    R, Ru, c = R + abs(c[0]), Ru + uslope * abs(c[0]), [origin, c[1], c[2]]   # mirror
    c = [x + y for x, y in zip(c, t2)]                                        # affine
    R, Ru = R * 1.0001 + 1e-4 * l1(c), Ru * 1.0001 + 1e-4 * l1(c)
    slope, uslope = slope * (1.0 - 1e-5), uslope * (1.0 + 1e-5)
    return [scale * x for x in c], scale * R, slope, scale * Ru, uslope       # scale


# parameter sets of chain(): as built, then each operator alone (the other two are the identity map on the bound), then extremes
CHAIN_SETS = [dict(), dict(scale=2.5, origin=0.0, halfsides=(0.0, 0.0, 0.0), t1=(0.0, 0.1, -0.2)),
              dict(scale=1.0, origin=-0.35, halfsides=(0.0, 0.0, 0.0), t1=(0.6, 0.1, -0.2)),
              dict(scale=1.0, origin=0.0, halfsides=(0.4, 0.0, 0.25), t1=(0.0, 0.1, -0.2)),
              dict(scale=0.05, origin=1.5, halfsides=(1.0, 2.0, 0.5), t1=(-0.7, 0.0, 0.0), t2=(0.0, 0.0, 0.0), radius=0.01)]


def liar_scene():
    """A cheap child (no cull test: below the cost threshold), then the lying warp over a sphere of 0.5 behind its CULL_MIN."""
    from ray_marching_amd.scene.primitives import SDFSphere
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    return SDFUnion([A(SDFSphere(0.1), orientation=IDENT, translation=[3.0, 0.0, 0.0]), LiarWarp(SDFSphere(0.5))])


def gpu_test_programs():
    """Every test-defined program the GPU legs launch: build() compiles their libraries, so that a GPU run of the same tree
    finds them; the fixture `libraries` builds what is missing."""
    from ray_marching_amd import specialize
    from ray_marching_amd.scene.primitives import SDFSphere
    _register()
    out = []
    for make in _twin_factories().values():
        out += [_compile(lambda: with_ubaffine(make()), {}), _compile(make, {})]
    out += [_compile(cull_scene, env) for env in (CULL_OFF, {}, dict(RM_CULL_MIN_COST="0"), LSE)]
    out += [_compile(chain, {}), _compile(liar_scene, {}), _compile(lambda: LiarWarp(SDFSphere(0.5)), {})]
    return list({specialize.scene_hash(cs): cs for cs in out}.values())


def _sites_over_warps(program):
    """[(op, rows of USER_PUSH inside its range)] of the cull instructions whose skip range holds a USER_PUSH ... USER_POP pair."""
    from ray_marching_amd import _abi
    rows = np.asarray(program).reshape(-1, 4)
    found = []
    for i in np.flatnonzero((rows[:, 0] == _abi.OP_CULL_MIN) | (rows[:, 0] == _abi.OP_CULL_LSE)):
        n = int(rows[i, 3]) >> 8 if rows[i, 0] == _abi.OP_CULL_MIN else int(rows[i, 3])
        inside = rows[i + 1:i + n]
        pushes = [int(i) + 1 + int(j) for j in np.flatnonzero(inside[:, 0] == _abi.OP_USER_PUSH)]
        assert len(pushes) == int((inside[:, 0] == _abi.OP_USER_POP).sum()), "a cull range cuts a warp's frame in two"
        if pushes:
            found.append((int(rows[i, 0]), pushes))
    return found


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
def test_registration_of_a_warp_bound():
    from ray_marching_amd import contrib
    from ray_marching_amd.extensions import UserWarp, register_warp, warp_spec
    from ray_marching_amd.scene.primitives import SDFSphere
    _register()
    ball = SDFSphere(0.3)
    assert warp_spec(UBAffine(ball, IDENT, [0.0, 0.0, 0.0])).bounded and warp_spec(UBAffine(ball, IDENT, [0.0, 0.0, 0.0])).name == "ubaffine"
    assert warp_spec(Same(ball)).bounded and warp_spec(LiarWarp(ball)).bounded and not warp_spec(Plain(ball)).bounded
    assert UserWarp.__dataclass_fields__["bounded"].default is False and list(UserWarp.__dataclass_fields__)[-1] == "bounded"
    shipped = [contrib.SDFScale(ball, 0.5), contrib.SDFMirror(ball, 0.0), contrib.SDFRepeat(ball, (1.0, 1.0, 1.0)), contrib.SDFElongate(ball, (0.1, 0.1, 0.1))]
    assert [warp_spec(w).bounded for w in shipped] == [False] * 4
    bounded = [contrib.SDFBoundedScale(ball, 0.5), contrib.SDFBoundedMirror(ball, 0.0), contrib.SDFBoundedElongate(ball, (0.1, 0.1, 0.1))]
    assert [warp_spec(w).bounded for w in bounded] == [True] * 3
    assert [warp_spec(w).name for w in bounded] == ["sdf_bscale", "sdf_bmirror", "sdf_belongate"]
    assert [(warp_spec(w).has_out, warp_spec(w).cost, warp_spec(w).params) for w in bounded] == \
        [(warp_spec(w).has_out, warp_spec(w).cost, warp_spec(w).params) for w in shipped[:2] + shipped[3:]]
    # the bounded classes keep the PyTorch methods of their parents
    p = _points(64)
    for cls, arg in ((contrib.SDFScale, 0.5), (contrib.SDFMirror, 0.1), (contrib.SDFElongate, (0.1, 0.2, 0.3))):
        twin = getattr(contrib, cls.__name__.replace("SDF", "SDFBounded"))
        assert issubclass(twin, cls) and torch.equal(twin(WBall((0.4, 0.1, -0.2), 0.3), arg)(p), cls(WBall((0.4, 0.1, -0.2), 0.3), arg)(p))
    register_warp(UBAffine, params=("translation", "orientation"), hip=UBAFFINE_HIP, cost=25)            # the same again: fine
    with pytest.raises(ValueError, match="already registered"):                                         # the bound is part of the source
        register_warp(UBAffine, params=("translation", "orientation"), hip=UAFFINE_HIP.replace("uaffine_", "ubaffine_"), cost=25)

    class Fresh(_Unary):
        def warp(self, points):
            return points

    src, keep = SAME_HIP.replace("NAME", "wb_fresh"), BOUND_KEEP.replace("NAME", "wb_fresh")
    with pytest.raises(ValueError, match=r"the warp 'wb_fresh' must be .*wb_fresh_bound.*found wb_other_bound"):      # another NAME
        register_warp(Fresh, hip=src + BOUND_KEEP.replace("NAME", "wb_other"))
    with pytest.raises(ValueError, match=r"at most one.*the warp 'wb_fresh'"):
        register_warp(Fresh, hip=src + keep + keep)
    with pytest.raises(ValueError, match=r"the warp 'wb_fresh' must not be a template"):
        register_warp(Fresh, hip=src + keep.replace("RM_DEV void", "template <bool Fast> RM_DEV void"))
    with pytest.raises(ValueError, match="inline assembly"):                                            # the whole source is checked
        register_warp(Fresh, hip=src + keep.replace("{}", '{ asm volatile(""); }'))
    assert warp_spec(Fresh(ball)) is None                                                               # nothing of the above registered it
    register_warp(Fresh, hip=src + "// " + keep)                                                        # a bound in a comment is no bound
    assert warp_spec(Fresh(ball)).name == "wb_fresh" and not warp_spec(Fresh(ball)).bounded


def test_programs_of_bounded_warps():
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import _boundable, compile_scene
    from ray_marching_amd.scene.primitives import SDFPlane, SDFSphere
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as Aff
    import tests.test_user_warp as T
    _register()
    A = _abi
    ok = lambda cs: _abi.lib.rm_validate_program(cs.program.ctypes.data, cs.n_instr, cs.n_params, cs.n_derived, cs.stack_floats, cs.n_slots)
    assert _abi.ABI_VERSION == 14
    # ---- the room, a bounded sibling and a placed scaled torus: a CULL_MIN over the PUSH ... POP pair exactly when the scale signs a bound
    cs = _compile(lambda: scaled_torus_scene(contrib.SDFBoundedScale), {})
    rows = cs.program.reshape(-1, 4)
    sites = _sites_over_warps(cs.program)
    assert len(sites) == 1 and sites[0][0] == A.OP_CULL_MIN and len(sites[0][1]) == 1 and ok(cs) == 0
    push = sites[0][1][0]
    assert rows[push - 1, 0] == A.OP_AFFINE_PUSH and rows[push - 2, 0] == A.OP_CULL_MIN and rows[push + 2, 0] == A.OP_USER_POP
    assert cs.user_warps[0][:3] == ("sdf_bscale", 1, True) and len(cs.user_warps[0]) == 4 and cs.user_warp_bounded == (True,)
    assert cs.signature[-1] == cs.user_warps and len(cs.signature) == 9
    plain = _compile(lambda: scaled_torus_scene(contrib.SDFScale), {})
    assert not _sites_over_warps(plain.program) and plain.user_warp_bounded == (False,)
    assert int((plain.program[:, 0] == A.OP_CULL_MIN).sum()) == 1                                       # (the sibling keeps its own)
    # the unbounded twin is evaluated before every cullable sibling, the bounded one in the reference's child order
    first_user = lambda c: int(np.flatnonzero(c.program[:, 0] == A.OP_USER_PUSH)[0])
    first_cull = lambda c: int(np.flatnonzero(c.program[:, 0] == A.OP_CULL_MIN)[0])
    assert first_user(plain) < first_cull(plain) and first_cull(cs) < first_user(cs)
    assert not _sites_over_warps(_compile(lambda: scaled_torus_scene(contrib.SDFBoundedScale), CULL_OFF).program)
    # ---- a bounded warp is boundable exactly when its child is
    ball = lambda: SDFSphere(0.3)
    for cls, arg in ((contrib.SDFBoundedScale, 0.5), (contrib.SDFBoundedMirror, 0.1), (contrib.SDFBoundedElongate, (0.1, 0.2, 0.3))):
        assert _boundable(cls(ball(), arg)) and _boundable(cls(WBall((0.1, 0.0, 0.0), 0.3), arg))
        assert _boundable(cls(Aff(contrib.SDFBoundedMirror(contrib.SDFBoundedScale(ball(), 2.0), 0.0), orientation=IDENT, translation=[0.1, 0.0, 0.0]), arg))
        assert not _boundable(cls(SDFPlane(), arg))
        assert not _boundable(cls(contrib.SDFMirror(ball(), 0.0), arg)) and not _boundable(cls(Plain(ball()), arg))
        assert not _boundable(cls(contrib.SDFRepeat(ball(), (1.0, 1.0, 1.0)), arg))
        assert not _boundable(cls(contrib.SDFIntersection([ball(), ball()]), arg))
        assert not _boundable(cls(contrib.SDFLink(0.3, 0.3, 0.1), arg)) and _boundable(cls(contrib.SDFBoundedLink(0.3, 0.3, 0.1), arg))
    assert _boundable(Same(UBAffine(ball(), IDENT, [0.0, 0.0, 0.0]))) and not _boundable(Plain(contrib.SDFBoundedScale(ball(), 2.0)))
    T._register()
    for unbounded in (contrib.SDFScale(ball(), 0.5), contrib.SDFMirror(ball(), 0.0), contrib.SDFElongate(ball(), (0.1, 0.1, 0.1)), UAffine(ball(), IDENT, [0.0] * 3)):
        assert not _boundable(unbounded)
    # ---- the shipped scene keeps its program; its bounded variant has cull tests over the mirrored pair
    old = compile_scene(contrib.make_warped_scene())
    assert not (old.program[:, 0] == A.OP_CULL_MIN).any() and old.user_warp_bounded == (False,) * 4
    assert [w[0] for w in old.user_warps] == ["sdf_mirror", "sdf_scale", "sdf_elongate", "sdf_repeat"]
    new = compile_scene(contrib.make_warped_scene(bounded=True))
    sites = _sites_over_warps(new.program)
    assert [w[0] for w in new.user_warps] == ["sdf_repeat", "sdf_bmirror", "sdf_bscale", "sdf_belongate"] and ok(new) == 0
    assert new.user_warp_bounded == (False, True, True, True)
    assert len(sites) == 2 and all(op == A.OP_CULL_MIN for op, _ in sites), sites
    assert len(sites[0][1]) == 3 and len(sites[1][1]) == 1, "a test over the mirror (three frames inside), one inside it over a placed child"
    assert sorted(new.leaf_names) == sorted(old.leaf_names) and new.n_slots == old.n_slots and new.stack_floats == old.stack_floats
    # the intersection that holds the SDFRepeat stays uncullable, and is evaluated first now
    repeat_push = int(np.flatnonzero((new.program[:, 0] == A.OP_USER_PUSH) & (new.program[:, 2] == 0))[0])
    assert repeat_push < first_cull(new)
    # ---- the scene of the culling legs
    # (CULL_MINs over the mirror, over the placed scale inside it, and over the stiff smooth union; with a test in front of every
    # child the scaled torus is evaluated first and has none, the cheap sphere and the elongated one behind it get theirs)
    sites = {}
    for name, env, kinds in (("off", CULL_OFF, []), ("default", {}, [A.OP_CULL_MIN] * 3), ("eager", dict(RM_CULL_MIN_COST="0"), [A.OP_CULL_MIN] * 3),
                             ("lse", LSE, [A.OP_CULL_MIN] * 3 + [A.OP_CULL_LSE])):
        cs = _compile(cull_scene, env)
        sites[name] = _sites_over_warps(cs.program)
        assert sorted(op for op, _ in sites[name]) == sorted(kinds) and ok(cs) == 0, (env, sites[name])
        # the GPU legs take gradients: above the limit the backward would go to the interpreter, which has no handler for warps
        assert specialize.static_backward(cs) and cs.n_params + cs.n_grad_derived == 93, env
    assert sites["default"] != sites["eager"]
    for cs in gpu_test_programs():
        assert specialize.static_backward(cs)
    # the stiff smooth union is a cullable child of the root now, tested with its children's own bounds: it has a bound table
    rows = _compile(cull_scene, {}).program.reshape(-1, 4)
    sb = rows[rows[:, 0] == A.OP_SMOOTH_BEGIN]
    assert len(sb) == 1 and sb[0, 2] != 0 and (sb[0, 3] & 255) == 8 and any(r[0] == A.OP_CULL_MIN and r[1] == 1 for r in rows.tolist())
    old_tight = _compile(T.scaled_with_a_tight_neighbour, {}).program.reshape(-1, 4)
    assert not (old_tight[:, 0] == A.OP_CULL_MIN).any()                                                 # SDFScale stays as it was
    assert _sites_over_warps(_compile(liar_scene, {}).program) and not _sites_over_warps(_compile(liar_scene, CULL_OFF).program)
    # ---- bounded and unbounded sources differ in their sha1, hence in the library key; user_warp_bounded is no part of it
    a, b = compile_scene(contrib.SDFBoundedScale(ball(), 0.5)), compile_scene(contrib.SDFScale(ball(), 0.5))
    assert a.program.tolist() == b.program.tolist() and a.signature != b.signature and specialize.scene_hash(a) != specialize.scene_hash(b)
    assert a.user_warp_bounded not in a.signature and a.signature[-1] == a.user_warps


def test_restated_affine_bound_compiles_to_the_builtin_program():
    """UBAffine in place of every SDFAffineTransformation: the built-in program with 7 -> 22 and 8 -> 23 -- cull tests, their
    derived offsets and the order in which the children are evaluated included."""
    from ray_marching_amd import _abi
    _register()
    for env in ({}, dict(RM_CULL_MIN_COST="0"), LSE, CULL_OFF):
        for name, make in _twin_factories().items():
            twin, user = _compile(make, env), _compile(lambda: with_ubaffine(make()), env)
            want = twin.program.copy()
            is_push, is_pop = want[:, 0] == _abi.OP_AFFINE_PUSH, want[:, 0] == _abi.OP_AFFINE_POP
            assert is_push.any() and is_push.sum() == is_pop.sum()
            want[is_push, 0], want[is_push, 3] = _abi.OP_USER_PUSH, 7
            want[is_pop, 0], want[is_pop, 3] = _abi.OP_USER_POP, 7 << 16
            assert user.program.tolist() == want.tolist() and user.leaf_names == twin.leaf_names, (name, env)
            assert (user.n_derived, user.n_slots, user.stack_floats, user.n_grad_derived) == (twin.n_derived, twin.n_slots, twin.stack_floats, twin.n_grad_derived)
            assert user.user_warps[0][:3] == ("ubaffine", 7, False) and user.user_warp_bounded == (True,)
            n_cull = int(np.isin(twin.program[:, 0], (_abi.OP_CULL_MIN, _abi.OP_CULL_LSE)).sum())
            assert (n_cull > 0) == (env != CULL_OFF), (name, env)
            if env in ({}, LSE):       # (with a test in front of every child the closed scene's blob goes first, and has none)
                assert _sites_over_warps(user.program), (name, env)


def test_the_header_has_the_bound_dispatch_only_where_a_warp_is_bounded():
    from ray_marching_amd import contrib, specialize
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.scene.scene_registry import make_test_scene2
    from ray_marching_amd.scene.primitives import SDFSphere
    import tests.test_user_warp as T
    _register()
    T._register()
    hdr = specialize.code_header(compile_scene(contrib.make_warped_scene(bounded=True)))
    assert hdr.count("#define RM_USER_WARP_BOUNDS") == 1 and hdr.count("user_warp_bound(int type") == 1
    assert "sdf_repeat_bound" not in hdr                                                            # (type 0, the SDFRepeat: in no bound case)
    for t, name in ((1, "sdf_bmirror"), (2, "sdf_bscale"), (3, "sdf_belongate")):
        assert f"    case {t}: {name}_bound(theta, b); return true;\n" in hdr and f"RM_DEV void {name}_bound(" in hdr
    assert "    case 0: sdf_repeat_bound" not in hdr and hdr.index("#define RM_USER_WARP_BOUNDS") < hdr.index("#else")
    mixed = specialize.code_header(compile_scene(Plain(Same(SDFSphere(0.3)))))                      # one bounded type among two
    assert "case 1: wb_same_bound(theta, b); return true;" in mixed and "wb_plain_bound" not in mixed and "RM_USER_WARP_BOUNDS" in mixed
    unbounded = [contrib.make_warped_scene(), contrib.make_carved_scene(), contrib.make_link_scene(), contrib.make_link_scene(bounded=True),
                 make_test_scene2(), T.with_uaffine(scene2_placed()), T.nesting_scene(), Plain(SDFSphere(0.3))]
    for scene in unbounded:
        text = specialize.code_header(compile_scene(scene))
        assert "RM_USER_WARP_BOUNDS" not in text and "user_warp_bound" not in text and "_bound(theta, b); return" not in text
    # the header of the shipped scene is what it was before warps could sign a bound: sha1 at the parent commit
    import hashlib
    assert hashlib.sha1(specialize.code_header(compile_scene(contrib.make_warped_scene())).encode()).hexdigest() == PARENT_WARPED_HEADER
    # in the device header every line of the new walk sits behind the guard
    src = open(os.path.join(specialize.CSRC, "rm_device.h")).read()
    assert src.count("#ifdef RM_USER_WARP_BOUNDS") == 1 and src.count("user_warp_bound(") == 1
    guarded = src[src.index("#ifdef RM_USER_WARP_BOUNDS"):]
    guarded = guarded[:guarded.index("#else")]
    assert "user_warp_bound(w.z, P + off, b)" in guarded
    assert "      case RM_OP_USER_POP: --sp; cx = cy = cz = 0.0f; R = Ru = inf; slope = uslope = 1.0f; break;\n" in src


PARENT_WARPED_HEADER = "4efb8b9974f745f041133c101b1871d51208b8ea"


def _resource_usage(cs, tmp):
    """{mangled kernel name: scratch bytes per lane} of the scene's library, compiled as specialize.build does."""
    from ray_marching_amd import specialize
    os.makedirs(tmp, exist_ok=True)
    header = os.path.join(tmp, "code.h")
    with open(header, "w") as f:
        f.write(specialize.code_header(cs))
    cmd = [specialize._hipcc(), *specialize.variant("exact")[1], f'-DRM_STATIC_CODE="{header}"', "-Rpass-analysis=kernel-resource-usage",
           os.path.join(specialize.CSRC, "rm_abi.hip"), "-o", os.path.join(tmp, "lib.so")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=specialize.CSRC)
    assert r.returncode == 0, r.stderr[-3000:]
    scratch, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
    return scratch


def test_bounded_library_cross_compiles_without_new_scratch(monkeypatch, tmp_path):
    from concurrent.futures import ThreadPoolExecutor
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import compile_scene
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    _register()
    bounded, plain = compile_scene(contrib.make_warped_scene(bounded=True)), compile_scene(contrib.make_warped_scene())
    programs = gpu_test_programs()
    # (one pool for every library of the GPU legs and the two resource reports: hipcc takes 15-40 s each)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as ex:
        usage = [ex.submit(_resource_usage, cs, str(tmp_path / name)) for name, cs in (("bounded", bounded), ("plain", plain))]
        paths = list(ex.map(specialize.build, programs + [bounded]))
        usage = [u.result() for u in usage]
    assert all(os.path.isfile(p) for p in paths) and len(programs) == 11
    monkeypatch.setenv("RM_SPECIALIZE", "prebuilt")
    specialize._loaded.clear()
    lib = bounded.lib()
    assert lib is not _abi.lib and (lib.rm_user_warps(), lib.rm_user_combinators(), lib.rm_user_leaves()) == (4, 1, 0)
    assert lib.rm_abi_version() == _abi.ABI_VERSION == 14
    for cs in programs:
        assert cs.lib().rm_user_warps() == len(cs.user_warps) and cs.lib().rm_user_leaves() == 0
    specialize._loaded.clear()
    with_scratch = {k: v for k, v in usage[0].items() if v > 0}
    print(f"kernels of the bounded library: {len(usage[0])}, with scratch: {with_scratch}; of the unbounded twin: "
          f"{ {k: v for k, v in usage[1].items() if v > 0} }")
    assert len(usage[0]) >= 10 and set(usage[0]) == set(usage[1])
    assert not [k for k, v in usage[0].items() if v > usage[1][k]], "a kernel of the bounded library uses scratch its unbounded twin does not"


def _restated(node, child_bound):
    """The bound contrib.py's HIP signs for a shipped bounded operator, restated: (c, R, slope, Ru, uslope) of the child in."""
    from ray_marching_amd import contrib
    (cx, cy, cz), R, slope, Ru, uslope = child_bound
    if isinstance(node, contrib.SDFBoundedScale):
        s = float(node.scale.detach())
        return ((s * cx, s * cy, s * cz), s * R, slope, s * Ru, uslope) if s > 0 else ((cx, cy, cz), math.inf, slope, math.inf, uslope)
    if isinstance(node, contrib.SDFBoundedMirror):
        return (float(node.origin.detach()), cy, cz), R + abs(cx), slope, Ru + uslope * abs(cx), uslope
    assert isinstance(node, contrib.SDFBoundedElongate)
    h = node.halfsides.detach().double()
    if bool((h < 0).any()):
        return (cx, cy, cz), math.inf, slope, math.inf, uslope
    hn = float(h.norm()) * 1.00001
    return (cx, cy, cz), R + hn, slope, Ru + uslope * hn, uslope


def test_the_shipped_bounds_keep_what_they_sign():
    """Each shipped bound, restated in Python, applied to the known sphere of a ball with a PyTorch forward, against the
    operator's own PyTorch forward at 2^16 points: node(p) >= slope |p - c'| - R' and node(p) <= uslope |p - c'| + Ru' within
    check_bound's tolerance 1e-5 (1 + |p| + R').  The points: half in a box of 6, half on rays from c' out to 8 R'."""
    from ray_marching_amd import contrib
    _register()
    gen = torch.Generator().manual_seed(43)
    balls = [((0.4, 0.1, -0.2), 0.3), ((-0.7, 0.0, 0.5), 0.05), ((0.0, 0.0, 0.0), 1.0), ((1.5, -1.0, 0.2), 0.6)]
    cases = [(contrib.SDFBoundedScale, s) for s in (0.05, 0.7, 1.0, 3.0)]
    cases += [(contrib.SDFBoundedMirror, o) for o in (0.0, 0.15, -0.8, 2.0)]
    cases += [(contrib.SDFBoundedElongate, h) for h in ((0.05, 0.3, 0.1), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 2.0, 0.25))]
    worst = {}
    for cls, arg in cases:
        for centre, radius in balls:
            node = cls(WBall(centre, radius), arg)
            c, R, slope, Ru, uslope = _restated(node, (centre, radius, 1.0, radius, 1.0))
            assert math.isfinite(R) and math.isfinite(Ru)
            ct = torch.tensor(c, dtype=torch.float64)
            u = torch.nn.functional.normalize(torch.randn(1 << 15, 3, generator=gen), dim=-1).double()
            pts = torch.cat([(torch.rand(1 << 15, 3, generator=gen).double() * 2 - 1) * 6.0, ct + u * (torch.rand(1 << 15, 1, generator=gen).double() * 8 * R)])
            with torch.no_grad():
                f = node(pts.float()).reshape(-1).double()
            pts = pts.float().double()
            dist = (pts - ct).norm(dim=-1)
            tol = 1e-5 * (1 + pts.norm(dim=-1) + R)
            lo, hi = float((f - (slope * dist - R) + tol).min()), float(((uslope * dist + Ru) - f + tol).min())
            worst[cls.__name__] = min(worst.get(cls.__name__, math.inf), lo, hi)
            assert lo >= 0 and hi >= 0, (cls.__name__, arg, centre, radius, lo, hi)
    print(f"smallest margin (tolerance included) per operator: { {k: round(v, 9) for k, v in worst.items()} }")
    # no bound where the parameters allow none, and the restatement is sharp enough to catch a bound that is too small
    assert _restated(contrib.SDFBoundedScale(WBall((0.0, 0.0, 0.0), 0.3), -0.5), ((0.0, 0.0, 0.0), 0.3, 1.0, 0.3, 1.0))[1] == math.inf
    assert _restated(contrib.SDFBoundedElongate(WBall((0.0, 0.0, 0.0), 0.3), (0.1, -0.1, 0.1)), ((0.0, 0.0, 0.0), 0.3, 1.0, 0.3, 1.0))[1] == math.inf
    node = contrib.SDFBoundedMirror(WBall((0.4, 0.1, -0.2), 0.3), 0.15)
    pts = (torch.rand(1 << 16, 3, generator=gen) * 2 - 1) * 2.0
    with torch.no_grad():
        f = node(pts).reshape(-1).double()
    dist = (pts.double() - torch.tensor((0.15, 0.1, -0.2), dtype=torch.float64)).norm(dim=-1)
    assert float((f - (dist - 0.3)).min()) < -0.3, "the child's radius alone is no bound for the mirrored ball"


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def libraries():
    """The libraries of the GPU legs: build() has made them; what is missing is built here, in one pool."""
    from concurrent.futures import ThreadPoolExecutor
    from ray_marching_amd import specialize
    programs = gpu_test_programs()
    with ThreadPoolExecutor(max_workers=min(16, len(programs))) as ex:
        list(ex.map(specialize.build, programs))
    return programs


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scene2_placed", "closed_scene1"])
def test_restated_affine_bound_is_bit_identical_with_the_builtin(which, libraries, monkeypatch):
    """Zero tolerance: UBAffine restates the map, the VJP and the bound of the built-in affine node, so a scene with it in
    place of every SDFAffineTransformation has the built-in scene's program (cull tests included, test above), the built-in
    scene's derived constants -- `rm_scene_bound` float for float -- and every bit of its values, point gradients, frames and
    parameter gradients (no deferred-ray list: the one part that is no function of the program)."""
    from ray_marching_amd import _abi, ops
    from ray_marching_amd.compiler import compiled_for
    _register()
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)
    make = _twin_factories()[which]
    (user, cu), (twin, ct) = _on_device(lambda: with_ubaffine(make()), {}), _on_device(make, {})
    assert cu.lib().rm_user_warps() == 1 and ct.specialised and _sites_over_warps(cu.program)
    assert int((ct.program[:, 0] == _abi.OP_CULL_MIN).sum()) == int((cu.program[:, 0] == _abi.OP_CULL_MIN).sum()) > 0
    assert [n for n, _ in user.named_parameters()] == [n for n, _ in twin.named_parameters()]
    bu, bt = ops.scene_bound(user), ops.scene_bound(twin)
    print(f"{which}: scene bound {bu[0].tolist()} {bu[1:]} (built-in {bt[0].tolist()} {bt[1:]})")
    assert torch.equal(bu[0], bt[0]) and bu[1:] == bt[1:] and math.isfinite(bu[1])
    pts = _points(4096, seed=11).to(DEV)
    q, t = _pose(-1.0 if which == "closed_scene1" else -3.0)
    res = {}
    for name, scene in (("user", user), ("twin", twin)):
        p = pts.clone().requires_grad_(True)
        d = scene(p)
        d.sum().backward()
        gw = [x.grad.clone() for x in scene.parameters()]
        loop = H.make_loop(scene, 40, 72)
        with torch.no_grad():
            frames = [loop(q, t, m, 1, 48) for m in (0, 4, 2, 5)]
        for x in scene.parameters():
            x.grad = None
        loop(q, t, 0, 1, 24).pow(2).mean().backward()
        res[name] = dict(d=d.detach(), gp=p.grad, frames=frames, gw=gw, gf=[x.grad.clone() for x in scene.parameters()])
    assert torch.equal(res["user"]["d"], res["twin"]["d"]) and torch.equal(res["user"]["gp"], res["twin"]["gp"])
    for a, b in zip(res["user"]["frames"], res["twin"]["frames"]):
        assert _same(a, b)
    for key in ("gw", "gf"):
        for a, b in zip(res["user"][key], res["twin"][key]):
            assert _same(a, b), key
        assert any(bool((b != 0).any()) for b in res["twin"][key]), key


@pytest.mark.gpu
def test_warp_bounds_against_hand_computed_numbers(libraries):
    """rm_scene_bound of chain(): scale over affine over mirror over elongate over affine over a sphere, for five parameter
    sets (one library: the parameters are live) -- as built, each operator alone, extremes -- against chain_bound(), which
    restates the operators' rules and the factors the walk applies around them.  2e-6 relative: the fp32 rounding of a dozen
    operations."""
    from ray_marching_amd import ops
    from ray_marching_amd.compiler import compiled_for
    _register()
    lib = None
    for kw in CHAIN_SETS:
        node = chain(**kw).to(DEV)
        lib = lib or compiled_for(node).lib()
        assert compiled_for(node).lib() is lib and lib.rm_user_warps() == 3
        c, R, slope, Ru, uslope = ops.scene_bound(node)
        wc, wR, wslope, wRu, wuslope = chain_bound(**kw)
        print(f"chain({kw}): centre {c.tolist()} R {R} slope {slope} Ru {Ru} uslope {uslope}; by hand {wc} {wR} {wslope} {wRu} {wuslope}")
        assert c.tolist() == pytest.approx(wc, rel=2e-6, abs=1e-7)
        assert R == pytest.approx(wR, rel=2e-6) and Ru == pytest.approx(wRu, rel=2e-6)
        assert slope == pytest.approx(wslope, rel=2e-6) and uslope == pytest.approx(wuslope, rel=2e-6)
    # each operator alone, in plain numbers: the sphere of 0.3 placed at t1 (R = 0.3 * 1.0001 + 1e-4 |t1|_1 after its affine node)
    c, R, _, Ru, _ = ops.scene_bound(chain(**CHAIN_SETS[1]).to(DEV))                                    # scale 2.5 about the origin
    assert c.tolist() == pytest.approx([0.5, -0.5, 0.75], rel=1e-6, abs=1e-7) and R == pytest.approx(2.5 * 0.3, rel=2e-3) and Ru == pytest.approx(R, rel=1e-4)
    c, R, _, _, _ = ops.scene_bound(chain(**CHAIN_SETS[2]).to(DEV))                                     # mirror: centre onto the plane, R + |c.x|
    assert c.tolist() == pytest.approx([-0.35 + 0.2, 0.1 - 0.3, -0.2 + 0.5], rel=1e-6) and R == pytest.approx(0.3 + 0.6, rel=2e-3)
    c, R, _, _, _ = ops.scene_bound(chain(**CHAIN_SETS[3]).to(DEV))                                     # elongate: R + |h|
    assert R == pytest.approx(0.3 + math.hypot(0.4, 0.25), rel=2e-3)


def _coherent_waves(gen, tight):
    """64 waves of 64 points each, so that culls fire; `tight`: half of them on the scaled sphere, next to its neighbour."""
    centres = (torch.rand(64, 1, 3, generator=gen) * 2 - 1) * 2.5
    if tight:
        centres[:32] = torch.tensor(TIGHT_END) + 0.05 * (torch.rand(32, 1, 3, generator=gen) * 2 - 1)
    pts = (centres + (0.01 if tight else 0.05) * torch.randn(64, 64, 3, generator=gen)).reshape(-1, 3).to(DEV)
    return pts, torch.randn(pts.shape[0], 1, generator=gen).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["nested", "tight_neighbour"])
def test_culling_over_a_bounded_warp_changes_no_bit(leg, libraries, monkeypatch):
    """tests/test_user_warp.py's culling test with the bounded operators: now cull ranges CONTAIN the warps' frames, so their
    bounds decide whether they are evaluated.  `nested`: compiled without cull tests, by default and with a test in front of
    every boundable child; `tight_neighbour`: without cull tests and with the exact logsumexp culling, half of the waves on
    the scaled sphere next to its neighbour, where a table entry that is too small for the scaled node skips it.  Values,
    both kinds of gradient, and frames with their gradients are the same bits."""
    from ray_marching_amd import _abi, ops
    _register()
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)      # bitwise parameter gradients: no atomically ordered deferred-ray list
    tight = leg == "tight_neighbour"
    pts, wts = _coherent_waves(torch.Generator().manual_seed(5), tight)
    q, t = _pose(-3.5)
    if tight:      # close to the scaled sphere's top, looking at it
        t = torch.tensor([[TIGHT_END[0], TIGHT_END[1], -1.5]], device=DEV)
    res = []
    for env in CULL_LEGS[leg]:
        scene, cs = _on_device(cull_scene, env)
        assert cs.lib().rm_user_warps() == 3
        p = pts.clone().requires_grad_(True)
        d = scene(p)
        (d * wts).sum().backward()
        gw = [x.grad.clone() for x in scene.parameters()]
        loop = H.make_loop(scene, 40, 72)
        with torch.no_grad():
            frames = [loop(q, t, m, 1, 48) for m in (0, 4, 2, 5)]
        for x in scene.parameters():
            x.grad = None
        loop(q, t, 0, 1, 24).pow(2).mean().backward()
        res.append(dict(env=env, sites=_sites_over_warps(cs.program), d=d.detach(), gp=p.grad, frames=frames, gw=gw,
                        gf=[x.grad.clone() for x in scene.parameters()],
                        n_cull=int(np.isin(cs.program[:, 0], (_abi.OP_CULL_MIN, _abi.OP_CULL_LSE)).sum())))
    print(f"culling leg {leg}: cull instructions per variant {[r['n_cull'] for r in res]}, of them over a warp {[len(r['sites']) for r in res]}")
    assert res[0]["n_cull"] == 0
    for got in res[1:]:
        assert got["sites"], "no cull range covers a warp"
    if tight:
        assert _abi.OP_CULL_LSE in [op for op, _ in res[1]["sites"]], "RM_CULL_LSE=1 put no cull test in front of the scaled sphere"
        near = (pts.cpu() - torch.tensor(TIGHT_END)).norm(dim=-1) < 0.1
        assert int(near.sum()) > 1000 and res[0]["d"].cpu()[near].abs().max().item() < 0.12      # those waves ARE at the surface
    else:
        assert res[1]["n_cull"] == 3 and res[2]["n_cull"] == 4 and res[1]["sites"] != res[2]["sites"]
    ref = res[0]
    for got in res[1:]:
        assert _same(ref["d"], got["d"]) and _same(ref["gp"], got["gp"]), got["env"]
        for x, y in zip(ref["frames"], got["frames"]):
            assert _same(x, y), got["env"]
        for name in ("gw", "gf"):
            for x, y in zip(ref[name], got[name]):
                assert _same(x, y), (got["env"], name)


@pytest.mark.gpu
def test_the_warp_bound_follows_the_live_parameters(libraries):
    """NAME_bound runs on the device at staging time, from the parameters the launch reads: after in-place edits of `scale`,
    `origin` and `halfsides` the culled program still renders the frames of the program without cull tests, and
    rm_scene_bound (of chain(), edited the same way) has moved; scale <= 0 or NaN, or a negative half-side, give "no bound"
    (and the same frames)."""
    from ray_marching_amd import ops
    _register()
    culled, cs = _on_device(cull_scene, {})
    plain, cs0 = _on_device(cull_scene, CULL_OFF)
    assert len(_sites_over_warps(cs.program)) == 3 and not _sites_over_warps(cs0.program)
    loops = [H.make_loop(s, 40, 72) for s in (culled, plain)]
    q, t = _pose(-3.5)
    node = chain().to(DEV)
    parts = lambda n: (n.sdf.sdf, [n], n.sdf.sdf.sdf)                     # (mirror, [scale], elongate) of a chain()

    def edit(fn):
        """fn(mirror, scales, elongation) on both scenes and on the chain."""
        with torch.no_grad():
            for s in (culled, plain):
                fn(*cull_scene_warps(s))
            fn(*parts(node))

    def frames_agree(what):
        with torch.no_grad():
            for mode in (0, 4, 1):
                a, b = (loop(q, t, mode, 1, 48) for loop in loops)
                assert _same(a, b), (what, mode)
        return ops.scene_bound(node)

    kw = dict()
    c, R, slope, Ru, uslope = frames_agree("as built")
    assert R == pytest.approx(chain_bound()[1], rel=2e-6) and c.tolist() == pytest.approx(chain_bound()[0], rel=2e-6)
    edit(lambda m, scales, e: [s.scale.mul_(1.25) for s in scales])
    kw["scale"] = 1.7 * 1.25
    c, R, _, Ru, _ = frames_agree("scale")
    assert R == pytest.approx(chain_bound(**kw)[1], rel=2e-6) and Ru == pytest.approx(chain_bound(**kw)[3], rel=2e-6)
    edit(lambda m, scales, e: m.origin.add_(0.2))
    kw["origin"] = 0.15 + 0.2
    c, R, _, _, _ = frames_agree("origin")
    assert c.tolist() == pytest.approx(chain_bound(**kw)[0], rel=2e-6) and R == pytest.approx(chain_bound(**kw)[1], rel=2e-6)
    edit(lambda m, scales, e: e.halfsides.mul_(2.0))
    kw["halfsides"] = (0.1, 0.6, 0.2)
    c, R, _, _, _ = frames_agree("halfsides")
    assert R == pytest.approx(chain_bound(**kw)[1], rel=2e-6) and R > chain_bound(scale=kw["scale"], origin=kw["origin"])[1] + 0.3
    edit(lambda m, scales, e: e.halfsides.mul_(torch.tensor([1.0, -1.0, 1.0], device=DEV)))
    assert frames_agree("negative half-side")[1] == math.inf
    edit(lambda m, scales, e: e.halfsides.abs_())
    assert frames_agree("half-sides back")[1] == pytest.approx(chain_bound(**kw)[1], rel=2e-6)
    for bad in (-0.5, 0.0, float("nan")):
        edit(lambda m, scales, e: [s.scale.fill_(bad) for s in scales])
        b = frames_agree(f"scale {bad}")
        assert b[1] == math.inf and b[3] == math.inf, bad
    edit(lambda m, scales, e: [s.scale.fill_(0.6) for s in scales])
    kw["scale"] = 0.6
    assert frames_agree("scale back")[1] == pytest.approx(chain_bound(**kw)[1], rel=2e-6)


@pytest.mark.gpu
def test_the_warp_bound_is_consumed_and_check_bound_catches_a_wrong_one(libraries):
    """LiarWarp is the identity map over a sphere of 0.5 around the origin but signs a sphere of 0.1 around (40, 0, 0).  Behind
    a cheap child, waves near the origin skip it (the program answers the cheap child's distance, where the true minimum is
    the sphere's): the bound is consumed, not just carried.  check_bound names a point where it fails; the shipped operators
    pass, each alone and all together; an unbounded warp has nothing to check.  Wrong numbers on purpose, nothing else:
    evaluation only, every access in range."""
    from ray_marching_amd import contrib
    from ray_marching_amd.extensions import check_bound
    from ray_marching_amd.scene.primitives import SDFSphere
    _register()
    gen = torch.Generator().manual_seed(9)
    pts = (0.3 * (torch.rand(64, 1, 3, generator=gen) * 2 - 1) + 0.05 * torch.randn(64, 64, 3, generator=gen)).reshape(-1, 3).to(DEV)
    culled, cs = _on_device(liar_scene, {})
    assert _sites_over_warps(cs.program)
    with torch.no_grad():
        wrong = culled(pts)
    sphere, cheap = pts.norm(dim=-1, keepdim=True) - 0.5, (pts - torch.tensor([3.0, 0.0, 0.0], device=DEV)).norm(dim=-1, keepdim=True) - 0.1
    true = torch.minimum(sphere, cheap)      # (the LiarWarp is the identity map over the sphere)
    assert torch.equal(true, sphere), "the sphere under the LiarWarp decides the minimum near the origin"
    assert (wrong - cheap).abs().max().item() <= 1e-5, "with its cull test the LiarWarp was not skipped: the bound is not consumed"
    assert (wrong - true).min().item() > 2.0
    with pytest.raises(ValueError, match=r"lower bound of LiarWarp fails .*liarwarp_bound.* at p = \["):
        check_bound(LiarWarp(SDFSphere(0.5)).to(DEV))
    for kw in CHAIN_SETS:
        c, R, slope, Ru, uslope = check_bound(chain(**kw).to(DEV))
        assert math.isfinite(R) and math.isfinite(Ru) and 0.5 < slope <= 1.0
    with pytest.raises(ValueError, match="defines no sdf_scale_bound"):
        check_bound(contrib.SDFScale(SDFSphere(0.5), 0.5).to(DEV))
    with pytest.raises(ValueError, match="defines no wb_plain_bound"):
        check_bound(Plain(SDFSphere(0.5)).to(DEV))
    with pytest.raises(ValueError, match="sdf_bscale_bound gives no finite bound"):      # (same library as chain(): parameters are live)
        check_bound(chain(scale=-1.0).to(DEV))
    with pytest.raises(TypeError, match="not a registered leaf or warp"):
        check_bound(SDFSphere(0.5).to(DEV))
