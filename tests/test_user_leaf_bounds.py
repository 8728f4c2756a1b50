"""Bounding spheres of user-defined SDF leaves (`RM_DEV void NAME_bound(const float* theta, rm::LeafBound& b)` in the
leaf's HIP source, ray_marching_amd/extensions.py): registration, the programs the compiler emits once a leaf is
boundable, the generated `user_leaf_bound` dispatch, and -- on the GPU -- that the exact cull tests which now cover such
a leaf change no bit, that the bound follows the live parameters, that it is really consumed (a leaf that lies about
its sphere renders wrong numbers and `extensions.check_bound` says where), and `rm_scene_bound`, the entry point that
makes any scene's bound observable.

Zero tolerance wherever two programs of one scene are compared: a correct bound changes no bit.
"""
import math
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import helpers as H
from tests.helpers import _points, _pose, _same, environment
from tests.test_user_leaf import LINK, LINK_Q, LINK_T, TIGHT_END, closed_scene_with, scene2_with

DEV = "cuda"
IDENT = [1.0, 0.0, 0.0, 0.0]


# --------------------------------------------------------------------------------------------------------------
# test-defined leaves
# --------------------------------------------------------------------------------------------------------------
class _Ball(nn.Module):
    def __init__(self, radius: float = 0.5):
        super().__init__()
        self.radius = nn.Parameter(torch.tensor(radius, dtype=torch.float32))

    def forward(self, query_positions):
        return torch.linalg.vector_norm(query_positions, dim=-1, keepdim=True) - self.radius


class BSphere(_Ball):
    """SDFSphere restated as a user leaf (the op stream of the built-in handler) that signs the built-in sphere's bound."""


class NoBound(_Ball):
    """The same without a bound (what every user leaf was before NAME_bound existed)."""


class Liar(_Ball):
    """A sphere around the origin that signs a sphere of 0.1 around (40, 0, 0): a wrong bound, on purpose."""


class HalfBall(_Ball):
    """0.6 (|p| - r): a conservative distance (leaf contract (i)).  slope = 1 would be false for it; it signs
    slope = 0.6, R = 0.6 r and no upper bound."""

    def forward(self, query_positions):
        return (torch.linalg.vector_norm(query_positions, dim=-1, keepdim=True) - self.radius) * 0.6


_BALL_HIP = """
template <bool Fast> RM_DEV float NAME_fwd(rm::V3 p, const float* theta) { return norm3_t<Fast>(p) - theta[0]; }
template <bool Fast> RM_DEV void NAME_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) {
  const float n = norm3_t<Fast>(p);
  const float s = (n == 0.0f) ? 0.0f : div_t<Fast>(g, n);
  gp = gp + mk3(p.x * s, p.y * s, p.z * s);
  gtheta[0] = -g;
}
"""
BSPHERE_BOUND = """
// |p| - r: an exact distance, the surface is the sphere itself
RM_DEV void bsphere_bound(const float* theta, rm::LeafBound& b) {
  if (theta[0] >= 0.0f) b.R = b.Ru = theta[0];
}
"""
BSPHERE_HIP = _BALL_HIP.replace("NAME", "bsphere") + BSPHERE_BOUND
NOBOUND_HIP = _BALL_HIP.replace("NAME", "nobound")
LIAR_HIP = _BALL_HIP.replace("NAME", "liar") + """
RM_DEV void liar_bound(const float* theta, rm::LeafBound& b) { b.c = mk3(40.0f, 0.0f, 0.0f); b.R = b.Ru = 0.1f; }
"""
HALFBALL_HIP = """
template <bool Fast> RM_DEV float halfball_fwd(rm::V3 p, const float* theta) { return (norm3_t<Fast>(p) - theta[0]) * 0.6f; }
template <bool Fast> RM_DEV void halfball_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) {
  const float g6 = g * 0.6f;
  const float n = norm3_t<Fast>(p);
  const float s = (n == 0.0f) ? 0.0f : div_t<Fast>(g6, n);
  gp = gp + mk3(p.x * s, p.y * s, p.z * s);
  gtheta[0] = -g6;
}
RM_DEV void halfball_bound(const float* theta, rm::LeafBound& b) {
  if (theta[0] >= 0.0f) { b.slope = 0.6f; b.R = 0.6f * theta[0]; }
}
"""


def _register():
    from ray_marching_amd.extensions import register_leaf
    register_leaf(BSphere, params=("radius",), hip=BSPHERE_HIP, cost=13)        # SDFSphere's cost: the twins' programs must agree
    register_leaf(NoBound, params=("radius",), hip=NOBOUND_HIP, cost=13)
    register_leaf(Liar, params=("radius",), hip=LIAR_HIP, cost=40)              # (compiler._CULL_MIN_CHILD_COST: gets a site of its own)
    register_leaf(HalfBall, params=("radius",), hip=HALFBALL_HIP, cost=40)


# Python restatements of the bounds the leaves sign: (centre, R, slope, Ru, uslope) from the parameters
def _sign_ball(leaf):
    r = float(leaf.radius.detach())
    return (0.0, 0.0, 0.0), r, 1.0, r, 1.0


def _sign_halfball(leaf):
    return (0.0, 0.0, 0.0), 0.6 * float(leaf.radius.detach()), 0.6, math.inf, 1.0


def _sign_link(leaf):
    r = sum(float(x.detach()) for x in (leaf.length, leaf.radius1, leaf.radius2))
    return (0.0, 0.0, 0.0), r, 1.0, r, 1.0


LINK_SETS = [(0.35, 0.3, 0.08), (0.8, 0.3, 0.08), (0.2, 0.25, 0.05), (0.0, 0.5, 0.1), (1.5, 0.1, 0.4)]


# --------------------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------------------
def siblings():
    """tests/test_user_leaf.py: link_among_cullable_siblings() with the bounded link."""
    from ray_marching_amd.contrib import SDFBoundedLink
    from ray_marching_amd.scene.primitives import SDFLine, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    return SDFUnion([
        make_room(),
        A(SDFTorus(radius1=0.5, radius2=0.12), orientation=[0.0, 0.5 ** 0.5, 0.5 ** 0.5, 0.0], translation=[1.1, 0.4, 0.5]),
        A(SDFBoundedLink(**LINK), orientation=LINK_Q, translation=LINK_T),
        A(SDFSphere(0.4), orientation=IDENT, translation=[0.2, -0.9, 0.8]),
        SDFLine(start=(-1.5, 1.0, 1.0), end=(-0.5, 1.2, 0.4), radius=0.1),
    ])


def blob():
    """tests/test_user_leaf.py: link_inside_a_blob() with the bounded link."""
    from ray_marching_amd.contrib import SDFBoundedLink
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFSmoothUnion, SDFUnion
    g = torch.Generator().manual_seed(77)
    t = (torch.rand(8, 3, generator=g) * 5.0 - 2.5).tolist()
    q = torch.nn.functional.normalize(torch.randn(8, 4, generator=g), dim=-1).tolist()
    pair = SDFUnion([SDFSphere(0.1), A(SDFBoundedLink(**LINK), orientation=LINK_Q, translation=[0.3, 0.0, 0.0])])
    prims = [SDFSphere(0.3), SDFBox((0.2, 0.3, 0.15)), SDFTorus(0.4, 0.1), pair,
             SDFSphere(0.25), SDFBox((0.3, 0.1, 0.2)), SDFTorus(0.35, 0.08), SDFSphere(0.35)]
    return SDFUnion([make_room(), SDFSmoothUnion([A(p, orientation=q[i], translation=t[i]) for i, p in enumerate(prims)], blend_k=22.0)])


def tight_neighbour():
    """tests/test_user_leaf.py: link_with_a_tight_neighbour() with the bounded link: the stiff smooth union in which a bound
    that is too small for the link shows as a jump of 0.07 at the link's far end."""
    from ray_marching_amd.contrib import SDFBoundedLink
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFSmoothUnion, SDFUnion
    pair = SDFUnion([SDFSphere(0.05), A(SDFBoundedLink(0.8, 0.3, 0.08), orientation=IDENT, translation=[0.9, 0.0, 0.0])])
    far = [A(SDFSphere(0.3), orientation=IDENT, translation=[-2.0, -1.5, 1.0]), A(SDFBox((0.2, 0.3, 0.15)), orientation=LINK_Q, translation=[2.0, -1.0, 0.5]),
           A(SDFTorus(0.4, 0.1), orientation=LINK_Q, translation=[-1.5, 1.5, -1.0]), A(SDFSphere(0.25), orientation=IDENT, translation=[0.0, -2.0, -1.5]),
           A(SDFBox((0.3, 0.1, 0.2)), orientation=IDENT, translation=[2.2, 1.8, 1.5]), A(SDFTorus(0.35, 0.08), orientation=IDENT, translation=[-2.2, 0.0, 2.0])]
    neighbour = A(SDFSphere(0.05), orientation=IDENT, translation=[TIGHT_END[0], TIGHT_END[1] + 0.12, TIGHT_END[2]])
    return SDFUnion([make_room(), SDFSmoothUnion([pair, neighbour] + far, blend_k=300.0)])


# |q|^2 = 0.97: the affine rule multiplies the leaf's slope by min(1, 2 |q|^2 - 1) - 1e-5 = 0.94: 0.6 * 0.94 = 0.564, above the
# walker's floor of 0.5
HALF_Q = [x * math.sqrt(0.97 / sum(y * y for y in LINK_Q)) for x in LINK_Q]


def halfball_holder():
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A
    return A(HalfBall(0.5), orientation=HALF_Q, translation=[-0.8, 0.2, 0.3])


def halfball_scene():
    from ray_marching_amd.scene.primitives import SDFSphere
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    return SDFUnion([make_room(), A(SDFSphere(0.4), orientation=IDENT, translation=[1.2, 0.0, 0.4]), halfball_holder()])


def live_scene():
    """The scene whose leaf parameters the live-parameter leg edits: a BSphere and a bounded link, each behind a cull test
    of its own under RM_CULL_MIN_COST=0."""
    from ray_marching_amd.contrib import SDFBoundedLink
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    return SDFUnion([make_room(), A(BSphere(0.5), orientation=IDENT, translation=[0.9, 0.0, 0.0]),
                     A(SDFBoundedLink(**LINK), orientation=LINK_Q, translation=LINK_T)])


def liar_scene():
    """A cheap child (no cull test: below the cost threshold), then the Liar behind its CULL_MIN."""
    from ray_marching_amd.scene.primitives import SDFSphere
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    return SDFUnion([A(SDFSphere(0.1), orientation=IDENT, translation=[3.0, 0.0, 0.0]), Liar(0.5)])


def moved_bsphere():
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A
    return A(BSphere(0.4), orientation=IDENT, translation=[0.5, -0.25, 1.0])


def mixed_union():
    from ray_marching_amd.scene.primitives import SDFSphere
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    return SDFUnion([SDFSphere(0.1), A(BSphere(0.3), orientation=IDENT, translation=[1.0, 0.0, 0.0]),
                     A(NoBound(0.3), orientation=IDENT, translation=[-1.0, 0.0, 0.0])])


CULL_OFF = dict(RM_CULL="0")
CULL_ENVS = [CULL_OFF, dict(), dict(RM_CULL_MIN_COST="0"), dict(RM_CULL_LSE="1", RM_CULL_LSE_MIN="2")]
CULL_SCENES = {"siblings": siblings, "blob": blob, "tight_neighbour": tight_neighbour}
_KNOBS = ("RM_CULL", "RM_CULL_MIN_COST", "RM_CULL_LSE", "RM_CULL_LSE_MIN", "RM_CULL_REORDER", "RM_CULL_UNION_TABLE")


def _compile(make, env):
    """compile_scene(make()) with exactly these culling knobs set."""
    from ray_marching_amd.compiler import compile_scene
    with environment(**env):
        saved = {k: os.environ.pop(k) for k in _KNOBS if k not in env and k in os.environ}
        try:
            return compile_scene(make())
        finally:
            os.environ.update(saved)


def _lone_leaves():
    from ray_marching_amd.contrib import SDFBoundedLink, SDFLink
    return [lambda: BSphere(0.5), lambda: SDFBoundedLink(**LINK), lambda: HalfBall(0.5), lambda: Liar(0.5), lambda: NoBound(0.5),
            lambda: SDFLink(**LINK)]


def gpu_test_programs():
    """Every test-defined program the GPU legs launch: build() compiles their libraries, so that a GPU run of the same tree
    finds them; where one is missing it builds itself on first use."""
    from ray_marching_amd import specialize
    from ray_marching_amd.contrib import make_link_scene
    _register()
    out = [_compile(lambda: scene2_with(BSphere), {}), _compile(lambda: closed_scene_with(BSphere), {})]
    out += [_compile(make, env) for make in CULL_SCENES.values() for env in CULL_ENVS]
    out += [_compile(halfball_scene, env) for env in (CULL_OFF, {})] + [_compile(halfball_holder, {}), _compile(moved_bsphere, {})]
    out += [_compile(live_scene, env) for env in (CULL_OFF, dict(RM_CULL_MIN_COST="0"))]
    out += [_compile(liar_scene, env) for env in (CULL_OFF, {})]
    out += [_compile(make, {}) for make in _lone_leaves()]
    out += [_compile(lambda: make_link_scene(bounded=True), CULL_OFF)]
    return list({specialize.scene_hash(cs): cs for cs in out}.values())


def _covered(program, op):
    """USER rows (as [off, aux0]) that lie inside the range of a cull instruction `op` of this program."""
    from ray_marching_amd import _abi
    rows = np.asarray(program).reshape(-1, 4)
    found = []
    for i in np.flatnonzero(rows[:, 0] == op):
        n = int(rows[i, 3]) >> 8 if op == _abi.OP_CULL_MIN else int(rows[i, 3])
        found += [tuple(r[1:3]) for r in rows[i + 1:i + n].tolist() if r[0] == _abi.OP_USER]
    return found


def _on_device(make, env):
    """(scene on the GPU, its CompiledScene) compiled with exactly these culling knobs; later launches keep that program."""
    from ray_marching_amd.compiler import compiled_for
    holder = {}

    def build():
        holder["scene"] = make().to(DEV)
        return holder["scene"]

    with environment(**env):
        saved = {k: os.environ.pop(k) for k in _KNOBS if k not in env and k in os.environ}
        try:
            cs = compiled_for(build())
        finally:
            os.environ.update(saved)
    return holder["scene"], cs


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
def test_registration_of_a_bound():
    from ray_marching_amd import contrib
    from ray_marching_amd.extensions import leaf_spec, register_leaf
    _register()
    assert leaf_spec(BSphere(0.3)).bounded and leaf_spec(BSphere(0.3)).name == "bsphere"
    assert leaf_spec(HalfBall(0.3)).bounded and leaf_spec(Liar(0.3)).bounded
    assert not leaf_spec(NoBound(0.3)).bounded
    assert leaf_spec(contrib.SDFBoundedLink(**LINK)).bounded and not leaf_spec(contrib.SDFLink(**LINK)).bounded
    assert leaf_spec(contrib.SDFBoundedLink(**LINK)).name == "blink"
    register_leaf(BSphere, params=("radius",), hip=BSPHERE_HIP, cost=13)                       # the same again: fine
    # the bound is part of the source, hence of what identifies the registration
    with pytest.raises(ValueError, match="already registered"):
        register_leaf(BSphere, params=("radius",), hip=_BALL_HIP.replace("NAME", "bsphere"), cost=13)
    with pytest.raises(ValueError, match="already registered"):
        register_leaf(NoBound, params=("radius",), hip=NOBOUND_HIP + BSPHERE_BOUND.replace("bsphere", "nobound"), cost=13)

    class Fresh(_Ball):
        pass

    src = _BALL_HIP.replace("NAME", "fresh")
    with pytest.raises(ValueError, match="fresh_bound"):                                       # another NAME
        register_leaf(Fresh, params=("radius",), hip=src + BSPHERE_BOUND, cost=13)
    two = BSPHERE_BOUND.replace("bsphere", "fresh")
    with pytest.raises(ValueError, match="at most one"):
        register_leaf(Fresh, params=("radius",), hip=src + two + two, cost=13)
    with pytest.raises(ValueError, match="template"):
        register_leaf(Fresh, params=("radius",), hip=src + two.replace("RM_DEV void", "template <bool Fast> RM_DEV void"), cost=13)
    with pytest.raises(ValueError, match="exactly two device functions"):                      # fwd / vjp are still required
        register_leaf(Fresh, params=("radius",), hip=two, cost=13)
    with pytest.raises(ValueError, match="inline assembly"):                                   # the whole source is checked
        register_leaf(Fresh, params=("radius",), hip=src + two.replace("if (", 'asm volatile(""); if ('), cost=13)
    assert leaf_spec(Fresh(0.3)) is None                                                       # nothing of the above registered it
    # a bound in a comment is no bound
    register_leaf(Fresh, params=("radius",), hip=src + "// RM_DEV void fresh_bound(const float* theta, rm::LeafBound& b) {}\n", cost=13)
    assert leaf_spec(Fresh(0.3)).name == "fresh" and not leaf_spec(Fresh(0.3)).bounded

    # a registered subclass of a registered class evaluates CPU points through the PyTorch forward it inherits
    class SubLink(contrib.SDFLink):
        pass

    register_leaf(SubLink, params=("length", "radius1", "radius2"),
                  hip=contrib._LINK_HIP.replace("link_", "sublink_"), cost=30)
    p = _points(64)
    assert leaf_spec(SubLink(**LINK)).name == "sublink"
    assert torch.equal(SubLink(**LINK)(p), contrib.SDFLink(**LINK)(p)) and SubLink(**LINK)(torch.zeros(2, 3)).shape == (2, 1)
    assert torch.equal(contrib.SDFBoundedLink(**LINK)(p), contrib.SDFLink(**LINK)(p))
    assert torch.equal(BSphere(0.3)(p), NoBound(0.3)(p))


def test_programs_of_bounded_leaves():
    from ray_marching_amd import _abi, contrib
    from ray_marching_amd.scene.primitives import SDFSphere
    _register()
    A = _abi
    ok = lambda cs: _abi.lib.rm_validate_program(cs.program.ctypes.data, cs.n_instr, cs.n_params, cs.n_derived, cs.stack_floats, cs.n_slots)
    # a restated built-in leaf with its bound: the program of the built-in twin, row for row, except the leaf's own row
    for make in (scene2_with, closed_scene_with):
        for env in ({}, dict(RM_CULL_MIN_COST="0"), dict(RM_CULL_LSE="1", RM_CULL_LSE_MIN="2")):
            user, twin = _compile(lambda: make(BSphere), env), _compile(lambda: make(SDFSphere), env)
            mine, theirs = user.program.reshape(-1, 4).tolist(), twin.program.reshape(-1, 4).tolist()
            assert len(mine) == len(theirs) and (user.n_derived, user.n_slots, user.stack_floats) == (twin.n_derived, twin.n_slots, twin.stack_floats)
            n_user = 0
            for a, b in zip(mine, theirs):
                if b[0] == A.OP_SPHERE:
                    assert a == [A.OP_USER, b[1], 0, 1]
                    n_user += 1
                else:
                    assert a == b
            assert n_user == 1 and ok(user) == 0
            assert user.user_bounded == (True,) and user.user_leaves[0][:2] == ("bsphere", 1) and len(user.user_leaves[0]) == 3
            if not env:
                assert _covered(user.program, A.OP_CULL_MIN), "the cull test over the twin's inner union covers the leaf"
    # ... and without its bound: every cull test over it is gone, as before
    plain = _compile(lambda: scene2_with(NoBound), {})
    assert plain.user_bounded == (False,) and not (plain.program.reshape(-1, 4)[:, 0] == A.OP_CULL_MIN).any()
    # a union of a bounded and an unbounded leaf: a test over the first, none over the second
    cs = _compile(mixed_union, dict(RM_CULL_MIN_COST="0"))
    names = [name for name, _, _ in cs.user_leaves]
    assert sorted(names) == ["bsphere", "nobound"] and cs.user_bounded == tuple(n == "bsphere" for n in names)
    assert [t for _, t in _covered(cs.program, A.OP_CULL_MIN)] == [names.index("bsphere")] and ok(cs) == 0
    assert not (_compile(mixed_union, {}).program.reshape(-1, 4)[:, 0] == A.OP_CULL_MIN).any()      # (too cheap by default)
    # the contrib scene: its inner union and the link's affine node get their tests; without the bound it has none
    from ray_marching_amd.contrib import make_link_scene
    assert not (_compile(make_link_scene, {}).program.reshape(-1, 4)[:, 0] == A.OP_CULL_MIN).any()
    bounded = _compile(lambda: make_link_scene(bounded=True), {})
    assert len(_covered(bounded.program, A.OP_CULL_MIN)) == 2 and bounded.user_leaves[0][0] == "blink"
    # a smooth union of 8 children, one of them holding the bounded link, under a min-union: the bound table and the
    # by-children CULL_MIN it had lost
    for make, unbounded_twin in ((blob, "link_inside_a_blob"), (tight_neighbour, "link_with_a_tight_neighbour")):
        cs = _compile(make, {})
        rows = cs.program.reshape(-1, 4)
        sb = rows[rows[:, 0] == A.OP_SMOOTH_BEGIN]
        cm = rows[rows[:, 0] == A.OP_CULL_MIN]
        assert len(sb) == 1 and sb[0, 2] != 0 and (sb[0, 3] & 255) == 8, "the smooth union has no bound table"
        assert any(r[1] == 1 for r in cm.tolist()) and _covered(cs.program, A.OP_CULL_MIN) and ok(cs) == 0
        import tests.test_user_leaf as T
        old = _compile(getattr(T, unbounded_twin), {})
        assert not (old.program.reshape(-1, 4)[:, 0] == A.OP_CULL_MIN).any()                      # SDFLink stays as it was
        lse = _compile(make, dict(RM_CULL_LSE="1", RM_CULL_LSE_MIN="2"))
        assert _covered(lse.program, A.OP_CULL_LSE) and ok(lse) == 0
    # siblings: the link's affine node is expensive enough for a test of its own by default
    assert _covered(_compile(siblings, {}).program, A.OP_CULL_MIN)
    assert _covered(_compile(halfball_scene, {}).program, A.OP_CULL_MIN) and _covered(_compile(liar_scene, {}).program, A.OP_CULL_MIN)
    assert not _covered(_compile(siblings, CULL_OFF).program, A.OP_CULL_MIN)


def test_bound_dispatch_cross_compiles(monkeypatch):
    from concurrent.futures import ThreadPoolExecutor
    from ray_marching_amd import _abi, specialize
    from ray_marching_amd.extensions import register_leaf
    _register()
    cs = _compile(mixed_union, dict(RM_CULL_MIN_COST="0"))
    hdr = specialize.code_header(cs)
    t = [name for name, _, _ in cs.user_leaves].index("bsphere")
    assert "RM_DEV void user_leaf_bound(int type, const float* theta, LeafBound& b)" in hdr
    assert f"case {t}: bsphere_bound(theta, b); break;" in hdr and "RM_DEV void bsphere_bound(" in hdr
    assert "nobound_bound" not in hdr and "nobound_fwd<Fast>" in hdr
    # also for a scene whose leaves have none: the walker calls it for every RM_OP_USER
    assert "user_leaf_bound" in specialize.code_header(_compile(lambda: NoBound(0.5), {}))
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    with ThreadPoolExecutor(max_workers=4) as ex:
        paths = list(ex.map(specialize.build, [cs] + gpu_test_programs()))
    assert all(os.path.isfile(p) for p in paths)
    monkeypatch.setenv("RM_SPECIALIZE", "prebuilt")
    specialize._loaded.clear()
    lib = cs.lib()
    assert lib is not _abi.lib and lib.rm_user_leaves() == 2 and lib.rm_abi_version() == _abi.ABI_VERSION
    assert hasattr(lib, "rm_scene_bound") and hasattr(_abi.lib, "rm_scene_bound")

    class BrokenBound(_Ball):
        pass

    register_leaf(BrokenBound, params=("radius",), cost=13, hip=_BALL_HIP.replace("NAME", "brokenbound") +
                  "RM_DEV void brokenbound_bound(const float* theta, rm::LeafBound& b) { b.R = no_such_helper(theta[0]); }\n")
    monkeypatch.setenv("RM_SPECIALIZE", "jit")
    with pytest.raises(_abi.RmError, match="no_such_helper"):
        _compile(lambda: BrokenBound(0.5), {}).lib()
    specialize._loaded.clear()


def _contract_margins(leaf, sign, pts):
    """(min over pts of f - (slope |p - c| - R),  min of (uslope |p - c| + Ru) - f) for the leaf's PyTorch forward."""
    c, R, slope, Ru, uslope = sign(leaf)
    with torch.no_grad():
        f = leaf(pts).reshape(-1).double()
    dist = (pts.double() - torch.tensor(c, dtype=torch.float64)).norm(dim=-1)
    return float((f - (slope * dist - R)).min()), float(((uslope * dist + Ru) - f).min())


def test_the_leaves_of_this_file_keep_what_they_sign():
    """Each leaf's PyTorch forward against a Python restatement of its bound: a wrong fixture must not be blamed on the
    kernels.  f >= slope |p - c| - R - 1e-5 (fp32 rounding of f at |p| <= 11), f <= uslope |p - c| + Ru + 1e-5."""
    from ray_marching_amd import contrib
    _register()
    pts = (torch.rand(400_000, 3, generator=torch.Generator().manual_seed(41)) * 2 - 1) * 6.0
    cases = [(BSphere(r), _sign_ball) for r in (0.5, 0.05, 2.0, 0.0)] + [(HalfBall(r), _sign_halfball) for r in (0.5, 0.05, 2.0)]
    cases += [(contrib.SDFLink(*s), _sign_link) for s in LINK_SETS]          # (SDFBoundedLink inherits this forward)
    for leaf, sign in cases:
        lo, hi = _contract_margins(leaf, sign, pts)
        print(f"{type(leaf).__name__}{[round(float(p.detach()), 3) for p in leaf.parameters()]}: lower margin {lo:.3g}, upper margin {hi:.3g}")
        assert lo >= -1e-5 and hi >= -1e-5
    # ... and the restatement is sharp enough to catch the leaf that lies
    lo, _ = _contract_margins(Liar(0.5), lambda leaf: ((40.0, 0.0, 0.0), 0.1, 1.0, 0.1, 1.0), pts)
    assert lo < -30.0


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scene2", "closed_scene1"])
def test_bounded_sphere_is_bit_identical_with_the_builtin(which):
    """BSphere restates SDFSphere's op stream AND its bound: the same program, the same derived constants, hence every bit
    of every value, point gradient and frame; parameter and pose gradients to summation order (1e-5 relative)."""
    from ray_marching_amd import _abi
    from ray_marching_amd.compiler import compiled_for
    from ray_marching_amd.scene.primitives import SDFSphere
    _register()
    make = scene2_with if which == "scene2" else closed_scene_with
    user, twin = make(BSphere).to(DEV), make(SDFSphere).to(DEV)
    assert compiled_for(user).lib().rm_user_leaves() == 1 and compiled_for(twin).specialised
    assert _covered(compiled_for(user).program, _abi.OP_CULL_MIN)
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
    lu, lt = H.make_loop(user, h, w, n=2), H.make_loop(twin, h, w, n=2)                 # two cameras in one batch
    q2, t2 = torch.cat([c[0] for c in cams]), torch.cat([c[1] for c in cams])
    for mode in (0, 1, 4):
        with torch.no_grad():
            assert _same(lu(q2, t2, mode, 1, steps), lt(q2, t2, mode, 1, steps)), mode
    grads = {}
    for name, scene in (("user", user), ("twin", twin)):                                 # Lambertian MSE step
        for x in scene.parameters():
            x.grad = None
        loop = H.make_loop(scene, 32, 32)
        q, t = _pose(-1.0 if which == "closed_scene1" else -3.0)
        q.requires_grad_(True); t.requires_grad_(True)
        loop(q, t, 0, 1, 16).pow(2).mean().backward()
        grads[name] = [x.grad.clone() for x in scene.parameters()] + [q.grad, t.grad]
    for a, b in zip(grads["user"], grads["twin"]):
        assert (a - b).abs().max().item() <= 1e-5 * max(1.0, b.abs().max().item())
    # the whole-scene bounds agree too (same walk, same numbers)
    from ray_marching_amd import ops
    bu, bt = ops.scene_bound(user), ops.scene_bound(twin)
    assert torch.equal(bu[0], bt[0]) and bu[1:] == bt[1:]
    lu, lt = H.make_loop(user, h, w).to(torch.float16), H.make_loop(twin, h, w).to(torch.float16)      # fp16 module: cast last
    q, t = cams[0][0].half(), cams[0][1].half()
    for mode in (0, 4):
        with torch.no_grad():
            a, b = lu(q, t, mode, 1, steps), lt(q, t, mode, 1, steps)
        assert a.dtype == torch.float16 and _same(a, b)


def _variants(make, envs, pts, wts, pose, monkeypatch):
    """Values, point gradients, four frames and the parameter gradients of two backward passes for every program variant."""
    from ray_marching_amd import _abi, ops
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)      # bitwise parameter gradients: no atomically ordered deferred-ray list
    res = []
    for env in envs:
        scene, cs = _on_device(make, env)
        assert cs.lib().rm_user_leaves() == len(cs.user_leaves) >= 1
        p = pts.clone().requires_grad_(True)
        d = scene(p)
        (d * wts).sum().backward()
        gw = [x.grad.clone() for x in scene.parameters()]
        loop = H.make_loop(scene, 40, 72)
        q, t = pose
        with torch.no_grad():
            frames = [loop(q, t, m, 1, 48) for m in (0, 4, 2, 5)]
        for x in scene.parameters():
            x.grad = None
        loop(q, t, 0, 1, 24).pow(2).mean().backward()
        res.append(dict(env=env, cs=cs, d=d.detach(), gp=p.grad, frames=frames, gw=gw, gf=[x.grad.clone() for x in scene.parameters()],
                        min=_covered(cs.program, _abi.OP_CULL_MIN), lse=_covered(cs.program, _abi.OP_CULL_LSE)))
    ref = res[0]
    assert not ref["min"] and not ref["lse"] and not np.isin(ref["cs"].program.reshape(-1, 4)[:, 0], (_abi.OP_CULL_MIN, _abi.OP_CULL_LSE)).any()
    for got in res[1:]:
        assert _same(ref["d"], got["d"]) and _same(ref["gp"], got["gp"]), got["env"]
        for x, y in zip(ref["frames"], got["frames"]):
            assert _same(x, y), got["env"]
        for name in ("gw", "gf"):
            for x, y in zip(ref[name], got[name]):
                assert _same(x, y), (got["env"], name)
    return res


def _coherent_waves(case, gen):
    centres = (torch.rand(64, 1, 3, generator=gen) * 2 - 1) * 2.5
    if case == "tight_neighbour":      # half of the waves at the far end of the long link
        centres[:32] = torch.tensor(TIGHT_END) + 0.05 * (torch.rand(32, 1, 3, generator=gen) * 2 - 1)
    pts = (centres + (0.01 if case == "tight_neighbour" else 0.05) * torch.randn(64, 64, 3, generator=gen)).reshape(-1, 3).to(DEV)
    return pts, torch.randn(pts.shape[0], 1, generator=gen).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["siblings", "blob", "tight_neighbour"])
def test_culling_over_a_bounded_link_changes_no_bit(case, monkeypatch):
    """The three scenes of tests/test_user_leaf.py's culling test with the bounded link: now a CULL_MIN / CULL_LSE range
    CONTAINS the leaf, so its bound decides whether it is evaluated.  Compiled without cull tests, by default, with a test
    in front of every boundable child and with the exact logsumexp culling: values, gradients and frames are the same bits."""
    _register()
    pts, wts = _coherent_waves(case, torch.Generator().manual_seed(5))
    q, t = _pose(-3.5)
    if case == "tight_neighbour":      # close to the link's far end, looking at it
        t = torch.tensor([[TIGHT_END[0], TIGHT_END[1], -1.0]], device=DEV)
    res = _variants(CULL_SCENES[case], CULL_ENVS, pts, wts, (q, t), monkeypatch)
    print(f"culling leg {case}: USER rows under a CULL_MIN per variant {[len(r['min']) for r in res]}, under a CULL_LSE {[len(r['lse']) for r in res]}")
    assert res[1]["min"] and res[2]["min"], "no CULL_MIN range contains the bounded leaf"
    if case != "siblings":
        assert res[3]["lse"], "no CULL_LSE range contains the bounded leaf"


@pytest.mark.gpu
def test_conservative_leaf_under_a_non_unit_quaternion(monkeypatch):
    """Slope composition: HalfBall signs slope 0.6; its affine node (|q|^2 = 0.97) multiplies that by 0.94.  The composed
    bound is finite, is the one rm_scene_bound reports, and the cull test that uses it changes no bit."""
    from ray_marching_amd import ops
    _register()
    pts, wts = _coherent_waves("halfball", torch.Generator().manual_seed(6))
    res = _variants(halfball_scene, [CULL_OFF, {}], pts, wts, _pose(-3.5), monkeypatch)
    assert res[1]["min"], "no CULL_MIN range contains the HalfBall"
    c, R, slope, Ru, uslope = ops.scene_bound(halfball_holder().to(DEV))
    print(f"HalfBall under |q|^2 = 0.97: centre {c.tolist()}, R {R}, slope {slope}, Ru {Ru}, uslope {uslope}")
    s2 = sum(x * x for x in HALF_Q)
    assert math.isfinite(R) and slope == pytest.approx(0.6 * (2 * s2 - 1 - 1e-5), rel=1e-4) and 0.5 < slope < 0.6
    assert c.tolist() == pytest.approx([-0.8, 0.2, 0.3], abs=1e-6) and Ru == math.inf
    assert R == pytest.approx(0.3 * 1.0001 + 1e-4 * 1.3, rel=1e-4)


@pytest.mark.gpu
def test_scene_bound_against_hand_computed_numbers(monkeypatch):
    """rm_scene_bound.  The walker's own arithmetic (csrc/rm_device.h: subtree_bound): a leaf gives its sphere as is; an
    affine node with a unit quaternion moves the centre by its translation t, multiplies the slope by 1 - 1e-5 and turns R
    into 1.0001 R + 1e-4 |t + c|_1; a capsule's half length is inflated by 1.00001; 1e-4 relative covers the rest."""
    from ray_marching_amd import _abi, ops, specialize
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.contrib import SDFBoundedLink, SDFLink
    from ray_marching_amd.scene.primitives import SDFLine, SDFPlane, SDFSphere
    from ray_marching_amd.scene.scene_registry import make_test_scene2
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    _register()
    approx = lambda x: pytest.approx(x, rel=1e-4)
    t = [1.0, -2.0, 3.0]
    moved = lambda: A(SDFSphere(0.5), orientation=IDENT, translation=t)
    capsule = lambda: SDFLine(start=(1.0, 0.5, 0.0), end=(-1.0, 0.5, 2.0), radius=0.1)
    room_R = math.sqrt(75.0) + 0.1           # scene 2: everything lies inside the room's sphere
    for policy in ("off", "prebuilt"):       # the interpreter (generic library), then specialised libraries where build() made one
        monkeypatch.setenv("RM_SPECIALIZE", policy)
        specialize._loaded.clear()
        for make, special in ((lambda: SDFSphere(0.5), True), (make_test_scene2, True), (moved, False), (capsule, False),
                              (SDFPlane, False), (lambda: SDFUnion([SDFSphere(0.5), SDFPlane()]), False)):
            scene = make().to(DEV)
            cs = compile_scene(scene)
            assert (cs.lib() is not _abi.lib) == (policy == "prebuilt" and special)
            c, R, slope, Ru, uslope = ops.scene_bound(cs, DEV)
            if make is moved:
                assert c.tolist() == t and R == approx(0.5 * 1.0001 + 1e-4 * 6.0) and Ru == approx(0.5 * 1.0001 + 1e-4 * 6.0)
                assert slope == approx(1 - 1e-5) and uslope == approx(1 + 1e-5)
            elif make is capsule:
                assert c.tolist() == [0.0, 0.5, 1.0] and R == approx(math.sqrt(2.0) + 0.1) and Ru == approx(math.sqrt(2.0) + 0.1)
            elif make is make_test_scene2:
                assert c.tolist() == [0.0, 0.0, 0.0] and R == approx(room_R) and slope == 1.0 and Ru == math.inf      # (a union has no upper bound)
            elif special:
                assert (c.tolist(), R, slope, Ru, uslope) == ([0.0, 0.0, 0.0], 0.5, 1.0, 0.5, 1.0)
            else:
                assert R == math.inf and Ru == math.inf
    monkeypatch.delenv("RM_SPECIALIZE")
    specialize._loaded.clear()
    # user leaves: their own numbers, through the affine rule; without NAME_bound: none
    assert ops.scene_bound(BSphere(0.5).to(DEV))[1:] == (0.5, 1.0, 0.5, 1.0)
    c, R, slope, Ru, uslope = ops.scene_bound(HalfBall(0.5).to(DEV))
    assert (R, slope, Ru, uslope) == (approx(0.3), approx(0.6), math.inf, 1.0)
    c, R, slope, Ru, uslope = ops.scene_bound(SDFBoundedLink(**LINK).to(DEV))
    assert c.tolist() == [0.0, 0.0, 0.0] and R == Ru == approx(0.73) and slope == uslope == 1.0
    c, R, slope, Ru, uslope = ops.scene_bound(moved_bsphere().to(DEV))
    assert c.tolist() == [0.5, -0.25, 1.0] and R == approx(0.4 * 1.0001 + 1e-4 * 1.75) and Ru == approx(0.4 * 1.0001 + 1e-4 * 1.75)
    assert slope == approx(1 - 1e-5) and uslope == approx(1 + 1e-5)
    for unbounded in (NoBound(0.5), SDFLink(**LINK)):
        b = ops.scene_bound(unbounded.to(DEV))
        assert b[1] == math.inf and b[3] == math.inf
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.scene_bound(BSphere(0.5))


@pytest.mark.gpu
def test_the_bound_follows_the_live_parameters():
    """NAME_bound runs on the device at staging time, from the parameters the launch reads: after an in-place edit, a
    .data write and an optimiser step the culled program still renders the frames of the program without cull tests, and
    rm_scene_bound has moved; a negative or NaN parameter gives "no bound" (and the same frames)."""
    from ray_marching_amd import _abi, ops
    _register()
    culled, cs = _on_device(live_scene, dict(RM_CULL_MIN_COST="0"))
    plain, cs0 = _on_device(live_scene, CULL_OFF)
    assert len(_covered(cs.program, _abi.OP_CULL_MIN)) == 2 and not _covered(cs0.program, _abi.OP_CULL_MIN)
    loops = [H.make_loop(s, 40, 72) for s in (culled, plain)]
    q, t = _pose(-3.0)
    leaves = lambda s: (s.sdfs[1].sdf, s.sdfs[2].sdf)                    # (BSphere, SDFBoundedLink)

    def frames_agree(what):
        with torch.no_grad():
            for mode in (0, 4, 1):
                a, b = (loop(q, t, mode, 1, 48) for loop in loops)
                assert _same(a, b), (what, mode)
        return ops.scene_bound(leaves(culled)[0])[1], ops.scene_bound(leaves(culled)[1])[1]

    r0, l0 = frames_agree("as built")
    assert r0 == 0.5 and l0 == pytest.approx(0.73, rel=1e-6)
    for s in (culled, plain):
        with torch.no_grad():
            leaves(s)[0].radius += 0.25
            leaves(s)[1].length.mul_(2.0)
    r1, l1 = frames_agree("in place")
    assert r1 == 0.75 and l1 == pytest.approx(1.08, rel=1e-6)
    for s in (culled, plain):
        leaves(s)[0].radius.data = torch.tensor(0.3, device=DEV)
        leaves(s)[1].length.data = torch.tensor(0.1, device=DEV)
    r2, l2 = frames_agree(".data")
    assert r2 == pytest.approx(0.3, rel=1e-6) and l2 == pytest.approx(0.48, rel=1e-6)
    for s in (culled, plain):
        moving = [leaves(s)[0].radius, leaves(s)[1].length]
        opt = torch.optim.SGD(moving, lr=0.5)
        for x in moving:
            x.grad = torch.full_like(x, -1.0)
        opt.step()
    r3, l3 = frames_agree("optimiser step")
    assert r3 == pytest.approx(0.8, rel=1e-6) and l3 == pytest.approx(0.98, rel=1e-6)
    for s in (culled, plain):
        with torch.no_grad():
            leaves(s)[0].radius.fill_(-0.2)
    r4, l4 = frames_agree("negative radius")
    assert r4 == math.inf and l4 == l3
    for s in (culled, plain):
        with torch.no_grad():
            leaves(s)[0].radius.fill_(0.5)
            leaves(s)[1].length.fill_(float("nan"))
    r5, l5 = frames_agree("NaN length")
    assert r5 == 0.5 and l5 == math.inf


@pytest.mark.gpu
def test_the_bound_is_consumed_and_check_bound_catches_a_wrong_one():
    """Liar evaluates a sphere of 0.5 around the origin but signs a sphere of 0.1 around (40, 0, 0).  Behind a cheap child,
    waves near the origin skip it (the default program answers the cheap child's distance, the program without cull tests
    the Liar's): the bound is consumed, not just carried.  check_bound names a point where it fails; the honest leaves pass.
    Wrong numbers on purpose, nothing else: evaluation only, every access in range."""
    from ray_marching_amd import _abi
    from ray_marching_amd.contrib import SDFBoundedLink
    from ray_marching_amd.extensions import check_bound
    _register()
    gen = torch.Generator().manual_seed(9)
    pts = (0.3 * (torch.rand(64, 1, 3, generator=gen) * 2 - 1) + 0.05 * torch.randn(64, 64, 3, generator=gen)).reshape(-1, 3).to(DEV)
    plain, cs0 = _on_device(liar_scene, CULL_OFF)
    culled, cs = _on_device(liar_scene, {})
    assert _covered(cs.program, _abi.OP_CULL_MIN) and not _covered(cs0.program, _abi.OP_CULL_MIN)
    with torch.no_grad():
        true, wrong = plain(pts), culled(pts)
    sphere, cheap = pts.norm(dim=-1, keepdim=True) - 0.5, (pts - torch.tensor([3.0, 0.0, 0.0], device=DEV)).norm(dim=-1, keepdim=True) - 0.1
    assert (true - sphere).abs().max().item() <= 1e-5, "without cull tests the Liar decides the minimum near the origin"
    assert (wrong - cheap).abs().max().item() <= 1e-5, "with its cull test the Liar was not skipped: the bound is not consumed"
    assert (wrong - true).min().item() > 2.0
    with pytest.raises(ValueError, match=r"lower bound of Liar fails .* at p = \["):
        check_bound(Liar(0.5).to(DEV))
    for leaf in (BSphere(0.5), HalfBall(0.5), SDFBoundedLink(**LINK)):
        c, R, slope, Ru, uslope = check_bound(leaf.to(DEV))
        assert math.isfinite(R) and 0.5 < slope <= 1.0
    with pytest.raises(ValueError, match="nobound_bound"):
        check_bound(NoBound(0.5).to(DEV))


@pytest.mark.gpu
def test_training_step_moves_a_perturbed_bounded_link_back(monkeypatch):
    """tests/test_user_leaf.py's training leg on make_link_scene(bounded=True): 20 captured Adam steps, each giving the loss
    of the eager step from the same parameters, the last loss below the first.  Then, without the atomically ordered
    deferred-ray list, the per-step losses of the culled program and of the program without cull tests: the same bits."""
    from ray_marching_amd import _abi, ops
    from ray_marching_amd.contrib import make_link_scene
    h, w, steps = 64, 96, 32
    q, t = _pose(-1.5)
    with torch.no_grad():
        target = H.make_loop(make_link_scene(bounded=True), h, w)(q, t, 4, 1, steps).clone()
    loss_fn = lambda image: (image - target).pow(2).mean()

    def perturbed(env):
        scene, cs = _on_device(lambda: make_link_scene(bounded=True), env)
        holder = scene.sdfs[1].sdfs[1]                      # the affine node that places the link
        with torch.no_grad():
            holder.sdf.length += 0.04; holder.sdf.radius1 -= 0.03; holder.sdf.radius2 += 0.015
            holder.translation += torch.tensor([0.04, -0.03, 0.03], device=DEV)
        return scene, list(holder.parameters()), cs

    def train(env, against_eager):
        scene, moving, cs = perturbed(env)
        assert bool(_covered(cs.program, _abi.OP_CULL_MIN)) == (env != CULL_OFF)
        loop = H.make_loop(scene, h, w)
        opt = torch.optim.Adam(moving, lr=2e-3, capturable=True)
        step = loop.training_step(loss_fn, mode=4, marching_steps=steps, optimizer=opt)
        twin, _, _ = perturbed(env)
        twin_loop = H.make_loop(twin, h, w)
        with torch.no_grad():
            first = float(loss_fn(loop(q, t, 4, 1, steps)))
        losses = []
        for it in range(20):
            if it == 0:
                step(q, t)                                   # warm-up iterations, the capture, one replay
            if against_eager:
                with torch.no_grad():
                    for a, b in zip(twin.parameters(), scene.parameters()):
                        a.copy_(b)
            got = float(step(q, t))
            if against_eager:
                want = loss_fn(twin_loop(q, t, 4, 1, steps))
                want.backward()
                for x in twin.parameters():
                    x.grad = None
                assert abs(got - float(want.detach())) <= 1e-6 * max(1.0, abs(float(want.detach()))), (it, got, float(want.detach()))
            losses.append(got)
        return first, losses

    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*AccumulateGrad node's stream does not match.*")
        first, losses = train({}, True)
        print(f"training leg (bounded link): loss before {first:.6g}, per step {[round(x, 6) for x in losses]}")
        assert losses[-1] < first and losses[-1] < losses[0]
        monkeypatch.setattr(ops, "bwd_hard_capacity", 0)
        _, culled = train({}, False)
        _, plain = train(CULL_OFF, False)
    print(f"training leg (bounded link), no deferred-ray list: culled {culled[-1]!r}, without cull tests {plain[-1]!r}")
    assert culled == plain
