"""User-defined SDF combinators (ray_marching_amd/extensions.py: register_combinator): registration, the RM_OP_USER_FOLD /
RM_OP_USER_END program, the specialised libraries that carry the combinators' HIP source, and -- on the GPU -- parity of such
scenes with built-in twins (UMin restates SDFUnion), with CPU autograd through the combinators' own ``combine``, with
culling on and off around them, and through a captured training loop.

The CPU side of every GPU comparison is `cpu_eval()` below: ``combine`` of the combinator instance over the oracle's
evaluation (oracle.sdf_oracle.sdf_eval) of its children, the way tests/test_user_leaf.py::composition does for the link.
"""
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
# test-defined combinators
# --------------------------------------------------------------------------------------------------------------
class _Node(nn.Module):
    def __init__(self, sdfs):
        super().__init__()
        self.sdfs = nn.ModuleList(sdfs)

    def forward(self, query_coords):
        return self.combine(torch.stack([sdf(query_coords) for sdf in self.sdfs], dim=-2).squeeze(-1))


class UMin(_Node):
    """SDFUnion restated as a user combinator: the t_min chain of FOLD_MIN and the winner rule of UNION_END, so a scene built
    with it must agree with the built-in one bit for bit."""

    def combine(self, values):
        return values.unsqueeze(-1).min(dim=-2).values


UMIN_HIP = """
template <bool Fast, int N> RM_DEV float umin_fwd(const float (&d)[N], const float* theta) {
  float m = __builtin_inff();
#pragma unroll
  for (int i = 0; i < N; ++i) m = t_min(m, d[i]);
  return m;
}
template <bool Fast, int N> RM_DEV void umin_vjp(const float (&d)[N], const float* theta, float g, float (&gd)[N], float* gtheta) {
  float m = __builtin_inff();
#pragma unroll
  for (int i = 0; i < N; ++i) m = t_min(m, d[i]);
  int win = N - 1;
#pragma unroll
  for (int i = N - 1; i >= 0; --i)
    if (d[i] == m || (m != m && d[i] != d[i])) win = i;
#pragma unroll
  for (int i = 0; i < N; ++i) gd[i] = (i == win) ? g : 0.0f;
}
"""


class UScaledMax(_Node):
    """max_i(w_i d_i) over three children: a combinator with parameters of its own and more than two children."""

    def __init__(self, sdfs, w):
        super().__init__(sdfs)
        self.w = nn.Parameter(torch.tensor(w, dtype=torch.float32))

    def combine(self, values):
        return values.mul(self.w).unsqueeze(-1).max(dim=-2).values


USCALEDMAX_HIP = """
template <bool Fast, int N> RM_DEV float uscaledmax_fwd(const float (&d)[N], const float* theta) {
  float m = d[0] * theta[0];
#pragma unroll
  for (int i = 1; i < N; ++i) m = t_max(m, d[i] * theta[i]);
  return m;
}
template <bool Fast, int N> RM_DEV void uscaledmax_vjp(const float (&d)[N], const float* theta, float g, float (&gd)[N], float* gtheta) {
  float m = d[0] * theta[0];
#pragma unroll
  for (int i = 1; i < N; ++i) m = t_max(m, d[i] * theta[i]);
  bool open = true;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float x = d[i] * theta[i];
    const bool win = open && (x == m || (m != m && x != x));
    gd[i] = win ? g * theta[i] : 0.0f;
    gtheta[i] = win ? g * d[i] : 0.0f;
    open = open && !win;
  }
}
"""


def _register():
    from ray_marching_amd.extensions import register_combinator
    register_combinator(UMin, hip=UMIN_HIP, cost=2)
    register_combinator(UScaledMax, params=("w",), hip=USCALEDMAX_HIP, cost=8)


# --------------------------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------------------------
Q_ROT, IDENT = [0.9014, 0.25, 0.25, 0.25], [1.0, 0.0, 0.0, 0.0]


def scene2_with(union_cls):
    """make_test_scene2() with every SDFUnion replaced by ``union_cls``."""
    from ray_marching_amd.scene.primitives import SDFLine, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    return union_cls([make_room(), union_cls([SDFSphere(radius=0.5), SDFTorus(radius1=1.0, radius2=0.25),
                                              SDFLine(start=(1.0, 0.0, 0.0), end=(-1.0, 0.0, 0.0), radius=0.1)])])


def closed_scene_with(union_cls):
    """make_closed_test_scene() with its SDFUnion replaced by ``union_cls``."""
    from ray_marching_amd.scene.scene_registry import make_room, make_test_scene
    return union_cls([make_test_scene(), make_room()])


def mixed_scene():
    """CPU leg: two combinator classes, one of them at two arities, a user leaf among the children, and a min-union with a
    cullable child nested inside a combinator."""
    from ray_marching_amd.contrib import SDFIntersection, SDFLink
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFUnion
    return SDFUnion([
        make_room(),
        UScaledMax([SDFSphere(0.5), SDFLink(0.35, 0.3, 0.08), A(SDFBox((0.3, 0.2, 0.4)), orientation=Q_ROT, translation=[0.1, 0.0, 0.2])],
                   w=[1.0, 0.9, 0.8]),
        SDFIntersection([SDFUnion([SDFSphere(0.3), A(SDFTorus(0.5, 0.12), orientation=IDENT, translation=[1.1, 0.4, 0.5])]),
                         SDFBox((0.6, 0.6, 0.6))]),
        A(SDFIntersection([SDFSphere(0.4), SDFBox((0.3, 0.3, 0.3)), SDFSphere(0.45)]), orientation=Q_ROT, translation=[-1.0, 0.5, 0.0]),
    ])


def scaled_max_scene():
    """GPU leg: UScaledMax over two IDENTICAL spheres with equal weights (ties wherever they win) and a rotated box."""
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A
    return UScaledMax([SDFSphere(0.5), SDFSphere(0.5), A(SDFBox((0.3, 0.2, 0.4)), orientation=Q_ROT, translation=[0.1, 0.0, 0.2])],
                      w=[0.9, 0.9, 0.8])


def scaled_max_spec(dtype=torch.float32):
    box = ("affine", {"translation": O._t((0.1, 0.0, 0.2), dtype), "orientation": O._t(Q_ROT, dtype)},
           ("box", {"halfsides": O._t((0.3, 0.2, 0.4), dtype)}))
    node = UScaledMax([nn.Identity()] * 3, w=[0.9, 0.9, 0.8]).to(dtype)
    return ("comb", node, [("sphere", {"radius": O._t(0.5, dtype)}), ("sphere", {"radius": O._t(0.5, dtype)}), box])


def nested_scene():
    """Culling leg: an intersection under an affine node, under a smooth union, under a min-union next to the room and a
    bounded built-in sibling (an affine torus: the child that gets a CULL_MIN)."""
    from ray_marching_amd.contrib import SDFIntersection
    from ray_marching_amd.scene.primitives import SDFBox, SDFSphere, SDFTorus
    from ray_marching_amd.scene.scene_registry import make_room
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFSmoothUnion, SDFUnion
    carved = A(SDFIntersection([SDFBox((0.4, 0.4, 0.4)), SDFSphere(0.5)]), orientation=Q_ROT, translation=[-0.6, 0.1, 0.2])
    blob = SDFSmoothUnion([carved, A(SDFSphere(0.3), orientation=IDENT, translation=[-0.1, 0.3, 0.2])], blend_k=22.0)
    return SDFUnion([make_room(), blob,
                     A(SDFTorus(radius1=0.5, radius2=0.12), orientation=[0.0, 0.5 ** 0.5, 0.5 ** 0.5, 0.0], translation=[1.1, 0.4, 0.5])])


NESTED_ENVS = [dict(RM_CULL="0"), dict()]


def carved_spec(dtype=torch.float32, blend=0.15):
    """contrib.make_carved_scene() for cpu_eval(): ("comb", combinator instance, [children]) around oracle specs."""
    from ray_marching_amd.contrib import SDFIntersection, SDFSmoothSubtraction, SDFSubtraction
    two = [nn.Identity(), nn.Identity()]

    def placed(child, t, q=IDENT):
        return ("affine", {"translation": O._t(t, dtype), "orientation": O._t(q, dtype)}, child)

    inter = ("comb", SDFIntersection(two), [placed(("box", {"halfsides": O._t((0.5, 0.5, 0.5), dtype)}), (-0.7, 0.0, 0.0), Q_ROT),
                                            placed(("sphere", {"radius": O._t(0.66, dtype)}), (-0.7, 0.0, 0.0))])
    capsule = ("line", {"start": O._t((-1.6, 0.0, 0.0), dtype), "end": O._t((0.2, 0.0, 0.0), dtype), "radius": O._t(0.22, dtype)})
    smooth = ("comb", SDFSmoothSubtraction(two, blend=blend).to(dtype),
              [placed(("sphere", {"radius": O._t(0.5, dtype)}), (0.9, 0.0, 0.0)),
               placed(("sphere", {"radius": O._t(0.35, dtype)}), (0.9, 0.1, -0.45))])
    return ("union", {}, [O.scene_room(dtype), ("comb", SDFSubtraction(two), [inter, capsule]), smooth])


def cpu_eval(spec, p):
    """oracle.sdf_eval with one more node kind: ("comb", instance, children) = instance.combine of the children's values."""
    if spec[0] == "comb":
        return spec[1].combine(torch.cat([cpu_eval(c, p) for c in spec[2]], dim=-1))
    if spec[0] == "union":
        return torch.stack([cpu_eval(c, p) for c in spec[2]], dim=-2).min(dim=-2).values
    return O.sdf_eval(spec, p)


def cpu_parameters(spec):
    """Parameter tensors of a cpu_eval() spec in the scene's named_parameters() order (own first, then the children)."""
    if spec[0] == "comb":
        return list(spec[1].parameters()) + [x for c in spec[2] for x in cpu_parameters(c)]
    if spec[0] == "union":
        return [x for c in spec[2] for x in cpu_parameters(c)]
    return [v for _, v in O.spec_parameters(spec)]


def cpu_grad_spec(spec):
    """The same spec with every oracle tensor a leaf that requires grad (combinator instances carry nn.Parameters already)."""
    if spec[0] == "comb":
        return ("comb", spec[1], [cpu_grad_spec(c) for c in spec[2]])
    if spec[0] == "union":
        return ("union", {}, [cpu_grad_spec(c) for c in spec[2]])
    return O.map_spec(spec, lambda x: x.clone().requires_grad_(True))


def gpu_test_programs():
    """Every test-defined program the GPU legs launch: the CPU suite and build() compile their libraries, so that a GPU run of
    the same tree finds them; where they are missing the library builds itself on first use."""
    from ray_marching_amd import specialize
    from ray_marching_amd.compiler import compile_scene
    _register()
    out = [compile_scene(scene2_with(UMin)), compile_scene(closed_scene_with(UMin)), compile_scene(scaled_max_scene())]
    for env in NESTED_ENVS:
        with environment(**env):
            out.append(compile_scene(nested_scene()))
    return list({specialize.scene_hash(cs): cs for cs in out}.values())


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
NARY = ("template <bool Fast, int N> RM_DEV float NAME_fwd(const float (&d)[N], const float* theta) { return d[0]; }\n"
        "template <bool Fast, int N> RM_DEV void NAME_vjp(const float (&d)[N], const float* theta, float g, float (&gd)[N], "
        "float* gtheta) { gd[0] = g; }\n")


def test_registration_errors():
    from ray_marching_amd import contrib
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.extensions import combinator_spec, leaf_spec, register_combinator, register_leaf
    from ray_marching_amd.scene.primitives import SDFSphere
    from ray_marching_amd.scene.transformations import SDFUnion
    _register()
    node = UMin([SDFSphere(0.3)])
    assert combinator_spec(node).name == "umin" and combinator_spec(node).children == "sdfs" and leaf_spec(node) is None
    assert combinator_spec(SDFSphere(0.3)) is None and combinator_spec(nn.Linear(2, 2)) is None
    assert combinator_spec(contrib.SDFSmoothSubtraction([SDFSphere(0.3), SDFSphere(0.2)], 0.1)).params == ("blend",)
    register_combinator(UMin, hip=UMIN_HIP, cost=2)                                          # the same again: fine
    with pytest.raises(ValueError, match="already registered"):
        register_combinator(UMin, hip=UMIN_HIP.replace("gd[i] = (i == win)", "gd[i] = (win == i)"), cost=2)
    with pytest.raises(ValueError, match="already registered"):
        register_combinator(UMin, hip=UMIN_HIP, cost=3)

    class First(_Node):
        def combine(self, values):
            return values[..., :1]

    with pytest.raises(TypeError, match="not an nn.Module"):
        register_combinator(dict, hip=NARY.replace("NAME", "first"))
    with pytest.raises(TypeError, match="already a ray_marching_amd node"):
        register_combinator(SDFUnion, hip=NARY.replace("NAME", "first"))

    class NoCombine(nn.Module):
        def __init__(self, sdfs):
            super().__init__()
            self.sdfs = nn.ModuleList(sdfs)

        def forward(self, query_coords):
            return self.sdfs[0](query_coords)

    with pytest.raises(TypeError, match="combine"):
        register_combinator(NoCombine, hip=NARY.replace("NAME", "no_combine"))
    with pytest.raises(ValueError, match="exactly two device functions"):
        register_combinator(First, hip=NARY.replace("NAME_vjp", "other_vjp").replace("NAME", "first"))
    with pytest.raises(ValueError, match="already used by SDFLink"):                         # a registered LEAF owns `link`
        register_combinator(First, hip=NARY.replace("NAME", "link"))
    with pytest.raises(ValueError, match="already used by UMin"):
        register_combinator(First, hip=NARY.replace("NAME", "umin"))
    with pytest.raises(ValueError, match="already used by UMin"):                            # ... and the other way round
        class Flat(nn.Module):
            def forward(self, p):
                return p[..., :1]
        register_leaf(Flat, params=(), cost=1, hip=(
            "template <bool Fast> RM_DEV float umin_fwd(rm::V3 p, const float* theta) { return p.x; }\n"
            "template <bool Fast> RM_DEV void umin_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) { gp.x += g; }\n"))
    with pytest.raises(ValueError, match="inline assembly"):
        register_combinator(First, hip=NARY.replace("NAME", "first").replace("gd[0] = g;", 'asm volatile(""); gd[0] = g;'))
    assert combinator_spec(First([SDFSphere(0.3)])) is None                                  # none of the failures registered it

    # the children attribute: missing on the instance, empty, or not a sequence of modules
    class Elsewhere(First):
        pass

    register_combinator(Elsewhere, hip=NARY.replace("NAME", "elsewhere"), children="parts")
    with pytest.raises(ValueError, match="parts"):
        compile_scene(Elsewhere([SDFSphere(0.3)]))
    register_combinator(First, hip=NARY.replace("NAME", "first"))
    with pytest.raises(ValueError, match="at least one"):
        compile_scene(First([]))
    cs = compile_scene(First([SDFSphere(0.3)]))                                              # one child is fine
    assert cs.program.tolist() == [[1, 0, 0, 0], [20, 0, 0, 1], [21, 0, 0, 1]] and cs.user_combinators[0][:3] == ("first", 1, 0)
    # the cap on the children, named in the message
    from ray_marching_amd import _abi
    assert _abi.USER_COMB_MAX_CHILDREN == 16
    compile_scene(UMin([SDFSphere(0.1 + 0.01 * i) for i in range(16)]))
    with pytest.raises(ValueError, match="at most 16 children"):
        compile_scene(UMin([SDFSphere(0.1 + 0.01 * i) for i in range(17)]))

    class Gap(First):
        def __init__(self, sdfs):
            super().__init__(sdfs)
            self.a = nn.Parameter(torch.tensor(1.0)); self.b = nn.Parameter(torch.tensor(2.0)); self.c = nn.Parameter(torch.tensor(3.0))

    register_combinator(Gap, params=("a", "c"), hip=NARY.replace("NAME", "comb_gap"))        # b lies between them
    with pytest.raises(ValueError, match="not contiguous"):
        compile_scene(Gap([SDFSphere(0.3)]))


# signatures of two scenes without combinators, as compile_scene() gave them before this extension point existed
SIGNATURE_SCENE2 = (((9, 0, 0, 0), (2, 1, 0, 0), (16, 0, 2, 0), (10, 0, 0, 0), (17, 0, 20, 2305), (9, 0, 0, 0), (1, 4, 0, 0), (10, 0, 3, 0),
                     (6, 5, 0, 0), (10, 0, 4, 0), (4, 7, 14, 0), (10, 0, 5, 0), (11, 0, 3, 3), (10, 0, 1, 9), (11, 0, 0, 2)), 14, 11, 4, 6, 6)
SIGNATURE_LINK_SCENE = (((9, 0, 0, 0), (2, 1, 0, 0), (16, 0, 2, 0), (10, 0, 0, 0), (9, 0, 0, 0), (7, 4, 0, 0), (1, 11, 0, 0), (8, 4, 0, 0),
                         (10, 0, 3, 0), (7, 12, 0, 0), (19, 19, 0, 3), (8, 12, 0, 0), (10, 0, 4, 0), (11, 0, 3, 2), (10, 0, 1, 0), (11, 0, 0, 2)),
                        22, 0, 10, 5, 0, (('link', 3, '879f5b4409b7cbbf36a763329dfb181a3193a051'),))


def test_program_of_scenes_with_combinators():
    import copy
    import hashlib
    import pickle
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import compile_scene
    _register()
    assert (_abi.OP_USER_FOLD, _abi.OP_USER_END) == (20, 21)
    # ---- the shipped scene
    cs = compile_scene(contrib.make_carved_scene())
    rows = cs.program.reshape(-1, 4)
    offs = dict(zip(cs.leaf_names, cs.leaf_offsets))
    new = rows[rows[:, 0] >= 20].tolist()
    # slots: root union 0-2, the room's onion 3; subtraction 4-5 (+ gradients 6-7), intersection 8-9 (+ 10-11), smooth
    # subtraction 12-13 (+ 14-15).  Types in order of first appearance, parents before their children.
    assert new == [[20, 0, 8, 10], [20, 0, 9, 11], [21, 0, 8, (0 << 16) | (1 << 8) | 2],
                   [20, 0, 4, 6], [20, 0, 5, 7], [21, 0, 4, (0 << 16) | (0 << 8) | 2],
                   [20, 0, 12, 14], [20, 0, 13, 15], [21, offs["sdfs.2.blend"], 12, (1 << 16) | (2 << 8) | 2]]
    sha = lambda text: hashlib.sha1(text.encode()).hexdigest()
    assert cs.n_slots == 16 and cs.user_leaves == () and cs.user_combinators == (
        ("sdf_subtraction", 2, 0, sha(contrib._SUBTRACTION_HIP)), ("sdf_intersection", 2, 0, sha(contrib._INTERSECTION_HIP)),
        ("sdf_smooth_subtraction", 2, 1, sha(contrib._SMOOTH_SUBTRACTION_HIP)))
    assert cs.signature[-1] == cs.user_combinators and cs.signature[-2] == ()
    assert not (rows[:, 0] == _abi.OP_CULL_MIN).any()          # both solids hold a combinator: nothing to cull in this scene
    # ---- two classes, one of them at two arities, a user leaf
    scene = mixed_scene()
    cs = compile_scene(scene)
    rows = cs.program.reshape(-1, 4)
    offs = dict(zip(cs.leaf_names, cs.leaf_offsets))
    ends = rows[rows[:, 0] == _abi.OP_USER_END].tolist()
    # slots: root union 0-3, onion 4, UScaledMax 5-7 (+ 8-10), intersection of two 11-12 (+ 13-14), its nested union 15-16,
    # intersection of three 17-19 (+ 20-22)
    assert ends == [[21, offs["sdfs.1.w"], 5, (3 << 16) | (0 << 8) | 3], [21, 0, 11, (0 << 16) | (1 << 8) | 2],
                    [21, 0, 17, (0 << 16) | (2 << 8) | 3]]
    folds = rows[rows[:, 0] == _abi.OP_USER_FOLD][:, 2:].tolist()
    assert folds == [[5, 8], [6, 9], [7, 10], [11, 13], [12, 14], [17, 20], [18, 21], [19, 22]] and cs.n_slots == 23
    assert rows[rows[:, 0] == _abi.OP_USER].tolist() == [[19, offs["sdfs.1.sdfs.1.length"], 0, 3]]
    assert cs.user_leaves == (("link", 3, sha(contrib._LINK_HIP)),)
    assert cs.user_combinators == (("uscaledmax", 3, 3, sha(USCALEDMAX_HIP)), ("sdf_intersection", 2, 0, sha(contrib._INTERSECTION_HIP)),
                                   ("sdf_intersection", 3, 0, sha(contrib._INTERSECTION_HIP)))
    assert len(cs.user_combinator_sources) == 2               # one text per class, however many arities
    assert cs.signature[-2] == cs.user_leaves and cs.signature[-1] == cs.user_combinators
    # no cull test in front of a child that contains a combinator, even when every child is asked for one; the union nested
    # inside the intersection keeps its own
    with environment(RM_CULL_MIN_COST="0"):
        eager = compile_scene(mixed_scene()).program.reshape(-1, 4)
    sites = np.flatnonzero(eager[:, 0] == _abi.OP_CULL_MIN)
    assert len(sites) == 2                                     # the room (last of the root's children now) and the nested torus
    for i in sites:
        inside = eager[i + 1:i + (eager[i, 3] >> 8), 0]
        assert not ((inside == _abi.OP_USER_END) | (inside == _abi.OP_USER_FOLD)).any()
    nested = [i for i in sites if eager[i + 1, 0] == _abi.OP_AFFINE_PUSH]
    assert len(nested) == 1 and eager[nested[0] + 2, 0] == _abi.OP_TORUS
    end2 = int(np.flatnonzero((eager[:, 0] == _abi.OP_USER_END) & ((eager[:, 3] >> 8) & 255 == 1))[0])
    assert np.flatnonzero(eager[:, 0] == _abi.OP_USER_END)[0] < nested[0] < end2      # ... and lies inside the intersection's range
    # (default costs: the nested torus, 49 instructions, gets its test as well)
    default_sites = np.flatnonzero(rows[:, 0] == _abi.OP_CULL_MIN)
    assert len(default_sites) == 1 and rows[default_sites[0] + 2, 0] == _abi.OP_TORUS
    # ---- rm_validate_program
    ok = lambda prog, slots=cs.n_slots: _abi.lib.rm_validate_program(prog.ctypes.data, prog.shape[0], cs.n_params, cs.n_derived,
                                                                    cs.stack_floats, slots)
    err = lambda: _abi.lib.rm_last_error().decode()
    assert ok(cs.program) == 0
    first_end = int(np.flatnonzero(cs.program[:, 0] == _abi.OP_USER_END)[0])
    last_end = int(np.flatnonzero(cs.program[:, 0] == _abi.OP_USER_END)[-1])
    last_fold = int(np.flatnonzero(cs.program[:, 0] == _abi.OP_USER_FOLD)[-1])
    assert ok(cs.program, 22) == -2 and "slot" in err()       # the last gradient slot lies past the tape
    bad = cs.program.copy(); bad[last_fold, 2] = 99
    assert ok(bad) == -2 and "USER_FOLD slot out of range" in err()
    bad = cs.program.copy(); bad[last_end, 2] = 18             # 18 + 2 * 3 > 23
    assert ok(bad) == -2 and "USER_END slots out of range" in err()
    bad = cs.program.copy(); bad[last_end, 3] &= ~255          # n = 0
    assert ok(bad) == -2 and "combinator of 0 children" in err()
    bad = cs.program.copy(); bad[last_end, 3] = (bad[last_end, 3] & ~255) | 17
    assert ok(bad) == -2 and "combinator of 17 children (1 to 16)" in err()
    bad = cs.program.copy(); bad[first_end, 1] = cs.n_params - 2      # three floats of theta from there
    assert ok(bad) == -2 and "user combinator params out of range" in err()
    bad = cs.program.copy(); bad[first_end, 3] = (cs.n_params << 16) | 3
    assert ok(bad) == -2 and "user combinator params out of range" in err()
    bad = np.delete(cs.program, last_fold, axis=0)             # the last child's fold is gone
    assert ok(bad) == -2 and "the fold of child 2 (slot 19) is missing" in err()
    bad = cs.program.copy(); bad[last_fold, 3] -= 1            # a fold that leaves its gradient slot to its neighbour
    assert ok(bad) == -2 and "expects the fold of child 2 at instr" in err() and "gradient slot 22" in err()
    bad = np.delete(cs.program, int(np.flatnonzero(cs.program[:, 0] == _abi.OP_USER_FOLD)[0]), axis=0)      # a fold in the middle
    assert ok(bad) == -2 and "unbalanced" in err()
    # ---- scenes without combinators keep the signatures they had
    from ray_marching_amd.scene.scene_registry import make_test_scene2
    assert compile_scene(make_test_scene2()).signature == SIGNATURE_SCENE2
    link = compile_scene(contrib.make_link_scene())
    assert link.signature == SIGNATURE_LINK_SCENE and link.user_combinators == () and link.signature[-1] == link.user_leaves
    # ---- the sources are part of the library key; pickle / deepcopy keep the scene whole
    hdr = specialize.code_header(cs)
    assert "#define RM_USER_COMBINATORS 3" in hdr and "#define RM_USER_LEAVES 1" in hdr
    assert "uscaledmax_fwd<Fast, 3>" in hdr and "sdf_intersection_vjp<Fast, 2>" in hdr and "sdf_intersection_vjp<Fast, 3>" in hdr
    assert hdr.count("RM_DEV float sdf_intersection_fwd") == 1
    plain = specialize.code_header(compile_scene(make_test_scene2()))
    assert "RM_USER_COMBINATORS" not in plain and "RM_USER_LEAVES" not in plain
    assert "RM_USER_COMBINATORS" not in specialize.code_header(link)
    cs2 = pickle.loads(pickle.dumps(cs))
    assert cs2.user_combinators == cs.user_combinators and cs2.user_combinator_sources == cs.user_combinator_sources
    assert specialize.code_header(cs2) == hdr and specialize.scene_hash(cs2) == specialize.scene_hash(cs)
    cs3 = copy.deepcopy(cs)
    assert cs3.user_combinators == cs.user_combinators and specialize.code_header(cs3) == hdr
    assert compile_scene(copy.deepcopy(scene)).signature == cs.signature
    # ---- CPU points run the class's own PyTorch forward: children with a CPU path (user leaves), combine on their values
    from ray_marching_amd.contrib import SDFIntersection, SDFLink, SDFSmoothSubtraction
    a, b = SDFLink(0.35, 0.3, 0.08), SDFLink(0.2, 0.25, 0.05)
    p = _points(64)
    both = SDFIntersection([a, b])
    assert torch.equal(both(p), torch.maximum(a(p), b(p))) and both(p).shape == (64, 1)
    assert torch.equal(both(p), SDFIntersection._rm_torch_forward(both, p))
    smooth = SDFSmoothSubtraction([a, b], blend=0.15)
    x, y = a(p), -b(p)
    h = torch.relu(0.15 - (x - y).abs()) / 0.15
    assert torch.allclose(smooth(p), torch.maximum(x, y) + h * h * 0.15 / 4, rtol=0, atol=1e-6)
    assert [n for n, _ in smooth.named_parameters()][0] == "blend"


def test_specialised_library_cross_compiles_and_reports_its_combinators(monkeypatch, tmp_path):
    from concurrent.futures import ThreadPoolExecutor
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.scene.scene_registry import make_test_scene2
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    _register()
    cs = compile_scene(mixed_scene())
    # (one pool for this library and for those of the GPU legs: hipcc takes 15-40 s each)
    with ThreadPoolExecutor(max_workers=4) as ex:
        paths = list(ex.map(specialize.build, [cs, compile_scene(contrib.make_carved_scene()), compile_scene(contrib.make_link_scene()),
                                               compile_scene(make_test_scene2())] + gpu_test_programs()))
    assert all(os.path.isfile(p) for p in paths)
    monkeypatch.setenv("RM_SPECIALIZE", "prebuilt")
    specialize._loaded.clear()
    lib = cs.lib()
    assert lib is not _abi.lib and lib.rm_user_combinators() == 3 and lib.rm_user_leaves() == 1
    assert lib.rm_abi_version() == _abi.ABI_VERSION
    assert cs.lib(True) is lib and cs.specialised
    carved = compile_scene(contrib.make_carved_scene()).lib()
    assert carved.rm_user_combinators() == 3 and carved.rm_user_leaves() == 0
    assert _abi.lib.rm_user_combinators() == 0 and _abi.fast_lib().rm_user_combinators() == 0
    plain = compile_scene(make_test_scene2())
    assert plain.specialised and plain.lib().rm_user_combinators() == 0           # a specialised library of built-in nodes
    assert compile_scene(contrib.make_link_scene()).lib().rm_user_combinators() == 0
    assert "rm_user_combinators" in _abi.EXPORTED_SYMBOLS
    # the interpreter is never an option
    monkeypatch.setenv("RM_SPECIALIZE", "off")
    with pytest.raises(_abi.RmError, match="combinators: uscaledmax, sdf_intersection"):
        compile_scene(mixed_scene()).lib()
    with pytest.raises(_abi.RmError, match=r"user-defined combinators \(sdf_subtraction, sdf_intersection, sdf_smooth_subtraction\)"):
        compile_scene(contrib.make_carved_scene()).lib()
    with pytest.raises(_abi.RmError, match=r"user-defined leaves \(link\)"):      # leaf-only scenes read as they did
        compile_scene(contrib.make_link_scene()).lib()
    monkeypatch.setattr(specialize, "SPEC_DIR", str(tmp_path))
    monkeypatch.setenv("RM_SPECIALIZE", "prebuilt")
    specialize._loaded.clear()
    with pytest.raises(_abi.RmError, match="librm_spec_"):
        compile_scene(contrib.make_carved_scene()).lib()
    monkeypatch.setenv("RM_STATIC_BACKWARD_ACC", "8")
    with pytest.raises(_abi.RmError, match="RM_STATIC_BACKWARD_ACC"):
        compile_scene(contrib.make_carved_scene()).lib(True)
    monkeypatch.delenv("RM_STATIC_BACKWARD_ACC")
    # a combinator that does not compile: hipcc's own words reach the caller
    from ray_marching_amd.extensions import register_combinator
    from ray_marching_amd.scene.primitives import SDFSphere

    class Broken(_Node):
        def combine(self, values):
            return values[..., :1]

    register_combinator(Broken, hip=NARY.replace("NAME", "broken_comb").replace("return d[0];", "return no_such_helper(d[0]);"))
    monkeypatch.setenv("RM_SPECIALIZE", "jit")
    with pytest.raises(_abi.RmError, match="no_such_helper"):
        compile_scene(Broken([SDFSphere(0.3)])).lib()
    specialize._loaded.clear()


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scene2", "closed_scene1"])
def test_restated_union_is_bit_identical_with_the_builtin(which, monkeypatch):
    """Zero tolerance: UMin restates SDFUnion, so a scene with it in place of every SDFUnion and the built-in scene (culling
    on: it changes no bit) agree in every bit of every value, point gradient and frame; parameter and pose gradients to
    summation order."""
    from ray_marching_amd.compiler import compiled_for
    from ray_marching_amd.scene.transformations import SDFUnion
    _register()
    make = scene2_with if which == "scene2" else closed_scene_with
    user, twin = make(UMin).to(DEV), make(SDFUnion).to(DEV)
    lib = compiled_for(user).lib()
    assert lib.rm_user_combinators() == (2 if which == "scene2" else 1) and lib.rm_user_leaves() == 0 and compiled_for(twin).specialised
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
def test_carved_scene_against_cpu_autograd_and_the_stand_alone_modules():
    """contrib.make_carved_scene() (library prebuilt by build()) against cpu_eval(): values <= 1e-5, gradients <= 1e-4 (the
    contracts of smoke()); march positions <= 1e-5 or on a ray the CPU's own fp32 and fp64 marches split by more than that
    (at most 5 % of the frame may be excused); RenderLoop == the stand-alone chain; capture / display_frame == the frame."""
    from ray_marching_amd.compiler import compiled_for
    from ray_marching_amd.contrib import make_carved_scene
    scene = make_carved_scene().to(DEV)
    lib = compiled_for(scene).lib()
    assert lib.rm_user_combinators() == 3 and lib.rm_user_leaves() == 0
    spec = cpu_grad_spec(carved_spec())
    pts = _points(4096, seed=21)
    wts = torch.randn(4096, 1, generator=torch.Generator().manual_seed(22))
    pc = pts.clone().requires_grad_(True)
    want = cpu_eval(spec, pc)
    (want * wts).sum().backward()
    pg = pts.to(DEV).requires_grad_(True)
    got = scene(pg)
    (got * wts.to(DEV)).sum().backward()
    err = (got.detach().cpu() - want.detach()).abs().max().item()
    n_diff = int((got.detach().cpu() != want.detach()).sum())
    print(f"carved scene: scene(points) max|err| {err:.3g}; {n_diff} of 4096 values not bit-identical with the CPU composition")
    assert err <= 1e-5
    gerr = (pg.grad.cpu() - pc.grad).abs().max().item()
    print(f"carved scene: point gradient max|err| {gerr:.3g}")
    assert gerr <= 1e-4
    cpu_params = cpu_parameters(spec)
    names = [n for n, _ in scene.named_parameters()]
    assert len(cpu_params) == len(names) == 18 and names[11] == "sdfs.2.blend"
    for (name, g), c in zip(scene.named_parameters(), cpu_params):
        assert g.shape == c.shape, name
        cg = c.grad if c.grad is not None else torch.zeros_like(c)
        e = (g.grad.cpu() - cg).abs().max().item()
        print(f"carved scene: grad {name} max|err| {e:.3g} (|g| {cg.abs().max().item():.3g})")
        assert e <= 1e-4, name
    assert cpu_params[11].grad.abs().item() > 1e-3, "the blend takes part on too few points for this test to mean anything"
    # march, 64 x 96 rays, 32 steps, from two camera positions
    h, w, steps = 64, 96, 32
    loop = H.make_loop(scene, h, w)
    bufs = O.camera_buffers(1, w, h, H.PX * h, H.PX * w, H.PX * h)
    from ray_marching_amd.rendering.ray_marching import SDFMarcher
    for z in (-3.0, -1.5):
        q, t = _pose(z)
        marches = {}
        for dtype in (torch.float32, torch.float64):
            s = carved_spec(dtype)
            pos, _, dirs = O.camera_forward(bufs[0].to(dtype), bufs[1].to(dtype), q.cpu().to(dtype), t.cpu().to(dtype))
            with torch.no_grad():
                for _ in range(steps):
                    pos = cpu_eval(s, pos) * dirs + pos
            marches[dtype] = pos.double()
        with torch.no_grad():
            pos, frames, _, dirs = loop.camera(q, t)
            p_gpu = SDFMarcher(scene)(pos, dirs, steps)
        e = (p_gpu.cpu().double() - marches[torch.float32]).abs()
        ill = ((marches[torch.float32] - marches[torch.float64]).abs().max(dim=-1, keepdim=True).values > 1e-5)
        off = e > 1e-5
        n_exc = int(ill.sum())
        print(f"carved scene march from z = {z}: max|err| {e.max().item():.3g}; {int(off.sum())} coordinates beyond 1e-5, "
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
def test_combinator_with_parameters_and_three_children_against_cpu_autograd():
    """UScaledMax as the root: values <= 1e-5, point gradients (gd through the children) and parameter gradients (gtheta, and
    gd again through the children's parameters) <= 1e-4 against CPU autograd through its combine.  Two of the children are
    the same sphere with the same weight, so wherever it wins the maximum is a tie and the sub-gradient must go to the first
    child as on the CPU; a second batch has NaN coordinates, whose NaN pattern must match the CPU's."""
    from ray_marching_amd.compiler import compiled_for
    _register()
    scene = scaled_max_scene().to(DEV)
    assert compiled_for(scene).lib().rm_user_combinators() == 1
    spec = cpu_grad_spec(scaled_max_spec())
    pts = _points(4096, seed=41, lo=-1.0, hi=1.0)
    wts = torch.randn(4096, 1, generator=torch.Generator().manual_seed(42))
    pc = pts.clone().requires_grad_(True)
    want = cpu_eval(spec, pc)
    (want * wts).sum().backward()
    pg = pts.to(DEV).requires_grad_(True)
    got = scene(pg)
    (got * wts.to(DEV)).sum().backward()
    with torch.no_grad():
        kids = torch.cat([O.sdf_eval(c, pts) for c in spec[2]], dim=-1) * spec[1].w
        tied = int((kids[:, 0] >= kids[:, 2]).sum())
    assert 400 < tied < 3700, "the tied spheres decide the maximum on too few (or all) points for this test to mean anything"
    err = (got.detach().cpu() - want.detach()).abs().max().item()
    gerr = (pg.grad.cpu() - pc.grad).abs().max().item()
    print(f"scaled max: {tied} of 4096 points are ties; values max|err| {err:.3g}, point gradient max|err| {gerr:.3g}")
    assert err <= 1e-5 and gerr <= 1e-4
    cpu_params = cpu_parameters(spec)
    assert [n for n, _ in scene.named_parameters()][:3] == ["w", "sdfs.0.radius", "sdfs.1.radius"] and len(cpu_params) == 6
    for (name, g), c in zip(scene.named_parameters(), cpu_params):
        cg = c.grad if c.grad is not None else torch.zeros_like(c)
        e = (g.grad.cpu() - cg).abs().max().item()
        print(f"scaled max: grad {name} max|err| {e:.3g} (|g| {cg.abs().max().item():.3g})")
        assert e <= 1e-4, name
    # the tie sub-gradient: everything to the first sphere, nothing to its twin
    assert scene.sdfs[0].radius.grad.abs().item() > 1.0 and scene.sdfs[1].radius.grad.item() == 0.0 == cpu_params[2].grad.item()
    assert scene.w.grad[1].item() == 0.0 == cpu_params[0].grad[1].item()
    # NaN inputs: the same NaN pattern in values and point gradients
    bad = _points(256, seed=43, lo=-1.0, hi=1.0)
    bad[::4, 0] = float("nan"); bad[1::8, 2] = float("nan")
    pc = bad.clone().requires_grad_(True)
    want = cpu_eval(cpu_grad_spec(scaled_max_spec()), pc)
    want.sum().backward()
    pg = bad.to(DEV).requires_grad_(True)
    got = scene(pg)
    got.sum().backward()
    assert int(want.isnan().sum()) == 96 and torch.equal(got.detach().cpu().isnan(), want.detach().isnan())
    assert torch.equal(pg.grad.cpu().isnan(), pc.grad.isnan())
    clean = ~want.detach().isnan().squeeze(-1)
    assert (got.detach().cpu()[clean] - want.detach()[clean]).abs().max().item() <= 1e-5
    assert (pg.grad.cpu()[clean] - pc.grad[clean]).abs().max().item() <= 1e-4


@pytest.mark.gpu
def test_culling_around_a_nested_combinator_changes_no_bit(monkeypatch):
    """An intersection under an affine node under a smooth union under a min-union, next to the room and a bounded built-in
    sibling.  Compiled without cull tests (RM_CULL=0) and by default -- a CULL_MIN in front of the sibling, none over the
    smooth union that holds the combinator -- values, gradients and frames are the same bits."""
    from ray_marching_amd import _abi, ops
    from ray_marching_amd.compiler import compiled_for
    _register()
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)      # bitwise parameter gradients: no atomically ordered deferred-ray list
    gen = torch.Generator().manual_seed(5)
    centres = (torch.rand(64, 1, 3, generator=gen) * 2 - 1) * 2.5
    pts = (centres + 0.05 * torch.randn(64, 64, 3, generator=gen)).reshape(-1, 3).to(DEV)      # coherent waves: culls fire
    wts = torch.randn(pts.shape[0], 1, generator=gen).to(DEV)
    res = []
    for env in NESTED_ENVS:
        for k in ("RM_CULL", "RM_CULL_MIN_COST", "RM_CULL_LSE", "RM_CULL_LSE_MIN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        scene = nested_scene().to(DEV)
        cs = compiled_for(scene)
        rows = cs.program.reshape(-1, 4)
        sites = np.flatnonzero(rows[:, 0] == _abi.OP_CULL_MIN)
        for i in sites:
            assert not (rows[i + 1:i + (rows[i, 3] >> 8), 0] == _abi.OP_USER_END).any()
        assert cs.lib().rm_user_combinators() == 1
        p = pts.clone().requires_grad_(True)
        d = scene(p)
        (d * wts).sum().backward()
        gw = [x.grad.clone() for x in scene.parameters()]
        loop = H.make_loop(scene, 40, 72)
        q, t = _pose(-3.5)
        with torch.no_grad():
            frames = [loop(q, t, m, 1, 48) for m in (0, 4, 2, 5)]
        for x in scene.parameters():
            x.grad = None
        loop(q, t, 0, 1, 24).pow(2).mean().backward()
        res.append(dict(env=env, n_cull=len(sites), d=d.detach(), gp=p.grad, frames=frames, gw=gw,
                        gf=[x.grad.clone() for x in scene.parameters()]))
    assert res[0]["n_cull"] == 0 and res[1]["n_cull"] == 1, "the default compile did not put a cull test in front of the torus"
    ref, got = res
    assert _same(ref["d"], got["d"]) and _same(ref["gp"], got["gp"])
    for x, y in zip(ref["frames"], got["frames"]):
        assert _same(x, y)
    for name in ("gw", "gf"):
        for x, y in zip(ref[name], got[name]):
            assert _same(x, y), name


@pytest.mark.gpu
def test_training_step_moves_a_perturbed_carved_scene_back():
    """20 Adam steps on SDFSmoothSubtraction.blend and the pose of the sphere that is subtracted, towards a frame of the
    unperturbed scene: each replayed step of the captured graph gives the loss of the eager step taken from the same
    parameters (tolerance of test_training_step_helper_matches_the_eager_loop), and the last loss is below the first.  The
    loss is the MSE of the normal-shader image (mode 4), as in the link scene's training leg."""
    from ray_marching_amd.contrib import make_carved_scene
    h, w, steps = 64, 96, 32
    q, t = _pose(-1.5)
    with torch.no_grad():
        target = H.make_loop(make_carved_scene(), h, w)(q, t, 4, 1, steps).clone()
    loss_fn = lambda image: (image - target).pow(2).mean()

    def perturbed():
        scene = make_carved_scene().to(DEV)
        smooth = scene.sdfs[2]
        with torch.no_grad():
            smooth.blend += 0.05
            smooth.sdfs[1].translation += torch.tensor([0.04, -0.03, 0.03], device=DEV)
        return scene, [smooth.blend, smooth.sdfs[1].translation, smooth.sdfs[1].orientation]

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
