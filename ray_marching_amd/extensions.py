"""User-defined SDF leaves: an ``nn.Module`` with its own PyTorch ``forward`` plus two (or three) HIP device functions.

The scene compiler lowers a closed vocabulary (the reference's six primitives and five combinators).  This module
is the extension point: ``register_leaf`` teaches it one more *leaf* class, defined in the user's code, without
touching the mirrored ``scene/`` modules.  The class keeps its PyTorch ``forward`` -- that is what runs on CPU
tensors and inside the reference's own combinators, and it is the oracle the HIP code is tested against -- and
brings the same function as HIP source:

    template <bool Fast> RM_DEV float NAME_fwd(rm::V3 p, const float* theta);
    template <bool Fast> RM_DEV void  NAME_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta);

``theta`` is the leaf's parameter block (``params`` in ``named_parameters()`` order, flattened); the VJP adds
``g * grad_p f`` to ``gp`` and writes ``gtheta[i] = g * df/dtheta_i``.  ``Fast`` is the flag the built-in handlers
carry (1-ulp square roots and reciprocals inside a VJP's own forward half); INTEGRATION.md lists the helpers a leaf
may call and the contract it signs (an exact or conservative distance, a pure function of ``p`` and ``theta``, no
inline assembly).

A third function is optional, in the same source and with the same NAME (not a template: a bound has no fast variant):

    RM_DEV void NAME_bound(const float* theta, rm::LeafBound& b);

the leaf's bounding sphere, which is what lets the exact cull tests cover it like a built-in primitive (without one,
every min-union that holds the leaf loses its CULL_MIN).  ``b`` arrives as "nothing known" (``c = 0, R = +inf, slope = 1,
Ru = +inf, uslope = 1``); by filling it in the leaf signs, for every ``p`` and the ``theta`` it is handed,

    NAME_fwd(p) >= slope  * |p - c| - R     with 0.5 < slope <= 1      (needed for any culling)
    NAME_fwd(p) <= uslope * |p - c| + Ru    with 1 <= uslope < 8       (optional; logsumexp culling's nearest-child estimate)

and leaves ``R = +inf`` where it knows no bound for these parameters (a negative radius).  It runs on the device, once
per block, from the live parameters, so it follows in-place edits and optimiser steps; the margins the kernels need
are added by them, not by the leaf.  A wrong bound gives silently wrong pixels: run ``check_bound`` once per leaf.

User-defined *combinators* are the second half of the extension point: ``register_combinator`` teaches the compiler an
n-ary node whose value is a function of its children's values,

    template <bool Fast, int N> RM_DEV float NAME_fwd(const float (&d)[N], const float* theta);
    template <bool Fast, int N> RM_DEV void  NAME_vjp(const float (&d)[N], const float* theta, float g, float (&gd)[N], float* gtheta);

``d`` holds the children's values in the module's child order, ``theta`` the node's own parameters; the VJP writes
``gd[i] = g * df/dd_i`` and ``gtheta[j] = g * df/dtheta_j``.  ``N`` is a template parameter so that every index into ``d`` /
``gd`` is a compile-time constant after unrolling (loops over ``N`` carry ``#pragma unroll``): an array indexed at run time
goes to scratch memory.  The class keeps two PyTorch methods: ``combine(values [..., n]) -> [..., 1]``, the fold alone (the
CPU path and the oracle of the HIP code), and a ``forward`` that evaluates the children and calls it.  A combinator signs no
bound: no cull test covers a subtree that contains one (culling inside its children is untouched).

User-defined *domain operators* are the third: ``register_warp`` teaches the compiler a unary node that moves the query point
before its one child is evaluated and, optionally, edits the value the child returns (uniform scale, mirror symmetry,
repetition, elongation: what neither a leaf, which has no child, nor a combinator, which never sees the point, can say),

    template <bool Fast> RM_DEV rm::V3 NAME_fwd(rm::V3 p, const float* theta);
    template <bool Fast> RM_DEV void   NAME_vjp(rm::V3 p, const float* theta, rm::V3 gq, rm::V3& gp, float* gtheta);
    template <bool Fast> RM_DEV float  NAME_out_fwd(float d, rm::V3 p, const float* theta);
    template <bool Fast> RM_DEV void   NAME_out_vjp(float d, rm::V3 p, const float* theta, float g, float& gd, rm::V3& gp, float* gtheta);

``NAME_fwd`` returns the child's query point; its VJP adds ``J_p^T gq`` to ``gp`` and writes ``gtheta[i] = gq . dq/dtheta_i``.  The
``out`` pair is optional (both or neither, found in the source by name): the node's value from the child's value ``d``, with
``gd = g df/dd``, ``gp += g df/dp``, ``gtheta[i] = g df/dtheta_i``.  ``p`` is the point in the node's own frame in all four.  The
class keeps ``warp(points) -> points``, ``out(values, points) -> values`` where the source has the pair, and a ``forward`` that
is ``out(child(warp(p)), p)``.  The field must stay a conservative distance (Lipschitz <= 1): that is the user's to see to, as
for leaves.  A warp may sign a bound too, with the leaf's signature and under its own NAME,

    RM_DEV void NAME_bound(const float* theta, rm::LeafBound& b);

but ``b`` ARRIVES holding the child's bound in the child's frame (``child(q) >= b.slope |q - b.c| - b.R`` and ``child(q) <= b.uslope
|q - b.c| + b.Ru``, ``Ru = +inf`` where the child has none) and LEAVES holding the node's bound in the node's own frame, for the
node's final value (its ``out`` included): ``node(p) >= slope' |p - c'| - R'`` with ``0.5 < slope' <= 1`` and, optionally, ``node(p) <=
uslope' |p - c'| + Ru'``.  A scale maps the child's sphere, a mirror widens it; ``R = +inf`` says "no bound for these parameters",
and a child without a bound keeps the node without one whatever the function writes.  Without the function no cull test covers
a subtree that contains the warp (culling inside its child is untouched); ``check_bound`` takes a warp instance as well.

User-defined *shaders* are the fourth kind, and the only one that is no scene node: ``register_shader`` teaches the frame kernels a
per-pixel shader, passed to ``RenderLoop.forward`` (``capture``, ``training_step``, ``display_frame``) as ``mode``,

    template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta);
    template <bool Fast> RM_DEV void   NAME_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta);

``s`` holds the pixel's ray origin ``o``, direction ``v``, surface point ``p``, unit normal ``n``, the pose quaternion ``qw, qv`` and
``col2``, the third column of the camera rotation (``lap`` and ``dist`` read as 0); ``theta`` is the shader's own parameters,
flattened in ``named_parameters()`` order; ``g`` is dL/d(rgb); ``gs`` arrives zeroed, the VJP adds dL/d(input) into it and writes
``gtheta[i]``.  The class keeps its PyTorch ``forward(px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords,
surface_normals) -> [..., 3]`` untouched: called directly, a shader is the user's PyTorch code on whatever device its inputs
are on.  A (scene, shader) pair is compiled into one library (compiler.compiled_with_shader); the shader's parameters follow the
scene's in the parameter block and receive their gradients through the same accumulators.

Scenes that contain such a leaf, combinator or warp, and frames shaded by such a shader, run only through their per-scene specialised library (specialize.py), into which
the source is compiled; the LDS interpreter has no handler for them and ``CompiledScene.lib()`` says so instead of
rendering a wrong picture.
"""
from __future__ import annotations

import hashlib
import re
from dataclasses import dataclass

import torch
import torch.nn as nn

__all__ = ["register_leaf", "leaf_spec", "check_bound", "UserLeaf", "register_combinator", "combinator_spec", "UserCombinator",
           "register_warp", "warp_spec", "UserWarp", "register_shader", "shader_spec", "UserShader"]


@dataclass(frozen=True)
class UserLeaf:
    cls: type
    name: str           # NAME of NAME_fwd / NAME_vjp
    params: tuple       # attribute names of the nn.Parameters, named_parameters() order
    hip: str
    cost: int           # VALU estimate per evaluation (compiler._cost)
    sha1: str           # of the source: part of the scene signature, hence of the library hash
    bounded: bool = False   # the source brings NAME_bound: cull tests may cover the leaf (read from the source, like NAME)


@dataclass(frozen=True)
class UserCombinator:
    cls: type
    name: str           # NAME of NAME_fwd / NAME_vjp
    params: tuple       # attribute names of the node's own nn.Parameters, named_parameters() order
    hip: str
    cost: int           # VALU estimate of the fold itself (compiler._cost adds the children's)
    sha1: str
    children: str       # attribute that holds the children (an nn.ModuleList or sequence of SDF modules)


@dataclass(frozen=True)
class UserWarp:
    cls: type
    name: str           # NAME of NAME_fwd / NAME_vjp (/ NAME_out_fwd / NAME_out_vjp)
    params: tuple       # attribute names of the node's own nn.Parameters, named_parameters() order
    hip: str
    cost: int           # VALU estimate of the map (and the `out`) itself (compiler._cost adds the child's)
    sha1: str
    child: str          # attribute that holds the one child
    has_out: bool       # the source brings NAME_out_fwd / NAME_out_vjp (and the class an ``out`` method)
    bounded: bool = False   # the source brings NAME_bound: cull tests may cover the node where its child is boundable too


@dataclass(frozen=True)
class UserShader:
    cls: type
    name: str           # NAME of NAME_fwd / NAME_vjp
    params: tuple       # attribute names of the shader's nn.Parameters, named_parameters() order
    hip: str
    sha1: str


_registry: dict[type, UserLeaf] = {}
_combinators: dict[type, UserCombinator] = {}
_warps: dict[type, UserWarp] = {}
_shaders: dict[type, UserShader] = {}

_DEF = r"\b([A-Za-z_]\w*)_%s\s*\("


def _identifier(hip: str) -> str:
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", hip, flags=re.S)
    fwd, vjp = (set(re.findall(r"RM_DEV\s+%s\s+" % ret + _DEF % kind, text)) for ret, kind in (("float", "fwd"), ("void", "vjp")))
    if len(fwd) != 1 or fwd != vjp:
        raise ValueError("hip must define exactly two device functions, `template <bool Fast> RM_DEV float NAME_fwd(rm::V3 p, "
                         "const float* theta)` and `template <bool Fast> RM_DEV void NAME_vjp(rm::V3 p, const float* theta, "
                         f"float g, rm::V3& gp, float* gtheta)`, with one NAME (found fwd: {sorted(fwd)}, vjp: {sorted(vjp)})")
    if re.search(r"\basm\b|__asm", text):
        raise ValueError("a user leaf must not contain inline assembly (INTEGRATION.md: leaf contract)")
    return fwd.pop()


def _combinator_identifier(hip: str) -> str:
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", hip, flags=re.S)
    fwd, vjp = (set(re.findall(r"RM_DEV\s+%s\s+" % ret + _DEF % kind, text)) for ret, kind in (("float", "fwd"), ("void", "vjp")))
    if len(fwd) != 1 or fwd != vjp:
        raise ValueError("hip must define exactly two device functions, `template <bool Fast, int N> RM_DEV float NAME_fwd(const "
                         "float (&d)[N], const float* theta)` and `template <bool Fast, int N> RM_DEV void NAME_vjp(const float "
                         f"(&d)[N], const float* theta, float g, float (&gd)[N], float* gtheta)`, with one NAME (found fwd: "
                         f"{sorted(fwd)}, vjp: {sorted(vjp)})")
    if re.search(r"\basm\b|__asm", text):
        raise ValueError("a user combinator must not contain inline assembly (INTEGRATION.md: combinator contract)")
    return fwd.pop()


def _warp_identifier(hip: str):
    """(NAME, has_out) of a warp source.  NAME is that of the one V3-returning ``NAME_fwd``; ``NAME_vjp`` must be there, and
    ``NAME_out_fwd`` / ``NAME_out_vjp`` come as a pair or not at all (looked up by their full names, like NAME_bound)."""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", hip, flags=re.S)
    fwd = set(re.findall(r"RM_DEV\s+(?:rm::)?V3\s+" + _DEF % "fwd", text))
    name = next(iter(fwd)) if len(fwd) == 1 else None

    def defines(ret, fn):
        return re.search(r"RM_DEV\s+%s\s+%s\s*\(" % (ret, re.escape(fn)), text) is not None

    if name is None or not defines("void", f"{name}_vjp"):
        raise ValueError("hip must define `template <bool Fast> RM_DEV rm::V3 NAME_fwd(rm::V3 p, const float* theta)` and `template "
                         "<bool Fast> RM_DEV void NAME_vjp(rm::V3 p, const float* theta, rm::V3 gq, rm::V3& gp, float* gtheta)`, with "
                         f"one NAME (found fwd: {sorted(fwd)})")
    out_fwd, out_vjp = defines("float", f"{name}_out_fwd"), defines("void", f"{name}_out_vjp")
    if out_fwd != out_vjp:
        raise ValueError(f"hip may define `template <bool Fast> RM_DEV float {name}_out_fwd(float d, rm::V3 p, const float* theta)` and "
                         f"`template <bool Fast> RM_DEV void {name}_out_vjp(float d, rm::V3 p, const float* theta, float g, float& gd, "
                         f"rm::V3& gp, float* gtheta)`: both or neither (found {name}_out_fwd: {out_fwd}, {name}_out_vjp: {out_vjp})")
    if re.search(r"\basm\b|__asm", text):
        raise ValueError("a user warp must not contain inline assembly (INTEGRATION.md: warp contract)")
    return name, out_fwd


def _shader_identifier(hip: str) -> str:
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", hip, flags=re.S)
    fwd, vjp = (set(re.findall(r"RM_DEV\s+%s\s+" % ret + _DEF % kind, text)) for ret, kind in ((r"(?:rm::)?V3", "fwd"), ("void", "vjp")))
    if len(fwd) != 1 or fwd != vjp:
        raise ValueError("hip must define exactly two device functions, `template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, "
                         "const float* theta)` and `template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, "
                         f"rm::V3 g, rm::ShadeGrad& gs, float* gtheta)`, with one NAME (found fwd: {sorted(fwd)}, vjp: {sorted(vjp)})")
    if re.search(r"\basm\b|__asm", text):
        raise ValueError("a user shader must not contain inline assembly (INTEGRATION.md: shader contract)")
    return fwd.pop()


def _has_bound(hip: str, name: str, what: str = "leaf") -> bool:
    """Whether the source defines ``RM_DEV void NAME_bound(`` (at most one, the own NAME of the leaf or warp, not a template)."""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", hip, flags=re.S)
    found = re.findall(r"(template\s*<[^<>]*>\s*)?RM_DEV\s+void\s+" + _DEF % "bound", text)
    if not found:
        return False
    want = f"`RM_DEV void {name}_bound(const float* theta, rm::LeafBound& b)`"
    if len(found) > 1:
        raise ValueError(f"hip may define at most one bound function, {want}" + ("" if what == "leaf" else f" of the {what} {name!r}")
                         + f" (found: {sorted(n for _, n in found)})")
    template, got = found[0]
    if got != name:
        raise ValueError(f"the bound function of the {what} {name!r} must be {want}, found {got}_bound")
    if template:
        raise ValueError(f"{want}" + ("" if what == "leaf" else f" of the {what} {name!r}") + " must not be a template: a bound has no fast variant")
    return True


def _device_forward(self, *args, **kwargs):
    """forward() installed by register_leaf: CUDA points go to the HIP evaluator (the leaf as a one-node scene), anything
    else to the class's own PyTorch forward."""
    points = args[0] if args else next(iter(kwargs.values()))
    if isinstance(points, torch.Tensor) and points.is_cuda:
        from .scene._base import SDFNode
        return SDFNode._evaluate(self, points)
    return type(self)._rm_torch_forward(self, *args, **kwargs)


def _torch_forward(cls):
    """The PyTorch forward of ``cls``: the first one in its MRO that is not the forward installed here (a subclass of a
    registered class inherits _device_forward; its base keeps the original under _rm_torch_forward)."""
    for c in cls.__mro__:
        f = c.__dict__.get("forward")
        if f is _device_forward:
            f = c.__dict__["_rm_torch_forward"]
        if f is not None:
            return f
    raise TypeError(f"register_leaf: {cls.__name__} has no forward")


def _registered_class(cls, registry=None):
    registry = _registry if registry is None else registry
    for c in cls.__mro__:
        if c in registry:
            return c
    return None


def register_leaf(cls, *, params, hip: str, cost: int):
    """Make ``cls`` (an ``nn.Module`` subclass with a PyTorch ``forward``) compilable as a scene leaf.

    params: names of its ``nn.Parameter`` attributes in ``named_parameters()`` order (may be empty).
    hip:    source of NAME_fwd / NAME_vjp (module docstring).
    cost:   VALU instructions per evaluation, roughly (a sphere is 13, a torus 24); only steers cull placement.

    Registering a class again with the same source is a no-op; with other source, parameters or cost it is an error
    (libraries already built from the first registration would no longer describe the class)."""
    if not (isinstance(cls, type) and issubclass(cls, nn.Module)):
        raise TypeError(f"register_leaf: {cls!r} is not an nn.Module subclass")
    if getattr(cls, "_rm_kind", None) is not None:
        raise TypeError(f"register_leaf: {cls.__name__} is already a ray_marching_amd node")
    params = tuple(params)
    if not all(isinstance(p, str) for p in params) or len(set(params)) != len(params):
        raise ValueError("register_leaf: params must be distinct attribute names")
    name = _identifier(hip)
    spec = UserLeaf(cls, name, params, hip, int(cost), hashlib.sha1(hip.encode()).hexdigest(), _has_bound(hip, name))
    if spec.cost < 0:
        raise ValueError("register_leaf: cost must be >= 0")
    old = _registry.get(cls)
    if old is not None:
        if (old.sha1, old.params, old.cost) != (spec.sha1, spec.params, spec.cost):
            raise ValueError(f"register_leaf: {cls.__name__} is already registered with different source, parameters or cost")
        return cls
    for other in list(_registry.values()) + list(_combinators.values()) + list(_warps.values()) + list(_shaders.values()):
        if other.name == spec.name:          # (the user types of one scene are compiled into one translation unit)
            raise ValueError(f"register_leaf: the identifier {spec.name!r} is already used by {other.cls.__name__}")
    if _registered_class(cls, _combinators) is not None:
        raise TypeError(f"register_leaf: {cls.__name__} is already registered as a combinator")
    if _registered_class(cls, _warps) is not None:
        raise TypeError(f"register_leaf: {cls.__name__} is already registered as a warp")
    if _registered_class(cls, _shaders) is not None:
        raise TypeError(f"register_leaf: {cls.__name__} is already registered as a shader")
    cls._rm_torch_forward = _torch_forward(cls)
    cls.forward = _device_forward
    _registry[cls] = spec
    return cls


def leaf_spec(node):
    """The registration of this module's class (or of the registered class it derives from), or None."""
    c = _registered_class(type(node))
    return None if c is None else _registry[c]


def register_combinator(cls, *, params=(), hip: str, cost: int = 4, children: str = "sdfs"):
    """Make ``cls`` (an ``nn.Module`` subclass) compilable as an n-ary scene node whose value is ``combine`` of its
    children's values.

    params:   names of the node's OWN ``nn.Parameter`` attributes in ``named_parameters()`` order (may be empty); a module's
              own parameters precede its children's, so they are contiguous in the scene block.
    hip:      source of NAME_fwd / NAME_vjp (module docstring).
    cost:     VALU instructions of the fold itself, roughly; the children's are added by the compiler.
    children: the attribute that holds the children, an ``nn.ModuleList`` or sequence of SDF modules, n >= 1.

    ``cls`` has ``combine(self, values [..., n]) -> [..., 1]`` and a ``forward(self, query_coords)`` that evaluates the
    children and calls it.  Registration installs the same dispatch as ``register_leaf``: CUDA points go to the HIP
    evaluator, anything else to the class's own forward (kept under ``_rm_torch_forward``).  Registering a class again with
    the same source is a no-op; with other source, parameters, cost or children attribute it is an error.  Identifiers are
    unique across leaves and combinators."""
    if not (isinstance(cls, type) and issubclass(cls, nn.Module)):
        raise TypeError(f"register_combinator: {cls!r} is not an nn.Module subclass")
    if getattr(cls, "_rm_kind", None) is not None:
        raise TypeError(f"register_combinator: {cls.__name__} is already a ray_marching_amd node")
    if not callable(getattr(cls, "combine", None)):
        raise TypeError(f"register_combinator: {cls.__name__} has no combine(values [..., n]) -> [..., 1] method")
    if not isinstance(children, str) or not children:
        raise ValueError("register_combinator: children must name the attribute that holds the child modules")
    params = tuple(params)
    if not all(isinstance(p, str) for p in params) or len(set(params)) != len(params):
        raise ValueError("register_combinator: params must be distinct attribute names")
    name = _combinator_identifier(hip)
    spec = UserCombinator(cls, name, params, hip, int(cost), hashlib.sha1(hip.encode()).hexdigest(), children)
    if spec.cost < 0:
        raise ValueError("register_combinator: cost must be >= 0")
    old = _combinators.get(cls)
    if old is not None:
        if (old.sha1, old.params, old.cost, old.children) != (spec.sha1, spec.params, spec.cost, spec.children):
            raise ValueError(f"register_combinator: {cls.__name__} is already registered with different source, parameters, "
                             "cost or children attribute")
        return cls
    if _registered_class(cls) is not None:
        raise TypeError(f"register_combinator: {cls.__name__} is already registered as a leaf")
    if _registered_class(cls, _warps) is not None:
        raise TypeError(f"register_combinator: {cls.__name__} is already registered as a warp")
    if _registered_class(cls, _shaders) is not None:
        raise TypeError(f"register_combinator: {cls.__name__} is already registered as a shader")
    for other in list(_registry.values()) + list(_combinators.values()) + list(_warps.values()) + list(_shaders.values()):
        if other.name == spec.name:
            raise ValueError(f"register_combinator: the identifier {spec.name!r} is already used by {other.cls.__name__}")
    cls._rm_torch_forward = _torch_forward(cls)
    cls.forward = _device_forward
    _combinators[cls] = spec
    return cls


def combinator_spec(node):
    """The combinator registration of this module's class (or of the registered class it derives from), or None."""
    c = _registered_class(type(node), _combinators)
    return None if c is None else _combinators[c]


def combinator_children(node, spec: UserCombinator):
    """The children of a combinator instance, in the order ``combine`` receives their values."""
    kids = getattr(node, spec.children, None)
    if kids is None or isinstance(kids, nn.Module) and not isinstance(kids, (nn.ModuleList, nn.Sequential)):
        raise ValueError(f"{type(node).__name__}: the children attribute {spec.children!r} is missing or not a sequence of modules")
    kids = list(kids)
    if not kids or not all(isinstance(k, nn.Module) for k in kids):
        raise ValueError(f"{type(node).__name__}: the children attribute {spec.children!r} must hold at least one SDF module")
    return kids


def register_warp(cls, *, params=(), hip: str, cost: int = 10, child: str = "sdf"):
    """Make ``cls`` (an ``nn.Module`` subclass) compilable as a unary scene node that evaluates its child at ``warp(p)`` and,
    where it has an ``out``, returns ``out(child value, p)``.

    params: names of the node's OWN ``nn.Parameter`` attributes in ``named_parameters()`` order (may be empty); a module's own
            parameters precede its child's, so they are contiguous in the scene block.
    hip:    source of NAME_fwd / NAME_vjp and, optionally, NAME_out_fwd / NAME_out_vjp (module docstring).
    cost:   VALU instructions of the map and the ``out``, roughly; the child's are added by the compiler.
    child:  the attribute that holds the one child, an SDF module.

    ``cls`` has ``warp(self, points [..., 3]) -> [..., 3]``, ``out(self, values [..., 1], points [..., 3]) -> [..., 1]`` exactly when
    the source has the ``out`` pair, and a ``forward(self, query_coords)`` that composes them around the child.  Registration
    installs the same dispatch as ``register_leaf``: CUDA points go to the HIP evaluator, anything else to the class's own
    forward (kept under ``_rm_torch_forward``).  Registering a class again with the same source is a no-op; with other source,
    parameters, cost or child attribute it is an error.  Identifiers are unique across leaves, combinators and warps."""
    if not (isinstance(cls, type) and issubclass(cls, nn.Module)):
        raise TypeError(f"register_warp: {cls!r} is not an nn.Module subclass")
    if getattr(cls, "_rm_kind", None) is not None:
        raise TypeError(f"register_warp: {cls.__name__} is already a ray_marching_amd node")
    if _registered_class(cls) is not None:
        raise TypeError(f"register_warp: {cls.__name__} is already registered as a leaf")
    if _registered_class(cls, _combinators) is not None:
        raise TypeError(f"register_warp: {cls.__name__} is already registered as a combinator")
    if _registered_class(cls, _shaders) is not None:
        raise TypeError(f"register_warp: {cls.__name__} is already registered as a shader")
    if not callable(getattr(cls, "warp", None)):
        raise TypeError(f"register_warp: {cls.__name__} has no warp(points [..., 3]) -> [..., 3] method")
    if not isinstance(child, str) or not child:
        raise ValueError("register_warp: child must name the attribute that holds the child module")
    params = tuple(params)
    if not all(isinstance(p, str) for p in params) or len(set(params)) != len(params):
        raise ValueError("register_warp: params must be distinct attribute names")
    name, has_out = _warp_identifier(hip)
    if has_out != callable(getattr(cls, "out", None)):
        raise TypeError(f"register_warp: {cls.__name__} " + (
            f"has no out(values, points) method, but its source defines {name}_out_fwd / {name}_out_vjp" if has_out else
            f"has an out(values, points) method, but its source defines no {name}_out_fwd / {name}_out_vjp"))
    spec = UserWarp(cls, name, params, hip, int(cost), hashlib.sha1(hip.encode()).hexdigest(), child, has_out,
                    _has_bound(hip, name, "warp"))
    if spec.cost < 0:
        raise ValueError("register_warp: cost must be >= 0")
    old = _warps.get(cls)
    if old is not None:
        if (old.sha1, old.params, old.cost, old.child) != (spec.sha1, spec.params, spec.cost, spec.child):
            raise ValueError(f"register_warp: {cls.__name__} is already registered with different source, parameters, cost or "
                             "child attribute")
        return cls
    for other in list(_registry.values()) + list(_combinators.values()) + list(_warps.values()) + list(_shaders.values()):
        if other.name == spec.name:
            raise ValueError(f"register_warp: the identifier {spec.name!r} is already used by {other.cls.__name__}")
    cls._rm_torch_forward = _torch_forward(cls)
    cls.forward = _device_forward
    _warps[cls] = spec
    return cls


def warp_spec(node):
    """The warp registration of this module's class (or of the registered class it derives from), or None."""
    c = _registered_class(type(node), _warps)
    return None if c is None else _warps[c]


def warp_child(node, spec: UserWarp):
    """The one child of a warp instance."""
    kid = getattr(node, spec.child, None)
    if not isinstance(kid, nn.Module):
        raise ValueError(f"{type(node).__name__}: the child attribute {spec.child!r} is missing or not an SDF module")
    return kid


def register_shader(cls, *, params=(), hip: str):
    """Make instances of ``cls`` (an ``nn.Module`` subclass) usable as the ``mode`` of ``RenderLoop.forward``: a per-pixel shader
    that runs fused at the end of the frame kernels and in the fused backward.

    params: names of ALL its ``nn.Parameter`` attributes in ``named_parameters()`` order (may be empty): ``theta``.
    hip:    source of NAME_fwd / NAME_vjp (module docstring).

    ``cls`` has ``forward(px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals) -> [..., 3]``,
    the first six arguments of the reference's ``Shader.forward`` (``camera_orientation`` [N,4], ``pixel_frames`` [N,3,3]); it is
    the CPU statement of the shader and is NOT replaced.  Registering a class again with the same source is a no-op; with other
    source or parameters it is an error.  Identifiers are unique across leaves, combinators, warps and shaders."""
    if not (isinstance(cls, type) and issubclass(cls, nn.Module)):
        raise TypeError(f"register_shader: {cls!r} is not an nn.Module subclass")
    if getattr(cls, "_rm_kind", None) is not None:
        raise TypeError(f"register_shader: {cls.__name__} is already a ray_marching_amd node")
    for registry, what in ((_registry, "leaf"), (_combinators, "combinator"), (_warps, "warp")):
        if _registered_class(cls, registry) is not None:
            raise TypeError(f"register_shader: {cls.__name__} is already registered as a {what}")
    if cls.forward is nn.Module.forward:
        raise TypeError(f"register_shader: {cls.__name__} has no forward(px_coords, camera_orientation, pixel_frames, ray_directions, "
                        "surface_coords, surface_normals)")
    params = tuple(params)
    if not all(isinstance(p, str) for p in params) or len(set(params)) != len(params):
        raise ValueError("register_shader: params must be distinct attribute names")
    name = _shader_identifier(hip)
    spec = UserShader(cls, name, params, hip, hashlib.sha1(hip.encode()).hexdigest())
    old = _shaders.get(cls)
    if old is not None:
        if (old.sha1, old.params) != (spec.sha1, spec.params):
            raise ValueError(f"register_shader: {cls.__name__} is already registered with different source or parameters")
        return cls
    for other in list(_registry.values()) + list(_combinators.values()) + list(_warps.values()) + list(_shaders.values()):
        if other.name == spec.name:          # (a scene's user types and the shader are compiled into one translation unit)
            raise ValueError(f"register_shader: the identifier {spec.name!r} is already used by {other.cls.__name__}")
    _shaders[cls] = spec
    return cls


def shader_spec(node):
    """The shader registration of this module's class (or of the registered class it derives from), or None."""
    c = _registered_class(type(node), _shaders)
    return None if c is None else _shaders[c]


def shader_parameters(shader, spec: UserShader):
    """The shader's nn.Parameters in theta order: the registered names, which must be all of its parameters in
    ``named_parameters()`` order."""
    params = leaf_parameters(shader, spec)
    own = [p for _, p in shader.named_parameters()]
    if len(own) != len(params) or any(a is not b for a, b in zip(own, params)):
        raise ValueError(f"{type(shader).__name__}: the registered params {spec.params} are not all of the shader's parameters in "
                         f"named_parameters() order ({[n for n, _ in shader.named_parameters()]})")
    return params


def leaf_parameters(node, spec):
    """The leaf's nn.Parameters in block order (the compiler checks that they are contiguous in the scene's block)."""
    missing = [n for n in spec.params if not isinstance(getattr(node, n, None), nn.Parameter)]
    if missing:
        raise ValueError(f"{type(node).__name__}: registered parameter(s) {missing} are not nn.Parameter attributes of the instance")
    return [getattr(node, n) for n in spec.params]


def check_bound(leaf, extent: float = 4.0, n: int = 1 << 16, seed: int = 0):
    """Check the bound a leaf signs with NAME_bound against its own HIP ``NAME_fwd`` (needs a GPU; moves nothing: the
    leaf must already be on the device).  ``n`` random points in ``[-extent, extent]^3`` and ``n`` concentrated around its
    sphere (on it, inside it, and a few radii out) are evaluated by the kernels; the bound is read back through
    ``rm_scene_bound`` for the leaf's current parameters.  Raises ValueError naming the worst point and by how much

        fwd(p) >= slope |p - c| - R      (and, where Ru is finite,  fwd(p) <= uslope |p - c| + Ru)

    fails beyond ``1e-5 * (1 + |p| + R)`` -- the fp32 rounding of the value, a tenth of the margin the kernels add.
    Returns ``(centre, R, slope, Ru, uslope)``.  Run it once per leaf and for the parameter ranges you use: a wrong bound
    gives silently wrong pixels.

    ``leaf`` may also be an instance of a registered warp, with its child: the node (map, child, ``out``) is what the kernels
    evaluate at the same two point sets, and the bound is the node's, i.e. what ``NAME_bound`` made of the child's.  The child
    must be boundable itself ("no finite bound" otherwise)."""
    import math
    from . import ops
    from .scene._base import SDFNode
    spec = leaf_spec(leaf) or warp_spec(leaf)
    if spec is None:
        raise TypeError(f"check_bound: {type(leaf).__name__} is not a registered leaf or warp")
    if not spec.bounded:
        raise ValueError(f"check_bound: the source of {type(leaf).__name__} defines no {spec.name}_bound")
    value = f"{spec.name}_fwd(p)" if isinstance(spec, UserLeaf) else f"{type(leaf).__name__}(p)"
    params = list(leaf.parameters())
    dev = params[0].device if params else torch.device("cuda", torch.cuda.current_device())
    c, R, slope, Ru, uslope = ops.scene_bound(leaf, dev)
    if not math.isfinite(R):
        raise ValueError(f"check_bound: {spec.name}_bound gives no finite bound for these parameters (R = {R}, slope = {slope})")
    gen = torch.Generator().manual_seed(seed)
    box = (torch.rand(n, 3, generator=gen) * 2 - 1) * extent
    u = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    rho = torch.rand(n, 1, generator=gen)
    # thirds: a shell around the sphere, the ball inside it, rays out to 8 radii (+ extent)
    radius = torch.where(rho < 1 / 3, abs(R) * (1 + 0.1 * (rho * 6 - 1)),
                         torch.where(rho < 2 / 3, abs(R) * (rho * 3 - 1), abs(R) + (8 * abs(R) + extent) * (rho * 3 - 2)))
    pts = torch.cat([box, c + radius * u]).to(dev)
    with torch.no_grad():
        f = SDFNode._evaluate(leaf, pts).reshape(-1).double().cpu()
    pts = pts.cpu().double()
    dist = (pts - c.double()).norm(dim=-1)
    tol = 1e-5 * (1 + pts.norm(dim=-1) + abs(R))
    checks = [("lower", f - (slope * dist - R) + tol, f"{value} >= {slope:g} |p - c| - {R:g}")]
    if math.isfinite(Ru):
        checks.append(("upper", (uslope * dist + Ru) - f + tol, f"{value} <= {uslope:g} |p - c| + {Ru:g}"))
    for which, margin, text in checks:
        bad = margin.isnan() | (margin < 0)
        if bad.any():
            i = int(torch.where(margin.isnan(), torch.full_like(margin, -math.inf), margin).argmin())
            raise ValueError(f"check_bound: the {which} bound of {type(leaf).__name__} fails at {int(bad.sum())} of {len(f)} points: "
                             f"{text}" + ("" if isinstance(spec, UserLeaf) else f" ({spec.name}_bound)") + f" with c = {c.tolist()} "
                             f"is off by {-float(margin[i] - tol[i]):.6g} at p = {pts[i].tolist()} (value {float(f[i]):.6g})")
    return c, R, slope, Ru, uslope
