"""User-defined SDF leaves: an ``nn.Module`` with its own PyTorch ``forward`` plus two HIP device functions.

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

Scenes that contain such a leaf run only through their per-scene specialised library (specialize.py), into which
the source is compiled; the LDS interpreter has no handler for them and ``CompiledScene.lib()`` says so instead of
rendering a wrong picture.
"""
from __future__ import annotations

import hashlib
import re
from dataclasses import dataclass

import torch
import torch.nn as nn

__all__ = ["register_leaf", "leaf_spec", "UserLeaf"]


@dataclass(frozen=True)
class UserLeaf:
    cls: type
    name: str           # NAME of NAME_fwd / NAME_vjp
    params: tuple       # attribute names of the nn.Parameters, named_parameters() order
    hip: str
    cost: int           # VALU estimate per evaluation (compiler._cost)
    sha1: str           # of the source: part of the scene signature, hence of the library hash


_registry: dict[type, UserLeaf] = {}

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


def _device_forward(self, *args, **kwargs):
    """forward() installed by register_leaf: CUDA points go to the HIP evaluator (the leaf as a one-node scene), anything
    else to the class's own PyTorch forward."""
    points = args[0] if args else next(iter(kwargs.values()))
    if isinstance(points, torch.Tensor) and points.is_cuda:
        from .scene._base import SDFNode
        return SDFNode._evaluate(self, points)
    return type(self)._rm_torch_forward(self, *args, **kwargs)


def _registered_class(cls):
    for c in cls.__mro__:
        if c in _registry:
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
    spec = UserLeaf(cls, _identifier(hip), params, hip, int(cost), hashlib.sha1(hip.encode()).hexdigest())
    if spec.cost < 0:
        raise ValueError("register_leaf: cost must be >= 0")
    old = _registry.get(cls)
    if old is not None:
        if (old.sha1, old.params, old.cost) != (spec.sha1, spec.params, spec.cost):
            raise ValueError(f"register_leaf: {cls.__name__} is already registered with different source, parameters or cost")
        return cls
    for other in _registry.values():
        if other.name == spec.name:          # (two leaf types of one scene are compiled into one translation unit)
            raise ValueError(f"register_leaf: the identifier {spec.name!r} is already used by {other.cls.__name__}")
    cls._rm_torch_forward = cls.forward
    cls.forward = _device_forward
    _registry[cls] = spec
    return cls


def leaf_spec(node):
    """The registration of this module's class (or of the registered class it derives from), or None."""
    c = _registered_class(type(node))
    return None if c is None else _registry[c]


def leaf_parameters(node, spec: UserLeaf):
    """The leaf's nn.Parameters in block order (the compiler checks that they are contiguous in the scene's block)."""
    missing = [n for n in spec.params if not isinstance(getattr(node, n, None), nn.Parameter)]
    if missing:
        raise ValueError(f"{type(node).__name__}: registered parameter(s) {missing} are not nn.Parameter attributes of the instance")
    return [getattr(node, n) for n in spec.params]
