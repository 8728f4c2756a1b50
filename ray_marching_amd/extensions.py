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

*Scene probes* let a shader ask the SDF questions (ambient occlusion, fixed-step soft shadows, thickness, edge cues, glow):
``register_shader(..., probes=K)`` with ``1 <= K <= RM_USER_SHADER_MAX_PROBES`` (8).  The source then brings two more functions
and its own pair takes the probe values,

    template <bool Fast> RM_DEV rm::V3 NAME_probe    (int k, const rm::ShadeIn& s, const float* theta);
    template <bool Fast> RM_DEV void   NAME_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, rm::V3 gq,
                                                      rm::ShadeGrad& gs, float* gtheta);
    template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta, const float* d);
    template <bool Fast> RM_DEV void   NAME_vjp(const rm::ShadeIn& s, const float* theta, const float* d, rm::V3 g,
                                                rm::ShadeGrad& gs, float* gtheta, float* gd);

``NAME_probe`` returns probe ``k``, a point in world space that is a function of the pixel's ``ShadeIn`` and of ``theta`` ONLY: probes
are independent, none may depend on the value of another (a marched shadow ray, whose next point depends on the last distance,
needs ``chained=True``, below; fixed-step shadows and fixed-height occlusion do not).  The kernels evaluate ``d[k] = scene(NAME_probe(k, ..))``
with the full evaluator the normal's taps use and hand ``d`` to ``NAME_fwd``; ``NAME_vjp`` writes ``gtheta[i]`` and ``gd[k] = dL/dd[k]``,
the kernels turn each ``gd[k]`` into the scene-parameter gradients and ``gq = dL/d(probe k)``, and ``NAME_probe_vjp`` ADDS ``J^T gq``
into ``gs`` and ``gtheta``.  ``k`` is a run-time value in both (the probe loop stays rolled: one inlined copy of the scene): compute
with it or select on it, never index an array with it, and index ``d`` / ``gd`` / ``theta`` / ``gtheta`` with constants only (an array
indexed at run time goes to scratch memory).  The class's PyTorch ``forward`` takes one more trailing argument, ``scene``, a
callable ``points[..., 3] -> [..., 1]``; with ``probes=0`` (the default) everything is as described above.

*Chained probes* lift the independence: ``register_shader(..., probes=K, chained=True)`` with ``2 <= K <= RM_USER_SHADER_MAX_PROBES``
lets probe ``k`` depend on the values the scene returned at the probes before it (a sphere-traced shadow ray, a thickness march
along ``-n``, a short reflection march, adaptive-height occlusion).  The probe pair then takes a *history*,

    template <bool Fast> RM_DEV rm::V3 NAME_probe    (int k, const rm::ShadeIn& s, const float* theta, const float* h);
    template <bool Fast> RM_DEV void   NAME_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, const float* h, rm::V3 gq,
                                                      rm::ShadeGrad& gs, float* gtheta, float* gh);

``h`` and ``gh`` have K-1 entries and are RELATIVE to ``k``: ``h[i]`` is the scene's value at probe ``k-1-i`` for ``i < k`` (``h[0]`` the
most recent one, ``h[1]`` the one before) and exactly ``0.0f`` for ``i >= k``, so that a marched ray's ``t_k = t_0 + sum_i f(h[i])`` needs no
masking where the author sees to ``f(0) = 0``.  ``NAME_probe_vjp`` ADDS ``dL/d(value of probe k-1-i)`` into ``gh[i]``; whatever it adds to
``gh[i]`` with ``i >= k`` is ignored.  ``NAME_fwd`` / ``NAME_vjp`` keep the probing signature (``d[0..K-1]`` in probe order, ``gd`` out): the
kernels evaluate the probes in order, run ``NAME_vjp``, then walk the probes last to first and hand each one's ``gh`` back to the
earlier values before their own scene VJP runs (K <= 8: the whole chain is in registers, nothing is checkpointed).  ``h``, ``gh``,
``d`` and ``gd`` must only be indexed by constants, like ``d`` / ``gd`` above: ``k`` is a run-time value, and the window slides by one place
per probe through constant indices precisely so that no array is ever indexed with it.  The class's PyTorch ``forward(..., scene)``
needs nothing new: it calls ``scene`` in sequence and autograd does the rest.

*Frame-normalised shaders* depend on a statistic of the whole frame: ``register_shader(..., normalise="minmax")`` (orthogonal to
``probes=`` and ``chained=``).  What ``NAME_fwd`` returns is then the RAW triple of the pixel, not its colour; the frame takes ``lo =
min raw.x`` and ``hi = max raw.x`` over every pixel of every camera (a NaN anywhere makes both NaN, as ``torch.min`` / ``torch.max``
do; ``raw.y`` and ``raw.z`` ride along untouched), and a second pass maps every pixel through a pair the source brings as well,

    template <bool Fast> RM_DEV rm::V3 NAME_finish    (rm::V3 raw, float lo, float hi, const float* theta);
    template <bool Fast> RM_DEV void   NAME_finish_vjp(rm::V3 raw, float lo, float hi, const float* theta, rm::V3 g,
                                                       rm::V3& graw, float& glo, float& ghi, float* gtheta);

``theta`` is the vector ``NAME_fwd`` sees; the VJP WRITES all four outputs (they arrive zeroed): ``graw = dL/d(raw)`` through the
pixel's own value, ``glo`` / ``ghi`` the pixel's share of ``dL/dlo`` / ``dL/dhi``, ``gtheta[i]`` its share of ``dL/dtheta_i``.  The kernels
sum ``glo``, ``ghi`` and ``gtheta`` over the frame (in a fixed order: two backwards give the same bits), hand ``sum glo / n_lo`` to every
pixel with ``raw.x == lo`` and ``sum ghi / n_hi`` to every pixel with ``raw.x == hi`` -- ties share evenly, as autograd's ``min()`` /
``max()`` do -- and pass the completed ``graw`` to ``NAME_vjp`` as its ``g``.  The PyTorch ``forward`` needs nothing new: it calls ``.min()`` /
``.max()`` on its own tensor.  A backward through a minimum / maximum taken across ranks (``rows=`` with ``allreduce_minmax``) raises
NotImplementedError, as for the built-in distance, proximity and Laplacian modes; a frame with ``lo == hi`` is whatever
``NAME_finish`` makes of it.

*Lookup tables* give a shader storage it may index at run time (``theta`` lives in registers and is indexed by constants only): a
palette, a transfer function, a learnable 1-D texture.  ``register_shader(..., table="ATTR", table_taps=T)`` names an attribute of
the instance -- a registered buffer or an ``nn.Parameter`` (NOT listed in ``params``), float32, contiguous, ``[L, 3]`` with ``2 <= L <=
4096`` -- and the most rows ``T`` (1 to 4) one pixel's VJP contributes to (1: a nearest lookup, 2: a linear interpolation).  The pair
becomes

    template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta, const rm::Table& tab);
    template <bool Fast> RM_DEV void   NAME_vjp(const rm::ShadeIn& s, const float* theta, const rm::Table& tab, rm::V3 g,
                                                rm::ShadeGrad& gs, float* gtheta, rm::TableGrad& gt);

``tab.n`` is ``L`` (a run-time value, like the table's contents: one library serves every length) and ``tab.row(i)`` is row ``i`` as a
``V3``, read from global memory, with ``i`` clamped to ``[0, L-1]`` inside ``row``: a wild index reads a valid row and never faults (an
index made from a NaN is the author's business).  ``gt.row[k]`` / ``gt.g[k]`` arrive as ``-1`` / zero for ``k < T``; the VJP writes ``gt.row[k] =
i; gt.g[k] = dL/d(row i)`` (``i`` as ``tab.row`` clamps it: ``tab.clamp(i)``), indexes them with constants only like ``gtheta``, and
leaves at ``-1`` what it does not use.  Where the table is a Parameter that requires grad, the fused backward stores the ``T`` records
of every pixel and a second kernel sums them into the ``[L, 3]`` gradient without float atomics, in an order that depends only on
the pixel's index: two backwards give the same bits.  A buffer table (or ``requires_grad=False``) stores nothing.  The PyTorch
``forward`` needs nothing new: it indexes ``self.ATTR``.  ``table=`` together with ``probes`` or ``normalise=`` is refused at registration
(not built yet).

*Material nodes* give every object a colour of its own: ``contrib.SDFMaterial(sdf, albedo=(r, g, b))`` is a unary scene node whose
value is its child's, unchanged, and whose ``albedo`` no distance depends on.  The scene's value at ``p`` is ``f(p)``; with ``a_j =
|df / d(value passing through material j)|`` -- computed by exactly the rules of the scene's reverse pass: the winner of a union
(ties to the first child), the softmax weights of a smooth union, 0 for a culled child, whatever a user combinator's ``NAME_vjp`` or
a warp's ``NAME_out_vjp`` says -- the surface colour is

    m(p) = sum_j a_j c_j / sum_j a_j        (the default colour (1, 1, 1) where sum_j a_j == 0).

Under unions, smooth unions, rounding, onion and affine nodes ``sum_j a_j`` is 1 up to rounding; dividing by it keeps ``m`` a convex
blend under a scaling warp or a subtraction as well, and the surface cut by ``contrib.SDFSubtraction`` takes the cutter's colour.
A material node may not sit inside another one's subtree (``ValueError`` at compile time), and in a scene that holds at least one,
every maximal subtree without a material node above or inside it is covered by an implicit material of the default colour, so that
every leaf is under exactly one.  The weights are treated as CONSTANTS: gradients reach the albedos, because ``m`` is linear in
them, and the geometry through ``p`` and ``n`` as before; no gradient flows through ``a_j`` into shape parameters or into ``p`` (that
needs second derivatives of the scene), and PyTorch references detach the weights.  ``contrib.surface_albedo(scene, points)`` is
``m`` at chosen points.  A shader reads it with ``register_shader(..., material=True)``; the pair becomes

    template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta, rm::V3 m);
    template <bool Fast> RM_DEV void   NAME_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 m, rm::V3 g, rm::ShadeGrad& gs,
                                                float* gtheta, rm::V3& gm);

``gm = dL/dm`` arrives zeroed; the kernels add ``a_j / sum a * gm`` into the albedos' accumulators in a fixed order (two backwards
give the same bits).  The PyTorch ``forward`` takes one more trailing argument, ``material[..., 3]``.  On a scene without material
nodes ``m`` is the default colour, no sweep is compiled and there are no albedos.  A scene with material nodes rendered with a
built-in mode, or with a shader registered without ``material=True``, renders bit-identically to the same scene with the nodes
stripped, and its albedos get zero gradients.  ``material=True`` together with ``probes``, ``normalise=`` or ``table=`` is refused at
registration (not built yet).  Scenes with material nodes run only through their specialised library, like user nodes.

*Traced rays* let a shader follow a secondary ray through the scene (a mirror reflection; a chain of probes ends at 8 because the
whole chain lives in registers): ``register_shader(..., trace=S)`` with ``1 <= S <= RM_USER_SHADER_MAX_TRACE_STEPS`` (64).  The source
brings two more functions and its own pair takes the hit,

    template <bool Fast> RM_DEV void   NAME_ray    (const rm::ShadeIn& s, const float* theta, rm::TraceRay& r);
    template <bool Fast> RM_DEV void   NAME_ray_vjp(const rm::ShadeIn& s, const float* theta, const rm::TraceRay& gr,
                                                    rm::ShadeGrad& gs, float* gtheta);
    template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta, const rm::TraceHit& h);
    template <bool Fast> RM_DEV void   NAME_vjp(const rm::ShadeIn& s, const float* theta, const rm::TraceHit& h, rm::V3 g,
                                                rm::ShadeGrad& gs, float* gtheta, rm::TraceGrad& gh);

``NAME_ray`` writes the one secondary ray of the pixel, ``rm::TraceRay {V3 o, v}``: origin and direction, the direction used as given
(it need not be a unit vector).  The kernels march it with SDFMarcher's recurrence in its operation order and the full evaluator,
``p_0 = r.o``, ``p_{i+1} = scene(p_i) * r.v + p_i`` for ``i < S`` -- exactly ``S`` steps, no early exit, ``S`` a constant of the (scene, shader)
library like ``probes=K`` -- and hand ``NAME_fwd`` the hit ``rm::TraceHit {V3 p, n; float d}``: ``h.p = p_S``, ``h.d = scene(p_S)`` and ``h.n`` the
4-tap tetrahedral normal at ``p_S`` with the loop's own tetrahedron (what SDFNormals computes).  ``NAME_vjp`` writes ``gtheta[i]`` and
dL/d(hit) into ``gh`` (``rm::TraceGrad``, the fields of ``TraceHit``; it arrives zeroed); the kernels carry it through the normal, the
value and every step of the secondary march -- into the scene parameters at each of them, and into the ray's origin and direction
-- and ``NAME_ray_vjp`` ADDS ``J^T gr`` into ``gs`` and ``gtheta``, from where the primary hit and the pose get their share as for every shader.
The backward recomputes the secondary march (the forward stores nothing for it) into a checkpoint workspace in global memory,
one float4 per step and launched lane, which ``ops`` provides (rm_trace_ws_floats / rm_render_backward_trace).  The reverse secondary
march sums in program order: where every ray is walked in place two backwards give the same bits (the deferred-ray list of the
primary march, on by default, sums in the order the rays reached it, for every shader).  The class's PyTorch ``forward`` takes one more trailing argument, ``trace``, a callable ``(origins[..., 3], directions[..., 3])
-> (points, normals, values[..., 1])`` built from plain torch ops; ``reference_trace(scene_fn, steps, normals_eps)`` builds it from any
``points -> [..., 1]`` scene function.  ``trace=`` together with ``probes``, ``chained``, ``normalise=``, ``table=`` or ``material=`` is refused at
registration (not built yet).

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
           "register_warp", "warp_spec", "UserWarp", "register_shader", "shader_spec", "UserShader", "reference_trace"]


@dataclass(frozen=True)
class _UserSpec:
    """What the four kinds of registration share.  ``sha1`` (of the source) is part of the scene signature, hence of the library
    hash; ``cost`` (not for shaders) is the VALU estimate of the node's own code, to which compiler._cost adds its children's."""
    cls: type
    name: str           # NAME of NAME_fwd / NAME_vjp (/ NAME_out_fwd / NAME_out_vjp / NAME_bound)
    params: tuple       # attribute names of the node's own nn.Parameters, named_parameters() order
    hip: str


@dataclass(frozen=True)
class UserLeaf(_UserSpec):
    kind = "leaf"
    cost: int
    sha1: str
    bounded: bool = False   # the source brings NAME_bound: cull tests may cover the leaf (read from the source, like NAME)


@dataclass(frozen=True)
class UserCombinator(_UserSpec):
    kind = "combinator"
    cost: int
    sha1: str
    children: str       # attribute that holds the children (an nn.ModuleList or sequence of SDF modules)


@dataclass(frozen=True)
class UserWarp(_UserSpec):
    kind = "warp"
    cost: int
    sha1: str
    child: str          # attribute that holds the one child
    has_out: bool       # the source brings NAME_out_fwd / NAME_out_vjp (and the class an ``out`` method)
    bounded: bool = False   # the source brings NAME_bound: cull tests may cover the node where its child is boundable too


@dataclass(frozen=True)
class UserShader(_UserSpec):
    kind = "shader"
    sha1: str
    probes: int = 0     # K: the scene evaluations the shader asks for per pixel (NAME_probe / NAME_probe_vjp); 0: none
    chained: bool = False   # probe k may depend on the values of the probes before it (the pair takes the history h / gh)
    normalise: object = None    # "minmax": NAME_fwd returns the raw triple, NAME_finish / NAME_finish_vjp map it through the frame's min / max
    table: str = ""     # attribute that holds the lookup table ([L, 3] float32 buffer or nn.Parameter; the pair takes tab / gt); "": none
    table_taps: int = 0     # T: the most table rows one pixel's VJP contributes to (1..RM_USER_SHADER_MAX_TABLE_TAPS); 0: no table
    material: bool = False  # the pair takes the surface colour of the scene's material nodes, `rm::V3 m` (and the VJP `rm::V3& gm`)
    trace: int = 0      # S: the steps of the secondary ray the frame kernels march for it (NAME_ray / NAME_ray_vjp; the pair takes the hit); 0: none


@dataclass(frozen=True)
class _Kind:
    """What tells one kind of user-defined code from another at registration: a row of _KINDS, walked by _register."""
    spec: type              # the dataclass of its registrations
    ret: str                # regex of NAME_fwd's return type
    signature: str          # the fwd / vjp pair, as the error message of a source without it quotes them
    methods: tuple = ()     # (name, as the error message writes it) of the Python methods the class must have
    attr: str = ""          # the argument that names the attribute with the children ...
    holds: str = ""         # ... and what the message says the attribute holds
    same: tuple = ("sha1", "params")                # fields a second registration of the class must repeat ...
    different: str = "source or parameters"         # ... and how the message lists them
    device_forward: bool = True     # forward() is replaced by _device_forward (a shader keeps its own)
    out_pair: bool = False          # the source may bring NAME_out_fwd / NAME_out_vjp
    bound: str = ""                 # the noun under which NAME_bound is looked for ("": the kind signs no bound)
    probe_pair: bool = False        # the source may bring NAME_probe / NAME_probe_vjp (a shader's scene probes)
    finish_pair: bool = False       # the source may bring NAME_finish / NAME_finish_vjp (a shader normalised by the frame's min / max)
    ray_pair: bool = False          # the source may bring NAME_ray / NAME_ray_vjp (a shader that traces a secondary ray)


_KINDS = {
    "leaf": _Kind(
        UserLeaf, "float",
        "exactly two device functions, `template <bool Fast> RM_DEV float NAME_fwd(rm::V3 p, const float* theta)` and `template "
        "<bool Fast> RM_DEV void NAME_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta)`",
        same=("sha1", "params", "cost"), different="source, parameters or cost", bound="leaf"),
    "combinator": _Kind(
        UserCombinator, "float",
        "exactly two device functions, `template <bool Fast, int N> RM_DEV float NAME_fwd(const float (&d)[N], const float* theta)` "
        "and `template <bool Fast, int N> RM_DEV void NAME_vjp(const float (&d)[N], const float* theta, float g, float (&gd)[N], "
        "float* gtheta)`",
        methods=(("combine", "combine(values [..., n]) -> [..., 1] method"),), attr="children", holds="child modules",
        same=("sha1", "params", "cost", "children"), different="source, parameters, cost or children attribute"),
    "warp": _Kind(
        UserWarp, r"(?:rm::)?V3",
        "`template <bool Fast> RM_DEV rm::V3 NAME_fwd(rm::V3 p, const float* theta)` and `template <bool Fast> RM_DEV void "
        "NAME_vjp(rm::V3 p, const float* theta, rm::V3 gq, rm::V3& gp, float* gtheta)`",
        methods=(("warp", "warp(points [..., 3]) -> [..., 3] method"),), attr="child", holds="child module",
        same=("sha1", "params", "cost", "child"), different="source, parameters, cost or child attribute",
        out_pair=True, bound="warp"),
    "shader": _Kind(
        UserShader, r"(?:rm::)?V3",
        "exactly two device functions, `template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta)` and "
        "`template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* "
        "gtheta)`",
        methods=(("forward", "forward(px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals)"),),
        same=("sha1", "params", "probes", "chained", "normalise", "table", "table_taps", "material", "trace"), device_forward=False, probe_pair=True, finish_pair=True,
        ray_pair=True),
}

NORMALISATIONS = (None, "minmax")    # register_shader(normalise=...): the frame statistics a shader may be normalised by
RM_USER_SHADER_MAX_TABLE_TAPS = 4   # the most table rows one pixel's VJP may contribute to (gt.row[] / gt.g[] live in registers)
RM_USER_SHADER_MAX_TABLE_ROWS = 4096    # the longest lookup table (the size of the reference's own colormap: 48 KB of float32)
RM_USER_SHADER_MAX_TRACE_STEPS = 64  # the most steps of a shader's secondary ray (one float4 of the backward's checkpoint workspace each)
RM_USER_SHADER_MAX_PROBES = 8       # the most scene probes a shader may ask for (d[] / gd[] live in registers: INTEGRATION.md)

_registry: dict[type, _UserSpec] = {}       # registered class -> its registration, of whichever kind

_DEF = r"\b([A-Za-z_]\w*)_%s\s*\("


def _parse(kind: str, hip: str):
    """(NAME, has_out, bounded, has_probe, has_finish, has_ray) of the source of a ``kind``.  NAME is that of the one ``NAME_fwd`` with the kind's return
    type and must be that of the ``NAME_vjp`` too (of one of them where the kind may bring ``NAME_out_fwd`` / ``NAME_out_vjp``, which
    come as a pair or not at all and are looked up by their full names, like NAME_bound).  A shader's ``NAME_probe`` /
    ``NAME_probe_vjp`` are such a pair too: ``NAME_probe_vjp`` is no second shader; so are its ``NAME_finish`` / ``NAME_finish_vjp`` and
    its ``NAME_ray`` / ``NAME_ray_vjp`` (reported as they are found: which of the two a ``trace=`` lacks is register_shader's to say)."""
    row = _KINDS[kind]
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", hip, flags=re.S)

    def names(ret, fn):
        return set(re.findall(r"RM_DEV\s+%s\s+" % ret + _DEF % fn, text))

    fwd, vjp = names(row.ret, "fwd"), names("void", "vjp")
    name = next(iter(fwd)) if len(fwd) == 1 else None
    probe_fwd = probe_vjp = False
    if row.probe_pair and name is not None:
        probe_fwd, probe_vjp = name in names(row.ret, "probe"), f"{name}_probe" in vjp
        vjp = vjp - {f"{name}_probe"}
    finish_fwd = finish_vjp = False
    if row.finish_pair and name is not None:
        finish_fwd, finish_vjp = name in names(row.ret, "finish"), f"{name}_finish" in vjp
        vjp = vjp - {f"{name}_finish"}
    ray_fwd = ray_vjp = False
    if row.ray_pair and name is not None:
        ray_fwd, ray_vjp = name in names("void", "ray"), f"{name}_ray" in vjp
        vjp = vjp - {f"{name}_ray"}
    if name is None or (name not in vjp if row.out_pair else vjp != fwd):
        raise ValueError(f"hip must define {row.signature}, with one NAME (found fwd: {sorted(fwd)}"
                         + ("" if row.out_pair else f", vjp: {sorted(vjp)}") + ")")
    out_fwd, out_vjp = row.out_pair and f"{name}_out" in names("float", "fwd"), row.out_pair and f"{name}_out" in vjp
    if out_fwd != out_vjp:
        raise ValueError(f"hip may define `template <bool Fast> RM_DEV float {name}_out_fwd(float d, rm::V3 p, const float* theta)` and "
                         f"`template <bool Fast> RM_DEV void {name}_out_vjp(float d, rm::V3 p, const float* theta, float g, float& gd, "
                         f"rm::V3& gp, float* gtheta)`: both or neither (found {name}_out_fwd: {out_fwd}, {name}_out_vjp: {out_vjp})")
    if re.search(r"\basm\b|__asm", text):
        raise ValueError(f"a user {kind} must not contain inline assembly (INTEGRATION.md: {kind} contract)")
    if probe_fwd != probe_vjp:
        raise ValueError(f"hip may define `template <bool Fast> RM_DEV rm::V3 {name}_probe(int k, const rm::ShadeIn& s, const float* theta)` "
                         f"and `template <bool Fast> RM_DEV void {name}_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, rm::V3 gq, "
                         f"rm::ShadeGrad& gs, float* gtheta)`: both or neither (found {name}_probe: {probe_fwd}, {name}_probe_vjp: {probe_vjp})")
    if finish_fwd != finish_vjp:
        raise ValueError(f"hip may define `template <bool Fast> RM_DEV rm::V3 {name}_finish(rm::V3 raw, float lo, float hi, const float* theta)` "
                         f"and `template <bool Fast> RM_DEV void {name}_finish_vjp(rm::V3 raw, float lo, float hi, const float* theta, rm::V3 g, "
                         f"rm::V3& graw, float& glo, float& ghi, float* gtheta)`: both or neither (found {name}_finish: {finish_fwd}, "
                         f"{name}_finish_vjp: {finish_vjp})")
    return name, out_fwd, bool(row.bound) and _has_bound(text, name, row.bound), probe_fwd, finish_fwd, (ray_fwd, ray_vjp)


def _table_arguments(hip: str, name: str):
    """(NAME_fwd takes a ``rm::Table``, NAME_vjp takes a ``rm::TableGrad``): read from the two parameter lists of the source."""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", hip, flags=re.S)

    def arguments(fn):
        m = re.search(r"\b%s_%s\s*\(([^)]*)\)" % (re.escape(name), fn), text)
        return m.group(1) if m else ""

    return (re.search(r"\bTable\s*&", arguments("fwd")) is not None and re.search(r"\bTable\s*&", arguments("vjp")) is not None,
            re.search(r"\bTableGrad\s*&", arguments("vjp")) is not None)


def _trace_arguments(hip: str, name: str):
    """(NAME_fwd and NAME_vjp take a ``rm::TraceHit``, NAME_vjp takes a ``rm::TraceGrad``): read from the two parameter lists of the source."""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", hip, flags=re.S)

    def arguments(fn):
        m = re.search(r"\b%s_%s\s*\(([^)]*)\)" % (re.escape(name), fn), text)
        return m.group(1) if m else ""

    return (re.search(r"\bTraceHit\s*&", arguments("fwd")) is not None and re.search(r"\bTraceHit\s*&", arguments("vjp")) is not None,
            re.search(r"\bTraceGrad\s*&", arguments("vjp")) is not None)


def _material_arguments(hip: str, name: str):
    """(NAME_fwd and NAME_vjp take a ``rm::V3 m``, NAME_vjp takes a ``rm::V3& gm``): read from the two parameter lists of the source."""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", hip, flags=re.S)

    def arguments(fn):
        m = re.search(r"\b%s_%s\s*\(([^)]*)\)" % (re.escape(name), fn), text)
        return m.group(1) if m else ""

    return (re.search(r"\bV3\s+m\b", arguments("fwd")) is not None and re.search(r"\bV3\s+m\b", arguments("vjp")) is not None,
            re.search(r"\bV3\s*&\s*gm\b", arguments("vjp")) is not None)


def _has_bound(text: str, name: str, what: str) -> bool:
    """Whether the source (``text``: without its comments) defines ``RM_DEV void NAME_bound(`` (at most one, the own NAME of the
    leaf or warp, not a template)."""
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
    """forward() installed by register_leaf / register_combinator / register_warp: CUDA points go to the HIP evaluator (the node as
    a scene of its own), anything else to the class's own PyTorch forward."""
    points = args[0] if args else next(iter(kwargs.values()))
    if isinstance(points, torch.Tensor) and points.is_cuda:
        from .scene._base import SDFNode
        return SDFNode._evaluate(self, points)
    return type(self)._rm_torch_forward(self, *args, **kwargs)


def _torch_forward(cls, fn: str):
    """The PyTorch forward of ``cls``: the first one in its MRO that is not the forward installed here (a subclass of a
    registered class inherits _device_forward; its base keeps the original under _rm_torch_forward)."""
    for c in cls.__mro__:
        f = c.__dict__.get("forward")
        if f is _device_forward:
            f = c.__dict__["_rm_torch_forward"]
        if f is not None:
            return f
    raise TypeError(f"{fn}: {cls.__name__} has no forward")


def _registrations(cls):
    """The registrations of ``cls`` and of its ancestors, nearest first."""
    return (_registry[c] for c in cls.__mro__ if c in _registry)


def user_spec(node, kind: str = None):
    """The registration of this module's class (or of the nearest registered class it derives from), of whichever kind or, with
    ``kind``, where it is of that one; else None."""
    spec = next(_registrations(type(node)), None)
    return spec if spec is not None and kind in (None, spec.kind) else None


def _register(kind: str, cls, *, params, hip: str, **own):
    """What the four ``register_*`` do, in one order of checks: the class, its kind, its methods and child attribute, the parameter
    names, the source, the cost, a second registration of the class, the identifier.  ``own``: the arguments only some kinds
    take (``cost``, ``children`` / ``child``), under the names of the fields they become."""
    row, fn = _KINDS[kind], f"register_{kind}"
    if not (isinstance(cls, type) and issubclass(cls, nn.Module)):
        raise TypeError(f"{fn}: {cls!r} is not an nn.Module subclass")
    if getattr(cls, "_rm_kind", None) is not None:
        raise TypeError(f"{fn}: {cls.__name__} is already a ray_marching_amd node")
    for other in _registrations(cls):
        if other.kind != kind:
            raise TypeError(f"{fn}: {cls.__name__} is already registered as a {other.kind}")
    for method, text in row.methods:
        if not callable(getattr(cls, method, None)) or getattr(cls, method) is getattr(nn.Module, method, None):
            raise TypeError(f"{fn}: {cls.__name__} has no {text}")
    if row.attr and (not isinstance(own[row.attr], str) or not own[row.attr]):
        raise ValueError(f"{fn}: {row.attr} must name the attribute that holds the {row.holds}")
    params = tuple(params)
    if not all(isinstance(p, str) for p in params) or len(set(params)) != len(params):
        raise ValueError(f"{fn}: params must be distinct attribute names")
    name, has_out, bounded, has_probe, has_finish, has_ray = _parse(kind, hip)
    if row.ray_pair:           # (before the other shapes' own checks: the combination is what is refused, whatever the source looks like)
        trace = own["trace"]
        if isinstance(trace, bool) or not isinstance(trace, int) or not 0 <= trace <= RM_USER_SHADER_MAX_TRACE_STEPS:
            raise ValueError(f"{fn}: trace must be an int from 1 to RM_USER_SHADER_MAX_TRACE_STEPS = {RM_USER_SHADER_MAX_TRACE_STEPS} (the steps of "
                             f"the secondary ray; 0: none), not {trace!r}")
        if trace and (own["probes"] or own["chained"] or own["normalise"] is not None or own["table"] or own["material"]):
            raise ValueError(f"{fn}: trace= together with probes > 0, chained=, normalise=, table= or material= is not built yet (DESIGN.md "
                             f"section 11): a shader traces a secondary ray or probes the scene / is normalised by the frame / reads a "
                             f"lookup table / reads the surface colour")
    if row.probe_pair:
        probes = own["probes"]
        if isinstance(probes, bool) or not isinstance(probes, int) or not 0 <= probes <= RM_USER_SHADER_MAX_PROBES:
            raise ValueError(f"{fn}: probes must be an int from 0 to RM_USER_SHADER_MAX_PROBES = {RM_USER_SHADER_MAX_PROBES}, not {probes!r}")
        if has_probe and probes == 0:
            raise ValueError(f"{fn}: the source of {cls.__name__} defines {name}_probe / {name}_probe_vjp, but probes=0")
        if probes > 0 and not has_probe:
            raise ValueError(f"{fn}: probes={probes}, but the source of {cls.__name__} defines no {name}_probe / {name}_probe_vjp")
        chained = own["chained"]
        if not isinstance(chained, bool):
            raise ValueError(f"{fn}: chained must be a bool, not {chained!r}")
        if chained and probes < 2:
            raise ValueError(f"{fn}: chained=True needs probes from 2 to RM_USER_SHADER_MAX_PROBES = {RM_USER_SHADER_MAX_PROBES} (a chain of "
                             f"one probe has no history), not probes={probes}")
    if row.finish_pair:
        normalise = own["normalise"]
        if normalise not in NORMALISATIONS:
            raise ValueError(f"{fn}: normalise must be None or \"minmax\", not {normalise!r}")
        if has_finish and normalise is None:
            raise ValueError(f"{fn}: the source of {cls.__name__} defines {name}_finish / {name}_finish_vjp, but normalise=None")
        if normalise is not None and not has_finish:
            raise ValueError(f"{fn}: normalise={normalise!r}, but the source of {cls.__name__} defines no {name}_finish / {name}_finish_vjp")
    if row.ray_pair:
        trace = own["trace"]
        if trace and not all(has_ray):
            missing = " / ".join(f"{name}_{fn_}" for fn_, have in zip(("ray", "ray_vjp"), has_ray) if not have)
            raise ValueError(f"{fn}: trace={trace}, but the source of {cls.__name__} defines no {missing} (`template <bool Fast> RM_DEV void "
                             f"{name}_ray(const rm::ShadeIn& s, const float* theta, rm::TraceRay& r)` and `template <bool Fast> RM_DEV void "
                             f"{name}_ray_vjp(const rm::ShadeIn& s, const float* theta, const rm::TraceRay& gr, rm::ShadeGrad& gs, float* gtheta)`)")
        if not trace and any(has_ray):
            raise ValueError(f"{fn}: the source of {cls.__name__} defines {name}_ray / {name}_ray_vjp, but trace=0")
        has_h, has_gh = _trace_arguments(hip, name)
        if trace and not (has_h and has_gh):
            raise ValueError(f"{fn}: trace={trace}, but the source of {cls.__name__} does not define `template <bool Fast> RM_DEV rm::V3 "
                             f"{name}_fwd(const rm::ShadeIn& s, const float* theta, const rm::TraceHit& h)` and `template <bool Fast> RM_DEV "
                             f"void {name}_vjp(const rm::ShadeIn& s, const float* theta, const rm::TraceHit& h, rm::V3 g, rm::ShadeGrad& gs, "
                             f"float* gtheta, rm::TraceGrad& gh)` (found h: {has_h}, gh: {has_gh})")
    if "material" in own:      # (before the table's own checks: the combination is what is refused, whatever the source looks like)
        material = own["material"]
        if not isinstance(material, bool):
            raise ValueError(f"{fn}: material must be a bool, not {material!r}")
        if material and (own["probes"] > 0 or own["normalise"] is not None or own["table"]):
            raise ValueError(f"{fn}: material=True together with probes > 0, normalise= or table= is not built yet (DESIGN.md section 11): "
                             f"a shader reads the surface colour or probes the scene / is normalised by the frame / reads a lookup table")
    if "table" in own:
        table, taps = own["table"], own["table_taps"]
        if not isinstance(table, str):
            raise ValueError(f"{fn}: table must name the attribute that holds the lookup table, not {table!r}")
        if isinstance(taps, bool) or not isinstance(taps, int) or not 0 <= taps <= RM_USER_SHADER_MAX_TABLE_TAPS or (table and taps == 0):
            raise ValueError(f"{fn}: table_taps must be an int from 1 to RM_USER_SHADER_MAX_TABLE_TAPS = {RM_USER_SHADER_MAX_TABLE_TAPS} "
                             f"(the most rows one pixel's VJP contributes to), not {taps!r}")
        if taps and not table:
            raise ValueError(f"{fn}: table_taps={taps} without table= (the attribute that holds the lookup table)")
        if table and (own["probes"] > 0 or own["normalise"] is not None):
            raise ValueError(f"{fn}: table= together with probes > 0 or normalise= is not built yet (DESIGN.md section 11): a shader reads "
                             f"a lookup table or probes the scene / is normalised by the frame, not both")
        if table in params:
            raise ValueError(f"{fn}: the table attribute {table!r} must not be listed in params (it is no part of theta)")
        has_tab, has_gt = _table_arguments(hip, name)
        if table and not (has_tab and has_gt):
            raise ValueError(f"{fn}: table={table!r}, but the source of {cls.__name__} does not define `template <bool Fast> RM_DEV rm::V3 "
                             f"{name}_fwd(const rm::ShadeIn& s, const float* theta, const rm::Table& tab)` and `template <bool Fast> RM_DEV "
                             f"void {name}_vjp(const rm::ShadeIn& s, const float* theta, const rm::Table& tab, rm::V3 g, rm::ShadeGrad& gs, "
                             f"float* gtheta, rm::TableGrad& gt)` (found tab: {has_tab}, gt: {has_gt})")
        if not table and (has_tab or has_gt):
            raise ValueError(f"{fn}: the source of {cls.__name__} takes a rm::Table / rm::TableGrad, but no table= was given")
    if "material" in own:
        material = own["material"]
        has_m, has_gm = _material_arguments(hip, name)
        if material and not (has_m and has_gm):
            raise ValueError(f"{fn}: material=True, but the source of {cls.__name__} does not define `template <bool Fast> RM_DEV rm::V3 "
                             f"{name}_fwd(const rm::ShadeIn& s, const float* theta, rm::V3 m)` and `template <bool Fast> RM_DEV void "
                             f"{name}_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 m, rm::V3 g, rm::ShadeGrad& gs, float* gtheta, "
                             f"rm::V3& gm)` (found m: {has_m}, gm: {has_gm})")
        if not material and has_gm:
            raise ValueError(f"{fn}: the source of {cls.__name__} takes a surface colour (rm::V3 m / rm::V3& gm), but material=True was not given")
    if row.out_pair and has_out != callable(getattr(cls, "out", None)):
        raise TypeError(f"{fn}: {cls.__name__} " + (
            f"has no out(values, points) method, but its source defines {name}_out_fwd / {name}_out_vjp" if has_out else
            f"has an out(values, points) method, but its source defines no {name}_out_fwd / {name}_out_vjp"))
    if "cost" in own:
        own["cost"] = int(own["cost"])
        if own["cost"] < 0:
            raise ValueError(f"{fn}: cost must be >= 0")
    if row.out_pair:
        own["has_out"] = has_out
    if row.bound:
        own["bounded"] = bounded
    spec = row.spec(cls=cls, name=name, params=params, hip=hip, sha1=hashlib.sha1(hip.encode()).hexdigest(), **own)
    old = _registry.get(cls)
    if old is not None:
        if any(getattr(old, f) != getattr(spec, f) for f in row.same):
            raise ValueError(f"{fn}: {cls.__name__} is already registered with different {row.different}"
                             + (" (or another number of probes)" if row.probe_pair and old.probes != spec.probes else "")
                             + (f" (chained={old.chained} before, chained={spec.chained} now)" if row.probe_pair and old.chained != spec.chained else "")
                             + (f" (normalise={old.normalise!r} before, normalise={spec.normalise!r} now)"
                                if row.finish_pair and old.normalise != spec.normalise else "")
                             + (f" (table={old.table!r}, table_taps={old.table_taps} before, table={spec.table!r}, table_taps={spec.table_taps} now)"
                                if "table" in own and (old.table, old.table_taps) != (spec.table, spec.table_taps) else "")
                             + (f" (material={old.material} before, material={spec.material} now)"
                                if "material" in own and old.material != spec.material else "")
                             + (f" (trace={old.trace} before, trace={spec.trace} now)" if row.ray_pair and old.trace != spec.trace else ""))
        return cls
    for other in _registry.values():
        if other.name == spec.name:          # (a scene's user types and the shader are compiled into one translation unit)
            raise ValueError(f"{fn}: the identifier {spec.name!r} is already used by {other.cls.__name__}")
    if row.device_forward:
        cls._rm_torch_forward = _torch_forward(cls, fn)
        cls.forward = _device_forward
    _registry[cls] = spec
    return cls


def register_leaf(cls, *, params, hip: str, cost: int):
    """Make ``cls`` (an ``nn.Module`` subclass with a PyTorch ``forward``) compilable as a scene leaf.

    params: names of its ``nn.Parameter`` attributes in ``named_parameters()`` order (may be empty).
    hip:    source of NAME_fwd / NAME_vjp (module docstring).
    cost:   VALU instructions per evaluation, roughly (a sphere is 13, a torus 24); only steers cull placement.

    Registering a class again with the same source is a no-op; with other source, parameters or cost it is an error
    (libraries already built from the first registration would no longer describe the class).  Identifiers are unique
    across all four kinds (leaves, combinators, warps and shaders)."""
    return _register("leaf", cls, params=params, hip=hip, cost=cost)


def leaf_spec(node):
    """The registration of this module's class (or of the registered class it derives from), or None."""
    return user_spec(node, "leaf")


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
    unique across all four kinds (leaves, combinators, warps and shaders)."""
    return _register("combinator", cls, params=params, hip=hip, cost=cost, children=children)


def combinator_spec(node):
    """The combinator registration of this module's class (or of the registered class it derives from), or None."""
    return user_spec(node, "combinator")


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
    parameters, cost or child attribute it is an error.  Identifiers are unique across all four kinds (leaves, combinators,
    warps and shaders)."""
    return _register("warp", cls, params=params, hip=hip, cost=cost, child=child)


def warp_spec(node):
    """The warp registration of this module's class (or of the registered class it derives from), or None."""
    return user_spec(node, "warp")


def warp_child(node, spec: UserWarp):
    """The one child of a warp instance."""
    kid = getattr(node, spec.child, None)
    if not isinstance(kid, nn.Module):
        raise ValueError(f"{type(node).__name__}: the child attribute {spec.child!r} is missing or not an SDF module")
    return kid


def register_shader(cls, *, params=(), hip: str, probes: int = 0, chained: bool = False, normalise=None, table: str = "",
                    table_taps: int = 0, material: bool = False, trace: int = 0):
    """Make instances of ``cls`` (an ``nn.Module`` subclass) usable as the ``mode`` of ``RenderLoop.forward``: a per-pixel shader
    that runs fused at the end of the frame kernels and in the fused backward.

    params: names of ALL its ``nn.Parameter`` attributes in ``named_parameters()`` order (may be empty): ``theta``.
    hip:    source of NAME_fwd / NAME_vjp (module docstring) and, with ``probes``, of NAME_probe / NAME_probe_vjp.
    probes: K, the number of scene evaluations the shader asks for per pixel, 0 (none: the default) to
            RM_USER_SHADER_MAX_PROBES = 8.  With K > 0 the source brings NAME_probe / NAME_probe_vjp, NAME_fwd / NAME_vjp take the
            probe values ``d`` (and ``gd``), and ``forward`` takes a trailing ``scene`` argument, a callable ``points[..., 3] ->
            [..., 1]`` (module docstring: "scene probes").
    chained: probe ``k`` may depend on the values of the probes before it (needs ``2 <= K``): NAME_probe / NAME_probe_vjp take the
            history ``const float* h`` behind theta (the VJP also ``float* gh`` at its end), K-1 entries relative to ``k``, ``h[0]`` the
            most recent value, zeros where there is none yet; index ``h`` / ``gh`` / ``d`` / ``gd`` with constants only (module docstring:
            "chained probes").
    normalise: None (the default: ``NAME_fwd`` returns the pixel's colour), or "minmax": ``NAME_fwd`` returns the pixel's raw triple, the
            frame takes ``lo = min raw.x`` / ``hi = max raw.x`` over all pixels of all cameras, and the source brings NAME_finish /
            NAME_finish_vjp, which make the colour of ``(raw, lo, hi, theta)`` (module docstring: "frame-normalised shaders").
    table:  the attribute of the INSTANCE that holds a lookup table: a registered buffer or an ``nn.Parameter``, float32, contiguous,
            ``[L, 3]`` with ``2 <= L <= 4096``.  NAME_fwd / NAME_vjp then take ``const rm::Table& tab`` behind theta and the VJP ``rm::TableGrad&
            gt`` at its end (module docstring: "lookup tables").  A Parameter table is NOT listed in ``params``; it receives its ``.grad``
            through a deterministic scatter.  Not together with ``probes`` or ``normalise`` (not built yet).
    table_taps: T, 1 to 4: the most table rows one pixel's VJP contributes to (1: a nearest lookup, 2: a linear interpolation).
    material: the shader reads the surface colour of the scene's material nodes at the hit point: NAME_fwd / NAME_vjp take ``rm::V3 m``
            behind theta and the VJP ``rm::V3& gm`` at its end, and ``forward`` takes a trailing ``material[..., 3]`` (module docstring:
            "material nodes").  Not together with ``probes``, ``normalise`` or ``table`` (not built yet).
    trace:  S, 1 to RM_USER_SHADER_MAX_TRACE_STEPS = 64 (0, the default: none): the shader names one secondary ray per pixel (NAME_ray /
            NAME_ray_vjp), the frame kernels sphere-trace it S steps through the scene, and NAME_fwd / NAME_vjp take the hit, ``const
            rm::TraceHit& h`` behind theta (the VJP also ``rm::TraceGrad& gh`` at its end); ``forward`` takes a trailing ``trace``, a callable
            ``(origins[..., 3], directions[..., 3]) -> (points, normals, values[..., 1])`` (module docstring: "traced rays";
            ``reference_trace`` builds one).  Not together with ``probes``, ``chained``, ``normalise``, ``table`` or ``material`` (not built yet).

    ``cls`` has ``forward(px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals) -> [..., 3]``,
    the first six arguments of the reference's ``Shader.forward`` (``camera_orientation`` [N,4], ``pixel_frames`` [N,3,3]); it is
    the CPU statement of the shader and is NOT replaced.  Registering a class again with the same source is a no-op; with other
    source, parameters, number of probes or value of ``chained`` / ``normalise`` / ``table`` / ``table_taps`` it is an error.  Identifiers are unique across all four kinds (leaves, combinators, warps and shaders)."""
    return _register("shader", cls, params=params, hip=hip, probes=probes, chained=chained, normalise=normalise, table=table,
                     table_taps=table_taps, material=material, trace=trace)


def shader_spec(node):
    """The shader registration of this module's class (or of the registered class it derives from), or None."""
    return user_spec(node, "shader")


def reference_trace(scene_fn, steps: int, normals_eps: float, tetra=None):
    """The ``trace`` callable of a shader registered with ``trace=steps``, from any scene function ``points[..., 3] -> [..., 1]``: plain
    torch ops, so autograd differentiates it.  ``(origins, directions) -> (points, normals, values)`` with SDFMarcher's recurrence in
    its operation order, ``p_0 = origins``, ``p_{i+1} = scene(p_i) * directions + p_i`` for ``i < steps`` (no early exit), ``points = p_S``,
    ``values = scene(p_S)`` and ``normals`` the 4-tap tetrahedral normal of SDFNormals at ``p_S`` for ``normals_eps``.  ``tetra``: (offsets
    [4, 3], inverse [3, 3]) in the place of the constants of ``normals_eps`` (a module cast to float16 rounds its own)."""
    from .rendering.ray_marching import tetrahedron_constants
    steps = int(steps)

    def trace(origins, directions):
        p = origins
        for _ in range(steps):
            p = scene_fn(p) * directions + p
        if tetra is not None:
            offsets, inverse = tetra
        else:
            offsets, _, inverse = tetrahedron_constants(normals_eps)
        offsets, inverse = offsets.to(p), inverse.to(p)
        taps = scene_fn(p[..., None, :] + offsets)                        # [..., 4, 1]
        d = taps[..., 1:, :] - taps[..., :1, :]                           # [..., 3, 1]
        n = torch.nn.functional.normalize((inverse * d[..., None, :, 0]).sum(dim=-1), dim=-1, p=2, eps=0.0)
        return p, n, scene_fn(p)

    return trace


def shader_parameters(shader, spec: UserShader):
    """The shader's nn.Parameters in theta order: the registered names, which must be all of its parameters in
    ``named_parameters()`` order."""
    params = leaf_parameters(shader, spec)
    table = getattr(shader, spec.table, None) if spec.table else None      # (a Parameter table is no part of theta)
    own = [p for _, p in shader.named_parameters() if p is not table]
    if len(own) != len(params) or any(a is not b for a, b in zip(own, params)):
        raise ValueError(f"{type(shader).__name__}: the registered params {spec.params} are not all of the shader's parameters in "
                         f"named_parameters() order ({[n for n, _ in shader.named_parameters()]})")
    return params


def shader_table(shader, spec: UserShader):
    """The lookup table of a shader instance registered with ``table=``: the tensor the kernels read in place (a buffer or an
    ``nn.Parameter``; float32, contiguous, ``[L, 3]``, ``2 <= L <= RM_USER_SHADER_MAX_TABLE_ROWS``), or None for a shader without one."""
    if not spec.table:
        return None
    t = getattr(shader, spec.table, None)
    what = f"{type(shader).__name__}.{spec.table}"
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: the registered table attribute is missing or no tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: a lookup table is float32, not {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3 or not 2 <= t.shape[0] <= RM_USER_SHADER_MAX_TABLE_ROWS:
        raise ValueError(f"{what}: a lookup table is [L, 3] with 2 <= L <= {RM_USER_SHADER_MAX_TABLE_ROWS}, not {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: a lookup table must be contiguous (the kernels read it in place)")
    return t


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
