"""Scene compiler: nn.Module SDF tree -> flat program + packed parameter block.

The reference evaluates a scene by recursing through ``nn.Module.forward``
calls (scene/primitives.py, scene/transformations.py), one ATen op at a time.
Here the tree is walked once on the host and lowered to the instruction list of
``include/rm_abi.h`` (opcode, parameter offset, aux0, aux1), which the HIP
kernels evaluate per ray.

Parameter block layout = ``module.named_parameters()`` order (the reference's
state_dict order), so gradient vectors map 1:1 back onto the ``nn.Parameter``s.
Derived constants (capsule AB, AB/|AB|^2) get slots after the raw block; the
kernels fill them in LDS.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _abi
from .extensions import (combinator_children, leaf_parameters, shader_parameters, shader_spec, user_spec,
                         warp_child)

import os

# backward-pass stack cost of each frame kind, in floats (forward uses fewer)
_STACK_UNION, _STACK_SMOOTH, _STACK_AFFINE = 2, 2, 6


# rough VALU cost of evaluating a subtree (instructions per ray), used only to decide whether a cull test
# (~9 instructions when it fails) is worth emitting in front of it
_LEAF_COST = {"sphere": 13, "box": 22, "plane": 1, "line": 30, "disk": 20, "torus": 24}
_CULL_MIN_CHILD_COST = 40
# smooth unions with at least this many children get the exact logsumexp culling (RM_OP_CULL_LSE; the wave-wide test
# costs ~45 instructions per evaluation whatever the number of children)
_CULL_LSE_MIN_CHILDREN = 8
# user types (RM_OP_USER*), per kind: what two instances with different parameter floats are "one" of, how many types a scene
# holds at the most (None: no limit of its own), and what that message adds
_USER_TYPES = {"leaf": ("type", None, ""), "combinator": ("class", 255, " ((class, children) pairs)"), "warp": ("class", 256, "")}


def _user(node):
    """Registration of a user-defined leaf, combinator or warp (extensions.register_*) and its kind, or (None, None)."""
    spec = user_spec(node) if getattr(node, "_rm_kind", None) is None else None
    return spec, getattr(spec, "kind", None)


def _cost(node) -> int:
    kind = getattr(node, "_rm_kind", None)
    if kind in _LEAF_COST:
        return _LEAF_COST[kind]
    spec, user = _user(node)
    if user == "leaf":
        return spec.cost
    if user == "combinator":
        return spec.cost + sum(_cost(c) + 1 for c in combinator_children(node, spec))
    if user == "warp":
        return spec.cost + _cost(warp_child(node, spec))
    if kind == "affine":
        return 25 + _cost(node.sdf)
    if kind in ("rounding", "onion"):
        return 1 + _cost(node.sdf)
    if kind == "material":            # (the identity: no instruction of the march is spent on it)
        return _cost(node.sdf)
    if kind == "union":
        return sum(_cost(c) + 1 for c in node.sdfs)
    if kind == "smooth_union":
        return sum(_cost(c) + 25 for c in node.sdfs) + 20
    return 0


def _boundable(node) -> bool:
    """Can the kernels derive a bounding sphere for this subtree (csrc/rm_device.h: subtree_bound)?
    Everything except an SDFPlane, a user-defined leaf or warp registered without a NAME_bound, or a user-defined combinator
    (which signs no bound) somewhere inside.  A warp's NAME_bound maps its child's bound, so a bounded warp is boundable exactly
    when its child is; whether the bound is finite is decided on the device from the live parameter values."""
    kind = getattr(node, "_rm_kind", None)
    if kind in ("sphere", "box", "line", "disk", "torus"):
        return True
    spec, user = _user(node)
    if user == "leaf":
        return spec.bounded
    if user == "warp":
        return spec.bounded and _boundable(warp_child(node, spec))
    if kind in ("affine", "rounding", "onion", "material"):
        return _boundable(node.sdf)
    if kind in ("union", "smooth_union"):
        return all(_boundable(c) for c in node.sdfs)
    return False


def _is_material(node) -> bool:
    return getattr(node, "_rm_kind", None) == "material"


def _has_material(node) -> bool:
    """A material node (contrib.SDFMaterial) at or below this node."""
    return any(_is_material(m) for m in node.modules())


def _bare(node):
    """The node with the material node around it, if any, taken off: what decides how its parent treats it."""
    return node.sdf if _is_material(node) else node


@dataclass
class CompiledScene:
    program: np.ndarray                 # int32 [n_instr, 4]
    leaves: list                        # nn.Parameter objects in block order
    leaf_names: list
    leaf_offsets: list
    n_params: int
    n_derived: int
    n_grad_derived: int                 # leading derived floats that carry gradients (capsule constants)
    stack_floats: int
    n_slots: int
    signature: tuple                    # topology key (ops + offsets + user leaf / combinator / warp sources), parameters excluded
    user_leaves: tuple = ()             # (identifier, parameter floats, sha1 of the HIP source) per user leaf type, in aux0 order
    user_sources: tuple = ()            # their HIP source texts (what specialize.code_header compiles in)
    user_bounded: tuple = ()            # ... and whether each source brings a NAME_bound (a bounding sphere: extensions.py)
    user_combinators: tuple = ()        # (identifier, children, parameter floats, sha1) per user combinator type, in type order
    user_combinator_sources: tuple = () # the HIP source of every combinator CLASS among them (one text per identifier)
    user_warps: tuple = ()              # (identifier, parameter floats, has an `out`, sha1) per user warp type, in aux0 order
    user_warp_sources: tuple = ()       # their HIP source texts
    user_warp_bounded: tuple = ()       # ... and whether each source brings a NAME_bound (the node's bound from its child's)
    user_shader: tuple = ()             # (identifier, parameter floats, sha1) of the user shader of a (scene, shader) program, else ()
    user_shader_source: str = ""        # its HIP source text
    user_shader_probes: int = 0         # K: the scene probes it asks for per pixel (register_shader(probes=K)); 0: none
    user_shader_chained: bool = False   # its probes take the history of the values before them (register_shader(chained=True))
    user_shader_normalise: object = None    # "minmax": its NAME_fwd returns a raw triple that NAME_finish maps through the frame's min / max
    user_shader_table: str = ""         # the attribute that holds its lookup table (register_shader(table=...)); "": none
    user_shader_table_taps: int = 0     # T: the most table rows one pixel's VJP contributes to; 0: no table
    user_shader_material: bool = False  # its pair takes the surface colour of the material nodes (register_shader(material=True))
    user_shader_trace: int = 0          # S: the steps of the secondary ray the frame kernels march for it (register_shader(trace=S)); 0: none
    materials: int = 0                  # RM_OP_MATERIAL instructions, the implicit ones included (contrib.SDFMaterial); 0: none, the scene
                                        # is what it always was.  > 0: the scene runs only through its specialised library (RM_MATERIALS)
    shader_offset: int = 0              # where its theta starts in the block (= the scene's own n_params)
    _device_programs: dict = field(default_factory=dict)
    _table: dict = field(default_factory=dict)
    _leaf_sizes: object = None
    _lib: object = None

    # the loaded libraries (ctypes) and device tensors are process state, not scene state: a pickled / deep-copied
    # CompiledScene carries the program only and re-resolves the rest on first use
    def __getstate__(self):
        state = dict(self.__dict__)
        state["_device_programs"], state["_table"], state["_lib"] = {}, {}, None
        state.pop("_block_caches", None)          # (ops.scene_cache: per-stream device buffers)
        return state

    def lib(self, backward: bool = False, precision: str = "exact"):
        """Kernel library for this scene: the per-scene specialised build when one is available
        (ray_marching_amd/specialize.py), else the generic interpreter library.  Backward of
        scenes with many parameters always uses the generic library (accumulators in LDS).
        ``precision="fast"`` selects the opt-in fast-arithmetic builds."""
        from . import specialize
        if self.has_user_types:
            return self._user_leaf_lib(backward, precision)
        generic = _abi.generic_lib(precision)
        if backward and not specialize.static_backward(self):
            return generic
        if precision != "exact":
            return specialize.load(self, precision) or generic
        if self._lib is None:
            self._lib = specialize.load(self) or _abi.lib
        if self._lib is _abi.lib and specialize.note_interpreted_launch(self):
            self._lib = specialize.load(self) or _abi.lib      # a background build has finished
        return self._lib

    def _user_leaf_lib(self, backward: bool, precision: str):
        """Scenes with user-defined leaves, combinators or warps (RM_OP_USER*) and (scene, shader) programs (RM_MODE_USER) exist only as
        specialised kernels: the interpreter has no handler for them, so everything that would fall back to it raises instead."""
        from . import specialize
        names, what = specialize.user_names(self)
        if backward and not specialize.static_backward(self):
            raise _abi.RmError(
                f"backward of a scene with user-defined {what} ({names}) and {self.n_params + self.n_grad_derived} gradient "
                f"accumulators: above RM_STATIC_BACKWARD_ACC={specialize._backward_limit()} the backward runs through the LDS "
                f"interpreter, which has no handler for user {what}; raise RM_STATIC_BACKWARD_ACC")
        if precision == "exact" and self._lib is not None:
            return self._lib
        lib = specialize.load_user(self, precision)
        for built, have, what in ((lib.rm_user_leaves(), self.user_leaves, "user leaf types, the scene"),
                                  (lib.rm_user_combinators(), self.user_combinators, "user combinator types, the scene"),
                                  (lib.rm_user_warps(), self.user_warps, "user warp types, the scene"),
                                  (lib.rm_user_shaders(), self.user_shader[:1], "user shaders, the program")):
            if built != len(have):
                raise _abi.RmError(f"{lib._name} was built with {built} {what} has {len(have)}")
        if precision == "exact":
            self._lib = lib
        return lib

    @property
    def has_user_types(self) -> bool:
        """User-defined leaves, combinators or warps in the scene, a user shader on it, or material nodes in it: no interpreter
        path (_user_leaf_lib)."""
        return bool(self.user_leaves or self.user_combinators or self.user_warps or self.user_shader or self.materials)

    @property
    def albedo_leaves(self):
        """(index into ``leaves``, block offset) of the albedo of every SDFMaterial, in program order."""
        at = {off: i for i, off in enumerate(self.leaf_offsets)}
        return [(at[int(off)], int(off)) for op, off, a0, _ in self.program.tolist() if op == _abi.OP_MATERIAL and a0 == 0]

    @property
    def specialised(self) -> bool:
        return self.lib() is not _abi.lib

    @property
    def n_instr(self):
        return int(self.program.shape[0])

    def device_program(self, device):
        key = str(device)
        t = self._device_programs.get(key)
        if t is None:
            t = torch.from_numpy(self.program.reshape(-1).copy()).to(device)
            self._device_programs[key] = t
        return t

    def pack_params(self, device):
        """fp32 parameter block on ``device`` as ONE tensor (torch.cat of the leaves: differentiable, so
        gradients flow back to every nn.Parameter).  Always rebuilt from the live values -- no cache that an
        in-place ``.data`` edit could leave stale.  Inference frames do not need it at all: see param_table."""
        leaves = self.leaves
        if not leaves:
            return torch.zeros(1, dtype=torch.float32, device=device)
        return torch.cat([p.reshape(-1).to(device=device, dtype=torch.float32) for p in leaves])

    @property
    def leaf_sizes(self):
        if self._leaf_sizes is None:
            self._leaf_sizes = [p.numel() for p in self.leaves]
        return self._leaf_sizes

    def param_table(self, device):
        """Device table of RmParamRef {pointer, element, dtype} for every float of the block, so the kernels
        gather the parameters from the nn.Parameter storages themselves (no packing pass; in-place edits,
        optimiser steps and ``.data`` writes are simply what the next launch reads).  The table only depends
        on where the leaves live -- (data_ptr, dtype), all visible on the host -- and is rebuilt when that
        changes.  None when a leaf cannot be read in place (not on ``device``, not fp32/fp16, not contiguous);
        the caller then packs."""
        leaves = self.leaves
        if not leaves:
            return None
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = (str(dev),) + tuple((p.data_ptr(), p.dtype) for p in leaves)
        hit = self._table.get("key")
        if hit == key:
            return self._table["value"]
        rows = np.zeros((self.n_params, 2), dtype=np.int64)        # {base pointer, elem | dtype << 32}
        at = 0
        for p in leaves:
            if p.device != dev or p.dtype not in (torch.float32, torch.float16) or not p.is_contiguous():
                self._table = {"key": key, "value": None}
                return None
            n = p.numel()
            rows[at:at + n, 0] = p.data_ptr()
            rows[at:at + n, 1] = np.arange(n, dtype=np.int64) | (np.int64(_abi.dtype_code(p.dtype)) << 32)
            at += n
        table = torch.from_numpy(rows.reshape(-1)).to(dev)
        self._table = {"key": key, "value": table}
        return table

    def scene_struct(self, params, device, table=None, block=None, block_out=None, block_cache=None):
        """RmScene for a launch; keeps the referenced tensors alive via the return tuple.  ``params``: the packed
        fp32 block, or None to gather from ``table`` (default: param_table(device)); packs when neither works.
        ``block``: the finished scene block (n_params + n_derived floats) a previous launch left in its ``block_out``:
        the kernels then skip gathering the parameters and deriving the constants.  ``block_cache``: a block the kernels
        reuse after comparing the parameters it was derived from with the live ones (ops.scene_caches)."""
        prog = self.device_program(device)
        if params is None and table is None:
            table = self.param_table(device)
            if table is None:
                with torch.no_grad():
                    params = self.pack_params(device)
        s = _abi.RmScene(program=prog.data_ptr(), params=None if params is None else params.data_ptr(),
                         param_refs=None if (params is not None or table is None) else table.data_ptr(),
                         n_instr=self.n_instr, n_params=self.n_params, n_derived=self.n_derived,
                         stack_floats=self.stack_floats, n_slots=self.n_slots, n_grad_derived=self.n_grad_derived,
                         block=None if block is None else block.data_ptr(),
                         block_out=None if block_out is None else block_out.data_ptr(),
                         block_cache=None if block_cache is None else block_cache.data_ptr())
        return s, (prog, params, table, block, block_out, block_cache)


class _Emitter:
    def __init__(self, offsets):
        self.offsets = offsets        # id(param) -> float offset
        self.code = []
        self.n_slots = 0
        self.n_derived = 0
        self.n_grad_derived = 0        # capsule constants: reserved at the front of the derived block (they carry gradients)
        self.next_line = 0
        self.depth = 0
        self.max_depth = 0
        self.cull = os.environ.get("RM_CULL", "1") != "0"    # RM_CULL=0: no CULL_MIN instructions (A/B tests)
        # RM_CULL_MIN_COST=0: a cull test in front of every boundable child, however cheap (stress tests)
        self.cull_min_cost = int(os.environ.get("RM_CULL_MIN_COST", _CULL_MIN_CHILD_COST))
        self.cull_reorder = os.environ.get("RM_CULL_REORDER", "1") != "0"
        # RM_CULL_LSE=1: exact culling inside smooth unions (opt-in: it pays when the children are spread over much more
        # than 104 / blend_k; in the config-5 scene 2.8 % of the child evaluations qualify, profiles/r03_lse_cull_rate.txt,
        # and the wave-wide test costs more than they save); RM_CULL_LSE_MIN: children from which on it is emitted
        self.cull_lse = os.environ.get("RM_CULL_LSE", "0") == "1"
        self.cull_lse_min = int(os.environ.get("RM_CULL_LSE_MIN", _CULL_LSE_MIN_CHILDREN))
        # RM_CULL_UNION_TABLE=0: a smooth union that is a cullable child of a min-union is tested with ONE bounding sphere only
        # (default: also with the minimum of its children's own bounds, rm_device.h: cull_union_children)
        self.cull_union_table = os.environ.get("RM_CULL_UNION_TABLE", "1") != "0"
        self.want_table = False        # set by the parent union for the child it emits next
        # material nodes (contrib.SDFMaterial): `cover` in a scene that holds one -- every leaf then ends up under exactly one
        # RM_OP_MATERIAL, explicit or implicit -- and `covered` while the subtree of one is being emitted
        self.cover = False
        self.covered = False
        self.materials = 0
        # the user types of each kind -> type index, in order of first appearance: (extensions.UserLeaf, parameter floats),
        # (extensions.UserCombinator, children, parameter floats), (extensions.UserWarp, parameter floats)
        self.user_types = {kind: {} for kind in _USER_TYPES}

    def off(self, *params):
        """Offset of the first parameter; the rest must follow contiguously."""
        base = self.offsets[id(params[0])]
        expect = base
        for p in params:
            if self.offsets[id(p)] != expect:
                raise ValueError("scene parameters of one node are not contiguous in named_parameters() "
                                 "order (shared nn.Parameter between fields of one node is not supported)")
            expect += p.numel()
        return base

    def user_type(self, node, spec, *shape, floats):
        """Index of the type (spec, *shape, floats) among the user types of its kind, entered on first appearance."""
        types, (unit, limit, note) = self.user_types[spec.kind], _USER_TYPES[spec.kind]
        if any(key[0] is spec and key[-1] != floats for key in types):
            raise ValueError(f"{type(node).__name__}: instances of one user {spec.kind} {unit} must have the same number of parameter floats")
        key = (spec, *shape, floats)
        if key not in types:
            if limit is not None and len(types) >= limit:
                raise ValueError(f"a scene holds at most {limit} user {spec.kind} types{note}")
            types[key] = len(types)
        return types[key]

    def push(self, n):
        self.depth += n
        self.max_depth = max(self.max_depth, self.depth)

    def pop(self, n):
        self.depth -= n

    def ins(self, op, off=0, a0=0, a1=0):
        self.code.append((op, off, a0, a1))


def _emit(node, em: _Emitter, n_params: int):
    kind = getattr(node, "_rm_kind", None)
    spec, user = _user(node)
    A = _abi
    if em.cover and not em.covered and kind != "material" and not _has_material(node):
        # a maximal subtree with no material node above or inside it: the implicit material, default colour, no parameters
        # (em.want_table stays as the parent set it: the subtree is emitted as it always was)
        em.covered = True
        _emit(node, em, n_params)
        em.covered = False
        em.ins(A.OP_MATERIAL, 0, 1, 0)
        em.materials += 1
        return
    if kind == "material":
        if em.covered:
            raise ValueError("an SDFMaterial inside the subtree of another SDFMaterial: every leaf has exactly one material")
        em.covered = True
        _emit(node.sdf, em, n_params)
        em.covered = False
        em.ins(A.OP_MATERIAL, em.off(node.albedo), 0, 0)
        em.materials += 1
    elif kind == "sphere":
        em.ins(A.OP_SPHERE, em.off(node.radius))
    elif kind == "box":
        em.ins(A.OP_BOX, em.off(node.halfsides))
    elif kind == "plane":
        em.ins(A.OP_PLANE)
    elif kind == "line":
        derived = n_params + em.next_line       # one of the slots reserved at the front of the derived block
        em.next_line += 6
        em.ins(A.OP_LINE, em.off(node.start, node.end, node.radius), derived)
    elif kind == "disk":
        em.ins(A.OP_DISK, em.off(node.radius))
    elif kind == "torus":
        em.ins(A.OP_TORUS, em.off(node.radius1, node.radius2))
    elif kind == "affine":
        off = em.off(node.translation, node.orientation)
        em.ins(A.OP_AFFINE_PUSH, off)
        em.push(_STACK_AFFINE)
        _emit(node.sdf, em, n_params)
        em.pop(_STACK_AFFINE)
        em.ins(A.OP_AFFINE_POP, off)
    elif kind in ("union", "smooth_union"):
        kids = list(node.sdfs)
        if not kids:
            raise ValueError("SDFUnion / SDFSmoothUnion needs at least one child")
        if kind == "smooth_union" and len(kids) >= 512:
            raise NotImplementedError("SDFSmoothUnion with 512 or more children: ATen's sum kernel switches to cascade "
                                      "levels there, which the kernels' summation order (aten_inner_sum) does not follow")
        base = em.n_slots
        smooth = kind == "smooth_union"
        em.n_slots += len(kids) + (1 if smooth else 0)     # smooth union: one more slot for the logsumexp value
        koff = em.off(node.blend_k) if smooth else 0
        # Exact culling inside a smooth union: a child whose term of the logsumexp is exactly +0.0f for every ray of the
        # wave (k (d_i - d_min) > 104) is skipped -- value, argmax and gradients unchanged (rm_device.h: lse_cull_mask).
        # The test runs once per evaluation, one child per lane, from a table of bounds (8 floats per child, 16-byte
        # aligned, filled in on the device); the skip bits live at the children's tape slots, hence slots < 64.
        lse_table = 0
        want_table, em.want_table = em.want_table, False
        cull_children = smooth and em.cull and em.cull_lse and em.cull_lse_min <= len(kids)
        want_table = want_table and em.cull_lse_min <= len(kids)        # ~45 instructions per test: not for a handful of children
        if smooth and em.cull and (cull_children or want_table) and len(kids) <= 64 and base + len(kids) <= 64:
            em.n_derived += (-(n_params + em.n_derived)) % 4
            lse_table = n_params + em.n_derived
            em.n_derived += 8 * len(kids)
        cull_children = cull_children and bool(lse_table)
        if smooth:
            em.ins(A.OP_SMOOTH_BEGIN, koff if lse_table else 0, lse_table,
                   ((int(cull_children) << 16) | (base << 8) | len(kids)) if lse_table else 0)
        else:
            em.ins(A.OP_UNION_BEGIN)
        em.push(_STACK_SMOOTH if smooth else _STACK_UNION)
        # Exact culling of min-union children.  min() does not care about the order its operands arrive in,
        # and the reverse pass finds the winner from the tape slots, which stay in the reference's child
        # order (ties -> first child); so the children may be EVALUATED in any order.  Children that cannot
        # be culled (cheap, or without a bounding sphere: the room shell, planes) go first, so that the
        # running minimum is already small when the expensive, boundable ones are tested against it.
        cullable = [(not smooth and em.cull and base + i < 64 and _cost(child) >= em.cull_min_cost
                     and _boundable(child)) for i, child in enumerate(kids)]
        order = list(range(len(kids)))
        if em.cull_reorder:
            order = [i for i in order if not cullable[i]] + [i for i in order if cullable[i]]
        for pos, i in enumerate(order):
            child = kids[i]
            cull_at = None
            if cullable[i] and pos > 0:       # never the first one evaluated: nothing to compare with yet
                cull_at = len(em.code)
                em.ins(A.OP_CULL_MIN, 0, n_params + em.n_derived, 0)      # aux1 patched below
                em.n_derived += 5      # {cx, cy, cz, K, slope}, filled in on the device
            lse_at = None
            if cull_children:
                lse_at = len(em.code)
                em.ins(A.OP_CULL_LSE, lse_table + 8 * i, base + i, 0)           # aux1 patched below
            if cull_at is not None and em.cull_union_table and getattr(_bare(child), "_rm_kind", None) == "smooth_union":
                em.want_table = True           # the child emits a bound table on its SMOOTH_BEGIN when its slots allow
            _emit(child, em, n_params)
            em.want_table = False
            if cull_at is not None:
                skip = len(em.code) - cull_at
                nxt = em.code[cull_at + 1]
                by_children = int(nxt[0] == A.OP_SMOOTH_BEGIN and nxt[2] != 0)     # also tested with the children's own bounds
                em.code[cull_at] = (A.OP_CULL_MIN, by_children, em.code[cull_at][2], (skip << 8) | (base + i))
                em.ins(A.OP_FOLD_MIN, 0, base + i, skip)
            elif lse_at is not None:
                skip = len(em.code) - lse_at
                em.code[lse_at] = (A.OP_CULL_LSE, lse_table + 8 * i, base + i, skip)
                em.ins(A.OP_FOLD_LSE, koff, base + i, skip)
            else:
                em.ins(A.OP_FOLD_LSE if smooth else A.OP_FOLD_MIN, koff, base + i)
        em.pop(_STACK_SMOOTH if smooth else _STACK_UNION)
        em.ins(A.OP_SMOOTH_END if smooth else A.OP_UNION_END, koff, base, len(kids))
    elif kind == "rounding":
        _emit(node.sdf, em, n_params)
        em.ins(A.OP_ROUND, em.off(node.rounding))
    elif kind == "onion":
        _emit(node.sdf, em, n_params)
        slot = em.n_slots
        em.n_slots += 1
        em.ins(A.OP_ONION, em.off(node.radius), slot)
    elif user == "leaf":
        params = leaf_parameters(node, spec)
        n = sum(p.numel() for p in params)
        em.ins(A.OP_USER, em.off(*params) if params else 0, em.user_type(node, spec, floats=n), n)
    elif user == "combinator":
        kids = combinator_children(node, spec)
        n = len(kids)
        if n > A.USER_COMB_MAX_CHILDREN:
            raise ValueError(f"{type(node).__name__}: a user combinator takes at most {A.USER_COMB_MAX_CHILDREN} children "
                             f"(RM_USER_COMB_MAX_CHILDREN), this one has {n}; nest it")
        params = leaf_parameters(node, spec)
        floats = sum(p.numel() for p in params)
        t = em.user_type(node, spec, n, floats=floats)
        # n value slots, then n slots for the children's upstream gradients (the reverse pass leaves the values in place)
        base = em.n_slots
        em.n_slots += 2 * n
        em.want_table = False          # (a bound table is asked of cullable smooth unions only)
        for i, child in enumerate(kids):
            _emit(child, em, n_params)
            em.ins(A.OP_USER_FOLD, 0, base + i, base + n + i)
        em.ins(A.OP_USER_END, em.off(*params) if params else 0, base, (floats << 16) | (t << 8) | n)
    elif user == "warp":
        kid = warp_child(node, spec)
        params = leaf_parameters(node, spec)
        floats = sum(p.numel() for p in params)
        t = em.user_type(node, spec, floats=floats)
        if floats > 32767:
            raise ValueError(f"{type(node).__name__}: a user warp takes at most 32767 parameter floats")
        off = em.off(*params) if params else 0
        # a type with an `out` keeps its child's value in a tape slot of its own (the reverse pass reads it)
        slot1 = 0
        if spec.has_out:
            slot1 = em.n_slots + 1
            em.n_slots += 1
            if slot1 > 65535:
                raise ValueError("too many tape slots for a user warp with an `out` (65535)")
        em.want_table = False          # (a bound table is asked of cullable smooth unions only)
        em.ins(A.OP_USER_PUSH, off, t, floats)
        em.push(_STACK_AFFINE)
        _emit(kid, em, n_params)
        em.pop(_STACK_AFFINE)
        em.ins(A.OP_USER_POP, off, t, (floats << 16) | slot1)
    else:
        raise TypeError(
            f"{type(node).__name__} is not a ray_marching_amd SDF node; only the node types of "
            "ray_marching_amd.scene (the reference's 6 primitives and 5 combinators) can be compiled "
            "for the HIP kernels")


def compile_scene(module: nn.Module, shader: nn.Module = None) -> CompiledScene:
    """Lower an SDF module tree.  Pure host logic (no GPU needed).  ``shader``: an instance of a class registered with
    extensions.register_shader; its parameters follow the scene's in the block (compiled_with_shader)."""
    names, leaves, offsets, table = [], [], [], {}
    cursor = 0
    for name, p in module.named_parameters():
        names.append(name)
        leaves.append(p)
        offsets.append(cursor)
        table[id(p)] = cursor
        cursor += p.numel()
    shader_offset, user_shader, shader_source, shader_probes, shader_chained, shader_normalise = cursor, (), "", 0, False, None
    shader_table, shader_table_taps, shader_material, shader_trace = "", 0, False, 0
    if shader is not None:
        spec = shader_spec(shader)
        if spec is None:
            raise TypeError(f"{type(shader).__name__} is not a registered shader (extensions.register_shader)")
        for name, p in zip(spec.params, shader_parameters(shader, spec)):
            if id(p) in table:
                raise ValueError(f"{type(shader).__name__}.{name} is also a parameter of the scene (shared parameters are not supported)")
            names.append("shader." + name)
            leaves.append(p)
            offsets.append(cursor)
            cursor += p.numel()
        user_shader, shader_source, shader_probes = (spec.name, cursor - shader_offset, spec.sha1), spec.hip, spec.probes
        shader_chained, shader_normalise = spec.chained, spec.normalise
        shader_table, shader_table_taps, shader_material, shader_trace = spec.table, spec.table_taps, spec.material, spec.trace
    n_params = cursor                 # (derived constants start behind the shader's floats)
    em = _Emitter(table)
    # derived block = [capsule constants of every SDFLine (gradients flow through them) | cull bounds, bound tables]
    em.n_grad_derived = em.n_derived = 6 * sum(1 for m in module.modules() if getattr(m, "_rm_kind", None) == "line")
    em.cover = _has_material(module)
    _emit(module, em, n_params)
    if em.next_line != em.n_grad_derived:
        raise ValueError("an SDF node instance appears more than once in the scene tree (shared sub-modules are not supported)")
    program = np.asarray(em.code, dtype=np.int32).reshape(-1, 4)
    rc = _abi.lib.rm_validate_program(program.ctypes.data, program.shape[0], n_params, em.n_derived,
                                      em.max_depth, em.n_slots)
    _abi.check(rc, "rm_validate_program")
    leaf_types, comb_types, warp_types = (tuple(em.user_types[k]) for k in ("leaf", "combinator", "warp"))
    user_leaves = tuple((u.name, floats, u.sha1) for u, floats in leaf_types)
    user_combinators = tuple((u.name, n, floats, u.sha1) for u, n, floats in comb_types)
    user_warps = tuple((u.name, floats, u.has_out, u.sha1) for u, floats in warp_types)
    # the six entries every scene has, then one slot per kind of user code with the trailing empty ones dropped: scenes of built-in
    # nodes keep the signature they always had, and signature[6:] reads (leaves, combinators, warps, shader) as far as it goes
    slots = [user_leaves, user_combinators, user_warps, user_shader]
    while slots and not slots[-1]:
        slots.pop()
    if shader_probes:                 # (the same source registered with another K is another header; K = 0 adds nothing)
        slots.append(("probes", shader_probes))
    if shader_chained:                # (... and registered as a chain it is another header again; a flat shader adds nothing)
        slots.append(("chained",))
    if shader_normalise:              # (... and so is one normalised by the frame's min / max: its header brings the second pass)
        slots.append(("normalise", shader_normalise))
    if shader_table:                  # (... and one that reads a lookup table: its pair takes tab / gt.  L and the values stay run-time)
        slots.append(("table", shader_table, shader_table_taps))
    if shader_material:               # (... and one that reads the surface colour: its pair takes m / gm)
        slots.append(("material",))
    if shader_trace:                  # (... and one that traces a secondary ray: S is a constant of its header, like the probes' K)
        slots.append(("trace", shader_trace))
    signature = (tuple(map(tuple, program.tolist())), n_params, em.n_derived, em.max_depth, em.n_slots, em.n_grad_derived, *slots)
    return CompiledScene(program=program, leaves=leaves, leaf_names=names, leaf_offsets=offsets,
                         n_params=n_params, n_derived=em.n_derived, n_grad_derived=em.n_grad_derived, stack_floats=em.max_depth,
                         n_slots=em.n_slots, signature=signature, user_leaves=user_leaves,
                         user_sources=tuple(u.hip for u, _ in leaf_types), user_bounded=tuple(u.bounded for u, _ in leaf_types),
                         user_combinators=user_combinators,
                         user_combinator_sources=tuple({u.name: u.hip for u, _, _ in comb_types}.values()),
                         user_warps=user_warps, user_warp_sources=tuple(u.hip for u, _ in warp_types),
                         user_warp_bounded=tuple(u.bounded for u, _ in warp_types),
                         user_shader=user_shader, user_shader_source=shader_source, shader_offset=shader_offset,
                         user_shader_probes=shader_probes, user_shader_chained=shader_chained,
                         user_shader_normalise=shader_normalise, user_shader_table=shader_table,
                         user_shader_table_taps=shader_table_taps, materials=em.materials,
                         user_shader_material=shader_material, user_shader_trace=shader_trace)


def structure_key(module: nn.Module):
    """Cheap fingerprint that changes when the tree topology or parameter identity changes: the ids of
    every sub-module and parameter, walked through ``_modules`` / ``_parameters`` directly
    (``module.parameters()`` builds dotted name strings on every call: 25 us for a 7-node scene)."""
    out = []
    stack = [module]
    while stack:
        m = stack.pop()
        out.append(id(m))
        for p in m._parameters.values():
            out.append(id(p))
        stack.extend(m._modules.values())
    return tuple(out)


_compiled = weakref.WeakKeyDictionary()      # module -> (structure key, CompiledScene); NOT in the module's own
                                              # state: copy.deepcopy / torch.save of a scene or RenderLoop must work


def compiled_for(module: nn.Module) -> CompiledScene:
    """Compile once per (module instance, topology)."""
    key = structure_key(module)
    cache = _compiled.get(module)
    if cache is None or cache[0] != key:
        cache = (key, compile_scene(module))
        _compiled[module] = cache
    return cache[1]


_with_shader = weakref.WeakKeyDictionary()   # scene -> WeakKeyDictionary(shader -> (structure keys, CompiledScene))


def compiled_with_shader(module: nn.Module, shader: nn.Module) -> CompiledScene:
    """The program of ``module`` shaded by ``shader`` (an instance of a class registered with extensions.register_shader):
    the scene's instructions, with the shader's parameters behind the scene's in ``leaves`` / ``leaf_names`` /
    ``leaf_offsets`` and ``n_params`` grown by their floats, so that the prologue gathers theta with the scene's parameters
    and its gradients leave through the scene's accumulators.  The derived constants keep starting at ``n_params``: the
    instruction fields that point into the derived block (capsule constants, cull bounds, bound tables) move up by
    the shader's floats (a bound table to the next multiple of 4) and every other field is the scene's, row for row.
    Cached weakly per (scene, shader) pair and recompiled when the topology of either changes, like compiled_for."""
    base = compiled_for(module)
    key = (structure_key(module), structure_key(shader))
    per_scene = _with_shader.get(module)
    if per_scene is None:
        per_scene = _with_shader[module] = weakref.WeakKeyDictionary()
    cache = per_scene.get(shader)
    if cache is None or cache[0] != key:
        cs = compile_scene(module, shader)
        if cs.program.shape != base.program.shape or not np.array_equal(cs.program[:, 0], base.program[:, 0]):
            raise AssertionError("compiled_with_shader: the instructions differ from the scene's own program")
        cache = (key, cs)
        per_scene[shader] = cache
    return cache[1]
