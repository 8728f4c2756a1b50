"""Per-scene specialised kernel libraries.

The generic library interprets any scene program from LDS.  For a scene whose *topology* is
known ahead of time the same kernels are rebuilt with the program as a compile-time constant
(csrc/rm_abi.hip with -DRM_STATIC_CODE=...): rm::StaticProgram unrolls the handlers, the
evaluation stack / tape / gradient accumulators become VGPRs and the scalar interpreter loop
disappears.  Parameters stay run-time values (staged through LDS), so optimising or animating
a scene never recompiles; only a change of tree structure does.

This replaces what ``torch.compile(render_loop, mode='max-autotune')`` does in the reference's
main.py:44 (which re-traces on every change of ``marching_steps``, here a run-time argument).

Libraries are built in-tree under ray_marching_amd/lib/spec/ (so they travel with the repo
snapshot to the GPU box) and are keyed by a hash of the program.

Policy (env RM_SPECIALIZE):
  "auto"     (default) use a prebuilt library when one exists; a scene that keeps being rendered
             through the interpreter (RM_SPECIALIZE_AFTER launches, default 64) gets its library
             built by ONE background hipcc process and is switched over when that finishes --
             no stall, no compile storm for throw-away scenes;
  "prebuilt" only ever use libraries that already exist;
  "jit"      build a missing library synchronously on first use (3-14 s of hipcc);
  "off"      always interpret.

Scenes with user-defined leaves, combinators or warps (extensions.register_leaf / register_combinator / register_warp; their
HIP source is compiled into the library) and (scene, shader) programs (extensions.register_shader) have no
interpreter to start on: "auto" and "jit" both build a missing library synchronously on first use, "prebuilt" and
"off" raise RmError (load_user).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess
import sys
import threading
import time

from . import _abi
from .compiler import CompiledScene, compile_scene

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
from ._build import LIBDIR, variant  # noqa: E402  (same flags as the generic libraries)
SPEC_DIR = os.path.join(LIBDIR, "spec")

# Scenes with more gradient accumulators than this run their backward through the interpreter's kernels: the unrolled
# backward of a big scene takes minutes to compile (32-primitive scene, 347 accumulators: 4 min of hipcc against 40 s
# forward-only).  RM_STATIC_BACKWARD_ACC raises the limit for users who train such scenes and accept the build: above
# RM_STATIC_REG_ACC_MAX (96, rm_kernels.h) the specialised backward keeps its accumulators in LDS rows like the
# interpreter and is ~2x faster than it (many32 fwd+bwd at 512^2: 15.7 -> 7.3 ms, profiles/r03_wide_ab.txt).
MAX_STATIC_BACKWARD_ACC = 96

_loaded: dict[str, object] = {}


def _backward_limit() -> int:
    return int(os.environ.get("RM_STATIC_BACKWARD_ACC", MAX_STATIC_BACKWARD_ACC))


def static_backward(cs: CompiledScene) -> bool:
    return cs.n_params + cs.n_grad_derived <= _backward_limit()


_SOURCES = ("csrc/rm_abi.hip", "csrc/rm_kernels.h", "csrc/rm_device.h", "csrc/rm_math.h", "../include/rm_abi.h")
_src_hash = None


def sources_hash() -> str:
    """Content hash of the kernel sources (file times do not survive a repo snapshot copy)."""
    global _src_hash
    if _src_hash is None:
        h = hashlib.sha1()
        for rel in _SOURCES:
            with open(os.path.join(_HERE, rel), "rb") as f:
                h.update(f.read())
        from ._build import extra_flags
        h.update(" ".join(extra_flags()).encode())
        _src_hash = h.hexdigest()[:12]
    return _src_hash


def scene_hash(cs: CompiledScene, precision: str = "exact") -> str:
    """Library key: program topology + kernel sources (+ arithmetic variant), so a stale library is
    simply never found."""
    tag = "" if precision == "exact" else "|" + precision
    if cs.n_params + cs.n_grad_derived > MAX_STATIC_BACKWARD_ACC and static_backward(cs):
        tag += "|bwd"          # (a forward-only library of the same scene may exist)
    return hashlib.sha1((repr(cs.signature) + sources_hash() + tag).encode()).hexdigest()[:16]


_NAN = '__builtin_nanf("")'


def _dispatcher(prototype: str, cases, default: str = "break;", after: str = "") -> str:
    """A device function that switches over the user type: ``cases`` are (type, statements) pairs, ``after`` follows the switch."""
    return (prototype + " {\n  switch (type) {\n" + "".join(f"    case {t}: {body}\n" for t, body in cases)
            + f"    default: {default}\n  }}\n{after}}}\n")


def _leaf_section(cs: CompiledScene) -> str:
    """User leaf sources and the dispatch over the leaf type (RM_OP_USER: aux0), for the header's first inclusion from
    inside namespace rm (csrc/rm_device.h); user_leaf_bound calls the NAME_bound of the types that bring one."""
    names = [(t, name) for t, (name, _, _) in enumerate(cs.user_leaves)]
    sources = "".join(f"// user leaf {t}: {name}, {n} parameter floats, sha1 {sha}\n{src.strip()}\n"
                      for t, ((name, n, sha), src) in enumerate(zip(cs.user_leaves, cs.user_sources)))
    return (
        f"#define RM_USER_LEAVES {len(cs.user_leaves)}\n"
        f"#define RM_USER_MAX_PARAMS {max(1, max(n for _, n, _ in cs.user_leaves))}\n"
        + sources
        + _dispatcher("template <bool Fast> RM_DEV float user_leaf_fwd(int type, V3 p, const float* theta)",
                      [(t, f"return {name}_fwd<Fast>(p, theta);") for t, name in names], f"return {_NAN};")
        + _dispatcher("template <bool Fast> RM_DEV void user_leaf_vjp(int type, V3 p, const float* theta, float g, V3& gp, float* gtheta)",
                      [(t, f"{name}_vjp<Fast>(p, theta, g, gp, gtheta); break;") for t, name in names])
        # (leaf types without a NAME_bound leave `b` as it arrives: nothing known)
        + _dispatcher("RM_DEV void user_leaf_bound(int type, const float* theta, LeafBound& b)",
                      [(t, f"{name}_bound(theta, b); break;") for t, name in names if cs.user_bounded[t]]))


def _combinator_section(cs: CompiledScene) -> str:
    """User combinator sources and the dispatch over the combinator type (RM_OP_USER_END: aux1 bits 8-15), for the same first
    inclusion as the leaf section and independent of it.  A type is a (class, children) pair; the caller's N selects, at
    compile time, the one instantiation of NAME_fwd / NAME_vjp a case can mean."""
    types = cs.user_combinators
    listing = "".join(f"// user combinator type {t}: {name}, {n} children, {floats} parameter floats, sha1 {sha}\n"
                      for t, (name, n, floats, sha) in enumerate(types))
    sources = "".join(src.strip() + "\n" for src in cs.user_combinator_sources)
    return (
        f"#define RM_USER_COMBINATORS {len(types)}\n"
        f"#define RM_USER_COMB_MAX_PARAMS {max(1, max(floats for _, _, floats, _ in types))}\n"
        + listing + sources
        + _dispatcher("template <bool Fast, int N> RM_DEV float user_comb_fwd(int type, const float (&d)[N], const float* theta)",
                      [(t, f"if constexpr (N == {n}) return {name}_fwd<Fast, {n}>(d, theta); break;") for t, (name, n, _, _) in enumerate(types)],
                      after=f"  return {_NAN};\n")
        + _dispatcher("template <bool Fast, int N> RM_DEV void user_comb_vjp(int type, const float (&d)[N], const float* theta, float g, "
                      "float (&gd)[N], float* gtheta)",
                      [(t, f"if constexpr (N == {n}) {name}_vjp<Fast, {n}>(d, theta, g, gd, gtheta); break;")
                       for t, (name, n, _, _) in enumerate(types)]))


def _warp_section(cs: CompiledScene) -> str:
    """User warp sources and the dispatch over the warp type (RM_OP_USER_PUSH / _POP: aux0), for the same first inclusion as
    the leaf and combinator sections and independent of both.  The `out` switches list the types that bring one, and so does
    user_warp_bound, which exists (with RM_USER_WARP_BOUNDS) only where at least one type brings a NAME_bound."""
    types = cs.user_warps
    names = [(t, name) for t, (name, _, _, _) in enumerate(types)]
    with_out = [(t, name) for t, name in names if types[t][2]]
    sources = "".join(f"// user warp {t}: {name}, {n} parameter floats, {'with' if out else 'no'} out, sha1 {sha}\n{src.strip()}\n"
                      for t, ((name, n, out, sha), src) in enumerate(zip(types, cs.user_warp_sources)))
    # (only where a type brings NAME_bound: every other scene keeps the header, hence the library, it always had)
    bounded = [(t, f"{name}_bound(theta, b); return true;") for t, name in names if cs.user_warp_bounded[t]]
    bound = "" if not bounded else "#define RM_USER_WARP_BOUNDS 1\n" + _dispatcher(
        "RM_DEV bool user_warp_bound(int type, const float* theta, LeafBound& b)", bounded, "return false;")
    return (
        f"#define RM_USER_WARPS {len(types)}\n"
        f"#define RM_USER_WARP_MAX_PARAMS {max(1, max(n for _, n, _, _ in types))}\n"
        + sources
        + _dispatcher("template <bool Fast> RM_DEV V3 user_warp_fwd(int type, V3 p, const float* theta)",
                      [(t, f"return {name}_fwd<Fast>(p, theta);") for t, name in names], f"return mk3({_NAN}, {_NAN}, {_NAN});")
        + _dispatcher("template <bool Fast> RM_DEV void user_warp_vjp(int type, V3 p, const float* theta, V3 gq, V3& gp, float* gtheta)",
                      [(t, f"{name}_vjp<Fast>(p, theta, gq, gp, gtheta); break;") for t, name in names])
        + _dispatcher("template <bool Fast> RM_DEV float user_warp_out_fwd(int type, float d, V3 p, const float* theta)",
                      [(t, f"return {name}_out_fwd<Fast>(d, p, theta);") for t, name in with_out], f"return {_NAN};")
        + _dispatcher("template <bool Fast> RM_DEV void user_warp_out_vjp(int type, float d, V3 p, const float* theta, float g, float& gd, "
                      "V3& gp, float* gtheta)",
                      [(t, f"{name}_out_vjp<Fast>(d, p, theta, g, gd, gp, gtheta); break;") for t, name in with_out])
        + bound)


def _shader_section(cs: CompiledScene) -> str:
    """The user shader's source and the functions the frame kernels call, for the header's inclusion from csrc/rm_kernels.h
    (behind rm::ShadeIn / rm::ShadeGrad, inside namespace rm): two, or -- a shader with scene probes, RM_USER_SHADER_PROBES --
    four, of which user_shader_fwd / user_shader_vjp then carry the probe values; the probe pair of a chained shader
    (RM_USER_SHADER_PROBES_CHAINED) also carries the history ``h`` of the values before probe ``k`` and, in the VJP, ``gh``.  A shader
    normalised by the frame's min / max (RM_USER_SHADER_NORMALISE) adds user_shader_finish / user_shader_finish_vjp, the second
    pass; every other header is, byte for byte, what it was without them.  A shader that reads a lookup table (RM_USER_SHADER_TABLE,
    RM_USER_SHADER_TABLE_TAPS; never with probes or a second pass) has user_shader_fwd / user_shader_vjp carry ``tab`` (and ``gt``); one that
    traces a secondary ray (RM_USER_SHADER_TRACE; never with any of the others) has them carry the hit ``h`` (and ``gh``) and adds
    user_shader_ray / user_shader_ray_vjp."""
    text = _shader_passes(cs)
    if not cs.user_shader_normalise:
        return text
    name = cs.user_shader[0]
    return (
        "#define RM_USER_SHADER_NORMALISE 1\n" + text +
        "template <bool Fast> RM_DEV V3 user_shader_finish(V3 raw, float lo, float hi, const float* theta) {\n"
        f"  return {name}_finish<Fast>(raw, lo, hi, theta);\n}}\n"
        "template <bool Fast> RM_DEV void user_shader_finish_vjp(V3 raw, float lo, float hi, const float* theta, V3 g, V3& graw, float& glo, "
        "float& ghi, float* gtheta) {\n"
        f"  {name}_finish_vjp<Fast>(raw, lo, hi, theta, g, graw, glo, ghi, gtheta);\n}}\n")


def _shader_passes(cs: CompiledScene) -> str:
    """The shader section without the second pass: the source, and the forwarders of the per-pixel pair and of the probe pair."""
    name, floats, sha = cs.user_shader
    k = cs.user_shader_probes
    head = ("#define RM_USER_SHADER 1\n"
            f"#define RM_USER_SHADER_THETA {cs.shader_offset}\n"
            f"#define RM_USER_SHADER_PARAMS {floats}\n")
    if cs.user_shader_table:        # (register_shader(table=..., table_taps=T): never with probes; the pair carries tab and gt)
        return (
            head + "#define RM_USER_SHADER_TABLE 1\n" + f"#define RM_USER_SHADER_TABLE_TAPS {cs.user_shader_table_taps}\n"
            + f"// user shader: {name}, {floats} parameter floats, a lookup table of {cs.user_shader_table_taps} taps, sha1 {sha}\n"
            + f"{cs.user_shader_source.strip()}\n"
            "template <bool Fast> RM_DEV V3 user_shader_fwd(const ShadeIn& s, const float* theta, const Table& tab) {\n"
            f"  return {name}_fwd<Fast>(s, theta, tab);\n}}\n"
            "template <bool Fast> RM_DEV void user_shader_vjp(const ShadeIn& s, const float* theta, const Table& tab, V3 g, ShadeGrad& gs, "
            "float* gtheta, TableGrad& gt) {\n"
            f"  {name}_vjp<Fast>(s, theta, tab, g, gs, gtheta, gt);\n}}\n")
    if cs.user_shader_material:     # (register_shader(material=True): never with probes, a table or a second pass; the pair carries m and gm)
        return (
            head + "#define RM_USER_SHADER_MATERIAL 1\n"
            + f"// user shader: {name}, {floats} parameter floats, reads the surface colour, sha1 {sha}\n{cs.user_shader_source.strip()}\n"
            "template <bool Fast> RM_DEV V3 user_shader_fwd(const ShadeIn& s, const float* theta, V3 m) {\n"
            f"  return {name}_fwd<Fast>(s, theta, m);\n}}\n"
            "template <bool Fast> RM_DEV void user_shader_vjp(const ShadeIn& s, const float* theta, V3 m, V3 g, ShadeGrad& gs, "
            "float* gtheta, V3& gm) {\n"
            f"  {name}_vjp<Fast>(s, theta, m, g, gs, gtheta, gm);\n}}\n")
    if cs.user_shader_trace:        # (register_shader(trace=S): never with any of the above; the pair carries the hit, and a ray pair is added)
        return (
            head + f"#define RM_USER_SHADER_TRACE {cs.user_shader_trace}\n"
            + f"// user shader: {name}, {floats} parameter floats, traces a secondary ray of {cs.user_shader_trace} steps, sha1 {sha}\n"
            + f"{cs.user_shader_source.strip()}\n"
            "template <bool Fast> RM_DEV void user_shader_ray(const ShadeIn& s, const float* theta, TraceRay& r) {\n"
            f"  {name}_ray<Fast>(s, theta, r);\n}}\n"
            "template <bool Fast> RM_DEV void user_shader_ray_vjp(const ShadeIn& s, const float* theta, const TraceRay& gr, ShadeGrad& gs, "
            "float* gtheta) {\n"
            f"  {name}_ray_vjp<Fast>(s, theta, gr, gs, gtheta);\n}}\n"
            "template <bool Fast> RM_DEV V3 user_shader_fwd(const ShadeIn& s, const float* theta, const TraceHit& h) {\n"
            f"  return {name}_fwd<Fast>(s, theta, h);\n}}\n"
            "template <bool Fast> RM_DEV void user_shader_vjp(const ShadeIn& s, const float* theta, const TraceHit& h, V3 g, ShadeGrad& gs, "
            "float* gtheta, TraceGrad& gh) {\n"
            f"  {name}_vjp<Fast>(s, theta, h, g, gs, gtheta, gh);\n}}\n")
    if not k:
        return (
            head
            + f"// user shader: {name}, {floats} parameter floats, sha1 {sha}\n{cs.user_shader_source.strip()}\n"
            "template <bool Fast> RM_DEV V3 user_shader_fwd(const ShadeIn& s, const float* theta) {\n"
            f"  return {name}_fwd<Fast>(s, theta);\n}}\n"
            "template <bool Fast> RM_DEV void user_shader_vjp(const ShadeIn& s, const float* theta, V3 g, ShadeGrad& gs, float* gtheta) {\n"
            f"  {name}_vjp<Fast>(s, theta, g, gs, gtheta);\n}}\n")
    if cs.user_shader_chained:
        probe_pair = (
            "#define RM_USER_SHADER_PROBES_CHAINED 1\n"
            + f"// user shader: {name}, {floats} parameter floats, {k} chained scene probes, sha1 {sha}\n{cs.user_shader_source.strip()}\n"
            "template <bool Fast> RM_DEV V3 user_shader_probe(int k, const ShadeIn& s, const float* theta, const float* h) {\n"
            f"  return {name}_probe<Fast>(k, s, theta, h);\n}}\n"
            "template <bool Fast> RM_DEV void user_shader_probe_vjp(int k, const ShadeIn& s, const float* theta, const float* h, V3 gq, "
            "ShadeGrad& gs, float* gtheta, float* gh) {\n"
            f"  {name}_probe_vjp<Fast>(k, s, theta, h, gq, gs, gtheta, gh);\n}}\n")
    else:
        probe_pair = (
            f"// user shader: {name}, {floats} parameter floats, {k} scene probes, sha1 {sha}\n{cs.user_shader_source.strip()}\n"
            "template <bool Fast> RM_DEV V3 user_shader_probe(int k, const ShadeIn& s, const float* theta) {\n"
            f"  return {name}_probe<Fast>(k, s, theta);\n}}\n"
            "template <bool Fast> RM_DEV void user_shader_probe_vjp(int k, const ShadeIn& s, const float* theta, V3 gq, ShadeGrad& gs, "
            "float* gtheta) {\n"
            f"  {name}_probe_vjp<Fast>(k, s, theta, gq, gs, gtheta);\n}}\n")
    return (
        head + f"#define RM_USER_SHADER_PROBES {k}\n" + probe_pair +
        "template <bool Fast> RM_DEV V3 user_shader_fwd(const ShadeIn& s, const float* theta, const float* d) {\n"
        f"  return {name}_fwd<Fast>(s, theta, d);\n}}\n"
        "template <bool Fast> RM_DEV void user_shader_vjp(const ShadeIn& s, const float* theta, const float* d, V3 g, ShadeGrad& gs, "
        "float* gtheta, float* gd) {\n"
        f"  {name}_vjp<Fast>(s, theta, d, g, gs, gtheta, gd);\n}}\n")


def _material_section(cs: CompiledScene) -> str:
    """What switches the material sweeps on (csrc/rm_device.h: RM_OP_MATERIAL in the reverse machine, Scene::material_colour /
    material_grads; csrc/rm_kernels.h: k_material_fwd / k_material_bwd), for the same first inclusion as the user nodes'
    sections.  Only scenes that hold a contrib.SDFMaterial get it: every other header is what it always was."""
    return f"#define RM_MATERIALS {cs.materials}\n"


def user_names(cs: CompiledScene):
    """(names, what) of the user types of a scene, for messages: leaf-only scenes read as they always did."""
    kinds = [("leaves", [name for name, _, _ in cs.user_leaves]),
             ("combinators", list(dict.fromkeys(name for name, _, _, _ in cs.user_combinators))),
             ("warps", [name for name, _, _, _ in cs.user_warps]),
             ("shaders", [name for name in cs.user_shader[:1]]),
             ("material nodes", ["SDFMaterial"] if cs.materials else [])]
    kinds = [(what, names) for what, names in kinds if names]
    if len(kinds) <= 1:
        what, names = kinds[0] if kinds else ("leaves", [])
        return ", ".join(names), what
    whats = [what for what, _ in kinds]
    return "; ".join(f"{what}: " + ", ".join(names) for what, names in kinds), ", ".join(whats[:-1]) + " and " + whats[-1]


def code_header(cs: CompiledScene) -> str:
    rows = ",".join("{%d,%d,%d,%d}" % tuple(int(x) for x in ins) for ins in cs.program.tolist())
    program = (
        "struct RmStaticCode {\n"
        f"  static constexpr int n = {cs.n_instr}, n_params = {cs.n_params}, n_derived = {cs.n_derived},\n"
        f"                       stack_floats = {cs.stack_floats}, n_slots = {cs.n_slots}, n_grad_derived = {cs.n_grad_derived};\n"
        f"  static constexpr rm::Ins code[{cs.n_instr}] = {{{rows}}};\n"
        "};\n")
    # included three times: by csrc/rm_device.h in front of the handlers (RM_STATIC_CODE_LEAVES: the user leaves, combinators and
    # warps only), by csrc/rm_kernels.h behind ShadeIn / ShadeGrad (RM_STATIC_CODE_LEAVES and RM_STATIC_CODE_SHADER: the user
    # shader only), then by csrc/rm_abi.hip for the program
    head = "// generated by ray_marching_amd/specialize.py -- scene program as a compile-time constant\n"
    if not cs.has_user_types:
        return head + "#ifndef RM_STATIC_CODE_LEAVES\n" + program + "#endif\n"
    user = ((_leaf_section(cs) if cs.user_leaves else "") + (_combinator_section(cs) if cs.user_combinators else "")
            + (_warp_section(cs) if cs.user_warps else "") + (_material_section(cs) if cs.materials else ""))
    shader = _shader_section(cs) if cs.user_shader else ""
    return (head + "#if defined(RM_STATIC_CODE_SHADER)\n" + shader + "#elif defined(RM_STATIC_CODE_LEAVES)\n" + user
            + "#else\n" + program + "#endif\n")


def lib_path(cs: CompiledScene, precision: str = "exact") -> str:
    return os.path.join(SPEC_DIR, f"librm_spec_{sources_hash()[:8]}_{scene_hash(cs, precision)}.so")


def prune_stale():
    """Delete specialised libraries (and their code headers) built from other kernel sources."""
    if not os.path.isdir(SPEC_DIR):
        return
    keep = f"librm_spec_{sources_hash()[:8]}_"
    live = set()
    for name in os.listdir(SPEC_DIR):
        if name.startswith("librm_spec_") and name.endswith(".so"):
            if name.startswith(keep):
                live.add(name[len(keep):-3])
            else:
                os.remove(os.path.join(SPEC_DIR, name))
    for name in os.listdir(SPEC_DIR):
        if name.startswith("code_") and name.endswith(".h") and name[5:-2] not in live:
            os.remove(os.path.join(SPEC_DIR, name))


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand):
            return cand
    return "hipcc"


def build(cs: CompiledScene, force: bool = False, precision: str = "exact") -> str:
    """hipcc the specialised library for this program (no GPU needed)."""
    os.makedirs(SPEC_DIR, exist_ok=True)
    h = scene_hash(cs, precision)
    header = os.path.join(SPEC_DIR, f"code_{h}.h")
    target = lib_path(cs, precision)
    if not force and os.path.isfile(target):
        return target
    # several ranks may build the same scene at once: never let a concurrent hipcc read a half-written header
    text = code_header(cs)
    if not (os.path.isfile(header) and open(header).read() == text):
        htmp = header + f".tmp{os.getpid()}_{threading.get_ident()}"
        with open(htmp, "w") as f:
            f.write(text)
        os.replace(htmp, header)
    tmp = target + f".tmp{os.getpid()}_{threading.get_ident()}"      # (ranks and threads may build the same scene at once)
    cmd = [_hipcc(), *variant(precision)[1], f'-DRM_STATIC_CODE="{header}"']
    if not static_backward(cs):
        cmd.append("-DRM_NO_BACKWARD")
    cmd += [os.path.join(CSRC, "rm_abi.hip"), "-o", tmp]
    if not cs.has_user_types:
        subprocess.run(cmd, check=True, cwd=CSRC)
    else:
        # user source goes through the compiler here: its diagnostics belong in the exception, and the frame kernel's
        # occupancy in the log (a leaf slightly heavier than a torus can cost k_render_fwd its fifth wave: INTEGRATION.md)
        t0 = time.time()
        r = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True)
        if r.returncode != 0:
            errors = "\n".join(line for line in r.stderr.splitlines() if "remark:" not in line)
            raise _abi.RmError(f"hipcc failed ({r.returncode}) on the specialised library of a scene with user {user_names(cs)[1]} "
                               f"({user_names(cs)[0]}):\n{errors[-4000:]}")
        occ, cur = [], None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = m.group(1)
            m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
            if m and cur and "k_render_fwd" in cur:
                occ.append(int(m.group(1)))
        print(f"ray_marching_amd: built {os.path.basename(target)} for a scene of {cs.n_instr} instructions with user {user_names(cs)[1]} "
              f"{user_names(cs)[0]} ({precision}) in {time.time() - t0:.1f} s of hipcc; k_render_fwd "
              f"occupancy {'/'.join(map(str, sorted(set(occ)))) or '?'} waves per SIMD", file=sys.stderr, flush=True)
    os.replace(tmp, target)
    return target


_uses: dict[str, int] = {}
_builder = {"thread": None, "hash": None}
_lock = threading.Lock()


def _background_build(cs: CompiledScene, h: str):
    try:
        build(cs)
    except Exception:      # a failed background build just leaves the scene on the interpreter
        pass
    finally:
        with _lock:
            _loaded.pop(h, None)          # next load() finds (or does not find) the file
            _builder["thread"] = None
            _builder["hash"] = None


def _open(cs: CompiledScene, precision: str, h: str, path: str):
    """The tail of load and load_user: build the library where it is missing, load it and remember it."""
    if not os.path.isfile(path):
        build(cs, precision=precision)
    lib = _loaded[h] = _abi.bind(C.CDLL(path))
    return lib


def load(cs: CompiledScene, precision: str = "exact"):
    """The specialised library for this program, or None (policy in the module docstring)."""
    policy = os.environ.get("RM_SPECIALIZE", "auto")
    if policy == "off":
        return None
    h = scene_hash(cs, precision)
    if h in _loaded:
        return _loaded[h]
    path = lib_path(cs, precision)
    if not os.path.isfile(path) and policy != "jit":
        _loaded[h] = None
        return None
    return _open(cs, precision, h, path)


def load_user(cs: CompiledScene, precision: str = "exact"):
    """The library of a scene with user-defined leaves (combinators, warps, or a user shader): never None.  "auto" and "jit" build a missing library now, on
    first use (the interpreter cannot bridge the wait); "prebuilt" and "off" raise, naming it."""
    policy = os.environ.get("RM_SPECIALIZE", "auto")
    names, what = user_names(cs)
    path = lib_path(cs, precision)
    if policy == "off":
        raise _abi.RmError(f"RM_SPECIALIZE=off: a scene with user-defined {what} ({names}) runs only through its specialised "
                           f"library {path}; the LDS interpreter has no handler for them")
    h = scene_hash(cs, precision)
    lib = _loaded.get(h)
    if lib is not None:
        return lib
    if not os.path.isfile(path):
        if policy not in ("auto", "jit"):
            raise _abi.RmError(f"RM_SPECIALIZE={policy}: the specialised library {path} of a scene with user-defined {what} "
                               f"({names}) has not been built (specialize.build), and the LDS interpreter has no handler for them")
        if shutil.which(_hipcc()) is None:
            raise _abi.RmError(f"the specialised library {path} of a scene with user-defined {what} ({names}) is missing and "
                               "hipcc is not available to build it")
    return _open(cs, precision, h, path)


def note_interpreted_launch(cs: CompiledScene):
    """Called by CompiledScene.lib() each time a scene runs through the interpreter: under the "auto"
    policy a scene used often enough gets its library built in the background (one build at a time).
    Returns True when a finished build is waiting to be picked up."""
    if os.environ.get("RM_SPECIALIZE", "auto") != "auto":
        return False
    h = scene_hash(cs)
    n = _uses.get(h, 0) + 1
    _uses[h] = n
    after = int(os.environ.get("RM_SPECIALIZE_AFTER", "64"))
    if n < after:
        return False
    with _lock:
        if os.path.isfile(lib_path(cs)):
            _loaded.pop(h, None)
            return True
        if _builder["thread"] is None and n == after and shutil.which(_hipcc()) is not None:
            t = threading.Thread(target=_background_build, args=(cs, h), name="rm-specialize", daemon=True)
            _builder["thread"], _builder["hash"] = t, h
            t.start()
    return False


def wait_for_background_build(timeout: float = 120.0):
    t = _builder["thread"]
    if t is not None:
        t.join(timeout)


def ensure(module_or_cs):
    """Build (if needed) and load the specialised library for a scene module."""
    from .compiler import compiled_for
    cs = module_or_cs if isinstance(module_or_cs, CompiledScene) else compiled_for(module_or_cs)
    build(cs)
    _loaded.pop(scene_hash(cs), None)
    prev = os.environ.get("RM_SPECIALIZE")
    os.environ["RM_SPECIALIZE"] = "jit"
    try:
        lib = load(cs)
    finally:
        if prev is None:
            del os.environ["RM_SPECIALIZE"]
        else:
            os.environ["RM_SPECIALIZE"] = prev
    cs._lib = None
    return lib


def default_scenes():
    from .scene import scene_registry as R
    from .scene.primitives import SDFSphere
    from .contrib import make_carved_scene, make_link_scene, make_painted_scene, make_warped_scene
    return {
        "link_scene": make_link_scene(),
        "bounded_link_scene": make_link_scene(bounded=True),
        "sphere": SDFSphere(0.5),
        "make_test_scene2": R.make_test_scene2(),
        "make_test_scene": R.make_test_scene(),
        "make_closed_test_scene": R.make_closed_test_scene(),
        "make_many_primitive_scene32": R.make_many_primitive_scene(32),
        "carved_scene": make_carved_scene(),
        "warped_scene": make_warped_scene(),
        "bounded_warped_scene": make_warped_scene(bounded=True),
        "painted_scene": make_painted_scene(),
    }


def prebuild_default_scenes(parallel: int = 4):
    """Called by __graft_entry__.build(): specialised libraries for the BASELINE config scenes (exact
    arithmetic for all of them, plus the opt-in fast variant of the two frame-benchmark scenes)."""
    from concurrent.futures import ThreadPoolExecutor
    prune_stale()
    scenes = default_scenes()
    todo = [(compile_scene(m), "exact") for m in scenes.values()]
    todo += [(compile_scene(scenes[k]), "fast") for k in ("make_test_scene2", "make_closed_test_scene")]
    with ThreadPoolExecutor(max_workers=parallel) as ex:
        return list(ex.map(lambda job: build(job[0], precision=job[1]), todo))
