"""User-defined per-pixel shaders (ray_marching_amd/extensions.py: register_shader): registration, the (scene, shader) program
of compiler.compiled_with_shader, the specialised library that carries the shader's HIP source, and -- on the GPU -- parity of
test-defined twins of the Lambertian, normal and vignette shaders with the built-in modes (every bit, frames and gradients),
of contrib's DirectionalLightShader and DepthCueShader with the CPU (values <= 1e-5, gradients <= 1e-4: the contract of
smoke()), two shaders and a built-in mode in alternation on one RenderLoop, a shader on a scene with user-defined nodes, and a
captured training step that optimises a shader's parameters.

The CPU side of a frame with a user shader is oracle.render with ``O.shade`` replaced, for the length of that one call, by a
function that calls the shader's own PyTorch ``forward`` (cpu_frame below).

One statement of the issue cannot hold literally and is checked in the form that can: "the program is row for row the scene's"
AND "derived constants keep starting at n_params".  The instruction fields that point into the derived block (capsule
constants, cull bounds, bound tables) are absolute offsets, so they move up with n_params; every other field of every row is
the scene's (test_compiled_with_shader), and a scene without derived constants keeps its program bit for bit.
"""
import copy
import functools
import hashlib
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import sdf_oracle as O
from tests import helpers as H
from tests.helpers import _same

DEV = "cuda"


# --------------------------------------------------------------------------------------------------------------
# test-defined shaders: the built-in Lambertian (mode 0), normal (4) and vignette (3) restated, without parameters
# --------------------------------------------------------------------------------------------------------------
class _Shader(nn.Module):
    pass


class ULambert(_Shader):
    def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
        return (ray_directions * surface_normals).sum(dim=-1, keepdim=True).neg().clamp(0, 1).expand(*surface_normals.shape[:-1], 3)


ULAMBERT_HIP = """
template <bool Fast> RM_DEV rm::V3 ulambert_fwd(const rm::ShadeIn& s, const float* theta) {
  const float c = t_clamp(-dot_seq(s.v, s.n), 0.0f, 1.0f);
  return mk3(c, c, c);
}
template <bool Fast> RM_DEV void ulambert_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 gi, rm::ShadeGrad& gs, float* gtheta) {
  const float c = -dot_seq(s.v, s.n);
  const float g = (c >= 0.0f && c <= 1.0f) ? ((gi.x + gi.y) + gi.z) : 0.0f;
  gs.n = gs.n + mk3(-g * s.v.x, -g * s.v.y, -g * s.v.z);
  gs.v = gs.v + mk3(-g * s.n.x, -g * s.n.y, -g * s.n.z);
}
"""


class UNormal(_Shader):
    def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
        return surface_normals.abs().clamp(0, 1)


UNORMAL_HIP = """
template <bool Fast> RM_DEV rm::V3 unormal_fwd(const rm::ShadeIn& s, const float* theta) {
  return mk3(t_clamp(fabsf(s.n.x), 0.0f, 1.0f), t_clamp(fabsf(s.n.y), 0.0f, 1.0f), t_clamp(fabsf(s.n.z), 0.0f, 1.0f));
}
template <bool Fast> RM_DEV void unormal_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 gi, rm::ShadeGrad& gs, float* gtheta) {
  gs.n = gs.n + mk3((fabsf(s.n.x) <= 1.0f) ? gi.x * sgn0(s.n.x) : 0.0f,
                    (fabsf(s.n.y) <= 1.0f) ? gi.y * sgn0(s.n.y) : 0.0f,
                    (fabsf(s.n.z) <= 1.0f) ? gi.z * sgn0(s.n.z) : 0.0f);
}
"""


class UVignette(_Shader):
    def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
        col2 = pixel_frames[:, None, None, :, 2]
        return (ray_directions * col2).sum(dim=-1, keepdim=True).pow(3).expand(*ray_directions.shape[:-1], 3)


UVIGNETTE_HIP = """
template <bool Fast> RM_DEV rm::V3 uvignette_fwd(const rm::ShadeIn& s, const float* theta) {
  const float d = dot_seq(s.v, s.col2);
  const float c = (d * d) * d;
  return mk3(c, c, c);
}
template <bool Fast> RM_DEV void uvignette_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 gi, rm::ShadeGrad& gs, float* gtheta) {
  const float d = dot_seq(s.v, s.col2);
  const float gd = ((gi.x + gi.y) + gi.z) * (3.0f * (d * d));
  gs.v = gs.v + mk3(gd * s.col2.x, gd * s.col2.y, gd * s.col2.z);
  gs.col2 = gs.col2 + mk3(gd * s.v.x, gd * s.v.y, gd * s.v.z);
}
"""

TWINS = {"lambertian": (ULambert, 0), "normal": (UNormal, 4), "vignette": (UVignette, 3)}


def _register():
    from ray_marching_amd.extensions import register_shader
    register_shader(ULambert, hip=ULAMBERT_HIP)
    register_shader(UNormal, hip=UNORMAL_HIP)
    register_shader(UVignette, hip=UVIGNETTE_HIP)


def _scenes():
    from ray_marching_amd.scene import scene_registry as R
    return {"scene2": R.make_test_scene2, "closed_scene1": R.make_closed_test_scene}


def directional():
    from ray_marching_amd.contrib import DirectionalLightShader
    return DirectionalLightShader(light_direction=[0.35, 0.5, -0.8], albedo=[0.9, 0.55, 0.3], ambient=0.15)


def depth_cue():
    from ray_marching_amd.contrib import DepthCueShader
    return DepthCueShader(density=0.3, far_colour=[0.2, 0.35, 0.6])


CONTRIB = {"directional": directional, "depth_cue": depth_cue}


def gpu_test_programs():
    """Every (scene, shader) program the GPU legs launch: build() compiles their libraries, so that a GPU run of the same tree
    finds them; where they are missing the library builds itself on first use."""
    from ray_marching_amd import contrib, specialize
    from ray_marching_amd.compiler import compile_scene
    _register()
    out = [compile_scene(make(), cls()) for make in _scenes().values() for cls, _ in TWINS.values()]
    out += [compile_scene(_scenes()["scene2"](), make()) for make in CONTRIB.values()]
    out.append(compile_scene(contrib.make_warped_scene(), directional()))
    return list({specialize.scene_hash(cs): cs for cs in out}.values())


# --------------------------------------------------------------------------------------------------------------
# the CPU side
# --------------------------------------------------------------------------------------------------------------
def cpu_frame(spec, shader, monkeypatch, bufs, q, t, steps, sdf_eval=None):
    """oracle.render -- camera, march, normals, all on the CPU -- with the shader's own PyTorch forward where the oracle
    calls its ``shade`` (and, for scenes with user-defined nodes, ``sdf_eval`` where it evaluates the scene)."""
    def shade(mode, degree, px, orientation, frames, dirs, p, n, lap, dist, cmap=None):
        return shader(px, orientation, frames, dirs, p, n)

    with monkeypatch.context() as m:
        m.setattr(O, "shade", shade)
        if sdf_eval is not None:
            m.setattr(O, "sdf_eval", sdf_eval)
        return O.render(spec, bufs, q, t, 0, 1, steps, H.EPS)


def _unit(q):
    return torch.nn.functional.normalize(torch.tensor(q, dtype=torch.float32), dim=-1)


def two_cameras(z=-3.0):
    """Two poses with different orientations, neither about a coordinate axis."""
    q = torch.stack([_unit([0.98, -0.1, 0.15, 0.05]), _unit([1.0, 0.05, -0.1, 0.02])])
    t = torch.tensor([[0.0, 0.0, z], [0.3, -0.2, z + 1.0]])
    return q, t


def inside_the_torus():
    """The reference's default position (0, 0, 1), inside the torus of scene 2: rays that never settle and are deferred."""
    return _unit([0.99, 0.06, -0.08, 0.03])[None], torch.tensor([[0.0, 0.0, 1.0]])


def _bufs(n, h, w):
    return O.camera_buffers(n, w, h, H.PX * h, H.PX * w, H.PX * h)


def _weights(n, h, w, seed):
    return torch.rand(n, h, w, 3, generator=torch.Generator().manual_seed(seed)) + 0.5


def _loss(image, weights):
    """A weighted mean, scaled so that the shader parameters' gradients are of order 0.1 to 1 (the 1e-4 of the gradient
    contract is absolute: it must not be able to hide a wrong gradient)."""
    return (image * weights).mean() * 8.0


BACKWARD_LEGS = {"32x32x16": (32, 32, 16, two_cameras), "deferred_40x24x32": (24, 40, 32, inside_the_torus)}


@functools.lru_cache(maxsize=None)
def cpu_reference(which, leg, edited=False):
    """CPU autograd of one backward leg on scene 2, computed once per (shader, leg, parameters): (shader gradients by name,
    scene gradients in named_parameters() order, dL/dq, dL/dt)."""
    h, w, steps, pose = BACKWARD_LEGS[leg]
    shader = CONTRIB[which]()
    if edited:
        _edit(shader)
    q, t = pose()
    q, t = q.clone().requires_grad_(True), t.clone().requires_grad_(True)
    spec = O.map_spec(O.scene_test2(), lambda x: x.clone().requires_grad_(True))
    mp = pytest.MonkeyPatch()
    try:
        img = cpu_frame(spec, shader, mp, _bufs(q.shape[0], h, w), q, t, steps)
    finally:
        mp.undo()
    _loss(img, _weights(q.shape[0], h, w, 7)).backward()
    return ({n: p.grad.clone() for n, p in shader.named_parameters()}, [p.grad for _, p in O.spec_parameters(spec)], q.grad, t.grad)


def _edit(shader):
    """An in-place edit and a ``.data`` assignment of shader parameters (the same on the CPU and the GPU copy)."""
    first, last = list(shader.parameters())[0], list(shader.parameters())[-1]
    with torch.no_grad():
        first.mul_(0.5)
    last.data = (last.detach() * 1.5 + 0.05).clone()


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
FWD = "template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta) { return s.n; }\n"
VJP = ("template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta) "
       "{ gs.n = gs.n + g; }\n")


def test_registration_errors():
    from ray_marching_amd import contrib, extensions
    from ray_marching_amd.extensions import UserShader, register_combinator, register_leaf, register_shader, register_warp, shader_spec
    from ray_marching_amd.scene.primitives import SDFSphere
    _register()

    def fresh():
        class S(_Shader):
            def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
                return surface_normals
        return S

    src = lambda name: (FWD + VJP).replace("NAME", name)
    with pytest.raises(ValueError, match="exactly two device functions"):
        register_shader(fresh(), hip=FWD.replace("NAME", "novjp"))                                   # missing _vjp
    with pytest.raises(ValueError, match="one NAME"):
        register_shader(fresh(), hip=src("one_a") + FWD.replace("NAME", "one_b"))                    # two NAMEs
    with pytest.raises(ValueError, match="one NAME"):
        register_shader(fresh(), hip=FWD.replace("NAME", "mix_a") + VJP.replace("NAME", "mix_b"))
    with pytest.raises(ValueError, match="inline assembly"):
        register_shader(fresh(), hip=src("withasm").replace("return s.n;", 'asm volatile("" ::: "memory"); return s.n;'))
    with pytest.raises(TypeError, match="nn.Module subclass"):
        register_shader(object, hip=src("notamodule"))
    with pytest.raises(TypeError, match="no forward"):
        register_shader(_Shader, hip=src("noforward"))
    with pytest.raises(ValueError, match="distinct attribute names"):
        register_shader(fresh(), params=("a", "a"), hip=src("dupparams"))
    # a NAME already used by a leaf, a combinator, a warp or another shader
    for taken, owner in (("link", "SDFLink"), ("sdf_intersection", "SDFIntersection"), ("sdf_mirror", "SDFMirror"),
                         ("depth_cue", "DepthCueShader"), ("ulambert", "ULambert")):
        with pytest.raises(ValueError, match=f"identifier '{taken}' is already used by {owner}"):
            register_shader(fresh(), hip=src(taken))
    # ... and the other kinds refuse a shader's NAME
    leaf = ("template <bool Fast> RM_DEV float depth_cue_fwd(rm::V3 p, const float* theta) { return p.x; }\n"
            "template <bool Fast> RM_DEV void depth_cue_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) { gp.x += g; }\n")

    class Leaf(nn.Module):
        def forward(self, p):
            return p[..., :1]
    with pytest.raises(ValueError, match="identifier 'depth_cue' is already used by DepthCueShader"):
        register_leaf(Leaf, params=(), hip=leaf, cost=1)
    # a class already registered as another kind, both ways
    for cls, what in ((contrib.SDFLink, "leaf"), (contrib.SDFIntersection, "combinator"), (contrib.SDFMirror, "warp")):
        with pytest.raises(TypeError, match=f"already registered as a {what}"):
            register_shader(cls, hip=src("otherkind_" + what))
    with pytest.raises(TypeError, match="already registered as a shader"):
        register_leaf(ULambert, params=(), hip=leaf.replace("depth_cue", "shader_as_leaf"), cost=1)
    with pytest.raises(TypeError, match="already registered as a shader"):
        register_combinator(type("C", (UNormal,), {"combine": lambda self, v: v}), hip=(
            "template <bool Fast, int N> RM_DEV float shader_as_comb_fwd(const float (&d)[N], const float* theta) { return d[0]; }\n"
            "template <bool Fast, int N> RM_DEV void shader_as_comb_vjp(const float (&d)[N], const float* theta, float g, float (&gd)[N], "
            "float* gtheta) { gd[0] = g; }\n"))
    with pytest.raises(TypeError, match="already registered as a shader"):
        register_warp(type("W", (UVignette,), {"warp": lambda self, p: p}), hip=(
            "template <bool Fast> RM_DEV rm::V3 shader_as_warp_fwd(rm::V3 p, const float* theta) { return p; }\n"
            "template <bool Fast> RM_DEV void shader_as_warp_vjp(rm::V3 p, const float* theta, rm::V3 gq, rm::V3& gp, float* gtheta) { gp = gp + gq; }\n"))
    with pytest.raises(TypeError, match="already a ray_marching_amd node"):
        register_shader(SDFSphere, hip=src("builtin_node"))
    # registering again: the same source is a no-op, other source or parameters an error
    cls = fresh()
    forward = cls.forward
    assert register_shader(cls, hip=src("again")) is cls and register_shader(cls, hip=src("again")) is cls
    assert cls.forward is forward and "_rm_torch_forward" not in cls.__dict__              # registration leaves forward untouched
    with pytest.raises(ValueError, match="different source or parameters"):
        register_shader(cls, hip=src("again") + "// edited\n")
    with pytest.raises(ValueError, match="different source or parameters"):
        register_shader(cls, params=("gain",), hip=src("again"))
    spec = shader_spec(cls())
    assert isinstance(spec, UserShader) and (spec.cls, spec.name, spec.params, spec.hip) == (cls, "again", (), src("again"))
    assert spec.sha1 == hashlib.sha1(src("again").encode()).hexdigest()
    with pytest.raises(Exception):
        spec.name = "frozen"
    assert shader_spec(type("Derived", (cls,), {})()) is spec and shader_spec(nn.Identity()) is None
    assert {"register_shader", "shader_spec", "UserShader"} <= set(extensions.__all__)
    # called directly, a registered shader is its PyTorch code (CPU tensors here)
    n = torch.nn.functional.normalize(torch.randn(2, 3, 4, 3, generator=torch.Generator().manual_seed(1)), dim=-1)
    v = torch.nn.functional.normalize(torch.randn(2, 3, 4, 3, generator=torch.Generator().manual_seed(2)), dim=-1)
    assert torch.equal(ULambert()(None, None, None, v, None, n), O.shade_lambertian(v, n).expand(2, 3, 4, 3))
    sh = directional()
    light = sh.light_direction / sh.light_direction.norm()
    want = sh.albedo * (sh.ambient + (1 - sh.ambient) * (n * light).sum(-1, keepdim=True).clamp(0, 1))
    assert torch.allclose(sh(None, None, None, v, None, n), want, atol=1e-6)
    assert [k for k, _ in sh.named_parameters()] == ["light_direction", "albedo", "ambient"] and sum(p.numel() for p in sh.parameters()) == 7
    assert [k for k, _ in depth_cue().named_parameters()] == ["density", "far_colour"] and sum(p.numel() for p in depth_cue().parameters()) == 4


# sha1(repr(signature)) of scenes that compiled before this extension point existed, computed at the parent commit
PARENT_SIGNATURES = {
    "scene2": "663383d9a93e783b836a2cfdf8291c3546ab9718",
    "closed_scene1": "2c397b0264226da8c3d4e5a5f8636ae1c01493cb",
    "warped": "c1220fc920684711f47a45a2b7f1d7ba75ed04d9",
}


def _derived_fields(rows):
    """Boolean mask [n, 4] of the instruction fields that hold an offset into the derived block."""
    from ray_marching_amd import _abi
    mask = np.zeros(rows.shape, dtype=bool)
    op = rows[:, 0]
    mask[:, 2] = (op == _abi.OP_LINE) | (op == _abi.OP_CULL_MIN) | ((op == _abi.OP_SMOOTH_BEGIN) & (rows[:, 2] != 0))
    mask[:, 1] = op == _abi.OP_CULL_LSE
    return mask


def test_compiled_with_shader():
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import compile_scene, compiled_for, compiled_with_shader
    from ray_marching_amd.extensions import register_shader
    from ray_marching_amd.scene.primitives import SDFSphere
    _register()
    assert _abi.ABI_VERSION == 14 and _abi.MODE_USER == 8 and len(_abi.MODES) == 8
    sha = lambda text: hashlib.sha1(text.encode()).hexdigest()
    makers = dict(_scenes(), warped=contrib.make_warped_scene)
    before = {}
    for name, make in makers.items():
        scene = make()
        before[name] = (compiled_for(scene).signature, specialize.scene_hash(compiled_for(scene)), specialize.code_header(compiled_for(scene)))
        assert sha(repr(before[name][0])) == PARENT_SIGNATURES[name], name

    class Late(_Shader):       # a shader registered after the scenes were looked at
        def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
            return surface_normals
    register_shader(Late, hip=(FWD + VJP).replace("NAME", "late_shader"))
    for name, make in makers.items():
        scene, shader = make(), directional()
        base = compiled_for(scene)
        cs = compiled_with_shader(scene, shader)
        # the scene itself: signature, library hash and code header are what they were, before and after
        again = compiled_for(scene)
        assert again is base and base.user_shader == () and base.shader_offset == base.n_params
        assert (base.signature, specialize.scene_hash(base), specialize.code_header(base)) == before[name], name
        # the program: every row the scene's, except that offsets into the derived block move up with n_params
        rows, own = cs.program.reshape(-1, 4), base.program.reshape(-1, 4)
        mask = _derived_fields(own)
        assert rows.shape == own.shape and np.array_equal(rows[~mask], own[~mask]), name
        shift = rows[mask] - own[mask]
        assert ((shift >= 7) & (shift <= 10)).all(), name           # 7 floats (a bound table: to the next multiple of 4)
        assert (own[mask] >= base.n_params).all() and (rows[mask] >= cs.n_params).all()
        assert mask.any() == (base.n_derived > 0)
        assert cs.n_params == base.n_params + 7 and cs.shader_offset == base.n_params and cs.n_grad_derived == base.n_grad_derived
        assert (cs.stack_floats, cs.n_slots, cs.n_instr) == (base.stack_floats, base.n_slots, base.n_instr)
        assert len(cs.leaves) == len(base.leaves) + 3 and all(a is b for a, b in zip(cs.leaves, base.leaves))
        assert [id(p) for p in cs.leaves[-3:]] == [id(shader.light_direction), id(shader.albedo), id(shader.ambient)]
        assert cs.leaf_names == base.leaf_names + ["shader.light_direction", "shader.albedo", "shader.ambient"]
        assert cs.leaf_offsets == base.leaf_offsets + [base.n_params, base.n_params + 3, base.n_params + 6]
        assert cs.user_shader == ("directional_light", 7, sha(contrib._DIRECTIONAL_HIP)) and cs.user_shader_source == contrib._DIRECTIONAL_HIP
        assert (cs.user_leaves, cs.user_combinators, cs.user_warps) == (base.user_leaves, base.user_combinators, base.user_warps)
        # the signature: the scene's entries, padded with () to nine, then the shader's
        assert len(cs.signature) == 10 and cs.signature[-1] == cs.user_shader
        assert cs.signature[6:9] == (base.user_leaves, base.user_combinators, base.user_warps)
        rc = _abi.lib.rm_validate_program(cs.program.ctypes.data, cs.program.shape[0], cs.n_params, cs.n_derived, cs.stack_floats, cs.n_slots)
        assert rc == 0, _abi.lib.rm_last_error()
        # cached per (scene, shader) pair
        assert compiled_with_shader(scene, shader) is cs and compiled_with_shader(scene, directional()) is not cs
        assert pack_is_live(cs, shader)
    # a scene without derived constants keeps its program bit for bit
    ball = SDFSphere(0.5)
    assert np.array_equal(compiled_with_shader(ball, depth_cue()).program, compiled_for(ball).program)
    # two shaders on one scene: two hashes; one shader on two scenes: two
    scene, other = makers["scene2"](), makers["closed_scene1"]()
    light, cue = directional(), depth_cue()
    hashes = {specialize.scene_hash(compiled_with_shader(s, sh)) for s in (scene, other) for sh in (light, cue)}
    assert len(hashes) == 4 and not hashes & {specialize.scene_hash(compiled_for(scene)), specialize.scene_hash(compiled_for(other))}
    assert specialize.scene_hash(compiled_with_shader(makers["scene2"](), directional())) == specialize.scene_hash(compiled_with_shader(scene, light))
    # the staleness rule of compiled_for: a change of topology (of the scene or of the shader's parameters) compiles again
    cs = compiled_with_shader(scene, light)
    light.albedo = nn.Parameter(light.albedo.detach().clone())
    cs2 = compiled_with_shader(scene, light)
    assert cs2 is not cs and cs2.leaves[-2] is light.albedo and cs2.signature == cs.signature
    # parameterless shaders, an unregistered module, registered parameters that are not the module's own
    assert compiled_with_shader(scene, ULambert()).n_params == compiled_for(scene).n_params
    assert compiled_with_shader(scene, ULambert()).user_shader == ("ulambert", 0, sha(ULAMBERT_HIP))
    with pytest.raises(TypeError, match="not a registered shader"):
        compile_scene(scene, nn.Identity())
    odd = directional()
    odd.extra = nn.Parameter(torch.zeros(1))
    with pytest.raises(ValueError, match="not all of the shader's parameters"):
        compiled_with_shader(scene, odd)


def pack_is_live(cs, shader):
    """pack_params reads the live values, the shader's behind the scene's."""
    with torch.no_grad():
        shader.ambient.fill_(0.625)
        block = cs.pack_params("cpu")
    return block.numel() == cs.n_params and float(block[-1]) == 0.625 and torch.equal(block[cs.shader_offset:cs.shader_offset + 3], shader.light_direction.detach())


def test_code_header_of_a_scene_with_a_shader():
    from ray_marching_amd import contrib, specialize
    from ray_marching_amd.compiler import compile_scene, compiled_for, compiled_with_shader
    _register()
    scene = _scenes()["scene2"]()
    plain = specialize.code_header(compiled_for(scene))
    # byte for byte what it was before shaders existed: one guard around the program
    rows = ",".join("{%d,%d,%d,%d}" % tuple(r) for r in compiled_for(scene).program.tolist())
    cs0 = compiled_for(scene)
    assert plain == ("// generated by ray_marching_amd/specialize.py -- scene program as a compile-time constant\n"
                     "#ifndef RM_STATIC_CODE_LEAVES\nstruct RmStaticCode {\n"
                     f"  static constexpr int n = {cs0.n_instr}, n_params = {cs0.n_params}, n_derived = {cs0.n_derived},\n"
                     f"                       stack_floats = {cs0.stack_floats}, n_slots = {cs0.n_slots}, n_grad_derived = {cs0.n_grad_derived};\n"
                     f"  static constexpr rm::Ins code[{cs0.n_instr}] = {{{rows}}};\n}};\n#endif\n")
    assert "RM_USER_SHADER" not in plain and "RM_STATIC_CODE_SHADER" not in plain
    cs = compiled_with_shader(scene, depth_cue())
    hdr = specialize.code_header(cs)
    assert "#if defined(RM_STATIC_CODE_SHADER)\n#define RM_USER_SHADER 1\n" in hdr
    assert f"#define RM_USER_SHADER_THETA {cs0.n_params}\n" in hdr and "#define RM_USER_SHADER_PARAMS 4\n" in hdr
    assert contrib._DEPTH_CUE_HIP.strip() in hdr and hdr.count("RM_DEV rm::V3 depth_cue_fwd") == 1
    assert "return depth_cue_fwd<Fast>(s, theta);" in hdr and "depth_cue_vjp<Fast>(s, theta, g, gs, gtheta);" in hdr
    assert f"n_params = {cs0.n_params + 4}," in hdr and "RM_USER_LEAVES" not in hdr
    assert hdr.index("RM_USER_SHADER") < hdr.index("#elif defined(RM_STATIC_CODE_LEAVES)") < hdr.index("struct RmStaticCode")
    # a scene with user nodes and a shader: the four sections side by side; without a shader, no shader section
    warped = contrib.make_warped_scene()
    both = specialize.code_header(compile_scene(warped, directional()))
    assert "#define RM_USER_SHADER 1" in both and "#define RM_USER_WARPS 4" in both and "#define RM_USER_COMBINATORS 1" in both
    assert both.index("#define RM_USER_SHADER 1") < both.index("#elif defined(RM_STATIC_CODE_LEAVES)") < both.index("#define RM_USER_COMBINATORS 1")
    assert "RM_USER_SHADER" not in specialize.code_header(compile_scene(warped))
    assert specialize.user_names(compile_scene(warped, directional())) == (
        "combinators: sdf_intersection; warps: sdf_mirror, sdf_scale, sdf_elongate, sdf_repeat; shaders: directional_light",
        "combinators, warps and shaders")
    assert specialize.user_names(cs) == ("depth_cue", "shaders")


def test_specialised_library_cross_compiles_and_reports_its_shader(monkeypatch, tmp_path):
    from ray_marching_amd import _abi, specialize
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.extensions import register_shader
    from ray_marching_amd.scene.primitives import SDFSphere
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    assert "rm_user_shaders" in _abi.EXPORTED_SYMBOLS
    assert _abi.lib.rm_user_shaders() == 0 and _abi.lib.rm_abi_version() == _abi.ABI_VERSION == 14      # the generic library
    monkeypatch.setattr(specialize, "SPEC_DIR", str(tmp_path))
    specialize._loaded.clear()
    cs = compile_scene(SDFSphere(0.5), depth_cue())
    # the interpreter is never an option, and neither is a library that was not built
    monkeypatch.setenv("RM_SPECIALIZE", "off")
    with pytest.raises(_abi.RmError, match=r"user-defined shaders \(depth_cue\)"):
        cs.lib()
    monkeypatch.setenv("RM_SPECIALIZE", "prebuilt")
    with pytest.raises(_abi.RmError, match="librm_spec_"):
        cs.lib()
    path = specialize.build(cs)
    assert os.path.isfile(path) and os.path.dirname(path) == str(tmp_path)
    lib = cs.lib()
    assert lib is not _abi.lib and lib.rm_user_shaders() == 1 and lib.rm_abi_version() == _abi.ABI_VERSION
    assert (lib.rm_user_leaves(), lib.rm_user_combinators(), lib.rm_user_warps()) == (0, 0, 0)
    assert cs.lib(True) is lib and cs.specialised
    monkeypatch.setenv("RM_STATIC_BACKWARD_ACC", "4")              # 1 + 4 accumulators
    with pytest.raises(_abi.RmError, match="RM_STATIC_BACKWARD_ACC"):
        cs.lib(True)
    monkeypatch.delenv("RM_STATIC_BACKWARD_ACC")
    # a shader that does not compile: hipcc's own words reach the caller

    class Broken(_Shader):
        def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
            return surface_normals
    register_shader(Broken, hip=(FWD + VJP).replace("NAME", "broken_shader").replace("return s.n;", "return no_such_helper(s.n);"))
    monkeypatch.setenv("RM_SPECIALIZE", "jit")
    with pytest.raises(_abi.RmError, match="no_such_helper"):
        compile_scene(SDFSphere(0.5), Broken()).lib()
    specialize._loaded.clear()


def test_render_loop_argument_handling(monkeypatch):
    """Host side, before any device work: the loop lives on the CPU, where a frame that got as far as its camera buffers
    would be refused for that reason instead."""
    from ray_marching_amd import _abi, specialize
    from ray_marching_amd.scene.primitives import SDFSphere
    _register()
    loop = H.make_loop(SDFSphere(0.5), 8, 8, device="cpu")
    q, t = torch.tensor([[1.0, 0.0, 0.0, 0.0]]), torch.tensor([[0.0, 0.0, -3.0]])
    for call in (lambda m: loop(q, t, m, 1, 4), lambda m: loop(q, t, mode=m), lambda m: loop.display_frame(q, t, m),
                 lambda m: loop.capture(mode=m)):
        with pytest.raises(TypeError, match="register_shader"):
            call(nn.Identity())
        with pytest.raises(TypeError, match="register_shader"):
            call("lambertian")
    monkeypatch.setenv("RM_SPECIALIZE", "off")
    specialize._loaded.clear()
    for call in (lambda m: loop(q, t, m, 1, 4), lambda m: loop.display_frame(q, t, m), lambda m: loop.capture(mode=m)):
        with pytest.raises(_abi.RmError, match=r"RM_SPECIALIZE=off.*user-defined shaders \(depth_cue\)"):
            call(depth_cue())
    # an int keeps going through mode % 8: such a frame gets as far as the camera buffers
    for mode in (12, np.int64(3), True):
        with pytest.raises(RuntimeError, match="camera buffers is on cpu"):
            loop(q, t, mode, 1, 4)
    step = loop.training_step(lambda image: image.mean(), mode=depth_cue())
    assert isinstance(step.mode, nn.Module) and loop.training_step(lambda image: image.mean(), mode=3).mode == 3


@pytest.mark.parametrize("which", sorted(CONTRIB))
@pytest.mark.parametrize("leg", sorted(BACKWARD_LEGS))
def test_cpu_gradients_of_the_shader_parameters_are_not_small(which, leg):
    """The 1e-4 of the gradient contract is absolute: pose, parameters and loss of the GPU legs are chosen so that every
    component of every shader parameter's CPU gradient is at least 1e-2 (and finite), before and after the edit."""
    for edited in (False, True):
        grads = cpu_reference(which, leg, edited)[0]
        for name, g in grads.items():
            print(f"{which} {leg} edited={edited}: CPU grad {name} {g.tolist()}")
            assert bool(torch.isfinite(g).all()) and g.abs().min().item() >= 1e-2, (name, g)


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scene2", "closed_scene1"])
@pytest.mark.parametrize("twin", sorted(TWINS))
def test_restated_builtin_shader_is_bit_identical_with_the_builtin_mode(which, twin, monkeypatch):
    """Zero tolerance: the twin restates the built-in mode's forward and VJP operation for operation, so a 60x44 frame of two
    cameras (partial tiles on both edges, 32 steps) is the same bits through the tile kernel, the ray pools (regen=True), a
    captured replay, display_frame and a float16 module, and the scene-parameter and pose gradients of an MSE loss over a
    32x32x16 frame of two cameras are too.  Every ray is walked in place (no deferred-ray list, whose atomically ordered
    partial sums are the one thing here that is not a function of the program); the deferred rule has its own leg in
    test_contrib_shader_against_the_cpu."""
    from ray_marching_amd import ops
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    _register()
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)
    cls, mode = TWINS[twin]
    shader = cls()
    scene = _scenes()[which]().to(DEV)
    lib = compiled_with_shader(scene, shader).lib()
    assert lib.rm_user_shaders() == 1 and compiled_for(scene).lib().rm_user_shaders() == 0
    h, w, steps = 44, 60, 32
    q, t = two_cameras(-3.0 if which == "scene2" else -1.5)
    q, t = q.to(DEV), t.to(DEV)
    with torch.no_grad():
        for kw in (dict(), dict(regen=True)):
            loop = H.make_loop(scene, h, w, n=2, **kw)
            want = loop(q, t, mode, 1, steps)
            got = loop(q, t, shader, 1, steps)
            assert got.shape == (2, h, w, 3) and got.dtype == torch.float32 and _same(got, want.expand(2, h, w, 3)), kw
            assert _same(loop.capture(mode=shader, marching_steps=steps)(q, t), got), kw
            assert _same(loop(q, t, shader, 1, steps, rows=(9, 30)), got[:, 9:30]), kw
        one = H.make_loop(scene, h, w)
        assert _same(one.display_frame(q[1:], t[1:], shader, 1, steps), one.display_frame(q[1:], t[1:], mode, 1, steps))
        assert _same(one.capture(mode=shader, marching_steps=steps, display=True)(q[1:], t[1:]), one.display_frame(q[1:], t[1:], mode, 1, steps))
        half = H.make_loop(_scenes()[which](), h, w, n=2).to(torch.float16)
        got16, want16 = half(q.half(), t.half(), shader, 1, steps), half(q.half(), t.half(), mode, 1, steps)
        assert got16.dtype == torch.float16 and _same(got16, want16.expand(2, h, w, 3))
        assert _same(H.make_loop(_scenes()[which](), h, w).to(torch.float16).display_frame(q[:1].half(), t[:1].half(), shader, 1, steps),
                     H.make_loop(_scenes()[which](), h, w).to(torch.float16).display_frame(q[:1].half(), t[:1].half(), mode, 1, steps))
    # gradients
    h, w, steps = 32, 32, 16
    target = torch.rand(2, h, w, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    grads = {}
    for key, m in (("builtin", mode), ("twin", shader)):
        loop = H.make_loop(scene, h, w, n=2)
        for x in scene.parameters():
            x.grad = None
        qg, tg = q.clone().requires_grad_(True), t.clone().requires_grad_(True)
        (loop(qg, tg, m, 1, steps).expand(2, h, w, 3) - target).pow(2).mean().backward()
        grads[key] = [x.grad.clone() for x in scene.parameters()] + [qg.grad, tg.grad]
    names = [n for n, _ in scene.named_parameters()] + ["orientations", "translations"]
    for name, a, b in zip(names, grads["twin"], grads["builtin"]):
        print(f"{which} {twin}: grad {name} max|diff| {(a - b).abs().max().item():.3g} (|g| {b.abs().max().item():.3g})")
    for name, a, b in zip(names, grads["twin"], grads["builtin"]):
        assert _same(a, b), name
    assert any(float(g.abs().max()) > 0 for g in grads["builtin"][-2:])


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(CONTRIB))
def test_contrib_shader_against_the_cpu(which, monkeypatch):
    """DirectionalLightShader / DepthCueShader on scene 2 against the oracle with the shader's PyTorch forward as its shade():
    values of a 60x44x32 frame of two cameras <= 1e-5 (restated math mode of the oracle: host independent), gradients of the
    scene parameters, the pose and every shader parameter <= 1e-4 against CPU autograd, at 32x32x16 with two cameras and at
    40x24x32 from inside the torus, where rays are deferred (asserted) and the shader's direct dependence on the ray origin
    takes the deferred rule.  Then an in-place edit and a ``.data`` assignment of shader parameters: the next backward
    follows the new values."""
    from ray_marching_amd import ops
    from ray_marching_amd.compiler import compiled_with_shader
    shader = CONTRIB[which]().to(DEV)
    cpu_shader = CONTRIB[which]()
    scene = _scenes()["scene2"]().to(DEV)
    assert compiled_with_shader(scene, shader).lib().rm_user_shaders() == 1
    h, w, steps = 44, 60, 32
    q, t = two_cameras()
    with torch.no_grad(), O.math_mode("restated"):
        want = cpu_frame(O.scene_test2(), cpu_shader, monkeypatch, _bufs(2, h, w), q, t, steps)
    with torch.no_grad():
        for kw in (dict(), dict(regen=True)):
            got = H.make_loop(scene, h, w, n=2, **kw)(q.to(DEV), t.to(DEV), shader, 1, steps).cpu()
            err, frac = H.report(f"{which} frame", got, want)
            print(f"{which} {kw}: frame max|err| {err:.3g}, {frac:.3g} of the values beyond 1e-5")
            assert got.shape == (2, h, w, 3) and err <= 1e-5
    for edited in (False, True):
        if edited:
            _edit(shader)
        for leg, (h, w, steps, pose) in BACKWARD_LEGS.items():
            want_shader, want_scene, want_q, want_t = cpu_reference(which, leg, edited)
            q, t = pose()
            n = q.shape[0]
            qg, tg = q.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
            for x in list(scene.parameters()) + list(shader.parameters()):
                x.grad = None
            sink = torch.zeros(int(ops._lib.rm_wave_tiles(n, h, w, 2)), dtype=torch.int32, device=DEV)
            monkeypatch.setattr(ops, "bwd_tile_cost_sink", sink)          # (measurement hook: keeps the backward's workspace)
            _loss(H.make_loop(scene, h, w, n=n)(qg, tg, shader, 1, steps), _weights(n, h, w, 7).to(DEV)).backward()
            torch.cuda.synchronize()
            deferred = int(ops.bwd_last_work[32])
            monkeypatch.setattr(ops, "bwd_tile_cost_sink", None)
            print(f"{which} {leg} edited={edited}: {deferred} rays deferred")
            if leg.startswith("deferred"):
                assert deferred > 0, "no ray was deferred: the leg does not exercise the deferred rule"
            bad = []
            for name, p in shader.named_parameters():
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
                c = want_shader[name]
                assert c.abs().min().item() >= 1e-2, name
                e = (p.grad.cpu() - c).abs().max().item()
                print(f"{which} {leg} edited={edited}: shader grad {name} max|err| {e:.3g} (CPU {c.tolist()})")
                if not e <= 1e-4:
                    bad.append(name)
            for (name, p), c in zip(scene.named_parameters(), want_scene):
                c = c if c is not None else torch.zeros_like(p.grad.cpu())
                e = (p.grad.cpu() - c).abs().max().item()
                print(f"{which} {leg} edited={edited}: scene grad {name} max|err| {e:.3g} (|g| {c.abs().max().item():.3g})")
                if not e <= 1e-4:
                    bad.append(name)
            for name, g, c in (("orientations", qg.grad, want_q), ("translations", tg.grad, want_t)):
                e = (g.cpu() - c).abs().max().item()
                print(f"{which} {leg} edited={edited}: grad {name} max|err| {e:.3g} (|g| {c.abs().max().item():.3g})")
                if not e <= 1e-4:
                    bad.append(name)
            assert not bad, (leg, edited, bad)
    if which == "depth_cue":      # the shader that reads the ray origin: the pose translation gets a gradient through it
        assert cpu_reference(which, "32x32x16")[3].abs().max().item() > 1e-2


@pytest.mark.gpu
def test_two_shaders_and_a_builtin_mode_in_alternation_on_one_loop():
    """One scene, one RenderLoop; DirectionalLightShader, DepthCueShader and mode 0 in turn, twice: each frame is the bits of
    its own single-shader render on a loop of its own, so the (scene, shader) programs, their libraries and block caches do
    not bleed into each other or into the scene's own program."""
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    h, w, steps = 44, 60, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    modes = {"directional": directional().to(DEV), "depth_cue": depth_cue().to(DEV), "lambertian": 0}
    with torch.no_grad():
        want = {k: H.make_loop(_scenes()["scene2"]().to(DEV), h, w, n=2)(q, t, CONTRIB[k]().to(DEV) if k in CONTRIB else m, 1, steps)
                for k, m in modes.items()}
        scene = _scenes()["scene2"]().to(DEV)
        loop = H.make_loop(scene, h, w, n=2)
        for rnd in range(2):
            for k, m in modes.items():
                assert _same(loop(q, t, m, 1, steps), want[k].expand(2, h, w, 3)), (rnd, k)
    assert not _same(want["directional"], want["depth_cue"])
    base = compiled_for(scene)
    assert base.user_shader == () and base.lib().rm_user_shaders() == 0
    a, b = compiled_with_shader(scene, modes["directional"]), compiled_with_shader(scene, modes["depth_cue"])
    assert a is not b and a.lib() is not b.lib() and a.lib() is not base.lib() and a.lib().rm_user_shaders() == 1


@pytest.mark.gpu
def test_shader_on_a_scene_with_user_nodes(monkeypatch):
    """contrib.make_warped_scene() (user warps and a user combinator) shaded by DirectionalLightShader: the four guards in one
    translation unit.  Values <= 1e-5, gradients of the scene's and the shader's parameters <= 1e-4 against the CPU."""
    from ray_marching_amd import contrib
    from ray_marching_amd.compiler import compiled_with_shader
    from tests.test_user_warp import cpu_eval, cpu_parameters, spec_of
    scene = contrib.make_warped_scene()
    spec = spec_of(scene)
    scene = scene.to(DEV)
    shader, cpu_shader = directional().to(DEV), directional()
    lib = compiled_with_shader(scene, shader).lib()
    assert (lib.rm_user_shaders(), lib.rm_user_warps(), lib.rm_user_combinators(), lib.rm_user_leaves()) == (1, 4, 1, 0)
    h, w, steps = 44, 60, 32
    q, t = two_cameras()
    with torch.no_grad():
        want = cpu_frame(spec, cpu_shader, monkeypatch, _bufs(2, h, w), q, t, steps, sdf_eval=cpu_eval)
        got = H.make_loop(scene, h, w, n=2)(q.to(DEV), t.to(DEV), shader, 1, steps).cpu()
    err, frac = H.report("warped frame", got, want)
    print(f"warped scene + directional light: frame max|err| {err:.3g}, {frac:.3g} of the values beyond 1e-5")
    assert err <= 1e-5
    h, w, steps = 32, 32, 16
    wts = _weights(2, h, w, 7)
    _loss(cpu_frame(spec, cpu_shader, monkeypatch, _bufs(2, h, w), q, t, steps, sdf_eval=cpu_eval), wts).backward()
    _loss(H.make_loop(scene, h, w, n=2)(q.to(DEV), t.to(DEV), shader, 1, steps), wts.to(DEV)).backward()
    pairs = list(zip(scene.named_parameters(), cpu_parameters(spec))) + list(zip(shader.named_parameters(), cpu_shader.parameters()))
    assert len(pairs) == len(list(scene.parameters())) + 3
    bad = []
    for (name, g), c in pairs:
        cg = c.grad if c.grad is not None else torch.zeros_like(c)
        assert g.grad is not None, name
        e = (g.grad.cpu() - cg).abs().max().item()
        print(f"warped scene + directional light: grad {name} max|err| {e:.3g} (|g| {cg.abs().max().item():.3g})")
        if not e <= 1e-4:
            bad.append(name)
    assert not bad, bad
    assert min(p.grad.abs().min().item() for p in cpu_shader.parameters()) >= 1e-2


@pytest.mark.gpu
def test_training_step_moves_a_perturbed_shader_back():
    """Ten Adam steps on light_direction and albedo of a DirectionalLightShader, towards a frame of scene 2 rendered with the
    unperturbed shader: each replayed step of the captured graph gives the loss of the eager step taken from the same
    parameters (1e-6 max(1, |loss|), the tolerance of test_training_step_moves_a_perturbed_warped_scene_back), both
    parameters end nearer the values the target was rendered with, and the loss after the run is below the loss before."""
    h, w, steps = 32, 32, 16
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    truth = directional()
    with torch.no_grad():
        target = H.make_loop(_scenes()["scene2"]().to(DEV), h, w, n=2)(q, t, directional().to(DEV), 1, steps).clone()
    loss_fn = lambda image: (image - target).pow(2).mean()

    def perturbed():
        shader = directional().to(DEV)
        with torch.no_grad():
            shader.light_direction += torch.tensor([0.3, -0.25, 0.2], device=DEV)
            shader.albedo += torch.tensor([-0.2, 0.15, 0.2], device=DEV)
        return shader

    def distance(shader):
        light = torch.nn.functional.normalize(shader.light_direction.detach().cpu(), dim=0)
        return ((light - torch.nn.functional.normalize(truth.light_direction.detach(), dim=0)).norm().item(),
                (shader.albedo.detach().cpu() - truth.albedo.detach()).norm().item())

    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*AccumulateGrad node's stream does not match.*")
        scene, shader = _scenes()["scene2"]().to(DEV), perturbed()
        for x in scene.parameters():
            x.requires_grad_(False)
        loop = H.make_loop(scene, h, w, n=2)
        before = distance(shader)
        opt = torch.optim.Adam([shader.light_direction, shader.albedo], lr=2e-2, capturable=True)
        step = loop.training_step(loss_fn, mode=shader, marching_steps=steps, optimizer=opt)
        twin_scene, twin = _scenes()["scene2"]().to(DEV), perturbed()
        twin_loop = H.make_loop(twin_scene, h, w, n=2)
        with torch.no_grad():
            first = float(loss_fn(loop(q, t, shader, 1, steps)))
        losses = []
        for it in range(10):
            if it == 0:
                step(q, t)                                   # warm-up iterations, the capture, one replay
            with torch.no_grad():
                for a, b in zip(twin.parameters(), shader.parameters()):
                    a.copy_(b)
            got = float(step(q, t))
            want = loss_fn(twin_loop(q, t, twin, 1, steps))
            want.backward()                                  # the eager step's own backward (its gradients are not applied)
            for x in list(twin.parameters()) + list(twin_scene.parameters()):
                x.grad = None
            assert abs(got - float(want.detach())) <= 1e-6 * max(1.0, abs(float(want.detach()))), (it, got, float(want.detach()))
            losses.append(got)
        with torch.no_grad():
            last = float(loss_fn(loop(q, t, shader, 1, steps)))
    after = distance(shader)
    print(f"training leg: loss before {first:.6g}, per step {[round(x, 6) for x in losses]}, after {last:.6g}; "
          f"(light, albedo) distance to the target's {before} -> {after}")
    assert after[0] < before[0] and after[1] < before[1]
    assert last < first and losses[-1] < losses[0]
