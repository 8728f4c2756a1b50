"""User-defined shaders that probe the scene (extensions.register_shader(..., probes=K)): registration of the NAME_probe /
NAME_probe_vjp pair, the (scene, shader) program and header that carry K, and -- on the GPU -- a test-local twin of the
built-in normal shader that takes its four taps as probes (every bit of the frame, gradients <= 1e-6), contrib's
AmbientOcclusionShader (K = 5) and SoftShadowShader (K = 8) against the CPU (values <= 1e-5, gradients <= 1e-4: the contract
of smoke()), a float16 module, a captured replay, a captured training step, a scene with user-defined nodes, and probing
and probe-free shaders in alternation on one RenderLoop.

The CPU side of a frame is oracle.render with ``O.shade`` replaced, for the length of that one call, by a function that calls
the shader's own PyTorch ``forward`` and hands it ``lambda x: O.sdf_eval(spec, x)`` as ``scene`` (cpu_frame below).

Two statements of the issue are checked in the form that can hold:
  * "the twin's frame equals built-in mode 3": the built-in normal shader, which is what a restated ``normals_from_taps`` that
    returns |n| can equal, is mode 4 (``_abi.MODES.index("normal")``; 3 is the vignette, which reads no normal at all);
  * "the scene_hash of (scene2, DirectionalLightShader) is the parent's": the library key also hashes the kernel sources, which
    this feature edits, so the key itself moves with every such edit.  What must not move for a probe-free shader is checked:
    the sha1 of its header, the sha1 of its signature, and its key with the kernel-source hash held fixed -- all three recorded
    at the parent commit (PARENT below).
"""
import functools
import hashlib
import os
import warnings

import pytest
import torch
import torch.nn as nn

from oracle import sdf_oracle as O
from tests import helpers as H
from tests.helpers import _same

DEV = "cuda"


# --------------------------------------------------------------------------------------------------------------
# the test-local twin: the built-in normal shader (mode 4), with the tetrahedron's four taps as its own probes
# --------------------------------------------------------------------------------------------------------------
class UTapNormal(nn.Module):
    def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals, scene):
        offs, inv = O.tetra_constants(H.EPS, surface_coords.dtype)
        taps = scene(surface_coords[..., None, :] + offs)
        d = taps[..., 1:, :] - taps[..., :1, :]
        n = torch.nn.functional.normalize((inv * d[..., None, :, 0]).sum(dim=-1), dim=-1, p=2, eps=0.0)
        return n.abs().clamp(0, 1)


def _literal(x):
    return float(x).hex() + "f"         # an exact float literal


def utap_normal_hip():
    """The source of UTapNormal: offsets and inverse matrix printed as exact literals from the host constants the loop uploads
    in RmTetra (rendering/ray_marching.py: tetrahedron_constants -> ops.make_tetra).  ``fwd`` restates normals_from_taps and
    mode 4 of shade_pixel, ``vjp`` mode 4's branch of k_render_bwd and the head of normals_backward, operation for operation."""
    from ray_marching_amd.rendering.ray_marching import tetrahedron_constants
    taps, _, inv = tetrahedron_constants(H.EPS)
    o = [[_literal(v) for v in row] for row in taps.float().tolist()]
    m = [_literal(v) for v in inv.float().reshape(-1).tolist()]
    pick = lambda c: f"(k == 0) ? {o[0][c]} : ((k == 1) ? {o[1][c]} : ((k == 2) ? {o[2][c]} : {o[3][c]}))"
    normal = f"""
  const float d1 = d[1] - d[0], d2 = d[2] - d[0], d3 = d[3] - d[0];
  const rm::V3 u = mk3(({m[0]} * d1 + {m[1]} * d2) + {m[2]} * d3, ({m[3]} * d1 + {m[4]} * d2) + {m[5]} * d3, ({m[6]} * d1 + {m[7]} * d2) + {m[8]} * d3);
  const float nu = norm3(u);
  const rm::V3 n = mk3(u.x / nu, u.y / nu, u.z / nu);"""
    return f"""
template <bool Fast> RM_DEV rm::V3 utap_normal_probe(int k, const rm::ShadeIn& s, const float* theta) {{
  const rm::V3 ok = mk3({pick(0)}, {pick(1)}, {pick(2)});
  return s.p + ok;
}}
template <bool Fast> RM_DEV void utap_normal_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, rm::V3 gq, rm::ShadeGrad& gs, float* gtheta) {{
  gs.p = gs.p + gq;
}}
template <bool Fast> RM_DEV rm::V3 utap_normal_fwd(const rm::ShadeIn& s, const float* theta, const float* d) {{{normal}
  return mk3(t_clamp(fabsf(n.x), 0.0f, 1.0f), t_clamp(fabsf(n.y), 0.0f, 1.0f), t_clamp(fabsf(n.z), 0.0f, 1.0f));
}}
template <bool Fast> RM_DEV void utap_normal_vjp(const rm::ShadeIn& s, const float* theta, const float* d, rm::V3 gi, rm::ShadeGrad& gs,
                                                 float* gtheta, float* gd) {{{normal}
  const rm::V3 gn = mk3((fabsf(n.x) <= 1.0f) ? gi.x * sgn0(n.x) : 0.0f, (fabsf(n.y) <= 1.0f) ? gi.y * sgn0(n.y) : 0.0f,
                        (fabsf(n.z) <= 1.0f) ? gi.z * sgn0(n.z) : 0.0f);
  const float ng = (n.x * gn.x + n.y * gn.y) + n.z * gn.z;
  const rm::V3 gu = mk3((gn.x - n.x * ng) / nu, (gn.y - n.y * ng) / nu, (gn.z - n.z * ng) / nu);
  const float g1 = ({m[0]} * gu.x + {m[3]} * gu.y) + {m[6]} * gu.z;
  const float g2 = ({m[1]} * gu.x + {m[4]} * gu.y) + {m[7]} * gu.z;
  const float g3 = ({m[2]} * gu.x + {m[5]} * gu.y) + {m[8]} * gu.z;
  gd[0] = -((g1 + g2) + g3); gd[1] = g1; gd[2] = g2; gd[3] = g3;
}}
"""


def _register():
    from ray_marching_amd.extensions import register_shader
    register_shader(UTapNormal, hip=utap_normal_hip(), probes=4)


def _scenes():
    from ray_marching_amd.scene import scene_registry as R
    return {"scene2": R.make_test_scene2, "closed_scene1": R.make_closed_test_scene}


def ambient_occlusion():
    from ray_marching_amd.contrib import AmbientOcclusionShader
    return AmbientOcclusionShader(reach=0.4, strength=2.0, albedo=[0.9, 0.6, 0.4])


def soft_shadow():
    from ray_marching_amd.contrib import SoftShadowShader
    return SoftShadowShader(light_direction=[0.35, 0.5, -0.8], albedo=[0.9, 0.55, 0.3], ambient=0.15, sharpness=2.0, reach=2.0, bias=0.02)


def directional():
    from ray_marching_amd.contrib import DirectionalLightShader
    return DirectionalLightShader(light_direction=[0.35, 0.5, -0.8], albedo=[0.9, 0.55, 0.3], ambient=0.15)


CONTRIB = {"ambient_occlusion": ambient_occlusion, "soft_shadow": soft_shadow}


def gpu_test_programs():
    """Every (scene, shader) program the GPU legs launch: build() compiles their libraries, so that a GPU run of the same tree
    finds them; where they are missing the library builds itself on first use."""
    from ray_marching_amd import contrib, specialize
    from ray_marching_amd.compiler import compile_scene
    _register()
    out = [compile_scene(make(), UTapNormal()) for make in _scenes().values()]
    out += [compile_scene(_scenes()["scene2"](), make()) for make in CONTRIB.values()]
    out.append(compile_scene(contrib.make_warped_scene(), ambient_occlusion()))
    out.append(compile_scene(_scenes()["scene2"](), directional()))
    return list({specialize.scene_hash(cs): cs for cs in out}.values())


# --------------------------------------------------------------------------------------------------------------
# the CPU side
# --------------------------------------------------------------------------------------------------------------
def cpu_frame(spec, shader, monkeypatch, bufs, q, t, steps, sdf_eval=None, tetra=None):
    """oracle.render -- camera, march, normals, all on the CPU -- with the shader's own PyTorch forward where the oracle calls its
    ``shade``, the oracle's scene evaluator as the shader's ``scene`` (and, for scenes with user-defined nodes, ``sdf_eval``
    where the oracle evaluates the scene)."""
    def shade(mode, degree, px, orientation, frames, dirs, p, n, lap, dist, cmap=None):
        return shader(px, orientation, frames, dirs, p, n, lambda x: O.sdf_eval(spec, x))

    with monkeypatch.context() as m:
        m.setattr(O, "shade", shade)
        if sdf_eval is not None:
            m.setattr(O, "sdf_eval", sdf_eval)
        return O.render(spec, bufs, q, t, 0, 1, steps, H.EPS, tetra=tetra)


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


LOSS_SCALE = 8.0


def _loss(image, weights):
    """A weighted mean, scaled (with the constructor values above) so that every component of the shader parameters' gradients is
    between 1e-2 and about 10 (the 1e-4 of the gradient contract is absolute: it must not be able to hide a wrong gradient,
    and it must stay above fp32 rounding); the lower end is checked on the CPU by
    test_cpu_gradients_of_the_shader_parameters_are_not_small."""
    return (image * weights).mean() * LOSS_SCALE


BACKWARD_LEGS = {"32x32x16": (32, 32, 16, two_cameras), "deferred_40x24x32": (24, 40, 32, inside_the_torus)}


def _trainable(shader):
    """(name, parameter) of the shader's parameters that take a gradient (SoftShadowShader.bias is a frozen constant)."""
    return [(n, p) for n, p in shader.named_parameters() if p.requires_grad]


def _edit(shader):
    """An in-place edit and a ``.data`` assignment of shader parameters (the same on the CPU and the GPU copy)."""
    first, last = _trainable(shader)[0][1], _trainable(shader)[-1][1]
    with torch.no_grad():
        first.mul_(0.75)
    last.data = (last.detach() * 1.25 + 0.05).clone()


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
    return ({n: p.grad.clone() for n, p in _trainable(shader)}, [p.grad for _, p in O.spec_parameters(spec)], q.grad, t.grad)


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
FWD = "template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta) { return s.n; }\n"
VJP = ("template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta) "
       "{ gs.n = gs.n + g; }\n")
PFWD = "template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta, const float* d) { return d[0] * s.n; }\n"
PVJP = ("template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, const float* d, rm::V3 g, rm::ShadeGrad& gs, "
        "float* gtheta, float* gd) { gs.n = gs.n + d[0] * g; gd[0] = dot_seq(g, s.n); }\n")
PROBE = "template <bool Fast> RM_DEV rm::V3 NAME_probe(int k, const rm::ShadeIn& s, const float* theta) { return s.p + s.n; }\n"
PROBE_VJP = ("template <bool Fast> RM_DEV void NAME_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, rm::V3 gq, rm::ShadeGrad& gs, "
             "float* gtheta) { gs.p = gs.p + gq; gs.n = gs.n + gq; }\n")


def _fresh(probing=True):
    if probing:
        class S(nn.Module):
            def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals, scene):
                return scene(surface_coords + surface_normals) * surface_normals
    else:
        class S(nn.Module):
            def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
                return surface_normals
    return S


def test_registration_errors():
    from ray_marching_amd import contrib, extensions
    from ray_marching_amd.extensions import register_shader, shader_spec
    _register()
    full = lambda name: (PROBE + PROBE_VJP + PFWD + PVJP).replace("NAME", name)
    plain = lambda name: (FWD + VJP).replace("NAME", name)
    assert extensions.RM_USER_SHADER_MAX_PROBES == 8
    # the pairing, both ways
    with pytest.raises(ValueError, match="defines pa_probe / pa_probe_vjp, but probes=0"):
        register_shader(_fresh(), hip=full("pa"))                                             # the pair without probes=
    with pytest.raises(ValueError, match="defines pa2_probe / pa2_probe_vjp, but probes=0"):
        register_shader(_fresh(), hip=full("pa2"), probes=0)
    with pytest.raises(ValueError, match="probes=3, but the source of S defines no pb_probe / pb_probe_vjp"):
        register_shader(_fresh(), hip=plain("pb"), probes=3)                                  # probes= without the pair
    with pytest.raises(ValueError, match=r"both or neither \(found pc_probe: True, pc_probe_vjp: False\)"):
        register_shader(_fresh(), hip=(PROBE + PFWD + PVJP).replace("NAME", "pc"), probes=2)  # one of the two only
    with pytest.raises(ValueError, match=r"both or neither \(found pd_probe: False, pd_probe_vjp: True\)"):
        register_shader(_fresh(), hip=(PROBE_VJP + PFWD + PVJP).replace("NAME", "pd"), probes=2)
    with pytest.raises(ValueError, match=r"both or neither"):
        register_shader(_fresh(), hip=(PROBE_VJP + PFWD + PVJP).replace("NAME", "pd0"))       # ... whatever probes says
    # the range of K: the message names the cap
    for bad in (9, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="probes must be an int from 0 to RM_USER_SHADER_MAX_PROBES = 8"):
            register_shader(_fresh(), hip=full("pe"), probes=bad)
    # the probe pair of another NAME is not this shader's: NAME_probe_vjp of a second name still reads as a second shader
    with pytest.raises(ValueError, match="one NAME"):
        register_shader(_fresh(), hip=full("pf") + PROBE_VJP.replace("NAME", "other"), probes=1)
    with pytest.raises(ValueError, match="inline assembly"):
        register_shader(_fresh(), hip=full("pg").replace("return s.p + s.n;", 'asm volatile("" ::: "memory"); return s.p + s.n;'), probes=1)
    # a second registration: the same K is a no-op, another K an error (probes is one of the fields that must repeat)
    cls = _fresh()
    assert register_shader(cls, hip=full("ph"), probes=1) is cls and register_shader(cls, hip=full("ph"), probes=1) is cls
    with pytest.raises(ValueError, match="already registered with different source or parameters"):
        register_shader(cls, hip=full("ph"), probes=2)
    assert "probes" in extensions._KINDS["shader"].same
    spec = shader_spec(cls())
    assert (spec.name, spec.probes, spec.params) == ("ph", 1, ()) and shader_spec(type("Derived", (cls,), {})()) is spec
    for k in (1, 8):
        assert shader_spec(register_shader(_fresh(), hip=full(f"pk{k}"), probes=k)()).probes == k
    # the existing classes: a K = 0 registration (explicit, or none given) is what it always was
    for cls, params, hip in ((contrib.DirectionalLightShader, ("light_direction", "albedo", "ambient"), contrib._DIRECTIONAL_HIP),
                             (contrib.DepthCueShader, ("density", "far_colour"), contrib._DEPTH_CUE_HIP)):
        before = shader_spec(cls())
        assert register_shader(cls, params=params, hip=hip) is cls and register_shader(cls, params=params, hip=hip, probes=0) is cls
        spec = shader_spec(cls())
        assert spec is before and spec.probes == 0 and spec.sha1 == hashlib.sha1(hip.encode()).hexdigest() and spec.params == params
        with pytest.raises(ValueError, match="probes=1, but the source of"):
            register_shader(cls, params=params, hip=hip, probes=1)
    plain_cls = _fresh(False)
    assert shader_spec(register_shader(plain_cls, hip=plain("pz"))()).probes == 0
    # the messages of sources without probes stay word for word
    with pytest.raises(ValueError, match=r"exactly two device functions.*one NAME \(found fwd: \['novjp2'\], vjp: \[\]\)"):
        register_shader(_fresh(False), hip=FWD.replace("NAME", "novjp2"))
    with pytest.raises(ValueError, match=r"one NAME \(found fwd: \['mix_c'\], vjp: \['mix_d'\]\)"):
        register_shader(_fresh(False), hip=FWD.replace("NAME", "mix_c") + VJP.replace("NAME", "mix_d"))
    # contrib's two
    assert (shader_spec(ambient_occlusion()).probes, shader_spec(soft_shadow()).probes, shader_spec(UTapNormal()).probes) == (5, 8, 4)
    assert [k for k, _ in ambient_occlusion().named_parameters()] == ["reach", "strength", "albedo"]
    assert [k for k, _ in soft_shadow().named_parameters()] == ["light_direction", "albedo", "ambient", "sharpness", "reach", "bias"]
    assert [k for k, _ in _trainable(soft_shadow())] == ["light_direction", "albedo", "ambient", "sharpness", "reach"]


def test_header_of_a_probing_shader():
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    _register()
    assert _abi.ABI_VERSION == 14
    scene = _scenes()["scene2"]()
    base = compiled_for(scene)
    cs = compiled_with_shader(scene, ambient_occlusion())
    assert cs.user_shader_probes == 5 and base.user_shader_probes == 0
    assert cs.user_shader == ("ambient_occlusion", 5, hashlib.sha1(contrib._AMBIENT_OCCLUSION_HIP.encode()).hexdigest())   # still the 3-tuple
    assert len(cs.signature) == 11 and cs.signature[9] == cs.user_shader and cs.signature[10] == ("probes", 5)
    hdr = specialize.code_header(cs)
    assert "#define RM_USER_SHADER 1\n" in hdr and "#define RM_USER_SHADER_PROBES 5\n" in hdr and "#define RM_USER_SHADER_PARAMS 5\n" in hdr
    assert contrib._AMBIENT_OCCLUSION_HIP.strip() in hdr
    for forwarder in ("template <bool Fast> RM_DEV V3 user_shader_probe(int k, const ShadeIn& s, const float* theta) {\n"
                      "  return ambient_occlusion_probe<Fast>(k, s, theta);",
                      "template <bool Fast> RM_DEV void user_shader_probe_vjp(int k, const ShadeIn& s, const float* theta, V3 gq, ShadeGrad& gs, "
                      "float* gtheta) {\n  ambient_occlusion_probe_vjp<Fast>(k, s, theta, gq, gs, gtheta);",
                      "template <bool Fast> RM_DEV V3 user_shader_fwd(const ShadeIn& s, const float* theta, const float* d) {\n"
                      "  return ambient_occlusion_fwd<Fast>(s, theta, d);",
                      "template <bool Fast> RM_DEV void user_shader_vjp(const ShadeIn& s, const float* theta, const float* d, V3 g, ShadeGrad& gs, "
                      "float* gtheta, float* gd) {\n  ambient_occlusion_vjp<Fast>(s, theta, d, g, gs, gtheta, gd);"):
        assert hdr.count(forwarder) == 1, forwarder
    assert hdr.index("RM_USER_SHADER_PROBES") < hdr.index("#elif defined(RM_STATIC_CODE_LEAVES)") < hdr.index("struct RmStaticCode")
    shadow = compiled_with_shader(scene, soft_shadow())
    assert shadow.user_shader_probes == 8 and "#define RM_USER_SHADER_PROBES 8\n" in specialize.code_header(shadow)
    assert shadow.n_params == base.n_params + 10
    # K reaches the library hash: the same source under another K is another header and another library
    other = specialize.scene_hash(cs)
    import dataclasses
    assert specialize.scene_hash(dataclasses.replace(cs, signature=cs.signature[:10] + (("probes", 4),))) != other
    assert len({specialize.scene_hash(x) for x in (base, cs, shadow, compiled_with_shader(scene, directional()))}) == 4
    assert specialize.user_names(cs) == ("ambient_occlusion", "shaders")


# recorded at the parent commit (the one before scene probes existed) for make_test_scene2() + DirectionalLightShader: sha1 of
# specialize.code_header, sha1 of repr(signature), and specialize.scene_hash with the kernel-source hash held at "parent"
PARENT = {"header": "24e5a9549d00bd46a83baf19bcfe0e56514f78f9", "signature": "9b00658aa44148d305d6980b3e959c288ebb1d20",
          "scene_hash": "d709265ece5e9001"}


def test_header_of_a_probe_free_shader_and_of_a_scene_alone_are_unchanged(monkeypatch):
    from ray_marching_amd import specialize
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    sha = lambda text: hashlib.sha1(text.encode()).hexdigest()
    scene = _scenes()["scene2"]()
    cs = compiled_with_shader(scene, directional())
    hdr = specialize.code_header(cs)
    assert cs.user_shader_probes == 0 and len(cs.signature) == 10 and "PROBES" not in hdr and "_probe" not in hdr
    assert sha(hdr) == PARENT["header"] and sha(repr(cs.signature)) == PARENT["signature"]
    monkeypatch.setattr(specialize, "_src_hash", "parent")
    assert specialize.scene_hash(cs) == PARENT["scene_hash"]
    monkeypatch.undo()
    # the scene alone: one guard around the program, nothing of shaders or probes
    base = compiled_for(scene)
    plain = specialize.code_header(base)
    rows = ",".join("{%d,%d,%d,%d}" % tuple(r) for r in base.program.tolist())
    assert plain == ("// generated by ray_marching_amd/specialize.py -- scene program as a compile-time constant\n"
                     "#ifndef RM_STATIC_CODE_LEAVES\nstruct RmStaticCode {\n"
                     f"  static constexpr int n = {base.n_instr}, n_params = {base.n_params}, n_derived = {base.n_derived},\n"
                     f"                       stack_floats = {base.stack_floats}, n_slots = {base.n_slots}, n_grad_derived = {base.n_grad_derived};\n"
                     f"  static constexpr rm::Ins code[{base.n_instr}] = {{{rows}}};\n}};\n#endif\n")
    assert sha(repr(base.signature)) == "663383d9a93e783b836a2cfdf8291c3546ab9718" and base.user_shader_probes == 0


@pytest.mark.parametrize("which", sorted(CONTRIB))
def test_probing_library_cross_compiles_and_reports_its_shader(which, monkeypatch, tmp_path):
    from ray_marching_amd import _abi, specialize
    from ray_marching_amd.compiler import compile_scene
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    monkeypatch.setattr(specialize, "SPEC_DIR", str(tmp_path))
    specialize._loaded.clear()
    cs = compile_scene(_scenes()["scene2"](), CONTRIB[which]())
    path = specialize.build(cs)
    assert os.path.isfile(path) and os.path.dirname(path) == str(tmp_path)
    lib = cs.lib()
    assert lib is not _abi.lib and lib.rm_user_shaders() == 1 and lib.rm_abi_version() == _abi.ABI_VERSION == 14
    assert (lib.rm_user_leaves(), lib.rm_user_combinators(), lib.rm_user_warps()) == (0, 0, 0)
    assert cs.lib(True) is lib and cs.specialised
    specialize._loaded.clear()


@pytest.mark.parametrize("which", sorted(CONTRIB))
@pytest.mark.parametrize("leg", sorted(BACKWARD_LEGS))
def test_cpu_gradients_of_the_shader_parameters_are_not_small(which, leg):
    """The 1e-4 of the gradient contract is absolute: constructor values, poses and loss scale of the GPU legs are chosen so that
    every component of every trainable shader parameter's CPU gradient is at least 1e-2 (and finite), before and after the
    edit."""
    for edited in (False, True):
        grads = cpu_reference(which, leg, edited)[0]
        for name, g in grads.items():
            print(f"{which} {leg} edited={edited}: CPU grad {name} {g.tolist()}")
        for name, g in grads.items():
            assert bool(torch.isfinite(g).all()) and g.abs().min().item() >= 1e-2, (name, g)


@pytest.mark.parametrize("which", sorted(CONTRIB) + ["utap_normal"])
def test_stand_alone_cpu_call(which):
    """Called directly with a PyTorch scene as ``scene`` (a module around the oracle's evaluator: the product's own nodes have no
    CPU path by design), a probing shader is the user's PyTorch code: [..., 3], and it differentiates down to the scene's
    parameters, the inputs and its own."""
    class TorchScene(nn.Module):
        def __init__(self):
            super().__init__()
            self.spec = O.map_spec(O.scene_test2(), lambda x: nn.Parameter(x.clone()))
            self.leaves = nn.ParameterList([x for _, x in O.spec_parameters(self.spec)])

        def forward(self, points):
            return O.sdf_eval(self.spec, points)

    scene = TorchScene()
    shader = UTapNormal() if which == "utap_normal" else CONTRIB[which]()
    gen = torch.Generator().manual_seed(4)
    n = torch.nn.functional.normalize(torch.randn(2, 5, 7, 3, generator=gen), dim=-1).requires_grad_(True)
    v = torch.nn.functional.normalize(-n.detach() + 0.3 * torch.randn(2, 5, 7, 3, generator=gen), dim=-1)
    p = (0.9 * torch.randn(2, 5, 7, 3, generator=gen)).requires_grad_(True)
    out = shader(p + 3.0, None, None, v, p, n, scene)
    assert out.shape == (2, 5, 7, 3) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    out.sum().backward()
    assert p.grad is not None and float(p.grad.abs().max()) > 0
    assert any(x.grad is not None and float(x.grad.abs().max()) > 0 for x in scene.parameters())
    for name, x in _trainable(shader):
        assert x.grad is not None and bool(torch.isfinite(x.grad).all()), name
    # ... and equals the formula written out (ambient occlusion)
    if which == "ambient_occlusion":
        with torch.no_grad():
            occ = sum(2.0 ** -k * (shader.reach * (k + 1) / 5 - scene(p + shader.reach * (k + 1) / 5 * n)).clamp(min=0) for k in range(5)) / shader.reach
            want = shader.albedo * (-(v * n).sum(-1, keepdim=True)).clamp(0, 1) / (1 + shader.strength * occ)
        assert torch.allclose(out, want, atol=1e-6)


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scene2", "closed_scene1"])
def test_tap_normal_twin_is_bit_identical_with_the_builtin_normal_mode(which, monkeypatch):
    """UTapNormal takes the tetrahedron's four taps as its probes and restates normals_from_taps and the normal shader: the
    60x44x32 frame of two cameras (partial 8x8 wave tiles on both edges) is the bits of the built-in normal mode (mode 4)
    through the tile kernel and through the ray pools (regen=True).  Its scene-parameter and pose gradients at 32x32x16 run
    the same arithmetic in another accumulation order (the probes' scene VJPs ahead of the taps', which then add zeros):
    <= 1e-6.  Every ray is walked in place (no deferred-ray list: its atomically ordered partial sums are no function of the
    program)."""
    from ray_marching_amd import _abi, ops
    from ray_marching_amd.compiler import compiled_with_shader
    _register()
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)
    mode = _abi.MODES.index("normal")
    shader = UTapNormal()
    scene = _scenes()[which]().to(DEV)
    assert compiled_with_shader(scene, shader).lib().rm_user_shaders() == 1
    h, w, steps = 44, 60, 32
    q, t = two_cameras(-3.0 if which == "scene2" else -1.5)
    q, t = q.to(DEV), t.to(DEV)
    with torch.no_grad():
        for kw in (dict(), dict(regen=True)):
            loop = H.make_loop(scene, h, w, n=2, **kw)
            want = loop(q, t, mode, 1, steps)
            got = loop(q, t, shader, 1, steps)
            differ = int((got != want).sum())
            print(f"{which} {kw}: {differ} of {got.numel()} values differ from mode {mode}")
            assert got.shape == (2, h, w, 3) and got.dtype == torch.float32 and torch.equal(got, want), kw
    h, w, steps = 32, 32, 16
    target = torch.rand(2, h, w, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    grads = {}
    for key, m in (("builtin", mode), ("twin", shader)):
        loop = H.make_loop(scene, h, w, n=2)
        for x in scene.parameters():
            x.grad = None
        qg, tg = q.clone().requires_grad_(True), t.clone().requires_grad_(True)
        (loop(qg, tg, m, 1, steps) - target).pow(2).mean().backward()
        grads[key] = [x.grad.clone() for x in scene.parameters()] + [qg.grad, tg.grad]
    names = [n for n, _ in scene.named_parameters()] + ["orientations", "translations"]
    worst = 0.0
    for name, a, b in zip(names, grads["twin"], grads["builtin"]):
        e = (a - b).abs().max().item()
        worst = max(worst, e)
        print(f"{which}: grad {name} max|diff| {e:.3g} (|g| {b.abs().max().item():.3g})")
    assert worst <= 1e-6, worst
    assert any(float(g.abs().max()) > 0 for g in grads["builtin"])


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(CONTRIB))
def test_contrib_probing_shader_against_the_cpu(which, monkeypatch):
    """AmbientOcclusionShader / SoftShadowShader on scene 2 against the oracle with the shader's PyTorch forward as its shade():
    values of a 60x44x32 frame of two cameras <= 1e-5 (restated math mode of the oracle: host independent) through the tile
    kernel and the ray pools, gradients of the scene parameters, the pose and every trainable shader parameter <= 1e-4 against
    CPU autograd, at 32x32x16 with two cameras and at 40x24x32 from inside the torus, where rays are deferred (asserted).
    Then an in-place edit and a ``.data`` assignment of shader parameters: the next backward follows the new values."""
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
            for name, p in _trainable(shader):
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


@pytest.mark.gpu
def test_ambient_occlusion_on_a_float16_module(monkeypatch):
    """a module cast with .to(float16) stores fp16 and computes in fp32, so its 40x24x32 frame is the fp32
    oracle evaluated on the fp16-rounded inputs (camera buffers, tetrahedron constants, scene parameters, pose), rounded once
    to fp16.  The shader's parameters are fp16-representable values.  Bit for bit."""
    h, w, steps = 24, 40, 32
    r = lambda x: x.half().float()
    spec = O.scene_test2()
    loop = H.make_loop(H.spec_to_module(spec), h, w).to(torch.float16)
    shader = ambient_occlusion()
    with torch.no_grad():
        for p in shader.parameters():
            p.copy_(r(p))
    q, t = two_cameras()
    q, t = q[:1].half(), t[:1].half()
    bufs = tuple(r(b) for b in _bufs(1, h, w))
    tetra = tuple(r(c) for c in O.tetra_constants(H.EPS))
    with torch.no_grad(), O.math_mode("restated"):
        want = cpu_frame(O.map_spec(spec, r), shader, monkeypatch, bufs, q.float(), t.float(), steps, tetra=tetra).half()
    with torch.no_grad():
        got = loop(q.to(DEV), t.to(DEV), ambient_occlusion_like(shader).to(DEV), 1, steps).cpu()
    assert got.dtype == torch.float16 and got.shape == (1, h, w, 3)
    ulps = (got.view(torch.int16).int() - want.view(torch.int16).int()).abs()
    print(f"fp16 AO frame: {int((ulps > 0).sum())} of {ulps.numel()} values differ, max {int(ulps.max())} fp16 ulp")
    assert torch.equal(got, want)


def ambient_occlusion_like(shader):
    """A fresh AmbientOcclusionShader with the parameter values of ``shader``."""
    out = ambient_occlusion()
    with torch.no_grad():
        for a, b in zip(out.parameters(), shader.parameters()):
            a.copy_(b)
    return out


@pytest.mark.gpu
def test_captured_frame_of_a_probing_shader_replays_the_eager_frame():
    h, w, steps = 44, 60, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    scene, shader = _scenes()["scene2"]().to(DEV), ambient_occlusion().to(DEV)
    loop = H.make_loop(scene, h, w, n=2)
    with torch.no_grad():
        eager = loop(q, t, shader, 1, steps).clone()
        frame = loop.capture(shader, 1, steps)
        for replay in range(2):
            assert torch.equal(frame(q, t), eager), replay
    assert float(eager.max()) > 0.1


@pytest.mark.gpu
def test_training_step_moves_a_perturbed_ambient_occlusion_back():
    """Twenty Adam steps of a captured training step on ``reach`` and ``strength`` of an AmbientOcclusionShader, towards a frame
    of scene 2 rendered with the unperturbed shader: both end nearer the values the target was rendered with, and the loss
    decreases."""
    h, w, steps = 32, 32, 16
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    truth = ambient_occlusion()
    with torch.no_grad():
        target = H.make_loop(_scenes()["scene2"]().to(DEV), h, w, n=2)(q, t, ambient_occlusion().to(DEV), 1, steps).clone()
    loss_fn = lambda image: (image - target).pow(2).mean()
    shader = ambient_occlusion().to(DEV)
    with torch.no_grad():
        shader.reach += 0.15
        shader.strength -= 0.8
    distance = lambda: (abs(float(shader.reach.detach()) - float(truth.reach.detach())),
                        abs(float(shader.strength.detach()) - float(truth.strength.detach())))
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*AccumulateGrad node's stream does not match.*")
        scene = _scenes()["scene2"]().to(DEV)
        for x in scene.parameters():
            x.requires_grad_(False)
        loop = H.make_loop(scene, h, w, n=2)
        before = distance()
        opt = torch.optim.Adam([shader.reach, shader.strength], lr=2e-2, capturable=True)
        step = loop.training_step(loss_fn, mode=shader, marching_steps=steps, optimizer=opt)
        with torch.no_grad():
            first = float(loss_fn(loop(q, t, shader, 1, steps)))
        losses = [float(step(q, t)) for _ in range(20)]
        with torch.no_grad():
            last = float(loss_fn(loop(q, t, shader, 1, steps)))
    after = distance()
    print(f"training leg: loss before {first:.6g}, per step {[round(x, 7) for x in losses]}, after {last:.6g}; "
          f"(reach, strength) distance to the target's {before} -> {after}")
    assert after[0] < before[0] and after[1] < before[1]
    assert last < first and losses[-1] < losses[0]


@pytest.mark.gpu
def test_ambient_occlusion_on_a_scene_with_user_nodes(monkeypatch):
    """contrib.make_warped_scene() (user warps and a user combinator) shaded by AmbientOcclusionShader: the probes run through
    the user nodes' HIP code.  Values <= 1e-5 against the CPU, whose scene is the PyTorch forwards of the nodes."""
    from ray_marching_amd import contrib
    from ray_marching_amd.compiler import compiled_with_shader
    from tests.test_user_warp import cpu_eval, spec_of
    scene = contrib.make_warped_scene()
    spec = spec_of(scene)
    scene = scene.to(DEV)
    shader, cpu_shader = ambient_occlusion().to(DEV), ambient_occlusion()
    lib = compiled_with_shader(scene, shader).lib()
    assert lib.rm_user_warps() == 4 and (lib.rm_user_shaders(), lib.rm_user_combinators(), lib.rm_user_leaves()) == (1, 1, 0)
    h, w, steps = 44, 60, 32
    q, t = two_cameras()
    with torch.no_grad():
        want = cpu_frame(spec, cpu_shader, monkeypatch, _bufs(2, h, w), q, t, steps, sdf_eval=cpu_eval)
        got = H.make_loop(scene, h, w, n=2)(q.to(DEV), t.to(DEV), shader, 1, steps).cpu()
    err, frac = H.report("warped frame", got, want)
    print(f"warped scene + ambient occlusion: frame max|err| {err:.3g}, {frac:.3g} of the values beyond 1e-5")
    assert err <= 1e-5


@pytest.mark.gpu
def test_probing_shader_probe_free_shader_and_a_builtin_mode_in_alternation_on_one_loop():
    """One scene, one RenderLoop; AmbientOcclusionShader, DirectionalLightShader and mode 0 in turn, twice: three libraries,
    and each frame is the bits of its own render on a fresh loop."""
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    h, w, steps = 44, 60, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    make = {"ambient_occlusion": ambient_occlusion, "directional": directional}
    modes = {"ambient_occlusion": ambient_occlusion().to(DEV), "directional": directional().to(DEV), "lambertian": 0}
    with torch.no_grad():
        want = {k: H.make_loop(_scenes()["scene2"]().to(DEV), h, w, n=2)(q, t, make[k]().to(DEV) if k in make else m, 1, steps).clone()
                for k, m in modes.items()}
        scene = _scenes()["scene2"]().to(DEV)
        loop = H.make_loop(scene, h, w, n=2)
        for rnd in range(2):
            for k, m in modes.items():
                assert _same(loop(q, t, m, 1, steps), want[k].expand(2, h, w, 3)), (rnd, k)
    assert not _same(want["ambient_occlusion"], want["directional"])
    base = compiled_for(scene)
    a, b = compiled_with_shader(scene, modes["ambient_occlusion"]), compiled_with_shader(scene, modes["directional"])
    libs = [base.lib(), a.lib(), b.lib()]
    assert len({id(x) for x in libs}) == 3 and [x.rm_user_shaders() for x in libs] == [0, 1, 1]
    assert (a.user_shader_probes, b.user_shader_probes, base.user_shader_probes) == (5, 0, 0)
