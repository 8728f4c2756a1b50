"""Chained scene probes (extensions.register_shader(..., probes=K, chained=True)): probe k is placed from the values the scene
returned at the probes before it, handed to NAME_probe / NAME_probe_vjp as the history ``h`` / ``gh``.

Without a GPU: the registration errors, the header and signature of a chained shader, the headers and signatures of scene 2
alone and with the three shipped shaders that must not move (sha1s recorded at the parent commit), the cross-compile of the two
chained libraries, the compiler's resource remarks (profiles/user_shader_chained_probes_resource_usage.txt: no scratch), the size
of the CPU gradients the GPU legs are held against, and the guard of the chain test (dropping the chain term is visible).

On the GPU: UChain2, the chain term at its smallest (K = 2); SoftShadowShader's source registered as a chained shader that ignores
its history (every bit of the frame); contrib.MarchedShadowShader against the oracle with its PyTorch forward as shade() (frame
<= 1e-5, gradients <= max(1e-4, 4 E_ref) with E_ref = |autograd32 - autograd64| of the oracle alone); a float16 module, a captured
replay, a captured training step, and three libraries in alternation on one loop.

The CPU side of a frame is tests.test_user_shader_probes.cpu_frame, as for the flat probing shaders."""
import functools
import hashlib
import os
import re
import warnings

import pytest
import torch
import torch.nn as nn

from oracle import sdf_oracle as O
from tests import helpers as H
from tests.helpers import _same
from tests.test_user_shader_probes import BACKWARD_LEGS, _bufs, _loss, _weights, cpu_frame, inside_the_torus, two_cameras  # noqa: F401

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------------------
# the shaders
# --------------------------------------------------------------------------------------------------------------
class UChain2(nn.Module):
    """The chain term at its smallest: q_0 = p + a n, q_1 = p + (a + d_0) n, rgb = d_1 n.  ``detach``: the forward with d_0 cut
    out of the graph, i.e. what a kernel that drops ``gh`` would differentiate (the guard of the GPU test)."""

    def __init__(self, a: float = 0.3, detach: bool = False) -> None:
        super().__init__()
        self.a = nn.Parameter(torch.tensor(a, dtype=torch.float32))
        self.detach = detach

    def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals, scene):
        d0 = scene(surface_coords + self.a * surface_normals)
        d1 = scene(surface_coords + (self.a + (d0.detach() if self.detach else d0)) * surface_normals)
        return d1 * surface_normals


# theta = {a}; h[0] is d_0 for probe 1 and exactly 0 for probe 0, so one expression places both
UCHAIN2_HIP = r"""
template <bool Fast> RM_DEV rm::V3 uchain2_probe(int k, const rm::ShadeIn& s, const float* theta, const float* h) {
  const float t = theta[0] + h[0];
  return mk3(s.p.x + t * s.n.x, s.p.y + t * s.n.y, s.p.z + t * s.n.z);
}
template <bool Fast> RM_DEV void uchain2_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, const float* h, rm::V3 gq,
                                                   rm::ShadeGrad& gs, float* gtheta, float* gh) {
  const float t = theta[0] + h[0];
  gs.p = gs.p + gq;
  gs.n = gs.n + t * gq;
  const float gt = dot_seq(gq, s.n);
  gtheta[0] += gt;
  gh[0] += gt;                  // (probe 0 has no history: what it adds here is ignored)
}
template <bool Fast> RM_DEV rm::V3 uchain2_fwd(const rm::ShadeIn& s, const float* theta, const float* d) {
  return mk3(d[1] * s.n.x, d[1] * s.n.y, d[1] * s.n.z);
}
template <bool Fast> RM_DEV void uchain2_vjp(const rm::ShadeIn& s, const float* theta, const float* d, rm::V3 g, rm::ShadeGrad& gs,
                                             float* gtheta, float* gd) {
  gs.n = gs.n + d[1] * g;
  gd[0] = 0.0f;
  gd[1] = dot_seq(g, s.n);
  gtheta[0] = 0.0f;
}
"""


def soft_shadow_chain_hip():
    """contrib's SoftShadowShader source under another identifier and with the chained signatures: ``h`` is ignored, ``gh`` left
    alone."""
    from ray_marching_amd import contrib
    src = contrib._SOFT_SHADOW_HIP.replace("soft_shadow_", "soft_shadow_chain_")
    probe = "_probe(int k, const rm::ShadeIn& s, const float* theta)"
    probe_vjp = re.compile(r"(_probe_vjp\(int k, const rm::ShadeIn& s, const float\* theta,) (rm::V3 gq, rm::ShadeGrad& gs,\s*float\* gtheta)\)")
    assert src.count(probe) == 1 and len(probe_vjp.findall(src)) == 1
    src = src.replace(probe, "_probe(int k, const rm::ShadeIn& s, const float* theta, const float* h)")
    return probe_vjp.sub(r"\1 const float* h, \2, float* gh)", src)


def _soft_shadow_chain_class():
    from ray_marching_amd.contrib import SoftShadowShader

    class SoftShadowChain(SoftShadowShader):
        pass
    return SoftShadowChain


@functools.lru_cache(maxsize=None)
def _register():
    """(UChain2, SoftShadowChain), registered once."""
    from ray_marching_amd.extensions import register_shader
    register_shader(UChain2, params=("a",), hip=UCHAIN2_HIP, probes=2, chained=True)
    chain = _soft_shadow_chain_class()
    register_shader(chain, params=("light_direction", "albedo", "ambient", "sharpness", "reach", "bias"), hip=soft_shadow_chain_hip(),
                    probes=8, chained=True)
    return UChain2, chain


SOFT_SHADOW = dict(light_direction=[0.35, 0.5, -0.8], albedo=[0.9, 0.55, 0.3], ambient=0.15, sharpness=2.0, reach=2.0, bias=0.02)


def soft_shadow():
    from ray_marching_amd.contrib import SoftShadowShader
    return SoftShadowShader(**SOFT_SHADOW)


def soft_shadow_chain():
    return _register()[1](**SOFT_SHADOW)


def marched_shadow():
    """The constructor values of every leg (sharpness = 2 keeps its gradient large enough for the absolute 1e-4)."""
    from ray_marching_amd.contrib import MarchedShadowShader
    return MarchedShadowShader(light_direction=(0.4, 0.5, -0.75), albedo=(1.0, 0.9, 0.8), ambient=0.15, sharpness=2.0, start=0.1,
                               step_min=0.02, step_max=0.5, bias=0.02)


def directional():
    from ray_marching_amd.contrib import DirectionalLightShader
    return DirectionalLightShader(light_direction=[0.35, 0.5, -0.8], albedo=[0.9, 0.55, 0.3], ambient=0.15)


def ambient_occlusion():
    from ray_marching_amd.contrib import AmbientOcclusionShader
    return AmbientOcclusionShader(reach=0.4, strength=2.0, albedo=[0.9, 0.6, 0.4])


def scene2():
    from ray_marching_amd.scene.scene_registry import make_test_scene2
    return make_test_scene2()


def gpu_test_programs():
    """Every (scene, shader) program the GPU legs launch: build() compiles their libraries, so that a GPU run of the same tree
    finds them; where they are missing the library builds itself on first use."""
    from ray_marching_amd import specialize
    from ray_marching_amd.compiler import compile_scene
    _register()
    out = [compile_scene(scene2(), make()) for make in (UChain2, soft_shadow_chain, soft_shadow, marched_shadow)]
    return list({specialize.scene_hash(cs): cs for cs in out}.values())


def _trainable(shader):
    return [(n, p) for n, p in shader.named_parameters() if p.requires_grad]


def _edit(shader):
    """An in-place edit and a ``.data`` assignment of shader parameters (the same on the CPU and the GPU copy)."""
    first, last = _trainable(shader)[0][1], _trainable(shader)[-1][1]
    with torch.no_grad():
        first.mul_(0.75)
    last.data = (last.detach() * 1.25 + 0.05).clone()


MAKERS = {"marched_shadow": marched_shadow, "soft_shadow": soft_shadow, "uchain2": UChain2,
          "uchain2_detached": lambda: UChain2(detach=True)}


@functools.lru_cache(maxsize=None)
def cpu_reference(which, leg, edited=False, dtype=torch.float32):
    """CPU autograd of one backward leg on scene 2 in ``dtype``, computed once per (shader, leg, parameters) and never modified:
    (shader gradients by name, scene gradients in named_parameters() order, dL/dq, dL/dt)."""
    h, w, steps, pose = BACKWARD_LEGS[leg]
    shader = MAKERS[which]()
    if edited:
        _edit(shader)
    shader = shader.to(dtype)
    q, t = pose()
    q, t = q.to(dtype).requires_grad_(True), t.to(dtype).requires_grad_(True)
    spec = O.map_spec(O.scene_test2(), lambda x: x.to(dtype).clone().requires_grad_(True))
    mp = pytest.MonkeyPatch()
    try:
        img = cpu_frame(spec, shader, mp, tuple(b.to(dtype) for b in _bufs(q.shape[0], h, w)), q, t, steps)
    finally:
        mp.undo()
    _loss(img, _weights(q.shape[0], h, w, 7).to(dtype)).backward()
    zero = lambda p: p.grad if p.grad is not None else torch.zeros_like(p)
    return ({n: p.grad.clone() for n, p in _trainable(shader)}, [zero(p) for _, p in O.spec_parameters(spec)], q.grad, t.grad)


def _flat(ref):
    """[(name, tensor)] of a cpu_reference result, scene parameters by position."""
    shader, scene, q, t = ref
    return ([(f"shader.{n}", g) for n, g in shader.items()] + [(f"scene[{i}]", g) for i, g in enumerate(scene)]
            + [("orientations", q), ("translations", t)])


def gpu_gradients(scene, shader, leg, monkeypatch):
    """One backward of the leg on the GPU: ([(name, gradient)] in the order of _flat, scene-parameter names, rays deferred)."""
    from ray_marching_amd import ops
    h, w, steps, pose = BACKWARD_LEGS[leg]
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
    got = [(f"shader.{n}", p.grad.cpu()) for n, p in _trainable(shader)]
    got += [(f"scene[{i}]", p.grad.cpu() if p.grad is not None else torch.zeros_like(p).cpu()) for i, p in enumerate(scene.parameters())]
    got += [("orientations", qg.grad.cpu()), ("translations", tg.grad.cpu())]
    return got, [n for n, _ in scene.named_parameters()], deferred


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
PFWD = "template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta, const float* d) { return d[0] * s.n; }\n"
PVJP = ("template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, const float* d, rm::V3 g, rm::ShadeGrad& gs, "
        "float* gtheta, float* gd) { gs.n = gs.n + d[0] * g; gd[0] = dot_seq(g, s.n); }\n")
CPROBE = ("template <bool Fast> RM_DEV rm::V3 NAME_probe(int k, const rm::ShadeIn& s, const float* theta, const float* h) "
          "{ return s.p + (1.0f + h[0]) * s.n; }\n")
CPROBE_VJP = ("template <bool Fast> RM_DEV void NAME_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, const float* h, rm::V3 gq, "
              "rm::ShadeGrad& gs, float* gtheta, float* gh) { gs.p = gs.p + gq; gs.n = gs.n + (1.0f + h[0]) * gq; gh[0] += dot_seq(gq, s.n); }\n")
FWD = "template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta) { return s.n; }\n"
VJP = ("template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta) "
       "{ gs.n = gs.n + g; }\n")


def _fresh():
    class S(nn.Module):
        def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals, scene):
            return scene(surface_coords + surface_normals) * surface_normals
    return S


def test_registration_errors():
    from ray_marching_amd import contrib, extensions
    from ray_marching_amd.extensions import register_shader, shader_spec
    full = lambda name: (CPROBE + CPROBE_VJP + PFWD + PVJP).replace("NAME", name)
    # chained is a bool
    for bad in (1, 0, "yes", None, 2.0):
        with pytest.raises(ValueError, match="chained must be a bool"):
            register_shader(_fresh(), hip=full("ca"), probes=2, chained=bad)
    # a chain has at least two probes, and at most the cap
    with pytest.raises(ValueError, match=r"chained=True needs probes from 2 to RM_USER_SHADER_MAX_PROBES = 8.*not probes=1"):
        register_shader(_fresh(), hip=full("cb"), probes=1, chained=True)
    with pytest.raises(ValueError, match=r"chained=True needs probes from 2 to RM_USER_SHADER_MAX_PROBES = 8.*not probes=0"):
        register_shader(_fresh(), hip=(FWD + VJP).replace("NAME", "cb0"), probes=0, chained=True)
    with pytest.raises(ValueError, match=r"chained=True needs probes from 2"):
        register_shader(_fresh(), hip=(FWD + VJP).replace("NAME", "cb1"), chained=True)
    with pytest.raises(ValueError, match="probes must be an int from 0 to RM_USER_SHADER_MAX_PROBES = 8"):
        register_shader(_fresh(), hip=full("cc"), probes=9, chained=True)
    # the probe pair is still a pair, and still needed
    with pytest.raises(ValueError, match="probes=3, but the source of S defines no cd_probe / cd_probe_vjp"):
        register_shader(_fresh(), hip=(PFWD + PVJP).replace("NAME", "cd"), probes=3, chained=True)
    with pytest.raises(ValueError, match=r"both or neither \(found ce_probe: True, ce_probe_vjp: False\)"):
        register_shader(_fresh(), hip=(CPROBE + PFWD + PVJP).replace("NAME", "ce"), probes=2, chained=True)
    # a second registration: the same value is a no-op, the other value an error (chained is one of the fields that must repeat)
    cls = _fresh()
    assert register_shader(cls, hip=full("cf"), probes=2, chained=True) is cls and register_shader(cls, hip=full("cf"), probes=2, chained=True) is cls
    with pytest.raises(ValueError, match=r"already registered with different source or parameters.*chained=True before, chained=False now"):
        register_shader(cls, hip=full("cf"), probes=2)
    with pytest.raises(ValueError, match=r"already registered with different source or parameters.*chained=True before, chained=False now"):
        register_shader(cls, hip=full("cf"), probes=2, chained=False)
    with pytest.raises(ValueError, match=r"chained=False before, chained=True now"):
        register_shader(contrib.SoftShadowShader, params=("light_direction", "albedo", "ambient", "sharpness", "reach", "bias"),
                        hip=contrib._SOFT_SHADOW_HIP, probes=8, chained=True)
    assert "chained" in extensions._KINDS["shader"].same
    spec = shader_spec(cls())
    assert (spec.name, spec.probes, spec.chained) == ("cf", 2, True)
    for k in (2, 8):
        assert shader_spec(register_shader(_fresh(), hip=full(f"ck{k}"), probes=k, chained=True)()).chained is True
    # the existing classes are flat, whether chained is left out or given as False
    for make in (soft_shadow, ambient_occlusion, directional):
        assert shader_spec(make()).chained is False
    assert register_shader(contrib.SoftShadowShader, params=("light_direction", "albedo", "ambient", "sharpness", "reach", "bias"),
                           hip=contrib._SOFT_SHADOW_HIP, probes=8, chained=False) is contrib.SoftShadowShader
    # the shipped chained shader and the two of this file
    _register()
    spec = shader_spec(marched_shadow())
    assert (spec.name, spec.probes, spec.chained) == ("marched_shadow", 8, True)
    assert spec.params == ("light_direction", "albedo", "ambient", "sharpness", "start", "bias", "step_min", "step_max")
    assert [k for k, _ in marched_shadow().named_parameters()] == list(spec.params)
    assert [k for k, _ in _trainable(marched_shadow())] == ["light_direction", "albedo", "ambient", "sharpness", "start"]
    assert (shader_spec(UChain2()).probes, shader_spec(UChain2()).chained) == (2, True)
    chain = shader_spec(soft_shadow_chain())
    assert (chain.name, chain.probes, chain.chained) == ("soft_shadow_chain", 8, True) and shader_spec(soft_shadow()).name == "soft_shadow"


def test_header_of_a_chained_shader():
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    _register()
    assert _abi.ABI_VERSION == 14
    scene = scene2()
    base = compiled_for(scene)
    cs = compiled_with_shader(scene, marched_shadow())
    assert cs.user_shader_chained is True and cs.user_shader_probes == 8 and base.user_shader_chained is False
    assert cs.user_shader == ("marched_shadow", 12, hashlib.sha1(contrib._MARCHED_SHADOW_HIP.encode()).hexdigest())
    assert len(cs.signature) == 12 and cs.signature[9] == cs.user_shader and cs.signature[10] == ("probes", 8) and cs.signature[11] == ("chained",)
    assert cs.n_params == base.n_params + 12
    hdr = specialize.code_header(cs)
    for line in ("#define RM_USER_SHADER 1\n", "#define RM_USER_SHADER_PROBES 8\n", "#define RM_USER_SHADER_PROBES_CHAINED 1\n",
                 "#define RM_USER_SHADER_PARAMS 12\n"):
        assert hdr.count(line) == 1, line
    assert contrib._MARCHED_SHADOW_HIP.strip() in hdr
    for forwarder in ("template <bool Fast> RM_DEV V3 user_shader_probe(int k, const ShadeIn& s, const float* theta, const float* h) {\n"
                      "  return marched_shadow_probe<Fast>(k, s, theta, h);",
                      "template <bool Fast> RM_DEV void user_shader_probe_vjp(int k, const ShadeIn& s, const float* theta, const float* h, V3 gq, "
                      "ShadeGrad& gs, float* gtheta, float* gh) {\n  marched_shadow_probe_vjp<Fast>(k, s, theta, h, gq, gs, gtheta, gh);",
                      "template <bool Fast> RM_DEV V3 user_shader_fwd(const ShadeIn& s, const float* theta, const float* d) {\n"
                      "  return marched_shadow_fwd<Fast>(s, theta, d);",
                      "template <bool Fast> RM_DEV void user_shader_vjp(const ShadeIn& s, const float* theta, const float* d, V3 g, ShadeGrad& gs, "
                      "float* gtheta, float* gd) {\n  marched_shadow_vjp<Fast>(s, theta, d, g, gs, gtheta, gd);"):
        assert hdr.count(forwarder) == 1, forwarder
    assert hdr.index("RM_USER_SHADER_PROBES 8") < hdr.index("RM_USER_SHADER_PROBES_CHAINED") < hdr.index("#elif defined(RM_STATIC_CODE_LEAVES)")
    # the same source, flat and chained, are two headers and two libraries; the flat one says nothing of chains
    flat, chain = compiled_with_shader(scene, soft_shadow()), compiled_with_shader(scene, soft_shadow_chain())
    assert (flat.user_shader_chained, chain.user_shader_chained) == (False, True) and len(flat.signature) == 11 and len(chain.signature) == 12
    assert "CHAINED" not in specialize.code_header(flat) and "const float* h" not in specialize.code_header(flat)
    assert len({specialize.scene_hash(x) for x in (base, cs, flat, chain, compiled_with_shader(scene, UChain2()))}) == 5
    assert len({specialize.lib_path(x) for x in (base, cs, flat, chain)}) == 4
    import dataclasses
    assert specialize.scene_hash(dataclasses.replace(chain, signature=chain.signature[:11])) != specialize.scene_hash(chain)
    assert specialize.user_names(cs) == ("marched_shadow", "shaders")


# recorded at the parent commit (the one before chained probes existed) for make_test_scene2() alone and with the three shipped
# shaders as constructed above: sha1 of specialize.code_header, sha1 of repr(signature)
PARENT = {"scene2": ("e4e5ef0668783b70987df1014d07c501d0234054", "663383d9a93e783b836a2cfdf8291c3546ab9718"),
          "directional": ("24e5a9549d00bd46a83baf19bcfe0e56514f78f9", "9b00658aa44148d305d6980b3e959c288ebb1d20"),
          "ambient_occlusion": ("2168405dc1f746a9e5da2a39d1abb8bb61fd0082", "5eb601f6e157dab06f37f8ec4d022fdfc3b50b8e"),
          "soft_shadow": ("c02176ea850b7875a95d3a074b0c202ab94f9281", "177a043fd2131123c6edfc1a2fbc5d6e074025f8")}


@pytest.mark.parametrize("which", sorted(PARENT))
def test_headers_and_signatures_of_flat_programs_are_unchanged(which):
    from ray_marching_amd import specialize
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    sha = lambda text: hashlib.sha1(text.encode()).hexdigest()
    make = {"directional": directional, "ambient_occlusion": ambient_occlusion, "soft_shadow": soft_shadow}
    cs = compiled_for(scene2()) if which == "scene2" else compiled_with_shader(scene2(), make[which]())
    hdr = specialize.code_header(cs)
    assert cs.user_shader_chained is False and "CHAINED" not in hdr and not any(slot == ("chained",) for slot in cs.signature[6:])
    assert (sha(hdr), sha(repr(cs.signature))) == PARENT[which]


@pytest.mark.parametrize("which", ["marched_shadow", "uchain2"])
def test_chained_library_cross_compiles_and_reports_its_shader(which, monkeypatch, tmp_path):
    from ray_marching_amd import _abi, specialize
    from ray_marching_amd.compiler import compile_scene
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    _register()
    monkeypatch.setattr(specialize, "SPEC_DIR", str(tmp_path))
    specialize._loaded.clear()
    cs = compile_scene(scene2(), MAKERS[which]())
    path = specialize.build(cs)
    assert os.path.isfile(path) and os.path.dirname(path) == str(tmp_path)
    lib = cs.lib()
    assert lib is not _abi.lib and lib.rm_user_shaders() == 1 and lib.rm_abi_version() == _abi.ABI_VERSION == 14
    assert (lib.rm_user_leaves(), lib.rm_user_combinators(), lib.rm_user_warps()) == (0, 0, 0)
    assert cs.lib(True) is lib and cs.specialised
    specialize._loaded.clear()


def test_no_frame_kernel_of_the_marched_shadow_library_has_scratch_of_its_own():
    """profiles/user_shader_chained_probes_resource_usage.txt (hipcc's kernel-resource remarks, scene 2): every frame kernel of the
    MarchedShadowShader library is listed next to the DirectionalLightShader library's and uses no more scratch than it."""
    rows = {}
    with open(os.path.join(ROOT, "profiles", "user_shader_chained_probes_resource_usage.txt")) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            words = line.split()            # library, the kernel's name (may hold blanks), seven numbers
            assert len(words) >= 9 and all(x.isdigit() for x in words[-7:]), line
            rows.setdefault(words[0], {})[" ".join(words[1:-7])] = dict(zip(("vgpr", "agpr", "sgpr", "spill_s", "spill_v", "scratch", "occ"),
                                                                            map(int, words[-7:])))
    assert {"directional", "soft_shadow", "marched_shadow"} <= set(rows)
    kernels = set(rows["marched_shadow"])
    assert kernels == set(rows["directional"]) == set(rows["soft_shadow"])
    for family in ("k_render_fwd", "k_render_finish", "k_render_parked", "k_render_bwd<S64, 4>", "k_bwd_hard_a"):
        assert any(k.startswith(family) for k in kernels), family
    for kernel in sorted(kernels):
        a, b = rows["marched_shadow"][kernel], rows["directional"][kernel]
        assert a["scratch"] <= b["scratch"] and a["spill_v"] <= b["spill_v"], (kernel, a, b)
    bwd = rows["marched_shadow"]["k_render_bwd<S64, 4>"]
    print(f"k_render_bwd<.., 4>: marched shadow {bwd['vgpr']} VGPRs / {bwd['occ']} waves per SIMD, soft shadow "
          f"{rows['soft_shadow']['k_render_bwd<S64, 4>']['vgpr']} / {rows['soft_shadow']['k_render_bwd<S64, 4>']['occ']}")


@pytest.mark.parametrize("leg", sorted(BACKWARD_LEGS))
def test_cpu_gradients_of_the_marched_shadow_parameters_are_not_small(leg):
    """The 1e-4 floor of the gradient contract is absolute: every component of every trainable shader parameter's CPU gradient is
    at least 1e-2 (and finite) with the constructor values of marched_shadow(), before and after the edit."""
    for edited in (False, True):
        grads = cpu_reference("marched_shadow", leg, edited)[0]
        for name, g in grads.items():
            print(f"marched_shadow {leg} edited={edited}: CPU grad {name} {g.tolist()}")
        assert sorted(grads) == ["albedo", "ambient", "light_direction", "sharpness", "start"]
        for name, g in grads.items():
            assert bool(torch.isfinite(g).all()) and g.abs().min().item() >= 1e-2, (name, g)


CHAIN_LEG = "32x32x16"


def test_dropping_the_chain_term_is_visible_in_the_cpu_gradients():
    """The guard of test_chain_of_two_probes_against_the_cpu: with d_0 detached inside the forward -- what a kernel that drops gh
    computes -- the gradient of ``a`` and of at least one scene parameter is off by >= 1e-2, a hundred times the test's bound."""
    true, cut = cpu_reference("uchain2", CHAIN_LEG), cpu_reference("uchain2_detached", CHAIN_LEG)
    ea = (true[0]["a"] - cut[0]["a"]).abs().max().item()
    es = [(x - y).abs().max().item() for x, y in zip(true[1], cut[1])]
    print(f"chain guard: |grad a - grad a (d_0 detached)| = {ea:.3g} (grad a {true[0]['a'].item():.4g}); scene parameters {[round(e, 4) for e in es]}")
    assert ea >= 1e-2 and max(es) >= 1e-2


def test_stand_alone_cpu_call_of_the_marched_shadow():
    """Called directly with a PyTorch scene, the shader is the user's PyTorch code: [..., 3], differentiable down to the scene's
    parameters, the inputs and its own; and it is the formula of its docstring written out."""
    class TorchScene(nn.Module):
        def __init__(self):
            super().__init__()
            self.spec = O.map_spec(O.scene_test2(), lambda x: nn.Parameter(x.clone()))
            self.leaves = nn.ParameterList([x for _, x in O.spec_parameters(self.spec)])

        def forward(self, points):
            return O.sdf_eval(self.spec, points)

    scene, shader = TorchScene(), marched_shadow()
    gen = torch.Generator().manual_seed(4)
    n = torch.nn.functional.normalize(torch.randn(2, 5, 7, 3, generator=gen), dim=-1).requires_grad_(True)
    p = (0.9 * torch.randn(2, 5, 7, 3, generator=gen)).requires_grad_(True)
    out = shader(p + 3.0, None, None, -n.detach(), p, n, scene)
    assert out.shape == (2, 5, 7, 3) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    out.sum().backward()
    assert p.grad is not None and float(p.grad.abs().max()) > 0
    assert any(x.grad is not None and float(x.grad.abs().max()) > 0 for x in scene.parameters())
    for name, x in shader.named_parameters():
        assert (x.grad is not None and bool(torch.isfinite(x.grad).all())) if x.requires_grad else x.grad is None, name
    with torch.no_grad():
        l = shader.light_direction / shader.light_direction.norm()
        o, t, shadow = p + shader.bias * n, shader.start.expand(2, 5, 7, 1), torch.ones(2, 5, 7, 1)
        for k in range(8):
            d = scene(o + t * l)
            shadow = torch.minimum(shadow, (shader.sharpness * d / t).clamp(0, 1))
            t = t + d.clamp(0.02, 0.5)
        want = shader.albedo * (shader.ambient + (1 - shader.ambient) * (n * l).sum(-1, keepdim=True).clamp(0, 1) * shadow)
    assert torch.allclose(out, want, atol=1e-6)


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chain_of_two_probes_against_the_cpu(monkeypatch):
    """UChain2 on scene 2, 32x32x16 with two cameras: frame <= 1e-5, gradients of ``a``, the scene parameters and the pose <= 1e-4
    against CPU autograd of its PyTorch forward.  All of dL/da's chain share reaches it through gh
    (test_dropping_the_chain_term_is_visible_in_the_cpu_gradients: a kernel that drops gh is off by >= 1e-2)."""
    from ray_marching_amd.compiler import compiled_with_shader
    _register()
    shader, scene = UChain2().to(DEV), scene2().to(DEV)
    cs = compiled_with_shader(scene, shader)
    assert cs.user_shader_chained and cs.lib().rm_user_shaders() == 1
    h, w, steps, pose = BACKWARD_LEGS[CHAIN_LEG]
    q, t = pose()
    with torch.no_grad(), O.math_mode("restated"):
        want = cpu_frame(O.scene_test2(), UChain2(), monkeypatch, _bufs(2, h, w), q, t, steps)
    with torch.no_grad():
        got = H.make_loop(scene, h, w, n=2)(q.to(DEV), t.to(DEV), shader, 1, steps).cpu()
    err, frac = H.report("uchain2 frame", got, want)
    print(f"uchain2: frame max|err| {err:.3g}, {frac:.3g} of the values beyond 1e-5")
    assert got.shape == (2, h, w, 3) and err <= 1e-5
    got, names, _ = gpu_gradients(scene, shader, CHAIN_LEG, monkeypatch)
    bad = []
    for (name, g), (_, c) in zip(got, _flat(cpu_reference("uchain2", CHAIN_LEG))):
        e = (g - c).abs().max().item()
        print(f"uchain2 {CHAIN_LEG}: grad {name} max|err| {e:.3g} (|g| {c.abs().max().item():.3g})")
        if not e <= 1e-4:
            bad.append(name)
    assert not bad, bad


@pytest.mark.gpu
def test_flat_shader_written_as_a_chained_one_changes_no_bit_of_the_frame(monkeypatch):
    """SoftShadowShader's source under another identifier, registered with chained=True (h ignored, gh left alone): its 60x44x32
    two-camera frame is SoftShadowShader's bit for bit, through the tile kernel and the ray pools.  Its gradients run the probes'
    scene VJPs in the other order (last probe first), so they are held to the oracle instead: max(1e-4, 4 E_ref) per tensor."""
    from ray_marching_amd.compiler import compiled_with_shader
    _register()
    scene = scene2().to(DEV)
    flat, chain = soft_shadow().to(DEV), soft_shadow_chain().to(DEV)
    assert compiled_with_shader(scene, chain).user_shader_chained and not compiled_with_shader(scene, flat).user_shader_chained
    assert compiled_with_shader(scene, chain).lib() is not compiled_with_shader(scene, flat).lib()
    h, w, steps = 44, 60, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    with torch.no_grad():
        for kw in (dict(), dict(regen=True)):
            loop = H.make_loop(scene, h, w, n=2, **kw)
            want = loop(q, t, flat, 1, steps).clone()
            got = loop(q, t, chain, 1, steps)
            print(f"{kw}: {int((got != want).sum())} of {got.numel()} values differ from SoftShadowShader's")
            assert got.shape == (2, h, w, 3) and torch.equal(got, want), kw
        assert float(want.max()) > 0.1
    for leg in BACKWARD_LEGS:
        _gradients_against_the_oracle("soft_shadow", scene, chain, leg, False, monkeypatch)


def _gradients_against_the_oracle(which, scene, shader, leg, edited, monkeypatch):
    """Every tensor of one backward leg: |gpu - autograd32| <= max(1e-4, 4 E_ref), E_ref = |autograd32 - autograd64| of the oracle
    alone.  (4: two fp32 evaluations of one function that sum in different orders can each sit E_ref from the fp64 value, and a
    factor 2 on top covers the device's wave-order reduction.)"""
    ref32, ref64 = _flat(cpu_reference(which, leg, edited)), _flat(cpu_reference(which, leg, edited, torch.float64))
    got, names, deferred = gpu_gradients(scene, shader, leg, monkeypatch)
    print(f"{which} {leg} edited={edited}: {deferred} rays deferred")
    if leg.startswith("deferred"):
        assert deferred > 0, "no ray was deferred: the leg does not exercise the deferred rule"
    assert [n for n, _ in got] == [n for n, _ in ref32]
    bad = []
    for (name, g), (_, c32), (_, c64) in zip(got, ref32, ref64):
        assert bool(torch.isfinite(g).all()), name
        e_ref = (c32.double() - c64).abs().max().item()
        e = (g - c32).abs().max().item()
        bound = max(1e-4, 4 * e_ref)
        print(f"{which} {leg} edited={edited}: grad {name} max|err| {e:.3g}, E_ref {e_ref:.3g}, bound {bound:.3g} (|g| {c32.abs().max().item():.3g})")
        if name.startswith("shader."):
            assert c32.abs().min().item() >= 1e-2, name
        if not e <= bound:
            bad.append(name)
    assert not bad, (which, leg, edited, bad)


@pytest.mark.gpu
def test_marched_shadow_against_the_cpu(monkeypatch):
    """MarchedShadowShader on scene 2 against the oracle with the shader's PyTorch forward as its shade(): the 60x44x32 frame of two
    cameras <= 1e-5 (restated math mode of the oracle) through the tile kernel and the ray pools; gradients of the scene parameters,
    the pose and every trainable shader parameter <= max(1e-4, 4 E_ref) at 32x32x16 with two cameras and at 40x24x32 from inside
    the torus, where rays are deferred (asserted).  Then an in-place edit and a ``.data`` assignment of shader parameters: the
    next backward follows the new values."""
    from ray_marching_amd.compiler import compiled_with_shader
    shader, cpu_shader = marched_shadow().to(DEV), marched_shadow()
    scene = scene2().to(DEV)
    cs = compiled_with_shader(scene, shader)
    assert cs.user_shader_chained and cs.lib().rm_user_shaders() == 1
    h, w, steps = 44, 60, 32
    q, t = two_cameras()
    with torch.no_grad(), O.math_mode("restated"):
        want = cpu_frame(O.scene_test2(), cpu_shader, monkeypatch, _bufs(2, h, w), q, t, steps)
    with torch.no_grad():
        for kw in (dict(), dict(regen=True)):
            got = H.make_loop(scene, h, w, n=2, **kw)(q.to(DEV), t.to(DEV), shader, 1, steps).cpu()
            err, frac = H.report("marched shadow frame", got, want)
            print(f"marched_shadow {kw}: frame max|err| {err:.3g}, {frac:.3g} of the values beyond 1e-5")
            assert got.shape == (2, h, w, 3) and err <= 1e-5
    assert float(want.max()) > 0.1 and float((want.max(dim=-1).values - want.min(dim=-1).values).max()) > 0
    for edited in (False, True):
        if edited:
            _edit(shader)
        for leg in BACKWARD_LEGS:
            _gradients_against_the_oracle("marched_shadow", scene, shader, leg, edited, monkeypatch)


def _like(make, shader):
    """A fresh shader with the parameter values of ``shader``."""
    out = make()
    with torch.no_grad():
        for a, b in zip(out.parameters(), shader.parameters()):
            a.copy_(b)
    return out


@pytest.mark.gpu
def test_marched_shadow_on_a_float16_module(monkeypatch):
    """a module cast with .to(float16) stores fp16 and computes in fp32, so its 40x24x32 frame is the fp32
    oracle evaluated on the fp16-rounded inputs (camera buffers, tetrahedron constants, scene parameters, pose), rounded once
    to fp16.  The shader's parameters are fp16-representable values.  Bit for bit."""
    h, w, steps = 24, 40, 32
    r = lambda x: x.half().float()
    spec = O.scene_test2()
    loop = H.make_loop(H.spec_to_module(spec), h, w).to(torch.float16)
    shader = marched_shadow()
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
        got = loop(q.to(DEV), t.to(DEV), _like(marched_shadow, shader).to(DEV), 1, steps).cpu()
    assert got.dtype == torch.float16 and got.shape == (1, h, w, 3)
    ulps = (got.view(torch.int16).int() - want.view(torch.int16).int()).abs()
    print(f"fp16 marched shadow frame: {int((ulps > 0).sum())} of {ulps.numel()} values differ, max {int(ulps.max())} fp16 ulp")
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_captured_frame_of_the_marched_shadow_replays_the_eager_frame():
    h, w, steps = 24, 40, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    scene, shader = scene2().to(DEV), marched_shadow().to(DEV)
    loop = H.make_loop(scene, h, w, n=2)
    with torch.no_grad():
        eager = loop(q, t, shader, 1, steps).clone()
        frame = loop.capture(shader, 1, steps)
        for replay in range(2):
            assert torch.equal(frame(q, t), eager), replay
    assert float(eager.max()) > 0.1


@pytest.mark.gpu
def test_training_step_moves_a_perturbed_marched_shadow_back():
    """Twenty Adam steps of a captured training step on ``start`` and ``sharpness`` of a MarchedShadowShader, towards a 40x24x32
    frame of scene 2 rendered with the unperturbed shader: both end nearer the values the target was rendered with, and the loss
    decreases.  (lr 2e-3: twenty steps move a parameter by at most 0.04, less than either perturbation.)"""
    h, w, steps = 24, 40, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    truth = marched_shadow()
    with torch.no_grad():
        target = H.make_loop(scene2().to(DEV), h, w, n=2)(q, t, marched_shadow().to(DEV), 1, steps).clone()
    loss_fn = lambda image: (image - target).pow(2).mean()
    shader = marched_shadow().to(DEV)
    with torch.no_grad():
        shader.start += TRAIN_PERTURBATION["start"]
        shader.sharpness += TRAIN_PERTURBATION["sharpness"]
    distance = lambda: (abs(float(shader.start.detach()) - float(truth.start.detach())),
                        abs(float(shader.sharpness.detach()) - float(truth.sharpness.detach())))
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*AccumulateGrad node's stream does not match.*")
        scene = scene2().to(DEV)
        for x in scene.parameters():
            x.requires_grad_(False)
        loop = H.make_loop(scene, h, w, n=2)
        before = distance()
        opt = torch.optim.Adam([shader.start, shader.sharpness], lr=TRAIN_LR, capturable=True)
        step = loop.training_step(loss_fn, mode=shader, marching_steps=steps, optimizer=opt)
        with torch.no_grad():
            first = float(loss_fn(loop(q, t, shader, 1, steps)))
        losses = [float(step(q, t)) for _ in range(20)]
        with torch.no_grad():
            last = float(loss_fn(loop(q, t, shader, 1, steps)))
    after = distance()
    print(f"training leg: loss before {first:.6g}, per step {[round(x, 7) for x in losses]}, after {last:.6g}; "
          f"(start, sharpness) distance to the target's {before} -> {after}")
    assert after[0] < before[0] and after[1] < before[1]
    assert last < first and losses[-1] < losses[0]


TRAIN_PERTURBATION = {"start": 0.06, "sharpness": -0.6}
TRAIN_LR = 2e-3


@pytest.mark.gpu
def test_chained_shader_flat_shader_and_a_builtin_mode_in_alternation_on_one_loop():
    """One scene, one RenderLoop at 40x24x32; MarchedShadowShader, SoftShadowShader and mode 0 in turn, twice: three libraries, and
    each frame is the bits of its own render on a fresh loop."""
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    h, w, steps = 24, 40, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    make = {"marched_shadow": marched_shadow, "soft_shadow": soft_shadow}
    modes = {"marched_shadow": marched_shadow().to(DEV), "soft_shadow": soft_shadow().to(DEV), "lambertian": 0}
    with torch.no_grad():
        want = {k: H.make_loop(scene2().to(DEV), h, w, n=2)(q, t, make[k]().to(DEV) if k in make else m, 1, steps).clone()
                for k, m in modes.items()}
        scene = scene2().to(DEV)
        loop = H.make_loop(scene, h, w, n=2)
        for rnd in range(2):
            for k, m in modes.items():
                assert _same(loop(q, t, m, 1, steps), want[k].expand(2, h, w, 3)), (rnd, k)
    assert not _same(want["marched_shadow"], want["soft_shadow"]) and not _same(want["soft_shadow"], want["lambertian"])
    base = compiled_for(scene)
    a, b = compiled_with_shader(scene, modes["marched_shadow"]), compiled_with_shader(scene, modes["soft_shadow"])
    libs = [base.lib(), a.lib(), b.lib()]
    assert len({id(x) for x in libs}) == 3 and [x.rm_user_shaders() for x in libs] == [0, 1, 1]
    assert (a.user_shader_chained, b.user_shader_chained, base.user_shader_chained) == (True, False, False)
