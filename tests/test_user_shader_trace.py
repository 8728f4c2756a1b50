"""Traced secondary rays (extensions.register_shader(..., trace=S)): the shader names one secondary ray per pixel (NAME_ray /
NAME_ray_vjp), the frame kernels sphere-trace it S steps through the scene and hand NAME_fwd / NAME_vjp the hit (end point, tetrahedral
normal, scene value); the backward recomputes the march into a checkpoint workspace and walks it in reverse.

Without a GPU: the registration errors, the header and signature of a tracing shader, the headers of six shipped shaders on scene
2 that must not move (sha1s recorded at the parent commit), the cross-compile of the three libraries (MirrorShader also in the
fast build) with their entry points, the compiler's resource remarks (profiles/user_shader_trace_resource_usage.txt), the CPU
contract of MirrorShader with reference_trace, the size of the CPU gradients, the guard (dropping the reverse secondary march is
visible) and the cap on the oracle's own error.

On the GPU: UTrace1 (S = 1), UTrace12 (S = 12) and contrib.MirrorShader (S = 24) against the oracle with the shader's PyTorch
forward as its shade() and reference_trace over the oracle's evaluator as its ``trace``: frames <= 1e-5 through the tile kernel and
the ray pools, gradients <= max(1e-4, 4 E_ref) with E_ref = |autograd32 - autograd64| of the oracle alone; two backwards of one
frame, a float16 module, a captured replay, a captured training step, three libraries in alternation on one loop, and the
workspace checks of rm_render_backward_trace.

The loss.  Every tensor is compared under the suite's loss, the weighted mean times 8 (LOSS_SCALE of test_user_shader_probes),
wherever the oracle alone meets the cap 4 E_ref <= 1e-3 there: every shader parameter, nearly every scene parameter, everything
of the 40x24x32 leg but its translations.  The tensors of ``REDUCED`` do not: the pose gradient of the 32x32x16 frame at
two_cameras() -- the pose the issue sets -- has 4 E_ref = 7e-3 to 1.3e-2 under the mirror and 4e-3 under DirectionalLightShader
already (silhouette pixels whose primary ray has not settled after 16 steps), and scene[4], the radius of the capsule, follows
it.  Gradients and E_ref are both linear in the scale of the loss, and a power of two scales them exactly, so each of those
tensors is compared in a further backward at the largest 8 / 2^k at which 4 E_ref <= 0.75e-3 (a quarter of headroom: E_ref
is itself a float32 sum whose order may differ from box to box); the figures are next to the table.  At that scale the
tensor's largest component is >= 0.1, a thousand times the bound's floor (asserted), and the guard holds (below).  The
37x21x16 gradient leg uses two_cameras(-4.0): of the poses two_cameras(z), z = -2.5 .. -5.5 in the room, it is the one where the
oracle's error is smallest (only dL/dq exceeds the cap at scale 8, 2.8e-3; at two_cameras() it is 5e-2).  Its frame is compared
at two_cameras().

The CPU side of a frame is tests.test_user_shader_probes.cpu_frame, as for the probing shaders; ``Traced`` hands the shader a
``trace`` built from the ``scene`` callable cpu_frame passes."""
import ctypes as C
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
from tests.test_user_shader_probes import BACKWARD_LEGS, _bufs, _weights, cpu_frame, inside_the_torus, two_cameras  # noqa: F401

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RM_E_BADARG = -1         # include/rm_abi.h
SUITE_SCALE = 8.0        # LOSS_SCALE of tests.test_user_shader_probes
# (shader, leg) -> {tensor: the loss scale it is compared at}; every tensor not named here is compared at SUITE_SCALE.  In brackets
# 4 E_ref of the oracle at SUITE_SCALE, which fixes the scale (module docstring): the largest 8 / 2^k with 4 E_ref <= 0.75e-3.
REDUCED = {("utrace1", "32x32x16"): {"scene[4]": 1.0, "orientations": 0.5, "translations": 1.0},     # [3.5e-3, 7.1e-3, 3.0e-3]
           ("utrace12", "32x32x16"): {"orientations": 4.0},                                         # [1.3e-3]
           ("mirror", "32x32x16"): {"scene[4]": 1.0, "orientations": 0.25, "translations": 1.0},    # [3.5e-3, 1.25e-2, 3.6e-3]
           ("mirror", "37x21x16"): {"orientations": 2.0},                                           # [2.8e-3]
           ("mirror", "deferred_40x24x32"): {"translations": 4.0}}                                  # [9.3e-4]


# --------------------------------------------------------------------------------------------------------------
# the shaders
# --------------------------------------------------------------------------------------------------------------
class UTrace12(nn.Module):
    """A ray that depends on theta and on p, n and v, a colour that reads all of the hit: o2 = p + a n, v2 = (1 - b) v + b n (not a
    unit vector), rgb = h.d h.n + h.p / 4."""

    def __init__(self, a: float = 0.05, b: float = 0.3) -> None:
        super().__init__()
        self.a = nn.Parameter(torch.tensor(a, dtype=torch.float32))
        self.b = nn.Parameter(torch.tensor(b, dtype=torch.float32))

    def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals, trace):
        points, normals, values = trace(surface_coords + self.a * surface_normals, (1 - self.b) * ray_directions + self.b * surface_normals)
        return values * normals + 0.25 * points


class UTrace1(UTrace12):
    """The same shader registered with trace=1: a loop of one step, checkpoint row 0 only."""


# theta = {a, b}
UTRACE_HIP = r"""
template <bool Fast> RM_DEV void NAME_ray(const rm::ShadeIn& s, const float* theta, rm::TraceRay& r) {
  const float a = theta[0], b = theta[1], c = 1.0f - theta[1];
  r.o = mk3(s.p.x + a * s.n.x, s.p.y + a * s.n.y, s.p.z + a * s.n.z);
  r.v = mk3(c * s.v.x + b * s.n.x, c * s.v.y + b * s.n.y, c * s.v.z + b * s.n.z);
}
template <bool Fast> RM_DEV void NAME_ray_vjp(const rm::ShadeIn& s, const float* theta, const rm::TraceRay& gr, rm::ShadeGrad& gs,
                                              float* gtheta) {
  const float a = theta[0], b = theta[1], c = 1.0f - theta[1];
  gs.p = gs.p + gr.o;
  gs.n = (gs.n + a * gr.o) + b * gr.v;
  gs.v = gs.v + c * gr.v;
  gtheta[0] += dot_seq(gr.o, s.n);
  gtheta[1] += dot_seq(gr.v, s.n) - dot_seq(gr.v, s.v);
}
template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta, const rm::TraceHit& h) {
  return mk3(h.d * h.n.x + 0.25f * h.p.x, h.d * h.n.y + 0.25f * h.p.y, h.d * h.n.z + 0.25f * h.p.z);
}
template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, const rm::TraceHit& h, rm::V3 g, rm::ShadeGrad& gs,
                                          float* gtheta, rm::TraceGrad& gh) {
  gh.d = dot_seq(g, h.n);
  gh.n = h.d * g;
  gh.p = 0.25f * g;
  gtheta[0] = 0.0f; gtheta[1] = 0.0f;
}
"""


@functools.lru_cache(maxsize=None)
def _register():
    from ray_marching_amd.extensions import register_shader
    register_shader(UTrace12, params=("a", "b"), hip=UTRACE_HIP.replace("NAME", "utrace12"), trace=12)
    register_shader(UTrace1, params=("a", "b"), hip=UTRACE_HIP.replace("NAME", "utrace1"), trace=1)
    return UTrace12, UTrace1


MIRROR = dict(reflectivity=0.7, light_direction=(-0.35, -0.5, 0.8), ambient=0.5, sky=(0.5, 0.6, 0.8), bias=1e-3, hit_eps=0.05)


def mirror():
    """The constructor values of every leg.  A closed room has no sky: the weight 1 - w is on the reflected rays that have not
    reached a surface after 24 steps, and a bias of 1e-3 leaves enough of them (they start 1e-3 from the surface they leave)
    for the gradient of ``sky`` to be above 1e-2; those rays are further than hit_eps from everything, so w is exactly 0 there."""
    from ray_marching_amd.contrib import MirrorShader
    return MirrorShader(**MIRROR)


def directional():
    from ray_marching_amd.contrib import DirectionalLightShader
    return DirectionalLightShader(light_direction=[0.35, 0.5, -0.8], albedo=[0.9, 0.55, 0.3], ambient=0.15)


def scene2():
    from ray_marching_amd.scene.scene_registry import make_test_scene2
    return make_test_scene2()


MAKERS = {"utrace1": UTrace1, "utrace12": UTrace12, "mirror": mirror}
STEPS = {"utrace1": 1, "utrace12": 12, "mirror": 24}


def gpu_test_programs():
    """Every (scene, shader) program the GPU legs launch: build() compiles their libraries, so that a GPU run of the same tree
    finds them; where they are missing the library builds itself on first use."""
    from ray_marching_amd import specialize
    from ray_marching_amd.compiler import compile_scene
    _register()
    out = [compile_scene(scene2(), make()) for make in (UTrace1, UTrace12, mirror, directional)]
    return list({specialize.scene_hash(cs): cs for cs in out}.values())


# --------------------------------------------------------------------------------------------------------------
# the CPU side
# --------------------------------------------------------------------------------------------------------------
class Traced:
    """What cpu_frame calls in the shader's place: the shader with ``trace = reference_trace(scene, steps, eps)`` built from the scene
    callable cpu_frame hands over.  ``constant_hit``: the hit detached, i.e. what a backward that drops the reverse secondary march
    -- h constant in the scene parameters and in the ray -- would differentiate (the guard of the GPU legs)."""

    def __init__(self, shader, steps, tetra=None, constant_hit=False):
        self.shader, self.steps, self.tetra, self.constant_hit = shader, steps, tetra, constant_hit

    def __call__(self, px, orientation, frames, dirs, p, n, scene):
        from ray_marching_amd.extensions import reference_trace
        trace = reference_trace(scene, self.steps, H.EPS, self.tetra)
        if self.constant_hit:
            inner = trace
            trace = lambda o, v: tuple(x.detach() for x in inner(o, v))
        return self.shader(px, orientation, frames, dirs, p, n, trace)


def far_cameras():
    return two_cameras(-4.0)


# (shader, shape) pairs of the GPU legs: the frame's (h, w, steps, pose) and the gradient leg's
FRAMES = {"32x32x16": (32, 32, 16, two_cameras), "37x21x16": (21, 37, 16, two_cameras), "deferred_40x24x32": (24, 40, 32, inside_the_torus)}
LEGS = {"32x32x16": BACKWARD_LEGS["32x32x16"], "37x21x16": (21, 37, 16, far_cameras), "deferred_40x24x32": BACKWARD_LEGS["deferred_40x24x32"]}
CASES = [("utrace1", "32x32x16"), ("utrace12", "32x32x16"), ("mirror", "32x32x16"), ("mirror", "37x21x16"), ("mirror", "deferred_40x24x32")]


def _loss(image, weights, scale):
    """The suite's weighted mean (test_user_shader_probes._loss) at a scale of the caller's (module docstring)."""
    return (image * weights).mean() * scale


def _trainable(shader):
    return [(n, p) for n, p in shader.named_parameters() if p.requires_grad]


@functools.lru_cache(maxsize=None)
def cpu_reference(which, leg, scale, dtype=torch.float32, constant_hit=False):
    """CPU autograd of one backward leg on scene 2 in ``dtype``, computed once and never modified: [(name, gradient)], the shader's
    trainable parameters, the scene's in named_parameters() order, the pose."""
    h, w, steps, pose = LEGS[leg]
    shader = MAKERS[which]().to(dtype)
    q, t = pose()
    q, t = q.to(dtype).requires_grad_(True), t.to(dtype).requires_grad_(True)
    spec = O.map_spec(O.scene_test2(), lambda x: x.to(dtype).clone().requires_grad_(True))
    mp = pytest.MonkeyPatch()
    try:
        img = cpu_frame(spec, Traced(shader, STEPS[which], constant_hit=constant_hit), mp, tuple(b.to(dtype) for b in _bufs(q.shape[0], h, w)),
                        q, t, steps)
    finally:
        mp.undo()
    if img.requires_grad:             # (UTrace's colour is a function of the hit alone: with the hit detached nothing is left)
        _loss(img, _weights(q.shape[0], h, w, 7).to(dtype), scale).backward()
    zero = lambda p: p.grad.clone() if p.grad is not None else torch.zeros_like(p)
    return ([(f"shader.{n}", zero(p)) for n, p in _trainable(shader)]
            + [(f"scene[{i}]", zero(p)) for i, (_, p) in enumerate(O.spec_parameters(spec))] + [("orientations", zero(q)), ("translations", zero(t))])


def scale_of(which, leg, name):
    """The loss scale at which a tensor of a leg is compared (module docstring)."""
    return REDUCED.get((which, leg), {}).get(name, SUITE_SCALE)


def scales(which, leg):
    """The loss scales of a leg's backwards, the suite's first."""
    return sorted({SUITE_SCALE, *REDUCED.get((which, leg), {}).values()}, reverse=True)


def compared(which, leg, name, scale):
    return scale_of(which, leg, name) == scale


def gpu_gradients(scene, shader, leg, scale, monkeypatch):
    """One backward of the leg on the GPU: ([(name, gradient)] in the order of cpu_reference, rays deferred)."""
    from ray_marching_amd import ops
    h, w, steps, pose = LEGS[leg]
    q, t = pose()
    n = q.shape[0]
    qg, tg = q.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
    for x in list(scene.parameters()) + list(shader.parameters()):
        x.grad = None
    sink = torch.zeros(int(ops._lib.rm_wave_tiles(n, h, w, 2)), dtype=torch.int32, device=DEV)
    monkeypatch.setattr(ops, "bwd_tile_cost_sink", sink)          # (measurement hook: keeps the backward's workspace)
    _loss(H.make_loop(scene, h, w, n=n)(qg, tg, shader, 1, steps), _weights(n, h, w, 7).to(DEV), scale).backward()
    torch.cuda.synchronize()
    deferred = int(ops.bwd_last_work[32])
    monkeypatch.setattr(ops, "bwd_tile_cost_sink", None)
    got = [(f"shader.{n}", p.grad.cpu()) for n, p in _trainable(shader)]
    got += [(f"scene[{i}]", p.grad.cpu() if p.grad is not None else torch.zeros_like(p).cpu()) for i, p in enumerate(scene.parameters())]
    got += [("orientations", qg.grad.cpu()), ("translations", tg.grad.cpu())]
    return got, deferred


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
RAY = "template <bool Fast> RM_DEV void NAME_ray(const rm::ShadeIn& s, const float* theta, rm::TraceRay& r) { r.o = s.p; r.v = s.n; }\n"
RAY_VJP = ("template <bool Fast> RM_DEV void NAME_ray_vjp(const rm::ShadeIn& s, const float* theta, const rm::TraceRay& gr, rm::ShadeGrad& gs, "
           "float* gtheta) { gs.p = gs.p + gr.o; gs.n = gs.n + gr.v; }\n")
TFWD = "template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta, const rm::TraceHit& h) { return h.n; }\n"
TVJP = ("template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, const rm::TraceHit& h, rm::V3 g, rm::ShadeGrad& gs, "
        "float* gtheta, rm::TraceGrad& gh) { gh.n = g; }\n")
FWD = "template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta) { return s.n; }\n"
VJP = ("template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta) "
       "{ gs.n = gs.n + g; }\n")


def _fresh():
    class S(nn.Module):
        def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals, trace):
            return trace(surface_coords, surface_normals)[1]
    return S


def test_registration_errors():
    from ray_marching_amd import contrib, extensions
    from ray_marching_amd.extensions import register_shader, shader_spec
    full = lambda name: (RAY + RAY_VJP + TFWD + TVJP).replace("NAME", name)
    assert extensions.RM_USER_SHADER_MAX_TRACE_STEPS == 64
    # the range of S
    for bad in (-1, 65, 1.0, "3", None, True):
        with pytest.raises(ValueError, match="trace must be an int from 1 to RM_USER_SHADER_MAX_TRACE_STEPS = 64"):
            register_shader(_fresh(), hip=full("ta"), trace=bad)
    # S = 0 is "no trace": a source that brings the ray pair says otherwise
    with pytest.raises(ValueError, match="defines tb_ray / tb_ray_vjp, but trace=0"):
        register_shader(_fresh(), hip=full("tb"), trace=0)
    with pytest.raises(ValueError, match="defines tb_ray / tb_ray_vjp, but trace=0"):
        register_shader(_fresh(), hip=full("tb"))
    # every refused combination, whatever the source looks like
    for other in (dict(probes=2), dict(probes=2, chained=True), dict(chained=True), dict(normalise="minmax"), dict(table="palette", table_taps=1),
                  dict(material=True)):
        with pytest.raises(ValueError, match=r"trace= together with probes > 0, chained=, normalise=, table= or material= is not built yet"):
            register_shader(_fresh(), hip=full("tc"), trace=4, **other)
    # the four functions
    with pytest.raises(ValueError, match="trace=4, but the source of S defines no td_ray / td_ray_vjp"):
        register_shader(_fresh(), hip=(TFWD + TVJP).replace("NAME", "td"), trace=4)
    with pytest.raises(ValueError, match="trace=4, but the source of S defines no te_ray_vjp "):
        register_shader(_fresh(), hip=(RAY + TFWD + TVJP).replace("NAME", "te"), trace=4)
    with pytest.raises(ValueError, match="trace=4, but the source of S defines no tf_ray "):
        register_shader(_fresh(), hip=(RAY_VJP + TFWD + TVJP).replace("NAME", "tf"), trace=4)
    with pytest.raises(ValueError, match=r"const rm::TraceHit& h.*found h: False, gh: False"):
        register_shader(_fresh(), hip=(RAY + RAY_VJP + FWD + VJP).replace("NAME", "tg"), trace=4)
    # a second registration: the same S is a no-op, another S an error
    cls = _fresh()
    assert register_shader(cls, hip=full("th"), trace=1) is cls and register_shader(cls, hip=full("th"), trace=1) is cls
    with pytest.raises(ValueError, match=r"already registered with different source or parameters.*trace=1 before, trace=2 now"):
        register_shader(cls, hip=full("th"), trace=2)
    assert "trace" in extensions._KINDS["shader"].same
    spec = shader_spec(cls())
    assert (spec.name, spec.trace, spec.probes, spec.chained, spec.material) == ("th", 1, 0, False, False)
    assert shader_spec(register_shader(_fresh(), hip=full("ti"), trace=64)()).trace == 64
    # the shipped classes trace nothing, the mirror 24 steps, the two of this file 12 and 1
    for make in (directional, contrib.DepthCueShader, contrib.MarchedShadowShader, contrib.MaterialLambertShader):
        assert shader_spec(make()).trace == 0
    _register()
    spec = shader_spec(mirror())
    assert (spec.name, spec.trace) == ("mirror", 24)
    assert spec.params == ("reflectivity", "light_direction", "ambient", "sky", "bias", "hit_eps") == tuple(k for k, _ in mirror().named_parameters())
    assert [k for k, _ in _trainable(mirror())] == ["reflectivity", "light_direction", "ambient", "sky"]
    assert (shader_spec(UTrace12()).trace, shader_spec(UTrace1()).trace) == (12, 1)
    assert (shader_spec(UTrace12()).name, shader_spec(UTrace1()).name) == ("utrace12", "utrace1")


def test_header_of_a_tracing_shader():
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    _register()
    scene = scene2()
    base = compiled_for(scene)
    cs = compiled_with_shader(scene, mirror())
    assert cs.user_shader_trace == 24 and base.user_shader_trace == 0 and cs.user_shader_probes == 0
    assert cs.user_shader == ("mirror", 10, hashlib.sha1(contrib._MIRROR_SHADER_HIP.encode()).hexdigest())
    assert len(cs.signature) == 11 and cs.signature[9] == cs.user_shader and cs.signature[10] == ("trace", 24)
    assert cs.n_params == base.n_params + 10
    hdr = specialize.code_header(cs)
    for line in ("#define RM_USER_SHADER 1\n", "#define RM_USER_SHADER_TRACE 24\n", "#define RM_USER_SHADER_PARAMS 10\n"):
        assert hdr.count(line) == 1, line
    assert "RM_USER_SHADER_PROBES" not in hdr and contrib._MIRROR_SHADER_HIP.strip() in hdr
    for forwarder in ("template <bool Fast> RM_DEV void user_shader_ray(const ShadeIn& s, const float* theta, TraceRay& r) {\n"
                      "  mirror_ray<Fast>(s, theta, r);",
                      "template <bool Fast> RM_DEV void user_shader_ray_vjp(const ShadeIn& s, const float* theta, const TraceRay& gr, ShadeGrad& gs, "
                      "float* gtheta) {\n  mirror_ray_vjp<Fast>(s, theta, gr, gs, gtheta);",
                      "template <bool Fast> RM_DEV V3 user_shader_fwd(const ShadeIn& s, const float* theta, const TraceHit& h) {\n"
                      "  return mirror_fwd<Fast>(s, theta, h);",
                      "template <bool Fast> RM_DEV void user_shader_vjp(const ShadeIn& s, const float* theta, const TraceHit& h, V3 g, ShadeGrad& gs, "
                      "float* gtheta, TraceGrad& gh) {\n  mirror_vjp<Fast>(s, theta, h, g, gs, gtheta, gh);"):
        assert hdr.count(forwarder) == 1, forwarder
    assert hdr.index("RM_USER_SHADER_TRACE 24") < hdr.index("#elif defined(RM_STATIC_CODE_LEAVES)")
    # S is part of the signature: the same source at 12 and at 1 step are two headers and two libraries
    a, b = compiled_with_shader(scene, UTrace12()), compiled_with_shader(scene, UTrace1())
    assert (a.signature[10], b.signature[10]) == (("trace", 12), ("trace", 1))
    assert len({specialize.scene_hash(x) for x in (base, cs, a, b)}) == 4 and len({specialize.lib_path(x) for x in (base, cs, a, b)}) == 4
    import dataclasses
    assert specialize.scene_hash(dataclasses.replace(a, signature=a.signature[:10] + (("trace", 13),))) != specialize.scene_hash(a)
    assert specialize.user_names(cs) == ("mirror", "shaders")
    # the entry points: in the header, in the binding and in the generic library (bind() resolved every one at import)
    header = open(os.path.join(ROOT, "include", "rm_abi.h")).read()
    for name in ("rm_user_shader_trace", "rm_trace_ws_floats", "rm_render_backward_trace"):
        assert f" {name}(" in header and name in _abi.EXPORTED_SYMBOLS and getattr(_abi.lib, name) is not None, name
    assert f"#define RM_ABI_VERSION {_abi.ABI_VERSION}\n" in header
    assert _abi.lib.rm_user_shader_trace() == 0 and _abi.lib.rm_trace_ws_floats(2, 32, 32, 2) == 0


# recorded at the parent commit (the one before traced rays existed) for make_test_scene2() with six shipped shaders: sha1 of
# specialize.code_header, sha1 of repr(signature)
PARENT = {"DirectionalLightShader": ("24e5a9549d00bd46a83baf19bcfe0e56514f78f9", "9b00658aa44148d305d6980b3e959c288ebb1d20"),
          "SoftShadowShader": ("c02176ea850b7875a95d3a074b0c202ab94f9281", "177a043fd2131123c6edfc1a2fbc5d6e074025f8"),
          "MarchedShadowShader": ("21ab5f1fa764d3137dd0c55627a5897da2514e62", "8bf28613effdec09de4ad3a5e7e6bd139ec9bb82"),
          "DepthRampShader": ("abc4c12a1e73a8c2c5c7c6d72c310d0278b04211", "9a0da69b0a71d625da3cc3023b6bb4018710d35b"),
          "TangentPaletteShader": ("cb1607267cd781405b5264c5eb07285831ea6f63", "601527dde95d375abcdcebaf17643467b44c768c"),
          "MaterialLambertShader": ("9d097b5d282ae11092f4082436aa1697c46e81c3", "32e8fbfb45a1b92b984bc1c318a5cd6f280a0528")}


@pytest.mark.parametrize("which", sorted(PARENT))
def test_headers_of_the_shipped_shaders_are_unchanged(which):
    from ray_marching_amd import contrib, specialize
    from ray_marching_amd.compiler import compiled_with_shader
    sha = lambda text: hashlib.sha1(text.encode()).hexdigest()
    cls = getattr(contrib, which)
    shader = cls(torch.rand(16, 3, generator=torch.Generator().manual_seed(1))) if which == "TangentPaletteShader" else cls()
    cs = compiled_with_shader(scene2(), shader)
    hdr = specialize.code_header(cs)
    assert cs.user_shader_trace == 0 and "TRACE" not in hdr and not any(slot[:1] == ("trace",) for slot in cs.signature[6:])
    assert (sha(hdr), sha(repr(cs.signature))) == PARENT[which]


@pytest.mark.parametrize("which,precision", [("utrace1", "exact"), ("utrace12", "exact"), ("mirror", "exact"), ("mirror", "fast")])
def test_tracing_library_cross_compiles_and_reports_its_steps(which, precision, monkeypatch, tmp_path):
    from ray_marching_amd import _abi, specialize
    from ray_marching_amd.compiler import compile_scene
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    _register()
    monkeypatch.setattr(specialize, "SPEC_DIR", str(tmp_path))
    specialize._loaded.clear()
    cs = compile_scene(scene2(), MAKERS[which]())
    path = specialize.build(cs, precision=precision)
    assert os.path.isfile(path) and os.path.dirname(path) == str(tmp_path)
    lib = cs.lib(False, precision)
    assert lib is not _abi.generic_lib(precision) and lib.rm_user_shaders() == 1 and lib.rm_abi_version() == _abi.ABI_VERSION
    assert lib.rm_user_shader_trace() == STEPS[which] and lib.rm_user_shader_table() == 0
    assert (lib.rm_user_leaves(), lib.rm_user_combinators(), lib.rm_user_warps()) == (0, 0, 0)
    # one float4 per step and lane; 2 x 32 x 32 pixels in 8x8 tiles are 32 wave tiles, at most 33 waves are started for them
    assert lib.rm_trace_ws_floats(2, 32, 32, _abi.FLAG_TILE8X8) == 4 * STEPS[which] * 33 * 64
    assert lib.rm_trace_ws_floats(0, 32, 32, 0) == 0
    for name in ("rm_user_shader_trace", "rm_trace_ws_floats", "rm_render_backward_trace"):
        assert getattr(lib, name) is not None
    assert cs.lib(True, precision) is lib
    specialize._loaded.clear()


def test_no_frame_kernel_of_the_mirror_library_has_scratch_of_its_own():
    """profiles/user_shader_trace_resource_usage.txt (hipcc's kernel-resource remarks, scene 2): every frame kernel of the
    MirrorShader library is listed next to the DirectionalLightShader library's and uses no more scratch and spills no more VGPRs."""
    rows = {}
    with open(os.path.join(ROOT, "profiles", "user_shader_trace_resource_usage.txt")) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            words = line.split()            # library, the kernel's name (may hold blanks), seven numbers
            assert len(words) >= 9 and all(x.isdigit() for x in words[-7:]), line
            rows.setdefault(words[0], {})[" ".join(words[1:-7])] = dict(zip(("vgpr", "agpr", "sgpr", "spill_s", "spill_v", "scratch", "occ"),
                                                                            map(int, words[-7:])))
    assert {"directional", "mirror"} <= set(rows)
    kernels = set(rows["mirror"])
    assert kernels == set(rows["directional"])
    for family in ("k_render_fwd", "k_render_finish", "k_render_parked", "k_render_bwd<S64, 4>", "k_bwd_hard_a"):
        assert any(k.startswith(family) for k in kernels), family
    for kernel in sorted(kernels):
        a, b = rows["mirror"][kernel], rows["directional"][kernel]
        assert a["scratch"] <= b["scratch"] and a["spill_v"] <= b["spill_v"], (kernel, a, b)
    bwd, twin = rows["mirror"]["k_render_bwd<S64, 4>"], rows["directional"]["k_render_bwd<S64, 4>"]
    print(f"k_render_bwd<.., 4>: mirror {bwd['vgpr']} VGPRs / {bwd['occ']} waves per SIMD, directional {twin['vgpr']} / {twin['occ']}")


class TorchScene(nn.Module):
    def __init__(self):
        super().__init__()
        self.spec = O.map_spec(O.scene_test2(), lambda x: nn.Parameter(x.clone()))
        self.leaves = nn.ParameterList([x for _, x in O.spec_parameters(self.spec)])

    def forward(self, points):
        return O.sdf_eval(self.spec, points)


def test_mirror_forward_with_reference_trace_is_a_march_and_a_normal():
    """The CPU contract, the oracle alone: MirrorShader.forward with reference_trace over O.sdf_eval equals the composition written
    out by hand with O.march, O.normals and O.sdf_eval, to 1e-6; and it is differentiable down to the scene's parameters."""
    from ray_marching_amd.extensions import reference_trace
    scene, shader = TorchScene(), mirror()
    gen = torch.Generator().manual_seed(4)
    n = torch.nn.functional.normalize(torch.randn(2, 5, 7, 3, generator=gen), dim=-1).requires_grad_(True)
    v = torch.nn.functional.normalize(torch.randn(2, 5, 7, 3, generator=gen), dim=-1)
    p = (0.9 * torch.randn(2, 5, 7, 3, generator=gen)).requires_grad_(True)
    out = shader(p + 3.0, None, None, v, p, n, reference_trace(scene, 24, H.EPS))
    assert out.shape == (2, 5, 7, 3) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    out.sum().backward()
    assert p.grad is not None and float(p.grad.abs().max()) > 0 and float(n.grad.abs().max()) > 0
    assert any(x.grad is not None and float(x.grad.abs().max()) > 0 for x in scene.parameters())
    for name, x in shader.named_parameters():
        assert (x.grad is not None and bool(torch.isfinite(x.grad).all())) if x.requires_grad else x.grad is None, name
    with torch.no_grad():
        l = shader.light_direction / shader.light_direction.norm()
        lit = lambda m: shader.ambient + (1 - shader.ambient) * (-(m * l).sum(-1, keepdim=True)).clamp(0, 1)
        v2 = v - 2 * (v * n).sum(-1, keepdim=True) * n
        hp = O.march(scene.spec, p + shader.bias * n, v2, 24)
        hn, _ = O.normals(scene.spec, hp, H.EPS)
        w = (1 - O.sdf_eval(scene.spec, hp) / shader.hit_eps).clamp(0, 1)
        want = (1 - shader.reflectivity) * lit(n) + shader.reflectivity * (w * lit(hn) + (1 - w) * shader.sky)
        got_p, got_n, got_d = reference_trace(scene, 24, H.EPS)(p + shader.bias * n, v2)
    assert torch.equal(got_p, hp) and torch.allclose(got_n, hn, atol=1e-6) and torch.equal(got_d, O.sdf_eval(scene.spec, hp))
    assert float((out.detach() - want).abs().max()) <= 1e-6
    assert float(w.min()) == 0.0 and float(w.max()) == 1.0


@pytest.mark.parametrize("which,leg", CASES)
def test_cpu_gradients_of_the_shader_parameters_are_not_small(which, leg):
    """The 1e-4 floor of the gradient contract is absolute: at SUITE_SCALE every component of every trainable shader parameter's
    CPU gradient is at least 1e-2 (and finite) with the constructor values of the GPU legs."""
    grads = [(n, g) for n, g in cpu_reference(which, leg, SUITE_SCALE) if n.startswith("shader.")]
    for name, g in grads:
        print(f"{which} {leg}: CPU grad {name} {g.tolist()}")
    assert [n for n, _ in grads] == (["shader.reflectivity", "shader.light_direction", "shader.ambient", "shader.sky"] if which == "mirror"
                                      else ["shader.a", "shader.b"])
    for name, g in grads:
        assert bool(torch.isfinite(g).all()) and g.abs().min().item() >= 1e-2, (name, g)


@pytest.mark.parametrize("which,leg", CASES)
def test_dropping_the_reverse_secondary_march_is_visible_in_the_cpu_gradients(which, leg):
    """The guard of the GPU gradient legs: with the hit detached -- h constant in the scene parameters and in the ray, what a backward
    without the reverse secondary march computes -- the gradient of at least one scene parameter and of the pose (or, for the
    mirror, of ``reflectivity``) is off by >= 1e-2, each at the scale it is compared at: ten times the cap on the bound."""
    moved = {}
    for scale in scales(which, leg):
        true, cut = cpu_reference(which, leg, scale), cpu_reference(which, leg, scale, constant_hit=True)
        moved.update({n: (a - b).abs().max().item() for (n, a), (_, b) in zip(true, cut) if compared(which, leg, n, scale)})
    print(f"{which} {leg}: |grad - grad (hit detached)| " + ", ".join(f"{n} {e:.3g} (scale {scale_of(which, leg, n)})" for n, e in moved.items()))
    assert max(e for n, e in moved.items() if n.startswith("scene[")) >= 1e-2
    assert max(moved["orientations"], moved["translations"], moved.get("shader.reflectivity", 0.0)) >= 1e-2


@pytest.mark.parametrize("which,leg", CASES)
def test_the_self_widening_bound_is_capped(which, leg):
    """max(1e-4, 4 E_ref) widens with the oracle's own error: for every tensor, at the scale it is compared at on the GPU, 4 E_ref <=
    1e-3.  A tensor compared below the suite's scale does not meet the cap there (else it would not be in REDUCED), and its largest
    component at its own scale is >= 0.1, a thousand times the floor of the bound."""
    bad = []
    for scale in scales(which, leg):
        ref32, ref64 = cpu_reference(which, leg, scale), cpu_reference(which, leg, scale, torch.float64)
        for (name, c32), (_, c64) in zip(ref32, ref64):
            e_ref = (c32.double() - c64).abs().max().item()
            here = compared(which, leg, name, scale)
            print(f"{which} {leg} scale {scale}: {name} E_ref {e_ref:.3g}, |g| {c64.abs().max().item():.3g}" + ("" if here else " (not compared)"))
            if here and not 4 * e_ref <= 1e-3:
                bad.append((scale, name, e_ref))
            if here and scale != SUITE_SCALE and not c32.abs().max().item() >= 0.1:
                bad.append((scale, name, "small", c32.abs().max().item()))
            if scale == SUITE_SCALE and not here and not 4 * e_ref > 1e-3 * 0.75:
                bad.append((scale, name, "meets the cap at the suite's scale", e_ref))
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which,shape", CASES)
def test_frame_against_the_cpu(which, shape, monkeypatch):
    """cpu_frame with the shader's PyTorch forward, restated math mode: max|err| <= 1e-5, through the tile kernel and the ray pools."""
    from ray_marching_amd.compiler import compiled_with_shader
    _register()
    h, w, steps, pose = FRAMES[shape]
    shader, scene = MAKERS[which]().to(DEV), scene2().to(DEV)
    cs = compiled_with_shader(scene, shader)
    assert cs.user_shader_trace == STEPS[which] and cs.lib().rm_user_shader_trace() == STEPS[which]
    q, t = pose()
    n = q.shape[0]
    with torch.no_grad(), O.math_mode("restated"):
        want = cpu_frame(O.scene_test2(), Traced(MAKERS[which](), STEPS[which]), monkeypatch, _bufs(n, h, w), q, t, steps)
    with torch.no_grad():
        for kw in (dict(), dict(regen=True)):
            got = H.make_loop(scene, h, w, n=n, **kw)(q.to(DEV), t.to(DEV), shader, 1, steps).cpu()
            err, frac = H.report(f"{which} {shape} frame", got, want)
            print(f"{which} {shape} {kw}: frame max|err| {err:.3g}, {frac:.3g} of the values beyond 1e-5")
            assert got.shape == (n, h, w, 3) and err <= 1e-5
    assert float((want.max(dim=-1).values - want.min(dim=-1).values).max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("which,leg", CASES)
def test_gradients_against_the_oracle(which, leg, monkeypatch):
    """Scene parameters, pose and every trainable shader parameter: |gpu - autograd32| <= max(1e-4, 4 E_ref) per tensor, E_ref =
    |autograd32 - autograd64| of the oracle alone, under the suite's loss; the tensors of REDUCED in a further backward at their own
    scale (module docstring).  The 40x24x32 leg
    defers rays."""
    _register()
    scene, shader = scene2().to(DEV), MAKERS[which]().to(DEV)
    bad = []
    for scale in scales(which, leg):
        ref32, ref64 = cpu_reference(which, leg, scale), cpu_reference(which, leg, scale, torch.float64)
        got, deferred = gpu_gradients(scene, shader, leg, scale, monkeypatch)
        print(f"{which} {leg} scale {scale}: {deferred} rays deferred")
        if leg.startswith("deferred"):
            assert deferred > 0, "no ray was deferred: the leg does not exercise the deferred rule"
        assert [n for n, _ in got] == [n for n, _ in ref32]
        for (name, g), (_, c32), (_, c64) in zip(got, ref32, ref64):
            assert bool(torch.isfinite(g).all()), name
            e_ref = (c32.double() - c64).abs().max().item()
            e = (g - c32).abs().max().item()
            bound = max(1e-4, 4 * e_ref)
            print(f"{which} {leg} scale {scale}: grad {name} max|err| {e:.3g}, E_ref {e_ref:.3g}, bound {bound:.3g} (|g| {c32.abs().max().item():.3g})"
                  + ("" if compared(which, leg, name, scale) else " (not compared)"))
            if compared(which, leg, name, scale) and not e <= bound:
                bad.append((scale, name))
    assert not bad, (which, leg, bad)


@pytest.mark.gpu
def test_two_backwards_of_one_frame_give_the_same_bits(monkeypatch):
    """The checkpoint workspace is private to a lane and the reverse secondary march sums in program order, so a second backward
    of the same frame gives every gradient the same bits -- with every ray walked in place, as in the same test of the normalised
    shaders: the deferred-ray list sums in the order the rays reached it, which is no function of the program
    (tests/test_deferred_backward.py)."""
    from ray_marching_amd import ops
    _register()
    scene, shader = scene2().to(DEV), mirror().to(DEV)
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)
    for leg in ("32x32x16", "37x21x16", "deferred_40x24x32"):
        first, _ = gpu_gradients(scene, shader, leg, SUITE_SCALE, monkeypatch)
        second, _ = gpu_gradients(scene, shader, leg, SUITE_SCALE, monkeypatch)
        for (name, a), (_, b) in zip(first, second):
            assert _same(a, b), (leg, name)


def _like(make, shader):
    """A fresh shader with the parameter values of ``shader``."""
    out = make()
    with torch.no_grad():
        for a, b in zip(out.parameters(), shader.parameters()):
            a.copy_(b)
    return out


@pytest.mark.gpu
def test_mirror_on_a_float16_module(monkeypatch):
    """a module cast with .to(float16) stores fp16 and computes in fp32, so its 40x24x32 frame is the fp32
    oracle evaluated on the fp16-rounded inputs (camera buffers, tetrahedron constants, scene parameters, pose), rounded once
    to fp16.  The shader's parameters are fp16-representable values.  Bit for bit."""
    h, w, steps = 24, 40, 32
    r = lambda x: x.half().float()
    spec = O.scene_test2()
    loop = H.make_loop(H.spec_to_module(spec), h, w).to(torch.float16)
    shader = mirror()
    with torch.no_grad():
        for p in shader.parameters():
            p.copy_(r(p))
    q, t = two_cameras()
    q, t = q[:1].half(), t[:1].half()
    bufs = tuple(r(b) for b in _bufs(1, h, w))
    tetra = tuple(r(c) for c in O.tetra_constants(H.EPS))
    with torch.no_grad(), O.math_mode("restated"):
        want = cpu_frame(O.map_spec(spec, r), Traced(shader, 24, tetra=tetra), monkeypatch, bufs, q.float(), t.float(), steps, tetra=tetra).half()
    with torch.no_grad():
        got = loop(q.to(DEV), t.to(DEV), _like(mirror, shader).to(DEV), 1, steps).cpu()
    assert got.dtype == torch.float16 and got.shape == (1, h, w, 3)
    ulps = (got.view(torch.int16).int() - want.view(torch.int16).int()).abs()
    print(f"fp16 mirror frame: {int((ulps > 0).sum())} of {ulps.numel()} values differ, max {int(ulps.max())} fp16 ulp")
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_captured_frame_of_the_mirror_replays_the_eager_frame():
    h, w, steps = 24, 40, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    scene, shader = scene2().to(DEV), mirror().to(DEV)
    loop = H.make_loop(scene, h, w, n=2)
    with torch.no_grad():
        eager = loop(q, t, shader, 1, steps).clone()
        frame = loop.capture(shader, 1, steps)
        for replay in range(2):
            assert torch.equal(frame(q, t), eager), replay
    assert float(eager.max()) > 0.1


TRAIN_PERTURBATION = 0.15
TRAIN_LR = 2e-3


@pytest.mark.gpu
def test_training_step_moves_a_perturbed_reflectivity_back():
    """Twenty Adam steps of a captured training step on ``reflectivity`` of a MirrorShader, towards a 32x32x16 frame of scene 2
    rendered with the unperturbed shader: it ends nearer the value the target was rendered with, and the loss decreases.  The steps
    are replays of one graph, so the checkpoint workspace of the backward is a static buffer.  (lr 2e-3: twenty steps move the
    parameter by at most 0.04, less than the perturbation.)"""
    h, w, steps = 32, 32, 16
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    truth = float(mirror().reflectivity.detach())
    with torch.no_grad():
        target = H.make_loop(scene2().to(DEV), h, w, n=2)(q, t, mirror().to(DEV), 1, steps).clone()
    loss_fn = lambda image: (image - target).pow(2).mean()
    shader = mirror().to(DEV)
    with torch.no_grad():
        shader.reflectivity += TRAIN_PERTURBATION
    distance = lambda: abs(float(shader.reflectivity.detach()) - truth)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*AccumulateGrad node's stream does not match.*")
        scene = scene2().to(DEV)
        for x in scene.parameters():
            x.requires_grad_(False)
        loop = H.make_loop(scene, h, w, n=2)
        before = distance()
        opt = torch.optim.Adam([shader.reflectivity], lr=TRAIN_LR, capturable=True)
        step = loop.training_step(loss_fn, mode=shader, marching_steps=steps, optimizer=opt)
        with torch.no_grad():
            first = float(loss_fn(loop(q, t, shader, 1, steps)))
        losses = [float(step(q, t)) for _ in range(20)]
        with torch.no_grad():
            last = float(loss_fn(loop(q, t, shader, 1, steps)))
    after = distance()
    print(f"training leg: loss before {first:.6g}, per step {[round(x, 7) for x in losses]}, after {last:.6g}; "
          f"reflectivity distance to the target's {before:.4g} -> {after:.4g}")
    assert after < before and last < first and losses[-1] < losses[0]


@pytest.mark.gpu
def test_mirror_directional_and_a_builtin_mode_in_alternation_on_one_loop():
    """One scene, one RenderLoop at 40x24x32; MirrorShader, DirectionalLightShader and mode 0 in turn, twice: three libraries, and
    each frame is the bits of its own render on a fresh loop."""
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    h, w, steps = 24, 40, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    make = {"mirror": mirror, "directional": directional}
    modes = {"mirror": mirror().to(DEV), "directional": directional().to(DEV), "lambertian": 0}
    with torch.no_grad():
        want = {k: H.make_loop(scene2().to(DEV), h, w, n=2)(q, t, make[k]().to(DEV) if k in make else m, 1, steps).clone()
                for k, m in modes.items()}
        scene = scene2().to(DEV)
        loop = H.make_loop(scene, h, w, n=2)
        for rnd in range(2):
            for k, m in modes.items():
                assert _same(loop(q, t, m, 1, steps), want[k].expand(2, h, w, 3)), (rnd, k)
    assert not _same(want["mirror"], want["directional"]) and not _same(want["directional"], want["lambertian"])
    base = compiled_for(scene)
    a, b = compiled_with_shader(scene, modes["mirror"]), compiled_with_shader(scene, modes["directional"])
    libs = [base.lib(), a.lib(), b.lib()]
    assert len({id(x) for x in libs}) == 3 and [x.rm_user_shader_trace() for x in libs] == [0, 24, 0]


@pytest.mark.gpu
def test_the_workspace_checks_of_the_backward_entry(monkeypatch):
    """rm_render_backward_trace of a tracing library with a null, a misaligned or a short workspace is RM_E_BADARG with a message (and launches
    nothing); every other library reports rm_user_shader_trace() == 0 and answers a workspace it has no use for the same way."""
    from ray_marching_amd import _abi, ops
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    h, w, steps = 32, 32, 16
    q, t = two_cameras()
    scene = scene2().to(DEV)

    def backward(mode):
        qg = q.to(DEV).requires_grad_(True)
        H.make_loop(scene, h, w, n=2)(qg, t.to(DEV), mode, 1, steps).sum().backward()
        torch.cuda.synchronize()
        return qg.grad

    shader = mirror().to(DEV)
    lib = compiled_with_shader(scene, shader).lib(True)
    need = int(lib.rm_trace_ws_floats(2, h, w, _abi.FLAG_TILE8X8))
    assert lib.rm_user_shader_trace() == 24 and need == 4 * 24 * 33 * 64
    good = backward(shader)
    assert bool(torch.isfinite(good).all())
    # null and misaligned: the entry refuses them before it looks at anything else, so the call needs nothing but the workspace
    ws = torch.empty(need + 4, dtype=torch.float32, device=DEV)
    null = (None, 0, rb"secondary ray of 24 steps: its backward needs trace_ws")
    odd = (C.c_void_p(ws.data_ptr() + 4), need, rb"secondary ray of 24 steps: its backward needs trace_ws \(16-byte aligned")
    for pointer, floats, message in (null, odd):
        rc = lib.rm_render_backward_trace(*([None] * 17), 0, 0, _abi.MODE_USER, 1, steps, 0, h, _abi.FLAG_TILE8X8, None, None, 0, None,
                                          pointer, floats, None)
        assert rc == RM_E_BADARG and re.search(message, lib.rm_last_error()), (rc, lib.rm_last_error())
    # short: refused once the launch shape is known, so through a real backward whose workspace is too small
    monkeypatch.setattr(ops.workspaces, "trace", lambda dev, stream, floats: torch.empty(64, dtype=torch.float32, device=dev))
    with pytest.raises(_abi.RmError, match=r"rm_render_backward_trace failed \(-1\).*trace_ws holds 64 floats, this launch .* needs"):
        backward(shader)
    monkeypatch.undo()
    assert torch.allclose(backward(shader), good, rtol=1e-4, atol=1e-4)      # (the refused calls launched nothing and left nothing behind)
    # the generic library and the library of a shader that traces nothing
    plain = directional().to(DEV)
    for which, mode, other in (("generic", 0, _abi.lib), ("directional", plain, compiled_with_shader(scene, plain).lib(True))):
        assert other.rm_user_shader_trace() == 0 and other.rm_trace_ws_floats(2, h, w, _abi.FLAG_TILE8X8) == 0, which
    assert compiled_for(scene).lib(True).rm_user_shader_trace() == 0
    ws = torch.empty(1 << 16, dtype=torch.float32, device=DEV)
    for which, other in (("generic", _abi.lib), ("directional", compiled_with_shader(scene, plain).lib(True))):
        rc = other.rm_render_backward_trace(*([None] * 17), 0, 0, _abi.MODE_USER if which == "directional" else 0, 1, steps, 0, h, 0, None, None, 0,
                                            None, _abi.ptr(ws), ws.numel(), None)
        assert rc == RM_E_BADARG and b"trace_ws is written by RM_MODE_USER of a library whose user shader traces" in other.rm_last_error(), which
    torch.cuda.synchronize()
