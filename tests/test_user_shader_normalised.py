"""User shaders normalised by the frame's min / max (extensions.register_shader(..., normalise="minmax")): registration of the
NAME_finish / NAME_finish_vjp pair, the header, signature and library that carry it, the compiler's resource remarks for the
second-pass kernels (profiles/user_shader_normalised_resource_usage.txt: no scratch), the torch statement of the min / max VJP
against autograd, and -- on the GPU -- test-local twins of the built-in distance and proximity modes (every bit of the frame;
the distance twin's gradients against the built-in's), contrib's DepthRampShader against the CPU oracle (frame <= 1e-5,
gradients <= max(1e-4, 4 E_ref) with E_ref = |autograd32 - autograd64| of the oracle alone), ties at both ends, clipped frames,
shapes that make every grid-stride loop run more than once, row bands, a NaN pixel, a captured replay, a captured training
step, and alternation with a flat shader and built-in modes on one loop.

The CPU side of a frame is oracle.render with ``O.shade`` replaced by the shader's own PyTorch ``forward``, which calls ``.min()`` /
``.max()`` on its own tensor (cpu_frame of tests/test_user_shader.py).
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
from tests.test_user_shader import cpu_frame
from tests.test_user_shader_probes import _bufs, _loss, _weights, inside_the_torus, two_cameras

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 1.0 / 2.33


# --------------------------------------------------------------------------------------------------------------
# test-local shaders
# --------------------------------------------------------------------------------------------------------------
def _normalised(log_values):
    lo, hi = log_values.min(), log_values.max()
    return log_values.sub(lo).div(hi.sub(lo)).pow(GAMMA).expand(*log_values.shape[:-1], 3)


class UDistance(nn.Module):
    """The built-in distance mode (mode 1, shader.py:27-38) restated as a frame-normalised user shader."""
    def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
        return _normalised(torch.linalg.vector_norm(px_coords - surface_coords, dim=-1, keepdim=True).clamp(1e-2, float("inf")).log())


class UProximity(nn.Module):
    """The built-in proximity mode (mode 2, shader.py:45-55): scene(p) is its one probe, at ``s.p``."""
    def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals, scene):
        return _normalised(scene(surface_coords).clamp(1e-2, float("inf")).log())


# NAME_finish / NAME_finish_vjp of both twins: k_shade_finish and norm_bwd_terms (csrc/rm_kernels.h), operation for operation
_TWIN_FINISH = """
template <bool Fast> RM_DEV rm::V3 NAME_finish(rm::V3 raw, float lo, float hi, const float* theta) {
  const float y = rm_pow((raw.x - lo) / (hi - lo), (float)(1.0 / 2.33));
  return mk3(y, y, y);
}
template <bool Fast> RM_DEV void NAME_finish_vjp(rm::V3 raw, float lo, float hi, const float* theta, rm::V3 g, rm::V3& graw, float& glo,
                                                 float& ghi, float* gtheta) {
  const float gamma = (float)(1.0 / 2.33), gm1 = (float)(1.0 / 2.33 - 1.0);
  const float gy = (g.x + g.y) + g.z;
  const float r = hi - lo, a = raw.x - lo;
  const float gx = gy * (gamma * rm_pow(a / r, gm1));
  const float ga = gx / r, t1 = (-gx * a) / (r * r);
  graw = mk3(ga, 0.0f, 0.0f);
  ghi = t1;
  glo = -ga - t1;
}
"""
UDISTANCE_HIP = """
template <bool Fast> RM_DEV rm::V3 udistance_fwd(const rm::ShadeIn& s, const float* theta) {
  const float l = rm_log(t_clamp(norm3(s.o - s.p), 1e-2f, __builtin_inff()));
  return mk3(l, l, l);
}
template <bool Fast> RM_DEV void udistance_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta) {
  const rm::V3 d = s.o - s.p;                     // distance_vjp (csrc/rm_kernels.h)
  const float dn = norm3(d);
  const float gd = (dn >= 1e-2f) ? g.x / dn : 0.0f;
  const rm::V3 go = (dn == 0.0f) ? mk3(0.0f, 0.0f, 0.0f) : mk3(gd * (d.x / dn), gd * (d.y / dn), gd * (d.z / dn));
  gs.o = gs.o + go;
  gs.p = gs.p - go;
}
""" + _TWIN_FINISH.replace("NAME", "udistance")
UPROXIMITY_HIP = """
template <bool Fast> RM_DEV rm::V3 uproximity_probe(int k, const rm::ShadeIn& s, const float* theta) { return s.p; }
template <bool Fast> RM_DEV void uproximity_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, rm::V3 gq, rm::ShadeGrad& gs,
                                                      float* gtheta) {
  gs.p = gs.p + gq;
}
template <bool Fast> RM_DEV rm::V3 uproximity_fwd(const rm::ShadeIn& s, const float* theta, const float* d) {
  const float l = rm_log(t_clamp(d[0], 1e-2f, __builtin_inff()));
  return mk3(l, l, l);
}
template <bool Fast> RM_DEV void uproximity_vjp(const rm::ShadeIn& s, const float* theta, const float* d, rm::V3 g, rm::ShadeGrad& gs,
                                                float* gtheta, float* gd) {
  gd[0] = (d[0] >= 1e-2f) ? g.x / d[0] : 0.0f;
}
""" + _TWIN_FINISH.replace("NAME", "uproximity")


class UPoison(nn.Module):
    """|o - p| with one value poisoned: ``poison < 0`` shows the raw depth itself (the second pass passes raw.x through), otherwise
    the pixel(s) whose depth equals ``poison`` are NaN in the first pass and the frame is the min / max ramp of the rest -- that is,
    NaN everywhere, as ``torch.min`` / ``torch.max`` have it."""
    def __init__(self):
        super().__init__()
        self.poison = nn.Parameter(torch.tensor(-1.0), requires_grad=False)

    def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
        x = torch.linalg.vector_norm(px_coords - surface_coords, dim=-1, keepdim=True)
        if float(self.poison) < 0:
            return x.expand(*x.shape[:-1], 3)
        x = torch.where(x == self.poison, torch.full_like(x, float("nan")), x)
        lo, hi = x.min(), x.max()
        return ((x - lo) / (hi - lo)).expand(*x.shape[:-1], 3)


UPOISON_HIP = """
template <bool Fast> RM_DEV rm::V3 upoison_fwd(const rm::ShadeIn& s, const float* theta) {
  const float x = norm3(s.o - s.p);
  return mk3((theta[0] >= 0.0f && x == theta[0]) ? __builtin_nanf("") : x, 0.0f, 0.0f);
}
template <bool Fast> RM_DEV void upoison_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta) {
  const rm::V3 d = s.o - s.p;
  const float dist = norm3(d);
  const rm::V3 gd = ((dist == 0.0f) ? 0.0f : g.x / dist) * d;
  gs.o = gs.o + gd;
  gs.p = gs.p - gd;
  gtheta[0] = 0.0f;
}
template <bool Fast> RM_DEV rm::V3 upoison_finish(rm::V3 raw, float lo, float hi, const float* theta) {
  const float y = (theta[0] < 0.0f) ? raw.x : (raw.x - lo) / (hi - lo);
  return mk3(y, y, y);
}
template <bool Fast> RM_DEV void upoison_finish_vjp(rm::V3 raw, float lo, float hi, const float* theta, rm::V3 g, rm::V3& graw, float& glo,
                                                    float& ghi, float* gtheta) {
  const float gy = (g.x + g.y) + g.z, r = hi - lo, a = raw.x - lo;
  const bool through = theta[0] < 0.0f;
  const float ga = through ? gy : gy / r, gr = through ? 0.0f : (-gy * a) / (r * r);
  graw = mk3(ga, 0.0f, 0.0f);
  ghi = gr;
  glo = through ? 0.0f : -ga - gr;
  gtheta[0] = 0.0f;
}
"""


def _register():
    from ray_marching_amd.extensions import register_shader
    register_shader(UDistance, hip=UDISTANCE_HIP, normalise="minmax")
    register_shader(UProximity, hip=UPROXIMITY_HIP, probes=1, normalise="minmax")
    register_shader(UPoison, params=("poison",), hip=UPOISON_HIP, normalise="minmax")


def scene2():
    from ray_marching_amd.scene import scene_registry as R
    return R.make_test_scene2()


NEAR, FAR = [1.0, 0.9, 0.7], [0.05, 0.1, 0.3]
# 10th / 90th percentile of |o - p| over the 32x32x16 two-camera frame of scene 2 (measured on the CPU oracle)
CLIP_NEAR, CLIP_FAR = 0.855, 9.12


def ramp(**kw):
    from ray_marching_amd.contrib import DepthRampShader
    return DepthRampShader(NEAR, FAR, **kw)


def ramp_clipped():
    return ramp(clip_near=CLIP_NEAR, clip_far=CLIP_FAR)


def directional():
    from ray_marching_amd.contrib import DirectionalLightShader
    return DirectionalLightShader(light_direction=[0.35, 0.5, -0.8], albedo=[0.9, 0.55, 0.3], ambient=0.15)


def gpu_test_programs():
    """Every (scene, shader) program the GPU legs launch: build() compiles their libraries, so that a GPU run of the same tree
    finds them; where they are missing the library builds itself on first use."""
    from ray_marching_amd import specialize
    from ray_marching_amd.compiler import compile_scene
    _register()
    out = [compile_scene(scene2(), make()) for make in (UDistance, UProximity, UPoison, ramp, directional)]
    return list({specialize.scene_hash(cs): cs for cs in out}.values())


# --------------------------------------------------------------------------------------------------------------
# the CPU side
# --------------------------------------------------------------------------------------------------------------
def same_pose_twice():
    """Two cameras in ONE pose: every value of the frame appears twice, so both extremes are two-fold ties."""
    q, t = two_cameras()
    return q[:1].repeat(2, 1), t[:1].repeat(2, 1)


LEGS = {"32x32x16": (32, 32, 16, two_cameras), "deferred_40x24x32": (24, 40, 32, inside_the_torus),
        "ties_32x32x16": (32, 32, 16, same_pose_twice)}


def _leg_weights(leg, n, h, w):
    """The weights of a leg's loss; the two cameras of the tie leg share one set, so that the loss is symmetric in them."""
    weights = _weights(n, h, w, 7)
    return weights[:1].repeat(n, 1, 1, 1) if leg.startswith("ties") else weights


class _Detached:
    """The ramp with ``lo`` / ``hi`` treated as constants: what a NAME_finish_vjp that leaves glo and ghi at 0 computes."""
    minmax = staticmethod(lambda x: (x.min().detach(), x.max().detach()))


class _UndividedExtremum(torch.autograd.Function):
    """min / max whose backward hands the WHOLE gradient to every pixel that attains it: a forgotten division by the tie count."""
    @staticmethod
    def forward(ctx, x, largest):
        value = x.max() if largest else x.min()
        ctx.save_for_backward(x == value)
        return value

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0].to(g.dtype), None


class _Undivided:
    minmax = staticmethod(lambda x: (_UndividedExtremum.apply(x, False), _UndividedExtremum.apply(x, True)))


def _variant(kind, **kw):
    """DepthRampShader's forward with another pair of extremes (CPU only: never rendered by the kernels)."""
    from ray_marching_amd.contrib import DepthRampShader

    class Variant(DepthRampShader):
        def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
            x = torch.linalg.vector_norm(px_coords - surface_coords, dim=-1, keepdim=True).clamp(self.clip_near, self.clip_far)
            lo, hi = kind.minmax(x)
            return self.near_colour + (x - lo) / (hi - lo) * (self.far_colour - self.near_colour)

    return Variant(NEAR, FAR, **kw)


MAKERS = {"ramp": ramp, "ramp_clipped": ramp_clipped, "udistance": UDistance,
          "ramp_detached": lambda: _variant(_Detached), "ramp_undivided": lambda: _variant(_Undivided)}


def _trainable(shader):
    return [(n, p) for n, p in shader.named_parameters() if p.requires_grad]


def _edit(shader):
    """An in-place edit and a ``.data`` assignment of shader parameters (the same on the CPU and the GPU copy)."""
    first, last = _trainable(shader)[0][1], _trainable(shader)[-1][1]
    with torch.no_grad():
        first.mul_(0.75)
    last.data = (last.detach() * 1.25 + 0.05).clone()


def _depth(bufs, q, t, spec, steps):
    """|o - p| per pixel of the CPU frame, [N,H,W,1]."""
    seen = {}

    def shade(mode, degree, px, orientation, frames, dirs, p, n, lap, dist, cmap=None):
        seen["x"] = torch.linalg.vector_norm(px - p, dim=-1, keepdim=True)
        return seen["x"].expand(*p.shape[:-1], 3)

    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(O, "shade", shade)
        with torch.no_grad():
            O.render(spec, bufs, q, t, 0, 1, steps, H.EPS)
    finally:
        mp.undo()
    return seen["x"]


@functools.lru_cache(maxsize=None)
def cpu_reference(which, leg, edited=False, dtype=torch.float32):
    """CPU autograd of one backward leg on scene 2 in ``dtype``, computed once per (shader, leg, parameters) and never modified:
    (shader gradients by name, scene gradients in named_parameters() order, dL/dq, dL/dt)."""
    h, w, steps, pose = LEGS[leg]
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
    _loss(img, _leg_weights(leg, q.shape[0], h, w).to(dtype)).backward()
    zero = lambda p: p.grad if p.grad is not None else torch.zeros_like(p)
    return ({n: p.grad.clone() for n, p in _trainable(shader)}, [zero(p) for _, p in O.spec_parameters(spec)], q.grad, t.grad)


def _flat(ref):
    """[(name, tensor)] of a cpu_reference result, scene parameters by position."""
    shader, scene, q, t = ref
    return ([(f"shader.{n}", g) for n, g in shader.items()] + [(f"scene[{i}]", g) for i, g in enumerate(scene)]
            + [("orientations", q), ("translations", t)])


def gpu_gradients(scene, mode, leg, monkeypatch, loop=None):
    """One backward of the leg on the GPU: ([(name, gradient)] in the order of _flat, rays deferred)."""
    from ray_marching_amd import ops
    h, w, steps, pose = LEGS[leg]
    q, t = pose()
    n = q.shape[0]
    qg, tg = q.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
    own = list(mode.parameters()) if isinstance(mode, nn.Module) else []
    for x in list(scene.parameters()) + own:
        x.grad = None
    sink = torch.zeros(int(ops._lib.rm_wave_tiles(n, h, w, 2)), dtype=torch.int32, device=DEV)
    monkeypatch.setattr(ops, "bwd_tile_cost_sink", sink)          # (measurement hook: keeps the backward's workspace)
    loop = loop if loop is not None else H.make_loop(scene, h, w, n=n)
    _loss(loop(qg, tg, mode, 1, steps), _leg_weights(leg, n, h, w).to(DEV)).backward()
    torch.cuda.synchronize()
    deferred = int(ops.bwd_last_work[32])
    monkeypatch.setattr(ops, "bwd_tile_cost_sink", None)
    got = [(f"shader.{n}", p.grad.cpu()) for n, p in (_trainable(mode) if isinstance(mode, nn.Module) else [])]
    got += [(f"scene[{i}]", p.grad.cpu() if p.grad is not None else torch.zeros_like(p).cpu()) for i, p in enumerate(scene.parameters())]
    got += [("orientations", qg.grad.cpu()), ("translations", tg.grad.cpu())]
    return got, deferred


def _gradients_against_the_oracle(which, scene, shader, leg, edited, monkeypatch):
    """Every tensor of one backward leg: |gpu - autograd32| <= max(1e-4, 4 E_ref), E_ref = |autograd32 - autograd64| of the oracle
    alone; every gradient finite."""
    ref32, ref64 = _flat(cpu_reference(which, leg, edited)), _flat(cpu_reference(which, leg, edited, torch.float64))
    got, deferred = gpu_gradients(scene, shader, leg, monkeypatch)
    print(f"{which} {leg} edited={edited}: {deferred} rays deferred")
    if leg.startswith("deferred"):
        assert deferred > 0, "no ray was deferred: the leg does not exercise the deferred rule"
    assert [n for n, _ in got] == [n for n, _ in ref32]
    bad = []
    for (name, g), (_, c32), (_, c64) in zip(got, ref32, ref64):
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(c32).all()), name
        e_ref = (c32.double() - c64).abs().max().item()
        e = (g - c32).abs().max().item()
        bound = max(1e-4, 4 * e_ref)
        print(f"{which} {leg} edited={edited}: grad {name} max|err| {e:.3g}, E_ref {e_ref:.3g}, bound {bound:.3g} (|g| {c32.abs().max().item():.3g})")
        if name.startswith("shader."):
            assert c32.abs().min().item() >= 1e-2, name
        if not e <= bound:
            bad.append(name)
    assert not bad, (which, leg, edited, bad)
    return dict(got)


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
FWD = "template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta) { return s.n; }\n"
VJP = ("template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta) "
       "{ gs.n = gs.n + g; }\n")
FINISH = ("template <bool Fast> RM_DEV rm::V3 NAME_finish(rm::V3 raw, float lo, float hi, const float* theta) "
          "{ return (1.0f / (hi - lo)) * (raw - mk3(lo, lo, lo)); }\n")
FINISH_VJP = ("template <bool Fast> RM_DEV void NAME_finish_vjp(rm::V3 raw, float lo, float hi, const float* theta, rm::V3 g, rm::V3& graw, "
              "float& glo, float& ghi, float* gtheta) { graw = (1.0f / (hi - lo)) * g; }\n")


def _fresh():
    class S(nn.Module):
        def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
            return (surface_normals - surface_normals[..., :1].min()) / (surface_normals[..., :1].max() - surface_normals[..., :1].min())
    return S


def test_registration_errors():
    from ray_marching_amd import contrib, extensions
    from ray_marching_amd.extensions import register_shader, shader_spec
    _register()
    full = lambda name: (FWD + VJP + FINISH + FINISH_VJP).replace("NAME", name)
    plain = lambda name: (FWD + VJP).replace("NAME", name)
    # the pairing, both ways
    with pytest.raises(ValueError, match="defines na_finish / na_finish_vjp, but normalise=None"):
        register_shader(_fresh(), hip=full("na"))                                             # the pair without normalise=
    with pytest.raises(ValueError, match="normalise='minmax', but the source of S defines no nb_finish / nb_finish_vjp"):
        register_shader(_fresh(), hip=plain("nb"), normalise="minmax")                        # normalise= without the pair
    with pytest.raises(ValueError, match=r"both or neither \(found nc_finish: True, nc_finish_vjp: False\)"):
        register_shader(_fresh(), hip=(FWD + VJP + FINISH).replace("NAME", "nc"), normalise="minmax")     # one of the two only
    with pytest.raises(ValueError, match=r"both or neither \(found nd_finish: False, nd_finish_vjp: True\)"):
        register_shader(_fresh(), hip=(FWD + VJP + FINISH_VJP).replace("NAME", "nd"), normalise="minmax")
    with pytest.raises(ValueError, match=r"both or neither"):
        register_shader(_fresh(), hip=(FWD + VJP + FINISH_VJP).replace("NAME", "nd0"))        # ... whatever normalise says
    # the value
    for bad in ("meanstd", "MinMax", True, 1, ("minmax",)):
        with pytest.raises(ValueError, match="normalise must be None or \"minmax\""):
            register_shader(_fresh(), hip=full("ne"), normalise=bad)
    # the finish pair of another NAME is not this shader's: NAME_finish_vjp of a second name still reads as a second shader
    with pytest.raises(ValueError, match="one NAME"):
        register_shader(_fresh(), hip=full("nf") + FINISH_VJP.replace("NAME", "other"), normalise="minmax")
    # a second registration: the same value is a no-op, the other value an error (normalise is one of the fields that must repeat)
    cls = _fresh()
    assert register_shader(cls, hip=full("ng"), normalise="minmax") is cls and register_shader(cls, hip=full("ng"), normalise="minmax") is cls
    with pytest.raises(ValueError, match=r"both or neither|normalise=None"):
        register_shader(cls, hip=full("ng"))
    flat = _fresh()
    register_shader(flat, hip=plain("nh"))
    with pytest.raises(ValueError, match=r"normalise='minmax', but the source"):
        register_shader(flat, hip=plain("nh"), normalise="minmax")
    # (the same source cannot carry both values: registered directly, the two registrations are told apart by the field itself)
    assert "normalise" in extensions._KINDS["shader"].same
    old = extensions._registry[cls]
    import dataclasses
    extensions._registry[cls] = dataclasses.replace(old, normalise=None)
    try:
        with pytest.raises(ValueError, match=r"already registered with different source or parameters.*normalise=None before, normalise='minmax' now"):
            register_shader(cls, hip=full("ng"), normalise="minmax")
    finally:
        extensions._registry[cls] = old
    # shader_spec reports it; the option is orthogonal to probes= and chained=
    spec = shader_spec(cls())
    assert (spec.name, spec.normalise, spec.probes, spec.chained) == ("ng", "minmax", 0, False) and shader_spec(type("Derived", (cls,), {})()) is spec
    assert (shader_spec(UProximity()).probes, shader_spec(UProximity()).normalise) == (1, "minmax")
    assert shader_spec(UDistance()).normalise == "minmax" and shader_spec(UPoison()).params == ("poison",)
    assert shader_spec(ramp()).normalise == "minmax" and shader_spec(ramp()).params == ("near_colour", "far_colour", "clip_near", "clip_far")
    assert [n for n, _ in _trainable(ramp())] == ["near_colour", "far_colour"]
    # the existing classes are what they were: normalise is None, and saying so changes nothing
    for klass, params, hip in ((contrib.DirectionalLightShader, ("light_direction", "albedo", "ambient"), contrib._DIRECTIONAL_HIP),
                               (contrib.DepthCueShader, ("density", "far_colour"), contrib._DEPTH_CUE_HIP)):
        before = shader_spec(klass())
        assert register_shader(klass, params=params, hip=hip) is klass and register_shader(klass, params=params, hip=hip, normalise=None) is klass
        assert shader_spec(klass()) is before and before.normalise is None
    for klass in (contrib.AmbientOcclusionShader, contrib.SoftShadowShader, contrib.MarchedShadowShader):
        assert shader_spec(klass()).normalise is None
    # a rank without rows joins the min / max all-reduce of such a frame, as it does for modes 1, 2 and 5
    from ray_marching_amd.distributed import _takes_minmax
    assert _takes_minmax(ramp()) and _takes_minmax(UProximity()) and not _takes_minmax(directional())
    assert [m for m in range(8) if _takes_minmax(m)] == [1, 2, 5]
    # the messages of sources without the pair stay word for word
    with pytest.raises(ValueError, match=r"exactly two device functions.*one NAME \(found fwd: \['novjp3'\], vjp: \[\]\)"):
        register_shader(_fresh(), hip=FWD.replace("NAME", "novjp3"))


def test_header_signature_and_hash_of_a_normalised_shader():
    from ray_marching_amd import _abi, contrib, specialize
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    _register()
    assert _abi.ABI_VERSION == 14
    scene = scene2()
    base, cs, flat = compiled_for(scene), compiled_with_shader(scene, ramp()), compiled_with_shader(scene, directional())
    assert cs.user_shader_normalise == "minmax" and base.user_shader_normalise is None and flat.user_shader_normalise is None
    assert cs.user_shader == ("depth_ramp", 8, hashlib.sha1(contrib._DEPTH_RAMP_HIP.encode()).hexdigest())
    assert cs.n_params == base.n_params + 8 and cs.shader_offset == base.n_params
    assert len(cs.signature) == 11 and cs.signature[9] == cs.user_shader and cs.signature[10] == ("normalise", "minmax")
    hdr = specialize.code_header(cs)
    assert "#define RM_USER_SHADER_NORMALISE 1\n" in hdr and "#define RM_USER_SHADER 1\n" in hdr and "#define RM_USER_SHADER_PARAMS 8\n" in hdr
    assert contrib._DEPTH_RAMP_HIP.strip() in hdr
    for forwarder in ("template <bool Fast> RM_DEV V3 user_shader_finish(V3 raw, float lo, float hi, const float* theta) {\n"
                      "  return depth_ramp_finish<Fast>(raw, lo, hi, theta);",
                      "template <bool Fast> RM_DEV void user_shader_finish_vjp(V3 raw, float lo, float hi, const float* theta, V3 g, V3& graw, "
                      "float& glo, float& ghi, float* gtheta) {\n  depth_ramp_finish_vjp<Fast>(raw, lo, hi, theta, g, graw, glo, ghi, gtheta);",
                      "template <bool Fast> RM_DEV V3 user_shader_fwd(const ShadeIn& s, const float* theta) {\n  return depth_ramp_fwd<Fast>(s, theta);"):
        assert hdr.count(forwarder) == 1, forwarder
    assert hdr.index("RM_USER_SHADER_NORMALISE") < hdr.index("#elif defined(RM_STATIC_CODE_LEAVES)") < hdr.index("struct RmStaticCode")
    # a flat shader's header has none of it (its sha1 is pinned by tests/test_user_shader_chained_probes.py)
    flat_hdr = specialize.code_header(flat)
    assert "NORMALISE" not in flat_hdr and "_finish" not in flat_hdr and len(flat.signature) == 10
    assert "NORMALISE" not in specialize.code_header(base)
    # orthogonal to probes=: both slots, both sections
    prox = compiled_with_shader(scene, UProximity())
    assert prox.signature[10:] == (("probes", 1), ("normalise", "minmax")) and prox.user_shader_probes == 1
    phdr = specialize.code_header(prox)
    assert "#define RM_USER_SHADER_PROBES 1\n" in phdr and "#define RM_USER_SHADER_NORMALISE 1\n" in phdr and "user_shader_finish_vjp" in phdr
    # the field reaches the library hash
    import dataclasses
    assert specialize.scene_hash(dataclasses.replace(cs, signature=cs.signature[:10])) != specialize.scene_hash(cs)
    assert len({specialize.scene_hash(x) for x in (base, cs, flat, prox)}) == 4
    assert specialize.user_names(cs) == ("depth_ramp", "shaders")
    for name in ("rm_user_shade_finish", "rm_user_shade_norm_backward"):
        assert name in _abi.EXPORTED_SYMBOLS
    # the generic library answers both with an error, as it answers RM_MODE_USER
    assert _abi.lib.rm_user_shade_finish(None, None, None, 0, 0, None, 0, None) == -1 and b"no user shader normalised" in _abi.lib.rm_last_error()
    assert _abi.lib.rm_user_shade_norm_backward(None, None, None, None, None, None, None, 0, None) == -1
    assert b"no user shader normalised" in _abi.lib.rm_last_error()


def test_normalised_library_cross_compiles_and_exports_the_second_pass(monkeypatch, tmp_path):
    import ctypes as C
    from ray_marching_amd import _abi, specialize
    from ray_marching_amd.compiler import compile_scene
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    monkeypatch.setattr(specialize, "SPEC_DIR", str(tmp_path))
    specialize._loaded.clear()
    cs = compile_scene(scene2(), ramp())
    path = specialize.build(cs)
    assert os.path.isfile(path) and os.path.dirname(path) == str(tmp_path)
    lib = cs.lib()
    assert lib is not _abi.lib and lib.rm_user_shaders() == 1 and lib.rm_abi_version() == _abi.ABI_VERSION == 14
    assert (lib.rm_user_leaves(), lib.rm_user_combinators(), lib.rm_user_warps()) == (0, 0, 0)
    raw = C.CDLL(path)
    assert hasattr(raw, "rm_user_shade_finish") and hasattr(raw, "rm_user_shade_norm_backward")
    # compiled in: a null scene is refused as a scene, not as "no such shader in this library"
    assert lib.rm_user_shade_finish(None, None, None, 0, 0, None, 0, None) == -1 and b"scene" in lib.rm_last_error()
    assert lib.rm_user_shade_norm_backward(None, None, None, None, None, None, None, 0, None) == -1 and b"scene" in lib.rm_last_error()
    assert cs.lib(True) is lib and cs.specialised
    specialize._loaded.clear()


def test_second_pass_kernels_have_no_scratch():
    """profiles/user_shader_normalised_resource_usage.txt (hipcc's kernel-resource remarks, scene 2 + DepthRampShader, P = 8): the
    second-pass kernel and the two backward kernels use no scratch memory and spill nothing -- theta, gtheta and the row of 4 + P
    partial sums are registers --, only the depth-ramp library has them, and no frame kernel of it uses more scratch than the same
    kernel of the DirectionalLightShader library."""
    rows = {}
    with open(os.path.join(ROOT, "profiles", "user_shader_normalised_resource_usage.txt")) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            words = line.split()            # library, the kernel's name (may hold blanks), seven numbers
            assert len(words) >= 9 and all(x.isdigit() for x in words[-7:]), line
            rows.setdefault(words[0], {})[" ".join(words[1:-7])] = dict(zip(("vgpr", "agpr", "sgpr", "spill_s", "spill_v", "scratch", "occ"),
                                                                            map(int, words[-7:])))
    assert {"directional", "depth_ramp"} <= set(rows)
    new = ("k_user_shade_finish", "k_user_norm_bwd_a", "k_user_norm_bwd_b")
    assert set(rows["depth_ramp"]) - set(rows["directional"]) == set(new)
    for kernel in new:
        r = rows["depth_ramp"][kernel]
        print(f"{kernel}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['occ']} waves per SIMD")
        assert (r["scratch"], r["spill_v"], r["spill_s"]) == (0, 0, 0) and r["vgpr"] <= 64, (kernel, r)
    for family in ("k_render_fwd", "k_render_finish", "k_render_parked", "k_render_bwd<S64, 4>", "k_shade_finish"):
        assert any(k.startswith(family) for k in rows["directional"]), family
    for kernel in sorted(rows["directional"]):
        a, b = rows["depth_ramp"][kernel], rows["directional"][kernel]
        assert a["scratch"] <= b["scratch"] and a["spill_v"] <= b["spill_v"], (kernel, a, b)


def test_torch_statement_of_the_minmax_vjp_against_autograd():
    """ops.frame_minmax_vjp against autograd of x.min() / x.max(): unique extremes, a k-fold tie at each end, and a NaN (where the
    statement's selects hand the end terms to nobody and autograd hands them to the NaN elements: documented there)."""
    from ray_marching_amd.ops import frame_minmax_vjp
    gen = torch.Generator().manual_seed(11)
    cases = {"unique": torch.randn(4, 9, generator=gen)}
    tied = torch.randn(4, 9, generator=gen).clamp(-0.4, 0.3)            # many elements at both clamps
    cases["ties"] = tied
    cases["nan"] = torch.randn(4, 9, generator=gen).index_put((torch.tensor(1), torch.tensor(2)), torch.tensor(float("nan")))
    assert int((tied == tied.min()).sum()) >= 3 and int((tied == tied.max()).sum()) >= 3
    for name, x0 in cases.items():
        w = torch.randn(4, 9, generator=gen)
        x = x0.clone().requires_grad_(True)
        lo, hi = x.min(), x.max()
        lo.retain_grad(), hi.retain_grad()
        ((w * x).sum() + 3.0 * lo - 2.0 * hi).backward()
        got = frame_minmax_vjp(w, lo.grad, hi.grad, x0, x0.min(), x0.max())
        finite = ~x0.isnan()
        print(f"{name}: {int((x0 == x0.min()).sum())} at the minimum, {int((x0 == x0.max()).sum())} at the maximum, "
              f"max|diff| {(got - x.grad)[finite].abs().max().item():.3g}")
        assert torch.allclose(got[finite], x.grad[finite], rtol=0, atol=1e-6), name
        if name == "nan":
            assert torch.equal(got[finite], w[finite]) and torch.equal(got[~finite], w[~finite]) and not torch.equal(x.grad[~finite], w[~finite])
        else:
            assert not torch.equal(got, w)


def test_depth_ramp_stand_alone_on_the_cpu():
    """Called directly on CPU tensors DepthRampShader is plain PyTorch: [..., 3], the formula written out, gradients to its inputs and
    its colours, none to the frozen clips."""
    shader = ramp_clipped()
    gen = torch.Generator().manual_seed(4)
    p = (3.0 * torch.randn(2, 5, 7, 3, generator=gen)).requires_grad_(True)
    o = torch.randn(2, 5, 7, 3, generator=gen)
    out = shader(o, None, None, None, p, None)
    assert out.shape == (2, 5, 7, 3) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    with torch.no_grad():
        x = (o - p).norm(dim=-1, keepdim=True).clamp(CLIP_NEAR, CLIP_FAR)
        want = shader.near_colour + (x - x.min()) / (x.max() - x.min()) * (shader.far_colour - shader.near_colour)
    assert torch.allclose(out, want, atol=1e-6) and float(out.detach().min()) >= 0.05 - 1e-6 and float(out.detach().max()) <= 1.0 + 1e-6
    (out * (torch.rand(2, 5, 7, 3, generator=gen) + 0.5)).mean().mul(8.0).backward()
    assert p.grad is not None and float(p.grad.abs().max()) > 0
    for name, g in ((n, x.grad) for n, x in _trainable(shader)):
        print(f"stand-alone: grad {name} {g.tolist()}")
        assert bool(torch.isfinite(g).all()) and g.abs().min().item() >= 1e-2, name
    assert shader.clip_near.grad is None and shader.clip_far.grad is None


@pytest.mark.parametrize("which,leg", [("ramp", "32x32x16"), ("ramp", "deferred_40x24x32"), ("ramp", "ties_32x32x16"),
                                       ("ramp_clipped", "32x32x16")])
def test_cpu_frames_extremes_and_shader_gradients(which, leg):
    """What the GPU legs rely on, asserted on the CPU frame: the number of pixels at each extreme (1 and 1 where the poses differ, 2
    and 2 for one pose twice, between 2 and a quarter of the pixels for the clipped frame), no NaN, and every component of the
    colours' gradients at least 1e-2 (the 1e-4 floor of the gradient contract is absolute), before and after the edit."""
    h, w, steps, pose = LEGS[leg]
    q, t = pose()
    shader = MAKERS[which]()
    x = _depth(_bufs(q.shape[0], h, w), q, t, O.scene_test2(), steps).clamp(float(shader.clip_near), float(shader.clip_far))
    n_lo, n_hi, n = int((x == x.min()).sum()), int((x == x.max()).sum()), x.numel()
    print(f"{which} {leg}: min x {float(x.min()):.4g}, max x {float(x.max()):.4g}, {n_lo} at the minimum, {n_hi} at the maximum, "
          f"10th / 90th percentile {float(x.flatten().kthvalue(n // 10).values):.4g} / {float(x.flatten().kthvalue(9 * n // 10).values):.4g}")
    assert not bool(x.isnan().any())
    if which == "ramp_clipped":
        assert 2 <= n_lo <= n // 4 and 2 <= n_hi <= n // 4
    else:
        assert (n_lo, n_hi) == ((2, 2) if leg.startswith("ties") else (1, 1))
    for edited in (False, True):
        for name, g in cpu_reference(which, leg, edited)[0].items():
            print(f"{which} {leg} edited={edited}: CPU grad {name} {g.tolist()}")
            assert bool(torch.isfinite(g).all()) and g.abs().min().item() >= 1e-2, (name, g)


def _largest_scene_difference(a, b):
    return max((x - y).abs().max().item() for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("leg", ["32x32x16", "deferred_40x24x32"])
def test_cpu_end_terms_are_visible(leg):
    """A NAME_finish_vjp that leaves glo and ghi at 0 differentiates the ramp with lo / hi held constant: on the CPU statement its
    gradient is at least 1e-2 away in some scene tensor, a hundred times the floor of the contract -- the GPU legs see the two end
    terms, each of which reaches exactly one ray."""
    d = _largest_scene_difference(cpu_reference("ramp", leg), cpu_reference("ramp_detached", leg))
    print(f"{leg}: dropping the end terms moves a scene gradient by {d:.3g}")
    assert d >= 1e-2


def test_cpu_forgotten_division_is_visible():
    """One pose twice: n_lo = n_hi = 2.  End terms handed whole to both tied pixels (no division by the tie count) are at least
    1e-2 away in some scene tensor on the CPU statement."""
    d = _largest_scene_difference(cpu_reference("ramp", "ties_32x32x16"), cpu_reference("ramp_undivided", "ties_32x32x16"))
    print(f"ties: a forgotten division moves a scene gradient by {d:.3g}")
    assert d >= 1e-2


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
TWIN_RENDERS = {"deferred_40x24x32": (24, 40, 32, inside_the_torus), "32x32x16": (32, 32, 16, two_cameras)}


@pytest.mark.gpu
@pytest.mark.parametrize("render", sorted(TWIN_RENDERS))
def test_twins_of_the_builtin_distance_and_proximity_modes_are_bit_identical(render):
    """UDistance / UProximity restate modes 1 and 2 operation for operation: their frames are the built-in modes' bits on the same
    loop (NaN for NaN where the built-in's frame is NaN: torch.equal cannot say that), through the tile kernel and the ray pools
    (regen=True), on an fp32 and on a float16 module, and as display_frame."""
    from ray_marching_amd.compiler import compiled_with_shader
    _register()
    h, w, steps, pose = TWIN_RENDERS[render]
    q, t = pose()
    n = q.shape[0]
    twins = {1: UDistance(), 2: UProximity()}
    with torch.no_grad():
        for dtype in (torch.float32, torch.float16):
            scene = scene2().to(DEV)
            for kw in (dict(), dict(regen=True)):
                loop = H.make_loop(scene, h, w, n=n, **kw).to(dtype)
                qd, td = q.to(DEV, dtype), t.to(DEV, dtype)
                for mode, twin in twins.items():
                    assert compiled_with_shader(loop.scene, twin).user_shader_normalise == "minmax"
                    want = loop(qd, td, mode, 1, steps).clone()
                    got = loop(qd, td, twin, 1, steps)
                    nans = int(want.isnan().sum())       # (a ray that leaves for infinity makes mode 2's frame NaN, in the reference too)
                    differ = int(((got != want) & ~(got.isnan() & want.isnan())).sum())
                    print(f"{render} {dtype} {kw} mode {mode}: {differ} of {got.numel()} values differ ({nans} NaN in the built-in's frame)")
                    assert got.shape == (n, h, w, 3) and got.dtype == dtype and _same(got, want), (dtype, kw, mode)
                    assert nans in (0, want.numel()) and (nans or (float(want.float().max()) == 1.0 and float(want.float().min()) == 0.0))
                    if n == 1:
                        want4, got4 = loop.display_frame(qd, td, mode, 1, steps).clone(), loop.display_frame(qd, td, twin, 1, steps)
                        assert got4.shape == (h, w, 4) and got4.dtype == torch.float32 and _same(got4, want4), (dtype, kw, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["32x32x16", "deferred_40x24x32"])
def test_distance_twin_gradients_against_the_builtin_mode(leg, monkeypatch):
    """Gradients of the distance twin against the built-in mode 1's on the same frame: the same NaN pattern element for element in
    every tensor (pow(1 / 2.33) has an infinite slope at the minimum: the rays of the minimum and of the maximum carry NaN, in
    the reference as here), and |twin - builtin| <= max(1e-4, 4 E_ref) on the finite elements, E_ref the CPU oracle's own
    |autograd32 - autograd64| of the same shader."""
    _register()
    scene = scene2().to(DEV)
    twin, _ = gpu_gradients(scene, UDistance(), leg, monkeypatch)
    builtin, _ = gpu_gradients(scene, 1, leg, monkeypatch)
    ref32, ref64 = _flat(cpu_reference("udistance", leg)), _flat(cpu_reference("udistance", leg, False, torch.float64))
    assert [n for n, _ in twin] == [n for n, _ in builtin] == [n for n, _ in ref32]
    bad, nans = [], 0
    for (name, a), (_, b), (_, c32), (_, c64) in zip(twin, builtin, ref32, ref64):
        assert torch.equal(a.isnan(), b.isnan()), (name, a, b)
        ok = ~b.isnan()
        nans += int((~ok).sum())
        both = ok & ~c32.isnan() & ~c64.isnan()
        e_ref = (c32.double() - c64)[both].abs().max().item() if bool(both.any()) else 0.0
        e = (a - b)[ok].abs().max().item() if bool(ok.any()) else 0.0
        bound = max(1e-4, 4 * e_ref)
        print(f"udistance {leg}: grad {name} max|twin - builtin| {e:.3g}, E_ref {e_ref:.3g}, bound {bound:.3g}, {int((~ok).sum())} NaN")
        if not e <= bound:
            bad.append(name)
    assert not bad, bad
    assert nans > 0, "the rays of the extremes carry NaN gradients in mode 1: the leg must see them"


@pytest.mark.gpu
def test_depth_ramp_against_the_cpu(monkeypatch):
    """DepthRampShader on scene 2 against the oracle with the shader's PyTorch forward as its shade(): frames <= 1e-5 (restated math
    mode of the oracle) through the tile kernel and the ray pools; every gradient (colours, scene, orientation, translation) by the
    contract at 32x32x16 with two cameras and at 40x24x32 from inside the torus, where rays are deferred (asserted); then an in-place
    edit and a ``.data`` assignment of the colours: the next frame and backward follow the new values."""
    from ray_marching_amd.compiler import compiled_with_shader
    shader, cpu_shader = ramp().to(DEV), ramp()
    scene = scene2().to(DEV)
    cs = compiled_with_shader(scene, shader)
    assert cs.user_shader_normalise == "minmax" and cs.lib().rm_user_shaders() == 1
    for edited in (False, True):
        if edited:
            _edit(shader), _edit(cpu_shader)
        for leg in ("32x32x16", "deferred_40x24x32"):
            h, w, steps, pose = LEGS[leg]
            q, t = pose()
            with torch.no_grad(), O.math_mode("restated"):
                want = cpu_frame(O.scene_test2(), cpu_shader, monkeypatch, _bufs(q.shape[0], h, w), q, t, steps)
            with torch.no_grad():
                for kw in (dict(), dict(regen=True)):
                    got = H.make_loop(scene, h, w, n=q.shape[0], **kw)(q.to(DEV), t.to(DEV), shader, 1, steps).cpu()
                    err, frac = H.report("depth ramp frame", got, want)
                    print(f"depth ramp {leg} edited={edited} {kw}: frame max|err| {err:.3g} (expected 0)")
                    assert got.shape == want.shape and err <= 1e-5
            _gradients_against_the_oracle("ramp", scene, shader, leg, edited, monkeypatch)


@pytest.mark.gpu
def test_ties_share_the_end_terms(monkeypatch):
    """Two cameras in one pose: n_lo = n_hi = 2 (asserted on the CPU frame by test_cpu_frames_extremes_and_shader_gradients).  The
    gradients hold the contract, and -- the loss weighs both cameras alike -- both get the same orientation gradient, bit for bit."""
    scene, shader = scene2().to(DEV), ramp().to(DEV)
    got = _gradients_against_the_oracle("ramp", scene, shader, "ties_32x32x16", False, monkeypatch)
    gq = got["orientations"]
    assert torch.equal(gq[0], gq[1]) and float(gq[0].abs().max()) > 0, gq


@pytest.mark.gpu
def test_clipped_frame_has_many_ties_and_finite_gradients(monkeypatch):
    """clip_near / clip_far at the 10th / 90th percentile: about a tenth of the pixels tie at each end (asserted on the CPU frame), and
    their clamp passes no gradient.  Frame error 0 expected (<= 1e-5), all gradients finite and within the contract."""
    scene, shader, cpu_shader = scene2().to(DEV), ramp_clipped().to(DEV), ramp_clipped()
    h, w, steps, pose = LEGS["32x32x16"]
    q, t = pose()
    with torch.no_grad(), O.math_mode("restated"):
        want = cpu_frame(O.scene_test2(), cpu_shader, monkeypatch, _bufs(2, h, w), q, t, steps)
    with torch.no_grad():
        got = H.make_loop(scene, h, w, n=2)(q.to(DEV), t.to(DEV), shader, 1, steps).cpu()
    err, _ = H.report("clipped frame", got, want)
    print(f"clipped frame: max|err| {err:.3g} (expected 0)")
    assert err <= 1e-5
    _gradients_against_the_oracle("ramp_clipped", scene, shader, "32x32x16", False, monkeypatch)


@pytest.mark.gpu
def test_two_backwards_of_one_frame_are_bit_identical():
    """40x24 pixels (no multiple of 64 or 256): the frame sums are taken in a fixed order, and every ray is walked in place (no
    deferred-ray list: its atomically ordered partial sums are no function of the program), so a second backward of the same
    frame gives the same bits in every gradient."""
    from ray_marching_amd import ops
    scene, shader = scene2().to(DEV), ramp().to(DEV)
    h, w, steps = 24, 40, 16
    q, t = two_cameras()
    q, t = q[:1].to(DEV).requires_grad_(True), t[:1].to(DEV).requires_grad_(True)
    keep, ops.bwd_hard_capacity = ops.bwd_hard_capacity, 0
    try:
        image = H.make_loop(scene, h, w)(q, t, shader, 1, steps)
        loss = _loss(image, _weights(1, h, w, 7).to(DEV))
        tensors = [q, t] + _trainable_tensors(shader) + list(scene.parameters())
        first = torch.autograd.grad(loss, tensors, retain_graph=True)
        second = torch.autograd.grad(loss, tensors)
    finally:
        ops.bwd_hard_capacity = keep
    assert all(_same(a, b) for a, b in zip(first, second))
    assert all(bool(torch.isfinite(g).all()) for g in first) and float(first[2].abs().min()) >= 1e-2


def _trainable_tensors(shader):
    return [p for _, p in _trainable(shader)]


@pytest.mark.gpu
def test_frame_larger_than_the_second_pass_grids():
    """600x440 = 264000 pixels, more than the 1024 x 256 threads the second pass and both backward kernels are launched with: every
    grid-stride loop runs more than once.  Two marching steps.  The frame against the CPU on every 97th pixel (<= 1e-5), the
    colours' gradients against CPU autograd by the contract."""
    from ray_marching_amd import _abi
    h, w, steps = 440, 600, 2
    assert h * w > _abi.NORM_BWD_BLOCKS * 256 and (h * w) % 256
    q, t = two_cameras()
    q, t = q[:1], t[:1]
    weights = _weights(1, h, w, 7)
    grads, frames = {}, {}
    for dtype in (torch.float32, torch.float64):
        shader = ramp().to(dtype)
        mp = pytest.MonkeyPatch()
        try:
            img = cpu_frame(O.map_spec(O.scene_test2(), lambda x: x.to(dtype)), shader, mp, tuple(b.to(dtype) for b in _bufs(1, h, w)),
                            q.to(dtype), t.to(dtype), steps)
        finally:
            mp.undo()
        _loss(img, weights.to(dtype)).backward()
        grads[dtype], frames[dtype] = {n: p.grad for n, p in _trainable(shader)}, img.detach()
    scene, shader = scene2().to(DEV), ramp().to(DEV)
    for x in scene.parameters():
        x.requires_grad_(False)
    got = H.make_loop(scene, h, w)(q.to(DEV), t.to(DEV), shader, 1, steps)
    _loss(got, weights.to(DEV)).backward()
    sample = slice(None, None, 97)
    err = (got.detach().cpu().reshape(-1, 3)[sample] - frames[torch.float32].reshape(-1, 3)[sample]).abs().max().item()
    print(f"large frame: max|err| on every 97th pixel {err:.3g}")
    assert err <= 1e-5
    for name, p in _trainable(shader):
        c32, c64 = grads[torch.float32][name], grads[torch.float64][name]
        e_ref, e = (c32.double() - c64).abs().max().item(), (p.grad.cpu() - c32).abs().max().item()
        print(f"large frame: grad {name} max|err| {e:.3g}, E_ref {e_ref:.3g} (CPU {c32.tolist()})")
        assert c32.abs().min().item() >= 1e-2 and e <= max(1e-4, 4 * e_ref), name


@pytest.mark.gpu
def test_row_bands_with_the_allreduce_hook():
    """The 40x24 frame as two ``rows=`` bands on one GPU, the ``allreduce_minmax`` hook putting in the pair of the whole frame (what
    RowTileRenderer does across ranks): the bands concatenated are the whole frame's bits.  A backward through a min / max taken
    across ranks raises NotImplementedError, as for modes 1, 2 and 5."""
    scene, shader = scene2().to(DEV), ramp().to(DEV)
    h, w, steps = 24, 40, 16
    q, t = two_cameras()
    q, t = q[:1].to(DEV), t[:1].to(DEV)
    loop = H.make_loop(scene, h, w)
    bands = ((0, 10), (10, h))
    with torch.no_grad():
        whole = loop(q, t, shader, 1, steps).clone()
        seen = []
        for band in bands:
            loop(q, t, shader, 1, steps, rows=band, allreduce_minmax=lambda lohi: seen.append(lohi.clone()))
        pair = torch.stack([torch.stack(seen)[:, 0].min(), torch.stack(seen)[:, 1].max()])
        assert float(seen[0][0]) != float(seen[1][0]) or float(seen[0][1]) != float(seen[1][1])
        parts = [loop(q, t, shader, 1, steps, rows=band, allreduce_minmax=lambda lohi: lohi.copy_(pair)) for band in bands]
    assert [p.shape[1] for p in parts] == [10, h - 10] and torch.equal(torch.cat(parts, dim=1), whole)
    qg = q.clone().requires_grad_(True)
    band = loop(qg, t, shader, 1, steps, rows=bands[0], allreduce_minmax=lambda lohi: lohi.copy_(pair))
    with pytest.raises(NotImplementedError, match="across ranks"):
        band.sum().backward()


@pytest.mark.gpu
def test_a_nan_in_one_pixel_makes_the_whole_frame_nan(monkeypatch):
    """UPoison first shows the raw depth (an in-place edit of its parameter then reaches the second pass too); the depth of pixel
    (11, 17) is unique (asserted), and poisoning it makes that one pixel NaN in the first pass -- and the whole image NaN, as on the
    CPU, where min() and max() of a tensor with a NaN are NaN."""
    _register()
    scene, shader, cpu_shader = scene2().to(DEV), UPoison().to(DEV), UPoison()
    h, w, steps = 24, 40, 16
    q, t = two_cameras()
    q, t = q[:1], t[:1]
    loop = H.make_loop(scene, h, w)
    with torch.no_grad():
        depth = loop(q.to(DEV), t.to(DEV), shader, 1, steps).cpu()
        want_depth = cpu_frame(O.scene_test2(), cpu_shader, monkeypatch, _bufs(1, h, w), q, t, steps)
        assert H.report("raw depth", depth, want_depth)[0] <= 1e-5 and not bool(depth.isnan().any())
        value = depth[0, 11, 17, 0]
        assert int((depth[..., 0] == value).sum()) == 1
        shader.poison.fill_(float(value))
        cpu_shader.poison.fill_(float(want_depth[0, 11, 17, 0]))
        got = loop(q.to(DEV), t.to(DEV), shader, 1, steps).cpu()
        want = cpu_frame(O.scene_test2(), cpu_shader, monkeypatch, _bufs(1, h, w), q, t, steps)
    assert bool(want.isnan().all()) and bool(got.isnan().all()) and got.shape == (1, h, w, 3)


@pytest.mark.gpu
def test_captured_frame_and_captured_training_step():
    """``capture`` replays the eager frame bit for bit (image and display tensor); ``training_step`` -- forward, second pass, its VJP
    and the fused backward in one HIP graph -- moves perturbed colours back towards the frame of the unperturbed ones."""
    h, w, steps = 32, 32, 16
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    scene = scene2().to(DEV)
    for x in scene.parameters():
        x.requires_grad_(False)
    loop = H.make_loop(scene, h, w, n=2)
    truth = ramp().to(DEV)
    with torch.no_grad():
        target = loop(q, t, truth, 1, steps).clone()
        frame = loop.capture(truth, 1, steps)
        for replay in range(2):
            assert torch.equal(frame(q, t), target), replay
        one = H.make_loop(scene, h, w)
        eager4 = one.display_frame(q[:1], t[:1], truth, 1, steps).clone()
        assert torch.equal(one.capture(truth, 1, steps, display=True)(q[:1], t[:1]), eager4) and eager4.shape == (h, w, 4)
    assert float(target.max()) > 0.9 and float(target.min()) < 0.3
    shader = ramp().to(DEV)
    with torch.no_grad():
        shader.near_colour -= 0.3
        shader.far_colour += 0.25
    distance = lambda: (float((shader.near_colour.detach() - truth.near_colour.detach()).abs().max()),
                        float((shader.far_colour.detach() - truth.far_colour.detach()).abs().max()))
    loss_fn = lambda image: (image - target).pow(2).mean()
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*AccumulateGrad node's stream does not match.*")
        before = distance()
        opt = torch.optim.Adam([shader.near_colour, shader.far_colour], lr=2e-2, capturable=True)
        step = loop.training_step(loss_fn, mode=shader, marching_steps=steps, optimizer=opt)
        with torch.no_grad():
            first = float(loss_fn(loop(q, t, shader, 1, steps)))
        losses = [float(step(q, t)) for _ in range(20)]
        with torch.no_grad():
            last = float(loss_fn(loop(q, t, shader, 1, steps)))
    after = distance()
    print(f"training leg: loss before {first:.6g}, per step {[round(x, 7) for x in losses]}, after {last:.6g}; "
          f"(near, far) distance to the target's {before} -> {after}")
    assert after[0] < before[0] and after[1] < before[1]
    assert last < first and losses[-1] < losses[0]


@pytest.mark.gpu
def test_normalised_shader_flat_shader_and_builtin_modes_in_alternation_on_one_loop():
    """One scene, one RenderLoop; DepthRampShader, DirectionalLightShader and modes 0 and 1 in turn, twice: each frame is the bits of
    its own render on a fresh loop."""
    from ray_marching_amd.compiler import compiled_for, compiled_with_shader
    h, w, steps = 44, 60, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    make = {"ramp": ramp, "directional": directional}
    modes = {"ramp": ramp().to(DEV), "directional": directional().to(DEV), "lambertian": 0, "distance": 1}
    with torch.no_grad():
        want = {k: H.make_loop(scene2().to(DEV), h, w, n=2)(q, t, make[k]().to(DEV) if k in make else m, 1, steps).clone()
                for k, m in modes.items()}
        scene = scene2().to(DEV)
        loop = H.make_loop(scene, h, w, n=2)
        for rnd in range(2):
            for k, m in modes.items():
                assert _same(loop(q, t, m, 1, steps), want[k].expand(2, h, w, 3)), (rnd, k)
    assert not _same(want["ramp"], want["directional"]) and not _same(want["ramp"], want["distance"])
    base = compiled_for(scene)
    a, b = compiled_with_shader(scene, modes["ramp"]), compiled_with_shader(scene, modes["directional"])
    libs = [base.lib(), a.lib(), b.lib()]
    assert len({id(x) for x in libs}) == 3 and [x.rm_user_shaders() for x in libs] == [0, 1, 1]
    assert (a.user_shader_normalise, b.user_shader_normalise, base.user_shader_normalise) == ("minmax", None, None)
