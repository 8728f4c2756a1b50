"""User shaders that read a lookup table (extensions.register_shader(table="ATTR", table_taps=T)): registration, the code header
and the specialised library, contrib's TangentPaletteShader / DepthPaletteShader on the CPU, and -- on the GPU -- the table's
gradient: the records of the fused backward summed by k_table_scatter, without float atomics and in an order that depends on the
record index alone.

The scatter is checked EXACTLY (test_exact_scatter): a test-local shader whose colour is one table row, a loss of small-integer
weights, so that every sum is an integer far below 2^24 and the gradient must equal ``index_add`` whatever the order -- a lost,
doubled or misplaced record cannot hide behind a tolerance.  The other legs: two backwards give the same bits; TangentPaletteShader
is the built-in tangent mode bit for bit (frames and gradients); DepthPaletteShader against the CPU oracle at the tolerances of
test_user_shader.test_contrib_shader_against_the_cpu (frame 1e-5, gradients 1e-4), after the oracle's own fp32 and fp64
gradients were seen to agree within 1e-5 on the same legs; a captured training step over the palette alone; and a table shader, a
table-less shader and a built-in mode in alternation on one loop.
"""
import copy
import functools
import hashlib
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import sdf_oracle as O
from tests import helpers as H
from tests.helpers import _same
from tests.test_user_shader import _bufs, _loss, _scenes, _unit, _weights, cpu_frame, depth_cue, inside_the_torus, two_cameras

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------------------
# test-defined shaders: the colour is ONE row of the table, picked by the Lambertian term (T = 1)
# --------------------------------------------------------------------------------------------------------------
class _RowShader(nn.Module):
    def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
        c = (ray_directions * surface_normals).sum(dim=-1).neg().clamp(0, 1)
        return self.palette[(c * (self.palette.shape[0] - 1) + 0.5).floor().long()]


class UTableRow(_RowShader):
    """The table is a Parameter."""
    def __init__(self, palette):
        super().__init__()
        self.palette = nn.Parameter(palette.clone().float().contiguous())


class UTableBuffer(_RowShader):
    """The table is a registered buffer: no gradient, no records, no scatter."""
    def __init__(self, palette):
        super().__init__()
        self.register_buffer("palette", palette.clone().float().contiguous())


UTABLE_ROW_HIP = """
RM_DEV int utable_row_index(const rm::ShadeIn& s, const rm::Table& tab) {
  const float c = t_clamp(-dot_seq(s.v, s.n), 0.0f, 1.0f);
  return (int)floorf(c * (float)(tab.n - 1) + 0.5f);
}
template <bool Fast> RM_DEV rm::V3 utable_row_fwd(const rm::ShadeIn& s, const float* theta, const rm::Table& tab) {
  return tab.row(utable_row_index(s, tab));
}
template <bool Fast> RM_DEV void utable_row_vjp(const rm::ShadeIn& s, const float* theta, const rm::Table& tab, rm::V3 g,
                                                rm::ShadeGrad& gs, float* gtheta, rm::TableGrad& gt) {
  gt.row[0] = tab.clamp(utable_row_index(s, tab));
  gt.g[0] = g;
}
"""
UTABLE_BUFFER_HIP = UTABLE_ROW_HIP.replace("utable_row", "utable_buffer")


class UTableLit(UTableRow):
    """The row plus the Lambertian term on every channel: the table's gradient is still the upstream alone, but the scene now has
    one too -- without it no ray's reverse march has anything to carry and none is deferred."""
    def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
        c = (ray_directions * surface_normals).sum(dim=-1, keepdim=True).neg().clamp(0, 1)
        return super().forward(px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals) + c


UTABLE_LIT_HIP = """
RM_DEV int utable_lit_index(const rm::ShadeIn& s, const rm::Table& tab) {
  const float c = t_clamp(-dot_seq(s.v, s.n), 0.0f, 1.0f);
  return (int)floorf(c * (float)(tab.n - 1) + 0.5f);
}
template <bool Fast> RM_DEV rm::V3 utable_lit_fwd(const rm::ShadeIn& s, const float* theta, const rm::Table& tab) {
  const float c = t_clamp(-dot_seq(s.v, s.n), 0.0f, 1.0f);
  return tab.row(utable_lit_index(s, tab)) + mk3(c, c, c);
}
template <bool Fast> RM_DEV void utable_lit_vjp(const rm::ShadeIn& s, const float* theta, const rm::Table& tab, rm::V3 g,
                                                rm::ShadeGrad& gs, float* gtheta, rm::TableGrad& gt) {
  gt.row[0] = tab.clamp(utable_lit_index(s, tab));
  gt.g[0] = g;
  const float e = -dot_seq(s.v, s.n);
  const float ge = (e >= 0.0f && e <= 1.0f) ? ((g.x + g.y) + g.z) : 0.0f;
  gs.v = gs.v - ge * s.n;
  gs.n = gs.n - ge * s.v;
}
"""


def _register():
    from ray_marching_amd.extensions import register_shader
    register_shader(UTableRow, hip=UTABLE_ROW_HIP, table="palette", table_taps=1)
    register_shader(UTableBuffer, hip=UTABLE_BUFFER_HIP, table="palette", table_taps=1)
    register_shader(UTableLit, hip=UTABLE_LIT_HIP, table="palette", table_taps=1)


def ramp(n):
    """Row r = (r, r, r): a frame rendered with it returns every pixel's row index exactly."""
    return torch.arange(n, dtype=torch.float32)[:, None].expand(n, 3).contiguous()


def smooth_palette(n=16):
    """A short, smooth palette (rows sampled from three phase-shifted cosines): the interpolation's slope jumps little at the knots."""
    x = torch.linspace(0.0, 1.0, n)[:, None]
    return 0.5 + 0.4 * torch.cos(2.0 * x + torch.tensor([0.0, 2.0, 4.0]))


def depth_palette(n=16):
    from ray_marching_amd.contrib import DepthPaletteShader
    return DepthPaletteShader(density=0.3, palette=smooth_palette(n))


def two_cameras_inside():
    """Two cameras inside the room, near the solids.  The 32x32x16 leg of test_user_shader looks on from z = -3, where 16 steps
    leave rays unconverged and the oracle's OWN fp32 and fp64 gradients differ by 1.4e-3 (pose) -- with DepthCueShader as much as with
    a palette: the march, not the shader.  From here they agree within 3e-6 (test_cpu_reference_is_well_inside_the_tolerance), so
    the leg keeps its size and step count and takes this pose."""
    q = torch.stack([_unit([0.98, -0.1, 0.15, 0.05]), _unit([1.0, 0.05, -0.1, 0.02])])
    return q, torch.tensor([[0.0, 0.3, 0.8], [0.2, 0.0, 1.5]])


BACKWARD_LEGS = {"32x32x16": (32, 32, 16, two_cameras_inside), "deferred_40x24x32": (24, 40, 32, inside_the_torus)}


def cmap32():
    """The float32 cast of the reference's colormap ([4096, 3])."""
    return torch.from_numpy(H.gold("cmap.npz")["cyclic_cmap"]).float().contiguous()


def tangent_palette(palette=None):
    from ray_marching_amd.contrib import TangentPaletteShader
    return TangentPaletteShader(cmap32() if palette is None else palette)


def gpu_test_programs():
    """Every (scene, shader) program the GPU legs launch (the library does not depend on the table's length or values): build()
    compiles their libraries, so that a GPU run of the same tree finds them."""
    from ray_marching_amd import specialize
    from ray_marching_amd.compiler import compile_scene
    _register()
    scenes = _scenes()
    out = [compile_scene(scenes["scene2"](), make()) for make in (lambda: UTableRow(ramp(4)), lambda: UTableBuffer(ramp(4)), lambda: UTableLit(ramp(4)),
                                                                  depth_palette)]
    out += [compile_scene(make(), tangent_palette(ramp(4))) for make in scenes.values()]
    return list({specialize.scene_hash(cs): cs for cs in out}.values())


# --------------------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------------------
FWD = "template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta) { return s.n; }\n"
VJP = ("template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta) "
       "{ gs.n = gs.n + g; }\n")
TFWD = "template <bool Fast> RM_DEV rm::V3 NAME_fwd(const rm::ShadeIn& s, const float* theta, const rm::Table& tab) { return tab.row(0); }\n"
TVJP = ("template <bool Fast> RM_DEV void NAME_vjp(const rm::ShadeIn& s, const float* theta, const rm::Table& tab, rm::V3 g, "
        "rm::ShadeGrad& gs, float* gtheta, rm::TableGrad& gt) { gt.row[0] = 0; gt.g[0] = g; }\n")
PROBE = ("template <bool Fast> RM_DEV rm::V3 NAME_probe(int k, const rm::ShadeIn& s, const float* theta) { return s.p; }\n"
         "template <bool Fast> RM_DEV void NAME_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, rm::V3 gq, rm::ShadeGrad& gs, "
         "float* gtheta) { gs.p = gs.p + gq; }\n")
FINISH = ("template <bool Fast> RM_DEV rm::V3 NAME_finish(rm::V3 raw, float lo, float hi, const float* theta) { return raw; }\n"
          "template <bool Fast> RM_DEV void NAME_finish_vjp(rm::V3 raw, float lo, float hi, const float* theta, rm::V3 g, rm::V3& graw, "
          "float& glo, float& ghi, float* gtheta) { graw = g; }\n")


def test_registration_errors():
    from ray_marching_amd import extensions as E
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.scene.primitives import SDFSphere

    def fresh(table=None):
        class S(nn.Module):
            def __init__(self):
                super().__init__()
                if table is not None:
                    self.palette = table

            def forward(self, px_coords, camera_orientation, pixel_frames, ray_directions, surface_coords, surface_normals):
                return surface_normals
        return S

    src = lambda name, *parts: "".join(parts).replace("NAME", name)
    for taps in (0, 5, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="table_taps must be an int from 1 to"):
            E.register_shader(fresh(), hip=src("tt_taps", TFWD, TVJP), table="palette", table_taps=taps)
    with pytest.raises(ValueError, match="table_taps=2 without table="):
        E.register_shader(fresh(), hip=src("tt_alone", TFWD, TVJP), table_taps=2)
    with pytest.raises(ValueError, match="table must name the attribute"):
        E.register_shader(fresh(), hip=src("tt_name", TFWD, TVJP), table=3, table_taps=1)
    with pytest.raises(ValueError, match="not built yet"):
        E.register_shader(fresh(), hip=src("tt_probes", TFWD, TVJP, PROBE), probes=2, table="palette", table_taps=1)
    with pytest.raises(ValueError, match="not built yet"):
        E.register_shader(fresh(), hip=src("tt_norm", TFWD, TVJP, FINISH), normalise="minmax", table="palette", table_taps=1)
    with pytest.raises(ValueError, match="must not be listed in params"):
        E.register_shader(fresh(), params=("palette",), hip=src("tt_param", TFWD, TVJP), table="palette", table_taps=1)
    # a source whose pair lacks tab / gt -- and one that takes them without a table
    with pytest.raises(ValueError, match=r"const rm::Table& tab.*found tab: False, gt: False"):
        E.register_shader(fresh(), hip=src("tt_plain", FWD, VJP), table="palette", table_taps=1)
    with pytest.raises(ValueError, match=r"found tab: False, gt: True"):
        E.register_shader(fresh(), hip=src("tt_half", FWD, TVJP), table="palette", table_taps=1)
    with pytest.raises(ValueError, match="no table= was given"):
        E.register_shader(fresh(), hip=src("tt_unasked", TFWD, TVJP))
    assert not any(s.name.startswith("tt_") for s in E._registry.values())
    # a second registration must repeat both fields
    cls = fresh()
    E.register_shader(cls, hip=src("tt_twice", TFWD, TVJP), table="palette", table_taps=2)
    E.register_shader(cls, hip=src("tt_twice", TFWD, TVJP), table="palette", table_taps=2)
    spec = E.shader_spec(cls())
    assert (spec.table, spec.table_taps, spec.probes, spec.normalise) == ("palette", 2, 0, None)
    with pytest.raises(ValueError, match=r"already registered with different.*table_taps=2 before.*table_taps=3 now"):
        E.register_shader(cls, hip=src("tt_twice", TFWD, TVJP), table="palette", table_taps=3)
    with pytest.raises(ValueError, match=r"already registered with different.*table='palette'.*table='lut'"):
        E.register_shader(cls, hip=src("tt_twice", TFWD, TVJP), table="lut", table_taps=2)
    # the instance's attribute
    bad = {"missing": (None, "missing or no tensor"), "float64": (torch.zeros(4, 3, dtype=torch.float64), "float32, not torch.float64"),
           "flat": (torch.zeros(12), r"\[L, 3\]"), "wide": (torch.zeros(4, 4), r"\[L, 3\]"), "short": (torch.zeros(1, 3), "2 <= L <= 4096"),
           "long": (torch.zeros(4097, 3), "2 <= L <= 4096"), "strided": (torch.zeros(3, 8).t()[:, :3], "contiguous")}
    for k, (table, match) in bad.items():
        c = fresh(table)
        E.register_shader(c, hip=src(f"tt_attr_{k}", TFWD, TVJP), table="palette", table_taps=1)
        with pytest.raises(ValueError, match=match):
            E.shader_table(c(), E.shader_spec(c()))
    for table in (torch.zeros(2, 3), torch.zeros(4096, 3), nn.Parameter(torch.zeros(7, 3))):
        c = fresh(table)
        E.register_shader(c, hip=src(f"tt_ok_{table.shape[0]}", TFWD, TVJP), table="palette", table_taps=1)
        assert E.shader_table(c(), E.shader_spec(c())) is table
    # a Parameter table is no part of theta: shader_parameters exempts it, any other stray parameter is still refused
    shader = depth_palette()
    spec = E.shader_spec(shader)
    assert spec.params == ("density",) and [n for n, _ in shader.named_parameters()] == ["density", "palette"]
    assert E.shader_parameters(shader, spec) == [shader.density]
    cs = compile_scene(SDFSphere(0.5), shader)
    assert cs.n_params == 2 and cs.leaf_names[-1] == "shader.density" and all(p is not shader.palette for p in cs.leaves)
    shader.stray = nn.Parameter(torch.zeros(1))
    with pytest.raises(ValueError, match="not all of the shader's parameters"):
        E.shader_parameters(shader, spec)


PARENT_DEPTH_CUE_HEADER_SHA1 = "91fb47ec11121b7146ab3caae3bdd24be3a2cf92"     # code_header(scene 2, DepthCueShader()) at the commit before lookup tables


def test_code_header_and_signature():
    from ray_marching_amd import specialize
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.contrib import DepthCueShader
    scene = _scenes()["scene2"]
    cs = compile_scene(scene(), depth_palette())
    assert (cs.user_shader_table, cs.user_shader_table_taps, cs.user_shader_probes, cs.user_shader_normalise) == ("palette", 2, 0, None)
    assert cs.signature[-1] == ("table", "palette", 2)
    text = specialize.code_header(cs)
    assert "#define RM_USER_SHADER_TABLE 1\n#define RM_USER_SHADER_TABLE_TAPS 2\n" in text
    assert ("template <bool Fast> RM_DEV V3 user_shader_fwd(const ShadeIn& s, const float* theta, const Table& tab) {\n"
            "  return depth_palette_fwd<Fast>(s, theta, tab);\n}\n") in text
    assert ("template <bool Fast> RM_DEV void user_shader_vjp(const ShadeIn& s, const float* theta, const Table& tab, V3 g, ShadeGrad& gs, "
            "float* gtheta, TableGrad& gt) {\n  depth_palette_vjp<Fast>(s, theta, tab, g, gs, gtheta, gt);\n}\n") in text
    # L and the values are run-time: one library for every palette
    assert specialize.scene_hash(compile_scene(scene(), depth_palette(5))) == specialize.scene_hash(cs)
    assert specialize.scene_hash(compile_scene(scene(), tangent_palette(ramp(4)))) != specialize.scene_hash(cs)
    # a shader without a table: the header the parent commit generated, byte for byte
    plain = compile_scene(scene(), DepthCueShader())
    assert (plain.user_shader_table, plain.user_shader_table_taps) == ("", 0) and "table" not in str(plain.signature)
    assert "TABLE" not in specialize.code_header(plain)
    assert hashlib.sha1(specialize.code_header(plain).encode()).hexdigest() == PARENT_DEPTH_CUE_HEADER_SHA1


def _rows_of(lines, library, skip=()):
    return [" ".join(l.split()[1:]) for l in lines if l.split()[:1] == [library] and not l.split()[1].startswith(skip)]


def test_libraries_cross_compile_and_existing_kernels_keep_their_resources():
    """The specialised libraries of (scene 2, each new shader) cross-compile for gfx950 and report T; the compiler's
    kernel-resource-usage remarks of every frame and backward kernel of (scene 2, DepthCueShader) are the parent commit's
    (profiles/user_shader_table_parent_depth_cue.txt: registers, spills, scratch, occupancy, LDS) -- the evidence that libraries
    without a table did not get slower -- and no kernel of the new libraries, nor k_table_scatter, uses scratch.  The committed
    table is what this tree compiles to."""
    from ray_marching_amd import _abi, specialize
    from ray_marching_amd.compiler import compile_scene
    if specialize._hipcc() is None or not os.path.exists(specialize._hipcc()):
        pytest.skip("hipcc not available on this box")
    assert _abi.lib.rm_user_shader_table() == 0 and {"rm_user_shader_table", "rm_table_scatter", "rm_render_backward_table"} <= set(_abi.EXPORTED_SYMBOLS)
    for make, taps in ((depth_palette, 2), (tangent_palette, 1)):
        lib = compile_scene(_scenes()["scene2"](), make()).lib()
        assert lib.rm_user_shader_table() == taps and lib.rm_user_shaders() == 1
    assert compile_scene(_scenes()["scene2"](), depth_cue()).lib().rm_user_shader_table() == 0
    spec = importlib.util.spec_from_file_location("_table_resources", os.path.join(ROOT, "profiles", "user_shader_table_resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines, bad = mod.table(list(mod.LIBS))
    print("\n".join(lines))
    assert not bad, bad
    assert any(l.split()[:2] == ["depth_palette", "k_table_scatter"] for l in lines)
    read = lambda name: [l for l in open(os.path.join(ROOT, "profiles", name)).read().splitlines() if l and not l.startswith("#")]
    parent = read("user_shader_table_parent_depth_cue.txt")
    assert len(_rows_of(parent, "depth_cue")) >= 12
    assert _rows_of(lines, "depth_cue", skip=("k_table_scatter",)) == _rows_of(parent, "depth_cue")
    assert lines == read("user_shader_table_resource_usage.txt")


@functools.lru_cache(maxsize=None)
def cpu_reference(leg, edited=False, dtype=torch.float32):
    """CPU autograd of one backward leg of DepthPaletteShader on scene 2 (the legs, weights and loss of test_user_shader; the pose of the
    first leg is two_cameras_inside),
    computed once: (density gradient, palette gradient, scene gradients in named_parameters() order, dL/dq, dL/dt)."""
    h, w, steps, pose = BACKWARD_LEGS[leg]
    shader = depth_palette()
    if edited:
        _edit(shader)
    shader = shader.to(dtype)
    q, t = pose()
    q, t = q.to(dtype).requires_grad_(True), t.to(dtype).requires_grad_(True)
    spec = O.map_spec(O.scene_test2(dtype), lambda x: x.clone().requires_grad_(True))
    bufs = tuple(b.to(dtype) for b in _bufs(q.shape[0], h, w))
    mp = pytest.MonkeyPatch()
    try:
        img = cpu_frame(spec, shader, mp, bufs, q, t, steps)
    finally:
        mp.undo()
    _loss(img, _weights(q.shape[0], h, w, 7).to(dtype)).backward()
    return shader.density.grad, shader.palette.grad, [p.grad for _, p in O.spec_parameters(spec)], q.grad, t.grad


def _edit(shader):
    """An in-place edit of the palette and of the density (the same on the CPU and the GPU copy)."""
    with torch.no_grad():
        shader.palette.mul_(0.8).add_(0.1 * torch.sin(3.0 * torch.linspace(0.0, 1.0, shader.palette.shape[0], device=shader.palette.device))[:, None])
        shader.density.mul_(1.25)


@pytest.mark.parametrize("leg", sorted(BACKWARD_LEGS))
def test_cpu_reference_is_well_inside_the_tolerance(leg):
    """Before the GPU is asked for 1e-4: the oracle's own fp32 and fp64 gradients of the DepthPaletteShader legs agree within 1e-5
    (the interpolation's slope jumps at the knots; the palette is short and smooth so that a pixel that rounds across a knot moves
    nothing), density's gradient is not small, and neither are the gradients of the palette rows the frame reaches.  (u = (L - 1) /
    (1 + density |o - p|) spans a ratio of at most max|o - p| / min|o - p|, so no pose reaches all 16 rows: the rows it does not
    reach have gradient exactly 0, which the GPU must reproduce.)"""
    for edited in (False, True):
        g32, g64 = cpu_reference(leg, edited), cpu_reference(leg, edited, torch.float64)
        flat = lambda g: torch.cat([g[0].reshape(-1).double(), g[1].reshape(-1).double()] + [x.reshape(-1).double() for x in g[2] if x is not None]
                                   + [g[3].reshape(-1).double(), g[4].reshape(-1).double()])
        err = (flat(g32) - flat(g64)).abs().max().item()
        hit = g32[1].abs().sum(dim=1) > 0
        print(f"depth_palette {leg} edited={edited}: fp32 vs fp64 max|diff| {err:.3g}; density grad {g32[0].item():.4g}; "
              f"{int(hit.sum())} rows reached, largest |palette grad| per reached row {g32[1][hit].abs().amax(dim=1).tolist()}")
        assert err <= 1e-5
        assert abs(g32[0].item()) >= 1e-2 and int(hit.sum()) >= 3 and g32[1].abs().max().item() >= 1e-2
        assert bool(torch.isfinite(flat(g32)).all())


def test_cpu_gradients_of_the_tangent_palette_are_not_small():
    """TangentPaletteShader's PyTorch forward on the 32x32x16 leg with a palette of 8 rows: every entry of the palette's autograd
    gradient is at least 1e-2 (every row is reached by a few hundred pixels)."""
    h, w, steps = 32, 32, 16
    shader = tangent_palette(smooth_palette(8))
    q, t = two_cameras()
    mp = pytest.MonkeyPatch()
    try:
        img = cpu_frame(O.scene_test2(), shader, mp, _bufs(2, h, w), q, t, steps)
    finally:
        mp.undo()
    _loss(img, _weights(2, h, w, 7)).backward()
    g = shader.palette.grad
    print(f"tangent_palette: CPU palette grad {g.tolist()}")
    assert bool(torch.isfinite(g).all()) and g.abs().min().item() >= 1e-2


def test_tangent_palette_cpu_forward_is_the_oracles_tangent_mode(monkeypatch):
    """With the float32 cast of the reference's colormap as its palette, the shader's PyTorch forward equals the oracle's mode-6
    shade computed with that float32 colormap (degree 1), on scene 2 and on closed scene 1."""
    cmap = cmap32()
    shader = tangent_palette(cmap)
    for spec, z in ((O.scene_test2(), -3.0), (O.scene_test1_closed(), -1.5)):
        q, t = two_cameras(z)
        with torch.no_grad():
            want = O.render(spec, _bufs(2, 24, 40), q, t, 6, 1, 32, H.EPS, cmap=cmap)
            got = cpu_frame(spec, shader, monkeypatch, _bufs(2, 24, 40), q, t, 32)
        assert got.dtype == torch.float32 and got.shape == want.shape and _same(got, want)
        assert want.unique(dim=0).numel() > 100


# --------------------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------------------
def _exact_scatter(loop, shader, q, t, steps, monkeypatch, want_deferred=False):
    """One leg of test_exact_scatter; returns (row indices [n,h,w], table gradient) after asserting the gradient exact.  A UTableLit
    adds a term in [0, 1] to the row: its indices are recovered from the table row r = (4 r, 4 r, 4 r)."""
    from ray_marching_amd import _abi, ops
    L = shader.palette.shape[0]
    n, h, w = q.shape[0], loop.px_height, loop.px_width
    with torch.no_grad():
        lit = isinstance(shader, UTableLit)
        shader.palette.copy_(ramp(L) * (4 if lit else 1))
        index_image = loop(q, t, shader, 1, steps)
        idx = (index_image[..., 0] / 4).floor().long() if lit else index_image[..., 0].long()
        assert bool(torch.isfinite(index_image).all())
        if lit:
            extra = index_image - 4 * idx.float()[..., None]
            assert float(extra.min()) >= 0 and float(extra.max()) <= 1 and _same(index_image[..., 0], index_image[..., 2])
        else:
            assert _same(index_image, idx.float()[..., None].expand(n, h, w, 3))
        assert int(idx.min()) >= 0 and int(idx.max()) <= L - 1
        gen = torch.Generator().manual_seed(L + h)
        shader.palette.copy_(torch.rand(L, 3, generator=gen))
    weights = torch.randint(-8, 9, (n, h, w, 3), generator=gen).float().to(DEV)
    shader.palette.grad = None
    before = ops.table_scatter_calls
    sink = torch.zeros(int(ops._lib.rm_wave_tiles(n, h, w, 2)), dtype=torch.int32, device=DEV)
    monkeypatch.setattr(ops, "bwd_tile_cost_sink", sink)          # (measurement hook: keeps the backward's workspace)
    image = loop(q, t, shader, 1, steps)
    if not lit:
        assert _same(image.detach(), shader.palette.detach()[idx])
    (image * weights).sum().backward()
    torch.cuda.synchronize()
    deferred = int(ops.bwd_last_work[32])
    monkeypatch.setattr(ops, "bwd_tile_cost_sink", None)
    assert ops.table_scatter_calls == before + 1
    if want_deferred:
        assert deferred > 0, "no ray was deferred: the leg does not exercise the deferred rule"
    want = torch.zeros(L, 3, device=DEV).index_add_(0, idx.reshape(-1), weights.reshape(-1, 3))
    got = shader.palette.grad
    hits = torch.bincount(idx.reshape(-1), minlength=L)
    chunks = (n * h * w + _abi.TABLE_CHUNK - 1) // _abi.TABLE_CHUNK
    print(f"L={L} {n}x{h}x{w}: {n * h * w} records in {chunks} chunks, {int((hits > 0).sum())} rows hit (most: {int(hits.max())} times), "
          f"{deferred} rays deferred, max|got - want| {(got - want).abs().max().item():.3g}")
    assert got.shape == (L, 3) and torch.equal(got, want)
    assert bool((got[hits == 0] == 0).all())
    return idx, got


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [2, 4096])
@pytest.mark.parametrize("regen", [False, True])
def test_exact_scatter(rows, regen, monkeypatch):
    """Two cameras at 60x44 (partial wave tiles, lanes without a pixel; 5280 records: three scatter chunks, the last one partial),
    with L = 2 (up to 64 lanes of a wave on one row) and L = 4096 (most lanes on different rows, the largest LDS table), the row
    indices recovered through the tile kernel and through the ray pools: the table's gradient EQUALS index_add of the integer
    weights, and rows no pixel hit have gradient exactly 0."""
    from ray_marching_amd import _abi
    _register()
    h, w, steps = 44, 60, 32
    assert 2 * h * w > 2 * _abi.TABLE_CHUNK and (2 * h * w) % _abi.TABLE_CHUNK != 0       # at least three chunks, the last partial
    scene = _scenes()["scene2"]().to(DEV)
    shader = UTableRow(ramp(rows)).to(DEV)
    q, t = two_cameras()
    idx, grad = _exact_scatter(H.make_loop(scene, h, w, n=2, regen=regen), shader, q.to(DEV), t.to(DEV), steps, monkeypatch)
    hits = torch.bincount(idx.reshape(-1), minlength=rows)
    if rows == 2:
        assert int(hits.min()) > 64
    else:
        assert int((hits > 0).sum()) > 500 and int((hits == 0).sum()) > 0


@pytest.mark.gpu
def test_exact_scatter_with_deferred_rays_and_tables_that_want_no_gradient(monkeypatch):
    """From inside the torus at 40x24x32, where rays are deferred (asserted; the shader here adds the Lambertian term to the row, so
    that the scene has a gradient for the reverse march to carry): the shader's VJP runs in the fused kernel for those rays too,
    and the table's gradient is exact.  Then the tables that want no gradient -- a Parameter with requires_grad=False, and a
    registered buffer: the pose still gets its gradient, the table gets no ``.grad``, and no scatter is launched."""
    from ray_marching_amd import ops
    _register()
    h, w, steps, pose = BACKWARD_LEGS["deferred_40x24x32"]
    scene = _scenes()["scene2"]().to(DEV)
    q, t = pose()
    q, t = q.to(DEV), t.to(DEV)
    loop = H.make_loop(scene, h, w, n=1)
    _exact_scatter(loop, UTableLit(ramp(64)).to(DEV), q, t, steps, monkeypatch, want_deferred=True)
    shader = UTableRow(torch.rand(64, 3, generator=torch.Generator().manual_seed(9))).to(DEV)
    weights = torch.randint(-8, 9, (1, h, w, 3), generator=torch.Generator().manual_seed(5)).float().to(DEV)
    frozen = UTableRow(shader.palette.detach()).to(DEV)
    frozen.palette.requires_grad_(False)
    buffered = UTableBuffer(shader.palette.detach()).to(DEV)
    for other in (frozen, buffered):
        before = ops.table_scatter_calls
        qg = q.clone().requires_grad_(True)
        image = loop(qg, t, other, 1, steps)
        assert _same(image.detach(), loop(q, t, shader, 1, steps).detach())
        (image * weights).sum().backward()
        assert ops.table_scatter_calls == before and other.palette.grad is None
        assert qg.grad is not None and bool(torch.isfinite(qg.grad).all())


@pytest.mark.gpu
def test_two_backwards_give_the_same_bits():
    """Two backwards of the same DepthPaletteShader frame (two cameras, 60x44x32): torch.equal gradients of the palette and of density."""
    h, w, steps = 44, 60, 32
    scene = _scenes()["scene2"]().to(DEV)
    shader = depth_palette().to(DEV)
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    wts = _weights(2, h, w, 7).to(DEV)
    loop = H.make_loop(scene, h, w, n=2)
    grads = []
    for _ in range(2):
        shader.palette.grad = shader.density.grad = None
        _loss(loop(q, t, shader, 1, steps), wts).backward()
        grads.append((shader.palette.grad.clone(), shader.density.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert grads[0][0].abs().max().item() > 1e-2 and abs(grads[0][1].item()) > 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scene2", "closed_scene1"])
def test_tangent_palette_is_bit_identical_with_the_builtin_tangent_mode(which, monkeypatch):
    """TangentPaletteShader with the float32 cast of the reference's colormap against mode 6 (degree 1) on a loop whose
    Shader.cyclic_cmap is that same tensor: the 60x44x32 frames of two cameras are the same bits through the tile kernel, the ray
    pools, a captured replay and display_frame, and so are the scene-parameter and pose gradients of an MSE loss over a 32x32x16
    frame (every ray walked in place, as in test_restated_builtin_shader_is_bit_identical_with_the_builtin_mode)."""
    from ray_marching_amd import ops
    monkeypatch.setattr(ops, "bwd_hard_capacity", 0)
    cmap = cmap32().to(DEV)
    shader = tangent_palette(cmap).to(DEV)
    scene = _scenes()[which]().to(DEV)
    h, w, steps = 44, 60, 32
    q, t = two_cameras(-3.0 if which == "scene2" else -1.5)
    q, t = q.to(DEV), t.to(DEV)

    def loop_of(h, w, n, **kw):
        loop = H.make_loop(scene, h, w, n=n, **kw)
        loop.shader.cyclic_cmap = cmap
        return loop

    with torch.no_grad():
        for kw in (dict(), dict(regen=True)):
            loop = loop_of(h, w, 2, **kw)
            want = loop(q, t, 6, 1, steps)
            got = loop(q, t, shader, 1, steps)
            assert got.shape == (2, h, w, 3) and got.dtype == want.dtype == torch.float32 and _same(got, want), kw
            assert _same(loop.capture(mode=shader, marching_steps=steps)(q, t), got), kw
        one = loop_of(h, w, 1)
        assert _same(one.display_frame(q[1:], t[1:], shader, 1, steps), one.display_frame(q[1:], t[1:], 6, 1, steps))
        assert want.reshape(-1, 3).unique(dim=0).shape[0] > 100
    h, w, steps = 32, 32, 16
    target = torch.rand(2, h, w, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    grads = {}
    for key, m in (("builtin", 6), ("twin", shader)):
        loop = loop_of(h, w, 2)
        for x in scene.parameters():
            x.grad = None
        qg, tg = q.clone().requires_grad_(True), t.clone().requires_grad_(True)
        (loop(qg, tg, m, 1, steps) - target).pow(2).mean().backward()
        grads[key] = [x.grad.clone() for x in scene.parameters()] + [qg.grad, tg.grad]
    names = [n for n, _ in scene.named_parameters()] + ["orientations", "translations"]
    for name, a, b in zip(names, grads["twin"], grads["builtin"]):
        print(f"{which}: grad {name} max|diff| {(a - b).abs().max().item():.3g} (|g| {b.abs().max().item():.3g})")
    for name, a, b in zip(names, grads["twin"], grads["builtin"]):
        assert _same(a, b), name
    assert any(float(g.abs().max()) > 0 for g in grads["builtin"][-2:]) and shader.palette.grad is not None


@pytest.mark.gpu
def test_depth_palette_against_the_cpu(monkeypatch):
    """DepthPaletteShader on scene 2 against the oracle with the shader's PyTorch forward as its shade(), in the harness and at the
    tolerances of test_user_shader.test_contrib_shader_against_the_cpu: the 60x44x32 frame of two cameras <= 1e-5 (tile kernel and
    ray pools), the gradients of the scene parameters, the pose, density and EVERY palette entry <= 1e-4 at 32x32x16 with two
    cameras and at 40x24x32 from inside the torus, where rays are deferred (asserted); then again after an in-place edit of the
    palette and of density."""
    from ray_marching_amd import ops
    shader, cpu_shader = depth_palette().to(DEV), depth_palette()
    scene = _scenes()["scene2"]().to(DEV)
    h, w, steps = 44, 60, 32
    q, t = two_cameras()
    with torch.no_grad(), O.math_mode("restated"):
        want = cpu_frame(O.scene_test2(), cpu_shader, monkeypatch, _bufs(2, h, w), q, t, steps)
    with torch.no_grad():
        for kw in (dict(), dict(regen=True)):
            got = H.make_loop(scene, h, w, n=2, **kw)(q.to(DEV), t.to(DEV), shader, 1, steps).cpu()
            err, frac = H.report("depth_palette frame", got, want)
            print(f"depth_palette {kw}: frame max|err| {err:.3g}, {frac:.3g} of the values beyond 1e-5")
            assert got.shape == (2, h, w, 3) and err <= 1e-5
    for edited in (False, True):
        if edited:
            _edit(shader)
        for leg, (h, w, steps, pose) in BACKWARD_LEGS.items():
            want_density, want_palette, want_scene, want_q, want_t = cpu_reference(leg, edited)
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
            print(f"depth_palette {leg} edited={edited}: {deferred} rays deferred")
            if leg.startswith("deferred"):
                assert deferred > 0, "no ray was deferred: the leg does not exercise the deferred rule"
            bad = []
            pairs = [("density", shader.density.grad, want_density), ("palette", shader.palette.grad, want_palette)]
            pairs += [(name, p.grad, c if c is not None else torch.zeros_like(p.grad.cpu())) for (name, p), c in zip(scene.named_parameters(), want_scene)]
            pairs += [("orientations", qg.grad, want_q), ("translations", tg.grad, want_t)]
            for name, g, c in pairs:
                assert g is not None and bool(torch.isfinite(g).all()), name
                e = (g.cpu() - c).abs().max().item()
                print(f"depth_palette {leg} edited={edited}: grad {name} max|err| {e:.3g} (|g| {c.abs().max().item():.3g})")
                if not e <= 1e-4:
                    bad.append(name)
            assert not bad, (leg, edited, bad)
            unreached = want_palette.abs().sum(dim=1) == 0
            assert bool(unreached.any()) and bool((shader.palette.grad.cpu()[unreached] == 0).all())


@pytest.mark.gpu
def test_training_step_moves_a_perturbed_palette_back():
    """Eight Adam steps of a captured training step (64x64x32, scene 2) over the palette ALONE, towards a frame rendered with the
    unperturbed palette: each replayed step gives the loss of the eager step taken from the same palette (1e-6 max(1, |loss|)), the
    palette ends nearer the one that rendered the target, and the loss falls.  The palette's ``.grad`` is a static buffer of the graph."""
    h, w, steps = 64, 64, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    truth = smooth_palette()
    with torch.no_grad():
        target = H.make_loop(_scenes()["scene2"]().to(DEV), h, w, n=2)(q, t, depth_palette().to(DEV), 1, steps).clone()
    loss_fn = lambda image: (image - target).pow(2).mean()

    def perturbed():
        shader = depth_palette().to(DEV)
        with torch.no_grad():
            shader.palette += 0.2 * torch.cos(5.0 * torch.arange(48, device=DEV, dtype=torch.float32)).reshape(16, 3)
        shader.density.requires_grad_(False)
        return shader

    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*AccumulateGrad node's stream does not match.*")
        scene, shader = _scenes()["scene2"]().to(DEV), perturbed()
        for x in scene.parameters():
            x.requires_grad_(False)
        loop = H.make_loop(scene, h, w, n=2)
        with torch.no_grad():
            reached = (loop(q, t, shader, 1, steps) - target).abs().sum() > 0
        assert bool(reached)
        before = (shader.palette.detach().cpu() - truth).norm().item()
        opt = torch.optim.Adam([shader.palette], lr=2e-2, capturable=True)
        step = loop.training_step(loss_fn, mode=shader, marching_steps=steps, optimizer=opt)
        twin_scene, twin = _scenes()["scene2"]().to(DEV), perturbed()
        twin_loop = H.make_loop(twin_scene, h, w, n=2)
        with torch.no_grad():
            first = float(loss_fn(loop(q, t, shader, 1, steps)))
        for it in range(8):
            if it == 0:
                step(q, t)                                   # warm-up iterations, the capture, one replay
                grad_buffer = shader.palette.grad
            with torch.no_grad():
                twin.palette.copy_(shader.palette)
            got = float(step(q, t))
            want = loss_fn(twin_loop(q, t, twin, 1, steps))
            want.backward()
            twin.palette.grad = None
            assert abs(got - float(want.detach())) <= 1e-6 * max(1.0, abs(float(want.detach()))), (it, got, float(want.detach()))
            assert shader.palette.grad is grad_buffer
        with torch.no_grad():
            last = float(loss_fn(loop(q, t, shader, 1, steps)))
        after = (shader.palette.detach().cpu() - truth).norm().item()
        print(f"palette training: loss {first:.4g} -> {last:.4g}, |palette - truth| {before:.4g} -> {after:.4g}")
        assert last < first and after < before
        assert shader.density.grad is None and all(x.grad is None for x in scene.parameters())


@pytest.mark.gpu
def test_table_shader_tableless_shader_and_builtin_mode_in_alternation():
    """One scene, one RenderLoop; DepthPaletteShader, DepthCueShader (no table) and mode 0 in turn, twice: each frame is the bits of
    its own render on a loop of its own, so the table in the colormap slot does not bleed into the frames that have none.  An
    in-place edit of the palette is seen by the next frame and by the next replay of a captured one."""
    h, w, steps = 44, 60, 32
    q, t = two_cameras()
    q, t = q.to(DEV), t.to(DEV)
    modes = {"depth_palette": depth_palette().to(DEV), "depth_cue": depth_cue().to(DEV), "lambertian": 0}
    fresh = {"depth_palette": lambda: depth_palette().to(DEV), "depth_cue": lambda: depth_cue().to(DEV), "lambertian": lambda: 0}
    with torch.no_grad():
        want = {k: H.make_loop(_scenes()["scene2"]().to(DEV), h, w, n=2)(q, t, fresh[k](), 1, steps) for k in modes}
        loop = H.make_loop(_scenes()["scene2"]().to(DEV), h, w, n=2)
        for rnd in range(2):
            for k, m in modes.items():
                assert _same(loop(q, t, m, 1, steps), want[k].expand(2, h, w, 3)), (rnd, k)
        assert not _same(want["depth_palette"], want["depth_cue"].expand(2, h, w, 3))
        shader = modes["depth_palette"]
        captured = loop.capture(mode=shader, marching_steps=steps)
        assert _same(captured(q, t), want["depth_palette"])
        edited = depth_palette().to(DEV)
        _edit(shader)
        _edit(edited)
        again = H.make_loop(_scenes()["scene2"]().to(DEV), h, w, n=2)(q, t, edited, 1, steps)
        assert not _same(again, want["depth_palette"])
        assert _same(loop(q, t, shader, 1, steps), again) and _same(captured(q, t), again)
