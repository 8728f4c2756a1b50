"""The stand-alone surface -- scene(points), PinholeCamera, SDFMarcher, SDFNormals and the shader modules with a VJP -- and the
kernels behind its gradients (k_sdf_bwd, the recording k_march_fwd, k_march_bwd, k_normals_bwd, k_camera_bwd + _finish,
k_shade_bwd, k_reduce_partials) at ragged counts and edges: partial last waves and blocks, the grid-stride loops, trajectories
the early-out cut short, NaN rays, broadcast and fp16 inputs, empty inputs, and every choice of who asks for a gradient.

Every one of these kernels runs a lane with i >= n as a clone of ray n - 1 with zero upstream; nothing but a parameter
gradient can show a clone that contributes, so every case checks every parameter gradient.

References, computed on the CPU next to each device call: autograd on oracle.sdf_oracle in float32 and in float64.  Forward
values must equal the float32 oracle (its `restated` arithmetic) bit for bit, NaN and inf positions included, and are checked
before any gradient, so that no gradient is compared across two trajectories.  Gradients meet helpers.gradient_contract:
min(|got - g32|, |got - g64|) <= 1e-4 max(1, |g64|max), NaN exactly where the float32 oracle has NaN (point gradients of
scene(points): 1e-5, absolute).  Nothing here compiles: scene 2 and closed scene 1 run through their prebuilt specialised
libraries and through the interpreter, every other scene through the interpreter, and each case asserts which it ran on.
"""
import functools
import math

import pytest
import torch

from oracle import sdf_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda"

SOFT = "smooth_union_soft"
NODE_KINDS = ["sphere", "box", "plane", "line", "disk", "torus", "affine", "rounding", "onion", "union", "smooth_union"]
PREBUILT = {"scene2": O.scene_test2, "scene1_closed": O.scene_test1_closed}
CAMERA_AT = {"scene2": (0.0, 0.0, -3.0), "scene1_closed": (0.1, 0.0, -1.0)}
PATHS = ["interpreter", "specialised"]
BWD_BLOCK, BWD_GRID = 128, 1024       # rm_abi.hip: the backward grid is capped at 1024 blocks of at most 128 threads,
FWD_BLOCK, FWD_GRID = 256, 2048       # the forward grid at kMaxBlocks = 2048 blocks of at most 256
N_STRIDE_BWD = BWD_BLOCK * BWD_GRID + 65      # with the largest block there are already more tiles than blocks, so some block
N_STRIDE_FWD = FWD_BLOCK * FWD_GRID + 65      # takes a second tile (a smaller block only makes more tiles)
assert -(-N_STRIDE_BWD // BWD_BLOCK) > BWD_GRID and -(-N_STRIDE_FWD // FWD_BLOCK) > FWD_GRID


# --------------------------------------------------------------------------
# which library, references, comparisons
# --------------------------------------------------------------------------
@pytest.fixture
def library(monkeypatch):
    """library("specialised"): the prebuilt per-scene libraries; library("interpreter"): librm_hip.so."""
    from ray_marching_amd import specialize

    def choose(path):
        assert path in PATHS
        monkeypatch.setenv("RM_SPECIALIZE", "off" if path == "interpreter" else "auto")
        specialize._loaded.clear()

    yield choose
    specialize._loaded.clear()


def ran_on(module, path):
    """Assert the library the forward and the backward kernels of ``module`` take."""
    from ray_marching_amd import _abi
    from ray_marching_amd.compiler import compiled_for
    cs = compiled_for(module)
    for backward in (False, True):
        lib = cs.lib(backward)
        if path == "specialised":
            assert lib is not _abi.lib, "specialised library missing: __graft_entry__.build() makes it"
        else:
            assert lib is _abi.lib
    return cs


def scene_spec(name):
    if name == SOFT:
        return ("smooth_union", {"blend_k": O._t(1.0)}, H.node_specs()["smooth_union"][2])
    if name.startswith("many"):
        return O.scene_many(int(name[4:]))
    return H.node_specs()[name]


def on_device(spec, path, library, half=False):
    library(path)
    module = H.spec_to_module(spec).to(DEV)
    if half:
        module = module.half()
    ran_on(module, path)
    assert [k for k, _ in module.named_parameters()] == [k for k, _ in O.spec_parameters(spec)]
    return module


def cpu_grads(spec, inputs, forward, upstreams, dtype):
    """Autograd on the oracle in ``dtype``: loss = sum over the outputs of (out * upstream).sum().
    -> (outputs, input gradients, [(name, parameter gradient)]); a gradient nobody reached is zero."""
    s = O.map_spec(spec, lambda x: x.detach().to(dtype).clone().requires_grad_(True))
    xs = [x.detach().to(dtype).clone().requires_grad_(True) for x in inputs]
    outs = forward(s, *xs)
    sum((o * u.to(dtype)).sum() for o, u in zip(outs, upstreams) if u is not None).backward()

    def grad(t):
        return t.grad if t.grad is not None else torch.zeros_like(t)

    return [o.detach() for o in outs], [grad(x) for x in xs], [(k, grad(p)) for k, p in O.spec_parameters(s)]


def both_references(spec, inputs, forward, upstreams):
    return (cpu_grads(spec, inputs, forward, upstreams, torch.float32), cpu_grads(spec, inputs, forward, upstreams, torch.float64))


def dev_grads(module, inputs, forward, upstreams, input_grad=True):
    """The same loss on the device.  -> (outputs, input gradients, [(name, parameter .grad)])."""
    for p in module.parameters():
        p.grad = None
    xs = [x.detach().to(DEV).clone().requires_grad_(input_grad) for x in inputs]
    outs = forward(*xs)
    sum((o * u.to(DEV).to(o.dtype)).sum() for o, u in zip(outs, upstreams) if u is not None).backward()
    return outs, [x.grad for x in xs], [(k, p.grad) for k, p in module.named_parameters()]


def forward_equal(what, got, want):
    """Bit-equal with the float32 oracle, NaN and inf positions included."""
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    err = H.report(what, got, want)[0]
    assert err == 0.0, (what, err)


def restated(fn):
    with torch.no_grad(), O.math_mode("restated"):
        return fn()


def check_gradients(group, what, dev, refs, names, frozen=(), tol_inputs=1e-4, absolute_inputs=False):
    """Every input gradient (``names``) and every parameter gradient of ``dev`` against the two references."""
    (_, gin, gpar), ((_, a_in, a_par), (_, b_in, b_par)) = dev, refs
    for name, g, a, b in zip(names, gin, a_in, b_in):
        if name is None:
            continue
        assert g is not None and g.shape == a.shape and g.dtype == torch.float32, (what, name)
        H.gradient_contract(f"{group} inputs", f"{what} {name}", g, a, b, tol=tol_inputs, absolute=absolute_inputs)
    assert len(gpar) == len(a_par) == len(b_par)
    for (k, g), (_, a), (_, b) in zip(gpar, a_par, b_par):
        if k in frozen:
            assert g is None, (what, k)
            continue
        assert g is not None and g.shape == a.shape, (what, k)
        H.gradient_contract(f"{group} parameters", f"{what} {k}", g, a, b)


@functools.lru_cache(maxsize=None)
def seeded_points():
    """One seeded set in [-3, 3]^3 and one set of upstream weights; every count takes the first n of it."""
    gen = torch.Generator().manual_seed(7)
    return torch.rand(N_STRIDE_FWD, 3, generator=gen) * 6 - 3, torch.randn(N_STRIDE_FWD, 1, generator=gen)


@functools.lru_cache(maxsize=None)
def camera_rays(h, w, at):
    """The rays of an h x w camera at ``at`` (identity orientation), flattened: ([h w, 3], [h w, 3]) on the CPU."""
    bufs = O.camera_buffers(1, w, h, H.PX * h, H.PX * w, H.PX * h)
    pos, _, dirs = O.camera_forward(*bufs, torch.tensor([[1.0, 0.0, 0.0, 0.0]]), torch.tensor([at]))
    return pos.reshape(-1, 3).contiguous(), dirs.reshape(-1, 3).contiguous()


def first(x, n):
    """The first n rows of x, tiled when n exceeds them."""
    return x.repeat(-(-n // x.shape[0]), 1)[:n].contiguous()


# --------------------------------------------------------------------------
# A. scene(points): k_sdf_bwd, k_reduce_partials
# --------------------------------------------------------------------------
def sdf_forward(s, p):
    return (O.sdf_eval(s, p),)


def sdf_case(what, spec, module, n, group="A"):
    pts, w = (x[:n] for x in seeded_points())
    refs = both_references(spec, [pts], sdf_forward, [w])
    dev = dev_grads(module, [pts], lambda p: (module(p),), [w])
    assert dev[0][0].shape == (n, 1)
    forward_equal(f"{what} d", dev[0][0], restated(lambda: O.sdf_eval(spec, pts)))
    check_gradients(group, what, dev, refs, ["grad_points"], tol_inputs=1e-5, absolute_inputs=True)


@pytest.mark.parametrize("name", NODE_KINDS + [SOFT, "scene1_closed", "scene2", "scene_many8"])
def test_sdf_every_node_at_a_partial_wave_and_a_partial_block(name, library):
    """65 points: one full wave and one lane of the next; 385 = 3 x 128 + 1: one lane of a fourth block."""
    spec = scene_spec(name)
    module = on_device(spec, "interpreter", library)
    for n in (65, 385):
        sdf_case(f"{name} n={n}", spec, module, n)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(PREBUILT))
def test_sdf_counts_around_every_wave_and_block_edge(name, path, library):
    spec = PREBUILT[name]()
    module = on_device(spec, path, library)
    for n in (1, 63, 64, 65, 127, 128, 129, 257, 385):
        sdf_case(f"{name} {path} n={n}", spec, module, n)


@pytest.mark.parametrize("path", PATHS)
def test_sdf_grid_stride(path, library):
    """131 072 + 65 points through the backward (more tiles than its 1024 blocks), 524 288 + 65 through the forward."""
    spec = O.scene_test2()
    module = on_device(spec, path, library)
    sdf_case(f"scene2 {path} n={N_STRIDE_BWD}", spec, module, N_STRIDE_BWD, group="A grid-stride")
    pts = seeded_points()[0]
    with torch.no_grad():
        got = module(pts.to(DEV))
    forward_equal(f"scene2 {path} n={N_STRIDE_FWD} d", got, restated(lambda: O.sdf_eval(spec, pts)))


@pytest.mark.parametrize("name,n", [("many48", 65), ("many48", 129), ("many100", 65), ("many100", 129)])
def test_sdf_wide_scenes_take_smaller_blocks(name, n, library):
    """The scenes above all get the largest block; the 48- and 100-primitive scenes get smaller ones (restated from
    GenericCfg::lds_floats and pick_launch), so their partial tiles end elsewhere.  Values bit-equal as everywhere."""
    from ray_marching_amd.compiler import compiled_for
    spec = scene_spec(name)
    module = on_device(spec, "interpreter", library)
    small = on_device(O.scene_test2(), "interpreter", library)
    blocks = {(which, back): H.generic_block(compiled_for(m), back, which)
              for which, m in ((name, module), ("scene2", small)) for back in (False, True)}
    assert blocks[("scene2", False)] == FWD_BLOCK and blocks[("scene2", True)] == BWD_BLOCK
    assert blocks[(name, False)] < FWD_BLOCK, blocks
    if name == "many100":
        assert blocks[(name, True)] < BWD_BLOCK, blocks
    assert n % blocks[(name, False)] and n % blocks[(name, True)], "no partial tile"
    sdf_case(f"{name} n={n}", spec, module, n, group="A wide")


@pytest.mark.parametrize("path", PATHS)
def test_sdf_who_asks_for_a_gradient(path, library):
    spec = O.scene_test1_closed()
    n = 129
    pts, w = (x[:n] for x in seeded_points())
    refs = both_references(spec, [pts], sdf_forward, [w])
    # points only
    module = on_device(spec, path, library)
    for p in module.parameters():
        p.requires_grad_(False)
    dev = dev_grads(module, [pts], lambda p: (module(p),), [w])
    assert all(g is None for _, g in dev[2])
    H.gradient_contract("A inputs", f"scene1_closed {path} points only", dev[1][0], refs[0][1][0], refs[1][1][0], tol=1e-5, absolute=True)
    # parameters only
    module = on_device(spec, path, library)
    dev = dev_grads(module, [pts], lambda p: (module(p),), [w], input_grad=False)
    assert dev[1][0] is None
    check_gradients("A", f"scene1_closed {path} parameters only", dev, refs, [None])
    # one parameter frozen
    module = on_device(spec, path, library)
    frozen = [k for k, p in module.named_parameters() if p.numel() == 3][0]
    dict(module.named_parameters())[frozen].requires_grad_(False)
    dev = dev_grads(module, [pts], lambda p: (module(p),), [w])
    check_gradients("A", f"scene1_closed {path} {frozen} frozen", dev, refs, ["grad_points"], frozen=(frozen,),
                    tol_inputs=1e-5, absolute_inputs=True)


@pytest.mark.parametrize("path", PATHS)
def test_sdf_layouts(path, library):
    spec = O.scene_test2()
    module = on_device(spec, path, library)
    pts, w = seeded_points()
    # a leading shape
    x, u = pts[:70].reshape(2, 5, 7, 3), w[:70].reshape(2, 5, 7, 1)
    dev = dev_grads(module, [x], lambda p: (module(p),), [u])
    assert dev[0][0].shape == (2, 5, 7, 1) and dev[1][0].shape == (2, 5, 7, 3)
    forward_equal("leading shape d", dev[0][0], restated(lambda: O.sdf_eval(spec, x)))
    check_gradients("A", f"scene2 {path} [2, 5, 7, 3]", dev, both_references(spec, [x], sdf_forward, [u]), ["grad_points"],
                    tol_inputs=1e-5, absolute_inputs=True)
    # a strided slice: a leaf that is not contiguous
    x, u = pts[:65], w[:65]
    refs = both_references(spec, [x], sdf_forward, [u])
    for p in module.parameters():
        p.grad = None
    leaf = x.repeat(1, 2).to(DEV)[:, :3].detach().requires_grad_(True)
    assert not leaf.is_contiguous()
    d = module(leaf)
    (d * u.to(DEV)).sum().backward()
    forward_equal("strided d", d, restated(lambda: O.sdf_eval(spec, x)))
    check_gradients("A", f"scene2 {path} strided", ([d], [leaf.grad], [(k, p.grad) for k, p in module.named_parameters()]), refs,
                    ["grad_points"], tol_inputs=1e-5, absolute_inputs=True)
    # one point expanded to 65: its gradient is the sum over the copies
    one = pts[:1]

    def expanded(s, o):
        return (O.sdf_eval(s, o.expand(65, 3)),)

    dev = dev_grads(module, [one], lambda o: (module(o.expand(65, 3)),), [u])
    assert dev[0][0].shape == (65, 1) and dev[1][0].shape == (1, 3)
    check_gradients("A", f"scene2 {path} expanded", dev, both_references(spec, [one], expanded, [u]), ["grad_points"])


def test_sdf_empty_input_accumulation_and_degenerate_upstreams(library):
    spec = O.scene_test2()
    module = on_device(spec, "interpreter", library)
    # [0, 3] with grad: zero gradients of the right shapes and dtypes
    x = torch.empty(0, 3, device=DEV, requires_grad=True)
    d = module(x)
    assert d.shape == (0, 1)
    d.sum().backward()
    assert x.grad.shape == (0, 3) and x.grad.dtype == torch.float32
    for k, p in module.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and not bool(p.grad.any()), k
    # two backward calls accumulate: the kernels are deterministic, so the second call adds the same bits
    pts, w = (t[:65] for t in seeded_points())
    once = dev_grads(module, [pts], lambda p: (module(p),), [w])
    once = [g.clone() for g in once[1]] + [g.clone() for _, g in once[2]]
    for p in module.parameters():
        p.grad = None
    x = pts.to(DEV).requires_grad_(True)
    for _ in range(2):
        (module(x) * w.to(DEV)).sum().backward()
    for g1, g2 in zip(once, [x.grad] + [p.grad for p in module.parameters()]):
        assert torch.equal(g2, g1 + g1)
    # an all-zero upstream: exact zeros
    dev = dev_grads(module, [pts], lambda p: (module(p),), [torch.zeros(65, 1)])
    assert not bool(dev[1][0].any()) and all(not bool(g.any()) for _, g in dev[2])
    # one NaN upstream element: that point's gradient alone is NaN, the parameter gradients as the oracle's
    u = w.clone()
    u[37] = float("nan")
    dev = dev_grads(module, [pts], lambda p: (module(p),), [u])
    rows = torch.isnan(dev[1][0]).any(dim=-1).cpu()
    assert rows.tolist() == [i == 37 for i in range(65)]
    check_gradients("A", "scene2 NaN upstream", dev, both_references(spec, [pts], sdf_forward, [u]), ["grad_points"],
                    tol_inputs=1e-5, absolute_inputs=True)


@pytest.mark.parametrize("path", PATHS)
def test_sdf_fp16_module_and_points(path, library):
    """module.half()(x16): fp16 storage, fp32 arithmetic.  The reference is the float32 oracle on the fp16-rounded parameters
    and points; the returned point gradient is the fp32 gradient rounded once."""
    def r(x):
        return x.half().float()

    spec16 = O.map_spec(O.scene_test2(), r)
    n = 129
    pts, w = (r(x[:n]) for x in seeded_points())
    (out32, gin32, gpar32), (_, gin64, gpar64) = both_references(spec16, [pts], sdf_forward, [w])
    module = on_device(O.scene_test2(), path, library, half=True)
    assert all(p.dtype == torch.float16 for p in module.parameters())
    x16 = pts.half().to(DEV).requires_grad_(True)
    d16 = module(x16)
    assert d16.dtype == torch.float16 and torch.equal(d16.detach().cpu(), restated(lambda: O.sdf_eval(spec16, pts)).half())
    (d16 * w.half().to(DEV)).sum().backward()
    # the same call in fp32 on the rounded values: its gradient, rounded once, is the fp16 call's
    module32 = on_device(spec16, path, library)
    x32 = pts.to(DEV).requires_grad_(True)
    (module32(x32) * w.to(DEV)).sum().backward()
    assert x16.grad.dtype == torch.float16 and torch.equal(x16.grad, x32.grad.half())
    ulps = H.ulp16_distance(x16.grad, gin32[0].half())
    print(f"fp16 scene2 {path}: point gradient {int(ulps.max())} fp16 ulp from the rounded oracle gradient")
    assert int(ulps.max()) <= 1
    H.gradient_contract("A fp16", f"fp16 scene2 {path} fp32 twin grad_points", x32.grad, gin32[0], gin64[0], tol=1e-5, absolute=True)
    for (k, p), (_, p32), (_, a), (_, b) in zip(module.named_parameters(), module32.named_parameters(), gpar32, gpar64):
        assert p.grad is not None and p.grad.dtype == torch.float16 and p.grad.shape == p.shape, k
        H.gradient_contract("A fp16", f"fp16 scene2 {path} fp32 twin {k}", p32.grad, a, b)
        H.fp16_gradient_contract("A fp16", f"fp16 scene2 {path} {k}", p.grad, a, b)


# --------------------------------------------------------------------------
# B. SDFMarcher: k_march_fwd (recording) and k_march_bwd
# --------------------------------------------------------------------------
MARCH_COUNTS = (1, 63, 65, 129, 257)
MARCH_STEPS = (0, 1, 2, 3, 7, 8, 9, 12, 13, 33)
LEFT_EARLY = {"early": 0, "walked": 0}       # waves of scene 2 from z = -3 that left before / walked to the last step


def march_weights(n):
    return torch.randn(N_STRIDE_BWD, 3, generator=torch.Generator().manual_seed(11))[:n]


def dev_march(module, pos, dirs, steps, w, early, grad=(True, True)):
    """-> (out, grad_pos, grad_dirs, [(name, parameter .grad)], nexec or None)."""
    from ray_marching_amd.rendering.ray_marching import SDFMarcher
    for p in module.parameters():
        p.grad = None
    p = pos.detach().to(DEV).clone().requires_grad_(grad[0])
    v = dirs.detach().to(DEV).clone().requires_grad_(grad[1])
    out = SDFMarcher(module, early_out=early)(p, v, steps)
    saved = out.grad_fn.saved_tensors
    nexec = saved[3].cpu() if saved[3] is not None else None
    (out * w.to(DEV).to(out.dtype)).sum().backward()
    return out, p.grad, v.grad, [(k, q.grad) for k, q in module.named_parameters()], nexec


def march_case(group, what, spec, module, pos, dirs, steps, scene2_from_outside=False):
    """One ray list with the early-out on and off against the two references.  -> nexec of the run with the early-out."""
    n = pos.shape[0]
    w = march_weights(n)

    def forward(s, p, v):
        return (O.march(s, p, v, steps),)

    refs = both_references(spec, [pos, dirs], forward, [w])
    want = restated(lambda: O.march(spec, pos, dirs, steps))
    runs = {}
    for early in (True, False):
        out, gp, gv, gpar, nexec = dev_march(module, pos, dirs, steps, w, early)
        assert out.shape == (n, 3) and nexec.shape == (n,)
        forward_equal(f"{what} early_out={early} p", out, want)
        check_gradients(group, f"{what} early_out={early}", ([out], [gp, gv], gpar), refs, ["grad_pos", "grad_dirs"])
        runs[early] = (out, gp, gv, gpar, nexec)
    assert bool((runs[False][4] == steps).all())
    assert H._same(runs[True][0], runs[False][0])
    gap = max(float((a.double() - b.double()).abs().nan_to_num().max()) for a, b in
              [(runs[True][1], runs[False][1]), (runs[True][2], runs[False][2])] +
              [(a, b) for (_, a), (_, b) in zip(runs[True][3], runs[False][3])])
    nexec = runs[True][4]
    print(f"{what}: gradients with the early-out differ from those without by {gap:.3g}; nexec {sorted(set(nexec.tolist()))}")
    if scene2_from_outside and steps >= 2:
        for wave in range(0, n, 64):
            ne = nexec[wave:wave + 64]
            assert len(set(ne.tolist())) == 1, "nexec is one number per wave"
            LEFT_EARLY["early" if int(ne[0]) < steps else "walked"] += 1
    return nexec


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(PREBUILT))
def test_march_counts_and_steps(name, path, library):
    """Every step count at 65 rays, every count at 12 and 33 steps: the first n rays of a 16 x 16 camera."""
    spec = PREBUILT[name]()
    module = on_device(spec, path, library)
    pos, dirs = camera_rays(16, 16, CAMERA_AT[name])
    cases = [(65, s) for s in MARCH_STEPS] + [(n, s) for n in MARCH_COUNTS for s in (12, 33) if n != 65]
    for n, steps in cases:
        march_case("B", f"{name} {path} n={n} steps={steps}", spec, module, first(pos, n), first(dirs, n), steps,
                   scene2_from_outside=name == "scene2")


@pytest.mark.parametrize("path", PATHS)
def test_march_backward_on_a_trajectory_the_early_out_cut_short(path, library):
    """Scene 2 from z = -3, 257 rays at 32 and 128 steps: some wave leaves before the last step -- k_march_bwd then takes the
    last recorded iterate for every later one -- and some wave walks every step, or this test proves nothing."""
    spec = O.scene_test2()
    module = on_device(spec, path, library)
    pos, dirs = camera_rays(16, 16, CAMERA_AT["scene2"])
    before = dict(LEFT_EARLY)
    for steps in (32, 128):
        march_case("B early-out", f"scene2 {path} n=257 steps={steps}", spec, module, first(pos, 257), first(dirs, 257), steps,
                   scene2_from_outside=True)
    early, walked = (LEFT_EARLY[k] - before[k] for k in ("early", "walked"))
    print(f"scene2 {path}: {early} waves left early, {walked} walked every step")
    assert early > 0 and walked > 0, (early, walked)


@pytest.mark.parametrize("path", PATHS)
def test_march_grid_stride(path, library):
    spec = O.scene_test2()
    module = on_device(spec, path, library)
    pos, dirs = camera_rays(16, 16, CAMERA_AT["scene2"])
    march_case("B grid-stride", f"scene2 {path} n={N_STRIDE_BWD} steps=4", spec, module, first(pos, N_STRIDE_BWD),
               first(dirs, N_STRIDE_BWD), 4)
    from ray_marching_amd.rendering.ray_marching import SDFMarcher
    p, v = first(pos, N_STRIDE_FWD), first(dirs, N_STRIDE_FWD)
    with torch.no_grad():
        got = SDFMarcher(module)(p.to(DEV), v.to(DEV), 4)
    forward_equal(f"scene2 {path} n={N_STRIDE_FWD} p", got, restated(lambda: O.march(spec, p, v, 4)))


@pytest.mark.parametrize("n", [64, 33])
def test_march_open_scene_nan_rays(n, library):
    """Sphere 0.5 from z = -2, the first n rays of an 8 x 8 camera, 128 steps: rays that miss overflow in float32.  Gradients are
    NaN exactly where the float32 oracle's are, the rays that hit meet the bound, and the last ray is one that missed, so every
    lane without a ray clones a NaN ray."""
    spec = O.scene_sphere(0.5)
    module = on_device(spec, "interpreter", library)
    pos, dirs = camera_rays(8, 8, (0.0, 0.0, -2.0))
    pos, dirs = first(pos, n), first(dirs, n)
    w = march_weights(n)
    refs = both_references(spec, [pos, dirs], lambda s, p, v: (O.march(s, p, v, 128),), [w])
    bad = ~torch.isfinite(refs[0][0][0]).all(dim=-1)
    print(f"open sphere n={n}: the float32 oracle has {int(bad.sum())} non-finite and {int((~bad).sum())} finite rays")
    assert bool(bad.any()) and bool((~bad).any()) and bool(bad[-1])
    if n == 64:
        assert int(bad.sum()) == 52 and bool(torch.isfinite(refs[1][0][0]).all())
    assert bool(torch.isnan(refs[0][2][0][1]).all()), "the radius gradient of the float32 oracle is NaN"
    march_case("B open", f"open sphere n={n} steps=128", spec, module, pos, dirs, 128)
    # the rays that hit, on their own: the bound above already holds them to it element by element; here by count
    out, gp, _, gpar, _ = dev_march(module, pos, dirs, 128, w, True)
    assert torch.equal(torch.isnan(gp).any(dim=-1).cpu(), torch.isnan(refs[0][1][0]).any(dim=-1))
    assert int(torch.isfinite(gp).all(dim=-1).sum()) == int(torch.isfinite(refs[0][1][0]).all(dim=-1).sum()) > 0
    assert bool(torch.isnan(gpar[0][1]).all())


def test_march_open_scene_before_it_overflows(library):
    """The same rays at 32 steps: everything is finite, the radius gradient is -4.77e9 in float32 and in float64."""
    spec = O.scene_sphere(0.5)
    module = on_device(spec, "interpreter", library)
    pos, dirs = camera_rays(8, 8, (0.0, 0.0, -2.0))
    refs = both_references(spec, [pos, dirs], lambda s, p, v: (O.march(s, p, v, 32),), [march_weights(64)])
    assert all(bool(torch.isfinite(r[0][0]).all()) and bool(torch.isfinite(r[2][0][1]).all()) for r in refs)
    march_case("B open", "open sphere n=64 steps=32", spec, module, pos, dirs, 32)


@pytest.mark.parametrize("path", PATHS)
def test_march_broadcast(path, library):
    """One origin against many directions and one direction against many origins: the gradients come back in the inputs'
    shapes.  At steps = 0 the output is the broadcast origin, grad_pos the sum of the upstream and everything else zero."""
    from ray_marching_amd.rendering.ray_marching import SDFMarcher
    spec = O.scene_test2()
    module = on_device(spec, path, library)
    gen = torch.Generator().manual_seed(9)
    fan = torch.nn.functional.normalize(torch.randn(6, 9, 3, generator=gen) + torch.tensor([0.0, 0.0, 3.0]), dim=-1)
    origins = torch.cat([0.6 * torch.rand(65, 2, generator=gen) - 0.3, torch.full((65, 1), -3.0)], dim=1)
    calls = {"pos [1,1,3] dirs [6,9,3]": (torch.tensor([[[0.1, -0.2, -3.0]]]), fan),
             "pos [65,3] dirs [1,3]": (origins, torch.tensor([[0.0, 0.0, 1.0]]))}
    for what, (pos, dirs) in calls.items():
        shape = torch.broadcast_shapes(pos.shape, dirs.shape)
        w = march_weights(shape.numel() // 3).reshape(shape)

        def forward(s, p, v):
            return (O.march(s, p, v, 20),)

        refs = both_references(spec, [pos, dirs], forward, [w])
        want = restated(lambda: O.march(spec, pos, dirs, 20))
        for grad in ((True, True), (False, True), (False, False)):
            out, gp, gv, gpar, _ = dev_march(module, pos, dirs, 20, w, True, grad)
            assert out.shape == shape
            forward_equal(f"{what} p", out, want)
            assert (gp is not None) == grad[0] and (gv is not None) == grad[1]
            assert gp is None or gp.shape == pos.shape
            assert gv is None or gv.shape == dirs.shape
            check_gradients("B broadcast", f"scene2 {path} {what} grad={grad}", ([out], [gp, gv], gpar), refs,
                            ["grad_pos" if grad[0] else None, "grad_dirs" if grad[1] else None])
        # March.backward itself hands each gradient back in its input's shape (asked directly: the autograd engine would sum
        # a gradient left in the broadcast shape without a word, so the .grad checks above cannot see one)
        for steps in (20, 0):
            p, v = pos.to(DEV).requires_grad_(True), dirs.to(DEV).requires_grad_(True)
            out = SDFMarcher(module)(p, v, steps)      # (kept: the node drops its saved tensors with its output)
            raw = out.grad_fn.apply(w.to(DEV))
            assert raw[1].shape == pos.shape and raw[2].shape == dirs.shape, (what, steps, raw[1].shape, raw[2].shape)
        # no steps at all
        out, gp, gv, gpar, _ = dev_march(module, pos, dirs, 0, w, True)
        assert torch.equal(out.cpu(), pos.expand(shape))
        assert gp.shape == pos.shape and gv.shape == dirs.shape
        want_gp = w.double().sum_to_size(pos.shape)
        assert float((gp.cpu().double() - want_gp).abs().max()) <= 1e-4 * max(1.0, float(want_gp.abs().max()))
        assert not bool(gv.any()) and all(g is not None and not bool(g.any()) for _, g in gpar)


@pytest.mark.parametrize("path", PATHS)
def test_march_fp16_rays(path, library):
    """fp16 pos and dirs with grad: the march runs in fp32 on the fp16 values, the gradients come back in fp16."""
    spec = O.scene_test2()
    module = on_device(spec, path, library)
    pos, dirs = (first(x, 65).half() for x in camera_rays(16, 16, CAMERA_AT["scene2"]))
    w = march_weights(65).half()
    refs = both_references(spec, [pos.float(), dirs.float()], lambda s, p, v: (O.march(s, p, v, 12),), [w.float()])
    out, gp, gv, gpar, _ = dev_march(module, pos, dirs, 12, w, True)
    assert out.dtype == gp.dtype == gv.dtype == torch.float16
    assert torch.equal(out.detach().cpu(), restated(lambda: O.march(spec, pos.float(), dirs.float(), 12)).half())
    for name, g, a, b in (("grad_pos", gp, refs[0][1][0], refs[1][1][0]), ("grad_dirs", gv, refs[0][1][1], refs[1][1][1])):
        H.fp16_gradient_contract("B fp16", f"fp16 rays scene2 {path} {name}", g, a, b)
    for (k, g), (_, a), (_, b) in zip(gpar, refs[0][2], refs[1][2]):
        assert g.dtype == torch.float32
        H.gradient_contract("B fp16", f"fp16 rays scene2 {path} {k}", g, a, b)


# --------------------------------------------------------------------------
# C. SDFNormals: k_normals_bwd
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def surface_points(name, n):
    """Marched surface points of the scene's 16 x 16 camera (24 steps, on the CPU), tiled to n, plus seeded jitter of 1e-2;
    upstreams for the normals and -- scaled by 1e-3, as test_march_and_normals_backward_vs_oracle scales it: the Laplacian
    carries 6 / eps^2 = 2400 -- for the Laplacian.

    Both upstreams shrink with the count, by the power of two below 4 / sqrt(n).  A parameter every tap sees alike (the room's
    radius) has the gradient sum_k g_k = 0 per point, which float32 leaves at 4 x 2^-24 |g_k| with |g_k| ~ |inverse| |w| ~ 12 |w|
    (eps = 5e-2): 3e-6 |w| per point and 3e-6 sqrt(n) |w| over the sum -- 1.1e-3 at 131 137 points for |w| ~ 1, which is what the
    float32 oracle itself is off by there against float64, under a bound of 1e-4.  With |w| <= 4 / sqrt(n) that noise stays at
    1e-5, a tenth of the bound, at every count, while the gradients that are not zero keep their relative bound."""
    pos, dirs = camera_rays(16, 16, CAMERA_AT[name])
    with torch.no_grad():
        hit = O.march(PREBUILT[name](), pos, dirs, 24)
    assert bool(torch.isfinite(hit).all())
    gen = torch.Generator().manual_seed(13)
    pts = first(hit, n) + 1e-2 * torch.randn(n, 3, generator=gen)
    shrink = min(1.0, 2.0 ** math.floor(math.log2(4.0 / math.sqrt(n))))
    return pts, shrink * torch.randn(n, 3, generator=gen), shrink * 1e-3 * torch.randn(n, 1, generator=gen)


def normals_forward(s, p):
    return O.normals(s, p, H.EPS)


def normals_case(group, what, spec, module, normals, pts, wn, wl, input_grad=True):
    refs = both_references(spec, [pts], normals_forward, [wn, wl])
    dev = dev_grads(module, [pts], lambda p: normals(p), [wn, wl], input_grad=input_grad)
    n_want, lap_want = restated(lambda: O.normals(spec, pts, H.EPS))
    assert dev[0][0].shape == pts.shape and dev[0][1].shape == (*pts.shape[:-1], 1)
    forward_equal(f"{what} n", dev[0][0], n_want)
    forward_equal(f"{what} lap", dev[0][1], lap_want)
    check_gradients(group, what, dev, refs, ["grad_points" if input_grad else None])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(PREBUILT))
def test_normals_counts_and_upstreams(name, path, library):
    """Both upstreams at every count; the normals alone and the Laplacian alone at 65 and 257 points."""
    from ray_marching_amd.rendering.ray_marching import SDFNormals
    spec = PREBUILT[name]()
    module = on_device(spec, path, library)
    normals = SDFNormals(module, H.EPS).to(DEV)
    for n in (1, 63, 65, 129, 257):
        pts, wn, wl = surface_points(name, n)
        normals_case("C", f"{name} {path} n={n} both", spec, module, normals, pts, wn, wl)
        if n in (65, 257):
            normals_case("C", f"{name} {path} n={n} normals only", spec, module, normals, pts, wn, None)
            normals_case("C", f"{name} {path} n={n} laplacian only", spec, module, normals, pts, None, wl)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(PREBUILT))
def test_normals_grid_stride(name, path, library):
    from ray_marching_amd.rendering.ray_marching import SDFNormals
    spec = PREBUILT[name]()
    module = on_device(spec, path, library)
    pts, wn, wl = surface_points(name, N_STRIDE_BWD)
    normals_case("C grid-stride", f"{name} {path} n={N_STRIDE_BWD}", spec, module, SDFNormals(module, H.EPS).to(DEV), pts, wn, wl)


@pytest.mark.parametrize("path", PATHS)
def test_normals_who_asks_layout_dtype_and_empty(path, library):
    from ray_marching_amd.rendering.ray_marching import SDFNormals
    name = "scene1_closed"
    spec = PREBUILT[name]()
    pts, wn, wl = surface_points(name, 129)
    # points only
    module = on_device(spec, path, library)
    normals = SDFNormals(module, H.EPS).to(DEV)
    for p in module.parameters():
        p.requires_grad_(False)
    refs = both_references(spec, [pts], normals_forward, [wn, wl])
    dev = dev_grads(module, [pts], lambda p: normals(p), [wn, wl])
    assert all(g is None for _, g in dev[2])
    H.gradient_contract("C inputs", f"{name} {path} points only", dev[1][0], refs[0][1][0], refs[1][1][0])
    # parameters only
    module = on_device(spec, path, library)
    normals = SDFNormals(module, H.EPS).to(DEV)
    normals_case("C", f"{name} {path} parameters only", spec, module, normals, pts, wn, wl, input_grad=False)
    # a leading shape
    x, un, ul = (t[:70].reshape(2, 5, 7, -1) for t in (pts, wn, wl))
    normals_case("C", f"{name} {path} [2, 5, 7, 3]", spec, module, normals, x, un, ul)
    # empty input with grad: zero gradients of the right shapes
    x = torch.empty(0, 3, device=DEV, requires_grad=True)
    n, lap = normals(x)
    assert n.shape == (0, 3) and lap.shape == (0, 1)
    for p in module.parameters():
        p.grad = None
    (n.sum() + lap.sum()).backward()
    assert x.grad.shape == (0, 3) and x.grad.dtype == torch.float32
    for k, p in module.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and not bool(p.grad.any()), k
    # an fp16 module and fp16 points: fp16 storage (tap offsets included), fp32 arithmetic, gradients back in fp16
    def r(t):
        return t.half().float()

    spec16 = O.map_spec(PREBUILT["scene2"](), r)
    module = on_device(PREBUILT["scene2"](), path, library, half=True)
    normals = SDFNormals(module, H.EPS).to(DEV).half()
    tetra = tuple(r(c) for c in O.tetra_constants(H.EPS))
    pts, wn, wl = (r(t) for t in surface_points("scene2", 65))

    def forward16(s, p):
        return O.normals(s, p, H.EPS, tetra)

    refs = both_references(spec16, [pts], forward16, [wn, wl])
    x16 = pts.half().to(DEV).requires_grad_(True)
    n16, lap16 = normals(x16)
    n_want, lap_want = restated(lambda: O.normals(spec16, pts, H.EPS, tetra))
    assert n16.dtype == lap16.dtype == torch.float16
    assert H.report("fp16 normals", n16, n_want.half())[0] == 0.0 and H.report("fp16 laplacian", lap16, lap_want.half())[0] == 0.0
    ((n16 * wn.half().to(DEV)).sum() + (lap16 * wl.half().to(DEV)).sum()).backward()
    assert x16.grad.dtype == torch.float16 and x16.grad.shape == (65, 3)
    H.fp16_gradient_contract("C fp16", f"fp16 scene2 {path} grad_points", x16.grad, refs[0][1][0], refs[1][1][0])
    for (k, p), (_, a), (_, b) in zip(module.named_parameters(), refs[0][2], refs[1][2]):
        assert p.grad is not None and p.grad.dtype == torch.float16, k
        H.fp16_gradient_contract("C fp16", f"fp16 scene2 {path} {k}", p.grad, a, b)


# --------------------------------------------------------------------------
# D. PinholeCamera: k_camera_bwd, k_camera_bwd_finish
# --------------------------------------------------------------------------
def poses(n, seed):
    """Seeded poses; quaternions of norm 0.9 .. 1.1, not normalised."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(n, 4, generator=gen), dim=-1) * (0.9 + 0.2 * torch.rand(n, 1, generator=gen))
    return q, torch.randn(n, 3, generator=gen)


def camera_case(what, n, h, w, rows=None):
    from ray_marching_amd.rendering.ray_marching import PinholeCamera
    cam = PinholeCamera(n, w, h, H.PX * h, H.PX * w, H.PX * h, rows=rows).to(DEV)
    bufs = O.camera_buffers(n, w, h, H.PX * h, H.PX * w, H.PX * h)
    if rows is not None:
        bufs = tuple(b[:, rows[0]:rows[1]].contiguous() for b in bufs)      # the same rows of the full camera
    q, t = poses(n, 100 * h + w)
    gen = torch.Generator().manual_seed(h + w)
    wp, wd = (torch.randn(bufs[0].shape, generator=gen) for _ in range(2))
    want = O.camera_forward(*bufs, q, t)
    for up_name, up in (("positions", (wp, None)), ("directions", (None, wd)), ("both", (wp, wd))):
        refs = []
        for dtype in (torch.float32, torch.float64):
            qc, tc = (x.to(dtype).clone().requires_grad_(True) for x in (q, t))
            pos, _, dirs = O.camera_forward(*(b.to(dtype) for b in bufs), qc, tc)
            sum((o * u.to(dtype)).sum() for o, u in ((pos, up[0]), (dirs, up[1])) if u is not None).backward()
            refs.append({"orientation": qc.grad, "translation": tc.grad if tc.grad is not None else torch.zeros_like(tc)})
        for need in ((True, False), (False, True), (True, True)):
            qg, tg = q.to(DEV).requires_grad_(need[0]), t.to(DEV).requires_grad_(need[1])
            pos, frames, pos2, dirs = cam(qg, tg)
            assert pos2 is pos and not frames.requires_grad
            for name, got, ref in (("pos", pos, want[0]), ("frames", frames, want[1].reshape(n, 3, 3)), ("dirs", dirs, want[2])):
                forward_equal(f"{what} {name}", got, ref)
            sum((o * u.to(DEV)).sum() for o, u in ((pos, up[0]), (dirs, up[1])) if u is not None).backward()
            for name, leaf, asked in (("orientation", qg, need[0]), ("translation", tg, need[1])):
                if not asked:
                    assert leaf.grad is None
                    continue
                assert leaf.grad is not None and leaf.grad.shape == leaf.shape and leaf.grad.dtype == torch.float32
                H.gradient_contract("D camera", f"{what} upstream on {up_name}, {name}", leaf.grad, refs[0][name], refs[1][name])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (17, 13), (33, 70)])
def test_camera_pose_gradients(h, w, n):
    camera_case(f"camera {n} x {h} x {w}", n, h, w)


def test_camera_row_band_and_a_frame_that_fills_every_partial_row():
    """rows=(5, 12) of a 17 x 13 camera against the same rows of the full camera's oracle; and 255 x 257 = 65 535 pixels, more
    than 255 x 256, so that every one of the 256 per-block partial rows k_camera_bwd_finish adds carries a term."""
    camera_case("camera 1 x 17 x 13 rows 5..12", 1, 17, 13, rows=(5, 12))
    camera_case("camera 2 x 17 x 13 rows 5..12", 2, 17, 13, rows=(5, 12))
    assert 255 * 257 > 255 * 256
    camera_case("camera 1 x 255 x 257", 1, 255, 257)


# --------------------------------------------------------------------------
# E. LambertianShader, VignetteShader, NormalShader: k_shade_bwd
# --------------------------------------------------------------------------
def oracle_shade(mode, dirs, normals, frames):
    """The oracle's shader formulas; the vignette with each camera's own third column (the reference's broadcast, which only
    works for one camera, written out per camera)."""
    if mode == 0:
        return O.shade_lambertian(dirs, normals)
    if mode == 3:
        col = frames[..., 2].reshape(frames.shape[0], *([1] * (dirs.dim() - 2)), 3) if frames.shape[0] > 1 else frames[..., 2]
        return (dirs * col).sum(dim=-1, keepdim=True).pow(3)
    return O.shade_normal(normals)


def shader_inputs(lead, seed):
    gen = torch.Generator().manual_seed(seed)
    dirs = torch.nn.functional.normalize(torch.randn(*lead, 3, generator=gen), dim=-1)
    normals = torch.nn.functional.normalize(torch.randn(*lead, 3, generator=gen), dim=-1)
    frames = O.quat_to_so3(poses(lead[0], seed)[0])
    return dirs, normals, frames


def shader_case(what, mode, dirs, normals, frames, need=(True, True), half=False):
    """One shader module against float32 and float64 autograd on oracle_shade.  ``need``: (dirs, normals) require grad."""
    from ray_marching_amd.rendering import shader as S
    cast = (lambda x: x.half()) if half else (lambda x: x)
    dirs, normals, frames = (cast(x) for x in (dirs, normals, frames))
    lead = torch.broadcast_shapes(dirs.shape[:-1], normals.shape[:-1])
    gen = torch.Generator().manual_seed(17)
    up = cast(torch.randn(*lead, 3 if mode == 4 else 1, generator=gen))
    uses = {0: (True, True), 3: (True, False), 4: (False, True)}[mode]
    refs = []
    for dtype in (torch.float32, torch.float64):
        d, n = (x.to(dtype).clone().requires_grad_(True) for x in (dirs, normals))
        (oracle_shade(mode, d, n, frames.to(dtype)) * up.to(dtype)).sum().backward()
        refs.append((d.grad, n.grad))
    d = dirs.to(DEV).requires_grad_(need[0] and uses[0])
    n = normals.to(DEV).requires_grad_(need[1] and uses[1])
    module = {0: S.LambertianShader, 3: S.VignetteShader, 4: S.NormalShader}[mode]()
    img = {0: lambda: module(d, n), 3: lambda: module(d, frames.to(DEV)), 4: lambda: module(n)}[mode]()
    with torch.no_grad():
        want = oracle_shade(mode, dirs.float(), normals.float(), frames.float())
    assert img.shape == want.shape and img.dtype == dirs.dtype
    err = H.report(f"{what} image", img, cast(want))[0]
    print(f"{what}: image max|err| {err:.3g}")
    assert err <= (2.0 ** -10 if half else 1e-5)
    (img * up.to(DEV)).sum().backward()
    for k, (name, leaf) in enumerate((("grad_dirs", d), ("grad_normals", n))):
        if not leaf.requires_grad:
            assert leaf.grad is None
            continue
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape and leaf.grad.dtype == leaf.dtype, (what, name)
        rule = H.fp16_gradient_contract if half else H.gradient_contract
        rule("E shaders", f"{what} {name}", leaf.grad, refs[0][k], refs[1][k])


@pytest.mark.parametrize("mode", [0, 3, 4])
def test_shader_gradients(mode):
    for lead in ((1, 1, 1), (1, 1, 65), (1, 1, 257), (2, 5, 13)):
        dirs, normals, frames = shader_inputs(lead, 31 + lead[-1])
        what = f"shader mode {mode} {list(lead)}"
        shader_case(what, mode, dirs, normals, frames)
        if lead == (1, 1, 65):
            if mode == 0:      # (the other two shaders take one of the two only)
                shader_case(what + " only dirs", mode, dirs, normals, frames, need=(True, False))
                shader_case(what + " only normals", mode, dirs, normals, frames, need=(False, True))
            shader_case(what + " fp16", mode, dirs, normals, frames, half=True)
    if mode == 0:      # one normal for the whole frame: its gradient is the sum over the pixels
        dirs, normals, frames = shader_inputs((1, 5, 13), 5)
        shader_case("shader mode 0 normals [1, 1, 1, 3]", 0, dirs, normals[:, :1, :1], frames)


def test_vignette_with_flattened_rays_of_two_cameras_is_refused():
    """Flattened [N H W, 3] directions carry no camera axis, so with N = 2 frames the vignette cannot tell whose third column a
    pixel takes (the reference fails to broadcast there): a ValueError, in the forward and when a gradient is asked for.  One
    frame against any leading shape is the reference's broadcast: every pixel takes that frame."""
    from ray_marching_amd.rendering.shader import VignetteShader
    dirs, normals, frames = shader_inputs((2, 5, 13), 3)
    flat = dirs.reshape(-1, 3).to(DEV)
    for grad in (False, True):
        with pytest.raises(ValueError, match="camera"):
            VignetteShader()(flat.clone().requires_grad_(grad), frames.to(DEV))
    shader_case("vignette one frame, rays [2, 5, 13, 3]", 3, dirs, normals, frames[:1])
    shader_case("vignette one frame, rays [130, 3]", 3, dirs.reshape(-1, 3), normals.reshape(-1, 3), frames[:1])


# --------------------------------------------------------------------------
# F. the composed chain
# --------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_chain_camera_marcher_normals_shader(path, library):
    """camera -> marcher -> normals -> shader by hand, modes 0, 3 and 4, two cameras of 17 x 13 on scene 2, 24 steps: pose and
    parameter gradients against the oracle's frame in float32 and float64.  (The modules take ``frames`` as data, so the
    oracle's vignette gets them detached: the pose reaches it through the directions.)"""
    h, w, steps, n = 17, 13, 24, 2
    spec = O.scene_test2()
    module = on_device(spec, path, library)
    loop = H.make_loop(module, h, w, n=n)
    bufs = O.camera_buffers(n, w, h, H.PX * h, H.PX * w, H.PX * h)
    gen = torch.Generator().manual_seed(5)
    q = torch.nn.functional.normalize(torch.tensor([[0.98, 0.05, -0.12, 0.03], [0.95, -0.1, 0.2, 0.05]]), dim=-1)
    t = torch.tensor([[0.15, -0.1, -3.0], [-0.3, 0.2, -2.5]])

    def frame(s, qq, tt, mode):
        pos, frames, dirs = O.camera_forward(*(b.to(qq.dtype) for b in bufs), qq, tt)
        p = O.march(s, pos, dirs, steps)
        nrm, _ = O.normals(s, p, H.EPS)
        return oracle_shade(mode, dirs, nrm, frames.detach())

    for mode in (0, 3, 4):
        wimg = torch.rand(n, h, w, 3 if mode == 4 else 1, generator=gen)
        refs = both_references(spec, [q, t], lambda s, qq, tt: (frame(s, qq, tt, mode),), [wimg])
        for p in module.parameters():
            p.grad = None
        qg, tg = q.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
        pos, frames, _, dirs = loop.camera(qg, tg)
        p = loop.marcher(pos, dirs, steps)
        dist = loop.scene(p)
        nrm, lap = loop.normals(p)
        img = loop.shader(pos, qg, frames, dirs, p, nrm, lap, dist, mode=mode, degree=1)
        assert img.shape == wimg.shape
        err = H.report(f"chain mode {mode} image", img, refs[0][0][0])[0]
        print(f"chain {path} mode {mode}: image max|err| {err:.3g}")
        assert err <= 1e-5
        (img * wimg.to(DEV)).sum().backward()
        tgrad = tg.grad if tg.grad is not None else torch.zeros_like(tg)       # (the vignette does not see the translation)
        dev = ([img], [qg.grad, tgrad], [(k, x.grad if x.grad is not None else torch.zeros_like(x)) for k, x in module.named_parameters()])
        check_gradients("F chain", f"chain {path} mode {mode}", dev, refs, ["orientation", "translation"])


def test_zz_worst_figures():
    """The worst of every group, as measured by the tests above in this run (DESIGN.md 7 records them)."""
    for line in H.standalone_summary():
        print(line)
