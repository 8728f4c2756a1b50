"""Shared test helpers: oracle spec <-> product module conversion, fixtures, tolerances."""
import contextlib
import os

import numpy as np
import torch

from oracle import sdf_oracle as O

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PX = 3.45e-6
EPS = 5e-2


def gold(name):
    return np.load(os.path.join(GOLD, name))


@contextlib.contextmanager
def environment(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) and torch.equal(a.isnan(), b.isnan())


def _points(n=4096, seed=0, lo=-2.5, hi=2.5):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


def _pose(z, dev="cuda"):
    return torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev), torch.tensor([[0.0, 0.0, z]], device=dev)


def spec_to_module(spec):
    """Oracle scene spec -> ray_marching_amd nn.Module tree (parameter values copied)."""
    from ray_marching_amd.scene import primitives as P, transformations as T
    kind, prm = spec[0], spec[1]

    def f(x):
        return x.detach().tolist()

    if kind == "sphere":
        return P.SDFSphere(f(prm["radius"]))
    if kind == "box":
        return P.SDFBox(tuple(f(prm["halfsides"])))
    if kind == "plane":
        return P.SDFPlane()
    if kind == "line":
        return P.SDFLine(tuple(f(prm["start"])), tuple(f(prm["end"])), f(prm["radius"]))
    if kind == "disk":
        return P.SDFDisk(f(prm["radius"]))
    if kind == "torus":
        return P.SDFTorus(f(prm["radius1"]), f(prm["radius2"]))
    if kind == "affine":
        return T.SDFAffineTransformation(spec_to_module(spec[2]), orientation=f(prm["orientation"]),
                                         translation=f(prm["translation"]))
    if kind == "smooth_union":
        return T.SDFSmoothUnion([spec_to_module(c) for c in spec[2]], f(prm["blend_k"]))
    if kind == "union":
        return T.SDFUnion([spec_to_module(c) for c in spec[2]])
    if kind == "rounding":
        return T.SDFRounding(spec_to_module(spec[2]), f(prm["rounding"]))
    if kind == "onion":
        return T.SDFOnion(spec_to_module(spec[2]), f(prm["radius"]))
    raise ValueError(kind)


def node_specs():
    from oracle.gen_golden import node_specs as ns
    return ns()


def make_loop(module, h, w, n=1, device="cuda", **kw):
    from ray_marching_amd.control import RenderLoop
    return RenderLoop(module, num_cameras=n, px_width=w, px_height=h, focal_length=PX * h,
                      sensor_width=PX * w, sensor_height=PX * h, normals_eps=EPS, **kw).to(device)


def report(name, got, want):
    """max abs error, fraction of elements beyond 1e-5 (NaN positions must agree)."""
    got = torch.as_tensor(got).detach().double().cpu()
    want = torch.as_tensor(want).detach().double().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_g, nan_w), f"{name}: NaN pattern differs ({nan_g.sum()} vs {nan_w.sum()})"
    err = (torch.nan_to_num(got) - torch.nan_to_num(want)).abs()
    err = torch.where(torch.isinf(got) & (got == want), torch.zeros_like(err), err)
    return float(err.max()) if err.numel() else 0.0, float((err > 1e-5).double().mean()) if err.numel() else 0.0


def ulp_distance(got, want):
    """|got - want| in fp32 units in the last place (bit patterns as ordered integers), int64 tensor."""
    def ordered(t):
        b = torch.as_tensor(t).detach().float().cpu().contiguous().view(torch.int32).long()
        return torch.where(b < 0, -(b & 0x7fffffff), b)
    return (ordered(got) - ordered(want)).abs()


# --------------------------------------------------------------------------
# the rule of tests/test_fast_build.py: the precision="fast" build against the float64 oracle
# --------------------------------------------------------------------------
# E_fast = |fast - o64| must stay within FAST_FACTOR times E_ref = |o32 - o64|, the oracle's own float32 error on the same
# inputs, plus a floor of float32 resolution.  The factor is derived, not fitted: every operation the fast build swaps in is
# documented in csrc/rm_device.h as <= ~2 ulp (v_exp_f32 / v_log_f32), 1 ulp (v_sqrt_f32) or 1.5 ulp (v_rcp_f32 and a
# multiply) where the correctly rounded forms they replace have 0.5 ulp; FMA contraction only removes roundings.
FAST_FACTOR = 4.0
FAST_RATIOS = {}      # group -> (largest E_fast / E_ref seen, where), printed by fast_note as it grows


def fast_note(group, ratio, what):
    if ratio > FAST_RATIOS.get(group, (-1.0, ""))[0]:
        FAST_RATIOS[group] = (ratio, what)
    print(f"fast build [{group}]: largest E_fast / E_ref so far {FAST_RATIOS[group][0]:.3g} ({FAST_RATIOS[group][1]})")


def _ratio(fast, ref, floor):
    """E_fast / E_ref for the record; where the reference's own error is below the floor, against the floor."""
    return fast / max(ref, floor) if max(ref, floor) > 0.0 else (0.0 if fast == 0.0 else float("inf"))


def fast_errors(what, got, o32, o64):
    """(E_fast, E_ref, valid) as float64 CPU tensors.  NaN positions of ``got`` must equal the reference's wherever o32 and
    o64 agree on them; ``valid`` marks the elements finite in both, where the two errors are defined."""
    got, o32, o64 = (torch.as_tensor(x).detach().double().cpu() for x in (got, o32, o64))
    assert got.shape == o32.shape == o64.shape, (what, got.shape, o32.shape, o64.shape)
    agree = torch.isnan(o32) == torch.isnan(o64)
    bad = (torch.isnan(got) != torch.isnan(o64)) & agree
    assert not bool(bad.any()), f"{what}: NaN at {int(torch.isnan(got).sum())} positions, the reference at " \
                                f"{int(torch.isnan(o64).sum())}; {int(bad.sum())} positions differ"
    valid = ~torch.isnan(o32) & ~torch.isnan(o64)
    zero = torch.zeros_like(o64)
    return torch.where(valid, (got - o64).abs(), zero), torch.where(valid, (o32 - o64).abs(), zero), valid


def fast_value_rule(group, what, got, o32, o64, factor=FAST_FACTOR):
    """max E_fast <= max(factor max E_ref, u) and mean E_fast <= max(factor mean E_ref, u / 4) with u = 2^-23 max|o64|
    (E_ref is exactly 0 for a plane).  Prints every figure before it asserts; -> the larger of the two ratios."""
    e_fast, e_ref, valid = fast_errors(what, got, o32, o64)
    assert bool(valid.any()), what
    u = 2.0 ** -23 * float(torch.as_tensor(o64).detach().double().cpu()[valid].abs().max())
    mx_f, mx_r = float(e_fast[valid].max()), float(e_ref[valid].max())
    mn_f, mn_r = float(e_fast[valid].mean()), float(e_ref[valid].mean())
    ratio = max(_ratio(mx_f, mx_r, u), _ratio(mn_f, mn_r, u / 4))
    print(f"{what}: max E_fast {mx_f:.3g} E_ref {mx_r:.3g} (ratio {_ratio(mx_f, mx_r, u):.3g}), mean E_fast {mn_f:.3g} "
          f"E_ref {mn_r:.3g} (ratio {_ratio(mn_f, mn_r, u / 4):.3g}), u {u:.3g}")
    fast_note(group, ratio, what)
    assert mx_f <= max(factor * mx_r, u), (what, mx_f, mx_r, u)
    assert mn_f <= max(factor * mn_r, u / 4), (what, mn_f, mn_r, u)
    return ratio


def fast_frame_rule(group, what, got, o32, o64, factor=FAST_FACTOR):
    """Frames [N, H, W, 3], per-pixel error e = max over the channels:  q90(e_fast) <= max(factor q90(e_ref), 2^-22),  at most
    1 % of the pixels with e_fast > 1e-3 (so that no block of wrong pixels hides behind the quantile), and NaN positions
    equal to the reference's wherever o32 and o64 agree on them.  Prints every figure before it asserts; -> the q90 ratio."""
    e_fast, e_ref, valid = fast_errors(what, got, o32, o64)
    pixel = valid.all(dim=-1)
    assert bool(pixel.any()), what
    e_fast, e_ref = e_fast.amax(dim=-1)[pixel], e_ref.amax(dim=-1)[pixel]
    q_f, q_r = float(torch.quantile(e_fast, 0.9)), float(torch.quantile(e_ref, 0.9))
    share_f, share_r = float((e_fast > 1e-3).double().mean()), float((e_ref > 1e-3).double().mean())
    ratio = _ratio(q_f, q_r, 2.0 ** -22)
    print(f"{what}: q90 e_fast {q_f:.3g} e_ref {q_r:.3g} (ratio {ratio:.3g}), max e_fast {float(e_fast.max()):.3g} e_ref "
          f"{float(e_ref.max()):.3g}, share beyond 1e-3 fast {share_f:.3g} ref {share_r:.3g}, {int(pixel.sum())} of {pixel.numel()} pixels")
    fast_note(group, ratio, what)
    assert q_f <= max(factor * q_r, 2.0 ** -22), (what, q_f, q_r)
    assert share_f <= 0.01, (what, share_f)
    return ratio


def fast_gradient_rule(group, what, got, g32, g64, factor=FAST_FACTOR):
    """One gradient tensor:  max|got - g64| <= max(1e-4 max(1, |g64|max), factor max|g32 - g64|)  -- the project's gradient
    contract, or the rule above -- and a NaN pattern equal to the float64 reference's, element for element.  Prints every
    figure before it asserts; -> max|got - g64| / max|g32 - g64|."""
    got, g32, g64 = (torch.as_tensor(x).detach().double().cpu() for x in (got, g32, g64))
    assert got.shape == g32.shape == g64.shape, (what, got.shape, g32.shape, g64.shape)
    print(f"{what}: NaN at {int(torch.isnan(got).sum())} of {got.numel()} elements, g64 at {int(torch.isnan(g64).sum())}, "
          f"g32 at {int(torch.isnan(g32).sum())}")
    assert torch.equal(torch.isnan(got), torch.isnan(g64)), (what, got, g64)
    fin = ~torch.isnan(g64)
    if not bool(fin.any()):
        return 0.0
    both = fin & ~torch.isnan(g32)
    spread = float((g32 - g64)[both].abs().max()) if bool(both.any()) else 0.0
    scale = max(1.0, float(g64[fin].abs().max()))
    err = float((got - g64)[fin].abs().max())
    ratio = _ratio(err, spread, 2.0 ** -23 * scale)
    print(f"{what}: |got - g64| {err:.3g}, |g32 - g64| {spread:.3g} (ratio {ratio:.3g}), |g64|max {scale:.3g}")
    fast_note(group, ratio, what)
    assert err <= max(1e-4 * scale, factor * spread), (what, err, spread, scale)
    return ratio


def random_spec(gen, depth=0, max_depth=4):
    """Random SDF tree over all 11 node types (oracle spec); `gen` is a torch.Generator."""
    def u(lo, hi, n=None):
        x = torch.rand(n or 1, generator=gen) * (hi - lo) + lo
        return x if n else x[0]

    def leaf():
        k = int(torch.randint(0, 6, (1,), generator=gen))
        if k == 0:
            return ("sphere", {"radius": u(0.2, 1.0).clone()})
        if k == 1:
            return ("box", {"halfsides": u(0.1, 0.9, 3)})
        if k == 2:
            return ("plane", {})
        if k == 3:
            return ("line", {"start": u(-1.0, 1.0, 3), "end": u(-1.0, 1.0, 3) + 0.5, "radius": u(0.05, 0.3).clone()})
        if k == 4:
            return ("disk", {"radius": u(0.3, 1.0).clone()})
        return ("torus", {"radius1": u(0.5, 1.2).clone(), "radius2": u(0.05, 0.3).clone()})

    if depth >= max_depth or float(torch.rand(1, generator=gen)) < 0.25:
        return leaf()
    k = int(torch.randint(0, 5, (1,), generator=gen))
    if k == 0:
        q = torch.nn.functional.normalize(torch.randn(4, generator=gen), dim=0) * u(0.9, 1.1)   # not normalised on purpose
        return ("affine", {"translation": u(-1.0, 1.0, 3), "orientation": q}, random_spec(gen, depth + 1, max_depth))
    if k == 1:
        n = int(torch.randint(1, 5, (1,), generator=gen))
        return ("smooth_union", {"blend_k": u(4.0, 30.0).clone()}, [random_spec(gen, depth + 1, max_depth) for _ in range(n)])
    if k == 2:
        n = int(torch.randint(1, 5, (1,), generator=gen))
        return ("union", {}, [random_spec(gen, depth + 1, max_depth) for _ in range(n)])
    if k == 3:
        return ("rounding", {"rounding": u(0.0, 0.2).clone()}, random_spec(gen, depth + 1, max_depth))
    return ("onion", {"radius": u(0.02, 0.2).clone()}, random_spec(gen, depth + 1, max_depth))


def widen_spec(spec, gen):
    """A tree of random_spec pushed into the parameter ranges that function never draws: every `rounding` / `onion` parameter
    is negated with probability 0.4, every affine quaternion rescaled with probability 0.5 to the norm 0.88 + 0.5 u, i.e.
    |q|^2 in 0.77 .. 1.9 (the slopes min(1, 2 s - 1) and max(1, 2 s - 1) of the bound walk both leave 1).  Every |q|^2 stays
    0.01 away from 0.75 and 4, where the walk gives up, so that fp32 and fp64 decide finite versus inf alike.  Draws from
    `gen` only; returns a new spec."""
    def u():
        return float(torch.rand(1, generator=gen))

    kind, prm = spec[0], dict(spec[1])
    if kind in ("rounding", "onion"):
        name = "rounding" if kind == "rounding" else "radius"
        if u() < 0.4:
            prm[name] = -prm[name]
    if kind == "affine":
        q = prm["orientation"]
        if u() < 0.5:
            q = torch.nn.functional.normalize(q, dim=0) * (0.88 + 0.5 * u())
        s2 = float(q.double().pow(2).sum())
        assert abs(s2 - 0.75) >= 0.01 and abs(s2 - 4.0) >= 0.01, s2
        prm["orientation"] = q
    if kind in ("affine", "rounding", "onion"):
        return (kind, prm, widen_spec(spec[2], gen))
    if kind in ("smooth_union", "union"):
        return (kind, prm, [widen_spec(c, gen) for c in spec[2]])
    return (kind, prm)


def spec_has(spec, kind):
    if spec[0] == kind:
        return True
    kids = spec[2] if len(spec) > 2 else []
    kids = kids if isinstance(kids, list) else [kids]
    return any(spec_has(c, kind) for c in kids)


def random_blob_spec(gen, n_min=8, n_max=40):
    """A smooth union of many affine-placed random subtrees spread widely enough (relative to 104 / blend_k) that the
    exact logsumexp culling (RM_OP_CULL_LSE) finds children to skip, optionally inside a room and next to other
    nodes.  Oracle spec; `gen` is a torch.Generator."""
    def u(lo, hi, n=None):
        x = torch.rand(n or 1, generator=gen) * (hi - lo) + lo
        return x if n else x[0]

    k = float(u(3.0, 60.0))
    n = int(torch.randint(n_min, n_max + 1, (1,), generator=gen))
    spread = float(u(0.4, 3.0)) * 104.0 / k
    kids = []
    for _ in range(n):
        q = torch.nn.functional.normalize(torch.randn(4, generator=gen), dim=0) * u(0.93, 1.07)
        child = random_spec(gen, depth=2, max_depth=4)
        kids.append(("affine", {"translation": u(-spread, spread, 3), "orientation": q}, child))
    blob = ("smooth_union", {"blend_k": torch.tensor(k)}, kids)
    form = int(torch.randint(0, 3, (1,), generator=gen))
    if form == 0:
        return blob, spread
    if form == 1:
        room = ("onion", {"radius": torch.tensor(0.1)}, ("box", {"halfsides": torch.full((3,), 2.5 * spread + 3.0)}))
        return ("union", {}, [room, blob]), spread
    q = torch.nn.functional.normalize(torch.randn(4, generator=gen), dim=0)
    return ("union", {}, [("affine", {"translation": u(-1.0, 1.0, 3), "orientation": q}, blob), random_spec(gen, depth=2)]), spread


# --------------------------------------------------------------------------
# the rule of tests/test_standalone_backward.py: the exact build's stand-alone gradients against CPU autograd on the oracle
# --------------------------------------------------------------------------
# One gradient tensor against the oracle's float32 and float64 autograd on the same inputs: the project's gradient contract
# (1e-4, relative to the largest float64 component once that exceeds 1) with the min rule of test_backward_vs_golden -- the
# nearer of the two references counts, since float32 autograd carries its own rounding and float64 follows another trajectory
# where float32 rounds.  Non-finite elements are float32's business alone (float64 does not overflow where float32 does).
STANDALONE_WORST = {}      # group -> [(|got - g32|, what), (|got - g64|, what), (|g32 - g64|, what)], printed as it grows


def f64_spec(spec):
    return O.map_spec(spec, lambda x: x.detach().double())


def standalone_note(group, what, figures):
    worst = STANDALONE_WORST.setdefault(group, [(0.0, "")] * 3)
    for k, x in enumerate(figures):
        if x > worst[k][0]:
            worst[k] = (x, what)


def standalone_summary():
    lines = []
    for group in sorted(STANDALONE_WORST):
        (a, wa), (b, wb), (c, wc) = STANDALONE_WORST[group]
        lines.append(f"stand-alone gradients [{group}]: worst |got - g32| {a:.3g} ({wa}), |got - g64| {b:.3g} ({wb}), "
                     f"|g32 - g64| {c:.3g} ({wc})")
    return lines


def gradient_contract(group, what, got, g32, g64, tol=1e-4, absolute=False):
    """min(max|got - g32|, max|got - g64|) <= tol max(1, max|g64|) over the elements finite in the references (``absolute``:
    <= tol, the bound the point gradients of scene(points) have always had); NaN exactly where the float32 oracle has NaN,
    and equal to it where that is infinite.  Prints the three figures before it asserts; -> min(e32, e64)."""
    got, g32, g64 = (torch.as_tensor(x).detach().double().cpu() for x in (got, g32, g64))
    assert got.shape == g32.shape == g64.shape, (what, got.shape, g32.shape, g64.shape)
    nan_got, nan_ref = torch.isnan(got), torch.isnan(g32)
    assert torch.equal(nan_got, nan_ref), f"{what}: NaN at {int(nan_got.sum())} of {got.numel()} elements, the float32 oracle at " \
                                          f"{int(nan_ref.sum())}; {int((nan_got != nan_ref).sum())} positions differ"
    inf = torch.isinf(g32)
    assert torch.equal(got[inf], g32[inf]), (what, "infinite elements differ")
    fin32 = torch.isfinite(g32)
    fin = fin32 & torch.isfinite(g64)
    e32 = float((got - g32)[fin32].abs().max()) if bool(fin32.any()) else 0.0
    e64 = float((got - g64)[fin].abs().max()) if bool(fin.any()) else 0.0
    spread = float((g32 - g64)[fin].abs().max()) if bool(fin.any()) else 0.0
    scale = 1.0 if absolute or not bool(fin.any()) else max(1.0, float(g64[fin].abs().max()))
    print(f"{what}: |got - g32| {e32:.3g}, |got - g64| {e64:.3g}, |g32 - g64| {spread:.3g}, scale {scale:.3g}, "
          f"{int(nan_ref.sum())} NaN of {got.numel()}")
    standalone_note(group, what, (e32, e64, spread))
    best = min(e32, e64) if bool(fin.any()) else e32
    assert best <= tol * scale, (what, e32, e64, spread, scale)
    return best


def fp16_gradient_contract(group, what, got, g32, g64, tol=1e-4):
    """gradient_contract for a gradient handed back in fp16: the fp32 gradient rounded once, so each element may sit half an
    fp16 ulp (2^-11 relative, 2^-25 among the subnormals) further from the reference than the contract allows."""
    assert got.dtype == torch.float16, (what, got.dtype)
    got, g32, g64 = (torch.as_tensor(x).detach().double().cpu() for x in (got, g32, g64))
    assert got.shape == g32.shape == g64.shape, (what, got.shape, g32.shape, g64.shape)
    assert bool(torch.isfinite(g32).all()) and bool(torch.isfinite(g64).all()) and bool(torch.isfinite(got).all()), what
    scale = max(1.0, float(g64.abs().max()))
    beyond = [float(((got - ref).abs() - (2.0 ** -11 * ref.abs() + 2.0 ** -25)).clamp(min=0.0).max()) for ref in (g32, g64)]
    print(f"{what}: beyond fp16 rounding |got - g32| {beyond[0]:.3g}, |got - g64| {beyond[1]:.3g}, |g32 - g64| "
          f"{float((g32 - g64).abs().max()):.3g}, scale {scale:.3g}")
    standalone_note(group, what, (beyond[0], beyond[1], float((g32 - g64).abs().max())))
    assert min(beyond) <= tol * scale, (what, beyond, scale)
    return min(beyond)


def ulp16_distance(got, want):
    """|got - want| in fp16 units in the last place (bit patterns as ordered integers), int64 tensor."""
    def ordered(t):
        b = torch.as_tensor(t).detach().cpu().contiguous()
        assert b.dtype == torch.float16
        b = b.view(torch.int16).long()
        return torch.where(b < 0, -(b & 0x7fff), b)
    return (ordered(got) - ordered(want)).abs()


# --------------------------------------------------------------------------
# the references of tests/test_tree_frame_backward.py: frames of random scene trees, differentiated by CPU autograd on the oracle
# --------------------------------------------------------------------------
# A bare random_spec tree is nearly always an open scene (rays leave it, every gradient is NaN), so each tree stands in a closed
# room; the room is child 0 of the root union and the tree child 1, i.e. the tree's parameters are the "sdfs.1." ones.
TREE_POSE = ((0.98, 0.05, -0.12, 0.03), (0.1, -0.1, -4.0))
NODE_KINDS = ("sphere", "box", "plane", "line", "disk", "torus", "affine", "smooth_union", "union", "rounding", "onion")
_FRAME_REFERENCES = {}


def roomed(tree):
    """``tree`` next to the shell of a 10 x 9 x 11 box in a min-union: a closed scene around the camera of TREE_POSE."""
    room = ("onion", {"radius": torch.tensor(0.1)}, ("box", {"halfsides": torch.tensor([5.0, 4.5, 5.5])}))
    return ("union", {}, [room, tree])


def spec_key(spec):
    """The tree and every parameter value as nested tuples: hashable, equal for equal scenes."""
    kids = spec[2] if len(spec) > 2 else []
    kids = kids if isinstance(kids, list) else [kids]
    prm = tuple((k, tuple(torch.as_tensor(v).detach().double().flatten().tolist())) for k, v in spec[1].items())
    return (spec[0], prm, tuple(spec_key(c) for c in kids))


def frame_weights(h, w):
    return torch.rand(1, h, w, 3, generator=torch.Generator().manual_seed(3 + h + 131 * w))


def pose_tensors(pose, dtype=torch.float32):
    q = torch.nn.functional.normalize(torch.tensor([pose[0]], dtype=torch.float32), dim=-1)
    return q.to(dtype), torch.tensor([pose[1]], dtype=torch.float32).to(dtype)


def frame_loss(image, h, w):
    return (image * frame_weights(h, w).to(device=image.device, dtype=image.dtype)).sum() / (h * w * 3)


def frame_gradients_cpu(spec, h, w, pose, mode, steps, dtype=torch.float32):
    """The oracle's render of a one-camera h x w frame of ``spec`` (parameters rounded to fp32 first, then cast to ``dtype``)
    and CPU autograd of frame_loss through it.  -> (image, {parameter name in O.spec_parameters order, ..., "orientation",
    "translation": gradient}), all detached; a parameter the loss does not reach has a zero gradient.  Cached per (scene, frame,
    pose, mode, steps, dtype): callers must not modify what they get."""
    key = (spec_key(spec), h, w, pose, mode, steps, dtype)
    if key not in _FRAME_REFERENCES:
        live = O.map_spec(spec, lambda x: x.detach().clone().float().to(dtype).requires_grad_(True))
        bufs = tuple(b.to(dtype) for b in O.camera_buffers(1, w, h, PX * h, PX * w, PX * h))
        q, t = (x.requires_grad_(True) for x in pose_tensors(pose, dtype))
        cmap = torch.from_numpy(gold("cmap.npz")["cyclic_cmap"]) if mode in (6, 7) else None
        image = O.render(live, bufs, q, t, mode, 1, steps, EPS, cmap=cmap)
        frame_loss(image, h, w).backward()
        grads = {name: (torch.zeros_like(x) if x.grad is None else x.grad).detach() for name, x in O.spec_parameters(live)}
        for name, x in (("orientation", q), ("translation", t)):
            grads[name] = (torch.zeros_like(x) if x.grad is None else x.grad).detach()
        _FRAME_REFERENCES[key] = (image.detach(), grads)
    return _FRAME_REFERENCES[key]


def admit_frame_case(spec, h, w, pose, mode, steps, tol=1e-4):
    """Whether the oracle alone lets a frame stand as a gradient test.  Admitted when (a) the float32 image has no NaN, (b) the
    float32 and float64 gradients have NaN at the same elements, (c) every tensor has |g32 - g64| <= tol max(1, max|g64|) on its
    finite elements, (d) at least a third of all gradient components are finite and some parameter of the tree -- not only of
    the room -- has a non-zero one.  -> (admitted, reason, largest |g32 - g64| / max(1, max|g64|) over the tensors)."""
    i32, g32 = frame_gradients_cpu(spec, h, w, pose, mode, steps, torch.float32)
    _, g64 = frame_gradients_cpu(spec, h, w, pose, mode, steps, torch.float64)
    if bool(i32.isnan().any()):
        return False, f"{int(i32.isnan().sum())} NaN in the float32 image", float("nan")
    finite = total = 0
    worst, tree = 0.0, False
    for name, a in g32.items():
        a, b = a.double(), g64[name]
        if not torch.equal(a.isnan(), b.isnan()):
            return False, f"{name}: NaN pattern of float32 and float64 differs", float("nan")
        fin = torch.isfinite(a) & torch.isfinite(b)
        total += a.numel()
        finite += int(fin.sum())
        if bool(fin.any()):
            worst = max(worst, float((a - b)[fin].abs().max()) / max(1.0, float(b[fin].abs().max())))
            tree = tree or (name.startswith("sdfs.1.") and bool((a[fin] != 0).any()))
    if worst > tol:
        return False, f"|g32 - g64| is {worst:.3g} of the scale", worst
    if 3 * finite < total:
        return False, f"{finite} of {total} gradient components finite", worst
    if not tree:
        return False, "no parameter of the tree has a non-zero gradient", worst
    return True, "", worst


def spec_nodes(spec, ancestors=()):
    """Every node of the tree with the kinds above it, root first: [(node, (kind of the root, ..., kind of its parent))]."""
    kids = spec[2] if len(spec) > 2 else []
    kids = kids if isinstance(kids, list) else [kids]
    return [(spec, ancestors)] + [x for c in kids for x in spec_nodes(c, ancestors + (spec[0],))]


def spec_shapes(spec):
    """Which of the shapes the reverse pass treats specially occur in ``spec``: a subset of {"union of one", "smooth union of
    one", "rounding over onion", "onion over smooth union", "affine chain of three"} (three affine frames open at once: an affine
    node with two affine nodes among its ancestors)."""
    found = set()
    for node, above in spec_nodes(spec):
        kind = node[0]
        if kind in ("union", "smooth_union") and len(node[2]) == 1:
            found.add("union of one" if kind == "union" else "smooth union of one")
        if kind == "rounding" and node[2][0] == "onion":
            found.add("rounding over onion")
        if kind == "onion" and node[2][0] == "smooth_union":
            found.add("onion over smooth union")
        if kind == "affine" and above.count("affine") >= 2:
            found.add("affine chain of three")
    return found


def generic_lds_floats(cs, block, backward):
    """GenericCfg::lds_floats (csrc/rm_kernels.h) for the compiled scene ``cs``, restated."""
    pb = (cs.n_params + cs.n_derived + 3) & ~3
    prog = 4 * cs.n_instr
    columns = (cs.stack_floats + cs.n_slots) * (block + 1)
    if not backward:
        return pb + prog + columns
    work = columns + (cs.n_params + cs.n_grad_derived) * (block >> 6)
    return pb + max(prog, work)


def generic_block(cs, backward, what=""):
    """The block pick_launch (csrc/rm_abi.hip) gives the interpreter's stand-alone kernels: the largest of 256 (backward: 128),
    ... 64 threads whose LDS fits the default 64 KiB, else 64 with the limit raised.  Prints it."""
    block = 128 if backward else 256
    while block > 64 and 4 * generic_lds_floats(cs, block, backward) > 64 * 1024:
        block >>= 1
    print(f"launch shape {what}: {'backward' if backward else 'forward'} block {block}, "
          f"{4 * generic_lds_floats(cs, block, backward)} B of LDS ({cs.n_params} parameters, {cs.n_instr} instructions)")
    return block
