"""Every bounding sphere the kernels derive (csrc/rm_device.h: subtree_bound, derive_constants) against a float64 walk.

oracle/bound_ref.py restates the walk and the margins of the cull sites and bound tables in float64.  The CPU half checks
that restatement against the oracle's float64 values of random subtrees and against hand-computed numbers; the GPU half
checks that the device derives the same numbers -- rm_scene_bound for single subtrees, the staged block of the frame
kernels for the cull sites and table rows -- that they hold against the device's own fp32 values, and that a child whose
value is NaN everywhere is never culled into a finite pixel."""
import math

import numpy as np
import pytest
import torch

from oracle import bound_ref as B
from oracle import sdf_oracle as O
from tests import helpers as H

DEV = "cuda"
IDENT = [1.0, 0.0, 0.0, 0.0]
INF, NAN = math.inf, math.nan
N_POINTS = 4096


# ----------------------------------------------------------------------------------------------------------------------
# shared pieces
# ----------------------------------------------------------------------------------------------------------------------
def _subtrees(spec):
    yield spec
    kids = spec[2] if len(spec) > 2 else []
    for c in (kids if isinstance(kids, list) else [kids]):
        yield from _subtrees(c)


def _points(c, R, seed=0, n=N_POINTS, extent=6.0):
    """n/2 points uniform in [-extent, extent]^3 and n/2 around the sphere (c, R) in the three thirds of
    extensions.check_bound: a shell around it, the ball inside it, rays out to 8 R + 4.  fp32."""
    gen = torch.Generator().manual_seed(seed)
    h = n // 2
    box = (torch.rand(h, 3, generator=gen) * 2 - 1) * extent
    u = torch.nn.functional.normalize(torch.randn(h, 3, generator=gen), dim=-1)
    rho = torch.rand(h, 1, generator=gen)
    R = abs(float(R))
    radius = torch.where(rho < 1 / 3, R * (1 + 0.1 * (rho * 6 - 1)),
                         torch.where(rho < 2 / 3, R * (rho * 3 - 1), R + (8 * R + 4.0) * (rho * 3 - 2)))
    centre = torch.as_tensor(c, dtype=torch.float64).float()
    return torch.cat([box, centre + radius * u])


def _slacks(f, pts, c, R, slope, Ru, uslope):
    """(f - (slope |p - c| - R),  (uslope |p - c| + Ru) - f) in float64; None where that side has no bound."""
    f, pts = f.reshape(-1).double().cpu(), pts.double().cpu()
    dist = (pts - torch.as_tensor(c, dtype=torch.float64)).norm(dim=-1)
    lower = f - (slope * dist - R) if math.isfinite(R) else None
    upper = (uslope * dist + Ru) - f if math.isfinite(Ru) else None
    return lower, upper


def _holds(slack, tol):
    return slack is None or bool(((slack + tol) >= 0).all())        # (a NaN slack fails)


def _sphere_scale(R, Ru):
    return R if math.isfinite(R) else Ru


def _block64(cs):
    if not cs.leaves:
        return []
    return torch.cat([p.detach().reshape(-1).double().cpu() for p in cs.leaves]).tolist()


def _restated(cs):
    return B.bound(cs.program, _block64(cs), 0, cs.n_instr)


def _sites(program):
    return [pc for pc in range(len(program)) if int(program[pc][0]) == B.OP_CULL_MIN]


def _tables(program):
    return [pc for pc in range(len(program)) if int(program[pc][0]) == B.OP_SMOOTH_BEGIN and int(program[pc][2]) > 0]


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the restatement is true, and its helpers give the numbers worked out by hand
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widened", [False, True])
def test_restatement_bounds_the_float64_oracle(widened):
    """Seeds 5000..5039, as drawn and through helpers.widen_spec: for EVERY subtree of every tree the float64 bound holds
    against the oracle's float64 values at 4096 points (uniform in [-6, 6]^3 and around the sphere), both inequalities, to
    1e-12 (1 + |p| + R): float64 rounding only -- the walk's own inflation factors are its to keep.  Not vacuous: at least
    half of the subtrees have a finite lower bound and a third a finite upper one."""
    from ray_marching_amd.compiler import compile_scene
    n = n_lower = n_upper = 0
    worst, tightest_upper = 0.0, INF
    for seed in range(5000, 5040):
        gen = torch.Generator().manual_seed(seed)
        spec = H.random_spec(gen)
        if widened:
            spec = H.widen_spec(spec, gen)
        for k, sub in enumerate(_subtrees(spec)):
            cs = compile_scene(H.spec_to_module(sub))
            c, R, slope, Ru, uslope = _restated(cs)
            n += 1
            n_lower += math.isfinite(R)
            n_upper += math.isfinite(Ru)
            if not (math.isfinite(R) or math.isfinite(Ru)):
                continue
            pts = _points(c, _sphere_scale(R, Ru), seed=seed * 100 + k).double()
            with torch.no_grad():
                f = O.sdf_eval(O.map_spec(sub, lambda x: x.double()), pts)
            lower, upper = _slacks(f, pts, c, R, slope, Ru, uslope)
            tol = 1e-12 * (1 + pts.norm(dim=-1) + _sphere_scale(R, Ru))
            assert _holds(lower, tol), (seed, k, sub[0], "lower", float(lower.min()))
            assert _holds(upper, tol), (seed, k, sub[0], "upper", float(upper.min()))
            worst = max([worst] + [-float(s.min()) for s in (lower, upper) if s is not None])
            if upper is not None:
                tightest_upper = min(tightest_upper, float(upper.min()))
    print(f"restatement vs oracle (widened={widened}): {n} subtrees, {n_lower} finite lower, {n_upper} finite upper, "
          f"worst violation {worst:.3g}, tightest upper margin {tightest_upper:.3g}")
    assert 2 * n_lower >= n and 3 * n_upper >= n, (n, n_lower, n_upper)


def _compiled(module, monkeypatch, **env):
    from ray_marching_amd.compiler import compile_scene
    for k, v in dict(RM_CULL="1", RM_CULL_MIN_COST="0", **env).items():
        monkeypatch.setenv(k, v)
    return compile_scene(module)


def _K(R, c1):
    return ((R * 1.0001 + 1e-4) + 1e-5 * c1) * 1.000001


def test_cull_site_and_table_helpers_against_hand_computed_numbers(monkeypatch):
    """bound_ref.cull_min_site / smooth_table on scenes whose numbers can be written down: a moved sphere (the numbers of
    test_scene_bound_against_hand_computed_numbers plus the margins of derive_constants), two disjoint spheres (the smallest
    sphere around both, inflated), and one sphere inside the other in both child orders (the larger one, unchanged)."""
    from ray_marching_amd.scene.primitives import SDFPlane, SDFSphere
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A, SDFSmoothUnion, SDFUnion
    rel = lambda x: pytest.approx(x, rel=1e-12, abs=1e-15)
    t = [1.0, -2.0, 3.0]
    moved = lambda r=0.5, at=t: A(SDFSphere(r), orientation=IDENT, translation=at)
    R_moved = 0.5 * 1.0001 + 1e-4 * 6.0            # affine rule: 1.0001 R + 1e-4 |t|_1, slope (1 - 1e-5)

    # a moved sphere behind a plane: one site
    cs = _compiled(SDFUnion([SDFPlane(), moved()]), monkeypatch)
    (pc,) = _sites(cs.program)
    site = B.cull_min_site(cs.program, _block64(cs), pc)
    assert site[:3] == t and site[3] == rel(_K(R_moved, 6.0)) and site[4] == rel((1 - 1e-5) - 2e-4)
    assert int(cs.program[pc][2]) >= cs.n_params           # (where the device puts those 5 floats: the derived block)

    # ... as children of a smooth union with a bound table: rows {c, slope - 2e-4, K, uslope + 2e-4, Ku, 0}
    kids = lambda: [moved()] + [moved(0.25, [float(i), 0.0, 0.0]) for i in range(1, 8)]
    cs = _compiled(SDFUnion([SDFPlane(), SDFSmoothUnion(kids(), 16.0)]), monkeypatch)
    (tb,) = _tables(cs.program)
    rows = B.smooth_table(cs.program, _block64(cs), tb)
    assert len(rows) == 8 and [r[7] for r in rows] == [0.0] * 8
    assert rows[0][:3] == t and rows[0][3] == rel((1 - 1e-5) - 2e-4) and rows[0][5] == rel((1 + 1e-5) + 2e-4)
    assert rows[0][4] == rel(_K(R_moved, 6.0)) and rows[0][6] == rel(_K(R_moved, 6.0))
    for i in range(1, 8):
        Ri = 0.25 * 1.0001 + 1e-4 * i
        assert rows[i][:3] == [float(i), 0.0, 0.0] and rows[i][4] == rel(_K(Ri, i)) and rows[i][6] == rel(_K(Ri, i))
    # the site in front of that smooth union: the fold of the eight spheres, plus log(8) / k
    (pc,) = [p for p in _sites(cs.program) if p < tb]
    site = B.cull_min_site(cs.program, _block64(cs), pc)
    assert math.isfinite(site[3]) and site[4] == rel((1 - 1e-5) - 2e-4)

    # two disjoint spheres (1, 0, 0) r 0.5 and (-2, 0, 0) r 0.25 under identity affine nodes
    cs = _compiled(SDFUnion([SDFPlane(), SDFUnion([moved(0.5, [1.0, 0.0, 0.0]), moved(0.25, [-2.0, 0.0, 0.0])])]), monkeypatch)
    pc = _sites(cs.program)[0]                             # (the outer site; the inner union has one of its own)
    R1, R2 = 0.5 * 1.0001 + 1e-4 * 1.0, 0.25 * 1.0001 + 1e-4 * 2.0
    d = 3.0 * 1.00001
    Rn = 0.5 * ((d + R1) + R2)
    cx = 1.0 + (Rn - R1) / d * -3.0
    R = Rn * 1.00001 + 1e-6 * abs(cx)
    site = B.cull_min_site(cs.program, _block64(cs), pc)
    assert site[0] == rel(cx) and site[1:3] == [0.0, 0.0] and site[3] == rel(_K(R, abs(cx))) and site[4] == rel((1 - 1e-5) - 2e-4)
    assert cx - R < -2.25 and cx + R > 1.5                 # it does enclose both

    # one sphere inside the other, both orders: the enclosing sphere is the larger one, unchanged
    for order in (0, 1):
        pair = [SDFSphere(1.0), moved(0.2, [0.3, 0.0, 0.0])]
        cs = _compiled(SDFUnion([SDFPlane(), SDFUnion(pair[::-1] if order else pair)]), monkeypatch)
        site = B.cull_min_site(cs.program, _block64(cs), _sites(cs.program)[0])
        assert site[:3] == [0.0, 0.0, 0.0] and site[3] == rel(_K(1.0, 0.0)), order
        assert site[4] == rel((1 - 1e-5) - 2e-4)           # the smaller slope of the two children

    # the NaN contract of the restatement, and a user opcode
    for bad in (lambda: SDFSphere(NAN), lambda: moved(NAN), lambda: SDFUnion([SDFSphere(1.0), SDFSphere(NAN)])):
        cs = _compiled(bad(), monkeypatch)
        assert _restated(cs)[1] == INF and _restated(cs)[3] == INF
    with pytest.raises(ValueError, match="not a built-in node"):
        B.bound(np.array([[19, 0, 0, 1]]), [0.5], 0, 1)


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
def _equals_restatement(got, want, what):
    """Device bound == float64 restatement: finite / inf pattern exactly, R, Ru and the slopes to rel 1e-4 (the figure of
    test_scene_bound_against_hand_computed_numbers), the centre to 1e-4 (1 + |c|_1) (the centre margin of AFFINE_POP)."""
    (c, R, slope, Ru, uslope), (c64, R64, slope64, Ru64, uslope64) = got, want
    assert (R == INF) == (R64 == INF) and (Ru == INF) == (Ru64 == INF), (what, got, want)
    assert R == R and Ru == Ru, (what, got)
    if R64 < INF:
        assert R == pytest.approx(R64, rel=1e-4) and slope == pytest.approx(slope64, rel=1e-4), (what, got, want)
    if Ru64 < INF:
        assert Ru == pytest.approx(Ru64, rel=1e-4) and uslope == pytest.approx(uslope64, rel=1e-4), (what, got, want)
    if R64 < INF or Ru64 < INF:
        tol = 1e-4 * (1 + sum(abs(x) for x in c64))
        assert max(abs(float(a) - b) for a, b in zip(c, c64)) <= tol, (what, got, want)


def _device_bound_is_valid(module, got, seed, what):
    """The device's bound against the device's own fp32 values of the subtree, as extensions.check_bound does it:
    4096 points, tolerance 1e-5 (1 + |p| + R), the upper bound too where Ru is finite.  Returns the smallest slacks."""
    c, R, slope, Ru, uslope = got
    if not (math.isfinite(R) or math.isfinite(Ru)):
        return None, None
    scale = _sphere_scale(R, Ru)
    pts = _points(c.tolist(), scale, seed=seed)
    with torch.no_grad():
        f = module(pts.to(DEV))
    lower, upper = _slacks(f, pts, c.tolist(), R, slope, Ru, uslope)
    tol = 1e-5 * (1 + pts.double().norm(dim=-1) + scale)
    for side, slack in (("lower", lower), ("upper", upper)):
        assert _holds(slack, tol), (what, side, got, float(slack.min()), int(slack.isnan().sum()))
    return (None if lower is None else float(lower.min())), (None if upper is None else float(upper.min()))


@pytest.mark.gpu
def test_random_subtrees_bound_equals_restatement_and_holds(monkeypatch):
    """12 random trees through helpers.widen_spec, interpreter: for every subtree, compiled as its own scene, rm_scene_bound
    gives the restatement's numbers, and that bound holds against the kernels' own fp32 values of the subtree."""
    from ray_marching_amd import ops
    from ray_marching_amd.compiler import compile_scene
    monkeypatch.setenv("RM_SPECIALIZE", "off")
    n = n_lower = n_upper = 0
    worst = [INF, INF]
    for seed in range(5000, 5012):
        gen = torch.Generator().manual_seed(seed)
        spec = H.widen_spec(H.random_spec(gen), gen)
        for k, sub in enumerate(_subtrees(spec)):
            module = H.spec_to_module(sub).to(DEV)
            cs = compile_scene(module)
            got = ops.scene_bound(cs, DEV)
            _equals_restatement(got, _restated(cs), (seed, k, sub[0]))
            n += 1
            n_lower += math.isfinite(got[1])
            n_upper += math.isfinite(got[3])
            slacks = _device_bound_is_valid(module, got, seed * 100 + k, (seed, k, sub[0]))
            worst = [w if s is None else min(w, s) for w, s in zip(worst, slacks)]
    print(f"device bounds of random subtrees: {n} subtrees, {n_lower} finite lower, {n_upper} finite upper; smallest slack of "
          f"the untoleranced inequality: lower {worst[0]:.3g}, upper {worst[1]:.3g}")
    assert 2 * n_lower >= n and 3 * n_upper >= n, (n, n_lower, n_upper)


def _quat(s2):
    q = torch.nn.functional.normalize(torch.tensor([0.8, 0.2, -0.4, 0.4], dtype=torch.float64), dim=0) * math.sqrt(s2)
    return q.tolist()


def _chain(depth):
    from ray_marching_amd.scene.primitives import SDFSphere
    from ray_marching_amd.scene.transformations import SDFAffineTransformation as A
    node = SDFSphere(0.5)
    for i in range(depth):
        node = A(node, orientation=_quat(1.0), translation=[0.05 * (i % 3), -0.04, 0.03 * (i % 2)])
    return node


def _edge_cases():
    from ray_marching_amd.scene.primitives import SDFBox, SDFDisk, SDFLine, SDFPlane, SDFSphere, SDFTorus
    from ray_marching_amd.scene.transformations import (SDFAffineTransformation as A, SDFOnion, SDFRounding,
                                                        SDFSmoothUnion, SDFUnion)
    T = [0.4, -0.7, 0.2]
    box = lambda: SDFBox((0.3, 0.5, 0.2))
    cases = {}
    for name, x in (("zero", 0.0), ("negative", -0.25), ("nan", NAN), ("inf", INF)):
        cases[f"sphere_radius_{name}"] = lambda x=x: SDFSphere(x)
        cases[f"box_halfside_{name}"] = lambda x=x: SDFBox((0.3, x, 0.2))
        cases[f"disk_radius_{name}"] = lambda x=x: SDFDisk(x)
        cases[f"torus_tube_{name}"] = lambda x=x: SDFTorus(0.8, x)
        cases[f"torus_ring_{name}"] = lambda x=x: SDFTorus(x, 0.1)
        cases[f"capsule_radius_{name}"] = lambda x=x: SDFLine((-0.5, 0.1, 0.0), (0.6, 0.2, 0.3), x)
        cases[f"blend_k_{name}"] = lambda x=x: SDFSmoothUnion([SDFSphere(0.5), A(box(), IDENT, T)], x)
    for name, x in (("negative", -0.1), ("nan", NAN), ("inf", INF), ("minus_inf", -INF)):
        cases[f"rounding_{name}"] = lambda x=x: SDFRounding(box(), x)
        cases[f"onion_{name}"] = lambda x=x: SDFOnion(SDFSphere(0.5), x)
        cases[f"moved_rounding_{name}"] = lambda x=x: A(SDFRounding(box(), x), _quat(0.9), T)
        cases[f"moved_onion_{name}"] = lambda x=x: A(SDFOnion(box(), x), _quat(0.9), T)
    for s2 in (0.70, 0.80, 1.0, 1.5, 3.9, 4.1):
        cases[f"quaternion_norm2_{s2}"] = lambda s2=s2: A(box(), _quat(s2), T)
        cases[f"quaternion_norm2_{s2}_off_centre"] = lambda s2=s2: A(A(box(), IDENT, [0.5, 0.25, -0.5]), _quat(s2), T)
    cases["quaternion_nan_component"] = lambda: A(box(), [0.9, NAN, 0.1, 0.2], T)
    cases["translation_nan"] = lambda: A(box(), IDENT, [0.4, NAN, 0.2])
    cases["translation_nan_under_onion"] = lambda: SDFOnion(A(box(), IDENT, [0.4, NAN, 0.2]), 0.05)
    cases["union_of_one"] = lambda: SDFUnion([A(box(), _quat(1.1), T)])
    cases["union_with_plane"] = lambda: SDFUnion([SDFSphere(0.5), SDFPlane()])
    cases["union_with_nan_child"] = lambda: SDFUnion([SDFSphere(0.5), SDFSphere(NAN)])
    cases["concentric_spheres"] = lambda: SDFUnion([SDFSphere(0.5), SDFSphere(1.0), SDFSphere(0.75)])
    cases["equal_spheres"] = lambda: SDFUnion([SDFSphere(0.5), SDFSphere(0.5)])
    cases["nested_small_first"] = lambda: SDFUnion([A(SDFSphere(0.2), IDENT, [0.3, 0.0, 0.0]), SDFSphere(1.0)])
    cases["nested_large_first"] = lambda: SDFUnion([SDFSphere(1.0), A(SDFSphere(0.2), IDENT, [0.3, 0.0, 0.0])])
    cases["disjoint_spheres"] = lambda: SDFUnion([A(SDFSphere(0.5), IDENT, [1.0, 0.0, 0.0]), A(SDFSphere(0.25), IDENT, [-2.0, 0.5, 0.0])])
    cases["smooth_union_of_one"] = lambda: SDFSmoothUnion([A(box(), _quat(0.95), T)], 12.0)
    cases["smooth_union_k_negative"] = lambda: SDFSmoothUnion([SDFSphere(0.5), SDFSphere(0.25)], -8.0)
    cases["smooth_union_of_three"] = lambda: SDFSmoothUnion([SDFSphere(0.5), A(box(), IDENT, T), SDFTorus(0.8, 0.1)], 6.0)
    cases["capsule_start_equals_end"] = lambda: SDFLine((0.25, -0.5, 0.75), (0.25, -0.5, 0.75), 0.2)
    cases["moved_capsule_start_equals_end"] = lambda: A(SDFLine((0.25, -0.5, 0.75), (0.25, -0.5, 0.75), 0.2), IDENT, T)
    cases["capsule_nan_end"] = lambda: SDFLine((0.25, -0.5, 0.75), (0.5, NAN, 0.0), 0.2)
    cases["chain_of_12_frames"] = lambda: _chain(12)
    cases["chain_of_13_frames"] = lambda: _chain(13)
    return cases


# cases whose bound must be finite (both sides): the table also pins that the walk does not give up where it need not
_FINITE = {"sphere_radius_zero", "box_halfside_zero", "disk_radius_zero", "torus_tube_zero", "torus_ring_zero", "capsule_radius_zero",
           "rounding_negative", "onion_negative", "moved_rounding_negative", "moved_onion_negative",
           "quaternion_norm2_0.8", "quaternion_norm2_1.0", "quaternion_norm2_1.5", "quaternion_norm2_3.9", "chain_of_12_frames"}
_NO_BOUND = {"quaternion_norm2_0.7", "quaternion_norm2_4.1", "chain_of_13_frames", "union_with_plane", "smooth_union_k_negative",
             "capsule_start_equals_end", "moved_capsule_start_equals_end", "blend_k_inf", "blend_k_zero",
             "rounding_nan", "onion_nan", "moved_rounding_nan", "moved_onion_nan"}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_edge_cases()))
def test_edge_parameters_bound_equals_restatement_and_holds(case, monkeypatch):
    """One node (or a minimal tree) per branch of the walk that random trees never reach: zero, negative, NaN and infinite
    sizes, negative / NaN / infinite rounding and onion, |q|^2 on both sides of the two give-ups, NaN poses, unions of one
    child, with a plane, of concentric and nested spheres, smooth unions of one child and with k <= 0, a capsule of
    length zero, and 12 / 13 nested frames (kBoundDepth = 12: neither the compiler nor rm_validate_program refuses the
    13th, so it is the walk that gives it up as "no bound").  rm_scene_bound equals the restatement and, where it is
    finite, holds against the kernels' own values of that node."""
    from ray_marching_amd import ops
    from ray_marching_amd.compiler import compile_scene
    monkeypatch.setenv("RM_SPECIALIZE", "off")
    module = _edge_cases()[case]().to(DEV)
    cs = compile_scene(module)
    got, want = ops.scene_bound(cs, DEV), _restated(cs)
    print(f"{case}: device {[round(float(x), 6) for x in got[0]]} {got[1:]}, restatement {want[1:]}")
    _equals_restatement(got, want, case)
    if case in _FINITE:
        assert math.isfinite(got[1]) and math.isfinite(got[3]), (case, got)
    if case in _NO_BOUND:
        assert got[1] == INF and got[3] == INF, (case, got)
    _device_bound_is_valid(module, got, 7, case)


def _placed_children(seed=6000, n=9):
    """n random widened subtrees the compiler can bound (no plane), each placed by an affine node; oracle specs."""
    gen = torch.Generator().manual_seed(seed)
    kids = []
    while len(kids) < n:
        sub = H.widen_spec(H.random_spec(gen, depth=2), gen)
        if H.spec_has(sub, "plane"):
            continue
        q = torch.nn.functional.normalize(torch.randn(4, generator=gen), dim=0) * (0.95 + 0.1 * float(torch.rand(1, generator=gen)))
        t = torch.rand(3, generator=gen) * 6 - 3
        kids.append(("affine", {"translation": t, "orientation": q}, sub))
    return kids


def _staged_scene(name):
    """(module, environment of its compilation, the union whose sites / rows are checked for validity)."""
    from ray_marching_amd.scene.scene_registry import make_closed_test_scene, make_many_primitive_scene, make_test_scene2
    if name == "scene2":
        return make_test_scene2(), {}
    if name == "scene1c":
        return make_closed_test_scene(), {}
    if name == "many32":
        return make_many_primitive_scene(32), {}
    if name == "union9":
        return H.spec_to_module(("union", {}, [O.scene_room()] + _placed_children())), dict(RM_CULL_MIN_COST="0")
    assert name == "smooth9"
    blob = ("smooth_union", {"blend_k": torch.tensor(9.0)}, _placed_children())
    return H.spec_to_module(("union", {}, [O.scene_room(), blob])), dict(RM_CULL_MIN_COST="0")


def _entries_equal(got, want, what):
    """Staged floats of a site {c, K, slope} or the lower / upper half of a table row against the helper's float64 numbers."""
    c, K, slope = got[:3], got[3], got[4]
    c64, K64, slope64 = want[:3], want[3], want[4]
    assert math.isnan(K) == math.isnan(K64) and math.isinf(K) == math.isinf(K64), (what, got, want)
    if math.isfinite(K64):
        assert K == pytest.approx(K64, rel=1e-4) and slope == pytest.approx(slope64, rel=1e-4), (what, got, want)
        tol = 1e-4 * (1 + sum(abs(x) for x in c64))
        assert max(abs(a - b) for a, b in zip(c, c64)) <= tol, (what, got, want)


def _margined_slack(child, c, slope_lb, K_lb, slope_ub, K_ub, seed, what):
    """The premise of "cannot change a bit", with NO tolerance: slope_lb |p - c| - K_lb <= child(p) (<= slope_ub |p - c| + K_ub)
    in float64 from the fp32 entries, against the kernels' fp32 values of the child.  Returns the smallest slack of each side
    and the smallest share of the margin 2e-4 |p - c| + 1e-4 (1 + K) that is left."""
    scale = K_lb if math.isfinite(K_lb) else K_ub
    if scale is None or not math.isfinite(scale):
        return [None] * 4                 # "no bound": nothing is promised
    pts = _points(c, scale, seed=seed)
    with torch.no_grad():
        f = child(pts.to(DEV)).reshape(-1).double().cpu()
    dist = (pts.double() - torch.tensor(c, dtype=torch.float64)).norm(dim=-1)
    out = []
    for side, K in (("lower", K_lb), ("upper", K_ub)):
        if K is None or not math.isfinite(K):
            out += [None, None]
            continue
        slack = f - (slope_lb * dist - K_lb) if side == "lower" else (slope_ub * dist + K_ub) - f
        assert bool((slack >= 0).all()), (what, side, float(slack.min()), int(slack.isnan().sum()))
        out += [float(slack.min()), float((slack / (2e-4 * dist + 1e-4 * (1 + K))).min())]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,policy", [(n, "off") for n in ("scene2", "scene1c", "many32", "union9", "smooth9")] +
                         [(n, "prebuilt") for n in ("scene2", "scene1c", "many32")])
def test_staged_cull_sites_and_table_rows(name, policy, monkeypatch):
    """What the FRAME kernels stage (derive_constants: the sites dealt to four walkers, the child ranges of the tables):
    after one 40x72 inference frame the staged block is read back (ops.staged_block: the scene cache of the stream).  Every
    CULL_MIN site and every bound-table row of the program equals bound_ref's float64 numbers (a NaN K, "no bound",
    exactly); for the sites and rows of the outermost union the margined inequality holds WITHOUT tolerance against the
    kernels' own fp32 values of that child at 4096 points.  Interpreter, and the specialised libraries of the shipped scenes."""
    from ray_marching_amd import _abi, ops, specialize
    from ray_marching_amd.compiler import compiled_for
    module, env = _staged_scene(name)
    for k, v in dict(RM_SPECIALIZE=policy, RM_CULL="1", **env).items():
        monkeypatch.setenv(k, v)
    specialize._loaded.clear()
    try:
        loop = H.make_loop(module, 40, 72)
        q, t = H._pose(-3.0)
        with torch.no_grad():
            loop(q, t, 0, 1, 16)
        cs = compiled_for(loop.scene)
        assert (cs.lib() is not _abi.lib) == (policy == "prebuilt"), "specialised library missing: run __graft_entry__.build()"
        block = ops.staged_block(cs, DEV)
        assert block is not None and block.numel() == cs.n_params + cs.n_derived
        block = block.double().cpu().tolist()
        params = block[:cs.n_params]
        assert params == _block64(cs)
        prog = cs.program
        sites, tables = _sites(prog), _tables(prog)
        n_rows = 0
        for pc in sites:
            z = int(prog[pc][2])
            _entries_equal(block[z:z + 5], B.cull_min_site(prog, params, pc), (name, "site", pc))
        for pc in tables:
            z = int(prog[pc][2])
            for j, row in enumerate(B.smooth_table(prog, params, pc)):
                got = block[z + 8 * j:z + 8 * j + 8]
                _entries_equal(got[:3] + [got[4], got[3]], row[:3] + [row[4], row[3]], (name, "row lower", pc, j))
                _entries_equal(got[:3] + [got[6], got[5]], row[:3] + [row[6], row[5]], (name, "row upper", pc, j))
                assert got[7] == 0.0
                n_rows += 1
        if name == "union9":
            assert len(sites) >= 5, "fewer sites than walkers"
        if name in ("many32", "smooth9"):
            assert n_rows >= 9, "no bound table was emitted"
        # validity of what the outermost union tests with: its own sites, and the rows of a smooth union directly under it
        monkeypatch.setenv("RM_SPECIALIZE", "off")
        specialize._loaded.clear()
        depth, worst = 0, [INF] * 4
        for pc in range(len(prog)):
            op = int(prog[pc][0])
            if op == B.OP_CULL_MIN and depth == 1:
                z, child = int(prog[pc][2]), module.sdfs[int(prog[pc][3]) & 255]       # (outermost union: slot = child index)
                got = _margined_slack(child, block[z:z + 3], block[z + 4], block[z + 3], None, None, pc, (name, "site", pc))
                worst = [w if s is None else min(w, s) for w, s in zip(worst, got)]
                nxt = pc + 1
                if int(prog[nxt][0]) == B.OP_SMOOTH_BEGIN and int(prog[nxt][2]) > 0:
                    zt = int(prog[nxt][2])
                    for j, kid in enumerate(child.sdfs):
                        r = block[zt + 8 * j:zt + 8 * j + 8]
                        got = _margined_slack(kid, r[:3], r[3], r[4], r[5], r[6], 1000 * pc + j, (name, "row", nxt, j))
                        worst = [w if s is None else min(w, s) for w, s in zip(worst, got)]
            depth += op in (B.OP_UNION_BEGIN, B.OP_SMOOTH_BEGIN)
            depth -= op in (B.OP_UNION_END, B.OP_SMOOTH_END)
        print(f"staged block of {name} ({policy}): {len(sites)} sites, {n_rows} table rows; smallest slack of the margined inequality: "
              f"lower {worst[0]:.3g} ({worst[1]:.3g} of the margin 2e-4 |p - c| + 1e-4 (1 + K)), upper {worst[2]:.3g} ({worst[3]:.3g} of it)")
        assert worst[0] < INF, "no site of the outermost union was checked"
    finally:
        specialize._loaded.clear()


def _nan_child(which):
    box = ("box", {"halfsides": torch.tensor([0.3, 0.5, 0.2])})
    if which == "rounding_nan":
        return ("rounding", {"rounding": torch.tensor(NAN)}, box)
    if which == "onion_nan":
        return ("onion", {"radius": torch.tensor(NAN)}, ("sphere", {"radius": torch.tensor(0.5)}))
    assert which == "capsule_of_length_zero"
    end = torch.tensor([0.25, -0.5, 0.75])
    return ("line", {"start": end.clone(), "end": end.clone(), "radius": torch.tensor(0.2)})


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["rounding_nan", "onion_nan", "capsule_of_length_zero"])
def test_a_child_that_is_nan_everywhere_is_not_culled(which, monkeypatch):
    """The room shell and one cullable child whose value is NaN at every point (a NaN rounding / onion parameter, a capsule
    with start == end: AB / |AB|^2 = 0 / 0), placed away from the origin.  torch.min propagates the NaN, so the scene is NaN
    everywhere -- compiled without cull tests, with them, and in the oracle: the child must have no bound, or waves far from
    it would skip it and return the room's finite distance.  Points come in wave-coherent clusters of 64 so that whole waves
    do stand where a finite bound would cull."""
    from ray_marching_amd import _abi
    from ray_marching_amd.compiler import compiled_for
    monkeypatch.setenv("RM_SPECIALIZE", "off")
    monkeypatch.setenv("RM_CULL_MIN_COST", "0")
    placed = ("affine", {"translation": torch.tensor([2.0, -1.5, 1.0]), "orientation": torch.tensor([0.9, 0.1, -0.3, 0.2])}, _nan_child(which))
    spec = ("union", {}, [O.scene_room(), placed])
    gen = torch.Generator().manual_seed(78)
    centres = torch.rand(128, 1, 3, generator=gen) * 9 - 4.5
    pts = (centres + 0.05 * torch.randn(128, 64, 3, generator=gen)).reshape(-1, 3)
    q, t = H._pose(-3.0)
    res = {}
    for cull in ("0", "1"):
        monkeypatch.setenv("RM_CULL", cull)
        module = H.spec_to_module(spec).to(DEV)
        loop = H.make_loop(module, 40, 72)
        with torch.no_grad():
            res[cull] = [module(pts.to(DEV))] + [loop(q, t, m, 1, 48) for m in (0, 4)]
        n_sites = int((compiled_for(module).program[:, 0] == _abi.OP_CULL_MIN).sum())
        assert n_sites == (1 if cull == "1" else 0)
    for a, b in zip(res["0"], res["1"]):
        assert H._same(a, b), (which, int(a.isnan().sum()), int(b.isnan().sum()))
    with torch.no_grad():
        want = O.sdf_eval(spec, pts)
    assert bool(want.isnan().all())
    assert torch.equal(res["1"][0].isnan().cpu(), want.isnan())
