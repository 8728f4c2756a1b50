"""Leaves, combinators, domain operators and shaders beyond the reference's vocabulary, added through the public extension point
(extensions.register_leaf / register_combinator / register_warp / register_shader) exactly as a user would add their own: a
PyTorch ``forward`` / ``combine`` / ``warp`` (the CPU path and the oracle) and the same op stream in HIP."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
from torch import Tensor

from .extensions import register_combinator, register_leaf, register_shader, register_warp


class SDFLink(nn.Module):
    """Chain link: a torus of ring radius ``radius1`` and tube radius ``radius2`` in the xy plane, cut across y and
    pulled apart by ``2 * length``.  An exact distance (1-Lipschitz)."""

    def __init__(self, length: float, radius1: float, radius2: float) -> None:
        super().__init__()
        self.length = nn.Parameter(torch.tensor(length, dtype=torch.float32))
        self.radius1 = nn.Parameter(torch.tensor(radius1, dtype=torch.float32))
        self.radius2 = nn.Parameter(torch.tensor(radius2, dtype=torch.float32))

    def forward(self, query_positions: Tensor) -> Tensor:
        stretch = query_positions[..., [1]].abs().sub(self.length)
        ring = torch.linalg.vector_norm(
            torch.cat([query_positions[..., [0]], stretch.where(stretch > 0., 0.)], dim=-1),
            dim=-1, keepdim=True).sub(self.radius1)
        return torch.linalg.vector_norm(
            torch.cat([ring, query_positions[..., [2]]], dim=-1), dim=-1, keepdim=True).sub(self.radius2)


# theta = {length, radius1, radius2}; the forward restates the ATen op stream above (vector_norm of two elements is
# sqrt(fma(b, b, a * a)): norm2_t; x.where(x > 0, 0): t_relu_keep), the VJP is autograd's, written out
_LINK_HIP = r"""
template <bool Fast> RM_DEV float link_fwd(rm::V3 p, const float* theta) {
  const float qy = t_relu_keep(fabsf(p.y) - theta[0]);
  const float ring = norm2_t<Fast>(p.x, qy) - theta[1];
  return norm2_t<Fast>(ring, p.z) - theta[2];
}
template <bool Fast> RM_DEV void link_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) {
  const float a = fabsf(p.y) - theta[0];
  const float qy = t_relu_keep(a);
  const float n1 = norm2_t<Fast>(p.x, qy);
  const float ring = n1 - theta[1];
  const float d0 = norm2_t<Fast>(ring, p.z);
  const float sc = (d0 == 0.0f) ? 0.0f : div_t<Fast>(g, d0);      // norm backward: self * (grad / norm), 0 where norm == 0
  const float gring = ring * sc;
  const float sa = (n1 == 0.0f) ? 0.0f : div_t<Fast>(gring, n1);
  const float ga = (a > 0.0f) ? qy * sa : 0.0f;                   // where(a > 0): gradient only where a > 0
  gp.x += p.x * sa;
  gp.y += ga * sgn0(p.y);
  gp.z += p.z * sc;
  gtheta[0] = -ga;
  gtheta[1] = -gring;
  gtheta[2] = -g;
}
"""

register_leaf(SDFLink, params=("length", "radius1", "radius2"), hip=_LINK_HIP, cost=30)


class SDFBoundedLink(SDFLink):
    """SDFLink with its bounding sphere signed (extensions: NAME_bound), so that cull tests cover it like a built-in
    primitive: the same PyTorch forward, the same HIP op stream under an identifier of its own."""


# the link lies inside the sphere of radius length + radius1 + radius2 around its centre (the stretched ring reaches
# length + radius1 along y, the tube adds radius2), and it is an exact distance: slope 1 both ways
_BLINK_HIP = _LINK_HIP.replace("link_", "blink_") + r"""
RM_DEV void blink_bound(const float* theta, rm::LeafBound& b) {
  if (theta[0] >= 0.0f && theta[1] >= 0.0f && theta[2] >= 0.0f) b.R = b.Ru = theta[0] + theta[1] + theta[2];
}
"""

register_leaf(SDFBoundedLink, params=("length", "radius1", "radius2"), hip=_BLINK_HIP, cost=30)


def make_link_scene(bounded: bool = False):
    """The room of make_test_scene2() around a sphere of 0.5 moved to x = 0.9 and a link placed by an affine node: the
    scene whose specialised library build() compiles, so the shipped leaf renders on a box without a compiler.
    ``bounded``: the link is an SDFBoundedLink, and its affine node gets a cull test like the sphere's."""
    from .scene.primitives import SDFSphere
    from .scene.scene_registry import make_room
    from .scene.transformations import SDFAffineTransformation, SDFUnion
    return SDFUnion([
        make_room(),
        SDFUnion(sdfs=[
            SDFAffineTransformation(SDFSphere(radius=0.5), orientation=[1.0, 0.0, 0.0, 0.0], translation=[0.9, 0.0, 0.0]),
            SDFAffineTransformation((SDFBoundedLink if bounded else SDFLink)(length=0.35, radius1=0.3, radius2=0.08),
                                    orientation=[0.9014, 0.25, 0.25, 0.25], translation=[-0.6, 0.1, 0.2]),
        ]),
    ])


# --------------------------------------------------------------------------------------------------------------------
# CSG combinators (extensions.register_combinator): intersection, subtraction, polynomial smooth subtraction
# --------------------------------------------------------------------------------------------------------------------
class _Combinator(nn.Module):
    """Children in ``sdfs``; ``forward`` stacks their values the way the built-in unions do and hands them to ``combine``."""

    def __init__(self, sdfs) -> None:
        super().__init__()
        self.sdfs = nn.ModuleList(sdfs)

    def forward(self, query_coords: Tensor) -> Tensor:
        return self.combine(torch.stack([sdf(query_coords) for sdf in self.sdfs], dim=-2).squeeze(-1))


class SDFIntersection(_Combinator):
    """max over the children: NaN propagates, the gradient goes to the first child that attains the maximum.  A lower bound
    of the distance to the intersection (1-Lipschitz), exact on its surface."""

    def combine(self, values: Tensor) -> Tensor:
        return values.unsqueeze(-1).max(dim=-2).values


class SDFSubtraction(_Combinator):
    """The first child minus all the others: max(d_0, -d_1, ..., -d_{n-1}), same conventions as SDFIntersection."""

    def combine(self, values: Tensor) -> Tensor:
        return torch.cat([values[..., :1], values[..., 1:].neg()], dim=-1).unsqueeze(-1).max(dim=-2).values


class SDFSmoothSubtraction(_Combinator):
    """``sdfs = [a, b]``: a minus b with a polynomial fillet of width ``blend`` (> 0) instead of the crease -- the smooth maximum
    max(x, y) + h * h * blend / 4, h = relu(blend - |x - y|) / blend, of x = d_a and y = -d_b.  No exp / log."""

    def __init__(self, sdfs, blend: float) -> None:
        super().__init__(sdfs)
        if len(self.sdfs) != 2:
            raise ValueError("SDFSmoothSubtraction takes exactly two children, [a, b]")
        self.blend = nn.Parameter(torch.tensor(blend, dtype=torch.float32))

    def combine(self, values: Tensor) -> Tensor:
        x, y = values[..., 0:1], values[..., 1:2].neg()
        h = self.blend.sub(x.sub(y).abs()).relu().div(self.blend)
        return torch.stack([x, y], dim=-2).max(dim=-2).values.add(h.mul(h).mul(self.blend).div(4.))


# d holds the children's values; each forward restates its combine above op for op (max(dim) is a NaN-propagating maximum:
# t_max; the winner is the first index that attains it, or the first NaN), each VJP is autograd's, written out
_INTERSECTION_HIP = r"""
template <bool Fast, int N> RM_DEV float sdf_intersection_fwd(const float (&d)[N], const float* theta) {
  float m = d[0];
#pragma unroll
  for (int i = 1; i < N; ++i) m = t_max(m, d[i]);
  return m;
}
template <bool Fast, int N> RM_DEV void sdf_intersection_vjp(const float (&d)[N], const float* theta, float g, float (&gd)[N], float* gtheta) {
  float m = d[0];
#pragma unroll
  for (int i = 1; i < N; ++i) m = t_max(m, d[i]);
  bool open = true;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const bool win = open && (d[i] == m || (m != m && d[i] != d[i]));
    gd[i] = win ? g : 0.0f;
    open = open && !win;
  }
}
"""

_SUBTRACTION_HIP = r"""
template <bool Fast, int N> RM_DEV float sdf_subtraction_fwd(const float (&d)[N], const float* theta) {
  float m = d[0];
#pragma unroll
  for (int i = 1; i < N; ++i) m = t_max(m, -d[i]);
  return m;
}
template <bool Fast, int N> RM_DEV void sdf_subtraction_vjp(const float (&d)[N], const float* theta, float g, float (&gd)[N], float* gtheta) {
  float m = d[0];
#pragma unroll
  for (int i = 1; i < N; ++i) m = t_max(m, -d[i]);
  bool open = true;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float x = (i == 0) ? d[i] : -d[i];
    const bool win = open && (x == m || (m != m && x != x));
    gd[i] = win ? ((i == 0) ? g : -g) : 0.0f;
    open = open && !win;
  }
}
"""

# theta = {blend}
_SMOOTH_SUBTRACTION_HIP = r"""
template <bool Fast, int N> RM_DEV float sdf_smooth_subtraction_fwd(const float (&d)[N], const float* theta) {
  static_assert(N == 2, "SDFSmoothSubtraction is binary");
  const float x = d[0], y = -d[1], b = theta[0];
  const float h = t_max(b - fabsf(x - y), 0.0f) / b;
  return t_max(x, y) + ((h * h) * b) / 4.0f;
}
template <bool Fast, int N> RM_DEV void sdf_smooth_subtraction_vjp(const float (&d)[N], const float* theta, float g, float (&gd)[N], float* gtheta) {
  static_assert(N == 2, "SDFSmoothSubtraction is binary");
  const float x = d[0], y = -d[1], b = theta[0];
  const float t = x - y;
  const float r = t_max(b - fabsf(t), 0.0f);
  const float h = div_t<Fast>(r, b);
  const float m = t_max(x, y);
  const float g1 = g / 4.0f;                       // out = m + ((h h) b) / 4
  const float gh = 2.0f * h * (g1 * b);
  const float gr = div_t<Fast>(gh, b);             // h = r / b
  const float ge = (r > 0.0f) ? gr : 0.0f;         // r = relu(e), e = b - |t|
  const float gt = -ge * sgn0(t);
  const bool first = (x == m) || (m != m && x != x);
  const float gx = gt + (first ? g : 0.0f), gy = -gt + (first ? 0.0f : g);
  gd[0] = gx;
  gd[1] = -gy;
  gtheta[0] = (g1 * (h * h) - gh * div_t<Fast>(h, b)) + ge;
}
"""

register_combinator(SDFIntersection, hip=_INTERSECTION_HIP, cost=4)
register_combinator(SDFSubtraction, hip=_SUBTRACTION_HIP, cost=4)
register_combinator(SDFSmoothSubtraction, params=("blend",), hip=_SMOOTH_SUBTRACTION_HIP, cost=30)


def make_carved_scene():
    """The room of make_test_scene2() around two carved solids: a rotated box intersected with a sphere (rounded corners)
    with a capsule-shaped hole drilled through it, and a sphere with a smaller sphere smoothly subtracted.  The scene whose
    specialised library build() compiles, so the shipped combinators render on a box without a compiler."""
    from .scene.primitives import SDFBox, SDFLine, SDFSphere
    from .scene.scene_registry import make_room
    from .scene.transformations import SDFAffineTransformation as A, SDFUnion
    ident = [1.0, 0.0, 0.0, 0.0]
    return SDFUnion([
        make_room(),
        SDFSubtraction([
            SDFIntersection([A(SDFBox(halfsides=(0.5, 0.5, 0.5)), orientation=[0.9014, 0.25, 0.25, 0.25], translation=[-0.7, 0.0, 0.0]),
                             A(SDFSphere(radius=0.66), orientation=ident, translation=[-0.7, 0.0, 0.0])]),
            SDFLine(start=(-1.6, 0.0, 0.0), end=(0.2, 0.0, 0.0), radius=0.22),
        ]),
        SDFSmoothSubtraction([A(SDFSphere(radius=0.5), orientation=ident, translation=[0.9, 0.0, 0.0]),
                              A(SDFSphere(radius=0.35), orientation=ident, translation=[0.9, 0.1, -0.45])], blend=0.15),
    ])


# --------------------------------------------------------------------------------------------------------------------
# Domain operators (extensions.register_warp): uniform scale, mirror symmetry, repetition, elongation
# --------------------------------------------------------------------------------------------------------------------
class _Warp(nn.Module):
    """One child in ``sdf``; ``forward`` evaluates it at ``warp(p)`` and hands its value to ``out`` where the class has one."""

    def __init__(self, sdf) -> None:
        super().__init__()
        self.sdf = sdf

    def forward(self, query_coords: Tensor) -> Tensor:
        values = self.sdf(self.warp(query_coords))
        return self.out(values, query_coords) if hasattr(self, "out") else values


class SDFScale(_Warp):
    """The child scaled uniformly by ``scale`` (> 0) about the origin: ``scale * sdf(p / scale)``, an exact distance where the
    child's is."""

    def __init__(self, sdf, scale: float) -> None:
        super().__init__(sdf)
        self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float32))

    def warp(self, points: Tensor) -> Tensor:
        return points.div(self.scale)

    def out(self, values: Tensor, points: Tensor) -> Tensor:
        return values.mul(self.scale)


class SDFMirror(_Warp):
    """The half x >= ``origin`` of the child, mirrored in the plane x = ``origin`` (wrap it in an affine node for any other
    plane): ``sdf(|p.x - origin|, p.y, p.z)``.  A lower bound of the distance where the child crosses the plane."""

    def __init__(self, sdf, origin: float = 0.0) -> None:
        super().__init__(sdf)
        self.origin = nn.Parameter(torch.tensor(origin, dtype=torch.float32))

    def warp(self, points: Tensor) -> Tensor:
        return torch.cat([points[..., :1].sub(self.origin).abs(), points[..., 1:]], dim=-1)


class SDFRepeat(_Warp):
    """The child repeated without end on the grid of cell size ``period`` (> 0 on every axis): ``sdf(p - period * round(p /
    period))``.  A distance as long as the child stays inside its cell, |x_i| <= period_i / 2, and is symmetric enough that the
    neighbouring cell's copy is never nearer.  ``round`` is half-to-even and has a zero gradient, as in autograd.
    It has no bounded twin: the copies fill all of space, so no sphere holds the surface and every point is within half a cell
    diagonal of a copy -- ``node(p) >= slope |p - c| - R`` fails far from any centre whatever R is."""

    def __init__(self, sdf, period) -> None:
        super().__init__(sdf)
        self.period = nn.Parameter(torch.tensor(period, dtype=torch.float32))

    def warp(self, points: Tensor) -> Tensor:
        return points.sub(self.period.mul(points.div(self.period).round()))


class SDFElongate(_Warp):
    """The child pulled apart by ``2 * halfsides`` (> 0) along the axes: ``sdf(p - clamp(p, -halfsides, halfsides))``.  The map is
    1-Lipschitz, so the field stays a conservative distance."""

    def __init__(self, sdf, halfsides) -> None:
        super().__init__(sdf)
        self.halfsides = nn.Parameter(torch.tensor(halfsides, dtype=torch.float32))

    def warp(self, points: Tensor) -> Tensor:
        return points.sub(points.clamp(self.halfsides.neg(), self.halfsides))


# theta = {scale}.  The forwards are ATen's ops, one rounding each, with a plain `/`: values never go through Fast.  The VJPs
# are the gradients autograd computes (grad / other for the point; for the divisor the sum over the three coordinates, in
# index order, of -grad * self / other^2), not its op stream: ATen groups the divisor's term as -grad * ((self / other) /
# other), which differs in the last bits, far inside the 1e-4 a gradient is held to; `div_t<Fast>` as in the built-in VJPs.
_SCALE_HIP = r"""
template <bool Fast> RM_DEV rm::V3 sdf_scale_fwd(rm::V3 p, const float* theta) {
  return mk3(p.x / theta[0], p.y / theta[0], p.z / theta[0]);
}
template <bool Fast> RM_DEV void sdf_scale_vjp(rm::V3 p, const float* theta, rm::V3 gq, rm::V3& gp, float* gtheta) {
  const float s = theta[0], s2 = s * s;
  gp.x += div_t<Fast>(gq.x, s); gp.y += div_t<Fast>(gq.y, s); gp.z += div_t<Fast>(gq.z, s);
  gtheta[0] = (div_t<Fast>(-gq.x * p.x, s2) + div_t<Fast>(-gq.y * p.y, s2)) + div_t<Fast>(-gq.z * p.z, s2);
}
template <bool Fast> RM_DEV float sdf_scale_out_fwd(float d, rm::V3 p, const float* theta) { return d * theta[0]; }
template <bool Fast> RM_DEV void sdf_scale_out_vjp(float d, rm::V3 p, const float* theta, float g, float& gd, rm::V3& gp, float* gtheta) {
  gd = g * theta[0];
  gtheta[0] = g * d;
}
"""

# theta = {origin}; abs backward is grad * sign(x), 0 at 0: sgn0, as in the box handler
_MIRROR_HIP = r"""
template <bool Fast> RM_DEV rm::V3 sdf_mirror_fwd(rm::V3 p, const float* theta) {
  return mk3(fabsf(p.x - theta[0]), p.y, p.z);
}
template <bool Fast> RM_DEV void sdf_mirror_vjp(rm::V3 p, const float* theta, rm::V3 gq, rm::V3& gp, float* gtheta) {
  const float gx = gq.x * sgn0(p.x - theta[0]);
  gp.x += gx; gp.y += gq.y; gp.z += gq.z;
  gtheta[0] = -gx;
}
"""

# theta = {period[3]}; torch.round is half-to-even: rintf.  round has a zero gradient, so dq/dp = 1 and dq/dperiod_i = -round(.)
_REPEAT_HIP = r"""
template <bool Fast> RM_DEV rm::V3 sdf_repeat_fwd(rm::V3 p, const float* theta) {
  return mk3(p.x - theta[0] * rintf(p.x / theta[0]), p.y - theta[1] * rintf(p.y / theta[1]), p.z - theta[2] * rintf(p.z / theta[2]));
}
template <bool Fast> RM_DEV void sdf_repeat_vjp(rm::V3 p, const float* theta, rm::V3 gq, rm::V3& gp, float* gtheta) {
  gp.x += gq.x; gp.y += gq.y; gp.z += gq.z;
  gtheta[0] = -gq.x * rintf(p.x / theta[0]);
  gtheta[1] = -gq.y * rintf(p.y / theta[1]);
  gtheta[2] = -gq.z * rintf(p.z / theta[2]);
}
"""

# theta = {halfsides[3]}; clamp(x, lo, hi) = min(max(x, lo), hi) with NaN passing: t_clamp.  clamp passes its gradient to x on
# the closed interval [lo, hi] (as the capsule handler notes), to lo where x < lo and to hi where x > hi; lo = -h.
_ELONGATE_HIP = r"""
template <bool Fast> RM_DEV rm::V3 sdf_elongate_fwd(rm::V3 p, const float* theta) {
  return mk3(p.x - t_clamp(p.x, -theta[0], theta[0]), p.y - t_clamp(p.y, -theta[1], theta[1]), p.z - t_clamp(p.z, -theta[2], theta[2]));
}
template <bool Fast> RM_DEV void sdf_elongate_vjp(rm::V3 p, const float* theta, rm::V3 gq, rm::V3& gp, float* gtheta) {
  const float x[3] = {p.x, p.y, p.z}, g[3] = {gq.x, gq.y, gq.z};
  float out[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float h = theta[i];
    const bool inside = (x[i] >= -h) && (x[i] <= h);
    out[i] = inside ? 0.0f : g[i];                       // q = x - clamp(x): 1 - [lo <= x <= hi]
    const bool ordered = -h < h;                          // (autograd's rule for lo >= hi: everything goes to hi)
    const float glo = (ordered && x[i] < -h) ? -g[i] : 0.0f;
    const float ghi = (!ordered || x[i] > h) ? -g[i] : 0.0f;
    gtheta[i] = ghi - glo;
  }
  gp.x += out[0]; gp.y += out[1]; gp.z += out[2];
}
"""

register_warp(SDFScale, params=("scale",), hip=_SCALE_HIP, cost=36)
register_warp(SDFMirror, params=("origin",), hip=_MIRROR_HIP, cost=3)
register_warp(SDFRepeat, params=("period",), hip=_REPEAT_HIP, cost=45)
register_warp(SDFElongate, params=("halfsides",), hip=_ELONGATE_HIP, cost=12)


class SDFBoundedScale(SDFScale):
    """SDFScale with its bound signed (extensions: a warp's NAME_bound maps its child's bound), so that cull tests cover it where
    its child is boundable: the same PyTorch methods, the same HIP op stream under an identifier of its own."""


class SDFBoundedMirror(SDFMirror):
    """SDFMirror with its bound signed: one sphere, centred on the mirror plane, around the child's sphere and its image."""


class SDFBoundedElongate(SDFElongate):
    """SDFElongate with its bound signed: the child's sphere, wider by the length of ``halfsides``."""


# node(p) = s child(p / s) >= s (slope |p / s - c| - R) = slope |p - s c| - s R for s > 0, and the same from above: the child's
# sphere scaled about the origin, slopes unchanged.  s <= 0 (or NaN) is no scale: no bound.
_BSCALE_HIP = _SCALE_HIP.replace("sdf_scale_", "sdf_bscale_") + r"""
RM_DEV void sdf_bscale_bound(const float* theta, rm::LeafBound& b) {
  const float s = theta[0];
  if (s > 0.0f) { b.c = mk3(s * b.c.x, s * b.c.y, s * b.c.z); b.R = s * b.R; b.Ru = s * b.Ru; }
  else b.R = b.Ru = __builtin_inff();
}
"""

# node(p) = child(q), q = (|p.x - o|, p.y, p.z).  With c0 = (0, c.y, c.z):  |q - c0| = |p - (o, c.y, c.z)| and | |q - c| - |q - c0| |
# <= |c.x|, so  child(q) >= slope (|p - c'| - |c.x|) - R >= slope |p - c'| - (R + |c.x|)  (slope <= 1)  and  child(q) <= uslope |p - c'|
# + (Ru + uslope |c.x|)  around c' = (o, c.y, c.z).
_BMIRROR_HIP = _MIRROR_HIP.replace("sdf_mirror_", "sdf_bmirror_") + r"""
RM_DEV void sdf_bmirror_bound(const float* theta, rm::LeafBound& b) {
  const float ax = fabsf(b.c.x);
  b.c.x = theta[0];
  b.R = (theta[0] == theta[0]) ? b.R + ax : __builtin_inff();          // (a NaN plane: no bound, rather than a NaN centre)
  b.Ru = (theta[0] == theta[0]) ? b.Ru + b.uslope * ax : __builtin_inff();
}
"""

# q = p - clamp(p, -h, h) moves a point by at most |h| (every h_i >= 0), so | |q - c| - |p - c| | <= |h|:  child(q) >= slope |p - c|
# - (R + |h|)  and  child(q) <= uslope |p - c| + (Ru + uslope |h|).  |h| is rounded up like the capsule's half length.  A negative
# half-side turns the clamp inside out (the map moves points by more): no bound.
_BELONGATE_HIP = _ELONGATE_HIP.replace("sdf_elongate_", "sdf_belongate_") + r"""
RM_DEV void sdf_belongate_bound(const float* theta, rm::LeafBound& b) {
  const float hx = theta[0], hy = theta[1], hz = theta[2];
  if (hx >= 0.0f && hy >= 0.0f && hz >= 0.0f) {
    const float h = sqrtf(hx * hx + hy * hy + hz * hz) * 1.00001f;
    b.R = b.R + h;
    b.Ru = b.Ru + b.uslope * h;
  } else b.R = b.Ru = __builtin_inff();
}
"""

register_warp(SDFBoundedScale, params=("scale",), hip=_BSCALE_HIP, cost=36)
register_warp(SDFBoundedMirror, params=("origin",), hip=_BMIRROR_HIP, cost=3)
register_warp(SDFBoundedElongate, params=("halfsides",), hip=_BELONGATE_HIP, cost=12)


def make_warped_scene(bounded: bool = False):
    """The room of make_test_scene2() around an arrangement that uses all four operators: a scaled torus and an elongated
    sphere, each placed by an affine node, in a union that is mirrored in the plane x = 0 and lifted by another affine node;
    and a grid of small spheres (SDFRepeat) cut to a slab by an SDFIntersection with a box.  The scene whose specialised
    library build() compiles, so the shipped operators render on a box without a compiler.
    ``bounded``: scale, elongation and mirror are the SDFBounded* classes, so the mirrored pair gets a cull test, and so does
    the scaled torus inside it."""
    from .scene.primitives import SDFBox, SDFSphere, SDFTorus
    from .scene.scene_registry import make_room
    from .scene.transformations import SDFAffineTransformation as A, SDFUnion
    scale, mirror, elongate = (SDFBoundedScale, SDFBoundedMirror, SDFBoundedElongate) if bounded else (SDFScale, SDFMirror, SDFElongate)
    ident = [1.0, 0.0, 0.0, 0.0]
    pair = SDFUnion([
        A(scale(SDFTorus(radius1=0.5, radius2=0.12), scale=0.7), orientation=[0.9014, 0.25, 0.25, 0.25], translation=[0.9, 0.4, 0.2]),
        A(elongate(SDFSphere(radius=0.2), halfsides=(0.05, 0.3, 0.1)), orientation=ident, translation=[0.5, -0.5, -0.3]),
    ])
    return SDFUnion([
        make_room(),
        A(mirror(pair, origin=0.0), orientation=ident, translation=[0.0, 0.2, 0.0]),
        SDFIntersection([SDFRepeat(SDFSphere(radius=0.12), period=(0.5, 0.5, 0.5)),
                         A(SDFBox(halfsides=(1.2, 0.2, 1.2)), orientation=ident, translation=[0.0, -1.4, 0.0])]),
    ])


# --------------------------------------------------------------------------------------------------------------------
# Material nodes: a colour per object (extensions.py: "material nodes")
# --------------------------------------------------------------------------------------------------------------------
from .scene._base import SDFCoordsNode  # noqa: E402


class SDFMaterial(SDFCoordsNode):
    """The child, unchanged, carrying a surface colour: ``SDFMaterial(x)(points) == x(points)`` bit for bit.  ``albedo`` [3] is
    a float32 parameter that no distance depends on; ``surface_albedo`` reads it.  A material node may not sit inside the
    subtree of another one, and in a scene that holds one every subtree no material covers gets the default colour (1, 1, 1)."""
    _rm_kind = "material"

    def __init__(self, sdf: nn.Module, albedo=(1.0, 1.0, 1.0)) -> None:
        super().__init__()
        self.albedo = nn.Parameter(torch.tensor(albedo, dtype=torch.float32))
        self.sdf = sdf
        if self.albedo.shape != (3,):
            raise ValueError(f"SDFMaterial: albedo is (r, g, b), not a tensor of shape {tuple(self.albedo.shape)}")

    def forward(self, query_coords: Tensor) -> Tensor:
        # (CPU points: the child's own forward, where it has one -- the material is the identity)
        return self._evaluate(query_coords) if query_coords.is_cuda else self.sdf(query_coords)


def strip_materials(scene: nn.Module) -> nn.Module:
    """A deep copy of ``scene`` with every SDFMaterial replaced by its child: the geometry alone."""
    import copy
    scene = copy.deepcopy(scene)

    def strip(node):
        while isinstance(node, SDFMaterial):
            node = node.sdf
        for name, child in list(node._modules.items()):
            if child is not None:
                node._modules[name] = strip(child)
        return node

    return strip(scene)


def surface_albedo(scene: nn.Module, points: Tensor) -> Tensor:
    """The surface colour ``m(p) = sum_j a_j c_j / sum_j a_j`` of a scene with material nodes at ``points[..., 3]`` -> ``[..., 3]``
    (float32, on the scene's ROCm device): ``c_j`` the albedo of material ``j`` and ``a_j = |d scene / d(value passing through
    material j)|`` by the rules of the scene's own backward pass -- the winner of a union, the softmax weights of a smooth
    union, whatever a user combinator's VJP says; (1, 1, 1) where the sum is 0.  Differentiable with respect to the albedos
    only: the weights are constants, so the points and the shape parameters receive no gradient (None)."""
    from . import ops
    from .compiler import compiled_for
    cs = compiled_for(scene)
    if not cs.materials:
        raise ValueError("surface_albedo: the scene holds no SDFMaterial")
    if points.shape[-1] != 3:
        raise ValueError(f"points must be [..., 3], got {tuple(points.shape)}")
    return ops.SurfaceAlbedo.apply(points, cs, *(cs.leaves[i] for i, _ in cs.albedo_leaves))


def make_painted_scene():
    """The room of make_test_scene2() around a smooth union (``blend_k = 8``) of that scene's sphere, moved by (0.3, 0.2, 0), its
    torus and its capsule, each under a material of its own, and one on the room: red sphere, green torus, blue capsule, grey
    walls, blending where the smooth union blends."""
    from .scene.primitives import SDFLine, SDFSphere, SDFTorus
    from .scene.scene_registry import make_room
    from .scene.transformations import SDFAffineTransformation, SDFSmoothUnion, SDFUnion
    return SDFUnion([
        SDFMaterial(make_room(), albedo=(0.7, 0.7, 0.7)),
        SDFSmoothUnion(sdfs=[
            SDFMaterial(SDFAffineTransformation(SDFSphere(radius=0.5), orientation=[1.0, 0.0, 0.0, 0.0], translation=[0.3, 0.2, 0.0]),
                        albedo=(0.9, 0.2, 0.2)),
            SDFMaterial(SDFTorus(radius1=1.0, radius2=0.25), albedo=(0.2, 0.8, 0.3)),
            SDFMaterial(SDFLine(start=(1.0, 0.0, 0.0), end=(-1.0, 0.0, 0.0), radius=0.1), albedo=(0.2, 0.3, 0.9)),
        ], blend_k=8.0),
    ])


# --------------------------------------------------------------------------------------------------------------------
# Per-pixel shaders (extensions.register_shader): what lights a user's solid, with parameters of its own to optimise
# --------------------------------------------------------------------------------------------------------------------
class DirectionalLightShader(nn.Module):
    """A distant light and a coloured surface: ``rgb = albedo * (ambient + (1 - ambient) * clamp(n . l / |l|, 0, 1))``.  Seven
    parameter floats (``light_direction`` [3], ``albedo`` [3], ``ambient``); reads only the normal."""

    def __init__(self, light_direction=(0.0, 0.0, -1.0), albedo=(1.0, 1.0, 1.0), ambient: float = 0.1) -> None:
        super().__init__()
        self.light_direction = nn.Parameter(torch.tensor(light_direction, dtype=torch.float32))
        self.albedo = nn.Parameter(torch.tensor(albedo, dtype=torch.float32))
        self.ambient = nn.Parameter(torch.tensor(ambient, dtype=torch.float32))

    def forward(self, px_coords: Tensor, camera_orientation: Tensor, pixel_frames: Tensor, ray_directions: Tensor,
                surface_coords: Tensor, surface_normals: Tensor) -> Tensor:
        light = self.light_direction / torch.linalg.vector_norm(self.light_direction)
        c = (surface_normals * light).sum(dim=-1, keepdim=True).clamp(0, 1)
        return self.albedo * (self.ambient + (1 - self.ambient) * c)


# theta = {light_direction[3], albedo[3], ambient}; the forward restates the ATen op stream above (vector_norm: norm3, mul().sum(-1):
# dot_seq, clamp: t_clamp, every product and sum rounded on its own), the VJP is autograd's, written out
_DIRECTIONAL_HIP = r"""
template <bool Fast> RM_DEV rm::V3 directional_light_fwd(const rm::ShadeIn& s, const float* theta) {
  const rm::V3 L = mk3(theta[0], theta[1], theta[2]);
  const float ln = norm3(L);
  const rm::V3 l = mk3(L.x / ln, L.y / ln, L.z / ln);
  const float c = t_clamp(dot_seq(s.n, l), 0.0f, 1.0f);
  const float k = theta[6] + (1.0f - theta[6]) * c;
  return mk3(theta[3] * k, theta[4] * k, theta[5] * k);
}
template <bool Fast> RM_DEV void directional_light_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta) {
  const rm::V3 L = mk3(theta[0], theta[1], theta[2]);
  const float ln = norm3_t<Fast>(L);
  const rm::V3 l = mk3(div_t<Fast>(L.x, ln), div_t<Fast>(L.y, ln), div_t<Fast>(L.z, ln));
  const float d = dot_seq(s.n, l);
  const float c = t_clamp(d, 0.0f, 1.0f);
  const float k = theta[6] + (1.0f - theta[6]) * c;
  gtheta[3] = g.x * k; gtheta[4] = g.y * k; gtheta[5] = g.z * k;
  const float gk = (g.x * theta[3] + g.y * theta[4]) + g.z * theta[5];
  gtheta[6] = gk - gk * c;
  const float gc = gk * (1.0f - theta[6]);
  const float gd = (d >= 0.0f && d <= 1.0f) ? gc : 0.0f;       // clamp passes the gradient on the closed interval
  gs.n = gs.n + gd * l;
  // l = L / |L|: dL = (gl - l (gl . l)) / |L|
  const rm::V3 gl = gd * s.n;
  const float gll = dot_seq(gl, l);
  gtheta[0] = div_t<Fast>(gl.x - l.x * gll, ln);
  gtheta[1] = div_t<Fast>(gl.y - l.y * gll, ln);
  gtheta[2] = div_t<Fast>(gl.z - l.z * gll, ln);
}
"""

register_shader(DirectionalLightShader, params=("light_direction", "albedo", "ambient"), hip=_DIRECTIONAL_HIP)


class DepthCueShader(nn.Module):
    """The Lambertian term ``c = clamp(-(v . n), 0, 1)`` fading into ``far_colour`` with the distance the ray travelled:
    ``rgb = w * c + (1 - w) * far_colour``, ``w = 1 / (1 + density * |o - p|)``.  Four parameter floats (``density``,
    ``far_colour`` [3]); reads the ray origin, the surface point, the direction and the normal.  No transcendental function."""

    def __init__(self, density: float = 0.25, far_colour=(0.5, 0.6, 0.7)) -> None:
        super().__init__()
        self.density = nn.Parameter(torch.tensor(density, dtype=torch.float32))
        self.far_colour = nn.Parameter(torch.tensor(far_colour, dtype=torch.float32))

    def forward(self, px_coords: Tensor, camera_orientation: Tensor, pixel_frames: Tensor, ray_directions: Tensor,
                surface_coords: Tensor, surface_normals: Tensor) -> Tensor:
        c = (ray_directions * surface_normals).sum(dim=-1, keepdim=True).neg().clamp(0, 1)
        dist = torch.linalg.vector_norm(px_coords - surface_coords, dim=-1, keepdim=True)
        w = (self.density * dist + 1).reciprocal()
        return w * c + (1 - w) * self.far_colour


# theta = {density, far_colour[3]}
_DEPTH_CUE_HIP = r"""
template <bool Fast> RM_DEV rm::V3 depth_cue_fwd(const rm::ShadeIn& s, const float* theta) {
  const float c = t_clamp(-dot_seq(s.v, s.n), 0.0f, 1.0f);
  const float dist = norm3(s.o - s.p);
  const float w = 1.0f / (theta[0] * dist + 1.0f);
  const float wc = w * c, u = 1.0f - w;
  return mk3(wc + u * theta[1], wc + u * theta[2], wc + u * theta[3]);
}
template <bool Fast> RM_DEV void depth_cue_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta) {
  const float e = -dot_seq(s.v, s.n);
  const float c = t_clamp(e, 0.0f, 1.0f);
  const rm::V3 d = s.o - s.p;
  const float dist = norm3_t<Fast>(d);
  const float w = div_t<Fast>(1.0f, theta[0] * dist + 1.0f);
  const float u = 1.0f - w;
  gtheta[1] = g.x * u; gtheta[2] = g.y * u; gtheta[3] = g.z * u;
  const float gsum = (g.x + g.y) + g.z;
  const float gw = gsum * c - ((g.x * theta[1] + g.y * theta[2]) + g.z * theta[3]);
  const float gu = -(gw * (w * w));                            // w = 1 / u', u' = density * dist + 1
  gtheta[0] = gu * dist;
  const float gdist = gu * theta[0];
  const float sc = (dist == 0.0f) ? 0.0f : div_t<Fast>(gdist, dist);   // norm backward: self * (grad / norm), 0 where norm == 0
  const rm::V3 gd = sc * d;
  gs.o = gs.o + gd;
  gs.p = gs.p - gd;
  const float ge = (e >= 0.0f && e <= 1.0f) ? gsum * w : 0.0f;  // clamp passes the gradient on the closed interval
  gs.v = gs.v - ge * s.n;
  gs.n = gs.n - ge * s.v;
}
"""

register_shader(DepthCueShader, params=("density", "far_colour"), hip=_DEPTH_CUE_HIP)


# --------------------------------------------------------------------------------------------------------------------
# Shaders that probe the scene (register_shader(probes=K)): K more distance evaluations around the hit point
# --------------------------------------------------------------------------------------------------------------------
class AmbientOcclusionShader(nn.Module):
    """Fixed-height ambient occlusion on a Lambertian term: five probes at ``p + h_k n``, ``h_k = reach (k+1)/5``; where the
    scene is nearer than the height says, something occludes: ``occ = sum_k 2^-k max(h_k - d_k, 0) / reach`` and
    ``rgb = albedo * clamp(-(v . n), 0, 1) / (1 + strength * occ)``.  Five parameter floats (``reach``, ``strength``, ``albedo``
    [3]); the probe positions depend on the surface point, the normal and ``reach``.  No transcendental function.

    ``scene``: a callable ``points[..., 3] -> [..., 1]`` (an SDF module, or the frame kernels' scene on the GPU)."""

    def __init__(self, reach: float = 0.4, strength: float = 2.0, albedo=(1.0, 1.0, 1.0)) -> None:
        super().__init__()
        self.reach = nn.Parameter(torch.tensor(reach, dtype=torch.float32))
        self.strength = nn.Parameter(torch.tensor(strength, dtype=torch.float32))
        self.albedo = nn.Parameter(torch.tensor(albedo, dtype=torch.float32))

    def forward(self, px_coords: Tensor, camera_orientation: Tensor, pixel_frames: Tensor, ray_directions: Tensor,
                surface_coords: Tensor, surface_normals: Tensor, scene) -> Tensor:
        occ = 0.0
        for k in range(5):
            h = self.reach * ((k + 1) / 5)
            d = scene(surface_coords + h * surface_normals)
            occ = occ + (h - d).clamp(min=0) * (2.0 ** -k) / self.reach
        c = (ray_directions * surface_normals).sum(dim=-1, keepdim=True).neg().clamp(0, 1)
        return self.albedo * (c / (self.strength * occ + 1))


# theta = {reach, strength, albedo[3]}; the forward restates the ATen op stream above (mul().sum(-1): dot_seq, clamp: t_clamp,
# every product and sum rounded on its own), the VJPs are autograd's, written out.  k is a run-time value in the probe pair
# (the kernels' probe loop is rolled) and a constant wherever d / gd are indexed (loops over the five probes are unrolled).
_AMBIENT_OCCLUSION_HIP = r"""
template <bool Fast> RM_DEV rm::V3 ambient_occlusion_probe(int k, const rm::ShadeIn& s, const float* theta) {
  const float h = theta[0] * ((float)(k + 1) / 5.0f);
  return mk3(s.p.x + h * s.n.x, s.p.y + h * s.n.y, s.p.z + h * s.n.z);
}
template <bool Fast> RM_DEV void ambient_occlusion_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, rm::V3 gq, rm::ShadeGrad& gs,
                                                             float* gtheta) {
  const float ck = (float)(k + 1) / 5.0f;
  const float h = theta[0] * ck;
  gs.p = gs.p + gq;
  gs.n = gs.n + h * gq;
  gtheta[0] += dot_seq(gq, s.n) * ck;
}
template <bool Fast> RM_DEV rm::V3 ambient_occlusion_fwd(const rm::ShadeIn& s, const float* theta, const float* d) {
  float occ = 0.0f;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float h = theta[0] * ((float)(k + 1) / 5.0f);
    occ = occ + (t_clamp(h - d[k], 0.0f, __builtin_inff()) * (1.0f / (float)(1 << k))) / theta[0];
  }
  const float c = t_clamp(-dot_seq(s.v, s.n), 0.0f, 1.0f);
  const float shade = c / (theta[1] * occ + 1.0f);
  return mk3(theta[2] * shade, theta[3] * shade, theta[4] * shade);
}
template <bool Fast> RM_DEV void ambient_occlusion_vjp(const rm::ShadeIn& s, const float* theta, const float* d, rm::V3 g, rm::ShadeGrad& gs,
                                                       float* gtheta, float* gd) {
  float occ = 0.0f;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float h = theta[0] * ((float)(k + 1) / 5.0f);
    occ = occ + div_t<Fast>(t_clamp(h - d[k], 0.0f, __builtin_inff()) * (1.0f / (float)(1 << k)), theta[0]);
  }
  const float e = -dot_seq(s.v, s.n);
  const float c = t_clamp(e, 0.0f, 1.0f);
  const float den = theta[1] * occ + 1.0f;
  const float shade = div_t<Fast>(c, den);
  gtheta[2] = g.x * shade; gtheta[3] = g.y * shade; gtheta[4] = g.z * shade;
  const float gshade = (g.x * theta[2] + g.y * theta[3]) + g.z * theta[4];
  const float gc = div_t<Fast>(gshade, den);
  const float gden = -(gc * shade);                            // shade = c / den
  gtheta[1] = gden * occ;
  const float gocc = gden * theta[1];
  const float ge = (e >= 0.0f && e <= 1.0f) ? gc : 0.0f;        // clamp passes the gradient on the closed interval
  gs.v = gs.v - ge * s.n;
  gs.n = gs.n - ge * s.v;
  float greach = 0.0f;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const float ck = (float)(k + 1) / 5.0f, wk = 1.0f / (float)(1 << k);
    const float x = theta[0] * ck - d[k];
    const float term = div_t<Fast>(t_clamp(x, 0.0f, __builtin_inff()) * wk, theta[0]);
    const float gm = (x >= 0.0f) ? div_t<Fast>(gocc * wk, theta[0]) : 0.0f;    // clamp(min=0) passes the gradient at 0
    gd[k] = -gm;
    greach += gm * ck - div_t<Fast>(gocc * term, theta[0]);
  }
  gtheta[0] = greach;
}
"""

register_shader(AmbientOcclusionShader, params=("reach", "strength", "albedo"), hip=_AMBIENT_OCCLUSION_HIP, probes=5)


class SoftShadowShader(nn.Module):
    """A distant light with a fixed-step soft shadow: eight probes at ``p + bias n + t_k l``, ``t_k = reach (k+1)/8``, ``l`` the
    normalised ``light_direction`` (as in DirectionalLightShader); ``shadow = min_k clamp(sharpness d_k / t_k, 0, 1)`` and
    ``rgb = albedo * (ambient + (1 - ambient) * clamp(n . l, 0, 1) * shadow)``.  Nine trainable floats (``light_direction`` [3],
    ``albedo`` [3], ``ambient``, ``sharpness``, ``reach``).

    The gradient of the minimum goes to the one index that PyTorch's ``min(dim)`` reports, the first minimal one; ties occur
    only between clamped values (0 or 1), whose gradient is zero on both sides, so which of them is picked does not matter.
    ``bias`` is a constructor constant, not a trainable parameter: it is kept as a frozen ``nn.Parameter`` (``requires_grad =
    False``) only so that its value travels in ``theta`` like the others; it receives no gradient.  The steps are fixed: a
    marched shadow ray, whose next point depends on the last distance, is what MarchedShadowShader below does with chained
    probes (extensions.py).

    ``scene``: a callable ``points[..., 3] -> [..., 1]``."""

    def __init__(self, light_direction=(0.0, 0.0, -1.0), albedo=(1.0, 1.0, 1.0), ambient: float = 0.15, sharpness: float = 8.0,
                 reach: float = 1.5, bias: float = 0.02) -> None:
        super().__init__()
        self.light_direction = nn.Parameter(torch.tensor(light_direction, dtype=torch.float32))
        self.albedo = nn.Parameter(torch.tensor(albedo, dtype=torch.float32))
        self.ambient = nn.Parameter(torch.tensor(ambient, dtype=torch.float32))
        self.sharpness = nn.Parameter(torch.tensor(sharpness, dtype=torch.float32))
        self.reach = nn.Parameter(torch.tensor(reach, dtype=torch.float32))
        self.bias = nn.Parameter(torch.tensor(bias, dtype=torch.float32), requires_grad=False)

    def forward(self, px_coords: Tensor, camera_orientation: Tensor, pixel_frames: Tensor, ray_directions: Tensor,
                surface_coords: Tensor, surface_normals: Tensor, scene) -> Tensor:
        light = self.light_direction / torch.linalg.vector_norm(self.light_direction)
        start = surface_coords + self.bias * surface_normals
        steps = []
        for k in range(8):
            t = self.reach * ((k + 1) / 8)
            steps.append((self.sharpness * scene(start + t * light) / t).clamp(0, 1))
        shadow = torch.cat(steps, dim=-1).min(dim=-1, keepdim=True).values
        c = (surface_normals * light).sum(dim=-1, keepdim=True).clamp(0, 1)
        return self.albedo * (self.ambient + (1 - self.ambient) * c * shadow)


# theta = {light_direction[3], albedo[3], ambient, sharpness, reach, bias}
_SOFT_SHADOW_HIP = r"""
template <bool Fast> RM_DEV rm::V3 soft_shadow_probe(int k, const rm::ShadeIn& s, const float* theta) {
  const rm::V3 L = mk3(theta[0], theta[1], theta[2]);
  const float ln = norm3(L);
  const rm::V3 l = mk3(L.x / ln, L.y / ln, L.z / ln);
  const float t = theta[8] * ((float)(k + 1) / 8.0f);
  return mk3((s.p.x + theta[9] * s.n.x) + t * l.x, (s.p.y + theta[9] * s.n.y) + t * l.y, (s.p.z + theta[9] * s.n.z) + t * l.z);
}
template <bool Fast> RM_DEV void soft_shadow_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, rm::V3 gq, rm::ShadeGrad& gs,
                                                       float* gtheta) {
  const rm::V3 L = mk3(theta[0], theta[1], theta[2]);
  const float ln = norm3_t<Fast>(L);
  const rm::V3 l = mk3(div_t<Fast>(L.x, ln), div_t<Fast>(L.y, ln), div_t<Fast>(L.z, ln));
  const float ck = (float)(k + 1) / 8.0f;
  const float t = theta[8] * ck;
  gs.p = gs.p + gq;
  gs.n = gs.n + theta[9] * gq;
  gtheta[8] += dot_seq(gq, l) * ck;
  // l = L / |L|: dL = (gl - l (gl . l)) / |L|, gl = t gq
  const rm::V3 gl = t * gq;
  const float gll = dot_seq(gl, l);
  gtheta[0] += div_t<Fast>(gl.x - l.x * gll, ln);
  gtheta[1] += div_t<Fast>(gl.y - l.y * gll, ln);
  gtheta[2] += div_t<Fast>(gl.z - l.z * gll, ln);
}
template <bool Fast> RM_DEV rm::V3 soft_shadow_fwd(const rm::ShadeIn& s, const float* theta, const float* d) {
  const rm::V3 L = mk3(theta[0], theta[1], theta[2]);
  const float ln = norm3(L);
  const rm::V3 l = mk3(L.x / ln, L.y / ln, L.z / ln);
  float shadow = __builtin_inff();
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float t = theta[8] * ((float)(k + 1) / 8.0f);
    shadow = fminf(shadow, t_clamp((theta[7] * d[k]) / t, 0.0f, 1.0f));
  }
  const float c = t_clamp(dot_seq(s.n, l), 0.0f, 1.0f);
  const float k = theta[6] + ((1.0f - theta[6]) * c) * shadow;
  return mk3(theta[3] * k, theta[4] * k, theta[5] * k);
}
template <bool Fast> RM_DEV void soft_shadow_vjp(const rm::ShadeIn& s, const float* theta, const float* d, rm::V3 g, rm::ShadeGrad& gs,
                                                 float* gtheta, float* gd) {
  const rm::V3 L = mk3(theta[0], theta[1], theta[2]);
  const float ln = norm3_t<Fast>(L);
  const rm::V3 l = mk3(div_t<Fast>(L.x, ln), div_t<Fast>(L.y, ln), div_t<Fast>(L.z, ln));
  // the first minimal step, as min(dim) reports it: its index j, the unclamped value xj, its distance dj
  float shadow = __builtin_inff(), xj = 0.0f, dj = 0.0f;
  int j = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float x = div_t<Fast>(theta[7] * d[k], theta[8] * ((float)(k + 1) / 8.0f));
    const float v = t_clamp(x, 0.0f, 1.0f);
    const bool less = v < shadow;
    j = less ? k : j; xj = less ? x : xj; dj = less ? d[k] : dj; shadow = less ? v : shadow;
  }
  const float dn = dot_seq(s.n, l);
  const float c = t_clamp(dn, 0.0f, 1.0f);
  const float lit = (1.0f - theta[6]) * c;
  const float k = theta[6] + lit * shadow;
  gtheta[3] = g.x * k; gtheta[4] = g.y * k; gtheta[5] = g.z * k;
  const float gk = (g.x * theta[3] + g.y * theta[4]) + g.z * theta[5];
  const float glit = gk * shadow, gshadow = gk * lit;
  gtheta[6] = gk - glit * c;
  const float gc = glit * (1.0f - theta[6]);
  const float gdn = (dn >= 0.0f && dn <= 1.0f) ? gc : 0.0f;     // clamp passes the gradient on the closed interval
  gs.n = gs.n + gdn * l;
  const rm::V3 gl = gdn * s.n;
  const float gll = dot_seq(gl, l);
  gtheta[0] = div_t<Fast>(gl.x - l.x * gll, ln);
  gtheta[1] = div_t<Fast>(gl.y - l.y * gll, ln);
  gtheta[2] = div_t<Fast>(gl.z - l.z * gll, ln);
  // shadow = clamp(xj, 0, 1), xj = sharpness dj / tj, tj = reach (j+1)/8
  const float cj = (float)(j + 1) / 8.0f;
  const float tj = theta[8] * cj;
  const float gx = (xj >= 0.0f && xj <= 1.0f) ? gshadow : 0.0f;
  const float gxt = div_t<Fast>(gx, tj);
  gtheta[7] = gxt * dj;
  gtheta[8] = -(gxt * xj) * cj;
  gtheta[9] = 0.0f;                                              // bias: a constant (frozen), no gradient
  const float gdj = gxt * theta[7];
#pragma unroll
  for (int k = 0; k < 8; ++k) gd[k] = (k == j) ? gdj : 0.0f;
}
"""

register_shader(SoftShadowShader, params=("light_direction", "albedo", "ambient", "sharpness", "reach", "bias"), hip=_SOFT_SHADOW_HIP,
                probes=8)


# --------------------------------------------------------------------------------------------------------------------
# Shaders whose probes form a chain (register_shader(probes=K, chained=True)): each probe is placed from the values before it
# --------------------------------------------------------------------------------------------------------------------
class MarchedShadowShader(nn.Module):
    """A distant light with a sphere-traced penumbra shadow: eight probes marched from ``o = p + bias n`` towards the light ``l`` (the
    normalised ``light_direction``), ``t_0 = start``, ``q_k = o + t_k l``, ``d_k = scene(q_k)``, ``t_{k+1} = t_k + clamp(d_k, step_min,
    step_max)``; ``shadow = min_k clamp(sharpness d_k / t_k, 0, 1)`` and ``rgb = albedo * (ambient + (1 - ambient) * clamp(n . l, 0, 1) *
    shadow)``.  The same eight evaluations as SoftShadowShader, spent where the scene says: small steps next to an occluder,
    ``step_max`` in the open.  Nine trainable floats (``light_direction`` [3], ``albedo`` [3], ``ambient``, ``sharpness``, ``start``).

    The gradient of the minimum goes to the first minimal index, as in SoftShadowShader; both clamps pass their gradient on the
    closed interval.  ``bias``, ``step_min`` and ``step_max`` are constructor constants kept as frozen ``nn.Parameter``s
    (``requires_grad = False``) so that their values travel in ``theta``; they receive no gradient.

    ``scene``: a callable ``points[..., 3] -> [..., 1]``."""

    def __init__(self, light_direction=(0.0, 0.0, -1.0), albedo=(1.0, 1.0, 1.0), ambient: float = 0.15, sharpness: float = 8.0,
                 start: float = 0.1, bias: float = 0.02, step_min: float = 0.02, step_max: float = 0.5) -> None:
        super().__init__()
        self.light_direction = nn.Parameter(torch.tensor(light_direction, dtype=torch.float32))
        self.albedo = nn.Parameter(torch.tensor(albedo, dtype=torch.float32))
        self.ambient = nn.Parameter(torch.tensor(ambient, dtype=torch.float32))
        self.sharpness = nn.Parameter(torch.tensor(sharpness, dtype=torch.float32))
        self.start = nn.Parameter(torch.tensor(start, dtype=torch.float32))
        self.bias = nn.Parameter(torch.tensor(bias, dtype=torch.float32), requires_grad=False)
        self.step_min = nn.Parameter(torch.tensor(step_min, dtype=torch.float32), requires_grad=False)
        self.step_max = nn.Parameter(torch.tensor(step_max, dtype=torch.float32), requires_grad=False)

    def forward(self, px_coords: Tensor, camera_orientation: Tensor, pixel_frames: Tensor, ray_directions: Tensor,
                surface_coords: Tensor, surface_normals: Tensor, scene) -> Tensor:
        light = self.light_direction / torch.linalg.vector_norm(self.light_direction)
        origin = surface_coords + self.bias * surface_normals
        t = self.start
        steps = []
        for k in range(8):
            d = scene(origin + t * light)
            steps.append((self.sharpness * d / t).clamp(0, 1))
            if k < 7:
                t = t + d.clamp(self.step_min, self.step_max)
        shadow = torch.cat(steps, dim=-1).min(dim=-1, keepdim=True).values
        c = (surface_normals * light).sum(dim=-1, keepdim=True).clamp(0, 1)
        return self.albedo * (self.ambient + (1 - self.ambient) * c * shadow)


# theta = {light_direction[3], albedo[3], ambient, sharpness, start, bias, step_min, step_max}.  The probe pair sees the chain as the
# history h[i] = d_{k-1-i} (0 behind the start of the chain) and k as a run-time value: t_k = ((start + c_0) + c_1) + ... in the
# order the PyTorch forward adds them, oldest first, i.e. h from its far end -- the entries behind the start are masked by
# `i < k` (clamp(0, step_min, step_max) is step_min, not 0), and adding their 0.0f leaves `start` as it is.  NAME_fwd / NAME_vjp see
# d in probe order and rebuild the t_k the same way; the VJP of the minimum hands the winner's dL/dt_j back to d_0 .. d_{j-1}.
_MARCHED_SHADOW_HIP = r"""
template <bool Fast> RM_DEV rm::V3 marched_shadow_probe(int k, const rm::ShadeIn& s, const float* theta, const float* h) {
  const rm::V3 L = mk3(theta[0], theta[1], theta[2]);
  const float ln = norm3(L);
  const rm::V3 l = mk3(L.x / ln, L.y / ln, L.z / ln);
  float t = theta[8];
#pragma unroll
  for (int i = 6; i >= 0; --i) t = t + ((i < k) ? t_clamp(h[i], theta[10], theta[11]) : 0.0f);
  return mk3((s.p.x + theta[9] * s.n.x) + t * l.x, (s.p.y + theta[9] * s.n.y) + t * l.y, (s.p.z + theta[9] * s.n.z) + t * l.z);
}
template <bool Fast> RM_DEV void marched_shadow_probe_vjp(int k, const rm::ShadeIn& s, const float* theta, const float* h, rm::V3 gq,
                                                          rm::ShadeGrad& gs, float* gtheta, float* gh) {
  const rm::V3 L = mk3(theta[0], theta[1], theta[2]);
  const float ln = norm3_t<Fast>(L);
  const rm::V3 l = mk3(div_t<Fast>(L.x, ln), div_t<Fast>(L.y, ln), div_t<Fast>(L.z, ln));
  float t = theta[8];
#pragma unroll
  for (int i = 6; i >= 0; --i) t = t + ((i < k) ? t_clamp(h[i], theta[10], theta[11]) : 0.0f);
  gs.p = gs.p + gq;
  gs.n = gs.n + theta[9] * gq;
  // t_k = start + sum_{i < k} clamp(h[i], step_min, step_max): the clamp passes the gradient on the closed interval
  const float gt = dot_seq(gq, l);
  gtheta[8] += gt;
#pragma unroll
  for (int i = 0; i < 7; ++i) gh[i] += (i < k && h[i] >= theta[10] && h[i] <= theta[11]) ? gt : 0.0f;
  // l = L / |L|: dL = (gl - l (gl . l)) / |L|, gl = t gq
  const rm::V3 gl = t * gq;
  const float gll = dot_seq(gl, l);
  gtheta[0] += div_t<Fast>(gl.x - l.x * gll, ln);
  gtheta[1] += div_t<Fast>(gl.y - l.y * gll, ln);
  gtheta[2] += div_t<Fast>(gl.z - l.z * gll, ln);
}
template <bool Fast> RM_DEV rm::V3 marched_shadow_fwd(const rm::ShadeIn& s, const float* theta, const float* d) {
  const rm::V3 L = mk3(theta[0], theta[1], theta[2]);
  const float ln = norm3(L);
  const rm::V3 l = mk3(L.x / ln, L.y / ln, L.z / ln);
  float shadow = __builtin_inff(), t = theta[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    shadow = fminf(shadow, t_clamp((theta[7] * d[k]) / t, 0.0f, 1.0f));
    t = t + t_clamp(d[k], theta[10], theta[11]);
  }
  const float c = t_clamp(dot_seq(s.n, l), 0.0f, 1.0f);
  const float k = theta[6] + ((1.0f - theta[6]) * c) * shadow;
  return mk3(theta[3] * k, theta[4] * k, theta[5] * k);
}
template <bool Fast> RM_DEV void marched_shadow_vjp(const rm::ShadeIn& s, const float* theta, const float* d, rm::V3 g, rm::ShadeGrad& gs,
                                                    float* gtheta, float* gd) {
  const rm::V3 L = mk3(theta[0], theta[1], theta[2]);
  const float ln = norm3_t<Fast>(L);
  const rm::V3 l = mk3(div_t<Fast>(L.x, ln), div_t<Fast>(L.y, ln), div_t<Fast>(L.z, ln));
  // the first minimal step, as min(dim) reports it: its index j, the unclamped value xj, its distance dj and its ray parameter tj
  float shadow = __builtin_inff(), xj = 0.0f, dj = 0.0f, tj = 1.0f, t = theta[8];
  int j = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float x = div_t<Fast>(theta[7] * d[k], t);
    const float v = t_clamp(x, 0.0f, 1.0f);
    const bool less = v < shadow;
    j = less ? k : j; xj = less ? x : xj; dj = less ? d[k] : dj; tj = less ? t : tj; shadow = less ? v : shadow;
    t = t + t_clamp(d[k], theta[10], theta[11]);
  }
  const float dn = dot_seq(s.n, l);
  const float c = t_clamp(dn, 0.0f, 1.0f);
  const float lit = (1.0f - theta[6]) * c;
  const float k = theta[6] + lit * shadow;
  gtheta[3] = g.x * k; gtheta[4] = g.y * k; gtheta[5] = g.z * k;
  const float gk = (g.x * theta[3] + g.y * theta[4]) + g.z * theta[5];
  const float glit = gk * shadow, gshadow = gk * lit;
  gtheta[6] = gk - glit * c;
  const float gc = glit * (1.0f - theta[6]);
  const float gdn = (dn >= 0.0f && dn <= 1.0f) ? gc : 0.0f;     // clamp passes the gradient on the closed interval
  gs.n = gs.n + gdn * l;
  const rm::V3 gl = gdn * s.n;
  const float gll = dot_seq(gl, l);
  gtheta[0] = div_t<Fast>(gl.x - l.x * gll, ln);
  gtheta[1] = div_t<Fast>(gl.y - l.y * gll, ln);
  gtheta[2] = div_t<Fast>(gl.z - l.z * gll, ln);
  // shadow = clamp(xj, 0, 1), xj = sharpness dj / tj, tj = start + sum_{i < j} clamp(d_i, step_min, step_max)
  const float gx = (xj >= 0.0f && xj <= 1.0f) ? gshadow : 0.0f;
  const float gxt = div_t<Fast>(gx, tj);
  gtheta[7] = gxt * dj;
  const float gtj = -(gxt * xj);
  gtheta[8] = gtj;
  gtheta[9] = 0.0f; gtheta[10] = 0.0f; gtheta[11] = 0.0f;         // bias, step_min, step_max: constants (frozen), no gradient
  const float gdj = gxt * theta[7];
#pragma unroll
  for (int k = 0; k < 8; ++k)
    gd[k] = ((k == j) ? gdj : 0.0f) + ((k < j && d[k] >= theta[10] && d[k] <= theta[11]) ? gtj : 0.0f);
}
"""

register_shader(MarchedShadowShader, params=("light_direction", "albedo", "ambient", "sharpness", "start", "bias", "step_min", "step_max"),
                hip=_MARCHED_SHADOW_HIP, probes=8, chained=True)


# --------------------------------------------------------------------------------------------------------------------
# Shaders normalised by the frame's min / max (register_shader(normalise="minmax")): a first pass per pixel, the frame's extremes,
# a second pass -- what the reference's distance, proximity and Laplacian modes do, open to users
# --------------------------------------------------------------------------------------------------------------------
class DepthRampShader(nn.Module):
    """A depth ramp that adapts to the scene's extent: ``x = clamp(|o - p|, clip_near, clip_far)``, ``t = (x - min x) / (max x - min x)``
    over every pixel of every camera of the frame, ``rgb = near_colour + t * (far_colour - near_colour)``.  The two colours are
    trainable (six floats); ``clip_near`` and ``clip_far`` are constructor constants kept as frozen ``nn.Parameter``s, so that they
    travel in theta.  No power and no logarithm: its gradients are finite everywhere (the built-in distance mode's ``pow(1 / 2.33)``
    has an infinite slope at the frame's minimum), and a pixel the clamp cuts off passes none.  A frame in which every pixel has
    the same depth (``min == max``) is 0 / 0."""

    def __init__(self, near_colour=(1.0, 0.9, 0.7), far_colour=(0.05, 0.1, 0.3), clip_near: float = 0.0,
                 clip_far: float = float("inf")) -> None:
        super().__init__()
        self.near_colour = nn.Parameter(torch.tensor(near_colour, dtype=torch.float32))
        self.far_colour = nn.Parameter(torch.tensor(far_colour, dtype=torch.float32))
        self.clip_near = nn.Parameter(torch.tensor(clip_near, dtype=torch.float32), requires_grad=False)
        self.clip_far = nn.Parameter(torch.tensor(clip_far, dtype=torch.float32), requires_grad=False)

    def forward(self, px_coords: Tensor, camera_orientation: Tensor, pixel_frames: Tensor, ray_directions: Tensor,
                surface_coords: Tensor, surface_normals: Tensor) -> Tensor:
        x = torch.linalg.vector_norm(px_coords - surface_coords, dim=-1, keepdim=True).clamp(self.clip_near, self.clip_far)
        lo, hi = x.min(), x.max()
        t = (x - lo) / (hi - lo)
        return self.near_colour + t * (self.far_colour - self.near_colour)


# theta = {near_colour[3], far_colour[3], clip_near, clip_far}.  depth_ramp_fwd returns the raw triple (x, 0, 0); the frame takes
# lo = min x, hi = max x; depth_ramp_finish is the ramp.  Its VJP is autograd's, written out: t = a / r with a = x - lo, r = hi - lo,
# so dL/dx = gt / r, dL/dr = -gt a / r^2, dL/dlo = -dL/dx - dL/dr, dL/dhi = dL/dr (this pixel's shares: the kernels sum them).
_DEPTH_RAMP_HIP = r"""
template <bool Fast> RM_DEV rm::V3 depth_ramp_fwd(const rm::ShadeIn& s, const float* theta) {
  return mk3(t_clamp(norm3(s.o - s.p), theta[6], theta[7]), 0.0f, 0.0f);
}
template <bool Fast> RM_DEV void depth_ramp_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 g, rm::ShadeGrad& gs, float* gtheta) {
  const rm::V3 d = s.o - s.p;
  const float dist = norm3_t<Fast>(d);
  const float gdist = (dist >= theta[6] && dist <= theta[7]) ? g.x : 0.0f;   // clamp passes the gradient on the closed interval
  const float sc = (dist == 0.0f) ? 0.0f : div_t<Fast>(gdist, dist);         // norm backward: self * (grad / norm), 0 where norm == 0
  const rm::V3 gd = sc * d;
  gs.o = gs.o + gd;
  gs.p = gs.p - gd;
  gtheta[0] = 0.0f; gtheta[1] = 0.0f; gtheta[2] = 0.0f; gtheta[3] = 0.0f; gtheta[4] = 0.0f; gtheta[5] = 0.0f;   // the colours act in the second pass
  gtheta[6] = 0.0f; gtheta[7] = 0.0f;                                        // clip_near, clip_far: constants (frozen), no gradient
}
template <bool Fast> RM_DEV rm::V3 depth_ramp_finish(rm::V3 raw, float lo, float hi, const float* theta) {
  const float t = (raw.x - lo) / (hi - lo);
  return mk3(theta[0] + t * (theta[3] - theta[0]), theta[1] + t * (theta[4] - theta[1]), theta[2] + t * (theta[5] - theta[2]));
}
template <bool Fast> RM_DEV void depth_ramp_finish_vjp(rm::V3 raw, float lo, float hi, const float* theta, rm::V3 g, rm::V3& graw,
                                                       float& glo, float& ghi, float* gtheta) {
  const float a = raw.x - lo, r = hi - lo;
  const float t = div_t<Fast>(a, r);
  const rm::V3 gd = mk3(g.x * t, g.y * t, g.z * t);               // dL/d(far_colour - near_colour)
  gtheta[0] = g.x - gd.x; gtheta[1] = g.y - gd.y; gtheta[2] = g.z - gd.z;
  gtheta[3] = gd.x; gtheta[4] = gd.y; gtheta[5] = gd.z;
  gtheta[6] = 0.0f; gtheta[7] = 0.0f;
  const float gt = (g.x * (theta[3] - theta[0]) + g.y * (theta[4] - theta[1])) + g.z * (theta[5] - theta[2]);
  const float ga = div_t<Fast>(gt, r);
  const float gr = div_t<Fast>(-gt * a, r * r);
  graw = mk3(ga, 0.0f, 0.0f);
  ghi = gr;
  glo = -ga - gr;
}
"""

register_shader(DepthRampShader, params=("near_colour", "far_colour", "clip_near", "clip_far"), hip=_DEPTH_RAMP_HIP, normalise="minmax")


# --------------------------------------------------------------------------------------------------------------------
# Shaders that read a lookup table (register_shader(table=..., table_taps=T)): storage a shader may index at run time, and
# whose rows take gradients through a deterministic scatter
# --------------------------------------------------------------------------------------------------------------------
class TangentPaletteShader(nn.Module):
    """The built-in tangent mode (mode 6 at degree 1) restated as a user shader: the normal's tangential part, rotated into the
    camera frame, colours the pixel with ``brightness * palette[floor((atan2(im, re) / tau + 0.5) * L) mod L]``.  The ``palette`` ([L, 3]
    float32, ``2 <= L <= 4096``) is a Parameter: where the built-in mode reads a fixed colormap, this one learns its rows (one row
    per pixel: ``table_taps=1``).  No ``theta``."""

    def __init__(self, palette) -> None:
        super().__init__()
        self.palette = nn.Parameter(torch.as_tensor(palette, dtype=torch.float32).clone().contiguous())

    def forward(self, px_coords: Tensor, camera_orientation: Tensor, pixel_frames: Tensor, ray_directions: Tensor,
                surface_coords: Tensor, surface_normals: Tensor) -> Tensor:
        from .quaternion import conjugate, rotation
        n, v = surface_normals, ray_directions
        tangential = ((n * v).sum(dim=-1, keepdim=True) * v) * (-1.0) + n
        proj = rotation(tangential, conjugate(camera_orientation)[:, None, None, :])
        re, im = proj[..., 0], proj[..., 1]
        bright = torch.stack((re, im), dim=-1).pow(2).sum(dim=-1, keepdim=True).pow(1 / 2)
        size = self.palette.shape[0]
        idx = (torch.atan2(im, re) / math.tau + 0.5) * 1 * size
        return bright * self.palette[idx.floor().long().remainder(size), :]


# the forward is shade_pixel's RM_MODE_TANGENT case and domain_colour, the VJP shade_pixel_vjp's tangent branch, op for op; the row
# index is piecewise constant (no gradient through it), the row itself takes brightness * g
_TANGENT_PALETTE_HIP = r"""
template <bool Fast> RM_DEV rm::V3 tangent_palette_fwd(const rm::ShadeIn& s, const float* theta, const rm::Table& tab) {
  const float c = dot_seq(s.n, s.v);
  const rm::V3 tg = mk3((c * s.v.x) * -1.0f + s.n.x, (c * s.v.y) * -1.0f + s.n.y, (c * s.v.z) * -1.0f + s.n.z);
  const rm::V3 pr = qrot(tg, s.qw, neg(s.qv));
  const rm::Shaded sh = domain_colour(pr.x, pr.y, tab.n, 1);
  const rm::V3 row = tab.row(sh.idx);
  return mk3(sh.bright * row.x, sh.bright * row.y, sh.bright * row.z);
}
template <bool Fast> RM_DEV void tangent_palette_vjp(const rm::ShadeIn& s, const float* theta, const rm::Table& tab, rm::V3 g,
                                                     rm::ShadeGrad& gs, float* gtheta, rm::TableGrad& gt) {
  const float c = dot_seq(s.n, s.v);
  const rm::V3 tg = mk3((c * s.v.x) * -1.0f + s.n.x, (c * s.v.y) * -1.0f + s.n.y, (c * s.v.z) * -1.0f + s.n.z);
  const rm::V3 u = neg(s.qv);                 // rotation by conj(q): local = tg + w t + u x t, t = 2 u x tg
  const rm::V3 pr = qrot(tg, s.qw, u);
  const rm::Shaded sh = domain_colour(pr.x, pr.y, tab.n, 1);
  const rm::V3 row = tab.row(sh.idx);
  gt.row[0] = tab.clamp(sh.idx);
  gt.g[0] = mk3(sh.bright * g.x, sh.bright * g.y, sh.bright * g.z);
  const float gb = (g.x * row.x + g.y * row.y) + g.z * row.z;
  const float gsq = gb * (0.5f / sh.bright);  // brightness = (re^2 + im^2).pow(1/2)
  const rm::V3 gl = mk3(gsq * (2.0f * pr.x), gsq * (2.0f * pr.y), 0.0f);
  const rm::V3 t = 2.0f * cross(u, tg);
  const rm::V3 ugl = cross(u, gl);
  const rm::V3 gtg = (gl + 2.0f * cross(u, ugl)) - (2.0f * s.qw) * ugl;
  const rm::V3 gtt = s.qw * gl + cross(gl, u);
  const rm::V3 gu = cross(t, gl) + 2.0f * cross(tg, gtt);
  gs.qw += (gl.x * t.x + gl.y * t.y) + gl.z * t.z;
  gs.qv = gs.qv - gu;
  const float gtv = dot_seq(gtg, s.v);        // tg = n - (n.v) v
  gs.n = gs.n + mk3(gtg.x - gtv * s.v.x, gtg.y - gtv * s.v.y, gtg.z - gtv * s.v.z);
  gs.v = gs.v + mk3(-c * gtg.x - gtv * s.n.x, -c * gtg.y - gtv * s.n.y, -c * gtg.z - gtv * s.n.z);
}
"""

register_shader(TangentPaletteShader, hip=_TANGENT_PALETTE_HIP, table="palette", table_taps=1)


class DepthPaletteShader(nn.Module):
    """A transfer function over depth: ``rgb = c * lerp(palette[i], palette[i + 1], u - i)`` with ``u = (L - 1) / (1 + density * |o - p|)``
    (near: the last row, far: the first), ``i = min(floor(u), L - 2)`` and the Lambertian term ``c = clamp(-(v . n), 0, 1)``.  One
    parameter float (``density``) and the ``palette`` ([L, 3] float32, a Parameter); gradients go to ``density``, the pose, the scene
    and both rows (``table_taps=2``).  Continuous in ``u``; its slope jumps at the knots."""

    def __init__(self, density: float = 0.25, palette=((0.1, 0.2, 0.5), (1.0, 0.9, 0.7))) -> None:
        super().__init__()
        self.density = nn.Parameter(torch.tensor(density, dtype=torch.float32))
        self.palette = nn.Parameter(torch.as_tensor(palette, dtype=torch.float32).clone().contiguous())

    def forward(self, px_coords: Tensor, camera_orientation: Tensor, pixel_frames: Tensor, ray_directions: Tensor,
                surface_coords: Tensor, surface_normals: Tensor) -> Tensor:
        c = (ray_directions * surface_normals).sum(dim=-1, keepdim=True).neg().clamp(0, 1)
        dist = torch.linalg.vector_norm(px_coords - surface_coords, dim=-1, keepdim=True)
        size = self.palette.shape[0]
        u = (size - 1) * (self.density * dist + 1).reciprocal()
        i = u.detach().floor().clamp(0, size - 2)
        f = u - i
        lo, hi = self.palette[i.long().squeeze(-1)], self.palette[i.long().squeeze(-1) + 1]
        return c * (lo + f * (hi - lo))


# theta = {density}
_DEPTH_PALETTE_HIP = r"""
template <bool Fast> RM_DEV rm::V3 depth_palette_fwd(const rm::ShadeIn& s, const float* theta, const rm::Table& tab) {
  const float c = t_clamp(-dot_seq(s.v, s.n), 0.0f, 1.0f);
  const float dist = norm3(s.o - s.p);
  const float top = (float)(tab.n - 1);
  const float u = top * (1.0f / (theta[0] * dist + 1.0f));
  const float fi = t_clamp(floorf(u), 0.0f, top - 1.0f);
  const float f = u - fi;
  const int i = (int)fi;
  const rm::V3 lo = tab.row(i), hi = tab.row(i + 1);
  return mk3(c * (lo.x + f * (hi.x - lo.x)), c * (lo.y + f * (hi.y - lo.y)), c * (lo.z + f * (hi.z - lo.z)));
}
template <bool Fast> RM_DEV void depth_palette_vjp(const rm::ShadeIn& s, const float* theta, const rm::Table& tab, rm::V3 g,
                                                   rm::ShadeGrad& gs, float* gtheta, rm::TableGrad& gt) {
  const float e = -dot_seq(s.v, s.n);
  const float c = t_clamp(e, 0.0f, 1.0f);
  const rm::V3 d = s.o - s.p;
  const float dist = norm3_t<Fast>(d);
  const float top = (float)(tab.n - 1);
  const float w = div_t<Fast>(1.0f, theta[0] * dist + 1.0f);
  const float u = top * w;
  const float fi = t_clamp(floorf(u), 0.0f, top - 1.0f);
  const float f = u - fi;
  const int i = (int)fi;
  const rm::V3 lo = tab.row(i), hi = tab.row(i + 1);
  const rm::V3 dl = hi - lo;
  const rm::V3 mix = mk3(lo.x + f * dl.x, lo.y + f * dl.y, lo.z + f * dl.z);
  const rm::V3 gm = c * g;                                    // dL/d(mix)
  gt.row[0] = tab.clamp(i);     gt.g[0] = gm - f * gm;        // lo takes (1 - f), as autograd's lo + f * (hi - lo) hands it over
  gt.row[1] = tab.clamp(i + 1); gt.g[1] = f * gm;
  const float gf = (gm.x * dl.x + gm.y * dl.y) + gm.z * dl.z;
  const float gw = gf * top;                                  // u = top * w; floor(u) carries no gradient
  const float gup = -(gw * (w * w));                          // w = 1 / u', u' = density * dist + 1
  gtheta[0] = gup * dist;
  const float gdist = gup * theta[0];
  const float sc = (dist == 0.0f) ? 0.0f : div_t<Fast>(gdist, dist);   // norm backward: self * (grad / norm), 0 where norm == 0
  const rm::V3 gd = sc * d;
  gs.o = gs.o + gd;
  gs.p = gs.p - gd;
  const float gc = (g.x * mix.x + g.y * mix.y) + g.z * mix.z;
  const float ge = (e >= 0.0f && e <= 1.0f) ? gc : 0.0f;      // clamp passes the gradient on the closed interval
  gs.v = gs.v - ge * s.n;
  gs.n = gs.n - ge * s.v;
}
"""

register_shader(DepthPaletteShader, params=("density",), hip=_DEPTH_PALETTE_HIP, table="palette", table_taps=2)


class MaterialLambertShader(nn.Module):
    """The Lambertian term on the surface colour of the scene's material nodes (SDFMaterial): ``rgb = m * (ambient + (1 - ambient)
    * clamp(-(v . n), 0, 1))``.  One parameter float (``ambient``); reads the direction, the normal and the material colour ``m``,
    which is (1, 1, 1) on a scene without material nodes."""

    def __init__(self, ambient: float = 0.1) -> None:
        super().__init__()
        self.ambient = nn.Parameter(torch.tensor(ambient, dtype=torch.float32))

    def forward(self, px_coords: Tensor, camera_orientation: Tensor, pixel_frames: Tensor, ray_directions: Tensor,
                surface_coords: Tensor, surface_normals: Tensor, material: Tensor) -> Tensor:
        c = (ray_directions * surface_normals).sum(dim=-1, keepdim=True).neg().clamp(0, 1)
        return material * (self.ambient + (1 - self.ambient) * c)


# theta = {ambient}; the forward restates the ATen op stream above (mul().sum(-1): dot_seq, neg, clamp: t_clamp, every product and
# sum rounded on its own), the VJP is autograd's, written out; gm = dL/dm
_MATERIAL_LAMBERT_HIP = r"""
template <bool Fast> RM_DEV rm::V3 material_lambert_fwd(const rm::ShadeIn& s, const float* theta, rm::V3 m) {
  const float c = t_clamp(-dot_seq(s.v, s.n), 0.0f, 1.0f);
  const float k = theta[0] + (1.0f - theta[0]) * c;
  return mk3(m.x * k, m.y * k, m.z * k);
}
template <bool Fast> RM_DEV void material_lambert_vjp(const rm::ShadeIn& s, const float* theta, rm::V3 m, rm::V3 g, rm::ShadeGrad& gs,
                                                      float* gtheta, rm::V3& gm) {
  const float d = -dot_seq(s.v, s.n);
  const float c = t_clamp(d, 0.0f, 1.0f);
  const float k = theta[0] + (1.0f - theta[0]) * c;
  gm = mk3(g.x * k, g.y * k, g.z * k);
  const float gk = (g.x * m.x + g.y * m.y) + g.z * m.z;
  gtheta[0] = gk - gk * c;
  const float gc = gk * (1.0f - theta[0]);
  const float gd = (d >= 0.0f && d <= 1.0f) ? gc : 0.0f;       // clamp passes the gradient on the closed interval
  gs.n = gs.n + mk3(-gd * s.v.x, -gd * s.v.y, -gd * s.v.z);
  gs.v = gs.v + mk3(-gd * s.n.x, -gd * s.n.y, -gd * s.n.z);
}
"""

register_shader(MaterialLambertShader, params=("ambient",), hip=_MATERIAL_LAMBERT_HIP, material=True)


# --------------------------------------------------------------------------------------------------------------------
# Shaders that trace a secondary ray (register_shader(trace=S)): the frame kernels sphere-trace it and hand back the hit
# --------------------------------------------------------------------------------------------------------------------
class MirrorShader(nn.Module):
    """A distant light on a partly mirroring surface: the primary ray is reflected at the hit point, ``v2 = v - 2 (v . n) n`` from
    ``o2 = p + bias n``, and sphere-traced 24 steps through the scene.  With ``c(n) = ambient + (1 - ambient) clamp(-(l . n), 0, 1)``,
    the directional-light term for the normalised ``light_direction`` ``l``, and the hit weight ``w = clamp(1 - h.d / hit_eps, 0, 1)`` of
    the secondary ray's end point (1 on a surface, 0 where the scene is further than ``hit_eps`` away), the pixel is

        rgb = (1 - reflectivity) c(n) + reflectivity (w c(h.n) + (1 - w) sky).

    Eight trainable floats (``reflectivity``, ``light_direction`` [3], ``ambient``, ``sky`` [3]); ``bias`` and ``hit_eps`` are constructor
    constants kept as frozen ``nn.Parameter``s (``requires_grad = False``) so that their values travel in ``theta``.  Both clamps pass
    their gradient on the closed interval.  No transcendental function.

    ``trace``: a callable ``(origins[..., 3], directions[..., 3]) -> (points, normals, values[..., 1])`` (extensions.reference_trace)."""

    def __init__(self, reflectivity: float = 0.5, light_direction=(0.0, 0.0, 1.0), ambient: float = 0.15, sky=(0.5, 0.6, 0.8),
                 bias: float = 0.05, hit_eps: float = 0.25) -> None:
        super().__init__()
        self.reflectivity = nn.Parameter(torch.tensor(reflectivity, dtype=torch.float32))
        self.light_direction = nn.Parameter(torch.tensor(light_direction, dtype=torch.float32))
        self.ambient = nn.Parameter(torch.tensor(ambient, dtype=torch.float32))
        self.sky = nn.Parameter(torch.tensor(sky, dtype=torch.float32))
        self.bias = nn.Parameter(torch.tensor(bias, dtype=torch.float32), requires_grad=False)
        self.hit_eps = nn.Parameter(torch.tensor(hit_eps, dtype=torch.float32), requires_grad=False)

    def forward(self, px_coords: Tensor, camera_orientation: Tensor, pixel_frames: Tensor, ray_directions: Tensor,
                surface_coords: Tensor, surface_normals: Tensor, trace) -> Tensor:
        light = self.light_direction / torch.linalg.vector_norm(self.light_direction)

        def lit(normals):
            return self.ambient + (1 - self.ambient) * (normals * light).sum(dim=-1, keepdim=True).neg().clamp(0, 1)

        vn = (ray_directions * surface_normals).sum(dim=-1, keepdim=True)
        _, hit_normals, hit_values = trace(surface_coords + self.bias * surface_normals, ray_directions - (2 * vn) * surface_normals)
        w = (1 - hit_values / self.hit_eps).clamp(0, 1)
        reflected = w * lit(hit_normals) + (1 - w) * self.sky
        return (1 - self.reflectivity) * lit(surface_normals) + self.reflectivity * reflected


# theta = {reflectivity, light_direction[3], ambient, sky[3], bias, hit_eps}; the forward restates the ATen op stream above, the two
# VJPs are autograd's, written out (NAME_vjp writes gtheta, NAME_ray_vjp adds to it: bias and hit_eps are frozen and get nothing)
_MIRROR_SHADER_HIP = r"""
template <bool Fast> RM_DEV void mirror_ray(const rm::ShadeIn& s, const float* theta, rm::TraceRay& r) {
  const float k = 2.0f * dot_seq(s.v, s.n);
  r.o = mk3(s.p.x + theta[8] * s.n.x, s.p.y + theta[8] * s.n.y, s.p.z + theta[8] * s.n.z);
  r.v = mk3(s.v.x - k * s.n.x, s.v.y - k * s.n.y, s.v.z - k * s.n.z);
}
template <bool Fast> RM_DEV void mirror_ray_vjp(const rm::ShadeIn& s, const float* theta, const rm::TraceRay& gr, rm::ShadeGrad& gs,
                                                float* gtheta) {
  // o2 = p + bias n
  gs.p = gs.p + gr.o;
  gs.n = gs.n + theta[8] * gr.o;
  // v2 = v - k n, k = 2 (v . n)
  const float k = 2.0f * dot_seq(s.v, s.n);
  const float gk = -dot_seq(gr.v, s.n);
  const float gvn = 2.0f * gk;
  gs.v = (gs.v + gr.v) + gvn * s.n;
  gs.n = (gs.n - k * gr.v) + gvn * s.v;
}
template <bool Fast> RM_DEV rm::V3 mirror_fwd(const rm::ShadeIn& s, const float* theta, const rm::TraceHit& h) {
  const rm::V3 L = mk3(theta[1], theta[2], theta[3]);
  const float ln = norm3(L);
  const rm::V3 l = mk3(L.x / ln, L.y / ln, L.z / ln);
  const float a = theta[4];
  const float cs = a + (1.0f - a) * t_clamp(-dot_seq(s.n, l), 0.0f, 1.0f);
  const float ch = a + (1.0f - a) * t_clamp(-dot_seq(h.n, l), 0.0f, 1.0f);
  const float w = t_clamp(1.0f - h.d / theta[9], 0.0f, 1.0f);
  const float wc = w * ch, u = 1.0f - w;
  const float local = (1.0f - theta[0]) * cs;
  return mk3(local + theta[0] * (wc + u * theta[5]), local + theta[0] * (wc + u * theta[6]), local + theta[0] * (wc + u * theta[7]));
}
template <bool Fast> RM_DEV void mirror_vjp(const rm::ShadeIn& s, const float* theta, const rm::TraceHit& h, rm::V3 g, rm::ShadeGrad& gs,
                                            float* gtheta, rm::TraceGrad& gh) {
  const rm::V3 L = mk3(theta[1], theta[2], theta[3]);
  const float ln = norm3_t<Fast>(L);
  const rm::V3 l = mk3(div_t<Fast>(L.x, ln), div_t<Fast>(L.y, ln), div_t<Fast>(L.z, ln));
  const float a = theta[4], rho = theta[0];
  const float es = -dot_seq(s.n, l), eh = -dot_seq(h.n, l);
  const float ms = t_clamp(es, 0.0f, 1.0f), mh = t_clamp(eh, 0.0f, 1.0f);
  const float cs = a + (1.0f - a) * ms, ch = a + (1.0f - a) * mh;
  const float x = 1.0f - div_t<Fast>(h.d, theta[9]);
  const float w = t_clamp(x, 0.0f, 1.0f), u = 1.0f - w;
  const float wc = w * ch;
  const float gsum = (g.x + g.y) + g.z;
  // rgb = (1 - rho) cs + rho refl, refl = w ch + (1 - w) sky
  gtheta[0] = ((g.x * (wc + u * theta[5]) + g.y * (wc + u * theta[6])) + g.z * (wc + u * theta[7])) - gsum * cs;
  const float gcs = gsum * (1.0f - rho);
  const rm::V3 gr = rho * g;
  gtheta[5] = gr.x * u; gtheta[6] = gr.y * u; gtheta[7] = gr.z * u;
  const float grs = (gr.x + gr.y) + gr.z;
  const float gch = grs * w;
  const float gw = grs * ch - ((gr.x * theta[5] + gr.y * theta[6]) + gr.z * theta[7]);
  // w = clamp(1 - d / hit_eps, 0, 1): the clamp passes the gradient on the closed interval
  const float gx = (x >= 0.0f && x <= 1.0f) ? gw : 0.0f;
  gh.d = -div_t<Fast>(gx, theta[9]);
  // c = a + (1 - a) m, m = clamp(e, 0, 1), e = -(n . l), for the surface normal and for the hit's
  gtheta[4] = (gcs - gcs * ms) + (gch - gch * mh);
  const float gms = gcs * (1.0f - a), gmh = gch * (1.0f - a);
  const float ges = (es >= 0.0f && es <= 1.0f) ? gms : 0.0f;
  const float geh = (eh >= 0.0f && eh <= 1.0f) ? gmh : 0.0f;
  gs.n = gs.n - ges * l;
  gh.n = gh.n - geh * l;
  // l = L / |L|: dL = (gl - l (gl . l)) / |L|
  const rm::V3 gl = neg(ges * s.n + geh * h.n);
  const float gll = dot_seq(gl, l);
  gtheta[1] = div_t<Fast>(gl.x - l.x * gll, ln);
  gtheta[2] = div_t<Fast>(gl.y - l.y * gll, ln);
  gtheta[3] = div_t<Fast>(gl.z - l.z * gll, ln);
  gtheta[8] = 0.0f; gtheta[9] = 0.0f;                            // bias, hit_eps: constants (frozen), no gradient
}
"""

register_shader(MirrorShader, params=("reflectivity", "light_direction", "ambient", "sky", "bias", "hit_eps"), hip=_MIRROR_SHADER_HIP,
                trace=24)
