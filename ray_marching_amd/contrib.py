"""Leaves beyond the reference's six primitives, added through the public extension point (extensions.register_leaf)
exactly as a user would add their own: a PyTorch ``forward`` (the CPU path and the oracle) and the same op stream in HIP."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch import Tensor

from .extensions import register_leaf


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
