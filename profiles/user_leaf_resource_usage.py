"""Compiler-reported resources of the kernels of a scene with a user-defined leaf next to its built-in twin (no GPU needed):

    python profiles/user_leaf_resource_usage.py > profiles/user_leaf_resource_usage.txt

Three scenes of one shape -- the room, a sphere moved by an affine node, and an affine-placed X:
  link     X = contrib.SDFLink (a user leaf), the scene of contrib.make_link_scene()
  twin     X = SDFTorus (built-in)
  usphere  the twin with its SDFSphere restated as a user leaf (the glue alone: the same arithmetic as the built-in)
Compiled exactly as ray_marching_amd/specialize.py does, plus -Rpass-analysis=kernel-resource-usage.  Exits non-zero when a
kernel of a user-leaf scene uses scratch memory that the same kernel of the twin does not."""
import os
import re
import subprocess
import sys
import tempfile

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compile_scene  # noqa: E402
from ray_marching_amd.contrib import SDFLink, make_link_scene  # noqa: E402
from ray_marching_amd.extensions import register_leaf  # noqa: E402
from ray_marching_amd.scene.primitives import SDFSphere, SDFTorus  # noqa: E402


class USphere(nn.Module):
    def __init__(self, radius):
        super().__init__()
        self.radius = nn.Parameter(torch.tensor(radius))

    def forward(self, p):
        return torch.linalg.vector_norm(p, dim=-1, keepdim=True) - self.radius


register_leaf(USphere, params=("radius",), cost=13, hip="""
template <bool Fast> RM_DEV float usphere_fwd(rm::V3 p, const float* theta) { return norm3_t<Fast>(p) - theta[0]; }
template <bool Fast> RM_DEV void usphere_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) {
  const float n = norm3_t<Fast>(p);
  const float s = (n == 0.0f) ? 0.0f : div_t<Fast>(g, n);
  gp = gp + mk3(p.x * s, p.y * s, p.z * s);
  gtheta[0] = -g;
}
""")


def scene(which):
    s = make_link_scene()
    if which != "link":
        s.sdfs[1].sdfs[1].sdf = SDFTorus(0.3, 0.08)
    if which == "usphere":
        s.sdfs[1].sdfs[0].sdf = USphere(0.5)
    else:
        assert isinstance(s.sdfs[1].sdfs[0].sdf, SDFSphere)
    return s


def resources(cs):
    with tempfile.TemporaryDirectory() as tmp:
        header = os.path.join(tmp, "code.h")
        open(header, "w").write(specialize.code_header(cs))
        cmd = [specialize._hipcc(), *specialize.variant("exact")[1], f'-DRM_STATIC_CODE="{header}"',
               "-Rpass-analysis=kernel-resource-usage", os.path.join(specialize.CSRC, "rm_abi.hip"), "-o", os.path.join(tmp, "lib.so")]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=specialize.CSRC)
        if r.returncode:
            sys.exit(r.stderr[-3000:])
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            short = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            short = re.sub(r"\(.*", "", short.replace("void ", "").replace("rm::", ""))
            short = re.sub(r"StaticCfg<RmStaticCode, (\d+), (false|true)>", r"S\1", short)
            cur = rows.setdefault(short, {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z ]+(?:\[.*?\])?): (\S+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return rows


WANTED = ("k_render_fwd", "k_render_bwd", "k_march_bwd", "k_march_regen", "k_sdf_fwd", "k_sdf_bwd")
tables = {w: resources(compile_scene(scene(w))) for w in ("twin", "usphere", "link")}
print(f"# flags {' '.join(specialize.variant('exact')[1])}")
print(f"# {'scene':8s} {'kernel':52s} VGPR AGPR SGPR  spillS spillV scratch[B/lane]  occ[waves/SIMD]")
bad = []
for kernel in sorted(tables["twin"]):
    if not kernel.startswith(WANTED):
        continue
    for which in ("twin", "usphere", "link"):
        k = tables[which].get(kernel, {})
        print(f"{which:10s} {kernel[:52]:52s} {k.get('VGPRs', '?'):>4s} {k.get('AGPRs', '?'):>4s} {k.get('TotalSGPRs', '?'):>4s}  "
              f"{k.get('SGPRs Spill', '?'):>6s} {k.get('VGPRs Spill', '?'):>6s} {k.get('ScratchSize [bytes/lane]', '?'):>15s}  "
              f"{k.get('Occupancy [waves/SIMD]', '?'):>15s}")
        if which != "twin" and int(k.get("ScratchSize [bytes/lane]", "0")) > int(tables["twin"][kernel].get("ScratchSize [bytes/lane]", "0")):
            bad.append((which, kernel))
for which in ("usphere", "link"):
    extra = sorted(k for k, v in tables[which].items() if int(v.get("ScratchSize [bytes/lane]", "0")) >
                   int(tables["twin"].get(k, {}).get("ScratchSize [bytes/lane]", "0")))
    print(f"# {which}: kernels with more scratch than the twin's: {extra or 'none'}")
    bad += [(which, k) for k in extra]
sys.exit(1 if bad else 0)
