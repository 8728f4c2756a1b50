"""Compiler-reported resources of the kernels of a scene built with a user-defined warp next to its built-in twin (no GPU
needed):

    python profiles/user_warp_resource_usage.py > profiles/user_warp_resource_usage.txt

  twin     scene 2 with its sphere and torus placed by affine nodes, compiled without cull tests (RM_CULL=0)
  uaffine  the same scene with both SDFAffineTransformations restated as a user warp (profiles/user_warp_ab.py: UAffine),
           which gets no cull tests either: the glue alone
Compiled exactly as ray_marching_amd/specialize.py does, plus -Rpass-analysis=kernel-resource-usage.  Exits non-zero when a
kernel of the warp scene uses scratch memory that the same kernel of the twin does not."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from user_warp_ab import SCENES  # noqa: E402
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_for  # noqa: E402


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
tables = {"twin": resources(compiled_for(SCENES["placed scene2 built-in, RM_CULL=0"]())),
          "uaffine": resources(compiled_for(SCENES["placed scene2 UAffine twin"]()))}
print(f"# flags {' '.join(specialize.variant('exact')[1])}")
print(f"# {'scene':8s} {'kernel':52s} VGPR AGPR SGPR  spillS spillV scratch[B/lane]  occ[waves/SIMD]")
bad = []
for kernel in sorted(tables["twin"]):
    if not kernel.startswith(WANTED):
        continue
    for which in ("twin", "uaffine"):
        k = tables[which].get(kernel, {})
        print(f"{which:10s} {kernel[:52]:52s} {k.get('VGPRs', '?'):>4s} {k.get('AGPRs', '?'):>4s} {k.get('TotalSGPRs', '?'):>4s}  "
              f"{k.get('SGPRs Spill', '?'):>6s} {k.get('VGPRs Spill', '?'):>6s} {k.get('ScratchSize [bytes/lane]', '?'):>15s}  "
              f"{k.get('Occupancy [waves/SIMD]', '?'):>15s}")
extra = sorted(k for k, v in tables["uaffine"].items() if int(v.get("ScratchSize [bytes/lane]", "0")) >
               int(tables["twin"].get(k, {}).get("ScratchSize [bytes/lane]", "0")))
print(f"# uaffine: kernels with more scratch than the twin's: {extra or 'none'}")
sys.exit(1 if extra else 0)
