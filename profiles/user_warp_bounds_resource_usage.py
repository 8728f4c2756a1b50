"""Compiler-reported resources of the kernels of contrib.make_warped_scene(bounded=True) next to its unbounded twin (no GPU
needed):

    python profiles/user_warp_bounds_resource_usage.py > profiles/user_warp_bounds_resource_usage.txt

  plain    make_warped_scene(): no operator signs a bound, no cull test in the program
  bounded  make_warped_scene(bounded=True): two cull tests, and user_warp_bound in the walk that derives their constants
Compiled exactly as ray_marching_amd/specialize.py does, plus -Rpass-analysis=kernel-resource-usage.  Exits non-zero when a
kernel of the bounded scene uses scratch memory that the same kernel of the twin does not."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compile_scene  # noqa: E402
from ray_marching_amd.contrib import make_warped_scene  # noqa: E402


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


tables = {"plain": resources(compile_scene(make_warped_scene())), "bounded": resources(compile_scene(make_warped_scene(bounded=True)))}
print(f"# flags {' '.join(specialize.variant('exact')[1])}")
print(f"# {'scene':8s} {'kernel':52s} VGPR AGPR SGPR  spillS spillV scratch[B/lane]  occ[waves/SIMD]")
for kernel in sorted(tables["plain"]):
    for which in ("plain", "bounded"):
        k = tables[which].get(kernel, {})
        print(f"{which:10s} {kernel[:52]:52s} {k.get('VGPRs', '?'):>4s} {k.get('AGPRs', '?'):>4s} {k.get('TotalSGPRs', '?'):>4s}  "
              f"{k.get('SGPRs Spill', '?'):>6s} {k.get('VGPRs Spill', '?'):>6s} {k.get('ScratchSize [bytes/lane]', '?'):>15s}  "
              f"{k.get('Occupancy [waves/SIMD]', '?'):>15s}")
extra = sorted(k for k, v in tables["bounded"].items() if int(v.get("ScratchSize [bytes/lane]", "0")) >
               int(tables["plain"].get(k, {}).get("ScratchSize [bytes/lane]", "0")))
print(f"# bounded: kernels with more scratch than the unbounded twin's: {extra or 'none'}")
sys.exit(1 if extra else 0)
