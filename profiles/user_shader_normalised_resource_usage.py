"""Compiler-reported resources of the library of a user shader normalised by the frame's min / max (register_shader(normalise="minmax"))
next to those of a per-pixel shader's (no GPU needed):

    python profiles/user_shader_normalised_resource_usage.py > profiles/user_shader_normalised_resource_usage.txt

  directional          make_test_scene2() with contrib.DirectionalLightShader: per pixel, no second pass (seven parameter floats)
  depth_ramp           ... with contrib.DepthRampShader: the second pass k_user_shade_finish and its VJP k_user_norm_bwd_a / _b
                       (eight parameter floats: theta, gtheta and the row of 4 + 8 partial sums must all be registers)
Compiled exactly as ray_marching_amd/specialize.py does, plus -Rpass-analysis=kernel-resource-usage.  Exits non-zero when one of the
three new kernels uses scratch memory, or when a frame kernel of the depth-ramp library uses more than the same kernel of the
per-pixel library."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_with_shader  # noqa: E402
from ray_marching_amd.contrib import DepthRampShader, DirectionalLightShader  # noqa: E402
from ray_marching_amd.scene.scene_registry import make_test_scene2  # noqa: E402


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


LIBS = {"directional": lambda: DirectionalLightShader([0.35, 0.5, -0.8], [0.9, 0.55, 0.3], 0.15),
        "depth_ramp": lambda: DepthRampShader([1.0, 0.9, 0.7], [0.05, 0.1, 0.3])}
NEW = ("k_user_shade_finish", "k_user_norm_bwd_a", "k_user_norm_bwd_b")
with ThreadPoolExecutor(max_workers=2) as ex:
    tables = dict(zip(LIBS, ex.map(lambda make: resources(compiled_with_shader(make_test_scene2(), make())), LIBS.values())))
print(f"# flags {' '.join(specialize.variant('exact')[1])}")
print(f"# {'library':20s} {'kernel':30s} VGPR AGPR SGPR  spillS spillV scratch[B/lane]  occ[waves/SIMD]")
kernels = sorted({k for t in tables.values() for k in t if k.startswith(("k_render_fwd", "k_render_finish", "k_render_bwd", "k_render_parked",
                                                                         "k_bwd_hard", "k_shade_finish", "k_shade_norm_bwd") + NEW)})
bad = []
for kernel in kernels:
    for which in LIBS:
        k = tables[which].get(kernel)
        if k is None:
            continue
        print(f"{which:22s} {kernel[:30]:30s} {k.get('VGPRs', '?'):>4s} {k.get('AGPRs', '?'):>4s} {k.get('TotalSGPRs', '?'):>4s}  "
              f"{k.get('SGPRs Spill', '?'):>6s} {k.get('VGPRs Spill', '?'):>6s} {k.get('ScratchSize [bytes/lane]', '?'):>15s}  "
              f"{k.get('Occupancy [waves/SIMD]', '?'):>15s}")
        scratch = int(k.get("ScratchSize [bytes/lane]", "0"))
        twin = int(tables["directional"].get(kernel, {}).get("ScratchSize [bytes/lane]", "0"))
        if which == "depth_ramp" and scratch > (0 if kernel.startswith(NEW) else twin):
            bad.append(kernel)
missing = [k for k in NEW if k not in tables["depth_ramp"]] + [k for k in NEW if k in tables["directional"]]
print(f"# depth-ramp library: second-pass kernels with scratch, frame kernels with more scratch than the per-pixel library's: {bad or 'none'}")
sys.exit(1 if bad or missing else 0)
