"""Compiler-reported resources of the frame kernels of a (scene, ray-tracing shader) library next to those of a probe-free shader
and of the chained-probe shader (no GPU needed):

    python profiles/user_shader_trace_resource_usage.py > profiles/user_shader_trace_resource_usage.txt

  directional          make_test_scene2() with contrib.DirectionalLightShader: no probes (seven parameter floats)
  marched_shadow       ... with contrib.MarchedShadowShader: K = 8 chained probes, the whole chain in registers
  mirror               ... with contrib.MirrorShader: register_shader(trace=24), the secondary march checkpointed in global memory
Compiled exactly as ray_marching_amd/specialize.py does, plus -Rpass-analysis=kernel-resource-usage.  Exits non-zero when a frame
kernel of the mirror library uses more scratch memory or spills more VGPRs than the same kernel of the probe-free library."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_with_shader  # noqa: E402
from ray_marching_amd.contrib import DirectionalLightShader, MarchedShadowShader, MirrorShader  # noqa: E402
from ray_marching_amd.scene.scene_registry import make_test_scene2  # noqa: E402


def resources(cs, extra=()):
    with tempfile.TemporaryDirectory() as tmp:
        header = os.path.join(tmp, "code.h")
        open(header, "w").write(specialize.code_header(cs))
        cmd = [specialize._hipcc(), *specialize.variant("exact")[1], *extra, f'-DRM_STATIC_CODE="{header}"',
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


LIGHT = [0.35, 0.5, -0.8]
LIBS = {"directional": (lambda: DirectionalLightShader(LIGHT, [0.9, 0.55, 0.3], 0.15), ()),
        "marched_shadow": (lambda: MarchedShadowShader(LIGHT), ()),
        "mirror": (lambda: MirrorShader(0.5, LIGHT), ())}
with ThreadPoolExecutor(max_workers=4) as ex:
    tables = dict(zip(LIBS, ex.map(lambda job: resources(compiled_with_shader(make_test_scene2(), job[0]()), job[1]), LIBS.values())))
print(f"# flags {' '.join(specialize.variant('exact')[1])}")
print(f"# {'library':20s} {'kernel':30s} VGPR AGPR SGPR  spillS spillV scratch[B/lane]  occ[waves/SIMD]")
kernels = sorted({k for t in tables.values() for k in t if k.startswith(("k_render_fwd", "k_render_finish", "k_render_bwd", "k_render_hard",
                                                                         "k_render_parked", "k_bwd_hard"))})
extra = []
for kernel in kernels:
    for which in LIBS:
        k = tables[which].get(kernel)
        if k is None:
            continue
        print(f"{which:22s} {kernel[:30]:30s} {k.get('VGPRs', '?'):>4s} {k.get('AGPRs', '?'):>4s} {k.get('TotalSGPRs', '?'):>4s}  "
              f"{k.get('SGPRs Spill', '?'):>6s} {k.get('VGPRs Spill', '?'):>6s} {k.get('ScratchSize [bytes/lane]', '?'):>15s}  "
              f"{k.get('Occupancy [waves/SIMD]', '?'):>15s}")
        twin = tables["directional"].get(kernel, {})
        if which == "mirror" and (int(k.get("ScratchSize [bytes/lane]", "0")) > int(twin.get("ScratchSize [bytes/lane]", "0"))
                                  or int(k.get("VGPRs Spill", "0")) > int(twin.get("VGPRs Spill", "0"))):
            extra.append((which, kernel))
print(f"# mirror library: frame kernels with more scratch or more spilled VGPRs than the probe-free library's: {extra or 'none'}")
sys.exit(1 if extra else 0)
