"""Compiler-reported resources of the frame kernels of a (scene, shader) library next to the scene's own (no GPU needed):

    python profiles/user_shader_resource_usage.py > profiles/user_shader_resource_usage.txt

  scene        make_test_scene2() alone: k_render_fwd and k_render_bwd<.., 0> (built-in mode 0 runs through these)
  ulambert     the same scene with the restated-Lambertian twin (profiles/user_shader_ab.py): no parameters
  directional  ... with contrib.DirectionalLightShader: seven parameter floats (theta / gtheta must dissolve into registers)
  depth_cue    ... with contrib.DepthCueShader: four
Compiled exactly as ray_marching_amd/specialize.py does, plus -Rpass-analysis=kernel-resource-usage.  Exits non-zero when
k_render_fwd or k_render_bwd<.., 4> of a shader library uses more scratch memory than k_render_fwd / k_render_bwd<.., 0> of
the scene alone."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from user_shader_ab import MODES  # noqa: E402
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_for, compiled_with_shader  # noqa: E402
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


NAMES = {"scene": "scene2 built-in mode 0", "ulambert": "scene2 ULambert twin", "directional": "scene2 DirectionalLightShader",
         "depth_cue": "scene2 DepthCueShader"}
tables = {}
for which, name in NAMES.items():
    scene, mode = make_test_scene2(), MODES[name]()
    tables[which] = resources(compiled_for(scene) if isinstance(mode, int) else compiled_with_shader(scene, mode))
print(f"# flags {' '.join(specialize.variant('exact')[1])}")
print(f"# {'library':10s} {'kernel':52s} VGPR AGPR SGPR  spillS spillV scratch[B/lane]  occ[waves/SIMD]")


def scratch(which, kernel):
    return int(tables[which].get(kernel, {}).get("ScratchSize [bytes/lane]", "0"))


kernels = sorted({k for t in tables.values() for k in t if k.startswith(("k_render_fwd", "k_render_finish", "k_render_bwd"))})
bwd0 = next(k for k in kernels if re.match(r"k_render_bwd<S\d+, 0>", k))
bwd4 = bwd0.replace(", 0>", ", 4>")
extra = []
for kernel in kernels:
    for which in NAMES:
        k = tables[which].get(kernel)
        if k is None:
            continue
        print(f"{which:12s} {kernel[:52]:52s} {k.get('VGPRs', '?'):>4s} {k.get('AGPRs', '?'):>4s} {k.get('TotalSGPRs', '?'):>4s}  "
              f"{k.get('SGPRs Spill', '?'):>6s} {k.get('VGPRs Spill', '?'):>6s} {k.get('ScratchSize [bytes/lane]', '?'):>15s}  "
              f"{k.get('Occupancy [waves/SIMD]', '?'):>15s}")
        reference = bwd0 if kernel == bwd4 else kernel
        if which != "scene" and (kernel == bwd4 or kernel.startswith(("k_render_fwd", "k_render_finish"))) \
                and scratch(which, kernel) > scratch("scene", reference):
            extra.append((which, kernel))
print(f"# shader libraries: frame kernels with more scratch than the scene's own (k_render_bwd<.., 4> against kind 0): {extra or 'none'}")
sys.exit(1 if extra else 0)
