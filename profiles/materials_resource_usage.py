"""Compiler-reported resources of the libraries of scenes with material nodes (contrib.SDFMaterial) shaded by a shader that
reads the surface colour (register_shader(material=True)), next to those of a library that has neither (no GPU needed):

    python profiles/materials_resource_usage.py > profiles/materials_resource_usage.txt
    python profiles/materials_resource_usage.py depth_cue        # one library only (runs on older trees too)

  depth_cue            make_test_scene2() with contrib.DepthCueShader: no material node, no material shader.  Its rows are the
                       evidence that libraries without materials are what they were: profiles/materials_parent_depth_cue.txt holds
                       the same rows from the parent commit, and tests/test_materials.py compares the two.
  painted_lambert      contrib.make_painted_scene() with contrib.MaterialLambertShader: four materials under a smooth union
  carved_lambert       contrib.make_carved_scene() with a material on the body and one on the cutter of its subtraction (two more
                       implicit), same shader: user combinators in the sweep
and k_material_fwd / k_material_bwd, which the two material libraries carry.  Compiled exactly as ray_marching_amd/specialize.py
does, plus -Rpass-analysis=kernel-resource-usage.  Exits non-zero when a kernel of a material library uses scratch memory."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_marching_amd import contrib, specialize  # noqa: E402
from ray_marching_amd.compiler import compile_scene  # noqa: E402
from ray_marching_amd.scene.scene_registry import make_test_scene2  # noqa: E402

KERNELS = ("k_render_fwd", "k_render_finish", "k_render_bwd", "k_render_parked", "k_march_regen", "k_bwd_hard", "k_material")
FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
          "LDS Size [bytes/block]")


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


def carved_with_materials():
    scene = contrib.make_carved_scene()
    sub = scene.sdfs[1]
    sub.sdfs[0] = contrib.SDFMaterial(sub.sdfs[0], albedo=(0.8, 0.5, 0.2))
    sub.sdfs[1] = contrib.SDFMaterial(sub.sdfs[1], albedo=(0.1, 0.6, 0.9))
    return scene


LIBS = {"depth_cue": lambda: compile_scene(make_test_scene2(), contrib.DepthCueShader(0.25, (0.5, 0.6, 0.7))),
        "painted_lambert": lambda: compile_scene(contrib.make_painted_scene(), contrib.MaterialLambertShader()),
        "carved_lambert": lambda: compile_scene(carved_with_materials(), contrib.MaterialLambertShader())}


def table(names):
    """The lines of the table for these libraries (what this script prints), and the kernels that use scratch where none may."""
    with ThreadPoolExecutor(max_workers=3) as ex:
        tables = dict(zip(names, ex.map(lambda n: resources(LIBS[n]()), names)))
    lines, bad = [], []
    kernels = sorted({k for t in tables.values() for k in t if k.startswith(KERNELS)})
    for kernel in kernels:
        for which in names:
            k = tables[which].get(kernel)
            if k is None:
                continue
            lines.append(f"{which:16s} {kernel[:44]:44s} " + " ".join(f"{k.get(f, '?'):>6s}" for f in FIELDS))
            if which != "depth_cue" and int(k.get("ScratchSize [bytes/lane]", "0")) > 0:
                bad.append(f"{which}:{kernel}")
    return lines, bad


if __name__ == "__main__":
    names = sys.argv[1:] or list(LIBS)
    lines, bad = table(names)
    print(f"# flags {' '.join(specialize.variant('exact')[1])}")
    print(f"# {'library':14s} {'kernel':44s}   VGPR   AGPR   SGPR spillS spillV scratch    occ    LDS")
    print("\n".join(lines))
    print(f"# kernels of the material libraries with scratch: {bad or 'none'}")
    sys.exit(1 if bad else 0)
