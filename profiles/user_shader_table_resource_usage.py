"""Compiler-reported resources of the libraries of user shaders that read a lookup table (register_shader(table=..., table_taps=T))
next to those of a table-less shader's (no GPU needed):

    python profiles/user_shader_table_resource_usage.py > profiles/user_shader_table_resource_usage.txt
    python profiles/user_shader_table_resource_usage.py depth_cue        # one library only (runs on older trees too)

  depth_cue            make_test_scene2() with contrib.DepthCueShader: no table.  Its rows are the evidence that libraries without a
                       table are what they were: profiles/user_shader_table_parent_depth_cue.txt holds the same rows from the commit
                       before lookup tables, and tests/test_user_shader_table.py compares the two.  (Both files are
                       re-recorded whenever the frame kernels themselves change, as with the march in groups: the
                       depth_cue rows are then this tree's, and the comparison holds the two files to each other.)
  depth_palette        ... with contrib.DepthPaletteShader: T = 2, the fused backward stores two records per pixel
  tangent_palette      ... with contrib.TangentPaletteShader: T = 1
and k_table_scatter, which every library carries.  Compiled exactly as ray_marching_amd/specialize.py does, plus
-Rpass-analysis=kernel-resource-usage.  Exits non-zero when a kernel of a table library, or k_table_scatter, uses scratch memory."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ray_marching_amd import contrib, specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_with_shader  # noqa: E402
from ray_marching_amd.scene.scene_registry import make_test_scene2  # noqa: E402

KERNELS = ("k_render_fwd", "k_render_finish", "k_render_bwd", "k_render_parked", "k_march_regen", "k_bwd_hard", "k_table_scatter")
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


def palette(n):
    x = torch.linspace(0.0, 1.0, n)[:, None]
    return 0.5 + 0.4 * torch.cos(2.0 * x + torch.tensor([0.0, 2.0, 4.0]))


LIBS = {"depth_cue": lambda: contrib.DepthCueShader(0.25, (0.5, 0.6, 0.7)),
        "depth_palette": lambda: contrib.DepthPaletteShader(0.25, palette(16)),
        "tangent_palette": lambda: contrib.TangentPaletteShader(palette(64))}


def table(names):
    """The lines of the table for these libraries (what this script prints), and the kernels that use scratch where none may."""
    with ThreadPoolExecutor(max_workers=3) as ex:
        tables = dict(zip(names, ex.map(lambda n: resources(compiled_with_shader(make_test_scene2(), LIBS[n]())), names)))
    lines, bad = [], []
    kernels = sorted({k for t in tables.values() for k in t if k.startswith(KERNELS)})
    for kernel in kernels:
        for which in names:
            k = tables[which].get(kernel)
            if k is None:
                continue
            lines.append(f"{which:16s} {kernel[:44]:44s} " + " ".join(f"{k.get(f, '?'):>6s}" for f in FIELDS))
            if (which != "depth_cue" or kernel.startswith("k_table_scatter")) and int(k.get("ScratchSize [bytes/lane]", "0")) > 0:
                bad.append(f"{which}:{kernel}")
    return lines, bad


if __name__ == "__main__":
    names = sys.argv[1:] or list(LIBS)
    lines, bad = table(names)
    print(f"# flags {' '.join(specialize.variant('exact')[1])}")
    print(f"# {'library':14s} {'kernel':44s}   VGPR   AGPR   SGPR spillS spillV scratch    occ    LDS")
    print("\n".join(lines))
    print(f"# kernels of the table libraries (and k_table_scatter) with scratch: {bad or 'none'}")
    sys.exit(1 if bad else 0)
