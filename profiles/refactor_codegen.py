"""Device code of two source trees, kernel by kernel (no GPU needed): the check of a refactor that must not move codegen.

    python profiles/refactor_codegen.py emit --csrc PARENT/ray_marching_amd/csrc --out /tmp/cg/parent
    python profiles/refactor_codegen.py emit --out /tmp/cg/branch
    python profiles/refactor_codegen.py compare /tmp/cg/parent /tmp/cg/branch > profiles/refactor_codegen.txt

`emit` compiles rm_abi.hip of one tree (default: this one) to device assembly with the project's own flags (_build.HIPCC_FLAGS /
HIPCC_FLAGS_FAST with `--cuda-device-only -S` in place of `-shared`, plus -Rpass-analysis=kernel-resource-usage) for: the generic
library, exact and fast; every scene of specialize.default_scenes(), specialised (specialize.code_header; -DRM_NO_BACKWARD where
specialize.static_backward says so); make_test_scene2() with DirectionalLightShader (no probes) and with AmbientOcclusionShader
(probes).  `compare` prints, for every kernel of every build, parent -> branch of the metadata's .vgpr_count, .sgpr_count,
.private_segment_fixed_size, .group_segment_fixed_size, the reported occupancy and the instruction count (comments and directives
stripped, labels kept), or "identical" where the instruction streams are the same text, and exits non-zero when a resource
number or the occupancy moved, a kernel appeared or vanished, or a differing stream's count is more than 1 % off the parent's."""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def builds():
    """name -> (precision, CompiledScene or None)"""
    from ray_marching_amd import specialize
    from ray_marching_amd.compiler import compile_scene, compiled_with_shader
    from ray_marching_amd.contrib import AmbientOcclusionShader, DirectionalLightShader
    from ray_marching_amd.scene.scene_registry import make_test_scene2
    out = {"generic_exact": ("exact", None), "generic_fast": ("fast", None)}
    for name, scene in specialize.default_scenes().items():
        out["spec_" + name] = ("exact", compile_scene(scene))
    out["shader_directional"] = ("exact", compiled_with_shader(
        make_test_scene2(), DirectionalLightShader([0.35, 0.5, -0.8], [0.9, 0.55, 0.3], 0.15)))
    out["shader_ambient_occlusion"] = ("exact", compiled_with_shader(
        make_test_scene2(), AmbientOcclusionShader(0.4, 2.0, [0.9, 0.6, 0.4])))
    return out


def emit(csrc, out, only):
    from ray_marching_amd import specialize
    os.makedirs(out, exist_ok=True)

    def one(item):
        name, (precision, cs) = item
        flags = [f for f in specialize.variant(precision)[1] if f != "-shared"] + ["--cuda-device-only", "-S"]
        if cs is not None:
            header = os.path.join(out, name + ".code.h")
            with open(header, "w") as f:
                f.write(specialize.code_header(cs))
            flags.append(f'-DRM_STATIC_CODE="{header}"')
            if not specialize.static_backward(cs):
                flags.append("-DRM_NO_BACKWARD")
        cmd = [specialize._hipcc(), *flags, "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "rm_abi.hip"),
               "-o", os.path.join(out, name + ".s")]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=csrc)
        if r.returncode:
            sys.exit(f"{name}: hipcc failed\n{r.stderr[-3000:]}")
        with open(os.path.join(out, name + ".remarks"), "w") as f:
            f.write(r.stderr)
        return name

    todo = [(n, b) for n, b in builds().items() if not only or n in only]
    with ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", "8"))) as ex:
        for name in ex.map(one, todo):
            print("emitted", name, file=sys.stderr, flush=True)


def kernels_of(directory, name):
    """kernel -> {field: number, 'occupancy': n, 'stream': [lines]} of one build"""
    text = open(os.path.join(directory, name + ".s")).read()
    out = {}
    meta = text[text.index("amdhsa.kernels:"):].split("\namdhsa.")[0]
    for entry in re.split(r"\n  - ", meta)[1:]:
        kernel = re.search(r"\.name:\s+(\S+)", entry).group(1)
        out[kernel] = {f: int(re.search(re.escape(f) + r":\s+(\d+)", entry).group(1)) for f in FIELDS}
    lines = [line.split(";")[0].strip() for line in text.splitlines()]
    for kernel, k in out.items():
        start = lines.index(kernel + ":")
        stream = []
        for line in lines[start:]:
            if re.match(r"\.Lfunc_end\d+:", line):
                break
            if line and (not line.startswith(".") or line.endswith(":")):
                stream.append(line)
        k["stream"] = stream
    cur = None
    for line in open(os.path.join(directory, name + ".remarks")):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and cur in out:
            out[cur]["occupancy"] = int(m.group(1))
    return out


def short(kernel):
    name = subprocess.run(["c++filt", kernel], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"\(.*", "", name.replace("void ", "").replace("rm::", ""))
    return re.sub(r"StaticCfg<RmStaticCode, (\d+), (false|true)>", r"S\1", name)


def compare(parent, branch):
    names = sorted(f[:-2] for f in os.listdir(parent) if f.endswith(".s"))
    bad, differing, total = [], 0, 0
    print("# build / kernel: VGPR SGPR scratch[B] LDS[B] occupancy[waves/SIMD] instructions; parent -> branch where a number moved")
    for name in names:
        a, b = kernels_of(parent, name), kernels_of(branch, name)
        for kernel in sorted(set(a) ^ set(b)):
            bad.append(f"{name} {short(kernel)}: only in {'parent' if kernel in a else 'branch'}")
        for kernel in sorted(set(a) & set(b), key=short):
            ka, kb = a[kernel], b[kernel]
            total += 1
            cells = []
            for f in FIELDS + ("occupancy",):
                cells.append(str(ka[f]) if ka[f] == kb[f] else f"{ka[f]}->{kb[f]}")
                if ka[f] != kb[f]:
                    bad.append(f"{name} {short(kernel)}: {f} {ka[f]} -> {kb[f]}")
            na, nb = len(ka["stream"]), len(kb["stream"])
            if ka["stream"] == kb["stream"]:
                cells.append(f"{na} identical")
            else:
                differing += 1
                cells.append(f"{na}->{nb} ({100.0 * (nb - na) / na:+.3f} %)")
                if abs(nb - na) > 0.01 * na:
                    bad.append(f"{name} {short(kernel)}: {na} -> {nb} instructions")
            print(f"{name:28s} {short(kernel)[:44]:44s} " + " ".join(f"{c:>9s}" for c in cells[:5]) + "  " + cells[5])
    print(f"# {total} kernels in {len(names)} builds, {total - differing} with an identical instruction stream, {differing} that differ")
    print(f"# conditions broken: {bad or 'none'}")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("emit")
    e.add_argument("--csrc", default=os.path.join(ROOT, "ray_marching_amd", "csrc"))
    e.add_argument("--out", required=True)
    e.add_argument("--only", nargs="*")
    c = sub.add_parser("compare")
    c.add_argument("parent")
    c.add_argument("branch")
    args = ap.parse_args()
    if args.cmd == "emit":
        emit(os.path.abspath(args.csrc), os.path.abspath(args.out), args.only)
    else:
        sys.exit(compare(args.parent, args.branch))
