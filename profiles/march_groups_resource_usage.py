"""Compiler-reported resources of the kernels that march, for the three libraries the grouped march (march_groups,
rm_kernels.h) is judged on (no GPU needed):

    python profiles/march_groups_resource_usage.py [--asm DIR] [--only scene2,closed1] [--all] > table.txt

  scene2     make_test_scene2()                 the headline frame
  closed1    make_closed_test_scene()           the training scene
  many32     make_many_primitive_scene(32)      the long program (its evaluation is not copied per step of a group)
  generic    the interpreter's library          (only with --all or when named in --only)
  fast       the interpreter's library, precision="fast"     (likewise)
--all lists every kernel of every library, the backward kernels included, not only those that march.
Compiled exactly as ray_marching_amd/specialize.py does (RM_HIPCC_EXTRA included), plus -Rpass-analysis=kernel-resource-usage.
--asm DIR also leaves the device assembly of each library there (<name>.s) and prints, per kernel, its instruction
counts by class and its code size as the assembler's own symbol size comment gives it."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compile_scene  # noqa: E402
from ray_marching_amd.scene import scene_registry as R  # noqa: E402

KERNELS = ("k_render_fwd", "k_render_parked", "k_march_fwd", "k_march_regen")


def short_name(mangled):
    short = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    short = re.sub(r"\(.*", "", short.replace("void ", "").replace("rm::", ""))
    return re.sub(r"StaticCfg<RmStaticCode, (\d+), (false|true)>", r"S\1", short)


def resources(cs, asm=None, precision="exact"):
    """cs = None: the interpreter's library"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [specialize._hipcc(), *specialize.variant(precision)[1]]
        if cs is not None:
            header = os.path.join(tmp, "code.h")
            open(header, "w").write(specialize.code_header(cs))
            cmd.append(f'-DRM_STATIC_CODE="{header}"')
            if not specialize.static_backward(cs):
                cmd.append("-DRM_NO_BACKWARD")
        cmd.append(os.path.join(specialize.CSRC, "rm_abi.hip"))
        r = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "lib.so")],
                           capture_output=True, text=True, cwd=specialize.CSRC)
        if r.returncode:
            sys.exit(r.stderr[-3000:])
        if asm:
            flags = [f for f in cmd if f not in ("-shared", "-fPIC")]
            subprocess.run(flags + ["--cuda-device-only", "-S", "-o", asm], check=True, cwd=specialize.CSRC)
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(short_name(m.group(1)), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z ]+(?:\[.*?\])?): (\S+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return rows


def asm_counts(path):
    """kernel -> instruction counts by class, from the function bodies of the assembly"""
    out, cur, last = {}, None, None
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if m:
            cur = out.setdefault(short_name(m.group(1)), {"valu": 0, "salu": 0, "branch": 0, "readlane": 0, "vmov": 0, "bytes": 0})
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"\s+([sv]_\w+|ds_\w+|global_\w+|buffer_\w+|scratch_\w+|flat_\w+)\b", line)
        if cur is None or not m:
            m2 = re.match(r"; codeLenInByte = (\d+)", line)
            if m2 and last is not None:
                last["bytes"] = int(m2.group(1))
            continue
        last = cur
        op = m.group(1)
        if op.startswith(("s_branch", "s_cbranch")):
            cur["branch"] += 1
        elif op.startswith("s_"):
            cur["salu"] += 1
        elif op.startswith("v_"):
            cur["valu"] += 1
            cur["readlane"] += op.startswith("v_readlane")
            cur["vmov"] += op.startswith("v_mov")
    return out


if __name__ == "__main__":
    asm_dir = sys.argv[sys.argv.index("--asm") + 1] if "--asm" in sys.argv else None
    if asm_dir:
        os.makedirs(asm_dir, exist_ok=True)
    every = "--all" in sys.argv
    libs = {"scene2": R.make_test_scene2(), "closed1": R.make_closed_test_scene(), "many32": R.make_many_primitive_scene(32),
            "generic": None, "fast": None}
    if "--only" in sys.argv:
        libs = {k: m for k, m in libs.items() if k in sys.argv[sys.argv.index("--only") + 1].split(",")}
    elif not every:
        libs = {k: m for k, m in libs.items() if m is not None}
    compiled = {k: compile_scene(m) if m is not None else None for k, m in libs.items()}
    with ThreadPoolExecutor(max_workers=3) as ex:
        tables = dict(zip(libs, ex.map(lambda k: resources(compiled[k], asm_dir and os.path.join(asm_dir, k + ".s"),
                                                           "fast" if k == "fast" else "exact"), libs)))
    print(f"# flags {' '.join(specialize.variant('exact')[1])}")
    print(f"# {'library':8s} {'instr':>5s} {'kernel':34s} VGPR AGPR SGPR  spillS spillV scratch[B/lane]  occ[waves/SIMD]")
    for which in libs:
        for kernel in sorted(k for k in tables[which] if every or k.startswith(KERNELS)):
            k = tables[which][kernel]
            print(f"{which:10s} {compiled[which].n_instr if compiled[which] else 0:5d} {kernel[:34]:34s} {k.get('VGPRs', '?'):>4s} {k.get('AGPRs', '?'):>4s} "
                  f"{k.get('TotalSGPRs', '?'):>4s}  {k.get('SGPRs Spill', '?'):>6s} {k.get('VGPRs Spill', '?'):>6s} "
                  f"{k.get('ScratchSize [bytes/lane]', '?'):>15s}  {k.get('Occupancy [waves/SIMD]', '?'):>15s}")
    if asm_dir:
        print(f"# {'library':8s} {'kernel':34s}  VALU  SALU branch v_readlane v_mov  code[bytes]")
        for which in libs:
            counts = asm_counts(os.path.join(asm_dir, which + ".s"))
            for kernel in sorted(k for k in counts if every or k.startswith(KERNELS)):
                c = counts[kernel]
                print(f"{which:10s} {kernel[:34]:34s} {c['valu']:5d} {c['salu']:5d} {c['branch']:6d} {c['readlane']:10d} {c['vmov']:5d}  "
                      f"{c['bytes']:11d}")
