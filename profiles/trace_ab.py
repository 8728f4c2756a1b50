"""What a traced secondary ray costs on the GPU ("traced rays"):

    python profiles/trace_ab.py --build-only          # no GPU: hipcc the libraries the run below needs
    python profiles/trace_ab.py > profiles/trace_ab.txt
    python profiles/trace_ab.py --bench before.jsonl after.jsonl >> profiles/trace_ab.txt    # no GPU: the result lines of bench.py
                                                                   # runs of the commit before and of this one, in alternation

make_test_scene2() at pose (0, 0, -3), alternating in one process:
  0. as 1, but replays of captured frames (RenderLoop.capture): no Python and no launch path between the kernels, so what
     differs from 1 is the host's share of a 0.15 ms frame;
  1. the 1920x1080x128 frame under contrib.MirrorShader (24 secondary steps, a value and a normal at their end) against the same
     frame under contrib.DirectionalLightShader.  Counting scene evaluations alone the ratio would be (128 + 4 + 24 + 5) / (128 + 4);
  2. the same MirrorShader frame against the only way to get the picture without register_shader(trace=): the directional frame,
     then the stand-alone ops -- camera, SDFMarcher and SDFNormals for the hit point and its normal, SDFMarcher / SDFNormals / the
     scene on the reflected rays -- and MirrorShader's own PyTorch forward as the blend;
  3. the captured training step at 512x512x64 under either shader (forward, backward, Adam on every parameter).
Device events around windows of at least a second, after warm-up; medians over ROUNDS rounds; the spread between the rounds of
the first entry is the noise floor the gaps are read against."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_for, compiled_with_shader  # noqa: E402
from ray_marching_amd.contrib import DirectionalLightShader, MirrorShader  # noqa: E402
from ray_marching_amd.control import RenderLoop  # noqa: E402
from ray_marching_amd.scene.scene_registry import make_test_scene2  # noqa: E402

PX, EPS = 3.45e-6, 5e-2
LIGHT = [-0.35, -0.5, 0.8]
SHADERS = {"DirectionalLightShader": lambda: DirectionalLightShader([-x for x in LIGHT], [0.9, 0.55, 0.3], 0.15),
           "MirrorShader": lambda: MirrorShader(0.5, LIGHT, 0.15)}


def loop_for(scene, h, w, dev):
    return RenderLoop(scene, num_cameras=1, px_width=w, px_height=h, focal_length=PX * h, sensor_width=PX * w,
                      sensor_height=PX * h, normals_eps=EPS, regen=False).to(dev)


def time_ms(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / count


def ab(fns, rounds, what):
    names = list(fns)
    counts = {}
    for n, fn in fns.items():
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        counts[n] = max(50, math.ceil(1100.0 / time_ms(fn, 50)))          # a window of at least a second
    ms = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:                       # alternating
            ms[n].append(time_ms(fns[n], counts[n]))
    for n in names:
        v = ms[n]
        print(f"{what:24s} {n:36s} median {statistics.median(v):8.4f} ms  min {min(v):8.4f}  max {max(v):8.4f}  "
              f"({rounds} windows of {counts[n]}: {' '.join(f'{x:.4f}' for x in v)})", flush=True)
    base = ms[names[0]]
    print(f"{what:24s} window-to-window spread of {names[0]}: {max(base) - min(base):.4f} ms "
          f"({(max(base) - min(base)) / statistics.median(base):.2%} of its median)", flush=True)
    for n in names[1:]:
        print(f"{what:24s} {n} - {names[0]} = {statistics.median(ms[n]) - statistics.median(base):+.4f} ms "
              f"(ratio {statistics.median(ms[n]) / statistics.median(base):.4f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bench", nargs=2, metavar=("BEFORE", "AFTER"), help="two files of bench.py result lines: format them, no GPU")
    a = ap.parse_args()
    if a.bench:
        runs = [[json.loads(line) for line in open(f) if line.strip()] for f in a.bench]
        print("\n# bench.py --gpus 1 --steps 20 --warmup 3 on one box, the commit before and this commit in alternation")
        for k in range(max(map(len, runs))):
            for tag, rows in zip(("commit before", "this commit"), runs):
                if k < len(rows):
                    print(f"bench.py run {k + 1}  {tag:14s} value {rows[k]['value']:10.1f} {rows[k]['unit']}  ms_per_step {rows[k]['ms_per_step']:.4f}")
        p, n = ([d["value"] for d in rows] for rows in runs)
        print(f"# the commit before's own runs are {(max(p) - min(p)) / max(p):.1%} apart, this commit's {(max(n) - min(n)) / max(n):.1%}; "
              f"best of each: {max(p):.1f} and {max(n):.1f} ({max(n) / max(p) - 1:+.2%})")
        return
    if a.build_only:
        print("scene alone", specialize.build(compiled_for(make_test_scene2())))
        for name, shader in SHADERS.items():
            print(name, specialize.build(compiled_with_shader(make_test_scene2(), shader())))
        return
    dev = torch.device("cuda:0")
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev)
    t = torch.tensor([[0.0, 0.0, -3.0]], device=dev)

    def frame_fn(shader):
        scene, shader = make_test_scene2().to(dev), shader().to(dev)
        loop = loop_for(scene, 1080, 1920, dev)

        def fn():
            with torch.no_grad():
                loop(q, t, shader, 1, 128)
        return fn

    def captured_fn(shader):
        scene, shader = make_test_scene2().to(dev), shader().to(dev)
        frame = loop_for(scene, 1080, 1920, dev).capture(shader, 1, 128)
        return lambda: frame(q, t)

    def unfused_fn():
        scene, mirror, directional = make_test_scene2().to(dev), SHADERS["MirrorShader"]().to(dev), SHADERS["DirectionalLightShader"]().to(dev)
        loop = loop_for(scene, 1080, 1920, dev)

        def trace(origins, directions):
            points = loop.marcher(origins, directions, 24)
            return points, loop.normals(points)[0], scene(points)

        def fn():
            with torch.no_grad():
                loop(q, t, directional, 1, 128)
                pos, frames, _, dirs = loop.camera(q, t)
                p = loop.marcher(pos, dirs, 128)
                return mirror(pos, q, frames, dirs, p, loop.normals(p)[0], trace)
        return fn

    def train_fn(shader):
        scene, shader = make_test_scene2().to(dev), shader().to(dev)
        loop = loop_for(scene, 512, 512, dev)
        params = list(scene.parameters()) + [p for p in shader.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-5, capturable=True)
        step = loop.training_step(lambda image: image.pow(2).mean(), mode=shader, marching_steps=64, optimizer=opt)
        return lambda: step(q, t)

    print(f"# {torch.cuda.get_device_name(0)}; frame = RenderLoop.forward, tile kernel, pose (0,0,-3); training step = the captured graph "
          f"of RenderLoop.training_step (forward, backward, Adam on every trainable parameter)")
    print(f"# scene evaluations per pixel: directional 128 + 4 = 132, mirror 128 + 4 + 24 + 5 = 161: ratio {161 / 132:.4f}")
    with torch.no_grad():       # the two roads to the picture, once: what the unfused composition is compared with
        scene, mirror = make_test_scene2().to(dev), SHADERS["MirrorShader"]().to(dev)
        image = loop_for(scene, 1080, 1920, dev)(q, t, mirror, 1, 128)
        other = unfused_fn()().expand(1, 1080, 1920, 3)
        print(f"# fused frame against the unfused composition: max|difference| {float((image - other).abs().max()):.3g}, "
              f"{float(((image - other).abs() > 1e-5).float().mean()):.3g} of the values beyond 1e-5")
    ab({n: captured_fn(s) for n, s in SHADERS.items()}, a.rounds, "captured frame 1080p x128")
    ab({n: frame_fn(s) for n, s in SHADERS.items()}, a.rounds, "frame 1920x1080x128")
    ab({"MirrorShader (fused)": frame_fn(SHADERS["MirrorShader"]), "directional frame + stand-alone ops": unfused_fn()}, a.rounds,
       "frame 1920x1080x128")
    ab({n: train_fn(s) for n, s in SHADERS.items()}, a.rounds, "training step 512x512x64")


if __name__ == "__main__":
    main()
