"""What per-object colours cost on the GPU ("material nodes"):

    python profiles/materials_ab.py --build-only          # no GPU: hipcc the libraries the run below needs
    python profiles/materials_ab.py > profiles/materials_ab.txt

contrib.make_painted_scene() shaded by contrib.MaterialLambertShader -- one recording evaluation and one material sweep per pixel
on top of the march and the four taps -- against the same scene with its material nodes stripped, shaded by
contrib.DirectionalLightShader (one albedo for the whole scene): frame time at 1920x1080x128 and the captured training step at
512x512x64, alternating in one process.  Device events around windows of at least a second, after warm-up; medians over ROUNDS
rounds; the spread between the rounds of the stripped scene is the noise floor the gap is read against."""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_with_shader  # noqa: E402
from ray_marching_amd.contrib import DirectionalLightShader, MaterialLambertShader, make_painted_scene, strip_materials  # noqa: E402
from ray_marching_amd.control import RenderLoop  # noqa: E402

PX, EPS = 3.45e-6, 5e-2
PAIRS = {"stripped + DirectionalLightShader": (lambda: strip_materials(make_painted_scene()),
                                               lambda: DirectionalLightShader([0.0, 0.0, 1.0], [0.9, 0.55, 0.3], 0.15)),
         "painted + MaterialLambertShader": (make_painted_scene, lambda: MaterialLambertShader(0.15))}


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
    a = ap.parse_args()
    if a.build_only:
        for name, (scene, shader) in PAIRS.items():
            cs = compiled_with_shader(scene(), shader())
            print(name, cs.n_instr, "instructions", cs.n_params, "parameter floats", specialize.build(cs))
        return
    dev = torch.device("cuda:0")
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev)
    t = torch.tensor([[0.0, 0.0, -3.0]], device=dev)

    def frame_fn(scene, shader):
        scene, shader = scene().to(dev), shader().to(dev)
        loop = loop_for(scene, 1080, 1920, dev)

        def fn():
            with torch.no_grad():
                loop(q, t, shader, 1, 128)
        return fn

    def train_fn(scene, shader):
        scene, shader = scene().to(dev), shader().to(dev)
        loop = loop_for(scene, 512, 512, dev)
        params = list(scene.parameters()) + list(shader.parameters())
        opt = torch.optim.Adam(params, lr=1e-5, capturable=True)
        step = loop.training_step(lambda image: image.pow(2).mean(), mode=shader, marching_steps=64, optimizer=opt)
        return lambda: step(q, t)

    print(f"# {torch.cuda.get_device_name(0)}; frame = RenderLoop.forward, tile kernel, pose (0,0,-3); training step = the captured graph "
          f"of RenderLoop.training_step (forward, backward, Adam on every parameter)")
    ab({n: frame_fn(*pair) for n, pair in PAIRS.items()}, a.rounds, "frame 1920x1080x128")
    ab({n: train_fn(*pair) for n, pair in PAIRS.items()}, a.rounds, "training step 512x512x64")


if __name__ == "__main__":
    main()
