"""What shading a frame through a user-defined shader costs on the GPU ("user shaders"):

    python profiles/user_shader_ab.py --build-only          # no GPU: hipcc the libraries the run below needs
    python profiles/user_shader_ab.py > profiles/user_shader_ab.txt

make_test_scene2() shaded by the restated-Lambertian twin of the test suite (ULambert: the forward of built-in mode 0 as a
user shader without parameters -- the same arithmetic in the same kernel, reached through RM_MODE_USER) against built-in
mode 0 on the same scene: frame time at 1920x1080x128, alternating in one process.  The spread between the rounds of the
built-in mode is the noise floor the gap is read against; for orientation, contrib's DirectionalLightShader (seven
parameter floats) and DepthCueShader (four; reads origin and surface point) on the same scene.
Frame times are device events around FRAMES back-to-back frames, after warm-up; medians over ROUNDS rounds."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_for, compiled_with_shader  # noqa: E402
from ray_marching_amd.contrib import DepthCueShader, DirectionalLightShader  # noqa: E402
from ray_marching_amd.control import RenderLoop  # noqa: E402
from ray_marching_amd.scene.scene_registry import make_test_scene2  # noqa: E402
# the twin and its HIP source are those of the test suite: one definition, so that what is timed and what is compared bit for
# bit with the built-in mode are the same library
from tests.test_user_shader import ULambert, _register  # noqa: E402

PX, EPS = 3.45e-6, 5e-2
_register()

# name -> mode factory (an int: a built-in mode; else an instance of a registered shader class)
MODES = {"scene2 built-in mode 0": lambda: 0, "scene2 ULambert twin": ULambert,
         "scene2 DirectionalLightShader": lambda: DirectionalLightShader([0.35, 0.5, -0.8], [0.9, 0.55, 0.3], 0.15),
         "scene2 DepthCueShader": lambda: DepthCueShader(0.3, [0.2, 0.35, 0.6])}


def loop_for(scene, h, w, dev):
    return RenderLoop(scene, num_cameras=1, px_width=w, px_height=h, focal_length=PX * h, sensor_width=PX * w,
                      sensor_height=PX * h, normals_eps=EPS, regen=False).to(dev)


def time_ms(fn, frames):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(frames):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / frames


def ab(names, make_fn, rounds, frames, what):
    fns = {n: make_fn(MODES[n]()) for n in names}
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:                       # alternating
            ms[n].append(time_ms(fns[n], frames))
    for n in names:
        v = ms[n]
        print(f"{what:22s} {n:34s} median {statistics.median(v):8.4f} ms  min {min(v):8.4f}  max {max(v):8.4f}  "
              f"({rounds} rounds of {frames}: {' '.join(f'{x:.4f}' for x in v)})", flush=True)
    base = ms[names[0]]
    print(f"{what:22s} round-to-round spread of {names[0]}: {max(base) - min(base):.4f} ms "
          f"({(max(base) - min(base)) / statistics.median(base):.2%} of its median)", flush=True)
    for n in names[1:]:
        print(f"{what:22s} {n} - {names[0]} = {statistics.median(ms[n]) - statistics.median(base):+.4f} ms "
              f"(ratio {statistics.median(ms[n]) / statistics.median(base):.4f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=50)
    a = ap.parse_args()
    if a.build_only:
        for name, make in MODES.items():
            scene, mode = make_test_scene2(), make()
            cs = compiled_for(scene) if isinstance(mode, int) else compiled_with_shader(scene, mode)
            print(name, cs.n_instr, "instructions", cs.n_params, "parameter floats", specialize.build(cs))
        return
    dev = torch.device("cuda:0")
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev)
    t = torch.tensor([[0.0, 0.0, -3.0]], device=dev)

    def frame_fn(mode):
        scene = make_test_scene2()
        loop = loop_for(scene, 1080, 1920, dev)
        if not isinstance(mode, int):
            mode = mode.to(dev)
        assert (compiled_for(scene) if isinstance(mode, int) else compiled_with_shader(scene, mode)).specialised

        def fn():
            with torch.no_grad():
                loop(q, t, mode, 1, 128)
        return fn

    print(f"# {torch.cuda.get_device_name(0)}; frame = RenderLoop.forward, tile kernel, pose (0,0,-3)")
    ab(list(MODES), frame_fn, a.rounds, a.frames, "frame 1920x1080x128")


if __name__ == "__main__":
    main()
