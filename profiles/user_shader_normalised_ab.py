"""What a user shader normalised by the frame's min / max costs next to the built-in mode it restates:

    python profiles/user_shader_normalised_ab.py --build-only      # no GPU: hipcc the libraries the run below needs
    python profiles/user_shader_normalised_ab.py > profiles/user_shader_normalised_ab.txt

make_test_scene2() at pose (0, 0, -3), alternating in one process: the built-in distance mode (mode 1) and its twin written as a
user shader with normalise="minmax" (tests/test_user_shader_normalised.py: UDistance, the same arithmetic and the same bytes),
contrib's DepthRampShader, and the per-pixel DirectionalLightShader -- the frame at 1920x1080x128 through the tile kernel, and the
forward + backward step at 512x512x64 (loss = mean of squares; the distance mode's gradients carry the reference's NaN at the two
extreme rays, which costs nothing).  Times are device events around FRAMES back-to-back calls, after warm-up; medians over ROUNDS
alternating rounds, and the round-to-round spread of the first entry (the built-in mode) is what differences are read against.

``--root DIR --which directional --no-step``: the same measurement with the package imported from another checkout of the project
(the parent commit, built), in a process of its own: the flat shader's frame, whose device code is unchanged, before and after."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--build-only", action="store_true")
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap.add_argument("--root", default=HERE)
ap.add_argument("--which", default="distance,udistance,depth_ramp,directional")
ap.add_argument("--no-step", action="store_true")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=40)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))

import torch  # noqa: E402
from ray_marching_amd import contrib, specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_for, compiled_with_shader  # noqa: E402
from ray_marching_amd.control import RenderLoop  # noqa: E402
from ray_marching_amd.scene.scene_registry import make_test_scene2  # noqa: E402

PX, EPS = 3.45e-6, 5e-2


def _udistance():
    from tests import test_user_shader_normalised as T
    T._register()
    return T.UDistance()


MODES = {"distance": lambda: 1,
         "udistance": _udistance,
         "depth_ramp": lambda: contrib.DepthRampShader([1.0, 0.9, 0.7], [0.05, 0.1, 0.3]),
         "directional": lambda: contrib.DirectionalLightShader([0.35, 0.5, -0.8], [0.9, 0.55, 0.3], 0.15)}


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
        print(f"{what:22s} {n:12s} median {statistics.median(v):8.4f} ms  min {min(v):8.4f}  max {max(v):8.4f}  "
              f"({rounds} rounds of {frames}: {' '.join(f'{x:.4f}' for x in v)})", flush=True)
    base = ms[names[0]]
    print(f"{what:22s} round-to-round spread of {names[0]}: {max(base) - min(base):.4f} ms "
          f"({(max(base) - min(base)) / statistics.median(base):.2%} of its median)", flush=True)
    for n in names[1:]:
        print(f"{what:22s} {n} - {names[0]} = {statistics.median(ms[n]) - statistics.median(base):+.4f} ms "
              f"(ratio {statistics.median(ms[n]) / statistics.median(base):.4f})", flush=True)


def main():
    names = [n for n in ARGS.which.split(",") if n]
    if ARGS.build_only:
        for name in names:
            mode = MODES[name]()
            cs = compiled_for(make_test_scene2()) if isinstance(mode, int) else compiled_with_shader(make_test_scene2(), mode)
            print(name, cs.n_instr, "instructions", cs.n_params, "parameter floats", specialize.build(cs))
        return
    dev = torch.device("cuda:0")
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev)
    t = torch.tensor([[0.0, 0.0, -3.0]], device=dev)
    on = lambda mode: mode if isinstance(mode, int) else mode.to(dev)

    def frame_fn(mode):
        loop, mode = loop_for(make_test_scene2(), 1080, 1920, dev), on(mode)

        def fn():
            with torch.no_grad():
                loop(q, t, mode, 1, 128)
        return fn

    def step_fn(mode):
        scene = make_test_scene2()
        loop, mode = loop_for(scene, 512, 512, dev), on(mode)
        params = list(scene.parameters()) + ([] if isinstance(mode, int) else [p for p in mode.parameters() if p.requires_grad])

        def fn():
            for p in params:
                p.grad = None
            loop(q, t, mode, 1, 64).pow(2).mean().backward()
        return fn

    print(f"# {torch.cuda.get_device_name(0)}; package from {'this checkout' if os.path.abspath(ARGS.root) == HERE else 'the checkout given with --root'}; "
          f"tile kernel, scene 2, pose (0,0,-3)")
    ab(names, frame_fn, ARGS.rounds, ARGS.frames, "frame 1920x1080x128")
    if not ARGS.no_step:
        ab(names, step_fn, ARGS.rounds, ARGS.frames, "fwd+bwd 512x512x64")


if __name__ == "__main__":
    main()
