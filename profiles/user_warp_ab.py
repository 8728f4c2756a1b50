"""What the user-warp glue costs on the GPU ("user warps"):

    python profiles/user_warp_ab.py --build-only          # no GPU: hipcc the libraries the run below needs
    python profiles/user_warp_ab.py > profiles/user_warp_ab.txt

1. the glue alone: scene 2 with its sphere and torus placed by affine nodes (make_test_scene2() itself has no affine node to
   restate), every SDFAffineTransformation restated as a user warp (UAffine: the map and the VJP of RM_OP_AFFINE_PUSH),
   against the built-in scene compiled without cull tests (RM_CULL=0), which is the same work: a subtree that holds a warp
   gets no CULL_MIN -- frame time at 1920x1080x128, alternating in one process (the spread between rounds of ONE scene is
   the noise floor);
2. for orientation: the same built-in scene with default culling (what having no bound costs), make_test_scene2() and
   contrib.make_warped_scene().
Frame times are device events around FRAMES back-to-back frames, after warm-up; medians over ROUNDS rounds."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_for  # noqa: E402
from ray_marching_amd.contrib import make_warped_scene  # noqa: E402
from ray_marching_amd.control import RenderLoop  # noqa: E402
from ray_marching_amd.scene.scene_registry import make_test_scene2  # noqa: E402
# UAffine, its HIP source and the placed scene 2 are those of the test suite: one definition, so that what is timed and what
# is compared bit for bit with the built-in scene are the same library
from tests.test_user_warp import _register, scene2_placed, with_uaffine  # noqa: E402

PX, EPS = 3.45e-6, 5e-2
_register()


def without_cull_tests(make):
    """The scene compiled under RM_CULL=0 (compiler.compiled_for keeps the program with the module)."""
    def factory():
        scene = make()
        old = os.environ.get("RM_CULL")
        os.environ["RM_CULL"] = "0"
        try:
            compiled_for(scene)
        finally:
            if old is None:
                del os.environ["RM_CULL"]
            else:
                os.environ["RM_CULL"] = old
        return scene
    return factory


SCENES = {"placed scene2 built-in, RM_CULL=0": without_cull_tests(scene2_placed), "placed scene2 UAffine twin": lambda: with_uaffine(scene2_placed()),
          "placed scene2 built-in": scene2_placed, "scene2 built-in": make_test_scene2, "warped scene": make_warped_scene}


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
    fns = {n: make_fn(SCENES[n]()) for n in names}
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
    for n in names[1:]:
        print(f"{what:22s} {n} / {names[0]} = {statistics.median(ms[n]) / statistics.median(ms[names[0]]):.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=50)
    a = ap.parse_args()
    if a.build_only:
        for name, make in SCENES.items():
            scene = make()
            print(name, compiled_for(scene).n_instr, "instructions", specialize.build(compiled_for(scene)))
        return
    dev = torch.device("cuda:0")
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev)
    t = torch.tensor([[0.0, 0.0, -3.0]], device=dev)

    def frame_fn(scene):
        assert compiled_for(scene).specialised
        loop = loop_for(scene, 1080, 1920, dev)

        def fn():
            with torch.no_grad():
                loop(q, t, 0, 1, 128)
        return fn

    print(f"# {torch.cuda.get_device_name(0)}; frame = RenderLoop.forward, mode 0, tile kernel, pose (0,0,-3)")
    ab(list(SCENES), frame_fn, a.rounds, a.frames, "frame 1920x1080x128")


if __name__ == "__main__":
    main()
