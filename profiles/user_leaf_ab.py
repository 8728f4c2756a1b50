"""What a user-defined leaf costs on the GPU ("user leaves"):

    python profiles/user_leaf_ab.py --build-only          # no GPU: hipcc the libraries the runs below need
    python profiles/user_leaf_ab.py > profiles/user_leaf_ab.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/user_leaf_ab.py --trace-leg "link scene"      # kernel times, a run of its own

1. the glue alone: make_test_scene2() with its sphere restated as a user leaf against the built-in scene -- as compiled by
   default, and without cull tests (RM_CULL=0), which is the program the user-leaf scene gets: a union that holds a
   user leaf has no bounding sphere -- frame time at 1920x1080x128, alternating in one process (the spread between
   rounds of ONE scene is the noise floor);
2. the shipped leaf: contrib.make_link_scene() against the same scene with an SDFTorus in the link's place (again both
   ways), frame time at 1920x1080x128 and forward + backward of a Lambertian MSE step at 512x512x64.
Frame times are device events around FRAMES back-to-back frames, after warm-up; medians over ROUNDS rounds."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_marching_amd import specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_for  # noqa: E402
from ray_marching_amd.contrib import make_link_scene  # noqa: E402
from ray_marching_amd.control import RenderLoop  # noqa: E402
from ray_marching_amd.extensions import register_leaf  # noqa: E402
from ray_marching_amd.scene.primitives import SDFSphere, SDFTorus  # noqa: E402
from ray_marching_amd.scene.scene_registry import make_test_scene2  # noqa: E402

PX, EPS = 3.45e-6, 5e-2


class USphere(nn.Module):
    def __init__(self, radius):
        super().__init__()
        self.radius = nn.Parameter(torch.tensor(radius))

    def forward(self, p):
        return torch.linalg.vector_norm(p, dim=-1, keepdim=True) - self.radius


register_leaf(USphere, params=("radius",), cost=13, hip="""
template <bool Fast> RM_DEV float usphere_fwd(rm::V3 p, const float* theta) { return norm3_t<Fast>(p) - theta[0]; }
template <bool Fast> RM_DEV void usphere_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) {
  const float n = norm3_t<Fast>(p);
  const float s = (n == 0.0f) ? 0.0f : div_t<Fast>(g, n);
  gp = gp + mk3(p.x * s, p.y * s, p.z * s);
  gtheta[0] = -g;
}
""")


def scene2_user():
    s = make_test_scene2()
    assert isinstance(s.sdfs[1].sdfs[0], SDFSphere)
    s.sdfs[1].sdfs[0] = USphere(0.5)
    return s


def link_twin():
    s = make_link_scene()
    s.sdfs[1].sdfs[1].sdf = SDFTorus(0.3, 0.08)
    return s


def without_cull_tests(make):
    """The scene compiled under RM_CULL=0 (compiler.compiled_for keeps the program with the module).  A user leaf has no
    bounding sphere, so a union that holds one gets no CULL_MIN: this is the built-in program that is like for like."""
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


SCENES = {"scene2 built-in": make_test_scene2, "scene2 built-in, RM_CULL=0": without_cull_tests(make_test_scene2),
          "scene2 user sphere": scene2_user,
          "link scene": make_link_scene, "link scene, torus twin": link_twin,
          "torus twin, RM_CULL=0": without_cull_tests(link_twin)}


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
        print(f"{what:34s} {n:24s} median {statistics.median(v):8.4f} ms  min {min(v):8.4f}  max {max(v):8.4f}  "
              f"({rounds} rounds of {frames}: {' '.join(f'{x:.4f}' for x in v)})", flush=True)
    for n in names[:-1]:
        print(f"{what:34s} {names[-1]} / {n} = {statistics.median(ms[names[-1]]) / statistics.median(ms[n]):.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--trace-leg", metavar="SCENE", default=None, choices=sorted(SCENES),
                    help="a short run of one scene only (30 frames, 30 training steps), for rocprofv3 --kernel-trace --stats")
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

    def train_fn(scene):
        loop = loop_for(scene, 512, 512, dev)
        tt = torch.tensor([[0.0, 0.0, -1.5]], device=dev)

        def fn():
            for p in scene.parameters():
                p.grad = None
            loop(q, tt, 0, 1, 64).pow(2).mean().backward()
        return fn

    if a.trace_leg:
        f, g = frame_fn(SCENES[a.trace_leg]()), train_fn(SCENES[a.trace_leg]())
        for _ in range(30):
            f()
        for _ in range(30):
            g()
        torch.cuda.synchronize()
        return
    print(f"# {torch.cuda.get_device_name(0)}; frame = RenderLoop.forward, mode 0, tile kernel, pose (0,0,-3)")
    ab(["scene2 built-in", "scene2 built-in, RM_CULL=0", "scene2 user sphere"], frame_fn, a.rounds, a.frames, "frame 1920x1080x128")
    ab(["link scene, torus twin", "torus twin, RM_CULL=0", "link scene"], frame_fn, a.rounds, a.frames, "frame 1920x1080x128")
    ab(["link scene, torus twin", "torus twin, RM_CULL=0", "link scene"], train_fn, a.rounds, a.frames, "fwd+bwd 512x512x64 (Lambertian MSE)")


if __name__ == "__main__":
    main()
