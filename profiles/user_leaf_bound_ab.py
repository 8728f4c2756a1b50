"""What a user-defined leaf costs once it signs a bounding sphere ("user leaves"; INTEGRATION.md, "What
it costs").  One leg per process, each under its own time limit, the output appended to profiles/user_leaf_bound_ab.txt:

    python profiles/user_leaf_bound_ab.py --build-only          # no GPU: hipcc the libraries the legs need
    timeout -k 10 300 python profiles/user_leaf_bound_ab.py --leg scene2 > profiles/user_leaf_bound_ab.txt && \\
    timeout -k 10 300 python profiles/user_leaf_bound_ab.py --leg link >> profiles/user_leaf_bound_ab.txt && \\
    timeout -k 10 300 python profiles/user_leaf_bound_ab.py --leg train >> profiles/user_leaf_bound_ab.txt && \\
    timeout -k 10 300 python profiles/user_leaf_bound_ab.py --leg setup >> profiles/user_leaf_bound_ab.txt

scene2: make_test_scene2() with its sphere restated as a user leaf that signs the sphere's bound (BSphere: the program of
        the built-in scene, row for row) against the built-in scene and against the same leaf without a bound.  Same
        program, same handler arithmetic: the expectation is a ratio of 1 within the round-to-round spread of the built-in
        scene in this run.
link:   contrib.make_link_scene(bounded=True) against make_link_scene() (no bound: the program every commit before
        NAME_bound compiled) and against the same scene with an SDFTorus in the link's place (cull tests by default).
train:  the link scenes, forward + backward of a Lambertian MSE step at 512x512x64.
setup:  the prologue: module(64 points), one block whose work is one evaluation, launches back to back -- with the
        validated scene-block cache (the walk over the program runs once) and without it (every launch walks, one more
        site per bounded leaf).  Back to back these launches are bound by the host's enqueue; the kernel's own time comes
        from a kernel trace, one scene per process (the kernel name is the same for all of them):
            rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/user_leaf_bound_ab.py --leg setup --only "link scene + bound" --rounds 1
Frame times are device events around FRAMES back-to-back frames at 1920x1080x128, after warm-up, alternating between the
scenes; medians over ROUNDS rounds."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ray_marching_amd import ops, specialize  # noqa: E402
from ray_marching_amd.compiler import compiled_for  # noqa: E402
from ray_marching_amd.contrib import make_link_scene  # noqa: E402
from ray_marching_amd.control import RenderLoop  # noqa: E402
from ray_marching_amd.extensions import register_leaf  # noqa: E402
from ray_marching_amd.scene.primitives import SDFSphere, SDFTorus  # noqa: E402
from ray_marching_amd.scene.scene_registry import make_test_scene2  # noqa: E402

PX, EPS = 3.45e-6, 5e-2


class _Ball(nn.Module):
    def __init__(self, radius):
        super().__init__()
        self.radius = nn.Parameter(torch.tensor(radius))

    def forward(self, p):
        return torch.linalg.vector_norm(p, dim=-1, keepdim=True) - self.radius


class USphere(_Ball):
    pass


class BSphere(_Ball):
    pass


_HIP = """
template <bool Fast> RM_DEV float NAME_fwd(rm::V3 p, const float* theta) { return norm3_t<Fast>(p) - theta[0]; }
template <bool Fast> RM_DEV void NAME_vjp(rm::V3 p, const float* theta, float g, rm::V3& gp, float* gtheta) {
  const float n = norm3_t<Fast>(p);
  const float s = (n == 0.0f) ? 0.0f : div_t<Fast>(g, n);
  gp = gp + mk3(p.x * s, p.y * s, p.z * s);
  gtheta[0] = -g;
}
"""
register_leaf(USphere, params=("radius",), cost=13, hip=_HIP.replace("NAME", "usphere"))
register_leaf(BSphere, params=("radius",), cost=13, hip=_HIP.replace("NAME", "bsphere") + """
RM_DEV void bsphere_bound(const float* theta, rm::LeafBound& b) { if (theta[0] >= 0.0f) b.R = b.Ru = theta[0]; }
""")


def scene2_with(cls):
    def factory():
        s = make_test_scene2()
        assert isinstance(s.sdfs[1].sdfs[0], SDFSphere)
        s.sdfs[1].sdfs[0] = cls(0.5)
        return s
    return factory


def link_twin():
    s = make_link_scene()
    s.sdfs[1].sdfs[1].sdf = SDFTorus(0.3, 0.08)
    return s


SCENES = {"scene2 built-in": make_test_scene2, "scene2 user sphere, no bound": scene2_with(USphere),
          "scene2 user sphere + bound": scene2_with(BSphere),
          "link scene, no bound": make_link_scene, "link scene, torus twin": link_twin,
          "link scene + bound": lambda: make_link_scene(bounded=True)}
LEGS = {"scene2": ["scene2 user sphere, no bound", "scene2 built-in", "scene2 user sphere + bound"],
        "link": ["link scene, no bound", "link scene, torus twin", "link scene + bound"]}
LEGS["train"] = LEGS["setup"] = LEGS["link"]


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
        print(f"{what:36s} {n:30s} median {statistics.median(v):8.4f} ms  min {min(v):8.4f}  max {max(v):8.4f}  "
              f"spread {(max(v) - min(v)) / statistics.median(v) * 100:5.2f} %  ({rounds} rounds of {frames}: {' '.join(f'{x:.4f}' for x in v)})",
              flush=True)
    for n in names[:-1]:
        print(f"{what:36s} {names[-1]} / {n} = {statistics.median(ms[names[-1]]) / statistics.median(ms[n]):.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--leg", choices=sorted(LEGS), default="scene2")
    ap.add_argument("--only", metavar="SCENE", default=None, choices=sorted(SCENES), help="this scene of the leg only (a kernel trace per scene)")
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

    def setup_fn(scene):
        scene = scene.to(dev)
        assert compiled_for(scene).specialised
        p = torch.randn(64, 3, generator=torch.Generator().manual_seed(0)).to(dev)

        def fn():
            with torch.no_grad():
                scene(p)
        return fn

    if a.only:
        LEGS[a.leg] = [a.only]
    print(f"# {torch.cuda.get_device_name(0)}; leg {a.leg}; frame = RenderLoop.forward, mode 0, tile kernel, pose (0,0,-3)", flush=True)
    if a.leg in ("scene2", "link"):
        ab(LEGS[a.leg], frame_fn, a.rounds, a.frames, "frame 1920x1080x128")
    elif a.leg == "train":
        ab(LEGS[a.leg], train_fn, a.rounds, a.frames, "fwd+bwd 512x512x64 (Lambertian MSE)")
    else:
        for cache in ((False,) if a.only else (True, False)):      # (a trace of one scene: every launch walks)
            ops.use_scene_cache = cache
            ab(LEGS[a.leg], setup_fn, a.rounds, 40 * a.frames, f"module(64 points), scene cache {'on' if cache else 'off'}")


if __name__ == "__main__":
    main()
