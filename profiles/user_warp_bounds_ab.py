"""What the shipped domain operators gain once they sign a bound ("user warp bounds"):

    python profiles/user_warp_bounds_ab.py --build-only          # no GPU: hipcc the two libraries the run below needs
    python profiles/user_warp_bounds_ab.py                        # writes profiles/user_warp_bounds_ab.txt

contrib.make_warped_scene(bounded=True) -- SDFBoundedScale / SDFBoundedMirror / SDFBoundedElongate: a cull test over the
mirrored pair and one over a placed child inside it -- against contrib.make_warped_scene(), whose operators sign no bound and
whose program has no cull test at all.  The unbounded scene's library is the one every commit before warp bounds compiled
(same code header, same device assembly), so its time is the baseline.  Frame time at 1920x1080x128, mode 0, tile kernel,
alternating between the two scenes in one process: device events around FRAMES back-to-back frames, after warm-up; medians
over ROUNDS rounds.  The spread between the rounds of ONE scene is the noise floor: the bounded scene must not be slower than
the baseline by more than the baseline's own spread (the last line says so, and the exit status is 1 where it is)."""
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

PX, EPS = 3.45e-6, 5e-2
SCENES = {"warped scene, no bound": make_warped_scene, "warped scene + bounds": lambda: make_warped_scene(bounded=True)}
OUT = os.path.join(ROOT, "profiles", "user_warp_bounds_ab.txt")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.build_only:
        for name, make in SCENES.items():
            cs = compiled_for(make())
            print(name, cs.n_instr, "instructions,", int((cs.program[:, 0] == 17).sum()), "cull tests", specialize.build(cs))
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

    names = list(SCENES)
    fns = {n: frame_fn(SCENES[n]()) for n in names}
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    for _ in range(a.rounds):
        for n in names:                       # alternating
            ms[n].append(time_ms(fns[n], a.frames))
    what = "frame 1920x1080x128"
    lines = [f"# {torch.cuda.get_device_name(0)}; frame = RenderLoop.forward, mode 0, tile kernel, pose (0,0,-3)"]
    for n in names:
        v = ms[n]
        lines.append(f"{what:22s} {n:26s} median {statistics.median(v):8.4f} ms  min {min(v):8.4f}  max {max(v):8.4f}  "
                     f"spread {(max(v) - min(v)) / statistics.median(v) * 100:5.2f} %  ({a.rounds} rounds of {a.frames}: {' '.join(f'{x:.4f}' for x in v)})")
    base, new = ms[names[0]], ms[names[1]]
    slower_by = statistics.median(new) - statistics.median(base)
    ok = slower_by <= max(base) - min(base)
    lines.append(f"{what:22s} {names[1]} / {names[0]} = {statistics.median(new) / statistics.median(base):.4f}")
    lines.append(f"{what:22s} bounded - baseline = {slower_by:+.4f} ms, the baseline's spread over its rounds {max(base) - min(base):.4f} ms: "
                 f"{'not slower than the baseline beyond its spread' if ok else 'SLOWER than the baseline beyond its spread'}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(a.out, "w") as f:
        f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
