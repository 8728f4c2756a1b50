"""What the table gradient of a user shader costs (needs an MI355X):

    python profiles/user_shader_table_timing.py > profiles/user_shader_table_timing.txt

Scene 2 at the training shape (512x512, 64 steps, pose (0, 0, -3)) shaded by contrib.DepthPaletteShader (T = 2, L = 16):
  backward          one backward of the frame (`loss.backward(retain_graph=True)`, device events around blocks of 40, synchronised),
                    with the palette as a BUFFER-like table (requires_grad=False: no records, no scatter) and as a PARAMETER
                    (records + rm_table_scatter), alternating in one process, 7 rounds; the difference is what the records and
                    the scatter cost together, host launches included
  k_table_scatter   rm_table_scatter alone on the 524 288 records of that frame (ops.table_scatter: the scatter kernel and the
                    fixed-tree sum of its chunk tables), with rows drawn uniformly from L = 16 and from L = 4096 (the peel's worst
                    case: nearly every lane of a group on a row of its own), and on the frame's own records at L = 16
Prints medians over the rounds and the round-to-round spread (max - min) of each entry."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from ray_marching_amd import ops  # noqa: E402
from ray_marching_amd.contrib import DepthPaletteShader  # noqa: E402
from ray_marching_amd.control import RenderLoop  # noqa: E402
from ray_marching_amd.scene.scene_registry import make_test_scene2  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs a GPU"
DEV = torch.device("cuda:0")
H = W = 512
STEPS, PX, ROUNDS, BLOCK = 64, 3.45e-6, 7, 40


def timed(fn, n=BLOCK):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def palette(n):
    x = torch.linspace(0.0, 1.0, n)[:, None]
    return 0.5 + 0.4 * torch.cos(2.0 * x + torch.tensor([0.0, 2.0, 4.0]))


scene = make_test_scene2().to(DEV)
loop = RenderLoop(scene, num_cameras=1, px_width=W, px_height=H, focal_length=PX * H, sensor_width=PX * W, sensor_height=PX * H,
                  normals_eps=5e-2).to(DEV)
q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV)
t = torch.tensor([[0.0, 0.0, -3.0]], device=DEV)
target = torch.rand(1, H, W, 3, generator=torch.Generator().manual_seed(0)).to(DEV)
entries = {}
for name, learn in (("buffer", False), ("parameter", True)):
    shader = DepthPaletteShader(0.3, palette(16)).to(DEV)
    shader.palette.requires_grad_(learn)
    loss = (loop(q, t, shader, 1, STEPS) - target).pow(2).mean()
    entries[name] = (shader, loss)


def backward(name):
    shader, loss = entries[name]
    for p in list(scene.parameters()) + list(shader.parameters()):
        p.grad = None
    loss.backward(retain_graph=True)


records = {}
n = H * W * 2
gen = torch.Generator().manual_seed(1)
for rows in (16, 4096):
    r = torch.randn(n, 4, generator=gen)
    r[:, 0] = torch.randint(0, rows, (n,), generator=gen).int().view(torch.float32)
    records[f"uniform rows, L = {rows}"] = (r.to(DEV).view(H * W, 2, 4), rows)
# the frame's own records: taken from one backward of the parameter entry through the hook below
kept = {}
real_scatter = ops.table_scatter
ops.table_scatter = lambda rec, rows, stream=None: (kept.__setitem__("frame", rec.clone()), real_scatter(rec, rows, stream))[1]
backward("parameter")
ops.table_scatter = real_scatter
records["the frame's own records, L = 16"] = (kept["frame"], 16)

for name in entries:
    timed(lambda: backward(name), 5)
for rec, rows in records.values():
    timed(lambda: ops.table_scatter(rec, rows), 5)
times = {k: [] for k in list(entries) + list(records)}
for _ in range(ROUNDS):
    for name in entries:
        times[name].append(timed(lambda: backward(name)))
    for name, (rec, rows) in records.items():
        times[name].append(timed(lambda: ops.table_scatter(rec, rows), 200))
print(f"# {torch.cuda.get_device_name(0)}; scene 2, {H}x{W}x{STEPS}, DepthPaletteShader (T = 2, L = 16); {ROUNDS} rounds, blocks of {BLOCK} backwards / 200 scatters")
print(f"# {'entry':44s} median [ms]   spread (max - min) [ms]")
for name, v in times.items():
    what = f"backward, palette as {name}" if name in entries else f"rm_table_scatter, {n} records, {name}"
    print(f"{what:46s} {statistics.median(v):10.4f}   {max(v) - min(v):10.4f}")
d = statistics.median(times["parameter"]) - statistics.median(times["buffer"])
print(f"# records + scatter in the backward: {d:+.4f} ms per backward")
