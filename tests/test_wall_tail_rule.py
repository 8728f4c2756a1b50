"""The wall tail of the plain frame kernel (rm_kernels.h, `march`), restated on the CPU and held to the oracle.

A tile whose 64 rays all sit on one wall of the room keeps f bit for bit: the kernel then walks the steps that are left as
`p <- fl(f v) + p` with f held, without evaluating the scene.  This file restates the conditions under which it does so, with
the constants the kernel uses, on the oracle's fp32 trajectory, and asserts what the kernel relies on: wherever the
conditions hold for a whole tile, the tail's end point is the oracle's final iterate in every bit.

The one liberty: the kernel tests its carried lower bound `cull_lo` of every guarded child, this file the freshly computed
test value `slope |prev - c| - K` (oracle/bound_ref.py), which `cull_lo` never exceeds -- the restatement switches wherever
the kernel can, and sometimes a look earlier.  tests/test_wall_tail.py uses the same functions on the GPU's own trajectory.
"""
import math

import pytest
import torch

from oracle import bound_ref as B, sdf_oracle as O
from tests import helpers as H

OP_BOX, OP_UNION_BEGIN, OP_FOLD_MIN, OP_UNION_END, OP_ROUND, OP_ONION, OP_CULL_MIN = 2, 9, 10, 11, 15, 16, 17
F32 = torch.float32


def bits(x):
    return x.contiguous().view(torch.int32)


def same_bits(a, b):
    return (bits(a) == bits(b)).all(dim=-1)


def wall_program(cs):
    """StaticProgram::wall_box restated: (halfsides [3] fp32, [(c [3], K, slope) fp32 per guarded child]) of a room with
    guarded contents, None for every other program.  (Every CULL_MIN here sits in the outermost frame; the kernel also
    wants it among the first RM_CULL_TRACKED = 2.)"""
    prog = [[int(x) for x in row] for row in cs.program.tolist()]
    n = len(prog)
    if n < 4 or prog[0][0] != OP_UNION_BEGIN or prog[n - 1][0] != OP_UNION_END:
        return None
    block = torch.cat([p.detach().reshape(-1).double().cpu() for p in cs.leaves]).tolist()
    box, sites, pc = None, [], 1
    while pc < n - 1:
        if prog[pc][0] == OP_CULL_MIN:
            if len(sites) >= 2:
                return None
            s = B.cull_min_site(cs.program, block, pc)
            sites.append((torch.tensor(s[:3], dtype=F32), torch.tensor(s[3], dtype=F32), torch.tensor(s[4], dtype=F32)))
            pc += 1 + (prog[pc][3] >> 8)
            continue
        if box is not None or prog[pc][0] != OP_BOX:
            return None
        box = torch.tensor(block[prog[pc][1]:prog[pc][1] + 3], dtype=F32)
        pc += 1
        while pc < n - 1 and prog[pc][0] in (OP_ROUND, OP_ONION):
            pc += 1
        if pc >= n - 1 or prog[pc][0] != OP_FOLD_MIN:
            return None
        pc += 1
    return (box, sites) if (box is not None and pc == n - 1) else None


def looks_of(steps):
    """The look steps of the grouped march (tests/test_march_groups.py)."""
    return [d for d in (2, 4, 6, 8) if d <= steps] + list(range(12, steps + 1, 4))


def wall_rule(traj, f_of, v, h, sites, steps):
    """One tile.  traj [steps + 1, 64, 3] (row i = the iterate before step i), f_of(i) -> f(traj[i]) [64], v [64, 3], all
    fp32.  -> (nexec of the documented early-out, look at which the tile switches or None, the tail's end points or None)."""
    lam = torch.zeros(64, dtype=torch.int64)
    snap, snap_step, next_snap = traj[0], 0, 2
    vn = torch.tensor(1.0001, dtype=F32) * (v * v).sum(dim=-1).sqrt()
    hsum = h[0] + h[1] + h[2]
    for done in looks_of(steps):
        p, prev = traj[done], traj[done - 1]
        found = torch.where(same_bits(p, prev), 1, torch.where(same_bits(p, snap), done - snap_step, 0))
        lam = torch.where(lam == 0, found, lam)
        if bool((lam > 0).all()):
            return done, None, None
        if done == next_snap:
            snap, snap_step, next_snap = p, done, next_snap * 2
        if done < 12:           # the switch is tried behind the looks of the four-step groups only
            continue
        n = steps - done
        f = f_of(done - 1)
        move = f.abs() * vn + torch.tensor(4e-6, dtype=F32)
        D = (torch.tensor(1.0001, dtype=F32) * n) * (torch.tensor(2.1e-7, dtype=F32) * hsum + move) + torch.tensor(1e-6, dtype=F32) * hsum
        ok = torch.ones(64, dtype=torch.bool)
        for c, K, slope in sites:                                                   # (d)
            lhs = (prev - c).pow(2).sum(dim=-1).sqrt() * slope - K
            ok &= (lhs - D >= f)
        q = prev.abs() - h
        ok &= (q <= 0).all(dim=-1)                                                  # (a)
        m, a = q.max(dim=-1)
        frozen = bits(p).gather(1, a[:, None]) == bits(prev).gather(1, a[:, None])
        ok &= frozen[:, 0]                                                          # (b)
        second = q.sort(dim=-1).values[:, 1]
        ok &= (m - second >= D)                                                     # (c)
        if bool(ok.all()):
            for _ in range(n):
                p = f[:, None] * v + p
            return steps, done, p
    return steps, None, None


def tiles_of(x, h, w):
    """[h, w, 3] -> [tiles, 64, 3] in the frame kernels' 8x8 tile order (h and w multiples of 8)."""
    return x.reshape(h // 8, 8, w // 8, 8, 3).permute(0, 2, 1, 3, 4).reshape(-1, 64, 3)


def check_frame(spec, h, w, q, t, steps, what, check_march=False):
    """Every tile of one frame.  -> (tiles, switching tiles); asserts the tail of every switching tile."""
    from ray_marching_amd.compiler import compile_scene
    room = wall_program(compile_scene(H.spec_to_module(spec)))
    assert room is not None, what
    halfsides, sites = room
    bufs = O.camera_buffers(1, w, h, H.PX * h, H.PX * w, H.PX * h)
    pos, _, dirs = O.camera_forward(bufs[0], bufs[1], q, t)
    with torch.no_grad():
        # sdf_oracle.march_trajectory, keeping f(p_i) as well: the same expression, p <- f(p) v + p
        p, v = tiles_of(pos[0], h, w), tiles_of(dirs[0], h, w)
        traj, fs = [p], []
        for _ in range(steps):
            fs.append(O.sdf_eval(spec, p))
            p = fs[-1] * v + p
            traj.append(p)
        traj, fs = torch.stack(traj, dim=1), torch.stack(fs, dim=1)[..., 0]          # [tiles, steps + 1, 64, 3], [tiles, steps, 64]
        if check_march:
            assert bool(same_bits(traj[:, steps], tiles_of(O.march_trajectory(spec, pos[0], dirs[0], steps)[steps], h, w)).all())
        switched = 0
        for k in range(traj.shape[0]):
            f_of = lambda i: fs[k, i]
            _, done, end = wall_rule(traj[k], f_of, v[k], halfsides, sites, steps)
            if done is not None:
                switched += 1
                assert bool(same_bits(end, traj[k, steps]).all()), (what, k, done)
    return traj.shape[0], switched


IDENT = torch.tensor([[1.0, 0.0, 0.0, 0.0]])


@pytest.mark.parametrize("h,w,draft", [(72, 128, 54), (40, 64, 10)])
def test_scene2_frames(h, w, draft, monkeypatch):
    """Scene 2 at (0, 0, -3), 128 steps: the tail of every switching tile ends on the oracle's p_128, and at least half as
    many tiles switch as the draft rule of the issue found (54 of 144, 10 of 40)."""
    monkeypatch.setenv("RM_CULL_MIN_COST", "0")
    tiles, switched = check_frame(O.scene_test2(), h, w, IDENT, torch.tensor([[0.0, 0.0, -3.0]]), 128, (h, w), check_march=(h == 40))
    print(f"wall tail rule: scene 2 {h}x{w}x128: {switched} of {tiles} tiles switch")
    assert 2 * switched >= draft, (switched, tiles)


def random_room(gen):
    """A room of unequal half-sides under round / onion wrappers and one or two guarded children, one of them a sphere placed
    near a wall or far from all of them; the camera inside, aimed anywhere -- walls, edges and corners."""
    u = lambda lo, hi: float(torch.rand((), generator=gen)) * (hi - lo) + lo
    half = [u(1.5, 6.0), u(1.5, 6.0), u(1.5, 6.0)]
    room = ("box", {"halfsides": torch.tensor(half)})
    for _ in range(int(torch.randint(0, 3, (), generator=gen))):
        if u(0, 1) < 0.5:
            room = ("onion", {"radius": torch.tensor(u(0.02, 0.2))}, room)
        else:
            room = ("rounding", {"rounding": torch.tensor(u(0.0, 0.1))}, room)
    near = u(0, 1) < 0.5
    axis = int(torch.randint(0, 3, (), generator=gen))
    at = [u(-0.5, 0.5) * half[k] for k in range(3)]
    r = u(0.2, 0.6)
    if near:
        at[axis] = half[axis] - r - u(0.0, 0.3)
    aff = lambda child, at: ("affine", {"translation": torch.tensor(at), "orientation": torch.tensor([1.0, 0.0, 0.0, 0.0])}, child)
    kids = [room, aff(("union", {}, [("sphere", {"radius": torch.tensor(r)}), ("torus", {"radius1": torch.tensor(r), "radius2": torch.tensor(0.1)})]), at)]
    if u(0, 1) < 0.4:
        kids.append(aff(("smooth_union", {"blend_k": torch.tensor(16.0)},
                         [("sphere", {"radius": torch.tensor(0.3)}), ("box", {"halfsides": torch.tensor([0.2, 0.3, 0.1])})]),
                        [u(-0.4, 0.4) * half[k] for k in range(3)]))
    q = torch.nn.functional.normalize(torch.randn(1, 4, generator=gen), dim=-1)
    t = torch.tensor([[u(-0.3, 0.3) * half[k] for k in range(3)]])
    return ("union", {}, kids), q, t


def test_random_rooms(monkeypatch):
    """50 random rooms, 16 x 16 frames, step counts 33, 36, 64 and 128 in turn: wherever the rule switches, the tail is the
    oracle's final iterate bit for bit; it does switch somewhere and does refuse somewhere."""
    monkeypatch.setenv("RM_CULL_MIN_COST", "0")
    total = switched = 0
    for case in range(50):
        gen = torch.Generator().manual_seed(9100 + case)
        spec, q, t = random_room(gen)
        steps = (33, 36, 64, 128)[case % 4]
        n, s = check_frame(spec, 16, 16, q, t, steps, (case, steps))
        total += n
        switched += s
    print(f"wall tail rule: random rooms: {switched} of {total} tiles switch")
    assert switched >= 10 and total - switched >= 10, (switched, total)


def test_programs_that_qualify():
    """wall_program on the benchmark scenes: scene 2, the closed scene 1 and the 32-primitive scene are rooms with guarded
    contents; the open scene 1 and a room under an affine node are not."""
    from ray_marching_amd.compiler import compile_scene
    from ray_marching_amd.scene import scene_registry as R
    assert wall_program(compile_scene(R.make_test_scene2())) is not None
    assert wall_program(compile_scene(R.make_closed_test_scene())) is not None
    assert wall_program(compile_scene(R.make_many_primitive_scene(32))) is not None
    assert wall_program(compile_scene(R.make_test_scene())) is None
    moved = ("affine", {"translation": torch.tensor([0.1, 0.0, 0.0]), "orientation": torch.tensor([1.0, 0.0, 0.0, 0.0])}, O.scene_room())
    assert wall_program(compile_scene(H.spec_to_module(("union", {}, [moved, O.scene_test2()[2][1]])))) is None
    assert math.isfinite(float(wall_program(compile_scene(R.make_test_scene2()))[1][0][1]))
