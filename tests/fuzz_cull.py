"""Fuzz of the exactness of CULL_MIN: random scene trees (tests/helpers.random_spec: all 11 node types,
un-normalised quaternions, nested unions) with their parameters additionally scaled and shifted at random,
compiled with a cull test in front of EVERY boundable union child (RM_CULL_MIN_COST=0) and without any
(RM_CULL=0); values at 16 k points and point gradients must be bit-identical.  Parameter gradients are sums
over the points, reduced per block: the longer program changes the interpreter's LDS footprint and with it the
block size rm_abi.hip picks, so their partial sums may be grouped differently -- they are compared to 1e-3 of
the largest component plus 2e-6 of the scene's largest gradient instead (found by this fuzz: 11 of 134 trees, values and point gradients identical).
    python tests/fuzz_cull.py [n_seeds]        (a script, not collected by pytest: ~1 s per tree)
FUZZ_WIDEN=1 draws the trees through helpers.widen_spec as well (negative rounding / onion, |q|^2 in 0.77 .. 1.9)."""
import os, sys
root = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import torch
os.environ["RM_SPECIALIZE"] = "off"
os.environ["RM_CULL_MIN_COST"] = "0"
import helpers as H
from oracle import sdf_oracle as O          # spec utilities shared with tests/helpers.py
from ray_marching_amd import _abi
from ray_marching_amd.compiler import compiled_for

dev = torch.device("cuda:0")
n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 200
same = lambda x, y: torch.equal(torch.nan_to_num(x, nan=1234.5), torch.nan_to_num(y, nan=1234.5)) and torch.equal(x.isnan(), y.isnan())
bad, with_culls, total_culls = [], 0, 0
seeds = [int(x) for x in os.environ['FUZZ_SEEDS'].split(',')] if os.environ.get('FUZZ_SEEDS') else range(n_seeds)
for seed in seeds:
    gen = torch.Generator().manual_seed(900000 + seed)
    spec = O.map_spec(H.random_spec(gen), lambda x: x.clone().float())
    if os.environ.get("FUZZ_WIDEN"):        # negative rounding / onion, |q|^2 in 0.77 .. 1.9 (helpers.widen_spec; its own stream)
        spec = H.widen_spec(spec, torch.Generator().manual_seed(1900000 + seed))
    scale = float(torch.rand(1, generator=gen) * 3 + 0.2)
    pts = torch.cat([(torch.rand(8192, 3, generator=gen) * 2 - 1) * 6 * scale, (torch.rand(8192, 3, generator=gen) * 2 - 1) * scale]).to(dev)
    wts = torch.randn(pts.shape[0], 1, generator=gen).to(dev)
    res = {}
    for cull in ("0", "1"):
        os.environ["RM_CULL"] = cull
        g2 = torch.Generator().manual_seed(77 + seed)
        module = H.spec_to_module(spec)
        with torch.no_grad():
            for name, p in module.named_parameters():
                if name.endswith("orientation"):
                    p.mul_(0.75 + 0.6 * float(torch.rand(1, generator=g2)))
                elif name.endswith("translation") or name.endswith("start") or name.endswith("end"):
                    p.mul_(scale)
                else:
                    p.mul_(0.5 + float(torch.rand(1, generator=g2)))
        module = module.to(dev)
        cs = compiled_for(module)
        n_cull = int((cs.program.reshape(-1, 4)[:, 0] == _abi.OP_CULL_MIN).sum())
        p = pts.clone().requires_grad_(True)
        d = module(p)
        (d * wts).sum().backward()
        res[cull] = (d.detach(), p.grad, [None if x.grad is None else x.grad.clone() for x in module.parameters()], n_cull)
    a, b = res["0"], res["1"]
    gmax = max([float(torch.nan_to_num(x).abs().max()) for x in a[2] if x is not None] + [0.0])
    def close(x, y):
        # cancellation: a component of 1e-4 can be the sum of terms of order gmax, so part of the allowance
        # scales with the largest gradient of the scene
        fx, fy = torch.nan_to_num(x.double()), torch.nan_to_num(y.double())
        return torch.equal(x.isnan(), y.isnan()) and float((fx - fy).abs().max()) <= 1e-3 * float(fx.abs().max()) + 2e-6 * gmax + 1e-12
    ok = same(a[0], b[0]) and same(a[1], b[1]) and all((x is None) == (y is None) and (x is None or close(x, y)) for x, y in zip(a[2], b[2]))
    with_culls += b[3] > 0; total_culls += b[3]
    if not ok:
        bad.append(seed)
        print(f"seed {seed}: MISMATCH ({b[3]} cull sites), max |dd| {float((torch.nan_to_num(a[0]) - torch.nan_to_num(b[0])).abs().max()):.3g}", flush=True)
        if os.environ.get("FUZZ_VERBOSE"):
            dp = (torch.nan_to_num(a[1]) - torch.nan_to_num(b[1])).abs()
            print("   point grads: n diff", int((dp > 0).sum()), "max", float(dp.max()), "nan pattern equal", bool(torch.equal(a[1].isnan(), b[1].isnan())))
            names = [n for n, _ in module.named_parameters()]
            for n, x, y in zip(names, a[2], b[2]):
                if x is None or same(x, y):
                    continue
                print("   param", n, "nocull", x.flatten().tolist(), "cull", y.flatten().tolist())
            rows = cs.program.reshape(-1, 4).tolist()
            print("   program:", rows)
print(f"{n_seeds} random trees, {with_culls} with cull sites ({total_culls} sites in total): {len(bad)} mismatches {bad}")
if bad:
    sys.exit(1)


def fuzz_static(n_trees):
    """The specialised kernels (cull decisions carried from step to step) against the unculled interpreter:
    frames of random trees, bit for bit.  ~10 s of hipcc per tree."""
    from ray_marching_amd import specialize
    done = 0
    seed = 0
    bad_static = []
    while done < n_trees and seed < 2000:
        gen = torch.Generator().manual_seed(900000 + seed)
        spec = O.map_spec(H.random_spec(gen), lambda x: x.clone().float())
        seed += 1
        os.environ["RM_CULL"] = "1"; os.environ["RM_SPECIALIZE"] = "off"
        probe = compiled_for(H.spec_to_module(spec))
        rows = probe.program.reshape(-1, 4)
        if int((rows[:, 0] == _abi.OP_CULL_MIN).sum()) == 0:
            continue
        frames = {}
        for variant in ("interp_nocull", "static"):
            os.environ["RM_CULL"] = "0" if variant == "interp_nocull" else "1"
            os.environ["RM_SPECIALIZE"] = "off" if variant == "interp_nocull" else "jit"
            specialize._loaded.clear()
            module = H.spec_to_module(spec).to(dev)
            loop = H.make_loop(module, 48, 64)
            out = []
            with torch.no_grad():
                for t in ([0.0, 0.0, -4.0], [2.5, 1.0, -1.0]):
                    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev); tt = torch.tensor([t], device=dev)
                    out += [loop(q, tt, m, 1, 80) for m in (4, 0)]
            frames[variant] = out
            spec_flag = compiled_for(loop.scene).specialised
        ok = all(same(a, b) for a, b in zip(frames["interp_nocull"], frames["static"]))
        print(f"static tree seed {seed - 1}: specialised={spec_flag} {'ok' if ok else 'MISMATCH'}", flush=True)
        if not ok:
            bad_static.append(seed - 1)
        done += 1
    specialize._loaded.clear()
    return bad_static


if os.environ.get("FUZZ_STATIC"):
    bs = fuzz_static(int(os.environ["FUZZ_STATIC"]))
    print("static mismatches:", bs)
    sys.exit(1 if bs else 0)
