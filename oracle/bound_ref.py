"""Float64 restatement of the bounding-sphere walk of the kernels.  TEST INFRASTRUCTURE ONLY.

``ray_marching_amd/csrc/rm_device.h: subtree_bound`` derives, for the subtree encoded by the instructions
``[begin, end)`` of a compiled program, a centre ``c``, radii ``R`` / ``Ru`` and slopes with

    subtree(p) >= slope |p - c| - R        and, where known,        subtree(p) <= uslope |p - c| + Ru

and ``derive_constants`` stores them, with margins, as the 5 floats of every ``RM_OP_CULL_MIN`` site and the 8-float rows
of every smooth union's bound table.  This file states the same contract and the same arithmetic
-- inflation factors, give-ups and final checks included -- as a scalar walk in Python floats (IEEE double), over the
built-in opcodes only.  The tests compare the device's numbers with these and check these against the oracle's float64
values of the subtree (tests/test_scene_bounds.py).

The NaN contract, stated here once: a NaN in ANY parameter that the subtree reads gives ``R = Ru = inf`` ("no bound": the
node's value is NaN somewhere the bound would promise a number), and so does a capsule whose end points coincide (its
``AB / |AB|^2`` is 0 / 0).  A blend_k that is not a positive finite number gives no bound either (k = +inf makes
``-lse(-k d) / k`` NaN).  ``inf`` parameters are no NaNs: they go through the arithmetic.
"""
from __future__ import annotations

import math

OP_SPHERE, OP_BOX, OP_PLANE, OP_LINE, OP_DISK, OP_TORUS = 1, 2, 3, 4, 5, 6
OP_AFFINE_PUSH, OP_AFFINE_POP = 7, 8
OP_UNION_BEGIN, OP_FOLD_MIN, OP_UNION_END = 9, 10, 11
OP_SMOOTH_BEGIN, OP_FOLD_LSE, OP_SMOOTH_END = 12, 13, 14
OP_ROUND, OP_ONION = 15, 16
OP_CULL_MIN, OP_CULL_LSE = 17, 18

BOUND_DEPTH = 12          # kBoundDepth: frames (affine, union, smooth union) the walk can nest
INF, NAN = math.inf, math.nan

# parameter floats each opcode reads at its offset (the NaN contract looks at exactly these)
_READS = {OP_SPHERE: 1, OP_BOX: 3, OP_LINE: 7, OP_DISK: 1, OP_TORUS: 2, OP_AFFINE_POP: 7, OP_SMOOTH_END: 1,
          OP_ROUND: 1, OP_ONION: 1}


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _qrot(v, w, qv):
    """v + w t + qv x t with t = 2 qv x v: the reference's rotation, q NOT normalised."""
    t = tuple(2.0 * x for x in _cross(qv, v))
    y = _cross(qv, t)
    return tuple((y[i] + w * t[i]) + v[i] for i in range(3))


def _l1(c):
    return abs(c[0]) + abs(c[1]) + abs(c[2])


def _norm(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def bound(program_rows, params_f64, begin, end):
    """Bound of the subtree ``program_rows[begin:end]`` (rows ``(opcode, offset, aux0, aux1)``) for the parameter block
    ``params_f64`` (any sequence of floats): ``(c[3], R, slope, Ru, uslope)``; ``inf`` stands for "no bound".  A user opcode
    raises ValueError."""
    P = [float(x) for x in params_f64]
    c, R, slope, Ru, uslope = (0.0, 0.0, 0.0), INF, 1.0, INF, 1.0
    stack = []                 # ("affine", off) | ["union", c, R, slope, n]
    overflow = poisoned = False
    for pc in range(begin, end):
        op, off = int(program_rows[pc][0]), int(program_rows[pc][1])
        if any(math.isnan(x) for x in P[off:off + _READS.get(op, 0)]):
            poisoned = True
        if op in (OP_SPHERE, OP_DISK):
            c, slope, uslope = (0.0, 0.0, 0.0), 1.0, 1.0
            R = Ru = P[off] if P[off] >= 0.0 else INF
        elif op == OP_BOX:
            h = P[off:off + 3]
            c, slope, uslope = (0.0, 0.0, 0.0), 1.0, 1.0
            R = Ru = _norm(h) if all(x >= 0.0 for x in h) else INF
        elif op == OP_PLANE:
            slope = uslope = 1.0
            R = Ru = INF
        elif op == OP_LINE:    # capsule: sphere around the midpoint of AB, half length inflated by 1.00001
            a = P[off:off + 7]
            c = tuple(0.5 * (a[i] + a[3 + i]) for i in range(3))
            half = _norm(tuple(0.5 * (a[3 + i] - a[i]) for i in range(3)))
            slope = uslope = 1.0
            ab = tuple(a[3 + i] - a[i] for i in range(3))
            degenerate = not ((ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2] > 0.0)      # AB / |AB|^2 = 0 / 0
            R = Ru = half * 1.00001 + a[6] if a[6] >= 0.0 and not degenerate else INF
        elif op == OP_TORUS:
            c, slope, uslope = (0.0, 0.0, 0.0), 1.0, 1.0
            R = Ru = P[off] + P[off + 1] if P[off] >= 0.0 and P[off + 1] >= 0.0 else INF
        elif op == OP_ROUND:   # d - r <= ub + max(-r, 0);  d - r >= d - max(r, 0)
            r = P[off]
            if math.isnan(r):
                R = Ru = INF
            else:
                Ru = Ru + max(-r, 0.0)
                R = R + max(r, 0.0)
        elif op == OP_ONION:   # |d| <= uslope |p - c| + max(Ru, R)  (d >= -R);  |d| - r >= d - max(r, 0)
            r = P[off]
            if math.isnan(r) or math.isnan(R) or math.isnan(Ru):
                R = Ru = INF
            else:
                Ru = max(Ru, R) + max(-r, 0.0)
                R = R + max(r, 0.0)
        elif op == OP_AFFINE_PUSH:
            if len(stack) >= BOUND_DEPTH:
                overflow = True
                break
            stack.append(("affine", off))
        elif op == OP_AFFINE_POP:
            a = P[stack.pop()[1]:][:7]
            w4, qv = a[3], (a[4], a[5], a[6])
            s2 = ((w4 * w4 + qv[0] * qv[0]) + qv[1] * qv[1]) + qv[2] * qv[2]
            sigma = min(1.0, 2.0 * s2 - 1.0) - 1e-5          # smallest singular value of M, rounded down
            if not (sigma > 0.5) or not (s2 < 4.0):
                R = Ru = INF
                continue
            c1 = _qrot(c, w4, qv)
            back = _qrot(c1, w4, tuple(-x for x in qv))
            e = _norm(tuple(back[i] - c[i] for i in range(3)))
            c = tuple(c1[i] + a[i] for i in range(3))
            R = (R + e) * 1.0001 + 1e-4 * _l1(c)
            slope = slope * sigma
            Ru = (Ru + uslope * e) * 1.0001 + 1e-4 * _l1(c)
            uslope = uslope * (max(1.0, 2.0 * s2 - 1.0) + 1e-5)
        elif op in (OP_UNION_BEGIN, OP_SMOOTH_BEGIN):
            if len(stack) >= BOUND_DEPTH:
                overflow = True
                break
            stack.append(["union", (0.0, 0.0, 0.0), 0.0, 1.0, 0])
        elif op in (OP_FOLD_MIN, OP_FOLD_LSE):   # smallest sphere around the two spheres; the smallest slope
            f = stack[-1]
            if f[4] == 0:
                f[1], f[2], f[3] = c, R, slope
            else:
                dv = tuple(c[i] - f[1][i] for i in range(3))
                d = _norm(dv) * 1.00001
                if not (f[2] < INF) or not (R < INF):
                    f[2] = INF
                elif d + R <= f[2]:
                    pass                          # already inside
                elif d + f[2] <= R:
                    f[1], f[2] = c, R             # swallows what was folded so far
                else:
                    Rn = 0.5 * ((d + f[2]) + R)
                    tt = (Rn - f[2]) / d
                    f[1] = tuple(f[1][i] + tt * dv[i] for i in range(3))
                    f[2] = Rn * 1.00001 + 1e-6 * _l1(f[1])
                f[3] = min(f[3], slope)
            f[4] += 1
        elif op in (OP_UNION_END, OP_SMOOTH_END):
            _, c, R, slope, n = stack.pop()
            Ru, uslope = INF, 1.0                 # min / -lse of the children's upper bounds would need a sphere per child
            if op == OP_SMOOTH_END:               # -lse(-k d) / k >= min d - log(n) / k  for 0 < k < inf
                k = P[off]
                R = R + math.log(n) / k if 0.0 < k < INF else INF
        elif op in (OP_CULL_MIN, OP_CULL_LSE):
            pass                                  # no effect on the bound
        else:
            raise ValueError(f"bound_ref.bound: opcode {op} at instruction {pc} is not a built-in node")
    if overflow or poisoned or not (R == R) or not (slope > 0.5):
        R = INF
    if overflow or poisoned or not (Ru == Ru) or not (uslope >= 1.0) or not (uslope < 8.0):
        Ru = INF
    return c, R, slope, Ru, uslope


def _margined(c, R, Ru):
    c1 = _l1(c)
    Kl = ((R * 1.0001 + 1e-4) + 1e-5 * c1) * 1.000001
    Ku = ((Ru * 1.0001 + 1e-4) + 1e-5 * c1) * 1.000001
    return (Kl if Kl < INF else NAN), (Ku if Ku < INF else INF)


def cull_min_site(program_rows, params_f64, pc):
    """The 5 floats ``{cx, cy, cz, K, slope - 2e-4}`` that derive_constants stores at aux0 of the RM_OP_CULL_MIN at ``pc``:
    the bound of its child ``pc + 1 .. pc + (aux1 >> 8)`` (the child without its FOLD) with
    ``K = (1.0001 R + 1e-4 + 1e-5 |c|_1) 1.000001``; a NaN K stands for "no bound"."""
    row = program_rows[pc]
    if int(row[0]) != OP_CULL_MIN:
        raise ValueError(f"instruction {pc} is no CULL_MIN")
    c, R, slope, Ru, _ = bound(program_rows, params_f64, pc + 1, pc + (int(row[3]) >> 8))
    return [c[0], c[1], c[2], _margined(c, R, Ru)[0], slope - 2e-4]


def smooth_children(program_rows, pc):
    """Instruction ranges ``(begin, end)`` of the children of the smooth union that begins at ``pc``, found as the kernels
    find them: between the FOLD_LSEs of the union's own level, a CULL_LSE in front skipped."""
    n = int(program_rows[pc][3]) & 255
    out, q = [], pc + 1
    for _ in range(n):
        if int(program_rows[q][0]) == OP_CULL_LSE:
            q += 1
        end, depth = q, 0
        while True:
            op = int(program_rows[end][0])
            if op in (OP_UNION_BEGIN, OP_SMOOTH_BEGIN):
                depth += 1
            elif op in (OP_UNION_END, OP_SMOOTH_END):
                depth -= 1
            elif op == OP_FOLD_LSE and depth == 0:
                break
            end += 1
        out.append((q, end))
        q = end + 1
    return out


def smooth_table(program_rows, params_f64, pc):
    """The rows ``{cx, cy, cz, slope_lb, K_lb, slope_ub, K_ub, 0}`` of the bound table of the RM_OP_SMOOTH_BEGIN at ``pc``
    (stored at its aux0, one row per child in slot order); [] when the instruction carries no table.  A NaN K_lb and an
    infinite K_ub stand for "no bound"."""
    row = program_rows[pc]
    if int(row[0]) != OP_SMOOTH_BEGIN:
        raise ValueError(f"instruction {pc} is no SMOOTH_BEGIN")
    if int(row[2]) <= 0:
        return []
    rows = []
    for begin, end in smooth_children(program_rows, pc):
        c, R, slope, Ru, uslope = bound(program_rows, params_f64, begin, end)
        Kl, Ku = _margined(c, R, Ru)
        rows.append([c[0], c[1], c[2], slope - 2e-4, Kl, uslope + 2e-4, Ku, 0.0])
    return rows
