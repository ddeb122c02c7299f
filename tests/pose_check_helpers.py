"""For the pose-check tests (evaluation.pose_checks on the host, cbd_pose_checks on the GPU): a brute-force restatement of the four distance
checks in plain Python loops over pairs (Python floats are fp64; nothing here calls the code under test), and generators of raw-table
cases -- no molecule is needed.

Every coordinate and bound is a multiple of 1/8 A and every radius a multiple of 1/4, so squared distances, sums of radii and the
deliberate ties are exact in fp64.  Margins are true by construction and asserted on the brute force before any result is looked at:
  - bond and 1-3 bounds are ODD multiples of 1/8: with tolerance 0.25 their thresholds are 3 odd / 32 and 5 odd / 32, a distance
    sqrt(m) / 8 that is rational is q / 8, and 3 odd = 4 q or 5 odd = 4 q has no solution; an irrational one stays 1 / (32 sqrt(m)) of
    sqrt(m) away, relatively more than 3e-5 for the distances (below 4 A) that come near such a bound;
  - ligand radii are odd multiples of 1/4 and receptor radii multiples of 1/2: with rec_scale 0.75 the threshold is 3 odd / 16, never q / 8;
  - the clash tolerance 0.30 is not an fp32 number: (1 - fp32(0.30)) lower is no multiple of anything on the grid.
`assert_margins` checks what these arguments promise: no pair within a relative 1e-5 of one of its thresholds, and -- outside the tie
cases -- the two smallest receptor ratios of a pose more than a relative 1e-6 apart."""
import math

import numpy as np

THRESHOLDS = dict(bond_tol=0.25, angle_tol=0.25, clash_tol=0.30, rec_scale=0.75)
FLOATS = ("bond_lo", "bond_hi", "angle_lo", "angle_hi", "clash_ratio", "rec_ratio", "rec_dist")
INTS = ("n_bad_bond", "n_bad_angle", "n_internal_clash", "n_rec_clash", "rec_lig_atom", "rec_atom", "flags")
NAN, INF = float("nan"), float("inf")


def brute_checks(ligand_pos, tables, receptor, bond_tol=0.25, angle_tol=0.25, clash_tol=0.30, rec_scale=0.75):
    """The definition, pair by pair.  `tables` = (lower, upper, kind, radius) with the first three possibly None; `receptor` = (pos,
    radius) or None.  -> (dict name -> array [P]: FLOATS as float32, INTS as int32, valid bool; margin: the smallest relative distance of
    any pair from one of its thresholds; gap: the smallest relative difference between the two smallest receptor ratios of a pose)."""
    tb, ta, tc, rs = (float(np.float32(v)) for v in (bond_tol, angle_tol, clash_tol, rec_scale))
    lower, upper, kind, radius = tables
    lp = np.asarray(ligand_pos, dtype=np.float32)
    P, N = lp.shape[:2]
    has_tab = lower is not None
    has_rec = receptor is not None and len(receptor[0]) > 0
    radius = [float(np.float32(r)) for r in radius]
    static = (0 if has_tab else 16) | (0 if has_rec else 32)
    pairs = []
    if has_tab:
        for i in range(N):
            for j in range(i + 1, N):
                lo, up, kd = float(np.float32(lower[i][j])), float(np.float32(upper[i][j])), int(kind[i][j])
                if not (math.isfinite(lo) and math.isfinite(up) and lo > 0 and up >= lo and 0 <= kd <= 2):
                    static |= 128
                pairs.append((i, j, lo, up, kd))
    rec = []
    if has_rec:
        for a in range(len(receptor[0])):
            q = [float(np.float32(v)) for v in receptor[0][a]] + [float(np.float32(receptor[1][a]))]
            if not all(math.isfinite(v) for v in q[:3]):
                static |= 64
            if not (math.isfinite(q[3]) and q[3] > 0):
                static |= 128
            rec.append(q)
        if not all(math.isfinite(r) and r > 0 for r in radius):
            static |= 128
    out = {k: [] for k in FLOATS + INTS}
    margin, gap = INF, INF

    def near(d, threshold):
        return abs(d - threshold) / threshold

    for p in range(P):
        x = lp[p].astype(np.float64).tolist()
        flags = static | (0 if all(math.isfinite(v) for atom in x for v in atom) else 64)
        row = {k: NAN for k in FLOATS}
        row.update({k: -1 for k in INTS})
        if not flags & (64 | 128):
            if has_tab:
                lo_min, hi_max, count = [INF, INF, INF], [-INF, -INF, -INF], [0, 0, 0]
                for i, j, lo, up, kd in pairs:
                    dx, dy, dz = x[i][0] - x[j][0], x[i][1] - x[j][1], x[i][2] - x[j][2]
                    d = math.sqrt(dx * dx + dy * dy + dz * dz)
                    tol = (tc, tb, ta)[kd]
                    bad = d < (1.0 - tol) * lo
                    margin = min(margin, near(d, (1.0 - tol) * lo))
                    if kd:
                        bad = bad or d > (1.0 + tol) * up
                        margin = min(margin, near(d, (1.0 + tol) * up))
                    count[kd] += 1 if bad else 0
                    lo_min[kd], hi_max[kd] = min(lo_min[kd], d / lo), max(hi_max[kd], d / up)
                row.update(bond_lo=lo_min[1], bond_hi=hi_max[1], angle_lo=lo_min[2], angle_hi=hi_max[2], clash_ratio=lo_min[0],
                           n_bad_bond=count[1], n_bad_angle=count[2], n_internal_clash=count[0])
                flags |= (1 if count[1] else 0) | (2 if count[2] else 0) | (4 if count[0] else 0)
            if has_rec:
                best, second, at, closest, count = INF, INF, (-1, -1), INF, 0
                for i in range(N):
                    xi, yi, zi = x[i]
                    ri = radius[i]
                    for a, (qx, qy, qz, qr) in enumerate(rec):
                        dx, dy, dz = xi - qx, yi - qy, zi - qz
                        d = math.sqrt(dx * dx + dy * dy + dz * dz)
                        ratio = d / (ri + qr)
                        if ratio < rs:
                            count += 1
                        if ratio < rs * 1.1 and ratio > rs * 0.9:
                            margin = min(margin, near(ratio, rs))
                        if d < closest:
                            closest = d
                        if ratio < best:          # strictly: the first of equal ratios in (ligand atom, receptor atom) order stays
                            best, second, at = ratio, best, (i, a)
                        elif ratio < second:
                            second = ratio
                if second < INF:
                    gap = min(gap, (second - best) / best if best > 0 else INF)
                row.update(rec_ratio=best, rec_dist=closest, n_rec_clash=count, rec_lig_atom=at[0], rec_atom=at[1])
                flags |= 8 if count else 0
        row["flags"] = flags
        for k in FLOATS + INTS:
            out[k].append(row[k])
    res = {k: np.asarray(out[k], dtype=np.float32) for k in FLOATS}
    res.update({k: np.asarray(out[k], dtype=np.int32) for k in INTS})
    res["valid"] = (res["flags"] & (1 | 2 | 4 | 8 | 64 | 128)) == 0
    return res, margin, gap


def assert_margins(case, margin, gap):
    assert margin > 1e-5, (case["name"], "a pair within 1e-5 of a threshold", margin)
    if not case["tie"]:
        assert gap > 1e-6, (case["name"], "the two smallest receptor ratios are too close", gap)
    else:
        assert gap == 0.0, (case["name"], "the planted tie is not exact", gap)


def assert_same(got, want, label=""):
    """`got`: a PoseChecks (or anything with the fields as attributes); `want`: brute_checks' dict.  Counts, flags and atoms exactly; floats
    within ONE fp32 step (both sides evaluate the same fp64 expression on the same fp32 inputs to within a few 2^-53 and round once; fused
    multiply-adds may differ between them), NaN where NaN, the same infinity where infinite."""
    for k in INTS:
        g = np.asarray(getattr(got, k))
        assert g.dtype == np.int32 and np.array_equal(g, want[k]), (label, k, g.tolist(), want[k].tolist())
    assert np.array_equal(np.asarray(got.valid, dtype=bool), want["valid"]), (label, "valid")
    for k in FLOATS:
        g, w = np.asarray(getattr(got, k)), want[k]
        assert g.dtype == np.float32 and g.shape == w.shape, (label, k)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (label, k, g.tolist(), w.tolist())
        fin = np.isfinite(w)
        assert np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), (label, k, g.tolist(), w.tolist())
        steps = np.abs(g[fin].view(np.int32).astype(np.int64) - w[fin].view(np.int32).astype(np.int64))
        assert np.isfinite(g[fin]).all() and (steps.max(initial=0) <= 1), (label, k, g.tolist(), w.tolist())


def bitwise_equal(a, b):
    return all(np.array_equal(np.asarray(getattr(a, k)).view(np.int32), np.asarray(getattr(b, k)).view(np.int32)) for k in FLOATS + INTS)


# ---- generators ------------------------------------------------------------------------------------------------------------------------

def grid_points(rng, n, half_width):
    """n DISTINCT points with coordinates that are multiples of 1/8 in [-half_width, half_width)"""
    side = int(round(16 * half_width))
    assert side ** 3 >= 4 * n
    cells = rng.choice(side ** 3, size=n, replace=False)
    return (np.stack([cells % side, cells // side % side, cells // side ** 2], axis=1) / 8.0 - half_width).astype(np.float32)


def chain_tables(rng, n):
    """raw tables of a chain of n atoms: kind 1 for (i, i + 1), 2 for (i, i + 2), else 0; bond and 1-3 bounds ODD multiples of 1/8 (lower
    1.125 .. 1.875 / 2.125 .. 2.875, upper 0.25 .. 0.75 above), the others any multiple of 1/8 in 2.5 .. 4 with upper = 50; radii odd
    multiples of 1/4 in 1.25 .. 2.25"""
    kind = np.zeros((n, n), dtype=np.uint8)
    lower = np.zeros((n, n), dtype=np.float32)
    upper = np.zeros((n, n), dtype=np.float32)
    for i in range(n):
        for j in range(i + 1, n):
            k = 1 if j == i + 1 else 2 if j == i + 2 else 0
            if k:
                lo = (9 + 2 * int(rng.integers(4)) + 8 * (k - 1)) / 8.0
                up = lo + 2 * int(rng.integers(1, 4)) / 8.0
            else:
                lo, up = (20 + int(rng.integers(13))) / 8.0, 50.0
            kind[i, j] = kind[j, i] = k
            lower[i, j] = lower[j, i] = lo
            upper[i, j] = upper[j, i] = up
    radius = ((5 + 2 * rng.integers(3, size=n)) / 4.0).astype(np.float32)
    return lower, upper, kind, radius


def chain_poses(rng, n, p):
    """p poses of a chain of n atoms on the grid: a self-avoiding walk with steps of (1, 1, 0.5)-like vectors (1.5 A), plus a pose-wide
    shift; far from physical, which is the point: every count gets exercised"""
    steps = np.asarray([[1, 1, 0.5], [1, -1, 0.5], [-1, 1, 0.5], [1, 0.5, 1], [0.5, 1, -1], [1, 0.5, -1], [-1, 0.5, 1], [0.5, -1, 1]])
    poses = []
    for _ in range(p):
        walk = np.cumsum(steps[rng.integers(len(steps), size=n)] * np.where(rng.random((n, 1)) < 0.15, 2.0, 1.0), axis=0)
        walk = walk - np.round(walk.mean(axis=0) * 8) / 8
        poses.append(np.mod(walk + 8.0, 16.0) - 8.0 if n > 64 else walk)          # a long chain is folded back into a 16 A box
    return np.stack(poses).astype(np.float32)


def receptor_around(rng, lp, radius, a, hole=3.5, half_width=14.0):
    """`a` receptor atoms on the grid, none within `hole` of any ligand atom of any pose except ONE planted atom that is the unique closest in
    ratio for every pose -- chosen from candidates by the gap it leaves; radii multiples of 1/2 in 1.5 .. 2.0"""
    if a == 0:
        return np.zeros((0, 3), dtype=np.float32), np.zeros(0, dtype=np.float32)
    atoms = lp.reshape(-1, 3).astype(np.float64)
    pts = grid_points(rng, 6 * a + 64, half_width)
    far = pts[(np.linalg.norm(pts[:, None].astype(np.float64) - atoms[None], axis=2).min(axis=1) >= hole)][:max(a - 1, 0)]
    assert len(far) == a - 1, "not enough room for the receptor"
    rad = (rng.integers(3, 5, size=a) / 2.0).astype(np.float32)
    slot = int(rng.integers(a))
    for cand in (atoms[rng.integers(len(atoms), size=400)] + rng.integers(-20, 21, size=(400, 3)) / 8.0).astype(np.float32):
        rec = np.insert(far, slot, cand, axis=0)
        d = np.linalg.norm(lp[:, :, None].astype(np.float64) - rec[None, None].astype(np.float64), axis=3)
        ratio = np.sort((d / (radius.astype(np.float64)[None, :, None] + rad.astype(np.float64)[None, None])).reshape(len(lp), -1), axis=1)
        if ratio.shape[1] == 1 or ((ratio[:, 1] - ratio[:, 0]) > 1e-3 * ratio[:, 0]).all() and (ratio[:, 0] > 0).all():
            return rec.astype(np.float32), rad
    raise AssertionError("no receptor atom leaves a unique closest pair")


def random_case(name, seed, n, a, p, tables=True):
    rng = np.random.default_rng(seed)
    lower, upper, kind, radius = chain_tables(rng, n)
    lp = chain_poses(rng, n, p)
    rec = receptor_around(rng, lp, radius, a)
    return dict(name=name, lp=lp, tables=(lower, upper, kind, radius) if tables else (None, None, None, radius),
                receptor=rec if a else None, tie=False)


def line_case(name, bond=None, angle=None, other=None, rec_atom=None):
    """four atoms on a line, 1.5 A apart (bonds 1.5, 1-3 pairs 3.0, the 1-4 pair 4.5), tables that the pose satisfies; each keyword
    replaces one table entry or adds one receptor atom so that exactly ONE check fails"""
    n = 4
    lp = np.zeros((1, n, 3), dtype=np.float32)
    lp[0, :, 0] = 1.5 * np.arange(n)
    kind = np.zeros((n, n), dtype=np.uint8)
    lower, upper = np.full((n, n), 3.5, dtype=np.float32), np.full((n, n), 50.0, dtype=np.float32)
    for i in range(n):
        for j in range(n):
            if abs(i - j) == 1:
                kind[i, j], lower[i, j], upper[i, j] = 1, 1.375, 1.625
            if abs(i - j) == 2:
                kind[i, j], lower[i, j], upper[i, j] = 2, 2.625, 3.125
    for (i, j, lo, up) in [e for e in (bond, angle, other) if e is not None]:
        lower[i, j] = lower[j, i] = lo
        upper[i, j] = upper[j, i] = up
    radius = np.full(n, 1.75, dtype=np.float32)
    rec = (np.asarray([[0.0, 6.0, 0.0], [4.5, -6.5, 0.0]] + ([rec_atom] if rec_atom is not None else []), dtype=np.float32),
           np.asarray([1.5, 2.0] + ([1.5] if rec_atom is not None else []), dtype=np.float32))
    return dict(name=name, lp=lp, tables=(lower, upper, kind, radius), receptor=rec, tie=False)


def tie_case(name, n, a, lig_pair=None, rec_pair=None, cross=None, seed=0):
    """A ligand far from everything except planted receptor atoms.  `rec_pair` = (a1, a2): two receptor atoms mirrored about ligand atom 0
    (equal radii): the smaller receptor atom must win.  `lig_pair` = (i1, i2): two ligand atoms (equal radii) mirrored about one receptor
    atom: the smaller ligand atom must win.  `cross` = (i1, a1, i2, a2), i1 < i2 and a1 > a2: two separate pairs with the same geometry:
    the smaller LIGAND atom wins although its receptor atom is the larger."""
    rng = np.random.default_rng(seed)
    radius = np.full(n, 1.75, dtype=np.float32)
    lp = np.zeros((1, n, 3), dtype=np.float32)
    lp[0, :, 0] = 2.0 * np.arange(n) - 4.0          # a line along x, 2 A apart, in the plane y = z = 0
    rec = np.zeros((a, 3), dtype=np.float32)
    rec[:, 0] = ((np.arange(a) % 40) * 2.0 - 20.0)
    rec[:, 1] = 12.0 + 2.0 * (np.arange(a) // 40)   # a sheet far above the line
    rec[:, 2] = rng.integers(-8, 8, size=a) / 8.0
    rad = np.full(a, 1.5, dtype=np.float32)
    if rec_pair is not None:
        a1, a2 = rec_pair
        rec[a1] = lp[0, 0] + np.float32([0.0, 2.0, 1.5])
        rec[a2] = lp[0, 0] - np.float32([0.0, 2.0, 1.5])
    if lig_pair is not None:
        i1, i2 = lig_pair
        centre = np.float32([-9.0, -6.0, 0.0])
        lp[0, i1], lp[0, i2] = centre + np.float32([0.0, 2.0, 1.5]), centre - np.float32([0.0, 2.0, 1.5])
        rec[0] = centre
    if cross is not None:
        i1, a1, i2, a2 = cross
        rec[a1] = lp[0, i1] + np.float32([0.0, 2.0, 1.5])
        rec[a2] = lp[0, i2] + np.float32([0.0, -2.0, -1.5])
    return dict(name=name, lp=lp, tables=(None, None, None, radius), receptor=(rec, rad), tie=True)


def gpu_cases():
    """The ragged launch of tests/test_gpu_pose_checks.py (the CPU test runs the same cases through the host function): N in {1, 2, 63, 64,
    65, 256}, A in {0, 1, 255, 256, 257, 1000}, P in {1, 3}; one receptor object shared by two complexes; one complex without tables; one
    pose with a NaN coordinate; one table with a non-positive lower entry; the tie cases across a thread's own stride (256 apart), across
    waves (64 apart) and across lanes (1 apart); the four single-failure cases."""
    cases = [random_case("n1_a1000", 11, 1, 1000, 1), random_case("n2_a257", 12, 2, 257, 3), random_case("n63_a256", 13, 63, 256, 1),
             random_case("n64_a255", 14, 64, 255, 3), random_case("n65_a1", 15, 65, 1, 1), random_case("n256_a0", 16, 256, 0, 3),
             random_case("n256_a1000", 17, 256, 1000, 1), random_case("no_tables_n20_a300", 18, 20, 300, 3, tables=False)]
    shared = random_case("shared_a", 19, 30, 500, 3)
    other = random_case("shared_b", 20, 12, 0, 1)
    # the second complex sits inside the first one's receptor (the same array objects); moved as a whole until its closest pair is unique
    for shift in range(40):
        other["lp"] = (random_case("shared_b", 20, 12, 0, 1)["lp"] + np.float32([0.125 * shift, 0.0, 0.25 * shift])).astype(np.float32)
        other["receptor"] = shared["receptor"]
        if brute_checks(other["lp"], other["tables"], other["receptor"])[2] > 1e-3:
            break
    cases += [shared, other]
    nan_pose = random_case("nan_pose", 21, 9, 40, 3)
    nan_pose["lp"][1, 4, 2] = np.nan
    bad_table = random_case("bad_lower", 22, 9, 40, 3)
    bad_table["tables"][0][2, 5] = bad_table["tables"][0][5, 2] = 0.0
    cases += [nan_pose, bad_table]
    cases += [tie_case("tie_rec_256_apart", 5, 600, rec_pair=(300, 44), seed=1), tie_case("tie_rec_64_apart", 5, 600, rec_pair=(71, 135), seed=2),
              tie_case("tie_rec_1_apart", 5, 600, rec_pair=(200, 199), seed=3), tie_case("tie_lig_pair", 70, 300, lig_pair=(66, 2), seed=4),
              tie_case("tie_cross_lanes", 8, 600, cross=(1, 300, 6, 45), seed=5), tie_case("tie_cross_one_thread", 8, 600, cross=(1, 301, 6, 45), seed=6)]
    cases += [line_case("all_pass"), line_case("bad_bond_only", bond=(0, 1, 2.625, 2.875)), line_case("bad_angle_only", angle=(1, 3, 1.625, 2.125)),
              line_case("internal_clash_only", other=(0, 3, 7.0, 50.0)), line_case("rec_clash_only", rec_atom=[1.5, 2.0, 1.0])]
    return cases


def expected(cases):
    """brute force of every case, margins asserted: -> list of dicts (computed once; share it and leave it unchanged)"""
    out = []
    for case in cases:
        want, margin, gap = brute_checks(case["lp"], case["tables"], case["receptor"])
        assert_margins(case, margin, gap)
        out.append(want)
    return out
