"""Shared by tests/test_conformer_kernel_refs.py (CPU) and tests/test_gpu_conformer_kernels.py (GPU): the cases, the float64 references and
the a-priori fp32 bounds that hold csrc/conformer_embed.hip and csrc/torsion_match.hip to their definitions.  Nothing here calls a kernel.

Every numeric assertion is per element, |got - ref64| <= n * u * abs (+ what is said below), u = 2^-24.  `abs` is the same expression on
magnitudes (a cross-product component b_y c_z - b_z c_y becomes |b_y||c_z| + |b_z||c_y|), n is the number of fp32 roundings behind the
element, counted from the kernel source with every operation as one rounding (a contracted fma makes fewer, never more) and a value that
enters a term k times counted k times.  n is stated HERE, never fitted to a measured error.  Division and sqrtf are correctly rounded
(hipcc's default).  Library functions are allowed the error of the accuracy class the device library implements: cbrtf 2 ulp (the figure
HIP's math-API table gives, which is OpenCL's limit too), sinf / cosf 4 ulp, atan2f 6 ulp (OpenCL's limits; HIP's table lists no larger
ones).  1 ulp <= 2 u |x|.

1. Embedding (embed_conformers_kernel).  The start is restated exactly: unit = (mix64(key ^ (atom << 8 | dim)) >> 40) 2^-24 - 0.5 is exact
   in fp32; x = fl(unit * box), box = fl(3 cbrtf(N)).  START_ULPS = 6: cbrtf 2 ulp <= 4 u, the product by 3, the product by the unit.
   The GPU test also finds THE fp32 box (one of the values 3 * (cbrt(N) +- 2 ulp) rounds to) that reproduces every returned coordinate
   bitwise; the unobservable fourth coordinate is that box times the restated unit.
   With d = x_i - x_j (1 rounding per component), d2 = sum of four squares (3 per square, 2 more for the sums that are not + 0: 5), u2 = u u
   and l2 = l l (1 each):
     upper branch   t = d2 / u2 - 1        N_T_UP = 8    on d2 / u2 + 1       (5 + 1, the division 1, the subtraction 1)
                    e = 0.5 t t            N_E_UP = 17   on 0.5 abs_t^2       (t twice, the product)
                    coef dx = 4 t / u2 dx  N_G_UP = 12   on 4 abs_t / u2 |dx| (t 8, u2 1, the division 1, dx 1, the product 1)
     lower branch   den = l2 + d2 (6);  t = 2 l2 / den - 1      N_T_LO = 9  on 2 l2 / den + 1   (l2 1, den 6, division 1, subtraction 1)
                    e                      N_E_LO = 19
                    -8 t l2 / (den den) dx N_G_LO = 27   (t 9, l2 1 and its product 1, den den 13, the division 1, dx 1, the product 1)
     volume         a, b, c = p1 - p0, ... (1 each);  b x c component N_X = 4;  V = a . (b x c): N_V = 8 (a 1, b x c 4, product 1, two sums)
                    r = sg V - (edge +- m), m = fl(0.1f min(|lo|, |hi|)):  N_R = 11 on abs_V + |edge| + m   (V 8, m 1, edge +- m 1, the
                    subtraction 1);  planar: r = V, N_R = 8.   e = w r r: 2 N_R + 2.   f = 2 w r sg: N_R + 1 on 2 w abs_r.
                    gradient of role i1 / i2 / i3: f times a cross-product component: N_F + N_X + 1;  of i0: three of them summed: N_F + 6 + 1.
     w4 term        e = w4 w w: 2;  gradient 2 w4 w: 1 (the product by 2 w4 is one rounding at most).
   Sums.  A term that is an exact zero rounds nothing.  The gradient of atom i passes through at most (non-zero terms of i) + S additions
   (its slices' own chains, then the S partial sums in order); the energy through at most max_i (non-zero terms thread (i, .) adds) + 9
   (6 butterfly steps, 3 waves).  So  bound = u * sum_terms (n_term + n_sum) abs_term.
   One FIRE step from v = 0:  v = dt F (1), the mixing v = (1 - a) v + k F with k = a sqrt(vv) / sqrt(ff) returns dt F (1 + eta):
   vv, ff are sums of 4 N squares through 3 + 6 + 3 additions (13 u each, halved by the root, + 1 for the root: 7.5 u, + 1 u from v's own
   rounding), the division and the product by a 2 more: k = a dt (1 + 19 u);  (1 - a) 1, its product 1, v 1: eta <= 0.9 * 3 + 0.1 * 19 + 1 < 6.
   dx = dt v: N_STEP = 7 for an unclamped atom (sc = 1 exactly).  A clamped atom: |dx| (4 products, 3 sums, the root: 3.5), 0.25 / |dx| 1,
   dx sc 1: N_STEP_CLAMPED = 13; the error of F enters through the direction: 0.25 (bF_k / |F| + |F_k| sum_m |F_m| bF_m / |F|^3).
   The final x += dx sc adds half an ulp of the result, <= u |x|.  An atom whose force and force bound are exactly zero must not move.
   dt = fl(0.02), a = fl(0.1), w4 = fl(0.01), w_v = fl(0.2) and fl(0.1) of the narrowing are the kernel's fp32 constants, used as such.
   Only xyz is returned: in the 4-D stages the fourth component of the force (the w4 term's own gradient among it) is seen only through
   the clamp's norm.
   Branch decisions: every case asserts (on the CPU from the restated start, on the GPU from the returned one) that every d2 is at least
   MARGIN = 2^-16 (relative) from u2 and l2 (rounding moves them by 6 u and 1 u), every sg V from lo + m and hi - m and every V of an
   |V| constraint from 0 by MARGIN of the magnitude expression (11 u), every |dx| by CLAMP_MARGIN = 2^-10 from 0.25 (and the bound of |dx|
   is under a quarter of its own distance from 0.25), and the largest force component a factor 2 from CE_FTOL.

2. Matching (match_score_kernel).  First order in u, per rotation r and atom a of its rotating side, d = |x_a - x_v| from the fp64 replay:
     angle      e_phi (dihedral4 on magnitudes: b 1, n 4, n1 x n2 10, . b2 14, |b2| 3.5, y 18.5, x 11, atan2f 6 ulp of pi)
                + u (11 |delta| + 36): theta - phi 1, the axis times the angle and its norm again 10 |delta|, sinf and cosf 2 * 8 sqrt2 ~ 24,
                sin / ang and the three products 12                                                               -> times d
     tilt       u * 13 (unit axis 6.5 per component, times sqrt3, the products by k) + what the bond's own atoms carry: their
                per-atom rounding so far / |u - v| and 31 u per earlier rotation that moved the bond (the matrix's error)  -> times 2 d
     matrix     18 u per entry (two_s 5 -> 10, the entry 8), times |d|_1 <= sqrt3 d: C_COMMON = 31
     apply      dx 1, three products and sums, + v: 4 sqrt3 ~ 7 on d, and u |x'|: C_OWN = 7
   Rotations are rigid motions of subsets, so an error made once is carried isometrically and does not compound in first order; the
   bound of atom a is the sum over the rotations that move it.  The RMSD is 1-Lipschitz in the rms displacement E; the fp32 centring of
   probe and target adds u sqrt3 (|a| + |b|)_max as noise and the two centroids' own errors only in second order, (eps_p + eps_t)^2 in r^2
   with eps = (slots + 7) u sqrt3 max|x|.  The fp64 Horn part: 256 * 2^-53 (a2 + b2) / Nl in r^2 (ten summation steps, Jacobi's sweeps), and as much for the reference's own SVD.
   Everything is asserted on r^2, which also covers a target that is reached:  |got^2 - ref^2| <= 2 ref E + E^2 + (eps_p + eps_t)^2
   + 4 u (ref + E)^2 + the fp64 part.

3. The evolution's start: v = -pi + 2 pi ((perm + unit) / P) in numpy float32.  The device may contract 2 pi q - pi into one fma:
   DE_ULPS = 2 ulps of pi (the product's rounding is at most 1 ulp of pi, each final rounding half)."""
import functools
import math

import numpy as np

U = 2.0 ** -24
MARGIN = 2.0 ** -16
CLAMP_MARGIN = 2.0 ** -10
START_ULPS = 6
CBRT_ULPS = 2
FTOL, MAX_STEP = float(np.float32(1e-4)), 0.25
DT0, ALPHA0 = float(np.float32(0.02)), float(np.float32(0.1))
W4_WEAK, WV_STRONG, NARROW = float(np.float32(0.01)), float(np.float32(0.2)), float(np.float32(0.1))
KIND_VOLUME, KIND_ABS, KIND_PLANAR = 0, 1, 2
# (iters, w4, wv, wp, the start keeps its fourth coordinate)
STAGES = {"3d": ((0, 0, 1), 0.0, 1.0, 1.0, False), "4d_weak": ((1, 0, 0), W4_WEAK, 1.0, 0.0, True), "4d_strong": ((0, 1, 0), 1.0, WV_STRONG, 0.0, True)}
N_T_UP, N_E_UP, N_G_UP = 8, 17, 12
N_T_LO, N_E_LO, N_G_LO = 9, 19, 27
N_X, N_V, N_R, N_R_PLANAR = 4, 8, 11, 8
N_STEP, N_STEP_CLAMPED = 7, 13
M64 = (1 << 64) - 1


def mix64(z):
    """splitmix64 finaliser in Python integers"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def ratio(err, bound):
    """largest err / bound with 0 / 0 = 0: an element whose bound is zero must be exact"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    out = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    return float(out.max()) if out.size else 0.0


# ======================================================================================================== 1. embedding: the start
def embed_units(seed, mol_id, conf_id, n):
    """[n, 4] float64: the exact values of the kernel's draws in [-0.5, 0.5)"""
    key_m = mix64(mix64(seed & M64) ^ (mol_id & 0xffffffff))
    key = mix64(key_m ^ ((conf_id & 0xffffffff) << 32))
    return np.array([[(mix64(key ^ ((a << 8) | d)) >> 40) / 16777216.0 - 0.5 for d in range(4)] for a in range(n)])


def box_candidates(n):
    """the fp32 values fl(3 c) for every fp32 c within CBRT_ULPS ulps of cbrt(n)"""
    true = float(n) ** (1.0 / 3.0)
    if round(true) ** 3 == n:              # a perfect cube: pow may be an ulp of float64 off
        true = float(round(true))
    c = np.float32(true)
    cands = [c]
    for _ in range(CBRT_ULPS + 1):
        cands = [np.nextafter(cands[0], np.float32(0)), *cands, np.nextafter(cands[-1], np.float32(np.inf))]
    ulp = float(np.spacing(np.float32(true)))
    return sorted({float(np.float32(3.0) * x) for x in cands if abs(float(x) - true) <= CBRT_ULPS * ulp})


def start_from_box(units, box):
    """[n, 4] float64 of the fp32 start for a given fp32 box"""
    return (units.astype(np.float32) * np.float32(box)).astype(np.float64)


def restated_start(seed, mol_id, conf_id, n):
    """the start with the correctly rounded cube root: what the cases are built from"""
    units = embed_units(seed, mol_id, conf_id, n)
    true = float(n) ** (1.0 / 3.0)
    return start_from_box(units, float(np.float32(3.0) * np.float32(true)))


def start_ulps(pos32, units, n):
    """largest distance, in fp32 ulps, of returned coordinates [n, 3] from the exact units * 3 n^(1/3)"""
    exact = units[:, :3] * (3.0 * float(n) ** (1.0 / 3.0))
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    return float((np.abs(np.asarray(pos32, dtype=np.float64) - exact) / ulp).max())


def infer_start(pos32, units, n):
    """the [n, 4] start whose xyz is bitwise pos32, from the one candidate box that gives it; None when there is none.  Candidates that
    agree on every xyz must agree on every w (else the fourth coordinate is not determined: a test error, not a skip)"""
    pos32 = np.asarray(pos32, dtype=np.float32)
    hits = [start_from_box(units, b) for b in box_candidates(n)]
    hits = [h for h in hits if np.array_equal(h[:, :3].astype(np.float32), pos32)]
    if not hits:
        return None
    assert all(np.array_equal(h, hits[0]) for h in hits), "fourth coordinate not determined by the returned xyz"
    return hits[0]


# ======================================================================================================== 1. embedding: reference
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _cross_abs(a, b):
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)


def embed_eval(x, lower, upper, cons, w4, wv, wp, mut=None):
    """The objective of the header comment at x [N, 4] in float64, its analytic gradient and the a-priori bounds of both.
    lower / upper: the fp32 matrices the kernel reads; cons: idx [nc, 4], lo, hi (fp32 values), kind.
    -> dict E, bE, grad [N, 4], bG [N, 4], margin (smallest relative distance of a branch decision from its edge), counts."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    S = 256 // n
    lo_m, up_m = np.asarray(lower, dtype=np.float64).T, np.asarray(upper, dtype=np.float64).T       # thread i reads element [j][i]
    off = ~np.eye(n, dtype=bool)
    D = x[:, None, :] - x[None, :, :]
    d2 = (D * D).sum(-1)
    u2, l2 = up_m * up_m, lo_m * lo_m
    up_b = (d2 > u2) & (u2 > 0) & off
    lo_b = ~up_b & (d2 < l2) & off
    share = 1.0 if mut == "pair_share_1" else 0.5
    c_up = 2.0 if mut == "upper_coef_2" else 4.0
    su2, sden = np.where(up_b, u2, 1.0), np.where(lo_b, l2 + d2, 1.0)
    t_up, at_up = d2 / su2 - 1.0, d2 / su2 + 1.0
    t_lo, at_lo = 2.0 * l2 / sden - 1.0, 2.0 * l2 / sden + 1.0
    e_pair = np.where(up_b, share * t_up * t_up, 0.0) + np.where(lo_b, share * t_lo * t_lo, 0.0)
    ae_pair = np.where(up_b, 0.5 * at_up * at_up, 0.0) + np.where(lo_b, 0.5 * at_lo * at_lo, 0.0)
    ne_pair = np.where(up_b, N_E_UP, 0) + np.where(lo_b, N_E_LO, 0)
    coef = np.where(up_b, c_up * t_up / su2, 0.0) + np.where(lo_b, -8.0 * t_lo * l2 / (sden * sden), 0.0)
    acoef = np.where(up_b, 4.0 * at_up / su2, 0.0) + np.where(lo_b, 8.0 * at_lo * l2 / (sden * sden), 0.0)
    ncoef = np.where(up_b, N_G_UP, 0) + np.where(lo_b, N_G_LO, 0)
    grad = (coef[:, :, None] * D).sum(1)
    g_nabs = ((ncoef * acoef)[:, :, None] * np.abs(D)).sum(1)            # sum n_term abs_term
    g_abs = (acoef[:, :, None] * np.abs(D)).sum(1)                       # sum abs_term
    nz_g = (up_b | lo_b).sum(1).astype(np.float64)                       # non-zero gradient terms of atom i
    nz_e = (up_b | lo_b).sum(1).astype(np.float64)
    e_rows, e_nabs, e_abs = e_pair.sum(1), (ne_pair * ae_pair).sum(1), ae_pair.sum(1)
    # the fourth dimension's own term
    e_rows = e_rows + w4 * x[:, 3] ** 2
    e_nabs, e_abs = e_nabs + 2 * w4 * x[:, 3] ** 2, e_abs + w4 * x[:, 3] ** 2
    grad[:, 3] += 2.0 * w4 * x[:, 3]
    g_nabs[:, 3] += 1 * 2.0 * w4 * np.abs(x[:, 3])
    g_abs[:, 3] += 2.0 * w4 * np.abs(x[:, 3])
    if w4 != 0:
        nz_g, nz_e = nz_g + 1, nz_e + 1
    with np.errstate(divide="ignore", invalid="ignore"):
        m_pair = min(float(np.where(off, np.abs(d2 - u2) / u2, np.inf).min()) if n > 1 else np.inf,
                     float(np.where(off & (l2 > 0), np.abs(d2 - l2) / np.where(l2 > 0, l2, 1.0), np.inf).min()) if n > 1 else np.inf)
    margin = m_pair
    counts = {"upper": int(up_b.sum()) // 2, "lower": int(lo_b.sum()) // 2, "inside": (int((off & ~up_b & ~lo_b).sum())) // 2}
    idx = np.asarray(cons["idx"], dtype=np.int64).reshape(-1, 4)
    if len(idx):
        kind = np.asarray(cons["kind"], dtype=np.int64)
        clo, chi = np.asarray(cons["lo"], dtype=np.float64), np.asarray(cons["hi"], dtype=np.float64)
        p = x[idx][:, :, :3]
        a, b, c = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]
        bc, ca, ab = _cross(b, c), _cross(c, a), _cross(a, b)
        abc, aca, aab = _cross_abs(b, c), _cross_abs(c, a), _cross_abs(a, b)
        V, aV = (a * bc).sum(1), (np.abs(a) * abc).sum(1)
        planar = kind == KIND_PLANAR
        sg = np.where((kind == KIND_ABS) & (V < 0) & (mut != "sg_ignored"), -1.0, 1.0)
        m = np.where(planar | (mut == "no_narrowing"), 0.0, NARROW * np.minimum(np.abs(clo), np.abs(chi)))
        Ve = sg * V
        under, over = ~planar & (Ve < clo + m), ~planar & ~(Ve < clo + m) & (Ve > chi - m)
        r = np.where(planar, V, np.where(under, Ve - (clo + m), np.where(over, Ve - (chi - m), 0.0)))
        ar = np.where(planar, aV, aV + np.where(under, np.abs(clo), np.abs(chi)) + m)
        nr = np.where(planar, N_R_PLANAR, N_R)
        w = np.where(planar, wv if mut == "planar_wv" else wp, wv)
        live = (2.0 * w * r * sg) != 0
        ec, aec, nec = w * r * r, np.where(live, w * ar * ar, 0.0), 2 * nr + 2
        np.add.at(e_rows, idx[:, 0], ec)
        np.add.at(e_nabs, idx[:, 0], nec * aec)
        np.add.at(e_abs, idx[:, 0], aec)
        np.add.at(nz_e, idx[:, 0], live.astype(np.float64))
        f, af, nf = 2.0 * w * r * sg, np.where(live, 2.0 * w * ar, 0.0), nr + 1
        roles = [(-(bc + ca + ab), abc + aca + aab, 6), (bc, abc, N_X), (ca, aca, N_X), (ab, aab, N_X)]
        for role, (gv, ga, ng) in enumerate(roles):
            sign = -1.0 if mut == f"vol_sign_role{role}" else 1.0
            np.add.at(grad, (idx[:, role, None], np.arange(3)[None, :]), sign * f[:, None] * gv)
            np.add.at(g_nabs, (idx[:, role, None], np.arange(3)[None, :]), ((nf + ng + 1) * af)[:, None] * ga)
            np.add.at(g_abs, (idx[:, role, None], np.arange(3)[None, :]), af[:, None] * ga)
            np.add.at(nz_g, idx[:, role], live.astype(np.float64))
        nonpl = ~planar
        if nonpl.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.minimum(np.abs(Ve - (clo + m)) / (aV + np.abs(clo) + m), np.abs(Ve - (chi - m)) / (aV + np.abs(chi) + m))[nonpl]
            margin = min(margin, float(rel.min()))
        if (kind == KIND_ABS).any():
            margin = min(margin, float((np.abs(V) / aV)[kind == KIND_ABS].min()))
        for k, name in ((KIND_VOLUME, "volume"), (KIND_ABS, "abs")):
            counts[name + "_under"], counts[name + "_over"] = int((under & (kind == k)).sum()), int((over & (kind == k)).sum())
            counts[name + "_inside"] = int((~under & ~over & (kind == k)).sum())
        counts["abs_negative"], counts["planar"] = int(((kind == KIND_ABS) & (V < 0)).sum()), int(planar.sum())
    n_sum_e = float(nz_e.max()) + 9
    bG = U * (g_nabs + (nz_g + S)[:, None] * g_abs)
    return {"E": float(e_rows.sum()), "bE": U * float((e_nabs + n_sum_e * e_abs).sum()), "grad": grad, "bG": bG, "margin": margin, "counts": counts}


def embed_step(x, lower, upper, cons, stage, mut=None):
    """One FIRE step of `stage` from the start x [N, 4] with v = 0.  -> dict delta [N, 3] (= new xyz - old xyz), bound [N, 3], clamped [N],
    moves (False: the largest force component is under CE_FTOL), margin, clamp_margin, ftol_ratio, E (of the stage), counts."""
    _, w4, wv, wp, _ = STAGES[stage]
    ev = embed_eval(x, lower, upper, cons, w4, wv, wp, mut=mut)
    F, bF = -ev["grad"], ev["bG"]
    fm = float(np.abs(F).max())
    fm_b = float(bF.max())
    out = {"margin": ev["margin"], "counts": ev["counts"], "fm": fm, "E": ev["E"]}
    # CE_FTOL: either clearly above, or clearly below (bound included), or exactly zero
    out["ftol_ratio"] = np.inf if (fm == 0 and fm_b == 0) else (fm / FTOL if fm >= FTOL else FTOL / (fm + fm_b))
    if fm < FTOL:
        return dict(out, delta=np.zeros((len(x), 3)), bound=np.zeros((len(x), 3)), clamped=np.zeros(len(x), bool), moves=False, clamp_margin=np.inf)
    dx = DT0 * DT0 * F
    nrm = np.sqrt((dx * dx).sum(1))
    b_nrm = DT0 * DT0 * np.sqrt((bF * bF).sum(1)) + N_STEP_CLAMPED * U * nrm
    clamped = nrm > MAX_STEP
    out["clamp_margin"] = float((np.abs(nrm - MAX_STEP) / MAX_STEP).min())
    out["clamp_bound_ok"] = bool((b_nrm <= np.abs(nrm - MAX_STEP) / 4).all())          # the bound of |dx| cannot cross the clamp
    sc = np.where(clamped, MAX_STEP / np.where(clamped, nrm, 1.0), 1.0)
    delta = dx * sc[:, None]
    fn = np.sqrt((F * F).sum(1))
    fn = np.where(fn > 0, fn, 1.0)
    b_dir = MAX_STEP * (bF / fn[:, None] + np.abs(F) * ((np.abs(F) * bF).sum(1) / fn ** 3)[:, None])
    bound = np.where(clamped[:, None], b_dir + N_STEP_CLAMPED * U * np.abs(delta), DT0 * DT0 * bF + N_STEP * U * np.abs(delta))
    bound = bound + U * (np.abs(x) + np.abs(delta))
    bound = np.where((F == 0) & (bF == 0), 0.0, bound)
    return dict(out, delta=delta[:, :3], bound=bound[:, :3], clamped=clamped, moves=True)


# ======================================================================================================== 1. embedding: the cases
EMBED_SEED = 20240611
EMBED_NS = (1, 2, 4, 5, 64, 65, 85, 86, 100, 128, 129, 255, 256)
# conformer ids that are not 0: chosen on the CPU so that every margin of the case holds (tests/test_conformer_kernel_refs.py re-checks all)
EMBED_CONF_IDS = {'n5_c257': 1, 'n5_c1024': 1, 'n64_c1': 1, 'n86_c1024': 1, 'n100_c3': 1, 'n100_c257': 1, 'n128_c257': 1, 'n129_c0': 1, 'n129_c1': 1,
                  'n255_c257': 5, 'n256_c2': 1}


def _interval(Ve, mode, r):
    """(lo, hi) that puts sg V = Ve at distance r outside the narrowed interval (`over`: above hi - m, `under`: below lo + m) or inside"""
    if mode == "inside":
        return Ve - abs(Ve) - 1.0, Ve + abs(Ve) + 1.0
    if mode == "over":
        T = Ve - r
        return (-2.0 * T / 0.9, T / 0.9) if T > 0 else (3.0 * T / 1.1, T / 1.1)
    T = Ve + r
    return (T / 0.9, -2.0 * T / 0.9) if T < 0 else (T / 1.1, 3.0 * T / 1.1)


def embed_case_list():
    """(id, N, nc, flavour): every N with every nc of {0, 1, S-1, S, S+1, 257, 1024} it admits (a constraint needs four atoms), an
    all-satisfied molecule and one whose only force is under CE_FTOL in the 3-D stage"""
    out = []
    for n in EMBED_NS:
        S = 256 // n
        ncs = sorted({0, 1, S - 1, S, S + 1, 257, 1024} - {-1}) if n >= 4 else [0]
        out += [(f"n{n}_c{nc}", n, nc, "random") for nc in ncs]
    out += [("satisfied_n5_c6", 5, 6, "satisfied"), ("satisfied_n100_c0", 100, 0, "satisfied"), ("below_ftol_n2", 2, 0, "below_ftol")]
    return out


@functools.lru_cache(maxsize=None)
def embed_cases():
    """list of dicts: id, N, nc, mol_id, conf_id, lower, upper (float32 [N, N]), cons, bounds (the triple embed_conformers_batch takes)"""
    return [build_embed_case(mol_id, *spec, EMBED_CONF_IDS.get(spec[0], 0)) for mol_id, spec in enumerate(embed_case_list())]


def build_embed_case(mol_id, cid, n, nc, flavour, conf_id):
    """bounds and constraints drawn around the restated start of (EMBED_SEED, mol_id, conf_id), so that every branch is hit by design"""
    rng = np.random.default_rng([n, nc, len(flavour)])
    x = restated_start(EMBED_SEED, mol_id, conf_id, n)
    d3 = np.sqrt(((x[:, None, :3] - x[None, :, :3]) ** 2).sum(-1))
    d4 = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    quiet = np.zeros(n, bool)
    if flavour == "random" and n >= 3:
        quiet[rng.choice(n, max(1, n // 3), replace=False)] = True
    # one category per pair: 0 inside (in three and in four dimensions), 1 far above the upper bound, 2 a little above, 3 under the
    # lower bound, 4 the one mild violation of a quiet atom (below_ftol: t = 2 MARGIN in three dimensions)
    cat = rng.choice(4, size=(n, n), p=[0.3, 0.25, 0.15, 0.3])
    if n == 2:
        cat[:] = 2
    touch = quiet[:, None] | quiet[None, :]
    cat[touch] = 0
    if flavour == "satisfied":
        cat[:] = 0
    for q in np.nonzero(quiet)[0]:
        partner = int(rng.choice([a for a in range(n) if a != q]))
        cat[min(q, partner), max(q, partner)] = 4
    if flavour == "below_ftol":
        cat[:] = 4
    r1, r2 = rng.uniform(size=(n, n)), rng.uniform(size=(n, n))
    t_mild = np.full((n, n), 2 * MARGIN) if flavour == "below_ftol" else 10 ** (-3 + 1.5 * r1)
    d3s, d4s = np.where(d3 > 0, d3, 1.0), np.where(d4 > 0, d4, 1.0)
    up0, lo0 = d4s * (1.5 + 1.5 * r1), d3s * (0.1 + 0.5 * r2)
    up1 = d3s / (1.5 + 2.5 * r1)
    up2 = d3s / np.sqrt(1.0 + 10 ** (-2 + 1.7 * r1))
    lo3 = d4s * (1.1 + 0.9 * r1)
    up4 = d3s / np.sqrt(1.0 + t_mild)
    up_c = np.choose(cat, [up0, up1, up2, lo3 * (1.1 + 0.4 * r2), up4])
    lo_c = np.choose(cat, [lo0, up1 * (0.2 + 0.7 * r2), up2 * (0.2 + 0.7 * r2), lo3, up4 * 0.5])
    iu = np.triu(np.ones((n, n), bool), 1)
    lower, upper = np.where(iu, lo_c, 0.0), np.where(iu, up_c, 0.0)
    lower, upper = lower + lower.T, upper + upper.T + np.eye(n)
    lower, upper = lower.astype(np.float32), upper.astype(np.float32)
    assert (lower < upper).all() and np.array_equal(lower, lower.T) and np.array_equal(upper, upper.T)
    pool = np.nonzero(~quiet)[0] if (~quiet).sum() >= 4 else np.arange(n)
    idx, clo, chi, kind = [], [], [], []
    for c in range(nc):
        q = rng.choice(pool, 4, replace=False)
        k = KIND_VOLUME + (c % 2) if flavour == "satisfied" else c % 3
        sub = 2 if flavour == "satisfied" else (c // 3) % 4
        p = x[q, :3]
        a, b, cc = p[1] - p[0], p[2] - p[0], p[3] - p[0]
        V = float(np.dot(a, np.cross(b, cc)))
        aV = float((np.abs(a) * _cross_abs(b[None], cc[None])[0]).sum())
        Ve = abs(V) if k == KIND_ABS else V
        if k == KIND_PLANAR:
            lo, hi = 0.0, 0.1
        elif sub == 2:
            lo, hi = _interval(Ve, "inside", 0.0)
        else:
            r = aV * 2.0 ** -12 if sub == 3 else abs(Ve) * rng.uniform(0.05, 0.5) + 0.01
            mode = ("over", "under")[(c // 12) % 2] if sub == 3 else ("over", "under")[sub]
            if k == KIND_ABS and mode == "over":
                r = min(r, 0.9 * Ve)
            lo, hi = _interval(Ve, mode, r)
        idx.append(q); clo.append(lo); chi.append(hi); kind.append(k)
    cons = {"idx": np.asarray(idx, dtype=np.int32).reshape(-1, 4), "lo": np.asarray(clo, dtype=np.float32).astype(np.float64),
            "hi": np.asarray(chi, dtype=np.float32).astype(np.float64), "kind": np.asarray(kind, dtype=np.int32)}
    assert (cons["lo"] < cons["hi"]).all()
    return {"id": cid, "N": n, "nc": nc, "S": 256 // n, "flavour": flavour, "mol_id": mol_id, "conf_id": conf_id, "lower": lower,
            "upper": upper, "cons": cons, "bounds": (lower.astype(np.float64), upper.astype(np.float64), cons)}


def embed_checks(case, x4):
    """every margin of a case at the start x4 [N, 4]: -> (ok, text).  3-D objective, then the three stages"""
    x3 = x4.copy()
    x3[:, 3] = 0.0
    ev = embed_eval(x3, case["lower"], case["upper"], case["cons"], 0.0, 1.0, 1.0)
    bad = [] if ev["margin"] >= MARGIN else [f"objective margin {ev['margin']:.2e}"]
    for stage, (_, _, _, _, four) in STAGES.items():
        st = embed_step(x4 if four else x3, case["lower"], case["upper"], case["cons"], stage)
        if st["margin"] < MARGIN:
            bad.append(f"{stage} margin {st['margin']:.2e}")
        if st["ftol_ratio"] < 2:
            bad.append(f"{stage} force {st['fm']:.2e} too close to CE_FTOL")
        if st["moves"] and (st["clamp_margin"] < CLAMP_MARGIN or not st["clamp_bound_ok"]):
            bad.append(f"{stage} clamp margin {st['clamp_margin']:.2e}")
    return not bad, "; ".join(bad)


# ======================================================================================================== 2. matching: reference
def dihedral_with_bound(p, quad):
    """IUPAC dihedral of p[quad] in float64 (atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3))) and the bound of dihedral4's fp32 error"""
    k, u, v, l = (int(q) for q in quad)
    b1, b2, b3 = p[u] - p[k], p[v] - p[u], p[l] - p[v]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    nb2 = math.sqrt(float(b2 @ b2))
    y, x = nb2 * float(b1 @ n2), float(n1 @ n2)
    phi = math.atan2(y, x)
    a1, a2, a3 = np.abs(b1), np.abs(b2), np.abs(b3)
    an1, an2 = _cross_abs(a1[None], a2[None])[0], _cross_abs(a2[None], a3[None])[0]
    am = _cross_abs(an1[None], an2[None])[0]
    ay, ax = float(am @ a2) / nb2, float(an1 @ an2)
    ey, ex = 18.5 * U * ay, 11 * U * ax
    return phi, (abs(x) * ey + abs(y) * ex) / (x * x + y * y) + 6 * 2 * U * math.pi


def _rodrigues(d, khat, ang):
    """rows of d turned by ang about the unit vector khat"""
    c, s = math.cos(ang), math.sin(ang)
    return d * c + np.cross(khat[None, :], d) * s + khat[None, :] * (d @ khat)[:, None] * (1.0 - c)


def kabsch_rmsd(a, b):
    """aligned RMSD from the singular values of the covariance: (|a|^2 + |b|^2 - 2 (s1 + s2 + det s3)) / n"""
    a0, b0 = a - a.mean(0), b - b.mean(0)
    Uo, s, Vt = np.linalg.svd(a0.T @ b0)
    dsign = np.sign(np.linalg.det(Uo @ Vt))
    r2 = ((a0 * a0).sum() + (b0 * b0).sum() - 2.0 * (s[0] + s[1] + dsign * s[2])) / len(a)
    return math.sqrt(max(r2, 0.0)), r2


def match_ref(pos, target, theta, quads, mask, mut=None, want_bound=True, extra_angle=0.0):
    """The objective restated: rotations about u - v by sgn (theta - phi), sgn = -1 when the l side turns, then Kabsch by SVD.
    `extra_angle`: an error of every angle (radians) the bound is to cover on top of the kernel's own.
    -> (rmsd, bound of r^2 [None without want_bound], r^2); not a number when a mistake makes an axis vanish"""
    p = np.array(pos, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    quads = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    mask = np.asarray(mask).astype(bool)
    n = len(p)
    order = (0, 2, 1, 3) if mut == "phi_order" else (0, 1, 2, 3)
    phis = [dihedral_with_bound(p, q[list(order)]) for q in quads]
    E, own, moved = np.zeros(n), np.zeros(n), np.zeros(n)
    for r, (k, u, v, l) in enumerate(quads):
        side = mask[r]
        sgn = -1.0 if (side[l] and mut != "sgn_ignored") else 1.0
        delta = sgn * (float(theta[r]) - phis[r][0])
        au, av = (u & 63, v & 63) if mut == "slot_u63" else (u, v)
        axis = p[av] - p[au] if mut == "axis_v_minus_u" else p[au] - p[av]
        L = math.sqrt(float(axis @ axis))
        if L == 0.0:
            return float("nan"), None, float("nan")
        origin = p[av].copy()
        d = p[side] - origin
        p[side] = _rodrigues(d, axis / L, delta) + origin
        if want_bound:
            dn = np.sqrt((d * d).sum(1))
            e_ang = phis[r][1] + U * (11 * abs(delta) + 36) + extra_angle
            tilt = 13 * U + (own[u] + own[v]) / L + 31 * U * moved[u]
            mine = U * (7 * dn + np.sqrt((p[side] ** 2).sum(1)))
            E[side] += (e_ang + 2 * tilt + 31 * U) * dn + mine
            own[side] += mine
            moved[side] += 1
    rmsd, r2 = kabsch_rmsd(p, t)
    if not want_bound:
        return rmsd, None, r2
    a0, b0 = p - p.mean(0), t - t.mean(0)
    amax, bmax = math.sqrt((a0 * a0).sum(1).max()), math.sqrt((b0 * b0).sum(1).max())
    Erms = math.sqrt(float((E * E).mean())) + U * math.sqrt(3.0) * (amax + bmax)
    slots = (n + 63) // 64
    eps = (slots + 7) * U * math.sqrt(3.0) * (np.abs(p).max() + np.abs(t).max())
    b_r2 = 2 * rmsd * Erms + Erms ** 2 + eps ** 2 + 4 * U * (rmsd + Erms) ** 2 + 512 * 2.0 ** -53 * ((a0 * a0).sum() + (b0 * b0).sum()) / n
    return rmsd, b_r2, r2


# ======================================================================================================== 2. matching: the cases
def build_tree(nl, R, branched, rng):
    """A tree of nl atoms (bond length 1.5) with R torsion bonds.  -> pos [nl, 3], quads [R, 4] (k, u, v, l), mask [R, nl]: bond r turns the
    l side (the subtree under v) for even r and the k side (everything else) for odd r"""
    parent = np.full(nl, -1)
    pos = np.zeros((nl, 3))
    for i in range(1, nl):
        parent[i] = i - 1 if (not branched or rng.random() < 0.7) else rng.integers(max(0, i - 6), i)
        step = rng.normal(size=3)
        pos[i] = pos[parent[i]] + 1.5 * step / np.linalg.norm(step)
    children = [[] for _ in range(nl)]
    for i in range(1, nl):
        children[parent[i]].append(i)
    elig = [i for i in range(1, nl) if children[i] and (parent[parent[i]] >= 0 or len(children[parent[i]]) > 1)]
    assert len(elig) >= R, (nl, R, len(elig))
    quads, mask = [], np.zeros((R, nl), bool)
    for r, v in enumerate(sorted(rng.choice(elig, R, replace=False).tolist())):
        u = int(parent[v])
        k = int(parent[u]) if parent[u] >= 0 else [c for c in children[u] if c != v][0]
        sub, stack = np.zeros(nl, bool), [v]
        while stack:
            a = stack.pop()
            sub[a] = True
            stack += children[a]
        quads.append((k, u, v, children[v][0]))
        mask[r] = sub if r % 2 == 0 else ~sub
    return pos, np.asarray(quads, dtype=np.int64), mask


def slot_permutation(nl, quads, rng):
    """new label of every atom, so that (slot of u, slot of v) of the bonds runs through as many of the slot pairs as nl admits"""
    slots = (nl + 63) // 64
    free = [list(rng.permutation(np.arange(64 * s, min(64 * s + 64, nl)))) for s in range(slots)]
    lab = np.full(nl, -1)
    want = 0
    for (_, u, v, _) in quads:
        su, sv = want % slots, (want // slots) % slots
        if lab[u] < 0 and lab[v] < 0 and free[su] and free[sv] and (su != sv or len(free[su]) >= 2):
            lab[u] = free[su].pop()
            lab[v] = free[sv].pop()
            want += 1
    rest = list(rng.permutation([x for f in free for x in f]))
    for a in range(nl):
        if lab[a] < 0:
            lab[a] = rest.pop()
    assert sorted(lab.tolist()) == list(range(nl))
    return lab


def relabel(lab, pos, target, quads, mask):
    p, t, m = np.empty_like(pos), np.empty_like(target), np.empty_like(mask)
    p[lab], t[lab], m[:, lab] = pos, target, mask
    return p, t, lab[quads], m


def random_rigid(rng, p):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return (p - p.mean(0)) @ rot.T + rng.normal(size=3) * 3.0


# (Nl, R, branched, exact target)
MATCH_SHAPES = [(4, 1, False, False), (4, 1, False, True), (63, 2, True, False), (64, 31, False, False), (65, 32, True, False), (128, 1, True, True),
                (129, 2, False, False), (192, 31, True, False), (193, 32, False, True), (256, 32, True, False), (256, 1, False, False),
                (256, 2, True, True)]
N_THETA = 16
THETA_ROWS = ("phi", "phi+2pi", "phi-2pi", "phi+4pi", "phi+pi", "phi-pi", "+pi", "-pi", "beyond", "reached") + ("random",) * 6


@functools.lru_cache(maxsize=None)
def match_cases():
    """list of dicts: id, plain = (pos, target, quads, mask) as float32 / int, permuted = the same molecule relabelled, lab, theta
    [N_THETA, R] float32 (the same angles for both: a bond keeps its row), phi (float64, of the fp32 probe)"""
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    out = []
    for i, (nl, R, branched, exact) in enumerate(MATCH_SHAPES):
        rng = np.random.default_rng(500 + i)
        pos, quads, mask = build_tree(nl, R, branched, rng)
        pos = random_rigid(rng, pos).astype(np.float32)
        values = rng.uniform(-np.pi, np.pi, R).astype(np.float32)
        target = random_rigid(rng, cm.apply_changes(pos, values, quads, mask))
        if not exact:
            target = target + rng.normal(size=target.shape) * 0.2
        target = target.astype(np.float32)
        phi = np.array([dihedral_with_bound(pos.astype(np.float64), q)[0] for q in quads])
        th = rng.uniform(-np.pi, np.pi, (N_THETA, R))
        th[0], th[1], th[2], th[3], th[4], th[5] = phi, phi + 2 * np.pi, phi - 2 * np.pi, phi + 4 * np.pi, phi + np.pi, phi - np.pi
        th[6], th[7] = np.pi, -np.pi
        th[8] = rng.choice([-1.0, 1.0], R) * rng.uniform(2 * np.pi, 3 * np.pi, R)
        th[9] = values
        lab = slot_permutation(nl, quads, rng)
        plain = (pos, target, quads, mask)
        out.append({"id": f"nl{nl}_r{R}_{'tree' if branched else 'chain'}_{'exact' if exact else 'noisy'}", "nl": nl, "R": R, "exact": exact,
                    "plain": plain, "permuted": relabel(lab, *plain), "lab": lab, "theta": th.astype(np.float32), "phi": phi})
    return out


@functools.lru_cache(maxsize=None)
def match_expected(i):
    """(r^2 [N_THETA], bound of r^2 [N_THETA]) of match_cases()[i], from the unpermuted molecule"""
    c = match_cases()[i]
    res = [match_ref(*c["plain"][:2], t, *c["plain"][2:]) for t in c["theta"]]
    return np.array([r[2] for r in res]), np.array([r[1] for r in res])


def slot_pairs(case, which):
    """set of (slot of u, slot of v, the l side turns) over the bonds of a case"""
    _, _, quads, mask = case[which]
    return {(int(u) >> 6, int(v) >> 6, bool(mask[r, l])) for r, (k, u, v, l) in enumerate(quads)}


# ======================================================================================================== 3. the evolution's start
RP_INIT, RP_PERM = 1, 2
DE_ULPS = 2
PI32 = np.float32(3.14159265358979323846)


def draw_u32(key, individual, dim, purpose):
    return mix64(key ^ ((individual << 32) | ((dim << 8) & 0xffffffff) | purpose)) >> 32


def draw_unit(key, individual, dim, purpose):
    return np.float32(draw_u32(key, individual, dim, purpose) >> 8) * np.float32(1.0 / 16777216.0)


def keyed_perm(i, P, bits, key, dim):
    m, sh = (1 << bits) - 1, (bits + 1) >> 1
    k0, k1, k2 = (draw_u32(key, j, dim, RP_PERM) for j in range(3))
    x = i
    for _ in range(m + 1):
        x = (x + k0) & m; x = (x * (k1 | 1)) & m; x ^= x >> sh
        x = (x + k2) & m; x = (x * ((k0 >> 7) | 1)) & m; x ^= x >> sh
        x = (x + (k1 >> 5)) & m; x = (x * ((k2 >> 3) | 1)) & m; x ^= x >> sh
        if x < P:
            break
    return x


def de_bits(P):
    bits = 1
    while (1 << bits) < P:
        bits += 1
    return bits


def de_key(seed, problem_id):
    return mix64(mix64(mix64(seed & M64) ^ (problem_id & 0xffffffff)))          # generation 0


def de_population(seed, problem_id, popsize, R):
    """[P, R] float32: the Latin-hypercube start of match_de_kernel, every operation one numpy float32 rounding"""
    P = max(popsize * R, 5)
    key, bits = de_key(seed, problem_id), de_bits(P)
    pop = np.empty((P, R), np.float32)
    two_pi = np.float32(2.0) * PI32
    for i in range(P):
        for j in range(R):
            q = (np.float32(keyed_perm(i, P, bits, key, j)) + draw_unit(key, i, j, RP_INIT)) / np.float32(P)
            v = -PI32 + two_pi * q
            pop[i, j] = -PI32 if v >= PI32 else v
    return pop


# (popsize, R, Nl) -> P = max(popsize R, 5) in {5, 15, 17, 64, 65, 480, 512}
DE_SHAPES = [(1, 1, 6), (5, 3, 12), (17, 1, 6), (2, 32, 40), (65, 1, 6), (15, 32, 40), (16, 32, 40)]
DE_SEED = 11


@functools.lru_cache(maxsize=None)
def de_problems():
    """one noisy matching problem per entry of DE_SHAPES: (pos, target, quads, mask)"""
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    out = []
    for i, (_, R, nl) in enumerate(DE_SHAPES):
        rng = np.random.default_rng(900 + i)
        pos, quads, mask = build_tree(nl, R, R == 3, rng)          # a chain of 40 atoms has 37 bonds with a dihedral, a tree fewer
        pos = pos.astype(np.float32)
        target = random_rigid(rng, cm.apply_changes(pos, rng.uniform(-np.pi, np.pi, R), quads, mask)) + rng.normal(size=pos.shape) * 0.2
        out.append((pos, target.astype(np.float32), quads, mask))
    return out


# ======================================================================================================== 4. deliberate mistakes
EMBED_MUTATIONS = ("vol_sign_role0", "vol_sign_role1", "vol_sign_role2", "vol_sign_role3", "pair_share_1", "no_narrowing", "sg_ignored", "upper_coef_2",
                   "planar_wv")
MATCH_MUTATIONS = ("axis_v_minus_u", "sgn_ignored", "slot_u63", "phi_order")
