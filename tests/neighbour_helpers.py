"""Shared by tests/test_neighbour_refs.py (CPU) and tests/test_gpu_neighbours.py (GPU): references, bounds and seeded case tables of

  cbd_knn_graph, cbd_radius_neighbors     csrc/featurise.hip     process_mols.knn_graph / cutoff_graph
  cbd_radius_count, cbd_radius_fill       csrc/train_graph.hip   train_ops.RadiusQuery / radius_queries
  cbd_edge_geometry                       csrc/train_graph.hip   train_ops.edge_geometry
  cbd_symm_rmsd                           csrc/kernels.hip       molecules_utils.symmetry_rmsd

Three kinds of reference.

 * float32 (`*_ref_f32`): numpy restatements in the kernels' operation order -- subtract, (dx dx + dy dy) + dz dz with every operation
   rounded and no fma (numpy never contracts), order by (fp32 bit pattern of d^2, index), the centre excluded.  sqrt and the division by a
   per-graph cutoff are numpy float32 operations, which are correctly rounded.  They reproduce the five edge lists of
   tests/golden/g15_featurise_1a0q.npz, which the reference project produced (tests/test_neighbour_refs.py), and are EXACT: no tolerance.
   Every one takes `mut`, the name of one deliberate mistake (MUTATIONS); the CPU file shows that each mistake changes a GPU case.
 * integer (`*_ref_int`): the same rules on q = round(4 pos), D2 = sum (q_j - q_i)^2, compared as integers.  Valid for inputs on the
   quarter-Angstrom lattice only (asserted), where every fp32 difference, square and sum is exact; independent of any floating-point
   evaluation.  d < cutoff becomes D2 < 16 cutoff^2 in rationals; that is the fp32 test sqrt_f32(D2 / 16) < cutoff as long as no
   integer lies in [16 c^2 (1 - 2^-22), 16 c^2), which is asserted.  The batched search needs cutoffs that are powers of two (x / c exact).
 * float64 with a bound, u = 2^-24:
     unit vector  |err| <= 4.5 u |ref| + 2^-149       v is the fp32 difference (compared bit for bit), everything else float64 from it.
                  The sum of squares carries at most 3 u (a contracted fma makes fewer roundings, never more), the root halves that and
                  adds 0.5 u, the reciprocal 1 u, the product 1 u; 0.5 u covers second order.
     smear        t = d - mu, a = coeff t^2:  |da| <= |coeff| 2 |t| (2 u d + u |t|) + 2 u |a|,   |err| <= ref (1.01 |da| + 4 u) + 1e-37
                  d carries 2 u (above), the subtraction 1 u, t * t and coeff * () one rounding each.  ASSUMPTION: the `4 u` term allows
                  the device expf 2 ulp; it is the one figure here that is not derived from the source (the vendor documents 1 ulp).
     rmsd         |out - ref| <= 0.5 spacing(float32(ref)) (1 + 2^-20): the kernel accumulates in float64, so its error is the one
                  rounding to fp32; the reference is float64 with math.fsum.  On lattice coordinates every S(k) is an exact float64
                  (an integer / 16), so the first minimum of the reference must be matched exactly.

Case builders are seeded and return the inputs with the names of the paths they are meant to hit; the path counters (`*_paths`) work on
the references alone."""
import math
import types
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
MUTATIONS = ("tie_high",        # ties in distance go to the higher index
             "le",              # the cutoff comparison is <=
             "d2_vs_cutoff",    # the cutoff test is on d^2 against the cutoff
             "keep_centre",     # the centre is not excluded
             "switch_lt",       # the cutoff kernel switches to "nearest by distance" at total < cap, not total <= cap
             "rank_no_self",    # the batched rank does not count the query itself
             "nearest_cap",     # the batched search keeps the cap nearest, not the first cap in index order
             "no_first",        # the key (d2 = 0, index 0) is rejected, as `key > last` alone would (last starts at 0)
             "last_min",        # the RMSD takes the last minimum
             "mu_shift")        # the smear uses mu[k - 1]


# ------------------------------------------------------------------------------------------------------------------ fp32 references
def _d2_f32(a, b):
    """[len(a), len(b)] float32: d2[i, j] = ((b_j - a_i)_x^2 + (..)_y^2) + (..)_z^2, every operation rounded to fp32"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = b[None, :, :] - a[:, None, :]
    s = d * d
    return (s[..., 0] + s[..., 1]) + s[..., 2]


def _pack(d2, mut):
    """the kernels' 64-bit keys (fp32 bits of d2 << 32 | index) of a [rows, n] matrix"""
    n = d2.shape[1]
    low = np.arange(n, dtype=np.uint64)
    if mut == "tie_high":
        low = np.uint64(n - 1) - low
    keys = (np.ascontiguousarray(d2).view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[None, :]
    if mut == "no_first":
        keys[keys == 0] = ALL_ONES
    return keys


def _unpack(keys, n, mut):
    low = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    idx = low.view(np.int32).astype(np.int64)              # an exhausted selection (all ones) reads as -1, as in the kernel
    if mut == "tie_high":
        idx = np.where(keys == ALL_ONES, -1, n - 1 - idx)
    return idx


def _nearest_f32(pos, kmax, mut=None, block=1024):
    """[n, kmax] indices by increasing (d2 bits, index), the centre excluded, and the matching d2 [n, kmax]"""
    pos = np.asarray(pos, np.float32)
    n = pos.shape[0]
    out, dist = np.empty((n, kmax), np.int64), np.empty((n, kmax), np.float32)
    for r0 in range(0, n, block):
        rows = np.arange(r0, min(n, r0 + block))
        keys = _pack(_d2_f32(pos[rows], pos), mut)
        if mut != "keep_centre":
            keys[np.arange(len(rows)), rows] = ALL_ONES
        sel = np.sort(np.partition(keys, kmax - 1, axis=1)[:, :kmax], axis=1) if kmax < n else np.sort(keys, axis=1)[:, :kmax]
        out[rows] = _unpack(sel, n, mut)
        dist[rows] = (sel >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return out, dist


def _knn_edges(nbr):
    n, k = nbr.shape
    return np.stack([nbr.reshape(-1), np.repeat(np.arange(n, dtype=np.int64), k)])


def knn_ref_f32(pos, k, mut=None):
    """process_mols.knn_graph(pos, k): [2, n min(k, n - 1)] int64, row 0 = neighbour, row 1 = centre"""
    n = len(pos)
    k = max(0, min(int(k), n - 1))
    if k == 0:
        return np.zeros((2, 0), np.int64)
    return _knn_edges(_nearest_f32(pos, k, mut)[0])


def _table_edges(idx, cnt):
    n, cap = idx.shape
    keep = np.arange(cap)[None, :] < cnt[:, None]
    return np.stack([idx[keep], np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], (n, cap))[keep]])


def _cutoff_table(inm, nearest, cap, mut):
    """(idx [n, cap] with -1 in unused slots, cnt [n]) from the in-cutoff matrix and the [n, cap] nearest-by-distance table"""
    total = inm.sum(1)
    in_order = (total > 0) & ((total < cap) if mut == "switch_lt" else (total <= cap))
    by_index = np.argsort(~inm, axis=1, kind="stable")[:, :cap]
    cnt = np.where(in_order, total, np.where(total == 0, 1, cap))
    idx = np.where(in_order[:, None], by_index, nearest)
    idx = np.where(np.arange(cap)[None, :] < cnt[:, None], idx, -1)
    return idx.astype(np.int64), cnt.astype(np.int64)


def clip_cap(n, cap):
    """process_mols.cutoff_graph's clipping of max_neighbors"""
    return max(1, min(int(cap) if cap else 1000, n - 1))


def cutoff_table_f32(pos, cutoff, cap, mut=None):
    """what cbd_radius_neighbors writes: idx [n, cap] (unused slots -1 here, untouched there) and cnt [n]; n >= 2, 1 <= cap <= n - 1"""
    pos = np.asarray(pos, np.float32)
    n = pos.shape[0]
    d2 = _d2_f32(pos, pos)
    c = np.float32(cutoff)
    inm = (d2 < c) if mut == "d2_vs_cutoff" else (np.sqrt(d2) <= c) if mut == "le" else (np.sqrt(d2) < c)
    if mut != "keep_centre":
        inm[np.arange(n), np.arange(n)] = False
    return _cutoff_table(inm, _nearest_f32(pos, cap, mut)[0], cap, mut)


def cutoff_ref_f32(pos, cutoff, cap, mut=None):
    """process_mols.cutoff_graph(pos, cutoff, cap): [2, E] int64, row 0 = neighbour, row 1 = centre; a single node has no edges"""
    n = len(pos)
    if n < 2:
        return np.zeros((2, 0), np.int64)
    return _table_edges(*cutoff_table_f32(pos, cutoff, clip_cap(n, cap), mut))


def radius_batched_ref_f32(x, y, r, xptr, ybatch, cap, drop_self, cutoff=None, mut=None):
    """RadiusQuery(x, y, r, xptr, ybatch, cap, drop_self, cutoff): (counts [ny] int64, edges [2, E] int64 with row 0 = query, row 1 =
    point).  A query's in-radius points are taken in index order; the 1-based rank counts the query itself; a point is kept when its
    rank is at most cap and it is not the query (drop_self).  Queries ascending, points ascending within a query."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    xptr, ybatch = np.asarray(xptr, np.int64), np.asarray(ybatch, np.int64)
    r2 = np.float32(r) * np.float32(r)
    counts = np.zeros(len(y), np.int64)
    qs_all, js_all = [], []
    for b in range(len(xptr) - 1):
        lo, hi = int(xptr[b]), int(xptr[b + 1])
        qs = np.flatnonzero(ybatch == b)
        if hi == lo or len(qs) == 0:
            continue
        xg, yg = x[lo:hi], y[qs]
        if cutoff is not None:
            c = np.float32(np.asarray(cutoff, np.float32).reshape(-1)[b])
            xg, yg = xg / c, yg / c
        d2 = _d2_f32(yg, xg)
        inm = d2 < r2
        selfm = (np.arange(lo, hi)[None, :] == qs[:, None]) & bool(drop_self)
        if mut == "nearest_cap":
            order = np.argsort(_pack(np.where(inm, d2, np.float32(np.inf)), None), axis=1)
            rank = np.empty_like(order)
            np.put_along_axis(rank, order, np.broadcast_to(np.arange(1, hi - lo + 1), order.shape), axis=1)
        else:
            rank = np.cumsum(inm & ~selfm if mut == "rank_no_self" else inm, axis=1)
        keep = inm & (rank <= cap) & ~selfm
        counts[qs] = keep.sum(1)
        qi, ji = np.nonzero(keep)
        qs_all.append(qs[qi])
        js_all.append(lo + ji)
    if not qs_all:
        return counts, np.zeros((2, 0), np.int64)
    q, j = np.concatenate(qs_all), np.concatenate(js_all)
    order = np.lexsort((j, q))
    return counts, np.stack([q[order], j[order]])


# --------------------------------------------------------------------------------------------------------------- integer references
def _quarters(pos):
    q = np.rint(np.asarray(pos, np.float64) * 4).astype(np.int64)
    assert np.array_equal(q / 4.0, np.asarray(pos, np.float64)), "integer references need inputs on the quarter-Angstrom lattice"
    return q


def _D2(qa, qb):
    d = qb[None, :, :] - qa[:, None, :]
    return (d * d).sum(-1)


def _limit(c2_times_16):
    """D2 < thr (a rational) as D2 < lim for integers; refuses a threshold at which the fp32 evaluation could round the other way"""
    lim = math.ceil(c2_times_16)
    assert lim - 1 < c2_times_16 * (1 - Fraction(1, 2 ** 22)) or lim - 1 < 0, "an integer D2 lies within fp32 rounding of the cutoff"
    return lim


def _nearest_int(q, kmax):
    n = len(q)
    key = _D2(q, q) * (1 << 32) + np.arange(n)[None, :]
    key[np.arange(n), np.arange(n)] = np.iinfo(np.int64).max
    return np.argsort(key, axis=1, kind="stable")[:, :kmax].astype(np.int64)


def knn_ref_int(pos, k):
    n = len(pos)
    k = max(0, min(int(k), n - 1))
    return _knn_edges(_nearest_int(_quarters(pos), k)) if k else np.zeros((2, 0), np.int64)


def cutoff_ref_int(pos, cutoff, cap):
    n = len(pos)
    if n < 2:
        return np.zeros((2, 0), np.int64)
    cap, q = clip_cap(n, cap), _quarters(pos)
    inm = _D2(q, q) < _limit(16 * Fraction(float(np.float32(cutoff))) ** 2)
    inm[np.arange(n), np.arange(n)] = False
    return _table_edges(*_cutoff_table(inm, _nearest_int(q, cap), cap, None))


def radius_batched_ref_int(x, y, r, xptr, ybatch, cap, drop_self, cutoff=None):
    qx, qy = _quarters(x), _quarters(y)
    r2 = Fraction(float(np.float32(r) * np.float32(r)))
    assert r2 == Fraction(float(np.float32(r))) ** 2, "r * r must be exact in fp32"
    counts, qs_all, js_all = np.zeros(len(qy), np.int64), [], []
    for b in range(len(xptr) - 1):
        lo, hi = int(xptr[b]), int(xptr[b + 1])
        qs = np.flatnonzero(np.asarray(ybatch) == b)
        if hi == lo or len(qs) == 0:
            continue
        c = Fraction(1) if cutoff is None else Fraction(float(np.asarray(cutoff, np.float32).reshape(-1)[b]))
        assert c.numerator == 1 or c.denominator == 1, "x / c must be exact"
        assert (c.numerator & (c.numerator - 1)) == 0 and (c.denominator & (c.denominator - 1)) == 0, "cutoffs must be powers of two"
        inm = _D2(qy[qs], qx[lo:hi]) < _limit(16 * c * c * r2)
        selfm = (np.arange(lo, hi)[None, :] == qs[:, None]) & bool(drop_self)
        keep = inm & (np.cumsum(inm, axis=1) <= cap) & ~selfm
        counts[qs] = keep.sum(1)
        qi, ji = np.nonzero(keep)
        qs_all.append(qs[qi])
        js_all.append(lo + ji)
    if not qs_all:
        return counts, np.zeros((2, 0), np.int64)
    q, j = np.concatenate(qs_all), np.concatenate(js_all)
    order = np.lexsort((j, q))
    return counts, np.stack([q[order], j[order]])


# ---------------------------------------------------------------------------------------------------- float64 references and bounds
def edge_geometry_ref64(pos_a, pos_b, idx_a, idx_b, mu, coeff, mut=None):
    """dict: vec32 [E, 3] (the fp32 difference, to be matched bit for bit), unit / unit_bound [E, 3], smear / smear_bound [E, K], d [E];
    float64 from the fp32 vector, the fp32 mu and the fp32 coeff"""
    pa, pb = np.asarray(pos_a, np.float32), np.asarray(pos_b, np.float32)
    E = len(idx_a) if idx_a is not None else len(idx_b) if idx_b is not None else len(pb)
    a = np.arange(E) if idx_a is None else np.asarray(idx_a)
    b = np.arange(E) if idx_b is None else np.asarray(idx_b)
    vec32 = pb[b] - pa[a]
    v = vec32.astype(np.float64)
    d = np.sqrt((v * v).sum(-1))
    unit = v / np.maximum(d, 1e-12)[:, None]
    mu64 = np.asarray(mu, np.float32).astype(np.float64)
    if mut == "mu_shift":
        mu64 = np.roll(mu64, 1)
    c = float(np.float32(coeff))
    t = d[:, None] - mu64[None, :]
    arg = c * t * t
    smear = np.exp(arg)
    da = abs(c) * 2 * np.abs(t) * (2 * U * d[:, None] + U * np.abs(t)) + 2 * U * np.abs(arg)
    return {"vec32": vec32, "d": d, "unit": unit, "unit_bound": 4.5 * U * np.abs(unit) + 2.0 ** -149, "smear": smear,
            "smear_bound": smear * (1.01 * da + 4 * U) + 1e-37, "expf_share": smear * 4 * U}


def symm_rmsd_ref64(pos, ref, idx_ref, idx_pos, mut=None):
    """(rmsd [B] float64, argmin [B], S [B, K] float64): S by math.fsum over the 3 N squared float64 differences, the first minimum wins"""
    pos, ref = np.asarray(pos, np.float32).astype(np.float64), np.asarray(ref, np.float32).astype(np.float64)
    B, N, K = pos.shape[0], pos.shape[1], idx_ref.shape[0]
    S = np.empty((B, K))
    for b in range(B):
        for k in range(K):
            d = ref[idx_ref[k]] - pos[b][idx_pos[k]]
            S[b, k] = math.fsum((d * d).ravel().tolist())
    arg = (K - 1 - np.argmin(S[:, ::-1], axis=1)) if mut == "last_min" else np.argmin(S, axis=1)
    return np.sqrt(S[np.arange(B), arg] / N), arg.astype(np.int64), S


def rmsd_bound(ref64):
    return 0.5 * np.spacing(np.asarray(ref64, np.float64).astype(np.float32)).astype(np.float64) * (1 + 2.0 ** -20)


# ------------------------------------------------------------------------------------------------------------------------ the cases
GRAPH_NS = (2, 3, 63, 64, 65, 127, 128, 129, 200)
LATTICE_KINDS = ("lattice", "coincident", "identical", "line", "shifted")


def lattice_points(rng, n, lo=-12, hi=12):
    """n points on the quarter-Angstrom lattice in [lo / 4, hi / 4]^3"""
    return (rng.integers(lo, hi + 1, size=(n, 3)) / 4.0).astype(np.float32)


def graph_input(kind, n):
    """(pos [n, 3] float32, names of the paths the input is meant to hit) for the kNN and the cutoff graph; n = 2 and 3 are there for
    their size and name no path"""
    pos, names = _graph_input(kind, n)
    return pos, names if n >= 63 else ()


def _graph_input(kind, n):
    rng = np.random.default_rng(1000 * LATTICE_KINDS.index(kind) + n if kind in LATTICE_KINDS else 7000 + n)
    if kind == "lattice":
        return lattice_points(rng, n), ("tie_at_k", "tie_inside", "under", "equal", "plus1", "at_cutoff") + (("many_tie",) if n > 63 else ())
    if kind == "coincident":
        pos = lattice_points(rng, n)
        pos[n - 1] = pos[0]
        pos[n // 2] = pos[0]
        return pos, ("key_zero", "coincident")
    if kind == "identical":
        return np.tile(np.float32([0.25, -1.5, 2.0]), (n, 1)), ("key_zero", "coincident", "tie_at_k")
    if kind == "line":
        pos = np.zeros((n, 3), np.float32)
        pos[:, 0] = 0.5 * np.arange(n) - 3.0
        return pos, ("tie_inside", "at_cutoff", "none")
    if kind == "shifted":
        return lattice_points(rng, n) + np.float32(1000.0), ("tie_at_k",)
    if kind == "randn":
        return (rng.standard_normal((n, 3)) * 10).astype(np.float32), ()
    raise ValueError(kind)


def graph_inputs():
    """(kind, n) of every kNN / cutoff input: the lattice kinds at every n, randn * 10 (fp32 reference only) at 129 and 200"""
    return [(kind, n) for kind in LATTICE_KINDS for n in GRAPH_NS] + [("randn", 129), ("randn", 200)]


def knn_ks(n):
    return sorted({min(k, n - 1) for k in (1, 8, 24, n - 1)})


def cutoff_settings(n):
    return [(1.0, 3), (2.0, 8), (0.2, 4), (50.0, n - 1), (1.0, 1)]


def knn_paths(pos, k):
    """how many centres hit each path of knn_kernel, from the fp32 reference"""
    n = len(pos)
    nbr, d2 = _nearest_f32(pos, n - 1)
    p = {"tie_at_k": int((d2[:, k - 1] == d2[:, k]).sum()) if k < n - 1 else 0,
         "tie_inside": int((d2[:, :k - 1] == d2[:, 1:k]).any(1).sum()),
         "coincident": int((d2[:, :k] == 0).any(1).sum()),
         "key_zero": int(((nbr[:, :k] == 0) & (d2[:, :k] == 0)).any(1).sum()),
         "second_chunk": int((nbr[:, :k] >= 64).any(1).sum())}
    return p


def cutoff_paths(pos, cutoff, cap):
    """how many centres leave radius_neighbors_kernel by each exit, from the fp32 reference"""
    n = len(pos)
    if n < 2:
        return {"n1": 1}
    cap = clip_cap(n, cap)
    d2 = _d2_f32(pos, pos)
    dist = np.sqrt(d2)
    off = ~np.eye(n, dtype=bool)
    total = ((dist < np.float32(cutoff)) & off).sum(1)
    _, nd2 = _nearest_f32(pos, min(cap + 1, n - 1))
    tie = (nd2[:, cap - 1] == nd2[:, cap]) if cap < n - 1 else np.zeros(n, bool)
    return {"none": int((total == 0).sum()), "under": int(((total >= 1) & (total < cap)).sum()), "equal": int((total == cap).sum()),
            "plus1": int((total == cap + 1).sum()), "many": int((total > cap + 1).sum()), "many_tie": int(((total > cap + 1) & tie).sum()),
            "at_cutoff": int(((dist == np.float32(cutoff)) & off).any(1).sum()), "n2": int(n == 2)}


RADIUS_SIZES = (1, 63, 64, 65, 129, 0, 200)
RADIUS_QUERIES = (3, 5, 2, 4, 7, 3, 6)              # queries per graph of the cross form; graph 5 has queries and no points
RADIUS_CAPS = (1, 2, 33, 64, 65, 10000)
ALL_IN_CAPS = (63, 64, 65, 128, 129, 130)
ALL_IN_OFFSETS = (0, 63, 64, 128)


def _ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def radius_cases():
    """dicts with the arguments of RadiusQuery (numpy), `lattice` (the integer reference applies) and `paths`.  Random cases: the seven
    graphs of RADIUS_SIZES on the integer lattice in [-6, 6]^3 (graph form: y = x, drop_self, the cap passed as cap + 1 as the caller
    does; cross form: RADIUS_QUERIES queries per graph), cutoffs none (r = 6) / powers of two / arbitrary (r = 1).  All-in-radius
    cases: a graph of 129 points that all coincide, between two small graphs so that global and local offsets differ."""
    out = []
    for form in ("graph", "cross"):
        for cmode in ("none", "pow2", "arbitrary"):
            for cap in RADIUS_CAPS:
                rng = np.random.default_rng([31, form == "graph", ("none", "pow2", "arbitrary").index(cmode), cap])
                x = rng.integers(-6, 7, size=(sum(RADIUS_SIZES), 3)).astype(np.float32)      # integer coordinates: some points coincide
                nb = len(RADIUS_SIZES)
                cut = {"none": None, "pow2": np.float32([4, 8, 2, 16, 8, 4, 8]),
                       "arbitrary": np.float32([7.3, 19.1] + list(3.0 + 20.0 * rng.random(nb - 2)))}[cmode]
                r = 6.0 if cmode == "none" else 1.0
                xptr = _ptr(RADIUS_SIZES)
                if form == "graph":
                    y, ybatch, kcap, drop = x, np.repeat(np.arange(nb), RADIUS_SIZES), cap + 1, True
                else:
                    y = rng.integers(-6, 7, size=(sum(RADIUS_QUERIES), 3)).astype(np.float32)
                    ybatch, kcap, drop = np.repeat(np.arange(nb), RADIUS_QUERIES), cap, False
                out.append({"id": f"{form}-{cmode}-cap{cap}", "x": x, "y": y, "r": r, "xptr": xptr, "ybatch": ybatch.astype(np.int64),
                            "cap": kcap, "drop_self": drop, "cutoff": cut, "lattice": cmode != "arbitrary", "all_in": False,
                            "paths": ("empty_graph",) if form == "cross" else ("self_beyond_cap",) if cap < 33 else ()})
    sizes = (5, 129, 3)
    for form in ("graph", "cross"):
        for cap in ALL_IN_CAPS:
            rng = np.random.default_rng(50 + cap)
            x = rng.integers(-6, 7, size=(sum(sizes), 3)).astype(np.float32)
            x[5:134] = np.float32([2.0, -3.0, 1.0])
            xptr = _ptr(sizes)
            if form == "graph":
                y, ybatch, drop = x, np.repeat(np.arange(3), sizes), True
            else:                                                   # one query per offset; the offset matters only to drop_self
                y = np.tile(np.float32([2.0, -3.0, 1.0]), (len(ALL_IN_OFFSETS), 1))
                ybatch, drop = np.full(len(ALL_IN_OFFSETS), 1), False
            out.append({"id": f"allin-{form}-cap{cap}", "x": x, "y": y, "r": 0.5, "xptr": xptr, "ybatch": ybatch.astype(np.int64),
                        "cap": cap, "drop_self": drop, "cutoff": None, "lattice": True, "all_in": True,
                        "paths": ("cap_at_boundary",) if cap in (64, 128) else ("cap_after_boundary",) if cap in (65, 129) else ()})
    return out


def all_in_expected(case):
    """closed form for the queries of the 129-point graph of an all-in-radius case: min(cap, size), less one when drop_self is set and
    the query's own rank is at most cap -> {query index: kept count}"""
    qs = np.flatnonzero(case["ybatch"] == 1)
    own = (qs - 5 + 1) if case["drop_self"] else np.full(len(qs), 10 ** 9)
    return {int(q): min(case["cap"], 129) - int(o <= case["cap"]) for q, o in zip(qs, own)}


def radius_paths(case):
    """how many queries hit each path of radius_batched_kernel, from the fp32 reference (uncapped membership)"""
    big = 1 << 40
    _, edges = radius_batched_ref_f32(case["x"], case["y"], case["r"], case["xptr"], case["ybatch"], big, False, case["cutoff"])
    ny, cap, xptr, yb = len(case["y"]), case["cap"], case["xptr"], case["ybatch"]
    p = dict.fromkeys(("empty_graph", "none_kept", "full_scan", "early_exit", "capped", "cap_at_boundary", "cap_after_boundary",
                       "self_beyond_cap", "self_within_cap"), 0)
    at = np.searchsorted(edges[0], np.arange(ny + 1))
    members = [edges[1][at[q]:at[q + 1]] for q in range(ny)]
    for q in range(ny):
        lo, hi, m = int(xptr[yb[q]]), int(xptr[yb[q] + 1]), members[q]
        if hi == lo:
            p["empty_graph"] += 1
            continue
        own = int(np.searchsorted(m, q)) + 1 if case["drop_self"] else None          # 1-based rank of the query among its points
        kept = min(len(m), cap) - (1 if own is not None and own <= cap else 0)
        p["none_kept"] += kept == 0
        p["capped"] += len(m) > cap
        if len(m) >= cap:
            off = int(m[cap - 1]) - lo                                             # local offset of the cap-th in-radius point
            last_chunk = (hi - lo - 1) // 64
            p["early_exit"] += off // 64 < last_chunk
            p["cap_at_boundary"] += off % 64 == 63 and off // 64 < last_chunk      # seen reaches cap with the chunk's last lane
            p["cap_after_boundary"] += off % 64 == 0 and off >= 64                 # ... with the first lane of a later chunk
        else:
            p["full_scan"] += 1
        if own is not None:
            p["self_beyond_cap"] += own > cap
            p["self_within_cap"] += own <= cap
    return {k: int(v) for k, v in p.items()}


GEOM_ES = (1, 3, 4, 5, 257)
GEOM_KS = (1, 32, 64, 65, 130)
GEOM_IDX = ("both", "a_none", "b_none", "neither")
GEOM_SCALES = (1.0, 6.0, 200.0)


def smearing(K, stop):
    """(offset float32 [K], coeff) of GaussianSmearing(0, stop, K); K = 1 has no spacing: one Gaussian at 0 of width stop"""
    import torch
    if K == 1:
        return np.zeros(1, np.float32), -0.5 / float(stop) ** 2
    offset = torch.linspace(0.0, stop, K)
    return offset.numpy(), -0.5 / (offset[1] - offset[0]).item() ** 2


def geometry_case(E, K, idx_mode, scale):
    """inputs of train_ops.edge_geometry: one zero-length edge (edge E // 2; for E = 1 only at scale 1, so that the single edge is also
    seen with a length), every other length >= 1e-3"""
    rng = np.random.default_rng([32, E, K, GEOM_IDX.index(idx_mode), int(scale)])
    Na, Nb = (E if idx_mode in ("a_none", "neither") else 50), (E if idx_mode in ("b_none", "neither") else 70)
    pa, pb = (rng.standard_normal((Na, 3)) * scale).astype(np.float32), (rng.standard_normal((Nb, 3)) * scale).astype(np.float32)
    ia = None if idx_mode in ("a_none", "neither") else rng.integers(0, Na, E)
    ib = None if idx_mode in ("b_none", "neither") else rng.integers(0, Nb, E)
    zero = E > 1 or scale == 1.0
    if zero:
        e = E // 2
        pb[e if ib is None else ib[e]] = pa[e if ia is None else ia[e]]
    offset, coeff = smearing(K, 5.0 * scale)
    case = {"id": f"E{E}-K{K}-{idx_mode}-s{int(scale)}", "pos_a": pa, "pos_b": pb, "idx_a": ia, "idx_b": ib, "offset": offset, "coeff": coeff,
            "stop": 5.0 * scale, "paths": (("zero_edge",) if zero else ()) + (("second_pass",) if K > 64 else ()) + (("partial_block",) if E % 4 else ())}
    d = edge_geometry_ref64(pa, pb, ia, ib, offset, coeff)["d"]
    assert ((d == 0) | (d >= 1e-3)).all() and bool((d == 0).any()) == zero
    return case


def geometry_cases(E, K):
    return [geometry_case(E, K, m, s) for m in GEOM_IDX for s in GEOM_SCALES]


def expansion_of(case, device=None):
    """the object train_ops.edge_geometry reads (offset buffer, coeff): the package's GaussianSmearing; K = 1, which it cannot build
    (it takes its width from offset[1] - offset[0]), as a plain namespace"""
    import torch
    K = len(case["offset"])
    if K > 1:
        from confidence_bootstrapping_amd.score_model import GaussianSmearing
        exp = GaussianSmearing(0.0, case["stop"], K)
        assert np.array_equal(exp.offset.numpy(), case["offset"]) and exp.coeff == case["coeff"]
        return exp.to(device) if device is not None else exp
    off = torch.from_numpy(case["offset"])
    return types.SimpleNamespace(offset=off.to(device) if device is not None else off, coeff=case["coeff"])


RMSD_NS = (1, 2, 63, 64, 65, 130)
RMSD_KS = (1, 2, 7, 64)
RMSD_BS = (1, 5)
RMSD_KINDS = ("dup", "sym", "randn", "exact")


def rmsd_case(kind, N, K, B):
    """(pos [B, N, 3], ref [N, 3], idx_ref [K, N], idx_pos [K, N] int32) with random permutation tables.
      dup    lattice; rows k1 < k2 of the tables are the same permutation and every pose is the crystal under it plus lattice noise
      sym    lattice; row k2 is row k1 with idx_pos swapped at two atoms i, j whose crystal positions differ along x only and whose pose
             positions share x: (r_i - r_j) . (p_i - p_j) = 0, so S(k1) = S(k2) exactly although the permutations differ (N >= 2)
      randn  randn * 5, the pose a permuted crystal plus noise that grows with the pose index (float64 bound)
      exact  lattice; pose b is the crystal under permutation k_b exactly: RMSD 0 and argmin = the first row that maps it so"""
    rng = np.random.default_rng([33, RMSD_KINDS.index(kind), N, K, B])
    idx_ref = np.stack([rng.permutation(N) for _ in range(K)]).astype(np.int32)
    idx_pos = np.stack([rng.permutation(N) for _ in range(K)]).astype(np.int32)
    lattice = kind != "randn"
    ref = lattice_points(rng, N, -20, 20) if lattice else (rng.standard_normal((N, 3)) * 5).astype(np.float32)
    k1, k2 = (sorted(rng.choice(K, 2, replace=False).tolist()) if K > 1 else (0, 0))
    paths = []
    if kind == "dup" and K > 1:
        idx_ref[k2], idx_pos[k2] = idx_ref[k1], idx_pos[k1]
        paths.append("tie_duplicate")
    if kind == "sym" and K > 1 and N > 1:
        i, j = 0, N - 1
        idx_ref[k2], idx_pos[k2] = idx_ref[k1], idx_pos[k1]
        idx_pos[k2, i], idx_pos[k2, j] = idx_pos[k1, j], idx_pos[k1, i]
        ref[idx_ref[k1, j], 1:] = ref[idx_ref[k1, i], 1:]
        ref[idx_ref[k1, j], 0] = ref[idx_ref[k1, i], 0] + np.float32(1.25)
        paths.append("tie_symmetric")
    pos = np.empty((B, N, 3), np.float32)
    for b in range(B):
        k = k1 if kind in ("dup", "sym") else int(rng.integers(K))
        pos[b, idx_pos[k]] = ref[idx_ref[k]]
        if kind in ("dup", "sym"):
            pos[b] += (rng.integers(-1, 2, size=(N, 3)) / 4.0).astype(np.float32)
        elif kind == "randn":
            pos[b] += rng.normal(0.0, 0.05 + 0.5 * b, size=(N, 3)).astype(np.float32)
        if kind == "sym" and K > 1 and N > 1:
            pos[b, idx_pos[k1, j], 0] = pos[b, idx_pos[k1, i], 0]
    if kind == "exact":
        paths.append("zero")
    if N > 64:
        paths.append("second_pass")
    return {"id": f"{kind}-N{N}-K{K}-B{B}", "pos": pos, "ref": ref, "idx_ref": idx_ref, "idx_pos": idx_pos, "lattice": lattice,
            "paths": tuple(paths)}


def rmsd_cases():
    return [rmsd_case(kind, N, K, B) for kind in RMSD_KINDS for N in RMSD_NS for K in RMSD_KS for B in RMSD_BS]


def ndiff(a, b):
    """number of differing elements of two integer arrays; a difference in length counts element by element"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape == b.shape:
        return int((a != b).sum())
    m = min(a.shape[-1], b.shape[-1])
    return int((a[..., :m] != b[..., :m]).sum()) + abs(a.size - b.size)
