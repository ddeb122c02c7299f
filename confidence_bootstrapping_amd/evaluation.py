"""Evaluation of sampled poses (reference inference.py:500-548 per complex, :593-885 aggregate).

`pose_metrics`: per-pose symmetry-corrected RMSD (GPU kernel `cbd_symm_rmsd` via molecules_utils), centroid distance and smallest
intra-ligand distance.  `performance_metrics`: the reference's aggregate dictionary -- same keys, same rounding, and the same
selection rules, including the reference's own inconsistencies (e.g. the `reversefiltered_*centroid*` / `*self_intersect*`
entries index with the DESCENDING confidence order, inference.py:782-785, 812-819) so that numbers are comparable run to run.
Table-driven instead of the reference's 290 unrolled lines.
`cluster_poses` / `cluster_poses_batch` (no reference counterpart): the distinct binding modes among the poses of a complex, on the host
and on the GPU (`cbd_pose_modes`).
`pose_checks` / `pose_checks_batch` (no reference counterpart): is a pose physically possible -- bond lengths, 1-3 distances, internal and
receptor clashes, on the host and on the GPU (`cbd_pose_checks`).
"""
from __future__ import annotations

import numpy as np
import torch

from .molecules_utils import get_symmetry_rmsd


def pose_metrics(ligand_pos, orig_ligand_pos, mol=None, device=None):
    """ligand_pos [N, Nl, 3] (heavy atoms), orig_ligand_pos [Nl, 3] or [K, Nl, 3] reference pose(s), same frame.
    Returns (rmsd [N], centroid_distance [N], min_self_distance [N]) like inference.py:505-548."""
    lp = np.asarray(ligand_pos, dtype=np.float32)
    ref = np.asarray(orig_ligand_pos, dtype=np.float32)
    ref = ref[None] if ref.ndim == 2 else ref
    if mol is not None:
        try:
            rmsd = np.min(np.asarray([get_symmetry_rmsd(mol, r, [l for l in lp], device=device) for r in ref]), axis=0)
        except Exception as e:
            print("Using non corrected RMSD because of the error:", e)
            mol = None
    if mol is None:
        rmsd = np.min(np.sqrt(((lp[None] - ref[:, None]) ** 2).sum(axis=3).mean(axis=2)), axis=0)
    centroid = np.min(np.linalg.norm(lp.mean(axis=1)[None] - ref.mean(axis=1)[:, None], axis=2), axis=0)
    t = torch.from_numpy(lp)
    d = torch.cdist(t, t)
    d = d + torch.diag_embed(torch.full((lp.shape[1],), float("inf")))[None]
    return rmsd, centroid, d.flatten(1).min(dim=1).values.numpy()


METRICS_MAX_ATOMS, METRICS_MAX_REF_ATOMS = 512, 4096      # capacity of cbd_pose_metrics per complex: N and Q * N (include/cbdock.h)


def _iso_for_item(i, n, mol, given=None):
    """(key, entry) of item i's isomorphisms for n atoms: `given` (idx1, idx2) as it is (not cached), else the cache entry of `mol`, else --
    mol None, or an enumeration that raised, after the line the host route prints -- the identity mapping (K = 1)."""
    from . import molecules_utils as mu
    key = entry = None
    if given is not None:
        idx1, idx2 = (np.ascontiguousarray(np.asarray(x, dtype=np.int32)) for x in given)
        if idx1.ndim != 2 or idx1.shape != idx2.shape or idx1.shape[0] < 1 or idx1.shape[1] != n:
            raise ValueError(f"item {i}: isomorphism tables {idx1.shape} / {idx2.shape} for {n} atoms")
        entry = {"iso": (idx1, idx2), "exc": None, "dev": {}, "bytes": 0}
    elif mol is not None:
        try:
            key, entry = mu._iso_entry(*mu._graph_of(mol))
            if entry["exc"] is not None:
                raise entry["exc"][0](*entry["exc"][1])
            if entry["iso"][0].shape[1] != n:
                raise ValueError("coordinate / isomorphism shapes do not match")
        except Exception as e:
            print("Using non corrected RMSD because of the error:", e)
            key = entry = None
    if entry is None:
        key, entry = mu._identity_entry(n)
    return key, entry


def _prepare_metrics_items(items, isomorphisms=None):
    """Host half of pose_metrics_batch, no GPU: per item the fp32 arrays, the sizes and the isomorphism cache entry.
    `items`: (ligand_pos [P, N, 3], orig_pos [Q, N, 3] or [N, 3], mol or None); `isomorphisms`: optional list, one (idx1, idx2) or None per
    item, used as given instead of the cache.  mol None, or an enumeration that raised: the identity mapping (K = 1), after the line the
    host route prints.  -> list of dicts lp, ref, mol, P, N, Q, K, key, entry, fits."""
    out = []
    for i, (ligand_pos, orig_pos, mol) in enumerate(items):
        lp = np.ascontiguousarray(np.asarray(ligand_pos, dtype=np.float32))
        ref = np.asarray(orig_pos, dtype=np.float32)
        ref = np.ascontiguousarray(ref[None] if ref.ndim == 2 else ref)
        if lp.ndim != 3 or lp.shape[2] != 3 or ref.ndim != 3 or ref.shape[0] < 1 or ref.shape[1:] != lp.shape[1:]:
            raise ValueError(f"item {i}: poses {lp.shape} and crystal poses {ref.shape} do not match")
        n = lp.shape[1]
        key, entry = _iso_for_item(i, n, mol, isomorphisms[i] if isomorphisms is not None else None)
        out.append(dict(lp=lp, ref=ref, mol=mol, P=lp.shape[0], N=n, Q=ref.shape[0], K=entry["iso"][0].shape[0], key=key, entry=entry,
                        fits=1 <= n <= METRICS_MAX_ATOMS and ref.shape[0] * n <= METRICS_MAX_REF_ATOMS))
    return out


def _pack_pose_metrics(prepared):
    """The ragged batch cbd_pose_metrics reads, as host arrays, for prepared items that fit the kernel; one complex per item, its poses
    in order.  -> dict: pose_cplx [P], pose_ptr [P + 1], cplx_n, cplx_k, cplx_q [C], ref_ptr [C + 1] (int32; the ptr arrays count
    atoms), pos float32 [sum N over poses, 3], ref float32 [sum Q N, 3], idx_ref / idx_pos (lists of the C host tables [K, N]), max_n,
    max_ref."""
    from .staging import ptr
    cat = lambda arrays: np.concatenate([a.reshape(-1, 3) for a in arrays]) if arrays else np.zeros((0, 3), dtype=np.float32)
    return dict(
        pose_cplx=np.asarray([c for c, it in enumerate(prepared) for _ in range(it["P"])], dtype=np.int32),
        pose_ptr=ptr([it["N"] for it in prepared for _ in range(it["P"])]),
        cplx_n=np.asarray([it["N"] for it in prepared], dtype=np.int32), cplx_k=np.asarray([it["K"] for it in prepared], dtype=np.int32),
        cplx_q=np.asarray([it["Q"] for it in prepared], dtype=np.int32), ref_ptr=ptr([it["Q"] * it["N"] for it in prepared]),
        pos=cat([it["lp"] for it in prepared]), ref=cat([it["ref"] for it in prepared]),
        idx_ref=[it["entry"]["iso"][0] for it in prepared], idx_pos=[it["entry"]["iso"][1] for it in prepared],
        max_n=max((it["N"] for it in prepared), default=0), max_ref=max((it["Q"] * it["N"] for it in prepared), default=0))


def _pose_metrics_host(it, device):
    """an item over the kernel's capacity on the existing host route; that route does not report which crystal pose / isomorphism won (-1)"""
    rmsd, centroid, min_self = pose_metrics(it["lp"], it["ref"], it["mol"], device=device)
    none = np.full(it["P"], -1, dtype=np.int32)
    return (np.asarray(rmsd, dtype=np.float32), np.asarray(centroid, dtype=np.float32), np.asarray(min_self, dtype=np.float32), none, none.copy())


def pose_metrics_batch(items, device, isomorphisms=None):
    """pose_metrics for the poses of several complexes at once.  `items`: list of (ligand_pos [P, N, 3], orig_pos [Q, N, 3] or [N, 3],
    mol or None), heavy atoms, same frame.  -> per item (rmsd, centroid, min_self, argmin_ref, argmin_iso): float32 / int32 arrays [P].
    The isomorphisms come from the process-wide cache (molecules_utils.cached_isomorphisms' entries) and their index tables stay on the
    device between calls, in the same LRU; everything else goes into ONE pinned staging buffer: ONE upload, ONE cbd_pose_metrics launch
    on the current stream, ONE download.  rmsd is bitwise what get_symmetry_rmsd per crystal pose followed by np.min gives.  mol None, or
    a ligand whose enumeration raised: the identity mapping (K = 1, fp64 sums -- the host route's fp32 numpy fall-back can differ from it
    in the last bit).  An item over the kernel's capacity (N > 512 or Q * N > 4096) takes the host route (pose_metrics).  `isomorphisms`:
    optional list with one (idx1, idx2) or None per item, used as given (not cached).  There is no CPU path: `device` must be a GPU."""
    import ctypes as C
    from . import engine, staging, molecules_utils as mu
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("pose_metrics_batch measures the poses on the MI355X (cbd_pose_metrics); use pose_metrics on the host")
    lib = engine.load_library()
    prepared = _prepare_metrics_items(items, isomorphisms)
    empty = lambda: (np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    results = [None if it["fits"] and it["P"] else (_pose_metrics_host(it, dev) if it["P"] else empty()) for it in prepared]
    fit = [it for it, r in zip(prepared, results) if r is None]
    if not fit:
        return results
    pk = _pack_pose_metrics(fit)
    n_poses = len(pk["pose_cplx"])
    with torch.cuda.device(dev):
        tables = [mu._iso_device_tables(it["key"], it["entry"], dev) for it in fit]      # resident; uploaded only when first seen
        staged, at = staging.upload(dict(
            {k: pk[k] for k in ("pose_cplx", "pose_ptr", "cplx_n", "cplx_k", "cplx_q", "ref_ptr", "pos", "ref")},
            idx_ref_tab=np.asarray([t[0].data_ptr() for t in tables], dtype=np.uint64),
            idx_pos_tab=np.asarray([t[1].data_ptr() for t in tables], dtype=np.uint64)), dev)
        out = torch.empty(5, n_poses, dtype=torch.int32, device=dev)      # rmsd, centroid, min_self (fp32 bits), argmin_ref, argmin_iso
        row = lambda r: C.c_void_p(out.data_ptr() + 4 * r * n_poses)
        engine._check(lib.cbd_pose_metrics(
            n_poses, len(fit), int(pk["max_n"]), int(pk["max_ref"]), at("pose_cplx"), at("pose_ptr"), at("pos"), at("cplx_n"), at("cplx_k"),
            at("cplx_q"), at("ref_ptr"), at("ref"), at("idx_ref_tab"), at("idx_pos_tab"), row(0), row(1), row(2), row(3), row(4),
            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        got = out.cpu().numpy()      # the one download; it also orders `staged` and the index tables behind the kernel
    f32, p0 = got[:3].view(np.float32), 0
    fit_ids = [i for i, r in enumerate(results) if r is None]
    for i, it in zip(fit_ids, fit):
        p1 = p0 + it["P"]
        results[i] = (f32[0, p0:p1].copy(), f32[1, p0:p1].copy(), f32[2, p0:p1].copy(), got[3, p0:p1].copy(), got[4, p0:p1].copy())
        p0 = p1
    return results


MODES_MAX_ATOMS, MODES_MAX_POSES = 512, 256      # capacity of cbd_pose_modes per group: N and P (include/cbdock.h)


def pairwise_symmetry_rmsd(ligand_pos, idx1, idx2):
    """float32 [P, P]: for i < j  D[i, j] = float32(sqrt(min_k sum_a |x_i[idx1[k, a]] - x_j[idx2[k, a]]|^2 / N)), the sums in fp64 on the fp32
    coordinates; D[j, i] = D[i, j] from the same value, the diagonal 0; the row and the column (diagonal included) of a pose with a
    coordinate that is not finite are NaN.  The definition of cbd_pose_modes' matrix, on the host."""
    lp = np.asarray(ligand_pos, dtype=np.float32).astype(np.float64)
    P, N = lp.shape[:2]
    idx1, idx2 = np.asarray(idx1), np.asarray(idx2)
    best = np.full((P, P), np.inf)
    step = max(1, (1 << 22) // max(P * P * N * 3, 1))          # isomorphisms per pass: about 32 MB of differences
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(0, idx1.shape[0], step):
            a = lp[:, idx1[k:k + step]]                            # [P, k, N, 3]
            b = lp[:, idx2[k:k + step]]
            best = np.minimum(best, ((a[:, None] - b[None]) ** 2).sum(axis=(3, 4)).min(axis=2))
        d = np.sqrt(best / N).astype(np.float32)
    d = np.triu(d, 1)
    d = d + d.T
    bad = ~np.isfinite(lp).all(axis=(1, 2))
    d[bad, :] = np.nan
    d[:, bad] = np.nan
    return d


def modes_from_matrix(matrix, cutoff=2.0):
    """Leader clustering in rank order on a pose-against-pose matrix [P, P]: pose p joins the best-ranked existing head h with
    matrix[h, p] <= cutoff, else it becomes a head.  Only heads are compared against: a pose near a member but far from that member's head
    opens a new mode.  A pose whose diagonal entry is NaN gets -1 and is never a head.  -> (head int32 [P]: the index of the pose's head,
    mode int32 [P]: 0, 1, ... in order of appearance, n_modes)."""
    d = np.asarray(matrix, dtype=np.float64)
    P = d.shape[0]
    head, mode, heads = np.full(P, -1, dtype=np.int32), np.full(P, -1, dtype=np.int32), []
    for p in range(P):
        if np.isnan(d[p, p]):
            continue
        near = [m for m, h in enumerate(heads) if d[h, p] <= cutoff]
        if not near:
            heads.append(p)
            near = [len(heads) - 1]
        head[p], mode[p] = heads[near[0]], near[0]
    return head, mode, len(heads)


def cluster_poses(ligand_pos, mol=None, cutoff=2.0, isomorphisms=None):
    """Distinct binding modes among the poses of ONE complex, on the host (numpy fp64): `ligand_pos` [P, N, 3] heavy atoms IN RANK ORDER,
    in the receptor frame (no alignment); `mol` gives the graph isomorphisms (the process-wide cache; None, or an enumeration that raised:
    the identity mapping), `isomorphisms` = (idx1, idx2) is used as given.  -> (matrix float32 [P, P], head, mode int32 [P], n_modes) with
    the definitions of pairwise_symmetry_rmsd and modes_from_matrix -- those of cbd_pose_modes, for which this is the reference and the
    route of an item over its capacity."""
    lp = np.asarray(ligand_pos, dtype=np.float32)
    if lp.ndim != 3 or lp.shape[2] != 3:
        raise ValueError(f"poses {lp.shape}: expected [P, N, 3]")
    _, entry = _iso_for_item(0, lp.shape[1], mol, isomorphisms)
    matrix = pairwise_symmetry_rmsd(lp, *entry["iso"])
    return (matrix,) + modes_from_matrix(matrix, cutoff)


def _prepare_cluster_items(items, isomorphisms=None):
    """Host half of cluster_poses_batch, no GPU: per item (ligand_pos [P, N, 3], mol or None) the fp32 poses, the sizes and the
    isomorphism cache entry.  -> list of dicts lp, mol, P, N, K, key, entry, fits."""
    out = []
    for i, (ligand_pos, mol) in enumerate(items):
        lp = np.ascontiguousarray(np.asarray(ligand_pos, dtype=np.float32))
        if lp.ndim != 3 or lp.shape[2] != 3 or lp.shape[1] < 1:
            raise ValueError(f"item {i}: poses {lp.shape}: expected [P, N, 3]")
        key, entry = _iso_for_item(i, lp.shape[1], mol, isomorphisms[i] if isomorphisms is not None else None)
        out.append(dict(lp=lp, mol=mol, P=lp.shape[0], N=lp.shape[1], K=entry["iso"][0].shape[0], key=key, entry=entry,
                        fits=lp.shape[1] <= MODES_MAX_ATOMS and lp.shape[0] <= MODES_MAX_POSES))
    return out


def _pack_pose_modes(prepared, cutoff=2.0):
    """The ragged batch cbd_pose_modes reads, as host arrays, for prepared items that fit the kernel; one group per item.  -> dict: grp_n,
    grp_p, grp_k [G] int32, grp_cutoff [G] float64, pose_ptr, atom_ptr, mat_ptr [G + 1] int32 (prefix sums of P, P * N, P * P), pos
    float32 [sum P N, 3], idx_ref / idx_pos (lists of the G host tables [K, N]), max_n, max_p."""
    from .staging import ptr
    if sum(it["P"] * max(it["P"], it["N"]) for it in prepared) >= 2 ** 31:
        raise ValueError("cluster_poses_batch: the batch does not fit 32-bit offsets; split it")
    return dict(
        grp_n=np.asarray([it["N"] for it in prepared], dtype=np.int32), grp_p=np.asarray([it["P"] for it in prepared], dtype=np.int32),
        grp_k=np.asarray([it["K"] for it in prepared], dtype=np.int32), grp_cutoff=np.full(len(prepared), cutoff, dtype=np.float64),
        pose_ptr=ptr([it["P"] for it in prepared]), atom_ptr=ptr([it["P"] * it["N"] for it in prepared]),
        mat_ptr=ptr([it["P"] * it["P"] for it in prepared]),
        pos=np.concatenate([it["lp"].reshape(-1, 3) for it in prepared]) if prepared else np.zeros((0, 3), dtype=np.float32),
        idx_ref=[it["entry"]["iso"][0] for it in prepared], idx_pos=[it["entry"]["iso"][1] for it in prepared],
        max_n=max((it["N"] for it in prepared), default=0), max_p=max((it["P"] for it in prepared), default=0))


def cluster_poses_batch(items, device, cutoff=2.0, isomorphisms=None, return_matrix=False):
    """cluster_poses for the poses of several complexes at once.  `items`: list of (ligand_pos [P, N, 3] IN RANK ORDER, mol or None), heavy
    atoms, receptor frame.  -> per item (matrix float32 [P, P] or None, head, mode int32 [P], n_modes).  The isomorphisms come from the
    process-wide cache and their index tables stay on the device between calls, the same entries and the same LRU as pose_metrics_batch;
    everything else goes into ONE pinned staging buffer: ONE upload, ONE cbd_pose_modes call on the current stream (the pair kernel and the
    mode kernel behind it), ONE download, which holds the matrices only with `return_matrix`.  mol None, or a ligand whose enumeration
    raised: the identity mapping.  An item over the kernel's capacity (N > 512 or P > 256) takes the host route (cluster_poses).
    `isomorphisms`: optional list with one (idx1, idx2) or None per item, used as given (not cached).  There is no CPU path: `device` must
    be a GPU."""
    import ctypes as C
    from . import engine, staging, molecules_utils as mu
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("cluster_poses_batch groups the poses on the MI355X (cbd_pose_modes); use cluster_poses on the host")
    lib = engine.load_library()
    prepared = _prepare_cluster_items(items, isomorphisms)
    empty = lambda: (np.zeros((0, 0), np.float32) if return_matrix else None, np.zeros(0, np.int32), np.zeros(0, np.int32), 0)

    def host(it):
        matrix = pairwise_symmetry_rmsd(it["lp"], *it["entry"]["iso"])
        return (matrix if return_matrix else None,) + modes_from_matrix(matrix, cutoff)
    results = [None if it["fits"] and it["P"] else (host(it) if it["P"] else empty()) for it in prepared]
    fit = [it for it, r in zip(prepared, results) if r is None]
    if not fit:
        return results
    pk = _pack_pose_modes(fit, cutoff)
    G, n_poses, n_atoms, n_matrix = len(fit), int(pk["pose_ptr"][-1]), int(pk["atom_ptr"][-1]), int(pk["mat_ptr"][-1])
    with torch.cuda.device(dev):
        tables = [mu._iso_device_tables(it["key"], it["entry"], dev) for it in fit]      # resident; uploaded only when first seen
        staged, at = staging.upload(dict(
            {k: pk[k] for k in ("grp_cutoff", "grp_n", "grp_p", "grp_k", "pose_ptr", "atom_ptr", "mat_ptr", "pos")},
            idx_ref_tab=np.asarray([t[0].data_ptr() for t in tables], dtype=np.uint64),
            idx_pos_tab=np.asarray([t[1].data_ptr() for t in tables], dtype=np.uint64)), dev)
        small = 2 * n_poses + G
        out = torch.empty(small + n_matrix, dtype=torch.int32, device=dev)      # head, mode, n_modes, then the matrices (fp32 bits)
        part = lambda words: C.c_void_p(out.data_ptr() + 4 * words)
        engine._check(lib.cbd_pose_modes(
            G, int(pk["max_n"]), int(pk["max_p"]), n_poses, n_atoms, n_matrix, at("grp_n"), at("grp_p"), at("grp_k"), at("grp_cutoff"),
            at("pose_ptr"), at("atom_ptr"), at("mat_ptr"), at("pos"), at("idx_ref_tab"), at("idx_pos_tab"), part(small), part(0), part(n_poses),
            part(2 * n_poses), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        got = (out if return_matrix else out[:small]).cpu().numpy()      # the one download; it also orders `staged` and the tables behind the kernels
    fit_ids = [i for i, r in enumerate(results) if r is None]
    for g, (i, it) in enumerate(zip(fit_ids, fit)):
        p0, p1 = int(pk["pose_ptr"][g]), int(pk["pose_ptr"][g + 1])
        matrix = None
        if return_matrix:
            m0 = small + int(pk["mat_ptr"][g])
            matrix = got[m0:m0 + it["P"] ** 2].view(np.float32).reshape(it["P"], it["P"]).copy()
        results[i] = (matrix, got[p0:p1].copy(), got[n_poses + p0:n_poses + p1].copy(), int(got[2 * n_poses + g]))
    return results


CHECKS_MAX_ATOMS = 256      # capacity of cbd_pose_checks per ligand (include/cbdock.h)
CHECK_BAD_BOND, CHECK_BAD_ANGLE, CHECK_INTERNAL_CLASH, CHECK_REC_CLASH = 1, 2, 4, 8
CHECK_NO_TABLES, CHECK_NO_RECEPTOR, CHECK_BAD_COORD, CHECK_BAD_TABLE = 16, 32, 64, 128
CHECK_FAILED = CHECK_BAD_BOND | CHECK_BAD_ANGLE | CHECK_INTERNAL_CLASH | CHECK_REC_CLASH | CHECK_BAD_COORD | CHECK_BAD_TABLE
CHECK_THRESHOLDS = dict(bond_tol=0.25, angle_tol=0.25, clash_tol=0.30, rec_scale=0.75)      # the PoseBusters choices: DESIGN.md section 9
DEFAULT_RADIUS = 2.0          # Angstrom, for an element conformer_embedding._VDW does not list
CHECK_FLOATS = ("bond_lo", "bond_hi", "angle_lo", "angle_hi", "clash_ratio", "rec_ratio", "rec_dist")      # the rows of cbd_pose_checks' output, in order
CHECK_INTS = ("n_bad_bond", "n_bad_angle", "n_internal_clash", "n_rec_clash", "rec_lig_atom", "rec_atom", "flags")
PoseChecks = __import__("collections").namedtuple("PoseChecks", ("valid",) + CHECK_FLOATS + CHECK_INTS)
PoseChecks.__doc__ = """[P] arrays per pose: valid (bool: no check that ran failed), seven float32 and seven int32 (evaluation.pose_checks)"""


def _check_thresholds(thresholds):
    """the four thresholds as the kernel holds them: fp32 -> (bond_tol, angle_tol, clash_tol, rec_scale) as np.float32"""
    unknown = set(thresholds) - set(CHECK_THRESHOLDS)
    if unknown:
        raise TypeError(f"unknown threshold(s) {sorted(unknown)}: expected {sorted(CHECK_THRESHOLDS)}")
    t = {k: np.float32(thresholds.get(k, v)) for k, v in CHECK_THRESHOLDS.items()}
    if not all(0 <= t[k] < 1 for k in ("bond_tol", "angle_tol", "clash_tol")) or not (t["rec_scale"] > 0 and np.isfinite(t["rec_scale"])):
        raise ValueError(f"thresholds {t}: the three tolerances lie in [0, 1), rec_scale is positive")
    return t["bond_tol"], t["angle_tol"], t["clash_tol"], t["rec_scale"]


def _checks_from_rows(floats, ints):
    """float32 [7, P] and int32 [7, P] in the order of CHECK_FLOATS / CHECK_INTS -> PoseChecks"""
    return PoseChecks((ints[6] & CHECK_FAILED) == 0, *(np.ascontiguousarray(r) for r in floats), *(np.ascontiguousarray(r) for r in ints))


def pose_checks(ligand_pos, tables=None, receptor=None, **thresholds):
    """Is a pose physically possible?  Four distance checks in the style of PoseBusters on the poses of ONE complex, on the host (numpy
    fp64): the definition of cbd_pose_checks and the route of a ligand over its capacity.
    `ligand_pos` [P, N, 3] heavy atoms (fp32); `tables` = (lower, upper, kind, lig_radius) from ligand_check_tables -- lower / upper fp32
    [N, N], kind uint8 [N, N] (1 a bond, 2 a 1-3 pair, 0 any other pair; symmetric, only i < j is read), lig_radius fp32 [N]; the first
    three may be None (no internal checks), the whole may be None (then every ligand atom gets carbon's radius, 1.7 A); `receptor` =
    (rec_pos [A, 3], rec_radius [A]) in the frame of the poses, or None.  Thresholds (held as fp32): bond_tol = angle_tol = 0.25,
    clash_tol = 0.30, rec_scale = 0.75.
    Distances are sqrt(dx*dx + dy*dy + dz*dz) in fp64 on the fp32 coordinates; sums of radii and threshold products fp64 on the fp32 values;
    every float is rounded to fp32 once.  Per pose over the pairs i < j:
      kind 1: n_bad_bond counts d < (1 - bond_tol) lower or d > (1 + bond_tol) upper; bond_lo = min d / lower, bond_hi = max d / upper;
      kind 2: n_bad_angle, angle_lo, angle_hi, the same with angle_tol;
      kind 0: n_internal_clash counts d < (1 - clash_tol) lower; clash_ratio = min d / lower;
    and over all N x A pairs, ratio = d / (r_i + r_a): n_rec_clash counts ratio < rec_scale; rec_ratio = min ratio at (rec_lig_atom,
    rec_atom), ties to the smaller ligand atom, then the smaller receptor atom; rec_dist = min d (not necessarily the same pair).
    A category without pairs: count 0, +inf for a minimum, -inf for a maximum.
    flags: 1 bad bond, 2 bad angle, 4 internal clash, 8 receptor clash, 16 internal checks not evaluated (no tables), 32 receptor checks
    not evaluated (no receptor, or one without atoms), 64 a coordinate of the pose or of the receptor that is not finite, 128 a malformed
    table entry among i < j (not finite, lower <= 0, upper < lower, kind > 2) or, where the receptor checks run, a radius that is not
    finite and positive.  With 64 or 128 every float is NaN, every count and both atoms -1 and bits 1 to 8 are clear; with 16 the internal
    fields are NaN / -1, with 32 the receptor fields.  valid = none of 1, 2, 4, 8, 64, 128: a pose passes on the checks that ran.
    -> PoseChecks of [P] arrays."""
    bond_tol, angle_tol, clash_tol, rec_scale = (float(t) for t in _check_thresholds(thresholds))
    lp = np.asarray(ligand_pos, dtype=np.float32)
    if lp.ndim != 3 or lp.shape[2] != 3 or lp.shape[1] < 1:
        raise ValueError(f"poses {lp.shape}: expected [P, N, 3]")
    P, N = lp.shape[:2]
    lower, upper, kind, radius = tables if tables is not None else (None, None, None, None)
    radius = np.full(N, 1.7, dtype=np.float32) if radius is None else np.asarray(radius, dtype=np.float32)
    if radius.shape != (N,):
        raise ValueError(f"{radius.shape} ligand radii for {N} atoms")
    has_tab = lower is not None
    has_rec = receptor is not None and len(receptor[0]) > 0
    x = lp.astype(np.float64)
    floats, ints = np.full((7, P), np.nan, dtype=np.float32), np.full((7, P), -1, dtype=np.int32)
    flags = np.full(P, (0 if has_tab else CHECK_NO_TABLES) | (0 if has_rec else CHECK_NO_RECEPTOR), dtype=np.int32)
    flags[~np.isfinite(lp).all(axis=(1, 2))] |= CHECK_BAD_COORD
    if has_tab:
        lower, upper, kind = np.asarray(lower, dtype=np.float32), np.asarray(upper, dtype=np.float32), np.asarray(kind)
        if lower.shape != (N, N) or upper.shape != (N, N) or kind.shape != (N, N):
            raise ValueError(f"tables {lower.shape} / {upper.shape} / {kind.shape} for {N} atoms")
        i, j = np.triu_indices(N, 1)
        lo, up, kd = lower[i, j].astype(np.float64), upper[i, j].astype(np.float64), kind[i, j].astype(np.int64)
        with np.errstate(invalid="ignore"):
            if not (np.isfinite(lo) & np.isfinite(up) & (lo > 0) & (up >= lo) & (kd >= 0) & (kd <= 2)).all():
                flags |= CHECK_BAD_TABLE
    if has_rec:
        rec_pos, rec_radius = np.asarray(receptor[0], dtype=np.float32), np.asarray(receptor[1], dtype=np.float32)
        if rec_pos.ndim != 2 or rec_pos.shape[1] != 3 or rec_radius.shape != rec_pos.shape[:1]:
            raise ValueError(f"receptor {rec_pos.shape} / {rec_radius.shape}: expected [A, 3] and [A]")
        if not np.isfinite(rec_pos).all():
            flags |= CHECK_BAD_COORD
        if not all((np.isfinite(r) & (r > 0)).all() for r in (radius, rec_radius)):
            flags |= CHECK_BAD_TABLE
        y, radius_sum = rec_pos.astype(np.float64), radius.astype(np.float64)[:, None] + rec_radius.astype(np.float64)[None]
    for p in np.flatnonzero((flags & (CHECK_BAD_COORD | CHECK_BAD_TABLE)) == 0):
        if has_tab:
            dx, dy, dz = (x[p, i, a] - x[p, j, a] for a in range(3))
            d = np.sqrt(dx * dx + dy * dy + dz * dz)
            for k, (tol, n_row, lo_row, hi_row, bit) in enumerate(((clash_tol, 2, 4, None, CHECK_INTERNAL_CLASH), (bond_tol, 0, 0, 1, CHECK_BAD_BOND),
                                                                   (angle_tol, 1, 2, 3, CHECK_BAD_ANGLE))):
                m = kd == k
                bad = d[m] < (1.0 - tol) * lo[m]
                if hi_row is not None:
                    bad |= d[m] > (1.0 + tol) * up[m]
                    floats[hi_row, p] = (d[m] / up[m]).max(initial=-np.inf)
                floats[lo_row, p] = (d[m] / lo[m]).min(initial=np.inf)
                ints[n_row, p] = bad.sum()
                flags[p] |= bit if bad.any() else 0
        if has_rec:
            dx, dy, dz = (x[p, :, None, a] - y[None, :, a] for a in range(3))
            d = np.sqrt(dx * dx + dy * dy + dz * dz)
            ratio = d / radius_sum
            best = int(np.argmin(ratio))          # the first minimum in (ligand atom, receptor atom) order
            floats[5, p], floats[6, p] = ratio.flat[best], d.min()
            ints[3, p], ints[4, p], ints[5, p] = (ratio < rec_scale).sum(), best // ratio.shape[1], best % ratio.shape[1]
            flags[p] |= CHECK_REC_CLASH if ints[3, p] else 0
    ints[6] = flags
    return _checks_from_rows(floats, ints)


_CHECK_TABLES = __import__("collections").OrderedDict()      # key -> (lower, upper, kind, lig_radius)
_CHECK_TABLES_CFG = {"limit": 256}
_CHECK_TABLES_COUNT = {"hits": 0, "misses": 0}


def check_tables_cache_clear():
    _CHECK_TABLES.clear()
    _CHECK_TABLES_COUNT.update(hits=0, misses=0)


def check_tables_cache_stats():
    return {"entries": len(_CHECK_TABLES), **_CHECK_TABLES_COUNT}


def ligand_check_tables(mol, ref_pos=None):
    """What pose_checks needs of a ligand: (lower, upper fp32 [N, N], kind uint8 [N, N], lig_radius fp32 [N]) for its HEAVY atoms in their
    order (a molecule that carries hydrogens is stripped on a copy; the poses must be filtered likewise).  lower / upper: the
    triangle-smoothed matrices of conformer_embedding.distance_bounds(mol, ref_pos if given else mol.pos) -- the pose only settles which side
    of a double bond and which hand of a centre the 1-4 bounds describe; kind from the bond graph: topological distance 1 -> 1, 2 -> 2,
    3 and more (or another fragment) -> 0; lig_radius: conformer_embedding._VDW, DEFAULT_RADIUS = 2.0 A for an element it does not list.  The
    molecule is perceived (on a copy) if it is not.  When distance_bounds refuses the ligand -- more than 256 atoms, an element outside its
    bond-length table, an object that is only a graph (atomicnums / adjacency_matrix) -- the three tables are None and the radii are still
    returned.  Cached per ligand in a small LRU keyed on the graph as the isomorphism cache is (molecules_utils.isomorphism_key), plus bond
    orders, charges and the pose; check_tables_cache_clear() empties it."""
    import copy
    import hashlib
    from . import molecules_utils as mu
    from .datasets import conformer_embedding as ce, molfile
    nums, adjacency = mu._graph_of(mol)
    is_mol = isinstance(mol, molfile.Mol)
    if ref_pos is None and is_mol and len(mol.pos) == len(nums):
        ref_pos = mol.pos
    heavy = np.asarray(nums) != 1
    ref = None if ref_pos is None else np.ascontiguousarray(np.asarray(ref_pos, dtype=np.float64))
    if ref is not None and len(ref) == len(heavy):
        ref = np.ascontiguousarray(ref[heavy])
    h = hashlib.blake2b(digest_size=20)
    h.update(mu.isomorphism_key(nums, adjacency).encode())
    if is_mol:
        h.update(np.asarray([(b.a, b.b, b.type) for b in mol.bonds], dtype=np.int64).tobytes())
        h.update(np.asarray([a.charge for a in mol.atoms], dtype=np.int64).tobytes())
        h.update(b"-" if ref is None else ref.tobytes())
    key = h.hexdigest()
    hit = _CHECK_TABLES.get(key)
    if hit is not None:
        _CHECK_TABLES.move_to_end(key)
        _CHECK_TABLES_COUNT["hits"] += 1
        return hit
    _CHECK_TABLES_COUNT["misses"] += 1
    radius = np.asarray([ce._VDW.get(int(z), DEFAULT_RADIUS) for z in np.asarray(nums)[heavy]], dtype=np.float32)
    lower = upper = kind = None
    if is_mol:
        try:
            work = copy.deepcopy(mol)
            if not heavy.all():
                work = molfile.remove_hs(work)
            if not work.perceived:
                molfile.perceive(work)
            if work.GetNumAtoms() != len(radius):
                raise ValueError("hydrogens that RemoveHs keeps")
            lo64, up64, _ = ce.distance_bounds(work, ref if ref is not None and ref.shape == (len(radius), 3) else None)
            n = len(radius)
            am = np.asarray(work.adjacency_matrix) != 0
            two = (am.astype(np.int64) @ am.astype(np.int64)) > 0
            kind = np.where(am, 1, np.where(two, 2, 0)).astype(np.uint8)
            kind[np.arange(n), np.arange(n)] = 0
            lower, upper = lo64.astype(np.float32), up64.astype(np.float32)
        except (ValueError, KeyError) as e:
            print("pose checks: no internal checks for this ligand:", e)
            lower = upper = kind = None
    out = (lower, upper, kind, radius)
    _CHECK_TABLES[key] = out
    while len(_CHECK_TABLES) > _CHECK_TABLES_CFG["limit"]:
        _CHECK_TABLES.popitem(last=False)
    return out


def receptor_check_atoms(graph):
    """(rec_pos fp32 [A, 3], rec_radius fp32 [A]) of a complex's all-atom graph: graph['atom'].pos (the graph's frame: centred on
    original_center) and conformer_embedding._VDW of the atomic number behind graph['atom'].x[:, 1]
    (process_mols.allowable_features['possible_atomic_num_list']); the 'misc' entry and an element _VDW does not list get DEFAULT_RADIUS =
    2.0 A.  None when the graph has no 'atom' store.  Protein heavy atoms only: the graph holds neither hydrogens nor waters nor cofactors."""
    from .datasets import conformer_embedding as ce
    from .datasets.process_mols import allowable_features
    if graph is None or "atom" not in graph or getattr(graph["atom"], "pos", None) is None:
        return None
    cpu = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    store = graph["atom"]
    table = np.asarray([ce._VDW.get(z, DEFAULT_RADIUS) if isinstance(z, int) else DEFAULT_RADIUS
                        for z in allowable_features["possible_atomic_num_list"]], dtype=np.float32)
    index = np.clip(cpu(store.x)[:, 1].astype(np.int64), 0, len(table) - 1)
    return np.ascontiguousarray(cpu(store.pos), dtype=np.float32).reshape(-1, 3), table[index]


def _prepare_check_items(items):
    """Host half of pose_checks_batch, no GPU: per item (ligand_pos [P, N, 3], mol or (lower, upper, kind, lig_radius) or None, (rec_pos,
    rec_radius) or None) the fp32 arrays and sizes.  -> list of dicts lp, P, N, tables (the 4-tuple pose_checks takes), receptor (fp32
    pair or None), rec_key (the identity of the item's rec_pos object, None without atoms), fits."""
    out = []
    for k, (ligand_pos, ligand, receptor) in enumerate(items):
        lp = np.ascontiguousarray(np.asarray(ligand_pos, dtype=np.float32))
        if lp.ndim != 3 or lp.shape[2] != 3 or lp.shape[1] < 1:
            raise ValueError(f"item {k}: poses {lp.shape}: expected [P, N, 3]")
        n = lp.shape[1]
        if ligand is None:
            tables = (None, None, None, np.full(n, 1.7, dtype=np.float32))
        elif isinstance(ligand, (tuple, list)):
            tables = tuple(ligand)
        else:
            tables = ligand_check_tables(ligand)
        lower, upper, kind, radius = tables
        radius = np.ascontiguousarray(np.asarray(radius, dtype=np.float32))
        if radius.shape != (n,):
            raise ValueError(f"item {k}: {radius.shape} ligand radii for {n} atoms")
        if lower is not None:
            lower, upper, kind = np.asarray(lower, dtype=np.float32), np.asarray(upper, dtype=np.float32), np.asarray(kind).astype(np.uint8)
            if lower.shape != (n, n) or upper.shape != (n, n) or kind.shape != (n, n):
                raise ValueError(f"item {k}: tables {lower.shape} / {upper.shape} / {kind.shape} for {n} atoms")
        rec, rec_key = None, None
        if receptor is not None and len(receptor[0]) > 0:
            rec = (np.ascontiguousarray(np.asarray(receptor[0], dtype=np.float32)), np.ascontiguousarray(np.asarray(receptor[1], dtype=np.float32)))
            if rec[0].ndim != 2 or rec[0].shape[1] != 3 or rec[1].shape != rec[0].shape[:1]:
                raise ValueError(f"item {k}: receptor {rec[0].shape} / {rec[1].shape}: expected [A, 3] and [A]")
            rec_key = id(receptor[0])
        out.append(dict(lp=lp, P=lp.shape[0], N=n, tables=(lower, upper, kind, radius), receptor=rec, rec_key=rec_key, fits=n <= CHECKS_MAX_ATOMS))
    return out


def _pack_pose_checks(prepared):
    """The ragged batch cbd_pose_checks reads, as host arrays, for prepared items that fit the kernel; one complex per item, its poses in
    order; items with the same rec_key share one receptor.  -> dict: pose_cplx [P], pose_ptr [P + 1] (atoms), pos fp32 [sum N, 3],
    lig_radius fp32 [sum N] (one per atom of pos), cplx_n, cplx_rec (-1: none), cplx_tab (0 / 1) [C], tab_ptr [C + 1] (entries: N * N
    rounded up to a multiple of four for a complex with tables, else 0), bounds fp32 (per complex [N][N]: upper at i < j, lower at j < i, the
    diagonal 0) and kind uint8 of tab_ptr[-1] entries each, kind_words = kind viewed as int32 (what the staging buffer takes), rec_ptr
    [R + 1] (atoms), rec fp32 [sum A, 4] = (x, y, z, radius), max_n, n_receptors."""
    from .staging import ptr
    rec_ids, recs, cplx_rec = {}, [], []
    for it in prepared:
        if it["rec_key"] is None:
            cplx_rec.append(-1)
            continue
        if it["rec_key"] not in rec_ids:
            rec_ids[it["rec_key"]] = len(recs)
            recs.append(np.concatenate([it["receptor"][0], it["receptor"][1][:, None]], axis=1))
        cplx_rec.append(rec_ids[it["rec_key"]])
    sizes = [((it["N"] ** 2 + 3) & ~3) if it["tables"][0] is not None else 0 for it in prepared]
    if sum(sizes) >= 2 ** 31 or sum(it["P"] * it["N"] for it in prepared) >= 2 ** 31 or sum(len(r) for r in recs) >= 2 ** 31:
        raise ValueError("pose_checks_batch: the batch does not fit 32-bit offsets; split it")
    tab_ptr = ptr(sizes)
    bounds, kind = np.zeros(int(tab_ptr[-1]), dtype=np.float32), np.zeros(int(tab_ptr[-1]), dtype=np.uint8)
    for t0, it in zip(tab_ptr[:-1], prepared):
        lower, upper, kd, _ = it["tables"]
        if lower is not None:
            n = it["N"]
            bounds[t0:t0 + n * n] = (np.triu(upper, 1) + np.tril(lower, -1)).reshape(-1)
            kind[t0:t0 + n * n] = kd.reshape(-1)
    return dict(
        pose_cplx=np.asarray([c for c, it in enumerate(prepared) for _ in range(it["P"])], dtype=np.int32),
        pose_ptr=ptr([it["N"] for it in prepared for _ in range(it["P"])]),
        pos=np.concatenate([it["lp"].reshape(-1, 3) for it in prepared]) if prepared else np.zeros((0, 3), dtype=np.float32),
        lig_radius=np.concatenate([np.tile(it["tables"][3], it["P"]) for it in prepared]) if prepared else np.zeros(0, dtype=np.float32),
        cplx_n=np.asarray([it["N"] for it in prepared], dtype=np.int32), cplx_rec=np.asarray(cplx_rec, dtype=np.int32),
        cplx_tab=np.asarray([int(s > 0) for s in sizes], dtype=np.int32), tab_ptr=tab_ptr, bounds=bounds, kind=kind, kind_words=kind.view(np.int32),
        rec_ptr=ptr([len(r) for r in recs]), rec=np.concatenate(recs) if recs else np.zeros((0, 4), dtype=np.float32),
        max_n=max((it["N"] for it in prepared), default=0), n_receptors=len(recs))


def pose_checks_batch(items, device, **thresholds):
    """pose_checks for the poses of several complexes at once.  `items`: list of (ligand_pos [P, N, 3] heavy atoms, mol or (lower, upper,
    kind, lig_radius) or None, (rec_pos [A, 3], rec_radius [A]) in the frame of the poses or None) -> per item a PoseChecks of [P] arrays.  A
    mol goes through ligand_check_tables (cached); None: no internal checks and carbon's radius for every atom.  Items that hold the SAME
    rec_pos array object share one receptor entry: a screening run of many ligands against one receptor uploads it once.  Everything goes
    into ONE pinned staging buffer: ONE upload, ONE cbd_pose_checks launch on the current stream, ONE download.  An item with N > 256 takes
    the host route (pose_checks).  Thresholds as pose_checks.  There is no CPU path: `device` must be a GPU."""
    import ctypes as C
    from . import engine, staging
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("pose_checks_batch checks the poses on the MI355X (cbd_pose_checks); use pose_checks on the host")
    tols = _check_thresholds(thresholds)
    lib = engine.load_library()
    prepared = _prepare_check_items(items)
    empty = lambda: _checks_from_rows(np.zeros((7, 0), np.float32), np.zeros((7, 0), np.int32))
    results = [None if it["fits"] and it["P"] else (pose_checks(it["lp"], it["tables"], it["receptor"], **thresholds) if it["P"] else empty())
               for it in prepared]
    fit = [it for it, r in zip(prepared, results) if r is None]
    if not fit:
        return results
    pk = _pack_pose_checks(fit)
    n_poses = len(pk["pose_cplx"])
    with torch.cuda.device(dev):
        # rec first: with no 8-byte part in front of it, it starts at the buffer's base, aligned for the kernel's 16-byte loads
        staged, at = staging.upload({k: pk[k] for k in ("rec", "pose_cplx", "pose_ptr", "pos", "lig_radius", "cplx_n", "cplx_rec", "cplx_tab",
                                                        "tab_ptr", "bounds", "kind_words", "rec_ptr")}, dev)
        out = torch.empty(14, n_poses, dtype=torch.int32, device=dev)
        engine._check(lib.cbd_pose_checks(
            n_poses, len(fit), int(pk["n_receptors"]), int(pk["max_n"]), at("pose_cplx"), at("pose_ptr"), at("pos"), at("lig_radius"), at("cplx_n"),
            at("cplx_rec"), at("cplx_tab"), at("tab_ptr"), at("bounds"), at("kind_words"), at("rec_ptr"), at("rec"), *(C.c_float(float(t)) for t in tols),
            C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        got = out.cpu().numpy()      # the one download; it also orders `staged` behind the kernel
    p0 = 0
    for i in [i for i, r in enumerate(results) if r is None]:
        p1 = p0 + prepared[i]["P"]
        results[i] = _checks_from_rows(got[:7, p0:p1].view(np.float32), got[7:, p0:p1])
        p0 = p1
    return results


def _block(prefix, rmsd, centroid, self_dist=None):
    """the reference's standard group of entries for one selection of poses (one value per complex)"""
    pct = lambda a, thr: (100 * (a < thr).sum() / len(a)).__round__(2)
    out = {}
    if self_dist is not None:
        out[f"{prefix}self_intersect_fraction"] = pct(self_dist, 0.4)
    out.update({f"{prefix}rmsds_below_2": pct(rmsd, 2), f"{prefix}rmsds_below_5": pct(rmsd, 5)})
    out.update({f"{prefix}rmsds_percentile_{q}": np.percentile(rmsd, q).round(2) for q in (25, 50, 75)})
    out.update({f"{prefix}centroid_below_2": pct(centroid, 2), f"{prefix}centroid_below_5": pct(centroid, 5)})
    out.update({f"{prefix}centroid_percentile_{q}": np.percentile(centroid, q).round(2) for q in (25, 50, 75)})
    return out


def performance_metrics(rmsds, centroid_distances, min_self_distances, confidences=None, run_times=None, without_rec_overlap=None):
    """Aggregate metrics over complexes.  rmsds / centroid_distances / min_self_distances / confidences: [C, N] (N poses per
    complex, in sampling order); without_rec_overlap: optional [C] bool -> the `no_overlap_` copy of every entry."""
    R, Cd, S = (np.asarray(x, dtype=np.float64) for x in (rmsds, centroid_distances, min_self_distances))
    conf = None if confidences is None else np.asarray(confidences, dtype=np.float64)
    rt = np.asarray(run_times if run_times is not None else [0.0], dtype=np.float64)
    out = {}
    for overlap in ("", "no_overlap_"):
        if overlap:
            if without_rec_overlap is None or np.asarray(without_rec_overlap, dtype=bool).sum() == 0:
                continue
            m = np.asarray(without_rec_overlap, dtype=bool)
            r, c, s, cf = R[m], Cd[m], S[m], (None if conf is None else conf[m])
        else:
            r, c, s, cf = R, Cd, S, conf
        n_c, N = r.shape
        rows = np.arange(n_c)[:, None]
        out.update({f"{overlap}run_times_std": rt.std().__round__(2), f"{overlap}run_times_mean": rt.mean().__round__(2),
                    f"{overlap}mean_rmsd": r.mean(),
                    f"{overlap}rmsds_below_2": (100 * (r < 2).sum() / len(r) / N), f"{overlap}rmsds_below_5": (100 * (r < 5).sum() / len(r) / N)})
        out.update({f"{overlap}rmsds_percentile_{q}": np.percentile(r, q).round(2) for q in (25, 50, 75)})
        out.update({f"{overlap}min_rmsds_below_2": (100 * (np.min(r, axis=1) < 2).sum() / len(r)),
                    f"{overlap}min_rmsds_below_5": (100 * (np.min(r, axis=1) < 5).sum() / len(r)),
                    f"{overlap}mean_centroid": c.mean().__round__(2),
                    f"{overlap}centroid_below_2": (100 * (c < 2).sum() / len(c) / N).__round__(2),
                    f"{overlap}centroid_below_5": (100 * (c < 5).sum() / len(c) / N).__round__(2)})
        out.update({f"{overlap}centroid_percentile_{q}": np.percentile(c, q).round(2) for q in (25, 50, 75)})

        def best_of(order, k, r_order=None):
            """per complex: among the first k poses of `order`, the RMSD-best one (the RMSD values may come from another order:
            the reference's reverse-filtered entries take RMSDs from the ascending and everything else from the descending one)"""
            rr = r[rows, order][:, :k]
            pick = np.argsort(rr, axis=1)
            rm = np.min((r[rows, r_order] if r_order is not None else r[rows, order])[:, :k], axis=1)
            return rm, c[rows, order][:, :k][rows, pick][:, 0], s[rows, order][:, :k][rows, pick][:, 0]

        ident = np.tile(np.arange(N), (n_c, 1))
        for k in (5, 10):
            if N >= k:
                out.update(_block(f"{overlap}top{k}_", *best_of(ident, k)))
        if cf is not None:
            desc = np.argsort(cf, axis=1)[:, ::-1]
            asc = np.argsort(cf, axis=1)
            out.update(_block(f"{overlap}filtered_", r[rows, desc][:, 0], c[rows, desc][:, 0], s[rows, desc][:, 0]))
            for k in (5, 10):
                if N >= k:
                    rm, cc, _ = best_of(desc, k)
                    out.update(_block(f"{overlap}top{k}_filtered_", rm, cc))
            out.update(_block(f"{overlap}reversefiltered_", r[rows, asc][:, 0], c[rows, desc][:, 0], s[rows, desc][:, 0]))
            for k in (5, 10):
                if N >= k:
                    rm, cc, _ = best_of(desc, k, r_order=asc)
                    out.update(_block(f"{overlap}top{k}_reversefiltered_", rm, cc))
    return out
