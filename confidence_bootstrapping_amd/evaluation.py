"""Evaluation of sampled poses (reference inference.py:500-548 per complex, :593-885 aggregate).

`pose_metrics`: per-pose symmetry-corrected RMSD (GPU kernel `cbd_symm_rmsd` via molecules_utils), centroid distance and smallest
intra-ligand distance.  `performance_metrics`: the reference's aggregate dictionary -- same keys, same rounding, and the same
selection rules, including the reference's own inconsistencies (e.g. the `reversefiltered_*centroid*` / `*self_intersect*`
entries index with the DESCENDING confidence order, inference.py:782-785, 812-819) so that numbers are comparable run to run.
Table-driven instead of the reference's 290 unrolled lines.
`cluster_poses` / `cluster_poses_batch` (no reference counterpart): the distinct binding modes among the poses of a complex, on the host
and on the GPU (`cbd_pose_modes`).
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
