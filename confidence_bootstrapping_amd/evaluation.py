"""Evaluation of sampled poses (reference inference.py:500-548 per complex, :593-885 aggregate).

`pose_metrics`: per-pose symmetry-corrected RMSD (GPU kernel `cbd_symm_rmsd` via molecules_utils), centroid distance and smallest
intra-ligand distance.  `performance_metrics`: the reference's aggregate dictionary -- same keys, same rounding, and the same
selection rules, including the reference's own inconsistencies (e.g. the `reversefiltered_*centroid*` / `*self_intersect*`
entries index with the DESCENDING confidence order, inference.py:782-785, 812-819) so that numbers are comparable run to run.
Table-driven instead of the reference's 290 unrolled lines.
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


def _prepare_metrics_items(items, isomorphisms=None):
    """Host half of pose_metrics_batch, no GPU: per item the fp32 arrays, the sizes and the isomorphism cache entry.
    `items`: (ligand_pos [P, N, 3], orig_pos [Q, N, 3] or [N, 3], mol or None); `isomorphisms`: optional list, one (idx1, idx2) or None per
    item, used as given instead of the cache.  mol None, or an enumeration that raised: the identity mapping (K = 1), after the line the
    host route prints.  -> list of dicts lp, ref, mol, P, N, Q, K, key, entry, fits."""
    from . import molecules_utils as mu
    out = []
    for i, (ligand_pos, orig_pos, mol) in enumerate(items):
        lp = np.ascontiguousarray(np.asarray(ligand_pos, dtype=np.float32))
        ref = np.asarray(orig_pos, dtype=np.float32)
        ref = np.ascontiguousarray(ref[None] if ref.ndim == 2 else ref)
        if lp.ndim != 3 or lp.shape[2] != 3 or ref.ndim != 3 or ref.shape[0] < 1 or ref.shape[1:] != lp.shape[1:]:
            raise ValueError(f"item {i}: poses {lp.shape} and crystal poses {ref.shape} do not match")
        n = lp.shape[1]
        given = isomorphisms[i] if isomorphisms is not None else None
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
