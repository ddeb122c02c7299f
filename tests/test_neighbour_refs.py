"""CPU checks of the references and case tables in tests/neighbour_helpers.py, which tests/test_gpu_neighbours.py holds the neighbour-search,
edge-geometry and RMSD kernels to.  Nothing here runs a kernel:

  * the float32 references reproduce the five edge lists of g15_featurise_1a0q.npz, which the reference project produced (the kNN lists
    and the tight cutoff list as identical arrays; the 15.0 / 24 and 5.0 / 8 cutoff lists, whose order within a capped centre the
    reference takes from cdist's matmul distances, with the same shape and an empty symmetric difference);
  * on every lattice case the integer and the float32 references agree exactly;
  * every path of the kernels is hit by the cases, counted from the references alone; the counts are pinned, so that an edit of a case
    cannot silently lose a path;
  * each deliberate mistake of neighbour_helpers.MUTATIONS changes the expected output of at least one GPU case (counts pinned too);
  * torch's own fp32 evaluation of the unit vector and the smear meets the bounds the kernel is held to."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import neighbour_helpers as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_featurise_1a0q.npz")


@functools.lru_cache(maxsize=None)
def _input(kind, n):
    return H.graph_input(kind, n)


@functools.lru_cache(maxsize=None)
def _radius_cases():
    return H.radius_cases()


@functools.lru_cache(maxsize=None)
def _rmsd():
    return [(c, H.symm_rmsd_ref64(c["pos"], c["ref"], c["idx_ref"], c["idx_pos"])) for c in H.rmsd_cases()]


def _radius_ref(c, mut=None):
    return H.radius_batched_ref_f32(c["x"], c["y"], c["r"], c["xptr"], c["ybatch"], c["cap"], c["drop_self"], c["cutoff"], mut=mut)


def test_float32_references_reproduce_the_golden_edge_lists():
    z = np.load(GOLD)
    assert np.array_equal(H.knn_ref_f32(z["rec_pos"], 24), z["knn_rec_edge_index"])
    assert np.array_equal(H.knn_ref_f32(z["atom_pos"], 8), z["knn_atom_edge_index"])
    for name, pos, cutoff, cap in (("cut_rec_edge_index", "rec_pos", 15.0, 24), ("cut_atom_edge_index", "atom_pos", 5.0, 8),
                                   ("tight_rec_edge_index", "rec_pos", 4.2, 3)):
        got, want = H.cutoff_ref_f32(z[pos], cutoff, cap), z[name]
        assert got.shape == want.shape and not (set(map(tuple, got.T.tolist())) ^ set(map(tuple, want.T.tolist()))), name
    assert np.array_equal(H.cutoff_ref_f32(z["rec_pos"], 4.2, 3), z["tight_rec_edge_index"])


def test_integer_and_float32_references_agree_on_every_lattice_case():
    checked = 0
    for kind, n in H.graph_inputs():
        if kind not in H.LATTICE_KINDS:
            continue
        pos, _ = _input(kind, n)
        for k in H.knn_ks(n):
            assert np.array_equal(H.knn_ref_f32(pos, k), H.knn_ref_int(pos, k)), (kind, n, k)
        for cutoff, cap in H.cutoff_settings(n):
            assert np.array_equal(H.cutoff_ref_f32(pos, cutoff, cap), H.cutoff_ref_int(pos, cutoff, cap)), (kind, n, cutoff, cap)
        checked += 1
    for c in _radius_cases():
        if c["lattice"]:
            cf, ef = _radius_ref(c)
            ci, ei = H.radius_batched_ref_int(c["x"], c["y"], c["r"], c["xptr"], c["ybatch"], c["cap"], c["drop_self"], c["cutoff"])
            assert np.array_equal(cf, ci) and np.array_equal(ef, ei), c["id"]
            checked += 1
    assert checked == 45 + 24 + 12
    # degenerate sizes
    one = np.zeros((1, 3), np.float32)
    assert H.knn_ref_f32(one, 3).shape == (2, 0) and H.cutoff_ref_f32(one, 1.0, 3).shape == (2, 0) and H.cutoff_ref_int(one, 1.0, 3).shape == (2, 0)
    with pytest.raises(AssertionError):
        H.knn_ref_int(np.float32([[0.1, 0, 0], [0, 0, 0]]), 1)                       # off the lattice: refused, not silently wrong


def test_all_in_radius_cases_follow_the_closed_form():
    """min(cap, size), less one when drop_self is set and the query's own rank is at most cap"""
    seen = 0
    for c in _radius_cases():
        if c["all_in"]:
            counts, edges = _radius_ref(c)
            for q, want in H.all_in_expected(c).items():
                assert counts[q] == want, (c["id"], q)
                seen += 1
            assert counts.sum() == edges.shape[1]
    assert seen == 6 * (129 + 4)


# exact counts from the references: centres (kNN, cutoff graph), queries (batched search), cases (geometry), poses (RMSD)
PATHS = {
    "knn": {"coincident": 3260, "key_zero": 3142, "second_chunk": 10006, "tie_at_k": 4022, "tie_inside": 10516},
    "cutoff": {"at_cutoff": 2971, "equal": 4939, "many": 5215, "many_tie": 3475, "n1": 1, "n2": 25, "none": 5495, "plus1": 1651, "under": 3870},
    "radius": {"cap_after_boundary": 505, "cap_at_boundary": 297, "capped": 5720, "early_exit": 4933, "empty_graph": 54, "full_scan": 4680,
               "none_kept": 330, "self_beyond_cap": 3777, "self_within_cap": 6441},
    "geometry": {"cases": 300, "partial_block": 240, "second_pass": 120, "zero_edge": 260},
    "rmsd": {"argmin_not_first_row": 212, "poses": 576, "second_pass": 192, "tie_at_minimum": 246, "tie_between_different_rows": 90, "zero": 146},
}


def _sum(dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out[k] = out.get(k, 0) + int(v)
    return out


def test_every_path_is_hit_and_the_counts_are_pinned():
    got = {}
    per_case = []
    for kind, n in H.graph_inputs():
        pos, names = _input(kind, n)
        kp = _sum(H.knn_paths(pos, k) for k in H.knn_ks(n))
        cp = _sum(H.cutoff_paths(pos, cutoff, cap) for cutoff, cap in H.cutoff_settings(n))
        per_case.append(((kind, n), names, {**cp, **kp}))
        got["knn"] = _sum([got.get("knn", {}), kp])
        got["cutoff"] = _sum([got.get("cutoff", {}), cp])
    got["cutoff"] = _sum([got["cutoff"], H.cutoff_paths(np.zeros((1, 3), np.float32), 1.0, 3)])
    for c in _radius_cases():
        rp = H.radius_paths(c)
        per_case.append((c["id"], c["paths"], rp))
        got["radius"] = _sum([got.get("radius", {}), rp])
    geo = [c for E in H.GEOM_ES for K in H.GEOM_KS for c in H.geometry_cases(E, K)]
    got["geometry"] = _sum({p: 1 for p in c["paths"]} for c in geo)
    got["geometry"]["cases"] = len(geo)
    rm = {"poses": 0, "tie_at_minimum": 0, "tie_between_different_rows": 0, "zero": 0, "second_pass": 0, "argmin_not_first_row": 0}
    for c, (val, arg, S) in _rmsd():
        B = S.shape[0]
        rm["poses"] += B
        rm["second_pass"] += B * (c["pos"].shape[1] > 64)
        rm["zero"] += int((val == 0).sum())
        rm["argmin_not_first_row"] += int((arg > 0).sum())
        if c["lattice"]:
            tied = S == S.min(1, keepdims=True)
            rm["tie_at_minimum"] += int((tied.sum(1) > 1).sum())
            for b in np.flatnonzero(tied.sum(1) > 1):
                rows = np.flatnonzero(tied[b])
                order = np.argsort(c["idx_ref"][rows[0]])
                rm["tie_between_different_rows"] += any(
                    not np.array_equal(c["idx_pos"][r][np.argsort(c["idx_ref"][r])], c["idx_pos"][rows[0]][order]) for r in rows[1:])
    got["rmsd"] = rm
    for fam in PATHS:
        print(fam, dict(sorted(got[fam].items())))
    # a case hits every path it names
    for cid, names, counts in per_case:
        for name in names:
            assert counts.get(name, 0) >= 1, (cid, name, counts)
    for fam, want in PATHS.items():
        assert got[fam] == want, (fam, got[fam])
        assert all(v >= 1 for v in want.values()), fam


DISCRIMINATION = {"tie_high": 315500, "le": 130272, "d2_vs_cutoff": 885707, "keep_centre": 1218423, "switch_lt": 378273, "rank_no_self": 307605,
                  "nearest_cap": 197637, "no_first": 139716, "last_min": 282, "mu_shift": 337019}


def _mutation_counts():
    """per mutation: how many elements of the expected outputs of the GPU cases change (edge lists, counts, argmin; for mu_shift the smear
    elements that leave the bound)"""
    out = dict.fromkeys(H.MUTATIONS, 0)
    knn_muts, cut_muts = ("tie_high", "keep_centre", "no_first"), ("tie_high", "le", "d2_vs_cutoff", "keep_centre", "switch_lt", "no_first")
    for kind, n in H.graph_inputs():
        pos, _ = _input(kind, n)
        for k in H.knn_ks(n):
            base = H.knn_ref_f32(pos, k)
            for m in knn_muts:
                out[m] += H.ndiff(base, H.knn_ref_f32(pos, k, mut=m))
        for cutoff, cap in H.cutoff_settings(n):
            base = H.cutoff_ref_f32(pos, cutoff, cap)
            for m in cut_muts:
                out[m] += H.ndiff(base, H.cutoff_ref_f32(pos, cutoff, cap, mut=m))
    for c in _radius_cases():
        cb, eb = _radius_ref(c)
        for m in ("rank_no_self", "nearest_cap"):
            cm, em = _radius_ref(c, mut=m)
            out[m] += H.ndiff(cb, cm) + H.ndiff(eb, em)
    for c, (_, arg, _) in _rmsd():
        out["last_min"] += H.ndiff(arg, H.symm_rmsd_ref64(c["pos"], c["ref"], c["idx_ref"], c["idx_pos"], mut="last_min")[1])
    for E in H.GEOM_ES:
        for K in H.GEOM_KS:
            for c in H.geometry_cases(E, K):
                ref = H.edge_geometry_ref64(c["pos_a"], c["pos_b"], c["idx_a"], c["idx_b"], c["offset"], c["coeff"])
                bad = H.edge_geometry_ref64(c["pos_a"], c["pos_b"], c["idx_a"], c["idx_b"], c["offset"], c["coeff"], mut="mu_shift")
                out["mu_shift"] += int((np.abs(bad["smear"] - ref["smear"]) > ref["smear_bound"]).sum())
    return out


def test_each_deliberate_mistake_changes_a_gpu_case():
    got = _mutation_counts()
    for m in H.MUTATIONS:
        print(f"{m:14s} {got[m]:8d} differing elements")
    assert all(got[m] >= 1 for m in H.MUTATIONS), got
    assert got == DISCRIMINATION, got


def test_torch_fp32_meets_the_unit_and_smear_bounds():
    """the same formulas by torch in float32 on the CPU (F.normalize, exp(coeff (d - mu)^2)) against the float64 reference: ratio <= 1"""
    worst_u = worst_s = 0.0
    for E in H.GEOM_ES:
        for K in H.GEOM_KS:
            for c in H.geometry_cases(E, K):
                ref = H.edge_geometry_ref64(c["pos_a"], c["pos_b"], c["idx_a"], c["idx_b"], c["offset"], c["coeff"])
                vec = torch.from_numpy(ref["vec32"])
                exp = H.expansion_of(c)
                unit = torch.nn.functional.normalize(vec, dim=-1).numpy().astype(np.float64)
                smear = torch.exp(exp.coeff * torch.pow(vec.norm(dim=-1).view(-1, 1) - exp.offset.view(1, -1), 2)).numpy().astype(np.float64)
                assert (unit[ref["d"] == 0] == 0).all()
                worst_u = max(worst_u, float((np.abs(unit - ref["unit"]) / ref["unit_bound"]).max()))
                worst_s = max(worst_s, float((np.abs(smear - ref["smear"]) / ref["smear_bound"]).max()))
    print(f"torch fp32 on the CPU: unit {worst_u:.3f}, smear {worst_s:.3f} of the bound")
    assert worst_u <= 1.0 and worst_s <= 1.0


def test_rmsd_reference_on_the_lattice_is_exact_and_ties_go_to_the_first_row():
    for c, (val, arg, S) in _rmsd():
        if c["lattice"]:
            assert np.array_equal(S * 16, np.rint(S * 16)), c["id"]                # every S(k) is an integer / 16: exact in float64
        for b in range(S.shape[0]):
            assert arg[b] == min(np.flatnonzero(S[b] == S[b].min()))
        if "zero" in c["paths"]:
            assert (val == 0).all(), c["id"]
