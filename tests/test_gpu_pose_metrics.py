"""cbd_pose_metrics (csrc/pose_metrics.hip) through evaluation.pose_metrics_batch: one launch over a ragged batch of ligands with 1, 2, 6
and 12 graph isomorphisms, 5 to 130 atoms, 1 / 3 / 8 poses and 1 / 2 crystal poses each (tests/metrics_helpers.py).

rmsd, argmin_ref and argmin_iso are compared EXACTLY with the existing route: get_symmetry_rmsd per crystal pose, then np.min / np.argmin.
centroid and min_self are compared with an fp64 numpy restatement; the bound is not a chosen number: it is 4 x the largest deviation of
the existing host computation (evaluation.pose_metrics: fp32 numpy and torch.cdist) from that same restatement on these same inputs.  The
tests print both sides' figures before they assert."""
import copy
import ctypes as C
from argparse import Namespace
from functools import partial

import numpy as np
import pytest
import torch

from tests.metrics_helpers import LIGANDS, coords, metrics64

pytestmark = pytest.mark.gpu
SHAPES = {"chain5": (1, 1), "ring6": (3, 2), "star7": (8, 1), "fork65": (3, 2), "fork130": (8, 2)}       # ligand -> (P, Q)
CBD_ERR_CAPACITY = -4


def _table_row(iso, perm):
    """which isomorphism of the table is the (idx1, idx2) pair symmetry_rmsd(return_permutation=True) reports"""
    hit = np.flatnonzero((iso[0] == np.asarray(perm[0])).all(axis=1) & (iso[1] == np.asarray(perm[1])).all(axis=1))
    assert len(hit) >= 1
    return int(hit[0])


def _existing_route(lp, ref, mol, dev, iso=None):
    """get_symmetry_rmsd (symmetry_rmsd) per crystal pose, then np.min / np.argmin -> rmsd float64 [P], argmin_ref, argmin_iso"""
    import confidence_bootstrapping_amd.molecules_utils as mu
    iso = mu.graph_isomorphisms(mol.atomicnums, mol.adjacency_matrix) if iso is None else iso
    per_ref, rows = [], []
    for r in ref:
        vals, perms = mu.symmetry_rmsd(r, [l for l in lp], mol.atomicnums, mol.adjacency_matrix, device=dev, return_permutation=True,
                                       isomorphisms=iso)
        per_ref.append(np.asarray(vals))
        rows.append([_table_row(iso, p) for p in perms])
    per_ref, rows = np.asarray(per_ref), np.asarray(rows)
    q = np.argmin(per_ref, axis=0)
    return np.min(per_ref, axis=0), q, rows[q, np.arange(len(lp))]


def _poses(mol, iso, p, q, seed):
    """q crystal poses (the second one a displaced copy) and p poses: a crystal pose under a random isomorphism plus noise, so that the
    identity mapping is not the best one"""
    rng = np.random.default_rng(seed)
    n = len(mol.atomicnums)
    ref = rng.normal(0.0, 4.0, size=(1, n, 3)).astype(np.float32)
    if q == 2:
        ref = np.concatenate([ref, ref + rng.normal(0.0, 0.7, size=(1, n, 3)).astype(np.float32)])
    lp = np.empty((p, n, 3), dtype=np.float32)
    for i in range(p):
        k = int(rng.integers(iso[0].shape[0]))
        lp[i, iso[1][k]] = ref[i % q][iso[0][k]]
        lp[i] += rng.normal(0.0, 0.05 + 0.5 * i, size=(n, 3)).astype(np.float32)
    return lp, ref


@pytest.fixture(scope="module")
def case():
    """the ragged batch, ONE device launch over it, the existing route and the fp64 restatement -- computed once"""
    import confidence_bootstrapping_amd.molecules_utils as mu
    from confidence_bootstrapping_amd.evaluation import pose_metrics, pose_metrics_batch
    dev = torch.device("cuda:0")
    mu.iso_cache_clear()
    mols = {name: make() for name, make, _ in LIGANDS}
    isos = {name: mu.graph_isomorphisms(m.atomicnums, m.adjacency_matrix) for name, m in mols.items()}
    items = []
    for s, (name, _, _) in enumerate(LIGANDS):
        lp, ref = _poses(mols[name], isos[name], *SHAPES[name], seed=300 + s)
        items.append((lp, ref, mols[name]))
    got = pose_metrics_batch(items, dev)
    stats = mu.iso_cache_stats()
    again = pose_metrics_batch(items, dev)          # warm: same entries, same resident tables
    c = dict(dev=dev, mols=mols, isos=isos, items=items, got=got, again=again, stats=stats, stats_again=mu.iso_cache_stats())
    c["existing"] = [_existing_route(lp, ref, mol, dev) for lp, ref, mol in items]
    c["ref64"] = [metrics64(lp, ref, *isos[name]) for (lp, ref, _), (name, _, _) in zip(items, LIGANDS)]
    c["host"] = [pose_metrics(lp, ref, None) for lp, ref, _ in items]          # centroid and min_self of the host route (its RMSD is not used)
    return c


def test_rmsd_is_bitwise_the_existing_routes(case):
    for (name, _, k), got, want in zip(LIGANDS, case["got"], case["existing"]):
        rmsd, _, _, q, iso = got
        print(f"{name}: K={k} rmsd device {rmsd.tolist()} existing {want[0].tolist()} q {q.tolist()} / {want[1].tolist()} k {iso.tolist()} / {want[2].tolist()}")
        assert rmsd.dtype == np.float32 and rmsd.shape == (SHAPES[name][0],)
        assert np.array_equal(rmsd.astype(np.float64), want[0])
        assert np.array_equal(q, want[1]) and np.array_equal(iso, want[2])
    # the symmetry correction mattered on these inputs: some pose is NOT best under the identity mapping
    assert any((got[4] != 0).any() for got in case["got"])
    # and the fp64 restatement agrees to fp32 rounding (a check of the restatement the other tests lean on)
    for got, r64 in zip(case["got"], case["ref64"]):
        assert np.allclose(got[0], r64[0], rtol=3e-7, atol=0)


def test_repeat_call_hits_the_cache_and_repeats_bitwise(case):
    assert case["stats"]["entries"] == 5 and case["stats"]["misses"] == 5 and case["stats"]["hits"] == 0
    assert case["stats_again"]["entries"] == 5 and case["stats_again"]["misses"] == 5 and case["stats_again"]["hits"] == 5
    assert case["stats_again"]["bytes"] == case["stats"]["bytes"]             # the device tables were uploaded once and counted once
    want = sum(256 + 4 * 4 * k * len(case["mols"][name].atomicnums) for name, _, k in LIGANDS)       # host + device copies of both tables
    assert case["stats"]["bytes"] == want
    for a, b in zip(case["got"], case["again"]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_centroid_and_min_self_within_4x_the_host_routes_deviation(case):
    dev_c = max(np.abs(h[1].astype(np.float64) - r[1]).max() for h, r in zip(case["host"], case["ref64"]))
    dev_s = max(np.abs(h[2].astype(np.float64) - r[2]).max() for h, r in zip(case["host"], case["ref64"]))
    err_c = max(np.abs(g[1].astype(np.float64) - r[1]).max() for g, r in zip(case["got"], case["ref64"]))
    err_s = max(np.abs(g[2].astype(np.float64) - r[2]).max() for g, r in zip(case["got"], case["ref64"]))
    print(f"centroid: host route vs fp64 {dev_c:.3e} A, device vs fp64 {err_c:.3e} A; min_self: host route vs fp64 {dev_s:.3e} A, device {err_s:.3e} A")
    assert dev_c > 0 and dev_s > 0
    assert err_c <= 4 * dev_c and err_s <= 4 * dev_s
    assert all(g[1].dtype == np.float32 and g[2].dtype == np.float32 for g in case["got"])


def test_ties_go_to_the_lowest_isomorphism_then_the_lowest_crystal_pose(case):
    from confidence_bootstrapping_amd.evaluation import pose_metrics_batch
    dev, ring, star = case["dev"], case["mols"]["ring6"], case["mols"]["star7"]
    iso_r, iso_s = case["isos"]["ring6"], case["isos"]["star7"]
    # (a) a ring pose equal to its crystal pose rotated by one position; the crystal pose repeats after three atoms, so that the
    #     rotations by -1 and by +2 BOTH give a sum of exactly zero
    tri = coords(3, 1, 41)[0]
    crystal = np.concatenate([tri, tri])
    rot1 = crystal[(np.arange(6) + 1) % 6]
    # (b) all six ring atoms of the pose in one point: all twelve mappings give exactly the same sum (the coordinates are on a 1/64 grid)
    point = np.tile(coords(1, 1, 42)[0], (6, 1))
    ring_ref = coords(6, 1, 43)
    # (c) two fluorines of the pose coincide: the mappings tie in pairs
    star_ref = coords(7, 1, 44)
    twin = coords(7, 2, 45)
    twin[:, 5] = twin[:, 4]
    # (d) a pose equally far from two crystal poses, for every mapping: crystal poses pose + d and pose - d
    mid = coords(7, 1, 46)[0]
    d = coords(7, 1, 47, spread=0.5)[0]
    two = np.stack([mid + d, mid - d])
    items = [(rot1[None], crystal[None], ring), (np.stack([point, ring_ref[0]]), ring_ref, ring), (twin, star_ref, star), (mid[None], two, star),
             (mid[None], two[::-1].copy(), star)]
    got = pose_metrics_batch(items, dev)
    for (lp, ref, mol), g, iso in zip(items, got, (iso_r, iso_r, iso_s, iso_s, iso_s)):
        want = _existing_route(lp, ref, mol, dev, iso)
        r64 = metrics64(lp, ref, *iso)
        print("tie case: device", [x.tolist() for x in (g[0], g[3], g[4])], "existing", [x.tolist() for x in want], "fp64 first minimum", r64[3].tolist(), r64[4].tolist())
        assert np.array_equal(g[0].astype(np.float64), want[0]) and np.array_equal(g[3], want[1]) and np.array_equal(g[4], want[2])
        assert np.array_equal(g[3], r64[3]) and np.array_equal(g[4], r64[4])            # exact ties: the fp64 first minimum is the same choice
    S = lambda lp, ref, iso: ((ref[iso[0]].astype(np.float64) - lp[iso[1]].astype(np.float64)) ** 2).sum(axis=(1, 2))
    s = S(rot1, crystal, iso_r)
    assert (s == 0).sum() == 2 and got[0][0][0] == 0.0 and got[0][4][0] == np.flatnonzero(s == 0)[0]
    assert len(set(S(point, ring_ref[0], iso_r).tolist())) == 1 and got[1][4][0] == 0
    s = S(twin[0], star_ref[0], iso_s)
    assert (s == s.min()).sum() == 2 and got[2][4][0] == np.flatnonzero(s == s.min())[0]
    assert got[3][3][0] == 0 and got[4][3][0] == 0 and got[3][0][0] == got[4][0][0]


def test_isomorphism_counts_that_do_not_fill_the_four_waves(case):
    from confidence_bootstrapping_amd.evaluation import pose_metrics_batch
    dev, ring = case["dev"], case["mols"]["ring6"]
    full = case["isos"]["ring6"]
    lp, ref, _ = case["items"][1]
    for k in (7, 1, 2, 3, 5):
        cut = (full[0][-k:].copy(), full[1][-k:].copy())          # the LAST k mappings: the identity (k = 0 of the full table) is not among them
        got = pose_metrics_batch([(lp, ref, ring)], dev, isomorphisms=[cut])[0]
        want = _existing_route(lp, ref, ring, dev, cut)
        print(f"K={k}: device {got[0].tolist()} {got[3].tolist()} {got[4].tolist()} existing {[x.tolist() for x in want]}")
        assert np.array_equal(got[0].astype(np.float64), want[0]) and np.array_equal(got[3], want[1]) and np.array_equal(got[4], want[2])
        assert got[4].max() < k
    # K = 1 through the cache (the chain) is part of the big launch; mol = None is the identity mapping: the plain RMSD, fp64 sums
    plain = pose_metrics_batch([(lp, ref, None)], dev)[0]
    ident = np.arange(6, dtype=np.int32)[None]
    want = _existing_route(lp, ref, ring, dev, (ident, ident))
    assert np.array_equal(plain[0].astype(np.float64), want[0]) and np.array_equal(plain[3], want[1]) and not plain[4].any()


def _raw(lib, dev, n_poses, n_cplx, max_n, max_ref, pose_cplx, pose_ptr, pos, cplx_n, cplx_k, cplx_q, ref_ptr, ref, tabs_ref, tabs_pos):
    """cbd_pose_metrics on arrays given as they are -> (rc, [5, n_poses] int32 host array or None)"""
    t = lambda a, dt: torch.as_tensor(np.asarray(a, dtype=dt)).to(dev)
    keep = [t(pose_cplx, np.int32), t(pose_ptr, np.int32), t(pos, np.float32), t(cplx_n, np.int32), t(cplx_k, np.int32), t(cplx_q, np.int32),
            t(ref_ptr, np.int32), t(ref, np.float32)]
    dev_tabs = [[None if a is None else t(a, np.int32) for a in tabs] for tabs in (tabs_ref, tabs_pos)]
    ptrs = [t(np.asarray([0 if d is None else d.data_ptr() for d in tabs], dtype=np.uint64).view(np.int64), np.int64) for tabs in dev_tabs]
    out = torch.full((5, max(n_poses, 1)), 12345, dtype=torch.int32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = lib.cbd_pose_metrics(n_poses, n_cplx, max_n, max_ref, *[p(x) for x in keep], p(ptrs[0]), p(ptrs[1]),
                              *[C.c_void_p(out.data_ptr() + 4 * r * out.shape[1]) for r in range(5)],
                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    return rc, out.cpu().numpy()


def test_over_capacity_is_refused_and_takes_the_host_route(case, capsys):
    from confidence_bootstrapping_amd import engine
    from confidence_bootstrapping_amd.evaluation import pose_metrics, pose_metrics_batch
    dev, lib = case["dev"], engine.load_library()
    n = 513
    big_lp, big_ref = coords(n, 2, 61), coords(n, 1, 62)
    ident = np.arange(n, dtype=np.int32)[None]
    rc, out = _raw(lib, dev, 1, 1, n, n, [0], [0, n], big_lp[0], [n], [1], [1], [0, n], big_ref[0], [ident], [ident])
    assert rc == CBD_ERR_CAPACITY and "513" in lib.cbd_last_error().decode() and (out == 12345).all()          # nothing launched or written
    rc, _ = _raw(lib, dev, 1, 1, 512, 4097, [0], [0, 512], big_lp[0, :512], [512], [1], [1], [0, 512], big_ref[0, :512], [ident[:, :512]], [ident[:, :512]])
    assert rc == CBD_ERR_CAPACITY
    assert lib.cbd_pose_metrics(0, 0, 0, 0, *([None] * 16)) == 0                                                # nothing to do, nothing launched
    # through the API: the large item comes back with the host route's values, its neighbours with the device's
    lp, ref, mol = case["items"][2]
    got = pose_metrics_batch([(lp, ref, mol), (big_lp, big_ref, None), (lp, ref, mol)], dev)
    want = pose_metrics(big_lp, big_ref, None, device=dev)
    assert all(np.array_equal(g, w.astype(np.float32)) for g, w in zip(got[1][:3], want)) and (got[1][3] == -1).all() and (got[1][4] == -1).all()
    for k in (0, 2):
        assert all(np.array_equal(x, y) for x, y in zip(got[k], case["got"][2]))
    # 512 atoms fit (the last atom sits in lane 63 of the eighth pass); 8 crystal poses of 512 atoms fill the LDS budget exactly
    lp512, ref512 = coords(512, 2, 63), coords(512, 8, 64)
    g = pose_metrics_batch([(lp512, ref512, None)], dev)[0]
    r64 = metrics64(lp512, ref512, ident[:, :512], ident[:, :512])
    assert np.allclose(g[0], r64[0], rtol=3e-7, atol=0) and np.array_equal(g[3], r64[3]) and np.allclose(g[2], r64[2], rtol=3e-7, atol=0)


def test_a_contradictory_description_gives_nan_for_that_pose_only(case):
    from confidence_bootstrapping_amd import engine
    dev, lib = case["dev"], engine.load_library()
    iso = case["isos"]["ring6"]
    lp, ref = coords(6, 8, 71), coords(6, 2, 72)
    bad_idx = iso[1].copy()
    bad_idx[9, 4] = 6                                     # one index past the last atom, in a mapping that wave 1 walks
    neg_idx = iso[0].copy()
    neg_idx[2, 0] = -1
    # complexes: 0 good (Q = 2), 1 index too large, 2 K = 0, 3 Q = 0, 4 negative index, 5 good (Q = 1), 6 no table, 7 N over max_n
    cplx_n = [6, 6, 6, 6, 6, 6, 6, 7]
    cplx_k = [12, 12, 0, 12, 12, 12, 12, 12]
    cplx_q = [2, 1, 1, 0, 1, 1, 1, 1]
    ref_ptr = np.concatenate([[0], np.cumsum([12, 6, 6, 0, 6, 6, 6, 6])])
    refs = np.concatenate([ref.reshape(-1, 3)] + [ref[0]] * 6)
    pose_cplx = [0, 1, 2, 3, 4, 5, 6, 7, 8, -1, 0]       # poses 8 and 9 name no complex; pose 10 is good again
    pose_ptr = np.arange(12) * 6
    pos = np.concatenate([lp.reshape(-1, 3), lp[:3].reshape(-1, 3)])
    tabs_ref = [iso[0], iso[0], iso[0], iso[0], neg_idx, iso[0], None, iso[0]]
    tabs_pos = [iso[1], bad_idx, iso[1], iso[1], iso[1], iso[1], iso[1], iso[1]]
    rc, out = _raw(lib, dev, 11, 8, 6, 12, pose_cplx, pose_ptr, pos, cplx_n, cplx_k, cplx_q, ref_ptr, refs, tabs_ref, tabs_pos)
    assert rc == 0, lib.cbd_last_error().decode()
    f = out[:3].view(np.float32)
    good = [0, 5, 10]
    bad = [p for p in range(11) if p not in good]
    print("rmsd", f[0].tolist(), "argmin_ref", out[3].tolist(), "argmin_iso", out[4].tolist())
    assert np.isnan(f[:, bad]).all() and (out[3:, bad] == -1).all()
    for p, (l, r) in zip(good, ((lp[0], ref), (lp[5], ref[:1]), (pos[60:66], ref))):
        r64 = metrics64(l[None], r, *iso)
        assert np.allclose(f[0, p], r64[0], rtol=3e-7, atol=0) and out[3, p] == r64[3][0] and out[4, p] == r64[4][0]
        assert np.allclose(f[1, p], r64[1], rtol=1e-6, atol=1e-6) and np.allclose(f[2, p], r64[2], rtol=1e-6, atol=0)


def test_summarize_inference_is_the_same_with_device_metrics_on_one_sampling_run(case, monkeypatch):
    """ONE inference_epoch (one sampling() run, two small synthetic complexes, confidence model) whose `results` are recorded on their way
    into summarize_inference; the helper then runs on that one list with device_metrics off and on."""
    import confidence_bootstrapping_amd.finetune_train as ft
    import confidence_bootstrapping_amd.evaluation as ev
    from confidence_bootstrapping_amd.synthetic import make_complex, add_atoms
    from confidence_bootstrapping_amd.utils import make_score_model, make_confidence_model, load_model_args
    from confidence_bootstrapping_amd.diffusion_utils import t_to_sigma
    dev = case["dev"]
    margs = load_model_args()
    model, _ = make_score_model(device=dev, seed=0, args=margs)
    conf_model, conf_args = make_confidence_model(device=dev, seed=5)
    targets = []
    for i in range(2):
        g = add_atoms(make_complex(Nl=9 + i, Nr=36 + 4 * i, R=1 + i % 2, knn=8, seed=40 + i, name=f"{i}abc_A_l{i}"), seed=40 + i)
        center = g.original_center.numpy()
        crystal = g["ligand"].pos.numpy() + center
        g["ligand"].orig_pos = crystal if i == 0 else np.stack([crystal + np.float32(1.5), crystal])          # Q = 1 and Q = 2
        nums = np.minimum(g["ligand"].x[:, 0].numpy() + 1, 118)
        g["ligand"].x[:, 0] = torch.from_numpy(nums)
        ei = g["ligand", "ligand"].edge_index.numpy()
        am = np.zeros((len(nums), len(nums)), dtype=int)
        am[ei[0], ei[1]] = 1
        g.mol = Namespace(atomicnums=nums, adjacency_matrix=am)
        targets.append(g)
    args = copy.copy(margs)
    args.__dict__.update(inference_steps=4, inference_samples=4, inference_batch_size=4)
    recorded, real = [], ft.summarize_inference

    def record(results, *a, **k):
        recorded.append((results, k))
        return real(results, *a, **k)
    monkeypatch.setattr(ft, "summarize_inference", record)
    torch.manual_seed(0); np.random.seed(0)
    first = ft.inference_epoch(model, conf_model, targets, None, dev, partial(t_to_sigma, args=margs), args, conf_args, confidence_cutoff=-1e9)
    monkeypatch.setattr(ft, "summarize_inference", real)
    assert len(recorded) == 1 and len(recorded[0][0]) == 2
    results, kw = recorded[0]
    launches = []
    batch = ev.pose_metrics_batch
    monkeypatch.setattr(ev, "pose_metrics_batch", lambda items, device, **k: launches.append(len(items)) or batch(items, device, **k))
    for extra in ({}, {"oracle_confidence": True}):
        cutoff = -1e9
        off, on = copy.copy(args), copy.copy(args)
        off.__dict__.update(device_metrics=False, **extra)
        on.__dict__.update(device_metrics=True, **extra)
        n0 = len(launches)
        a = real(results, off, conf_args, cutoff, dev, **kw)
        assert len(launches) == n0
        b = real(results, on, conf_args, cutoff, dev, **kw)
        assert launches[n0:] == [2]                                   # both complexes in ONE pose_metrics_batch call
        print("losses", a[0], "top_rmsds", a[2].tolist(), b[2].tolist(), "kept", len(a[1]), len(b[1]))
        assert a[0] == b[0] and np.array_equal(a[2], b[2]) and len(a[2]) == 2
        assert len(a[1]) == len(b[1]) and all(x[0] is y[0] and x[1] == y[1] for x, y in zip(a[1], b[1]))
        assert len(a[1]) == 8
        if not extra:
            assert a[0] == first[0] and np.array_equal(a[2], first[2])
