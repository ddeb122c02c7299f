"""cbd_pose_modes (csrc/pose_cluster.hip) through evaluation.cluster_poses_batch: ONE ragged launch over the five ligands of
tests/metrics_helpers.py (1 to 12 graph isomorphisms, 5 to 130 atoms) with 1, 2, 8, 9, 17 and 40 poses each -- the diagonal tile alone, a
full tile, one pose past it, several tiles; the atom loop past 64 and 128.

On the grid inputs (tests/pose_mode_helpers.py) every fp64 sum is exact in any order, so the matrix is compared BITWISE with the rmsd the
existing route (evaluation.pose_metrics_batch) returns for pose j with pose i as its only crystal pose, and head / mode / n_modes with the
host reference evaluation.cluster_poses.  Off the grid the two routes add the same fp64 terms in different orders: each sum is within
N * 2^-53 of the exact one, relatively, far below half an fp32 ulp, so the two roundings to fp32 differ by one step at most -- a derived
bound, not a measured one.  The margin of the inputs (no pair within 1.0 A of the cutoff) is asserted on a brute-force fp64 matrix before
any device result is looked at."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.metrics_helpers import coords
from tests.pose_mode_helpers import CUTOFF, SIZES, assert_margin, brute_matrix, expected_modes, ligand_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CBD_ERR_CAPACITY = -4
FILL = 12345


def _same(a, b):
    """two results (matrix, head, mode, n_modes) bit for bit"""
    return (np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            and a[3] == b[3])


@pytest.fixture(scope="module")
def case():
    """the ragged batch, ONE launch over it (and a second one), the existing route for the 40-pose groups and the host reference"""
    import confidence_bootstrapping_amd.molecules_utils as mu
    from confidence_bootstrapping_amd.evaluation import cluster_poses, cluster_poses_batch, pose_metrics_batch
    dev = torch.device("cuda:0")
    mu.iso_cache_clear()
    ligands = ligand_cases()
    for name, mol, iso, lp, label in ligands:
        assert_margin(brute_matrix(lp, *iso), label)
    keys = [(name, p) for name, *_ in ligands for p in SIZES]
    items = [(lp[:p], mol) for _, mol, _, lp, _ in ligands for p in SIZES]
    got = cluster_poses_batch(items, dev, cutoff=CUTOFF, return_matrix=True)
    stats = mu.iso_cache_stats()
    again = cluster_poses_batch(items, dev, cutoff=CUTOFF, return_matrix=True)
    c = dict(dev=dev, ligands=ligands, keys=keys, items=items, got=dict(zip(keys, got)), again=dict(zip(keys, again)), stats=stats,
             stats_again=mu.iso_cache_stats())
    # pose i as the only crystal pose of all 40: one pose_metrics_batch launch for the five ligands
    rows = pose_metrics_batch([(lp, lp[i], mol) for _, mol, _, lp, _ in ligands for i in range(len(lp))], dev)
    c["existing"] = {name: np.stack([rows[40 * k + i][0] for i in range(40)]) for k, (name, *_) in enumerate(ligands)}
    c["host"] = {key: cluster_poses(lp, mol, cutoff=CUTOFF) for key, (lp, mol) in zip(keys, items)}
    return c


def test_matrix_is_bitwise_the_existing_routes_rmsd(case):
    for name, p in case["keys"]:
        matrix = case["got"][(name, p)][0]
        want = case["existing"][name][:p, :p]          # want[i, j]: pose j measured against pose i
        assert matrix.dtype == np.float32 and matrix.shape == (p, p)
        upper = np.triu_indices(p, 1)
        print(f"{name} P={p}: largest entry {matrix.max():.4f}, bits differing from the existing route {(matrix[upper].view(np.int32) != want[upper].view(np.int32)).sum()}")
        assert np.array_equal(matrix[upper].view(np.int32), want[upper].view(np.int32))
        assert np.array_equal(matrix.view(np.int32), matrix.T.view(np.int32)) and not matrix.diagonal().any()


def test_modes_equal_the_host_reference(case):
    for (name, p), (_, _, _, _, label) in zip(case["keys"], (lig for lig in case["ligands"] for _ in SIZES)):
        got, want = case["got"][(name, p)], case["host"][(name, p)]
        print(f"{name} P={p}: modes {got[3]} head {got[1].tolist()}")
        assert got[1].dtype == np.int32 and got[2].dtype == np.int32
        assert _same(got, want)
        assert (got[1].tolist(), got[2].tolist(), got[3]) == expected_modes(label[:p])
    assert case["got"][("ring6", 40)][3] == 5 and case["got"][("star7", 40)][3] == 5


def test_alone_in_the_batch_and_again_bitwise(case):
    from confidence_bootstrapping_amd.evaluation import cluster_poses_batch
    assert case["stats"]["entries"] == 5 and case["stats"]["misses"] == 5           # one enumeration per ligand, six groups each
    assert case["stats_again"]["misses"] == 5 and case["stats_again"]["bytes"] == case["stats"]["bytes"]          # resident tables, uploaded once
    for key in case["keys"]:
        assert _same(case["got"][key], case["again"][key])
    for key, item in zip(case["keys"], case["items"]):
        if key[1] in (9, 40):
            alone = cluster_poses_batch([item], case["dev"], cutoff=CUTOFF, return_matrix=True)[0]
            assert _same(alone, case["got"][key]), key
    # the matrix comes down only when asked for; the modes are the same
    plain = cluster_poses_batch(case["items"][:6], case["dev"], cutoff=CUTOFF)
    for key, r in zip(case["keys"][:6], plain):
        assert r[0] is None and np.array_equal(r[1], case["got"][key][1]) and np.array_equal(r[2], case["got"][key][2]) and r[3] == case["got"][key][3]


def test_off_the_grid_within_one_fp32_step_of_the_existing_route(case):
    from confidence_bootstrapping_amd.evaluation import cluster_poses_batch, pose_metrics_batch
    dev, p = case["dev"], 17
    rng = np.random.default_rng(91)
    poses = [(rng.normal(0.0, 2.0, size=(p, len(mol.atomicnums), 3)) + 30.0).astype(np.float32) for _, mol, *_ in case["ligands"]]
    got = cluster_poses_batch([(lp, mol) for lp, (_, mol, *_) in zip(poses, case["ligands"])], dev, return_matrix=True)
    rows = pose_metrics_batch([(lp, lp[i], mol) for lp, (_, mol, *_) in zip(poses, case["ligands"]) for i in range(p)], dev)
    upper = np.triu_indices(p, 1)
    for k, (name, *_) in enumerate(case["ligands"]):
        want = np.stack([rows[p * k + i][0] for i in range(p)])
        steps = np.abs(got[k][0][upper].view(np.int32).astype(np.int64) - want[upper].view(np.int32).astype(np.int64))
        print(f"{name}: entries that differ by one fp32 step {(steps == 1).sum()} of {len(steps)}, largest difference {steps.max()} steps")
        assert (got[k][0][upper] > 0).all() and steps.max() <= 1
        assert np.array_equal(got[k][0].view(np.int32), got[k][0].T.view(np.int32))


def test_poses_that_are_not_finite_get_minus_one(case):
    from confidence_bootstrapping_amd.evaluation import cluster_poses, cluster_poses_batch
    _, mol, _, lp, _ = case["ligands"][1]
    lp = lp[:17].copy()
    lp[0, 2, 1] = np.nan          # the best-ranked pose, in the first tile
    lp[8, 5, 0] = np.inf          # the first pose of the second tile
    lp[16, 0, 2] = -np.inf        # the only pose of the third
    got = cluster_poses_batch([(lp, mol)], case["dev"], return_matrix=True)[0]
    want = cluster_poses(lp, mol)
    print("head", got[1].tolist(), "mode", got[2].tolist())
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == want[3]
    for p in (0, 8, 16):
        assert got[1][p] == -1 and got[2][p] == -1 and np.isnan(got[0][p]).all() and np.isnan(got[0][:, p]).all()
    rest = [p for p in range(17) if p not in (0, 8, 16)]
    clean = case["got"][("ring6", 17)][0]
    assert np.array_equal(got[0][np.ix_(rest, rest)], clean[np.ix_(rest, rest)])          # the others are not disturbed


def _raw(lib, dev, max_n, max_p, grp_n, grp_p, grp_k, cutoff, pose_ptr, atom_ptr, mat_ptr, pos, tabs_ref, tabs_pos, n_poses=None, n_atoms=None,
         n_matrix=None):
    """cbd_pose_modes on arrays given as they are -> (rc, matrix bits int32, head, mode, n_modes), every output pre-filled with FILL"""
    t = lambda a, dt: torch.as_tensor(np.asarray(a, dtype=dt)).to(dev)
    G = len(grp_n)
    n_poses = int(pose_ptr[-1]) if n_poses is None else n_poses
    n_atoms = int(atom_ptr[-1]) if n_atoms is None else n_atoms
    n_matrix = int(mat_ptr[-1]) if n_matrix is None else n_matrix
    keep = [t(grp_n, np.int32), t(grp_p, np.int32), t(grp_k, np.int32), t(cutoff, np.float64), t(pose_ptr, np.int32), t(atom_ptr, np.int32),
            t(mat_ptr, np.int32), t(np.asarray(pos, dtype=np.float32).reshape(-1, 3), np.float32)]
    dev_tabs = [[None if a is None else t(a, np.int32) for a in tabs] for tabs in (tabs_ref, tabs_pos)]
    ptrs = [t(np.asarray([0 if d is None else d.data_ptr() for d in tabs], dtype=np.uint64).view(np.int64), np.int64) for tabs in dev_tabs]
    outs = [torch.full((max(n, 1),), FILL, dtype=torch.int32, device=dev) for n in (n_matrix, n_poses, n_poses, G)]
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = lib.cbd_pose_modes(G, max_n, max_p, n_poses, n_atoms, n_matrix, *[p(x) for x in keep], p(ptrs[0]), p(ptrs[1]), *[p(o) for o in outs],
                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    return (rc,) + tuple(o.cpu().numpy() for o in outs)


def test_a_contradictory_description_is_refused_without_indexing(case):
    from confidence_bootstrapping_amd import engine
    from confidence_bootstrapping_amd.staging import ptr
    dev, lib = case["dev"], engine.load_library()
    (_, _, ring_iso, ring_lp, _), (_, _, star_iso, star_lp, _) = case["ligands"][1], case["ligands"][2]
    bad_idx = ring_iso[1].copy()
    bad_idx[9, 4] = 6                                     # a table entry equal to N, in a mapping that wave 1 walks
    # groups: 0 ring6 good, 1 entry = N, 2 star7 good, 3 no table, 4 a P that contradicts the prefix arrays, 5 ring6 good again
    P = 9
    grp_n = [6, 6, 7, 6, 6, 6]
    grp_p = [P, P, P, P, P - 1, P]
    pos = np.concatenate([(star_lp if n == 7 else ring_lp)[:P].reshape(-1, 3) for n in grp_n])
    tabs_ref = [ring_iso[0], ring_iso[0], star_iso[0], None, ring_iso[0], ring_iso[0]]
    tabs_pos = [ring_iso[1], bad_idx, star_iso[1], ring_iso[1], ring_iso[1], ring_iso[1]]
    rc, matrix, head, mode, n_modes = _raw(lib, dev, 7, P, grp_n, grp_p, [12, 12, 6, 12, 12, 12], [CUTOFF] * 6, ptr([P] * 6),
                                           ptr([P * n for n in grp_n]), ptr([P * P] * 6), pos, tabs_ref, tabs_pos)
    assert rc == 0, lib.cbd_last_error().decode()
    print("n_modes", n_modes.tolist(), "head", head.reshape(6, P).tolist())
    assert n_modes.tolist() == [case["got"][("ring6", P)][3], -1, case["got"][("star7", P)][3], -1, -1, case["got"][("ring6", P)][3]]
    matrix, head, mode = matrix.view(np.float32).reshape(6, P, P), head.reshape(6, P), mode.reshape(6, P)
    for g in (1, 3, 4):
        assert np.isnan(matrix[g]).all() and (head[g] == -1).all() and (mode[g] == -1).all()
    for g, key in ((0, ("ring6", P)), (2, ("star7", P)), (5, ("ring6", P))):
        assert _same((matrix[g], head[g], mode[g], int(n_modes[g])), case["got"][key])          # the neighbours are not affected
    # prefix entries that point outside the outputs: the group is refused and nothing of it is written
    rc, matrix, head, mode, n_modes = _raw(lib, dev, 6, P, [6, 6], [P, P], [12, 12], [CUTOFF] * 2, [0, P, 2 * P + 5], [0, 6 * P, 12 * P],
                                           [0, P * P, 2 * P * P + 7], pos[:12 * P], [ring_iso[0]] * 2, [ring_iso[1]] * 2, n_poses=2 * P,
                                           n_atoms=12 * P, n_matrix=2 * P * P)
    assert rc == 0 and n_modes.tolist() == [case["got"][("ring6", P)][3], -1]
    assert (head[P:] == FILL).all() and (mode[P:] == FILL).all() and (matrix[P * P:] == FILL).all()
    assert np.array_equal(head[:P], case["got"][("ring6", P)][1])


def test_over_capacity_is_refused_and_takes_the_host_route(case):
    from confidence_bootstrapping_amd import engine
    from confidence_bootstrapping_amd.evaluation import cluster_poses, cluster_poses_batch
    dev, lib = case["dev"], engine.load_library()
    for n, p in ((513, 2), (3, 257)):
        ident = np.arange(n, dtype=np.int32)[None]
        rc, *outs = _raw(lib, dev, n, p, [n], [p], [1], [CUTOFF], [0, p], [0, p * n], [0, p * p], coords(n, p, 61), [ident], [ident])
        assert rc == CBD_ERR_CAPACITY and str(max(n, p)) in lib.cbd_last_error().decode()
        assert all((o == FILL).all() for o in outs)                                  # nothing launched or written
    assert lib.cbd_pose_modes(0, 0, 0, 0, 0, 0, *([None] * 15)) == 0                  # nothing to do, nothing launched
    # through the API: the large items come back with the host route's values, their neighbours with the device's
    big_n, big_p = coords(513, 3, 62), coords(3, 257, 63, spread=1.0)
    ring, star = case["items"][SIZES.index(9) + 6], case["items"][SIZES.index(9) + 12]
    got = cluster_poses_batch([ring, (big_n, None), (big_p, None), star], dev, return_matrix=True)
    assert _same(got[0], case["got"][("ring6", 9)]) and _same(got[3], case["got"][("star7", 9)])
    assert _same(got[1], cluster_poses(big_n, None)) and _same(got[2], cluster_poses(big_p, None))
    # at the capacity: 512 atoms (both tiles fill the 96 KB of LDS; nine poses: two tiles) and 256 poses (32 x 33 / 2 tile pairs)
    lp512, lp256 = coords(512, 9, 64, spread=0.25), coords(5, 256, 65, spread=0.7)
    got = cluster_poses_batch([(lp512, None), (lp256, case["ligands"][0][1])], dev, return_matrix=True)
    assert _same(got[0], cluster_poses(lp512, None)) and _same(got[1], cluster_poses(lp256, case["ligands"][0][1]))
    print("512 atoms: modes", got[0][3], "; 256 poses: modes", got[1][3])
    assert 1 <= got[0][3] <= 9 and 1 < got[1][3] < 256


def test_dock_front_door_writes_the_modes_and_nothing_else_changes(tmp_path):
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    from confidence_bootstrapping_amd.evaluation import cluster_poses
    from tools import dock
    D = os.path.join(HERE, "golden", "1a0q")
    base = ["--protein", os.path.join(D, "1a0q_protein_processed.pdb.gz"), "--ligand", os.path.join(D, "1a0q_ligand.sdf"), "--samples", "8",
            "--steps", "4"]
    plain, modes = str(tmp_path / "plain"), str(tmp_path / "modes")
    dock.main(base + ["--out", plain])
    dock.main(base + ["--out", modes, "--cluster-rmsd", "2.0"])
    tree = lambda d: {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
    before, after = tree(plain), tree(modes)
    extra = sorted(set(after) - set(before))
    assert {k: v for k, v in after.items() if k not in extra} == before          # the files of a run without the flag: bitwise unchanged
    assert "modes.csv" in extra and all(f == "modes.csv" or f.startswith("mode") for f in extra)
    ranked = sorted((f for f in after if f.startswith("rank") and "_confidence" in f), key=lambda f: int(f[4:f.index("_")]))
    assert len(ranked) == 8
    mols = [pm.read_molecule(os.path.join(modes, f)) for f in ranked]
    matrix, head, mode, n_modes = cluster_poses(np.stack([m.pos for m in mols]).astype(np.float32), mols[0], cutoff=2.0)
    off = matrix[np.triu_indices(8, 1)]
    print("modes", n_modes, "head", head.tolist(), "closest entry to the cutoff", float(np.abs(off - 2.0).min()))
    rows = [r.split(",") for r in after["modes.csv"].decode().splitlines()]
    assert rows[0] == ["mode", "head_rank", "population", "best_confidence", "mean_confidence"] and len(rows) == 1 + n_modes
    heads = sorted(set(head.tolist()))
    assert [int(r[0]) for r in rows[1:]] == list(range(1, n_modes + 1)) and [int(r[1]) for r in rows[1:]] == [h + 1 for h in heads]
    assert [int(r[2]) for r in rows[1:]] == np.bincount(mode, minlength=n_modes).tolist()
    for m, h in enumerate(heads):
        files = [f for f in extra if f.startswith(f"mode{m + 1}_rank{h + 1}_confidence")]
        assert len(files) == 1 and after[files[0]] == after[ranked[h]]
    assert len(extra) == 1 + n_modes
