"""Host side of the pose checks (evaluation.pose_checks, the definition of cbd_pose_checks): against the brute-force restatement of
tests/pose_check_helpers.py on the generator cases and on the 1a0q fixture (crystal pose, a pose pushed into the receptor, a torsion scan);
the ligand tables and their cache, the receptor atoms, the packed ragged batch, summarize_inference's args.keep_valid on the CPU route and
the CSV writer.  No GPU: everything here is host code."""
import gzip
import os
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.pose_check_helpers import FLOATS, INTS, assert_same, brute_checks, expected, gpu_cases, line_case, random_case

HERE = os.path.dirname(os.path.abspath(__file__))
D = os.path.join(HERE, "golden", "1a0q")


@pytest.fixture(scope="module")
def generated():
    cases = gpu_cases()
    return cases, expected(cases)


@pytest.fixture(scope="module")
def fixture_1a0q(tmp_path_factory):
    """the ligand (heavy atoms, perceived), its tables, the receptor's heavy atoms through parse_pdb + receptor_check_atoms, all in the
    frame of the file"""
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    from confidence_bootstrapping_amd.evaluation import check_tables_cache_clear, ligand_check_tables, receptor_check_atoms
    check_tables_cache_clear()
    mol = pm.read_molecule(os.path.join(D, "1a0q_ligand.sdf"), sanitize=True, remove_hs=True)
    pdb = str(tmp_path_factory.mktemp("1a0q") / "protein.pdb")
    with gzip.open(os.path.join(D, "1a0q_protein_processed.pdb.gz"), "rb") as src, open(pdb, "wb") as dst:
        dst.write(src.read())
    parsed = pm.parse_pdb(pdb)
    pos, feats = [], []
    for res, coords in zip(parsed.seq, parsed.coords):
        pos.append(coords[~np.isnan(coords).any(axis=1)])
        feats.append(pm.get_moad_atom_feats(res, coords))
    graph = _Graph(None, center=torch.zeros(1, 3), atom=SimpleNamespace(pos=torch.from_numpy(np.concatenate(pos)).float(),
                                                                        x=torch.from_numpy(np.concatenate(feats)).long()))
    rec = receptor_check_atoms(graph)
    return SimpleNamespace(mol=mol, tables=ligand_check_tables(mol), rec=rec, graph=graph, crystal=mol.pos.astype(np.float32))


class _Graph:
    """what the pose checks, write_ranked_poses and summarize_inference read of a graph: g['ligand'], g['atom'] when it has one,
    g.original_center"""

    def __init__(self, pos, center=None, x=None, atom=None):
        self._stores = {"ligand": SimpleNamespace(pos=pos, x=x, orig_pos=None)}
        if atom is not None:
            self._stores["atom"] = atom
        self.original_center = center

    def __contains__(self, key):
        return key in self._stores

    def __getitem__(self, key):
        return self._stores[key]


def _rotate_about(pos, u, v, side, degrees):
    axis = (pos[v] - pos[u]) / np.linalg.norm(pos[v] - pos[u])
    t, out = np.radians(degrees), pos.copy()
    r = pos[side] - pos[v]
    out[side] = pos[v] + r * np.cos(t) + np.cross(axis, r) * np.sin(t) + axis * (r @ axis)[:, None] * (1 - np.cos(t))
    return out


def _torsion_scan(mol, pos, step=10):
    """-> [((u, v), degrees, pose)]: every single bond that is in no ring and ends in no terminal atom, turned through 360 degrees"""
    out = []
    for b in mol.bonds:
        u, v = b.a, b.b
        if b.type != 1 or len(mol.neighbors(u)) < 2 or len(mol.neighbors(v)) < 2:
            continue
        side, todo = {v}, [v]
        while todo:
            k = todo.pop()
            for j, _ in mol.neighbors(k):
                if j not in side and not (k == v and j == u):
                    side.add(j)
                    todo.append(j)
        if u in side:          # a ring bond
            continue
        side = sorted(side - {v})
        out += [((u, v), deg, _rotate_about(pos.astype(np.float64), u, v, side, deg).astype(np.float32)) for deg in range(step, 360, step)]
    return out


def test_host_function_equals_the_brute_force_on_the_generator_cases(generated):
    from confidence_bootstrapping_amd.evaluation import pose_checks
    cases, want = generated
    names = [c["name"] for c in cases]
    for case, w in zip(cases, want):
        got = pose_checks(case["lp"], case["tables"], case["receptor"])
        print(case["name"], "flags", got.flags.tolist(), "counts", got.n_bad_bond.tolist(), got.n_bad_angle.tolist(), got.n_internal_clash.tolist(),
              got.n_rec_clash.tolist(), "closest", got.rec_lig_atom.tolist(), got.rec_atom.tolist())
        assert_same(got, w, case["name"])
    by = dict(zip(names, want))
    # what the cases were built for, read off the brute force
    assert by["n1_a1000"]["flags"].tolist() in ([0], [8]) and by["n1_a1000"]["bond_lo"][0] == np.inf and by["n1_a1000"]["bond_hi"][0] == -np.inf
    assert by["n1_a1000"]["n_bad_bond"].tolist() == [0] and by["n1_a1000"]["clash_ratio"][0] == np.inf
    assert (by["n256_a0"]["flags"] & 32).all() and np.isnan(by["n256_a0"]["rec_ratio"]).all() and (by["n256_a0"]["rec_atom"] == -1).all()
    assert (by["no_tables_n20_a300"]["flags"] & 16).all() and (by["no_tables_n20_a300"]["n_bad_bond"] == -1).all()
    assert by["nan_pose"]["flags"][1] & 64 and not (by["nan_pose"]["flags"][[0, 2]] & 64).any() and by["nan_pose"]["n_rec_clash"][1] == -1
    assert (by["bad_lower"]["flags"] & 128).all() and not by["bad_lower"]["valid"].any() and np.isnan(by["bad_lower"]["rec_dist"]).all()
    assert (by["tie_rec_256_apart"]["rec_lig_atom"][0], by["tie_rec_256_apart"]["rec_atom"][0]) == (0, 44)
    assert (by["tie_rec_64_apart"]["rec_lig_atom"][0], by["tie_rec_64_apart"]["rec_atom"][0]) == (0, 71)
    assert (by["tie_rec_1_apart"]["rec_lig_atom"][0], by["tie_rec_1_apart"]["rec_atom"][0]) == (0, 199)
    assert (by["tie_lig_pair"]["rec_lig_atom"][0], by["tie_lig_pair"]["rec_atom"][0]) == (2, 0)
    assert (by["tie_cross_lanes"]["rec_lig_atom"][0], by["tie_cross_lanes"]["rec_atom"][0]) == (1, 300)
    assert (by["tie_cross_one_thread"]["rec_lig_atom"][0], by["tie_cross_one_thread"]["rec_atom"][0]) == (1, 301)
    counts = lambda n: [int(by[n][k][0]) for k in ("n_bad_bond", "n_bad_angle", "n_internal_clash", "n_rec_clash")]
    assert counts("all_pass") == [0, 0, 0, 0] and by["all_pass"]["valid"][0] and by["all_pass"]["flags"][0] == 0
    assert counts("bad_bond_only") == [1, 0, 0, 0] and by["bad_bond_only"]["flags"][0] == 1
    assert counts("bad_angle_only") == [0, 1, 0, 0] and by["bad_angle_only"]["flags"][0] == 2
    assert counts("internal_clash_only") == [0, 0, 1, 0] and by["internal_clash_only"]["flags"][0] == 4
    assert counts("rec_clash_only")[:3] == [0, 0, 0] and counts("rec_clash_only")[3] >= 1 and by["rec_clash_only"]["flags"][0] == 8


def test_thresholds_are_per_call_and_held_as_fp32():
    from confidence_bootstrapping_amd.evaluation import pose_checks
    case = line_case("loose", bond=(0, 1, 2.625, 2.875))
    tight = pose_checks(case["lp"], case["tables"], case["receptor"])
    loose = pose_checks(case["lp"], case["tables"], case["receptor"], bond_tol=0.5)          # 1.5 >= 0.5 * 2.625
    assert tight.n_bad_bond.tolist() == [1] and loose.n_bad_bond.tolist() == [0] and loose.valid.tolist() == [True]
    assert_same(loose, brute_checks(case["lp"], case["tables"], case["receptor"], bond_tol=0.5)[0])
    with pytest.raises(ValueError):
        pose_checks(case["lp"], case["tables"], case["receptor"], clash_tol=1.0)
    with pytest.raises(TypeError):
        pose_checks(case["lp"], case["tables"], case["receptor"], bond_tolerance=0.1)


def test_ligand_tables_of_1a0q_and_their_cache(fixture_1a0q):
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    from confidence_bootstrapping_amd.evaluation import check_tables_cache_clear, check_tables_cache_stats, ligand_check_tables
    lower, upper, kind, radius = fixture_1a0q.tables
    n = 23
    upper_triangle = np.triu_indices(n, 1)
    assert lower.shape == upper.shape == kind.shape == (n, n) and radius.shape == (n,)
    assert lower.dtype == upper.dtype == radius.dtype == np.float32 and kind.dtype == np.uint8
    assert [(kind[upper_triangle] == k).sum() for k in (1, 2, 0)] == [23, 30, 200]
    assert np.array_equal(kind, kind.T) and np.array_equal(lower, lower.T) and np.array_equal(upper, upper.T)
    assert (lower[upper_triangle] > 0).all() and (upper[upper_triangle] >= lower[upper_triangle]).all() and (radius >= 1.5).all()
    before = check_tables_cache_stats()
    again = ligand_check_tables(pm.read_molecule(os.path.join(D, "1a0q_ligand.sdf"), sanitize=True, remove_hs=True))      # an equal molecule
    after = check_tables_cache_stats()
    assert again[0] is lower and after["hits"] == before["hits"] + 1 and after["misses"] == before["misses"] and after["entries"] == before["entries"]
    # the file's hydrogens are stripped: the same heavy-atom tables; an object that is only a graph has no tables but its radii
    raw = pm.read_molecule(os.path.join(D, "1a0q_ligand.sdf"))
    assert np.array_equal(ligand_check_tables(raw)[2], kind) and len(ligand_check_tables(raw)[3]) == n
    bare = ligand_check_tables(Namespace(atomicnums=np.asarray([6, 8, 1, 26]), adjacency_matrix=np.zeros((4, 4), dtype=int)))
    assert bare[:3] == (None, None, None) and bare[3].tolist() == [np.float32(1.7), np.float32(1.55), np.float32(2.0)]      # iron: not in the table
    check_tables_cache_clear()
    assert check_tables_cache_stats() == {"entries": 0, "hits": 0, "misses": 0}


def test_receptor_atoms_of_1a0q(fixture_1a0q):
    from confidence_bootstrapping_amd.evaluation import receptor_check_atoms
    pos, radius = fixture_1a0q.rec
    assert pos.shape == (3181, 3) and pos.dtype == np.float32 and radius.shape == (3181,) and radius.dtype == np.float32
    assert set(np.unique(radius).tolist()) <= {np.float32(1.7), np.float32(1.6), np.float32(1.55), np.float32(1.8)}
    assert receptor_check_atoms(_Graph(None)) is None and receptor_check_atoms(None) is None
    misc = _Graph(None, atom=SimpleNamespace(pos=torch.zeros(2, 3), x=torch.tensor([[0, 118, 0, 0], [0, 25, 0, 0]])))      # 'misc' and iron
    assert receptor_check_atoms(misc)[1].tolist() == [2.0, 2.0]


def test_crystal_pose_of_1a0q_passes_and_a_pose_pushed_into_the_receptor_does_not(fixture_1a0q):
    from confidence_bootstrapping_amd.evaluation import pose_checks
    f = fixture_1a0q
    got = pose_checks(f.crystal[None], f.tables, f.rec)
    print({k: getattr(got, k).tolist() for k in FLOATS + INTS})
    assert got.valid.tolist() == [True] and got.flags.tolist() == [0]
    assert [got.n_bad_bond[0], got.n_bad_angle[0], got.n_internal_clash[0], got.n_rec_clash[0]] == [0, 0, 0, 0]
    assert 0.75 < got.rec_ratio[0] < 1.0 and got.bond_lo[0] > 0.75 and got.bond_hi[0] < 1.25 and got.clash_ratio[0] > 0.7
    assert_same(got, brute_checks(f.crystal[None], f.tables, f.rec)[0], "crystal")
    i, a = int(got.rec_lig_atom[0]), int(got.rec_atom[0])
    towards = f.rec[0][a] - f.crystal[i]
    pushed = (f.crystal + 1.5 * towards / np.linalg.norm(towards)).astype(np.float32)
    bad = pose_checks(pushed[None], f.tables, f.rec)
    print("pushed", bad.n_rec_clash.tolist(), bad.rec_ratio.tolist())
    assert bad.n_rec_clash[0] >= 1 and bad.valid.tolist() == [False] and bad.flags[0] & 8
    assert [bad.n_bad_bond[0], bad.n_bad_angle[0], bad.n_internal_clash[0]] == [0, 0, 0]          # a translation: the ligand itself is unchanged


def test_torsion_scan_of_1a0q_clashes_internally_and_keeps_bonds_and_angles(fixture_1a0q):
    from confidence_bootstrapping_amd.evaluation import pose_checks
    f = fixture_1a0q
    scan = _torsion_scan(f.mol, f.crystal)
    bonds = sorted({b for b, _, _ in scan})
    assert len(scan) == 35 * len(bonds) and (1, 2) in bonds and (0, 21) in bonds
    lp = np.stack([pose for _, _, pose in scan])
    got = pose_checks(lp, f.tables, None)
    want, margin, _ = brute_checks(lp, f.tables, None)
    assert margin > 1e-5, margin          # off the grid: checked, not constructed
    assert_same(got, want, "scan")
    worst = int(np.argmin(got.clash_ratio))
    print(f"{len(bonds)} bonds {bonds}; poses with an internal clash {(got.n_internal_clash > 0).sum()} of {len(scan)}; smallest d / lower "
          f"{got.clash_ratio[worst]:.3f} at bond {scan[worst][0]}, {scan[worst][1]} degrees")
    assert (got.n_internal_clash >= 1).any() and (got.flags & 32).all()
    assert (got.n_bad_bond == 0).all() and (got.n_bad_angle == 0).all()          # a torsion preserves bond lengths and 1-3 distances


def test_packing_layout_of_a_ragged_batch():
    from confidence_bootstrapping_amd.evaluation import _pack_pose_checks, _prepare_check_items
    a, b, c = random_case("a", 31, 3, 5, 2), random_case("b", 32, 2, 0, 1), random_case("c", 33, 5, 7, 3, tables=False)
    shared = a["receptor"]
    items = [(a["lp"], a["tables"], shared), (b["lp"], b["tables"], shared), (c["lp"], c["tables"], shared),
             (a["lp"][:1], a["tables"], None), (c["lp"], None, c["receptor"]), (b["lp"], b["tables"], (shared[0].copy(), shared[1]))]
    prepared = _prepare_check_items(items)
    assert [(it["P"], it["N"], it["fits"]) for it in prepared] == [(2, 3, True), (1, 2, True), (3, 5, True), (1, 3, True), (3, 5, True), (1, 2, True)]
    pk = _pack_pose_checks(prepared)
    assert pk["n_receptors"] == 3 and pk["cplx_rec"].tolist() == [0, 0, 0, -1, 1, 2]          # the same array object: one entry; a copy: another
    assert pk["rec_ptr"].tolist() == [0, 5, 12, 17] and pk["rec"].shape == (17, 4) and pk["rec"].dtype == np.float32
    assert np.array_equal(pk["rec"][:5, :3], shared[0]) and np.array_equal(pk["rec"][:5, 3], shared[1]) and np.array_equal(pk["rec"][5:12, :3], c["receptor"][0])
    assert pk["pose_cplx"].tolist() == [0, 0, 1, 2, 2, 2, 3, 4, 4, 4, 5] and pk["cplx_n"].tolist() == [3, 2, 5, 3, 5, 2] and pk["max_n"] == 5
    assert pk["pose_ptr"].tolist() == [0, 3, 6, 8, 13, 18, 23, 26, 31, 36, 41, 43] and pk["pos"].shape == (43, 3) and pk["lig_radius"].shape == (43,)
    assert np.array_equal(pk["lig_radius"][3:6], a["tables"][3]) and np.array_equal(pk["lig_radius"][36:41], np.full(5, 1.7, np.float32))
    assert np.array_equal(pk["pos"][8:13], c["lp"][0])
    # N * N kind bytes per ligand, padded to a multiple of four: 9 -> 12, 4 -> 4; none for an item without tables
    assert pk["cplx_tab"].tolist() == [1, 1, 0, 1, 0, 1] and pk["tab_ptr"].tolist() == [0, 12, 16, 16, 28, 28, 32]
    assert pk["kind"].dtype == np.uint8 and len(pk["kind"]) == 32 and pk["kind_words"].dtype == np.int32 and len(pk["kind_words"]) == 8
    assert pk["kind"][:9].reshape(3, 3).tolist() == a["tables"][2].tolist() and pk["kind"][9:12].tolist() == [0, 0, 0]
    lower, upper = a["tables"][0], a["tables"][1]
    m = pk["bounds"][:9].reshape(3, 3)
    assert pk["bounds"].dtype == np.float32 and all(m[i, j] == upper[i, j] and m[j, i] == lower[i, j] for i in range(3) for j in range(i + 1, 3))
    assert all(pk[k].dtype == np.int32 for k in ("pose_cplx", "pose_ptr", "cplx_n", "cplx_rec", "cplx_tab", "tab_ptr", "rec_ptr"))
    # over the kernel's capacity: marked for the host route; nothing fits -> empty arrays, no receptor
    big = _prepare_check_items([(np.zeros((1, 257, 3), np.float32), None, None)])
    assert [it["fits"] for it in big] == [False]
    none = _pack_pose_checks([])
    assert none["n_receptors"] == 0 and len(none["pose_cplx"]) == 0 and none["tab_ptr"].tolist() == [0] and none["rec_ptr"].tolist() == [0]
    with pytest.raises(ValueError):
        _prepare_check_items([(np.zeros((1, 4, 3), np.float32), (None, None, None, np.ones(3, np.float32)), None)])
    with pytest.raises(RuntimeError, match="MI355X"):
        from confidence_bootstrapping_amd.evaluation import pose_checks_batch
        pose_checks_batch(items, "cpu")


def _inference_results(f):
    """one complex, six poses of the 1a0q ligand in the frame of `orig` (centre c0); the receptor comes from the filtering graph, which
    is centred elsewhere (c1): 0 the crystal pose, 1 the crystal pose 0.25 A off, 2 pushed 1.5 A into the receptor, 3 a torsion that
    clashes internally, 4 the crystal pose 30 A outside the protein, 5 pushed in, below the confidence cutoff"""
    from confidence_bootstrapping_amd.evaluation import pose_checks
    c0, c1 = np.float32([[10.0, -4.0, 2.5]]), np.float32([[-3.0, 8.0, 1.0]])
    first = pose_checks(f.crystal[None], f.tables, f.rec)
    towards = f.rec[0][int(first.rec_atom[0])] - f.crystal[int(first.rec_lig_atom[0])]
    pushed = f.crystal + 1.5 * towards / np.linalg.norm(towards)
    scan = _torsion_scan(f.mol, f.crystal)
    clashing = scan[int(np.argmin(pose_checks(np.stack([s[2] for s in scan]), f.tables, None).clash_ratio))][2]
    away = f.crystal + (f.crystal.mean(axis=0) - f.rec[0].mean(axis=0)) / np.linalg.norm(f.crystal.mean(axis=0) - f.rec[0].mean(axis=0)) * 60.0
    absolute = np.stack([f.crystal, f.crystal + np.float32([0.25, 0.0, 0.0]), pushed, clashing, away, pushed]).astype(np.float32)
    conf = np.float32([1.0, 0.75, 2.0, 1.5, 0.5, -1.0])
    x = torch.ones(23, 2, dtype=torch.long)
    graphs = [_Graph(torch.from_numpy(p - c0), x=x) for p in absolute]
    orig = _Graph(torch.from_numpy(absolute[0] - c0), center=torch.from_numpy(c0), x=x)
    orig.mol = [f.mol]
    filtering = _Graph(None, center=torch.from_numpy(c1), atom=SimpleNamespace(pos=torch.from_numpy(f.rec[0] - c1), x=f.graph["atom"].x))
    return [((orig, None, [filtering] * 6), (graphs, torch.from_numpy(conf)))], absolute, conf, graphs, (c0, c1)


def test_summarize_inference_keeps_only_valid_poses_when_asked(fixture_1a0q):
    import confidence_bootstrapping_amd.finetune_train as ft
    from confidence_bootstrapping_amd.evaluation import cluster_poses
    f = fixture_1a0q
    results, absolute, conf, graphs, (c0, c1) = _inference_results(f)
    # expected validity: the brute force in the frame summarize_inference works in (poses minus c0; receptor atoms minus c1, shifted by c1 - c0)
    lp, rec = absolute - c0, ((f.rec[0] - c1) + (c1 - c0), f.rec[1])
    valid = brute_checks(lp, f.tables, rec)[0]["valid"]
    print("valid", valid.tolist())
    assert valid.tolist() == [True, True, False, False, True, False]
    cutoff, fargs = 0.0, Namespace(rmsd_classification_cutoff=2.0)
    same = lambda got, want: len(got) == len(want) and all(a[0] is b[0] and a[1] == b[1] for a, b in zip(got, want))
    above = [i for i in range(6) if conf[i] > cutoff]
    absent = ft.summarize_inference(results, Namespace(), fargs, cutoff, "cpu", group=8)
    off = ft.summarize_inference(results, Namespace(keep_valid=False), fargs, cutoff, "cpu", group=8)
    on = ft.summarize_inference(results, Namespace(keep_valid=True), fargs, cutoff, "cpu", group=8)
    assert same(absent[1], [(graphs[i], float(conf[i])) for i in above]) and same(off[1], absent[1])
    assert absent[0] == off[0] == on[0] and np.array_equal(absent[2], on[2]) and np.array_equal(absent[2], off[2])
    assert same(on[1], [(graphs[i], float(conf[i])) for i in above if valid[i]]) and len(on[1]) == 3
    # with keep_distinct_rmsd the modes are formed among the valid poses: without validity the pushed-in pose 2 (the most confident) heads the
    # crystal mode; with it pose 0 does
    modes_only = ft.summarize_inference(results, Namespace(keep_distinct_rmsd=2.0), fargs, cutoff, "cpu", group=8)
    both = ft.summarize_inference(results, Namespace(keep_distinct_rmsd=2.0, keep_valid=True), fargs, cutoff, "cpu", group=8)
    ranked = sorted((i for i in above if valid[i]), key=lambda i: -conf[i])
    head = cluster_poses(lp[ranked], f.mol, cutoff=2.0)[1]
    heads = {ranked[h] for h in head}
    assert heads == {0, 4}
    assert same(both[1], [(graphs[i], float(conf[i])) for i in above if i in heads])
    assert graphs[2] in [g for g, _ in modes_only[1]] and graphs[0] not in [g for g, _ in modes_only[1]]
    assert both[0] == absent[0] and np.array_equal(both[2], absent[2])
    # a complex without an 'atom' store anywhere: only the internal checks run
    (orig, _, _), preds = results[0]
    internal = ft.summarize_inference([((orig, None, None), preds)], Namespace(keep_valid=True), fargs, cutoff, "cpu", group=1)
    assert same(internal[1], [(graphs[i], float(conf[i])) for i in (0, 1, 2, 4)])


def test_write_pose_checks_one_row_per_rank(fixture_1a0q, tmp_path):
    from confidence_bootstrapping_amd.docking import POSE_CHECK_COLUMNS, pose_check_rows, write_pose_checks
    f = fixture_1a0q
    results, absolute, conf, graphs, (c0, c1) = _inference_results(f)
    for g in graphs:
        g.original_center = torch.from_numpy(c0)
    receptor_graph = results[0][0][2][0]
    rows = pose_check_rows([(f.mol, graphs, torch.from_numpy(conf), receptor_graph)], "cpu")
    order, got_conf, checks = rows[0]
    assert list(order) == [2, 3, 0, 1, 4, 5] and checks.valid.tolist() == [False, False, True, True, True, False]
    path = write_pose_checks(str(tmp_path), rows[0])
    lines = open(path).read().splitlines()
    assert os.path.basename(path) == "pose_checks.csv" and lines[0].split(",") == list(POSE_CHECK_COLUMNS)
    assert POSE_CHECK_COLUMNS[:7] == ("rank", "confidence", "valid", "n_bad_bond", "n_bad_angle", "n_internal_clash", "n_rec_clash")
    cells = [line.split(",") for line in lines[1:]]
    assert len(cells) == 6 and [int(c[0]) for c in cells] == [1, 2, 3, 4, 5, 6]
    assert [float(c[1]) for c in cells] == [2.0, 1.5, 1.0, 0.75, 0.5, -1.0] and [int(c[2]) for c in cells] == [0, 0, 1, 1, 1, 0]
    want = brute_checks(absolute[order], f.tables, f.rec)[0]
    assert [int(c[6]) for c in cells] == want["n_rec_clash"].tolist() and [int(c[5]) for c in cells] == want["n_internal_clash"].tolist()
    assert [int(c[14]) for c in cells] == want["rec_lig_atom"].tolist() and [int(c[15]) for c in cells] == want["rec_atom"].tolist()
    assert all(abs(float(c[12]) - w) < 1e-5 for c, w in zip(cells, want["rec_ratio"]))
    # without confidences and without a receptor: data_list order, an empty confidence cell, nan in the receptor columns
    bare = pose_check_rows([(f.mol, graphs[:2], None, None)], "cpu")[0]
    lines = open(write_pose_checks(str(tmp_path / "bare"), bare)).read().splitlines()
    assert len(lines) == 3 and lines[1].split(",")[:3] == ["1", "", "1"] and lines[1].split(",")[12] == "nan" and lines[1].split(",")[16] == "32"
