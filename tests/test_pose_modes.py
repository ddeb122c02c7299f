"""Host side of grouping sampled poses into distinct binding modes: evaluation.cluster_poses (the reference of cbd_pose_modes) against a
brute-force triple loop, the ordering rules of the leader clustering on hand-built matrices, the packer of the ragged batch, the mode files
of docking.write_ranked_poses and the opt-in filter of finetune_train.summarize_inference.  No GPU.

The inputs (tests/pose_mode_helpers.py) keep every pair at least 1.0 A away from the 2.0 A cutoff; that margin is asserted on the brute-force
fp64 matrix before anything else is looked at."""
import os
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.metrics_helpers import coords
from tests.pose_mode_helpers import CUTOFF, assert_margin, brute_matrix, brute_modes, expected_modes, ligand_cases

HERE = os.path.dirname(os.path.abspath(__file__))
SDF = os.path.join(HERE, "golden", "1a0q", "1a0q_ligand.sdf")


@pytest.fixture(scope="module")
def cases():
    return ligand_cases()


def test_cluster_poses_equals_the_brute_force_loop(cases):
    from confidence_bootstrapping_amd.evaluation import cluster_poses
    without = {}
    for name, mol, iso, lp, label in cases:
        d = brute_matrix(lp, *iso)
        assert_margin(d, label)
        matrix, head, mode, n_modes = cluster_poses(lp, mol, cutoff=CUTOFF)
        assert matrix.dtype == np.float32 and head.dtype == np.int32 and mode.dtype == np.int32
        assert np.array_equal(matrix, d.astype(np.float32))          # the sums are exact on the grid: one rounding of the same fp64 value
        assert np.array_equal(matrix, matrix.T) and not matrix.diagonal().any()
        want = brute_modes(d, CUTOFF)
        assert (head.tolist(), mode.tolist(), n_modes) == want == expected_modes(label)
        given = cluster_poses(lp, None, cutoff=CUTOFF, isomorphisms=iso)
        assert np.array_equal(given[0], matrix) and np.array_equal(given[1], head) and given[3] == n_modes
        without[name] = cluster_poses(lp, None, cutoff=CUTOFF)[3]          # mol None: the identity mapping
    print("modes without the isomorphisms:", without)
    assert without["ring6"] > 5 and without["star7"] > 5          # the symmetry correction decides on these inputs


def _modes(matrix, cutoff):
    from confidence_bootstrapping_amd.evaluation import modes_from_matrix
    head, mode, n = modes_from_matrix(np.asarray(matrix, dtype=np.float32), cutoff)
    return head.tolist(), mode.tolist(), n


def test_ordering_rules_on_hand_built_matrices():
    from confidence_bootstrapping_amd.evaluation import cluster_poses
    # chain A - B - C: B joins A, C is near B only, and B is no head: C opens a mode
    assert _modes([[0, 1.5, 3.0], [1.5, 0, 1.5], [3.0, 1.5, 0]], 2.0) == ([0, 0, 2], [0, 0, 1], 2)
    # pose 2 lies within the cutoff of both heads (0 and 1) and nearer to 1: it joins the better-ranked one
    assert _modes([[0, 3.0, 1.9], [3.0, 0, 0.5], [1.9, 0.5, 0]], 2.0) == ([0, 1, 0], [0, 1, 0], 2)
    # a NaN pose gets -1; the others are what they are without it
    nan = float("nan")
    with_nan = [[0, nan, 1.5, 3.0], [nan, nan, nan, nan], [1.5, nan, 0, 1.5], [3.0, nan, 1.5, 0]]
    assert _modes(with_nan, 2.0) == ([0, -1, 0, 3], [0, -1, 0, 1], 2)
    # one pose: one mode
    assert _modes([[0.0]], 2.0) == ([0], [0], 1)
    # two grid poses exactly 2.0 A apart (every atom moved by 2 A along x): one mode at 2.0, two just below it
    a = coords(7, 1, 5)[0]
    pair = np.stack([a, a + np.float32([2.0, 0.0, 0.0])])
    matrix, head, mode, n = cluster_poses(pair, None, cutoff=2.0)
    assert matrix[0, 1] == np.float32(2.0) and (head.tolist(), mode.tolist(), n) == ([0, 0], [0, 0], 1)
    _, head, mode, n = cluster_poses(pair, None, cutoff=np.nextafter(2.0, 0))
    assert (head.tolist(), mode.tolist(), n) == ([0, 1], [0, 1], 2)
    # through the coordinates: a pose with a NaN coordinate, and one with an infinite one
    lp = np.stack([a, a, a + np.float32(0.25), a])
    lp[1, 3, 2] = np.nan
    lp[3, 0, 0] = np.inf
    matrix, head, mode, n = cluster_poses(lp, None, cutoff=2.0)
    assert (head.tolist(), mode.tolist(), n) == ([0, -1, 0, -1], [0, -1, 0, -1], 1)
    assert np.isnan(matrix[1]).all() and np.isnan(matrix[:, 1]).all() and np.isnan(matrix[3]).all() and np.isnan(matrix[:, 3]).all()
    assert matrix[0, 0] == 0 and matrix[2, 2] == 0 and matrix[0, 2] == matrix[2, 0] == np.float32(np.sqrt(3 * 0.25 ** 2))


def test_packer_arrays_for_a_ragged_batch(cases):
    from confidence_bootstrapping_amd.evaluation import _pack_pose_modes, _prepare_cluster_items
    import confidence_bootstrapping_amd.molecules_utils as mu
    mu.iso_cache_clear()
    (_, ring, ring_iso, ring_lp, _), (_, star, _, star_lp, _), (_, _, _, fork_lp, _) = cases[1], cases[2], cases[3]
    items = [(ring_lp[:9], ring), (star_lp[:1], star), (fork_lp[:3], None), (ring_lp[:2], ring)]
    prepared = _prepare_cluster_items(items)
    assert [it["K"] for it in prepared] == [12, 6, 1, 12] and all(it["fits"] for it in prepared)
    assert prepared[0]["entry"] is prepared[3]["entry"] and mu.iso_cache_stats()["misses"] == 2          # one enumeration per ligand
    pk = _pack_pose_modes(prepared, cutoff=1.5)
    assert pk["grp_n"].tolist() == [6, 7, 65, 6] and pk["grp_p"].tolist() == [9, 1, 3, 2] and pk["grp_k"].tolist() == [12, 6, 1, 12]
    assert pk["grp_cutoff"].dtype == np.float64 and pk["grp_cutoff"].tolist() == [1.5] * 4
    assert pk["pose_ptr"].tolist() == [0, 9, 10, 13, 15]
    assert pk["atom_ptr"].tolist() == [0, 54, 61, 256, 268]
    assert pk["mat_ptr"].tolist() == [0, 81, 82, 91, 95]
    assert all(pk[k].dtype == np.int32 for k in ("grp_n", "grp_p", "grp_k", "pose_ptr", "atom_ptr", "mat_ptr"))
    assert pk["pos"].dtype == np.float32 and pk["pos"].shape == (268, 3)
    assert np.array_equal(pk["pos"][54:61], star_lp[0]) and np.array_equal(pk["pos"][256:], ring_lp[:2].reshape(-1, 3))
    assert pk["max_n"] == 65 and pk["max_p"] == 9
    assert np.array_equal(pk["idx_ref"][0], ring_iso[0]) and np.array_equal(pk["idx_pos"][0], ring_iso[1])
    assert pk["idx_ref"][2].tolist() == [list(range(65))]
    # over the kernel's capacity: the item is marked for the host route
    big = _prepare_cluster_items([(np.zeros((257, 3, 3), np.float32), None), (np.zeros((2, 513, 3), np.float32), None)])
    assert [it["fits"] for it in big] == [False, False]
    with pytest.raises(ValueError):
        _prepare_cluster_items([(np.zeros((4, 3)), None)])
    mu.iso_cache_clear()


def test_cluster_poses_batch_has_no_cpu_path(cases):
    from confidence_bootstrapping_amd.evaluation import cluster_poses_batch
    with pytest.raises(RuntimeError, match="cluster_poses"):
        cluster_poses_batch([(cases[0][3], cases[0][1])], "cpu")


class _Graph:
    """what write_ranked_poses and summarize_inference read of a pose graph"""

    def __init__(self, pos, center=None, x=None):
        self._lig = SimpleNamespace(pos=pos, x=x, orig_pos=None)
        self.original_center = center

    def __getitem__(self, key):
        assert key == "ligand"
        return self._lig


def _tree(path):
    return {name: open(os.path.join(path, name), "rb").read() for name in sorted(os.listdir(path))}


def test_write_ranked_poses_writes_the_modes_and_is_unchanged_without_them(tmp_path):
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    from confidence_bootstrapping_amd.docking import ranked_modes, write_ranked_poses
    from confidence_bootstrapping_amd.evaluation import cluster_poses
    lig = pm.read_molecule(SDF, sanitize=True, remove_hs=True)
    n = lig.GetNumAtoms()
    rng = np.random.default_rng(3)
    center = torch.tensor([[20.0, 15.0, 50.0]])
    base = torch.from_numpy(rng.normal(0, 3, size=(n, 3)).astype(np.float32))
    shift = [0.0, 9.0, 0.1, 9.1, 18.0, 0.2]          # three places, 3 + 2 + 1 poses
    data_list = [_Graph(base + s, center) for s in shift]
    confidence = torch.tensor([0.5, 1.5, -2.0, 0.25, -1.0, 1.0])          # ranks: 1, 5, 0, 3, 4, 2
    modes = ranked_modes([(lig, data_list, confidence)], "cpu", cutoff=2.0)[0]
    assert modes[0].tolist() == [5, 1, 5, 1, 4, 5] and modes[1].tolist() == [1, 0, 1, 0, 2, 1]
    plain, again, with_modes = (str(tmp_path / d) for d in ("plain", "again", "modes"))
    order = write_ranked_poses(plain, lig, data_list, confidence)
    assert write_ranked_poses(again, lig, data_list, confidence, modes=None) == order == [1, 5, 0, 3, 4, 2]
    assert write_ranked_poses(with_modes, lig, data_list, confidence, modes=modes) == order
    before, same, after = _tree(plain), _tree(again), _tree(with_modes)
    assert before == same and not any(name.startswith("mode") for name in before)
    extra = sorted(set(after) - set(before))
    assert extra == ["mode1_rank1_confidence1.50.sdf", "mode2_rank2_confidence1.00.sdf", "mode3_rank5_confidence-1.00.sdf", "modes.csv"]
    assert {k: v for k, v in after.items() if k not in extra} == before
    assert after["mode1_rank1_confidence1.50.sdf"] == after["rank1_confidence1.50.sdf"]
    assert after["mode2_rank2_confidence1.00.sdf"] == after["rank2_confidence1.00.sdf"]
    assert after["mode3_rank5_confidence-1.00.sdf"] == after["rank5_confidence-1.00.sdf"]
    rows = after["modes.csv"].decode().splitlines()
    assert rows[0] == "mode,head_rank,population,best_confidence,mean_confidence"
    assert rows[1:] == ["1,1,2,1.500000,0.875000", "2,2,3,1.000000,-0.166667", "3,5,1,-1.000000,-1.000000"]
    # the csv agrees with cluster_poses on the coordinates the rank files hold
    ranked = np.stack([pm.read_molecule(os.path.join(with_modes, f)).pos for f in
                       sorted((f for f in after if f.startswith("rank") and "_confidence" in f), key=lambda f: int(f[4:f.index("_")]))])
    _, head, mode, n_modes = cluster_poses(ranked, lig, cutoff=2.0)
    assert n_modes == 3 and [int(r.split(",")[1]) for r in rows[1:]] == [int(h) + 1 for h in sorted(set(head.tolist()))]
    assert [int(r.split(",")[2]) for r in rows[1:]] == np.bincount(mode).tolist()
    # without confidences: data_list order, mode{m}_rank{k}.sdf
    bare = str(tmp_path / "bare")
    write_ranked_poses(bare, lig, data_list, None, modes=ranked_modes([(lig, data_list, None)], "cpu")[0])
    assert sorted(f for f in os.listdir(bare) if f.startswith("mode")) == ["mode1_rank1.sdf", "mode2_rank2.sdf", "mode3_rank5.sdf", "modes.csv"]
    assert open(os.path.join(bare, "modes.csv")).read().splitlines()[1:] == ["1,1,3,,", "2,2,2,,", "3,5,1,,"]
    with pytest.raises(ValueError):
        write_ranked_poses(bare, lig, data_list, None, modes=(modes[0][:3], modes[1][:3]))


def test_summarize_inference_keeps_only_the_heads_when_asked(cases):
    import confidence_bootstrapping_amd.finetune_train as ft
    results, want_all, want_heads = [], [], []
    cutoff = -0.5
    for c, (name, mol, iso, lp, label) in enumerate(cases[1:3]):          # ring6 and star7: the isomorphisms matter
        lp = lp[:17]
        rng = np.random.default_rng(20 + c)
        conf = rng.permutation(np.linspace(-2.0, 2.0, 17)).astype(np.float32)
        x = torch.ones(lp.shape[1], 2, dtype=torch.long)
        graphs = [_Graph(torch.from_numpy(p), x=x) for p in lp]
        orig = _Graph(torch.from_numpy(lp[0]), center=torch.zeros(1, 3), x=x)
        orig.mol = mol
        results.append(((orig, None, None), (graphs, torch.from_numpy(conf))))
        above = [i for i in range(17) if float(conf[i]) > cutoff]
        want_all += [(graphs[i], float(conf[i])) for i in above]
        ranked = sorted(above, key=lambda i: -float(conf[i]))
        d = brute_matrix(lp[ranked], *iso)
        assert_margin(d, label[ranked])
        head = brute_modes(d, 2.0)[0]
        heads = {ranked[h] for h in head}
        assert 1 < len(heads) < len(above)
        want_heads += [(graphs[i], float(conf[i])) for i in above if i in heads]
    fargs = Namespace(rmsd_classification_cutoff=2.0)
    same = lambda got, want: len(got) == len(want) and all(a[0] is b[0] and a[1] == b[1] for a, b in zip(got, want))
    absent = ft.summarize_inference(results, Namespace(), fargs, cutoff, "cpu", group=8)
    off = ft.summarize_inference(results, Namespace(keep_distinct_rmsd=None), fargs, cutoff, "cpu", group=8)
    on = ft.summarize_inference(results, Namespace(keep_distinct_rmsd=2.0), fargs, cutoff, "cpu", group=8)
    assert same(absent[1], want_all) and same(off[1], want_all)
    assert same(on[1], want_heads)
    assert absent[0] == off[0] == on[0] and np.array_equal(off[2], on[2])
    # a cutoff nothing passes: nothing is clustered, nothing kept
    assert ft.summarize_inference(results, Namespace(keep_distinct_rmsd=2.0), fargs, 1e9, "cpu", group=1)[1] == []
