"""Host side of the one-launch pose evaluation (evaluation.pose_metrics_batch behind args.device_metrics): the process-wide isomorphism
cache of molecules_utils, the packed ragged batch cbd_pose_metrics reads, and finetune_train.summarize_inference, the post-processing of
inference_epoch moved into a helper.  No GPU: everything here is host code."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests.metrics_helpers import LIGANDS, chain5, coords, fork, metrics64, ring6, star7


@pytest.fixture()
def mu():
    import confidence_bootstrapping_amd.molecules_utils as m
    m.iso_cache_clear()
    m.iso_cache_configure(enabled=True, limit_bytes=256 << 20)
    yield m
    m.iso_cache_clear()
    m.iso_cache_configure(enabled=True, limit_bytes=256 << 20)


def _counting(mu, monkeypatch):
    calls, real = [], mu.graph_isomorphisms

    def counted(atomicnums, *a, **k):
        calls.append(len(np.asarray(atomicnums)))
        return real(atomicnums, *a, **k)
    monkeypatch.setattr(mu, "graph_isomorphisms", counted)
    return calls


@pytest.mark.parametrize("name,make,k", LIGANDS, ids=[l[0] for l in LIGANDS])
def test_helper_ligands_have_the_stated_number_of_isomorphisms(mu, name, make, k):
    mol = make()
    idx1, idx2 = mu.graph_isomorphisms(mol.atomicnums, mol.adjacency_matrix)
    assert idx1.shape == idx2.shape == (k, len(mol.atomicnums))
    got1, got2 = mu.cached_isomorphisms(mol.atomicnums, mol.adjacency_matrix)
    assert np.array_equal(got1, idx1) and np.array_equal(got2, idx2) and got1.dtype == np.int32


def test_fp64_restatement_on_a_case_worked_by_hand():
    mol = ring6()
    idx = np.stack([np.roll(np.arange(6), -s) for s in range(6)]).astype(np.int32)       # the six rotations
    ref = np.zeros((1, 6, 3))
    ref[0, :, 0] = np.arange(6)
    lp = np.roll(ref, 2, axis=1) + np.array([0.0, 3.0, 4.0])                              # pose atom i + 2 sits over crystal atom i, 5 A away
    rmsd, centroid, min_self, q, k = metrics64(lp, ref, np.tile(np.arange(6), (6, 1)), idx)
    assert rmsd[0] == pytest.approx(5.0) and centroid[0] == pytest.approx(5.0) and min_self[0] == pytest.approx(1.0)
    assert (q[0], k[0]) == (0, 2) and len(mol.atomicnums) == 6


def test_one_enumeration_per_ligand(mu, monkeypatch):
    from confidence_bootstrapping_amd.evaluation import _prepare_metrics_items
    calls = _counting(mu, monkeypatch)
    mols = [make() for _, make, _ in LIGANDS]
    for _ in range(3):
        for mol, (_, _, k) in zip(mols, LIGANDS):
            assert mu.cached_isomorphisms(mol.atomicnums, mol.adjacency_matrix)[0].shape[0] == k
    assert sorted(calls) == [5, 6, 7, 65, 130]
    # the batch route reads the same entries: a fresh but equal molecule object, several crystal poses, repeated calls -- no enumeration
    items = [(coords(len(m.atomicnums), 2, 1), coords(len(m.atomicnums), 2, 2), make()) for m, (_, make, _) in zip(mols, LIGANDS)]
    for _ in range(2):
        prepared = _prepare_metrics_items(items)
    assert [it["K"] for it in prepared] == [k for _, _, k in LIGANDS] and len(calls) == 5
    st = mu.iso_cache_stats()
    assert st["entries"] == 5 and st["misses"] == 5 and st["hits"] == 10 + 10
    # the functions that existed before do not go through the cache
    mu.graph_isomorphisms(mols[0].atomicnums, mols[0].adjacency_matrix)
    assert len(calls) == 6 and mu.iso_cache_stats()["hits"] == 20


def test_a_cached_isomorphism_limit_is_raised_again_without_enumerating(mu, monkeypatch):
    calls = _counting(mu, monkeypatch)
    mol = ring6()
    for _ in range(3):
        with pytest.raises(mu.IsomorphismLimit, match="more than 3"):
            mu.cached_isomorphisms(mol.atomicnums, mol.adjacency_matrix, max_isomorphisms=3)
    assert len(calls) == 1
    # the cap is part of the key: the default cap enumerates (once) and succeeds
    assert mu.cached_isomorphisms(mol.atomicnums, mol.adjacency_matrix)[0].shape == (12, 6) and len(calls) == 2
    # graphs that are not isomorphic: the ValueError is cached as well
    a, b = chain5(), chain5()
    b.atomicnums = b.atomicnums[::-1].copy()
    b.atomicnums[2] = 15
    for _ in range(2):
        with pytest.raises(ValueError, match="not isomorphic"):
            mu.cached_isomorphisms(a.atomicnums, a.adjacency_matrix, b.atomicnums, b.adjacency_matrix)
    assert len(calls) == 3


def test_lru_eviction_by_bytes(mu, monkeypatch):
    calls = _counting(mu, monkeypatch)
    size = lambda k, n: mu._ISO_ENTRY_OVERHEAD + 2 * k * n * 4
    get = lambda mol: mu.cached_isomorphisms(mol.atomicnums, mol.adjacency_matrix)
    mu.iso_cache_configure(limit_bytes=size(12, 6) + size(6, 7))
    get(ring6()); get(star7())
    assert mu.iso_cache_stats()["bytes"] == size(12, 6) + size(6, 7) and mu.iso_cache_stats()["entries"] == 2
    get(ring6())                          # the ring is now the most recently used
    get(chain5())                         # does not fit next to both: the star goes, not the ring, and not everything
    st = mu.iso_cache_stats()
    assert st["entries"] == 2 and st["bytes"] == size(12, 6) + size(1, 5)
    n = len(calls)
    get(ring6()); get(chain5())
    assert len(calls) == n
    get(star7())
    assert len(calls) == n + 1
    # an entry larger than the whole limit is returned but not kept; shrinking the limit evicts; clear() empties
    mu.iso_cache_configure(limit_bytes=size(1, 5))
    assert mu.iso_cache_stats()["bytes"] <= size(1, 5)
    assert get(ring6())[0].shape == (12, 6) and mu.iso_cache_stats()["bytes"] <= size(1, 5)
    mu.iso_cache_clear()
    assert mu.iso_cache_stats() == {"entries": 0, "bytes": 0, "hits": 0, "misses": 0}
    mu.iso_cache_configure(enabled=False)
    get(chain5()); get(chain5())
    assert mu.iso_cache_stats()["entries"] == 0 and calls[-2:] == [5, 5]


def test_key_changes_with_one_element_or_one_bond(mu):
    mol = star7()
    key = mu.isomorphism_key(mol.atomicnums, mol.adjacency_matrix)
    assert key == mu.isomorphism_key(mol.atomicnums.astype(np.int32).tolist(), mol.adjacency_matrix.astype(bool))
    assert key == mu.isomorphism_key(mol.atomicnums, mol.adjacency_matrix * 3)             # bond orders are not part of the graph
    nums = mol.atomicnums.copy()
    nums[5] = 17
    assert key != mu.isomorphism_key(nums, mol.adjacency_matrix)
    am = mol.adjacency_matrix.copy()
    am[0, 2] = am[2, 0] = 1
    assert key != mu.isomorphism_key(mol.atomicnums, am)
    am = mol.adjacency_matrix.copy()
    am[0, 1] = am[1, 0] = 0
    assert key != mu.isomorphism_key(mol.atomicnums, am)
    assert key != mu.isomorphism_key(mol.atomicnums, mol.adjacency_matrix, mol.atomicnums, am)
    assert key != mu.isomorphism_key(mol.atomicnums, mol.adjacency_matrix, max_isomorphisms=3)
    # six carbons as a ring and as a chain differ only in one bond
    ring = ring6()
    chain = ring.adjacency_matrix.copy()
    chain[0, 5] = chain[5, 0] = 0
    assert mu.isomorphism_key(ring.atomicnums, ring.adjacency_matrix) != mu.isomorphism_key(ring.atomicnums, chain)


def test_packing_layout_of_a_ragged_batch(mu, capsys):
    from confidence_bootstrapping_amd.evaluation import _pack_pose_metrics, _prepare_metrics_items
    ring, star, f65 = ring6(), star7(), fork(65)
    items = [(coords(6, 3, 1), coords(6, 1, 2)[0], ring),            # Q = 1 given as [N, 3]
             (coords(7, 1, 3), coords(7, 2, 4), star),               # Q = 2
             (coords(65, 8, 5), coords(65, 2, 6), None),             # no molecule: identity mapping
             (coords(5, 2, 7), coords(5, 1, 8), star)]               # a molecule that does not match the coordinates: identity mapping
    prepared = _prepare_metrics_items(items)
    printed = capsys.readouterr().out
    assert printed.count("Using non corrected RMSD because of the error:") == 1       # the mismatch; mol = None is silent, as on the host route
    assert [(it["P"], it["N"], it["Q"], it["K"], it["fits"]) for it in prepared] == [(3, 6, 1, 12, True), (1, 7, 2, 6, True),
                                                                                       (8, 65, 2, 1, True), (2, 5, 1, 1, True)]
    pk = _pack_pose_metrics(prepared)
    assert pk["pose_cplx"].tolist() == [0] * 3 + [1] + [2] * 8 + [3] * 2 and pk["pose_cplx"].dtype == np.int32
    assert pk["pose_ptr"].tolist() == [0, 6, 12, 18, 25] + [25 + 65 * i for i in range(1, 9)] + [550, 555]
    assert pk["cplx_n"].tolist() == [6, 7, 65, 5] and pk["cplx_k"].tolist() == [12, 6, 1, 1] and pk["cplx_q"].tolist() == [1, 2, 2, 1]
    assert pk["ref_ptr"].tolist() == [0, 6, 20, 150, 155] and (pk["max_n"], pk["max_ref"]) == (65, 130)
    assert pk["pos"].shape == (555, 3) and pk["ref"].shape == (155, 3) and pk["pos"].dtype == pk["ref"].dtype == np.float32
    assert np.array_equal(pk["pos"][18:25], items[1][0][0]) and np.array_equal(pk["pos"][25 + 65:25 + 130], items[2][0][1])
    assert np.array_equal(pk["ref"][0:6], items[0][1]) and np.array_equal(pk["ref"][13:20], items[1][1][1])
    want = mu.graph_isomorphisms(ring.atomicnums, ring.adjacency_matrix)
    assert np.array_equal(pk["idx_ref"][0], want[0]) and np.array_equal(pk["idx_pos"][0], want[1])
    assert pk["idx_ref"][1].shape == (6, 7)
    for c, n in ((2, 65), (3, 5)):
        assert np.array_equal(pk["idx_ref"][c], np.arange(n)[None]) and np.array_equal(pk["idx_pos"][c], np.arange(n)[None])
        assert pk["idx_ref"][c].dtype == np.int32
    # explicit isomorphisms are used as given and not cached; sizes over the kernel's capacity are marked for the host route
    before = mu.iso_cache_stats()["entries"]
    cut = (want[0][:7], want[1][:7])
    prepared = _prepare_metrics_items(items[:1] + [(coords(513, 1, 9), coords(513, 1, 10), None), (coords(300, 1, 11), coords(300, 14, 12), None)],
                                      isomorphisms=[cut, None, None])
    assert prepared[0]["K"] == 7 and prepared[0]["key"] is None and [it["fits"] for it in prepared] == [True, False, False]
    assert mu.iso_cache_stats()["entries"] == before + 2          # the two identity tables
    with pytest.raises(ValueError):
        _prepare_metrics_items([(coords(6, 1, 1), coords(5, 1, 2), None)])


# ---- summarize_inference: the loop that used to be inline in inference_epoch ------------------------------------------------------------

class _G(dict):
    """a graph as far as the post-processing reads it: g['ligand'].pos / .x / .orig_pos, g.original_center, g.mol"""


def _recorded_results():
    """four complexes x three poses on a 1/8 A grid: (0) one crystal pose and a hydrogen to filter, (1) two crystal poses, (2) a crystal pose
    wrapped in a list and a molecule on which the RMSD function raises, (3) no crystal pose"""
    results = []
    for c in range(4):
        n_atoms = 5 + c
        base = (((np.arange(n_atoms * 3) * 37 + 11 * c) % 64) / 8.0 - 4.0).reshape(n_atoms, 3).astype(np.float32)
        center = torch.tensor([[float(c), -float(c), 0.5]])
        x = torch.ones(n_atoms, 2)
        if c == 0:
            x[1, 0] = 0
        orig = _G(ligand=Namespace(x=x))
        crystal = base + center.numpy()
        if c == 1:
            orig["ligand"].orig_pos = np.stack([crystal, crystal + np.float32(0.5)])
        elif c == 2:
            orig["ligand"].orig_pos = [crystal]
        elif c == 0:
            orig["ligand"].orig_pos = crystal
        orig.original_center = center
        heavy = int((x[:, 0] != 0).sum())
        am = np.zeros((heavy, heavy), dtype=int)
        for i in range(heavy - 1):
            am[i, i + 1] = am[i + 1, i] = 1
        orig.mol = [Namespace(atomicnums=np.arange(6, 6 + heavy), adjacency_matrix=am, raises=(c == 2))]
        preds = []
        for k in range(3):
            shift = np.float32([0.25 * (k + 1) * (c + 1), -0.5 * k, 0.125 * (c - 1) * (k + 2)])
            g = _G(ligand=Namespace(pos=torch.from_numpy(base + shift), x=x))
            g.tag = (c, k)
            preds.append(g)
        conf = torch.tensor([[0.5 * c - 0.25 * k, 9.0] for k in range(3)])
        results.append(((orig, None, None), (preds, conf)))
    return results


def _stand_in_rmsd(mol, ref, poses, device=None):
    if mol.raises:
        raise RuntimeError("stand-in failure")
    return [float(np.sqrt(((np.asarray(p, dtype=np.float64) - np.asarray(ref, dtype=np.float64)) ** 2).sum(axis=1).mean())) for p in poses]


# What the inline loop of inference_epoch produced on _recorded_results() with _stand_in_rmsd before it became summarize_inference
# (run on the parent commit's code, values copied here).
PINNED = {
    "plain": dict(
        losses={"rmsds_lt2": 88.88888888888889, "rmsds_lt5": 100.0, "filtered_rmsds_lt2": 66.66666666666667,
                "filtered_rmsds_lt5": 66.66666666666667, "min_rmsds_lt2": 100.0, "min_rmsds_lt5": 100.0,
                "avg_confidence": 0.4166666666666667, "median_confidence": 0.25},
        kept=[((1, 0), 0.5), ((1, 1), 0.25), ((3, 0), 1.5), ((3, 1), 1.25), ((3, 2), 1.0)],
        top_rmsds=[0.3535533905932738, 0.5]),
    "oracle": dict(
        losses={"rmsds_lt2": 88.88888888888889, "rmsds_lt5": 100.0, "filtered_rmsds_lt2": 100.0, "filtered_rmsds_lt5": 100.0,
                "min_rmsds_lt2": 100.0, "min_rmsds_lt5": 100.0, "avg_confidence": 2.654314449871277,
                "median_confidence": 3.0514041179340365},
        kept=[((0, 0), 3.7719243000541494), ((0, 1), 3.595558800512747), ((0, 2), 3.205541609510041), ((1, 0), 3.7244384346703105),
              ((1, 1), 3.39832307766508), ((2, 0), 3.600557804107666)],
        top_rmsds=[0.3535533905932738, 0.5, 0.7905694246292114]),
}


def _variant(name):
    """(args, filtering_args, confidences per complex, cutoff)"""
    results = _recorded_results()
    if name == "plain":      # one confidence per pose; the third complex was sampled without a confidence model
        results = [(it, (preds, None if it[0].mol[0].raises else conf[:, 0])) for it, (preds, conf) in results]
        return results, Namespace(), Namespace(rmsd_classification_cutoff=2.0), 0.1
    return results, Namespace(oracle_confidence=True), Namespace(rmsd_classification_cutoff=[2.0, 5.0]), 3.0


@pytest.mark.parametrize("name", ["plain", "oracle"])
def test_summarize_inference_returns_what_the_inline_loop_did(monkeypatch, capsys, name):
    import confidence_bootstrapping_amd.finetune_train as ft
    monkeypatch.setattr(ft, "get_symmetry_rmsd", _stand_in_rmsd)
    results, args, filtering_args, cutoff = _variant(name)
    losses, kept, top_rmsds = ft.summarize_inference(results, args, filtering_args, cutoff, device=None, group=8)
    want = PINNED[name]
    assert capsys.readouterr().out.count("Using non corrected RMSD because of the error: stand-in failure") == 1
    assert set(losses) == set(want["losses"])
    for k, v in want["losses"].items():
        assert losses[k] == (v if v is None else pytest.approx(v, rel=1e-12)), k
    assert [(g.tag, c) for g, c in kept] == [(tag, pytest.approx(c, rel=1e-12)) for tag, c in want["kept"]]
    assert top_rmsds.dtype == np.float64 and top_rmsds.tolist() == pytest.approx(want["top_rmsds"], rel=1e-12)
