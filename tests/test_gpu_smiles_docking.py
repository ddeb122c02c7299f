"""Docking ligands given as SMILES, on the GPU: conformers embedded from the stereo a SMILES carries (`stereo="tags"`),
InferenceDataset / ScreeningDataset (inference_utils.py) on the 1a0q receptor fixture, and the three input forms of tools/dock.py.

The acceptance test of a conformer is the float64 restatement in tests/embed_helpers.py with the band of
tests/test_gpu_conformer_embedding.py.  One launch embeds 32 conformers of each of six molecules; the tests share it.
Measured on an MI355X (seed 0): first attempts ok 32 of 32 for both enantiomers, the two difluoroethenes and indole, 29 of 32 for the
1a0q string; F...F 3.38 .. 3.58 A trans and 2.54 .. 2.87 A cis; indole flat to 0.0000 A.  DESIGN.md section 9 records the same figures."""
import copy
import glob
import gzip
import os

import networkx as nx
import numpy as np
import pytest
import torch

from tests import embed_helpers as eh

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
D = os.path.join(HERE, "golden", "1a0q")
PROTEIN_GZ = os.path.join(D, "1a0q_protein_processed.pdb.gz")
N_CONF = 32
BAND = 1e-3          # as tests/test_gpu_conformer_embedding.py: the band in which the kernel's fp32 evaluation may decide either way
SMILES_1A0Q = "CCCCC(NC(=O)CCC(=O)O)P(=O)(O)OC1=CC=CC=C1"
PARACETAMOL = "CC(=O)Nc1ccc(O)cc1"
EMBEDDED = ["[C@](F)(Cl)(Br)C", "[C@@](F)(Cl)(Br)C", SMILES_1A0Q, "F/C=C/F", "F/C=C\\F", "c1ccc2[nH]ccc2c1"]
HELD_TO_24 = EMBEDDED[:3]        # the molecules whose bounds tests/test_gpu_conformer_embedding.py already holds to 24 of 32
RECEPTOR = dict(receptor_radius=15.0, c_alpha_max_neighbors=24, remove_hs=True, all_atoms=True, atom_radius=5, atom_max_neighbors=8)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def protein(tmp_path_factory):
    pdb = tmp_path_factory.mktemp("rec") / "1a0q_protein_processed.pdb"
    pdb.write_bytes(gzip.open(PROTEIN_GZ).read())
    return str(pdb)


@pytest.fixture(scope="module")
def world():
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    from confidence_bootstrapping_amd.datasets.smiles import mol_from_smiles
    mols = {s: mol_from_smiles(s) for s in EMBEDDED}
    bounds = {s: ce.distance_bounds(m, None, stereo="tags") for s, m in mols.items()}
    res = ce.embed_conformers_batch([bounds[s] for s in EMBEDDED], N_CONF, seed=0)                # six molecules, one launch
    return {"mols": mols, "bounds": bounds, "res": dict(zip(EMBEDDED, res))}


def test_embedding_from_tags_acceptance(world):
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    for s in EMBEDDED:
        lower, upper, cons = world["bounds"][s]
        pos, ok, err = world["res"][s]
        assert pos.shape == (N_CONF, len(lower), 3) and np.isfinite(pos).all() and np.isfinite(err).all()
        for k in range(N_CONF):
            if ok[k]:
                assert eh.accepted(pos[k], lower, upper, cons, ce.BOUND_TOL, widen=BAND), (s, k, eh.violations(pos[k], lower, upper, cons))
            else:
                assert not eh.accepted(pos[k], lower, upper, cons, ce.BOUND_TOL, widen=-BAND), (s, k)
        print(f"{s}: {int(ok.sum())} of {N_CONF} first attempts ok; median error {np.median(err):.2e}")
        if s in HELD_TO_24:
            assert ok.sum() >= 24, (s, int(ok.sum()))
    for s in EMBEDDED[3:]:                                                          # the product's own retry contract
        lower, upper, cons = world["bounds"][s]
        pos, ok, _ = ce.embed_until_ok(world["mols"][s], 8, rounds=3, stereo="tags")
        assert ok.all() and all(eh.accepted(p, lower, upper, cons, ce.BOUND_TOL, widen=BAND) for p in pos), (s, ok)


def test_embedded_stereo_is_the_written_stereo(world):
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    from confidence_bootstrapping_amd.datasets.molfile import perceive
    signs = {}
    for s in EMBEDDED[:2]:
        mol = world["mols"][s]
        pos, ok, _ = world["res"][s]
        assert ok.any()
        for p in pos[ok]:
            seen = copy.deepcopy(mol)
            seen.pos = p.copy()
            assert perceive(seen).atoms[0].chiral_tag == mol.atoms[0].chiral_tag, s       # assigned from the coordinates alone
        vol = np.sign([ce.centre_volume(p, (0, 1, 2, 3)) for p in pos[ok]])
        assert (vol == vol[0]).all()
        signs[s] = vol[0]
    assert signs[EMBEDDED[0]] == 1.0 and signs[EMBEDDED[1]] == -1.0
    for s, trans in (("F/C=C/F", True), ("F/C=C\\F", False)):
        pos, ok, _ = world["res"][s]
        d = np.linalg.norm(pos[ok][:, 0] - pos[ok][:, 3], axis=1)
        print(f"{s}: F...F {d.min():.3f} .. {d.max():.3f} A")
        assert len(d) and ((d > 3.1).all() if trans else (d < 3.1).all()), (s, d)
    pos, ok, _ = world["res"]["c1ccc2[nH]ccc2c1"]
    off = []
    for p in pos[ok]:
        q = p - p.mean(0)
        off.append(float(np.abs(q @ np.linalg.svd(q)[2][-1]).max()))
    print(f"indole: largest distance of a ring atom from the plane of the nine {max(off):.4f} A")
    assert len(off) and max(off) <= ce.PLANAR_LIMIT


# ---- InferenceDataset ----------------------------------------------------------------------------------------------------------
def _inference(protein, descriptions, **kw):
    from confidence_bootstrapping_amd.inference_utils import InferenceDataset
    n = len(descriptions)
    return InferenceDataset("out", [f"c{i}" for i in range(n)], [protein] * n, descriptions, [None] * n, None, **dict(RECEPTOR, **kw))


def _graph(mol):
    g = nx.Graph()
    for a in mol.atoms:
        g.add_node(a.idx, z=a.z)
    for b in mol.bonds:
        g.add_edge(b.a, b.b, t=b.GetBondType())
    return g


def test_inference_dataset_from_the_default_smiles(protein, dev):
    from confidence_bootstrapping_amd.datasets import process_mols as pm, conformer_embedding as ce
    item = _inference(protein, [SMILES_1A0Q])[0]
    assert item.success is True and item.name == "c0" and item.mol.GetNumAtoms() == 23
    ref = pm.get_complex(protein, eh.SDF_1A0Q, "1a0q", dev)
    gm = nx.isomorphism.GraphMatcher(_graph(item.mol), _graph(ref.mol), node_match=lambda x, y: x["z"] == y["z"],
                                     edge_match=lambda x, y: x["t"] == y["t"])
    assert gm.is_isomorphic()
    perm = [gm.mapping[i] for i in range(23)]
    cols = [c for c in range(16) if c != 1]                                        # the crystal pose tags two atoms, the string none
    assert torch.equal(item["ligand"].x[:, cols], ref["ligand"].x[perm][:, cols]) and (item["ligand"].x[:, 1] == 0).all()
    assert item["ligand"].pos.shape == (23, 3) and float(item["ligand"].pos.mean(0).abs().max()) < 1e-5
    assert torch.equal(item.original_center, ref.original_center)
    assert torch.equal(item["receptor"].pos, ref["receptor"].pos) and torch.equal(item["atom"].pos, ref["atom"].pos)
    assert int(item["ligand"].edge_mask.sum()) == int(ref["ligand"].edge_mask.sum())
    lower, upper, cons = ce.distance_bounds(item.mol, None, stereo="tags")
    assert eh.accepted(item.mol.pos, lower, upper, cons, ce.BOUND_TOL, widen=BAND)
    assert np.allclose(item["ligand"].pos.numpy(), item.mol.pos - item.mol.pos.mean(0), atol=1e-5)


def test_inference_dataset_is_repeatable_and_one_launch(protein, monkeypatch):
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    calls = []
    real = ce.embed_conformers_batch

    def counting(items, *args, **kw):
        calls.append(len(items))
        return real(items, *args, **kw)

    monkeypatch.setattr(ce, "embed_conformers_batch", counting)
    three = [SMILES_1A0Q, PARACETAMOL, "[C@](F)(Cl)(Br)C"]
    abc = _inference(protein, three)
    assert calls == [3]                                                            # three good ligands: entered once
    again = _inference(protein, three)
    ab = _inference(protein, three[:2])
    with_bad = _inference(protein, [three[0], "C1CC", three[1]])                   # an unreadable ligand is left out of the launch
    assert calls == [3, 3, 2, 2]
    for i in range(3):
        assert np.array_equal(abc.mols[i].pos, again.mols[i].pos)
    for i in range(2):
        assert np.array_equal(abc.mols[i].pos, ab.mols[i].pos)
    assert with_bad.mols[1] is None and np.array_equal(with_bad.mols[0].pos, abc.mols[0].pos)
    assert not np.array_equal(with_bad.mols[2].pos, abc.mols[1].pos)               # its index in the list is its mol id
    assert not np.array_equal(_inference(protein, three[:1], seed=1).mols[0].pos, abc.mols[0].pos)


def test_inference_dataset_embeds_a_file_afresh(protein):
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    item = _inference(protein, [eh.SDF_1A0Q])[0]
    crystal = eh.ligand_1a0q()
    holo = crystal.GetConformer().GetPositions()
    assert item.success is True and [a.symbol for a in item.mol.atoms] == [a.symbol for a in crystal.atoms]
    new = item.mol.pos
    assert new.shape == holo.shape and not np.allclose(new - new.mean(0), holo - holo.mean(0), atol=0.05)
    d = lambda p: np.linalg.norm(p[:, None] - p[None], axis=-1)
    assert np.abs(d(new) - d(holo)).max() > 0.5                                    # another conformation, not the pose moved
    lower, upper, cons = ce.distance_bounds(crystal, holo)
    assert (cons["kind"] == ce.KIND_VOLUME).any()                                  # stereo from the file's pose
    assert eh.accepted(new, lower, upper, cons, ce.BOUND_TOL, widen=BAND), eh.violations(new, lower, upper, cons)


# ---- ScreeningDataset ----------------------------------------------------------------------------------------------------------
def _close_pairs(mol):
    n = mol.GetNumAtoms()
    topo = np.full((n, n), 99)
    np.fill_diagonal(topo, 0)
    for b in mol.bonds:
        topo[b.a, b.b] = topo[b.b, b.a] = 1
    for k in range(n):
        topo = np.minimum(topo, topo[:, k:k + 1] + topo[k:k + 1, :])
    return (topo == 1) | (topo == 2)


def test_screening_dataset_end_to_end(protein, dev):
    from functools import partial
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    from confidence_bootstrapping_amd.diffusion_utils import get_t_schedule, t_to_sigma
    from confidence_bootstrapping_amd.inference_utils import ScreeningDataset
    from confidence_bootstrapping_amd.sampling import sampling, randomize_position
    from confidence_bootstrapping_amd.utils import make_score_model, make_confidence_model
    model, margs = make_score_model(device=dev, seed=0)
    cmodel, cargs = make_confidence_model(device=dev, seed=5)
    lm = None
    if "precomputed" in (getattr(model, "lm_embedding_type", None), getattr(cmodel, "lm_embedding_type", None)):
        lm = np.zeros((416, 1280), dtype=np.float32)
    smiles = [SMILES_1A0Q, "C1CC", PARACETAMOL]
    ds = ScreeningDataset(protein, smiles, lm, **RECEPTOR)
    items = [ds[i] for i in range(3)]
    assert [it.success for it in items] == [True, False, True] and [it.name for it in items] == smiles
    a, b = items[0], items[2]
    assert a["receptor"].x is b["receptor"].x and a["receptor"].pos is b["receptor"].pos and a["atom"].pos is b["atom"].pos
    assert a["receptor", "receptor"].edge_index is b["receptor", "receptor"].edge_index and a.original_center is b.original_center
    assert a["ligand"].x.shape == (23, 16) and b["ligand"].x.shape == (11, 16)
    for it in (a, b):
        assert float(it["ligand"].pos.mean(0).abs().max()) < 1e-5
    torch.manual_seed(0)
    np.random.seed(0)
    data_list = []
    for it in (a, b):
        poses = [it.shallow_copy() for _ in range(2)]
        randomize_position(poses, margs.no_torsion, False, margs.tr_sigma_max)
        data_list += poses
    sched = get_t_schedule("expbeta", 2)
    out, confidence = sampling(data_list=data_list, model=model, inference_steps=2, tr_schedule=sched, rot_schedule=sched,
                               tor_schedule=sched, device=dev, t_to_sigma=partial(t_to_sigma, args=margs), model_args=margs,
                               confidence_model=cmodel, filtering_data_list=[it.shallow_copy() for it in (a, b) for _ in range(2)],
                               filtering_model_args=cargs, batch_size=2)
    assert len(out) == 4 and confidence.shape[0] == 4 and torch.isfinite(confidence).all()
    # rigid moves and torsion moves cannot change a 1-2 or a 1-3 distance; 1e-4 A covers fp32 coordinates tens of A from the origin
    for g, it in zip(out, (a, a, b, b)):
        p = g["ligand"].pos.detach().cpu().double().numpy()
        assert p.shape == (it.mol.GetNumAtoms(), 3) and np.isfinite(p).all()
        lower, upper, _ = ce.distance_bounds(it.mol, None, stereo="tags")
        dist = np.linalg.norm(p[:, None] - p[None], axis=-1)
        close = _close_pairs(it.mol)
        assert (dist[close] >= lower[close] - ce.BOUND_TOL - 1e-4).all() and (dist[close] <= upper[close] + ce.BOUND_TOL + 1e-4).all()
    assert a["receptor"].x is b["receptor"].x                                      # sampling re-binds, it does not write


# ---- tools/dock.py -------------------------------------------------------------------------------------------------------------
def _check_outputs(out, samples, symbols):
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    assert os.path.exists(os.path.join(out, "rank1.sdf"))
    for k in range(1, samples + 1):
        assert len(glob.glob(os.path.join(out, f"rank{k}_confidence*.sdf"))) == 1
    back = pm.read_molecule(os.path.join(out, "rank1.sdf"))
    assert [a.symbol for a in back.atoms] == symbols and np.isfinite(back.pos).all()
    return back


def test_dock_ligand_description(tmp_path):
    from confidence_bootstrapping_amd.datasets.smiles import mol_from_smiles
    from tools import dock
    out = str(tmp_path / "docked")
    order, data_list, confidence = dock.main(["--protein", PROTEIN_GZ, "--ligand-description", SMILES_1A0Q, "--out", out, "--samples", "2",
                                              "--steps", "2"])
    assert sorted(order) == [0, 1] and len(data_list) == 2 and confidence.shape[0] == 2
    symbols = [a.symbol for a in mol_from_smiles(SMILES_1A0Q).atoms]
    back = _check_outputs(out, 2, symbols)
    assert len(symbols) == 23
    best = data_list[order[0]]
    want = best["ligand"].pos.cpu().double().numpy() + best.original_center.cpu().double().numpy()
    assert np.abs(back.pos - want).max() <= 6e-5


def test_dock_csv(tmp_path):
    from confidence_bootstrapping_amd.datasets.smiles import mol_from_smiles
    from tools import dock
    table = tmp_path / "in.csv"
    table.write_text("complex_name,protein_path,ligand_description,protein_sequence\n"
                     f"first,{PROTEIN_GZ},{SMILES_1A0Q},\n"
                     f",{PROTEIN_GZ},{PARACETAMOL},\n"
                     f"broken,{PROTEIN_GZ},C1CC,\n")
    out = str(tmp_path / "docked")
    done = dock.main(["--protein-ligand-csv", str(table), "--out", out, "--samples", "2", "--steps", "2"])
    assert [d[0] for d in done] == ["first", "complex_1"]
    for (name, order, data_list, confidence), smiles in zip(done, (SMILES_1A0Q, PARACETAMOL)):
        assert sorted(order) == [0, 1] and confidence.shape[0] == 2
        _check_outputs(os.path.join(out, name), 2, [a.symbol for a in mol_from_smiles(smiles).atoms])
    assert not glob.glob(os.path.join(out, "broken", "*"))


def test_dock_ligand_file_is_unchanged_and_repeatable(tmp_path):
    from tools import dock
    runs = []
    for k in range(2):
        order, data_list, confidence = dock.main(["--protein", PROTEIN_GZ, "--ligand", eh.SDF_1A0Q, "--out", str(tmp_path / f"run{k}"),
                                                  "--samples", "2", "--steps", "2", "--seed", "3"])
        runs.append((order, [g["ligand"].pos.cpu().clone() for g in data_list], confidence.cpu().clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][2], runs[1][2])
    assert all(torch.equal(p, q) for p, q in zip(runs[0][1], runs[1][1]))
    # this form seeds the conformer from the file: the bond lengths of the crystal pose survive into the docked pose
    holo = eh.ligand_1a0q()
    bonds = [(b.a, b.b) for b in holo.bonds]
    length = lambda p: np.array([np.linalg.norm(p[i] - p[j]) for i, j in bonds])
    assert np.abs(length(runs[0][1][0].double().numpy()) - length(holo.pos)).max() < 1e-3
