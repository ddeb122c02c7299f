"""The pose writers on the host: `process_mols.write_mol_with_coords` (V2000 SDF of a `molfile.Mol`), `visualise.PDBFile` (MODEL frames
of a reverse process) and `docking.write_ranked_poses` (the file set of the reference's dock.py:158-184).  No GPU.

Tolerances: an SDF coordinate is written with four decimals (<= 5e-5 A) from an fp32 sum whose half-ulp below 128 A is 3.8e-6 A:
6e-5 A.  A PDB coordinate has three decimals (<= 5e-4 A) plus the same half-ulp: 5.1e-4 A."""
import glob
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SDF = os.path.join(HERE, "golden", "1a0q", "1a0q_ligand.sdf")
SDF_TOL, PDB_TOL = 6e-5, 5.1e-4


@pytest.fixture(scope="module")
def lig():
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    mol = pm.read_molecule(SDF, sanitize=True, remove_hs=True)
    assert mol.GetNumAtoms() == 23
    return mol


def _models(text):
    """-> list of (coords [n, 3] from columns 31-54, element column, number of CONECT lines) per MODEL ... ENDMDL pair"""
    out, cur = [], None
    for line in text.splitlines():
        if line == "MODEL":
            assert cur is None
            cur = ([], [], 0)
        elif line == "ENDMDL":
            out.append((np.asarray(cur[0]), cur[1], cur[2]))
            cur = None
        elif line.startswith("HETATM"):
            assert len(line) == 80 and line[17:20] == "UNL"
            cur[0].append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
            cur[1].append(line[76:78].strip())
        elif line.startswith("CONECT"):
            cur = (cur[0], cur[1], cur[2] + 1)
        else:
            raise AssertionError(f"unexpected line {line!r}")
    assert cur is None
    return out


def test_sdf_round_trip(lig, tmp_path):
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    before = lig.pos.copy()
    new = (lig.pos + np.array([1.23456, -7.654321, 0.5])).astype(np.float32)
    path = str(tmp_path / "pose.sdf")
    pm.write_mol_with_coords(lig, new, path)
    text = open(path).read()
    assert text.rstrip("\n").endswith("$$$$") and text.splitlines()[0] == lig.name
    back = pm.read_molecule(path)
    assert back.GetNumAtoms() == lig.GetNumAtoms() == 23
    assert [a.symbol for a in back.atoms] == [a.symbol for a in lig.atoms]
    assert [(b.a, b.b, b.type) for b in back.bonds] == [(b.a, b.b, b.type) for b in lig.bonds]
    assert 4 in {b.type for b in back.bonds}                     # the perceived aromatic ring travels as bond type 4
    assert [a.charge for a in back.atoms] == [a.charge for a in lig.atoms]
    err = np.abs(back.pos - new.astype(np.float64)).max()
    print(f"SDF round trip: max |dx| = {err:.2e} A")
    assert err <= SDF_TOL
    assert np.array_equal(lig.pos, before)


def test_sdf_charges_and_limits(lig, tmp_path):
    import copy
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    from confidence_bootstrapping_amd.datasets.molfile import Atom, Mol
    charged = copy.deepcopy(lig)
    for k, q in ((19, -1), (21, 1), (3, -4)):                   # -4 has no atom-block code: the M  CHG line carries it
        charged.atoms[k].charge = q
    path = str(tmp_path / "charged.sdf")
    pm.write_mol_with_coords(charged, torch.from_numpy(charged.pos), path)
    assert [a.charge for a in pm.read_molecule(path).atoms] == [a.charge for a in charged.atoms]
    big = Mol([Atom(i, 6, "C") for i in range(1000)], [], np.zeros((1000, 3)))
    with pytest.raises(ValueError):
        pm.write_mol_with_coords(big, big.pos, str(tmp_path / "big.sdf"))
    with pytest.raises(ValueError):
        pm.write_mol_with_coords(lig, lig.pos[:5], str(tmp_path / "short.sdf"))


def test_pdbfile_framing(lig, tmp_path):
    from confidence_bootstrapping_amd.visualise import PDBFile
    rng = np.random.default_rng(0)
    S, n = 3, lig.GetNumAtoms()
    center = np.array([[12.5, -3.25, 40.0]], dtype=np.float32)
    frame = lambda: torch.from_numpy((rng.normal(0, 5, size=(n, 3)).astype(np.float32) + center))
    pdb = PDBFile(lig)
    added = {}                                                   # (part, order) -> coordinates, repeat

    def add(coords, order, part, repeat=1):
        pdb.add(coords, order, part, repeat) if repeat != 1 else pdb.add(coords, order, part)
        added[(part, order)] = (lig.pos if coords is lig else np.asarray(coords, dtype=np.float64), repeat)
    # the pattern of the reference's dock.py:140-146, then S step frames added out of order, a negative order and a repeat
    add(lig, 0, 0)
    add(frame(), 0, 1)
    add(frame().numpy(), 1, 1)
    for k in (2, 0, 1):
        add(frame(), k + 2, 1, repeat=2 if k == 1 else 1)
    add(frame(), -1, 1)
    add(frame(), -3, 1)
    text = pdb.write()
    models = _models(text)
    # parts ascending; within a part the non-negative orders ascending, then the negative ones ascending
    expect = [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 3), (1, 4), (1, -3), (1, -1)]
    assert text.count("MODEL\n") == text.count("ENDMDL\n") == len(models) == len(expect) == (S + 3) + 1 + 2
    worst = 0.0
    for (coords, elements, n_conect), key in zip(models, expect):
        assert elements == [a.symbol.upper() for a in lig.atoms]
        worst = max(worst, np.abs(coords - added[key][0]).max())
    print(f"PDB frames: max |dx| = {worst:.2e} A")
    assert worst <= PDB_TOL
    assert models[0][2] == n and all(m[2] == 0 for m in models[1:])          # one CONECT line per (bonded) atom, first model only
    # without the two extra negative frames and the repeat: exactly S + 3 models
    plain = PDBFile(lig)
    plain.add(lig, 0, 0)
    for order in range(S + 2):
        plain.add(frame(), part=1, order=order)
    assert len(_models(plain.write())) == S + 3
    assert len(_models(plain.write(limit_parts=1))) == 1
    # the same text with a path
    path = str(tmp_path / "frames.pdb")
    assert pdb.write(path) is None
    assert open(path).read() == text
    with pytest.raises(ValueError):
        pdb.add(np.zeros((n + 1, 3)), 9, 1)


class _Store(dict):
    __getattr__ = dict.__getitem__


class _StubGraph:
    def __init__(self, pos, center):
        self._lig = _Store(pos=pos)
        self.original_center = center

    def __getitem__(self, key):
        assert key == "ligand"
        return self._lig


def test_write_ranked_poses(lig, tmp_path):
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    from confidence_bootstrapping_amd.docking import write_ranked_poses
    from confidence_bootstrapping_amd.visualise import PDBFile
    rng = np.random.default_rng(1)
    n, N = lig.GetNumAtoms(), 4
    center = torch.tensor([[20.0, 15.0, 50.0]])
    data_list = [_StubGraph(torch.from_numpy(rng.normal(0, 4, size=(n, 3)).astype(np.float32)), center) for _ in range(N)]
    confidence = torch.tensor([-1.5, 0.25, float("nan"), -0.125])
    vis = []
    for g in data_list:
        p = PDBFile(lig)
        p.add(g["ligand"].pos + center, 0, 0)
        vis.append(p)
    out = str(tmp_path / "ranked")
    order = write_ranked_poses(out, lig, data_list, confidence, vis)
    assert order == [1, 2, 3, 0]                                 # NaN counts as -1e-6: between +0.25 and -0.125
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, "*")))
    assert names == sorted(["rank1.sdf", "rank1_confidence0.25.sdf", "rank2_confidence-0.00.sdf", "rank3_confidence-0.12.sdf",
                            "rank4_confidence-1.50.sdf"] + [f"rank{k}_reverseprocess.pdb" for k in range(1, 5)])
    assert open(os.path.join(out, "rank1.sdf")).read() == open(os.path.join(out, "rank1_confidence0.25.sdf")).read()
    for rank, idx in enumerate(order):
        sdf = glob.glob(os.path.join(out, f"rank{rank + 1}_confidence*.sdf"))[0]
        want = data_list[idx]["ligand"].pos.double().numpy() + center.double().numpy()
        assert np.abs(pm.read_molecule(sdf).pos - want).max() <= SDF_TOL
        frames = _models(open(os.path.join(out, f"rank{rank + 1}_reverseprocess.pdb")).read())
        assert len(frames) == 1 and np.abs(frames[0][0] - want).max() <= PDB_TOL
    # no confidence: data_list order, rank{k}.sdf only
    out2 = str(tmp_path / "unranked")
    assert write_ranked_poses(out2, lig, data_list, None) == [0, 1, 2, 3]
    assert sorted(os.listdir(out2)) == [f"rank{k}.sdf" for k in range(1, 5)]
    want = data_list[2]["ligand"].pos.double().numpy() + center.double().numpy()
    assert np.abs(pm.read_molecule(os.path.join(out2, "rank3.sdf")).pos - want).max() <= SDF_TOL
