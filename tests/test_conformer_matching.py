"""Conformer matching, host side (datasets/conformer_matching.py; reference datasets/conformer_matching.py:16-84): the torsion
quadruples against `get_transformation_mask`, the dihedral convention, setting dihedrals, and the float64 objective that the GPU
tests (tests/test_gpu_conformer_matching.py) take as truth.  No GPU."""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SDF = os.path.join(HERE, "golden", "1a0q", "1a0q_ligand.sdf")


def _flagged_bonds(edge_index, edge_mask):
    ei = np.asarray(edge_index)
    return {frozenset((int(ei[0, k]), int(ei[1, k]))) for k in np.nonzero(np.asarray(edge_mask))[0]}


def _mol_of(n, edge_index):
    from confidence_bootstrapping_amd.datasets.molfile import Atom, Bond, Mol
    ei = np.asarray(edge_index)
    return Mol([Atom(i, 6, "C") for i in range(n)], [Bond(int(ei[0, k]), int(ei[1, k]), 1) for k in range(0, ei.shape[1], 2)], np.zeros((n, 3)))


def test_torsion_bonds_are_the_edges_the_transformation_mask_flags():
    from confidence_bootstrapping_amd.datasets import process_mols as pm, conformer_matching as cm
    from confidence_bootstrapping_amd.hetero import HeteroData
    from confidence_bootstrapping_amd.torsion import get_transformation_mask
    g = pm.get_ligand(SDF, "1a0q")
    quads = cm.get_torsion_angles(g.mol)
    assert len(quads) == 11
    assert {frozenset(q[1:3]) for q in quads} == _flagged_bonds(g["ligand", "ligand"].edge_index, g["ligand"].edge_mask)
    nbr = {i: [x for x, _ in g.mol.neighbors(i)] for i in range(g.mol.GetNumAtoms())}
    for n0, e0, e1, n1 in quads:          # the outer atoms are bonded to their end of the bond and are not the other end
        assert n0 in nbr[e0] and n1 in nbr[e1] and n0 != e1 and n1 != e0
    # the random branched and ringed graphs of g17 (tests/test_ligand_featurise.py)
    g17 = np.load(os.path.join(HERE, "golden", "g17_torsion_masks.npz"))
    off, total = g17["rand_offsets"], 0
    for k, n in enumerate(g17["rand_n"].tolist()):
        ei = g17["rand_edge_index"][:, off[k]:off[k + 1]]
        hd = HeteroData()
        hd["ligand"].x = torch.zeros(n, 16, dtype=torch.long)
        hd["ligand", "lig_bond", "ligand"].edge_index = torch.as_tensor(ei, dtype=torch.long)
        me, _ = get_transformation_mask(hd)
        try:
            quads = cm.get_torsion_angles(_mol_of(n, ei))
        except ValueError:                # a bond flagged through ANOTHER fragment has no dihedral: the reference fails there too
            assert len({int(c) for c in _component_labels(n, ei)}) > 1
            continue
        assert {frozenset(q[1:3]) for q in quads} == _flagged_bonds(ei, me), (k, g17["rand_kinds"][k])
        assert len(quads) == len(_flagged_bonds(ei, me))          # a bond that the edge list repeats is flagged once per copy
        total += len(quads)
    assert total > 100


def _component_labels(n, ei):
    from confidence_bootstrapping_amd.torsion import _components
    nbr = [set() for _ in range(n)]
    for a, b in np.asarray(ei).T:
        nbr[int(a)].add(int(b))
        nbr[int(b)].add(int(a))
    return _components(n, [sorted(s) for s in nbr], (-1, -1))[0]


def test_dihedral_convention_is_iupac():
    from confidence_bootstrapping_amd.datasets.conformer_matching import get_dihedral
    u, v, k = [0.0, 0, 0], [0.0, 0, 1.5], [1.0, 0, -0.5]
    at = lambda deg: [np.cos(np.radians(deg)), np.sin(np.radians(deg)), 2.0]
    q = (0, 1, 2, 3)
    assert get_dihedral(np.array([k, u, v, at(0)]), q) == pytest.approx(0.0, abs=1e-12)               # cis
    assert abs(get_dihedral(np.array([k, u, v, at(180)]), q)) == pytest.approx(np.pi, abs=1e-12)      # trans
    # looking down u -> v (along +z, so +x points to the left when +y is up) l at +y is a quarter turn CLOCKWISE from k at +x
    assert get_dihedral(np.array([k, u, v, at(90)]), q) == pytest.approx(np.pi / 2, abs=1e-12)
    assert get_dihedral(np.array([k, u, v, at(-60)]), q) == pytest.approx(-np.pi / 3, abs=1e-12)
    p = np.array([k, u, v, at(37)])
    assert get_dihedral(p * [1, -1, 1], q) == pytest.approx(-get_dihedral(p, q), abs=1e-12)           # mirror image: sign flips
    assert get_dihedral(p, (3, 2, 1, 0)) == pytest.approx(get_dihedral(p, q), abs=1e-12)              # read from the other end: same


@pytest.fixture(scope="module")
def ligands():
    from tools.match_bench import ligand_1a0q, synthetic_ligand
    return {"1a0q": ligand_1a0q()[1:], "branched": synthetic_ligand(12, 3, 3)[1:], "long": synthetic_ligand(65, 8, 4)[1:]}


def test_apply_changes_sets_every_dihedral(ligands):
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    rng = np.random.default_rng(0)
    for name, (pos, quads, mask) in ligands.items():
        bonded = np.linalg.norm(pos[[q[1] for q in quads]] - pos[[q[2] for q in quads]], axis=1)
        for _ in range(3):
            values = rng.uniform(-np.pi, np.pi, len(quads))
            new = cm.apply_changes(pos, values, quads, mask)
            got = np.array([cm.get_dihedral(new, q) for q in quads])
            assert np.abs(np.angle(np.exp(1j * (got - values)))).max() < 1e-12, name       # independent bridges: all hold at once
            assert np.allclose(np.linalg.norm(new[[q[1] for q in quads]] - new[[q[2] for q in quads]], axis=1), bonded, atol=1e-12)
            # rows of mask_rotate in another order, or the complementary side of a bond: the same internal geometry
            perm = rng.permutation(len(quads))
            flipped = mask[perm].copy()
            flipped[0] = ~flipped[0]
            other = cm.apply_changes(pos, values, quads, flipped)
            assert cm.rigid_align(other, new)[1] < 1e-10


def test_score_is_invariant_under_rigid_motion_and_zero_at_the_answer(ligands):
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    from tools.match_bench import random_rigid
    rng = np.random.default_rng(1)
    for name, (pos, quads, mask) in ligands.items():
        values = rng.uniform(-np.pi, np.pi, len(quads))
        target = random_rigid(rng, cm.apply_changes(pos, values, quads, mask))
        assert cm.score_conformation(pos, target, values, quads, mask) < 1e-10, name
        theta = rng.uniform(-np.pi, np.pi, len(quads))
        f = cm.score_conformation(pos, target, theta, quads, mask)
        assert f > 0.1
        assert cm.score_conformation(random_rigid(rng, pos), target, theta, quads, mask) == pytest.approx(f, abs=1e-10)
        assert cm.score_conformation(pos, random_rigid(rng, target), theta, quads, mask) == pytest.approx(f, abs=1e-10)
        assert cm.score_conformation(pos, target, theta + 2 * np.pi, quads, mask) == pytest.approx(f, abs=1e-10)
    moved, left = cm.rigid_align(random_rigid(rng, pos), pos)
    assert left < 1e-10 and np.abs(moved - pos).max() < 1e-9
    assert cm.rigid_align(pos * [1, 1, -1], pos)[1] > 0.1                                  # no reflections


def test_matching_without_conformers_still_raises():
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    from confidence_bootstrapping_amd.hetero import HeteroData
    mol = pm.read_molecule(SDF, sanitize=True)
    with pytest.raises(NotImplementedError):
        pm.get_lig_graph_with_matching(mol, HeteroData(), matching=True)


def test_limits_and_missing_gpu_are_errors(ligands):
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    pos, quads, mask = ligands["branched"]
    with pytest.raises(ValueError):
        cm.optimize_rotatable_bonds(pos, pos, quads, mask, popsize=200)                    # popsize * R > 512
    with pytest.raises(ValueError):
        cm.optimize_rotatable_bonds(pos, pos, quads, mask[:2])
    with pytest.raises(ValueError):
        cm.apply_changes(pos, np.zeros(3), quads, np.zeros_like(mask))                     # no side of any bond
    out, values, rmsd = cm.optimize_rotatable_bonds(pos + 1.0, pos, [], np.zeros((0, len(pos)), bool))     # R = 0: host only
    assert values.shape == (0,) and rmsd < 1e-10 and np.array_equal(out, pos + 1.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            cm.optimize_rotatable_bonds(pos, pos, quads, mask, maxiter=1)
