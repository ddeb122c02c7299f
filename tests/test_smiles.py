"""The SMILES reader (datasets/smiles.py) and stereo from the molecule in `distance_bounds(..., stereo="tags")`, on the CPU.

Oracles that do not use the parser: a table derived by hand; the 1a0q ligand read from its SDF fixture (the reference's default
`--ligand_description` is the same molecule); `tests/embed_helpers.chiral`, whose two enantiomers `perceive` tags from their poses."""
import collections
import itertools

import networkx as nx
import numpy as np
import pytest

from tests import embed_helpers as eh
from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
from confidence_bootstrapping_amd.datasets import process_mols as pm
from confidence_bootstrapping_amd.datasets.smiles import mol_from_smiles
from confidence_bootstrapping_amd.hetero import HeteroData

SMILES_1A0Q = "CCCCC(NC(=O)CCC(=O)O)P(=O)(O)OC1=CC=CC=C1"
CCW, CW, NONE = "CHI_TETRAHEDRAL_CCW", "CHI_TETRAHEDRAL_CW", "CHI_UNSPECIFIED"

# smiles: (elements in order, bonds, charges, hydrogens, aromatic flags, ring sizes) -- written down by hand from the structures
TABLE = {
    "C": ("C", 0, "0", "4", "0", []),
    "CCO": ("CCO", 2, "000", "321", "000", []),
    "C#N": ("CN", 1, "00", "10", "00", []),
    "C1CC1": ("CCC", 3, "000", "222", "000", [3]),
    "C%10CC%10": ("CCC", 3, "000", "222", "000", [3]),
    "c1ccccc1": ("CCCCCC", 6, "000000", "111111", "111111", [6]),
    "C1=CC=CC=C1": ("CCCCCC", 6, "000000", "111111", "111111", [6]),
    "n1ccccc1": ("NCCCCC", 6, "000000", "011111", "111111", [6]),
    "c1cc[nH]c1": ("CCCNC", 5, "00000", "11111", "11111", [5]),
    "c1ccc2[nH]ccc2c1": ("CCCCNCCCC", 10, "000000000", "111011101", "111111111", [5, 6]),
    "C[N+](C)(C)C": ("CNCCC", 4, "0+000", "30333", "00000", []),
    "[O-]C(=O)c1ccccc1": ("OCOCCCCCC", 9, "-00000000", "000011111", "000111111", [6]),
    "C[N+](=O)[O-]": ("CNOO", 3, "0+0-", "3000", "0000", []),
    "[NH4+]": ("N", 0, "+", "4", "0", []),
    "[13CH4]": ("C", 0, "0", "4", "0", []),
    "C(F)(F)(F)c1ccccc1": ("CFFFCCCCCC", 10, "0000000000", "0000011111", "0000111111", [6]),
    "C1CC2CCC1C2": ("CCCCCCC", 8, "0000000", "2212212", "0000000", [5, 5]),
    "C=1CCCCC1": ("CCCCCC", 6, "000000", "122221", "000000", [6]),
    "C1=CCCCC1": ("CCCCCC", 6, "000000", "112222", "000000", [6]),
}
REFUSED = ["C(", "C1CC", "C1CC=1", "Xx", "*", "C.C", "", "[C@TH1](F)(Cl)(Br)I", "c1cccc1", "[CH2]C"]


def _summary(mol):
    return ([a.symbol for a in mol.atoms], [a.charge for a in mol.atoms], [a.num_hs for a in mol.atoms], [bool(a.aromatic) for a in mol.atoms],
            [(b.a, b.b, b.type) for b in mol.bonds], sorted(len(r) for r in mol.GetRingInfo().AtomRings()))


@pytest.mark.parametrize("smiles", list(TABLE))
def test_hand_derived_table(smiles):
    elements, n_bonds, charges, hs, arom, rings = TABLE[smiles]
    mol = mol_from_smiles(smiles)
    assert mol.perceived and mol.GetNumConformers() == 0 and mol.pos.shape == (0, 3)
    assert mol.GetNumAtoms() == len(elements) and len(mol.GetBonds()) == n_bonds
    assert "".join(a.symbol for a in mol.atoms) == elements
    assert [a.charge for a in mol.atoms] == [{"0": 0, "+": 1, "-": -1}[c] for c in charges]
    assert [a.num_hs for a in mol.atoms] == [int(c) for c in hs]
    assert [int(a.aromatic) for a in mol.atoms] == [int(c) for c in arom]
    assert sorted(len(r) for r in mol.GetRingInfo().AtomRings()) == rings
    assert [a.idx for a in mol.atoms] == list(range(len(elements)))


def test_atom_and_bond_order_follow_the_string():
    mol = mol_from_smiles("C1CC2CCC1C2")
    # bonds in the order they are completed: a ring-closure bond when its second digit is read
    assert [{b.a, b.b} for b in mol.bonds] == [{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 0}, {5, 6}, {6, 2}]
    assert [b.GetBondType() for b in mol_from_smiles("C=CC#N").bonds] == ["DOUBLE", "SINGLE", "TRIPLE"]
    assert [b.GetBondType() for b in mol_from_smiles("c1ccccc1-c1ccccc1").bonds][6] == "SINGLE"
    assert [b.GetBondType() for b in mol_from_smiles("c1ccccc1c1ccccc1").bonds][6] == "SINGLE"       # not in a ring: not aromatic
    assert [a.symbol for a in mol_from_smiles("[H]C([H])([H])Cl").atoms] == ["H", "C", "H", "H", "Cl"]   # explicit [H] stay atoms
    for text, charge in (("[O-]C", -1), ("[O-1]C", -1), ("C[NH3+]", 1), ("C[NH3+1]", 1), ("[Cu+2]", 2), ("[Cu++]", 2), ("[Fe+3]", 3)):
        assert [a.charge for a in mol_from_smiles(text).atoms if a.charge] == [charge], text
    assert mol_from_smiles("[CH3:7]C").atoms[0].num_hs == 3                                           # atom class: read and dropped


def test_kekule_and_aromatic_spellings_are_one_molecule():
    assert _summary(mol_from_smiles("c1ccccc1")) == _summary(mol_from_smiles("C1=CC=CC=C1"))
    assert _summary(mol_from_smiles("c1ccccc1")) == _summary(mol_from_smiles("c:1:c:c:c:c:c1"))
    a, b = _summary(mol_from_smiles("C=1CCCCC1")), _summary(mol_from_smiles("C1=CCCCC1"))
    assert a[0] == b[0] and a[5] == b[5]
    # the same cyclohexene: one double bond, between the opening atom and the closing one / the first two atoms
    assert [t for _, _, t in a[4]].count(2) == 1 and {a[4][5][0], a[4][5][1]} == {0, 5} and a[4][5][2] == 2 and b[4][0] == (0, 1, 2)
    assert _summary(mol_from_smiles("C=1CCCCC=1")) == a
    indole = mol_from_smiles("c1ccc2[nH]ccc2c1")
    assert all(b.GetBondType() == "AROMATIC" for b in indole.bonds)


@pytest.mark.parametrize("smiles", REFUSED)
def test_refused(smiles):
    with pytest.raises(ValueError, match=r"position \d+"):
        mol_from_smiles(smiles)


def test_more_refusals_name_the_position():
    for text, pos in (("CC)", 2), ("CC$C", 2), ("C[Zz]", 2), ("C[C@SP1](F)(Cl)(Br)I", 4), ("C[C@AL1](F)(Cl)(Br)I", 4), ("CC(", 2),
                      ("C2CC", 1), ("CC*", 2), ("C-1CCC=1", 7), ("C=", 1)):
        with pytest.raises(ValueError, match=rf"position {pos}\b"):
            mol_from_smiles(text)


# ---- the reference's default ligand -----------------------------------------------------------------------------------------------
def _graph(mol):
    g = nx.Graph()
    for a in mol.atoms:
        g.add_node(a.idx, z=a.z)
    for b in mol.bonds:
        g.add_edge(b.a, b.b, t=b.GetBondType())
    return g


@pytest.fixture(scope="module")
def pair_1a0q():
    smi, ref = mol_from_smiles(SMILES_1A0Q), eh.ligand_1a0q()
    gm = nx.isomorphism.GraphMatcher(_graph(smi), _graph(ref), node_match=lambda x, y: x["z"] == y["z"], edge_match=lambda x, y: x["t"] == y["t"])
    return smi, ref, gm


def test_default_ligand_matches_the_sdf_fixture(pair_1a0q):
    smi, ref, gm = pair_1a0q
    assert ref.GetNumAtoms() == 23 and collections.Counter(a.symbol for a in ref.atoms) == {"C": 15, "N": 1, "O": 6, "P": 1}
    assert collections.Counter(b.GetBondType() for b in ref.bonds) == {"SINGLE": 14, "AROMATIC": 6, "DOUBLE": 3}
    assert smi.GetNumAtoms() == 23 and len(smi.bonds) == 23
    assert gm.is_isomorphic()
    to_ref = gm.mapping
    fs, fr = pm.lig_atom_featurizer(smi), pm.lig_atom_featurizer(ref)
    perm = [to_ref[i] for i in range(23)]
    cols = [c for c in range(16) if c != 1]
    assert (fs[:, cols] == fr[perm][:, cols]).all()
    assert (fs[:, 1] == 0).all()                                  # the string carries no tags
    assert sorted(int(i) for i in np.nonzero(fr[:, 1].numpy())[0]) == sorted(a.idx for a in ref.atoms if a.chiral_tag != NONE)
    tagged = [a for a in ref.atoms if a.chiral_tag != NONE]        # the crystal pose tags the C-N/P carbon and the phosphorus
    assert sorted(a.symbol for a in tagged) == ["C", "P"]


def test_default_ligand_has_the_same_rotatable_bonds(pair_1a0q):
    smi, ref, _ = pair_1a0q
    masks = []
    for mol in (smi, ref):
        g = HeteroData()
        pm.get_lig_graph(mol, g)
        edge_mask, mask_rotate = pm.get_transformation_mask(g)
        masks.append((int(np.asarray(edge_mask).sum()), sorted(int(r) for r in np.asarray(mask_rotate).sum(axis=1))))
        assert "pos" not in g["ligand"] or mol is ref
    assert masks[0] == masks[1] and masks[0][0] > 0


# ---- tetrahedral tags -------------------------------------------------------------------------------------------------------------
def _tag_in_reference_order(mol, centre, order=(9, 17, 35, 6)):
    """The centre's tag restated for its neighbours listed as F, Cl, Br, C (the order of embed_helpers.chiral): one flip per
    transposition between the molecule's bond order and that order.  Neighbours are told apart by element."""
    zs = [mol.atoms[j].z for j, _ in mol.neighbors(centre)]
    assert sorted(zs) == sorted(order)
    perm = [order.index(z) for z in zs]
    odd = sum(1 for x, y in itertools.combinations(range(4), 2) if perm[x] > perm[y]) % 2
    tag = mol.atoms[centre].chiral_tag
    assert tag in (CCW, CW)
    return tag if not odd else (CW if tag == CCW else CCW)


def test_tags_agree_with_the_poses_perceive_tags():
    want = {False: eh.chiral(False).atoms[0].chiral_tag, True: eh.chiral(True).atoms[0].chiral_tag}
    assert want == {False: CCW, True: CW}
    for mirror, text in ((False, "[C@](F)(Cl)(Br)C"), (True, "[C@@](F)(Cl)(Br)C")):
        mol = mol_from_smiles(text)
        assert mol.atoms[0].chiral_tag == want[mirror]
        assert [a.chiral_tag for a in mol.atoms[1:]] == [NONE] * 4
        ref = eh.chiral(mirror)
        lo_t, up_t, cons_t = ce.distance_bounds(mol, None, stereo="tags")
        lo_p, up_p, cons_p = ce.distance_bounds(ref, ref.GetConformer().GetPositions())
        assert np.array_equal(lo_t, lo_p) and np.array_equal(up_t, up_p)
        for k in ("idx", "kind", "lo", "hi"):
            assert np.array_equal(cons_t[k], cons_p[k]), k
        assert (cons_t["kind"] == ce.KIND_VOLUME).all()


SPELLINGS = [          # (the same enantiomer as chiral(False) -- [C@](F)(Cl)(Br)C --, index of the centre)
    ("F[C@](Cl)(Br)C", 1), ("Cl[C@](Br)(F)C", 1), ("C[C@@](F)(Cl)Br", 1), ("Br[C@@](C)(Cl)F", 1),       # another start atom
    ("[C@@](Cl)(F)(Br)C", 0), ("[C@@](Cl)(Br)(C)F", 0), ("[C@@](F)(Cl)(C)Br", 0), ("[C@](Br)(F)(Cl)C", 0),   # neighbours permuted
]


@pytest.mark.parametrize("text,centre", SPELLINGS)
def test_spellings_of_one_enantiomer(text, centre):
    assert _tag_in_reference_order(mol_from_smiles(text), centre) == CCW
    mirror = text.replace("@@", "!").replace("@", "@@").replace("!", "@")
    assert _tag_in_reference_order(mol_from_smiles(mirror), centre) == CW


def test_ring_closure_digits_count_where_they_are_written():
    # a four-ring through the centre: C1 (centre) F, Cl substituents; ring atoms N and O tell the two ring neighbours apart.
    # [C@]1(F)(Cl)NCO1 lists the centre's neighbours as O (the digit), F, Cl, N; the bond to O is completed last.
    # Looking from O: F, Cl, N counter-clockwise.  Written without a digit on the centre, from O: O1[C@](F)(Cl)NC1.
    ring = mol_from_smiles("[C@]1(F)(Cl)NCO1")
    chain = mol_from_smiles("O1[C@](F)(Cl)NC1")
    assert [a.symbol for a in ring.atoms] == ["C", "F", "Cl", "N", "C", "O"]

    def in_order(mol, centre, order=(8, 9, 17, 7)):
        return _tag_in_reference_order(mol, centre, order)
    assert ring.atoms[0].chiral_tag in (CCW, CW) and chain.atoms[1].chiral_tag in (CCW, CW)
    assert in_order(ring, 0) == in_order(chain, 1) == CCW            # written order (O, F, Cl, N) with @: CCW in that order
    assert ring.atoms[0].chiral_tag == CW                            # bond order is F, Cl, N, O: an odd permutation of it
    assert in_order(mol_from_smiles("[C@@]1(F)(Cl)NCO1"), 0) == CW
    # the digit written after the substituents: neighbours F, Cl, O, N
    assert in_order(mol_from_smiles("[C@](F)(Cl)1NCO1"), 0, (9, 17, 8, 7)) == CCW


def test_implicit_hydrogen():
    a, b = mol_from_smiles("N[C@@H](C)C(=O)O"), mol_from_smiles("N[C@H](C(=O)O)C")
    # neighbours of the centre: N, CH3, COOH in a / N, COOH, CH3 in b -- one transposition apart, so opposite tags are one molecule
    assert a.atoms[1].num_hs == 1 and b.atoms[1].num_hs == 1
    assert {a.atoms[1].chiral_tag, b.atoms[1].chiral_tag} == {CCW, CW}
    # L-alanine N[C@@H](C)C(=O)O: H is the neighbour written after the atom: (N, H, CH3, COOH) clockwise.  H moved to the end is
    # two transpositions: (N, CH3, COOH, H) clockwise
    assert a.atoms[1].chiral_tag == CW
    # the atom opens the string: H is the "from" neighbour.  [C@@H](N)(C)C(=O)O = (H, N, CH3, COOH) clockwise; H to the end is three
    # transpositions: (N, CH3, COOH, H) counter-clockwise -- D-alanine
    c = mol_from_smiles("[C@@H](N)(C)C(=O)O")
    assert c.atoms[0].chiral_tag == CCW
    assert mol_from_smiles("[C@H](N)(C)C(=O)O").atoms[0].chiral_tag == CW


def test_tag_on_a_non_stereocentre_is_dropped():
    assert [a.chiral_tag for a in mol_from_smiles("C[C@H](C)O").atoms] == [NONE] * 4
    assert [a.chiral_tag for a in mol_from_smiles("C[C@@](C)(F)Cl").atoms] == [NONE] * 5
    assert mol_from_smiles("C[C@H](N)O").atoms[1].chiral_tag != NONE


def test_perceive_uses_the_shared_stereocentre_test():
    from confidence_bootstrapping_amd.datasets import molfile
    mol = eh.chiral(False)
    cls = molfile._symmetry_classes(mol)
    assert [molfile.is_stereocentre(mol, i, cls) for i in range(5)] == [True, False, False, False, False]
    lig = eh.ligand_1a0q()
    cls = molfile._symmetry_classes(lig)
    assert [a.idx for a in lig.atoms if a.chiral_tag != NONE] == [i for i in range(23) if molfile.is_stereocentre(lig, i, cls)]


# ---- double bonds -----------------------------------------------------------------------------------------------------------------
def test_double_bond_stereo():
    trans1, trans2, cis = mol_from_smiles("F/C=C/F"), mol_from_smiles("F\\C=C\\F"), mol_from_smiles("F/C=C\\F")
    assert trans1.double_bond_stereo == [(0, 1, 2, 3, "trans")] and trans2.double_bond_stereo == [(0, 1, 2, 3, "trans")]
    assert cis.double_bond_stereo == [(0, 1, 2, 3, "cis")] and mol_from_smiles("F\\C=C/F").double_bond_stereo == [(0, 1, 2, 3, "cis")]
    assert mol_from_smiles("FC=CF").double_bond_stereo == [] and mol_from_smiles("F/C=CF").double_bond_stereo == []
    # a branch: C(/F)=C/F reads the first bond from the carbon: F above C0, F above C1 -> cis
    assert mol_from_smiles("C(/F)=C/F").double_bond_stereo == [(1, 0, 2, 3, "cis")]
    lo_t, up_t, _ = ce.distance_bounds(trans1, None, stereo="tags")
    lo_c, up_c, _ = ce.distance_bounds(cis, None, stereo="tags")
    assert lo_t[0, 3] > up_c[0, 3]
    assert lo_t[0, 3] < 3.56 < up_t[0, 3] and lo_c[0, 3] < 2.69 < up_c[0, 3]       # C=C 1.34, C-F 1.35 at 120 degrees
    plain = [ce.distance_bounds(m, None, stereo="pose") for m in (trans1, cis)]
    assert np.array_equal(plain[0][0], plain[1][0]) and np.array_equal(plain[0][1], plain[1][1])
    assert plain[0][0][0, 3] <= lo_c[0, 3] and plain[0][1][0, 3] >= up_t[0, 3]      # today's range holds both sides
    # the other substituent of an end lies on the other side: Cl is cis to the far F where the near F is trans
    mol = mol_from_smiles("F/C(Cl)=C/F")
    lo, up, _ = ce.distance_bounds(mol, None, stereo="tags")
    assert mol.double_bond_stereo == [(0, 1, 3, 4, "trans")] and lo[0, 4] > 3.1 and up[2, 4] < 3.3


# ---- unchanged behaviour ----------------------------------------------------------------------------------------------------------
def test_pose_mode_is_the_default_and_unchanged():
    for name, (mol, ref) in eh.molecules().items():
        a, b = ce.distance_bounds(mol, ref), ce.distance_bounds(mol, ref, stereo="pose")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
        for k in ("idx", "kind", "lo", "hi"):
            assert np.array_equal(a[2][k], b[2][k]), (name, k)
    mol = eh.chiral(False)
    kinds = ce.distance_bounds(mol, None)[2]["kind"]
    assert len(kinds) and (kinds == ce.KIND_ABS_VOLUME).all()
    assert (ce.distance_bounds(mol, None, stereo="tags")[2]["kind"] == ce.KIND_VOLUME).all()      # perceive's tag, no pose needed
    untagged = mol_from_smiles("C(F)(Cl)(Br)C")
    assert (ce.distance_bounds(untagged, None, stereo="tags")[2]["kind"] == ce.KIND_ABS_VOLUME).all()
    with pytest.raises(ValueError):
        ce.distance_bounds(mol, None, stereo="smiles")


def test_remove_hs_keeps_the_records():
    from confidence_bootstrapping_amd.datasets.molfile import remove_hs
    mol = remove_hs(mol_from_smiles("[H]C(/F)=C/F"))
    assert [a.symbol for a in mol.atoms] == ["C", "F", "C", "F"] and mol.double_bond_stereo == [(1, 0, 2, 3, "cis")]
    assert mol.atoms[0].num_hs == 1 and mol.GetNumConformers() == 0
