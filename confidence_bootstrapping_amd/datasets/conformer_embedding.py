"""Ligand conformers by distance geometry on the GPU (the first half of the reference's conformer matching, `generate_conformer` at
datasets/process_mols.py:591-607, which calls rdkit's ETKDG embedding).

What the pipeline needs from an embedded conformer is a sound LOCAL structure -- bond lengths, angles, ring shapes, planar sp2
centres, the right handedness -- because every rotatable torsion is overwritten afterwards (torsion matching, randomize_position).
So this is plain distance geometry, rdkit's `useRandomCoords` route without the "experimental torsion knowledge" of ETKDG:

host   `distance_bounds`: lower / upper bounds on every pair distance from hand-written tables (1-2 from bond lengths, 1-3 from
       angles, 1-4 from the cis / trans extremes of the torsion, the rest from van-der-Waals radii), triangle-smoothed, plus volume
       constraints (sp3 centres keep their handedness and do not flatten) and planarity constraints (sp2 centres, aromatic rings);
device `cbd_embed_conformers` (csrc/conformer_embed.hip): random 4-D coordinates, FIRE minimisation of rdkit's distance-violation
       error with the fourth dimension squeezed out, a 3-D refinement, and the acceptance test `ok` per conformer.

Deviations from the reference's ETKDG, all deliberate:
  * hydrogens are NOT added.  The reference embeds `AddHs(mol)` and strips them again; here the atoms are used as given (heavy atoms
    after `remove_hs`, or with the explicit hydrogens of the file).  Heavy-atom geometry is fixed by the 1-2 / 1-3 / 1-4 bounds alike.
  * no torsion preferences and no metric-matrix eigen-embedding (random start coordinates only).
  * stereo comes from a 3-D input pose (`ref_pos`; `stereo="pose"`, the default): the sign of every sp3 centre's neighbour volume,
    and the cis / trans side of double and amide bonds, are read from it.  A flat or missing `ref_pos` gives no sign constraints (the
    centres are still kept from flattening, with either hand) and leaves double / amide bonds their whole cis..trans range.
    A molecule without a pose -- one read from a SMILES (datasets/smiles.py) -- carries its stereo on itself: `stereo="tags"` takes
    the sign of a centre's volume from its `chiral_tag` and the side of a double bond from `mol.double_bond_stereo`; a centre without
    a tag and a double bond without a record get what a missing pose gives.  Amide bonds have no record: an unflagged amide may
    come out cis, where ETKDG's torsion preferences would make it trans.
  * at most 256 atoms.

Sources of the tables: covalent radii -- Cordero et al., Dalton Trans. 2008; typical bond lengths by class -- Allen et al., J. Chem.
Soc. Perkin Trans. 2 1987 (S1-S19); van-der-Waals radii -- the values rdkit's periodic table carries (Bondi / Blue Obelisk); the
1-5 / 1-6 scaling of the van-der-Waals sum -- rdkit's BoundsMatrixBuilder (0.7 / 0.85).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

MAX_ATOMS = 256            # csrc/conformer_embed.hip: CE_MAX_N
MAX_CONSTRAINTS = 1024     # CE_MAX_CONS
BOUND_TOL = 0.05           # A: the acceptance band around [lower, upper] (between the 0.09 A that separates the
#                            bond classes the table tells apart and the 0.02 A spread inside one class)
# largest out-of-plane distance of an sp2 centre of the 1a0q crystal ligand (measured in tests/test_conformer_embedding.py) + BOUND_TOL
PLANAR_LIMIT = 0.134 + BOUND_TOL
BOND_TOL = 0.01            # 1-2 bounds are ideal +- this
ANGLE_TOL = 0.04           # 1-3 bounds are ideal +- this (rdkit's), times the centre's softness below
GEN_TOL = 0.06             # 1-4 bounds are widened by this (rdkit's GEN_DIST_TOL)
VOLUME_FLOOR = 0.5         # |V| of an sp3 centre stays above this share of its ideal value
UMBRELLA_FLOOR = 0.7       # the same for the tetrahedron of a centre's four neighbours (an inverted umbrella has half the ideal volume)
UPPER_FAR = 1000.0
KIND_VOLUME, KIND_ABS_VOLUME, KIND_PLANAR = 0, 1, 2

# ---- tables -----------------------------------------------------------------------------------------------------------------------
_COVALENT = {1: 0.31, 5: 0.84, 6: 0.76, 7: 0.71, 8: 0.66, 9: 0.57, 14: 1.11, 15: 1.07, 16: 1.05, 17: 1.02, 33: 1.19, 34: 1.20, 35: 1.20,
             53: 1.39}
_VDW = {1: 1.2, 5: 2.0, 6: 1.7, 7: 1.6, 8: 1.55, 9: 1.5, 14: 2.1, 15: 1.95, 16: 1.8, 17: 1.8, 33: 2.05, 34: 1.9, 35: 1.9, 53: 2.1}
_ORDER_SHORTENING = {"DOUBLE": 0.19, "TRIPLE": 0.32, "AROMATIC": 0.13}      # C-C 1.52 -> C=C 1.33, C#C 1.20, aromatic 1.39
# (lower Z, higher Z, class) -> A.  Classes: S single, D double, T triple, A aromatic, C conjugated single (amide, ester, carboxylate,
# phosphonate / sulfonyl oxygen).  Whatever is not listed is the sum of the covalent radii less the bond-order shortening.
_BOND_LENGTH = {
    (1, 6, "S"): 1.09, (1, 7, "S"): 1.01, (1, 8, "S"): 0.96, (1, 16, "S"): 1.34,
    (6, 6, "S"): 1.53, (6, 6, "D"): 1.34, (6, 6, "T"): 1.20, (6, 6, "A"): 1.39,
    (6, 7, "S"): 1.47, (6, 7, "D"): 1.28, (6, 7, "T"): 1.14, (6, 7, "A"): 1.34, (6, 7, "C"): 1.34,
    (6, 8, "S"): 1.43, (6, 8, "D"): 1.23, (6, 8, "A"): 1.37, (6, 8, "C"): 1.34,
    (6, 9, "S"): 1.35, (6, 15, "S"): 1.78, (6, 16, "S"): 1.81, (6, 16, "D"): 1.67, (6, 16, "A"): 1.72, (6, 17, "S"): 1.77,
    (6, 35, "S"): 1.94, (6, 53, "S"): 2.14, (5, 6, "S"): 1.57, (5, 8, "S"): 1.37, (6, 14, "S"): 1.87, (8, 14, "S"): 1.63,
    (7, 7, "S"): 1.42, (7, 7, "D"): 1.25, (7, 7, "A"): 1.33, (7, 8, "S"): 1.40, (7, 8, "D"): 1.22, (7, 8, "A"): 1.40, (7, 8, "C"): 1.22,
    (7, 15, "S"): 1.65, (7, 16, "S"): 1.63, (7, 16, "A"): 1.65,
    (8, 15, "S"): 1.60, (8, 15, "D"): 1.48, (8, 15, "C"): 1.49, (8, 16, "S"): 1.58, (8, 16, "D"): 1.43, (8, 16, "C"): 1.45,
    (15, 16, "S"): 2.08, (15, 16, "D"): 1.92, (16, 16, "S"): 2.05,
}
_AROMATIC_SUBSTITUENT = {7: 1.39, 8: 1.39, 16: 1.77, 17: 1.74, 35: 1.90, 53: 2.10, 6: 1.51}     # single bond from an sp2 carbon
_SP2_SP2_SINGLE = 1.48
_ANGLE = {"SP": 180.0, "SP2": 120.0, "SP3": 109.47}


def _heavy_degree(mol, i):
    return sum(1 for j, _ in mol.neighbors(i) if mol.atoms[j].z > 1)


def _has_double_to(mol, i, zs, skip=-1):
    return any(mol.bonds[k].type == 2 and mol.atoms[j].z in zs and j != skip for j, k in mol.neighbors(i))


def _bond_class(mol, k):
    """S / D / T / A, or C for a single bond shortened by conjugation: C-N of an amide (carbonyl carbon, sp2 nitrogen), C-O of an
    ester or acid, the second oxygen of a carboxylate, a terminal oxygen on phosphorus / sulfur / nitrogen next to an X=O."""
    b = mol.bonds[k]
    t = b.GetBondType()
    if t in ("DOUBLE", "TRIPLE", "AROMATIC"):
        return t[0]
    for x, y in ((b.a, b.b), (b.b, b.a)):
        ax, ay = mol.atoms[x], mol.atoms[y]
        if ax.z == 6 and ay.z == 7 and _has_double_to(mol, x, (8, 16)) and ay.hybridization == "SP2":
            return "C"
        if ax.z == 6 and ay.z == 8 and _has_double_to(mol, x, (8,), skip=y):
            return "C"
        if ax.z in (15, 16, 7) and ay.z == 8 and _heavy_degree(mol, y) == 1 and _has_double_to(mol, x, (8, 16), skip=y):
            return "C"
    return "S"


def ideal_bond_length(mol, k):
    """Ideal length (A) of bond k of a perceived molecule."""
    b = mol.bonds[k]
    za, zb = sorted((mol.atoms[b.a].z, mol.atoms[b.b].z))
    cls = _bond_class(mol, k)
    if cls == "C" and (za, zb) == (6, 8):
        o = b.a if mol.atoms[b.a].z == 8 else b.b
        return 1.25 if _heavy_degree(mol, o) == 1 else 1.34          # carboxylate / acid oxygen (delocalised in crystals) : ester
    if cls == "D" and (za, zb) == (6, 8):
        c = b.a if mol.atoms[b.a].z == 6 else b.b
        o = b.b if c == b.a else b.a
        if any(mol.atoms[j].z == 8 and j != o and _heavy_degree(mol, j) == 1 and mol.bonds[kk].type == 1 for j, kk in mol.neighbors(c)):
            return 1.25                                              # the other oxygen of a carboxylate
    if (za, zb, cls) in _BOND_LENGTH:
        d = _BOND_LENGTH[(za, zb, cls)]
        if cls == "S":
            for x, y in ((b.a, b.b), (b.b, b.a)):
                ax, ay = mol.atoms[x], mol.atoms[y]
                if ax.z == 6 and ax.hybridization in ("SP2", "SP") and ay.z in _AROMATIC_SUBSTITUENT:
                    if ay.z == 6:
                        d = _SP2_SP2_SINGLE if ay.hybridization in ("SP2", "SP") else _AROMATIC_SUBSTITUENT[6]
                    else:
                        d = _AROMATIC_SUBSTITUENT[ay.z]
                    break
        return d
    if za not in _COVALENT or zb not in _COVALENT:
        raise ValueError(f"no covalent radius for element {za if za not in _COVALENT else zb}")
    return _COVALENT[za] + _COVALENT[zb] - _ORDER_SHORTENING.get(mol.bonds[k].GetBondType(), 0.0)


def _ring_tables(mol):
    rings = [tuple(r) for r in mol.GetRingInfo().AtomRings()]
    planar = []
    for r in rings:
        planar.append(len(r) <= 6 and all(mol.atoms[a].aromatic or mol.atoms[a].hybridization in ("SP2", "SP") for a in r) or len(r) == 3)
    return rings, planar


def ideal_angle(mol, i, j, k, rings=None, planar=None):
    """Ideal angle i-j-k (degrees) at the centre j."""
    if rings is None:
        rings, planar = _ring_tables(mol)
    centre = mol.atoms[j]
    small = None                          # the smallest ring that holds all three
    in_ring_of_j = []
    for r, pl in zip(rings, planar):
        if j in r:
            in_ring_of_j.append((len(r), pl))
            if i in r and k in r and (small is None or len(r) < small[0]):
                small = (len(r), pl)
    if small is not None:
        n, pl = small
        if n == 3:
            return 60.0
        if n == 4:
            return 90.0
        if pl:
            return 180.0 - 360.0 / n       # regular polygon: 108 / 120
        if n == 5:
            return 104.5
    elif in_ring_of_j:
        n, pl = min(in_ring_of_j)
        if n == 3:
            return 118.0
        if n == 4:
            return 114.0
        if pl and centre.hybridization == "SP2" and len(mol.neighbors(j)) == 3:
            inside = 180.0 - 360.0 / n
            if sum(1 for r in rings if j in r) == 1:
                return (360.0 - inside) / 2.0      # 126 outside a planar 5-ring, 120 outside a 6-ring
    hyb = centre.hybridization
    if centre.z in (15, 16, 33, 34) and len(mol.neighbors(j)) == 4:
        # phosphonates, phosphates, sulfonyls: the terminal oxygens spread (O=P-O- 117..120), the bridging substituents close up
        terminal = sum(1 for q in (i, k) if mol.atoms[q].z in (8, 16) and _heavy_degree(mol, q) == 1)
        return (117.0, 109.5, 102.0)[2 - terminal]
    if hyb == "SP3":
        if centre.z == 16 or centre.z == 34:
            return 100.0 if len(mol.neighbors(j)) + centre.num_hs <= 2 else 109.47
        if centre.z == 8:
            return 112.0                           # ethers, alcohols seen through their heavy atoms
        if centre.z == 6 and mol.atoms[i].z > 1 and mol.atoms[k].z > 1 and len(mol.neighbors(j)) + centre.num_hs == 4 and \
                sum(1 for q, _ in mol.neighbors(j) if mol.atoms[q].z > 1) <= 3:
            return 111.5                           # heavy-heavy angles open up against the hydrogens (propane: 112.4)
        return 109.47
    return _ANGLE.get(hyb, 109.47)


def _angle_softness(mol, j):
    """How far the real angles at centre j stray from one ideal value, as a multiple of ANGLE_TOL: second-row centres (P, S) carry
    angles from 100 to 120 degrees on one atom."""
    z = mol.atoms[j].z
    if z in (15, 16, 33, 34, 14):
        return 5.0
    return 3.0


def _third_side(a, b, deg):
    return math.sqrt(a * a + b * b - 2.0 * a * b * math.cos(math.radians(deg)))


def _d14(d12, d23, d34, a123, a234, phi):
    """1-4 distance for bond lengths, the two angles (radians) and the torsion phi (0 = cis)."""
    x1, y1 = d12 * math.cos(a123), d12 * math.sin(a123)            # atom 2 at the origin, atom 3 at (d23, 0, 0)
    x4, r4 = d23 - d34 * math.cos(a234), d34 * math.sin(a234)
    y4, z4 = r4 * math.cos(phi), r4 * math.sin(phi)
    return math.sqrt((x4 - x1) ** 2 + (y4 - y1) ** 2 + z4 * z4)


def _torsion(p, i, j, k, l):
    b1, b2, b3 = p[j] - p[i], p[k] - p[j], p[l] - p[k]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    return math.atan2(float(np.dot(np.cross(n1, n2), b2)) / max(float(np.linalg.norm(b2)), 1e-12), float(np.dot(n1, n2)))


def smooth_bounds(lower, upper):
    """Triangle smoothing (Floyd-Warshall, one vectorised pass per pivot): upper_ij <= upper_ik + upper_kj, then
    lower_ij >= lower_ik - upper_kj.  Raises when a lower bound ends above its upper bound."""
    lo, up = np.array(lower, dtype=np.float64), np.array(upper, dtype=np.float64)
    n = len(lo)
    for k in range(n):
        np.minimum(up, up[:, k:k + 1] + up[k:k + 1, :], out=up)
    for k in range(n):
        np.maximum(lo, np.maximum(lo[:, k:k + 1] - up[k:k + 1, :], lo[k:k + 1, :] - up[:, k:k + 1]), out=lo)
    np.fill_diagonal(lo, 0.0)
    np.fill_diagonal(up, 0.0)
    if (lo > up + 1e-9).any():
        i, j = np.argwhere(lo > up + 1e-9)[0]
        raise ValueError(f"the distance bounds of atoms {i} and {j} contradict each other ({lo[i, j]:.3f} > {up[i, j]:.3f})")
    return np.minimum(lo, up), up


def plane_height(p, quad):
    """Distance of atom quad[0] from the plane through quad[1:4]."""
    a, b, c, d = (np.asarray(p[q], dtype=np.float64) for q in quad)
    n = np.cross(c - b, d - b)
    return abs(float(np.dot(a - b, n))) / max(float(np.linalg.norm(n)), 1e-12)


def centre_volume(p, quad):
    """Signed volume (n1 - c) . ((n2 - c) x (n3 - c)) of quad = (c, n1, n2, n3)."""
    c, n1, n2, n3 = (np.asarray(p[q], dtype=np.float64) for q in quad)
    return float(np.dot(n1 - c, np.cross(n2 - c, n3 - c)))


def distance_bounds(mol, ref_pos=None, stereo="pose"):
    """-> (lower [N, N], upper [N, N], constraints) of a perceived `molfile.Mol`, float64, triangle-smoothed.

    The atoms are used as given -- heavy atoms after `remove_hs`, or with the file's explicit hydrogens; hydrogens are NOT added the
    way the reference's `AddHs` does (see the module text).  `ref_pos` [N, 3]: a 3-D pose that stereo is read from (the sign of each
    sp3 centre's volume; the cis / trans side of double and amide bonds).  A flat or missing `ref_pos` gives no sign constraints.
    `stereo`: "pose" -- stereo from `ref_pos` as just described; "tags" -- from the molecule: the sign of a centre's volume from its
    `chiral_tag` (CHI_TETRAHEDRAL_CCW: the first three neighbours in bond order span a positive volume), the cis / trans side of a
    double bond's 1-4 pairs from `mol.double_bond_stereo`; `ref_pos` is then not looked at, and an untagged centre or an unrecorded
    double bond gets what "pose" gives without a pose.

    `constraints` = dict(idx int32 [nc, 4], lo / hi float64 [nc], kind int32 [nc]):
      KIND_VOLUME      V = (n1 - c) . ((n2 - c) x (n3 - c)) of (c, n1, n2, n3), the first three listed neighbours of the sp3 centre c,
                       must lie in [lo, hi] (one sign, |V| above VOLUME_FLOOR of its ideal value);
      KIND_ABS_VOLUME  |V| must lie in [lo, hi] (no pose to read the sign from);
      KIND_PLANAR      atom idx[0] lies within hi of the plane through the other three (sp2 centres with three neighbours: the centre
                       over its neighbours; aromatic rings: each atom over the next three of its ring).
    """
    if not mol.perceived:
        raise ValueError("distance_bounds needs a perceived molecule (molfile.perceive)")
    n = mol.GetNumAtoms()
    if n < 1 or n > MAX_ATOMS:
        raise ValueError(f"{n} atoms: the embedding takes 1..{MAX_ATOMS}")
    for a in mol.atoms:
        if a.z not in _COVALENT:
            raise ValueError(f"element {a.symbol} is outside the organic subset the bond-length table covers")
    if stereo not in ("pose", "tags"):
        raise ValueError(f"stereo={stereo!r}: \"pose\" or \"tags\"")
    tags = stereo == "tags"
    side = {}                                # (b, c) -> (a, d, cis?) for the recorded double bonds, both directions
    if tags:
        for a_, b_, c_, d_, rel in getattr(mol, "double_bond_stereo", ()):
            side[(b_, c_)], side[(c_, b_)] = (a_, d_, rel == "cis"), (d_, a_, rel == "cis")
    tag_sign = lambda c: {"CHI_TETRAHEDRAL_CCW": 1, "CHI_TETRAHEDRAL_CW": -1}.get(mol.atoms[c].chiral_tag, 0) if tags else 0
    ref = None
    if ref_pos is not None and not tags:
        ref = np.asarray(ref_pos, dtype=np.float64)
        if ref.shape != (n, 3):
            raise ValueError(f"ref_pos {ref.shape} is not [{n}, 3]")
        if not np.isfinite(ref).all() or np.linalg.svd(ref - ref.mean(0), compute_uv=False)[-1] < 1e-3 * max(n, 1) ** 0.5:
            ref = None                       # flat (a 2-D depiction) or degenerate: nothing to read a hand from
    rings, planar = _ring_tables(mol)
    nbr = [[j for j, _ in mol.neighbors(i)] for i in range(n)]
    lower = np.zeros((n, n))
    upper = np.full((n, n), UPPER_FAR)
    fixed = np.zeros((n, n), dtype=np.int8)      # topological class that owns the pair: 1 = bond, 2 = angle, 3 = torsion

    def put(i, j, lo, up, cls):
        if fixed[i, j] and fixed[i, j] < cls:
            return
        if fixed[i, j] == cls:                  # the same pair through two paths (rings): keep what both allow, else the tighter path
            lo2, up2 = max(lo, lower[i, j]), min(up, upper[i, j])
            if lo2 <= up2:
                lo, up = lo2, up2
            elif up - lo > upper[i, j] - lower[i, j]:
                return
        lower[i, j] = lower[j, i] = lo
        upper[i, j] = upper[j, i] = up
        fixed[i, j] = fixed[j, i] = cls

    # 1-2
    blen = {}
    for k, b in enumerate(mol.bonds):
        if b.a == b.b:
            continue
        d = ideal_bond_length(mol, k)
        blen[(b.a, b.b)] = blen[(b.b, b.a)] = d
        put(b.a, b.b, d - BOND_TOL, d + BOND_TOL, 1)
    # 1-3
    d13 = {}
    for j in range(n):
        soft = _angle_softness(mol, j) * ANGLE_TOL
        for x in range(len(nbr[j])):
            for y in range(x + 1, len(nbr[j])):
                i, k = nbr[j][x], nbr[j][y]
                if i == k:
                    continue
                d = _third_side(blen[(i, j)], blen[(j, k)], ideal_angle(mol, i, j, k, rings, planar))
                d13[(i, j, k)] = d13[(k, j, i)] = d
                put(i, k, d - soft, d + soft, 2)
    # 1-4
    angle_of = lambda p, q, opposite: math.acos(max(-1.0, min(1.0, (p * p + q * q - opposite * opposite) / (2 * p * q))))
    ring_sets = [set(r) for r in rings]
    for kb, b in enumerate(mol.bonds):
        j, k = b.a, b.b
        if j == k:
            continue
        cls = _bond_class(mol, kb)
        shared = [q for q, r in enumerate(ring_sets) if j in r and k in r]
        flat_bond = cls in ("D", "A") or (cls == "C" and {mol.atoms[j].z, mol.atoms[k].z} == {6, 7})
        for i in nbr[j]:
            if i == k:
                continue
            for l in nbr[k]:
                if l == j or l == i:
                    continue
                a1 = angle_of(blen[(i, j)], blen[(j, k)], d13[(i, j, k)])
                a2 = angle_of(blen[(j, k)], blen[(k, l)], d13[(j, k, l)])
                dist = lambda phi: _d14(blen[(i, j)], blen[(j, k)], blen[(k, l)], a1, a2, phi)
                cis, trans = dist(0.0), dist(math.pi)
                soft = 0.5 * ANGLE_TOL * (_angle_softness(mol, j) + _angle_softness(mol, k))
                # a free torsion: from the cis extreme at the smallest angles the 1-3 bounds admit to the trans extreme at the largest,
                # so that no geometry inside the 1-2 / 1-3 bounds falls outside the 1-4 bounds at any torsion
                sj, sk = _angle_softness(mol, j) * ANGLE_TOL, _angle_softness(mol, k) * ANGLE_TOL
                wide = [[angle_of(blen[(i, j)], blen[(j, k)], d13[(i, j, k)] + sg * sj), angle_of(blen[(j, k)], blen[(k, l)], d13[(j, k, l)] + sg * sk)]
                        for sg in (-1.0, 1.0)]
                lo = _d14(blen[(i, j)], blen[(j, k)], blen[(k, l)], wide[0][0], wide[0][1], 0.0) - GEN_TOL
                up = _d14(blen[(i, j)], blen[(j, k)], blen[(k, l)], wide[1][0], wide[1][1], math.pi) + GEN_TOL
                same = [q for q in shared if i in ring_sets[q] and l in ring_sets[q]]
                small = [q for q in shared if len(rings[q]) <= 8]
                if same and min(len(rings[q]) for q in same) <= 8:
                    q = min(same, key=lambda q: len(rings[q]))
                    if planar[q]:
                        lo, up = cis - GEN_TOL, cis + GEN_TOL
                    else:                          # a puckered ring: on the cis side, torsion up to 70 (6-ring) / 100 degrees
                        lo, up = cis - GEN_TOL - soft, dist(math.radians(70.0 if len(rings[q]) <= 6 else 100.0)) + GEN_TOL + soft
                elif small and any(planar[q] for q in small):
                    # a bond of a planar ring: a ring atom and a substituent are trans, two substituents cis
                    q = [q for q in small if planar[q]][0]
                    inside = (i in ring_sets[q]) + (l in ring_sets[q])
                    v = trans if inside == 1 else cis
                    lo, up = v - GEN_TOL - soft, v + GEN_TOL + soft
                elif flat_bond and not shared and ref is not None:
                    v = cis if abs(_torsion(ref, i, j, k, l)) < 0.5 * math.pi else trans
                    lo, up = v - GEN_TOL - soft, v + GEN_TOL + soft
                elif cls == "D" and not shared and (j, k) in side:
                    a_, d_, same_side = side[(j, k)]              # the other substituent of an end lies on the other side
                    v = cis if same_side == ((i == a_) == (l == d_)) else trans
                    lo, up = v - GEN_TOL - soft, v + GEN_TOL + soft
                put(i, l, lo, up, 3)
    # everything further apart: van-der-Waals lower bounds by topological distance
    topo = np.full((n, n), 99, dtype=np.int64)
    np.fill_diagonal(topo, 0)
    for i in range(n):
        for j in nbr[i]:
            topo[i, j] = 1
    for k in range(n):
        np.minimum(topo, topo[:, k:k + 1] + topo[k:k + 1, :], out=topo)
    vdw = np.array([_VDW[a.z] for a in mol.atoms])
    for i in range(n):
        for j in range(i + 1, n):
            if fixed[i, j]:
                continue
            scale = 0.7 if topo[i, j] == 4 else 0.85 if topo[i, j] == 5 else 0.9
            lower[i, j] = lower[j, i] = scale * (vdw[i] + vdw[j])
    np.fill_diagonal(upper, 0.0)
    lower, upper = smooth_bounds(lower, upper)

    # ---- constraints
    idx, lo_c, hi_c, kind = [], [], [], []

    def add_volume(q, floor, ceil, sign):
        idx.append(q)
        if sign > 0:
            lo_c.append(floor); hi_c.append(ceil); kind.append(KIND_VOLUME)
        elif sign < 0:
            lo_c.append(-ceil); hi_c.append(-floor); kind.append(KIND_VOLUME)
        else:
            lo_c.append(floor); hi_c.append(ceil); kind.append(KIND_ABS_VOLUME)

    for c in range(n):
        a = mol.atoms[c]
        if a.hybridization == "SP3" and len(nbr[c]) >= 3 and a.z > 1:
            q = (c, nbr[c][0], nbr[c][1], nbr[c][2])
            r = [blen[(c, x)] for x in q[1:]]
            cosines = [(r[x] ** 2 + r[y] ** 2 - d13[(q[1 + x], c, q[1 + y])] ** 2) / (2 * r[x] * r[y]) for x, y in ((0, 1), (0, 2), (1, 2))]
            gram = np.array([[r[0] ** 2, r[0] * r[1] * cosines[0], r[0] * r[2] * cosines[1]],
                             [r[0] * r[1] * cosines[0], r[1] ** 2, r[1] * r[2] * cosines[2]],
                             [r[0] * r[2] * cosines[1], r[1] * r[2] * cosines[2], r[2] ** 2]])
            ideal = math.sqrt(max(float(np.linalg.det(gram)), 0.0))
            sign = tag_sign(c)
            if ref is not None:
                v = centre_volume(ref, q)
                if abs(v) > 0.25 * ideal:
                    sign = 1 if v > 0 else -1
            add_volume(q, VOLUME_FLOOR * ideal, 2.0 * ideal + 1.0, sign)
            if len(nbr[c]) >= 4:
                # the fourth neighbour on the wrong side of the other three (an inverted umbrella) halves the volume of the
                # neighbours' own tetrahedron: (n4, n1, n2, n3) with the same formula, ideal value by Cayley-Menger from the 1-3 distances
                t = (nbr[c][3], nbr[c][0], nbr[c][1], nbr[c][2])
                cm = np.ones((5, 5))
                cm[0, 0] = 0.0
                for x in range(4):
                    for y in range(4):
                        cm[1 + x, 1 + y] = 0.0 if x == y else d13[(t[x], c, t[y])] ** 2
                ideal4 = math.sqrt(max(float(np.linalg.det(cm)) / 288.0, 0.0)) * 6.0
                sign4 = tag_sign(c)      # the centre lies inside its neighbours' tetrahedron: both volumes have one sign
                if ref is not None:
                    v = centre_volume(ref, t)
                    if abs(v) > 0.25 * ideal4:
                        sign4 = 1 if v > 0 else -1
                add_volume(t, UMBRELLA_FLOOR * ideal4, 2.0 * ideal4 + 1.0, sign4)
        elif a.hybridization == "SP2" and len(nbr[c]) == 3:
            idx.append((c, nbr[c][0], nbr[c][1], nbr[c][2]))
            lo_c.append(0.0); hi_c.append(PLANAR_LIMIT); kind.append(KIND_PLANAR)
    for r in rings:
        if len(r) >= 4 and all(mol.atoms[a].aromatic for a in r):
            for q in range(len(r)):
                idx.append(tuple(r[(q + s) % len(r)] for s in range(4)))
                lo_c.append(0.0); hi_c.append(PLANAR_LIMIT); kind.append(KIND_PLANAR)
    if len(idx) > MAX_CONSTRAINTS:
        raise ValueError(f"{len(idx)} constraints: the embedding takes at most {MAX_CONSTRAINTS}")
    cons = {"idx": np.asarray(idx, dtype=np.int32).reshape(-1, 4), "lo": np.asarray(lo_c, dtype=np.float64),
            "hi": np.asarray(hi_c, dtype=np.float64), "kind": np.asarray(kind, dtype=np.int32)}
    return lower, upper, cons


# ---- device -------------------------------------------------------------------------------------------------------------------------
DEFAULT_ITERS = (1000, 500, 1000)      # FIRE iteration caps: 4-D weak, 4-D strong, 3-D (each stage leaves early once converged)


def _device(device):
    from .conformer_matching import _device as match_device
    return match_device(device)          # the same error as the matching path when there is no GPU


def _bounds_of(item):
    """(lower, upper, constraints) from a (mol, ref_pos) pair, a Mol, or bounds computed before."""
    if isinstance(item, tuple) and len(item) == 3 and isinstance(item[2], dict):
        lower, upper, cons = item
    elif isinstance(item, tuple):
        lower, upper, cons = distance_bounds(item[0], item[1])
    else:
        lower, upper, cons = distance_bounds(item, None)
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    n = len(lower)
    if lower.shape != (n, n) or upper.shape != (n, n) or not 1 <= n <= MAX_ATOMS:
        raise ValueError(f"bounds {lower.shape} / {upper.shape}: expected two [N, N] matrices, N in 1..{MAX_ATOMS}")
    idx = np.asarray(cons["idx"], dtype=np.int64).reshape(-1, 4)
    kind = np.asarray(cons["kind"], dtype=np.int64).reshape(-1)
    if len(idx) > MAX_CONSTRAINTS:
        raise ValueError(f"{len(idx)} constraints: the embedding takes at most {MAX_CONSTRAINTS}")
    if len(idx) and (idx.min() < 0 or idx.max() >= n or any(len(set(q)) != 4 for q in idx.tolist()) or kind.min() < 0 or kind.max() > 2):
        raise ValueError("constraint with an atom index outside the molecule, a repeated atom or an unknown kind")
    if not (len(idx) == len(kind) == len(cons["lo"]) == len(cons["hi"])):
        raise ValueError("constraint arrays of different lengths")
    return lower, upper, {"idx": idx, "lo": np.asarray(cons["lo"], dtype=np.float64), "hi": np.asarray(cons["hi"], dtype=np.float64), "kind": kind}


def embed_conformers_batch(items, n, seed=0, device=None, conf_ids=None, mol_ids=None, iters=DEFAULT_ITERS):
    """Conformers of several molecules in one upload, one launch and one download.

    items: one entry per molecule -- (mol, ref_pos), a perceived `Mol` (no pose), or the (lower, upper, constraints) of
    `distance_bounds`.  n: conformers per molecule (an int, or one int per molecule).  conf_ids: per molecule the ids of its
    conformers (default 0 .. n-1); mol_ids: one id per molecule (default: its position).  Both enter the random-number key, so a
    conformer launched alone under its ids is bitwise what it is inside any batch.
    -> list of (pos [n, N, 3] float64, ok [n] bool, error [n] float64), one per molecule."""
    import torch
    from .. import engine
    bounds = [_bounds_of(it) for it in items]
    counts = [int(n)] * len(bounds) if np.isscalar(n) else [int(k) for k in n]
    if len(counts) != len(bounds) or any(k < 0 for k in counts):
        raise ValueError("one non-negative conformer count per molecule")
    ids = [np.arange(k) for k in counts] if conf_ids is None else [np.asarray(c, dtype=np.int64).reshape(-1) for c in conf_ids]
    if [len(c) for c in ids] != counts:
        raise ValueError("conf_ids must name every conformer")
    mids = np.arange(len(bounds)) if mol_ids is None else np.asarray(mol_ids, dtype=np.int64).reshape(len(bounds))
    iters = tuple(int(k) for k in iters)
    if len(iters) != 3 or min(iters) < 0:
        raise ValueError("iters = (4-D weak, 4-D strong, 3-D) iteration caps")
    dev = _device(device)
    total = sum(counts)
    sizes = np.array([len(b[0]) for b in bounds], dtype=np.int64)
    if total == 0:
        return [(np.zeros((0, s, 3)), np.zeros(0, bool), np.zeros(0)) for s in sizes]
    ncs = np.array([len(b[2]["idx"]) for b in bounds], dtype=np.int64)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    conf_mol = np.repeat(np.arange(len(bounds)), counts)
    host = [i32(sizes), i32(np.concatenate([[0], np.cumsum(sizes * sizes)])),
            f32(np.concatenate([b[0].ravel() for b in bounds])), f32(np.concatenate([b[1].ravel() for b in bounds])),
            i32(np.concatenate([[0], np.cumsum(ncs)])), i32(np.concatenate([b[2]["idx"] for b in bounds]).reshape(-1, 4)),
            f32(np.concatenate([b[2]["lo"] for b in bounds])), f32(np.concatenate([b[2]["hi"] for b in bounds])),
            i32(np.concatenate([b[2]["kind"] for b in bounds])), i32(mids), i32(conf_mol), i32(np.concatenate(ids)),
            i32(np.concatenate([[0], np.cumsum(sizes[conf_mol])]))]
    # one upload: every array in one byte buffer, 16-byte aligned
    offs, nbytes = [], 0
    for a in host:
        offs.append(nbytes)
        nbytes += (a.nbytes + 15) // 16 * 16
    n_out = int(sizes[conf_mol].sum())
    out_off = nbytes
    nbytes += (n_out * 3 + 2 * total) * 4
    blob = np.zeros(nbytes, dtype=np.uint8)
    for a, o in zip(host, offs):
        blob[o:o + a.nbytes] = a.view(np.uint8).ravel()
    buf = torch.from_numpy(blob).to(dev)
    base = buf.data_ptr()
    ptr = [C.c_void_p(base + o) if a.size else None for a, o in zip(host, offs)]
    p_pos, p_err, p_ok = base + out_off, base + out_off + n_out * 12, base + out_off + n_out * 12 + total * 4
    with torch.cuda.device(dev):
        rc = engine.load_library().cbd_embed_conformers(
            len(bounds), total, int(sizes.max()), int(ncs.max()), *ptr, int(seed) & (2 ** 64 - 1), iters[0], iters[1], iters[2],
            float(BOUND_TOL), C.c_void_p(p_pos), C.c_void_p(p_err), C.c_void_p(p_ok), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        msg = engine.load_library().cbd_last_error().decode()
        raise (ValueError if rc in (-1, -4) else RuntimeError)(f"cbdock error {rc}: {msg}")
    back = buf[out_off:].cpu().numpy()            # one download (synchronises)
    pos = back[:n_out * 12].view(np.float32).reshape(-1, 3).astype(np.float64)
    err = back[n_out * 12:n_out * 12 + total * 4].view(np.float32).astype(np.float64)
    ok = back[n_out * 12 + total * 4:].view(np.int32)
    if (ok < 0).any():
        raise RuntimeError("the kernel refused a molecule description")
    out, a0, c0 = [], 0, 0
    for s, k in zip(sizes, counts):
        out.append((pos[a0:a0 + k * s].reshape(k, s, 3).copy(), ok[c0:c0 + k] == 1, err[c0:c0 + k].copy()))
        a0, c0 = a0 + k * s, c0 + k
    return out


def embed_conformers(mol, n, seed=0, ref_pos=None, device=None, conf_ids=None, mol_id=0, iters=DEFAULT_ITERS, stereo="pose"):
    """n conformers of one perceived molecule -> (pos [n, N, 3] float64, ok [n] bool, error [n] float64).  `ok`: the conformer
    passes the acceptance test (every pair distance within BOUND_TOL of its bounds, every sp3 centre with the hand of `ref_pos` and
    not flattened, every sp2 centre and aromatic ring atom planar within PLANAR_LIMIT); `error`: the final value of the objective.
    The same (seed, mol_id, conformer id) gives bitwise the same coordinates in any launch.  `stereo`: see `distance_bounds`."""
    return embed_conformers_batch([distance_bounds(mol, ref_pos, stereo=stereo)], n, seed=seed, device=device, conf_ids=None if conf_ids is None else [conf_ids],
                                  mol_ids=[mol_id], iters=iters)[0]


def embed_until_ok(mol, n, seed=0, ref_pos=None, device=None, rounds=3, stereo="pose"):
    """n conformers, each not-ok one replaced from further conformer ids (at most `rounds` more launches); what is still not ok after
    that stays as the least-violating candidate seen.  -> (pos [n, N, 3], ok [n], error [n])."""
    bounds = distance_bounds(mol, ref_pos, stereo=stereo)
    pos, ok, err = embed_conformers_batch([bounds], n, seed=seed, device=device)[0]
    nxt = n
    for _ in range(rounds):
        bad = np.nonzero(~ok)[0]
        if len(bad) == 0:
            break
        p2, ok2, e2 = embed_conformers_batch([bounds], len(bad), seed=seed, device=device, conf_ids=[np.arange(nxt, nxt + len(bad))])[0]
        nxt += len(bad)
        for k, b in enumerate(bad):
            if ok2[k] or e2[k] < err[b]:
                pos[b], ok[b], err[b] = p2[k], ok2[k], e2[k]
    return pos, ok, err
