"""Torsion matching of ligand conformers (reference datasets/conformer_matching.py:30-84, used at datasets/process_mols.py:621-650).

The reference embeds a fresh conformer with rdkit's ETKDG and then turns its rotatable bonds until it lies as close to the holo
ligand as a rigid alignment allows: `scipy.optimize.differential_evolution` over the R dihedral angles, a Python loop of
`SetDihedralRad` + `AlignMol` per evaluation.  The embedding needs rdkit and is not part of this package; the matching is pure
geometry and runs on the GPU here (csrc/torsion_match.hip, C ABI `cbd_match_score` / `cbd_match_torsions`): conformers from any
source -- a multi-record SDF written elsewhere, a second file -- can be matched.

Host side (numpy, float64): `get_torsion_angles`, `get_dihedral`, `apply_changes`, `score_conformation` (the CPU statement of the
objective: truth for the tests, objective of the polish step), `rigid_align`.
Device side: `match_score`, `match_torsions` (batches of problems, possibly of different molecules, one launch), and the
reference-shaped `optimize_rotatable_bonds`.

Objective f(theta) = min over rigid motions of RMSD(probe with its R dihedrals SET to theta, target).  Every torsion bond is a
bridge, so the four atoms of a quadruple either move rigidly together or lie on the axis of any other rotation: the dihedrals are
independent and can be set one after the other.  Sign convention: IUPAC / rdkit (cis 0, trans pi, looking down u -> v a clockwise
turn of l relative to k is positive).

Differences from the reference's optimiser, both deliberate: (1) a mutant angle outside [-pi, pi) is wrapped periodically instead of
re-drawn (the variable is an angle); the population is updated generation-synchronously (scipy's updating='deferred', the only
parallel form).  (2) `optimize_rotatable_bonds` lets the conformer's own dihedrals compete with the optimiser's result, so matching
never returns a conformer further from the target than the one it was given.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ..torsion import _components

MAX_TORSIONS = 32          # csrc/torsion_match.hip: TM_MAX_R
MAX_ATOMS = 256            # TM_MAX_NL
MAX_POPULATION = 512       # TM_MAX_POP: popsize * R


# ---- topology -----------------------------------------------------------------------------------------------------------------------
def get_torsion_angles(mol):
    """Quadruples (n0, e0, e1, n1) of the torsion bonds of `mol` (an rdkit-shaped `molfile.Mol`): the bonds whose removal splits the
    graph with at least 2 atoms in the smallest part, each with the first other neighbour of either end.  Order and choice of
    neighbours follow the reference's walk over a networkx graph: bonds grouped by their lower-numbered atom, neighbours in the order
    the bonds list them.  The bonds are exactly the edges `torsion.get_transformation_mask` flags -- also for a ligand of several
    fragments, where the reference looks at the smallest part of the WHOLE graph."""
    n = mol.GetNumAtoms()
    adj = [[] for _ in range(n)]
    for bond in mol.GetBonds():
        a, b = bond.GetBeginAtomIdx(), bond.GetEndAtomIdx()
        if b not in adj[a]:
            adj[a].append(b)
        if a not in adj[b]:
            adj[b].append(a)
    out, done = [], set()
    for a in range(n):
        for b in adj[a]:
            if b in done or b == a:
                continue
            comp, nc = _components(n, adj, (a, b))
            if nc < 2:
                continue
            if np.bincount(comp, minlength=nc).min() < 2:
                continue
            n0 = [x for x in adj[a] if x != b]
            n1 = [x for x in adj[b] if x != a]
            if not n0 or not n1:
                raise ValueError(f"bond {a}-{b} is flagged through another fragment of the molecule and has no dihedral")
            out.append((n0[0], a, b, n1[0]))
        done.add(a)
    return out


# ---- geometry (float64) -------------------------------------------------------------------------------------------------------------
def get_dihedral(pos, quad):
    """Dihedral angle (radians, IUPAC sign) of the atoms quad = (k, u, v, l) of pos [N, 3]."""
    p = np.asarray(pos, dtype=np.float64)
    k, u, v, l = (int(q) for q in quad)
    b1, b2, b3 = p[u] - p[k], p[v] - p[u], p[l] - p[v]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    y = np.dot(np.cross(n1, n2), b2) / np.linalg.norm(b2)
    return float(np.arctan2(y, np.dot(n1, n2)))


def _rows_of(rotable_bonds, mask_rotate):
    """mask_rotate rows in the order of rotable_bonds: the row of bond u-v is the one that holds exactly one of u, v (a side of another
    bridge holds both or neither)."""
    m = np.asarray(mask_rotate).astype(bool)
    quads = np.asarray(rotable_bonds, dtype=np.int64).reshape(-1, 4)
    if m.ndim != 2 or m.shape[0] != len(quads):
        raise ValueError(f"mask_rotate {m.shape} does not have one row per rotatable bond ({len(quads)})")
    if len(quads) and (quads.min() < 0 or quads.max() >= m.shape[1]):
        raise ValueError("rotatable bond with an atom index outside the molecule")
    rows = np.empty_like(m)
    for r, (k, u, v, l) in enumerate(quads):
        hit = np.nonzero(m[:, u] != m[:, v])[0]
        if len(hit) != 1 or m[hit[0], k] == m[hit[0], l]:
            raise ValueError(f"no row of mask_rotate belongs to the bond {u}-{v}")
        rows[r] = m[hit[0]]
    return quads, rows


def _rotation(axis, angle):
    """matrix of the right-handed turn by `angle` about `axis` (Rodrigues)."""
    x, y, z = (float(a) for a in axis)
    n = math.sqrt(x * x + y * y + z * z)
    x, y, z = x / n, y / n, z / n
    c, s = math.cos(angle), math.sin(angle)
    t = 1.0 - c
    return np.array([[c + x * x * t, x * y * t - z * s, x * z * t + y * s],
                     [y * x * t + z * s, c + y * y * t, y * z * t - x * s],
                     [z * x * t - y * s, z * y * t + x * s, c + z * z * t]])


def _set_dihedrals(pos, values, quads, rows, phi=None):
    """`phi`: the dihedrals of `pos` (computed when not given).  The bonds are bridges, so turning bond r leaves every other dihedral
    as it was: each is turned by the difference to its value in `pos`, one after the other."""
    p = np.array(pos, dtype=np.float64)
    if phi is None:
        phi = [get_dihedral(p, q) for q in quads]
    for r, (k, u, v, l) in enumerate(quads):
        delta = float(values[r]) - phi[r]
        side = rows[r]
        # turning the l side about u -> v raises the dihedral, turning the k side lowers it
        origin = p[v].copy()
        p[side] = (p[side] - origin) @ _rotation(p[v] - p[u], delta if side[l] else -delta).T + origin
    return p


def apply_changes(pos, values, rotable_bonds, mask_rotate):
    """pos [N, 3] with the dihedral of every rotable_bonds[r] = (k, u, v, l) set to values[r] by turning the mask_rotate side of the
    bond.  The reference's `apply_changes` on coordinates instead of an rdkit conformer."""
    quads, rows = _rows_of(rotable_bonds, mask_rotate)
    return _set_dihedrals(pos, values, quads, rows)


def rigid_align(pos, ref):
    """(pos moved rigidly onto ref in the least-squares sense, the RMSD left) -- Kabsch, proper rotations only."""
    a, b = np.asarray(pos, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ca, cb = a.mean(0), b.mean(0)
    a0, b0 = a - ca, b - cb
    U, _, Vt = np.linalg.svd(a0.T @ b0)
    d = np.sign(np.linalg.det(U @ Vt))
    rot = U @ np.diag([1.0, 1.0, d]) @ Vt
    out = a0 @ rot + cb
    return out, float(np.sqrt(((out - b) ** 2).sum() / len(a)))


def score_conformation(pos, true_pos, values, rotable_bonds, mask_rotate):
    """The objective in float64: RMSD to true_pos, after optimal rigid alignment, of pos with its dihedrals set to `values`."""
    return rigid_align(apply_changes(pos, values, rotable_bonds, mask_rotate), true_pos)[1]


# ---- device -------------------------------------------------------------------------------------------------------------------------
def _device(device):
    import torch
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("torsion matching runs on the MI355X (cbd_match_torsions); there is no CPU path in the package")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("torsion matching runs on the MI355X (cbd_match_torsions); there is no CPU path in the package")
    return device


class _Packed:
    """A list of problems (pos, true_pos, rotable_bonds, mask_rotate) as the padded device arrays of include/cbdock.h."""

    def __init__(self, problems, device, popsize=None):
        import torch
        prepared = []
        for pos, true_pos, bonds, mask in problems:
            p, t = np.asarray(pos, dtype=np.float32), np.asarray(true_pos, dtype=np.float32)
            if p.ndim != 2 or p.shape[1] != 3 or p.shape != t.shape:
                raise ValueError(f"probe {p.shape} and target {t.shape} must both be [N, 3]")
            quads, rows = _rows_of(bonds, mask)
            if rows.shape[1] != len(p):
                raise ValueError(f"mask_rotate has {rows.shape[1]} columns for {len(p)} atoms")
            if not 1 <= len(quads) <= MAX_TORSIONS:
                raise ValueError(f"{len(quads)} rotatable bonds: the kernel takes 1..{MAX_TORSIONS}")
            if not 1 <= len(p) <= MAX_ATOMS:
                raise ValueError(f"{len(p)} atoms: the kernel takes 1..{MAX_ATOMS}")
            prepared.append((p, t, quads, rows))
        self.n = len(prepared)
        self.nl = [len(p) for p, _, _, _ in prepared]
        self.r = [len(q) for _, _, q, _ in prepared]
        self.max_nl, self.max_r = max(self.nl, default=1), max(self.r, default=1)
        if popsize is not None and (popsize < 1 or popsize * self.max_r > MAX_POPULATION):
            raise ValueError(f"popsize * R = {popsize * self.max_r}: the kernel takes 1..{MAX_POPULATION}")
        probe = np.zeros((self.n, self.max_nl, 3), np.float32)
        target = np.zeros_like(probe)
        quads = np.zeros((self.n, self.max_r, 4), np.int32)
        mask = np.zeros((self.n, self.max_r, self.max_nl), np.uint8)
        for i, (p, t, q, m) in enumerate(prepared):
            probe[i, :len(p)], target[i, :len(p)] = p, t
            quads[i, :len(q)] = q
            mask[i, :len(q), :len(p)] = m
        self.device = _device(device)
        up = lambda a: torch.from_numpy(a).to(self.device)
        self.probe, self.target, self.quads, self.mask = up(probe), up(target), up(quads), up(mask)
        self.nl_dev, self.r_dev = up(np.asarray(self.nl, np.int32)), up(np.asarray(self.r, np.int32))


def _call(fn, device, *args):
    import torch
    from .. import engine
    with torch.cuda.device(device):
        rc = fn(*args, C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    if rc != 0:
        msg = engine.load_library().cbd_last_error().decode()
        raise (ValueError if rc == -1 else RuntimeError)(f"cbdock error {rc}: {msg}")


def match_score(problems, thetas, device=None):
    """f(theta) on the GPU.  problems: list of (pos [N, 3], true_pos [N, 3], rotable_bonds, mask_rotate); thetas: one [n_theta, R]
    array per problem (the same n_theta for all).  -> float32 [n_problems, n_theta]."""
    import torch
    from .. import engine
    pk = _Packed(problems, device)
    n_theta = len(thetas[0]) if pk.n else 0
    th = np.zeros((pk.n, n_theta, pk.max_r), np.float32)
    for i, t in enumerate(thetas):
        t = np.asarray(t, dtype=np.float32).reshape(-1, pk.r[i])
        if len(t) != n_theta:
            raise ValueError("every problem needs the same number of theta vectors")
        th[i, :, :pk.r[i]] = t
    th_dev = torch.from_numpy(th).to(pk.device)
    out = torch.empty(pk.n, n_theta, dtype=torch.float32, device=pk.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    _call(engine.load_library().cbd_match_score, pk.device, pk.n, pk.max_nl, pk.max_r, n_theta, ptr(pk.nl_dev), ptr(pk.r_dev), ptr(pk.probe),
          ptr(pk.target), ptr(pk.quads), ptr(pk.mask), ptr(th_dev), ptr(out))
    return out.cpu().numpy()


def match_torsions(problems, seed=0, popsize=15, maxiter=500, mutation=(0.5, 1), recombination=0.8, tol=0.01, problem_ids=None, device=None):
    """Differential evolution over the dihedrals of every problem, all in one launch (one workgroup each).
    -> list of (theta float32 [R], fitness, generations run).  `problem_ids` (default: the position in the list) enter the
    random-number key, so a problem launched alone under its id gives bitwise what it gives inside a batch."""
    import torch
    from .. import engine
    popsize, maxiter = int(popsize), int(maxiter)
    pk = _Packed(problems, device, popsize=popsize)
    if maxiter < 0:
        raise ValueError("maxiter < 0")
    mut = (float(mutation), float(mutation)) if np.isscalar(mutation) else (float(mutation[0]), float(mutation[1]))
    ids = np.arange(pk.n, dtype=np.int32) if problem_ids is None else np.asarray(problem_ids, dtype=np.int32).reshape(pk.n)
    ids_dev = torch.from_numpy(ids).to(pk.device)
    theta = torch.empty(pk.n, pk.max_r, dtype=torch.float32, device=pk.device)
    fit = torch.empty(pk.n, dtype=torch.float32, device=pk.device)
    gens = torch.empty(pk.n, dtype=torch.int32, device=pk.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    _call(engine.load_library().cbd_match_torsions, pk.device, pk.n, pk.max_nl, pk.max_r, ptr(pk.nl_dev), ptr(pk.r_dev), ptr(pk.probe),
          ptr(pk.target), ptr(pk.quads), ptr(pk.mask), ptr(ids_dev), int(seed) & (2 ** 64 - 1), popsize, maxiter, mut[0], mut[1],
          float(recombination), float(tol), ptr(theta), ptr(fit), ptr(gens))
    theta, fit, gens = theta.cpu().numpy(), fit.cpu().numpy(), gens.cpu().numpy()
    if (gens < 0).any():
        raise RuntimeError("the kernel refused a problem description")
    return [(theta[i, :pk.r[i]].copy(), float(fit[i]), int(gens[i])) for i in range(pk.n)]


def optimize_rotatable_bonds(pos, true_pos, rotable_bonds, mask_rotate, seed=0, popsize=15, maxiter=500, mutation=(0.5, 1),
                             recombination=0.8, polish=True, device=None):
    """The reference's `optimize_rotatable_bonds` on coordinates: turn the rotatable bonds of `pos` so that it lies as close to
    `true_pos` as a rigid alignment allows.  -> (opt_pos, values, rmsd): the coordinates with the optimal dihedrals set (not aligned),
    the dihedrals, the aligned RMSD (float64).  `pos` may be [T, N, 3] -- T tries, matched in one launch -- and every result gets a
    leading axis T.  `polish`: one L-BFGS-B run on `score_conformation` per try from the GPU's best theta, what scipy's own `polish`
    does.  The conformer's own dihedrals compete with the result (see the module text)."""
    pos = np.asarray(pos, dtype=np.float64)
    single = pos.ndim == 2
    tries = pos[None] if single else pos
    true_pos = np.asarray(true_pos, dtype=np.float64)
    if tries.ndim != 3 or tries.shape[2] != 3 or true_pos.shape[-2:] != tries.shape[1:] or true_pos.ndim not in (2, 3):
        raise ValueError(f"pos {pos.shape} / true_pos {true_pos.shape}: expected [N, 3] or [T, N, 3]")
    targets = np.broadcast_to(true_pos, tries.shape)
    quads, rows = _rows_of(rotable_bonds, mask_rotate)
    T, R = len(tries), len(quads)
    if R == 0:          # nothing to turn: no launch
        values, rmsds, out = np.zeros((T, 0)), np.array([rigid_align(p, t)[1] for p, t in zip(tries, targets)]), tries.copy()
    else:
        found = match_torsions([(p, t, quads, rows) for p, t in zip(tries, targets)], seed=seed, popsize=popsize, maxiter=maxiter,
                               mutation=mutation, recombination=recombination, device=device)
        values, rmsds, out = np.empty((T, R)), np.empty(T), np.empty_like(tries)
        for i, (theta, _, _) in enumerate(found):
            own = np.array([get_dihedral(tries[i], q) for q in quads])
            f = lambda x: rigid_align(_set_dihedrals(tries[i], x, quads, rows, own), targets[i])[1]
            x = theta.astype(np.float64)
            fx = f(x)
            if polish:
                from scipy.optimize import minimize
                # tolerances below scipy's defaults: the objective is smooth away from 0 and an evaluation is cheap next to the search
                res = minimize(f, x, method="L-BFGS-B", bounds=[(-np.pi, np.pi)] * R, options={"ftol": 1e-14, "gtol": 1e-9})
                if res.fun < fx:
                    x, fx = np.asarray(res.x, dtype=np.float64), float(res.fun)
            f_own = f(own)
            if f_own < fx:
                x, fx = own, f_own
            values[i], rmsds[i], out[i] = x, fx, _set_dihedrals(tries[i], x, quads, rows)
    return (out[0], values[0], float(rmsds[0])) if single else (out, values, rmsds)
