"""Torsion matching: GPU differential evolution (csrc/torsion_match.hip) against scipy's on the CPU, same problems, same arguments.

For the 1a0q ligand (tests/golden/1a0q, 23 heavy atoms) and a synthetic ligand with R = 16 rotatable bonds and Nl = 64 atoms, 10 tries
each (targets: the ligand with random torsions, a rigid motion and 0.2 A coordinate noise), prints matches per second on the GPU, the
time of `scipy.optimize.differential_evolution` on `conformer_matching.score_conformation` and the final RMSDs of both.

    python tools/match_bench.py [--maxiter 500] [--tries 10] [--cpu-tries 10] [--no-polish]

Also the home of the small problem generators that the conformer-matching tests share.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def synthetic_ligand(n_atoms, n_torsions, seed, branch=0.3):
    """A tree-shaped carbon skeleton with exactly `n_torsions` rotatable bonds: n_torsions + 1 inner atoms joined by the torsion bonds
    (a chain that branches with probability `branch`), the other atoms hang off them as end atoms.  Bond length 1.5 A, no bond
    collinear with its neighbour, no two atoms closer than 1 A.  -> (Mol, pos [n, 3] float64, quads, mask_rotate [R, n] bool)."""
    import torch
    from confidence_bootstrapping_amd.datasets.molfile import Atom, Bond, Mol
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    from confidence_bootstrapping_amd.hetero import HeteroData
    from confidence_bootstrapping_amd.torsion import get_transformation_mask
    rng = np.random.default_rng(seed)
    inner = n_torsions + 1
    spare = n_atoms - inner
    for _ in range(1000):
        parent = [-1] + [int(rng.integers(0, i)) if rng.random() < branch else i - 1 for i in range(1, inner)]
        deg = np.bincount([p for p in parent if p >= 0], minlength=inner) + (np.arange(inner) > 0)
        ends = [i for i in range(inner) if deg[i] < 2] if inner > 1 else [0]
        if len(ends) <= spare:
            break
        branch *= 0.5
    else:
        raise ValueError(f"{n_atoms} atoms cannot carry {n_torsions} torsion bonds")
    parent += ends + [int(rng.integers(0, inner)) for _ in range(spare - len(ends))]
    pos = np.zeros((n_atoms, 3))
    for i in range(1, n_atoms):
        p = parent[i]
        back = pos[parent[p]] - pos[p] if parent[p] >= 0 else None
        for _ in range(10000):
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            if back is not None and abs(d @ back) / np.linalg.norm(back) > 0.8:
                continue
            cand = pos[p] + 1.5 * d
            if i == 1 or np.linalg.norm(pos[:i] - cand, axis=1).min() > 1.0:
                break
        pos[i] = cand
    mol = Mol([Atom(i, 6, "C") for i in range(n_atoms)], [Bond(parent[i], i, 1) for i in range(1, n_atoms)], pos)
    g = HeteroData()
    g["ligand"].x = torch.zeros(n_atoms, 16, dtype=torch.long)
    ei = [[], []]
    for b in mol.GetBonds():
        ei[0] += [b.a, b.b]
        ei[1] += [b.b, b.a]
    g["ligand", "lig_bond", "ligand"].edge_index = torch.tensor(ei, dtype=torch.long)
    _, mask_rotate = get_transformation_mask(g)
    quads = cm.get_torsion_angles(mol)
    assert len(quads) == n_torsions == len(mask_rotate), (len(quads), n_torsions, len(mask_rotate))
    return mol, pos, quads, np.asarray(mask_rotate, dtype=bool)


def ligand_1a0q():
    """-> (Mol, pos, quads, mask_rotate) of the heavy-atom 1a0q ligand (11 rotatable bonds)."""
    from confidence_bootstrapping_amd.datasets import process_mols as pm, conformer_matching as cm
    g = pm.get_ligand(os.path.join(ROOT, "tests", "golden", "1a0q", "1a0q_ligand.sdf"), "1a0q")
    return g.mol, np.asarray(g["ligand"].orig_pos, dtype=np.float64), cm.get_torsion_angles(g.mol), np.asarray(g["ligand"].mask_rotate, dtype=bool)


def random_rigid(rng, pos, shift=5.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                    [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                    [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return (pos - pos.mean(0)) @ rot.T + pos.mean(0) + rng.normal(size=3) * shift


def make_target(pos, quads, mask_rotate, seed, noise=0.0):
    """The ligand with uniformly random torsions, moved rigidly, plus Gaussian coordinate noise of `noise` A."""
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    rng = np.random.default_rng(seed)
    t = cm.apply_changes(pos, rng.uniform(-np.pi, np.pi, len(quads)), quads, mask_rotate)
    return random_rigid(rng, t) + rng.normal(size=t.shape) * noise


def scipy_match(pos, target, quads, mask_rotate, seed=0, popsize=15, maxiter=500, mutation=(0.5, 1), recombination=0.8, polish=True):
    """The reference's optimiser call (datasets/conformer_matching.py:39-41) on the package's float64 objective."""
    from scipy.optimize import differential_evolution
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    qs, rows = cm._rows_of(quads, mask_rotate)
    phi = [cm.get_dihedral(pos, q) for q in qs]
    f = lambda x: cm.rigid_align(cm._set_dihedrals(pos, x, qs, rows, phi), target)[1]
    res = differential_evolution(f, [(-np.pi, np.pi)] * len(quads), maxiter=maxiter, popsize=popsize, mutation=mutation,
                                 recombination=recombination, disp=False, seed=seed, polish=polish)
    return res.x, float(res.fun), int(res.nfev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maxiter", type=int, default=500)
    ap.add_argument("--popsize", type=int, default=15)
    ap.add_argument("--tries", type=int, default=10)
    ap.add_argument("--cpu-tries", type=int, default=10, help="how many of the tries scipy also solves (its time is reported per try)")
    ap.add_argument("--no-polish", action="store_true")
    a = ap.parse_args()
    import torch
    from confidence_bootstrapping_amd.datasets import conformer_matching as cm
    cases = {"1a0q": ligand_1a0q()[1:], "synthetic_R16_Nl64": synthetic_ligand(64, 16, 1)[1:]}
    for name, (pos, quads, mask) in cases.items():
        target = make_target(pos, quads, mask, seed=11, noise=0.2)
        rng = np.random.default_rng(5)
        probes = np.stack([random_rigid(rng, cm.apply_changes(pos, rng.uniform(-np.pi, np.pi, len(quads)), quads, mask)) for _ in range(a.tries)])
        kw = dict(popsize=a.popsize, maxiter=a.maxiter)
        cm.optimize_rotatable_bonds(probes[:1], target, quads, mask, polish=False, popsize=a.popsize, maxiter=1)      # warm-up: library, LDS attribute
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = cm.match_torsions([(p, target, quads, mask) for p in probes], **kw)
        t_de = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, _, rmsd_gpu = cm.optimize_rotatable_bonds(probes, target, quads, mask, polish=not a.no_polish, **kw)
        t_all = time.perf_counter() - t0
        t0 = time.perf_counter()
        cpu = [scipy_match(p, target, quads, mask, polish=not a.no_polish, **kw) for p in probes[:a.cpu_tries]]
        t_cpu = time.perf_counter() - t0
        print(json.dumps({
            "case": name, "Nl": int(len(pos)), "R": int(len(quads)), "tries": a.tries, "maxiter": a.maxiter, "popsize": a.popsize,
            "gpu_de_seconds": round(t_de, 4), "gpu_matches_per_s": round(a.tries / t_de, 2), "gpu_generations": [g for _, _, g in found],
            "gpu_with_polish_seconds": round(t_all, 4), "gpu_rmsd": [round(float(r), 4) for r in rmsd_gpu],
            "scipy_seconds_per_try": round(t_cpu / max(len(cpu), 1), 3), "scipy_rmsd": [round(r, 4) for _, r, _ in cpu],
            "scipy_nfev": [n for _, _, n in cpu]}))


if __name__ == "__main__":
    main()
