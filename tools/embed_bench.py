"""Conformer embedding: conformers per second and the share that passes the acceptance test (csrc/conformer_embed.hip).

For the 1a0q ligand (tests/golden/1a0q, 23 heavy atoms, handedness from the crystal pose) and a synthetic branched 64-carbon alkane
(no pose), embeds `--conformers` conformers in one launch, `--repeats` times with fresh seeds, and prints one JSON line per case:
conformers per second of the whole call (bounds already built; upload, launch, download) and the share of `ok` first attempts.

    python tools/embed_bench.py [--conformers 1024] [--repeats 5]
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


def ligand_1a0q():
    """-> (perceived heavy-atom Mol, crystal pose)"""
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    mol = pm.read_molecule(os.path.join(ROOT, "tests", "golden", "1a0q", "1a0q_ligand.sdf"), sanitize=True, remove_hs=True)
    return mol, mol.GetConformer().GetPositions()


def synthetic_alkane(n_atoms=64, seed=1):
    """A random tree of `n_atoms` carbons with every degree <= 4 (no pose: volume constraints without a sign)."""
    from confidence_bootstrapping_amd.datasets.molfile import Atom, Bond, Mol, perceive
    rng = np.random.default_rng(seed)
    degree, bonds = [0] * n_atoms, []
    for i in range(1, n_atoms):
        open_atoms = [j for j in range(i) if degree[j] < (3 if j == i - 1 else 4)]
        p = i - 1 if rng.random() < 0.6 and degree[i - 1] < 4 else int(rng.choice(open_atoms))
        bonds.append(Bond(p, i, 1))
        degree[p] += 1
        degree[i] += 1
    return perceive(Mol([Atom(i, 6, "C") for i in range(n_atoms)], bonds, np.zeros((n_atoms, 3)))), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conformers", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    from confidence_bootstrapping_amd.datasets import conformer_embedding as ce
    for name, (mol, ref) in (("1a0q", ligand_1a0q()), ("synthetic_alkane_64", synthetic_alkane())):
        t0 = time.perf_counter()
        bounds = ce.distance_bounds(mol, ref)
        t_bounds = time.perf_counter() - t0
        ce.embed_conformers_batch([bounds], 4, seed=99)                      # warm-up: library, allocator
        torch.cuda.synchronize()
        times, shares = [], []
        for r in range(a.repeats):
            t0 = time.perf_counter()
            _, ok, _ = ce.embed_conformers_batch([bounds], a.conformers, seed=r)[0]        # the download synchronises
            times.append(time.perf_counter() - t0)
            shares.append(float(ok.mean()))
        best = min(times)
        print(json.dumps({"case": name, "atoms": int(mol.GetNumAtoms()), "constraints": int(len(bounds[2]["kind"])),
                          "conformers": a.conformers, "repeats": a.repeats, "bounds_host_seconds": round(t_bounds, 4),
                          "seconds_best": round(best, 5), "seconds_median": round(float(np.median(times)), 5),
                          "conformers_per_s": round(a.conformers / best, 1), "ok_share": round(float(np.mean(shares)), 4),
                          "iteration_caps": list(ce.DEFAULT_ITERS)}))


if __name__ == "__main__":
    main()
