"""Small ligands with known automorphism counts (no rdkit) and an fp64 numpy restatement of the five outputs of cbd_pose_metrics, for
tests/test_pose_metrics_batch.py (host) and tests/test_gpu_pose_metrics.py (device)."""
from argparse import Namespace

import numpy as np


def _mol(nums, bonds):
    nums = np.asarray(nums, dtype=np.int64)
    am = np.zeros((len(nums), len(nums)), dtype=int)
    for i, j in bonds:
        am[i, j] = am[j, i] = 1
    return Namespace(atomicnums=nums, adjacency_matrix=am)


def chain5():
    """C-N-O-S-F: five distinct elements, K = 1"""
    return _mol([6, 7, 8, 16, 9], [(i, i + 1) for i in range(4)])


def ring6():
    """a six-ring of one element: 6 rotations x 2 reflections, K = 12"""
    return _mol([6] * 6, [(i, (i + 1) % 6) for i in range(6)])


def star7():
    """N-O-C-C(F)(F)F: the three fluorines permute, K = 3! = 6"""
    return _mol([7, 8, 6, 6, 9, 9, 9], [(0, 1), (1, 2), (2, 3), (3, 4), (3, 5), (3, 6)])


def fork(n):
    """a tree of n atoms with ONE symmetric branch pair: a carbon path that starts at a nitrogen (so that it cannot be reversed) and ends
    in two fluorines, which swap: K = 2.  n = 65 and n = 130 cross the 64-lane boundary of the kernel's atom loop once and twice."""
    nums = [7] + [6] * (n - 3) + [9, 9]
    bonds = [(i, i + 1) for i in range(n - 3)] + [(n - 3, n - 2), (n - 3, n - 1)]
    return _mol(nums, bonds)


LIGANDS = (("chain5", chain5, 1), ("ring6", ring6, 12), ("star7", star7, 6), ("fork65", lambda: fork(65), 2), ("fork130", lambda: fork(130), 2))


def coords(n, rows, seed, spread=3.0):
    """`rows` sets of n fp32 coordinates on a 1/64 A grid (every difference and small sum of them is exact in fp32 and fp64)"""
    rng = np.random.default_rng(seed)
    return (np.round(rng.normal(0.0, spread, size=(rows, n, 3)) * 64.0) / 64.0).astype(np.float32)


def metrics64(lp, ref, idx1, idx2):
    """fp64 restatement: lp [P, N, 3], ref [Q, N, 3], isomorphisms idx1 / idx2 [K, N] (crystal atom idx1[k, i] <-> pose atom idx2[k, i])
    -> rmsd, centroid, min_self (float64 [P]), argmin_ref, argmin_iso (int [P]); the first minimum wins: per crystal pose the lowest k,
    then the lowest q."""
    lp, ref = np.asarray(lp, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ref = ref[None] if ref.ndim == 2 else ref
    P, N = lp.shape[:2]
    d = ref[:, None][:, :, idx1] - lp[None][:, :, idx2]          # [Q, P, K, N, 3]
    S = (d ** 2).sum(axis=(3, 4))                                # [Q, P, K]
    k_of = S.argmin(axis=2)                                      # [Q, P] lowest k
    r = np.sqrt(S.min(axis=2) / N)                               # [Q, P]
    q_of = r.argmin(axis=0)
    rmsd = r.min(axis=0)
    centroid = np.linalg.norm(lp.mean(axis=1)[None] - ref.mean(axis=1)[:, None], axis=2).min(axis=0)
    dd = np.linalg.norm(lp[:, :, None] - lp[:, None], axis=3) + np.where(np.eye(N, dtype=bool), np.inf, 0.0)[None]
    return rmsd, centroid, dd.reshape(P, -1).min(axis=1), q_of, k_of[q_of, np.arange(P)]
