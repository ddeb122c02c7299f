"""Inputs with known binding modes and a brute-force fp64 restatement of cbd_pose_modes' definitions, for tests/test_pose_modes.py (host) and
tests/test_gpu_pose_modes.py (device).  The ligands and the 1/64 A grid are tests/metrics_helpers.py's."""
import numpy as np

from tests.metrics_helpers import LIGANDS, coords

N_MODES, PER_MODE, CUTOFF = 5, 8, 2.0
SIZES = (1, 2, 8, 9, 17, 40)      # poses per group: the diagonal tile alone, a full tile, one pose past it, three tiles, 5 x 5 tiles


def mode_poses(mol, iso):
    """40 poses of `mol` on the grid around 5 centres, 8 per centre in shuffled order: a centre plus N(0, 0.3) jitter, written under a
    random isomorphism of the ligand (so that the identity mapping is not the best one).  -> (poses float32 [40, N, 3], centre of each)"""
    n = len(mol.atomicnums)
    centres = coords(n, N_MODES, seed=11)
    rng = np.random.default_rng(7)
    label = rng.permutation(np.repeat(np.arange(N_MODES), PER_MODE))
    lp = np.empty((len(label), n, 3), dtype=np.float32)
    for p, c in enumerate(label):
        x = centres[c] + (np.round(rng.normal(0.0, 0.3, size=(n, 3)) * 64.0) / 64.0).astype(np.float32)
        k = int(rng.integers(iso[0].shape[0]))
        lp[p, iso[1][k]] = x[iso[0][k]]
    return lp, label


def brute_matrix(lp, idx1, idx2):
    """float64 [P, P] by a triple loop over (i, j, k): sqrt(min_k sum_a |x_i[idx1[k, a]] - x_j[idx2[k, a]]|^2 / N) for i < j, mirrored;
    the diagonal 0.  Not rounded to fp32."""
    x = np.asarray(lp, dtype=np.float64)
    P, N = x.shape[:2]
    d = np.zeros((P, P))
    for i in range(P):
        for j in range(i + 1, P):
            best = np.inf
            for k in range(idx1.shape[0]):
                best = min(best, float(((x[i, idx1[k]] - x[j, idx2[k]]) ** 2).sum()))
            d[i, j] = d[j, i] = np.sqrt(best / N)
    return d


def brute_modes(d, cutoff):
    """leader clustering in rank order, written out as loops: -> head, mode (lists), n_modes"""
    heads, head, mode = [], [], []
    for p in range(len(d)):
        if np.isnan(d[p][p]):
            head.append(-1)
            mode.append(-1)
            continue
        m = -1
        for r, h in enumerate(heads):
            if d[h][p] <= cutoff:
                m = r
                break
        if m < 0:
            heads.append(p)
            m = len(heads) - 1
        head.append(heads[m])
        mode.append(m)
    return head, mode, len(heads)


def expected_modes(label):
    """what the construction says: modes numbered in order of appearance, the first pose of each its head"""
    first = {}
    for p, c in enumerate(label):
        first.setdefault(int(c), p)
    number = {c: m for m, c in enumerate(sorted(first, key=first.get))}
    return [first[int(c)] for c in label], [number[int(c)] for c in label], len(first)


def assert_margin(d, label):
    """on the fp64 side, before any device result is looked at: same-centre pairs at most 1.0 A, all others at least 3.0 A apart -- no pair
    within 1.0 A of the 2.0 A cutoff -- and the matrix exactly symmetric"""
    same = label[:, None] == label[None]
    off = ~np.eye(len(label), dtype=bool)
    assert np.array_equal(d, d.T)
    if (same & off).any():
        assert d[same & off].max() <= CUTOFF - 1.0, d[same & off].max()
    if (~same).any():
        assert d[~same].min() >= CUTOFF + 1.0, d[~same].min()


def ligand_cases():
    """[(name, mol, (idx1, idx2), poses [40, N, 3], centre labels [40])] for the five ligands"""
    import confidence_bootstrapping_amd.molecules_utils as mu
    out = []
    for name, make, _ in LIGANDS:
        mol = make()
        iso = mu.graph_isomorphisms(mol.atomicnums, mol.adjacency_matrix)
        lp, label = mode_poses(mol, iso)
        out.append((name, mol, iso, lp, label))
    return out
