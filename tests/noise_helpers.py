"""Shared by tests/test_noise_batch.py and tests/test_gpu_noise_batch.py: random-tree ligands with an exact number of rotatable bonds
(masks from the project's get_transformation_mask) and an fp64 numpy restatement of modify_conformer."""
import numpy as np
import torch


def tree_ligand(nl, r, seed, nr=6, name=None):
    """A complex whose ligand is a random tree of `nl` atoms with exactly `r` rotatable bonds.  In a tree every bond is a bridge and it is
    rotatable unless it ends in a leaf, so: a random tree of r + 1 inner atoms (r bonds), every inner atom that is a leaf of that tree gets
    a leaf atom of its own, the remaining leaf atoms hang on random inner atoms; atom labels are shuffled.  nl = 1, 2: no bonds / one bond."""
    from confidence_bootstrapping_amd.hetero import HeteroData
    from confidence_bootstrapping_amd.torsion import get_transformation_mask
    rng = np.random.default_rng(seed)
    bonds = []
    if nl == 2:
        assert r == 0
        bonds = [(0, 1)]
    elif nl > 2:
        inner = r + 1
        for attempt in range(1000):
            skel = [(int(rng.integers(0, k)), k) for k in range(1, inner)]
            deg = np.bincount(np.asarray(skel, dtype=np.int64).reshape(-1), minlength=inner) if skel else np.zeros(inner, dtype=np.int64)
            need = [k for k in range(inner) if deg[k] <= 1]
            if len(need) <= nl - inner:
                break
        else:
            raise RuntimeError(f"no tree with nl={nl}, r={r}")
        hosts = need + [int(rng.integers(0, inner)) for _ in range(nl - inner - len(need))]
        bonds = skel + [(h, inner + k) for k, h in enumerate(hosts)]
    else:
        assert r == 0
    # positions: every atom 1.5 A from its parent in a random direction (parents come first in `bonds`)
    pos = np.zeros((nl, 3))
    for a, b in bonds:
        step = rng.normal(size=3)
        pos[b] = pos[a] + 1.5 * step / np.linalg.norm(step)
    perm = rng.permutation(nl)
    pos_p = np.zeros_like(pos)
    pos_p[perm] = pos
    ei = np.zeros((2, 2 * len(bonds)), dtype=np.int64)
    for k, (a, b) in enumerate(bonds):
        a, b = (perm[a], perm[b]) if rng.random() < 0.5 else (perm[b], perm[a])
        ei[:, 2 * k], ei[:, 2 * k + 1] = (a, b), (b, a)
    g = HeteroData()
    g["ligand"].x = torch.zeros(nl, 16, dtype=torch.long)
    g["ligand"].pos = torch.from_numpy((pos_p - pos_p.mean(0) + rng.normal(0, 6, size=3)).astype(np.float32))
    g["ligand", "ligand"].edge_index = torch.from_numpy(ei)
    me, mr = get_transformation_mask(g)
    assert int(me.sum()) == r and mr.shape == (r, nl), (nl, r, int(me.sum()))
    g["ligand"].edge_mask = torch.from_numpy(me)
    g["ligand"].mask_rotate = mr
    g["receptor"].pos = torch.from_numpy(rng.normal(0, 10, size=(nr, 3)).astype(np.float32))
    g.name = name or f"tree_nl{nl}_r{r}_s{seed}"
    return g


def rot_edges(g):
    """[R, 2] (u, v) of the rotatable bonds in edge_mask order"""
    return g["ligand", "ligand"].edge_index.T[g["ligand"].edge_mask].numpy().reshape(-1, 2)


def bonds_of(g):
    return g["ligand", "ligand"].edge_index.numpy()[:, ::2].T.reshape(-1, 2)


def rotvec_matrix64(v):
    """Rodrigues in fp64"""
    v = np.asarray(v, dtype=np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def modify_conformer64(pos, edges, mask_rotate, tr, rot, tor):
    """(out, rigid) of modify_conformer (pivot = None) in fp64 on fp32 inputs: rigid move about the centroid, sequential torsions (a bond
    whose update is 0 is skipped), Kabsch alignment of the flexed pose onto the rigid one; tor = None or no bonds: out = rigid."""
    p = np.asarray(pos, dtype=np.float64)
    c = p.mean(0, keepdims=True)
    rigid = (p - c) @ rotvec_matrix64(rot).T + np.asarray(tr, dtype=np.float64).reshape(1, 3) + c
    if tor is None or len(edges) == 0:
        return rigid, rigid
    flex = rigid.copy()
    for k, (u, v) in enumerate(edges):
        if tor[k] == 0:
            continue
        axis = flex[u] - flex[v]
        q = rotvec_matrix64(axis * float(tor[k]) / np.linalg.norm(axis))
        m = np.asarray(mask_rotate[k], dtype=bool)
        flex[m] = (flex[m] - flex[v]) @ q.T + flex[v]
    ca, cb = flex.mean(0, keepdims=True), rigid.mean(0, keepdims=True)
    U, _, Vt = np.linalg.svd((flex - ca).T @ (rigid - cb))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return (flex - ca) @ R.T + cb, rigid
