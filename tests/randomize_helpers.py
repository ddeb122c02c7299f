"""Shared by tests/test_randomize_batch.py and tests/test_gpu_randomize_batch.py: an fp64 numpy restatement of randomize_position's
arithmetic fed with prescribed draws, and the per-graph arrays it takes."""
import numpy as np

from tests.noise_helpers import bonds_of, rot_edges, rotvec_matrix64, tree_ligand  # noqa: F401  (re-exported for the two test files)


def randomize64(pos, edges, mask_rotate, tor, rot_mat, center, tr):
    """randomize_position for one pose in fp64 on the given (fp32) inputs: sequential torsions in `edges` order (a bond whose update is
    0 is skipped, no alignment afterwards), then (flex - mean(flex)) rot_mat^T + center (+ tr).  tor = None: no_torsion; tr = None:
    no_random.  -> float64 [Nl, 3]"""
    flex = np.array(pos, dtype=np.float64)
    if tor is not None:
        for k, (u, v) in enumerate(edges):
            if tor[k] == 0:
                continue
            axis = flex[u] - flex[v]
            q = rotvec_matrix64(axis * float(tor[k]) / np.linalg.norm(axis))
            m = np.asarray(mask_rotate[k], dtype=bool)
            flex[m] = (flex[m] - flex[v]) @ q.T + flex[v]
    out = (flex - flex.mean(0, keepdims=True)) @ np.asarray(rot_mat, dtype=np.float64).reshape(3, 3).T + np.asarray(center, dtype=np.float64).reshape(1, 3)
    if tr is not None:
        out = out + np.asarray(tr, dtype=np.float64).reshape(1, 3)
    return out


def graph_arrays(g):
    """(pos float32 [Nl, 3], edges [R, 2], mask_rotate bool [R, Nl]) of a graph or a Batch of one graph"""
    from confidence_bootstrapping_amd.sampling import _mask_rotate_of
    pos = g["ligand"].pos.numpy()
    edges = rot_edges(g)
    return pos, edges, np.asarray(_mask_rotate_of(g), dtype=bool).reshape(len(edges), pos.shape[0])


def randomize64_list(data_list, center, draws):
    """randomize64 for every graph of a data_list with the draws of draw_randomization -> list of float64 [Nl, 3]"""
    tor, rot_mat, tr = draws
    return [randomize64(*graph_arrays(g), None if tor is None else tor[k], rot_mat[k].numpy(), center, None if tr is None else tr[k].numpy())
            for k, g in enumerate(data_list)]
