"""The output side of docking one complex: ranked pose files and the reverse-process frames, as the reference's dock.py:158-184 /
inference.py:532-560 write them."""
from __future__ import annotations

import copy
import os

import numpy as np
import torch

from .datasets.molfile import remove_hs as _remove_hs
from .datasets.process_mols import write_mol_with_coords


def _ranking(confidence, n, cpu):
    """-> (conf float64 [n] or None, order): descending confidence (NaN counts as -1e-6; a [N, k] confidence is ranked by its first
    column), `data_list` order without confidences"""
    if confidence is None:
        return None, np.arange(n)
    conf = cpu(confidence).astype(np.float64)
    if conf.ndim == 2:
        conf = conf[:, 0]
    if conf.shape != (n,):
        raise ValueError(f"{conf.shape} confidences for {n} poses")
    conf = np.nan_to_num(conf, nan=-1e-6)
    return conf, np.argsort(conf)[::-1]


def write_ranked_poses(out_dir, mol, data_list, confidence, visualization_list=None, remove_hs=True, modes=None):
    """Writes the poses of `data_list` (graphs of ONE complex after sampling(); positions = ['ligand'].pos + original_center) into
    `out_dir` as SDF files of `mol`, best first:
      rank1.sdf, rank{k}_confidence{c:.2f}.sdf for every pose      -- ranked by descending confidence (NaN counts as -1e-6; a
                                                                      [N, k] confidence is ranked by its first column)
      rank{k}.sdf for every pose when `confidence` is None         -- in `data_list` order
      rank{k}_reverseprocess.pdb                                   -- when a `visualization_list` (one PDBFile per pose) is given
      mode{m}_rank{k}_confidence{c:.2f}.sdf for every mode's head, -- only with `modes` = (head, mode) indexed like `data_list` (ranked_modes):
      modes.csv                                                       m = 1 for the best-ranked mode, k the head's rank; without
                                                                      confidences mode{m}_rank{k}.sdf.  modes.csv: mode, head_rank,
                                                                      population, best_confidence, mean_confidence (one row per mode)
    `remove_hs`: `mol` is written without its hydrogens, as the score model saw it (a molecule that is already stripped is unchanged).
    Returns the rank order: order[k] is the index in `data_list` of the pose ranked k + 1."""
    n = len(data_list)
    if visualization_list is not None and len(visualization_list) != n:
        raise ValueError("visualization_list must hold one PDBFile per pose")
    cpu = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    ligand_pos = [cpu(g["ligand"].pos).astype(np.float32) + cpu(g.original_center).astype(np.float32).reshape(1, 3) for g in data_list]
    conf, order = _ranking(confidence, n, cpu)
    mol_pred = copy.deepcopy(mol)
    if remove_hs:
        mol_pred = _remove_hs(mol_pred)
    os.makedirs(out_dir, exist_ok=True)
    for rank, idx in enumerate(order):
        pos = ligand_pos[idx]
        if conf is None:
            write_mol_with_coords(mol_pred, pos, os.path.join(out_dir, f"rank{rank + 1}.sdf"))
            continue
        if rank == 0:
            write_mol_with_coords(mol_pred, pos, os.path.join(out_dir, "rank1.sdf"))
        write_mol_with_coords(mol_pred, pos, os.path.join(out_dir, f"rank{rank + 1}_confidence{conf[idx]:.2f}.sdf"))
    if visualization_list is not None:
        for rank, idx in enumerate(order):
            visualization_list[idx].write(os.path.join(out_dir, f"rank{rank + 1}_reverseprocess.pdb"))
    if modes is not None:
        head, mode = (np.asarray(x, dtype=np.int64) for x in modes)
        if head.shape != (n,) or mode.shape != (n,):
            raise ValueError(f"modes {head.shape} / {mode.shape} for {n} poses")
        rank_of = np.empty(n, dtype=np.int64)
        rank_of[order] = np.arange(n)
        rows = []
        for idx in sorted((i for i in range(n) if head[i] == i), key=lambda i: mode[i]):
            members = np.flatnonzero(mode == mode[idx])
            m, k = int(mode[idx]) + 1, int(rank_of[idx]) + 1
            tail = "" if conf is None else f"_confidence{conf[idx]:.2f}"
            write_mol_with_coords(mol_pred, ligand_pos[idx], os.path.join(out_dir, f"mode{m}_rank{k}{tail}.sdf"))
            stats = ("", "") if conf is None else (f"{conf[members].max():.6f}", f"{conf[members].mean():.6f}")
            rows.append(f"{m},{k},{len(members)},{stats[0]},{stats[1]}\n")
        with open(os.path.join(out_dir, "modes.csv"), "w") as f:
            f.write("mode,head_rank,population,best_confidence,mean_confidence\n" + "".join(rows))
    return [int(i) for i in order]


def ranked_modes(groups, device, cutoff=2.0):
    """Distinct binding modes of the docked poses of several complexes: `groups` = [(mol, data_list, confidence or None), ...] as
    write_ranked_poses takes them.  The heavy-atom poses of each complex are put in rank order (write_ranked_poses' ranking) and compared in
    the receptor frame: ONE evaluation.cluster_poses_batch call for all groups on a GPU `device`, evaluation.cluster_poses per group on any
    other.  -> [(head, mode), ...] indexed like each `data_list` (head[i]: the index in `data_list` of pose i's mode representative,
    mode[i]: 0, 1, ... best-ranked mode first; -1 for a pose with a coordinate that is not finite): write_ranked_poses' `modes`."""
    from .evaluation import cluster_poses, cluster_poses_batch
    from .molecules_utils import _graph_of, remove_all_hs
    cpu = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    items, orders = [], []
    for mol, data_list, confidence in groups:
        pos = np.stack([cpu(g["ligand"].pos).astype(np.float32) + cpu(g.original_center).astype(np.float32).reshape(1, 3) for g in data_list])
        _, order = _ranking(confidence, len(data_list), cpu)
        graph = None
        if mol is not None:
            nums = _graph_of(mol)[0]
            graph = remove_all_hs(mol)
            if pos.shape[1] == len(nums) and (nums == 1).any():      # the graphs carry the hydrogens: modes are compared on heavy atoms
                pos = pos[:, nums != 1]
        items.append((pos[order], graph))
        orders.append(np.asarray(order))
    if torch.device(device).type == "cuda":
        found = cluster_poses_batch(items, device, cutoff=cutoff)
    else:
        found = [cluster_poses(lp, graph, cutoff=cutoff) for lp, graph in items]
    out = []
    for order, (_, head_r, mode_r, _) in zip(orders, found):
        head, mode = np.full(len(order), -1, dtype=np.int32), np.full(len(order), -1, dtype=np.int32)
        head[order] = np.where(head_r >= 0, order[np.maximum(head_r, 0)], -1)
        mode[order] = mode_r
        out.append((head, mode))
    return out


POSE_CHECK_COLUMNS = ("rank", "confidence", "valid", "n_bad_bond", "n_bad_angle", "n_internal_clash", "n_rec_clash", "bond_lo", "bond_hi",
                      "angle_lo", "angle_hi", "clash_ratio", "rec_ratio", "rec_dist", "rec_lig_atom", "rec_atom", "flags")


def pose_check_rows(groups, device, **thresholds):
    """Are the docked poses physically possible?  `groups` = [(mol, data_list, confidence or None, receptor graph or None), ...]: the first
    three as write_ranked_poses takes them, the fourth a graph with an 'atom' store (the complex that was docked; its protein heavy atoms
    are the receptor) or None (internal checks only).  The heavy-atom poses of each complex are put in rank order (write_ranked_poses'
    ranking) and checked in absolute coordinates with evaluation.pose_checks' four distance checks: ONE evaluation.pose_checks_batch call
    for all groups on a GPU `device`, evaluation.pose_checks per group on any other.  -> [(order, conf float64 [n] or None, PoseChecks whose
    arrays are IN RANK ORDER), ...]: write_pose_checks' `rows`."""
    from .evaluation import ligand_check_tables, pose_checks, pose_checks_batch, receptor_check_atoms
    from .molecules_utils import _graph_of
    cpu = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    items, ranked, receptors = [], [], {}
    for mol, data_list, confidence, graph in groups:
        pos = np.stack([cpu(g["ligand"].pos).astype(np.float32) + cpu(g.original_center).astype(np.float32).reshape(1, 3) for g in data_list])
        conf, order = _ranking(confidence, len(data_list), cpu)
        tables = None
        if mol is not None:
            nums = _graph_of(mol)[0]
            tables = ligand_check_tables(mol)
            if pos.shape[1] == len(nums) and (nums == 1).any():      # the graphs carry the hydrogens: the checks are on heavy atoms
                pos = pos[:, nums != 1]
            if len(tables[3]) != pos.shape[1]:
                tables = None
        if graph is not None and id(graph) not in receptors:      # complexes docked into the same graph object share one receptor upload
            rec = receptor_check_atoms(graph)
            receptors[id(graph)] = None if rec is None else (rec[0] + cpu(graph.original_center).astype(np.float32).reshape(1, 3), rec[1])
        items.append((pos[order], tables, receptors.get(id(graph)) if graph is not None else None))
        ranked.append((np.asarray(order), conf))
    if torch.device(device).type == "cuda":
        found = pose_checks_batch(items, device, **thresholds)
    else:
        found = [pose_checks(*item, **thresholds) for item in items]
    return [(order, conf, checks) for (order, conf), checks in zip(ranked, found)]


def write_pose_checks(out_dir, rows):
    """`rows` = one entry of pose_check_rows -> `out_dir`/pose_checks.csv, one row per rank (POSE_CHECK_COLUMNS): rank, confidence (empty
    without confidences), valid (1 / 0), the four counts, the seven ratios and distances (bond_lo .. rec_dist; nan where a check did not
    run), the closest receptor atom as (rec_lig_atom, rec_atom) and the flags of evaluation.pose_checks.  Returns the path."""
    order, conf, checks = rows
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "pose_checks.csv")
    with open(path, "w") as f:
        f.write(",".join(POSE_CHECK_COLUMNS) + "\n")
        for rank, idx in enumerate(order):
            cells = [str(rank + 1), "" if conf is None else f"{conf[idx]:.6f}", str(int(checks.valid[rank]))]
            for name in POSE_CHECK_COLUMNS[3:]:
                v = getattr(checks, name)[rank]
                cells.append(f"{float(v):.6f}" if v.dtype == np.float32 else str(int(v)))
            f.write(",".join(cells) + "\n")
    return path
