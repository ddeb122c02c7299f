"""The output side of docking one complex: ranked pose files and the reverse-process frames, as the reference's dock.py:158-184 /
inference.py:532-560 write them."""
from __future__ import annotations

import copy
import os

import numpy as np
import torch

from .datasets.molfile import remove_hs as _remove_hs
from .datasets.process_mols import write_mol_with_coords


def write_ranked_poses(out_dir, mol, data_list, confidence, visualization_list=None, remove_hs=True):
    """Writes the poses of `data_list` (graphs of ONE complex after sampling(); positions = ['ligand'].pos + original_center) into
    `out_dir` as SDF files of `mol`, best first:
      rank1.sdf, rank{k}_confidence{c:.2f}.sdf for every pose      -- ranked by descending confidence (NaN counts as -1e-6; a
                                                                      [N, k] confidence is ranked by its first column)
      rank{k}.sdf for every pose when `confidence` is None         -- in `data_list` order
      rank{k}_reverseprocess.pdb                                   -- when a `visualization_list` (one PDBFile per pose) is given
    `remove_hs`: `mol` is written without its hydrogens, as the score model saw it (a molecule that is already stripped is unchanged).
    Returns the rank order: order[k] is the index in `data_list` of the pose ranked k + 1."""
    n = len(data_list)
    if visualization_list is not None and len(visualization_list) != n:
        raise ValueError("visualization_list must hold one PDBFile per pose")
    cpu = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    ligand_pos = [cpu(g["ligand"].pos).astype(np.float32) + cpu(g.original_center).astype(np.float32).reshape(1, 3) for g in data_list]
    if confidence is not None:
        conf = cpu(confidence).astype(np.float64)
        if conf.ndim == 2:
            conf = conf[:, 0]
        if conf.shape != (n,):
            raise ValueError(f"{conf.shape} confidences for {n} poses")
        conf = np.nan_to_num(conf, nan=-1e-6)
        order = np.argsort(conf)[::-1]
    else:
        conf, order = None, np.arange(n)
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
    return [int(i) for i in order]
