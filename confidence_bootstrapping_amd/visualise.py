"""Multi-model PDB files of a ligand's reverse-diffusion frames: the reference's `utils/visualise.PDBFile` for a `molfile.Mol`.

The reference keeps an rdkit molecule, moves its conformer to every added pose and stores rdkit's `MolToPDBBlock` text of it; `write`
strings the stored blocks together as MODEL ... ENDMDL frames.  rdkit is not a dependency here, so the block is written by this module:
fixed-column HETATM records (residue UNL 1, atom names = element symbol + running number per element, coordinates %8.3f in columns
31-54, occupancy 1.00, B-factor 0.00, element right-justified in columns 77-78, formal charge in 79-80) followed by one CONECT record
per bonded atom that lists its neighbours once each.  The frame bookkeeping (parts, orders, repeats, CONECT only in the first written
frame) is the reference's.  What is NOT pinned: the exact text of rdkit's `MolToPDBBlock` (its atom naming, its repetition of a
neighbour in CONECT for a double bond) -- nothing in this project can run rdkit to compare; viewers read either form.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np
import torch

from .datasets.molfile import Mol


def _as_coords(coords, n_atoms):
    if torch.is_tensor(coords):
        coords = coords.detach().cpu().double().numpy()
    xyz = np.asarray(coords, dtype=np.float64)
    if xyz.ndim != 2 or xyz.shape != (n_atoms, 3):
        raise ValueError(f"coordinates of shape {tuple(xyz.shape)} for a molecule of {n_atoms} atoms")
    if not np.isfinite(xyz).all() or xyz.max(initial=0.0) >= 9999.9995 or xyz.min(initial=0.0) <= -999.9995:
        raise ValueError("coordinates must be finite and fit the eight columns of a PDB coordinate field")
    return xyz


def pdb_block(mol: Mol, coords=None):
    """The lines of one frame: HETATM records of `mol` at `coords` [N, 3] (default: its own), then the CONECT records."""
    atoms = mol.GetAtoms()
    if len(atoms) > 99999:
        raise ValueError("a PDB serial number holds five digits")
    xyz = _as_coords(mol.pos if coords is None else coords, len(atoms))
    lines, seen = [], {}
    for i, (a, (x, y, z)) in enumerate(zip(atoms, xyz)):
        sym = a.symbol or "X"
        seen[sym] = seen.get(sym, 0) + 1
        name = sym.upper() + str(seen[sym])
        if len(sym) == 1 and len(name) < 4:          # a one-letter element starts in column 14
            name = " " + name
        charge = "" if not a.charge else f"{abs(a.charge)}{'+' if a.charge > 0 else '-'}"
        lines.append("HETATM%5d %-4.4s %3s %1s%4d    %8.3f%8.3f%8.3f%6.2f%6.2f          %2s%-2s"
                     % (i + 1, name, "UNL", " ", 1, x, y, z, 1.0, 0.0, sym.upper(), charge))
    for i in range(len(atoms)):
        nbrs = sorted({j for j, _ in mol.neighbors(i)})
        if nbrs:
            lines.append("CONECT%5d" % (i + 1) + "".join("%5d" % (j + 1) for j in nbrs))
    return lines


class PDBFile:
    """Frames of one molecule, grouped into parts and ordered within a part (reference utils/visualise.py:10-52)."""

    def __init__(self, mol: Mol):
        self.parts = defaultdict(dict)
        self.mol = mol

    def add(self, coords, order, part=0, repeat=1):
        """`coords`: an [N, 3] ndarray or tensor for the molecule given at construction, or a `Mol`, written with its own atoms and
        coordinates.  A frame added under a (part, order) that is already taken replaces it."""
        block = pdb_block(coords) if isinstance(coords, Mol) else pdb_block(self.mol, coords)
        self.parts[part][order] = {"block": block, "repeat": repeat}

    def write(self, path=None, limit_parts=None):
        """Parts ascending (`limit_parts`: only the parts below it); within a part the non-negative orders ascending, then the negative
        ones ascending; every frame `repeat` times as MODEL ... ENDMDL; CONECT records in the first written frame only.  Returns the
        text when `path` is None, else writes it there."""
        is_first = True
        out = []
        for part in sorted(self.parts.keys()):
            if limit_parts and part >= limit_parts:
                break
            frames = self.parts[part]
            keys = sorted(k for k in frames if k >= 0) + sorted(k for k in frames if k < 0)
            for key in keys:
                block = frames[key]["block"]
                for _ in range(frames[key]["repeat"]):
                    if not is_first:
                        block = [line for line in block if not line.startswith("CONECT")]
                    is_first = False
                    out.append("MODEL\n" + "\n".join(block) + "\nENDMDL\n")
        text = "".join(out)
        if not path:
            return text
        with open(path, "w") as f:
            f.write(text)
