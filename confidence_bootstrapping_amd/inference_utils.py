"""The reference's inference-time datasets (utils/inference_utils.py:155-371) without rdkit, ESM or torch_geometric:

  InferenceDataset   a list of (protein file, SMILES or ligand file) pairs -- what dock.py builds from its arguments or its CSV;
  ScreeningDataset   one receptor and a list of SMILES.

Same constructor arguments and item layout as the reference, plus `device=None, seed=0`.  What differs:

  * A SMILES is read by datasets/smiles.py, a file by datasets/molfile.py.  Every ligand gets a FRESH conformer, also one that came
    from a file (the reference calls RemoveAllConformers() and embeds again): the docked ligand never carries the bond lengths and
    angles of its crystal pose.  The conformers come from the GPU distance-geometry embedding (datasets/conformer_embedding.py) in
    place of ETKDG: ALL ligands of a dataset in ONE `embed_conformers_batch` launch in the constructor, three conformer ids each,
    `mol_ids` = the ligand's index in the list, so a ligand's conformer does not depend on what else the list holds; one further
    launch (ids 3..5) covers only the ligands none of whose first three was accepted; if none of the six is, the least-violating one
    is taken.  Stereo comes from the tags of a SMILES (`stereo="tags"`) and from the pose of a file (`ref_pos`).
  * Hydrogens are not added (the reference embeds AddHs(mol)).  With `remove_hs=True` -- both shipped model configurations -- the
    model sees heavy atoms either way; `remove_hs=False` with a SMILES ligand raises NotImplementedError.
  * The receptor is featurised by `process_mols.get_receptor` (HIP neighbour search), with the k-nearest-neighbour graphs
    `get_complex` builds (`knn_only_graph=True`).
  * Language-model embeddings are passed in: `lm_embeddings` / `precomputed_lm_embeddings` take arrays, or paths of `.npy` files, of
    shape [residues, 1280], one per complex.  Computing ESM embeddings (`lm_embeddings=True` without precomputed ones) and folding a
    `protein_sequence` (a `protein_file` of None) raise NotImplementedError.
  * A ligand that cannot be read, parsed or given bounds makes an item with `success = False` and a printed reason, as in the
    reference; it is left out of the launches.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .datasets import conformer_embedding as ce
from .datasets import process_mols as pm
from .datasets.cache_reader import merge_ligand_receptor
from .datasets.molfile import remove_hs as _remove_hs
from .datasets.smiles import mol_from_smiles
from .hetero import HeteroData

ATTEMPTS = 3           # conformer ids per ligand and launch (reference generate_conformer: up to 3 embedding attempts)


def is_ligand_file(description) -> bool:
    """A ligand description names a file when it ends in .sdf or .mol2 and the file exists; anything else is read as a SMILES."""
    return isinstance(description, str) and description.endswith((".sdf", ".mol2")) and os.path.exists(description)


def _load_embedding(e):
    if e is None:
        return None
    if isinstance(e, (str, os.PathLike)):
        e = np.load(e)
    if isinstance(e, (list, tuple)):                    # per-chain blocks in chain order, as the reference keeps them
        e = np.concatenate([t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in e], axis=0)
    if torch.is_tensor(e):
        e = e.detach().cpu().numpy()
    return np.asarray(e, dtype=np.float32)


def _read_ligand(description, remove_hs):
    """-> (mol without hydrogens if remove_hs, ref_pos or None, stereo) ; raises with the reason when it cannot be read."""
    if is_ligand_file(description):
        mol = pm.read_molecule(description, remove_hs=False, sanitize=True)
        if mol is None or isinstance(mol, Exception):
            raise Exception("could not read the molecule file " + str(description))
        if remove_hs:
            mol = _remove_hs(mol)
        return mol, mol.GetConformer().GetPositions(), "pose"
    mol = mol_from_smiles(description)
    if remove_hs:
        mol = _remove_hs(mol)
    return mol, None, "tags"


def embed_ligands(descriptions, remove_hs, seed=0, device=None):
    """Reads every description and embeds a fresh conformer of every readable ligand: one launch for all of them, one more for those
    without an accepted conformer.  -> (mols, reasons): mols[i] with its new coordinates, or None and reasons[i] the exception."""
    mols, reasons, bounds = [None] * len(descriptions), [None] * len(descriptions), {}
    for i, d in enumerate(descriptions):
        try:
            mol, ref, stereo = _read_ligand(d, remove_hs)
            bounds[i] = ce.distance_bounds(mol, ref, stereo=stereo)
            mols[i] = mol
        except Exception as e:                                # the reference catches everything here as well
            reasons[i] = e
    good = sorted(bounds)
    if not good:
        return mols, reasons
    first = ce.embed_conformers_batch([bounds[i] for i in good], ATTEMPTS, seed=seed, device=device, mol_ids=good)
    retry = []
    for i, (pos, ok, err) in zip(good, first):
        if ok.any():
            mols[i].pos = pos[int(np.nonzero(ok)[0][0])].copy()
        else:
            retry.append(i)
    if retry:
        second = ce.embed_conformers_batch([bounds[i] for i in retry], ATTEMPTS, seed=seed, device=device, mol_ids=retry,
                                           conf_ids=[np.arange(ATTEMPTS, 2 * ATTEMPTS)] * len(retry))
        for i, (pos2, ok2, err2) in zip(retry, second):
            pos, _, err = first[good.index(i)]
            if ok2.any():
                mols[i].pos = pos2[int(np.nonzero(ok2)[0][0])].copy()
            else:
                allpos, allerr = np.concatenate([pos, pos2]), np.concatenate([err, err2])
                mols[i].pos = allpos[int(np.argmin(allerr))].copy()
    return mols, reasons


def _ligand_graph(mol, remove_hs):
    g = HeteroData()
    pm.get_lig_graph_with_matching(mol, g, popsize=None, maxiter=None, matching=False, keep_original=False, num_conformers=1,
                                   remove_hs=remove_hs)
    return g


class _Dataset:
    def __len__(self):
        return self.len()

    def __getitem__(self, idx):
        return self.get(idx)

    def __iter__(self):
        return (self.get(i) for i in range(self.len()))


class InferenceDataset(_Dataset):
    """Reference utils/inference_utils.py:155-281; see the module text.  An item is a HeteroData with the ligand stores (centred on the
    ligand's own centroid), the receptor stores (and `atom` with `all_atoms`; centred on the C-alpha centroid, kept as
    `original_center`), `mol` (with the embedded conformer), `name` and `success`."""

    def __init__(self, out_dir, complex_names, protein_files, ligand_descriptions, protein_sequences, lm_embeddings,
                 receptor_radius=30, c_alpha_max_neighbors=None, precomputed_lm_embeddings=None, remove_hs=False, all_atoms=False,
                 atom_radius=5, atom_max_neighbors=None, device=None, seed=0):
        self.receptor_radius, self.c_alpha_max_neighbors = receptor_radius, c_alpha_max_neighbors
        self.remove_hs, self.all_atoms = remove_hs, all_atoms
        self.atom_radius, self.atom_max_neighbors = atom_radius, atom_max_neighbors
        self.complex_names, self.protein_files = list(complex_names), list(protein_files)
        self.ligand_descriptions, self.protein_sequences = list(ligand_descriptions), protein_sequences
        self.device, self.seed = device, seed
        n = len(self.complex_names)
        if not (len(self.protein_files) == len(self.ligand_descriptions) == n):
            raise ValueError("one protein file and one ligand description per complex name")
        if lm_embeddings is None or lm_embeddings is False:
            self.lm_embeddings = [None] * n
        elif lm_embeddings is True:
            if precomputed_lm_embeddings is None or precomputed_lm_embeddings[0] is None:
                raise NotImplementedError("computing ESM embeddings is not covered: pass precomputed_lm_embeddings (arrays or .npy "
                                          "paths of shape [residues, 1280], one per complex)")
            self.lm_embeddings = [_load_embedding(e) for e in precomputed_lm_embeddings]
        else:
            self.lm_embeddings = [_load_embedding(e) for e in lm_embeddings]
        if len(self.lm_embeddings) != n:
            raise ValueError("one language-model embedding per complex")
        if any(p is None for p in self.protein_files):
            raise NotImplementedError("a protein_file of None means folding the protein_sequence with ESMFold, which is not covered")
        if not remove_hs and any(not is_ligand_file(d) for d in self.ligand_descriptions):
            raise NotImplementedError("remove_hs=False with a SMILES ligand: hydrogens would have to be added (both shipped model "
                                      "configurations use remove_hs: true)")
        self.mols, self.reasons = embed_ligands(self.ligand_descriptions, remove_hs, seed=seed, device=device)

    def len(self):
        return len(self.complex_names)

    def get(self, idx):
        name, protein_file, description, lm = (self.complex_names[idx], self.protein_files[idx], self.ligand_descriptions[idx],
                                               self.lm_embeddings[idx])
        mol = self.mols[idx]
        if mol is None:
            print("Failed to read molecule ", description, " We are skipping it. The reason is the exception: ", self.reasons[idx])
            failed = HeteroData()
            failed.name, failed.success = name, False
            return failed
        g = _ligand_graph(mol, self.remove_hs)
        g.name = name
        if lm is not None and len(pm.parse_pdb(protein_file).seq) != len(lm):
            print(f"LM embeddings for complex {name} did not have the right length for the protein. Skipping {name}.")
            failed = HeteroData()
            failed.name, failed.success = name, False
            return failed
        rec = pm.get_receptor(protein_file, name, ce._device(self.device), receptor_radius=self.receptor_radius,
                              c_alpha_max_neighbors=self.c_alpha_max_neighbors, knn_only_graph=True, all_atoms=self.all_atoms,
                              atom_radius=self.atom_radius, atom_max_neighbors=self.atom_max_neighbors,
                              lm_embeddings=None if lm is None else [lm])
        for key, st in rec._stores.items():
            g._stores[key] = st
        g.receptor_name = rec.receptor_name
        g.original_center = rec.original_center
        g["ligand"].pos = g["ligand"].pos - torch.mean(g["ligand"].pos, dim=0, keepdim=True)
        g.mol = mol
        g.success = True
        return g


class ScreeningDataset(_Dataset):
    """Reference utils/inference_utils.py:284-371: one receptor, featurised once by `process_mols.get_receptor`, and a list of SMILES.
    An item is `cache_reader.merge_ligand_receptor` of the shared receptor graph and the ligand's own stores, the ligand centred on
    its centroid, `name` = the SMILES.  The reference deep-copies the receptor for every item; here all items SHARE the receptor's
    tensors (1281 floats per residue and the all-atom stores): treat them as read-only -- re-bind attributes, never write into them.
    Items of one screening set go through `sampling()` together in one `data_list`; its co-scheduling advances up to eight per launch."""

    def __init__(self, protein_file, ligand_smiles, lm_embeddings, receptor_radius=30, c_alpha_max_neighbors=None,
                 precomputed_lm_embeddings=None, remove_hs=False, all_atoms=False, atom_radius=5, atom_max_neighbors=None, device=None,
                 seed=0):
        self.receptor_radius, self.c_alpha_max_neighbors = receptor_radius, c_alpha_max_neighbors
        self.remove_hs, self.all_atoms = remove_hs, all_atoms
        self.atom_radius, self.atom_max_neighbors = atom_radius, atom_max_neighbors
        self.ligand_smiles = list(ligand_smiles)
        self.device, self.seed = device, seed
        if lm_embeddings is None or lm_embeddings is False:
            lm = None
        elif lm_embeddings is True:
            if precomputed_lm_embeddings is None:
                raise NotImplementedError("computing ESM embeddings is not covered: pass precomputed_lm_embeddings (an array or .npy "
                                          "path of shape [residues, 1280])")
            lm = _load_embedding(precomputed_lm_embeddings)
        else:
            lm = _load_embedding(lm_embeddings)
        if protein_file is None:
            raise NotImplementedError("a protein_file of None means folding a sequence with ESMFold, which is not covered")
        if not remove_hs:
            raise NotImplementedError("remove_hs=False with SMILES ligands: hydrogens would have to be added (both shipped model "
                                      "configurations use remove_hs: true)")
        if lm is not None and len(pm.parse_pdb(protein_file).seq) != len(lm):
            raise ValueError("LM embeddings did not have the right length for the protein.")
        self.mols, self.reasons = embed_ligands(self.ligand_smiles, remove_hs, seed=seed, device=device)
        self.complex_graph = pm.get_receptor(protein_file, os.path.basename(str(protein_file)), ce._device(device),
                                             receptor_radius=receptor_radius, c_alpha_max_neighbors=c_alpha_max_neighbors,
                                             knn_only_graph=True, all_atoms=all_atoms, atom_radius=atom_radius,
                                             atom_max_neighbors=atom_max_neighbors, lm_embeddings=None if lm is None else [lm])

    def len(self):
        return len(self.ligand_smiles)

    def get(self, idx):
        smile, mol = self.ligand_smiles[idx], self.mols[idx]
        if mol is None:
            print("Failed to generate initial structure of molecule ", smile, " We are skipping it. The reason is the exception: ",
                  self.reasons[idx])
            failed = HeteroData()
            failed.name, failed.success = smile, False
            return failed
        g = merge_ligand_receptor(self.complex_graph, _ligand_graph(mol, self.remove_hs))
        g["ligand"].pos = g["ligand"].pos - torch.mean(g["ligand"].pos, dim=0, keepdim=True)
        g.name = smile
        g.mol = mol
        g.success = True
        return g
