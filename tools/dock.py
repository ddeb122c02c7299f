"""Dock one ligand into one protein and write the ranked poses: the flow of the reference's dock.py for one complex given as files.

  python tools/dock.py --protein P.pdb[.gz] --ligand L.sdf|.mol2 --out DIR [--samples 10] [--steps 20] [--lm-embeddings E.npy]
                       [--score-model-dir D --ckpt F] [--confidence-model-dir D --confidence-ckpt F] [--save-visualisation] [--seed 0]

get_complex -> N shallow copies -> randomize_position -> sampling() with the confidence model -> DIR/rank1.sdf,
DIR/rank{k}_confidence{c:.2f}.sdf and, with --save-visualisation, DIR/rank{k}_reverseprocess.pdb (the input ligand, the input pose,
the randomised pose and the pose after every reverse-diffusion step as MODEL frames).

A model directory holds model_parameters.yml and the checkpoint.  Without one the model of the shipped architecture is built with
random weights from --seed: the poses are then meaningless, which is good for a smoke run only.  --lm-embeddings: an .npy of shape
[residues, 1280] (the ESM2 embeddings of the receptor's residues in file order); without it a zero block is used.  A SMILES ligand,
computing ESM embeddings and .pdb / .pdbqt ligands are out of scope."""
import argparse
import gzip
import os
import sys
import tempfile
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _load_model(model_dir, ckpt, device, seed, confidence_mode):
    from confidence_bootstrapping_amd.utils import load_model_args, get_model, make_score_model, make_confidence_model
    from confidence_bootstrapping_amd.diffusion_utils import t_to_sigma
    if model_dir is None:
        print(f"WARNING: no {'confidence' if confidence_mode else 'score'} model directory given: RANDOM weights (seed {seed}); "
              "the result is a smoke run, not a docking", file=sys.stderr)
        return (make_confidence_model if confidence_mode else make_score_model)(device=device, seed=seed)
    args = load_model_args(os.path.join(model_dir, "model_parameters.yml"))
    model = get_model(args, device, partial(t_to_sigma, args=args), no_parallel=True, confidence_mode=confidence_mode)
    model.load_state_dict(torch.load(os.path.join(model_dir, ckpt), map_location="cpu"), strict=True)
    return model.to(device).eval(), args


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--protein", required=True, help="receptor .pdb or .pdb.gz")
    ap.add_argument("--ligand", required=True, help="ligand .sdf or .mol2 (its coordinates seed the conformer)")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lm-embeddings", default=None)
    ap.add_argument("--score-model-dir", default=None)
    ap.add_argument("--ckpt", default="best_ema_inference_epoch_model.pt")
    ap.add_argument("--confidence-model-dir", default=None)
    ap.add_argument("--confidence-ckpt", default="best_model_epoch75.pt")
    ap.add_argument("--save-visualisation", action="store_true")
    ap.add_argument("--batch-size", type=int, default=10)
    ap.add_argument("--no-final-step-noise", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    if not a.ligand.endswith((".sdf", ".mol2")):
        ap.error("the ligand must be an .sdf or .mol2 file")
    from confidence_bootstrapping_amd.datasets import process_mols as pm
    from confidence_bootstrapping_amd.sampling import sampling, randomize_position
    from confidence_bootstrapping_amd.diffusion_utils import get_t_schedule, t_to_sigma
    from confidence_bootstrapping_amd.visualise import PDBFile
    from confidence_bootstrapping_amd.docking import write_ranked_poses
    if not torch.cuda.is_available():
        raise RuntimeError("docking runs on the GPU: there is no CPU path")
    dev = torch.device("cuda:0")
    model, margs = _load_model(a.score_model_dir, a.ckpt, dev, a.seed, False)
    cmodel, cargs = _load_model(a.confidence_model_dir, a.confidence_ckpt, dev, a.seed + 5, True)
    with tempfile.TemporaryDirectory() as tmp:
        protein = a.protein
        if protein.endswith(".gz"):
            protein = os.path.join(tmp, os.path.basename(a.protein)[:-3])
            with gzip.open(a.protein, "rb") as src, open(protein, "wb") as dst:
                dst.write(src.read())
        lm = None
        if "precomputed" in (getattr(model, "lm_embedding_type", None), getattr(cmodel, "lm_embedding_type", None)):
            n_res = len(pm.parse_pdb(protein).seq)
            if a.lm_embeddings is not None:
                lm = np.load(a.lm_embeddings).astype(np.float32)
                if lm.shape != (n_res, 1280):
                    raise ValueError(f"--lm-embeddings holds {lm.shape}, the receptor needs ({n_res}, 1280)")
            else:
                print("WARNING: no --lm-embeddings given: the language-model block of the receptor features is ZERO", file=sys.stderr)
                lm = np.zeros((n_res, 1280), dtype=np.float32)
        name = os.path.basename(a.ligand).rsplit(".", 1)[0]
        sdf = a.ligand if a.ligand.endswith(".sdf") else None
        cplx = pm.get_complex(protein, sdf or a.ligand, name, dev, remove_hs=bool(getattr(margs, "remove_hs", True)),
                              mol2_file=None if sdf is None else sdf[:-4] + ".mol2" if os.path.exists(sdf[:-4] + ".mol2") else None,
                              lm_embeddings=None if lm is None else [lm])
    torch.manual_seed(a.seed)
    np.random.seed(a.seed)
    data_list = [cplx.shallow_copy() for _ in range(a.samples)]
    randomize_position(data_list, margs.no_torsion, False, margs.tr_sigma_max)
    lig = cplx.mol
    visualization_list = None
    if a.save_visualisation:
        visualization_list = []
        for graph in data_list:
            pdb = PDBFile(lig)
            pdb.add(lig, 0, 0)
            pdb.add((cplx["ligand"].pos + cplx.original_center).detach().cpu(), 1, 0)
            pdb.add((graph["ligand"].pos + graph.original_center).detach().cpu(), part=1, order=1)
            visualization_list.append(pdb)
    sched = get_t_schedule("expbeta", a.steps)
    out = sampling(data_list=data_list, model=model, inference_steps=a.steps, tr_schedule=sched, rot_schedule=sched, tor_schedule=sched,
                   device=dev, t_to_sigma=partial(t_to_sigma, args=margs), model_args=margs, visualization_list=visualization_list,
                   confidence_model=cmodel, filtering_data_list=[cplx.shallow_copy() for _ in range(a.samples)],
                   filtering_model_args=cargs, batch_size=a.batch_size, no_final_step_noise=a.no_final_step_noise,
                   return_full_trajectory=a.save_visualisation)
    data_list, confidence = out[0], out[1]
    order = write_ranked_poses(a.out, lig, data_list, confidence, visualization_list, remove_hs=bool(getattr(margs, "remove_hs", True)))
    conf = confidence.detach().cpu().numpy().reshape(len(data_list), -1)[:, 0]
    print(f"{a.samples} poses x {a.steps} steps -> {a.out}")
    for rank, i in enumerate(order[:5]):
        print(f"  rank {rank + 1}: pose {i:2d}  confidence {conf[i]:+.4f}")
    return order, data_list, confidence


if __name__ == "__main__":
    main()
