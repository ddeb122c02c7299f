"""The confidence-bootstrapping loop end to end on one MI355X (BASELINE.json configs[4], C5), with the reference's command-line
defaults for the loop shape (README.md:52 of the reference: 8 samples per complex, inference batch 4, training batch 5,
max_complexes_per_couple 20, EMA, 20 denoising steps) on a synthetic cluster of C2-sized complexes:

    python tools/cb_loop.py [--complexes 12] [--epochs 3] [--cb-inference-freq 1] [--device-noise] [--device-randomize]
                            [--device-metrics] [--keep-distinct-rmsd A] [--keep-valid]

Prints per-epoch logs and one JSON line with the time split (sampling + confidence + RMSD / training) and the rates."""
import argparse
import copy
import json
import os
import sys
import time
from argparse import Namespace
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(complexes=12, epochs=3, cb_inference_freq=1, samples=8, steps=20, workload="c2_dockgen_median", host_threads=16, quiet=False,
        device_noise=False, device_randomize=False, device_metrics=False, keep_distinct_rmsd=None, keep_valid=False):
    """-> dict with the time split of the loop (bench.py's `cb_round` leg calls this with the reference's loop shape)"""
    a = Namespace(complexes=complexes, epochs=epochs, cb_inference_freq=cb_inference_freq, samples=samples, steps=steps, workload=workload,
                  host_threads=host_threads, device_noise=device_noise, device_randomize=device_randomize,
                  device_metrics=device_metrics, keep_distinct_rmsd=keep_distinct_rmsd, keep_valid=keep_valid)
    threads_before = torch.get_num_threads()
    torch.set_num_threads(a.host_threads)
    try:
        from threadpoolctl import threadpool_limits
        threadpool_limits(limits=a.host_threads)
    except Exception:
        pass
    try:
        return _run(a, quiet)
    finally:
        torch.set_num_threads(threads_before)


def _run(a, quiet):
    from confidence_bootstrapping_amd.synthetic import make_complex, add_atoms, WORKLOADS
    from confidence_bootstrapping_amd.utils import make_score_model, make_confidence_model, load_model_args, ExponentialMovingAverage
    from confidence_bootstrapping_amd.diffusion_utils import t_to_sigma
    from confidence_bootstrapping_amd.bootstrapping.buffer import CBBuffer
    from confidence_bootstrapping_amd.datasets.pdbbind import NoiseTransform
    from confidence_bootstrapping_amd import finetune_train as ft
    dev = torch.device("cuda:0")
    margs = load_model_args()
    model, _ = make_score_model(device=dev, seed=0, args=margs)
    conf_model, conf_args = make_confidence_model(device=dev, seed=5)
    names = [f"{1000 + i}_A_lig{i}" for i in range(a.complexes)]
    targets = []
    for i, n in enumerate(names):
        g = add_atoms(make_complex(seed=900 + i, name=n, **WORKLOADS[a.workload]), seed=900 + i)
        g["ligand"].orig_pos = g["ligand"].pos.numpy() + g.original_center.numpy()
        nums = g["ligand"].x[:, 0].numpy() + 1
        g["ligand"].x[:, 0] = torch.from_numpy(nums)
        ei = g["ligand", "ligand"].edge_index.numpy()
        am = np.zeros((len(nums), len(nums)), dtype=int)
        am[ei[0], ei[1]] = 1
        g.mol = Namespace(atomicnums=nums, adjacency_matrix=am)
        targets.append(g)
    args = copy.copy(margs)
    args.__dict__.update(inference_steps=a.steps, inference_samples=a.samples, inference_batch_size=4, n_epochs=a.epochs,
                         cb_inference_freq=a.cb_inference_freq, initial_iterations=1, inference_iterations=1,
                         num_inference_complexes=a.complexes, batch_size=5, use_ema=True, tr_weight=0.33, rot_weight=0.33, tor_weight=0.33,
                         device_noise=a.device_noise,     # noise each training batch with one launch (NoiseTransform.apply_noise_batch)
                         device_randomize=a.device_randomize,     # starting poses of each group of complexes with one launch (randomize_position_batch)
                         device_metrics=a.device_metrics,     # RMSDs of each group of complexes with one launch and cached isomorphisms (pose_metrics_batch)
                         keep_distinct_rmsd=a.keep_distinct_rmsd,     # keep only the heads of each complex's binding modes (cluster_poses_batch)
                         keep_valid=a.keep_valid)     # keep only the poses that pass the distance checks (pose_checks_batch)
    t2s = partial(t_to_sigma, args=margs)
    buf = CBBuffer(cluster_name="c", cluster_to_ligands={"c": names}, max_complexes_per_couple=20,
                   transform=NoiseTransform(t_to_sigma=t2s, no_torsion=False, all_atom=False))
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=True)   # as utils.get_optimizer_and_scheduler builds it on a GPU
    ema = ExponentialMovingAverage(model.parameters(), decay=0.999)
    # time the two phases by wrapping the module-level functions the loop calls
    spent = {"inference": 0.0, "train": 0.0, "poses": 0, "train_items": 0}
    inf0, tr0 = ft.inference_epoch, ft.train_epoch

    def inf(*x, **k):
        torch.cuda.synchronize(); t = time.perf_counter()
        out = inf0(*x, **k)
        torch.cuda.synchronize(); spent["inference"] += time.perf_counter() - t
        spent["poses"] += a.samples * len(x[2])
        return out

    def tr(model_, loader, *x, **k):
        torch.cuda.synchronize(); t = time.perf_counter()
        out = tr0(model_, loader, *x, **k)
        torch.cuda.synchronize(); spent["train"] += time.perf_counter() - t
        spent["train_items"] += len(loader.dataset)
        return out

    ft.inference_epoch, ft.train_epoch = inf, tr
    # warm-up round (engine creation, weight packing, allocator) outside the timed loop
    wargs = copy.copy(args); wargs.n_epochs = 1
    ft.inference_finetune(wargs, model, conf_model, conf_args, None, -1e9, opt, ema,
                          CBBuffer(cluster_name="c", cluster_to_ligands={"c": names}, max_complexes_per_couple=20, transform=buf.transform),
                          targets[:4], t2s, dev, log=lambda s: None)
    for k in spent:
        spent[k] = 0 if isinstance(spent[k], int) else 0.0
    t0 = time.perf_counter()
    try:
        hist = ft.inference_finetune(args, model, conf_model, conf_args, None, -1e9, opt, ema, buf, targets, t2s, dev,
                                     **({"log": (lambda s_: None)} if quiet else {}))
    finally:
        ft.inference_epoch, ft.train_epoch = inf0, tr0
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    return {"what": "confidence-bootstrapping loop, synthetic cluster", "complexes": a.complexes, "epochs": a.epochs,
                      "samples_per_complex": a.samples, "denoise_steps": a.steps, "total_s": round(total, 2),
                      "sampling_confidence_rmsd_s": round(spent["inference"], 2),
                      "poses_per_s_incl_confidence_and_rmsd": round(spent["poses"] / max(spent["inference"], 1e-9), 1),
                      "training_s": round(spent["train"], 2),
                      "training_complexes_per_s": round(spent["train_items"] / max(spent["train"], 1e-9), 1),
                      "complexes_per_s_whole_loop": round(a.complexes * a.epochs / total, 2),
                      "buffer": len(buf.complexes), "final_train_loss": hist[-1].get("train_loss"),
                      "targetinf_metrics": {k[len("targetinf_"):]: v for k, v in hist[-1].items() if k.startswith("targetinf_")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--complexes", type=int, default=12)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--cb-inference-freq", type=int, default=1)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--workload", default="c2_dockgen_median")
    ap.add_argument("--host-threads", type=int, default=16, help="intra-op threads of the host-side numpy/torch code (the reference's "
                    "--restrict_cpu uses 16, inference.py:225-234); tiny LAPACK/BLAS calls crawl on an unrestricted 128-thread pool")
    ap.add_argument("--device-noise", action="store_true", help="noise every training batch on the GPU in one launch (off by default)")
    ap.add_argument("--device-randomize", action="store_true", help="randomise the starting poses of every group of complexes on the GPU "
                    "in one launch (off by default)")
    ap.add_argument("--device-metrics", action="store_true", help="measure the poses of every group of complexes on the GPU in one launch, "
                    "with cached graph isomorphisms (off by default)")
    ap.add_argument("--keep-distinct-rmsd", type=float, default=None, help="of each complex's poses above the confidence cutoff, push only "
                    "the heads of its binding modes into the buffer: RMSD cutoff in Angstrom (default: none, every pose is kept)")
    ap.add_argument("--keep-valid", action="store_true", help="push only the poses that pass the bond, 1-3, internal-clash and receptor-clash "
                    "checks into the buffer (off by default)")
    a = ap.parse_args()
    print(json.dumps(run(a.complexes, a.epochs, a.cb_inference_freq, a.samples, a.steps, a.workload, a.host_threads,
                         device_noise=a.device_noise, device_randomize=a.device_randomize, device_metrics=a.device_metrics,
                         keep_distinct_rmsd=a.keep_distinct_rmsd, keep_valid=a.keep_valid)))


if __name__ == "__main__":
    main()
