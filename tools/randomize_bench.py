"""Cost of randomising the starting poses of an inference epoch, host path against the one-launch device path:

    python tools/randomize_bench.py [--samples 40] [--complexes 1 8] [--reps 20] [--no-loop]

for the C2 workload (synthetic complex, DockGen median sizes) and the 1a0q ligand (23 atoms, 11 rotatable bonds; only its receptor's
centroid enters, so a two-residue stand-in serves), `samples` poses x 1 / 8 complexes:
  host:   randomize_position per complex -- what inference_epoch costs by default;
  device: randomize_position_batch over all complexes at once -- host wall time to the poses being back on the host (draws, packing,
          upload, launch, download) and, separately, the time between HIP events around the launch alone (the raw C call on a
          batch packed and uploaded beforehand);
and, unless --no-loop, one confidence-bootstrapping round (tools/cb_loop.py, 1 epoch) with `device_randomize` off and on.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_complexes(which, n):
    from confidence_bootstrapping_amd.hetero import Batch
    if which == "1a0q":
        from confidence_bootstrapping_amd.datasets import process_mols as pm
        g = pm.get_ligand(os.path.join(ROOT, "tests", "golden", "1a0q", "1a0q_ligand.sdf"), "1a0q")
        g["ligand"].pos = g["ligand"].pos.float()
        g["receptor"].pos = torch.tensor([[14.0, -2.5, 7.25], [10.0, 1.5, 3.75]])
        return [g.shallow_copy() for _ in range(n)]
    from confidence_bootstrapping_amd.synthetic import WORKLOADS, make_complex
    return [Batch.from_data_list([make_complex(seed=900 + i, name=f"c{i}", **WORKLOADS[which])]) for i in range(n)]


def kernel_ms(groups, sigma, dev, reps):
    """HIP-event time of the launch alone, on a batch packed and uploaded once"""
    from confidence_bootstrapping_amd import engine
    from confidence_bootstrapping_amd.sampling import _pack_randomization, _pocket_center, draw_randomization
    lib = engine.load_library()
    pk = _pack_randomization(groups, [_pocket_center(g) for g in groups], [draw_randomization(g, False, False, sigma) for g in groups])
    up = {k: torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.int32)).to(dev) for k, v in pk.items() if isinstance(v, np.ndarray) and v.size}
    p = lambda k: C.c_void_p(up[k].data_ptr()) if k in up else None
    out = torch.empty(int(pk["out_ptr"][-1]), 3, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    times = []
    for _ in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = lib.cbd_randomize_poses(len(pk["pose_lig"]), len(pk["lig_ptr"]) - 1, len(groups), int(pk["max_nl"]), int(pk["max_r"]), p("pose_lig"),
                                     p("pose_cplx"), p("out_ptr"), p("tor_ptr"), p("lig_ptr"), p("pos_in"), p("rot_ptr"), p("rot_edge"), p("mask_ptr"),
                                     p("mask_bits"), p("tor"), p("rot_mat"), p("tr"), p("center"), C.c_void_p(out.data_ptr()), stream)
        e1.record()
        assert rc == 0, lib.cbd_last_error()
        torch.cuda.synchronize(dev)
        times.append(e0.elapsed_time(e1))
    return round(float(np.median(times[3:])), 4)


def measure(which, n_complexes, samples, reps, dev, sigma):
    from confidence_bootstrapping_amd.sampling import randomize_position, randomize_position_batch
    base = make_complexes(which, n_complexes)
    fresh = lambda: [[g.shallow_copy() for _ in range(samples)] for g in base]
    host, device = [], []
    for _ in range(reps + 3):
        groups = fresh()
        t0 = time.perf_counter()
        for dl in groups:
            randomize_position(dl, False, False, sigma)
        host.append(time.perf_counter() - t0)
    for _ in range(reps + 3):
        groups = fresh()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        randomize_position_batch(groups, False, False, sigma, dev)
        device.append(time.perf_counter() - t0)
    ms = lambda xs: round(float(np.median(xs[3:])) * 1e3, 3)
    lig = base[0]["ligand"]
    return {"ligand": which, "Nl": int(lig.pos.shape[0]), "R": int(lig.edge_mask.sum()), "complexes": n_complexes, "poses": n_complexes * samples,
            "host_randomize_position_ms": ms(host), "device_batch_wall_ms": ms(device), "kernel_hip_events_ms": kernel_ms(fresh(), sigma, dev, reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--complexes", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    np.random.seed(0)
    torch.manual_seed(0)
    from confidence_bootstrapping_amd.utils import load_model_args
    sigma = load_model_args().tr_sigma_max
    out = {"what": "randomize_position per complex on the host vs randomize_position_batch in one launch", "samples_per_complex": a.samples,
           "cases": [measure(w, c, a.samples, a.reps, dev, sigma) for w in ("c2_dockgen_median", "1a0q") for c in a.complexes]}
    if not a.no_loop:
        import cb_loop
        for flag in (False, True):
            r = cb_loop.run(complexes=12, epochs=1, quiet=True, device_randomize=flag)
            out["cb_round_device_randomize_" + ("on" if flag else "off")] = {k: r[k] for k in ("total_s", "sampling_confidence_rmsd_s",
                                                                                               "poses_per_s_incl_confidence_and_rmsd")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
