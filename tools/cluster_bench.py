"""Cost of the pose-against-pose matrix and the binding modes of an inference epoch's poses, three routes:

    python tools/cluster_bench.py [--samples 40] [--complexes 8] [--reps 20]

on the ligands WITH real symmetry of tools/metrics_bench.py (12 to 576 graph isomorphisms, 12 to 28 heavy atoms), `samples` poses per
complex around five centres:
  host:     evaluation.cluster_poses per complex -- numpy fp64 over every (pair, isomorphism), the clustering loop in Python;
  rows:     the matrix through the EXISTING one-launch route: `samples` evaluation.pose_metrics_batch calls over all complexes, call i with
            pose i of every complex as its only crystal pose (row i of every matrix), then modes_from_matrix on the host;
  device:   ONE evaluation.cluster_poses_batch call -- cached isomorphisms, resident index tables, one upload, cbd_pose_modes (pair kernel +
            mode kernel), one download.
Each route runs once to warm up (isomorphism cache, code objects) and then `reps` times (the host route three times at most); every repeat is timed by a host clock around work
that ends in a device synchronise and by HIP events around the same region.  Reported: median, min, max and the quartile spread of the
repeats, and whether the three routes agree (modes exactly; the matrices of the two device routes bitwise on their upper triangles).
Prints one JSON line.  There is no CPU path."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_items(n_complexes, samples, centres=5):
    from metrics_bench import SHAPES, aryl
    rng = np.random.default_rng(23)
    items = []
    for c in range(n_complexes):
        mol = aryl(*SHAPES[c % len(SHAPES)])
        mol.atomicnums = mol.atomicnums.copy()
        if c >= len(SHAPES):
            mol.atomicnums[0] = 8 + c // len(SHAPES)      # another head atom: another ligand (another cache entry), the same symmetry
        n = len(mol.atomicnums)
        centre = rng.normal(0.0, 4.0, size=(centres, n, 3))
        lp = (centre[rng.integers(centres, size=samples)] + rng.normal(0.0, 0.4, size=(samples, n, 3))).astype(np.float32)
        items.append((lp, mol))
    return items


def timed(fn, dev):
    """-> (result, host wall ms, HIP-event ms) of one call"""
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return out, (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def spread(xs):
    q = np.percentile(xs, [25, 50, 75])
    return {"median": round(float(q[1]), 3), "min": round(float(np.min(xs)), 3), "max": round(float(np.max(xs)), 3),
            "q25": round(float(q[0]), 3), "q75": round(float(q[2]), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--complexes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cutoff", type=float, default=2.0)
    a = ap.parse_args()
    from confidence_bootstrapping_amd import engine, molecules_utils as mu
    from confidence_bootstrapping_amd.evaluation import cluster_poses, cluster_poses_batch, modes_from_matrix, pose_metrics_batch
    if not torch.cuda.is_available():
        raise RuntimeError("cluster_bench measures on the GPU: there is no CPU path")
    engine.load_library()
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    items = make_items(a.complexes, a.samples)

    def host():
        return [cluster_poses(lp, mol, cutoff=a.cutoff) for lp, mol in items]

    def rows():
        per_pose = [pose_metrics_batch([(lp, lp[i], mol) for lp, mol in items], dev) for i in range(a.samples)]
        out = []
        for c in range(len(items)):
            matrix = np.triu(np.stack([per_pose[i][c][0] for i in range(a.samples)]), 1)
            matrix = matrix + matrix.T
            out.append((matrix,) + modes_from_matrix(matrix, a.cutoff))
        return out

    def device():
        return cluster_poses_batch(items, dev, cutoff=a.cutoff, return_matrix=True)

    out = {"what": "pose-against-pose symmetry-corrected RMSD and binding modes: host, rows through pose_metrics_batch, one cbd_pose_modes call",
           "complexes": a.complexes, "samples": a.samples, "pairs_per_complex": a.samples * (a.samples - 1) // 2, "reps": a.reps,
           "isomorphisms": [int(mu.cached_isomorphisms(m.atomicnums, m.adjacency_matrix)[0].shape[0]) for _, m in items],
           "atoms": [int(len(m.atomicnums)) for _, m in items]}
    results = {}
    for name, fn in (("host", host), ("rows", rows), ("device", device)):
        results[name] = fn()      # warm-up: isomorphism cache, resident tables, code objects
        runs = [timed(fn, dev)[1:] for _ in range(min(a.reps, 3) if name == "host" else a.reps)]      # the host route takes seconds
        out[name + "_ms"] = {"wall": spread([r[0] for r in runs]), "hip_events": spread([r[1] for r in runs])}
    modes = lambda r: [(x[1].tolist(), x[2].tolist(), x[3]) for x in r]
    out["modes_per_complex"] = [x[3] for x in results["device"]]
    out["modes_equal_host_rows_device"] = modes(results["host"]) == modes(results["rows"]) == modes(results["device"])
    out["matrix_bitwise_equal_rows_device"] = bool(all(np.array_equal(r[0].view(np.int32), d[0].view(np.int32))
                                                       for r, d in zip(results["rows"], results["device"])))
    out["matrix_max_abs_diff_host_device"] = float(max(np.abs(h[0] - d[0]).max() for h, d in zip(results["host"], results["device"])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
