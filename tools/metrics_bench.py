"""Cost of measuring the sampled poses of an inference epoch, host route against the one-launch device route:

    python tools/metrics_bench.py [--samples 8] [--complexes 16] [--crystal-poses 2] [--reps 10] [--no-loop]

on a fixed set of ligands WITH real symmetry (para-substituted phenyl rings and CF3 groups: 12 to 576 graph isomorphisms, 12 to 28
heavy atoms), `samples` poses and `crystal-poses` crystal poses per complex:
  host:   evaluation.pose_metrics per complex -- get_symmetry_rmsd per crystal pose (a networkx enumeration, two index-table uploads,
          one launch and one synchronising download each), numpy centroid, torch.cdist;
  device: evaluation.pose_metrics_batch over groups of 8 complexes -- cached isomorphisms, resident index tables, one upload, one
          cbd_pose_metrics launch, one download per group;
each as the FIRST call (cold isomorphism cache; the host route has no cache, so its first call only carries the one-time costs of the
process) and as the median of `reps` repeat calls, by host wall time and by HIP events around the same region (GPU time between the
first and the last operation queued, host gaps included).  Unless --no-loop, also one confidence-bootstrapping round (tools/cb_loop.py,
1 epoch, whose synthetic ligands are random trees with few isomorphisms) with `device_metrics` off and on.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def aryl(rings, cf3):
    """a chain of `rings` para-linked phenyl rings that starts at a nitrogen and carries `cf3` CF3 groups on one carbon at the far end
    (cf3 = 2: a C(CF3)2 fork).  Each ring can flip (x 2), each CF3 turns (x 6), two CF3 swap (x 2)."""
    nums, bonds = [7], []
    last = 0
    for _ in range(rings):
        first = len(nums)
        nums += [6] * 6
        bonds += [(first + i, first + (i + 1) % 6) for i in range(6)] + [(last, first)]
        last = first + 3
    hub = len(nums)
    nums.append(6)
    bonds.append((last, hub))
    for _ in range(cf3):
        c = len(nums)
        nums += [6, 9, 9, 9]
        bonds += [(hub, c), (c, c + 1), (c, c + 2), (c, c + 3)]
    am = np.zeros((len(nums), len(nums)), dtype=int)
    for i, j in bonds:
        am[i, j] = am[j, i] = 1
    return Namespace(atomicnums=np.asarray(nums), adjacency_matrix=am)


SHAPES = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 1), (3, 2)]      # (rings, cf3): 12, 24, 144, 288, 48, 576 isomorphisms


def make_items(n_complexes, samples, crystal_poses):
    rng = np.random.default_rng(11)
    items = []
    for c in range(n_complexes):
        mol = aryl(*SHAPES[c % len(SHAPES)])
        mol.atomicnums = mol.atomicnums.copy()
        if c >= len(SHAPES):
            mol.atomicnums[0] = 8 + c // len(SHAPES)      # another head atom: another ligand (another cache entry), the same symmetry
        n = len(mol.atomicnums)
        ref = rng.normal(0.0, 4.0, size=(crystal_poses, n, 3)).astype(np.float32)
        lp = (ref[0][None] + rng.normal(0.0, 1.0, size=(samples, n, 3))).astype(np.float32)
        items.append((lp, ref, mol))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--complexes", type=int, default=16)
    ap.add_argument("--crystal-poses", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    from confidence_bootstrapping_amd import engine, molecules_utils as mu
    from confidence_bootstrapping_amd.evaluation import pose_metrics, pose_metrics_batch
    engine.load_library()
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    items = make_items(a.complexes, a.samples, a.crystal_poses)
    host = lambda: [pose_metrics(lp, ref, mol, device=dev) for lp, ref, mol in items]
    device = lambda: [r for k in range(0, len(items), 8) for r in pose_metrics_batch(items[k:k + 8], dev)]
    out = {"what": "pose metrics of an inference epoch, host route vs one launch per 8 complexes", "complexes": a.complexes,
           "samples": a.samples, "crystal_poses": a.crystal_poses, "reps": a.reps,
           "isomorphisms": [int(mu.graph_isomorphisms(m.atomicnums, m.adjacency_matrix)[0].shape[0]) for _, _, m in items[:len(SHAPES)]],
           "atoms": [int(len(m.atomicnums)) for _, _, m in items[:len(SHAPES)]]}
    mu.iso_cache_clear()
    want, w, e = timed(host, dev)
    out["host_first_call_ms"] = {"wall": round(w, 2), "hip_events": round(e, 2)}
    got, w, e = timed(device, dev)
    out["device_first_call_cold_cache_ms"] = {"wall": round(w, 2), "hip_events": round(e, 2)}
    out["rmsd_bitwise_equal"] = bool(all(np.array_equal(np.asarray(h[0], dtype=np.float64), d[0].astype(np.float64)) for h, d in zip(want, got)))
    for name, fn in (("host_repeat_ms", host), ("device_repeat_warm_cache_ms", device)):
        runs = [timed(fn, dev)[1:] for _ in range(a.reps)]
        out[name] = {"wall_median": round(float(np.median([r[0] for r in runs])), 2), "hip_events_median": round(float(np.median([r[1] for r in runs])), 2)}
    out["cache"] = mu.iso_cache_stats()
    if not a.no_loop:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import cb_loop
        for flag in (False, True):
            r = cb_loop.run(complexes=12, epochs=1, quiet=True, device_metrics=flag)
            out["cb_round_device_metrics_" + ("on" if flag else "off")] = {k: r[k] for k in ("total_s", "sampling_confidence_rmsd_s",
                                                                                             "poses_per_s_incl_confidence_and_rmsd",
                                                                                             "targetinf_metrics")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
