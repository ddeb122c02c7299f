"""Cost of the pose checks (bond lengths, 1-3 distances, internal and receptor clashes) on an inference epoch's poses, two routes:

    python tools/checks_bench.py [--samples 40] [--complexes 8] [--atoms 32] [--receptor-atoms 3000 20000] [--reps 20]

`complexes` synthetic chain ligands of `atoms` heavy atoms, `samples` poses each, all against ONE receptor of the given size (a screening
run: the receptor is uploaded once), for every receptor size:
  host:     evaluation.pose_checks per complex -- numpy fp64 over every ligand pair and every (ligand atom, receptor atom) pair;
  device:   ONE evaluation.pose_checks_batch call -- one upload, one cbd_pose_checks launch, one download.
Each route runs once to warm up and then `reps` times (the host route three times at most); every repeat is timed by a host clock around
work that ends in a device synchronise and by HIP events around the same region.  Reported: median, min, max and the quartile spread of the
repeats, and whether the two routes agree (counts, flags and atoms exactly; the floats in fp32 steps).  Prints one JSON line.  There is no
CPU path."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOATS = ("bond_lo", "bond_hi", "angle_lo", "angle_hi", "clash_ratio", "rec_ratio", "rec_dist")
INTS = ("n_bad_bond", "n_bad_angle", "n_internal_clash", "n_rec_clash", "rec_lig_atom", "rec_atom", "flags")


def make_items(n_complexes, samples, n_atoms, n_rec, seed=29):
    """chain ligands with plausible bounds (bonds 1.5 A, 1-3 pairs 2.5 A, others at least 3 A), poses = a random walk of 1.5 A steps jittered
    per pose, in a pocket of a receptor whose atoms fill a ball at protein density (about 0.05 heavy atoms per cubic Angstrom)"""
    rng = np.random.default_rng(seed)
    radius_of_ball = (n_rec / 0.05 * 3 / (4 * np.pi)) ** (1 / 3)
    pts = rng.normal(size=(2 * n_rec + 4096, 3))
    pts = pts / np.linalg.norm(pts, axis=1, keepdims=True) * radius_of_ball * rng.random((len(pts), 1)) ** (1 / 3)
    rec_pos = pts[np.linalg.norm(pts, axis=1) > 6.0][:n_rec].astype(np.float32)          # the pocket: a 6 A hole at the centre
    rec_radius = rng.choice(np.float32([1.7, 1.6, 1.55, 1.8]), size=len(rec_pos), p=[0.63, 0.17, 0.19, 0.01])
    items = []
    for _ in range(n_complexes):
        idx = np.arange(n_atoms)
        sep = np.abs(idx[:, None] - idx[None])
        kind = np.where(sep == 1, 1, np.where(sep == 2, 2, 0)).astype(np.uint8)
        lower = np.where(sep == 1, 1.4, np.where(sep == 2, 2.3, 3.0)).astype(np.float32)
        upper = np.where(sep == 1, 1.6, np.where(sep == 2, 2.7, 100.0)).astype(np.float32)
        steps = rng.normal(size=(n_atoms, 3))
        walk = np.cumsum(1.5 * steps / np.linalg.norm(steps, axis=1, keepdims=True), axis=0)
        walk -= walk.mean(axis=0)
        lp = (walk[None] + rng.normal(0.0, 0.3, size=(samples, n_atoms, 3)) + rng.normal(0.0, 1.5, size=(samples, 1, 3))).astype(np.float32)
        items.append((lp, (lower, upper, kind, np.full(n_atoms, 1.7, dtype=np.float32)), (rec_pos, rec_radius)))
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
    ap.add_argument("--atoms", type=int, default=32)
    ap.add_argument("--receptor-atoms", type=int, nargs="+", default=[3000, 20000])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from confidence_bootstrapping_amd import engine
    from confidence_bootstrapping_amd.evaluation import pose_checks, pose_checks_batch
    if not torch.cuda.is_available():
        raise RuntimeError("checks_bench measures on the GPU: there is no CPU path")
    engine.load_library()
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    out = {"what": "pose checks (bonds, 1-3 distances, internal and receptor clashes): host per complex, one cbd_pose_checks launch",
           "complexes": a.complexes, "samples": a.samples, "ligand_atoms": a.atoms, "reps": a.reps, "receptors": []}
    for n_rec in a.receptor_atoms:
        items = make_items(a.complexes, a.samples, a.atoms, n_rec)
        routes = {"host": lambda: [pose_checks(*item) for item in items], "device": lambda: pose_checks_batch(items, dev)}
        entry = {"receptor_atoms": int(len(items[0][2][0])), "pair_distances": a.complexes * a.samples * a.atoms * int(len(items[0][2][0]))}
        results = {}
        for name, fn in routes.items():
            results[name] = fn()      # warm-up: code objects, allocator
            runs = [timed(fn, dev)[1:] for _ in range(min(a.reps, 3) if name == "host" else a.reps)]      # the host route takes seconds
            entry[name + "_ms"] = {"wall": spread([r[0] for r in runs]), "hip_events": spread([r[1] for r in runs])}
        cat = lambda r, k: np.concatenate([getattr(x, k) for x in r])
        entry["ints_equal_host_device"] = bool(all(np.array_equal(cat(results["host"], k), cat(results["device"], k)) for k in INTS))
        steps = [np.abs(cat(results["host"], k).view(np.int32).astype(np.int64) - cat(results["device"], k).view(np.int32).astype(np.int64))
                 for k in FLOATS]
        entry["floats_max_fp32_steps_host_device"] = int(max(s[np.isfinite(cat(results["host"], k))].max(initial=0) for s, k in zip(steps, FLOATS)))
        entry["valid_poses"] = int(cat(results["device"], "valid").sum())
        entry["speedup_wall_median"] = round(entry["host_ms"]["wall"]["median"] / entry["device_ms"]["wall"]["median"], 1)
        out["receptors"].append(entry)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
