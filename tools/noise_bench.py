"""Cost of the forward-diffusion transform per fine-tuning batch, host path against the one-launch device path, on the buffer shape
that tools/cb_loop.py builds (12 synthetic C2-sized complexes x 8 poses, at most 20 per couple):

    python tools/noise_bench.py [--batches 5 8 32] [--reps 30] [--no-loop]

  host:   NoiseTransform.__call__ per item (the buffer's `__getitem__`) + one upload of `pos` per item -- what the default loader costs;
  device: NoiseTransform.apply_noise_batch on the raw items -- host wall time (draws, packing, enqueue) and, separately, the time
          between HIP events around the upload + launch;
and, unless --no-loop, one confidence-bootstrapping round (tools/cb_loop.py, 1 epoch) with `device_noise` off and on.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_buffer(complexes=12, samples=8, workload="c2_dockgen_median"):
    from confidence_bootstrapping_amd.bootstrapping.buffer import CBBuffer
    from confidence_bootstrapping_amd.datasets.pdbbind import NoiseTransform
    from confidence_bootstrapping_amd.diffusion_utils import t_to_sigma
    from confidence_bootstrapping_amd.synthetic import WORKLOADS, make_complex
    from confidence_bootstrapping_amd.utils import load_model_args
    names = [f"{1000 + i}_A_lig{i}" for i in range(complexes)]
    nt = NoiseTransform(t_to_sigma=partial(t_to_sigma, args=load_model_args()), no_torsion=False, all_atom=False)
    buf = CBBuffer(cluster_name="c", cluster_to_ligands={"c": names}, max_complexes_per_couple=20, transform=nt)
    rng = np.random.default_rng(0)
    kept = []
    for i, n in enumerate(names):
        g = make_complex(seed=900 + i, name=n, **WORKLOADS[workload])
        for _ in range(samples):                       # the sampled poses of one complex: shallow copies that differ in `pos`
            s = g.shallow_copy()
            s["ligand"].pos = g["ligand"].pos + torch.from_numpy(rng.normal(0, 0.5, size=tuple(g["ligand"].pos.shape)).astype(np.float32))
            kept.append((s, float(rng.normal())))
    buf.add_complexes(kept)
    return buf, nt


def measure(buf, nt, batch, reps, dev):
    n = len(buf)
    idx = lambda k: [(k * batch + j) % n for j in range(batch)]
    host, wall, gpu = [], [], []
    for k in range(reps + 3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        items = [buf[i] for i in idx(k)]
        up = [d["ligand"].pos.to(dev) for d in items]
        torch.cuda.synchronize(dev)
        host.append(time.perf_counter() - t0)
        del up
    for k in range(reps + 3):
        raw = [buf.get(i) for i in idx(k)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        e0.record()
        nt.apply_noise_batch(raw, dev)
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize(dev)
        wall.append((t1 - t0, time.perf_counter() - t0))
        gpu.append(e0.elapsed_time(e1))
    ms = lambda xs: round(float(np.median(xs[3:])) * 1e3, 3)
    return {"batch": batch, "host_transform_plus_upload_ms": ms(host), "device_enqueue_wall_ms": ms([w[0] for w in wall]),
            "device_wall_to_done_ms": ms([w[1] for w in wall]), "device_hip_events_ms": round(float(np.median(gpu[3:])), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[5, 8, 32])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    np.random.seed(0)
    torch.manual_seed(0)
    buf, nt = build_buffer()
    out = {"what": "NoiseTransform per batch, host path vs one-launch device path", "buffer_items": len(buf),
           "per_batch": [measure(buf, nt, b, a.reps, dev) for b in a.batches]}
    if not a.no_loop:
        import cb_loop
        for flag in (False, True):
            r = cb_loop.run(complexes=12, epochs=1, quiet=True, device_noise=flag)
            out["cb_round_device_noise_" + ("on" if flag else "off")] = {k: r[k] for k in ("total_s", "training_s", "training_complexes_per_s",
                                                                                         "final_train_loss")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
