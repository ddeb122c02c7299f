"""A SET of complexes on one rank (BASELINE.json configs[2]; reference inference.py:409-580 walks its test loader one complex at a
time): per-complex set-up, reverse diffusion of `samples` poses x `steps` denoising steps in co-scheduled groups of up to four
complexes (ONE cbd_sample_multi call per group), confidence model on the final poses, ranking by confidence
(inference.py:537-547).  `distributed.run_complex_set` partitions the set over the ranks (LPT) and calls `sample_group` here.

Used by tools/run_set.py, bench.py (`complex_set` leg) and tests/test_gpu_configs.py, so that the number the bench prints and the
parity test are about the same code.
"""
from __future__ import annotations

import copy
import time
from typing import Dict, List, Sequence

import numpy as np
import torch

from .engine import DockEngine, make_steps
from .hetero import Batch
from .sampling import randomize_position, randomize_position_batch
from .wave_pipeline import Group, LoaderBatch, WavePipeline, score_wave, switch_on_async_setup


class ComplexSetRunner:
    """Engines (one score engine + `group - 1` partners sharing its weights, one confidence engine) and the per-group work."""

    def __init__(self, score_model, score_args, conf_model, conf_args, device, samples=40, denoise_steps=20, group=4, keep_poses=False,
                 device_randomize=False):
        from .diffusion_utils import get_t_schedule
        self.dev = torch.device(device)
        self.samples, self.S, self.group = int(samples), int(denoise_steps), max(1, min(int(group), 8))
        self.score_args, self.conf_args = score_args, conf_args
        self.sched = get_t_schedule("expbeta", self.S)
        self.steps = make_steps(self.sched, score_args, score_model.timestep_emb_func)
        # two alternating sets of `group` engines (the partners share the first engine's weights): the complexes of the NEXT group are
        # set up on the idle set while the current group runs (wave_pipeline: cbd_set_complex with "async_setup", uploads on a side stream)
        self.engines = [DockEngine.from_model(score_model, self.dev, max_batch=self.samples)]
        self.engines += [self.engines[0].partner() for _ in range(2 * self.group - 1)]
        switch_on_async_setup(self.engines, {})
        self.sets = [self.engines[:self.group], self.engines[self.group:]]
        self.pipe = WavePipeline(self.dev, self.sets)
        self._ahead = None           # the group staged ahead: (its complex indices, engine set, wave_pipeline.Staged per complex)
        self._turn = 0
        self.ceng = conf_model.engine(max_batch=self.samples) if conf_model is not None else None
        # one confidence engine per complex of a group: up to four complexes are scored in ONE set of fused-conv launches
        self.cengs = ([self.ceng] + conf_model.co_engines(min(self.group, 4) - 1, self.ceng)) if conf_model is not None else []
        self.keep_poses = keep_poses
        self.device_randomize = bool(device_randomize)      # opt-in: a complex's starting poses in one cbd_randomize_poses launch
        self.times = {"setup": 0.0, "sample": 0.0, "conf": 0.0}
        self.prepared: Dict[int, tuple] = {}

    def set_option(self, name, value):
        for e in self.engines:
            e.set_option(name, value)

    def prepare(self, i, cplx):
        """Host-side inputs of complex i (data loading, outside any timed region): initial poses by the reference's
        randomize_position and pre-drawn N(0,1) noise, both seeded by the complex index -> independent of the partitioning."""
        state = (np.random.get_state(), torch.random.get_rng_state())
        try:
            torch.manual_seed(i)
            np.random.seed(i)
            dl = [Batch.from_data_list([copy.deepcopy(cplx)]) for _ in range(self.samples)]
            if self.device_randomize:
                randomize_position_batch([dl], False, False, self.score_args.tr_sigma_max, self.dev)
            else:
                randomize_position(dl, False, False, self.score_args.tr_sigma_max)
            pos0 = torch.stack([d["ligand"].pos for d in dl]).contiguous()
            R = int(cplx["ligand"].edge_mask.sum())
            noise = (torch.randn(self.S, self.samples, 3), torch.randn(self.S, self.samples, 3), torch.randn(self.S, self.samples * R))
        finally:
            np.random.set_state(state[0])
            torch.random.set_rng_state(state[1])
        self.prepared[i] = (cplx, pos0, noise)
        return self.prepared[i]

    def _groups(self, items):
        groups = []
        for i, c in items:
            cplx, pos0, noise = self.prepared[i] if i in self.prepared else self.prepare(i, c)
            groups.append(Group(cplx, None, [LoaderBatch(i, pos0, noise, cplx)]))
        return groups

    def sample_group(self, items: Sequence, next_items: Sequence = None) -> List[dict]:
        """`items` = [(index, complex), ...] (<= group): set-up of every complex (graph upload, receptor embedding, all-atom tables),
        ONE co-scheduled sampling call, confidence ranking.  One picklable dict per complex.  `next_items`: the group that will be
        asked for next -- its set-up runs on the other engine set while this group's step loop is on the GPU."""
        ta = time.perf_counter()
        indices, which, staged = self._ahead or (None, None, None)
        self._ahead = None
        if indices != tuple(i for i, _ in items):
            which, staged = self._turn, self.pipe.stage(self._groups(items), self._turn)
        self._turn = 1 - which
        tb = time.perf_counter()
        self.pipe.launch(staged, self.steps)
        t_ahead = 0.0
        if next_items:
            t0 = time.perf_counter()
            self._ahead = (tuple(i for i, _ in next_items), 1 - which, self.pipe.stage(self._groups(next_items), 1 - which, ahead=True))
            t_ahead = time.perf_counter() - t0
        torch.cuda.synchronize(self.dev)
        tc = time.perf_counter()
        confs = [None] * len(staged)
        if self.ceng is not None:
            confs = score_wave(self.cengs, [(s.group.cplx, None, s.pos) for s in staged], self.conf_args.crop_beyond)
        out = []
        for s, conf in zip(staged, confs):
            res = {"complex": s.group.first}
            if conf is not None:
                order = torch.argsort(conf, descending=True, stable=True)
                best = int(order[0])
                res.update(confidence=float(conf[best]), best=best, pos=s.pos[best].cpu().numpy(), order=order.cpu().numpy())
            else:
                res.update(confidence=None, best=0, pos=s.pos[0].cpu().numpy())
            if self.keep_poses:
                res["all_pos"] = s.pos.cpu()
            out.append(res)
        td = time.perf_counter()
        self.times["setup"] += tb - ta + t_ahead       # the part spent ahead ran under the step loop (inside "sample" as well)
        self.times["sample"] += tc - tb
        self.times["conf"] += td - tc
        return out
