"""The host pipeline that keeps the GPU fed during inference, used by `sampling()` and `complex_set.ComplexSetRunner`.

A WAVE is up to eight GROUPS (the poses of one complex each) that advance in lockstep in ONE call (cbd_sample_multi).  The set-up of the
NEXT wave runs under the step loop of the current one: two alternating sets of engines (the partners share the first engine's weights),
cbd_set_complex on a stream of its own ("async_setup": it waits for the launches of ITS engine only), the pose / noise uploads on a side
stream.  The host is free for that as soon as the launch of the current wave returns, so `stage` and `launch` are separate calls:
launch k, stage k + 1, finish k.

`plan_waves` (which loader batches form a group, which groups a wave) is host arithmetic on keys and sizes; `score_wave` is the
confidence scoring of a wave's final poses.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence

import torch


class LoaderBatch(NamedTuple):
    """one pending loader batch: b poses of one complex with their N(0,1) draws (host tensors; None where the sampler draws none)"""
    first: int                          # index of its first pose in the caller's list
    pos: torch.Tensor                   # [b, Nl, 3]
    noise: tuple                        # (tr [S, b, 3], rot [S, b, 3], tor [S, b * R]), None in the place of a part that is not drawn
    graph: object                       # the batch's first graph as the caller holds it


class Group(NamedTuple):
    """a closed group: consecutive loader batches of ONE complex that advance as one engine batch"""
    cplx: object                        # the un-batched complex (DockEngine.set_complex)
    key: object                         # its complex_key (None: never recognised as already set up)
    batches: List[LoaderBatch]

    @property
    def first(self):
        return self.batches[0].first

    def host_pos(self):
        return _cat([b.pos for b in self.batches], 0)

    def host_noise(self):
        return tuple(None if zs[0] is None else _cat(zs, 1) for zs in zip(*(b.noise for b in self.batches)))


class Staged(NamedTuple):
    """a group set up on an engine, its inputs uploaded (or on their way on the side stream)"""
    group: Group
    engine: object
    pos: torch.Tensor                   # [B, Nl, 3] on the device, advanced in place by the launch
    noise: tuple                        # (tr, rot, tor)


def _cat(tensors, dim):
    return tensors[0] if len(tensors) == 1 else torch.cat(tensors, dim=dim)


def plan_waves(keys: Sequence, sizes: Sequence[int], max_batch: int, n_co: int):
    """Which loader batches run together.  `keys[c]` / `sizes[c]`: complex fingerprint and pose count of loader batch c.  Consecutive
    batches of one complex merge into a group until `max_batch` poses would be exceeded, a key change closes the group; `n_co` closed
    groups make a wave, the remainder the last one.  -> list of waves, a wave a list of groups, a group a list of batch indices."""
    groups, poses = [], 0
    for c, (key, b) in enumerate(zip(keys, sizes)):
        if groups and key == keys[groups[-1][-1]] and poses + b <= max_batch:
            groups[-1].append(c)
            poses += b
        else:
            groups.append([c])
            poses = b
    return [groups[i:i + n_co] for i in range(0, len(groups), n_co)]


def switch_on_async_setup(engines, before):
    """"async_setup" = 1 on every engine (cbd_set_complex then runs on a stream of the engine's own, beside the running wave);
    `before[engine]` = the previous value of those it changes, noted first, so that a caller can restore it whatever happens"""
    for e in engines:
        was = e.get_option("async_setup", 0)
        if was != 1:
            before[e] = was
            e.set_option("async_setup", 1)


class WavePipeline:
    """Staging and launch of waves on alternating engine sets `sets[0]`, `sets[1]` (the same set twice without look-ahead).
    `side_fills`: upload poses and noise on a side stream (the default on a GPU); without it -- the host-stepped samplers, a CPU
    device -- the poses go to the device on the current stream and the noise stays on the host.
    `order_fills`: test hook, see sampling._ORDER_SIDE_FILLS."""

    def __init__(self, device, sets, side_fills=True, order_fills=True):
        self.device, self.sets, self.order_fills = torch.device(device), sets, order_fills
        self.side = torch.cuda.Stream(self.device) if side_fills and self.device.type == "cuda" else None
        # Ordering of the side-stream fills: their device buffers come from the CURRENT stream's allocator pool, and a
        # block the host has freed may still be read by work already queued there (e.g. the confidence kernels of the previous wave).
        # `fill_after` is an event on the current stream recorded just BEFORE a wave is launched: the fills of the next wave follow
        # everything queued up to it, but not the running wave itself.
        self.fill_after = None

    def _up(self, t):
        """Device tensors are allocated from the CURRENT stream's pool (whatever it hands out was last used before the running wave
        was launched) and only filled on the side stream: an allocation ON the side stream would wait for the running wave
        (caching-allocator events)."""
        t = t.to(torch.float32).contiguous()
        d = torch.empty(t.shape, dtype=torch.float32, device=self.device)
        with torch.cuda.stream(self.side):
            d.copy_(t, non_blocking=True)
        return d

    def stage(self, groups, which, ahead=False, skip_same_key=False):
        """per-complex set-up (graph upload, receptor embedding) and the uploads of `groups` on engine set `which`.  `ahead`: a wave of
        this pipeline is running.  `skip_same_key`: an engine whose complex_key equals the group's is not set up again."""
        if self.side is not None and self.order_fills:
            if ahead and self.fill_after is not None:
                self.side.wait_event(self.fill_after)
            else:       # nothing of this pipeline is on the GPU: simply behind whatever the caller has queued
                self.side.wait_stream(torch.cuda.current_stream(self.device))
        staged = []
        for g, e in zip(groups, self.sets[which]):
            if not (skip_same_key and e.complex_key == g.key):
                e.set_complex(g.cplx, g.key)
            if self.side is None:
                pos, noise = g.host_pos().to(self.device, torch.float32).contiguous(), g.host_noise()
            else:
                pos, noise = self._up(g.host_pos()), tuple(None if z is None else self._up(z) for z in g.host_noise())
            staged.append(Staged(g, e, pos, noise))
        return staged

    def launch(self, staged, steps, trajectory=False, host_step=None):
        """Up to eight complexes advance in lockstep (cbd_sample_multi: their tensor-product launches are merged, so a launch carries
        several times the waves -- +24 % poses/s at 8 samples per complex); one group runs on cbd_sample.  Results are bitwise those
        of separate calls (tests/test_gpu_parity.py::test_sample_pair_equals_two_samples).  `host_step(staged group)`: a host-stepped
        sampler in place of the one-launch step loop.  -> the groups' trajectories [S, b, Nl, 3] with `trajectory`, else None."""
        if self.side is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_stream(self.side)
            self.fill_after = torch.cuda.Event()
            self.fill_after.record(cur)
        if host_step is not None:
            for s in staged:
                host_step(s)
            return None
        engines, poses, noises = zip(*((s.engine, s.pos, s.noise) for s in staged))
        if len(staged) == 1:
            trajs = [engines[0].sample(poses[0], steps, *noises[0], trajectory=trajectory)]
        else:
            trajs = type(engines[0]).sample_multi(list(engines), list(poses), steps, list(noises), trajectory=trajectory)
        return trajs if trajectory else None


def score_wave(cengs, items, crop_beyond=None, check=True, skip_same_key=False):
    """Confidence of a wave's final poses: up to four complexes per set of fused-conv launches (cbd_conf_score_multi: a launch then
    covers ~4x the waves and its last, partly filled round of resident waves costs ~1 % instead of ~6 %; bitwise the results of separate
    score() calls).  `items`: (all-atom complex, complex_key, poses [B, Nl, 3]) per group; the k-th group of a launch runs on `cengs[k]`.
    `check=False`: no host sync per launch -- the capacity flag of a confidence engine is sticky, the caller checks it once at the end.
    -> the confidences [B] per group."""
    cengs = cengs[:4]
    out = []
    for k0 in range(0, len(items), len(cengs)):
        part = items[k0:k0 + len(cengs)]
        for ce, (cplx, key, _) in zip(cengs, part):
            if not (skip_same_key and ce.complex_key == key):
                ce.set_complex(cplx, key)
        out += [c for c, _ in type(cengs[0]).score_multi(cengs[:len(part)], [pos for _, _, pos in part], crop_beyond, check=check)]
    return out
