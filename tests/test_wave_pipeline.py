"""The host pipeline under sampling() and ComplexSetRunner (confidence_bootstrapping_amd/wave_pipeline.py) and the pieces of sampling()
around it, on stand-in engines that record their calls.  No GPU, no library: on a CPU device the pipeline has no side stream."""
import copy
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from confidence_bootstrapping_amd import sampling as smp
from confidence_bootstrapping_amd.wave_pipeline import Group, LoaderBatch, WavePipeline, plan_waves


class _Engine:
    """records set_complex / sample / sample_multi / set_option into the shared `log`"""

    def __init__(self, log, name, fail=False):
        self.log, self.name, self.fail = log, name, fail
        self.complex_key, self.max_batch, self.R, self._options = None, 64, 0, {}

    def set_complex(self, graph, key=None):
        self.log.append(("set_complex", self.name, key))
        self.complex_key = key

    def sample(self, pos, steps, noise_tr=None, noise_rot=None, noise_tor=None, trajectory=False):
        return _Engine.sample_multi([self], [pos], steps, [(noise_tr, noise_rot, noise_tor)], trajectory)

    @staticmethod
    def sample_multi(engines, poses, steps, noises, trajectory=False):
        engines[0].log.append(("launch", tuple(e.name for e in engines)))
        if any(e.fail for e in engines):
            raise RuntimeError("boom")

    def set_option(self, name, value):
        self.log.append(("set_option", self.name, name, value))
        self._options[name] = int(value)

    def get_option(self, name, default=None):
        return self._options.get(name, default)


class _Model:
    def __init__(self, partners):
        self.partners = partners

    def co_engines(self, n, main):
        assert n <= len(self.partners)
        return self.partners[:n]


def _groups(n):
    """n one-batch groups of two poses, keys k0 .. k(n-1)"""
    return [Group(f"complex{i}", f"k{i}", [LoaderBatch(2 * i, torch.zeros(2, 3, 3), (None, None, None), f"graph{i}")]) for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------- wave planning
@pytest.mark.parametrize("keys, sizes, max_batch, n_co, want", [
    ("aaa", [2, 2, 1], 64, 4, [[[0, 1, 2]]]),                       # 1 complex x 5 poses at batch_size 2: one group, one wave
    ("abc", [2, 2, 2], 64, 2, [[[0], [1]], [[2]]]),                 # 3 complexes x 2 poses at n_co 2: the remainder is the last wave
    ("abc", [2, 2, 2], 64, 1, [[[0]], [[1]], [[2]]]),               # n_co 1: one group per wave
    ("aaa", [32, 32, 32], 64, 2, [[[0, 1], [2]]]),                  # a complex over max_batch: closed before the batch that would exceed it
    ("aaa", [32, 32, 1], 64, 1, [[[0, 1]], [[2]]]),                 # ... exactly max_batch still merges
    ("aaba", [2, 2, 2, 2], 64, 8, [[[0, 1], [2], [3]]]),            # a key change closes a group; the same complex later is a new group
    ("", [], 64, 4, []),                                            # an empty data_list
])
def test_plan_waves(keys, sizes, max_batch, n_co, want):
    assert plan_waves(list(keys), sizes, max_batch, n_co) == want


def test_default_co_schedule_aims_at_160_poses_per_launch():
    named = lambda per, n: [SimpleNamespace(name=f"c{k}") for k in range(n) for _ in range(per)]
    assert smp._co_count(None, named(40, 6), 10) == 4
    assert smp._co_count(None, named(8, 30), 8) == 8              # 20 would reach 160: capped at the eight engines of a launch
    assert smp._co_count(None, [SimpleNamespace() for _ in range(5)], 32) == 5      # unnamed graphs: batch_size poses per complex
    assert smp._co_count(3, named(40, 6), 10) == 3 and smp._co_count(0, named(40, 6), 10) == 1
    assert smp._co_count(4, named(40, 6), 10, n_streams=2) == 1 and smp._co_count(4, named(40, 6), 10, score_crop=5.0) == 1


def test_walk_merges_the_loader_batches_of_a_complex_and_draws_in_reference_order():
    from confidence_bootstrapping_amd import Batch
    from confidence_bootstrapping_amd.synthetic import make_complex
    cplx = make_complex(Nl=9, Nr=30, R=2, knn=8, seed=3, name="one")
    data_list = [Batch.from_data_list([copy.deepcopy(cplx)]) for _ in range(5)]
    for k, d in enumerate(data_list):
        d["ligand"].pos = d["ligand"].pos + float(k)
    torch.manual_seed(4)
    waves = smp._walk(data_list, 2, 64, 4, False, 3, None, True, False)
    assert len(waves) == 1 and len(waves[0]) == 1
    group = waves[0][0]
    assert [b.first for b in group.batches] == [0, 2, 4] and [b.pos.shape[0] for b in group.batches] == [2, 2, 1] and group.first == 0
    assert torch.equal(group.host_pos(), torch.stack([d["ligand"].pos for d in data_list]))
    torch.manual_seed(4)
    want = smp.draw_noise_like_reference(5, 2, 3, 2)
    for got, name in zip(group.host_noise(), ("tr", "rot", "tor")):
        assert torch.equal(got, want[name]), name
    # pre-drawn noise is sliced per pose (and per pose and torsion), none is drawn; the ODE sampler takes none
    state = torch.random.get_rng_state()
    sliced = smp._walk(data_list, 2, 64, 4, False, 3, want, True, False)[0][0]
    assert all(torch.equal(a, b) for a, b in zip(sliced.host_noise(), group.host_noise()))
    assert smp._walk(data_list, 2, 64, 4, False, 3, None, False, False)[0][0].host_noise() == (None, None, None)
    assert torch.equal(state, torch.random.get_rng_state())
    batches_of = lambda waves: [[len(g.batches) for g in w] for w in waves]
    assert batches_of(smp._walk(data_list, 2, 4, 4, False, 3, want, True, False)) == [[2, 1]]       # capacity 4: a second group ...
    assert batches_of(smp._walk(data_list, 2, 4, 1, False, 3, want, True, False)) == [[2], [1]]     # ... a second wave at n_co 1
    assert smp._walk([], 2, 64, 4, False, 3, None, True, False) == []
    with pytest.raises(RuntimeError, match="exceeds the engine capacity"):
        smp._walk(data_list, 5, 4, 4, False, 3, want, True, False)


# ------------------------------------------------------------------------------------------------------------------- call order
def test_three_waves_alternate_engine_sets_and_stage_ahead():
    log = []
    sets = [[_Engine(log, "a0"), _Engine(log, "a1")], [_Engine(log, "b0"), _Engine(log, "b1")]]
    groups = _groups(5)
    waves = [groups[0:2], groups[2:4], groups[4:5]]
    pipe = WavePipeline("cpu", sets)
    assert pipe.side is None
    finish = lambda staged, trajs: log.append(("finish", tuple(s.group.first for s in staged)))
    sets[0][1].complex_key = "k1"                      # already holds its complex: not set up again when skipping is asked for
    smp._run_waves(pipe, waves, finish, True, steps=None)
    assert log == [
        ("set_complex", "a0", "k0"), ("launch", ("a0", "a1")),                                                  # stage 0, launch 0
        ("set_complex", "b0", "k2"), ("set_complex", "b1", "k3"), ("finish", (0, 2)),                           # stage 1, finish 0
        ("launch", ("b0", "b1")), ("set_complex", "a0", "k4"), ("finish", (4, 6)),                              # launch 1, stage 2, finish 1
        ("launch", ("a0",)), ("finish", (8,))]                                                                  # launch 2, finish 2
    # without look-ahead the next wave is staged after the current one is finished
    del log[:]
    sets[1][0].complex_key = sets[1][1].complex_key = None
    smp._run_waves(pipe, waves[:2], finish, False, steps=None)
    assert [entry[0] for entry in log] == ["set_complex", "launch", "finish", "set_complex", "set_complex", "launch", "finish"]
    # without skipping every engine is set up again, equal key or not
    del log[:]
    staged = pipe.stage(waves[1], 1)
    assert log == [("set_complex", "b0", "k2"), ("set_complex", "b1", "k3")]
    assert [s.engine.name for s in staged] == ["b0", "b1"] and [s.group for s in staged] == waves[1]
    assert staged[0].pos.shape == (2, 3, 3) and staged[0].noise == (None, None, None)


# -------------------------------------------------------------------------------------------------------------- end-of-call duties
def test_call_scope_restores_async_setup_and_clears_capacity_flags_after_an_exception():
    log = []
    eng, p1, p2, p3 = (_Engine(log, n) for n in ("main", "p1", "p2", "p3"))
    eng.set_option("async_setup", 0)
    eng.set_option("graph", 0)
    p2.set_option("async_setup", 1)                    # switched on by somebody else: this call must leave it on
    p3.fail = True                                     # wave 1 runs on (p2, p3)
    checked = []

    class Conf:
        def __init__(self, k):
            self.k = k

        def check(self):
            checked.append(self.k)
            if self.k == 2:
                raise RuntimeError("a per-atom edge capacity was exceeded")       # the stale flag: swallowed, the call's own error goes up
    cengs = [Conf(k) for k in range(3)]
    groups = _groups(4)
    waves = [groups[:2], groups[2:]]
    with pytest.raises(RuntimeError, match="boom"):
        with smp._call_scope() as scope:
            sets = smp._engine_sets(_Model([p1, p2, p3]), eng, waves, True, scope)
            assert sets == [[eng, p1], [p2, p3]]
            assert [e.get_option("async_setup") for e in (eng, p1, p2, p3)] == [1, 1, 1, 1] and set(scope.async_before) == {eng, p1, p3}
            assert [e.get_option("graph") for e in (p1, p2, p3)] == [0, 0, 0]      # the partners run with the main engine's options
            scope.conf_used.update(cengs)
            smp._run_waves(WavePipeline("cpu", sets), waves, lambda staged, trajs: None, True, steps=None)
    assert [e.get_option("async_setup") for e in (eng, p1, p2, p3)] == [0, 0, 1, 0]
    assert sorted(checked) == [0, 1, 2]                # every confidence engine used, a raising check() included
    # a call that ends well leaves the flags to the caller's final check and still restores the option
    del checked[:]
    with smp._call_scope() as scope:
        smp._engine_sets(_Model([p1, p2, p3]), eng, waves, True, scope)
        scope.conf_used.update(cengs)
    assert checked == [] and [e.get_option("async_setup") for e in (eng, p1, p2, p3)] == [0, 0, 1, 0]
    # no look-ahead: one set serves every wave and "async_setup" is left alone
    with smp._call_scope() as scope:
        sets = smp._engine_sets(_Model([p1, p2, p3]), eng, waves, False, scope)
        assert sets == [[eng, p1], [eng, p1]] and not scope.async_before


# --------------------------------------------------------------------------------------------------------------------- steps cache
def test_cached_steps():
    from confidence_bootstrapping_amd.diffusion_utils import get_timestep_embedding
    args = Namespace(tr_sigma_min=0.1, tr_sigma_max=19.0, rot_sigma_min=0.03, rot_sigma_max=1.55, tor_sigma_min=0.0314, tor_sigma_max=3.14)
    model = type("Model", (), {})()                    # weakly referenceable, like a torch module
    model.timestep_emb_func = get_timestep_embedding("sinusoidal", 32, 10000)
    sched = lambda k: np.array([1.0, 0.5 - 0.01 * k])
    get = lambda k, **kw: smp._cached_steps(model, args, sched(k), sched(k), sched(k), None, **kw)
    first = get(0)
    assert len(first) == 2 and get(0) is first
    assert get(0, ode=True) is not first and get(0) is first
    # another embedding on the same model: its output is part of the steps
    old_emb = model.timestep_emb_func
    model.timestep_emb_func = get_timestep_embedding("sinusoidal", 32, 1000)
    fresh = get(0)
    assert fresh is not first and list(fresh[0].sigma_emb) != list(first[0].sigma_emb)
    model.timestep_emb_func = old_emb
    assert get(0) is first
    # eight entries: a ninth key evicts the oldest
    other = type("Model", (), {})()
    other.timestep_emb_func = old_emb
    get_other = lambda k: smp._cached_steps(other, args, sched(k), sched(k), sched(k), None)
    kept = [get_other(k) for k in range(8)]
    assert all(get_other(k) is kept[k] for k in range(8))
    ninth = get_other(8)
    assert get_other(8) is ninth and all(get_other(k) is kept[k] for k in range(1, 8))
    assert get_other(0) is not kept[0]
    assert get(0) is first                             # per model
